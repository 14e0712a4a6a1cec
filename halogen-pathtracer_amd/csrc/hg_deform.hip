// hg_deform.hip — deforming geometry from where its users hold it, the vertices: hg_set_mesh_vertices binds a mesh's
// index list to its tree on the device, hg_deform_mesh / hg_deform_mesh_device pack the 72-byte triangles from vertex
// arrays there, hg_set_mesh_skin / hg_skin_mesh / hg_skin_mesh_device produce those vertices by linear-blend skinning
// (the contract: hg_skin.h; the host twin: hg_skin_vertices, hg_host_mesh.cpp).  The deform and skin entry points fill
// a MeshUpdate whose source is vertices or a palette; update_mesh (hg_refit.hip) takes from here the checks of that
// source (vertex_source_check, before the tree's checks and before anything is launched) and the source as packed
// triangles (vertex_source_device, after the quiesce), and goes on as for any other triangles.  Not in the reference.
//
// With HG_DEFORM_NORMALS the vertex normals are recomputed from the moved faces between the vertex source and the pack
// (the contract: hg_normals.h; the host twin: hg_vertex_normals), through the adjacency hg_set_mesh_vertices_opt bound.
//
// Five kernels, all on the context stream and ordered by it alone: no atomics, no kernel that waits on another
// workgroup.  The kernels first, then the two halves of a vertex source, then the entry points of the C-ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "halogen_abi.h"
#include "hg_normals.h"
#include "hg_rt.h"
#include "hg_skin.h"
#include "hg_tunables.h"

using namespace hgrt;

namespace {

constexpr int kBlock = 256;

// Pack: out[t] = the HalogenTriangle of indices[3t .. 3t + 2], byte for byte what hg_pack_triangles writes.  A workgroup
// takes 256 triangles: its 768 indices are read by consecutive lanes, a lane per corner; each corner's position and
// normal (two scattered 12-byte reads, the part a gather cannot avoid) go to their places in the triangle's 18 floats in
// LDS, and the 18 KiB leave as consecutive float4 (`out` is 16-byte aligned and a workgroup's part starts a multiple of
// 16 bytes into it): the mirror image of hg_refit_repack's read side.  Every index is below the vertex count
// (hg_set_mesh_vertices checked the list, and only deform_follow_order's permutation has touched it since).
__global__ __launch_bounds__(kBlock) void hg_deform_pack(const int32_t* __restrict__ indices, uint32_t n_tris,
                                                         const float* __restrict__ positions,
                                                         const float* __restrict__ normals, float* __restrict__ out) {
    __shared__ float4 s_out4[kBlock * kTriWords / 4];
    float* s_out = reinterpret_cast<float*>(s_out4);
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * uint32_t(kBlock);  // < n_tris: the grid is ceil(n_tris / 256)
    const uint32_t cnt = min(uint32_t(kBlock), n_tris - base);
    const int32_t* idx = indices + size_t(base) * 3;
    for (uint32_t i = tid; i < cnt * 3; i += kBlock) {
        const size_t v = size_t(uint32_t(idx[i])) * 3;
        const uint32_t t = i / 3, k = i - 3 * t;
        float* o = s_out + t * kTriWords + k * 3;  // pointA, pointB, pointC, normalA, normalB, normalC
        o[0] = positions[v];
        o[1] = positions[v + 1];
        o[2] = positions[v + 2];
        o[9] = normals[v];
        o[10] = normals[v + 1];
        o[11] = normals[v + 2];
    }
    __syncthreads();
    const uint32_t words = cnt * kTriWords;
    float* g = out + size_t(base) * kTriWords;
    float4* g4 = reinterpret_cast<float4*>(g);
    for (uint32_t i = tid; i < words / 4; i += kBlock) g4[i] = s_out4[i];
    for (uint32_t i = (words & ~3u) + tid; i < words; i += kBlock) g[i] = s_out[i];
}

// Skin: a lane per vertex over hg_skin_vertex.  A workgroup's 256 rest positions and normals (3 KiB each) come in and
// the results go out through LDS as consecutive words; the influences are one 8-byte and one 16-byte read per lane (the
// library's own arrays, aligned).  kLds: the palette (n_bones <= HG_SKIN_LDS_BONES) is copied to LDS first; otherwise a
// lane reads its four bones from global memory.  Every bone index is below n_bones (hg_set_mesh_skin checked them).
template <bool kLds>
__global__ __launch_bounds__(kBlock) void hg_deform_skin(const float* __restrict__ rest_positions,
                                                         const float* __restrict__ rest_normals,
                                                         const uint2* __restrict__ bone_indices,
                                                         const float4* __restrict__ weights, uint32_t n_vertices,
                                                         const float* __restrict__ bones, uint32_t n_bones,
                                                         float* __restrict__ out_positions,
                                                         float* __restrict__ out_normals) {
    __shared__ float s_p[kBlock * 3];
    __shared__ float s_n[kBlock * 3];
    __shared__ float s_bones[kLds ? HG_SKIN_LDS_BONES * HG_SKIN_BONE_FLOATS : 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * uint32_t(kBlock);  // < n_vertices: the grid is ceil(n_vertices / 256)
    const uint32_t cnt = min(uint32_t(kBlock), n_vertices - base);
    const size_t off = size_t(base) * 3;
    for (uint32_t i = tid; i < cnt * 3; i += kBlock) {
        s_p[i] = rest_positions[off + i];
        s_n[i] = rest_normals[off + i];
    }
    if (kLds)
        for (uint32_t i = tid; i < n_bones * HG_SKIN_BONE_FLOATS; i += kBlock) s_bones[i] = bones[i];
    __syncthreads();
    if (tid < cnt) {
        const uint2 bi = bone_indices[base + tid];
        const float4 wv = weights[base + tid];
        const uint16_t idx[4] = {uint16_t(bi.x & 0xFFFFu), uint16_t(bi.x >> 16), uint16_t(bi.y & 0xFFFFu),
                                 uint16_t(bi.y >> 16)};
        const float w[4] = {wv.x, wv.y, wv.z, wv.w};
        const float p[3] = {s_p[tid * 3], s_p[tid * 3 + 1], s_p[tid * 3 + 2]};
        const float n[3] = {s_n[tid * 3], s_n[tid * 3 + 1], s_n[tid * 3 + 2]};
        float op[3], on[3];
        hg_skin_vertex(kLds ? s_bones : bones, idx, w, p, n, op, on);
        for (int k = 0; k < 3; ++k) {  // (the lane's own three words)
            s_p[tid * 3 + k] = op[k];
            s_n[tid * 3 + k] = on[k];
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < cnt * 3; i += kBlock) {
        out_positions[off + i] = s_p[i];
        out_normals[off + i] = s_n[i];
    }
}

// The bound index list after a rebuild: dst[k] = src[order[k]], an int3 per lane (order[k] < n_tris: a permutation)
__global__ __launch_bounds__(kBlock) void hg_deform_permute(const int32_t* __restrict__ src,
                                                            const uint32_t* __restrict__ order, uint32_t n_tris,
                                                            int32_t* __restrict__ dst) {
    const uint32_t k = blockIdx.x * uint32_t(kBlock) + threadIdx.x;
    if (k >= n_tris) return;
    const int32_t* s = src + size_t(order[k]) * 3;
    const int32_t a = s[0], b = s[1], c2 = s[2];
    int32_t* d = dst + size_t(k) * 3;
    d[0] = a;
    d[1] = b;
    d[2] = c2;
}

// HG_DEFORM_NORMALS, first pass: out[t] = hg_face_normal of frozen[3t .. 3t + 2], 3 floats a triangle.  A workgroup takes
// 256 triangles as hg_deform_pack does: its 768 indices are read by consecutive lanes, a lane per corner, whose position
// (one scattered 12-byte read, the part a gather cannot avoid) goes to LDS; then a lane per triangle does the
// arithmetic, and the 3 KiB of results leave as consecutive words.  Every index is below the vertex count
// (hg_set_mesh_vertices_opt checked the list; nothing permutes the frozen copy).
__global__ __launch_bounds__(kBlock) void hg_deform_face_normals(const int32_t* __restrict__ frozen, uint32_t n_tris,
                                                                 const float* __restrict__ positions,
                                                                 float* __restrict__ out) {
    __shared__ float s_p[kBlock * 9];
    __shared__ float s_f[kBlock * 3];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * uint32_t(kBlock);  // < n_tris: the grid is ceil(n_tris / 256)
    const uint32_t cnt = min(uint32_t(kBlock), n_tris - base);
    const int32_t* idx = frozen + size_t(base) * 3;
    for (uint32_t i = tid; i < cnt * 3; i += kBlock) {
        const size_t v = size_t(uint32_t(idx[i])) * 3;
        s_p[i * 3] = positions[v];
        s_p[i * 3 + 1] = positions[v + 1];
        s_p[i * 3 + 2] = positions[v + 2];
    }
    __syncthreads();
    if (tid < cnt) {
        const float* p = s_p + tid * 9;
        float f[3];
        hg_face_normal(p, p + 3, p + 6, f);
        for (int k = 0; k < 3; ++k) s_f[tid * 3 + k] = f[k];
    }
    __syncthreads();
    float* g = out + size_t(base) * 3;
    for (uint32_t i = tid; i < cnt * 3; i += kBlock) g[i] = s_f[i];
}

// HG_DEFORM_NORMALS, second pass: out[v] = hg_vertex_normal over the vertex's range of the adjacency, a lane per vertex:
// the sum in the list's order, never split (a lane with a very long list runs long; its wave waits for it).  Every face id
// is below the triangle count and the offsets ascend to 3 * n_tris (hg_normals_build_adjacency made them).  The
// results leave through LDS as consecutive words.
__global__ __launch_bounds__(kBlock) void hg_deform_vertex_normals(const int32_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ faces,
                                                                   const float* __restrict__ face_normals,
                                                                   uint32_t n_vertices, float* __restrict__ out) {
    __shared__ float s_n[kBlock * 3];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * uint32_t(kBlock);  // < n_vertices: the grid is ceil(n_vertices / 256)
    const uint32_t cnt = min(uint32_t(kBlock), n_vertices - base);
    if (tid < cnt) {
        float n[3];
        hg_vertex_normal(face_normals, faces, offsets[base + tid], offsets[base + tid + 1], n);
        for (int k = 0; k < 3; ++k) s_n[tid * 3 + k] = n[k];
    }
    __syncthreads();
    float* g = out + size_t(base) * 3;
    for (uint32_t i = tid; i < cnt * 3; i += kBlock) g[i] = s_n[i];
}

// The scene, the mesh and its binding, for the entry point `who`
int binding_of(hg_ctx* c, const char* who, int32_t mesh_index, hg_ctx::VertexBinding*& b) {
    if (!c->has_scene) return fail(c, HG_E_NOSCENE, "%s: hg_upload_scene not called", who);
    if (mesh_index < 0 || mesh_index >= c->n_meshes)
        return fail(c, HG_E_INVALID, "%s: mesh_index %d out of range (%d meshes)", who, mesh_index, c->n_meshes);
    auto it = c->vertex_bindings.find(c->dev_meshes[size_t(mesh_index)].tri_offset);
    if (it == c->vertex_bindings.end())
        return fail(c, HG_E_INVALID, "%s: mesh %d has no vertex binding (hg_set_mesh_vertices; a full upload drops it)", who,
                    mesh_index);
    b = &it->second;
    return HG_OK;
}

// `bytes` of a host or device array into a context-owned device buffer, or the device array itself
int on_device(hg_ctx* c, const MeshUpdate& u, const void* src, DevBuf& buf, size_t bytes, const void*& d) {
    d = src;
    if (u.device) return HG_OK;
    if (int rc = ensure(c, buf, bytes)) return rc;
    HG_HIP(c, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    d = buf.p;
    return HG_OK;
}

}  // namespace

namespace hgrt {

void release_binding(hg_ctx::VertexBinding& b) {
    for (DevBuf* d : {&b.indices, &b.spare, &b.rest_positions, &b.rest_normals, &b.bone_indices, &b.weights, &b.positions,
                      &b.normals, &b.frozen, &b.adj_offsets, &b.adj_faces, &b.face_normals, &b.vertex_normals})
        release(*d);
}

// What an update from vertices or from a bone palette checks of its source, before the tree's checks: the binding,
// the skin, the arrays and their counts, the kind
int vertex_source_check(hg_ctx* c, const MeshUpdate& u, hg_ctx::VertexBinding*& b) {
    if (int rc = binding_of(c, u.who, u.mesh_index, b)) return rc;
    if (u.source == MeshUpdate::kBones) {
        if (b->n_bones == 0) return fail(c, HG_E_INVALID, "%s: mesh %d has no skin (hg_set_mesh_skin)", u.who, u.mesh_index);
        if (!u.a) return fail(c, HG_E_INVALID, "%s: null bone palette", u.who);
        if (u.count != b->n_bones)
            return fail(c, HG_E_INVALID, "%s: mesh %d: %d bones, its skin was bound with %d", u.who, u.mesh_index, u.count,
                        b->n_bones);
    } else {
        if (u.recompute_normals ? !u.a : !u.a || !u.b)
            return fail(c, HG_E_INVALID, "%s: null position%s array", u.who, u.recompute_normals ? "" : " or normal");
        if (u.count != b->n_vertices)
            return fail(c, HG_E_INVALID, "%s: mesh %d: %d vertices, its binding holds %d", u.who, u.mesh_index, u.count,
                        b->n_vertices);
    }
    if (u.recompute_normals && !b->adjacency)
        return fail(c, HG_E_INVALID,
                    "%s: HG_DEFORM_NORMALS: mesh %d was bound without adjacency (hg_set_mesh_vertices_opt, HG_BIND_ADJACENCY)",
                    u.who, u.mesh_index);
    if (u.how != HG_DEFORM_REFIT && u.how != HG_DEFORM_REBUILD && u.how != HG_DEFORM_REBUILD_SAH)
        return fail(c, HG_E_INVALID, "%s: unknown kind of deform %d", u.who, u.how);
    return HG_OK;
}

// The source of such an update as b.n_tris triangles in c->refit_in (large enough), on the context stream: a palette
// through the skin kernel into the binding's vertex buffers, vertices (the caller's, or those) through the pack kernel
int vertex_source_device(hg_ctx* c, const MeshUpdate& u, hg_ctx::VertexBinding& b) {
    const void* d_positions = nullptr;
    const void* d_normals = nullptr;
    if (u.source == MeshUpdate::kBones) {
        const void* d_bones = nullptr;
        if (int rc = on_device(c, u, u.a, c->deform_bones, size_t(u.count) * HG_SKIN_BONE_FLOATS * sizeof(float), d_bones))
            return rc;
        const uint32_t nv = uint32_t(b.n_vertices);
        const dim3 grid((nv + kBlock - 1) / kBlock);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, c->stream, static_cast<const float*>(b.rest_positions.p),
                               static_cast<const float*>(b.rest_normals.p), static_cast<const uint2*>(b.bone_indices.p),
                               static_cast<const float4*>(b.weights.p), nv, static_cast<const float*>(d_bones),
                               uint32_t(b.n_bones), static_cast<float*>(b.positions.p), static_cast<float*>(b.normals.p));
        };
        if (b.n_bones <= HG_SKIN_LDS_BONES)
            launch(hg_deform_skin<true>);
        else
            launch(hg_deform_skin<false>);
        HG_HIP(c, hipGetLastError());
        b.skinned = true;
        d_positions = b.positions.p;
        d_normals = b.normals.p;
    } else {
        const size_t bytes = size_t(u.count) * 3 * sizeof(float);
        if (int rc = on_device(c, u, u.a, c->deform_positions, bytes, d_positions)) return rc;
        if (!u.recompute_normals)
            if (int rc = on_device(c, u, u.b, c->deform_normals, bytes, d_normals)) return rc;
    }
    if (u.recompute_normals) {  // the normals from the moved faces: the face pass, then the vertex pass (hg_normals.h)
        float* out = static_cast<float*>(u.source == MeshUpdate::kBones ? b.normals.p : b.vertex_normals.p);
        hipLaunchKernelGGL(hg_deform_face_normals, dim3(uint32_t((b.n_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           c->stream, static_cast<const int32_t*>(b.frozen.p), uint32_t(b.n_tris),
                           static_cast<const float*>(d_positions), static_cast<float*>(b.face_normals.p));
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(hg_deform_vertex_normals, dim3(uint32_t((b.n_vertices + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           c->stream, static_cast<const int32_t*>(b.adj_offsets.p),
                           static_cast<const int32_t*>(b.adj_faces.p), static_cast<const float*>(b.face_normals.p),
                           uint32_t(b.n_vertices), out);
        HG_HIP(c, hipGetLastError());
        d_normals = out;
    }
    hipLaunchKernelGGL(hg_deform_pack, dim3(uint32_t((b.n_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                       static_cast<const int32_t*>(b.indices.p), uint32_t(b.n_tris), static_cast<const float*>(d_positions),
                       static_cast<const float*>(d_normals), static_cast<float*>(c->refit_in.p));
    HG_HIP(c, hipGetLastError());
    return HG_OK;
}

int deform_follow_order(hg_ctx* c, uint32_t tri_offset, const uint32_t* d_order, uint32_t n_tris) {
    auto it = c->vertex_bindings.find(tri_offset);
    if (it == c->vertex_bindings.end()) return HG_OK;
    hg_ctx::VertexBinding& b = it->second;
    if (uint32_t(b.n_tris) != n_tris)  // (a rebuild takes the tree's extent, which is what was bound)
        return fail(c, HG_E_INVALID, "hg_rebuild_mesh: the bound index list holds %d triangles, the rebuild %u", b.n_tris, n_tris);
    if (int rc = ensure(c, b.spare, size_t(n_tris) * 3 * sizeof(int32_t))) return rc;
    hipLaunchKernelGGL(hg_deform_permute, dim3((n_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                       static_cast<const int32_t*>(b.indices.p), d_order, n_tris, static_cast<int32_t*>(b.spare.p));
    HG_HIP(c, hipGetLastError());
    std::swap(b.indices, b.spare);
    return HG_OK;
}

}  // namespace hgrt

namespace {

// hg_set_mesh_vertices (flags 0) and hg_set_mesh_vertices_opt
int bind_vertices(hg_ctx* c, const char* who, int32_t mesh_index, const int32_t* indices, int32_t n_tris,
                  int32_t n_vertices, uint32_t flags) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (c->has_scene && !indices) return fail(c, HG_E_INVALID, "%s: null index array", who);
    const HgRefitPlan* plan = nullptr;
    std::vector<int32_t> instances;
    HgPackError err;
    if (c->trees.check_refit(c->has_scene, c->dev_meshes, mesh_index, indices != nullptr, n_tris, plan, instances, err))
        return fail(c, err);
    if (n_tris == 0 || uint32_t(n_tris) != plan->extent)
        return fail(c, HG_E_INVALID, "%s: mesh %d: %d triangles, its tree holds %u", who, mesh_index, n_tris, plan->extent);
    if (n_vertices <= 0) return fail(c, HG_E_INVALID, "%s: mesh %d: %d vertices", who, mesh_index, n_vertices);
    const int64_t bad = hg_skin_first_bad_index(indices, n_tris, n_vertices);
    if (bad >= 0)
        return fail(c, HG_E_INVALID, "%s: mesh %d: index %d of triangle %lld is outside the %d vertices", who, mesh_index,
                    indices[bad], static_cast<long long>(bad / 3), n_vertices);
    if (flags & ~uint32_t(HG_BIND_ADJACENCY))
        return fail(c, HG_E_INVALID, "%s: unknown flags 0x%x", who, flags & ~uint32_t(HG_BIND_ADJACENCY));
    const bool adjacency = (flags & HG_BIND_ADJACENCY) != 0;
    if (adjacency && n_tris > HG_NORMALS_MAX_TRIANGLES)
        return fail(c, HG_E_INVALID, "%s: mesh %d: an adjacency holds at most %d triangles", who, mesh_index,
                    HG_NORMALS_MAX_TRIANGLES);
    if (int rc = set_device(c)) return rc;
    const uint32_t key = c->dev_meshes[size_t(mesh_index)].tri_offset;
    auto old = c->vertex_bindings.find(key);
    if (old != c->vertex_bindings.end()) {  // a new list: the old one goes, and its skin with it
        HG_HIP(c, hipStreamSynchronize(c->stream));
        release_binding(old->second);
        c->vertex_bindings.erase(old);
    }
    hg_ctx::VertexBinding b;
    if (int rc = upload(c, b.indices, indices, size_t(n_tris) * 3 * sizeof(int32_t))) return rc;
    std::vector<int32_t> offsets, faces;  // (alive until the stream has taken them)
    if (adjacency) {
        offsets.resize(size_t(n_vertices) + 1);
        faces.resize(size_t(n_tris) * 3);
        hg_normals_build_adjacency(indices, n_tris, n_vertices, offsets.data(), faces.data());
        int rc;
        if ((rc = upload(c, b.frozen, indices, size_t(n_tris) * 3 * sizeof(int32_t))) ||
            (rc = upload(c, b.adj_offsets, offsets.data(), offsets.size() * sizeof(int32_t))) ||
            (rc = upload(c, b.adj_faces, faces.data(), faces.size() * sizeof(int32_t))) ||
            (rc = ensure(c, b.face_normals, size_t(n_tris) * 3 * sizeof(float))) ||
            (rc = ensure(c, b.vertex_normals, size_t(n_vertices) * 3 * sizeof(float)))) {
            (void)hipStreamSynchronize(c->stream);  // (no copy in flight reads a freed buffer)
            release_binding(b);
            return rc;
        }
        b.adjacency = true;
    }
    const hipError_t e = hipStreamSynchronize(c->stream);  // the caller's array is free again
    if (e != hipSuccess) {
        release_binding(b);
        return fail(c, HG_E_HIP, "%s failed: %s", "hipStreamSynchronize(c->stream)", hipGetErrorString(e));
    }
    b.n_tris = n_tris;
    b.n_vertices = n_vertices;
    c->vertex_bindings[key] = b;
    return HG_OK;
}

// `how` of the deform and skin entry points without HG_DEFORM_NORMALS, and the flag
int kind_of(int32_t how) { return how & ~int32_t(HG_DEFORM_NORMALS); }
bool normals_of(int32_t how) { return (how & HG_DEFORM_NORMALS) != 0; }

}  // namespace

extern "C" {

int hg_set_mesh_vertices(hg_ctx* c, int32_t mesh_index, const int32_t* indices, int32_t n_tris, int32_t n_vertices) {
    return bind_vertices(c, "hg_set_mesh_vertices", mesh_index, indices, n_tris, n_vertices, 0);
}

int hg_set_mesh_vertices_opt(hg_ctx* c, int32_t mesh_index, const int32_t* indices, int32_t n_tris, int32_t n_vertices,
                             uint32_t flags) {
    return bind_vertices(c, "hg_set_mesh_vertices_opt", mesh_index, indices, n_tris, n_vertices, flags);
}

int hg_deform_mesh_device(hg_ctx* c, int32_t mesh_index, const void* d_positions, const void* d_normals,
                          int32_t n_vertices, int32_t how, int32_t leaf_size, float node_cost, void* d_order,
                          uint64_t geometry_generation) {
    return update_mesh(c, {"hg_deform_mesh_device", mesh_index, MeshUpdate::kVertices, d_positions,
                           normals_of(how) ? nullptr : d_normals, n_vertices, true, kind_of(how), leaf_size, node_cost,
                           d_order, geometry_generation, normals_of(how)});
}

int hg_deform_mesh(hg_ctx* c, int32_t mesh_index, const float* positions, const float* normals, int32_t n_vertices,
                   int32_t how, int32_t leaf_size, float node_cost, int32_t* order, uint64_t geometry_generation) {
    return update_mesh(c, {"hg_deform_mesh", mesh_index, MeshUpdate::kVertices, positions, normals_of(how) ? nullptr : normals,
                           n_vertices, false, kind_of(how), leaf_size, node_cost, order, geometry_generation,
                           normals_of(how)});
}

int hg_set_mesh_skin(hg_ctx* c, int32_t mesh_index, const float* rest_positions, const float* rest_normals,
                     const uint16_t* bone_indices, const float* weights, int32_t n_vertices, int32_t n_bones) {
    static const char* who = "hg_set_mesh_skin";
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    hg_ctx::VertexBinding* b = nullptr;
    if (int rc = binding_of(c, who, mesh_index, b)) return rc;
    if (!rest_positions || !rest_normals || !bone_indices || !weights)
        return fail(c, HG_E_INVALID, "%s: null rest pose, bone index or weight array", who);
    if (n_vertices != b->n_vertices)
        return fail(c, HG_E_INVALID, "%s: mesh %d: %d vertices, its binding holds %d", who, mesh_index, n_vertices,
                    b->n_vertices);
    if (n_bones < 1 || n_bones > 65536) return fail(c, HG_E_INVALID, "%s: n_bones %d outside 1..65536", who, n_bones);
    const int64_t bad = hg_skin_first_bad_bone(bone_indices, n_vertices, n_bones);
    if (bad >= 0)
        return fail(c, HG_E_INVALID, "%s: mesh %d: bone index %d of vertex %lld is not below the %d bones", who, mesh_index,
                    int(bone_indices[bad]), static_cast<long long>(bad / HG_SKIN_INFLUENCES), n_bones);
    if (int rc = set_device(c)) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));  // (a reallocation frees the old arrays)
    const size_t nv = size_t(n_vertices);
    int rc;
    if ((rc = upload(c, b->rest_positions, rest_positions, nv * 3 * sizeof(float)))) return rc;
    if ((rc = upload(c, b->rest_normals, rest_normals, nv * 3 * sizeof(float)))) return rc;
    if ((rc = upload(c, b->bone_indices, bone_indices, nv * HG_SKIN_INFLUENCES * sizeof(uint16_t)))) return rc;
    if ((rc = upload(c, b->weights, weights, nv * HG_SKIN_INFLUENCES * sizeof(float)))) return rc;
    if ((rc = ensure(c, b->positions, nv * 3 * sizeof(float)))) return rc;
    if ((rc = ensure(c, b->normals, nv * 3 * sizeof(float)))) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays are free again
    b->n_bones = n_bones;
    b->skinned = false;
    return HG_OK;
}

int hg_skin_mesh_device(hg_ctx* c, int32_t mesh_index, const void* d_bones, int32_t n_bones, int32_t how,
                        int32_t leaf_size, float node_cost, void* d_order, uint64_t geometry_generation) {
    return update_mesh(c, {"hg_skin_mesh_device", mesh_index, MeshUpdate::kBones, d_bones, nullptr, n_bones, true,
                           kind_of(how), leaf_size, node_cost, d_order, geometry_generation, normals_of(how)});
}

int hg_skin_mesh(hg_ctx* c, int32_t mesh_index, const float* bones, int32_t n_bones, int32_t how, int32_t leaf_size,
                 float node_cost, int32_t* order, uint64_t geometry_generation) {
    return update_mesh(c, {"hg_skin_mesh", mesh_index, MeshUpdate::kBones, bones, nullptr, n_bones, false, kind_of(how),
                           leaf_size, node_cost, order, geometry_generation, normals_of(how)});
}

int hg_mesh_vertices_readback(hg_ctx* c, int32_t mesh_index, float* positions, float* normals, int32_t n_vertices) {
    static const char* who = "hg_mesh_vertices_readback";
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    hg_ctx::VertexBinding* b = nullptr;
    if (int rc = binding_of(c, who, mesh_index, b)) return rc;
    if (!b->skinned) return fail(c, HG_E_INVALID, "%s: mesh %d has not been skinned (hg_skin_mesh)", who, mesh_index);
    if (n_vertices != b->n_vertices)
        return fail(c, HG_E_INVALID, "%s: mesh %d: %d vertices, its binding holds %d", who, mesh_index, n_vertices,
                    b->n_vertices);
    if (int rc = set_device(c)) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    const size_t bytes = size_t(n_vertices) * 3 * sizeof(float);
    if (positions) HG_HIP(c, hipMemcpy(positions, b->positions.p, bytes, hipMemcpyDeviceToHost));
    if (normals) HG_HIP(c, hipMemcpy(normals, b->normals.p, bytes, hipMemcpyDeviceToHost));
    return HG_OK;
}

}  // extern "C"
