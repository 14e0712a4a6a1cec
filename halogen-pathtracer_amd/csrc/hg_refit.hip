// hg_refit.hip — deforming geometry: hg_refit_mesh / hg_refit_mesh_device replace one mesh's triangles in the device
// scene and recompute every box of its tree there, topology unchanged (the contract: hg_refit.h; the host twin:
// hg_refit_blas, hg_host.cpp); hg_scene_readback hands out the device scene's arrays for tests.  Not in the reference.
//
// A translation unit of its own: the traversal kernels compile to what they compile to without it.  The kernels and
// their launchers first, then the entry points of the C-ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "halogen_abi.h"
#include "hg_refit.h"
#include "hg_rt.h"
#include "hg_scene_pack.h"

using namespace hgrt;

static_assert(sizeof(HalogenTriangle) == 72, "the repack kernel moves a triangle as 18 floats");

namespace {

constexpr int kRefitBlock = 256;
constexpr int kTriWords = 18;  // floats of a HalogenTriangle

// Repack: HalogenTriangle (72 B, AoS) -> the traversal's 9-float (v0, e1, e2) stream and the three normal float4
// (n0, n1 - n0, n2 - n0), the subtractions of hg_pack_geometry.  A lane-per-triangle read of 72-B structs is a strided
// access, so a workgroup's 256 triangles (18 KiB, a multiple of 16 B from the array's start) go through LDS: read with
// consecutive lanes on consecutive 16-B (kVec; the array is 16-B aligned) or 4-B words, converted one triangle per lane
// out of LDS (stride 18 words in, 9 and 12 out), and written back out as consecutive words / float4.
template <bool kVec>
__global__ __launch_bounds__(kRefitBlock) void hg_refit_repack(const float* __restrict__ src, uint32_t n_tris,
                                                               float* __restrict__ t9, float4* __restrict__ nrm) {
    __shared__ float4 s_in4[kRefitBlock * kTriWords / 4];
    __shared__ float s_t9[kRefitBlock * 9];
    __shared__ float4 s_nrm[kRefitBlock * 3];
    float* s_in = reinterpret_cast<float*>(s_in4);
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * uint32_t(kRefitBlock);  // < n_tris: the grid is ceil(n_tris / 256)
    const uint32_t cnt = min(uint32_t(kRefitBlock), n_tris - base);
    const uint32_t words = cnt * kTriWords;
    const float* g = src + size_t(base) * kTriWords;
    if (kVec) {
        const float4* g4 = reinterpret_cast<const float4*>(g);
        for (uint32_t i = tid; i < words / 4; i += kRefitBlock) s_in4[i] = g4[i];
        for (uint32_t i = (words & ~3u) + tid; i < words; i += kRefitBlock) s_in[i] = g[i];
    } else {
        for (uint32_t i = tid; i < words; i += kRefitBlock) s_in[i] = g[i];
    }
    __syncthreads();
    if (tid < cnt) {
        const float* p = s_in + tid * kTriWords;  // pointA, pointB, pointC, normalA, normalB, normalC
        float* o = s_t9 + tid * 9;
        for (int k = 0; k < 3; ++k) {
            o[k] = p[k];
            o[3 + k] = p[3 + k] - p[k];
            o[6 + k] = p[6 + k] - p[k];
        }
        s_nrm[tid * 3] = make_float4(p[9], p[10], p[11], 0.0f);
        s_nrm[tid * 3 + 1] = make_float4(p[12] - p[9], p[13] - p[10], p[14] - p[11], 0.0f);
        s_nrm[tid * 3 + 2] = make_float4(p[15] - p[9], p[16] - p[10], p[17] - p[11], 0.0f);
    }
    __syncthreads();
    float* out9 = t9 + size_t(base) * 9;
    for (uint32_t i = tid; i < cnt * 9; i += kRefitBlock) out9[i] = s_t9[i];
    float4* outn = nrm + size_t(base) * 3;
    for (uint32_t i = tid; i < cnt * 3; i += kRefitBlock) outn[i] = s_nrm[i];
}

// The raw box of a child: a leaf's from the caller's triangles (inline or through the leaf table, any length), an inner
// child's from the scratch array, where its own launch (a lower height, earlier in the stream) left it
__device__ HgRawBox child_raw(uint32_t ref, const uint2* __restrict__ leaves, const HalogenTriangle* __restrict__ tris,
                              uint32_t tri_offset, uint32_t rec_min, const float* __restrict__ raw) {
    HgRawBox b;
    if (ref & HG_LEAF_BIT) {
        uint32_t first = ref & HG_LEAF_PAYLOAD, count = (ref >> HG_LEAF_CNT_SHIFT) & HG_LEAF_INLINE_MAX;
        if (count == 0) {
            const uint2 e = leaves[first];
            first = e.x;
            count = e.y;
        }
        b = hg_refit_empty();
        const HalogenTriangle* t = tris + (first - tri_offset);
        for (uint32_t i = 0; i < count; ++i) hg_refit_add_triangle(b, t[i]);
    } else {
        const float* p = raw + size_t(ref - rec_min) * 6;
        for (int k = 0; k < 3; ++k) {
            b.lo[k] = p[k];
            b.hi[k] = p[3 + k];
        }
    }
    return b;
}

// One height of a tree's plan: a lane takes record list[i], reads the two refs from the record itself, writes the
// record's own raw box and the two stored boxes (refs and the zero q2.w / q3.w as they were).  The order between
// heights is the stream's: nothing here waits on another workgroup.
__global__ __launch_bounds__(kRefitBlock) void hg_refit_level(const uint32_t* __restrict__ list, uint32_t begin,
                                                              uint32_t end, float4* __restrict__ nodes,
                                                              const uint2* __restrict__ leaves,
                                                              const HalogenTriangle* __restrict__ tris,
                                                              uint32_t tri_offset, uint32_t rec_min,
                                                              float* __restrict__ raw) {
    const uint32_t i = begin + blockIdx.x * uint32_t(kRefitBlock) + threadIdx.x;
    if (i >= end) return;
    const uint32_t r = list[i];
    float4* q = nodes + size_t(r) * 4;
    const float wa = q[0].w, wb = q[1].w;
    const HgRawBox A = child_raw(__float_as_uint(wa), leaves, tris, tri_offset, rec_min, raw);
    const HgRawBox B = child_raw(__float_as_uint(wb), leaves, tris, tri_offset, rec_min, raw);
    const HgRawBox U = hg_refit_union(A, B);
    float* p = raw + size_t(r - rec_min) * 6;
    for (int k = 0; k < 3; ++k) {
        p[k] = U.lo[k];
        p[3 + k] = U.hi[k];
    }
    float lo[3], hi[3];
    hg_refit_stored(A, true, lo, hi);
    q[0] = make_float4(lo[0], lo[1], lo[2], wa);
    q[1] = make_float4(hi[0], hi[1], hi[2], wb);
    hg_refit_stored(B, true, lo, hi);
    q[2] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    q[3] = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

}  // namespace

namespace hgrt {

// Everything hg_refit_mesh* checks before the first device write.  On success: the tree (its plan built and cached on
// first use) and the meshes refitted together (the instances of the tree: same root ref, same triangle offset).
int refit_check(hg_ctx* c, int32_t mesh_index, const void* tris, int32_t n_tris, hg_ctx::RefitTree*& tree,
                std::vector<int32_t>& instances) {
    if (!c->has_scene) return fail(c, HG_E_NOSCENE, "hg_refit_mesh: hg_upload_scene not called");
    if (mesh_index < 0 || mesh_index >= c->n_meshes)
        return fail(c, HG_E_INVALID, "hg_refit_mesh: mesh_index %d out of range (%d meshes)", mesh_index, c->n_meshes);
    if (!tris) return fail(c, HG_E_INVALID, "hg_refit_mesh: null triangle array");
    if (n_tris < 0) return fail(c, HG_E_INVALID, "hg_refit_mesh: negative triangle count");
    const HgDevMesh& dm = c->dev_meshes[size_t(mesh_index)];
    const size_t n_rec = c->rec_refs.size() / 2, n_leaf = c->leaf_table.size() / 2;
    auto plan_of = [&](const HgDevMesh& m, HgRefitPlan& plan) {
        return hg_refit_plan(c->rec_refs.data(), n_rec, c->leaf_table.data(), n_leaf, m.root_ref, m.tri_offset, plan);
    };
    const uint64_t key = (uint64_t(dm.root_ref) << 32) | dm.tri_offset;
    auto it = c->refit_trees.find(key);
    if (it == c->refit_trees.end()) {
        hg_ctx::RefitTree t;
        if (!plan_of(dm, t.plan)) return fail(c, HG_E_INVALID, "hg_refit_mesh: mesh %d: the device records are not a tree", mesh_index);
        it = c->refit_trees.emplace(key, std::move(t)).first;
    }
    tree = &it->second;
    if (uint32_t(n_tris) < tree->plan.extent)
        return fail(c, HG_E_INVALID, "hg_refit_mesh: mesh %d: %d triangles, its tree's leaves reach %u", mesh_index,
                    n_tris, tree->plan.extent);
    if (uint64_t(dm.tri_offset) + uint64_t(n_tris) > uint64_t(c->n_tris))
        return fail(c, HG_E_INVALID, "hg_refit_mesh: mesh %d: triangles %u + %d past the scene's %d", mesh_index,
                    dm.tri_offset, n_tris, c->n_tris);
    instances.clear();
    const uint64_t lo = dm.tri_offset, hi = lo + uint64_t(n_tris);
    for (int32_t j = 0; j < c->n_meshes; ++j) {
        const HgDevMesh& o = c->dev_meshes[size_t(j)];
        if (o.root_ref == dm.root_ref && o.tri_offset == dm.tri_offset) {
            instances.push_back(j);
            continue;
        }
        // another tree over some of these triangles would go stale
        const uint64_t okey = (uint64_t(o.root_ref) << 32) | o.tri_offset;
        auto oit = c->refit_trees.find(okey);
        if (oit == c->refit_trees.end()) {  // (std::map: `tree` stays valid)
            hg_ctx::RefitTree t;
            if (!plan_of(o, t.plan))
                return fail(c, HG_E_INVALID, "hg_refit_mesh: mesh %d: the device records are not a tree", j);
            oit = c->refit_trees.emplace(okey, std::move(t)).first;
        }
        const uint64_t olo = o.tri_offset, ohi = olo + oit->second.plan.extent;
        if (olo < hi && lo < ohi)
            return fail(c, HG_E_UNSUPPORTED,
                        "hg_refit_mesh: mesh %d shares triangles with mesh %d, which has another tree", mesh_index, j);
    }
    return HG_OK;
}

// Steps 1-5 of a refit with the triangles on the device (d_tris: n_tris HalogenTriangle, at least 4-B aligned)
int refit_device(hg_ctx* c, hg_ctx::RefitTree& tree, const std::vector<int32_t>& instances, const void* d_tris,
                 int32_t n_tris, uint64_t geometry_generation) {
    const HgDevMesh first = c->dev_meshes[size_t(instances[0])];
    const HgRefitPlan& plan = tree.plan;
    c->guides_valid = false;  // the device scene changes: the guide images (hg_update_guides) are another scene's
    // (the tile cost order stays: the geometry moved, the image is similar)
    if (n_tris > 0) {
        float* t9 = static_cast<float*>(c->tris.p) + size_t(first.tri_offset) * 9;
        float4* nrm = static_cast<float4*>(c->normals.p) + size_t(first.tri_offset) * 3;
        const dim3 grid(uint32_t((n_tris + kRefitBlock - 1) / kRefitBlock));
        if ((reinterpret_cast<uintptr_t>(d_tris) & 15u) == 0)
            hipLaunchKernelGGL(hg_refit_repack<true>, grid, dim3(kRefitBlock), 0, c->stream,
                               static_cast<const float*>(d_tris), uint32_t(n_tris), t9, nrm);
        else
            hipLaunchKernelGGL(hg_refit_repack<false>, grid, dim3(kRefitBlock), 0, c->stream,
                               static_cast<const float*>(d_tris), uint32_t(n_tris), t9, nrm);
        HG_HIP(c, hipGetLastError());
    }
    HgRootPair pair{};
    if (!plan.records.empty()) {
        if (!tree.list.p) {
            if (int rc = upload(c, tree.list, plan.records.data(), plan.records.size() * sizeof(uint32_t))) return rc;
        }
        if (int rc = ensure(c, c->refit_raw, size_t(plan.rec_span) * 6 * sizeof(float))) return rc;
        for (size_t h = 1; h < plan.level_off.size(); ++h) {
            const uint32_t begin = plan.level_off[h - 1], end = plan.level_off[h];
            hipLaunchKernelGGL(hg_refit_level, dim3((end - begin + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0,
                               c->stream, static_cast<const uint32_t*>(tree.list.p), begin, end,
                               static_cast<float4*>(c->nodes.p), static_cast<const uint2*>(c->leaves.p),
                               static_cast<const HalogenTriangle*>(d_tris), first.tri_offset, plan.rec_min,
                               static_cast<float*>(c->refit_raw.p));
            HG_HIP(c, hipGetLastError());
        }
        // the root's two children, for the exact-cull boxes: one small copy
        float4 q[4];
        HG_HIP(c, hipMemcpyAsync(q, static_cast<const float4*>(c->nodes.p) + size_t(first.root_ref) * 4, sizeof q,
                                 hipMemcpyDeviceToHost, c->stream));
        HG_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 4; ++k) std::memcpy(&pair.box[3 * k], &q[k], 12);
    }
    const HalogenMeshData* meshes = reinterpret_cast<const HalogenMeshData*>(c->scene_copy[1].data());
    for (int32_t j : instances) {
        c->root_pairs[size_t(j)] = pair;
        set_cull_boxes_kept(meshes[j], pair, c->dev_meshes[size_t(j)]);
    }
    if (int rc = upload(c, c->meshes, c->dev_meshes.data(), c->dev_meshes.size() * sizeof(HgDevMesh))) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    c->geometry_stale = true;
    c->geometry_gen = geometry_generation;
    c->scene_refits++;
    return HG_OK;
}

void refit_reset(hg_ctx* c) {
    for (auto& kv : c->refit_trees) release(kv.second.list);
    c->refit_trees.clear();
    c->rebuild_slots.clear();
    for (auto& kv : c->vertex_bindings) {
        hg_ctx::VertexBinding& b = kv.second;
        for (DevBuf* d : {&b.indices, &b.spare, &b.rest_positions, &b.rest_normals, &b.bone_indices, &b.weights,
                          &b.positions, &b.normals})
            release(*d);
    }
    c->vertex_bindings.clear();
}

}  // namespace hgrt

extern "C" {

int hg_refit_mesh_device(hg_ctx* c, int32_t mesh_index, const void* d_tris, int32_t n_tris,
                         uint64_t geometry_generation) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    hg_ctx::RefitTree* tree = nullptr;
    std::vector<int32_t> instances;
    if (int rc = refit_check(c, mesh_index, d_tris, n_tris, tree, instances)) return rc;
    if (reinterpret_cast<uintptr_t>(d_tris) & 3u)
        return fail(c, HG_E_INVALID, "hg_refit_mesh_device: the triangle array must be 4-byte aligned");
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;  // no trace in flight reads the arrays rewritten below
    return refit_device(c, *tree, instances, d_tris, n_tris, geometry_generation);
}

int hg_refit_mesh(hg_ctx* c, int32_t mesh_index, const HalogenTriangle* tris, int32_t n_tris,
                  uint64_t geometry_generation) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    hg_ctx::RefitTree* tree = nullptr;
    std::vector<int32_t> instances;
    if (int rc = refit_check(c, mesh_index, tris, n_tris, tree, instances)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;
    const size_t bytes = size_t(n_tris) * sizeof(HalogenTriangle);
    if (int rc = ensure(c, c->refit_in, bytes)) return rc;
    if (bytes) HG_HIP(c, hipMemcpyAsync(c->refit_in.p, tris, bytes, hipMemcpyHostToDevice, c->stream));
    return refit_device(c, *tree, instances, c->refit_in.p, n_tris, geometry_generation);
}

int hg_scene_readback(hg_ctx* c, int32_t which, void* dst, size_t capacity, size_t* n_bytes) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (!c->has_scene) return fail(c, HG_E_NOSCENE, "hg_scene_readback: hg_upload_scene not called");
    const DevBuf* buf[5] = {&c->nodes, &c->leaves, &c->tris, &c->normals, &c->meshes};
    if (which < HG_SCENE_NODES || which > HG_SCENE_MESHES)
        return fail(c, HG_E_INVALID, "hg_scene_readback: unknown array %d", which);
    const size_t need = which == HG_SCENE_MESHES ? c->dev_meshes.size() * sizeof(HgDevMesh) : c->geometry_bytes[which];
    if (n_bytes) *n_bytes = need;
    if (!dst) return HG_OK;  // the size only
    if (capacity < need) return fail(c, HG_E_INVALID, "hg_scene_readback: destination too small (%zu < %zu)", capacity, need);
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;
    if (need) HG_HIP(c, hipMemcpy(dst, buf[which]->p, need, hipMemcpyDeviceToHost));
    return HG_OK;
}

}  // extern "C"
