// hg_refit.hip — deforming geometry: the one path of every update of a mesh of the device scene (update_mesh), the
// refit itself, which every kind of update ends with, and the entry points hg_refit_mesh / hg_refit_mesh_device;
// hg_scene_readback hands out the device scene's arrays for tests.  Not in the reference.
//
// An update replaces one mesh's triangles and recomputes every box of its tree on the device (the contract: hg_refit.h;
// the host twin: hg_refit_blas, hg_host_mesh.cpp), over the old topology (a refit) or a new one (hg_lbvh.hip), from
// 72-byte triangles or from vertices or a bone palette (hg_deform.hip).  The ten entry points fill a MeshUpdate
// (hg_rt.h); update_mesh runs, once and in this order:
//   1  null context, hg_ctx_flush;
//   2  every refusal that needs no device, with nothing launched or allocated before the last of them: the vertex
//      binding and skin (hg_deform.hip), the tree (hg_mesh_trees.h, which has no HIP in it and is tested on the CPU),
//      pointer alignment;
//   3  set_device, quiesce;
//   4  the source as triangles on the device: the caller's, staged from the host, or skinned and packed;
//   5  the refit, or the sort and the build of hg_lbvh.hip (a build by surface area has one late refusal, before the
//      first write to the scene);
//   6  for a rebuild: the new tree into the host's picture (HgMeshTrees::adopt), its plan list to the device, the refit,
//      the bound index list into the new order, stack depth and counters;
//   7  the order to the host, for the host forms.
//
// A translation unit of its own: the traversal kernels compile to what they compile to without it.  The kernels and
// their launchers first, then the path, then the entry points of the C-ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "halogen_abi.h"
#include "hg_refit.h"
#include "hg_rt.h"
#include "hg_scene_pack.h"

using namespace hgrt;

namespace {

constexpr int kRefitBlock = 256;

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

namespace {

// Steps 1-5 of a refit with the triangles on the device (d_tris: n_tris HalogenTriangle, at least 4-B aligned), for a
// context that is quiesced.  plan, list: the tree's plan and its records on the device (uploaded here on first use).
int refit_device(hg_ctx* c, const HgRefitPlan& plan, DevBuf& list, const std::vector<int32_t>& instances,
                 const void* d_tris, int32_t n_tris, uint64_t geometry_generation) {
    const HgDevMesh first = c->dev_meshes[size_t(instances[0])];
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
        if (!list.p) {
            if (int rc = upload(c, list, plan.records.data(), plan.records.size() * sizeof(uint32_t))) return rc;
        }
        if (int rc = ensure(c, c->refit_raw, size_t(plan.rec_span) * 6 * sizeof(float))) return rc;
        for (size_t h = 1; h < plan.level_off.size(); ++h) {
            const uint32_t begin = plan.level_off[h - 1], end = plan.level_off[h];
            hipLaunchKernelGGL(hg_refit_level, dim3((end - begin + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0,
                               c->stream, static_cast<const uint32_t*>(list.p), begin, end,
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
    hg_cull_table(c->dev_meshes.data(), c->dev_meshes.size(), c->cull_table);
    if (int rc = upload(c, c->meshes, c->dev_meshes.data(), c->dev_meshes.size() * sizeof(HgDevMesh))) return rc;
    if (int rc = upload(c, c->cull, c->cull_table.q.data(), c->cull_table.q.size() * sizeof(float4))) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    c->geometry_stale = true;
    c->geometry_gen = geometry_generation;
    c->scene_refits++;
    return HG_OK;
}

// What follows the records of either kind of rebuild: n_records records from slot.rec_min on hold the new tree's refs
// (c->lbvh.refs has the compact copy), c->lbvh.tris the triangles in the new order and c->lbvh.index_sorted the order.
// The host's picture of the new topology (hg_mesh_trees.h), the tree's device list, then the refit.
int adopt_device(hg_ctx* c, const MeshUpdate& u, const std::vector<int32_t>& instances, const HgMeshTrees::Slot& slot,
                 uint32_t n_records, int32_t n_tris) {
    const uint32_t tri_offset = c->dev_meshes[size_t(instances[0])].tri_offset;
    std::vector<uint32_t> refs(size_t(n_records) * 2);
    if (n_records)
        HG_HIP(c, hipMemcpyAsync(refs.data(), c->lbvh.refs.p, refs.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
    HgMeshTrees::Adopted tree;
    HgPackError err;
    if (c->trees.adopt(c->dev_meshes, u.mesh_index, instances, slot, refs.data(), n_records, uint32_t(n_tris), tree, err)) {
        // (the tree's records are overwritten, so the context is left without a scene and nothing else of its
        // bookkeeping is touched: the next call is a full upload)
        c->has_scene = false;
        return fail(c, err);
    }
    // the old tree's device list is kept for the new plan (the same size at the same leaf size: no free and allocation,
    // which would synchronise the device, per rebuild)
    DevBuf list;
    auto old = c->refit_lists.find(tree.old_key);
    if (old != c->refit_lists.end()) {
        list = old->second;
        c->refit_lists.erase(old);
    }
    const std::vector<uint32_t>& records = tree.plan->records;
    if (records.empty()) release(list);
    DevBuf& kept = c->refit_lists[tree.new_key] = list;
    int rc;
    if (!records.empty())
        if ((rc = upload(c, kept, records.data(), records.size() * sizeof(uint32_t)))) return rc;
    if ((rc = refit_device(c, *tree.plan, kept, instances, c->lbvh.tris.p, n_tris, u.generation))) return rc;
    // an index list bound to the tree (hg_set_mesh_vertices) follows the triangles into the new order
    if ((rc = deform_follow_order(c, tri_offset, static_cast<const uint32_t*>(c->lbvh.index_sorted.p), uint32_t(n_tris))))
        return rc;
    c->stack_depth = tree.stack_depth;
    c->scene_rebuilds++;
    return HG_OK;
}

}  // namespace

namespace hgrt {

// The one path of every mesh update; the steps are numbered as in this file's header
int update_mesh(hg_ctx* c, const MeshUpdate& u) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;  // 1
    // 2: every refusal that needs no device; nothing is launched or allocated before the last of them
    const bool from_tris = u.source == MeshUpdate::kTriangles;
    hg_ctx::VertexBinding* binding = nullptr;
    if (!from_tris)
        if (int rc = vertex_source_check(c, u, binding)) return rc;
    const int32_t n_tris = from_tris ? u.count : binding->n_tris;
    const bool have_tris = !from_tris || u.a;
    HgPackError err;
    const HgRefitPlan* plan = nullptr;
    std::vector<int32_t> instances;
    HgMeshTrees::Slot slot;
    uint32_t L = 0, K = 0;
    const int refused =
        u.how == HG_DEFORM_REBUILD
            ? c->trees.check_rebuild(c->has_scene, c->dev_meshes, u.mesh_index, have_tris, n_tris, u.leaf_size, instances,
                                     slot, L, K, err)
        : u.how == HG_DEFORM_REBUILD_SAH
            ? c->trees.check_rebuild_sah(c->has_scene, c->dev_meshes, u.mesh_index, have_tris, n_tris, u.node_cost,
                                         instances, slot, err)
            : c->trees.check_refit(c->has_scene, c->dev_meshes, u.mesh_index, have_tris, n_tris, plan, instances, err);
    if (refused) return fail(c, err);
    if (u.device && ((reinterpret_cast<uintptr_t>(u.a) | reinterpret_cast<uintptr_t>(u.b) |
                      reinterpret_cast<uintptr_t>(u.order)) & 3u)) {
        static const char* const arrays[3] = {"triangle and order arrays", "position, normal and order arrays",
                                              "bone and order arrays"};
        return fail(c, HG_E_INVALID, "%s: the %s must be 4-byte aligned", u.who,
                    from_tris && u.how == HG_DEFORM_REFIT ? "triangle array" : arrays[u.source]);
    }
    if (int rc = set_device(c)) return rc;  // 3
    if (int rc = quiesce(c)) return rc;     // no trace in flight reads the arrays rewritten below
    // 4: the source as triangles on the device
    const void* d_tris = u.a;
    if (!from_tris || !u.device) {
        const size_t bytes = size_t(n_tris) * sizeof(HalogenTriangle);
        if (int rc = ensure(c, c->refit_in, bytes)) return rc;
        d_tris = c->refit_in.p;
        if (!from_tris) {
            if (int rc = vertex_source_device(c, u, *binding)) return rc;
        } else if (bytes) {
            HG_HIP(c, hipMemcpyAsync(c->refit_in.p, u.a, bytes, hipMemcpyHostToDevice, c->stream));
        }
    }
    // 5, 6
    if (u.how == HG_DEFORM_REFIT)
        return refit_device(c, *plan, c->refit_lists[HgMeshTrees::key(c->dev_meshes[size_t(u.mesh_index)])], instances,
                            d_tris, n_tris, u.generation);
    const uint32_t tri_offset = c->dev_meshes[size_t(instances[0])].tri_offset;
    void* d_order = u.device ? u.order : nullptr;
    uint32_t n_records = K - 1;
    if (int rc = u.how == HG_DEFORM_REBUILD
                     ? build_lbvh_device(c, tri_offset, slot, L, K, d_tris, uint32_t(n_tris), d_order)
                     : build_sah_device(c, u.mesh_index, tri_offset, slot, u.node_cost, d_tris, uint32_t(n_tris), d_order,
                                        n_records))
        return rc;
    if (int rc = adopt_device(c, u, instances, slot, n_records, n_tris)) return rc;
    if (!u.device && u.order)  // 7
        HG_HIP(c, hipMemcpy(u.order, c->lbvh.index_sorted.p, size_t(n_tris) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HG_OK;
}

void refit_reset(hg_ctx* c) {
    for (auto& kv : c->refit_lists) release(kv.second);
    c->refit_lists.clear();
    c->trees.clear();
    for (auto& kv : c->vertex_bindings) release_binding(kv.second);
    c->vertex_bindings.clear();
}

}  // namespace hgrt

extern "C" {

int hg_refit_mesh_device(hg_ctx* c, int32_t mesh_index, const void* d_tris, int32_t n_tris,
                         uint64_t geometry_generation) {
    return update_mesh(c, {"hg_refit_mesh_device", mesh_index, MeshUpdate::kTriangles, d_tris, nullptr, n_tris, true,
                           HG_DEFORM_REFIT, 0, 0.0f, nullptr, geometry_generation});
}

int hg_refit_mesh(hg_ctx* c, int32_t mesh_index, const HalogenTriangle* tris, int32_t n_tris,
                  uint64_t geometry_generation) {
    return update_mesh(c, {"hg_refit_mesh", mesh_index, MeshUpdate::kTriangles, tris, nullptr, n_tris, false,
                           HG_DEFORM_REFIT, 0, 0.0f, nullptr, geometry_generation});
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
