// hg_lbvh.hip — hg_rebuild_mesh / hg_rebuild_mesh_device: a new tree for one mesh of the device scene, built on the
// device over the mesh's own triangle and record storage (the contract: hg_lbvh.h; the host twin: hg_build_blas_lbvh,
// hg_host.cpp).  Not in the reference.
//
// The build, all on the context stream and ordered by it alone (no float atomics, no kernel that waits on another
// workgroup): key points and per-workgroup bounds, the final bounds in one small workgroup, the Morton codes, rocprim's
// radix sort of (code, index) pairs (stable, so ties keep the caller's order), one lane per internal node of Karras'
// tree writing the records' refs, the gather of the triangles into the new order; then the refit of hg_refit.hip on
// the new topology writes the triangle and normal records and every box.
//
// hg_rebuild_mesh_sah / hg_rebuild_mesh_sah_device (the second contract of hg_lbvh.h; the twin: hg_build_blas_lbvh_sah):
// the same order, the radix tree at L = 1 in scratch, one lane per internal node deciding the small subtrees below it,
// rocprim's exclusive scan of the live flags, whose total the host reads to pick the rung of the node cost ladder and
// to refuse a tree that does not fit, then one lane per live node writing its record; the same refit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
// (the narrow header: the umbrella rocprim.hpp pulls in the texture cache iterator, which does not compile here)
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "halogen_abi.h"
#include "hg_lbvh.h"
#include "hg_rt.h"
#include "hg_scene_pack.h"

using namespace hgrt;

namespace {

constexpr int kBlock = 256;
constexpr int kTriWords = 18;  // floats of a HalogenTriangle
static_assert(sizeof(HalogenTriangle) == 72, "the kernels move a triangle as 18 floats");

// pmin / pmax of the workgroup's 256 lanes: s[k][tid] holds lane tid's value of component k (0..2 min, 3..5 max)
__device__ void block_bounds(float (*s)[kBlock], uint32_t tid) {
    for (uint32_t half = kBlock / 2; half > 0; half /= 2) {
        __syncthreads();
        if (tid < half)
            for (int k = 0; k < 3; ++k) {
                s[k][tid] = hg_fminf(s[k][tid], s[k][tid + half]);
                s[3 + k][tid] = hg_fmaxf(s[3 + k][tid], s[3 + k][tid + half]);
            }
    }
    __syncthreads();
}

// Key points.  A workgroup's 256 triangles go through LDS as in hg_refit_repack (consecutive lanes read consecutive
// 16-B or 4-B words), a lane computes its triangle's key point out of LDS, and the workgroup reduces its bounds:
// partial[6 * block] = pmin, pmax.  Lanes past the end contribute (+Inf, -Inf).
template <bool kVec>
__global__ __launch_bounds__(kBlock) void hg_lbvh_points(const float* __restrict__ src, uint32_t n_tris,
                                                         float* __restrict__ points, float* __restrict__ partial) {
    __shared__ float4 s_in4[kBlock * kTriWords / 4];
    __shared__ float s_red[6][kBlock];
    float* s_in = reinterpret_cast<float*>(s_in4);
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * uint32_t(kBlock);  // < n_tris: the grid is ceil(n_tris / 256)
    const uint32_t cnt = min(uint32_t(kBlock), n_tris - base);
    const uint32_t words = cnt * kTriWords;
    const float* g = src + size_t(base) * kTriWords;
    if (kVec) {
        const float4* g4 = reinterpret_cast<const float4*>(g);
        for (uint32_t i = tid; i < words / 4; i += kBlock) s_in4[i] = g4[i];
        for (uint32_t i = (words & ~3u) + tid; i < words; i += kBlock) s_in[i] = g[i];
    } else {
        for (uint32_t i = tid; i < words; i += kBlock) s_in[i] = g[i];
    }
    __syncthreads();
    const float inf = hg_u2f(0x7F800000u);
    float p[3] = {inf, inf, inf}, q[3] = {-inf, -inf, -inf};
    if (tid < cnt) {
        const float* w = s_in + tid * kTriWords;  // pointA, pointB, pointC first
        for (int k = 0; k < 3; ++k) {
            const float lo = hg_fminf(hg_fminf(w[k], w[3 + k]), w[6 + k]);
            const float hi = hg_fmaxf(hg_fmaxf(w[k], w[3 + k]), w[6 + k]);
            p[k] = q[k] = lo + hi;  // hg_lbvh_key_point
        }
        float* o = points + size_t(base + tid) * 3;
        o[0] = p[0];
        o[1] = p[1];
        o[2] = p[2];
    }
    for (int k = 0; k < 3; ++k) {
        s_red[k][tid] = p[k];
        s_red[3 + k][tid] = q[k];
    }
    block_bounds(s_red, tid);
    if (tid < 6) partial[size_t(blockIdx.x) * 6 + tid] = s_red[tid][0];
}

// The final bounds: one workgroup over the n_partial per-workgroup bounds
__global__ __launch_bounds__(kBlock) void hg_lbvh_bounds(const float* __restrict__ partial, uint32_t n_partial,
                                                         float* __restrict__ bounds) {
    __shared__ float s_red[6][kBlock];
    const uint32_t tid = threadIdx.x;
    const float inf = hg_u2f(0x7F800000u);
    float v[6] = {inf, inf, inf, -inf, -inf, -inf};
    for (uint32_t i = tid; i < n_partial; i += kBlock)
        for (int k = 0; k < 3; ++k) {
            v[k] = hg_fminf(v[k], partial[size_t(i) * 6 + k]);
            v[3 + k] = hg_fmaxf(v[3 + k], partial[size_t(i) * 6 + 3 + k]);
        }
    for (int k = 0; k < 6; ++k) s_red[k][tid] = v[k];
    block_bounds(s_red, tid);
    if (tid < 6) bounds[tid] = s_red[tid][0];
}

__global__ __launch_bounds__(kBlock) void hg_lbvh_codes(const float* __restrict__ points,
                                                        const float* __restrict__ bounds, uint32_t n_tris,
                                                        uint32_t* __restrict__ codes, uint32_t* __restrict__ index) {
    const uint32_t t = blockIdx.x * uint32_t(kBlock) + threadIdx.x;
    if (t >= n_tris) return;
    const float pmin[3] = {bounds[0], bounds[1], bounds[2]}, pmax[3] = {bounds[3], bounds[4], bounds[5]};
    const float p[3] = {points[size_t(t) * 3], points[size_t(t) * 3 + 1], points[size_t(t) * 3 + 2]};
    codes[t] = hg_lbvh_code(p, pmin, pmax);
    index[t] = t;
}

// One lane per internal node i of the K leaves: record rec_min + i gets its two refs (boxes zero until the refit's
// level launches write them; q2.w = q3.w = 0 as hg_pack_geometry leaves them), and refs[i] the same two refs for the
// host.  Karras' numbering keeps a subtree's records contiguous and two inner siblings adjacent (g, g + 1).
__global__ __launch_bounds__(kBlock) void hg_lbvh_topology(const uint32_t* __restrict__ codes, uint32_t n_tris,
                                                           uint32_t L, uint32_t K, uint32_t rec_min,
                                                           uint32_t tri_offset, float4* __restrict__ nodes,
                                                           uint2* __restrict__ refs) {
    const uint32_t i = blockIdx.x * uint32_t(kBlock) + threadIdx.x;
    if (i + 1 >= K) return;
    const HgLbvhNode nd = hg_lbvh_node(codes, L, int32_t(K), int32_t(i));
    uint32_t ref[2];
    for (int k = 0; k < 2; ++k) {
        const uint32_t g = uint32_t(nd.split) + uint32_t(k);
        const bool leaf = k == 0 ? nd.first == nd.split : nd.last == nd.split + 1;
        if (leaf) {
            uint32_t first, count;
            hg_lbvh_leaf(n_tris, L, g, first, count);
            ref[k] = HG_LEAF_BIT | (count << HG_LEAF_CNT_SHIFT) | (tri_offset + first);
        } else {
            ref[k] = rec_min + g;
        }
    }
    float4* q = nodes + size_t(rec_min + i) * 4;
    q[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ref[0]));
    q[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ref[1]));
    q[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    q[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    refs[i] = make_uint2(ref[0], ref[1]);
}

// The caller's triangles in the new order: dst[k] = src[order[k]], 72 bytes each.  A workgroup's 256 output triangles
// are gathered into LDS word by word (consecutive lanes read the consecutive words of one triangle: 72-B runs, which
// is what a gather allows) and leave as consecutive float4 (dst is 16-B aligned and a workgroup's part starts a multiple
// of 16 B into it).  Also the order itself, to the caller's array if there is one.
__global__ __launch_bounds__(kBlock) void hg_lbvh_gather(const float* __restrict__ src,
                                                         const uint32_t* __restrict__ order, uint32_t n_tris,
                                                         float* __restrict__ dst, int32_t* __restrict__ order_out) {
    __shared__ float4 s_t4[kBlock * kTriWords / 4];
    __shared__ uint32_t s_from[kBlock];
    float* s_t = reinterpret_cast<float*>(s_t4);
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * uint32_t(kBlock);
    const uint32_t cnt = min(uint32_t(kBlock), n_tris - base);
    if (tid < cnt) {
        const uint32_t from = order[base + tid];
        s_from[tid] = from;
        if (order_out) order_out[base + tid] = int32_t(from);
    }
    __syncthreads();
    const uint32_t words = cnt * kTriWords;
    for (uint32_t w = tid; w < words; w += kBlock) {
        const uint32_t t = w / kTriWords, k = w - t * kTriWords;
        s_t[w] = src[size_t(s_from[t]) * kTriWords + k];
    }
    __syncthreads();
    float* g = dst + size_t(base) * kTriWords;
    float4* g4 = reinterpret_cast<float4*>(g);
    for (uint32_t i = tid; i < words / 4; i += kBlock) g4[i] = s_t4[i];
    for (uint32_t i = (words & ~3u) + tid; i < words; i += kBlock) g[i] = s_t[i];
}

// ---- leaves chosen by surface area (hg_rebuild_mesh_sah; the second contract of hg_lbvh.h) ------------------------------
// The radix tree at L = 1 into scratch: one lane per internal node (n - 1 nodes do not fit the mesh's records)
__global__ __launch_bounds__(kBlock) void hg_lbvh_sah_topology(const uint32_t* __restrict__ codes, uint32_t n_tris,
                                                               HgLbvhNode* __restrict__ topo) {
    const uint32_t i = blockIdx.x * uint32_t(kBlock) + threadIdx.x;
    if (i + 1 >= n_tris) return;
    topo[i] = hg_lbvh_node(codes, 1u, int32_t(n_tris), int32_t(i));
}

// The collapse: one lane per internal node; the lanes of nodes above 15 triangles decide the maximal small subtrees
// below them (hg_lbvh_sah_node), each alone: at most 14 nodes listed in a register, their best costs in the lane's
// column of LDS (consecutive lanes, consecutive banks), the at most 15 sorted triangles read from `tris`.  No lane waits
// for another, and every live flag has one writer.
__global__ __launch_bounds__(kBlock) void hg_lbvh_sah_collapse(const HgLbvhNode* __restrict__ topo,
                                                               const HalogenTriangle* __restrict__ tris, uint32_t n_tris,
                                                               float node_cost, uint32_t* __restrict__ live) {
    __shared__ float s_cost[HG_LBVH_SAH_SLOTS][kBlock];
    const uint32_t i = blockIdx.x * uint32_t(kBlock) + threadIdx.x;
    if (i + 1 >= n_tris) return;
    hg_lbvh_sah_node(topo, tris, int32_t(i), node_cost, &s_cost[0][threadIdx.x], uint32_t(kBlock), live);
}

// One lane per live node: record rec_min + new index gets its two refs (boxes zero until the refit writes them, as
// hg_lbvh_topology leaves them), and refs[new index] the same two refs for the host
__global__ __launch_bounds__(kBlock) void hg_lbvh_sah_emit(const HgLbvhNode* __restrict__ topo,
                                                           const uint32_t* __restrict__ live,
                                                           const uint32_t* __restrict__ new_index, uint32_t n_tris,
                                                           uint32_t rec_min, uint32_t tri_offset,
                                                           float4* __restrict__ nodes, uint2* __restrict__ refs) {
    const uint32_t i = blockIdx.x * uint32_t(kBlock) + threadIdx.x;
    if (i + 1 >= n_tris || !live[i]) return;
    uint32_t ref[2];
    hg_lbvh_sah_refs(topo, live, new_index, int32_t(i), rec_min, tri_offset, ref);
    const uint32_t j = new_index[i];
    float4* q = nodes + size_t(rec_min + j) * 4;
    q[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ref[0]));
    q[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ref[1]));
    q[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    q[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    refs[j] = make_uint2(ref[0], ref[1]);
}

struct RebuildArgs {
    hg_ctx::RebuildSlot slot;
    uint32_t L = 0, K = 0;
};

// What both kinds of rebuild check after a refit's checks and their own argument's: the triangle count, the range of
// inline leaf refs; and the tree's slot of records
int rebuild_check_mesh(hg_ctx* c, int32_t mesh_index, int32_t n_tris, const hg_ctx::RefitTree* tree,
                       hg_ctx::RebuildSlot& slot) {
    if (uint32_t(n_tris) != tree->plan.extent || n_tris == 0)
        return fail(c, HG_E_INVALID, "hg_rebuild_mesh: mesh %d: %d triangles, its tree holds %u", mesh_index, n_tris,
                    tree->plan.extent);
    const HgDevMesh& dm = c->dev_meshes[size_t(mesh_index)];
    if (uint64_t(dm.tri_offset) + uint64_t(n_tris) > uint64_t(HG_LBVH_MAX_TRIS))
        return fail(c, HG_E_UNSUPPORTED, "hg_rebuild_mesh: mesh %d: triangles %u + %d past 2^27 (inline leaves only)",
                    mesh_index, dm.tri_offset, n_tris);
    auto it = c->rebuild_slots.find(dm.tri_offset);
    if (it != c->rebuild_slots.end()) {
        slot = it->second;
    } else {  // not rebuilt since the last full upload: the plan is the uploaded tree's
        slot.rec_min = tree->plan.records.empty() ? 0u : tree->plan.rec_min;
        slot.capacity = tree->plan.records.empty() ? 0u : tree->plan.rec_span;
    }
    return HG_OK;
}

// Everything a rebuild checks before the first device write: a refit's checks, then its own
int rebuild_check(hg_ctx* c, int32_t mesh_index, const void* tris, int32_t n_tris, int32_t leaf_size,
                  std::vector<int32_t>& instances, RebuildArgs& a) {
    hg_ctx::RefitTree* tree = nullptr;
    if (int rc = refit_check(c, mesh_index, tris, n_tris, tree, instances)) return rc;
    if (leaf_size < 0 || leaf_size > int32_t(HG_LBVH_MAX_LEAF))
        return fail(c, HG_E_INVALID, "hg_rebuild_mesh: leaf_size %d outside 0..%u", leaf_size, HG_LBVH_MAX_LEAF);
    if (int rc = rebuild_check_mesh(c, mesh_index, n_tris, tree, a.slot)) return rc;
    a.L = leaf_size ? uint32_t(leaf_size) : hg_lbvh_auto_leaf(uint32_t(n_tris), a.slot.capacity);
    if (a.L == 0)
        return fail(c, HG_E_UNSUPPORTED, "hg_rebuild_mesh: mesh %d: no leaf size up to %u fits %d triangles into %u records",
                    mesh_index, HG_LBVH_MAX_LEAF, n_tris, a.slot.capacity);
    a.K = hg_lbvh_leaf_count(uint32_t(n_tris), a.L);
    if (a.K - 1 > a.slot.capacity)
        return fail(c, HG_E_UNSUPPORTED, "hg_rebuild_mesh: mesh %d: %u records at leaf size %u, the tree's capacity is %u",
                    mesh_index, a.K - 1, a.L, a.slot.capacity);
    return HG_OK;
}

// The order of both kinds of rebuild, into the context's scratch (nothing of the scene is written): key points, bounds,
// codes, the sort.  Leaves the sorted codes in c->lbvh.codes_sorted and the order in c->lbvh.index_sorted, and
// c->lbvh.tris large enough for the gather.
int sort_device(hg_ctx* c, const void* d_tris, uint32_t n) {
    hg_ctx::Lbvh& B = c->lbvh;
    const uint32_t blocks = (n + kBlock - 1) / kBlock;
    size_t temp_bytes = 0;
    HG_HIP(c, rocprim::radix_sort_pairs(nullptr, temp_bytes, static_cast<uint32_t*>(nullptr),
                                        static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                        static_cast<uint32_t*>(nullptr), size_t(n), 0u, 30u, c->stream));
    int rc;
    if ((rc = ensure(c, B.points, size_t(n) * 3 * sizeof(float)))) return rc;
    if ((rc = ensure(c, B.partial, size_t(blocks) * 6 * sizeof(float)))) return rc;
    if ((rc = ensure(c, B.bounds, 6 * sizeof(float)))) return rc;
    for (DevBuf* b : {&B.codes, &B.index, &B.codes_sorted, &B.index_sorted})
        if ((rc = ensure(c, *b, size_t(n) * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, B.sort_temp, temp_bytes))) return rc;
    if ((rc = ensure(c, B.tris, size_t(n) * sizeof(HalogenTriangle)))) return rc;

    const float* src = static_cast<const float*>(d_tris);
    if ((reinterpret_cast<uintptr_t>(d_tris) & 15u) == 0)
        hipLaunchKernelGGL(hg_lbvh_points<true>, dim3(blocks), dim3(kBlock), 0, c->stream, src, n,
                           static_cast<float*>(B.points.p), static_cast<float*>(B.partial.p));
    else
        hipLaunchKernelGGL(hg_lbvh_points<false>, dim3(blocks), dim3(kBlock), 0, c->stream, src, n,
                           static_cast<float*>(B.points.p), static_cast<float*>(B.partial.p));
    HG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(hg_lbvh_bounds, dim3(1), dim3(kBlock), 0, c->stream, static_cast<const float*>(B.partial.p),
                       blocks, static_cast<float*>(B.bounds.p));
    HG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(hg_lbvh_codes, dim3(blocks), dim3(kBlock), 0, c->stream, static_cast<const float*>(B.points.p),
                       static_cast<const float*>(B.bounds.p), n, static_cast<uint32_t*>(B.codes.p),
                       static_cast<uint32_t*>(B.index.p));
    HG_HIP(c, hipGetLastError());
    HG_HIP(c, rocprim::radix_sort_pairs(B.sort_temp.p, temp_bytes, static_cast<uint32_t*>(B.codes.p),
                                        static_cast<uint32_t*>(B.codes_sorted.p), static_cast<uint32_t*>(B.index.p),
                                        static_cast<uint32_t*>(B.index_sorted.p), size_t(n), 0u, 30u, c->stream));
    return HG_OK;
}

int finish_device(hg_ctx* c, int32_t mesh_index, const std::vector<int32_t>& instances, const hg_ctx::RebuildSlot& slot,
                  uint32_t n_records, int32_t n_tris, uint64_t geometry_generation);

// The build and the refit, for a quiesced context.  d_tris: n_tris HalogenTriangle on the device, 4-byte aligned;
// d_order: optional.  The order is left in c->lbvh.index_sorted as well.
int rebuild_device(hg_ctx* c, int32_t mesh_index, const std::vector<int32_t>& instances, const RebuildArgs& a,
                   const void* d_tris, int32_t n_tris, void* d_order, uint64_t geometry_generation) {
    hg_ctx::Lbvh& B = c->lbvh;
    const uint32_t n = uint32_t(n_tris), L = a.L, K = a.K, rec_min = a.slot.rec_min;
    const HgDevMesh first = c->dev_meshes[size_t(instances[0])];
    const uint32_t blocks = (n + kBlock - 1) / kBlock;
    if (int rc = ensure(c, B.refs, size_t(K) * sizeof(uint2))) return rc;
    c->guides_valid = false;
    if (int rc = sort_device(c, d_tris, n)) return rc;
    const float* src = static_cast<const float*>(d_tris);
    c->geometry_stale = true;  // (from the next launch on the device is no longer the last upload's, whatever fails)
    if (K > 1) {
        hipLaunchKernelGGL(hg_lbvh_topology, dim3((K - 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                           static_cast<const uint32_t*>(B.codes_sorted.p), n, L, K, rec_min, first.tri_offset,
                           static_cast<float4*>(c->nodes.p), static_cast<uint2*>(B.refs.p));
        HG_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(hg_lbvh_gather, dim3(blocks), dim3(kBlock), 0, c->stream, src,
                       static_cast<const uint32_t*>(B.index_sorted.p), n, static_cast<float*>(B.tris.p),
                       static_cast<int32_t*>(d_order));
    HG_HIP(c, hipGetLastError());
    return finish_device(c, mesh_index, instances, a.slot, K - 1, n_tris, geometry_generation);
}

// What follows the records of either kind of rebuild: n_records records from slot.rec_min on hold the new tree's refs
// (c->lbvh.refs has the compact copy) and c->lbvh.tris the triangles in the new order.  The host's picture of the new
// topology (the records' refs, the tree's plan, the root of every instance), then the refit.
int finish_device(hg_ctx* c, int32_t mesh_index, const std::vector<int32_t>& instances, const hg_ctx::RebuildSlot& slot,
                  uint32_t n_records, int32_t n_tris, uint64_t geometry_generation) {
    hg_ctx::Lbvh& B = c->lbvh;
    const uint32_t n = uint32_t(n_tris), rec_min = slot.rec_min;
    const HgDevMesh first = c->dev_meshes[size_t(instances[0])];
    int rc;
    std::vector<uint32_t> refs(size_t(n_records) * 2);
    if (n_records)
        HG_HIP(c, hipMemcpyAsync(refs.data(), B.refs.p, refs.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
    if (!refs.empty()) std::memcpy(&c->rec_refs[size_t(rec_min) * 2], refs.data(), refs.size() * 4);
    const uint32_t root = n_records ? rec_min : (HG_LEAF_BIT | (n << HG_LEAF_CNT_SHIFT) | first.tri_offset);
    hg_ctx::RefitTree t;
    if (!hg_refit_plan(c->rec_refs.data(), c->rec_refs.size() / 2, c->leaf_table.data(), c->leaf_table.size() / 2, root,
                       first.tri_offset, t.plan)) {
        // (cannot happen for sorted keys; the tree's records are overwritten, so the context is left without a scene
        // and nothing else of its bookkeeping is touched: the next call is a full upload)
        c->has_scene = false;
        return fail(c, HG_E_INVALID, "hg_rebuild_mesh: mesh %d: the rebuilt records are not a tree; upload the scene again",
                    mesh_index);
    }
    c->rebuild_slots[first.tri_offset] = slot;
    // the old tree's plan goes; its device list is kept for the new plan (the same size at the same leaf size: no
    // free and allocation, which would synchronise the device, per rebuild)
    const uint64_t old_key = (uint64_t(first.root_ref) << 32) | first.tri_offset;
    auto old = c->refit_trees.find(old_key);
    if (old != c->refit_trees.end()) {
        t.list = old->second.list;
        c->refit_trees.erase(old);
    }
    if (t.plan.records.empty()) release(t.list);
    for (int32_t j : instances) c->dev_meshes[size_t(j)].root_ref = root;
    hg_ctx::RefitTree& tree = c->refit_trees[(uint64_t(root) << 32) | first.tri_offset] = std::move(t);
    if (!tree.plan.records.empty())
        if ((rc = upload(c, tree.list, tree.plan.records.data(), tree.plan.records.size() * sizeof(uint32_t)))) return rc;
    if ((rc = refit_device(c, tree, instances, B.tris.p, n_tris, geometry_generation))) return rc;
    // an index list bound to the tree (hg_set_mesh_vertices) follows the triangles into the new order
    if ((rc = deform_follow_order(c, first.tri_offset, static_cast<const uint32_t*>(B.index_sorted.p), n))) return rc;
    // the traversal's stack: what a full upload of the scene with this tree sets (every mesh's tree has its plan cached:
    // refit_check walked the others)
    uint32_t max_depth = 0;
    for (const HgDevMesh& m : c->dev_meshes) {
        auto it = c->refit_trees.find((uint64_t(m.root_ref) << 32) | m.tri_offset);
        if (it != c->refit_trees.end() && !it->second.plan.level_off.empty())
            max_depth = std::max(max_depth, uint32_t(it->second.plan.level_off.size() - 1));
    }
    c->stack_depth = hg_stack_depth(max_depth);
    c->scene_rebuilds++;
    return HG_OK;
}

// Everything hg_rebuild_mesh_sah* checks before the first device launch: a refit's checks, the node cost, what every
// rebuild checks.  (Whether the live records fit is known only after the collapse: rebuild_sah_device refuses that,
// still before the first write to the scene.)
int rebuild_sah_check(hg_ctx* c, int32_t mesh_index, const void* tris, int32_t n_tris, float node_cost,
                      std::vector<int32_t>& instances, hg_ctx::RebuildSlot& slot) {
    hg_ctx::RefitTree* tree = nullptr;
    if (int rc = refit_check(c, mesh_index, tris, n_tris, tree, instances)) return rc;
    if (!(node_cost >= 0.0f) || node_cost == hg_u2f(0x7F800000u))
        return fail(c, HG_E_INVALID, "hg_rebuild_mesh_sah: node_cost %g is negative or not finite", double(node_cost));
    return rebuild_check_mesh(c, mesh_index, n_tris, tree, slot);
}

// The build with leaves chosen by surface area and the refit, for a quiesced context.  The order, the gather into
// scratch, the L = 1 tree, and per rung of the ladder the collapse, the scan and the live count, which the host reads:
// all of it in the context's scratch, so a tree that does not fit is refused with the scene as it was.  Then the
// records, the caller's order, and what every rebuild ends with.
int rebuild_sah_device(hg_ctx* c, int32_t mesh_index, const std::vector<int32_t>& instances,
                       const hg_ctx::RebuildSlot& slot, float node_cost, const void* d_tris, int32_t n_tris,
                       void* d_order, uint64_t geometry_generation) {
    hg_ctx::Lbvh& B = c->lbvh;
    const uint32_t n = uint32_t(n_tris);
    const HgDevMesh first = c->dev_meshes[size_t(instances[0])];
    const uint32_t blocks = (n + kBlock - 1) / kBlock, node_blocks = (n - 1 + kBlock - 1) / kBlock;
    int rc;
    if ((rc = sort_device(c, d_tris, n))) return rc;
    hipLaunchKernelGGL(hg_lbvh_gather, dim3(blocks), dim3(kBlock), 0, c->stream, static_cast<const float*>(d_tris),
                       static_cast<const uint32_t*>(B.index_sorted.p), n, static_cast<float*>(B.tris.p),
                       static_cast<int32_t*>(nullptr));
    HG_HIP(c, hipGetLastError());
    uint32_t n_live = 0;
    if (n > 1) {
        uint32_t* live = nullptr;
        uint32_t* new_index = nullptr;
        size_t temp_bytes = 0;
        HG_HIP(c, rocprim::exclusive_scan(nullptr, temp_bytes, live, new_index, 0u, size_t(n - 1),
                                          rocprim::plus<uint32_t>(), c->stream));
        if ((rc = ensure(c, B.topo, size_t(n - 1) * sizeof(HgLbvhNode)))) return rc;
        if ((rc = ensure(c, B.live, size_t(n - 1) * sizeof(uint32_t)))) return rc;
        if ((rc = ensure(c, B.new_index, size_t(n - 1) * sizeof(uint32_t)))) return rc;
        if ((rc = ensure(c, B.scan_temp, temp_bytes))) return rc;
        live = static_cast<uint32_t*>(B.live.p);
        new_index = static_cast<uint32_t*>(B.new_index.p);
        hipLaunchKernelGGL(hg_lbvh_sah_topology, dim3(node_blocks), dim3(kBlock), 0, c->stream,
                           static_cast<const uint32_t*>(B.codes_sorted.p), n, static_cast<HgLbvhNode*>(B.topo.p));
        HG_HIP(c, hipGetLastError());
        const uint32_t rungs = node_cost == 0.0f ? HG_LBVH_SAH_RUNGS : 1u;
        float used = node_cost;
        bool fits = false;
        for (uint32_t r = 0; r < rungs && !fits; ++r) {
            if (node_cost == 0.0f) used = hg_lbvh_sah_rung(r);
            hipLaunchKernelGGL(hg_lbvh_sah_collapse, dim3(node_blocks), dim3(kBlock), 0, c->stream,
                               static_cast<const HgLbvhNode*>(B.topo.p), static_cast<const HalogenTriangle*>(B.tris.p), n,
                               used, live);
            HG_HIP(c, hipGetLastError());
            HG_HIP(c, rocprim::exclusive_scan(B.scan_temp.p, temp_bytes, live, new_index, 0u, size_t(n - 1),
                                              rocprim::plus<uint32_t>(), c->stream));
            uint32_t last[2] = {0u, 0u};  // of the last node: its new index, its flag
            HG_HIP(c, hipMemcpyAsync(&last[0], new_index + (n - 2), 4, hipMemcpyDeviceToHost, c->stream));
            HG_HIP(c, hipMemcpyAsync(&last[1], live + (n - 2), 4, hipMemcpyDeviceToHost, c->stream));
            HG_HIP(c, hipStreamSynchronize(c->stream));
            n_live = last[0] + last[1];
            fits = n_live <= slot.capacity;
        }
        if (!fits && node_cost == 0.0f)
            return fail(c, HG_E_UNSUPPORTED,
                        "hg_rebuild_mesh_sah: mesh %d: %u records at node cost %g, the last of the ladder; the tree's "
                        "capacity is %u", mesh_index, n_live, double(used), slot.capacity);
        if (!fits)
            return fail(c, HG_E_UNSUPPORTED, "hg_rebuild_mesh_sah: mesh %d: %u records at node cost %g, the tree's capacity is %u",
                        mesh_index, n_live, double(used), slot.capacity);
    }
    if ((rc = ensure(c, B.refs, size_t(std::max(n_live, 1u)) * sizeof(uint2)))) return rc;
    c->guides_valid = false;
    c->geometry_stale = true;  // (from the next launch on the device is no longer the last upload's, whatever fails)
    if (n_live) {
        hipLaunchKernelGGL(hg_lbvh_sah_emit, dim3(node_blocks), dim3(kBlock), 0, c->stream,
                           static_cast<const HgLbvhNode*>(B.topo.p), static_cast<const uint32_t*>(B.live.p),
                           static_cast<const uint32_t*>(B.new_index.p), n, slot.rec_min, first.tri_offset,
                           static_cast<float4*>(c->nodes.p), static_cast<uint2*>(B.refs.p));
        HG_HIP(c, hipGetLastError());
    }
    if (d_order)
        HG_HIP(c, hipMemcpyAsync(d_order, B.index_sorted.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                 c->stream));
    return finish_device(c, mesh_index, instances, slot, n_live, n_tris, geometry_generation);
}

}  // namespace

extern "C" {

int hg_rebuild_mesh_sah_device(hg_ctx* c, int32_t mesh_index, const void* d_tris, int32_t n_tris, float node_cost,
                               void* d_order, uint64_t geometry_generation) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    std::vector<int32_t> instances;
    hg_ctx::RebuildSlot slot;
    if (int rc = rebuild_sah_check(c, mesh_index, d_tris, n_tris, node_cost, instances, slot)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_tris) & 3u) || (reinterpret_cast<uintptr_t>(d_order) & 3u))
        return fail(c, HG_E_INVALID, "hg_rebuild_mesh_sah_device: the triangle and order arrays must be 4-byte aligned");
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;  // no trace in flight reads the arrays rewritten below
    return rebuild_sah_device(c, mesh_index, instances, slot, node_cost, d_tris, n_tris, d_order, geometry_generation);
}

int hg_rebuild_mesh_sah(hg_ctx* c, int32_t mesh_index, const HalogenTriangle* tris, int32_t n_tris, float node_cost,
                        int32_t* order, uint64_t geometry_generation) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    std::vector<int32_t> instances;
    hg_ctx::RebuildSlot slot;
    if (int rc = rebuild_sah_check(c, mesh_index, tris, n_tris, node_cost, instances, slot)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;
    const size_t bytes = size_t(n_tris) * sizeof(HalogenTriangle);
    if (int rc = ensure(c, c->refit_in, bytes)) return rc;
    HG_HIP(c, hipMemcpyAsync(c->refit_in.p, tris, bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = rebuild_sah_device(c, mesh_index, instances, slot, node_cost, c->refit_in.p, n_tris, nullptr,
                                    geometry_generation))
        return rc;
    if (order)
        HG_HIP(c, hipMemcpy(order, c->lbvh.index_sorted.p, size_t(n_tris) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HG_OK;
}

int hg_rebuild_mesh_device(hg_ctx* c, int32_t mesh_index, const void* d_tris, int32_t n_tris, int32_t leaf_size,
                           void* d_order, uint64_t geometry_generation) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    std::vector<int32_t> instances;
    RebuildArgs a;
    if (int rc = rebuild_check(c, mesh_index, d_tris, n_tris, leaf_size, instances, a)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_tris) & 3u) || (reinterpret_cast<uintptr_t>(d_order) & 3u))
        return fail(c, HG_E_INVALID, "hg_rebuild_mesh_device: the triangle and order arrays must be 4-byte aligned");
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;  // no trace in flight reads the arrays rewritten below
    return rebuild_device(c, mesh_index, instances, a, d_tris, n_tris, d_order, geometry_generation);
}

int hg_rebuild_mesh(hg_ctx* c, int32_t mesh_index, const HalogenTriangle* tris, int32_t n_tris, int32_t leaf_size,
                    int32_t* order, uint64_t geometry_generation) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    std::vector<int32_t> instances;
    RebuildArgs a;
    if (int rc = rebuild_check(c, mesh_index, tris, n_tris, leaf_size, instances, a)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;
    const size_t bytes = size_t(n_tris) * sizeof(HalogenTriangle);
    if (int rc = ensure(c, c->refit_in, bytes)) return rc;
    HG_HIP(c, hipMemcpyAsync(c->refit_in.p, tris, bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = rebuild_device(c, mesh_index, instances, a, c->refit_in.p, n_tris, nullptr, geometry_generation))
        return rc;
    if (order)
        HG_HIP(c, hipMemcpy(order, c->lbvh.index_sorted.p, size_t(n_tris) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HG_OK;
}

}  // extern "C"
