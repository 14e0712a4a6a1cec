// hg_lbvh.hip — hg_rebuild_mesh / hg_rebuild_mesh_device: a new tree for one mesh of the device scene, built on the
// device over the mesh's own triangle and record storage (the contract: hg_lbvh.h; the host twin: hg_build_blas_lbvh,
// hg_host_lbvh.cpp).  Not in the reference.  Here: the kernels, the two builds (build_lbvh_device, build_sah_device:
// step 5 of update_mesh, hg_refit.hip, which checks before them and adopts the tree after them) and the four entry
// points, which fill a MeshUpdate.
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
// to refuse a tree that does not fit (HgMeshTrees::check_sah_records), then one lane per live node writing its record;
// the same refit.
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

}  // namespace

namespace hgrt {

// The records and the sorted triangles of a rebuild with K leaves of L, for a quiesced context.  d_tris: n
// HalogenTriangle on the device, 4-byte aligned; d_order: optional.  Leaves the K - 1 records' refs in c->lbvh.refs, the
// triangles in the new order in c->lbvh.tris and the order in c->lbvh.index_sorted.
int build_lbvh_device(hg_ctx* c, uint32_t tri_offset, const HgMeshTrees::Slot& slot, uint32_t L, uint32_t K,
                      const void* d_tris, uint32_t n, void* d_order) {
    hg_ctx::Lbvh& B = c->lbvh;
    const uint32_t blocks = (n + kBlock - 1) / kBlock;
    if (int rc = ensure(c, B.refs, size_t(K) * sizeof(uint2))) return rc;
    c->guides_valid = false;
    if (int rc = sort_device(c, d_tris, n)) return rc;
    c->geometry_stale = true;  // (from the next launch on the device is no longer the last upload's, whatever fails)
    if (K > 1) {
        hipLaunchKernelGGL(hg_lbvh_topology, dim3((K - 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                           static_cast<const uint32_t*>(B.codes_sorted.p), n, L, K, slot.rec_min, tri_offset,
                           static_cast<float4*>(c->nodes.p), static_cast<uint2*>(B.refs.p));
        HG_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(hg_lbvh_gather, dim3(blocks), dim3(kBlock), 0, c->stream, static_cast<const float*>(d_tris),
                       static_cast<const uint32_t*>(B.index_sorted.p), n, static_cast<float*>(B.tris.p),
                       static_cast<int32_t*>(d_order));
    HG_HIP(c, hipGetLastError());
    return HG_OK;
}

// The same with leaves chosen by surface area.  The order, the gather into scratch, the L = 1 tree, and per rung of the
// ladder the collapse, the scan and the live count, which the host reads: all of it in the context's scratch, so a tree
// that does not fit is refused with the scene as it was.  Then the n_records records and the caller's order.
int build_sah_device(hg_ctx* c, int32_t mesh_index, uint32_t tri_offset, const HgMeshTrees::Slot& slot, float node_cost,
                     const void* d_tris, uint32_t n, void* d_order, uint32_t& n_records) {
    hg_ctx::Lbvh& B = c->lbvh;
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
        HgPackError err;
        if (HgMeshTrees::check_sah_records(mesh_index, n_live, node_cost, used, slot, err)) return fail(c, err);
    }
    if ((rc = ensure(c, B.refs, size_t(std::max(n_live, 1u)) * sizeof(uint2)))) return rc;
    c->guides_valid = false;
    c->geometry_stale = true;  // (from the next launch on the device is no longer the last upload's, whatever fails)
    if (n_live) {
        hipLaunchKernelGGL(hg_lbvh_sah_emit, dim3(node_blocks), dim3(kBlock), 0, c->stream,
                           static_cast<const HgLbvhNode*>(B.topo.p), static_cast<const uint32_t*>(B.live.p),
                           static_cast<const uint32_t*>(B.new_index.p), n, slot.rec_min, tri_offset,
                           static_cast<float4*>(c->nodes.p), static_cast<uint2*>(B.refs.p));
        HG_HIP(c, hipGetLastError());
    }
    if (d_order)
        HG_HIP(c, hipMemcpyAsync(d_order, B.index_sorted.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                 c->stream));
    n_records = n_live;
    return HG_OK;
}

}  // namespace hgrt

extern "C" {

int hg_rebuild_mesh_sah_device(hg_ctx* c, int32_t mesh_index, const void* d_tris, int32_t n_tris, float node_cost,
                               void* d_order, uint64_t geometry_generation) {
    return update_mesh(c, {"hg_rebuild_mesh_sah_device", mesh_index, MeshUpdate::kTriangles, d_tris, nullptr, n_tris, true,
                           HG_DEFORM_REBUILD_SAH, 0, node_cost, d_order, geometry_generation});
}

int hg_rebuild_mesh_sah(hg_ctx* c, int32_t mesh_index, const HalogenTriangle* tris, int32_t n_tris, float node_cost,
                        int32_t* order, uint64_t geometry_generation) {
    return update_mesh(c, {"hg_rebuild_mesh_sah", mesh_index, MeshUpdate::kTriangles, tris, nullptr, n_tris, false,
                           HG_DEFORM_REBUILD_SAH, 0, node_cost, order, geometry_generation});
}

int hg_rebuild_mesh_device(hg_ctx* c, int32_t mesh_index, const void* d_tris, int32_t n_tris, int32_t leaf_size,
                           void* d_order, uint64_t geometry_generation) {
    return update_mesh(c, {"hg_rebuild_mesh_device", mesh_index, MeshUpdate::kTriangles, d_tris, nullptr, n_tris, true,
                           HG_DEFORM_REBUILD, leaf_size, 0.0f, d_order, geometry_generation});
}

int hg_rebuild_mesh(hg_ctx* c, int32_t mesh_index, const HalogenTriangle* tris, int32_t n_tris, int32_t leaf_size,
                    int32_t* order, uint64_t geometry_generation) {
    return update_mesh(c, {"hg_rebuild_mesh", mesh_index, MeshUpdate::kTriangles, tris, nullptr, n_tris, false,
                           HG_DEFORM_REBUILD, leaf_size, 0.0f, order, geometry_generation});
}

}  // extern "C"
