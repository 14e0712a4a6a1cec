// hg_host_lbvh.cpp — the host twins of the device rebuilds (hg_lbvh.hip), over the two contracts of hg_lbvh.h
// (product code).  The boxes come from hg_refit_blas (hg_host_mesh.cpp).  Compiled with -ffp-contract=off.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "halogen_abi.h"
#include "hg_lbvh.h"

// The order of hg_lbvh.h for one mesh's triangles: key points, grid, codes, the stable sort.  out_order, out_tris and
// `sorted` (the codes in the new order) hold n elements each.
static void lbvh_sort(const HalogenTriangle* tris, uint32_t n, int32_t* out_order, HalogenTriangle* out_tris,
                      std::vector<uint32_t>& sorted) {
    const float inf = std::numeric_limits<float>::infinity();
    float pmin[3] = {inf, inf, inf}, pmax[3] = {-inf, -inf, -inf};
    std::vector<float> pts(size_t(n) * 3);
    for (uint32_t t = 0; t < n; ++t) {
        float* p = &pts[size_t(t) * 3];
        hg_lbvh_key_point(tris[t], p);
        for (int k = 0; k < 3; ++k) {
            pmin[k] = hg_fminf(pmin[k], p[k]);
            pmax[k] = hg_fmaxf(pmax[k], p[k]);
        }
    }
    std::vector<uint32_t> code(n);
    sorted.resize(n);
    for (uint32_t t = 0; t < n; ++t) code[t] = hg_lbvh_code(&pts[size_t(t) * 3], pmin, pmax);
    for (uint32_t t = 0; t < n; ++t) out_order[t] = int32_t(t);
    std::stable_sort(out_order, out_order + n, [&](int32_t a, int32_t b) { return code[size_t(a)] < code[size_t(b)]; });
    for (uint32_t k = 0; k < n; ++k) {
        sorted[k] = code[size_t(out_order[k])];
        out_tris[k] = tris[size_t(out_order[k])];
    }
}

// The depth of the deepest entry below entry 0, or HG_LBVH_MAX_DEPTH + 1 for a tree deeper than that (or cyclic, which
// a defect of the construction could make).  It only measures; hg_refit_blas's walk validates.
static uint32_t lbvh_depth(const BVHEntry* nodes) {
    uint32_t depth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> walk{{0u, 0u}};
    while (!walk.empty()) {
        const auto [g, d] = walk.back();
        walk.pop_back();
        depth = std::max(depth, d);
        if (d > HG_LBVH_MAX_DEPTH) break;
        if (nodes[g].triangleCount) continue;
        walk.push_back({nodes[g].indexA + 1, d + 1});
        walk.push_back({nodes[g].indexA, d + 1});
    }
    return depth;
}

// hg_build_blas_lbvh: the host twin of the device rebuild (hg_lbvh.hip), over the contract of hg_lbvh.h: key points,
// grid, codes, the stable order, leaves of L, Karras' tree; then the boxes by hg_refit_blas.  Entry 0 is the root, the
// children of internal node i are entries 1 + 2i and 2 + 2i.
extern "C" int64_t hg_build_blas_lbvh(const HalogenTriangle* tris, int32_t n_tris, int32_t leaf_size, int32_t* out_order,
                                      HalogenTriangle* out_tris, BVHEntry* out_nodes, int64_t max_nodes) {
    if (!tris || !out_order || !out_tris || !out_nodes || n_tris < 1 || leaf_size < 1 ||
        leaf_size > int32_t(HG_LBVH_MAX_LEAF) || uint32_t(n_tris) > HG_LBVH_MAX_TRIS)
        return HG_E_INVALID;
    const uint32_t n = uint32_t(n_tris), L = uint32_t(leaf_size), K = hg_lbvh_leaf_count(n, L);
    const int64_t n_nodes = 2 * int64_t(K) - 1;
    if (max_nodes < n_nodes) return -(n_nodes + 1);
    std::vector<uint32_t> sorted;
    lbvh_sort(tris, n, out_order, out_tris, sorted);
    auto leaf_entry = [&](uint32_t j) {
        uint32_t first, count;
        hg_lbvh_leaf(n, L, j, first, count);
        return BVHEntry{first, count, {0, 0, 0}, {0, 0, 0}};
    };
    auto inner_entry = [](uint32_t i) { return BVHEntry{1u + 2u * i, 0u, {0, 0, 0}, {0, 0, 0}}; };
    out_nodes[0] = K == 1 ? leaf_entry(0) : inner_entry(0);
    for (uint32_t i = 0; i + 1 < K; ++i) {
        const HgLbvhNode nd = hg_lbvh_node(sorted.data(), L, int32_t(K), int32_t(i));
        const uint32_t g = uint32_t(nd.split);
        out_nodes[1 + 2 * size_t(i)] = nd.first == nd.split ? leaf_entry(g) : inner_entry(g);
        out_nodes[2 + 2 * size_t(i)] = nd.last == nd.split + 1 ? leaf_entry(g + 1) : inner_entry(g + 1);
    }
    // the depth bound of hg_lbvh.h, asserted: a deeper tree would be a defect of the construction
    if (lbvh_depth(out_nodes) > hg_lbvh_depth_bound(K)) return HG_E_UNSUPPORTED;
    if (int rc = hg_refit_blas(out_tris, n_tris, out_nodes, int32_t(n_nodes))) return rc;
    return n_nodes;
}

// hg_build_blas_lbvh_sah: the host twin of the device rebuild with leaves chosen by surface area (hg_lbvh.hip), over
// the second contract of hg_lbvh.h: the order and Karras' tree at L = 1, the collapse of hg_lbvh_sah_node per internal
// node, the exclusive scan of the live flags, the refs of hg_lbvh_sah_refs; then the boxes by hg_refit_blas.  Entry 0
// is the root; the children of the live node with new index j are entries 1 + 2j and 2 + 2j, so the device's record of
// that node is rec_min + j and an inner entry e stands for the record ref rec_min + (indexA(e) - 1) / 2.
extern "C" int64_t hg_build_blas_lbvh_sah(const HalogenTriangle* tris, int32_t n_tris, float node_cost,
                                          int64_t max_records, int32_t* out_order, HalogenTriangle* out_tris,
                                          BVHEntry* out_nodes, int64_t max_nodes, float* out_node_cost) {
    if (!tris || !out_order || !out_tris || !out_nodes || n_tris < 1 || uint32_t(n_tris) > HG_LBVH_MAX_TRIS ||
        !(node_cost >= 0.0f) || node_cost == std::numeric_limits<float>::infinity())
        return HG_E_INVALID;
    const uint32_t n = uint32_t(n_tris);
    std::vector<int32_t> order(n);
    std::vector<HalogenTriangle> sorted_tris(n);
    std::vector<uint32_t> sorted;
    lbvh_sort(tris, n, order.data(), sorted_tris.data(), sorted);
    std::vector<HgLbvhNode> topo(n - 1);
    for (uint32_t i = 0; i + 1 < n; ++i) topo[i] = hg_lbvh_node(sorted.data(), 1u, int32_t(n), int32_t(i));
    std::vector<uint32_t> live(n - 1), new_index(n - 1);
    uint32_t n_live = 0;
    float used = node_cost;
    bool fits = false;
    for (uint32_t r = 0; r < (node_cost == 0.0f ? HG_LBVH_SAH_RUNGS : 1u) && !fits; ++r) {
        if (node_cost == 0.0f) used = hg_lbvh_sah_rung(r);
        float cost[HG_LBVH_SAH_SLOTS];
        for (uint32_t i = 0; i + 1 < n; ++i)
            hg_lbvh_sah_node(topo.data(), sorted_tris.data(), int32_t(i), used, cost, 1u, live.data());
        n_live = 0;
        for (uint32_t i = 0; i + 1 < n; ++i) {
            new_index[i] = n_live;
            n_live += live[i];
        }
        fits = max_records < 0 || int64_t(n_live) <= max_records;
    }
    if (!fits) return HG_E_UNSUPPORTED;  // before anything of the caller's is written
    const int64_t n_nodes = 2 * int64_t(n_live) + 1;
    if (max_nodes < n_nodes) return -(n_nodes + 1);
    auto entry = [](uint32_t ref) {  // (refs at rec_min = 0, tri_offset = 0)
        if (ref & HG_LEAF_BIT)
            return BVHEntry{ref & HG_LEAF_PAYLOAD, (ref & ~HG_LEAF_BIT) >> HG_LEAF_CNT_SHIFT, {0, 0, 0}, {0, 0, 0}};
        return BVHEntry{1u + 2u * ref, 0u, {0, 0, 0}, {0, 0, 0}};
    };
    out_nodes[0] = n_live ? entry(0u) : BVHEntry{0u, n, {0, 0, 0}, {0, 0, 0}};  // (no live node: n <= 15, one leaf)
    for (uint32_t i = 0; i + 1 < n; ++i) {
        if (!live[i]) continue;
        uint32_t ref[2];
        hg_lbvh_sah_refs(topo.data(), live.data(), new_index.data(), int32_t(i), 0u, 0u, ref);
        out_nodes[1 + 2 * size_t(new_index[i])] = entry(ref[0]);
        out_nodes[2 + 2 * size_t(new_index[i])] = entry(ref[1]);
    }
    std::memcpy(out_order, order.data(), size_t(n) * sizeof(int32_t));
    std::memcpy(out_tris, sorted_tris.data(), size_t(n) * sizeof(HalogenTriangle));
    if (out_node_cost) *out_node_cost = used;
    if (lbvh_depth(out_nodes) > hg_lbvh_depth_bound(n)) return HG_E_UNSUPPORTED;
    if (int rc = hg_refit_blas(out_tris, n_tris, out_nodes, int32_t(n_nodes))) return rc;
    return n_nodes;
}
