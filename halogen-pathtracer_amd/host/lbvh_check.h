// lbvh_check.h — what the two sanitizer programs of the host rebuilds share (asan_lbvh.cpp, asan_lbvh_sah.cpp): the
// triangle generator, and the checks of an order and of a tree that both builds must pass.
#pragma once
#include <algorithm>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "expect.h"
#include "halogen_abi.h"
#include "hg_lbvh.h"

// n triangles with coordinates drawn from [lo, hi), those of the axes in flat_mask all 0.25
static std::vector<HalogenTriangle> make(std::mt19937& rng, int n, float lo, float hi, int flat_mask) {
    std::uniform_real_distribution<float> pos(lo, hi);
    std::vector<HalogenTriangle> t(static_cast<size_t>(n));
    for (HalogenTriangle& h : t) {
        float* p = &h.pointA.x;  // pointA, pointB, pointC: nine floats
        for (int k = 0; k < 9; ++k) p[k] = (flat_mask >> (k % 3)) & 1 ? 0.25f : pos(rng);
        h.normalA = h.normalB = h.normalC = {0.0f, 1.0f, 0.0f};
    }
    return t;
}

// `order` is a permutation of the triangles and `out` holds them in that order.  False: an index out of range.
static bool check_order(const std::vector<HalogenTriangle>& tris, const std::vector<int32_t>& order,
                        const std::vector<HalogenTriangle>& out) {
    const int32_t n = int32_t(tris.size());
    std::vector<int> seen(size_t(n), 0);
    for (int32_t k = 0; k < n; ++k) {
        EXPECT(order[size_t(k)] >= 0 && order[size_t(k)] < n);
        if (order[size_t(k)] < 0 || order[size_t(k)] >= n) return false;
        seen[size_t(order[size_t(k)])]++;
        EXPECT(!std::memcmp(&out[size_t(k)], &tris[size_t(order[size_t(k)])], sizeof(HalogenTriangle)));
    }
    for (int s : seen) EXPECT(s == 1);
    return true;
}

// The walk: every entry once; the leaves a partition of the triangles `out`, each starting at a multiple of leaf_step
// and no larger than max_leaf; depth inside the bound for `leaves` leaves; and hg_refit_blas leaves the tree as it is.
// False: an entry out of range.
static bool check_tree(const std::vector<BVHEntry>& nodes, const std::vector<HalogenTriangle>& out, uint32_t leaf_step,
                       uint32_t max_leaf, uint32_t leaves) {
    const int32_t n = int32_t(out.size());
    std::vector<int> covered(size_t(n), 0);
    std::vector<std::pair<uint32_t, uint32_t>> stack{{0u, 0u}};
    size_t reached = 0;
    uint32_t deepest = 0;
    while (!stack.empty() && reached <= nodes.size()) {
        const auto [g, d] = stack.back();
        stack.pop_back();
        ++reached;
        deepest = std::max(deepest, d);
        EXPECT(g < nodes.size());
        if (g >= nodes.size()) return false;
        const BVHEntry& e = nodes[g];
        if (e.triangleCount) {
            EXPECT(e.indexA % leaf_step == 0 && e.triangleCount <= max_leaf &&
                   uint64_t(e.indexA) + e.triangleCount <= uint64_t(n));
            for (uint32_t t = e.indexA; t < e.indexA + e.triangleCount && t < uint32_t(n); ++t) covered[t]++;
        } else {
            stack.push_back({e.indexA + 1, d + 1});
            stack.push_back({e.indexA, d + 1});
        }
    }
    EXPECT(reached == nodes.size());
    for (int s : covered) EXPECT(s == 1);
    EXPECT(deepest <= hg_lbvh_depth_bound(leaves) && deepest <= HG_LBVH_MAX_DEPTH);
    std::vector<BVHEntry> again = nodes;
    EXPECT(hg_refit_blas(out.data(), n, again.data(), int32_t(again.size())) == HG_OK);
    EXPECT(!std::memcmp(again.data(), nodes.data(), nodes.size() * sizeof(BVHEntry)));
    return true;
}
