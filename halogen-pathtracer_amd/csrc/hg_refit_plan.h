// hg_refit_plan.h — the host side of a device refit (hg_refit.hip): the plan of one tree of the device scene, and the
// local boxes of a mesh root's two children that the context keeps for the exact-cull boxes.  Plain functions of
// plain arrays and nothing of HIP (tests/test_refit.py and host/asan_refit.cpp run them with no GPU).
//
// A plan lists the tree's child-pair records (hg_layout.h) grouped by height: a record whose two children are leaves
// has height 1, any other 1 + the larger of its inner children's.  A record of height h reads only triangles and
// records of lower heights, so one launch per height, lowest first, in stream order, refits the tree.  The tree is
// walked through the refs the records themselves hold (q0.w, q1.w), as the traversal follows them: pad records are
// never reached.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hg_tunables.h"

// A.lo, A.hi, B.lo, B.hi of a mesh root's two children, in the mesh's local space (all zero for a leaf root)
struct HgRootPair {
    float box[12];
};

struct HgRefitPlan {
    std::vector<uint32_t> records;    // record numbers, by ascending height
    std::vector<uint32_t> level_off;  // height h (1-based) is records[level_off[h - 1] .. level_off[h])
    uint32_t rec_min = 0, rec_span = 0;  // the records lie in [rec_min, rec_min + rec_span)
    uint32_t extent = 0;              // the tree's leaves cover the mesh-relative triangles [0, extent) at most
};

// The (first global triangle, count) a leaf ref names; false: the ref or its table index is out of range
inline bool hg_refit_leaf_range(uint32_t ref, const uint32_t* leaves, size_t n_leaves, uint32_t& first,
                                uint32_t& count) {
    const uint32_t cnt = (ref >> HG_LEAF_CNT_SHIFT) & HG_LEAF_INLINE_MAX;
    if (cnt) {
        first = ref & HG_LEAF_PAYLOAD;
        count = cnt;
        return true;
    }
    const uint32_t idx = ref & HG_LEAF_PAYLOAD;
    if (idx >= n_leaves) return false;
    first = leaves[2 * size_t(idx)];
    count = leaves[2 * size_t(idx) + 1];
    return true;
}

// The plan of the tree under `root_ref` of a mesh whose triangles start at `tri_offset`.  refs: (q0.w, q1.w) of every
// device record; leaves: (first, count) of every leaf-table entry.  False: the records are not a tree of this scene
// (a ref out of range, a leaf below tri_offset, a record reached while it is open) — cannot happen for what
// hg_pack_geometry laid out.
inline bool hg_refit_plan(const uint32_t* refs, size_t n_records, const uint32_t* leaves, size_t n_leaves,
                          uint32_t root_ref, uint32_t tri_offset, HgRefitPlan& plan) {
    plan = HgRefitPlan{};
    uint64_t extent = 0;
    auto leaf = [&](uint32_t ref) {
        uint32_t first, count;
        if (!hg_refit_leaf_range(ref, leaves, n_leaves, first, count) || first < tri_offset) return false;
        extent = std::max(extent, uint64_t(first - tri_offset) + count);
        return true;
    };
    if (root_ref & HG_LEAF_BIT) {
        if (!leaf(root_ref)) return false;
        plan.extent = uint32_t(std::min<uint64_t>(extent, 0xFFFFFFFFu));
        return extent <= 0xFFFFFFFFu;
    }
    constexpr uint32_t kOpen = 0xFFFFFFFFu;
    std::vector<uint32_t> height(n_records, 0u);  // 0: not reached yet
    std::vector<uint32_t> stack{root_ref}, found;
    uint32_t top = 0;
    while (!stack.empty()) {
        const uint32_t r = stack.back();
        if (r >= n_records) return false;
        const uint32_t c[2] = {refs[2 * size_t(r)], refs[2 * size_t(r) + 1]};
        if (height[r] == 0) {
            height[r] = kOpen;
            for (int k = 1; k >= 0; --k) {
                if (c[k] & HG_LEAF_BIT) {
                    if (!leaf(c[k])) return false;
                } else {
                    if (c[k] >= n_records || height[c[k]] == kOpen) return false;
                    if (height[c[k]] == 0) stack.push_back(c[k]);
                }
            }
        } else {
            stack.pop_back();
            if (height[r] != kOpen) continue;  // reached a second time, already done
            uint32_t h = 0;
            for (int k = 0; k < 2; ++k)
                if (!(c[k] & HG_LEAF_BIT)) h = std::max(h, height[c[k]]);
            height[r] = h + 1;
            top = std::max(top, h + 1);
            found.push_back(r);
        }
    }
    if (extent > 0xFFFFFFFFu) return false;
    plan.extent = uint32_t(extent);
    plan.level_off.assign(size_t(top) + 1, 0u);
    for (uint32_t r : found) plan.level_off[height[r]]++;
    for (uint32_t h = 1; h <= top; ++h) plan.level_off[h] += plan.level_off[h - 1];
    std::vector<uint32_t> at(plan.level_off.begin(), plan.level_off.end() - 1);
    plan.records.resize(found.size());
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t r : found) {
        plan.records[at[height[r] - 1]++] = r;
        lo = std::min(lo, r);
        hi = std::max(hi, r);
    }
    plan.rec_min = lo;
    plan.rec_span = hi - lo + 1;
    return true;
}
