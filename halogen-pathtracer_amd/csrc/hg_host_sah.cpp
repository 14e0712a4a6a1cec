// hg_host_sah.cpp — the binned-SAH BLAS builder on the host (product code).
//
// Fast BLAS ("an SAH variant behind a non-parity flag"): a binned surface-area-heuristic build
// that emits the reference's BVHEntry format — children of entry g at indexA and indexA + 1, leaves holding a range of
// the reordered triangle list — so hg_upload_scene, the traversal and the CPU oracle take it unchanged.  Its images are
// those of a different (valid) hierarchy, not the reference builder's: rays find the same nearest triangle except
// where two lie within rounding of each other, and every traversal counter differs.  The GPU render of an SAH
// hierarchy is still bit-exact against the oracle's render of the same hierarchy (tests/test_gpu_fast_bvh.py).
// Boxes are their triangles' float min / max through the reference's Bounds arithmetic (padded when thin).  The exact
// tree is pinned (tests/test_bvh_sah.py), so every box here is folded new value first (hg_host_bounds.h).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "halogen_abi.h"
#include "hg_host_bounds.h"

using namespace hg_host;

namespace {

double area(const Box& b) {
    if (!(b.mx[0] >= b.mn[0])) return 0.0;
    const double dx = double(b.mx[0]) - b.mn[0], dy = double(b.mx[1]) - b.mn[1], dz = double(b.mx[2]) - b.mn[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

constexpr int kSahBins = 32;

// The bin of a centroid coordinate: computed and clamped in float, so that no float -> int conversion is out of range
// (a centroid span of a few ulps gives a scale near FLT_MAX, and (c - lo) * scale may then overflow to inf)
inline int sah_bin(float c, float lo, float scale) {
    const float f = (c - lo) * scale;
    if (!(f > 0.0f)) return 0;
    if (!(f < float(kSahBins - 1))) return kSahBins - 1;
    return int(f);
}

}  // namespace

extern "C" int64_t hg_build_blas_sah(const float* V, int32_t n_vertices, int32_t* idx, int32_t n_tris,
                                     int32_t max_leaf, int32_t max_depth, BVHEntry* out_nodes, int64_t max_nodes) {
    if (!V || !idx || n_tris < 0 || n_vertices < 0 || max_leaf < 1 || max_leaf > 15 || max_depth < 1) return HG_E_INVALID;
    for (int64_t i = 0; i < 3 * int64_t(n_tris); ++i) {
        if (idx[i] < 0 || idx[i] >= n_vertices) return HG_E_INVALID;
        const float* p = V + 3 * size_t(idx[i]);  // a NaN or infinite vertex has no box (and no bin)
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return HG_E_INVALID;
    }
    const size_t n = size_t(n_tris);
    std::vector<Box> tb(n);
    std::vector<float> cen(3 * n);
    for (size_t t = 0; t < n; ++t) {
        for (int v = 0; v < 3; ++v) tb[t].add_keep_first(V + 3 * size_t(idx[3 * t + v]));
        for (int k = 0; k < 3; ++k) cen[3 * t + k] = 0.5f * tb[t].mn[k] + 0.5f * tb[t].mx[k];
    }
    std::vector<uint32_t> ord(n);  // triangle order; idx is rewritten from it at the end
    for (size_t t = 0; t < n; ++t) ord[t] = uint32_t(t);
    std::vector<BVHEntry> nodes;
    nodes.reserve(2 * n + 1);
    // boxes through the reference's Bounds arithmetic (centre / extents round trip, and the AABBEpsilon pad of a box
    // thinner than it on any axis, BVHGenerator.cs:154-186): a flat wall's leaves keep the thickness every traversal
    // of the reference relies on
    auto entry = [&](uint32_t first, uint32_t count, const Box& b) { return MakeEntry(PaddedBounds(b), first, count); };
    auto range_box = [&](uint32_t first, uint32_t count) {
        Box b;
        for (uint32_t i = first; i < first + count; ++i) b.add_keep_first(tb[ord[i]]);
        return b;
    };
    nodes.push_back(entry(0, uint32_t(n), range_box(0, uint32_t(n))));
    if (n == 0) nodes[0].triangleCount = 0, nodes[0].indexA = 0;
    struct Job {
        uint32_t node, depth;
    };
    std::vector<Job> jobs{{0u, 0u}};
    while (!jobs.empty()) {
        const Job j = jobs.back();
        jobs.pop_back();
        const uint32_t first = nodes[j.node].indexA, count = nodes[j.node].triangleCount;
        if (count <= uint32_t(max_leaf) || j.depth + 1 >= uint32_t(max_depth)) {
            if (count > 15u && j.depth + 1 >= uint32_t(max_depth)) return HG_E_UNSUPPORTED;  // too deep to split
            continue;
        }
        Box cb;  // centroid bounds
        for (uint32_t i = first; i < first + count; ++i) cb.add_keep_first(&cen[3 * size_t(ord[i])]);
        int best_axis = -1;
        uint32_t best_bin = 0;
        double best_cost = std::numeric_limits<double>::infinity();
        for (int ax = 0; ax < 3; ++ax) {
            const float ext = cb.mx[ax] - cb.mn[ax];
            const float scale = float(kSahBins) / ext;
            if (!(ext > 0.0f) || !(scale < FLT_MAX)) continue;  // one centroid plane (or a span of denormals)
            Box bins[kSahBins];
            uint32_t cnt[kSahBins] = {};
            for (uint32_t i = first; i < first + count; ++i) {
                const uint32_t t = ord[i];
                const int b = sah_bin(cen[3 * size_t(t) + ax], cb.mn[ax], scale);
                bins[b].add_keep_first(tb[t]);
                cnt[b]++;
            }
            double right_area[kSahBins];
            uint32_t right_cnt[kSahBins];
            Box acc;
            uint32_t c = 0;
            for (int b = kSahBins - 1; b > 0; --b) {
                acc.add_keep_first(bins[b]);
                c += cnt[b];
                right_area[b] = area(acc);
                right_cnt[b] = c;
            }
            Box left;
            uint32_t lc = 0;
            for (int b = 0; b < kSahBins - 1; ++b) {
                left.add_keep_first(bins[b]);
                lc += cnt[b];
                if (lc == 0 || right_cnt[b + 1] == 0) continue;
                const double cost = area(left) * lc + right_area[b + 1] * right_cnt[b + 1];
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = ax;
                    best_bin = uint32_t(b);
                }
            }
        }
        const double parent_area = nodes[j.node].triangleCount ? area(range_box(first, count)) : 0.0;
        // leaf if no split separates the centroids, or (small enough to be an inline leaf) splitting costs more than
        // testing every triangle (traversal step ~ one triangle test)
        uint32_t mid = first;
        if (best_axis >= 0) {
            const float ext = cb.mx[best_axis] - cb.mn[best_axis], scale = float(kSahBins) / ext;
            uint32_t* lo = ord.data() + first;
            uint32_t* hi = ord.data() + first + count;
            while (lo < hi) {
                const int b = sah_bin(cen[3 * size_t(*lo) + best_axis], cb.mn[best_axis], scale);
                if (uint32_t(b) <= best_bin) ++lo;
                else std::swap(*lo, *--hi);
            }
            mid = uint32_t(lo - ord.data());
            if (count <= 15u && parent_area > 0.0 && 1.0 + best_cost / parent_area >= double(count)) continue;
        }
        if (mid == first || mid == first + count) {  // degenerate centroids: split the range in half
            if (count <= 15u) continue;
            mid = first + count / 2;
        }
        const uint32_t a = uint32_t(nodes.size());
        nodes.push_back(entry(first, mid - first, range_box(first, mid - first)));
        nodes.push_back(entry(mid, first + count - mid, range_box(mid, first + count - mid)));
        nodes[j.node].indexA = a;
        nodes[j.node].triangleCount = 0;
        jobs.push_back({a + 1, j.depth + 1});
        jobs.push_back({a, j.depth + 1});
    }
    std::vector<int32_t> re(3 * n);
    for (size_t i = 0; i < n; ++i)
        for (int v = 0; v < 3; ++v) re[3 * i + v] = idx[3 * size_t(ord[i]) + v];
    if (!re.empty()) std::memcpy(idx, re.data(), re.size() * sizeof(int32_t));
    const int64_t nn = int64_t(nodes.size());
    if (out_nodes) {
        if (nn > max_nodes) return -(nn + 1);
        std::memcpy(out_nodes, nodes.data(), size_t(nn) * sizeof(BVHEntry));
    }
    return nn;
}
