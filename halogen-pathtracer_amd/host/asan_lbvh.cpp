// asan_lbvh.cpp — hg_build_blas_lbvh (hg_host_lbvh.cpp over csrc/hg_lbvh.h), the host twin of the device rebuild,
// under AddressSanitizer + UBSan (make asan_lbvh; tests/test_lbvh.py), on the input classes of the CPU tests: meshes of
// every small count, identical triangles, meshes flat on one, two and three axes, tiny, huge and denormal extents, sums
// that overflow, key points one ulp apart, a key point at pmax, NaN coordinates.  Whatever the input: a code or a tree
// that is a partition of the triangles, no deeper than the bound, which hg_refit_blas leaves as it is; nothing outside
// the arrays is touched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "lbvh_check.h"

static void run(const std::vector<HalogenTriangle>& tris, int32_t L) {
    const int32_t n = int32_t(tris.size());
    const uint32_t K = hg_lbvh_leaf_count(uint32_t(n), uint32_t(L));
    // exactly the sizes the call may write: the sanitizer sees a step past any of them
    std::vector<int32_t> order(size_t(n), -1);
    std::vector<HalogenTriangle> out(static_cast<size_t>(n));
    std::vector<BVHEntry> nodes(size_t(2 * K - 1));
    EXPECT(hg_build_blas_lbvh(tris.data(), n, L, order.data(), out.data(), nodes.data(), int64_t(nodes.size()) - 1) ==
           -(int64_t(nodes.size()) + 1));
    const int64_t rc = hg_build_blas_lbvh(tris.data(), n, L, order.data(), out.data(), nodes.data(), int64_t(nodes.size()));
    EXPECT(rc == int64_t(nodes.size()));
    if (rc < 0) return;
    if (!check_order(tris, order, out)) return;
    check_tree(nodes, out, uint32_t(L), uint32_t(L), K);  // leaves a partition in steps of L
}

int main() {
    std::mt19937 rng(2468);
    const int32_t leaf_sizes[] = {1, 4, 15};
    for (int32_t L : leaf_sizes) {
        for (int n : {1, 2, L, L + 1, 12, 200, 4097}) run(make(rng, n, -4.0f, 4.0f, 0), L);
        std::vector<HalogenTriangle> same = make(rng, 1, -1.0f, 1.0f, 0);
        same.resize(100, same[0]);
        run(same, L);
        for (int mask : {2, 5, 7}) run(make(rng, 60, -2.0f, 2.0f, mask), L);
        run(make(rng, 60, 0.0f, 1e-30f, 0), L);
        run(make(rng, 60, -1e30f, 1e30f, 0), L);
        std::vector<HalogenTriangle> den = make(rng, 60, 0.0f, 1e-40f, 0);
        std::memset(&den[5].pointA, 0, 36);
        run(den, L);
        std::vector<HalogenTriangle> over = make(rng, 60, -1.0f, 1.0f, 0);
        for (size_t k = 0; k < over.size(); k += 2) over[k] = make(rng, 1, 3.0e38f, 3.3e38f, 0)[0];
        run(over, L);
        // two point triangles whose key points differ by one ulp in x; point triangles at (0, 0, 0) and (1, 1, 1), so the
        // extent is 2, the scale exactly 512 and the key point at pmax lands, unclamped, exactly on 1024
        std::vector<HalogenTriangle> ulp = make(rng, 12, 0.1f, 0.9f, 0);
        auto point = [](HalogenTriangle& h, float x, float y, float z) { h.pointA = h.pointB = h.pointC = {x, y, z}; };
        point(ulp[3], 0.5f, 0.75f, 0.25f);
        point(ulp[4], std::nextafter(0.5f, 1.0f), 0.75f, 0.25f);
        point(ulp[0], 0.0f, 0.0f, 0.0f);
        point(ulp[11], 1.0f, 1.0f, 1.0f);
        {
            float p[3], lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {2.0f, 2.0f, 2.0f};
            hg_lbvh_key_point(ulp[11], p);
            EXPECT(p[0] == 2.0f && (p[0] - lo[0]) * (1024.0f / (hi[0] - lo[0])) == 1024.0f);
            EXPECT(hg_lbvh_cell(p[0], lo[0], hi[0]) == 1023u);
            float q[3];
            hg_lbvh_key_point(ulp[3], p);
            hg_lbvh_key_point(ulp[4], q);
            EXPECT(p[0] == 1.0f && q[0] == std::nextafter(1.0f, 2.0f));
        }
        run(ulp, L);
        std::vector<HalogenTriangle> nan = make(rng, 60, -1.0f, 1.0f, 0);
        nan[7].pointA.x = nan[8].pointB.y = std::numeric_limits<float>::quiet_NaN();
        nan[9].pointA.z = nan[9].pointB.z = nan[9].pointC.z = std::numeric_limits<float>::quiet_NaN();
        nan[10].pointC.x = std::numeric_limits<float>::infinity();
        run(nan, L);
        std::vector<HalogenTriangle> all_nan = nan;
        for (HalogenTriangle& h : all_nan) h.pointA.x = h.pointB.x = h.pointC.x = std::numeric_limits<float>::quiet_NaN();
        run(all_nan, L);
    }
    // refusals write nothing
    std::vector<HalogenTriangle> t = make(rng, 12, -1.0f, 1.0f, 0);
    int32_t order[12];
    HalogenTriangle out[12];
    BVHEntry nodes[23];
    EXPECT(hg_build_blas_lbvh(t.data(), 0, 4, order, out, nodes, 23) == HG_E_INVALID);
    EXPECT(hg_build_blas_lbvh(t.data(), 12, 0, order, out, nodes, 23) == HG_E_INVALID);
    EXPECT(hg_build_blas_lbvh(t.data(), 12, 16, order, out, nodes, 23) == HG_E_INVALID);
    EXPECT(hg_build_blas_lbvh(nullptr, 12, 4, order, out, nodes, 23) == HG_E_INVALID);
    if (failures) return 1;
    std::printf("asan_lbvh ok\n");
    return 0;
}
