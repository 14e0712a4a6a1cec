// asan_lbvh_sah.cpp — hg_build_blas_lbvh_sah (hg_host_lbvh.cpp over the second contract of csrc/hg_lbvh.h), the host
// twin of the device rebuild with leaves chosen by surface area, under AddressSanitizer + UBSan (make asan_lbvh_sah;
// tests/test_lbvh_sah.py), on the input classes of the CPU tests: meshes of every count around the largest leaf and
// around a workgroup, identical triangles, meshes flat on one, two and three axes, tiny, huge and denormal extents, sums
// that overflow, NaN and infinite coordinates; at a cheap, the default and a dear inner node, through the ladder and with
// a record limit.  Whatever the input: a code, or a tree whose leaves of 1..15 triangles are a partition, no deeper than
// the bound, which hg_refit_blas leaves as it is; nothing outside the arrays is touched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "lbvh_check.h"

// Returns the inner entries of the tree, or -1
static int64_t run(const std::vector<HalogenTriangle>& tris, float node_cost, int64_t max_records) {
    const int32_t n = int32_t(tris.size());
    std::vector<int32_t> order(size_t(n), -1);
    std::vector<HalogenTriangle> out(static_cast<size_t>(n));
    float used = -1.0f;
    // the count first, from a call with room for every tree; then arrays of exactly the sizes the call may write: the
    // sanitizer sees a step past any of them
    std::vector<BVHEntry> all(size_t(2 * n - 1));
    const int64_t count = hg_build_blas_lbvh_sah(tris.data(), n, node_cost, max_records, order.data(), out.data(), all.data(),
                                                 int64_t(all.size()), &used);
    if (count == HG_E_UNSUPPORTED) {
        EXPECT(max_records >= 0 && used == -1.0f);
        return -1;
    }
    EXPECT(count >= 1 && count % 2 == 1 && count <= int64_t(all.size()));
    if (count < 1) return -1;
    EXPECT(node_cost == 0.0f ? used >= HG_LBVH_SAH_NODE_COST : used == node_cost);
    EXPECT(max_records < 0 || (count - 1) / 2 <= max_records);
    std::vector<BVHEntry> nodes(static_cast<size_t>(count));
    EXPECT(hg_build_blas_lbvh_sah(tris.data(), n, node_cost, max_records, order.data(), out.data(), nodes.data(), count - 1,
                                  nullptr) == -(count + 1));
    EXPECT(hg_build_blas_lbvh_sah(tris.data(), n, node_cost, max_records, order.data(), out.data(), nodes.data(), count,
                                  nullptr) == count);
    EXPECT(!std::memcmp(nodes.data(), all.data(), nodes.size() * sizeof(BVHEntry)));
    if (!check_order(tris, order, out)) return -1;
    if (!check_tree(nodes, out, 1u, HG_LBVH_MAX_LEAF, uint32_t(n))) return -1;  // leaves of 1..15 a partition
    return (count - 1) / 2;
}

static void run_all(const std::vector<HalogenTriangle>& tris) {
    int64_t inner = 0;
    for (float node_cost : {1e-6f, 0.5f, HG_LBVH_SAH_NODE_COST, 64.0f, 1e30f, 0.0f}) inner = run(tris, node_cost, -1);
    // the ladder against a limit: room for the start rung, one record short of it, none at all
    if (inner < 0) return;
    run(tris, 0.0f, inner);
    if (inner > 0) run(tris, 0.0f, inner - 1);
    run(tris, 0.0f, 0);
    run(tris, 1e-6f, 0);
}

// small triangles around random centres: subtrees that are worth a leaf and subtrees that are not
static std::vector<HalogenTriangle> cloud(std::mt19937& rng, int n) {
    std::uniform_real_distribution<float> centre(0.1f, 0.9f), off(-0.05f, 0.05f);
    std::vector<HalogenTriangle> t = make(rng, n, 0.0f, 1.0f, 0);
    for (HalogenTriangle& h : t) {
        const float c[3] = {centre(rng), centre(rng), centre(rng)};
        float* p = &h.pointA.x;
        for (int k = 0; k < 9; ++k) p[k] = c[k % 3] + off(rng);
    }
    return t;
}

int main() {
    std::mt19937 rng(1357);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int n : {1, 2, 3, 14, 15, 16, 17, 31, 200, 257, 4097}) run_all(cloud(rng, n));
    std::vector<HalogenTriangle> same = make(rng, 1, -1.0f, 1.0f, 0);
    same.resize(40, same[0]);
    run_all(same);
    for (int mask : {2, 5, 7}) run_all(make(rng, 60, -2.0f, 2.0f, mask));
    run_all(make(rng, 60, 0.0f, 1e-30f, 0));
    run_all(make(rng, 60, -1e30f, 1e30f, 0));
    std::vector<HalogenTriangle> den = make(rng, 60, 0.0f, 1e-40f, 0);
    std::memset(&den[5].pointA, 0, 36);
    run_all(den);
    std::vector<HalogenTriangle> over = make(rng, 60, -1.0f, 1.0f, 0);
    for (size_t k = 0; k < over.size(); k += 2) over[k] = make(rng, 1, 3.0e38f, 3.3e38f, 0)[0];
    run_all(over);
    std::vector<HalogenTriangle> bad = make(rng, 60, -1.0f, 1.0f, 0);
    bad[7].pointA.x = bad[8].pointB.y = nan;
    bad[9].pointA.z = bad[9].pointB.z = bad[9].pointC.z = nan;
    bad[10].pointC.x = inf;
    bad[11].pointA.x = bad[11].pointB.x = bad[11].pointC.x = inf;  // extent Inf - Inf: a NaN cost
    run_all(bad);
    {   // the NaN rule: the comparison is false, the node stays inner, at any node cost
        std::vector<HalogenTriangle> two(bad.begin() + 11, bad.begin() + 13);
        EXPECT(run(two, 1e30f, -1) == 1);
        EXPECT(std::isnan(hg_lbvh_sah_area(two.data(), 0, 0)));
    }
    std::vector<HalogenTriangle> all_nan = bad;
    for (HalogenTriangle& h : all_nan) h.pointA.x = h.pointB.x = h.pointC.x = nan;
    run_all(all_nan);
    // refusals write nothing
    std::vector<HalogenTriangle> t = cloud(rng, 16);
    int32_t order[16];
    HalogenTriangle out[16];
    BVHEntry nodes[31];
    float used;
    EXPECT(hg_build_blas_lbvh_sah(t.data(), 0, 2.0f, -1, order, out, nodes, 31, &used) == HG_E_INVALID);
    EXPECT(hg_build_blas_lbvh_sah(t.data(), 16, -1.0f, -1, order, out, nodes, 31, &used) == HG_E_INVALID);
    EXPECT(hg_build_blas_lbvh_sah(t.data(), 16, nan, -1, order, out, nodes, 31, &used) == HG_E_INVALID);
    EXPECT(hg_build_blas_lbvh_sah(t.data(), 16, inf, -1, order, out, nodes, 31, &used) == HG_E_INVALID);
    EXPECT(hg_build_blas_lbvh_sah(nullptr, 16, 2.0f, -1, order, out, nodes, 31, &used) == HG_E_INVALID);
    EXPECT(hg_build_blas_lbvh_sah(t.data(), 16, 1e-6f, 0, order, out, nodes, 31, &used) == HG_E_UNSUPPORTED);
    if (failures) return 1;
    std::printf("asan_lbvh_sah ok\n");
    return 0;
}
