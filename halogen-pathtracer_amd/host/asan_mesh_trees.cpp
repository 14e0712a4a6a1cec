// asan_mesh_trees.cpp — the host bookkeeping of the mesh updates under AddressSanitizer + UBSan (make asan_mesh_trees;
// tests/test_mesh_trees.py): csrc/hg_mesh_trees.h driven through host/mesh_trees_check.h on scenes built here, the
// sequences and refusals of the test, and adopt() on adversarial refs.  Whatever the input, every call must return a
// code and touch nothing outside its arrays; a refusal leaves the bookkeeping as it was.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "expect.h"
#include "mesh_trees_check.h"

static bool starts(const std::string& s, const char* with) { return s.rfind(with, 0) == 0; }

// A mesh of n_tris scattered triangles under hg_build_blas's tree, appended to the harness's arrays `instances` times
static void add_mesh(HgTreesHarness& h, std::mt19937& rng, int n_tris, int instances) {
    std::uniform_real_distribution<float> pos(-4.0f, 4.0f), off(-0.3f, 0.3f);
    std::vector<float> V(size_t(n_tris) * 9), N(size_t(n_tris) * 9, 0.0f);
    std::vector<int32_t> idx(size_t(n_tris) * 3);
    float mn[3] = {1e30f, 1e30f, 1e30f}, mx[3] = {-1e30f, -1e30f, -1e30f};
    for (int t = 0; t < n_tris; ++t) {
        const float c[3] = {pos(rng), pos(rng), pos(rng)};
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 3; ++k) {
                const float x = c[k] + off(rng);
                V[size_t(t) * 9 + v * 3 + k] = x;
                mn[k] = std::min(mn[k], x);
                mx[k] = std::max(mx[k], x);
            }
    }
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = int32_t(i);
    std::vector<BVHEntry> nodes(size_t(2 * n_tris + 2));
    const int64_t n = hg_build_blas(V.data(), n_tris * 3, idx.data(), n_tris, mn, mx, 32, nodes.data(), int64_t(nodes.size()));
    EXPECT(n > 0);
    nodes.resize(size_t(std::max<int64_t>(n, 1)));
    std::vector<HalogenTriangle> tris(size_t(n_tris), HalogenTriangle{});
    EXPECT(hg_pack_triangles(V.data(), N.data(), n_tris * 3, idx.data(), n_tris, tris.data()) == HG_OK);
    HalogenMeshData d{};
    d.worldToLocal.m[0] = d.worldToLocal.m[5] = d.worldToLocal.m[10] = d.worldToLocal.m[15] = 1.0f;
    d.localToWorld = d.worldToLocal;
    d.triangleBufferOffset = uint32_t(h.tris.size());
    d.accelerationBufferOffset = uint32_t(h.blas.size());
    for (int k = 0; k < instances; ++k) {
        d.worldToLocal.m[12] = float(k);
        h.meshes.push_back(d);
    }
    h.tris.insert(h.tris.end(), tris.begin(), tris.end());
    h.blas.insert(h.blas.end(), nodes.begin(), nodes.end());
}

int main() {
    std::mt19937 rng(4321);
    std::uniform_int_distribution<uint32_t> any(0u, 0xFFFFFFFFu);
    const int sizes[4] = {1, 6, 450, 30};  // meshes 0, 1, 2 + 3 (two instances), 4
    HgTreesHarness fresh;
    fresh.materials.push_back(PackedHalogenMaterial{});
    for (int k = 0; k < 4; ++k) add_mesh(fresh, rng, sizes[k], k == 2 ? 2 : 1);
    const int mesh_of[4] = {0, 1, 2, 4};
    {   // before any upload, and the refusals of a scene that is there
        HgTreesHarness h = fresh;
        EXPECT(starts(h.refit(0, true, 1), "refused -"));
        EXPECT(h.upload().empty());
        for (const HgDevMesh& m : h.dm) EXPECT(h.trees.plan_of(m) != nullptr);
        const HgTreesHarness::Snapshot before = h.snapshot();
        const float nan = std::nanf("");
        EXPECT(starts(h.refit(-1, true, 1), "refused "));
        EXPECT(starts(h.refit(5, true, 1), "refused "));
        EXPECT(starts(h.refit(2, false, 450), "refused "));
        EXPECT(starts(h.refit(2, true, 449), "refused "));
        EXPECT(starts(h.refit(2, true, -3), "refused "));
        EXPECT(starts(h.refit(4, true, 31), "refused "));
        EXPECT(starts(h.refit(1, true, 7), "refused "));
        EXPECT(starts(h.rebuild(2, true, 450, HG_DEFORM_REBUILD, 16, 0.0f), "refused "));
        EXPECT(starts(h.rebuild(2, true, 450, HG_DEFORM_REBUILD, 1, 0.0f), "refused "));
        EXPECT(starts(h.rebuild(2, true, 449, HG_DEFORM_REBUILD, 4, 0.0f), "refused "));
        EXPECT(starts(h.rebuild(0, true, 0, HG_DEFORM_REBUILD, 4, 0.0f), "refused "));
        for (float cost : {-1.0f, nan, HUGE_VALF}) EXPECT(starts(h.rebuild(3, true, 450, HG_DEFORM_REBUILD_SAH, 0, cost), "refused "));
        EXPECT(starts(h.rebuild(2, true, 450, HG_DEFORM_REBUILD_SAH, 0, 0.01f), "refused "));  // (the late one)
        EXPECT(h.same_as(before));
    }
    {   // the sequences, on every mesh
        HgTreesHarness h = fresh;
        EXPECT(h.upload().empty());
        for (int k = 0; k < 4; ++k) {
            const int m = mesh_of[k], n = sizes[k];
            for (int round = 0; round < 2; ++round) {
                std::string s;
                EXPECT(starts(s = h.rebuild(m, true, n, HG_DEFORM_REBUILD_SAH, 0, 0.0f), "ok ") || (std::puts(s.c_str()), false));
                EXPECT(starts(s = h.rebuild(m, true, n, HG_DEFORM_REBUILD, 0, 0.0f), "ok ") || (std::puts(s.c_str()), false));
                EXPECT(starts(s = h.rebuild(m + (k == 2), true, n, HG_DEFORM_REBUILD, 15, 0.0f), "ok ") || (std::puts(s.c_str()), false));
                EXPECT(starts(s = h.refit(m, true, n), "ok ") || (std::puts(s.c_str()), false));
                EXPECT(!starts(s = h.rebuild(m, true, n, HG_DEFORM_REBUILD, 2, 0.0f), "bad") || (std::puts(s.c_str()), false));
            }
        }
    }
    // adopt() on refs that are not a tree, and on random ones (which may be a tree: then the bookkeeping must still
    // walk without leaving its arrays)
    HgTreesHarness up = fresh;
    EXPECT(up.upload().empty());
    for (const char* what : {"cycle", "range"})
        for (int m : {2, 4}) {
            HgTreesHarness h = up;
            EXPECT(starts(h.adopt_bad(m, what), "refused "));
            EXPECT(starts(h.refit(m, true, 1), "refused "));
        }
    for (int k = 0; k < 400; ++k) {
        HgTreesHarness h = up;
        const int m = k % 2 ? 2 : 4;
        const uint32_t n_rec = uint32_t(h.trees.rec_refs.size() / 2);
        std::vector<uint32_t> refs(2 * size_t(1 + any(rng) % 6));
        for (uint32_t& r : refs) {
            switch (any(rng) % 4) {
                case 0: r = any(rng); break;
                case 1: r = any(rng) % (n_rec + 3); break;
                case 2: r = HG_LEAF_BIT | ((any(rng) % 16) << HG_LEAF_CNT_SHIFT) | (any(rng) % 600); break;
                default: r = HG_LEAF_BIT | (any(rng) % 8); break;  // the leaf table
            }
        }
        const std::string s = h.adopt_bad(m, "given", &refs);
        EXPECT(starts(s, "refused ") || s == "ok adopted" || (std::puts(s.c_str()), false));
        if (s == "ok adopted") {
            (void)h.refit(m, true, 1);
            (void)h.rebuild(m, true, int32_t(h.trees.plan_of(h.dm[size_t(m)])->extent), HG_DEFORM_REBUILD, 0, 0.0f);
        }
    }
    if (failures) return 1;
    std::printf("asan_mesh_trees ok\n");
    return 0;
}
