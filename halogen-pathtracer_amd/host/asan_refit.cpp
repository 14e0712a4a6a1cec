// asan_refit.cpp — the host side of a refit under AddressSanitizer + UBSan (make asan_refit; tests/test_refit.py):
// hg_refit_blas (hg_host_mesh.cpp), the refit plan (csrc/hg_refit_plan.h) and the upload decision after a refit
// (csrc/hg_scene_pack.h), on builder output and on corrupted copies of it.  Whatever the input, every call must return
// a code and touch nothing outside its arrays; on good input the refit of unchanged triangles changes nothing.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "expect.h"
#include "hg_scene_pack.h"

struct Mesh {
    std::vector<HalogenTriangle> tris;
    std::vector<BVHEntry> nodes;
};

static Mesh build(std::mt19937& rng, int n_tris, bool flat) {
    std::uniform_real_distribution<float> pos(-4.0f, 4.0f), off(-0.3f, 0.3f);
    std::vector<float> V(size_t(n_tris) * 9), N(size_t(n_tris) * 9, 0.0f);
    std::vector<int32_t> idx(size_t(n_tris) * 3);
    float mn[3] = {1e30f, 1e30f, 1e30f}, mx[3] = {-1e30f, -1e30f, -1e30f};
    for (int t = 0; t < n_tris; ++t) {
        const float c[3] = {pos(rng), flat ? 0.0f : pos(rng), pos(rng)};
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 3; ++k) {
                const float x = (flat && k == 1) ? 0.0f : c[k] + off(rng);
                V[size_t(t) * 9 + v * 3 + k] = x;
                mn[k] = std::min(mn[k], x);
                mx[k] = std::max(mx[k], x);
            }
    }
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = int32_t(i);
    Mesh m;
    m.nodes.resize(size_t(2 * n_tris + 2));
    const int64_t n = hg_build_blas(V.data(), n_tris * 3, idx.data(), n_tris, mn, mx, 32, m.nodes.data(),
                                    int64_t(m.nodes.size()));
    EXPECT(n > 0);
    m.nodes.resize(size_t(std::max<int64_t>(n, 1)));
    m.tris.resize(size_t(n_tris));
    EXPECT(hg_pack_triangles(V.data(), N.data(), n_tris * 3, idx.data(), n_tris, m.tris.data()) == HG_OK);
    return m;
}

int main() {
    std::mt19937 rng(12345);
    for (int round = 0; round < 6; ++round) {
        const int n_tris = round == 0 ? 1 : round == 1 ? 6 : 50 + 400 * round;
        Mesh m = build(rng, n_tris, round == 3);
        // unchanged triangles: unchanged boxes
        std::vector<BVHEntry> nodes = m.nodes;
        EXPECT(hg_refit_blas(m.tris.data(), n_tris, nodes.data(), int32_t(nodes.size())) == HG_OK);
        EXPECT(!std::memcmp(nodes.data(), m.nodes.data(), nodes.size() * sizeof(BVHEntry)));
        // moved triangles: accepted, topology untouched
        std::vector<HalogenTriangle> moved = m.tris;
        for (HalogenTriangle& t : moved) t.pointB.y += 0.5f;
        EXPECT(hg_refit_blas(moved.data(), n_tris, nodes.data(), int32_t(nodes.size())) == HG_OK);
        for (size_t g = 0; g < nodes.size(); ++g)
            EXPECT(nodes[g].indexA == m.nodes[g].indexA && nodes[g].triangleCount == m.nodes[g].triangleCount);
        // corrupted trees: any code, no access outside the arrays, nothing written on a refusal
        std::uniform_int_distribution<uint32_t> any(0u, 0xFFFFFFFFu), small(0u, uint32_t(2 * nodes.size() + 4));
        for (int k = 0; k < 200; ++k) {
            std::vector<BVHEntry> bad = m.nodes;
            const int hits = 1 + k % 3;
            for (int h = 0; h < hits; ++h) {
                BVHEntry& e = bad[any(rng) % bad.size()];
                switch (any(rng) % 4) {
                    case 0: e.indexA = any(rng); break;
                    case 1: e.indexA = small(rng); break;
                    case 2: e.triangleCount = any(rng) % 3 ? small(rng) : any(rng); break;
                    default: e.triangleCount = 0; e.indexA = small(rng) % uint32_t(bad.size()); break;
                }
            }
            const std::vector<BVHEntry> before = bad;
            const int rc = hg_refit_blas(m.tris.data(), n_tris, bad.data(), int32_t(bad.size()));
            EXPECT(rc == HG_OK || rc == HG_E_INVALID || rc == HG_E_UNSUPPORTED);
            if (rc != HG_OK) EXPECT(!std::memcmp(bad.data(), before.data(), bad.size() * sizeof(BVHEntry)));
            const int short_rc = hg_refit_blas(m.tris.data(), n_tris / 2, bad.data(), int32_t(bad.size()));
            EXPECT(short_rc == HG_OK || short_rc == HG_E_INVALID || short_rc == HG_E_UNSUPPORTED);
        }
        // the plan of the packed scene (two instances of the tree), on the packer's refs and on corrupted ones
        HalogenMeshData md[2] = {};
        for (HalogenMeshData& d : md) {
            d.worldToLocal.m[0] = d.worldToLocal.m[5] = d.worldToLocal.m[10] = d.worldToLocal.m[15] = 1.0f;
            d.localToWorld = d.worldToLocal;
        }
        md[1].worldToLocal.m[12] = 2.0f;
        PackedHalogenMaterial mat{};
        const HgSceneIn in{nullptr, 0, md, 2, &mat, 1, m.tris.data(), n_tris, m.nodes.data(), int32_t(m.nodes.size())};
        HgScenePack p;
        HgPackError err;
        EXPECT(hg_pack_geometry(in, p, err) == HG_OK);
        const size_t n_rec = p.rec.size() / 4;
        std::vector<uint32_t> refs(2 * n_rec), leaves(2 * p.leaf.size());
        for (size_t r = 0; r < n_rec; ++r) {
            std::memcpy(&refs[2 * r], &p.rec[4 * r].w, 4);
            std::memcpy(&refs[2 * r + 1], &p.rec[4 * r + 1].w, 4);
        }
        std::memcpy(leaves.data(), p.leaf.data(), leaves.size() * 4);
        HgRefitPlan plan;
        EXPECT(hg_refit_plan(refs.data(), n_rec, leaves.data(), p.leaf.size(), p.dm[0].root_ref, 0, plan));
        EXPECT(plan.extent == uint32_t(n_tris));
        size_t inner = 0;
        for (const BVHEntry& e : m.nodes) inner += e.triangleCount == 0;
        EXPECT(plan.records.size() == inner);
        for (uint32_t r : plan.records) EXPECT(r >= plan.rec_min && r - plan.rec_min < plan.rec_span && r < n_rec);
        for (int k = 0; k < 200; ++k) {
            std::vector<uint32_t> bad = refs;
            bad[any(rng) % bad.size()] = k % 2 ? any(rng) : small(rng);
            HgRefitPlan q;
            if (hg_refit_plan(bad.data(), n_rec, leaves.data(), p.leaf.size(), p.dm[0].root_ref, 0, q))
                for (uint32_t r : q.records) EXPECT(r < n_rec);
            (void)hg_refit_plan(bad.data(), n_rec, leaves.data(), p.leaf.size(), any(rng), any(rng) % 8, q);
        }
        // kept root boxes give a full upload's cull boxes; the decision after a refit
        std::vector<HgRootPair> kept;
        hg_root_pairs(in, kept);
        HgScenePack part;
        EXPECT(hg_pack_mesh_table_kept(in, p.dm, kept, part, err) == HG_OK);
        EXPECT(!std::memcmp(part.dm.data(), p.dm.data(), p.dm.size() * sizeof(HgDevMesh)));
        std::vector<uint8_t> copy[5];
        for (int k = 0; k < 5; ++k) copy_bytes(copy[k], in.src(k), in.bytes(k));
        EXPECT(hg_upload_decide_refit(true, true, copy, 9, 2, n_tris, in.n_nodes, in, 9).kind == HG_UPLOAD_SKIP);
        EXPECT(hg_upload_decide_refit(true, true, copy, 9, 2, n_tris, in.n_nodes, in, 8).kind == HG_UPLOAD_FULL);
        EXPECT(hg_upload_decide_refit(true, true, copy, 9, 2, n_tris, in.n_nodes, in, 0).kind == HG_UPLOAD_FULL);
        EXPECT(hg_upload_decide_refit(true, true, copy, 9, 2, n_tris + 1, in.n_nodes, in, 9).kind == HG_UPLOAD_FULL);
        md[1].worldToLocal.m[12] = 3.0f;
        EXPECT(hg_upload_decide_refit(true, true, copy, 9, 2, n_tris, in.n_nodes, in, 9).kind == HG_UPLOAD_PARTIAL);
        EXPECT(hg_upload_decide_refit(true, false, copy, 9, 2, n_tris, in.n_nodes, in, 8).kind == HG_UPLOAD_PARTIAL);
    }
    if (failures) return 1;
    std::printf("asan_refit ok\n");
    return 0;
}
