// asan_cull_table.cpp — the cull table (csrc/hg_cull.h) under AddressSanitizer + UBSan, as a stand-alone program
// (make asan_cull_table; tests/test_cull_table_asan.py).  It packs
//   - hand-made scenes: a leaf root and a singular matrix among cullable meshes, 70 meshes (entries below 64 only), no
//     cullable mesh at all, one mesh (an odd number of entries: the zero pad), and a partial re-upload of each;
//   - seeded synthetic mesh tables of 0 to 80 records (children that tile, with a gap, offset, nested; leaf roots and
//     singular matrices between them),
// checks each table's invariants (cull_table_check.h) and walks it as the kernel does, two entries per fetch, for every
// launch length from no mesh to all of them, with rays of every kind the CPU test throws: the walk reads through
// std::vector::at and the sanitizer watches the rest.
// Usage: asan_cull_table [tables] [seed]
#include <cstdlib>

#include "cull_table_check.h"
#include "scene_pack_check.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what, const std::string& detail = "") {
    if (ok) return;
    ++failures;
    std::printf("FAILED: %s %s\n", what, detail.c_str());
}

BVHEntry entry(uint32_t indexA, uint32_t count, float lo_x = -1.0f, float hi_x = 1.0f) {
    return BVHEntry{indexA, count, {lo_x, -1.0f, -1.0f}, {hi_x, 1.0f, 1.0f}};
}

HalogenMeshData mesh(uint32_t off, float x, bool singular = false) {
    HalogenMeshData m{};
    m.accelerationBufferOffset = off;
    for (int i = 0; i < 4; ++i) m.worldToLocal.m[5 * i] = m.localToWorld.m[5 * i] = 1.0f;
    m.worldToLocal.m[12] = -x;
    m.localToWorld.m[12] = x;
    if (singular)
        for (int i = 0; i < 12; ++i) m.worldToLocal.m[i] = 0.0f;
    return m;
}

// a root over two leaves that tile it (offset 0), one over two leaves with a gap (offset 3), a leaf root (offset 6)
HgSceneFile base() {
    HgSceneFile s;
    s.materials.resize(1);
    s.tris.resize(2);
    s.blas = {entry(1, 0), entry(0, 1, -1.0f, 0.0f), entry(1, 1, 0.0f, 1.0f),
              entry(1, 0), entry(0, 1, -1.0f, -0.5f), entry(1, 1, 0.5f, 1.0f), entry(0, 2)};
    return s;
}

// every launch length over the table, every kind of ray: no bit cleared that the two-box test keeps
void walk(const std::vector<HgDevMesh>& dm, const HgCullTable& t, HgCullRng& r, const char* what) {
    const std::string verdict = hg_check_cull_table(dm.data(), dm.size(), t);
    expect(verdict.empty(), what, verdict);
    for (size_t n = 0; n <= dm.size(); ++n) {
        const uint32_t entries = hg_cull_count(t, int32_t(n));
        expect(entries <= t.n, what, "more entries than the table has");
        for (uint64_t i = 0; i < 12; ++i) {
            const HgCullRay ray = hg_cull_ray(r, dm.data(), n, i);
            uint32_t c2 = 0, ct = 0;
            const uint64_t two = hg_two_box_mask(dm.data(), n, ray, c2);
            const uint64_t tab = hg_table_mask(t, entries, ray, ct);
            expect((~tab & two) == 0, what, "the table culls a mesh the two-box test keeps");
            expect(ct == uint32_t(__builtin_popcountll(~tab)), what, "culled count");
        }
    }
}

size_t packed(const HgSceneFile& s, HgCullRng& r, const char* what) {
    HgScenePack p, part, kept;
    HgPackError err;
    const HgSceneIn in = s.in();
    if (hg_scene_check_limits(in, err) || hg_pack_spheres_materials(in, p, err) || hg_pack_geometry(in, p, err)) {
        expect(false, what, err.text);
        return 0;
    }
    walk(p.dm, p.cull, r, what);
    // the partial re-upload of the same arrays, both ways: the same table
    std::vector<HgRootPair> pairs;
    hg_root_pairs(in, pairs);
    expect(!hg_pack_mesh_table(in, p.dm, part, err) && !hg_pack_mesh_table_kept(in, p.dm, pairs, kept, err), what,
           "partial pack refused");
    for (const HgScenePack* q : {&part, &kept})
        expect(q->cull.n == p.cull.n && q->cull.q.size() == p.cull.q.size() &&
                   (p.cull.q.empty() ||
                    !std::memcmp(q->cull.q.data(), p.cull.q.data(), p.cull.q.size() * sizeof(float4))),
               what, "a partial pack's table differs");
    return p.cull.n;
}

void hand_made(HgCullRng& r) {
    HgSceneFile s = base();
    s.meshes = {mesh(6, 0.0f), mesh(0, 5.0f), mesh(3, 10.0f, true), mesh(3, 15.0f)};
    expect(packed(s, r, "leaf root and singular matrix") == 3, "leaf root and singular matrix: 1 + 2 entries");
    s.meshes.clear();
    for (int i = 0; i < 70; ++i) s.meshes.push_back(mesh(i % 2 ? 3 : 0, 3.0f * float(i)));
    expect(packed(s, r, "70 meshes") == 96, "70 meshes: 32 + 64 entries, none for meshes 64-69");
    s.meshes = {mesh(6, 0.0f), mesh(6, 1.0f)};
    expect(packed(s, r, "no cullable mesh") == 0, "no cullable mesh: an empty table");
    s.meshes = {mesh(0, 0.0f)};
    expect(packed(s, r, "one mesh") == 1, "one mesh: one entry and the pad");
    s.meshes.clear();
    expect(packed(s, r, "no mesh") == 0, "no mesh: an empty table");
}

}  // namespace

int main(int argc, char** argv) {
    const int tables = argc > 1 ? std::atoi(argv[1]) : 200;
    HgCullRng r{argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 5ull};
    hand_made(r);
    std::printf("hand-made scenes done\n");
    size_t entries = 0, meshes = 0;
    for (int k = 0; k < tables; ++k) {
        const std::vector<HgDevMesh> dm = hg_cull_synth_table(r, r.below(81));
        HgCullTable t;
        hg_cull_table(dm.data(), dm.size(), t);
        walk(dm, t, r, "synthetic table");
        entries += t.n;
        meshes += dm.size();
    }
    std::printf("%d synthetic tables: %zu records, %zu entries\n", tables, meshes, entries);
    expect(entries > 0 && meshes > entries / 2, "the synthetic tables hold entries");
    if (failures) {
        std::printf("%d FAILED\n", failures);
        return 1;
    }
    std::printf("cull table ok\n");
    return 0;
}
