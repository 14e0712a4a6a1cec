// asan_scene_pack.cpp — the scene validation and packing of hg_upload_scene (csrc/hg_scene_pack.h) under
// AddressSanitizer + UBSan, as a stand-alone program (make asan_scene_pack; tests/test_sanitizers.py).  It packs
//   - the smallest trees with each shape the layout distinguishes, and every rejection with its code and text;
//   - seeded random valid scenes (leaves of 1 to 40 triangles, 1 to 5 meshes, some instancing an earlier mesh's tree,
//     some with a matrix that cannot be inverted), each checked by the host walk of scene_pack_check.h;
//   - single-field corruptions of them (one mesh offset, indexA or triangleCount replaced by a random value, wide or
//     near the valid range): each must be rejected, or pack into a scene the same walk finds in bounds throughout.
// Usage: asan_scene_pack [scenes] [seed]
#include <cstdlib>
#include <random>

#include "scene_pack_check.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what, const std::string& detail = "") {
    if (ok) return;
    ++failures;
    std::printf("FAILED: %s %s\n", what, detail.c_str());
}

BVHEntry entry(uint32_t indexA, uint32_t count, float lo = -1.0f, float hi = 1.0f) {
    return BVHEntry{indexA, count, {lo, lo, lo}, {hi, hi, hi}};
}

HalogenMeshData mesh(uint32_t toff, uint32_t off, uint32_t material = 0) {
    HalogenMeshData m{};
    m.triangleBufferOffset = toff;
    m.accelerationBufferOffset = off;
    m.materialIndex = material;
    for (int i = 0; i < 4; ++i) m.worldToLocal.m[5 * i] = m.localToWorld.m[5 * i] = 1.0f;
    return m;
}

HgSceneFile base(size_t n_tris, size_t n_materials = 1) {
    HgSceneFile s;
    s.materials.resize(n_materials);
    s.tris.resize(n_tris);
    for (size_t t = 0; t < n_tris; ++t) {
        const float f = float(t);
        s.tris[t] = HalogenTriangle{{f, 0, 0}, {f + 1, 0, 0}, {f, 1, 0}, {0, 0, 1}, {0, 1, 0}, {1, 0, 0}};
    }
    return s;
}

// packs and checks; returns the error text ("" when accepted and sound)
std::string pack(const HgSceneFile& s, HgPackStats& st, int* code = nullptr) {
    const HgSceneIn in = s.in();
    HgScenePack p;
    HgPackError err;
    if (hg_scene_check_limits(in, err) || hg_pack_spheres_materials(in, p, err) || hg_pack_geometry(in, p, err)) {
        if (code) *code = err.code;
        return err.text;
    }
    if (code) *code = HG_OK;
    const std::string walk = hg_check_pack(in, p, st);
    expect(walk.empty(), "accepted scene fails the walk:", walk);
    return "";
}

void rejects(const char* what, const HgSceneFile& s, int code, const char* text) {
    HgPackStats st;
    int got = 0;
    const std::string t = pack(s, st, &got);
    expect(got == code && t == text, what, "-> " + std::to_string(got) + " '" + t + "'");
}

void hand_made() {
    HgPackStats st;
    {  // a single-leaf root: no record but the dummy
        HgSceneFile s = base(3);
        s.blas = {entry(0, 3)};
        s.meshes = {mesh(0, 0)};
        expect(pack(s, st).empty() && st.inner == 0 && st.inline_leaves == 1 && st.not_cullable == 1, "single leaf");
    }
    {  // a 3-entry tree; a 7-entry tree whose root's children are both inner (records 2 and 3 after one pad)
        HgSceneFile s = base(8);
        s.blas = {entry(1, 0), entry(0, 2), entry(2, 2),
                  entry(1, 0), entry(3, 0), entry(5, 0), entry(0, 1), entry(1, 1), entry(2, 1), entry(3, 1)};
        s.meshes = {mesh(0, 0), mesh(4, 3)};
        st = HgPackStats{};
        expect(pack(s, st).empty() && st.inner == 4 && st.paired == 1 && st.pads == 0 && st.cullable == 2, "3 + 7 entries");
        s.meshes = {mesh(4, 3)};  // alone its root takes record 0, so the pair needs a pad at record 1
        st = HgPackStats{};
        expect(pack(s, st).empty() && st.inner == 3 && st.paired == 1 && st.pads == 1, "7 entries, padded pair");
    }
    {  // 15 triangles inline beside 16 through the table; two meshes instancing the tree
        HgSceneFile s = base(31);
        s.blas = {entry(1, 0), entry(0, 15), entry(15, 16)};
        s.meshes = {mesh(0, 0), mesh(0, 0)};
        st = HgPackStats{};
        expect(pack(s, st).empty() && st.inline_leaves == 1 && st.table_leaves == 1 && st.inner == 1, "15 | 16, instanced");
        s.tris.resize(40);
        s.meshes = {mesh(0, 0), mesh(9, 0)};
        rejects("different triangle offsets over one tree", s, HG_E_UNSUPPORTED,
                "BLAS entry 0 shared by meshes with different offsets");
    }
    HgSceneFile s = base(4, 2);
    s.blas = {entry(1, 0), entry(0, 2), entry(2, 2)};
    s.meshes = {mesh(0, 0)};
    HgSceneFile b = s;
    b.spheres.resize(1);
    b.spheres[0].materialIndex = 2;
    rejects("sphere material", b, HG_E_INVALID, "sphere 0: materialIndex 2 out of range");
    b = s;
    b.meshes[0].materialIndex = 7;
    rejects("mesh material", b, HG_E_INVALID, "mesh 0: materialIndex 7 out of range");
    b = s;
    b.meshes[0].accelerationBufferOffset = 3;
    rejects("acceleration offset", b, HG_E_INVALID, "mesh 0: accelerationBufferOffset out of range");
    b = s;
    b.blas[2].triangleCount = 3;
    rejects("leaf range", b, HG_E_INVALID, "mesh 0: leaf 2 references triangles out of range");
    b = s;
    b.blas[0].indexA = 2;  // a + 1 == n_nodes
    rejects("children range", b, HG_E_INVALID, "mesh 0: node 0 has children out of range");
    b = s;
    b.blas[0].indexA = 0;  // the root is its own first child, its sibling a leaf
    rejects("self reference", b, HG_E_UNSUPPORTED, "mesh 0: BLAS deeper than 62 levels (or cyclic)");
    b = base(64);
    for (uint32_t d = 0; d < 63; ++d) {  // a chain: entry 2d inner, 2d + 1 a leaf; the last inner entry at depth 63
        b.blas.push_back(entry(2 * d + 2, 0));
        b.blas.push_back(entry(d, 1));
    }
    b.blas.push_back(entry(63, 1));
    b.blas.push_back(entry(62, 1));
    b.meshes = {mesh(0, 0)};
    rejects("chain of 63", b, HG_E_UNSUPPORTED, "mesh 0: BLAS deeper than 62 levels (or cyclic)");
    b.blas[2 * 62] = entry(0, 1);  // the entry at depth 62 a leaf: the deepest tree that fits the stack
    st = HgPackStats{};
    expect(pack(b, st).empty() && st.max_depth == 62, "chain of 62 accepted");
    b = s;
    b.materials.resize(256);
    rejects("256 materials", b, HG_E_UNSUPPORTED, "at most 255 materials (medium stack packs material indices in bytes)");
    // the size limits look at the counts alone
    HgPackError err;
    HgSceneIn big{};
    big.n_nodes = 1 << 26;
    expect(hg_scene_check_limits(big, err) == HG_E_UNSUPPORTED &&
               err.text == "scene too large: 67108864 BLAS entries (max 2^26-1), 0 triangles (max 2^28-1)",
           "2^26 BLAS entries", err.text);
    big.n_nodes = (1 << 26) - 1;
    big.n_tris = 1 << 28;
    expect(hg_scene_check_limits(big, err) == HG_E_UNSUPPORTED &&
               err.text == "scene too large: 67108863 BLAS entries (max 2^26-1), 268435456 triangles (max 2^28-1)",
           "2^28 triangles", err.text);
    big.n_tris = (1 << 28) - 1;
    big.n_materials = 255;
    expect(hg_scene_check_limits(big, err) == HG_OK, "the largest counts");
}

struct Rng {
    std::mt19937 g;
    uint32_t below(uint32_t n) { return n ? uint32_t(g() % n) : 0u; }
    float unit() { return float(g() % 20001) / 10000.0f - 1.0f; }
};

void grow(std::vector<BVHEntry>& e, size_t at, uint32_t first, uint32_t count, uint32_t leaf_max, Rng& r) {
    const float lo = r.unit() - 1.0f, hi = r.unit() + 1.0f;
    if (count <= leaf_max) {
        e[at] = entry(first, count, lo, hi);
        return;
    }
    const size_t c = e.size();
    e.resize(c + 2);
    e[at] = entry(uint32_t(c), 0, lo, hi);
    const uint32_t k = count / 4 + r.below(count / 2) + (count < 4 ? 1 : 0);  // neither side empty, depth <= ~25
    grow(e, c, first, k, leaf_max, r);
    grow(e, c + 1, first + k, count - k, leaf_max, r);
}

HgSceneFile random_scene(Rng& r) {
    HgSceneFile s = base(0, 1 + r.below(4));
    const uint32_t n_meshes = 1 + r.below(5);
    s.spheres.resize(r.below(3));
    for (auto& sp : s.spheres) sp.materialIndex = r.below(uint32_t(s.materials.size()));
    for (uint32_t mi = 0; mi < n_meshes; ++mi) {
        if (mi && r.below(3) == 0) {  // an instance of an earlier mesh's tree
            HalogenMeshData m = s.meshes[r.below(mi)];
            m.worldToLocal.m[12] = r.unit();
            s.meshes.push_back(m);
            continue;
        }
        const uint32_t count = 1 + r.below(300), toff = uint32_t(s.tris.size()), off = uint32_t(s.blas.size());
        HgSceneFile t = base(count);
        s.tris.insert(s.tris.end(), t.tris.begin(), t.tris.end());
        std::vector<BVHEntry> e(1);
        grow(e, 0, 0, count, 1 + r.below(40), r);
        s.blas.insert(s.blas.end(), e.begin(), e.end());
        HalogenMeshData m = mesh(toff, off, r.below(uint32_t(s.materials.size())));
        for (int i = 0; i < 16; ++i) m.worldToLocal.m[i] += 0.3f * r.unit();
        if (r.below(5) == 0)
            for (int i = 0; i < 12; ++i) m.worldToLocal.m[i] = 0.0f;  // singular: not cullable
        s.meshes.push_back(m);
    }
    return s;
}

// The validation's depth-first search visits a graph in which both children of an entry lead back to it once per path,
// exponentially many times before the depth bound ends it.  A corruption that costs more visits than any scene here
// could honestly need is left out (counted); the search below is the validation's own, stopped where that rejects.
bool affordable(const HgSceneFile& s) {
    const uint64_t n = s.blas.size();
    size_t visits = 0;
    std::vector<std::pair<uint32_t, uint32_t>> dfs;
    for (const HalogenMeshData& m : s.meshes) {
        const uint32_t off = m.accelerationBufferOffset;
        if (off >= n) return true;
        dfs.assign(1, {off, 0u});
        while (!dfs.empty()) {
            auto [g, depth] = dfs.back();
            dfs.pop_back();
            if (depth + 2 > kMaxStack) return true;
            if (++visits > 2000000) return false;
            if (s.blas[g].triangleCount > 0) continue;
            const uint64_t a = uint64_t(off) + s.blas[g].indexA;
            if (a + 1 >= n) return true;
            dfs.push_back({uint32_t(a + 1), depth + 1});
            dfs.push_back({uint32_t(a), depth + 1});
        }
    }
    return true;
}

// An object moved: the decision is a partial re-upload, and its tables equal a full upload's of the same arrays
void partial_equals_full(const HgSceneFile& s) {
    HgSceneFile b = s;
    b.meshes.back().worldToLocal.m[12] += 0.05f;
    std::vector<uint8_t> copy[5];
    for (int k = 0; k < 5; ++k) copy_bytes(copy[k], s.in().src(k), s.in().bytes(k));
    expect(hg_upload_decide(true, copy, 0, s.meshes.size(), s.in(), 0).kind == HG_UPLOAD_SKIP, "same arrays: skip");
    expect(hg_upload_decide(true, copy, 0, s.meshes.size(), b.in(), 0).kind == HG_UPLOAD_PARTIAL, "moved: partial");
    HgScenePack first, full, part;
    HgPackError err;
    const bool ok = !hg_pack_spheres_materials(s.in(), first, err) && !hg_pack_geometry(s.in(), first, err) &&
                    !hg_pack_spheres_materials(b.in(), full, err) && !hg_pack_geometry(b.in(), full, err) &&
                    !hg_pack_spheres_materials(b.in(), part, err) && !hg_pack_mesh_table(b.in(), first.dm, part, err);
    expect(ok && part.dm.size() == full.dm.size() &&
               !std::memcmp(part.dm.data(), full.dm.data(), full.dm.size() * sizeof(HgDevMesh)),
           "partial mesh table differs from a full upload's", err.text);
}

}  // namespace

int main(int argc, char** argv) {
    const int scenes = argc > 1 ? std::atoi(argv[1]) : 300;
    Rng r{std::mt19937(argc > 2 ? uint32_t(std::atoi(argv[2])) : 1u)};
    hand_made();
    std::printf("hand-made trees and rejections done\n");
    HgPackStats all;
    size_t rejected = 0, accepted = 0, skipped = 0;
    for (int k = 0; k < scenes; ++k) {
        const HgSceneFile s = random_scene(r);
        HgPackStats st;
        int code = 0;
        const std::string t = pack(s, st, &code);
        expect(code == HG_OK, "random valid scene rejected:", t);
        partial_equals_full(s);
        all.inner += st.inner; all.inline_leaves += st.inline_leaves; all.table_leaves += st.table_leaves;
        all.pads += st.pads; all.cullable += st.cullable; all.not_cullable += st.not_cullable; all.paired += st.paired;
        for (int j = 0; j < 8; ++j) {
            HgSceneFile b = s;
            const uint32_t n = uint32_t(b.blas.size());
            const uint32_t v = r.below(2) ? uint32_t(r.g()) : r.below(2 * n + 2);
            switch (r.below(4)) {
                case 0: b.meshes[r.below(uint32_t(b.meshes.size()))].triangleBufferOffset = v; break;
                case 1: b.meshes[r.below(uint32_t(b.meshes.size()))].accelerationBufferOffset = v; break;
                case 2: b.blas[r.below(n)].indexA = v; break;
                default: b.blas[r.below(n)].triangleCount = r.below(2) ? v : r.below(48); break;
            }
            if (!affordable(b)) {
                ++skipped;
                continue;
            }
            HgPackStats bst;
            pack(b, bst, &code);  // accepted: the walk inside has checked every ref, table index and triangle range
            (code == HG_OK ? accepted : rejected)++;
        }
    }
    std::printf("%d random scenes: %zu records, %zu inline leaves, %zu table leaves, %zu pads, %zu paired siblings, "
                "%zu cullable and %zu other meshes\n", scenes, all.inner, all.inline_leaves, all.table_leaves, all.pads,
                all.paired, all.cullable, all.not_cullable);
    std::printf("corruptions: %zu rejected, %zu accepted and in bounds, %zu too costly to validate\n", rejected, accepted,
                skipped);
    expect(all.table_leaves && all.inline_leaves && all.pads && all.cullable && all.not_cullable && rejected && accepted,
           "the random scenes miss a case");
    std::printf(failures ? "%d FAILURES\n" : "scene pack ok\n", failures);
    return failures ? 1 : 0;
}
