// scene_pack_check.h — test support for csrc/hg_scene_pack.h, shared by tests/test_scene_pack.py's driver and
// host/asan_scene_pack.cpp: a scene file reader, digests of the staging arrays, and a host walk of a packed scene
// beside the BVHEntry trees it came from.  The walk reads nothing out of bounds itself: every ref, table index and
// triangle range is checked before it is followed, so it can judge the pack of a corrupted input.
#pragma once
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hg_scene_pack.h"

// A scene as the tests write it: five int32 counts (spheres, meshes, materials, triangles, BLAS entries), then the raw
// arrays in that order
struct HgSceneFile {
    std::vector<HalogenSphere> spheres;
    std::vector<HalogenMeshData> meshes;
    std::vector<PackedHalogenMaterial> materials;
    std::vector<HalogenTriangle> tris;
    std::vector<BVHEntry> blas;
    HgSceneIn in() const {
        return HgSceneIn{spheres.data(), int32_t(spheres.size()), meshes.data(), int32_t(meshes.size()),
                         materials.data(), int32_t(materials.size()), tris.data(), int32_t(tris.size()),
                         blas.data(), int32_t(blas.size())};
    }
    bool read(const char* path) {
        FILE* f = std::fopen(path, "rb");
        if (!f) return false;
        int32_t n[5];
        bool ok = std::fread(n, 4, 5, f) == 5 && n[0] >= 0 && n[1] >= 0 && n[2] >= 0 && n[3] >= 0 && n[4] >= 0;
        if (ok) {
            spheres.resize(size_t(n[0]));
            meshes.resize(size_t(n[1]));
            materials.resize(size_t(n[2]));
            tris.resize(size_t(n[3]));
            blas.resize(size_t(n[4]));
            ok = get(f, spheres) && get(f, meshes) && get(f, materials) && get(f, tris) && get(f, blas);
        }
        std::fclose(f);
        return ok;
    }

   private:
    template <class T>
    static bool get(FILE* f, std::vector<T>& v) {
        return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    }
};

inline uint64_t hg_fnv1a64(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}

template <class T>
void hg_print_digest(const char* name, const std::vector<T>& v) {
    std::printf(" %s=%016" PRIx64 " %s_bytes=%zu", name, hg_fnv1a64(v.data(), v.size() * sizeof(T)), name,
                v.size() * sizeof(T));
}

struct HgPackStats {
    size_t inner = 0, inline_leaves = 0, table_leaves = 0, pads = 0, cullable = 0, not_cullable = 0, paired = 0;
    uint32_t max_depth = 0;
};

// Walks every mesh of the packed scene `p` from its root_ref beside the BVHEntry tree of `in`, in the packer's own
// order (mesh by mesh, child A's subtree first).  Returns "" when everything holds, else the first thing that does not:
//   - array sizes; the triangle repack (v0, e1, e2) and the normals (n0, n1 - n0, n2 - n0);
//   - every ref is in bounds and never HG_NONE; a leaf ref decodes to the entry's (toff + indexA, triangleCount), inline
//     for 1..15 triangles and through the table from 16 on; an inner ref names a record with both children's boxes;
//   - every reachable inner entry has exactly one record and no record serves two entries; two inner siblings that were
//     both new sit at records 2k and 2k + 1;
//   - the mesh records' root_ref, tri_offset, material and matrix; stack_depth even and >= the deepest entry + 2;
//   - the leaf table and the records hold nothing beyond what the walk reached, the sibling pads and the one dummy
//     entry of an empty table.
inline std::string hg_check_pack(const HgSceneIn& in, const HgScenePack& p, HgPackStats& st) {
    char msg[256];
    auto bad = [&](const char* fmt, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
        std::snprintf(msg, sizeof msg, fmt, a, b, c);
        return std::string(msg);
    };
    const size_t nt = size_t(in.n_tris), nn = size_t(in.n_nodes), n_rec = p.rec.size() / 4;
    if (p.sph.size() != size_t(in.n_spheres) * 3 || p.mat.size() != size_t(in.n_materials) * 5 ||
        p.dm.size() != size_t(in.n_meshes) || p.t9.size() != nt * 9 || p.nrm.size() != nt * 3 || p.rec.size() % 4 ||
        n_rec == 0 || p.leaf.empty())
        return bad("staging array sizes");
    for (size_t t = 0; t < nt; ++t) {
        const HalogenTriangle& h = in.tris[t];
        const float v[9] = {h.pointA.x, h.pointA.y, h.pointA.z, h.pointB.x - h.pointA.x, h.pointB.y - h.pointA.y,
                            h.pointB.z - h.pointA.z, h.pointC.x - h.pointA.x, h.pointC.y - h.pointA.y,
                            h.pointC.z - h.pointA.z};
        const float4 n[3] = {f4(h.normalA.x, h.normalA.y, h.normalA.z, 0.0f),
                             f4(h.normalB.x - h.normalA.x, h.normalB.y - h.normalA.y, h.normalB.z - h.normalA.z, 0.0f),
                             f4(h.normalC.x - h.normalA.x, h.normalC.y - h.normalA.y, h.normalC.z - h.normalA.z, 0.0f)};
        if (std::memcmp(&p.t9[9 * t], v, sizeof v) || std::memcmp(&p.nrm[3 * t], n, sizeof n))
            return bad("triangle %llu repacked wrong", t);
    }
    std::vector<uint32_t> ref_of(nn, HG_NONE);        // the ref the walk found for each entry
    std::vector<int64_t> entry_of(n_rec, -1);         // the entry each record serves
    std::vector<uint8_t> table_used(p.leaf.size(), 0);
    struct Item { uint32_t g, depth; };
    std::vector<Item> stack;
    // a ref found for entry g (the parent is being expanded, or g is a root): checked, and noted on first sight
    auto meet = [&](uint32_t g, uint32_t r, uint32_t toff, uint32_t depth, bool& fresh) -> std::string {
        fresh = false;
        if (r == HG_NONE) return bad("entry %llu: ref is HG_NONE", g);
        if (ref_of[g] != HG_NONE) return ref_of[g] == r ? "" : bad("entry %llu has two refs", g);
        const BVHEntry& e = in.blas[g];
        if (r & HG_LEAF_BIT) {
            if (e.triangleCount == 0) return bad("inner entry %llu has a leaf ref", g);
            const uint32_t cnt = (r >> HG_LEAF_CNT_SHIFT) & 15u;
            uint64_t first, count;
            if (cnt) {
                first = r & HG_LEAF_PAYLOAD;
                count = cnt;
                st.inline_leaves++;
            } else {
                const uint32_t idx = r & HG_LEAF_PAYLOAD;
                if (idx >= p.leaf.size()) return bad("entry %llu: leaf table index %llu out of range", g, idx);
                if (table_used[idx]++) return bad("leaf table entry %llu used twice", idx);
                first = p.leaf[idx].x;
                count = p.leaf[idx].y;
                st.table_leaves++;
            }
            if (first != uint64_t(toff) + e.indexA || count != e.triangleCount)
                return bad("leaf %llu decodes to (%llu, %llu)", g, first, count);
            if (first + count > nt) return bad("leaf %llu: triangles out of range", g);
            if ((cnt != 0) != (count <= HG_LEAF_INLINE_MAX && first < HG_LEAF_PAYLOAD))
                return bad("leaf %llu of %llu triangles in the wrong form", g, count);
        } else {
            if (e.triangleCount != 0) return bad("leaf entry %llu has a record ref", g);
            if (r >= n_rec) return bad("entry %llu: record %llu out of range", g, r);
            if (entry_of[r] != -1) return bad("record %llu serves two entries", r);
            entry_of[r] = g;
            st.inner++;
            fresh = true;
        }
        ref_of[g] = r;
        st.max_depth = std::max(st.max_depth, depth);
        return "";
    };
    for (int mi = 0; mi < in.n_meshes; ++mi) {
        const HalogenMeshData& m = in.meshes[mi];
        const HgDevMesh& dm = p.dm[size_t(mi)];
        const uint32_t off = m.accelerationBufferOffset, toff = m.triangleBufferOffset;
        if (off >= nn) return bad("mesh %llu: root out of range", mi);
        if (dm.tri_offset != toff || dm.material != m.materialIndex || m.materialIndex >= uint32_t(in.n_materials) ||
            std::memcmp(dm.w2l, m.worldToLocal.m, sizeof dm.w2l))
            return bad("mesh record %llu", mi);
        if (dm.cullable > 1 || (dm.cullable && in.blas[off].triangleCount != 0)) return bad("mesh %llu: cullable", mi);
        const float4 zero[4] = {f4(0, 0, 0, 0), f4(0, 0, 0, 0), f4(0, 0, 0, 0), f4(0, 0, 0, 0)};
        if (!dm.cullable && std::memcmp(&dm.cull_a_lo, zero, sizeof zero)) return bad("mesh %llu: stale cull boxes", mi);
        (dm.cullable ? st.cullable : st.not_cullable)++;
        bool fresh;
        std::string s = meet(off, dm.root_ref, toff, 0, fresh);
        if (!s.empty()) return s;
        stack.clear();
        if (fresh) stack.push_back({off, 0});
        while (!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            if (it.depth > 4096) return bad("walk deeper than 4096 below mesh %llu", mi);
            const uint64_t a64 = uint64_t(off) + in.blas[it.g].indexA;
            if (a64 + 1 >= nn) return bad("entry %llu: children out of range", it.g);
            const uint32_t a = uint32_t(a64);
            const BVHEntry& A = in.blas[a];
            const BVHEntry& B = in.blas[a + 1];
            const float4* r = &p.rec[4 * size_t(ref_of[it.g])];
            const float box[12] = {r[0].x, r[0].y, r[0].z, r[1].x, r[1].y, r[1].z,
                                   r[2].x, r[2].y, r[2].z, r[3].x, r[3].y, r[3].z};
            if (std::memcmp(box, &A.boundingCornerA, 24) || std::memcmp(box + 6, &B.boundingCornerA, 24))
                return bad("record of entry %llu: child boxes", it.g);
            uint32_t ra, rb;
            std::memcpy(&ra, &r[0].w, 4);
            std::memcpy(&rb, &r[1].w, 4);
            const bool both_new = ref_of[a] == HG_NONE && ref_of[a + 1] == HG_NONE && A.triangleCount == 0 &&
                                  B.triangleCount == 0;
            bool fresh_a, fresh_b;
            if (!(s = meet(a, ra, toff, it.depth + 1, fresh_a)).empty()) return s;
            if (!(s = meet(a + 1, rb, toff, it.depth + 1, fresh_b)).empty()) return s;
            if (both_new) {
                if (ra % 2 != 0 || rb != ra + 1) return bad("siblings %llu: records %llu and %llu", a, ra, rb);
                st.paired++;
            }
            if (fresh_b) stack.push_back({a + 1, it.depth + 1});
            if (fresh_a) stack.push_back({a, it.depth + 1});
        }
    }
    if (p.stack_depth % 2 != 0 || p.stack_depth < st.max_depth + 2) return bad("stack_depth %llu", p.stack_depth);
    if (st.inner > n_rec) return bad("more entries than records");
    st.pads = n_rec - st.inner - (st.inner == 0 ? 1 : 0);
    for (size_t r = 0; r < n_rec; ++r)
        if (entry_of[r] == -1) {
            const float4 z[4] = {f4(0, 0, 0, 0), f4(0, 0, 0, 0), f4(0, 0, 0, 0), f4(0, 0, 0, 0)};
            if (std::memcmp(&p.rec[4 * r], z, sizeof z)) return bad("record %llu is neither used nor a zero pad", r);
        }
    if (st.table_leaves != (st.table_leaves ? p.leaf.size() : p.leaf.size() - 1))
        return bad("leaf table holds %llu entries for %llu table leaves", p.leaf.size(), st.table_leaves);
    return "";
}
