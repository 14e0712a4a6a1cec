// cull_table_check.h — test support for csrc/hg_cull.h, shared by tests/test_cull_table.py's driver and
// host/asan_cull_table.cpp: host twins of the kernel's two forms of the exact mesh skip (hg_dev_isect.h), synthetic mesh
// records whose root children tile, leave a gap or are offset, and the rays both programs throw at them.
//
//   hg_two_box_mask   the skip as it read the mesh records before the table: both padded child boxes of every cullable
//                     mesh below 64, the mesh's bit cleared when both are far.
//   hg_table_mask     the skip as mesh_live_mask walks the table: two entries per step, the tag in the entry.
// Both use ray_aabb with hg_fmath.h's min / max (NaN dropped, as the device's) and the same limit rule.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "hg_fmath.h"
#include "hg_scene_pack.h"

constexpr float kCullInf = std::numeric_limits<float>::infinity();

inline float hg_host_ray_aabb(const float A[3], const float B[3], const float o[3], const float inv[3]) {
    float t1[3], t2[3];
    for (int r = 0; r < 3; ++r) {
        t1[r] = (A[r] - o[r]) * inv[r];
        t2[r] = (B[r] - o[r]) * inv[r];
    }
    float tMin = hg_fminf(t1[0], t2[0]);
    float tMax = hg_fmaxf(t1[0], t2[0]);
    tMin = hg_fmaxf(tMin, hg_fminf(t1[1], t2[1]));
    tMax = hg_fminf(tMax, hg_fmaxf(t1[1], t2[1]));
    tMin = hg_fmaxf(tMin, hg_fminf(t1[2], t2[2]));
    tMax = hg_fminf(tMax, hg_fmaxf(t1[2], t2[2]));
    return tMax > hg_fmaxf(0.0f, tMin) ? tMin : kCullInf;
}

struct HgCullRay {
    float o[3], d[3], best_t;
};

inline void hg_cull_inv(const HgCullRay& r, float inv[3]) {
    for (int k = 0; k < 3; ++k) inv[k] = 1.0f / r.d[k];  // rcp_exact is the IEEE division
}

inline bool hg_cull_far(const float4& lo, const float4& hi, const HgCullRay& r, const float inv[3], float lim) {
    const float A[3] = {lo.x, lo.y, lo.z}, B[3] = {hi.x, hi.y, hi.z};
    const float d = hg_host_ray_aabb(A, B, r.o, inv);
    return d == kCullInf || d > lim;
}

inline uint64_t hg_two_box_mask(const HgDevMesh* dm, size_t n_meshes, const HgCullRay& r, uint32_t& culled) {
    uint64_t live = ~0ull;
    float inv[3];
    hg_cull_inv(r, inv);
    const float lim = r.best_t * 1.0001f + 1e-4f;
    const size_t n = n_meshes < 64 ? n_meshes : 64;
    for (size_t m = 0; m < n; ++m) {
        if (!dm[m].cullable) continue;
        if (hg_cull_far(dm[m].cull_a_lo, dm[m].cull_a_hi, r, inv, lim) &&
            hg_cull_far(dm[m].cull_b_lo, dm[m].cull_b_hi, r, inv, lim)) {
            live &= ~(1ull << m);
            culled++;
        }
    }
    return live;
}

// `entries`: the entries the launch walks (hg_cull_count).  Reads the table two entries at a time, as the kernel does:
// an out-of-range read here is an out-of-range fetch there.
inline uint64_t hg_table_mask(const HgCullTable& t, uint32_t entries, const HgCullRay& r, uint32_t& culled) {
    uint64_t live = ~0ull;
    float inv[3];
    hg_cull_inv(r, inv);
    const float lim = r.best_t * 1.0001f + 1e-4f;
    bool far = true;
    auto entry = [&](const float4& lo, const float4& hi) {
        far = far && hg_cull_far(lo, hi, r, inv, lim);
        uint32_t tag;
        std::memcpy(&tag, &lo.w, 4);
        if (!(tag & HG_CULL_MORE)) {
            if (far) {
                live &= ~(1ull << (tag & HG_CULL_MESH_MASK));
                culled++;
            }
            far = true;
        }
    };
    for (uint32_t i = 0; i < entries; i += 2u) {
        const float4 q[4] = {t.q.at(2 * size_t(i)), t.q.at(2 * size_t(i) + 1), t.q.at(2 * size_t(i) + 2),
                             t.q.at(2 * size_t(i) + 3)};
        entry(q[0], q[1]);
        if (i + 1u < entries) entry(q[2], q[3]);
    }
    return live;
}

// The table's own invariants: an even number of entries allocated, mesh order, at most two entries per mesh and
// HG_CULL_MORE exactly on the first of two, only cullable meshes below 64, a single entry containing both child boxes,
// two entries equal to the child boxes.  Returns "" or what is wrong.
inline std::string hg_check_cull_table(const HgDevMesh* dm, size_t n_meshes, const HgCullTable& t) {
    char buf[160];
    auto bad = [&](const char* what, size_t i) {
        std::snprintf(buf, sizeof buf, "%s at entry %zu", what, i);
        return std::string(buf);
    };
    if (t.q.size() != 2 * size_t((t.n + 1u) & ~1u)) return bad("allocation", t.q.size());
    std::vector<int> seen(n_meshes, 0);
    int64_t last = -1;
    for (size_t i = 0; i < t.n; ++i) {
        uint32_t tag;
        std::memcpy(&tag, &t.q[2 * i].w, 4);
        const size_t m = tag & ~HG_CULL_MORE;
        if (m >= n_meshes || m >= HG_CULL_MAX_MESHES || !dm[m].cullable) return bad("mesh without a cull box", i);
        const bool more = tag & HG_CULL_MORE;
        const float4 &lo = t.q[2 * i], &hi = t.q[2 * i + 1];
        if (more) {
            if (int64_t(m) <= last || i + 1 >= t.n) return bad("order", i);
            if (std::memcmp(&lo, &dm[m].cull_a_lo, 12) || std::memcmp(&hi, &dm[m].cull_a_hi, 12)) return bad("box A", i);
            uint32_t next;
            std::memcpy(&next, &t.q[2 * i + 2].w, 4);
            if (next != uint32_t(m)) return bad("second entry", i);
            ++i;
            if (std::memcmp(&t.q[2 * i], &dm[m].cull_b_lo, 12) || std::memcmp(&t.q[2 * i + 1], &dm[m].cull_b_hi, 12))
                return bad("box B", i);
        } else {
            if (int64_t(m) <= last) return bad("order", i);
            const float4* c[2][2] = {{&dm[m].cull_a_lo, &dm[m].cull_a_hi}, {&dm[m].cull_b_lo, &dm[m].cull_b_hi}};
            for (auto& b : c)
                if (!(lo.x <= b[0]->x && lo.y <= b[0]->y && lo.z <= b[0]->z && hi.x >= b[1]->x && hi.y >= b[1]->y &&
                      hi.z >= b[1]->z))
                    return bad("union does not contain a child box", i);
        }
        last = int64_t(m);
        seen[m] = 1;
    }
    for (size_t m = 0; m < n_meshes && m < HG_CULL_MAX_MESHES; ++m)
        if (dm[m].cullable && !seen[m]) return bad("cullable mesh without an entry, mesh", m);
    return "";
}

// ---- synthetic records and rays ------------------------------------------------------------------------------------------
struct HgCullRng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return uint32_t(s >> 33);
    }
    uint32_t below(uint32_t n) { return next() % n; }
    float uni(float a, float b) { return a + (b - a) * (float(next() & 0xFFFFFF) / 16777216.0f); }
};

enum HgCullShape { HG_SHAPE_TILE, HG_SHAPE_GAP, HG_SHAPE_OFFSET, HG_SHAPE_NESTED, HG_SHAPE_LEAF, HG_SHAPE_SINGULAR };

// A mesh record whose cull boxes come from mesh_cull_boxes (hg_scene_pack.h) over an identity-rotation matrix at `pos`
// with scale `scale`: a local box [-1, 1]^3 (flat on axis `flat` when >= 0) cut on axis `cut` at `at`; the second child
// starts `gap` beyond the cut and is moved by `offset` on the next axis.
inline HgDevMesh hg_cull_synth(HgCullShape shape, const float pos[3], float scale, int cut, float at, int flat, float gap,
                               float offset) {
    HgDevMesh dm{};
    hg_mat4 w2l{};
    for (int i = 0; i < 3; ++i) {
        w2l.m[5 * i] = 1.0f / scale;
        w2l.m[12 + i] = -pos[i] / scale;
    }
    w2l.m[15] = 1.0f;
    if (shape == HG_SHAPE_SINGULAR)
        for (int i = 0; i < 12; ++i) w2l.m[i] = 0.0f;
    std::memcpy(dm.w2l, w2l.m, sizeof dm.w2l);
    dm.root_ref = shape == HG_SHAPE_LEAF ? (HG_LEAF_BIT | (1u << HG_LEAF_CNT_SHIFT)) : 0u;
    if (shape == HG_SHAPE_LEAF) return dm;
    float lo[2][3], hi[2][3];
    for (int k = 0; k < 2; ++k)
        for (int r = 0; r < 3; ++r) {
            lo[k][r] = flat == r ? 0.0f : -1.0f;
            hi[k][r] = flat == r ? 0.0f : 1.0f;
        }
    hi[0][cut] = at;
    lo[1][cut] = at + gap;
    if (shape == HG_SHAPE_NESTED) {  // B inside A on every axis
        hi[0][cut] = 1.0f;
        for (int r = 0; r < 3; ++r) {
            lo[1][r] = flat == r ? 0.0f : -0.5f;
            hi[1][r] = flat == r ? 0.0f : 0.25f;
        }
    }
    const int side = (cut + 1) % 3;
    lo[1][side] += offset;
    hi[1][side] += offset;
    BVHEntry ab[2] = {};
    for (int k = 0; k < 2; ++k) {
        std::memcpy(&ab[k].boundingCornerA, lo[k], 12);
        std::memcpy(&ab[k].boundingCornerB, hi[k], 12);
    }
    if (mesh_cull_boxes(w2l, ab[0], ab[1], dm)) dm.cullable = 1;
    else dm.cull_a_lo = dm.cull_a_hi = dm.cull_b_lo = dm.cull_b_hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return dm;
}

// n records of mixed shapes scattered in [-8, 8]^3
inline std::vector<HgDevMesh> hg_cull_synth_table(HgCullRng& r, size_t n) {
    std::vector<HgDevMesh> dm;
    for (size_t m = 0; m < n; ++m) {
        const float pos[3] = {r.uni(-8, 8), r.uni(-8, 8), r.uni(-8, 8)};
        const uint32_t k = r.below(10);
        const HgCullShape shape = k < 4 ? HG_SHAPE_TILE : k < 6 ? HG_SHAPE_GAP : k < 7 ? HG_SHAPE_OFFSET
                                  : k < 8 ? HG_SHAPE_NESTED : k < 9 ? HG_SHAPE_LEAF : HG_SHAPE_SINGULAR;
        const int flat = r.below(3) == 0 ? int(r.below(3)) : -1;
        int cut = int(r.below(3));
        if (cut == flat) cut = (cut + 1) % 3;
        dm.push_back(hg_cull_synth(shape, pos, r.uni(0.2f, 3.0f), cut, r.uni(-0.6f, 0.6f), flat,
                                   shape == HG_SHAPE_GAP ? r.uni(0.05f, 0.5f) : 0.0f,
                                   shape == HG_SHAPE_OFFSET ? r.uni(0.05f, 0.5f) : 0.0f));
    }
    return dm;
}

// Ray i of a sweep over the records dm: kinds in turn — random; one or two zero direction components; origin inside a
// cull box; origin on a face of one (a coordinate equal to the box's); a NaN origin component, or all three — each with
// best_t drawn from small, mid and infinite.
inline HgCullRay hg_cull_ray(HgCullRng& r, const HgDevMesh* dm, size_t n_meshes, uint64_t i) {
    HgCullRay ray;
    const uint32_t kind = uint32_t(i % 6);
    for (int k = 0; k < 3; ++k) {
        ray.o[k] = r.uni(-12, 12);
        ray.d[k] = r.uni(-1, 1);
    }
    const HgDevMesh* pick = nullptr;
    for (int tries = 0; tries < 8 && n_meshes && !pick; ++tries) {
        const HgDevMesh& m = dm[r.below(uint32_t(n_meshes))];
        if (m.cullable) pick = &m;
    }
    if (pick && kind != 4) {  // aim at a cull box of the picked mesh: hits and near misses, not only far misses
        const bool b = r.below(2);
        const float4 &lo = b ? pick->cull_b_lo : pick->cull_a_lo, &hi = b ? pick->cull_b_hi : pick->cull_a_hi;
        const float L[3] = {lo.x, lo.y, lo.z}, H[3] = {hi.x, hi.y, hi.z};
        float target[3];
        for (int k = 0; k < 3; ++k) {
            const float ext = (H[k] - L[k]) * 0.6f + 0.05f;
            target[k] = r.uni(L[k] - ext, H[k] + ext);
        }
        if (kind == 2 || kind == 3) {
            for (int k = 0; k < 3; ++k) ray.o[k] = r.uni(L[k], H[k]);
            if (kind == 3) {
                const int k = int(r.below(3));
                ray.o[k] = r.below(2) ? L[k] : H[k];
            }
        } else {
            for (int k = 0; k < 3; ++k) ray.d[k] = target[k] - ray.o[k];
        }
    }
    float len = std::sqrt(ray.d[0] * ray.d[0] + ray.d[1] * ray.d[1] + ray.d[2] * ray.d[2]);
    if (!(len > 0.0f)) {
        ray.d[0] = 1.0f;
        len = 1.0f;
    }
    for (int k = 0; k < 3; ++k) ray.d[k] /= len;
    if (kind == 1 || (kind == 3 && r.below(2))) {  // one or two exact zeros (either sign): 1 / d is +-inf
        const int z = int(r.below(3));
        ray.d[z] = r.below(2) ? 0.0f : -0.0f;
        if (r.below(2)) ray.d[(z + 1) % 3] = r.below(2) ? 0.0f : -0.0f;
        if (kind == 1 && pick && r.below(2)) {  // ... starting exactly on a slab plane of that axis
            const float4& lo = pick->cull_a_lo;
            const float L[3] = {lo.x, lo.y, lo.z};
            ray.o[z] = L[z];
        }
    }
    if (kind == 5) {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        const uint32_t w = r.below(4);
        for (int k = 0; k < 3; ++k)
            if (w == 3 || uint32_t(k) == w) ray.o[k] = nan;
    }
    const uint32_t t = r.below(3);
    ray.best_t = t == 0 ? r.uni(0.001f, 1.0f) : t == 1 ? r.uni(1.0f, 30.0f) : kCullInf;
    return ray;
}

struct HgCullSweep {
    uint64_t cases = 0, violations = 0;       // ray x mesh below 64; bits the table clears and the two-box test keeps
    uint64_t single_cases = 0, single_two_box = 0, single_table = 0, single_lost = 0;  // on meshes with one entry
    uint64_t count_mismatch = 0;              // `culled` differs from the cleared bits
};

inline void hg_cull_sweep(const std::vector<HgDevMesh>& dm, const HgCullTable& t, HgCullRng& r, uint64_t rays,
                          HgCullSweep& s) {
    const uint32_t entries = hg_cull_count(t, int32_t(dm.size()));
    uint64_t single = 0;  // meshes with one entry
    for (uint32_t i = 0; i < t.n; ++i) {
        uint32_t tag, prev = HG_CULL_MORE;
        std::memcpy(&tag, &t.q[2 * size_t(i)].w, 4);
        if (i) std::memcpy(&prev, &t.q[2 * size_t(i) - 2].w, 4);
        if (!(tag & HG_CULL_MORE) && (i == 0 || !(prev & HG_CULL_MORE))) single |= 1ull << (tag & HG_CULL_MESH_MASK);
    }
    const uint64_t below = dm.size() < 64 ? dm.size() : 64;
    for (uint64_t i = 0; i < rays; ++i) {
        const HgCullRay ray = hg_cull_ray(r, dm.data(), dm.size(), i);
        uint32_t c2 = 0, ct = 0;
        const uint64_t two = hg_two_box_mask(dm.data(), dm.size(), ray, c2);
        const uint64_t tab = hg_table_mask(t, entries, ray, ct);
        s.cases += below;
        s.violations += uint64_t(__builtin_popcountll(~tab & two));
        s.count_mismatch += ct != uint32_t(__builtin_popcountll(~tab)) || c2 != uint32_t(__builtin_popcountll(~two));
        s.single_cases += uint64_t(__builtin_popcountll(single));
        s.single_two_box += uint64_t(__builtin_popcountll(~two & single));
        s.single_table += uint64_t(__builtin_popcountll(~tab & single));
        s.single_lost += uint64_t(__builtin_popcountll(~two & tab & single));
    }
}
