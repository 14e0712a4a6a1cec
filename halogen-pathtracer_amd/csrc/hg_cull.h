// hg_cull.h — the cull table: the boxes of the exact mesh skip (hg_dev_isect.h mesh_live_mask) in an array of their
// own, derived from the mesh records (HgDevMesh::cull_*, hg_scene_pack.h).  A ray start walks this table and nothing
// else: 32 B per entry, two entries per 64-B scalar fetch, the mesh index in the same fetch as the box.
//
//   entry      (lo.xyz, tag), (hi.xyz, 0): a padded world box.  tag = mesh index | HG_CULL_MORE when the next entry
//              belongs to the same mesh.  A mesh's bit is cleared only when every one of its entries is far.
//   order      mesh order; only cullable meshes below HG_CULL_MAX_MESHES have entries.  A mesh without an entry (leaf
//              root, non-invertible matrix, index 64 and above) stays live.
//   one box    a mesh whose root's two child boxes tile their union (hg_cull_tiles) gets one entry, the union.  The
//              union contains both padded child boxes and the slab test is monotone in the box corners, so a ray
//              that misses the union, or meets it only beyond the limit, does the same for both children: the skip
//              stays conservative.  A mesh kept that the two-box test would skip costs one root visit, whose two
//              box tests are the two the skip would have counted.
//   padding    the array is padded with zeros to an even number of entries, so a fetch of two never leaves it.
//
// Plain functions of plain arrays: plain g++ compiles this header (tests/test_cull_table.py, host/asan_cull_table.cpp).
// The includer provides float4 (hg_scene_pack.h's shim, or HIP's).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hg_layout.h"

struct HgCullTable {
    std::vector<float4> q;  // 2 float4 per entry, an even number of entries (the last may be the zero pad)
    uint32_t n = 0;         // entries
};

// world_box's pad rule (hg_scene_pack.h) evaluated on a box
inline double hg_cull_pad(const float lo[3], const float hi[3]) {
    double size = 0.0, mag = 0.0;
    for (int r = 0; r < 3; ++r) {
        size = std::max(size, double(hi[r]) - double(lo[r]));
        mag = std::max({mag, std::fabs(double(lo[r])), std::fabs(double(hi[r]))});
    }
    return 1e-3 * size + 1e-4 * mag + 1e-5;
}

// Do the two padded boxes A and B tile their union U?  On two axes both span U's whole interval within the pad, and on
// the third their unpadded intervals overlap or touch.  The boxes at hand are the padded ones, so "touch" reads: the
// padded intervals overlap by at least 0.99 of the two pads, each estimated by the pad rule on the padded box (which
// gives at most 1.0021 of the true pad).  On success lo / hi hold U, the componentwise union of the padded boxes: it
// contains both, as a box padded by the union's own (larger) pad would.
inline bool hg_cull_tiles(const float alo[3], const float ahi[3], const float blo[3], const float bhi[3], float lo[3],
                          float hi[3]) {
    for (int r = 0; r < 3; ++r) {
        if (!(alo[r] <= ahi[r]) || !(blo[r] <= bhi[r])) return false;  // (NaN or inverted: keep both boxes)
        if (!std::isfinite(alo[r]) || !std::isfinite(ahi[r]) || !std::isfinite(blo[r]) || !std::isfinite(bhi[r]))
            return false;
        lo[r] = std::min(alo[r], blo[r]);
        hi[r] = std::max(ahi[r], bhi[r]);
    }
    const double tol = hg_cull_pad(lo, hi);
    const double touch = 0.99 * (hg_cull_pad(alo, ahi) + hg_cull_pad(blo, bhi));
    bool span[3], meet[3];
    for (int r = 0; r < 3; ++r) {
        span[r] = double(alo[r]) - lo[r] <= tol && double(blo[r]) - lo[r] <= tol && double(hi[r]) - ahi[r] <= tol &&
                  double(hi[r]) - bhi[r] <= tol;
        meet[r] = double(std::min(ahi[r], bhi[r])) - double(std::max(alo[r], blo[r])) >= touch;
    }
    for (int t = 0; t < 3; ++t)
        if (meet[t] && span[(t + 1) % 3] && span[(t + 2) % 3]) return true;
    return false;
}

// The cull table of the mesh records dm[0 .. n_meshes)
inline void hg_cull_table(const HgDevMesh* dm, size_t n_meshes, HgCullTable& out) {
    out.q.clear();
    out.n = 0;
    auto put = [&](const float lo[3], const float hi[3], uint32_t tag) {
        float w;
        std::memcpy(&w, &tag, 4);
        out.q.push_back(make_float4(lo[0], lo[1], lo[2], w));
        out.q.push_back(make_float4(hi[0], hi[1], hi[2], 0.0f));
        out.n++;
    };
    const size_t n = std::min<size_t>(n_meshes, HG_CULL_MAX_MESHES);
    for (size_t m = 0; m < n; ++m) {
        if (!dm[m].cullable) continue;
        const float alo[3] = {dm[m].cull_a_lo.x, dm[m].cull_a_lo.y, dm[m].cull_a_lo.z};
        const float ahi[3] = {dm[m].cull_a_hi.x, dm[m].cull_a_hi.y, dm[m].cull_a_hi.z};
        const float blo[3] = {dm[m].cull_b_lo.x, dm[m].cull_b_lo.y, dm[m].cull_b_lo.z};
        const float bhi[3] = {dm[m].cull_b_hi.x, dm[m].cull_b_hi.y, dm[m].cull_b_hi.z};
        float lo[3], hi[3];
        if (hg_cull_tiles(alo, ahi, blo, bhi, lo, hi)) {
            put(lo, hi, uint32_t(m));
        } else {
            put(alo, ahi, uint32_t(m) | HG_CULL_MORE);
            put(blo, bhi, uint32_t(m));
        }
    }
    if (out.n & 1u) {
        out.q.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        out.q.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    }
}

// The entries a launch over the first n_meshes meshes walks (bufferCounts.y may be less than the uploaded count): those
// of meshes below n_meshes, a prefix of the table
inline uint32_t hg_cull_count(const HgCullTable& t, int32_t n_meshes) {
    uint32_t k = 0;
    for (; k < t.n; ++k) {
        uint32_t tag;
        std::memcpy(&tag, &t.q[2 * size_t(k)].w, 4);
        if (int64_t(tag & HG_CULL_MESH_MASK) >= int64_t(n_meshes)) break;
    }
    return k;
}
