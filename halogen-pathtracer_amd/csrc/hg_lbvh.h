// hg_lbvh.h — the topology of a rebuilt BLAS (hg_build_blas_lbvh, hg_rebuild_mesh, hg_rebuild_mesh_device;
// include/halogen_abi.h), one definition for the device kernels (hg_lbvh.hip) and the host twin (hg_host.cpp).  A
// rebuild gives one mesh a new tree over its moved triangles: a linear BVH, that is the triangles in Morton order, cut
// into leaves of L, under Karras' radix tree (Karras 2012, "Maximizing Parallelism in the Construction of BVHs,
// Octrees, and k-d Trees").  Every choice is made here, so that both sides build the same tree from the same floats.
// The boxes are hg_refit.h's contract on the new topology.  Not in the reference.
//
// The contract (fp32, no contraction: both sides build with -ffp-contract=off):
//   key point   of triangle t, per axis: lo = fmin(fmin(A, B), C), hi = fmax(fmax(A, B), C) with hg_fminf / hg_fmaxf,
//               p = lo + hi: twice the box centre, one IEEE addition, no division.
//   grid        per axis pmin / pmax over the mesh's key points with hg_fminf / hg_fmaxf (associative, commutative,
//               NaN dropped, -0 < +0: any reduction order gives the same bits), ext = pmax - pmin.  hg_lbvh_cell has the
//               rule and names the operation that settles each special input.
//   code        30 bits: the three 10-bit cells interleaved, x in the highest bit of each triple.
//   order       triangles ascending by (code, caller's index): a stable sort of the indices by code.
//   leaves      L in 1..15; K = ceil(n / L) leaves; leaf j is the sorted positions [jL, min(n, jL + L)); its key is the
//               code at sorted position jL.  Keys are non-decreasing.
//   topology    Karras' construction over the K keys: delta(i, j) = clz(key_i ^ key_j) for different keys,
//               32 + clz(i ^ j) for equal keys, -1 for j out of range.  Internal node i (0 .. K - 2) covers a range of
//               leaves with a split g: child A is the left part (leaf g if that is one leaf, else internal node g),
//               child B the right part (leaf g + 1, or internal node g + 1).  Node 0 is the root; K = 1: the root is
//               that leaf and there are no internal nodes.
//   depth       a leaf lies at most 30 + bits(K - 1) entries below the root (bits(x): the length of x in binary): on a
//               path down, delta grows by at least one per internal node, the 30 code bits first (delta 2 .. 31), then
//               the index bits of a run of equal keys (at most bits(K - 1) of them differ inside a run).  K <= 2^27 + 1
//               by far, so the depth is at most 58: inside the 62 levels hg_upload_scene accepts.
#pragma once
#include <stdint.h>

#include "halogen_abi.h"
#include "hg_fmath.h"
#include "hg_refit.h"

#define HG_LBVH_MAX_LEAF 15u       // HG_LEAF_INLINE_MAX: a rebuilt tree's leaves are inline refs only
#define HG_LBVH_AUTO_MIN_LEAF 4u   // leaf_size 0: the smallest L >= this whose K - 1 records fit
#define HG_LBVH_MAX_TRIS (1u << 27)  // inline leaf refs hold 27 bits of the first (global) triangle
#define HG_LBVH_MAX_DEPTH 58u      // 30 + bits(2^27)
static_assert(HG_LBVH_MAX_DEPTH <= HG_REFIT_MAX_DEPTH, "a rebuilt tree is one hg_upload_scene accepts");

HG_FN void hg_lbvh_key_point(const HalogenTriangle& t, float p[3]) {
    const float a[3] = {t.pointA.x, t.pointA.y, t.pointA.z};
    const float b[3] = {t.pointB.x, t.pointB.y, t.pointB.z};
    const float c[3] = {t.pointC.x, t.pointC.y, t.pointC.z};
    for (int k = 0; k < 3; ++k) {
        const float lo = hg_fminf(hg_fminf(a[k], b[k]), c[k]);
        const float hi = hg_fmaxf(hg_fmaxf(a[k], b[k]), c[k]);
        p[k] = lo + hi;
    }
}

// The cell (0 .. 1023) of key point coordinate p on an axis whose key points span [pmin, pmax].
//   ext not both finite and > 0 (a flat axis or a single point: ext = 0; sums that overflowed: ext = +Inf, or NaN from
//   Inf - Inf; no non-NaN point at all: pmin = +Inf, pmax = -Inf, ext = -Inf): the two comparisons below, cell 0.
//   Otherwise p >= pmin or p is NaN, so p - pmin is >= +0 (x - x is +0 in round-to-nearest) or NaN, and the scale is
//   positive: the product is >= +0, +Inf or NaN, never negative.
//   ext denormal: the IEEE division gives scale = +Inf; a positive difference times +Inf is +Inf, which hg_fminf clamps
//   to 1023; 0 * Inf is NaN, which hg_fminf drops: 1023 as well.  A NaN p likewise: 1023.
//   p == pmax: the product is 1024 or a rounding step beside it; hg_fminf clamps it to 1023.
//   The conversion truncates a value in [0, 1023]: exact on both sides.
HG_FN uint32_t hg_lbvh_cell(float p, float pmin, float pmax) {
    const float ext = pmax - pmin;
    if (!(ext > 0.0f) || ext == hg_u2f(0x7F800000u)) return 0u;
    const float scale = 1024.0f / ext;
    const float v = hg_fminf((p - pmin) * scale, 1023.0f);
    return (uint32_t)v;
}

// Bit i of a 10-bit value to bit 3i
HG_FN uint32_t hg_lbvh_spread(uint32_t v) {
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

HG_FN uint32_t hg_lbvh_code(const float p[3], const float pmin[3], const float pmax[3]) {
    return (hg_lbvh_spread(hg_lbvh_cell(p[0], pmin[0], pmax[0])) << 2) |
           (hg_lbvh_spread(hg_lbvh_cell(p[1], pmin[1], pmax[1])) << 1) |
           hg_lbvh_spread(hg_lbvh_cell(p[2], pmin[2], pmax[2]));
}

HG_FN uint32_t hg_lbvh_leaf_count(uint32_t n_tris, uint32_t L) { return (n_tris + L - 1u) / L; }

// leaf_size 0: the smallest L in [HG_LBVH_AUTO_MIN_LEAF, 15] whose K - 1 records fit `capacity`; 0: none does
HG_FN uint32_t hg_lbvh_auto_leaf(uint32_t n_tris, uint32_t capacity) {
    for (uint32_t L = HG_LBVH_AUTO_MIN_LEAF; L <= HG_LBVH_MAX_LEAF; ++L)
        if (hg_lbvh_leaf_count(n_tris, L) - 1u <= capacity) return L;
    return 0u;
}

// 30 + bits(K - 1): the depth bound of a tree of K leaves
HG_FN uint32_t hg_lbvh_depth_bound(uint32_t K) {
    uint32_t bits = 0;
    for (uint32_t x = K - 1u; x; x >>= 1) ++bits;
    return 30u + bits;
}

// delta(i, j) over the leaf keys; leaf j's key is codes[j * L] (codes: the sorted codes of the triangles)
HG_FN int hg_lbvh_delta(const uint32_t* codes, uint32_t L, int32_t K, int32_t i, int32_t j) {
    if (j < 0 || j >= K) return -1;
    const uint32_t a = codes[(size_t)i * L], b = codes[(size_t)j * L];
    if (a != b) return __builtin_clz(a ^ b);
    return 32 + __builtin_clz((uint32_t)(i ^ j));  // (i != j wherever this is called)
}

// Internal node i of the K >= 2 leaves: the leaves [first, last] it covers and its split (child A covers
// [first, split], child B [split + 1, last]).  Karras 2012, section 4, figure 4.
struct HgLbvhNode {
    int32_t first, last, split;
};

HG_FN HgLbvhNode hg_lbvh_node(const uint32_t* codes, uint32_t L, int32_t K, int32_t i) {
    const int d = hg_lbvh_delta(codes, L, K, i, i + 1) > hg_lbvh_delta(codes, L, K, i, i - 1) ? 1 : -1;
    const int dmin = hg_lbvh_delta(codes, L, K, i, i - d);
    int32_t lmax = 2;
    while (hg_lbvh_delta(codes, L, K, i, i + lmax * d) > dmin) lmax *= 2;  // (lmax <= 2K <= 2^29: no overflow)
    int32_t l = 0;
    for (int32_t t = lmax / 2; t >= 1; t /= 2)
        if (hg_lbvh_delta(codes, L, K, i, i + (l + t) * d) > dmin) l += t;
    const int32_t j = i + l * d;
    const int dnode = hg_lbvh_delta(codes, L, K, i, j);
    int32_t s = 0;
    for (int32_t t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (hg_lbvh_delta(codes, L, K, i, i + (s + t) * d) > dnode) s += t;
        if (t == 1) break;
    }
    HgLbvhNode n;
    n.first = d > 0 ? i : j;
    n.last = d > 0 ? j : i;
    n.split = i + s * d + (d < 0 ? -1 : 0);
    return n;
}

// The first triangle (mesh-relative) and the count of leaf j
HG_FN void hg_lbvh_leaf(uint32_t n_tris, uint32_t L, uint32_t j, uint32_t& first, uint32_t& count) {
    first = j * L;
    count = n_tris - first < L ? n_tris - first : L;
}
