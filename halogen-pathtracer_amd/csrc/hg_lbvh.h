// hg_lbvh.h — the topology of a rebuilt BLAS (hg_build_blas_lbvh, hg_rebuild_mesh, hg_rebuild_mesh_device;
// include/halogen_abi.h), one definition for the device kernels (hg_lbvh.hip) and the host twin (hg_host_lbvh.cpp).  A
// rebuild gives one mesh a new tree over its moved triangles: a linear BVH, that is the triangles in Morton order, cut
// into leaves of L, under Karras' radix tree (Karras 2012, "Maximizing Parallelism in the Construction of BVHs,
// Octrees, and k-d Trees").  Every choice is made here, so that both sides build the same tree from the same floats.
// The boxes are hg_refit.h's contract on the new topology.  Not in the reference.  The second kind of rebuild
// (hg_build_blas_lbvh_sah, hg_rebuild_mesh_sah*), whose leaves are chosen by surface area, has its contract further down.
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
#include "hg_tunables.h"

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

// ---- leaves chosen by surface area (hg_build_blas_lbvh_sah, hg_rebuild_mesh_sah, hg_rebuild_mesh_sah_device) ----------
// The second kind of rebuilt tree: the radix tree above at L = 1 (K = n: key points, grid, code, order and topology
// unchanged; depth at most 30 + bits(n - 1) <= 57, and collapsing only shortens paths), with every subtree of at most
// HG_LBVH_MAX_LEAF triangles made one leaf where a leaf is no dearer than the subtree by the surface area heuristic.
//   raw box     of the triangles at sorted positions [first, last]: hg_refit.h's raw box (hg_fminf / hg_fmaxf over all
//               corner coordinates from (+inf, -inf)), no Bounds round trip and no pad.  Used for the cost only: the
//               boxes the tracer sees stay hg_refit.h's stored boxes.
//   area        A = (dx * dy + dy * dz) + dz * dx with d = hi - lo per axis, in this association.
//   cost        one triangle: A * 1; a leaf of N triangles: A * (float)N; an inner node: node_cost * A + (cost(child A) +
//               cost(child B)), the children at their best costs.
//   collapse    bottom-up, an internal node covering N <= 15 triangles becomes a leaf iff leaf_cost <= inner_cost, and
//               its best cost is then leaf_cost, else inner_cost.  A NaN on either side (0 * Inf of a flat axis beside an
//               overflowed one, Inf - Inf of overflowed costs, a triangle set with no non-NaN coordinate on an axis:
//               lo = +Inf, hi = -Inf, d = -Inf) makes the comparison false: the node stays inner.  Nodes covering more
//               than 15 triangles never collapse and their cost is never formed, so a decision reads only the maximal
//               subtree of at most 15 triangles it lies in: at most 14 internal nodes, whose indices lie in first ..
//               last of the subtree's range (a node's index is one end of its own range).
//   live        an internal node is live iff neither it nor an ancestor collapsed.  Live nodes keep their relative order:
//               the new index of a live node is the exclusive prefix sum of the live flags, so a subtree's records stay
//               contiguous.  No live node (n = 1, or the root collapsed, which needs n <= 15): the tree is one leaf.
//   refs        of live node i: a child that is one triangle or a collapsed node is an inline leaf ref HG_LEAF_BIT |
//               count << 27 | first triangle; a live child is rec_min + its new index.
//   capacity    node_cost > 0 is taken as given.  node_cost == 0: HG_LBVH_SAH_NODE_COST, doubled up to 6 times, the
//               first rung whose live count fits; only the collapse, the count and the scan depend on the rung.
// The cost of an inner node against 1 per leaf triangle: the best of 0.5, 1, 2 and 4 on the C3 dragon twisted by 1.2 rad
// per unit height (tools/bench_rebuild_sah.py, profiles/rebuild_sah.json), and the one with the
// fewest records
#define HG_LBVH_SAH_NODE_COST 4.0f
#define HG_LBVH_SAH_RUNGS 7u        // the start value and 6 doublings
#define HG_LBVH_SAH_SLOTS HG_LBVH_MAX_LEAF  // node index less the first of its subtree: 0 .. 14

HG_FN float hg_lbvh_sah_rung(uint32_t r) { return HG_LBVH_SAH_NODE_COST * (float)(1u << r); }

// A of the raw box of the sorted triangles [first, last]
HG_FN float hg_lbvh_sah_area(const HalogenTriangle* sorted_tris, int32_t first, int32_t last) {
    HgRawBox b = hg_refit_empty();
    for (int32_t t = first; t <= last; ++t) hg_refit_add_triangle(b, sorted_tris[t]);
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return (dx * dy + dy * dz) + dz * dx;
}

// The decisions of the maximal small subtree under internal node `root`, which covers [first, last], last - first < 15:
// live[i] for each of its last - first internal nodes.  cost: HG_LBVH_SAH_SLOTS floats of the caller's, element k
// (node first + k) at cost[k * stride] (a device lane's column of LDS; the host: stride 1).  The subtree's nodes are listed breadth-first
// (4 bits each: the node index less `first`), parents before children; walked backwards for the costs, forwards for
// the live flags.
HG_FN void hg_lbvh_sah_subtree(const HgLbvhNode* topo, const HalogenTriangle* sorted_tris, int32_t root, int32_t first,
                               int32_t last, float node_cost, float* cost, uint32_t stride, uint32_t* live) {
    uint64_t list = (uint64_t)(uint32_t)(root - first);
    const int count = last - first;  // internal nodes of the subtree
    for (int head = 0, tail = 1; head < count; ++head) {
        const HgLbvhNode nd = topo[first + (int32_t)((list >> (4 * head)) & 15u)];
        if (nd.first != nd.split) list |= (uint64_t)(uint32_t)(nd.split - first) << (4 * tail++);
        if (nd.last != nd.split + 1) list |= (uint64_t)(uint32_t)(nd.split + 1 - first) << (4 * tail++);
    }
    uint32_t collapsed = 0;  // bit k: node first + k is a leaf at its best
    for (int h = count - 1; h >= 0; --h) {
        const uint32_t k = (uint32_t)((list >> (4 * h)) & 15u);
        const HgLbvhNode nd = topo[first + (int32_t)k];
        const float A = hg_lbvh_sah_area(sorted_tris, nd.first, nd.last);
        const float ca = nd.first == nd.split ? hg_lbvh_sah_area(sorted_tris, nd.split, nd.split) * 1.0f
                                              : cost[(uint32_t)(nd.split - first) * stride];
        const float cb = nd.last == nd.split + 1 ? hg_lbvh_sah_area(sorted_tris, nd.last, nd.last) * 1.0f
                                                 : cost[(uint32_t)(nd.split + 1 - first) * stride];
        const float inner_cost = node_cost * A + (ca + cb);
        const float leaf_cost = A * (float)(nd.last - nd.first + 1);
        const bool leaf = leaf_cost <= inner_cost;  // (false with a NaN on either side)
        collapsed |= (leaf ? 1u : 0u) << k;
        cost[k * stride] = leaf ? leaf_cost : inner_cost;
    }
    uint32_t dead = 0;  // bit k: an ancestor of node first + k collapsed
    for (int h = 0; h < count; ++h) {
        const uint32_t k = (uint32_t)((list >> (4 * h)) & 15u);
        const HgLbvhNode nd = topo[first + (int32_t)k];
        const bool off = ((dead | collapsed) >> k) & 1u;
        live[first + (int32_t)k] = off ? 0u : 1u;
        if (off) {
            if (nd.first != nd.split) dead |= 1u << (uint32_t)(nd.split - first);
            if (nd.last != nd.split + 1) dead |= 1u << (uint32_t)(nd.split + 1 - first);
        }
    }
}

// Internal node i's part of the collapse over the n - 1 internal nodes (n >= 2): a node covering more than 15 triangles
// is live and decides the maximal small subtrees that are its children; node 0 decides the whole tree if n <= 15; every
// other node's flag is written by the node above its subtree.  Every live[] is written exactly once.
HG_FN void hg_lbvh_sah_node(const HgLbvhNode* topo, const HalogenTriangle* sorted_tris, int32_t i, float node_cost,
                            float* cost, uint32_t stride, uint32_t* live) {
    const HgLbvhNode nd = topo[i];
    if (nd.last - nd.first < (int32_t)HG_LBVH_MAX_LEAF) {
        if (i == 0) hg_lbvh_sah_subtree(topo, sorted_tris, 0, nd.first, nd.last, node_cost, cost, stride, live);
        return;
    }
    live[i] = 1u;
    if (nd.first != nd.split && nd.split - nd.first < (int32_t)HG_LBVH_MAX_LEAF)
        hg_lbvh_sah_subtree(topo, sorted_tris, nd.split, nd.first, nd.split, node_cost, cost, stride, live);
    if (nd.last != nd.split + 1 && nd.last - (nd.split + 1) < (int32_t)HG_LBVH_MAX_LEAF)
        hg_lbvh_sah_subtree(topo, sorted_tris, nd.split + 1, nd.split + 1, nd.last, node_cost, cost, stride, live);
}

// The two refs of live node i; new_index: the exclusive prefix sum of live[]
HG_FN void hg_lbvh_sah_refs(const HgLbvhNode* topo, const uint32_t* live, const uint32_t* new_index, int32_t i,
                            uint32_t rec_min, uint32_t tri_offset, uint32_t ref[2]) {
    const HgLbvhNode nd = topo[i];
    for (int k = 0; k < 2; ++k) {
        const int32_t cf = k == 0 ? nd.first : nd.split + 1, cl = k == 0 ? nd.split : nd.last;
        const int32_t c = k == 0 ? nd.split : nd.split + 1;  // the child's node index where it is internal
        if (cf != cl && live[c])
            ref[k] = rec_min + new_index[c];
        else  // one triangle, or a collapsed node (a child of a live node is not dead, so it covers at most 15)
            ref[k] = HG_LEAF_BIT | ((uint32_t)(cl - cf + 1) << HG_LEAF_CNT_SHIFT) | (tri_offset + (uint32_t)cf);
    }
}
