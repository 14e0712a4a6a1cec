// hg_refit.h — the boxes of a refitted BLAS (hg_refit_blas, hg_refit_mesh, hg_refit_mesh_device; include/halogen_abi.h),
// one definition for the device kernels (hg_refit.hip) and the host twin (hg_host_mesh.cpp).  A refit keeps a tree's
// topology and recomputes every box from the (moved) triangles, so that the result is what BVHGenerator's arithmetic
// (hg_host_bounds.h: a folded range's UnityBounds, padded) gives for the same triangle sets.  Not in the reference.
//
// The contract, in the order the arithmetic is done (fp32, no contraction: both sides build with -ffp-contract=off):
//   raw box     of a triangle set: per component hg_fminf / hg_fmaxf over the nine coordinates pointA/B/C of each
//               HalogenTriangle (never v0 + e1), starting from (+inf, -inf).  hg_fminf / hg_fmaxf are associative and
//               commutative and pin the sign of zero (-0 < +0), so every reduction order gives the same bits; the raw
//               box of an inner entry is therefore the union of its two children's raw boxes.
//   stored box  the UnityEngine.Bounds round trip of the raw box: extents = (max - min) * 0.5f, center = min + extents,
//               Min = center - extents, Max = center + extents; then the thin-box pad: if any extents * 2.0f < 1e-5f,
//               Max = Max + 1e-5f * 1.0f per component and the box is rebuilt from (Min, Max) by the same round trip.
//   root        rounded without the pad (BVHGenerator's root is mesh.bounds).  One exception, on the host only (the
//               device layout holds no root box, and no traversal reads one): builders differ in whether they pad a
//               root (hg_build_blas_sah pads it like every entry), so a root that already is, bit for bit, the padded
//               stored box of its triangles is left as it is.  A refit of a tree that is current is therefore the
//               identity for either builder's output, and refitting twice gives what refitting once gives.
// Vertices are assumed finite and are not checked; host and device agree bit for bit on whatever they are given.
#pragma once
#include <stdint.h>

#include "halogen_abi.h"
#include "hg_fmath.h"

#define HG_REFIT_EPSILON 0.00001f  // RayTracingMesh.AABBEpsilon
#define HG_REFIT_MAX_DEPTH 62u     // deepest entry hg_upload_scene accepts (hg_scene_pack.h: kMaxStack - 2)

struct HgRawBox {
    float lo[3], hi[3];
};

HG_FN HgRawBox hg_refit_empty() {
    const float inf = hg_u2f(0x7F800000u);
    return HgRawBox{{inf, inf, inf}, {-inf, -inf, -inf}};
}

HG_FN void hg_refit_add_point(HgRawBox& b, float x, float y, float z) {
    b.lo[0] = hg_fminf(b.lo[0], x);
    b.lo[1] = hg_fminf(b.lo[1], y);
    b.lo[2] = hg_fminf(b.lo[2], z);
    b.hi[0] = hg_fmaxf(b.hi[0], x);
    b.hi[1] = hg_fmaxf(b.hi[1], y);
    b.hi[2] = hg_fmaxf(b.hi[2], z);
}

HG_FN void hg_refit_add_triangle(HgRawBox& b, const HalogenTriangle& t) {
    hg_refit_add_point(b, t.pointA.x, t.pointA.y, t.pointA.z);
    hg_refit_add_point(b, t.pointB.x, t.pointB.y, t.pointB.z);
    hg_refit_add_point(b, t.pointC.x, t.pointC.y, t.pointC.z);
}

HG_FN HgRawBox hg_refit_union(const HgRawBox& a, const HgRawBox& b) {
    HgRawBox u;
    for (int k = 0; k < 3; ++k) {
        u.lo[k] = hg_fminf(a.lo[k], b.lo[k]);
        u.hi[k] = hg_fmaxf(a.hi[k], b.hi[k]);
    }
    return u;
}

// Bounds.SetMinMax, then Bounds.min / Bounds.max
HG_FN void hg_refit_round_trip(const float mn[3], const float mx[3], float out_min[3], float out_max[3], float size[3]) {
    for (int k = 0; k < 3; ++k) {
        const float extents = (mx[k] - mn[k]) * 0.5f;
        const float center = mn[k] + extents;
        out_min[k] = center - extents;
        out_max[k] = center + extents;
        size[k] = extents * 2.0f;
    }
}

// The box an entry stores for a raw box; `pad`: every entry but a tree's root
HG_FN void hg_refit_stored(const HgRawBox& raw, bool pad, float out_min[3], float out_max[3]) {
    float size[3];
    hg_refit_round_trip(raw.lo, raw.hi, out_min, out_max, size);
    if (pad && (size[0] < HG_REFIT_EPSILON || size[1] < HG_REFIT_EPSILON || size[2] < HG_REFIT_EPSILON)) {
        float mn[3], mx[3];
        for (int k = 0; k < 3; ++k) {
            mn[k] = out_min[k];
            mx[k] = out_max[k] + HG_REFIT_EPSILON * 1.0f;
        }
        hg_refit_round_trip(mn, mx, out_min, out_max, size);
    }
}

// The root's exception: `root` already holds, bit for bit, the padded stored box of `raw`
HG_FN bool hg_refit_root_is_current_padded(const HgRawBox& raw, const BVHEntry& root) {
    float mn[3], mx[3];
    hg_refit_stored(raw, true, mn, mx);
    const float have[6] = {root.boundingCornerA.x, root.boundingCornerA.y, root.boundingCornerA.z,
                           root.boundingCornerB.x, root.boundingCornerB.y, root.boundingCornerB.z};
    for (int k = 0; k < 3; ++k)
        if (hg_f2u(have[k]) != hg_f2u(mn[k]) || hg_f2u(have[3 + k]) != hg_f2u(mx[k])) return false;
    return true;
}
