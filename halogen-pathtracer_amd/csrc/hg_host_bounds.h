// hg_host_bounds.h — Unity's Bounds arithmetic and the min/max box of the host BLAS builders (internal, host-only:
// hg_host_blas.cpp, hg_host_sah.cpp).
//
// The reference's builder (Assets/Scripts/BVHGenerator.cs:154-186, RayTracingMesh.cs:106-117) keeps every box in a
// UnityEngine.Bounds, which stores centre/extents, so every min/max goes through  e=(max-min)*0.5, c=min+e, min=c-e,
// max=c+e.  The builders must produce the SAME node array as the C# code (triangle order and traversal counts depend
// on it), so the float arithmetic is kept in the reference's order.  Compiled with -ffp-contract=off.
#pragma once
#include <cstdint>
#include <limits>

#include "halogen_abi.h"

namespace hg_host {

constexpr float kAabbEpsilon = 0.00001f;  // RayTracingMesh.AABBEpsilon (RayTracingMesh.cs:11)
constexpr uint32_t kMaxNodeTriangleCount = 5;  // BVHGenerator.maxNodeTriangleCount (BVHGenerator.cs:8)

struct Vec3 {
    float v[3];
    float& operator[](int k) { return v[k]; }
    float operator[](int k) const { return v[k]; }
    static Vec3 load(const float* p) { return Vec3{{p[0], p[1], p[2]}}; }
};

// UnityEngine.Bounds: centre + extents storage.
struct UnityBounds {
    Vec3 center, extents;
    static UnityBounds FromMinMax(const Vec3& mn, const Vec3& mx) {  // Bounds.SetMinMax
        UnityBounds b;
        for (int k = 0; k < 3; ++k) {
            b.extents[k] = (mx[k] - mn[k]) * 0.5f;
            b.center[k] = mn[k] + b.extents[k];
        }
        return b;
    }
    Vec3 Min() const { Vec3 r; for (int k = 0; k < 3; ++k) r[k] = center[k] - extents[k]; return r; }
    Vec3 Max() const { Vec3 r; for (int k = 0; k < 3; ++k) r[k] = center[k] + extents[k]; return r; }
    Vec3 Size() const { Vec3 r; for (int k = 0; k < 3; ++k) r[k] = extents[k] * 2.0f; return r; }
    // `bounds.max += Vector3.one * AABBEpsilon` when any side is thinner than the epsilon
    void PadIfThin() {
        Vec3 s = Size();
        if (s[0] < kAabbEpsilon || s[1] < kAabbEpsilon || s[2] < kAabbEpsilon) {
            Vec3 mx = Max();
            for (int k = 0; k < 3; ++k) mx[k] = mx[k] + kAabbEpsilon * 1.0f;
            *this = FromMinMax(Min(), mx);
        }
    }
};

// initializeLeafEntry over a Bounds: the entry stores the corners the Bounds gives back
inline BVHEntry MakeEntry(const UnityBounds& b, uint32_t indexA, uint32_t count) {
    const Vec3 mn = b.Min(), mx = b.Max();
    BVHEntry e;
    e.indexA = indexA;
    e.triangleCount = count;
    e.boundingCornerA = {mn[0], mn[1], mn[2]};
    e.boundingCornerB = {mx[0], mx[1], mx[2]};
    return e;
}

// A min/max box, empty until something is added.  Vector3.Min/Max are Mathf.Min/Max (a<b?a:b / a>b?a:b) with the
// accumulator first: of equal extremes (+0 and -0) the LAST one added stays, and a NaN added replaces the accumulator.
// The reference's builder folds that way (add); the SAH builder has always compared the new value first, which keeps
// the FIRST of equal extremes (add_keep_first), and its trees are pinned bit for bit.
struct Box {
    Vec3 mn{{std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity(),
             std::numeric_limits<float>::infinity()}};
    Vec3 mx{{-std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
             -std::numeric_limits<float>::infinity()}};
    void add(const float* p) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = mn[k] < p[k] ? mn[k] : p[k];
            mx[k] = mx[k] > p[k] ? mx[k] : p[k];
        }
    }
    void add(const Box& b) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = mn[k] < b.mn[k] ? mn[k] : b.mn[k];
            mx[k] = mx[k] > b.mx[k] ? mx[k] : b.mx[k];
        }
    }
    void add_keep_first(const float* p) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = p[k] < mn[k] ? p[k] : mn[k];
            mx[k] = p[k] > mx[k] ? p[k] : mx[k];
        }
    }
    void add_keep_first(const Box& b) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = b.mn[k] < mn[k] ? b.mn[k] : mn[k];
            mx[k] = b.mx[k] > mx[k] ? b.mx[k] : mx[k];
        }
    }
};

// The fold of calculateBounds (BVHGenerator.cs:154-186) over the triangles [lo, hi) of an index list
inline Box fold_range(uint64_t lo, uint64_t hi, const int32_t* idx, const float* V) {
    Box b;
    for (uint64_t i = lo; i < hi; ++i)
        for (int c = 0; c < 3; ++c) b.add(V + 3 * int64_t(idx[3 * i + c]));
    return b;
}

// ... and its end: the Bounds of the folded box, padded when thin
inline UnityBounds PaddedBounds(const Box& b) {
    UnityBounds u = UnityBounds::FromMinMax(b.mn, b.mx);
    u.PadIfThin();
    return u;
}

}  // namespace hg_host
