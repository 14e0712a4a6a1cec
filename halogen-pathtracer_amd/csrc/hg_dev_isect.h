// hg_dev_isect.h — intersection with one primitive (:244-376): boxes, spheres, the exact mesh cull, the triangle test,
// a mesh's local ray and resolved hit, and the distributed leaf test (part of hg_device.h).
#pragma once
#include <hip/hip_runtime.h>

#include "hg_dev_records.h"
#include "hg_dev_wave.h"

namespace hgd {

__device__ __forceinline__ float ray_aabb(f3 A, f3 B, f3 o, f3 inv) {  // :244-259
    f3 t1 = (A - o) * inv;
    f3 t2 = (B - o) * inv;
    float tMin = hg_fminf(t1.x, t2.x);
    float tMax = hg_fmaxf(t1.x, t2.x);
    tMin = hg_fmaxf(tMin, hg_fminf(t1.y, t2.y));
    tMax = hg_fminf(tMax, hg_fmaxf(t1.y, t2.y));
    tMin = hg_fmaxf(tMin, hg_fminf(t1.z, t2.z));
    tMax = hg_fminf(tMax, hg_fmaxf(t1.z, t2.z));
    return tMax > hg_fmaxf(0.0f, tMin) ? tMin : HG_INF;
}

// ray_aabb (:244-259) of both children: dA, dB
__device__ __forceinline__ void pair_dist(const NodePair& r, f3 o, f3 inv, float& dA, float& dB) {
    dA = ray_aabb(xyz(r.q0), xyz(r.q1), o, inv);
    dB = ray_aabb(xyz(r.q2), xyz(r.q3), o, inv);
}

// One sphere of isect_spheres: record (cr, am, b) of sphere i against the ray; updates the closest accepted sphere
__device__ __forceinline__ void isect_sphere(const HgKernelParams& kp, const Ray& ray, f3 inv, uint32_t i, float4 cr,
                                             float4 am, float4 b, float& closest, uint32_t& best) {
    if (!(ray_aabb(xyz(am), xyz(b), ray.o, inv) < kp.far_)) return;
    // sphere_intersection :266-303
    f3 center = xyz(cr);
    f3 sh = ray.o - center;
    float bq = 2.0f * dot(sh, ray.d);
    float cq = dot(sh, sh) - cr.w * cr.w;
    float disc = bq * bq - 4.0f * cq;
    if (!(disc >= 0.0f)) return;  // rayT = INF: never accepted
    float hd = (-bq - __builtin_sqrtf(disc)) / 2.0f;
    uint32_t back = 0;
    if (hd < 0.0f) {
        hd = (-bq + __builtin_sqrtf(disc)) / 2.0f;
        back = 0x80000000u;
    }
    if (hd < closest && hd > 0.0001f) {
        closest = hd;
        best = i | back;
    }
}

// Returns the closest accepted sphere as index | (orientation < 0) << 31 (HG_NONE if none), its distance in t;
// position/normal/material are resolved after the mesh pass (resolve_sphere), with the same arithmetic.
// inv: 1 / ray.d by rcp_exact, which the mesh cull of the same ray start uses too.  The records of two spheres are
// fetched before the first is tested (one wait on the scalar cache per pair); they are tested in buffer order.
__device__ uint32_t isect_spheres(const HgKernelParams& kp, const Ray& ray, float& t, f3 inv) {  // :357-376
    float closest = t;
    uint32_t best = HG_NONE;
    const uint32_t n = uint32_t(kp.n_spheres);
    for (uint32_t i = 0; i < n; i += 2u) {
        const uint32_t j = i + 1u < n ? i + 1u : i;  // (an odd count's last pair: the same record twice, tested once)
        const float4 cr0 = ldc(kp.spheres, 3 * i), am0 = ldc(kp.spheres, 3 * i + 1), b0 = ldc(kp.spheres, 3 * i + 2);
        const float4 cr1 = ldc(kp.spheres, 3 * j), am1 = ldc(kp.spheres, 3 * j + 1), b1 = ldc(kp.spheres, 3 * j + 2);
        isect_sphere(kp, ray, inv, i, cr0, am0, b0, closest, best);
        if (j != i) isect_sphere(kp, ray, inv, j, cr1, am1, b1, closest, best);
    }
    t = closest;
    return best;
}
__device__ __forceinline__ uint32_t isect_spheres(const HgKernelParams& kp, const Ray& ray, float& t) {
    return isect_spheres(kp, ray, t, mk(rcp_exact(ray.d.x), rcp_exact(ray.d.y), rcp_exact(ray.d.z)));
}
__device__ __forceinline__ void resolve_sphere(const HgKernelParams& kp, const Ray& ray, uint32_t ref, Hit& h) {
    const uint32_t i = ref & 0x7FFFFFFFu;
    const float orient = (ref & 0x80000000u) ? -1.0f : 1.0f;
    const float4 cr = kp.spheres[3 * i];
    h.orient = orient;
    h.pos = ray.o + ray.d * h.t;
    h.n = normalize(h.pos - xyz(cr)) * orient;
    h.mat = __float_as_uint(kp.spheres[3 * i + 1].w);
}

// Exact mesh skip over the cull table (hg_cull.h; the boxes are HgDevMesh::cull_*): bit m of the result is clear when
// the ray certainly misses both children of mesh m's root in the reference's local-space test, or meets them only
// beyond `best_t` — the reference would test those two boxes, push nothing and find nothing there.  A mesh has one
// entry (its children tile their union: the union box) or two (HG_CULL_MORE on the first), and its bit is cleared only
// when every one is far.  Meshes without an entry (not cullable, or >= 64) are never culled.  Two entries, tags
// included, come with one 64-B scalar fetch.
__device__ __forceinline__ void cull_entry(float4 lo, float4 hi, f3 wo, f3 winv, float lim, bool& far, uint64_t& live,
                                           uint32_t& culled) {
    const float d = ray_aabb(xyz(lo), xyz(hi), wo, winv);
    far = far && (d == HG_INF || d > lim);  // NaN never skips
    const uint32_t tag = __float_as_uint(lo.w);
    if (!(tag & HG_CULL_MORE)) {  // the mesh's last entry
        if (far) {
            live &= ~(1ull << (tag & HG_CULL_MESH_MASK));
            culled++;
        }
        far = true;
    }
}
__device__ __forceinline__ uint64_t mesh_live_mask(const HgKernelParams& kp, f3 wo, f3 winv, float best_t,
                                                   uint32_t& culled) {
    uint64_t live = ~0ull;
    const float lim = best_t * 1.0001f + 1e-4f;
    const uint32_t n = kp.n_cull;
    bool far = true;  // every entry of the current mesh so far is far
    for (uint32_t i = 0; i < n; i += 2u) {  // (the table is allocated to an even number of entries)
        const float4 lo0 = ldc(kp.cull, 2 * i), hi0 = ldc(kp.cull, 2 * i + 1), lo1 = ldc(kp.cull, 2 * i + 2),
                     hi1 = ldc(kp.cull, 2 * i + 3);
        cull_entry(lo0, hi0, wo, winv, lim, far, live, culled);
        if (i + 1u < n) cull_entry(lo1, hi1, wo, winv, lim, far, live, culled);
    }
    return live;
}

// Triangle test of triangle_intersection_doublesided (:307-355) with every term computed and one combined accept
// (same values as the early-out form).  Returns true when the hit is accepted as the new closest (:416).
// kFlat (the distributed leaf test, measured: stream C3 +0.7 %; the regenerating kernel's sequential loop loses
// 1.5-3 % with it, tools/sweeps/NOTES_r02.md) evaluates the accept without short-circuit branches.
template <bool kFlat = false>
__device__ __forceinline__ bool tri_accept(f3 lo, f3 ld, float4 a, float4 b, float cz, float best_t, float& t,
                                           float& U, float& V, bool& front) {
    const f3 e1 = mk(a.w, b.x, b.y);
    const f3 e2 = mk(b.z, b.w, cz);
    const f3 pvec = cross(ld, e2);
    const float det = dot(pvec, e1);
    const float inv_det = rcp_exact(det);
    const f3 tvec = lo - xyz(a);
    U = dot(tvec, pvec) * inv_det;
    const f3 qvec = cross(tvec, e1);
    V = dot(ld, qvec) * inv_det;
    t = dot(e2, qvec) * inv_det;
    front = det > 0.0f;
    if (kFlat)  // bitwise & of the conditions: one straight compare chain instead of a branch per short-circuit step
        return bool(int(!(fabsf(det) < 0.00000001f)) & int(!(U < 0.0f || U > 1.0f)) & int(!(V < 0.0f || U + V > 1.0f)) &
                    int(t > 0.0f) & int(t > 0.0001f) & int(t < best_t));
    return !(fabsf(det) < 0.00000001f) && !(U < 0.0f || U > 1.0f) && !(V < 0.0f || U + V > 1.0f) && t > 0.0f &&
           t > 0.0001f && t < best_t;
}

// first mesh index >= m whose cull bit is set (meshes >= 64 carry no bit and are always live); n if none
__device__ __forceinline__ uint32_t next_live_mesh(uint64_t live, uint32_t m, uint32_t n) {
    uint32_t r = 64u;
    if (m < 64u) {
        const uint64_t b = live & (~0ull << m);
        if (b) r = uint32_t(__builtin_ctzll(b));
    } else {
        r = m;
    }
    return r < n ? r : n;
}

// world -> local ray of mesh m, direction NOT normalized (:390-392), its reciprocal and the root ref
template <bool kLds = false>
__device__ __forceinline__ void mesh_local_ray(const HgKernelParams& kp, const Ray& ray, uint32_t m, f3& lo, f3& ld,
                                               f3& inv, uint32_t& root) {
    const float4 c0 = mesh_f4<kLds>(kp, m, 0), c1 = mesh_f4<kLds>(kp, m, 1), c2 = mesh_f4<kLds>(kp, m, 2),
                 c3 = mesh_f4<kLds>(kp, m, 3);  // worldToLocal columns
    root = __float_as_uint(mesh_f4<kLds>(kp, m, 4).x);
    lo = mk(((c0.x * ray.o.x + c1.x * ray.o.y) + c2.x * ray.o.z) + c3.x * 1.0f,
            ((c0.y * ray.o.x + c1.y * ray.o.y) + c2.y * ray.o.z) + c3.y * 1.0f,
            ((c0.z * ray.o.x + c1.z * ray.o.y) + c2.z * ray.o.z) + c3.z * 1.0f);
    ld = mk(((c0.x * ray.d.x + c1.x * ray.d.y) + c2.x * ray.d.z) + c3.x * 0.0f,
            ((c0.y * ray.d.x + c1.y * ray.d.y) + c2.y * ray.d.z) + c3.y * 0.0f,
            ((c0.z * ray.d.x + c1.z * ray.d.y) + c2.z * ray.d.z) + c3.z * 0.0f);
    inv = mk(rcp_exact(ld.x), rcp_exact(ld.y), rcp_exact(ld.z));
}

// Accepted mesh hit (:452-471): interpolated normal x orientation through the inverse-transpose, hit position.
template <bool kLds = false>
__device__ __forceinline__ void resolve_mesh(const HgKernelParams& kp, const Ray& ray, float best_t, float best_u,
                                             float best_v, uint32_t best_tri, uint32_t best_mesh, Hit& h) {
    const uint32_t tri = best_tri & 0x7FFFFFFFu;
    const float orient = (best_tri & 0x80000000u) ? -1.0f : 1.0f;
    h.t = best_t;
    h.mat = __float_as_uint(mesh_f4<kLds>(kp, best_mesh, 4).z);  // HgDevMesh::material
    h.orient = orient;
    const float4 n0 = kp.normals[3 * tri], d1 = kp.normals[3 * tri + 1], d2 = kp.normals[3 * tri + 2];
    f3 n = (xyz(n0) + xyz(d1) * best_u) + xyz(d2) * best_v;
    n = n * orient;
    // mul(float4(n,0), worldToLocal): row vector times matrix (inverse-transpose normal transform); w2l is column-major,
    // so m[4c + r] = column c, row r and the dot products run down the columns
    const float4 m0 = mesh_f4<kLds>(kp, best_mesh, 0), m1 = mesh_f4<kLds>(kp, best_mesh, 1),
                 m2 = mesh_f4<kLds>(kp, best_mesh, 2);
    f3 w = mk(((n.x * m0.x + n.y * m0.y) + n.z * m0.z) + 0.0f * m0.w,
              ((n.x * m1.x + n.y * m1.y) + n.z * m1.z) + 0.0f * m1.w,
              ((n.x * m2.x + n.y * m2.y) + n.z * m2.z) + 0.0f * m2.w);
    h.n = normalize(w);
    h.pos = ray.o + ray.d * best_t;
}

// Per-wave LDS scratch of the distributed leaf test (HG_LEAF_DIST): per lane, the best (t bits << 32 | triangle)
// key found for its ray, and one word of the owner table.  3 words per lane.
constexpr uint32_t kLeafShareWords = 3;
struct LeafShare {
    uint32_t w;  // word offset of this wave's 192-word region (even: the keys are u64)
    __device__ __forceinline__ unsigned long long* key(uint32_t i) const {
        return reinterpret_cast<unsigned long long*>(hg_lds_stack + w) + i;
    }
    __device__ __forceinline__ uint32_t& tab(uint32_t i) const { return hg_lds_stack[w + 128u + i]; }
};

// Distributed leaf test (HG_LEAF_DIST; HC:404-420): the triangles of every lane's current leaf form (ray, triangle)
// pairs numbered lane by lane (a wave prefix sum of the leaf sizes), and each round all 64 lanes test 64 of them.
// A pair's lane finds its owner through a per-wave table (the owner's lane id stored at the pair index where its
// run starts, then a running max over the lanes), fetches the owner's local ray and best_t by ds_bpermute, and
// folds an accepted hit into the owner's key (t bits << 32 | triangle) with an LDS 64-bit atomic min.  After each
// round an owner whose key came from that round pulls u, v and the facing from the winning pair's lane.
// Exact: in the reference's sequential loop every acceptance condition but `t < closest` is independent of the
// other triangles, and `closest` only falls, so the loop ends on the first triangle (in leaf order) of minimal t
// among those with t < best_t at the leaf's start.  t > 1e-4 is positive, so its bit pattern orders like its
// value, and the lower triangle index wins a tie: the key minimum is that triangle.  Counters are the same
// (one triangle test per pair).
// Precondition: every lane of the wave is active (the DPP scans and ds_bpermute read other lanes' registers; under a
// partial EXEC a disabled lane's register is stale and the prefix sums skip it).  The streaming kernel meets it by
// construction: trav_step runs at the top level of loops whose exits are wave-uniform (ballot counts).  Debug builds
// (HG_CHECK_EXEC=1) check it and take the sequential leaf loop when a lane is off (returns false); the check is
// compiled out of the product build because keeping the fallback loop live costs the kernel 16 B/lane of scratch.
struct LeafRay {  // the lane's side of a leaf test: its mesh-local ray and running best hit
    const f3& lo;
    const f3& ld;
    float& best_t;
    float& best_u;
    float& best_v;
    uint32_t& best_tri;
    uint32_t& best_mesh;
    uint32_t mi;
};
__device__ __forceinline__ bool leaf_dist(const HgKernelParams& kp, const LeafRay& t, Counters& c, const LeafShare& ls,
                                          uint32_t first, uint32_t n) {
#if HG_CHECK_EXEC
    if (__ballot(1) != ~0ull) {  // partial EXEC: the sequential loop instead (see above), counted in counter slot 17
        if (kp.counters) atomicAdd(kp.counters + 17, 1ull);
        return false;
    }
#endif
    const uint32_t lane = __lane_id();
    const uint32_t incl = wave_incl_add(n);
    const uint32_t total = uint32_t(__builtin_amdgcn_readlane(int(incl), 63));
    if (total == 0u) return true;
    const uint32_t start = incl - n;
    const uint32_t fo = first - start;  // owner's triangle index = fo + pair index (mod 2^32)
    if (n) *ls.key(lane) = ~0ull;
    for (uint32_t base = 0; base < total; base += 64u) {
        c.tri_rounds += wave_once();
        ls.tab(lane) = 0u;
        wave_lds_sync();
        if (n && start < base + 64u && incl > base) ls.tab(start > base ? start - base : 0u) = lane + 1u;
        wave_lds_sync();
        const uint32_t o = wave_incl_max(ls.tab(lane)) - 1u;  // owner lane of pair base + lane
        const int addr = int(o << 2);
        const f3 olo = mk(bperm_f(addr, t.lo.x), bperm_f(addr, t.lo.y), bperm_f(addr, t.lo.z));
        const f3 old = mk(bperm_f(addr, t.ld.x), bperm_f(addr, t.ld.y), bperm_f(addr, t.ld.z));
        const float obt = bperm_f(addr, t.best_t);
        const uint32_t ti = uint32_t(__builtin_amdgcn_ds_bpermute(addr, int(fo))) + base + lane;
        bool acc = false;
        float tt = 0.0f, U = 0.0f, V = 0.0f;
        bool front = false;
        if (base + lane < total) {
            float4 a, b;
            float cz;
            tri_load(kp, ti, a, b, cz);
            c.tri++;
            acc = tri_accept<true>(olo, old, a, b, cz, obt, tt, U, V, front);
        }
        wave_lds_sync();
        if (acc) atomicMin(ls.key(o), (static_cast<unsigned long long>(__float_as_uint(tt)) << 32) | ti);
        wave_lds_sync();
        // owners: did this round's pairs improve the key?  Then pull u, v, facing from the winning pair's lane.
        unsigned long long k = ~0ull;
        if (n) k = *ls.key(lane);
        const uint32_t wp = uint32_t(k) - fo - base;  // winning pair's lane, when it is in this round
        const bool mine = n && k != ~0ull && wp < 64u && uint32_t(k) - fo < total;
        const int src = int((wp & 63u) << 2);
        const float wu = bperm_f(src, U), wv = bperm_f(src, V);
        const uint32_t wf = uint32_t(__builtin_amdgcn_ds_bpermute(src, front ? 1 : 0));
        if (mine) {
            t.best_t = __uint_as_float(uint32_t(k >> 32));
            t.best_u = wu;
            t.best_v = wv;
            t.best_tri = uint32_t(k) | (wf ? 0u : 0x80000000u);
            t.best_mesh = t.mi;
        }
    }
    return true;
}

}  // namespace hgd
