// hg_dev_trav.h — the walk over the meshes' trees (:378-485): the one mesh traversal, get_ray_intersection over it,
// its form for ray queries and its resumable form for the streaming kernel (part of hg_device.h).
#pragma once
#include <hip/hip_runtime.h>

#include "hg_dev_isect.h"

namespace hgd {

// get_ray_scene_intersection_mesh, :378-472.
// Per-lane mesh cursor: each lane walks its own live meshes in buffer order (the reference's order, so ties resolve
// identically) and moves to its next mesh as soon as it finishes one, so a wave waits for the lane with the most total
// work instead of the slowest lane of every mesh in turn.  Inside a mesh the traversal keeps the current node in a
// register (the reference's push-near-then-pop-near is a no-op on order) and runs a relaxed while-while: the lanes
// descend inner nodes together while more than kp.descent_t of them are still descending (0: until every lane is at a
// leaf), and in any case until at least one lane can make other progress; then each tests its leaf.  Each lane's own
// sequence of node / leaf steps is the reference's.
// One body for the path tracer's kernels (intersect below calls it as it stands: behind a wrapper of its own the
// counting kernels compile to the same instructions in another order) and for the ray queries (isect_meshes_best):
// kCount keeps the work counters in c; without it c is not touched and the accepted hit's u, v, triangle and mesh go to
// *mb beside Hit.  kAny (occlusion): the lane leaves the mesh cursor at the first triangle that would make the closest
// query report a mesh hit, i.e. one accepted below seed - 1e-4 (:452); accepted triangles inside that 1e-4 band only
// lower best_t, as in the closest query, so up to the exit both traversals are the same and `found` equals "the
// closest query reports a mesh hit".
struct MeshBest {
    float u, v;
    uint32_t tri;   // global triangle index | (orientation < 0) << 31, HG_NONE: no mesh hit
    uint32_t mesh;
};

template <bool kMeshLds = false, bool kCount = true, bool kAny = false, class Stk>
__device__ bool isect_meshes(const HgKernelParams& kp, const Ray& ray, Hit& h, Counters& c, const Stk& stk,
                             MeshBest* mb = nullptr) {
    const float eps = 0.0001f;
    float best_t = h.t;  // closestIntersection.rayT starts at the seed: the sphere hit (:381), else the ray's t_max
    float best_u = 0.0f, best_v = 0.0f;
    uint32_t best_tri = HG_NONE;  // global triangle index | (orientation < 0) << 31
    uint32_t best_mesh = 0;
    uint32_t culled = 0;
    bool found = false;  // (kAny)
    const f3 winv = mk(rcp_exact(ray.d.x), rcp_exact(ray.d.y), rcp_exact(ray.d.z));
    const uint64_t live = mesh_live_mask(kp, ray.o, winv, best_t, culled);
    if constexpr (kCount) c.aabb += 2 * culled;
    const uint32_t nm = uint32_t(kp.n_meshes);
    uint32_t mi = next_live_mesh(live, 0u, nm);
    bool active = mi < nm;
    f3 lo = mk(0, 0, 0), ld = mk(0, 0, 0), inv = mk(0, 0, 0);
    uint32_t node = HG_NONE, sp = 0;
    if (active) mesh_local_ray<kMeshLds>(kp, ray, mi, lo, ld, inv, node);
    while (__any(active)) {
        const uint64_t act_mask = wave_ballot(active);
        const uint32_t dt = kp.descent_t;
        for (uint64_t dm = act_mask & wave_ballot(int32_t(node) >= 0);
             dm != 0ull && (uint32_t(__builtin_popcountll(dm)) > dt || dm == act_mask);
             dm = act_mask & wave_ballot(int32_t(node) >= 0)) {
            if constexpr (kCount) c.node_rounds += wave_once();
            if (active && int32_t(node) >= 0) {
                const NodePair np = node_pair(kp, node);
                float dA, dB;
                pair_dist(np, lo, inv, dA, dB);
                if constexpr (kCount) c.aabb += 2;
                const uint32_t refA = pair_ref_a(np), refB = pair_ref_b(np);
                // reference (:430-444): push far, push near (each only if tEntry < closest), pop near
                const bool bFirst = dB < dA;
                const uint32_t nearRef = bFirst ? refB : refA, farRef = bFirst ? refA : refB;
                const bool nearOk = (bFirst ? dB : dA) < best_t, farOk = (bFirst ? dA : dB) < best_t;
                if (nearOk) {
                    if (farOk) stk.push(sp, farRef);
                    node = nearRef;
                } else if (farOk) {
                    node = farRef;
                } else {
                    node = sp > 0 ? stk.pop(sp) : HG_NONE;
                }
            }
        }
        if (active && node != HG_NONE && (node & HG_LEAF_BIT)) {  // a leaf: its triangles in order (:404-420)
            const uint2 leaf = leaf_range(kp, node);
            const uint32_t end = leaf.x + leaf.y;
            for (uint32_t ti = leaf.x; ti < end; ++ti) {
                if constexpr (kCount) c.tri_rounds += wave_once();
                float4 a, b;
                float cz;
                tri_load(kp, ti, a, b, cz);
                if constexpr (kCount) c.tri++;
                float t, U, V;
                bool front;
                if (tri_accept(lo, ld, a, b, cz, best_t, t, U, V, front)) {
                    best_t = t;
                    best_u = U;
                    best_v = V;
                    best_tri = ti | (front ? 0u : 0x80000000u);
                    best_mesh = mi;
                    if constexpr (kAny) {
                        if (t < (h.t - eps)) {
                            found = true;
                            break;
                        }
                    }
                }
            }
            node = sp > 0 ? stk.pop(sp) : HG_NONE;
        }
        if constexpr (kAny) {
            if (found) active = false;  // the wave loop's __any(active) ends once every lane has its answer
        }
        if (active && node == HG_NONE) {  // this mesh is done: the lane's next live mesh
            mi = next_live_mesh(live, mi + 1u, nm);
            if (mi < nm) mesh_local_ray<kMeshLds>(kp, ray, mi, lo, ld, inv, node);
            else active = false;
        }
    }
    if constexpr (!kCount) *mb = MeshBest{best_u, best_v, best_tri, best_mesh};
    if constexpr (kAny) return found;
    // :452-471
    if (best_t < (h.t - eps) && best_t < kp.far_) {
        resolve_mesh<kMeshLds>(kp, ray, best_t, best_u, best_v, best_tri, best_mesh, h);
        return true;
    }
    return false;
}
// a ray query's traversal (hg_query.hip): get_ray_intersection for a caller's ray, handing out which primitive was hit
template <bool kAny, class Stk>
__device__ bool isect_meshes_best(const HgKernelParams& kp, const Ray& ray, Hit& h, MeshBest& mb, const Stk& stk) {
    Counters none;  // (not touched without kCount)
    return isect_meshes<false, false, kAny>(kp, ray, h, none, stk, &mb);
}

template <bool kMeshLds = false, class Stk>
__device__ __forceinline__ Hit intersect(const HgKernelParams& kp, const Ray& ray, Counters& c, const Stk& stk) {  // get_ray_intersection :474-485
    Hit h = hit_none(HG_INF);
    c.rays++;
    const uint32_t sph = isect_spheres(kp, ray, h.t);  // (its 1 / d and isect_meshes' are one computation once inlined)
    if (!isect_meshes<kMeshLds>(kp, ray, h, c, stk) && sph != HG_NONE) resolve_sphere(kp, ray, sph, h);
    return h;
}

// ---------------------------------------------------------------------------------------------------
// Resumable get_ray_intersection (:474-485) for the streaming kernel: the same spheres / exact mesh cull /
// per-lane mesh cursor / while-while traversal as intersect(), with its state in a struct so a lane can stop
// between steps (other lanes shade) and resume.  Same visit order, same counters, same result.
// ---------------------------------------------------------------------------------------------------
struct Trav {
    f3 lo, ld;             // ray in the current mesh's local space (1/ld is recomputed per round, trav_step)
    float best_t, best_u, best_v, sph_t;
    uint32_t best_tri;     // triangle | orientation<0 << 31, HG_NONE: no mesh hit yet
    uint32_t best_mesh, sph, node, sp, mi;  // mi == n_meshes: traversal finished
    uint64_t live;         // exact-cull mask of the meshes
};

template <bool kMeshLds = false>
__device__ __forceinline__ void trav_begin(const HgKernelParams& kp, const Ray& ray, Trav& t, Counters& c) {
    c.rays++;
    t.sph_t = HG_INF;
    const f3 winv = mk(rcp_exact(ray.d.x), rcp_exact(ray.d.y), rcp_exact(ray.d.z));  // once for spheres and cull
    t.sph = isect_spheres(kp, ray, t.sph_t, winv);
    t.best_t = t.sph_t;  // closestIntersection.rayT starts at the sphere hit (:381)
    t.best_u = 0.0f;
    t.best_v = 0.0f;
    t.best_tri = HG_NONE;
    t.best_mesh = 0;
    uint32_t culled = 0;
    t.live = mesh_live_mask(kp, ray.o, winv, t.best_t, culled);
    c.aabb += 2 * culled;
    t.sp = 0;
    t.node = HG_NONE;
    const uint32_t nm = uint32_t(kp.n_meshes);
    t.mi = next_live_mesh(t.live, 0u, nm);
    f3 inv;
    if (t.mi < nm) mesh_local_ray<kMeshLds>(kp, ray, t.mi, t.lo, t.ld, inv, t.node);
}

// One while-while round for the lanes with `act`: descend until each is at a leaf (or out of nodes), test that
// leaf, and move to the next live mesh when the current one is exhausted.
template <bool kMeshLds = false, class Stk>
__device__ __forceinline__ void trav_step(const HgKernelParams& kp, const Ray& ray, Trav& t, Counters& c,
                                          const Stk& stk, bool act, const LeafShare& ls) {
    // 1/ld (the same rcp_exact values mesh_local_ray computes) is not kept in Trav: live only during this round, it
    // stays out of the registers held across the streaming kernel's shading code
    const f3 inv = mk(rcp_exact(t.ld.x), rcp_exact(t.ld.y), rcp_exact(t.ld.z));
    const uint64_t act_mask = wave_ballot(act);  // act is fixed for the round
    const uint32_t dt = kp.descent_t;
    // lanes at an inner node (HG_NONE has the leaf bit): the wave descends while more than dt of them are left, or
    // while every active lane is still descending (relaxed while-while, as in isect_meshes)
    uint64_t dm = act_mask & wave_ballot(int32_t(t.node) >= 0);
    while (dm != 0ull && (uint32_t(__builtin_popcountll(dm)) > dt || dm == act_mask)) {
        c.node_rounds += wave_once();
        if (act && int32_t(t.node) >= 0) {
            const NodePair np = node_pair(kp, t.node);
            const uint32_t refA = pair_ref_a(np), refB = pair_ref_b(np);
            float dA, dB;
            pair_dist(np, t.lo, inv, dA, dB);
            c.aabb += 2;
            const bool bFirst = dB < dA;  // :430-444
            const uint32_t nearRef = bFirst ? refB : refA, farRef = bFirst ? refA : refB;
            const bool nearOk = (bFirst ? dB : dA) < t.best_t, farOk = (bFirst ? dA : dB) < t.best_t;
            // (isect_meshes' if/else chain as selects, the same decision: either form in both places changes kernels)
            if (nearOk && farOk) stk.push(t.sp, farRef);
            t.node = nearOk ? nearRef : farRef;
            if (!nearOk && !farOk) t.node = t.sp > 0 ? stk.pop(t.sp) : HG_NONE;
        }
        dm = act_mask & wave_ballot(int32_t(t.node) >= 0);
    }
    // Distributed leaf test (HG_LEAF_DIST of rounds 1-4: C3 2013 -> 2074 Mpaths/s, leaf-loop lane utilisation 25 % ->
    // 70 %, tools/sweeps/sweep52.txt); check builds fall back to the lane's own sequential loop under a partial EXEC
    const bool at_leaf = act && t.node != HG_NONE && (t.node & HG_LEAF_BIT);
    uint32_t first = 0u, n = 0u;
    if (at_leaf) {
        const uint2 lr = leaf_range(kp, t.node);
        first = lr.x;
        n = lr.y;
    }
    if (leaf_dist(kp, LeafRay{t.lo, t.ld, t.best_t, t.best_u, t.best_v, t.best_tri, t.best_mesh, t.mi}, c, ls, first,
                  n)) {
        if (at_leaf) t.node = t.sp > 0 ? stk.pop(t.sp) : HG_NONE;
    } else if (at_leaf) {  // (HG_CHECK_EXEC builds only) :404-420, the next triangle's loads out before this one's test
        const uint2 leaf = leaf_range(kp, t.node);
        const uint32_t end = leaf.x + leaf.y;
        float4 na, nb;
        float nc;
        tri_load(kp, leaf.x, na, nb, nc);
        for (uint32_t ti = leaf.x; ti < end; ++ti) {
            c.tri_rounds += wave_once();
            const float4 a = na, b = nb;
            const float cz = nc;
            const uint32_t tn = ti + 1 < end ? ti + 1 : ti;
            tri_load(kp, tn, na, nb, nc);
            c.tri++;
            float tt, U, V;
            bool front;
            if (tri_accept(t.lo, t.ld, a, b, cz, t.best_t, tt, U, V, front)) {
                t.best_t = tt;
                t.best_u = U;
                t.best_v = V;
                t.best_tri = ti | (front ? 0u : 0x80000000u);
                t.best_mesh = t.mi;
            }
        }
        t.node = t.sp > 0 ? stk.pop(t.sp) : HG_NONE;
    }
    if (act && t.node == HG_NONE) {
        const uint32_t nm = uint32_t(kp.n_meshes);
        t.mi = next_live_mesh(t.live, t.mi + 1u, nm);
        f3 inv_next;
        if (t.mi < nm) mesh_local_ray<kMeshLds>(kp, ray, t.mi, t.lo, t.ld, inv_next, t.node);
    }
}

// The hit get_ray_intersection returns, from a finished traversal (:452-471 and the sphere pass).
template <bool kMeshLds = false>
__device__ __forceinline__ Hit trav_hit(const HgKernelParams& kp, const Ray& ray, const Trav& t) {
    Hit h = hit_none(t.sph_t);
    if (t.best_t < (t.sph_t - 0.0001f) && t.best_t < kp.far_)
        resolve_mesh<kMeshLds>(kp, ray, t.best_t, t.best_u, t.best_v, t.best_tri, t.best_mesh, h);
    else if (t.sph != HG_NONE)
        resolve_sphere(kp, ray, t.sph, h);
    return h;
}

}  // namespace hgd
