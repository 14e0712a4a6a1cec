// hg_dev_shade.h — the BSDF, the medium stack, the bounce loops and the camera ray (part of hg_device.h).
#pragma once
#include <hip/hip_runtime.h>

#include "hg_dev_sampler.h"
#include "hg_dev_sky.h"
#include "hg_dev_trav.h"

namespace hgd {

// ---------------------------------------------------------------------------------------------------
// BSDF (:491-741) and medium stack (:582-665)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ f3 lambert(f3 n, f3 rv) {  // :491-501
    f3 p = rv + n;
    if (len(p) < 1e-8f) p = n;
    return normalize(p);
}
__device__ __forceinline__ f3 reflect(f3 i, f3 n) { return i - n * (2.0f * dot(i, n)); }  // :506-509

__device__ __forceinline__ float schlick_adjusted(float n1, float n2, f3 nrm, f3 inc, float mn, float mx) {
    float r0 = (n1 - n2) / (n1 + n2);  // :519-540
    r0 *= r0;
    float cosX = -dot(nrm, inc);
    if (n1 > n2) {
        float n = n1 / n2;
        float sinT2 = n * n * (1.0f - cosX * cosX);
        if (sinT2 > 1.0f) return mx;
        cosX = __builtin_sqrtf(1.0f - sinT2);
    }
    float x = 1.0f - cosX;
    float ret = r0 + (1.0f - r0) * x * x * x * x * x;
    return mn + ret * (mx - mn);
}

__device__ __forceinline__ f3 refract_tir(f3 inc, f3 nrm, float n1, float n2, bool& tir) {  // :557-572
    float ct = hg_fminf(dot(-inc, nrm), 1.0f);
    float st = __builtin_sqrtf(1.0f - ct * ct);
    float n12 = n1 / n2;
    if (n12 * st > 1.0f) {
        tir = true;
        return reflect(inc, nrm);
    }
    f3 perp = (inc + nrm * ct) * n12;
    float lp = len(perp);
    f3 par = nrm * (-__builtin_sqrtf(fabsf(1.0f - lp * lp)));
    return perp + par;
}

struct Medium {
    float ior;
    f3 absorb;
    uint32_t id;
};
template <bool kMatLds = false>
__device__ __forceinline__ Medium medium_of(const HgKernelParams& kp, uint32_t m) {
    const float4 ai = mat_f4<kMatLds>(kp, m, 3);
    const float4 pr = mat_f4<kMatLds>(kp, m, 4);
    return Medium{ai.w, xyz(ai), __float_as_uint(pr.y)};
}
__device__ __forceinline__ Medium empty_medium() { return Medium{1.0f, mk(0, 0, 0), 0xFFFFFFFFu}; }
template <bool kMatLds = false>
__device__ __forceinline__ Medium top_medium(const HgKernelParams& kp, const MediumStack& ms) {
    return ms.sp > 0 ? medium_of<kMatLds>(kp, ms.get(ms.sp - 1)) : empty_medium();
}
template <bool kMatLds = false>
__device__ void medium_push(const HgKernelParams& kp, MediumStack& ms, uint32_t m) {  // :582-622
    if (ms.sp == 0) {
        ms.s = uint64_t(m);
        ms.sp = 1;
        return;
    }
    const int32_t prio = mat_priority<kMatLds>(kp, m);
    int ins = ms.sp;
    if (prio > mat_priority<kMatLds>(kp, ms.get(ms.sp - 1))) {
        for (int i = ms.sp - 1; i >= 0; --i) {
            if (prio < mat_priority<kMatLds>(kp, ms.get(i))) {
                ins = i + 1;
                break;
            }
        }
        if (ins == ms.sp) ins = 0;
    }
    if (ms.sp >= 8) return;  // overflow: dropped (reference UB; same rule in the oracle)
    const uint64_t low_mask = ins == 0 ? 0ull : (~0ull >> (64 - 8 * ins));
    const uint64_t low = ms.s & low_mask;
    const uint64_t high = ms.s & ~low_mask;
    ms.s = low | (high << 8) | (uint64_t(m) << (8 * ins));
    ms.sp++;
}
template <bool kMatLds = false>
__device__ void medium_pop(const HgKernelParams& kp, MediumStack& ms, uint32_t id) {  // :627-642
    for (int i = 0; i < ms.sp; ++i) {
        if (medium_of<kMatLds>(kp, ms.get(i)).id == id) {
            const uint64_t low_mask = i == 0 ? 0ull : (~0ull >> (64 - 8 * i));
            const uint64_t low = ms.s & low_mask;
            const uint64_t high = (i + 1 < 8) ? ((ms.s >> (8 * (i + 1))) << (8 * i)) : 0ull;
            ms.s = low | high;
            ms.sp--;
            return;
        }
    }
}

// material_BRDF :672-741
__device__ f3 material_brdf(const HgKernelParams& kp, const Sampler& smp, Ray& ray, const Hit& hit, const Mat& mt,
                            const Medium& cur, const Medium& hm, uint32_t& bt) {
    f3 att;
    float rr0, rr1, pr0, pr1;
    smp.get2(ID_ROUGH, rr0, rr1);
    smp.get2(ID_PROPERTY, pr0, pr1);
    // get_random_unit_vector (HalogenRandom.hlsl:282-298)
    const float theta = rr0 * 2.0f * HLSL_PI;
    const float phi = hg_acosf_fused(2.0f * rr1 - 1.0f);  // = hg_acosf (tests/test_fmath.py, every input)
    float sT, cT, sP, cP;  // = hg_sinf / hg_cosf of each angle, one reduction per angle (tests/test_fmath.py)
    hg_sincosf(theta, &sT, &cT);
    hg_sincosf(phi, &sP, &cP);
    const f3 rv = mk(1.0f * sP * cT, 1.0f * sP * sT, 1.0f * cP);
    const float rough2 = mt.prio_id_r2.z;
    if (!(pr0 > mt.albedo.w)) {
        att = xyz(mt.albedo);
        const f3 diffuse = lambert(hit.n, rv);
        const float metallic = mt.spec_metal.w;
        const float thr = (metallic > 0.0f) ? schlick_adjusted(cur.ior, hm.ior, hit.n, ray.d, metallic, 1.0f)
                                            : metallic;
        const bool spec = pr1 < thr;
        bt = spec ? 1u : 0u;
        if (spec) {
            ray.d = lerp(reflect(ray.d, hit.n), diffuse, rough2);
            att = xyz(mt.spec_metal);
        } else {
            ray.d = diffuse;
        }
        ray.o = hit.pos + hit.n * 0.0001f;
    } else {
        bt = 2u;
        att = mk(1, 1, 1);
        bool tir = false;
        ray.d = refract_tir(ray.d, hit.n, cur.ior, hm.ior, tir);
        const f3 dd = tir ? lambert(hit.n, rv) : lambert(-hit.n, rv);
        ray.d = lerp(ray.d, dd, rough2);
        ray.o = hit.pos - hit.n * 0.0001f;
    }
    ray.d = normalize(ray.d);
    return att;
}

// evaluate_material_hit :743-817
// bt_out: the bounceTypes[] slot this hit increments (0 diffuse, 1 glossy, 2 transmission; a false hit counts as
// transmission, :806)
template <bool kMatLds = false>
__device__ f3 evaluate_hit(const HgKernelParams& kp, const Sampler& smp, MediumStack& ms, Ray& ray, const Hit& hit,
                           const Mat& mt, uint32_t& bt_out) {
    const Medium internal = medium_of<kMatLds>(kp, hit.mat);
    const int32_t prio = __float_as_int(mt.prio_id_r2.x);
    Medium cur, hm;
    bool trueHit = true;
    if (prio >= 0) {
        trueHit = ms.sp == 0 || prio <= mat_priority<kMatLds>(kp, ms.get(ms.sp - 1));
        if (hit.orient == 1.0f) {
            cur = top_medium<kMatLds>(kp, ms);
            hm = internal;
            medium_push<kMatLds>(kp, ms, hit.mat);
        } else {
            cur = ms.sp == 0 ? internal : top_medium<kMatLds>(kp, ms);
            medium_pop<kMatLds>(kp, ms, internal.id);
            hm = top_medium<kMatLds>(kp, ms);
        }
    } else {
        if (hit.orient == 1.0f) {
            cur = top_medium<kMatLds>(kp, ms);
            hm = internal;
        } else {
            cur = internal;
            hm = top_medium<kMatLds>(kp, ms);
        }
    }
    f3 att;
    if (trueHit) {
        uint32_t bt = 0;
        att = material_brdf(kp, smp, ray, hit, mt, cur, hm, bt);
        bt_out = bt;
        if (hit.orient > 0.0f && bt != 2u) medium_pop<kMatLds>(kp, ms, internal.id);
    } else {
        ray.o = hit.pos - hit.n * 0.0001f;
        att = mk(1, 1, 1);
        bt_out = 2u;
    }
    if (cur.id != 0xFFFFFFFFu) {
        att = mk(att.x * hg_expf(-cur.absorb.x * hit.t), att.y * hg_expf(-cur.absorb.y * hit.t),
                 att.z * hg_expf(-cur.absorb.z * hit.t));
    }
    return att;
}

// trace_ray :876-950
template <class Stk>
__device__ f3 trace_ray(const HgKernelParams& kp, Sampler& smp, MediumStack& ms, Ray ray, Counters& c,
                        const Stk& stk) {
    f3 acc = mk(0, 0, 0), thr = mk(1, 1, 1);
    float acc_rough = 0.0f;
    Bounces bounce{0, 0, 0};
    for (uint32_t it = 0; it <= kp.max_bounces; ++it) {
        if (bounce.diffuse > kp.max_diff || bounce.glossy > kp.max_glossy || bounce.transmission > kp.max_trans)
            break;
        const Hit hit = intersect(kp, ray, c, stk);
        if (hit.t < kp.far_) {
            c.hits++;
            const Mat mt = load_mat(kp, hit.mat);
            acc = acc + xyz(mt.emis_rough) * thr;
            uint32_t bt = 0;
            const f3 att = evaluate_hit(kp, smp, ms, ray, hit, mt, bt);
            bounce.bump(bt);
            thr = thr * att;
            acc_rough += mt.emis_rough.w * thr.x;  // float3 -> float truncation (:911)
            const float rr = smp.get1(ID_RR);
            smp.offset += BOUNCE_INC;
            const float contribution = hg_fmaxf(hg_fmaxf(thr.x, thr.y), thr.z);
            if (rr > contribution) break;
            thr = thr * rcp_exact(contribution);
        } else {
            c.primary_miss += it == 0u;
            acc = acc + sample_sky(kp, ray.d, sky_level(kp, acc_rough)) * thr;
            break;
        }
    }
    return acc;
}

// trace_ray_debug :952-982
template <class Stk>
__device__ f3 trace_ray_debug(const HgKernelParams& kp, Sampler& smp, MediumStack& ms, Ray ray, Counters& c,
                              const Stk& stk) {
    const uint32_t tri0 = c.tri, box0 = c.aabb;  // TriangleTests = AABBTests = 0
    switch (kp.debug_mode) {
        default:
            return mk(0, 0, 0);
        case 1: {
            const Hit h = intersect(kp, ray, c, stk);
            if (h.t < kp.far_) return xyz(kp.materials[5 * h.mat]);
            return sample_sky(kp, ray.d, kp.default_mip);
        }
        case 2: {
            const Hit h = intersect(kp, ray, c, stk);
            if (h.t < kp.far_) return mk((h.n.x + 1.0f) / 2.0f, (h.n.y + 1.0f) / 2.0f, (h.n.z + 1.0f) / 2.0f);
            return sample_sky(kp, ray.d, kp.default_mip);
        }
        case 3:
        case 4:
        case 5: {
            trace_ray(kp, smp, ms, ray, c, stk);
            const uint32_t tt = c.tri - tri0, bb = c.aabb - box0;
            if (kp.debug_mode == 3) {
                if (tt > kp.tri_range) return mk(1, 1, 1);
                return mk(float(tt) / float(kp.tri_range), 0, 0);
            }
            if (kp.debug_mode == 4) {
                if (bb > kp.box_range) return mk(1, 1, 1);
                return mk(float(bb) / float(kp.box_range), 0, 0);
            }
            if (tt > kp.tri_range || bb > kp.box_range) return mk(1, 1, 1);
            return mk(float(tt) / float(kp.tri_range), 0, float(bb) / float(kp.box_range));
        }
    }
}

// inverted_blackman_harris_cdf_approximation (HalogenRandom.hlsl:319-330)
__device__ __forceinline__ float inv_blackman_harris(float x) {
    const float a = (x * 1.99221575606f) - 0.99610787803f;
    return (0.5f * hg_logf((1.0f + a) / (1.0f - a))) / 6.24f;
}

// get_ray :996-1013 (+ get_ray_jitter :984-994, get_random_point_circle HalogenRandom.hlsl:303-308)
__device__ Ray camera_ray(const HgKernelParams& kp, const Sampler& smp, float ndcx, float ndcy) {
    float j0, j1;
    f3 ap = mk(0.0f, 0.0f, 0.0f);
    // Pinhole (disc radius 0): ap is (+-0, +-0, 0), the zeros' signs those of cos / sin.  Nothing below can see them
    // when the camera translation has no zero component (m[3] + (+-0) = m[3] in xform) and pf has no -0 component:
    // ndcx, ndcy are never -0 (x - 1 rounds an exact 0 to +0), so with vw, vh > 0 screen.x, .y are never -0 either
    // (+0 + -0 = +0; no sum underflows), and normalize / the focal distance > 0 keep the sign.  Then pf - (+-0) = pf,
    // and the focal sample and its sincos are skipped: the same bits.
    if (!(kp.focal_disc_radius == 0.0f && kp.cam[3] != 0.0f && kp.cam[7] != 0.0f && kp.cam[11] != 0.0f &&
          kp.vw > 0.0f && kp.vh > 0.0f && kp.near_ > 0.0f && kp.focal_dist > 0.0f)) {
        float fd0, fd1;
        smp.get2(ID_FOCAL, fd0, fd1);
        const float th = (fd0 * 360.0f) * HG_DEG2RAD;
        float sth, cth;
        hg_sincosf(th, &sth, &cth);
        ap = mk(cth * kp.focal_disc_radius * fd1, sth * kp.focal_disc_radius * fd1, 0.0f);
    }
    f3 screen = mk(ndcx * kp.vw, ndcy * kp.vh, 1.0f * kp.near_);
    smp.get2(ID_JITTER, j0, j1);
    const float jx = (inv_blackman_harris(j0) - 0.5f) * 2.0f * kp.filter_radius * kp.psx;
    const float jy = (inv_blackman_harris(j1) - 0.5f) * 2.0f * kp.filter_radius * kp.psy;
    screen = screen + mk(jx, jy, 0.0f);
    const f3 pf = normalize(screen) * kp.focal_dist;
    const f3 csd = normalize(pf - ap);
    Ray r;
    r.o = xform(kp.cam, ap, 1.0f);
    r.d = normalize(xform(kp.cam, csd, 0.0f));
    return r;
}
}  // namespace hgd
