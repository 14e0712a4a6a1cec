// hg_atrous.h — the display denoiser of hg_readback_begin_denoised (include/halogen_abi.h), one definition for the
// device kernels (hg_denoise.hip) and the host twin hg_denoise_host (hg_host_denoise.cpp): an edge-avoiding a-trous
// filter (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination
// Filtering", HPG 2010) over the colour, the first-hit normal and the first-hit distance along the ray (in place of
// the paper's position).  Not in the reference.
//
// The contract, in the order the arithmetic is done (fp32, no contraction: both sides build with -ffp-contract=off):
//   input       colour C (rgba), guide0 = (normal.xyz, t), guide1 = (albedo.rgb, kind); a miss has t = +inf
//   demodulate  a = hg_fmaxf(albedo, 1e-3f) per channel, c = C.rgb / a             (else c = C.rgb)
//   iteration i s = 1 << i, sigma_c = sigma_color * 2^-i, r = 1.0f / (sigma * sigma) for each term that is on
//     taps      dy = -2..2 outer, dx = -2..2 inner, q = p + s * (dx, dy); a tap outside the image is skipped
//     h         k[|dy|] * k[|dx|], k = {0.375f, 0.25f, 0.0625f}
//     e         0; colour term on: d = c_p - c_q, e = e + ((d.x*d.x + d.y*d.y) + d.z*d.z) * r_c; the normal term the
//               same over guide0.xyz with r_n; depth term on and t_p != t_q: dz = t_p - t_q, e = e + (dz * dz) * r_z.
//               Exactly one of p, q a miss: e = +inf (whatever terms are on); two misses compare as equal depths
//     w         h * hg_expf(-e); sum = sum + w * c_q per channel; wsum = wsum + w
//     result    c'_p = sum / wsum (the centre tap has e = 0, so wsum >= 9/64); alpha is carried unchanged
//     every iteration reads the previous iteration's whole image
//   output      rgb = c * a when demodulated, else c; alpha = C_p.a
#pragma once
#include <stdint.h>

#include "halogen_abi.h"
#include "hg_fmath.h"

#define HG_ATROUS_MAX_ITERATIONS 6
#define HG_ATROUS_ALBEDO_FLOOR 1e-3f
#define HG_ATROUS_MAX_PIXELS (int64_t(1) << 28)  // the device filter addresses a pixel's 16-B record with 32-bit byte offsets

// What one iteration reads of hg_denoise_params: the step and the reciprocal squared sigmas (0: the term is off)
struct HgAtrousIter {
    int32_t step;
    float rc, rn, rz;
};

HG_FN bool hg_atrous_sigma_ok(float s) { return !(s > 0.0f) ? s == s : (s >= 1e-4f && s <= 1e4f); }

// hg_denoise_params as the entry points accept them (everything else is HG_E_INVALID)
HG_FN bool hg_atrous_params_ok(const hg_denoise_params& p) {
    return p.iterations >= 1 && p.iterations <= HG_ATROUS_MAX_ITERATIONS && p.flags == 0u &&
           (p.demodulate == 0 || p.demodulate == 1) && hg_atrous_sigma_ok(p.sigma_color) &&
           hg_atrous_sigma_ok(p.sigma_normal) && hg_atrous_sigma_ok(p.sigma_depth);
}

HG_FN float hg_atrous_rsq(float sigma) { return sigma > 0.0f ? 1.0f / (sigma * sigma) : 0.0f; }

HG_FN HgAtrousIter hg_atrous_iter(const hg_denoise_params& p, int32_t i) {
    // sigma_color * 2^-i: exact (a sigma that is on is >= 1e-4, i <= 5)
    const float sc = p.sigma_color > 0.0f ? p.sigma_color * hg_u2f(uint32_t(127 - i) << 23) : 0.0f;
    return HgAtrousIter{int32_t(1) << i, hg_atrous_rsq(sc), hg_atrous_rsq(p.sigma_normal), hg_atrous_rsq(p.sigma_depth)};
}

HG_FN float hg_atrous_albedo(float a) { return hg_fmaxf(a, HG_ATROUS_ALBEDO_FLOOR); }

// The demodulated colour of a pixel: c (rgba) divided per channel by its floored albedo (guide1.rgb), alpha kept
HG_FN void hg_atrous_demodulate(float c[4], const float albedo[3]) {
    c[0] = c[0] / hg_atrous_albedo(albedo[0]);
    c[1] = c[1] / hg_atrous_albedo(albedo[1]);
    c[2] = c[2] / hg_atrous_albedo(albedo[2]);
}

HG_FN void hg_atrous_remodulate(float c[3], const float albedo[3]) {
    c[0] = c[0] * hg_atrous_albedo(albedo[0]);
    c[1] = c[1] * hg_atrous_albedo(albedo[1]);
    c[2] = c[2] * hg_atrous_albedo(albedo[2]);
}

// One tap of pixel p (colour cp, guide gp) at q (cq, gq) with the kernel weight h, added to sum[0..2] and *wsum
HG_FN void hg_atrous_tap(const HgAtrousIter& it, float h, const float cp[3], const float gp[4], const float cq[3],
                         const float gq[4], float sum[3], float* wsum) {
    float e = 0.0f;
    if (it.rc > 0.0f) {
        const float dx = cp[0] - cq[0], dy = cp[1] - cq[1], dz = cp[2] - cq[2];
        e = e + ((dx * dx + dy * dy) + dz * dz) * it.rc;
    }
    if (it.rn > 0.0f) {
        const float dx = gp[0] - gq[0], dy = gp[1] - gq[1], dz = gp[2] - gq[2];
        e = e + ((dx * dx + dy * dy) + dz * dz) * it.rn;
    }
    if (it.rz > 0.0f && gp[3] != gq[3]) {
        const float dz = gp[3] - gq[3];
        e = e + (dz * dz) * it.rz;
    }
    if ((gp[3] == HG_INF) != (gq[3] == HG_INF)) e = HG_INF;
    const float w = h * hg_expf(-e);
    sum[0] = sum[0] + w * cq[0];
    sum[1] = sum[1] + w * cq[1];
    sum[2] = sum[2] + w * cq[2];
    *wsum = *wsum + w;
}

HG_FN float hg_atrous_k(int32_t d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// One iteration's output at pixel (x, y) of a W x H image: fetch(qx, qy, c, g) hands out the previous iteration's
// colour (rgb) and guide0 at a pixel inside the image.  out = c'_p.rgb; the caller carries c_p.a over (the device
// kernel reads it again after the taps: one register less across the loop, hg_denoise.hip HG_ATROUS_VGPRS)
template <class Fetch>
HG_FN void hg_atrous_pixel(const HgAtrousIter& it, int32_t W, int32_t H, int32_t x, int32_t y, Fetch&& fetch,
                           float out[3]) {
    float cp[3], gp[4];
    fetch(x, y, cp, gp);
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    for (int32_t dy = -2; dy <= 2; ++dy) {
        const int32_t qy = y + it.step * dy;
        if (qy < 0 || qy >= H) continue;
        for (int32_t dx = -2; dx <= 2; ++dx) {
            const int32_t qx = x + it.step * dx;
            if (qx < 0 || qx >= W) continue;
            float cq[3], gq[4];
            fetch(qx, qy, cq, gq);
            hg_atrous_tap(it, hg_atrous_k(dy) * hg_atrous_k(dx), cp, gp, cq, gq, sum, &wsum);
        }
    }
    out[0] = sum[0] / wsum;
    out[1] = sum[1] / wsum;
    out[2] = sum[2] / wsum;
}
