// hg_denoise.hip — the denoised display (hg_update_guides, hg_readback_begin_denoised; include/halogen_abi.h): the
// guide-buffer kernel (one closest-hit camera ray per pixel, no shading) and the edge-avoiding a-trous filter whose
// arithmetic csrc/hg_atrous.h defines for this file and for the host twin hg_denoise_host alike.  Not in the reference.
//
// A translation unit of its own: the kernels of hg_mega.hip and hg_query.hip compile to what they compile to without it.
// The kernels and their launchers first, then the entry points of the C-ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "halogen_abi.h"
#include "hg_atrous.h"
#include "hg_device.h"
#include "hg_rt.h"
#include "hg_tiling.h"

using namespace hgd;

#ifndef HG_GUIDE_WAVES
#define HG_GUIDE_WAVES 8  // as the closest-hit query kernel, whose traversal this is
#endif
constexpr int kGuideBlock = 256;  // four waves per workgroup, the lockstep kernel's [depth][thread] LDS stack

// One lane per pixel, 64 consecutive pixels of the row-major image per wave.  The ray is hg_camera_rays_kernel's, the
// answer hg_query_kernel<false>'s for it (t_max = +inf), statement for statement.  Lanes past the image in the last
// wave stay in the wave with a ray that can hit nothing (t_max = -inf) and write nothing: the traversal's wave loop
// ballots over all 64 lanes.
__global__ __launch_bounds__(kGuideBlock, HG_GUIDE_WAVES) void hg_guides_kernel(const HgKernelParams kp, uint32_t frame,
                                                                                float4* __restrict__ guide0,
                                                                                float4* __restrict__ guide1,
                                                                                uint32_t first, uint32_t n) {
    const uint32_t k = blockIdx.x * uint32_t(kGuideBlock) + threadIdx.x;  // this launch's pixels [first, first + n)
    const uint32_t i = first + k;
    const bool live = k < n;
    Ray ray{mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 1.0f)};
    float t_max = -HG_INF;
    if (live) {
        const uint32_t px = i % kp.Wu, py = i / kp.Wu;
        const float ndcx = (float(px) / kp.W) * 2.0f - 1.0f;
        const float ndcy = (float(py) / kp.H) * 2.0f - 1.0f;
        const Sampler smp{frame, pcg_hash(px + py * kp.Wu), 0u};
        ray = camera_ray(kp, smp, ndcx, ndcy);
        t_max = HG_INF;
    }
    const MegaStack stk{threadIdx.x, uint32_t(kGuideBlock), kp.spill + k, kp.spill_stride};
    Hit h = hit_none(t_max);
    const uint32_t sph = isect_spheres(kp, ray, h.t);
    MeshBest mb{0.0f, 0.0f, HG_NONE, 0u};
    uint32_t kind = HG_HIT_NONE;
    if (isect_meshes_best<false>(kp, ray, h, mb, stk)) {
        kind = HG_HIT_MESH;
    } else if (sph != HG_NONE) {
        resolve_sphere(kp, ray, sph, h);
        kind = HG_HIT_SPHERE;
    }
    if (!live) return;
    if (kind == HG_HIT_NONE) {
        guide0[i] = make_float4(0.0f, 0.0f, 0.0f, HG_INF);
        guide1[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    } else {
        const float4 a = kp.materials[5u * h.mat];
        guide0[i] = make_float4(h.n.x, h.n.y, h.n.z, h.t);
        guide1[i] = make_float4(a.x, a.y, a.z, float(kind));
    }
}

// threads of a guide launch over n pixels (the spill buffer has one column per thread: kp.spill_stride)
uint32_t hg_guides_threads(uint32_t n) {
    return (n + uint32_t(kGuideBlock) - 1u) / uint32_t(kGuideBlock) * uint32_t(kGuideBlock);
}

hipError_t hg_launch_guides(const HgKernelParams& kp, uint32_t frame, void* guide0, void* guide1, uint32_t first,
                            uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = hg_guides_threads(n) / uint32_t(kGuideBlock);
    const size_t lds = size_t(kp.stack_depth < HG_MEGA_LDS_STACK ? kp.stack_depth : HG_MEGA_LDS_STACK) *
                       size_t(kGuideBlock) * sizeof(uint32_t);
    hipLaunchKernelGGL(hg_guides_kernel, dim3(grid), dim3(kGuideBlock), lds, stream, kp, frame,
                       static_cast<float4*>(guide0), static_cast<float4*>(guide1), first, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The filter.  Every kernel here is a one-wave workgroup with no LDS, as the display untile is (hg_display.hip
// launch_untile): a per-frame display runs them beside the render server's persistent trace waves, which hold most
// wave slots, and a larger workgroup would wait for a CU to drain.
// ---------------------------------------------------------------------------------------------------------------------

// Step 1: the accumulator (tile-major, one rank) untiled into a row-major colour image, demodulated by guide1's albedo
template <bool kDemod>
__global__ __launch_bounds__(64) void hg_atrous_prepare(float4* __restrict__ dst, const float4* __restrict__ acc,
                                                         const float4* __restrict__ guide1, int32_t W, int32_t H,
                                                         int32_t tiles_x) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= uint32_t(W) * uint32_t(H)) return;
    const HgPixelSource s = hg_pixel_source(i % uint32_t(W), i / uint32_t(W), uint32_t(tiles_x), 1u);
    const float4 v = acc[size_t(s.local_tile) * 64u + s.lane];
    float c[4] = {v.x, v.y, v.z, v.w};
    if constexpr (kDemod) {
        const float4 g = guide1[i];
        const float a[3] = {g.x, g.y, g.z};
        hg_atrous_demodulate(c, a);
    }
    dst[i] = make_float4(c[0], c[1], c[2], c[3]);
}

// The iteration kernel's register budget.  The render server's persistent waves hold 5 x 96 of a SIMD's 512 VGPRs
// (hg_trace_stream_kernel, HG_SV_WAVES), so a kernel of more than 32 cannot start beside them: at 37-39 VGPRs (the
// compiler's choice without the cap) the per-frame display loop with the server on ran at 20 Mpaths/s against the plain
// display's 2,837, every filter launch waiting for the server's waves to leave.  The kernel below needs exactly 32 (the
// alpha re-read after the taps, one 32-bit byte offset for both of a tap's loads); the attribute holds it there.  (The
// backend doubles an amdgpu_num_vgpr request on this target, whose AGPRs share the file: 16 asks for 32 in all.)
#ifndef HG_ATROUS_VGPRS
#define HG_ATROUS_VGPRS 16
#endif

// Step 2: one iteration, src -> dst.  A wave covers a (1 << kTx) x (64 >> kTx) block of pixels, one per lane; the 25
// taps of a lane are global loads of the colour and guide0 records (16 B each), which the wave's neighbours share
// through L1 / L2.  kRemod: the last iteration of a demodulated filter multiplies the albedo back in its store.
template <int kTx, bool kRemod>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(HG_ATROUS_VGPRS))) void hg_atrous_iterate(float4* __restrict__ dst, const float4* __restrict__ src,
                                                         const float4* __restrict__ guide0,
                                                         const float4* __restrict__ guide1, int32_t W, int32_t H,
                                                         const HgAtrousIter it) {
    const int32_t x = int32_t(blockIdx.x << kTx) + int32_t(threadIdx.x & ((1u << kTx) - 1u));
    const int32_t y = int32_t(blockIdx.y * (64u >> kTx)) + int32_t(threadIdx.x >> kTx);
    if (x >= W || y >= H) return;
    // a pixel's record in the three images at one 32-bit byte offset from each base (at most HG_ATROUS_MAX_PIXELS
    // pixels): one address register for both of a tap's loads
    const auto at = [](const float4* base, uint32_t off) {
        return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + off);
    };
    float out[3];
    hg_atrous_pixel(it, W, H, x, y,
                    [&](int32_t qx, int32_t qy, float c[3], float g[4]) {
                        const uint32_t q = (uint32_t(qy) * uint32_t(W) + uint32_t(qx)) * 16u;
                        const float4 cv = at(src, q), gv = at(guide0, q);
                        c[0] = cv.x, c[1] = cv.y, c[2] = cv.z;
                        g[0] = gv.x, g[1] = gv.y, g[2] = gv.z, g[3] = gv.w;
                    },
                    out);
    const uint32_t p = (uint32_t(y) * uint32_t(W) + uint32_t(x)) * 16u;
    if constexpr (kRemod) {
        const float4 g = at(guide1, p);
        const float a[3] = {g.x, g.y, g.z};
        hg_atrous_remodulate(out, a);
    }
    *reinterpret_cast<float4*>(reinterpret_cast<char*>(dst) + p) = make_float4(out[0], out[1], out[2], at(src, p).w);
}

namespace {

// The block of pixels a wave covers: 0 = 64 x 1 (a row segment; the default: every tap of the wave is one contiguous
// 1-KB load, the fastest at every step), 1 = 16 x 4, 2 = 8 x 8.  HALOGEN_ATROUS_TILE selects
// another (a measuring aid, tools/bench_denoise.py); same images.
int atrous_tile() {  // (read per call: the tool switches it between timed blocks of one process)
    const char* e = std::getenv("HALOGEN_ATROUS_TILE");
    const int v = e ? std::atoi(e) : 0;
    return v >= 0 && v <= 2 ? v : 0;
}

template <int kTx>
void launch_iterate(void* dst, const void* src, const void* guide0, const void* guide1, int32_t W, int32_t H,
                    const HgAtrousIter& it, bool remod, hipStream_t stream) {
    const uint32_t tx = 1u << kTx, ty = 64u >> kTx;
    const dim3 g((uint32_t(W) + tx - 1u) / tx, (uint32_t(H) + ty - 1u) / ty), b(64);
    if (remod)
        hipLaunchKernelGGL((hg_atrous_iterate<kTx, true>), g, b, 0, stream, static_cast<float4*>(dst),
                           static_cast<const float4*>(src), static_cast<const float4*>(guide0),
                           static_cast<const float4*>(guide1), W, H, it);
    else
        hipLaunchKernelGGL((hg_atrous_iterate<kTx, false>), g, b, 0, stream, static_cast<float4*>(dst),
                           static_cast<const float4*>(src), static_cast<const float4*>(guide0),
                           static_cast<const float4*>(guide1), W, H, it);
}

}  // namespace

// The whole filter on `stream`: acc (tile-major, untiled here) -> work[0], then the iterations between work[0] and
// work[1].  Returns through *result the image that holds the output (row-major W x H float4).  The parameters are
// valid (hg_atrous_params_ok) and the image has at most HG_ATROUS_MAX_PIXELS pixels.
hipError_t hg_launch_denoise(const void* acc, const void* guide0, const void* guide1, void* const work[2], int32_t W,
                             int32_t H, int32_t tiles_x, const hg_denoise_params& p, hipStream_t stream,
                             const void** result) {
    const size_t pixels = size_t(W) * size_t(H);
    const dim3 g(uint32_t((pixels + 63) / 64)), b(64);
    if (p.demodulate)
        hipLaunchKernelGGL(hg_atrous_prepare<true>, g, b, 0, stream, static_cast<float4*>(work[0]),
                           static_cast<const float4*>(acc), static_cast<const float4*>(guide1), W, H, tiles_x);
    else
        hipLaunchKernelGGL(hg_atrous_prepare<false>, g, b, 0, stream, static_cast<float4*>(work[0]),
                           static_cast<const float4*>(acc), static_cast<const float4*>(guide1), W, H, tiles_x);
    const int tile = atrous_tile();
    int at = 0;
    for (int32_t i = 0; i < p.iterations; ++i, at ^= 1) {
        const HgAtrousIter it = hg_atrous_iter(p, i);
        const bool remod = p.demodulate && i == p.iterations - 1;
        switch (tile) {
            case 1: launch_iterate<4>(work[at ^ 1], work[at], guide0, guide1, W, H, it, remod, stream); break;
            case 2: launch_iterate<3>(work[at ^ 1], work[at], guide0, guide1, W, H, it, remod, stream); break;
            default: launch_iterate<6>(work[at ^ 1], work[at], guide0, guide1, W, H, it, remod, stream); break;
        }
    }
    *result = work[at];
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The entry points
// ---------------------------------------------------------------------------------------------------------------------
using namespace hgrt;

extern "C" {

int hg_update_guides(hg_ctx* c, const hg_params* p, int32_t frame_count) {
    if (!c) return HG_E_INVALID;
    if (!p) return fail(c, HG_E_INVALID, "null params");
    if (!c->has_scene) return fail(c, HG_E_NOSCENE, "hg_upload_scene not called");
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (!(p->screenParameters.x == float(c->W) && p->screenParameters.y == float(c->H)))
        return fail(c, HG_E_INVALID, "screenParameters (%g,%g) are not the target's size %dx%d", p->screenParameters.x,
                    p->screenParameters.y, c->W, c->H);
    if (int rc = query_begin(c)) return rc;
    // the context is idle: the four images may move
    c->guides_valid = false;
    const size_t pixels = size_t(c->W) * size_t(c->H);
    for (DevBuf* b : {&c->guide0, &c->guide1, &c->denoise_work[0], &c->denoise_work[1]})
        if (int rc = ensure(c, *b, pixels * sizeof(float4))) return rc;
    // the closest-hit query's parameter block (the whole uploaded scene, far = +inf) with the caller's camera
    HgKernelParams kp;
    if (int rc = query_params(c, hg_guides_threads(uint32_t(std::min<size_t>(pixels, size_t(kQueryChunk)))), kp)) return rc;
    const float far_ = kp.far_;
    set_camera(kp, *p);
    kp.far_ = far_;
    for (size_t at = 0; at < pixels; at += size_t(kQueryChunk)) {  // in stream order: the launches share the spill buffer
        const uint32_t m = uint32_t(std::min(pixels - at, size_t(kQueryChunk)));
        HG_HIP(c, hg_launch_guides(kp, uint32_t(frame_count), c->guide0.p, c->guide1.p, uint32_t(at), m, c->stream));
    }
    HG_HIP(c, hipStreamSynchronize(c->stream));
    c->guides_valid = true;
    return HG_OK;
}

int hg_readback_guides(hg_ctx* c, float* guide0, float* guide1, size_t n_floats_each) {
    if (!c) return HG_E_INVALID;
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (!c->guides_valid) return fail(c, HG_E_INVALID, "no guide images for this scene and target: call hg_update_guides");
    const size_t bytes = size_t(c->W) * size_t(c->H) * sizeof(float4);
    if (n_floats_each * sizeof(float) < bytes) return fail(c, HG_E_INVALID, "guide buffer too small");
    if (int rc = set_device(c)) return rc;
    if (guide0) HG_HIP(c, hipMemcpyAsync(guide0, c->guide0.p, bytes, hipMemcpyDeviceToHost, c->stream));
    if (guide1) HG_HIP(c, hipMemcpyAsync(guide1, c->guide1.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

int hg_readback_begin_denoised(hg_ctx* c, int32_t format, const hg_denoise_params* p) {
    if (!c) return HG_E_INVALID;
    if (!p) return fail(c, HG_E_INVALID, "null denoise params");
    if (!hg_atrous_params_ok(*p))
        return fail(c, HG_E_INVALID,
                    "bad denoise params: iterations %d (1..%d), sigmas %g %g %g (off, or in [1e-4, 1e4]), demodulate %d, "
                    "flags %u", p->iterations, HG_ATROUS_MAX_ITERATIONS, p->sigma_color, p->sigma_normal, p->sigma_depth,
                    p->demodulate, p->flags);
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = display_check(c, format)) return rc;  // (a full ring refuses before the filter is launched)
    if (c->n_ranks > 1)
        return fail(c, HG_E_UNSUPPORTED, "denoised display of a tiled context (rank %d of %d): a rank's share has no "
                    "neighbours", c->rank, c->n_ranks);
    if (int64_t(c->W) * c->H > HG_ATROUS_MAX_PIXELS)
        return fail(c, HG_E_UNSUPPORTED, "denoised display of more than 2^28 pixels (%dx%d)", c->W, c->H);
    if (!c->guides_valid) return fail(c, HG_E_INVALID, "no guide images for this scene and target: call hg_update_guides");
    if (int rc = set_device(c)) return rc;
    // on the context stream, after every frame rendered so far (the server keeps tracing: nothing here waits)
    void* const work[2] = {c->denoise_work[0].p, c->denoise_work[1].p};
    const void* denoised = nullptr;
    HG_HIP(c, hg_launch_denoise(c->acc.p, c->guide0.p, c->guide1.p, work, c->W, c->H, c->tiles_x, *p, c->stream, &denoised));
    return hg_ctx_display_begin(c, denoised, format);
}

}  // extern "C"
