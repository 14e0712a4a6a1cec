// hg_query.hip — ray queries over the uploaded scene (hg_trace_rays, hg_trace_rays_device, hg_camera_rays): the
// reference's get_ray_intersection (HalgoenCompute.compute:474-485) for a caller's rays, with no shading, no sampler and
// no accumulation, and the camera rays a frame traces (get_ray, :996-1013) handed out as such rays.
//
// A translation unit of its own: the megakernels of hg_mega.hip compile to what they compile to without it.  The
// kernels and their launchers first, then the entry points of the C-ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "halogen_abi.h"
#include "hg_device.h"
#include "hg_plan.h"
#include "hg_rt.h"

using namespace hgd;

static_assert(sizeof(hg_ray) == 32 && sizeof(hg_ray_hit) == 48, "the kernels move these records as float4");

#ifndef HG_QUERY_WAVES
#define HG_QUERY_WAVES 8  // waves/SIMD target: the traversal alone needs 59 (closest) / 48 (any) VGPRs, no scratch
#endif
constexpr int kQueryBlock = 256;  // four waves per workgroup, the lockstep kernel's [depth][thread] LDS stack

// One lane per ray, 64 consecutive rays per wave.  Record i is two float4: (origin, t_max), (direction, flags); result
// i is three: (t, kind, object, primitive), (u, v, material, orientation), (normal, 0).  Lanes past n in the last wave
// stay in the wave with a ray that can hit nothing (t_max = -inf: no triangle is accepted below it and every node
// test fails) and write nothing: the traversal's wave loop ballots over all 64 lanes.
template <bool kAny>
__global__ __launch_bounds__(kQueryBlock, HG_QUERY_WAVES) void hg_query_kernel(const HgKernelParams kp,
                                                                               const float4* __restrict__ rays,
                                                                               float4* __restrict__ hits, uint32_t n) {
    const uint32_t i = blockIdx.x * uint32_t(kQueryBlock) + threadIdx.x;
    const bool live = i < n;
    float4 ro = make_float4(0.0f, 0.0f, 0.0f, -HG_INF), rd = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    if (live) {
        ro = rays[2u * i];
        rd = rays[2u * i + 1u];
    }
    const MegaStack stk{threadIdx.x, uint32_t(kQueryBlock), kp.spill + i, kp.spill_stride};
    const Ray ray{mk(ro.x, ro.y, ro.z), mk(rd.x, rd.y, rd.z)};
    Hit h = hit_none(ro.w);  // the closest distance is seeded with t_max (+inf: the path tracer's get_ray_intersection)
    const uint32_t sph = isect_spheres(kp, ray, h.t);
    MeshBest mb{0.0f, 0.0f, HG_NONE, 0u};
    uint32_t kind = HG_HIT_NONE, object = 0u, prim = 0u;
    if constexpr (kAny) {
        // a sphere hit alone makes the closest query report a hit; such a lane brings a ray that hits no mesh
        if (sph != HG_NONE) h.t = -HG_INF;
        const bool mesh = isect_meshes_best<true>(kp, ray, h, mb, stk);
        kind = sph != HG_NONE ? uint32_t(HG_HIT_SPHERE) : mesh ? uint32_t(HG_HIT_MESH) : uint32_t(HG_HIT_NONE);
        h.t = kind != HG_HIT_NONE ? 0.0f : HG_INF;
        mb.u = mb.v = 0.0f;
    } else {
        if (isect_meshes_best<false>(kp, ray, h, mb, stk)) {
            kind = HG_HIT_MESH;
            object = mb.mesh;
            prim = mb.tri & 0x7FFFFFFFu;
        } else if (sph != HG_NONE) {
            resolve_sphere(kp, ray, sph, h);
            kind = HG_HIT_SPHERE;
            object = sph & 0x7FFFFFFFu;
            mb.u = mb.v = 0.0f;  // (a mesh hit inside the 1e-4 band behind the sphere is not the answer)
        } else {
            h.t = HG_INF;  // a miss: +inf whatever t_max was, everything else 0
            mb.u = mb.v = 0.0f;
        }
    }
    if (live) {
        hits[3u * i] = make_float4(h.t, __uint_as_float(kind), __uint_as_float(object), __uint_as_float(prim));
        hits[3u * i + 1u] = make_float4(mb.u, mb.v, __uint_as_float(h.mat), h.orient);
        hits[3u * i + 2u] = make_float4(h.n.x, h.n.y, h.n.z, 0.0f);
    }
}

// The first camera ray (sample 0) frame `frame` traces for each listed pixel: camera_ray seeded as hg_trace_kernel
// seeds it (hg_mega.hip), ndc of :1023-1033.  (Spelled out here and in the guide kernel of hg_denoise.hip, not shared:
// a helper that reads W, H and Wu through a reference to kp moves those loads to the kernel's entry.)
__global__ __launch_bounds__(kQueryBlock) void hg_camera_rays_kernel(const HgKernelParams kp, uint32_t frame,
                                                                     const int2* __restrict__ pixels,
                                                                     float4* __restrict__ rays, uint32_t n) {
    const uint32_t i = blockIdx.x * uint32_t(kQueryBlock) + threadIdx.x;
    if (i >= n) return;
    const int2 p = pixels[i];
    const uint32_t px = uint32_t(p.x), py = uint32_t(p.y);
    const float ndcx = (float(px) / kp.W) * 2.0f - 1.0f;
    const float ndcy = (float(py) / kp.H) * 2.0f - 1.0f;
    const Sampler smp{frame, pcg_hash(px + py * kp.Wu), 0u};
    const Ray r = camera_ray(kp, smp, ndcx, ndcy);
    rays[2u * i] = make_float4(r.o.x, r.o.y, r.o.z, HG_INF);
    rays[2u * i + 1u] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
}

// threads of a query launch over n rays (the spill buffer has one column per thread: kp.spill_stride)
uint32_t hg_query_threads(uint32_t n) {
    return (n + uint32_t(kQueryBlock) - 1u) / uint32_t(kQueryBlock) * uint32_t(kQueryBlock);
}
// LDS stack entries per lane of the query kernel; deeper entries go to kp.spill
uint32_t hg_query_lds_stack() { return HG_MEGA_LDS_STACK; }

hipError_t hg_launch_query(const HgKernelParams& kp, const void* rays, void* hits, uint32_t n, bool any,
                           hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = hg_query_threads(n) / uint32_t(kQueryBlock);
    const size_t lds = size_t(kp.stack_depth < HG_MEGA_LDS_STACK ? kp.stack_depth : HG_MEGA_LDS_STACK) *
                       size_t(kQueryBlock) * sizeof(uint32_t);
    if (any)
        hipLaunchKernelGGL((hg_query_kernel<true>), dim3(grid), dim3(kQueryBlock), lds, stream, kp,
                           static_cast<const float4*>(rays), static_cast<float4*>(hits), n);
    else
        hipLaunchKernelGGL((hg_query_kernel<false>), dim3(grid), dim3(kQueryBlock), lds, stream, kp,
                           static_cast<const float4*>(rays), static_cast<float4*>(hits), n);
    return hipGetLastError();
}

hipError_t hg_launch_camera_rays(const HgKernelParams& kp, uint32_t frame, const void* pixels, void* rays, uint32_t n,
                                 hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = hg_query_threads(n) / uint32_t(kQueryBlock);
    hipLaunchKernelGGL(hg_camera_rays_kernel, dim3(grid), dim3(kQueryBlock), 0, stream, kp, frame,
                       static_cast<const int2*>(pixels), static_cast<float4*>(rays), n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The entry points
// ---------------------------------------------------------------------------------------------------------------------
namespace hgrt {

// What every entry point but hg_render does first, as far as hg_synchronize takes it: the held frames launched, the
// render server stopped, every stream of the context idle
int query_begin(hg_ctx* c) {
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = set_device(c)) return rc;
    return quiesce(c);
}

// The parameter block of a query launch of `threads` threads: the uploaded scene (all of it: no bufferCounts, no
// tiling), far = +inf, the lockstep kernel's descent threshold; nothing of the target, the uniforms or the counters
int query_params(hg_ctx* c, uint32_t threads, HgKernelParams& kp) {
    kp = HgKernelParams{};
    kp.far_ = HG_INF;
    kp.n_spheres = c->n_spheres;
    kp.n_meshes = c->n_meshes;
    set_scene(kp, c, hg_descent_t(c->descent_t, c->stack_depth, HG_KERNEL_MEGA));
    kp.spill_stride = threads;
    const uint32_t lds_part = hg_query_lds_stack();
    if (kp.stack_depth > lds_part) {  // one spill column per thread (the context is idle: the buffer may move)
        if (int rc = ensure(c, c->spill, size_t(threads) * (kp.stack_depth - lds_part) * sizeof(uint32_t))) return rc;
        kp.spill = static_cast<uint32_t*>(c->spill.p);
    }
    return HG_OK;
}

}  // namespace hgrt

using namespace hgrt;

namespace {

int query_args(hg_ctx* c, const void* in, int64_t n, int32_t mode, const void* out) {
    if (n < 0) return fail(c, HG_E_INVALID, "negative ray count");
    if (mode != HG_RAYS_CLOSEST && mode != HG_RAYS_ANY) return fail(c, HG_E_INVALID, "unknown ray query mode %d", mode);
    if (!in || !out) return fail(c, HG_E_INVALID, "null array with a non-zero ray count");
    if (!c->has_scene) return fail(c, HG_E_NOSCENE, "hg_upload_scene not called");
    return HG_OK;
}

// n rays at device pointers, in launches of at most kQueryChunk; the context is idle (query_begin) and the caller waits
// for the stream
int query_launch(hg_ctx* c, const void* d_rays, int64_t n, int32_t mode, void* d_hits) {
    HgKernelParams kp;
    if (int rc = query_params(c, hg_query_threads(uint32_t(std::min(n, kQueryChunk))), kp)) return rc;
    for (int64_t at = 0; at < n; at += kQueryChunk) {
        const uint32_t m = uint32_t(std::min(n - at, kQueryChunk));
        HG_HIP(c, hg_launch_query(kp, static_cast<const hg_ray*>(d_rays) + at, static_cast<hg_ray_hit*>(d_hits) + at, m,
                                  mode == HG_RAYS_ANY, c->stream));
    }
    return HG_OK;
}

}  // namespace

extern "C" {

int hg_trace_rays_device(hg_ctx* c, const void* d_rays, int64_t n, int32_t mode, void* d_hits) {
    if (!c) return HG_E_INVALID;
    if (n == 0) return HG_OK;
    if (int rc = query_args(c, d_rays, n, mode, d_hits)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_rays) | reinterpret_cast<uintptr_t>(d_hits)) & 15u)
        return fail(c, HG_E_INVALID, "device ray / hit arrays must be 16-byte aligned");
    if (int rc = query_begin(c)) return rc;
    if (int rc = query_launch(c, d_rays, n, mode, d_hits)) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

int hg_trace_rays(hg_ctx* c, const hg_ray* rays, int64_t n, int32_t mode, hg_ray_hit* hits) {
    if (!c) return HG_E_INVALID;
    if (n == 0) return HG_OK;
    if (int rc = query_args(c, rays, n, mode, hits)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        const hg_ray& r = rays[i];
        if (!(std::isfinite(r.origin.x) && std::isfinite(r.origin.y) && std::isfinite(r.origin.z)))
            return fail(c, HG_E_INVALID, "ray %lld: origin is not finite", (long long)i);
        if (!(std::isfinite(r.direction.x) && std::isfinite(r.direction.y) && std::isfinite(r.direction.z)))
            return fail(c, HG_E_INVALID, "ray %lld: direction is not finite", (long long)i);
        if (r.direction.x == 0.0f && r.direction.y == 0.0f && r.direction.z == 0.0f)
            return fail(c, HG_E_INVALID, "ray %lld: zero direction", (long long)i);
        if (std::isnan(r.t_max)) return fail(c, HG_E_INVALID, "ray %lld: t_max is NaN", (long long)i);
    }
    if (int rc = query_begin(c)) return rc;
    const size_t cap = size_t(std::min(n, kQueryChunk));
    if (int rc = ensure(c, c->query_in, cap * sizeof(hg_ray))) return rc;
    if (int rc = ensure(c, c->query_out, cap * sizeof(hg_ray_hit))) return rc;
    for (int64_t at = 0; at < n; at += kQueryChunk) {  // in stream order: a chunk's copies and launch reuse the staging
        const size_t m = size_t(std::min(n - at, kQueryChunk));
        HG_HIP(c, hipMemcpyAsync(c->query_in.p, rays + at, m * sizeof(hg_ray), hipMemcpyHostToDevice, c->stream));
        if (int rc = query_launch(c, c->query_in.p, int64_t(m), mode, c->query_out.p)) return rc;
        HG_HIP(c, hipMemcpyAsync(hits + at, c->query_out.p, m * sizeof(hg_ray_hit), hipMemcpyDeviceToHost, c->stream));
    }
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

int hg_camera_rays(hg_ctx* c, const hg_params* p, int32_t frame_count, const int32_t* pixels_xy, int64_t n,
                   hg_ray* rays) {
    if (!c) return HG_E_INVALID;
    if (n == 0) return HG_OK;
    if (n < 0) return fail(c, HG_E_INVALID, "negative pixel count");
    if (!p || !pixels_xy || !rays) return fail(c, HG_E_INVALID, "null params or array with a non-zero pixel count");
    const float Wf = p->screenParameters.x, Hf = p->screenParameters.y;
    if (!(Wf >= 1.0f && Hf >= 1.0f && Wf <= 65536.0f && Hf <= 65536.0f))
        return fail(c, HG_E_INVALID, "screenParameters (%g,%g) out of range", Wf, Hf);
    const int32_t W = int32_t(Wf), H = int32_t(Hf);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t x = pixels_xy[2 * i], y = pixels_xy[2 * i + 1];
        if (x < 0 || x >= W || y < 0 || y >= H)
            return fail(c, HG_E_INVALID, "pixel %lld: (%d,%d) outside the %dx%d screen", (long long)i, x, y, W, H);
    }
    if (int rc = query_begin(c)) return rc;
    HgKernelParams kp{};
    set_camera(kp, *p);
    const size_t cap = size_t(std::min(n, kQueryChunk));
    if (int rc = ensure(c, c->query_in, cap * 2 * sizeof(int32_t))) return rc;
    if (int rc = ensure(c, c->query_out, cap * sizeof(hg_ray))) return rc;
    for (int64_t at = 0; at < n; at += kQueryChunk) {
        const size_t m = size_t(std::min(n - at, kQueryChunk));
        HG_HIP(c, hipMemcpyAsync(c->query_in.p, pixels_xy + 2 * at, m * 2 * sizeof(int32_t), hipMemcpyHostToDevice,
                                 c->stream));
        HG_HIP(c, hg_launch_camera_rays(kp, uint32_t(frame_count), c->query_in.p, c->query_out.p, uint32_t(m), c->stream));
        HG_HIP(c, hipMemcpyAsync(rays + at, c->query_out.p, m * sizeof(hg_ray), hipMemcpyDeviceToHost, c->stream));
    }
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

}  // extern "C"
