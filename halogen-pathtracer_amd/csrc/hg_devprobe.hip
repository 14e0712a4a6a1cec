// hg_devprobe.hip — TEST INFRASTRUCTURE ONLY (make devprobe -> halogen/devprobe/libhg_devprobe.so; never linked into
// libhalogen_hip.so).  One elementwise entry point that evaluates the device building blocks of hg_device.h,
// hg_fmath.h and hg_pack.h themselves — the functions the megakernels call, not restatements — on caller-supplied
// inputs, so tests/test_gpu_device_units.py can put each next to its CPU-oracle counterpart (oracle/hg_oracle.c
// hgo_fmath and the hgo_*_batch exports) bit for bit.
//
// hg_devprobe(fn, in, in_bytes, out, out_bytes, n): element i reads kIn[fn] words at in + i * kIn[fn] and writes
// kOut[fn] words at out + i * kOut[fn] (host pointers; 4-byte words, float or uint32 bits):
//   0..11  hg_fmath.h, the codes of hgo_fmath: 0 sin, 1 cos, 2 acos, 3 tan, 4 log, 5 exp, 6 round, 7 rnorm, 8 asin,
//          9 / 10 sin / cos of hg_sincosf, 11 acos_fused                              in: x                  out: y
//   12/13  hg_fminf / hg_fmaxf                                                       in: a, b               out: y
//   20     hgd::rcp_exact                                                            in: x                  out: 1/x
//   21     hgd::pcg_hash                                                             in: v                  out: hash
//   22     hgd::Sampler::get1                                in: frame, pixel, offset, id                   out: u
//   23     hgd::Sampler::get2                                in: frame, pixel, offset, id                   out: a, b
//   30     hgd::ray_aabb                                     in: A, B, o, inv (12 floats)                   out: t
//   31/32  hgd::tri_accept<false> / <true>                   in: lo, ld, best_t, record v0 e1 e2 (16)       out: accept, t, U, V, front
//   33     hgd::isect_spheres, n_spheres = 1                 in: o, d, t, far_, the sphere's 3 float4 (20)  out: ref, t
//   40     hg_pack_r11g11b10                                 in: r, g, b                                    out: word
//   41     hg_pack_rgba16f                                   in: r, g, b, a                                 out: 2 words
// Returns the HIP status (0 = hipSuccess); hipErrorInvalidValue for an unknown fn or a buffer too small for n.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "hg_device.h"
#include "hg_fmath.h"
#include "hg_pack.h"

namespace {

__host__ __device__ constexpr uint32_t words_in(int fn) {
    return (fn >= 0 && fn <= 11) || fn == 20 || fn == 21 ? 1u
           : fn == 12 || fn == 13                        ? 2u
           : fn == 22 || fn == 23                        ? 4u
           : fn == 30                                    ? 12u
           : fn == 31 || fn == 32                        ? 16u
           : fn == 33                                    ? 20u
           : fn == 40                                    ? 3u
           : fn == 41                                    ? 4u
                                                         : 0u;
}
__host__ __device__ constexpr uint32_t words_out(int fn) {
    return (fn >= 0 && fn <= 13) || fn == 20 || fn == 21 || fn == 22 || fn == 30 || fn == 40 ? 1u
           : fn == 23 || fn == 33 || fn == 41                                                  ? 2u
           : fn == 31 || fn == 32                                                              ? 5u
                                                                                               : 0u;
}

__device__ float fmath_eval(int fn, float v) {
    float r, o;
    switch (fn) {
        case 0: return hg_sinf(v);
        case 1: return hg_cosf(v);
        case 2: return hg_acosf(v);
        case 3: return hg_tanf(v);
        case 4: return hg_logf(v);
        case 5: return hg_expf(v);
        case 6: return hg_roundf(v);
        case 7: return hg_rnorm(v);
        case 9: hg_sincosf(v, &r, &o); return r;
        case 10: hg_sincosf(v, &o, &r); return r;
        case 11: return hg_acosf_fused(v);
        default: return hg_asinf(v);
    }
}

template <bool kFlat>
__device__ void tri_probe(const float* e, uint32_t* o) {
    const float4 a = make_float4(e[7], e[8], e[9], e[10]), b = make_float4(e[11], e[12], e[13], e[14]);
    float t, U, V;
    bool front;
    const bool acc = hgd::tri_accept<kFlat>(hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5]), a, b, e[15], e[6], t,
                                            U, V, front);
    o[0] = acc ? 1u : 0u;
    o[1] = __float_as_uint(t);
    o[2] = __float_as_uint(U);
    o[3] = __float_as_uint(V);
    o[4] = front ? 1u : 0u;
}

__global__ __launch_bounds__(256) void hg_devprobe_kernel(int fn, const uint32_t* __restrict__ in,
                                                          uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* ui = in + i * words_in(fn);
    const float* e = reinterpret_cast<const float*>(ui);
    uint32_t* o = out + i * words_out(fn);
    if (fn >= 0 && fn <= 11) {
        o[0] = __float_as_uint(fmath_eval(fn, e[0]));
    } else if (fn == 12 || fn == 13) {
        o[0] = __float_as_uint(fn == 12 ? hg_fminf(e[0], e[1]) : hg_fmaxf(e[0], e[1]));
    } else if (fn == 20) {
        o[0] = __float_as_uint(hgd::rcp_exact(e[0]));
    } else if (fn == 21) {
        o[0] = hgd::pcg_hash(ui[0]);
    } else if (fn == 22 || fn == 23) {
        const hgd::Sampler s{ui[0], ui[1], ui[2]};
        if (fn == 22) {
            o[0] = __float_as_uint(s.get1(ui[3]));
        } else {
            float a, b;
            s.get2(ui[3], a, b);
            o[0] = __float_as_uint(a);
            o[1] = __float_as_uint(b);
        }
    } else if (fn == 30) {
        o[0] = __float_as_uint(hgd::ray_aabb(hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5]),
                                             hgd::mk(e[6], e[7], e[8]), hgd::mk(e[9], e[10], e[11])));
    } else if (fn == 31) {
        tri_probe<false>(e, o);
    } else if (fn == 32) {
        tri_probe<true>(e, o);
    } else if (fn == 33) {
        HgKernelParams kp = {};
        kp.n_spheres = 1;
        kp.far_ = e[7];
        kp.spheres = reinterpret_cast<const float4*>(e + 8);  // 80-B elements: 16-B aligned
        const hgd::Ray ray{hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5])};
        float t = e[6];
        o[0] = hgd::isect_spheres(kp, ray, t);
        o[1] = __float_as_uint(t);
    } else if (fn == 40) {
        o[0] = hg_pack_r11g11b10(e[0], e[1], e[2]);
    } else if (fn == 41) {
        hg_pack_rgba16f(e[0], e[1], e[2], e[3], o);
    }
}

}  // namespace

extern "C" int hg_devprobe(int fn, const void* in, size_t in_bytes, void* out, size_t out_bytes, int64_t n) {
    const size_t wi = words_in(fn), wo = words_out(fn);
    if (wi == 0 || wo == 0 || n < 0 || (n > 0 && (!in || !out))) return int(hipErrorInvalidValue);
    if (n > (int64_t(1) << 28)) return int(hipErrorInvalidValue);  // the grid below stays far inside 2^31 workgroups
    const size_t nb_in = size_t(n) * wi * 4, nb_out = size_t(n) * wo * 4;
    if (in_bytes < nb_in || out_bytes < nb_out) return int(hipErrorInvalidValue);
    if (n == 0) return int(hipSuccess);
    uint32_t *d_in = nullptr, *d_out = nullptr;
    hipError_t rc = hipMalloc(&d_in, nb_in);
    if (rc == hipSuccess) rc = hipMalloc(&d_out, nb_out);
    if (rc == hipSuccess) rc = hipMemcpy(d_in, in, nb_in, hipMemcpyHostToDevice);
    if (rc == hipSuccess) {
        const unsigned groups = unsigned((n + 255) / 256);  // whole workgroups; the kernel checks i < n
        hipLaunchKernelGGL(hg_devprobe_kernel, dim3(groups), dim3(256), 0, 0, fn, d_in, d_out, n);
        rc = hipGetLastError();
    }
    if (rc == hipSuccess) rc = hipDeviceSynchronize();
    if (rc == hipSuccess) rc = hipMemcpy(out, d_out, nb_out, hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return int(rc);
}
