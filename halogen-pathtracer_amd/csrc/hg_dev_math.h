// hg_dev_math.h — float3 arithmetic in the reference's evaluation order and the exact reciprocal (part of hg_device.h).
// Every other hg_dev_*.h header includes this one, so each of them carries the contraction pragma when compiled alone.
#pragma once
#include <hip/hip_runtime.h>

#include "hg_fmath.h"

#pragma clang fp contract(off)

namespace hgd {

// ---------------------------------------------------------------------------------------------------
// float3 helpers with the reference's evaluation order (no FMA)
// ---------------------------------------------------------------------------------------------------
struct f3 {
    float x, y, z;
};
__device__ __forceinline__ f3 mk(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator*(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ f3 operator-(f3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 cross(f3 a, f3 b) {
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ float len(f3 a) { return __builtin_sqrtf(dot(a, a)); }
// normalize = v * (1/sqrt(dot(v,v))) (hg_fmath.h hg_rnorm)
__device__ __forceinline__ f3 normalize(f3 a) { return a * hg_rnorm(dot(a, a)); }
__device__ __forceinline__ f3 lerp(f3 a, f3 b, float s) { return a + (b - a) * s; }
__device__ __forceinline__ f3 xyz(float4 v) { return mk(v.x, v.y, v.z); }

// mul(M, float4(v, w)), M given row-major in m[r*4+c] (rows 0..2)
__device__ __forceinline__ f3 xform(const float* m, f3 v, float w) {
    return mk(((m[0] * v.x + m[1] * v.y) + m[2] * v.z) + m[3] * w,
              ((m[4] * v.x + m[5] * v.y) + m[6] * v.z) + m[7] * w,
              ((m[8] * v.x + m[9] * v.y) + m[10] * v.z) + m[11] * w);
}

// 1/x, correctly rounded (the reference's `1 / det`, `1 / dir` in IEEE fp32).  With HG_FAST_RCP the hardware
// reciprocal (<= 1 ulp) is refined by one FMA Newton step, correctly rounded for every x whose exponent keeps x
// and 1/x normal (the same three operations are checked for all 2^32 inputs by hg_selftest, tests/test_gpu_selftest.py);
// zeros, denormals, huge values, infinities and NaNs take the IEEE division.  This function itself, fallback exponents
// (0, 1, 253-255) included, is run against float32(1) / x by tests/test_gpu_device_units.py
// (test_gpu_rcp_exact_is_ieee_division, through csrc/hg_devprobe.hip).
__device__ __forceinline__ float rcp_exact(float x) {
#if HG_FAST_RCP
    const uint32_t ex = (__float_as_uint(x) >> 23) & 0xFFu;
    if (__builtin_expect(ex - 2u <= 250u, 1)) {
        const float r = __builtin_amdgcn_rcpf(x);
        const float e = __builtin_fmaf(-x, r, 1.0f);
        return __builtin_fmaf(e, r, r);
    }
#endif
    return 1.0f / x;
}

}  // namespace hgd
