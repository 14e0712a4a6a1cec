// hg_dev_sampler.h — the hashes, the closed-form Owen-scrambled Sobol points and the Sampler (part of hg_device.h).
#pragma once
#include <hip/hip_runtime.h>

#include "hg_fmath.h"

namespace hgd {

// ---------------------------------------------------------------------------------------------------
// Sampler (HalogenRandom.hlsl)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pcg_hash(uint32_t v) {  // u32_hash :110-115
    uint32_t state = v * 747796405u + 2891336453u;
    uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
__device__ __forceinline__ uint32_t hash_combine(uint32_t seed, uint32_t v) {  // :131-133
    return seed ^ (v + (seed << 6) + (seed >> 2));
}
// the Laine–Karras-style body of owen_scramble (:154-158), on the already bit-reversed value
__device__ __forceinline__ uint32_t lk_body(uint32_t x, uint32_t seed) {
    x ^= x * 0x3d20adeau;
    x += seed;
    x *= (seed >> 16) | 1u;
    x ^= x * 0x05526c56u;
    x ^= x * 0x53a22864u;
    return x;
}
__device__ __forceinline__ uint32_t brev(uint32_t x) { return __builtin_bitreverse32(x); }
// owen_scramble(v, s) = brev(lk(brev(v), s))
__device__ __forceinline__ uint32_t owen(uint32_t v, uint32_t s) { return brev(lk_body(brev(v), s)); }
// Sobol dimension 1 (Pascal matrix mod 2): bit p (MSB-first) of sobol(i,1) = XOR over set bits k of i
// with k ⊇ p  ->  superset-XOR transform of i, then bit-reversed.
__device__ __forceinline__ uint32_t superset_xor(uint32_t z) {
    z ^= (z >> 1) & 0x55555555u;
    z ^= (z >> 2) & 0x33333333u;
    z ^= (z >> 4) & 0x0F0F0F0Fu;
    z ^= (z >> 8) & 0x00FF00FFu;
    z ^= (z >> 16) & 0x0000FFFFu;
    return z;
}
constexpr float kInv2_32 = 4294967296.0f;

struct Sampler {
    uint32_t frame;   // Sobol index (FrameCount)
    uint32_t pixel;   // pixelID = u32_hash(x + y*W)
    uint32_t offset;  // SobolDimensionOffset
    // float_owen_scrambled_sobol (:252-259): owen(sobol(i,0), pcg(seed)) = brev(lk(i, pcg(seed)))
    __device__ __forceinline__ float get1(uint32_t id) const {
        uint32_t seed = pixel ^ pcg_hash(offset + id);
        return float(brev(lk_body(frame, pcg_hash(seed)))) / kInv2_32;
    }
    // float2_owen_scrambled_sobol (:261-268, :215-228)
    __device__ __forceinline__ void get2(uint32_t id, float& a, float& b) const {
        uint32_t seed = pixel ^ pcg_hash(offset + id);
        uint32_t sh = owen(frame, seed);  // shuffled index
        a = float(brev(lk_body(sh, hash_combine(seed, 0u)))) / kInv2_32;
        b = float(brev(lk_body(superset_xor(sh), hash_combine(seed, 1u)))) / kInv2_32;
    }
};

constexpr uint32_t ID_FOCAL = 0, ID_JITTER = 1, ID_ROUGH = 2, ID_PROPERTY = 3, ID_RR = 4, BOUNCE_INC = 5;
#define HLSL_PI (180.0f * HG_DEG2RAD)

}  // namespace hgd
