// hg_dev_wave.h — wave64 primitives: the wave clock, scalar loads of uncached words, ballots, DPP scans, the LDS
// exchange fence and the lane permute (part of hg_device.h).
#pragma once
#include <hip/hip_runtime.h>

namespace hgd {

// Wave clock (s_memtime) for the counting instantiations' phase split; volatile + memory clobber keep the
// compiler from moving it across the code it brackets.
__device__ __forceinline__ uint64_t wave_clock() {
    uint64_t t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    return t;
}
// A word of uncached device memory read by a scalar load that bypasses the scalar cache (glc); p wave-uniform (a kernel
// argument).  The blends read the context's lost word so (hg_server_gate: once a server frame was lost, every later
// blend into the accumulator is skipped until a clear or a checkpoint load resets the word), one load per workgroup;
// the render server's waves and its gate poll their control words so.  The runtime allocates those words uncached (no
// L2 holds them either), and the polling of idle waves stays off the CU's vector-memory pipe, whose texture units
// return data in order: a vector poll of a contended coherent word held up the loads of the busy waves beside it (with
// the idle waves of a frame's end polling, a posted frame took several times its trace time).
__device__ __forceinline__ uint32_t sload_u32(const uint32_t* p) {
    uint32_t v;
    asm volatile("s_load_dword %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}
__device__ __forceinline__ unsigned long long sv_sload(const unsigned long long* p) {
    unsigned long long v;
    asm volatile("s_load_dwordx2 %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}
// The same for a 32-bit word whose address the compiler takes for divergent (lane 0's branch: a value read from LDS
// counts as divergent), made wave-uniform.  readfirstlane returns int: each half through uint32_t, or a low half
// >= 2^31 would sign-extend over the high one.
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(a >> 32)));
    const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(a)));
    return sload_u32(reinterpret_cast<const uint32_t*>((uint64_t(hi) << 32) | lo));
}
// 64-lane ballot of a bool straight from the compare mask (the HIP __ballot(int) materialises the predicate in a
// VGPR and compares it again)
__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t wave_count(bool p) { return uint32_t(__builtin_popcountll(wave_ballot(p))); }
// 1 in exactly one active lane (the lowest): summed over lanes, counts the wave-level executions of a code point
__device__ __forceinline__ uint32_t wave_once() {
    return __lane_id() == uint32_t(__builtin_ctzll(__ballot(1))) ? 1u : 0u;
}

// ---- wave-wide inclusive scans over 64 lanes (DPP row shifts + row broadcasts, the GFX9 form); every lane of the
// wave must be active
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t dpp_(uint32_t x) {
    return uint32_t(__builtin_amdgcn_update_dpp(0, int(x), kCtrl, kRowMask, 0xF, false));  // invalid source: 0
}
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t x) {
    x += dpp_<0x111, 0xF>(x);  // row_shr:1
    x += dpp_<0x112, 0xF>(x);  // row_shr:2
    x += dpp_<0x114, 0xF>(x);  // row_shr:4
    x += dpp_<0x118, 0xF>(x);  // row_shr:8
    x += dpp_<0x142, 0xA>(x);  // row_bcast:15 into rows 1 and 3
    x += dpp_<0x143, 0xC>(x);  // row_bcast:31 into rows 2 and 3
    return x;
}
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x) {
    x = max(x, dpp_<0x111, 0xF>(x));
    x = max(x, dpp_<0x112, 0xF>(x));
    x = max(x, dpp_<0x114, 0xF>(x));
    x = max(x, dpp_<0x118, 0xF>(x));
    x = max(x, dpp_<0x142, 0xA>(x));
    x = max(x, dpp_<0x143, 0xC>(x));
    return x;
}
// Lanes of one wave exchanging data through LDS: the fences make the other lanes' LDS writes visible to this lane's
// later reads (and keep the compiler from forwarding its own stores across them).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float bperm_f(int addr, float x) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(x)));
}

// wave64 sum (all 64 lanes active at the call site)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace hgd
