// hg_blend.hip — the frame blends: every trace launch of the pipeline writes each frame's colour to frame_color and
// these kernels blend them into the accumulator in frame order afterwards; and the render server's per-frame gate and
// blend on the context stream.  A translation unit of its own: the megakernels of hg_mega.hip compile to what they
// compile to without it.
#include <hip/hip_runtime.h>

#include "hg_dev_records.h"
#include "hg_dev_wave.h"
#include "hg_launch.h"

using namespace hgd;

// Frame-parallel epilogue: acc = acc*(1-w) + c_f*w for f in frame order (AccumulationShader.shader:33), exactly the
// per-frame blend the kernels do themselves when they blend in place.
// Over the [slot][frame] colour layout each wave owns 64 slots (a tile) and moves their colours 8 frames at
// a time through LDS, so every load instruction reads whole 128-B lines (8 lanes per line: one slot's 8 frames)
// instead of 64 lanes on 64 lines; then each lane blends its slot's 8 frames in frame order.
__global__ __launch_bounds__(256) void hg_blend_frames_sm(float4* __restrict__ acc, const float4* __restrict__ colors,
                                                          uint32_t n_slots, int32_t n_frames, int32_t first_frame,
                                                          int32_t accumulate, const uint32_t* lost) {
    if (sload_u32(lost)) return;
    constexpr uint32_t kRow = 9;  // float4 per slot row: 8 frames + 1 pad (spreads the lanes' rows over the banks)
    __shared__ float4 stage[4][64 * kRow];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t slot0 = (blockIdx.x * 4u + w) * 64u;
    if (slot0 >= n_slots) return;  // whole wave: n_slots is a multiple of 64
    const uint32_t nf = uint32_t(n_frames);
    float4* st = stage[w];
    float4 a = acc[slot0 + lane];
    for (uint32_t f0 = 0; f0 < nf; f0 += 8u) {
#pragma unroll
        for (uint32_t r = 0; r < 8u; ++r) {
            const uint32_t j = lane + 64u * r, s = j >> 3, ff = j & 7u;
            if (f0 + ff < nf) st[s * kRow + ff] = fc_load(colors + size_t(slot0 + s) * nf + f0 + ff);
        }
        wave_lds_sync();
        const uint32_t fe = nf - f0 < 8u ? nf - f0 : 8u;
        for (uint32_t ff = 0; ff < fe; ++ff) {
            const float4 c = st[lane * kRow + ff];
            a = accumulate ? blend_frame(a, xyz(c), float(uint32_t(first_frame) + f0 + ff)) : frame_alone(xyz(c));
        }
        wave_lds_sync();
    }
    acc[slot0 + lane] = a;
}

// The blend of a launch of few frames (at most HG_QUEUE_MAX_FRAMES): one thread per slot, no LDS, 64-thread groups and
// few registers.  A 1-frame launch's blend runs while the next launch's persistent trace waves hold the CUs' wave slots
// and most of their LDS: this one fits beside them (the LDS-staged hg_blend_frames_sm, 36 KB per group, waited for
// the trace to wind down: 0.7 ms per 1-frame blend on C3).  Same operations in the same order.
__global__ __launch_bounds__(64) void hg_blend_frames_lean(float4* __restrict__ acc, const float4* __restrict__ colors,
                                                           uint32_t n_slots, int32_t n_frames, int32_t first_frame,
                                                           int32_t accumulate, const uint32_t* lost) {
    if (sload_u32(lost)) return;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_slots) return;
    float4 a = acc[i];
    for (int32_t f = 0; f < n_frames; ++f) {
        const float4 c = fc_load(colors + fc_slot_frame(i, uint32_t(f), uint32_t(n_frames)));
        a = accumulate ? blend_frame(a, xyz(c), float(uint32_t(first_frame + f))) : frame_alone(xyz(c));
    }
    acc[i] = a;
}

hipError_t hg_launch_blend_frames(const HgKernelParams& kp, const uint32_t* lost, hipStream_t stream) {
    const uint32_t n_slots = uint32_t(kp.n_local_tiles) * 64u;
    if (n_slots == 0) return hipSuccess;
    if (kp.n_frames <= HG_QUEUE_MAX_FRAMES) {
        hipLaunchKernelGGL(hg_blend_frames_lean, dim3((n_slots + 63) / 64), dim3(64), 0, stream, kp.acc, kp.frame_color,
                           n_slots, kp.n_frames, kp.first_frame, kp.accumulate, lost);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(hg_blend_frames_sm, dim3((n_slots + 255) / 256), dim3(256), 0, stream, kp.acc,
                       kp.frame_color, n_slots, kp.n_frames, kp.first_frame, kp.accumulate, lost);
    return hipGetLastError();
}

// The render server's per-frame work on the context stream (hg_render.hip server_commit): the gate waits until the
// frame's ring-slot count reaches `target` (one wave; agent-scope polls with a sleep).  It gives up when every wave of
// the server has left with the count still short (the frame can no longer complete), or after `timeout_ticks`: then
// the frame is lost, and the gate raises the context's lost word (device memory: every later blend into the
// accumulator is skipped, until a clear or a checkpoint load resets it) and the host's lost-frame word (HG_SV_LOST |
// the accumulator epoch of the frame: the host marks the accumulator invalid).  The blend reads the frame's colours from
// the uncached ring and blends them into the accumulator: acc*(1-w) + c*w, w = 1/FrameCount
// (AccumulationShader.shader:33), the same operations as every other blend.  Both fit beside the server's waves
// (64-thread groups, no LDS, few registers).
__global__ __launch_bounds__(64) void hg_server_gate(const uint32_t* __restrict__ done, uint32_t target,
                                                     uint64_t timeout_ticks, const unsigned long long* exitw,
                                                     uint32_t* lost, unsigned long long* __restrict__ err,
                                                     uint32_t epoch) {
    // (the whole wave polls with scalar loads of uncached words: nothing on the vector-memory pipe of the CU it shares
    // with the server's waves; sv_sload)
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    for (uint32_t spin = 0;; ++spin) {
        if (sload_u32(done) >= target) return;
        bool gone = false;
        if ((spin & 15u) == 15u) {  // every server wave has left: a count still short now stays short
            const unsigned long long w = sv_sload(exitw);
            gone = (w >> 32) != 0ull && uint32_t(w) == uint32_t(w >> 32) && sload_u32(done) < target;
        }
        if (gone || __builtin_amdgcn_s_memrealtime() - t0 > timeout_ticks) break;
        if (spin < 256u) __builtin_amdgcn_s_sleep(1);
        else __builtin_amdgcn_s_sleep(8);
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(lost, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(err, HG_SV_LOST | epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
__global__ __launch_bounds__(64) void hg_server_blend(float4* __restrict__ acc, const float4* __restrict__ colors,
                                                      uint32_t n_slots, int32_t frame_count, const uint32_t* lost) {
    if (sload_u32(lost)) return;  // a frame before this one was lost: the accumulator stays as it was
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_slots) return;
    const float4 c = fc_load(colors + i);  // (uncached memory: the server's stores, whichever XCD made them)
    acc[i] = blend_frame(acc[i], xyz(c), float(uint32_t(frame_count)));
}
hipError_t hg_launch_server_frame(float4* acc, const float4* colors, uint32_t n_slots, int32_t frame_count,
                                  const uint32_t* done, uint32_t target, uint64_t timeout_ticks,
                                  const unsigned long long* exitw, uint32_t* lost, unsigned long long* err,
                                  uint32_t epoch, hipStream_t stream) {
    hipLaunchKernelGGL(hg_server_gate, dim3(1), dim3(64), 0, stream, done, target, timeout_ticks, exitw, lost, err,
                       epoch);
    if (n_slots)
        hipLaunchKernelGGL(hg_server_blend, dim3((n_slots + 63) / 64), dim3(64), 0, stream, acc, colors, n_slots,
                           frame_count, static_cast<const uint32_t*>(lost));
    return hipGetLastError();
}
