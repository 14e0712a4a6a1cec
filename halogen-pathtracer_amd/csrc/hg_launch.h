// hg_launch.h — the kernel launchers and size helpers that one translation unit of libhalogen_hip.so defines and
// another calls.  Definers and callers both include it, so a changed signature fails to compile instead of to link.
// (The launchers and size helpers of hg_query.hip and hg_denoise.hip, and hg_mega_lds_bytes, are called from their own
// files only and are not declared here.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "hg_layout.h"

// hg_mega.hip (the trace kernels)
hipError_t hg_launch_mega(const HgKernelParams& kp, int block, bool counters, hipStream_t stream);
hipError_t hg_launch_mega_regen(const HgKernelParams& kp, int block, bool counters, hipStream_t stream);
hipError_t hg_launch_mega_stream(const HgKernelParams& kp, int block, bool counters, hipStream_t stream,
                                 bool server = false);

// hg_blend.hip
hipError_t hg_launch_blend_frames(const HgKernelParams& kp, const uint32_t* lost, hipStream_t stream);
hipError_t hg_launch_server_frame(float4* acc, const float4* colors, uint32_t n_slots, int32_t frame_count,
                                  const uint32_t* done, uint32_t target, uint64_t timeout_ticks,
                                  const unsigned long long* exitw, uint32_t* lost, unsigned long long* err,
                                  uint32_t epoch, hipStream_t stream);

// hg_order.hip
hipError_t hg_launch_order_tiles(unsigned long long* cost, uint32_t* order, uint32_t n, void* scratch,
                                 unsigned long long* faults, hipStream_t stream);
size_t hg_order_scratch_bytes(uint32_t n);
// HG_CHECK_EXEC builds (nothing otherwise): words that every use leaves zeroed must read zero when the next use starts
void hg_launch_check_zeroed(const uint32_t* p, uint32_t n, unsigned long long* faults, hipStream_t stream);

// hg_selftest.hip
int64_t hg_selftest_rcp_all(int64_t* tested);
