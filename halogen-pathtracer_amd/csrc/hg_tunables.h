// hg_tunables.h — the constants and build-time tunables of the device layout, the kernels and the launch plan.
//
// Plain preprocessor constants and nothing of HIP: hg_layout.h includes this first, and hg_plan.h (the launch plan,
// compiled by its CPU test with g++) needs nothing else.  Every #ifndef default can be overridden with -D.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define HG_LEAF_BIT 0x80000000u
// Leaf refs: HG_LEAF_BIT | count << HG_LEAF_CNT_SHIFT | first triangle, for leaves of 1..15 triangles starting
// below 2^27 (no memory access to find a leaf's range); count field 0: the low bits index the leaf table instead.
#define HG_LEAF_CNT_SHIFT 27
#define HG_LEAF_INLINE_MAX 15u
#define HG_LEAF_PAYLOAD ((1u << HG_LEAF_CNT_SHIFT) - 1u)
#define HG_TILE 8
#define HG_MAX_CUBE_MIPS 16
#define HG_REGEN_MAX_BOUNCES 250  // regenerating megakernel: byte-packed bounce counters (larger: lockstep kernel)
#define HG_REGEN_MAX_CHUNK 65535  // regenerating megakernel: frames per launch and spp limit (16-bit fields)
#ifndef HG_LOCK_WAVES
#define HG_LOCK_WAVES 4  // lockstep megakernel (debug views, large-maxBounces fallback): waves/SIMD target
#endif
#ifndef HG_MEGA_WAVES
#define HG_MEGA_WAVES 6  // regenerating megakernel: waves/SIMD target
#endif
#ifndef HG_STREAM_WAVES
#define HG_STREAM_WAVES 5  // streaming kernel: waves/SIMD target (its resumable traversal state needs ~96 VGPRs)
#endif
#ifndef HG_STREAM_TMIN
#define HG_STREAM_TMIN 16  // streaming kernel: shade once at most this many lanes are still traversing (12 before the
                           // item scheduling, tools/sweeps/sweep54.txt; 16 with it, +1.1 %, tools/sweep_r02_ac.txt)
#endif
#ifndef HG_DESCENT_T
#define HG_DESCENT_T 3  // deep scenes (BLAS depth > HG_DESCENT_DEEP): leave the descent loop at <= T descending lanes
#endif
#ifndef HG_STREAM_TMIN_DEEP
#define HG_STREAM_TMIN_DEEP 20  // ... for a deep BLAS (C3 +0.6 %, C3F +1.0 %, strict 1-frame +1.5 %; C2 keeps 16: -1.2 %;
#endif                          // tools/sweeps/sweep_r04_results.txt)
#ifndef HG_STREAM_RESHADE_DEEP
#define HG_STREAM_RESHADE_DEEP 24
#endif
#ifndef HG_STREAM_RESHADE
#define HG_STREAM_RESHADE 16  // streaming kernel: repeat the shading pass while at least this many lanes need it
#endif
#ifndef HG_STREAM_DESCENT_T
#define HG_STREAM_DESCENT_T 12  // the same for the streaming kernel (tools/sweeps/sweep42.txt; 8 with the unsplit launch,
                                // sweep74; 12 with the in-place item scheduling, +2.4 %, tools/sweep_r02_al.txt)
#endif
#ifndef HG_DESCENT_DEEP
#define HG_DESCENT_DEEP 16
#endif
// Wave priorities (s_setprio): the streaming kernel's waves run at 1 while traversing (traversal waits on memory: its
// waves issue first) and 0 while shading (C3 2,097 -> 2,111, tools/sweeps/sweep67-68.txt); the regenerating kernel's
// at 1 during get_ray_intersection (C2 +1 %, C5 +2 %, tools/sweeps/sweep69.txt).
#define HG_TRAVERSE_PRIO 1
#ifndef HG_TILE_ORDER
#define HG_TILE_ORDER 1  // regen / stream kernels: dispatch tiles in descending cost of the previous launch (hg_order.hip)
#endif
#ifndef HG_ORDER_MIN_FRAMES
#define HG_ORDER_MIN_FRAMES 16  // hg_render re-sorts the tile order once at least this many frames of costs were recorded
#endif                          // since the last sort (64-frame launches: every launch; 1-frame launches: every 16th)
// Every mesh's world->local matrix and header (80 B) in the wave's LDS when they fit (hg_wave_lds_plan): the per-lane
// mesh switch reads LDS, not global memory
#define HG_MESH_LDS_F4 5  // float4 per cached mesh record: w2l columns 0-3, header (root, tri offset, material, cull)
// The material table in the wave's LDS too (hg_layout.h hg_wave_lds_plan; 0: that kernel reads it from global memory)
#ifndef HG_MAT_LDS_STREAM
#define HG_MAT_LDS_STREAM 1
#endif
#ifndef HG_MAT_LDS_REGEN
#define HG_MAT_LDS_REGEN 1
#endif
// Bytes of LDS per one-wave workgroup that still keep 20 waves (5 per SIMD) on a CU.  Measured, not derived from
// 160 KiB / 20: 7,424 and 7,472 B run at full occupancy, 7,936 / 7,984 / 8,192 B lose 8-12 % (one wave fewer per
// CU; tools/sweep_r02_h.txt); 7,680 is the largest multiple of 512 below the first failing size.
#ifndef HG_WAVE_LDS_BUDGET
#define HG_WAVE_LDS_BUDGET 7680
#endif
#ifndef HG_REGEN_LDS_BUDGET
// The same for the regenerating kernel at its 6 waves per SIMD (24 per CU): 163,840 / 24 = 6,826, less the same
// reserve; 0 keeps its mesh records in global memory
#define HG_REGEN_LDS_BUDGET 6144
#endif
#ifndef HG_COALESCE
#define HG_COALESCE 32  // default HG_OPT_COALESCE: frames of consecutive hg_render calls held for one launch
#endif
#ifndef HG_TRACE_LANES
#define HG_TRACE_LANES 12  // trace streams of the render pipeline (hg_ctx.h): chunks traced in turn on them, blended in
#endif                    // order.  1-frame launches, C3, all waves per launch: 2 streams 1,970, 3: 2,143, 4: 2,265,
                          // 6: 2,242, 8: 2,302 Mpaths/s; with HG_QUEUE_WAVES_DIV 6 and 8 streams 2,745, with 8 and 10 / 12
                          // streams 2,808 / 2,790 (tools/sweeps/sweep_r03_u/v/y/z/aa; streams 3+ on hardware queues of
                          // their own).  Round 4 (queue heads reset in-kernel, small sort), streams / divisor 8/6
                          // 2,779-2,793, 12/8 2,874-2,878, 12/12 2,748-2,753, 16/12 2,893-2,908, 16/16 2,800-2,808
                          // (tools/sweeps/sweep_r04_a.txt): 12/8, +3 % for four more queues per context
#ifndef HG_TRACE_LANES_BIG
#define HG_TRACE_LANES_BIG 2  // of those, the ones chunks of more than HG_QUEUE_MAX_FRAMES frames take in turn (a third
#endif                        // 64-frame launch beside two others: C3 -1.5 %)
// Trace streams: HIP spreads plain streams over a pool of GPU_MAX_HW_QUEUES (default 4) hardware queues shared by every
// stream of the process, and two streams on one queue run their launches one after the other (a third plain trace
// stream cost 1-frame launches 16 %: 1,663 vs 1,970).  A stream created with a CU mask gets a hardware queue of its
// own: the first HG_TRACE_LANES_BIG trace streams are plain and non-blocking, the others (and the render server's and
// the side copy stream) carry an all-CU mask (create_masked_stream, hg_runtime.hip).
#ifndef HG_QUEUE_WAVES_DIV
#define HG_QUEUE_WAVES_DIV 8  // queue launches beside >= 2 other traces in flight: at most this many times fewer persistent
#endif                        // waves than resident slots (hg_render; C3 1-frame launches, 8 streams: 1 2,265 -> 6 2,745;
                              // 12 streams: 8 2,874-2,878, 12 2,748-2,753)
#ifndef HG_READBACK_SIDE
#define HG_READBACK_SIDE 0  // default HG_OPT_READBACK_STREAM (display copies on a side stream)
#endif
#ifndef HG_WAVE_UNITS_MAX
#define HG_WAVE_UNITS_MAX 1     // streaming launches without the queue: at most this many tiles per wave (automatic)
#endif
#ifndef HG_WAVE_UNITS_ROUNDS
#define HG_WAVE_UNITS_ROUNDS 3  // ... while the launch keeps at least this many waves per resident wave slot
#endif
#ifndef HG_LANE_PICK
#define HG_LANE_PICK 1  // default HG_OPT_LANE_PICK (display one frame behind +5 %, strict -0.5 %: sweep_r04_depth)
#endif
#define HG_WAVE_UNITS_LIMIT 4  // HG_OPT_WAVE_UNITS range (the units' tiles sit in scalar registers)
#ifndef HG_QUEUE_FILL
// default HG_OPT_QUEUE_FILL: streaming launches of more than HG_QUEUE_MAX_FRAMES frames whose tiles give fewer rounds of
// the GPU's wave slots than this run the queue form (a rank's share at N = 8, 1080p: 0.79 rounds).  With about 24
// (tile, frame chunk) units per wave slot the queue form costs 6 % against per-tile waves at N = 1 (C3: 3,288 vs 3,491
// Mpaths/s); emulated shares, queue vs per-tile: N = 2 3,229 vs 3,366, N = 4 3,114 vs 3,122, N = 8 2,937 vs 2,803
#define HG_QUEUE_FILL 1
#endif
#define HG_QUEUE_FILL_UNITS 24  // queue-form shares: (tile, frame chunk) units per wave slot
#ifndef HG_SHARE_HOLD_ROUNDS
// A rank's share of the image (hg_set_tiling, N > 1) holds consecutive hg_render calls (HG_OPT_COALESCE > 1) until the
// held launch has this many rounds of the GPU's wave slots in 64-frame tile waves, as one context's 64-frame launch of
// the whole 1080p image has (32,400 tiles / 5,120 slots): 8 calls of 64 frames at N = 8, 4 at N = 4, 2 at N = 2.
// Emulated strong shares of C3 (tools/gpu_strong_coalesce.sh): N = 8 3,000 -> 3,526 Mpaths/s, N = 4 3,128 -> 3,465.
#define HG_SHARE_HOLD_ROUNDS 6
#endif
#define HG_SHARE_HOLD_MAX 1024  // frames: the most a share holds (its frame colours: 2 trace streams x 4 GiB at most)
#ifndef HG_QUEUE_MAX_FRAMES
#define HG_QUEUE_MAX_FRAMES 8  // streaming launches of at most this many frames run the persistent work-queue form (kQueue)
#endif
// The queue of a kQueue launch: 8 unit heads, 128 B apart (words 32 h), then the count of waves that have left (its own
// 128-B line): the last wave out zeroes them for the next launch (the runtime zeroes the buffer once, at allocation)
#define HG_QUEUE_DONE_WORD 256u
#define HG_QUEUE_BYTES (9u * 128u)
// Render server control words (kp.queue of a server launch, HG_SV_CTL_BYTES, zeroed at each server start), each on a
// 128-B line of its own: the 8 unit heads (as above), then HG_SV_MIRRORS copies of the device mirror of the host's post
// word (u64, raised by atomic max by whichever wave read the host word; an idle
// wave reads copy blockIdx.x % HG_SV_MIRRORS: the polling of thousands of idle waves spread over as many lines), one
// host-poll ticket per XCD (blockIdx.x % 8), the count of waves that left (read by the gates: a frame whose count is
// short once every wave has left is lost), and the closing word (0 open, 1 closing: the one wave that won it runs the
// close handshake, hg_server.h sv_close)
#define HG_SV_MIRRORS 16u
#define HG_SV_MIRROR_WORD 288u
#define HG_SV_TICKET_WORD (HG_SV_MIRROR_WORD + 32u * HG_SV_MIRRORS)
#define HG_SV_EXIT_WORD (HG_SV_TICKET_WORD + 32u * 8u)  // waves of the server that left | grid << 32
#define HG_SV_CLOSE_WORD (HG_SV_EXIT_WORD + 32u)
#ifndef HG_SV_DIAG_TIMES
#define HG_SV_DIAG_TIMES 0  // analysis builds: per frame (< 256) the device time of its first claim and its last count
#endif
#define HG_SV_DIAG_WORD (HG_SV_CLOSE_WORD + 32u)
#define HG_SV_CTL_BYTES ((HG_SV_DIAG_WORD + (HG_SV_DIAG_TIMES ? 1024u : 0u)) * 4u)
#ifndef HG_SV_POLL_TICKS
#define HG_SV_POLL_TICKS 200u  // 2 us between reads of the host word over PCIe, per XCD
#endif
#ifndef HG_SV_SLEEP_LONG  // an idle server wave's wait between polls: HG_SV_SPIN_SHORT spins of s_sleep SHORT, then LONG
#define HG_SV_SLEEP_SHORT 8
#define HG_SV_SLEEP_LONG 127
#define HG_SV_SPIN_SHORT 16u
#define HG_SV_POLL_EVERY 4u  // an idle wave reads the host word (if its XCD's ticket is free) every this many spins
#endif
#ifndef HG_SV_WAVES
#define HG_SV_WAVES 5  // the render server's persistent waves per SIMD (hg_render.hip server_start)
#endif
#ifndef HG_SV_TILE_RUN
// The render server's XCD heads take runs of this many consecutive tiles (hg_server.h sv_pull, hg_items.h hg_sv_run_place): head h (the XCD whose
// waves pull it first) runs h, h + 8, ..., so a CU's waves pull neighbouring tiles and the heads still interleave
// finely over the frame (one contiguous band per head lost 1-3 %: per-XCD balance).  C3, server forced, one box, two
// rounds (tools/sweeps/sweep_r06_server_runs.txt), runs of 1 / 4 / 8 / 16: strict 3,169-3,176 / 3,183-3,194 /
// 3,187-3,193 / 3,181-3,183, display at once 2,643-2,714 / 2,706-2,716 / 2,724-2,735 / 2,701, one behind
// 2,811-2,847 / 2,837-2,868 / 2,879-2,881 / 2,789-2,862 Mpaths/s.
#define HG_SV_TILE_RUN 8u
#endif
#ifndef HG_SV_CLAIM
#define HG_SV_CLAIM 4u  // units per claim of a server wave far behind the posted units (the rest held for its next pulls)
#endif
#ifndef HG_SV_RING
#define HG_SV_RING 16  // colour ring slots of the render server (frames traced ahead of their blend), at most
#endif
#define HG_SV_STOP (1ull << 32)  // the post word's stop flag (posted frames in the low 32 bits)
// The host words of a server (pinned, coherent; u64 each): the post word (frames posted | HG_SV_STOP), the lost-frame
// word (a gate that gave up: HG_SV_LOST | the accumulator epoch of its frame), the closing word (raised by the wave
// that closes the server, before it reads the post word) and the close word (the post word as that wave read it, with
// HG_SV_STOP, | HG_SV_CLOSED once written)
#define HG_SV_HOST_POST 0
#define HG_SV_HOST_LOST 1
#define HG_SV_HOST_CLOSING 2
#define HG_SV_HOST_CLOSED 3
#define HG_SV_CLOSED (1ull << 33)
#define HG_SV_LOST (1ull << 32)
#ifndef HG_SV_AHEAD
#define HG_SV_AHEAD 4  // default HG_OPT_SERVER_AHEAD: frames the render server traces ahead of the host's calls (4 and 8 measured equal)
#endif
#define HG_SV_IDLE_US 200000  // default HG_OPT_SERVER_IDLE_US: the server closes after this long with nothing posted
#ifndef HG_REGEN_ITEMS
#define HG_REGEN_ITEMS 1  // regenerating kernel: (pixel, frame) item scheduling (0: the A/B build of make noitems)
#endif
#ifndef HG_STREAM_MIN_MESHES
#define HG_STREAM_MIN_MESHES 4  // HG_KERNEL_AUTO: the streaming kernel from this many meshes on (or for a deep BLAS)
#endif
#ifndef HG_STREAM_LB
#define HG_STREAM_LB 64  // regen / stream kernels: __launch_bounds__ max threads = their one-wave workgroup (256: scratch 32 B vs 24-28 B)
#endif
#ifndef HG_CHECK_EXEC
#define HG_CHECK_EXEC 0  // debug builds: leaf_dist checks its all-lanes-active precondition (hg_dev_isect.h)
#endif
#ifndef HG_MEGA_LDS_STACK
#define HG_MEGA_LDS_STACK 16  // megakernels: traversal stack entries per lane kept in LDS (deeper ones spill)
#endif
#ifndef HG_STREAM_LDS_STACK
#define HG_STREAM_LDS_STACK 12  // the same for the streaming kernel (12 and 14 measured equal, 10 equal to 16 without the
                                // mesh records in LDS; 12 leaves LDS room for 16 meshes, HG_WAVE_LDS_BUDGET)
#endif
#ifndef HG_SKIN_LDS_BONES
#define HG_SKIN_LDS_BONES 256  // skin kernel (hg_deform.hip): a palette of at most this many bones sits in the workgroup's
                               // LDS (12 KiB of 48-B bones beside 6 KiB of staging); a larger one is read from global memory
#endif

constexpr size_t kFrameColorCap = size_t(4) << 30;  // frame-parallel colour buffer cap (bytes)
