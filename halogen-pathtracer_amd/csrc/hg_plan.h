// hg_plan.h — the launch plan of hg_render: every decision about the shape of a launch, as plain functions of plain
// integers.  No HIP, no hg_ctx, no streams, no allocation: hg_render.hip fills an HgPlanIn from the context, asks
// here, and issues the HIP calls; tests/test_launch_plan.py compiles this header with g++ and checks the arithmetic
// (every plan renders the same image, so a wrong plan shows only as a slower one: no rendering test can see it).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "halogen_abi.h"
#include "hg_tunables.h"

struct HgPlanIn {
    // device, target, scene
    int32_t n_cu, n_local_tiles, W, H;
    uint32_t stack_depth;
    int32_t n_meshes;
    // options (hg_ctx.h)
    int32_t kernel, block, frame_split, wave_units, queue_fill, descent_t, tile_order_on, coalesce, n_ranks;
    // uniforms
    uint32_t debug_mode, max_bounces, spp;
    int32_t n_frames;  // the call's
};

// Wave slots of the GPU for a kernel that runs `waves` waves per SIMD (HG_STREAM_WAVES, HG_MEGA_WAVES, the server's)
inline int64_t hg_wave_slots(int32_t n_cu, int waves) { return int64_t(n_cu) * 4 * waves; }

// deep scenes (BLAS depth > HG_DESCENT_DEEP) take the relaxed descent and the streaming kernel's deep thresholds
inline bool hg_deep_blas(uint32_t stack_depth) { return stack_depth > HG_DESCENT_DEEP + 2; }

// relaxed descent threshold: HG_DESCENT_T for the regen / lockstep kernels, HG_STREAM_DESCENT_T for the streaming one
inline uint32_t hg_descent_t(int32_t option, uint32_t stack_depth, int32_t kernel) {
    return option >= 0                       ? uint32_t(option)
           : !hg_deep_blas(stack_depth)      ? 0u
           : kernel == HG_KERNEL_MEGA_STREAM ? uint32_t(HG_STREAM_DESCENT_T)
                                             : uint32_t(HG_DESCENT_T);
}

// A streaming launch of `frames` frames gives fewer than queue_fill rounds of the GPU's wave slots (HG_OPT_QUEUE_FILL).
// Asked twice: by the call's frame split with the call's frames and by each chunk's queue decision with the chunk's.
inline bool hg_queue_fill(const HgPlanIn& in, int64_t frames) {
    return in.queue_fill > 0 &&
           int64_t(in.n_local_tiles) * frames < int64_t(in.queue_fill) * hg_wave_slots(in.n_cu, HG_STREAM_WAVES) * 64;
}

struct HgCallPlan {
    int status;           // HG_OK, or HG_E_UNSUPPORTED: the target has more work units than one dispatch takes
    int32_t kernel;       // the variant that runs, HG_KERNEL_AUTO resolved (before the lockstep fallback)
    uint64_t last_kernel;  // hg_counters.last_kernel
    bool regen;           // the regenerating or the streaming kernel (else the lockstep one)
    bool stream_k, items_k, pipelined, ordered;
    uint32_t stream_deep, descent_t;
    int block;            // workgroup size
    int split;            // frame split of the call (a chunk takes min(split, its frames))
    int chunk_max;        // frames per launch at most
    int grid;             // workgroups
    uint32_t spill_stride;
    size_t per_frame;     // bytes of one frame's colours
    size_t spill_bytes;
    // trace streams: the streams beyond HG_TRACE_LANES_BIG are needed (the call has a chunk of at most
    // HG_QUEUE_MAX_FRAMES frames: the first, the last, or all of them), and the frames each class of stream holds
    bool short_chunks;
    int big_frames, short_frames;
};

inline HgCallPlan hg_plan_call(const HgPlanIn& in) {
    HgCallPlan P{};
    const int32_t n_frames = in.n_frames;
    // HG_KERNEL_AUTO: the streaming kernel for deep BLAS or many meshes, where traversals are long or uneven and its
    // resumable traversal lets a lane move on without waiting for the wave's slowest one (C3; C2's 9 meshes: 4,080
    // vs 3,891 Mpaths/s, tools/sweep_r02_ai.txt); the regenerating kernel for a few shallow meshes, where shading
    // dominates (C5's 2 meshes: 10,407 vs 9,718).  (Round 1, before the item scheduling and the mesh records in LDS,
    // the streaming kernel lost C2 too, tools/sweeps/sweep35.txt.)
    const bool deep_blas = hg_deep_blas(in.stack_depth);
    const bool stream_auto = deep_blas || in.n_meshes >= HG_STREAM_MIN_MESHES;
    const int32_t kern = in.kernel == HG_KERNEL_AUTO ? (stream_auto ? HG_KERNEL_MEGA_STREAM : HG_KERNEL_MEGA_REGEN)
                                                     : in.kernel;
    P.kernel = kern;
    P.stream_deep = deep_blas ? 1u : 0u;
    P.descent_t = hg_descent_t(in.descent_t, in.stack_depth, kern);
    const bool regen = (kern == HG_KERNEL_MEGA_REGEN || kern == HG_KERNEL_MEGA_STREAM) && in.debug_mode == 0 &&
                       in.max_bounces <= HG_REGEN_MAX_BOUNCES && in.spp < HG_REGEN_MAX_CHUNK;
    P.regen = regen;
    P.last_kernel = uint64_t(regen ? kern : HG_KERNEL_MEGA);
    // default block (option 128): 64 for the regenerating kernel (one tile per workgroup schedules best,
    // tools/sweeps/sweep12.txt), 256 for the lockstep one
    // the regenerating / streaming kernels run one wave per workgroup (their LDS row layout assumes it)
    const int mblock = regen ? 64 : (in.block == 128 ? 256 : in.block);
    P.block = mblock;
    // Frame-parallel split: `split` waves share each tile, each tracing a chunk of the frames, so a launch has
    // about 6x (formerly 16x, 12x) as many waves as the GPU holds at once (short waves: small drain tail; a rank's 1/N share
    // of the tiles at N GPUs still fills the GPU); the per-frame colours are then blended in frame order
    // (bit-identical).  Measured (tools/sweeps/sweep16-17.txt): C3 1080p 1180 -> 1251 Mpaths/s at N=1, and one
    // rank's share at N=8 314 -> 1212.
    const bool stream_k = regen && kern == HG_KERNEL_MEGA_STREAM;
    P.stream_k = stream_k;
    const int64_t tiles = in.n_local_tiles;
    const int64_t units = tiles;  // work units: one tile per wave
    const int64_t resident = hg_wave_slots(in.n_cu, stream_k ? HG_STREAM_WAVES : HG_MEGA_WAVES);
    int split = 1;
    if (regen && n_frames > 1 && tiles > 0) {
        if (in.frame_split > 0) split = std::min(n_frames, int(in.frame_split));
        // about 6 launches' worth of wave slots: with the cost order and a tile's chunks on consecutive waves
        // (wave_unit), fewer, longer waves win: a rank's share at N=2 split 2 vs 4 -> 2,409 vs 2,308, N=8 8 vs 16
        // -> 2,440 vs 2,337, C2 / C5 2 vs 3 -> +1.5 / +2.7 %, C3 at N=1 stays unsplit (tools/sweeps/sweep82-83.txt;
        // the multiplier was 16, then 12 with the chunk-major cost order)
        else split = int(std::min<int64_t>(n_frames, (6 * resident + units - 1) / units));
        // a share that runs the queue form (HG_OPT_QUEUE_FILL, hg_plan_chunk): smaller units, about 24 per wave slot,
        // so the launch's end leaves little behind (emulated N = 8 share of C3: split 8 / 16 / 32 -> 2,708 / 2,861 /
        // 2,933 Mpaths/s; per-tile waves at split 8: 2,790)
        // (the call's frames here, the chunk's in hg_plan_chunk: the two can disagree on a short last chunk)
        if (in.frame_split <= 0 && kern == HG_KERNEL_MEGA_STREAM && n_frames > HG_QUEUE_MAX_FRAMES &&
            hg_queue_fill(in, n_frames))
            split = int(std::min<int64_t>(n_frames, (int64_t(HG_QUEUE_FILL_UNITS) * resident + units - 1) / units));
    }
    // the AQL dispatch packet's grid size is a 32-bit count of work-items: at most 2^26 - 1 waves of 64 lanes
    constexpr int64_t kMaxWaves = (int64_t(1) << 26) - 1;
    if (units > kMaxWaves) {
        P.status = HG_E_UNSUPPORTED;
        return P;
    }
    if (units > 0) split = int(std::min<int64_t>(split, kMaxWaves / units));
    P.split = split;
    int chunk_max = HG_REGEN_MAX_CHUNK;
    // The streaming kernel (always) and the regenerating kernel (item scheduling or a frame split) store every
    // frame's colour and blend them into the accumulator in frame order afterwards (hg_blend.hip hg_blend_frames_*): such a launch
    // is traced on a trace stream and blended on the context stream (the trace pipeline, hg_ctx.h).
    P.items_k = regen && (stream_k || HG_REGEN_ITEMS);
    P.pipelined = regen && (P.items_k || split > 1);
    P.ordered = P.pipelined && in.tile_order_on && tiles > 0;
    P.per_frame = size_t(tiles) * 64 * 16;  // a float4 per pixel slot
    if (P.pipelined && P.per_frame)
        chunk_max = int(std::max<size_t>(1, std::min<size_t>(size_t(chunk_max), kFrameColorCap / P.per_frame)));
    P.chunk_max = chunk_max;
    P.grid = int((units * split + mblock / 64 - 1) / (mblock / 64));
    P.spill_stride = uint32_t(P.grid) * uint32_t(mblock);
    // stack entries beyond the LDS part: one column per thread (the streaming kernel's LDS part may be shorter)
    const uint32_t lds_part = std::min<uint32_t>(HG_MEGA_LDS_STACK, HG_STREAM_LDS_STACK);
    P.spill_bytes = in.stack_depth > lds_part ? size_t(P.spill_stride) * (in.stack_depth - lds_part) * 4 : 0;
    const int last_chunk = n_frames % chunk_max;
    P.short_chunks = std::min(n_frames, chunk_max) <= HG_QUEUE_MAX_FRAMES ||
                     (last_chunk != 0 && last_chunk <= HG_QUEUE_MAX_FRAMES);
    P.big_frames = std::min(n_frames, chunk_max);
    P.short_frames = std::min(n_frames, std::min(chunk_max, HG_QUEUE_MAX_FRAMES));
    return P;
}

struct HgChunkPlan {
    int frame_split;
    bool queue;         // the persistent work-queue form
    uint32_t wave_units;
    bool short_stream;  // traced on any trace stream in turn (else on the first HG_TRACE_LANES_BIG)
};

// One chunk of `frames` frames of a call planned as P
inline HgChunkPlan hg_plan_chunk(const HgPlanIn& in, const HgCallPlan& P, int32_t frames) {
    HgChunkPlan k{};
    // short chunks (the reference's one dispatch per frame) in turn on every trace stream, so that more
    // launches' tails overlap; long ones on the first HG_TRACE_LANES_BIG (a third 64-frame launch beside
    // two others cost C3 1.5 %)
    k.short_stream = frames <= HG_QUEUE_MAX_FRAMES;
    k.frame_split = std::min(P.split, int(frames));
    // the persistent work-queue form for launches of few frames (the reference's one dispatch per frame),
    // and for a launch too small to fill the GPU with 64-frame tile waves (a rank's 1/N of the image at N
    // GPUs, HG_OPT_QUEUE_FILL): persistent waves pull (tile, frame chunk) units, so a wave's lanes drain
    // once per launch, not once per short wave.  A share's launch of many frames fills the GPU with split
    // tile waves instead (emulated N = 8 share of C3, 512 frames: queue 3,289, split tile waves 3,543)
    k.queue = P.stream_k && (frames <= HG_QUEUE_MAX_FRAMES || hg_queue_fill(in, frames));
    // Streaming launches without the queue and without a frame split: each wave traces wave_units
    // consecutive tiles of the cost order, its lanes draining once per wave instead of once per tile
    // (UnitItems), while the launch keeps at least HG_WAVE_UNITS_ROUNDS waves per resident slot
    k.wave_units = 1;
    // (whole tiles only: a wave's units are all 8 x 8, UnitItems)
    if (P.stream_k && !k.queue && k.frame_split == 1 && in.n_local_tiles > 0 && in.W % HG_TILE == 0 &&
        in.H % HG_TILE == 0) {
        const int64_t slots = hg_wave_slots(in.n_cu, HG_STREAM_WAVES);
        const int64_t auto_wu =
            std::min<int64_t>(HG_WAVE_UNITS_MAX, int64_t(in.n_local_tiles) / (int64_t(HG_WAVE_UNITS_ROUNDS) * slots));
        k.wave_units = uint32_t(in.wave_units > 0 ? in.wave_units : std::max<int64_t>(1, auto_wu));
    }
    return k;
}

// Persistent waves of a queue launch.  A launch's end costs each of its waves the time its last paths take, with its
// lanes draining; fewer, longer-lived waves pay that less often.  So while two or more other traces are in flight
// (which fill the slots), a launch takes slots / min(HG_QUEUE_WAVES_DIV, traces in flight + 1); alone or beside one
// other (e.g. a caller that reads every frame back), all.
inline uint32_t hg_queue_waves(uint32_t slots, int busy) {
    return HG_QUEUE_WAVES_DIV > 1 && busy >= 2 ? slots / uint32_t(std::min(HG_QUEUE_WAVES_DIV, busy + 1)) : slots;
}

// Frames of consecutive calls held for one launch (HG_OPT_COALESCE).  A rank's share of the image (N > 1) holds until
// its launch fills the GPU as one context's launch of the whole image does (HG_SHARE_HOLD_ROUNDS): a 1/8 share's
// 64-frame launch has 4,050 tiles for 5,120 wave slots, and its tail is as long as a full launch's.
inline int32_t hg_hold_window(const HgPlanIn& in) {
    int64_t w = in.coalesce;
    if (w > 1 && in.n_ranks > 1 && in.n_local_tiles > 0) {
        const int64_t slots = hg_wave_slots(in.n_cu, HG_STREAM_WAVES);
        const int64_t share = (int64_t(HG_SHARE_HOLD_ROUNDS) * slots * 64 + in.n_local_tiles - 1) / in.n_local_tiles;
        w = std::max(w, std::min<int64_t>(share, HG_SHARE_HOLD_MAX));
    }
    return int32_t(w);
}

struct HgServerPlan {
    uint32_t ring;        // colour ring slots: HG_SV_RING halved until the ring fits 2 GiB (2 at least)
    uint32_t slots, grid;  // persistent waves the GPU holds, and the launch's
    size_t per_frame, spill_bytes;
    uint32_t frames_cap;  // frames of one lifetime: tiles * frames < 2^31
    uint32_t div_magic, div_shift;  // unit -> frame (hg_server.h sv_frame): a shift, or a multiply-high and a shift
};

// The render server's launch for `tiles` > 0 local tiles at `waves` persistent waves per SIMD
inline HgServerPlan hg_plan_server(int32_t n_cu, uint32_t tiles, uint32_t stack_depth, int waves) {
    HgServerPlan S{};
    S.per_frame = size_t(tiles) * 64u * 16u;
    S.ring = HG_SV_RING;
    while (S.ring > 2u && size_t(S.ring) * S.per_frame > (size_t(2) << 30)) S.ring >>= 1;
    S.slots = uint32_t(hg_wave_slots(n_cu, waves));
    S.grid = std::min(tiles, S.slots);
    const uint32_t lds_part = HG_STREAM_LDS_STACK;
    S.spill_bytes = stack_depth > lds_part ? size_t(S.grid) * 64u * (stack_depth - lds_part) * 4u : 0;
    S.frames_cap = std::min<uint32_t>(1u << 24, uint32_t((uint64_t(1) << 31) / std::max<uint32_t>(tiles, 1u)));
    if ((tiles & (tiles - 1u)) == 0u) {
        S.div_magic = 0u;
        S.div_shift = uint32_t(__builtin_ctz(tiles));
    } else {
        const uint32_t l = 31u - uint32_t(__builtin_clz(tiles));
        S.div_magic = uint32_t(((uint64_t(1) << (32 + l)) + tiles - 1u) / tiles);
        S.div_shift = l;
    }
    return S;
}
