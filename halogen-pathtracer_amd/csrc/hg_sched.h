// hg_sched.h — how the regenerating and streaming kernels hand work to their waves and lanes: the wave's unit (tile,
// frame chunk), the wave cost clock behind the cost order, and the (pixel, frame) item schedulers (TileItems, UnitItems,
// the two-unit queue).  The integer arithmetic is hg_items.h's (tested on the CPU); here are the LDS objects, the
// atomics and the loads.  Included by hg_mega.hip only: the __shared__ objects below belong to that translation unit.
#pragma once
#include "hg_device.h"
#include "hg_items.h"

using namespace hgd;

// Cost-ordered dispatch (HgKernelParams::tile_order): the wave's tile, read through the scalar cache (the order is
// written by hg_order_tiles before this launch and never during it).
__device__ __forceinline__ int ordered_tile(const HgKernelParams& kp, uint32_t w) {
    if (!kp.tile_order) return int(w);
    return int(kp.tile_order[w]);
}
// The wave's work unit (tile, frame chunk): hg_wave_unit_pos (cost order: tools/sweeps/sweep81.txt) and the read of the
// order.  Waves past the last unit get chunk = split (no work).
__device__ __forceinline__ void wave_unit(const HgKernelParams& kp, uint32_t gw, uint32_t nlt, uint32_t split,
                                          int& tile, uint32_t& chunk) {
    // (the order flag a constant in each branch: decided once, the branches compile as they did written out)
    if (kp.tile_order) {
        const uint32_t w = hg_wave_unit_pos(gw, nlt, split, true);
        tile = w < nlt ? ordered_tile(kp, w) : 0;
        chunk = hg_wave_unit_chunk(gw, nlt, split, true);
        return;
    }
    tile = ordered_tile(kp, hg_wave_unit_pos(gw, nlt, split, false));
    chunk = hg_wave_unit_chunk(gw, nlt, split, false);
}
// The image rectangle of local tile t.  The tile's integer type is the division's: the kernels' prologues hold the tile
// as int and divide signed, the schedulers as uint32_t (hg_global_tile_rect).
template <class I>
__device__ __forceinline__ I global_tile(const HgKernelParams& kp, I t) {
    return hg_global_tile<I>(t, I(kp.rank), I(kp.n_ranks));
}
template <class I>
__device__ __forceinline__ void tile_rect(const HgKernelParams& kp, I t, HgTileRect& r) {
    hg_global_tile_rect<I>(global_tile(kp, t), I(kp.tiles_x), kp.Wu, kp.Hu, r);
}

// The wave's clock time (s_memtime cycles), added to its tile's 64-bit cost for the next launch's order (no wrap for
// any launch: 2^64 cycles).  The start time and the tile wait in LDS, not in registers that would stay live across
// the whole kernel.
__shared__ uint64_t hg_wave_t0[4];
__shared__ unsigned long long* hg_wave_cost[4];  // &tile_cost[tile], null: not recorded
// a global-memory atomic add through a pointer kept in LDS (a generic pointer would compile to a FLAT atomic)
__device__ __forceinline__ void cost_add(unsigned long long* p, uint64_t v) {
    typedef __attribute__((address_space(1))) unsigned long long* gptr;
    __hip_atomic_fetch_add((gptr)(uintptr_t)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void tile_cost_begin(const HgKernelParams& kp, uint32_t lane, int tile, bool valid) {
    if (lane == 0) {
        hg_wave_cost[threadIdx.x >> 6] = kp.tile_cost && valid ? kp.tile_cost + tile : nullptr;
        hg_wave_t0[threadIdx.x >> 6] = wave_clock();
    }
}
// A persistent wave moves on to `tile` (one lane): the clock since the previous switch goes to the previous tile's cost
__device__ __forceinline__ void cost_switch(const HgKernelParams& kp, int tile) {
    const uint64_t now = wave_clock();
    unsigned long long* const prev = hg_wave_cost[threadIdx.x >> 6];
    if (prev) cost_add(prev, now - hg_wave_t0[threadIdx.x >> 6]);
    hg_wave_cost[threadIdx.x >> 6] = kp.tile_cost ? kp.tile_cost + tile : nullptr;
    hg_wave_t0[threadIdx.x >> 6] = now;
}
__device__ __forceinline__ void record_tile_cost(uint32_t lane) {
    if (lane != 0) return;
    unsigned long long* const p = hg_wave_cost[threadIdx.x >> 6];
    if (p) cost_add(p, wave_clock() - hg_wave_t0[threadIdx.x >> 6]);
}

// (pixel, frame) items of a wave's tile (HG_STREAM_ITEMS / HG_REGEN_ITEMS): with the v pixels of the tile inside the
// image (a w x h rectangle; all 64 for a whole tile) and the nf frames of the chunk, item k is valid pixel k / nf of
// frame f_begin + k mod nf (hg_item_split).  Lane l starts with item l; a lane whose frame is done takes the next
// unassigned item (its rank among the wave's lanes that need one), so the lanes stay busy until the tile's items run
// out instead of each waiting for its own pixel's slowest frames.  Every frame's colour goes to frame_color and
// hg_blend_frames applies the accumulation blend in frame order afterwards: the same operations in the same order as a
// lane tracing its pixel's frames in turn.
__shared__ uint32_t hg_next_item;  // items of the wave's tile handed out so far (one wave per workgroup)
// Called by exactly the lanes that need an item (the active lanes): they take the wave's next item numbers in lane
// order.  The first of them advances the LDS counter with one atomic add and its old value goes to the others by
// readfirstlane.  The caller decodes the number inside its branch (decoded here, the frame was held across a
// control-flow merge and spilled to scratch at every take).
__device__ __forceinline__ uint32_t wave_take() {
    const uint64_t m = __builtin_amdgcn_read_exec();
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
    uint32_t base = 0;
    if (rank == 0u) base = atomicAdd(&hg_next_item, uint32_t(__builtin_popcountll(m)));
    base = __builtin_amdgcn_readfirstlane(base);
    return base + rank;
}
struct TileItems {
    uint32_t tx0, ty0, tw, nv, n_items, f_begin;  // wave-uniform (scalar registers)
    uint32_t nf;  // frames of the chunk
    __device__ TileItems() : tx0(0), ty0(0), tw(0), nv(0), n_items(0), f_begin(0), nf(1u) {}  // unused
    __device__ TileItems(const HgKernelParams& kp, int local_tile, bool valid, uint32_t fb, uint32_t fe, uint32_t lane) {
        const int g = __builtin_amdgcn_readfirstlane(global_tile(kp, local_tile));
        hg_global_tile_origin<int>(g, kp.tiles_x, tx0, ty0);
        // (hg_global_tile_rect in its steps: each extent is made uniform before the next is computed)
        tw = __builtin_amdgcn_readfirstlane(hg_tile_extent(kp.Wu, tx0));
        const uint32_t th = __builtin_amdgcn_readfirstlane(hg_tile_extent(kp.Hu, ty0));
        nv = tw * th;
        n_items = __builtin_amdgcn_readfirstlane(valid && fe > fb ? nv * (fe - fb) : 0u);
        f_begin = fb;
        nf = __builtin_amdgcn_readfirstlane(fe > fb ? fe - fb : 1u);
        if (lane == 0) hg_next_item = 64u;  // lane l starts with item l
        wave_lds_sync();
    }
    // item k (k >= n_items: the tile's items are all handed out) -> its pixel within the tile (x + 8 y) and frame; a
    // wave's lanes trace one pixel's frames (with the [slot][frame] colours: C3 +0.4 %, C2 +0.5 %, C5 -0.4 %;
    // tools/sweeps/sweep_r02_be/bf)
    __device__ __forceinline__ void get(uint32_t k, uint32_t& pix, uint32_t& frame) const {
        const HgItem it = hg_item_split(k, nf);
        pix = hg_item_pixel(it.i, tw, nv);
        frame = f_begin + it.f;
    }
};

// LDS words read / written by different lanes of the wave (see the queue's note below)
__device__ __forceinline__ uint32_t lds_get(uint32_t& x) {
    return __hip_atomic_load(&x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_put(uint32_t& x, uint32_t v) {
    __hip_atomic_store(&x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// (pixel, frame) items of a streaming wave's units (launches without the queue).  The wave traces the nu units
// [u0, u0 + nu) of the launch's unit order (wave_unit; nu = kp.wave_units <= HG_WAVE_UNITS_LIMIT, more than one only
// without a frame split, where unit u is tile ordered_tile(u) with all the launch's frames), their items numbered one
// unit after another and pixel-major within a unit as in TileItems.  A lane that finishes a frame takes the wave's
// next item whichever unit holds it, so the wave's lanes drain once per nu tiles instead of once per tile; which wave
// traces an item changes nothing (every item runs with its own pixel's and frame's inputs and writes its own colour
// slot).  A lane's item is held as v = unit j << 6 | pixel (x + 8 y); the units' tiles and image origins sit in the
// wave's LDS (the kernel's scalar registers are all taken), read once when a path starts and once when it ends.
__shared__ uint32_t hg_unit_tile[HG_WAVE_UNITS_LIMIT];  // unit j's local tile
__shared__ uint32_t hg_unit_org[HG_WAVE_UNITS_LIMIT];   // its image origin x | y << 16
__shared__ uint32_t hg_unit_shape;                      // unit 0's valid width | valid pixels << 8
struct UnitItems {
    uint32_t nu, nf, f_begin, n_items, full;  // wave-uniform (scalar registers)
    __device__ UnitItems() : nu(0), nf(1), f_begin(0), n_items(0), full(1) {}  // unused (kQueue)
    __device__ UnitItems(const HgKernelParams& kp, uint32_t u_first, int first_tile, bool valid, uint32_t fb,
                         uint32_t fe, uint32_t lane) {
        const uint32_t nlt = uint32_t(kp.n_local_tiles), u0 = __builtin_amdgcn_readfirstlane(u_first);
        nu = valid ? (kp.wave_units > 1u && u0 < nlt ? min(min(kp.wave_units, uint32_t(HG_WAVE_UNITS_LIMIT)), nlt - u0)
                                                     : 1u)
                   : 0u;
        nu = __builtin_amdgcn_readfirstlane(nu);
        nf = __builtin_amdgcn_readfirstlane(fe > fb ? fe - fb : 1u);
        f_begin = fb;
        n_items = 0u;
        full = 1u;
        for (uint32_t j = 0; j < nu; ++j) {
            const uint32_t t = __builtin_amdgcn_readfirstlane(j == 0u ? first_tile : ordered_tile(kp, u0 + j));
            HgTileRect r;
            tile_rect(kp, t, r);
            if (lane == 0) {
                hg_unit_tile[j] = t;
                hg_unit_org[j] = r.x0 | (r.y0 << 16);
                if (j == 0u) hg_unit_shape = r.tw | ((r.tw * r.th) << 8);
            }
            n_items += r.tw * r.th * (fe > fb ? fe - fb : 0u);
            full &= r.tw * r.th == 64u ? 1u : 0u;
        }
        n_items = __builtin_amdgcn_readfirstlane(n_items);
        full = __builtin_amdgcn_readfirstlane(full);
        if (lane == 0) hg_next_item = 64u;  // lane l starts with item l
        wave_lds_sync();
    }
    // item k -> v (unit j << 6 | pixel) and its frame.  Whole tiles: hg_unit_item (hg_items.h, tested there), its unit
    // split written out here: through a function these kernels compile to other instructions, and theirs are held fixed
    __device__ __forceinline__ void get(const HgKernelParams& kp, uint32_t k, uint32_t& v, uint32_t& frame) const {
        uint32_t j = 0u, kk = k, nv = 64u, tw = 8u;
        if (full) {
            if ((nf & (nf - 1u)) == 0u) {
                const uint32_t lg = 6u + uint32_t(__builtin_ctz(nf));
                j = k >> lg;
                kk = k & ((1u << lg) - 1u);
            } else {
                j = k / (64u * nf);
                kk = k - j * (64u * nf);
            }
        } else {  // a tile at the image edge (only ever a wave's one unit: the runtime gives such images one tile per wave)
            const uint32_t sh = lds_get(hg_unit_shape);
            tw = sh & 0xFFu;
            nv = sh >> 8;
        }
        const HgItem it = hg_item_split(kk, nf);
        v = (j << 6) | hg_item_pixel(it.i, tw, nv);
        frame = f_begin + it.f;
    }
    __device__ __forceinline__ uint32_t slot(uint32_t v) const {
        return nu <= 1u ? (lds_get(hg_unit_tile[0]) * 64u + v) : lds_get(hg_unit_tile[v >> 6]) * 64u + (v & 63u);
    }
    __device__ __forceinline__ void pixel(uint32_t v, uint32_t& x, uint32_t& y) const {
        const uint32_t o = lds_get(hg_unit_org[v >> 6]);
        x = (o & 0xFFFFu) + (v & 7u);
        y = (o >> 16) + ((v >> 3) & 7u);
    }
    // the wave's clock since tile_cost_begin, shared out over its units' tiles (the first one's pointer is in LDS)
    __device__ __forceinline__ void record_cost(const HgKernelParams& kp, uint32_t lane) const {
        if (nu <= 1u) {
            record_tile_cost(lane);
            return;
        }
        if (lane != 0 || !hg_wave_cost[threadIdx.x >> 6]) return;
        const uint64_t share = (wave_clock() - hg_wave_t0[threadIdx.x >> 6]) / nu;
        for (uint32_t j = 0; j < nu; ++j) cost_add(kp.tile_cost + lds_get(hg_unit_tile[j]), share);
    }
};

// Persistent streaming waves over a work queue (kQueue: launches of at most HG_QUEUE_MAX_FRAMES frames, e.g. the
// reference's one dispatch per frame, RP:327).  The launch has one wave per resident wave slot
// (kp.resident_waves, at most one per unit); each wave pulls (tile, frame chunk) units from the queue and hands their
// (pixel, frame) items to its lanes in order (pixel-major, as TileItems).  A lane that finishes a frame takes the
// wave's next item in place; a lane that finds the current unit spent idles until the top of the wave's loop, where
// the wave pulls the next unit for its idle lanes, while the lanes still on the old unit's items carry on.  So a lane
// idles only between a unit's end and the next loop top, and at the very end of the queue, not until its tile's
// slowest path is done.  Without it a 1-frame launch (one item per pixel) kept each wave's 64 lanes waiting for its
// tile's slowest path: 899 -> 1,383 Mpaths/s on C3 as 1-frame launches.  With 64-frame launches the per-tile waves win
// (one tile's 4,096 items keep the lanes busy anyway; the queue's per-take LDS reads cost C3 2.6 %, C2 6.6 %).  The
// queue is 8 heads, one per XCD
// (workgroups are placed on XCD blockIdx mod 8): head h hands out units h, h + 8, h + 16, ... in the cost order
// (wave_unit), and a wave whose head is dry steals from the others.  Which wave traces an item changes nothing: every
// item runs with the inputs the reference's dispatch of that frame gives its pixel, and writes its own colour slot.
// LDS words read / written by different lanes of the wave: relaxed workgroup-scope atomics on the __shared__ object
// itself compile to plain ds_read / ds_write that the compiler may not cache in registers (a volatile access through
// a cast pointer became a FLAT access with a 64-bit generic address and cost the kernel 60 B of scratch)
constexpr uint32_t kFreshLane = 0xFFFFFFFFu;  // `bounce` of a lane that has no path yet (it takes its item when shading)
// The wave's two current units (double-buffered), in LDS (one wave per workgroup).  Item numbers (hg_next_item) run on
// across units: unit hg_q_cur covers [base, end), the other one the numbers after it, so a lane whose take runs past
// the first unit's items gets the second's at once; the loop top refills the spent unit.
struct QueueUnit {
    uint32_t base, end;                            // the wave's item numbers [base, end) are this unit's items
    uint32_t tile, tx0, ty0, tw, nv, f_begin, nf;  // its tile (local index, origin, width, valid pixels), frames
};
__shared__ QueueUnit hg_qu[2];
__shared__ uint32_t hg_q_cur;  // the unit whose items come first
__shared__ uint32_t hg_q_dry;  // the queue has no unit left
__shared__ uint32_t hg_q_empty;  // the queue has no unit left and both units are spent (the wave's lanes retire)
// (kQueue launches, not the server) a lane's take reached past the first unit (or found both spent): the loop top must
// refill.  Raised by the taking lanes, cleared by the refill; the loop top reads this one word instead of running the
// refill (lane 0's reads of the item count, the current unit and its end) on every trace / shade round.
__shared__ uint32_t hg_q_need;

// Pull the next unit of the queue into hg_qu[slot], its items numbered from `base` (one lane).  When the queue is dry
// the unit is empty (end = base) and hg_q_dry is set.  Attributes the wave clock since the previous pull to the
// previous unit's tile cost (the cost order of the next launches).
__device__ __forceinline__ void queue_pull(const HgKernelParams& kp, uint32_t n_units, uint32_t split, uint32_t slot,
                                           uint32_t base) {
    const uint32_t x = blockIdx.x & 7u;
    uint32_t u = n_units;
    for (uint32_t t = 0; t < 8u && u >= n_units; ++t) {  // own XCD's head first, then steal
        const uint32_t h = (x + t) & 7u;
        if (h >= n_units) continue;
        const uint32_t j = atomicAdd(kp.queue + 32u * h, 1u);
        if (uint64_t(h) + 8ull * j < n_units) u = h + 8u * j;
    }
    QueueUnit& q = hg_qu[slot];
    lds_put(q.base, base);
    if (u >= n_units) {
        lds_put(q.end, base);
        lds_put(hg_q_dry, 1u);
        return;  // the last unit's cost is recorded at the wave's end (record_tile_cost)
    }
    int tile;
    uint32_t chunk;
    wave_unit(kp, u, uint32_t(kp.n_local_tiles), split, tile, chunk);
    // hg_chunk_begin of chunk and chunk + 1, written out: through the function, this one site (its chunk in a vector
    // register) compiles with two operands of a multiply exchanged, and the kernels' instructions are held fixed
    const uint32_t fb = uint32_t((uint64_t(chunk) * uint32_t(kp.n_frames)) / split);
    const uint32_t fe = uint32_t((uint64_t(chunk + 1) * uint32_t(kp.n_frames)) / split);
    HgTileRect r;
    tile_rect(kp, uint32_t(tile), r);
    cost_switch(kp, tile);
    lds_put(q.tile, uint32_t(tile));
    lds_put(q.tx0, r.x0);
    lds_put(q.ty0, r.y0);
    lds_put(q.tw, r.tw);
    lds_put(q.nv, r.tw * r.th);
    lds_put(q.f_begin, fb);
    lds_put(q.nf, fe > fb ? fe - fb : 1u);
    lds_put(q.end, base + r.tw * r.th * (fe - fb));
}

// Loop top (lane 0, the whole wave converged): keep both units filled.  Returns true when no item is left anywhere.
__device__ __forceinline__ bool queue_refill(const HgKernelParams& kp, uint32_t n_units, uint32_t split) {
    const uint32_t cnt = lds_get(hg_next_item);
    uint32_t a = lds_get(hg_q_cur);
    if (cnt >= lds_get(hg_qu[a].end) && !lds_get(hg_q_dry)) {  // the first unit is spent
        const uint32_t b = a ^ 1u, b_end = lds_get(hg_qu[b].end);
        if (cnt < b_end) {  // the second one is in use: it comes first now, the spent one is refilled after it
            lds_put(hg_q_cur, b);
            queue_pull(kp, n_units, split, a, b_end);
            a = b;
        } else {  // both spent (numbers taken by lanes that found them so are skipped): two new units
            queue_pull(kp, n_units, split, a, cnt);
            queue_pull(kp, n_units, split, b, lds_get(hg_qu[a].end));
        }
    }
    return lds_get(hg_q_dry) && cnt >= lds_get(hg_qu[a ^ 1u].end) && cnt >= lds_get(hg_qu[a].end);
}

// Item number k of the wave, if one of the two current units holds it: its accumulator slot, frame and pixel
// (pixel-major, as TileItems::get).  Called by the lanes that took k.
__device__ __forceinline__ bool queue_item(uint32_t k, uint32_t& slot, uint32_t& frame, uint32_t& px, uint32_t& py) {
    const uint32_t a = __builtin_amdgcn_readfirstlane(lds_get(hg_q_cur));
    const uint32_t a_end = __builtin_amdgcn_readfirstlane(lds_get(hg_qu[a].end));
    const uint32_t b_end = __builtin_amdgcn_readfirstlane(lds_get(hg_qu[a ^ 1u].end));
    if (k >= a_end) lds_put(hg_q_need, 1u);  // the first unit is spent (the server's loop top refills every round)
    if (k >= b_end && k >= a_end) return false;
    QueueUnit& q = hg_qu[k < a_end ? a : a ^ 1u];
    const uint32_t base = lds_get(q.base);
    if (k < base) return false;  // (never: numbers below the first unit were all handed out before it)
    const uint32_t kk = k - base, nf = lds_get(q.nf), nv = lds_get(q.nv), tw = lds_get(q.tw);
    const HgItem it = hg_item_split(kk, nf);
    const uint32_t pix = hg_item_pixel(it.i, tw, nv);
    slot = lds_get(q.tile) * 64u + pix;
    frame = lds_get(q.f_begin) + it.f;
    px = lds_get(q.tx0) + (pix & 7u);
    py = lds_get(q.ty0) + (pix >> 3);
    return true;
}

// The image pixel of accumulator slot `slot` (local tile slot / 64, pixel slot % 64)
__device__ __forceinline__ void slot_pixel(const HgKernelParams& kp, uint32_t slot, uint32_t& x, uint32_t& y) {
    HgTileRect r;
    tile_rect(kp, slot >> 6, r);
    x = r.x0 + (slot & 7u);
    y = r.y0 + ((slot >> 3) & 7u);
}
