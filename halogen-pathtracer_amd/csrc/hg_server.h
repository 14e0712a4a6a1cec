// hg_server.h — the device half of the render server (the host half: hg_render.hip).  Included by hg_mega.hip only, after
// hg_sched.h: the server's waves are the streaming kernel's queue waves, and hg_sv below belongs to that translation
// unit.
#pragma once
#include "hg_sched.h"

// The render server (kServer): the persistent queue waves outlive hg_render calls.  The reference dispatches once per
// frame (RP:327, RP:406); a launch per frame ends with every wave draining its last paths, its other lanes idle (0.63 ms
// of a C3 frame's 1.2 ms).  Here one launch serves every frame the host posts while it lives:
// unit u of the server is (frame k = u / tiles, the tile at cost-order position u mod tiles), handed out through the
// same 8 per-XCD heads, bounded by the frames posted so far; so the lanes that frame k's last paths leave idle take
// frame k+1's items at once.  Which wave traces an item changes nothing: every item runs with the inputs the
// reference's dispatch of frame k gives its pixel (FrameCount = first_frame + k) and writes its own colour slot.
//   posting   the host raises the post word (pinned host memory: frames posted | stop << 32).  A wave that finds no
//             posted unit reads the device mirror of that word; at most one wave per HG_SV_POLL_TICKS reads the host
//             word itself (a ticket) and raises the mirror by atomic max.
//   frames    a wave counts, per frame in a window of 4 (LDS), the units it pulled and the items of them its lanes
//             finished; once they match, after a store drain, it adds the units to the frame's ring-slot count
//             (frames_done).  Colours go to the frame's ring slot, and the ring and the counts are uncached device
//             memory (no XCD's L2 holds their lines): the gate kernel on the context stream waits for the count, and
//             the blend after it reads the colours, whichever XCD wrote them (plain stores then the drain, then the
//             count's atomic: the colours are in memory before the count says so).
//   leaving   a wave with no item and no posted unit left waits (s_sleep); it leaves once the stop flag is in its view
//             and nothing posted is left to claim.  The stop flag comes from the host (server_stop), or from the close
//             handshake: after sv_idle_ticks with nothing new posted, one wave closes the server (sv_close).  It raises
//             the closing word in host memory, then reads the post word, and publishes what it read with the stop flag
//             (to the host and to every mirror): every frame it read is traced before the waves leave.  The host raises
//             the post word, then reads the closing word; a post that finds it raised counts only if the closing wave
//             read it (both sides store, then load: at least one sees the other's store), else the host restarts the
//             server and posts there.  So no posted frame can meet a server whose waves have all left.
// Only the lane 0 of a wave runs these (the whole wave converged at the loop top).
// Per-wave LDS state (lane 0 reads and writes it; the constants are copied from the kernel arguments once, so that no
// server value stays in a scalar register across the kernel's loop: its scalar registers are all taken, and every
// value kept live there spilled the traversal's vector registers to scratch — 84 B per lane in the first form)
struct SvWave {
    uint32_t view;   // units posted as this wave last saw them
    uint32_t dry;    // the view at which this wave last found every head dry (HG_NONE: none)
    uint32_t pend;   // a unit claimed beyond the view, or whose frame window was busy (HG_NONE: none)
    uint32_t more, more_n;  // the rest of a multi-unit claim: more_n units from `more` in steps of 8, after pend
    uint32_t stop;   // the stop flag as this wave last saw it
    uint32_t nlt, mask, cap, magic, shift, idle_ticks;  // tiles per frame, ring slots - 1, frames cap, u / nlt, leave after
    uint32_t post_lo, post_hi, done_lo, done_hi;        // the host post word and the ring-slot counts (pointers)
    uint32_t win_frame[4], win_units[4], win_items[4], win_done[4];  // frame window (k & 3)
};
__shared__ SvWave hg_sv;

__device__ __forceinline__ unsigned long long* sv_word64(const HgKernelParams& kp, uint32_t word) {
    return reinterpret_cast<unsigned long long*>(kp.queue + word);
}
template <class T>
__device__ __forceinline__ T* sv_ptr(uint32_t lo, uint32_t hi) {
    return reinterpret_cast<T*>((uint64_t(hi) << 32) | lo);
}
__device__ void sv_init(const HgKernelParams& kp) {  // lane 0, at the kernel's start
    lds_put(hg_sv.view, 0u);
    lds_put(hg_sv.dry, HG_NONE);
    lds_put(hg_sv.pend, HG_NONE);
    lds_put(hg_sv.more_n, 0u);
    lds_put(hg_sv.stop, 0u);
    lds_put(hg_sv.nlt, uint32_t(kp.n_local_tiles));
    lds_put(hg_sv.mask, kp.sv_ring - 1u);
    lds_put(hg_sv.cap, kp.sv_frames_cap);
    lds_put(hg_sv.magic, kp.sv_div_magic);
    lds_put(hg_sv.shift, kp.sv_div_shift);
    lds_put(hg_sv.idle_ticks, kp.sv_idle_ticks);
    lds_put(hg_sv.post_lo, uint32_t(uintptr_t(kp.sv_post)));
    lds_put(hg_sv.post_hi, uint32_t(uintptr_t(kp.sv_post) >> 32));
    lds_put(hg_sv.done_lo, uint32_t(uintptr_t(kp.frames_done)));
    lds_put(hg_sv.done_hi, uint32_t(uintptr_t(kp.frames_done) >> 32));
    for (uint32_t w = 0; w < 4u; ++w) {
        lds_put(hg_sv.win_frame[w], 0u);
        lds_put(hg_sv.win_units[w], 0u);
        lds_put(hg_sv.win_items[w], 0u);
        lds_put(hg_sv.win_done[w], 0u);
    }
}
// frame of unit u: u / nlt by the host's multiplier (exact for every u < 2^31; a power of two nlt: magic 0, a shift)
__device__ __forceinline__ uint32_t sv_frame(uint32_t u) {
    const uint32_t m = lds_get(hg_sv.magic);
    return (m ? __umulhi(u, m) : u) >> lds_get(hg_sv.shift);
}
// the posted units of a post word value
__device__ __forceinline__ uint32_t sv_units(unsigned long long w) {
    const uint32_t cap = lds_get(hg_sv.cap);
    return (uint32_t(w) < cap ? uint32_t(w) : cap) * lds_get(hg_sv.nlt);
}
// Refresh the view from the device mirror of the post word
__device__ uint32_t sv_view(const HgKernelParams& kp) {
    uint32_t v = lds_get(hg_sv.view);
    const unsigned long long m = sv_sload(sv_word64(kp, HG_SV_MIRROR_WORD + 32u * (blockIdx.x % HG_SV_MIRRORS)));
    const uint32_t u = sv_units(m);
    // a post word with the stop flag is final: its count may be below the frames posted ahead of the host's calls
    // (hg_render.hip server_speculate), which are abandoned (the units already pulled are traced)
    if (u > v || ((m & HG_SV_STOP) && u != v)) {
        v = u;
        lds_put(hg_sv.view, v);
    }
    if (m & HG_SV_STOP) lds_put(hg_sv.stop, 1u);
    return v;
}
// Take this XCD's host-poll ticket if it is free, read the host word over PCIe (system scope) and raise every mirror
// copy; then refresh the view.  (Idle waves call it every few spins, busy ones when they find the heads dry.)
__device__ uint32_t sv_poll(const HgKernelParams& kp) {
    unsigned long long* const ticket = sv_word64(kp, HG_SV_TICKET_WORD + 32u * (blockIdx.x & 7u));
    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
    unsigned long long t = sv_sload(ticket);
    if (now >= t && __hip_atomic_compare_exchange_strong(ticket, &t, now + HG_SV_POLL_TICKS, __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        const unsigned long long h = __hip_atomic_load(
            sv_ptr<const unsigned long long>(lds_get(hg_sv.post_lo), lds_get(hg_sv.post_hi)), __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        for (uint32_t m = 0; m < HG_SV_MIRRORS; ++m)
            __hip_atomic_fetch_max(sv_word64(kp, HG_SV_MIRROR_WORD + 32u * m), h, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
    return sv_view(kp);
}
// Pull the next posted unit into hg_qu[slot], its items numbered from `base` (empty when there is none for now)
__device__ void sv_pull(const HgKernelParams& kp, uint32_t slot, uint32_t base) {
    QueueUnit& q = hg_qu[slot];
    lds_put(q.base, base);
    lds_put(q.end, base);
    uint32_t u = lds_get(hg_sv.pend);
    uint32_t view = lds_get(hg_sv.view);
    if (u == HG_NONE) {
        if (view == lds_get(hg_sv.dry)) {  // every head was dry at this view: anything new posted?  (A busy wave
            view = sv_poll(kp);            // polls the host word too: no wave may be waiting to do it)
            if (view == lds_get(hg_sv.dry)) return;
        }
        const uint32_t x = blockIdx.x & 7u;
        uint32_t take = 1u;
        for (uint32_t t = 0; t < 8u && u == HG_NONE; ++t) {  // own XCD's head first, then steal
            const uint32_t h = (x + t) & 7u;
            const uint32_t n = ld_agent(kp.queue + 32u * h);
            if (h + 8u * n >= view) continue;
            // HG_SV_CLAIM units per atomic while the head holds posted units for as many claims of every wave of its
            // XCD (one wave per block): no frame's end is left to a wave holding several
            if (HG_SV_CLAIM > 1u) take = h + 8u * (n + HG_SV_CLAIM * (1u + gridDim.x / 8u)) < view ? HG_SV_CLAIM : 1u;
            u = h + 8u * atomicAdd(kp.queue + 32u * h, take);
        }
        if (u == HG_NONE) {
            lds_put(hg_sv.dry, view);
            return;
        }
        lds_put(hg_sv.more, u + 8u);  // (placed after u)
        lds_put(hg_sv.more_n, take - 1u);
    }
    if (u >= view) view = sv_view(kp);
    const uint32_t k = sv_frame(u), w = k & 3u;
    if (u >= view || (lds_get(hg_sv.win_units[w]) != 0u && lds_get(hg_sv.win_frame[w]) != k)) {
        lds_put(hg_sv.pend, u);  // (claimed past the posted frames by a race, or its frame window still busy): later
        return;
    }
    const uint32_t more_n = lds_get(hg_sv.more_n);  // the next unit of a multi-unit claim, if any, is pulled next
    lds_put(hg_sv.pend, more_n ? lds_get(hg_sv.more) : HG_NONE);
    if (more_n) {
        lds_put(hg_sv.more, lds_get(hg_sv.more) + 8u);
        lds_put(hg_sv.more_n, more_n - 1u);
    }
    if (HG_SV_DIAG_TIMES && k < 256u)  // (analysis builds) the frame's first claim: max of the complement
        __hip_atomic_fetch_max(sv_word64(kp, HG_SV_DIAG_WORD + 4u * k), ~(unsigned long long)__builtin_amdgcn_s_memrealtime(),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t i = u - k * lds_get(hg_sv.nlt);  // the unit's place in its frame
    if (HG_SV_TILE_RUN > 1u && !kp.tile_order) i = hg_sv_run_place(i, lds_get(hg_sv.nlt));
    const int tile = ordered_tile(kp, i);
    HgTileRect r;
    tile_rect(kp, uint32_t(tile), r);
    cost_switch(kp, tile);
    lds_put(q.tile, uint32_t(tile));
    lds_put(q.tx0, r.x0);
    lds_put(q.ty0, r.y0);
    lds_put(q.tw, r.tw);
    lds_put(q.nv, r.tw * r.th);
    lds_put(q.f_begin, k);
    lds_put(q.nf, 1u);
    lds_put(q.end, base + r.tw * r.th);
    lds_put(hg_sv.win_frame[w], k);
    lds_put(hg_sv.win_units[w], lds_get(hg_sv.win_units[w]) + 1u);
    lds_put(hg_sv.win_items[w], lds_get(hg_sv.win_items[w]) + r.tw * r.th);
}
// Frames of the window whose pulled items the lanes have all finished: after a drain of the wave's colour stores, their
// units go to the frame's ring-slot count
__device__ void sv_flush(const HgKernelParams& kp) {
    (void)kp;
    bool drained = false;
    for (uint32_t w = 0; w < 4u; ++w) {
        const uint32_t n = lds_get(hg_sv.win_units[w]);
        if (n == 0u || lds_get(hg_sv.win_done[w]) != lds_get(hg_sv.win_items[w])) continue;
        if (!drained) {  // every lane's colour stores complete before the count moves
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __builtin_amdgcn_s_waitcnt(0);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            drained = true;
        }
        uint32_t* const done = sv_ptr<uint32_t>(lds_get(hg_sv.done_lo), lds_get(hg_sv.done_hi));
        __hip_atomic_fetch_add(done + 32u * (lds_get(hg_sv.win_frame[w]) & lds_get(hg_sv.mask)), n, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if (HG_SV_DIAG_TIMES && lds_get(hg_sv.win_frame[w]) < 256u)  // (analysis builds) the frame's last count
            __hip_atomic_fetch_max(sv_word64(kp, HG_SV_DIAG_WORD + 4u * lds_get(hg_sv.win_frame[w]) + 2u),
                                   (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        lds_put(hg_sv.win_units[w], 0u);
        lds_put(hg_sv.win_items[w], 0u);
        lds_put(hg_sv.win_done[w], 0u);
    }
}
// Loop top: flush finished frames, keep both units filled (the spent one refilled after the other; both spent: two
// new units, in turn).  Returns true when the wave has no item to hand out now.
__device__ bool sv_refill(const HgKernelParams& kp) {
    sv_flush(kp);
    const uint32_t cnt = lds_get(hg_next_item);
    uint32_t a = lds_get(hg_q_cur);
    if (cnt >= lds_get(hg_qu[a].end)) {  // the first unit is spent
        const uint32_t b_end = lds_get(hg_qu[a ^ 1u].end);
        const bool both = cnt >= b_end;
        if (!both) lds_put(hg_q_cur, a ^ 1u);  // the second one is in use: it comes first now
        for (uint32_t i = 0; i < (both ? 2u : 1u); ++i) {  // (one inlined pull: every copy costs the loop registers)
            const uint32_t slot = a ^ i;
            sv_pull(kp, slot, i ? lds_get(hg_qu[a].end) : both ? cnt : b_end);
        }
        if (!both) a ^= 1u;
    }
    return cnt >= lds_get(hg_qu[a ^ 1u].end) && cnt >= lds_get(hg_qu[a].end);
}
// The close handshake (lane 0 of an idle wave, after sv_idle_ticks with nothing new posted).  One wave wins the closing
// word of the control block; it raises the host's closing word, then reads the post word (system scope, sequentially
// consistent: the store is visible to the host before the load is performed), and publishes the post word it read with
// the stop flag, to the host (the close word, HG_SV_CLOSED) and to every mirror (atomic max: the stop flag outranks
// every post word without it, so a poller that read a later post word cannot raise a view past it).  Every wave then
// drains the frames of that view and leaves.  The host's side is hg_render.hip server_post_frame.
__device__ void sv_close(const HgKernelParams& kp) {
    uint32_t* const word = kp.queue + HG_SV_CLOSE_WORD;
    if (ld_agent(word) != 0u || atomicCAS(word, 0u, 1u) != 0u) return;  // another wave closes it
    unsigned long long* const host = sv_ptr<unsigned long long>(lds_get(hg_sv.post_lo), lds_get(hg_sv.post_hi));
    __hip_atomic_store(host + HG_SV_HOST_CLOSING, 1ull, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_SYSTEM);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    const unsigned long long p = __hip_atomic_load(host + HG_SV_HOST_POST, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long fin = (p & 0xFFFFFFFFull) | HG_SV_STOP;
    __hip_atomic_store(host + HG_SV_HOST_CLOSED, fin | HG_SV_CLOSED, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_SYSTEM);
    for (uint32_t m = 0; m < HG_SV_MIRRORS; ++m)
        __hip_atomic_fetch_max(sv_word64(kp, HG_SV_MIRROR_WORD + 32u * m), fin, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}
// A wave with no path: poll (the host word through the ticket) and wait until a unit is posted (returns 0: refill) or
// it may leave (1): the stop flag in its view and nothing posted left to claim.  A wave that saw nothing new posted for
// sv_idle_ticks closes the server (sv_close); it never leaves on its own clock.
__device__ uint32_t sv_wait(const HgKernelParams& kp) {
    hg_wave_cost[threadIdx.x >> 6] = nullptr;  // the wait is no tile's cost
    uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint32_t seen = HG_NONE;  // the view at which the heads were last read
    uint32_t idle_view = lds_get(hg_sv.view);  // the view at t0 (a new post restarts the idle clock)
    for (uint32_t spin = 0;; ++spin) {
        // one coherent load per spin (this wave's mirror copy); the host word through the ticket every few spins
        const uint32_t view = (spin % HG_SV_POLL_EVERY) == 0u ? sv_poll(kp) : sv_view(kp);
        // A wave holding a unit (claimed past the posted ones by a race with another claimer, or with its frame
        // window busy) claims nothing else until it is placed: it waits for that unit alone.  (No wave set can end
        // up all holding unposted units while posted ones remain: the last claimer's overshoot needs a concurrent
        // claimer, which then holds none.)
        const uint32_t pend = lds_get(hg_sv.pend);
        bool open = pend != HG_NONE && pend < view;
        if (pend == HG_NONE && view != seen) {  // the heads, only when the posted units changed
            seen = view;
            for (uint32_t h = 0; h < 8u && !open; ++h) open = h + 8u * ld_agent(kp.queue + 32u * h) < view;
        }
        if (open) {
            lds_put(hg_sv.dry, HG_NONE);
            return 0u;
        }
        if (lds_get(hg_sv.stop)) return 1u;  // the final post word: nothing posted is left to claim
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (view != idle_view) {
            idle_view = view;
            t0 = now;
        } else if (now - t0 > uint64_t(lds_get(hg_sv.idle_ticks))) {
            sv_close(kp);  // (then the stop flag reaches this wave's view through the mirrors)
        }
        // short sleeps between the first polls, then longer ones (s_sleep counts 64 clocks)
        if (spin < HG_SV_SPIN_SHORT) __builtin_amdgcn_s_sleep(HG_SV_SLEEP_SHORT);
        else __builtin_amdgcn_s_sleep(HG_SV_SLEEP_LONG);
    }
}
// (the colour stores of a server frame: fc_store into the uncached ring)
