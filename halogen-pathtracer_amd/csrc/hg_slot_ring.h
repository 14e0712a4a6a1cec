// hg_slot_ring.h — the ring of display readback slots (hg_ctx::slots, HG_OPT_READBACK_DEPTH): which slot the next begin
// fills and which begun readback is the oldest.  No HIP: tests/test_launch_plan.py compiles it with g++.  Every index
// computation of the ring is here.
#pragma once

struct HgSlotRing {
    int depth = 2;    // slots in use: readbacks that may be outstanding
    int next = 0;     // the slot the next begin fills: the one after the newest, so never an outstanding one
    int pending = 0;  // begun readbacks not yet ended (<= depth)

    bool full() const { return pending >= depth; }
    int begin() {  // (not full) the slot filled; the next begin fills the one after it
        const int k = next;
        next = (k + 1) % depth;
        pending++;
        return k;
    }
    int oldest() const { return (next - pending + depth) % depth; }  // (pending > 0) the oldest begun
    int end() {  // (pending > 0) the oldest begun, no longer outstanding
        const int k = oldest();
        pending--;
        return k;
    }
    void reset() { next = pending = 0; }  // every begun readback is dropped
    void set_depth(int d) {  // (pending == 0)
        depth = d;
        next = 0;
    }
};
