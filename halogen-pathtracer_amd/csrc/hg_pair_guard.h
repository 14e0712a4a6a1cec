// hg_pair_guard.h — scope guard of a timing event pair taken from a context's free list (hg_runtime.hip event_pair).
// The pair goes back to the free list when the guard dies, unless it was handed to a list that drain_events reads
// (pending, pending_trace): so no return between taking a pair and queueing it, an HG_HIP return included, leaks one.
// A template over the pair type, so that tests/test_launch_plan.py compiles it with a stub in place of hipEvent_t.
#pragma once
#include <vector>

template <class Pair>
class HgPairGuard {
public:
    explicit HgPairGuard(std::vector<Pair>& free_list) : free_(free_list) {}
    HgPairGuard(const HgPairGuard&) = delete;
    HgPairGuard& operator=(const HgPairGuard&) = delete;
    ~HgPairGuard() { hand_to(free_); }
    void hold(const Pair& p) {  // (a pair already held goes back first)
        hand_to(free_);
        pair = p;
        held_ = true;
    }
    bool held() const { return held_; }
    void hand_to(std::vector<Pair>& list) {  // at most once per pair held: later calls do nothing
        if (held_) list.push_back(pair);
        held_ = false;
    }
    Pair pair{};

private:
    std::vector<Pair>& free_;
    bool held_ = false;
};
