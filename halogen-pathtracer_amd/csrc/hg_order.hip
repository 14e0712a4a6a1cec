// hg_order.hip — the tile cost sort of the regenerating and streaming kernels' cost-ordered dispatch.  A translation
// unit of its own: it shares nothing with the trace kernels but the costs their waves record (hg_sched.h).
#include <hip/hip_runtime.h>

#include "hg_items.h"
#include "hg_launch.h"

// Cost order (hg_render, per trace stream): tile_order = the local tiles, most expensive first, then the costs are
// cleared for the next launches.  A counting sort over 1024 log-scale cost buckets (hg_order_bucket, hg_items.h: 16 per
// octave of the wave-clock cost; two tiles share one only within ~4 % of each other), in two launches of one-wave
// workgroups (1,024 tiles each) with 8-12 KB of LDS and few registers, so that they fit on CUs beside the persistent
// trace waves of the other streams (round 3's single 1,024-thread, 36-KB workgroup waited for a whole CU to drain:
// ~1 ms per sort at the one-dispatch-per-frame operating point):
//   hg_order_hist     each workgroup histograms its tiles in LDS and adds the counts to the global histogram;
//   hg_order_scatter  each workgroup derives the buckets' starts (exclusive prefix of the global histogram), claims its
//                     share of every bucket with one global atomic per (workgroup, bucket) and places its tiles there;
//                     the last workgroup to finish clears the histogram and the claims for the next sort.
// Within a bucket the order is not tile-index order (it depends on which workgroup claims first): no result depends on
// the order (tiles are independent), only the drain tail.  The order is a permutation of the tiles whenever the costs
// hold still during the sort (the runtime sorts a stream's own costs on that stream); HG_CHECK_EXEC builds also verify
// that (hg_order_verify) and count every placement out of range into hg_counters.order_faults.
struct HgOrderScratch {  // per trace stream, zeroed at allocation; every sort leaves it zeroed again
    uint32_t hist[1024];   // tiles per bucket
    uint32_t claim[1024];  // tiles per bucket claimed by workgroups so far
    uint32_t done;         // workgroups of the scatter launch finished
    uint32_t pad[31];
};
static_assert(sizeof(HgOrderScratch) == 8320, "order scratch");
constexpr uint32_t kOrderTilesPerGroup = 1024;

__global__ __launch_bounds__(64) void hg_order_hist(const unsigned long long* __restrict__ cost, uint32_t n,
                                                    HgOrderScratch* __restrict__ sc) {
    __shared__ uint32_t h[1024];
    const uint32_t t = threadIdx.x, base = blockIdx.x * kOrderTilesPerGroup;
    for (uint32_t b = t; b < 1024u; b += 64u) h[b] = 0u;
    __syncthreads();
    for (uint32_t k = t; k < kOrderTilesPerGroup && base + k < n; k += 64u) atomicAdd(&h[hg_order_bucket(cost[base + k])], 1u);
    __syncthreads();
    for (uint32_t b = t; b < 1024u; b += 64u)
        if (h[b]) atomicAdd(&sc->hist[b], h[b]);
}

__global__ __launch_bounds__(64) void hg_order_scatter(unsigned long long* __restrict__ cost, uint32_t* __restrict__ order,
                                                       uint32_t n, HgOrderScratch* __restrict__ sc,
                                                       unsigned long long* __restrict__ faults) {
    __shared__ uint32_t pos[1024];  // bucket -> next place of this workgroup's tiles
    __shared__ uint32_t cnt[1024];  // bucket -> this workgroup's tiles
    const uint32_t t = threadIdx.x, base = blockIdx.x * kOrderTilesPerGroup;
    // exclusive prefix of the global histogram: lane t sums buckets [16t, 16t + 16), a wave scan of the 64 sums
    uint32_t run = 0;
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t v = __hip_atomic_load(&sc->hist[16u * t + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pos[16u * t + j] = run;
        run += v;
    }
    uint32_t incl = run;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (t >= d) incl += o;
    }
    const uint32_t excl = incl - run;
    for (uint32_t j = 0; j < 16u; ++j) {
        pos[16u * t + j] += excl;
        cnt[16u * t + j] = 0u;
    }
    __syncthreads();
    for (uint32_t k = t; k < kOrderTilesPerGroup && base + k < n; k += 64u) atomicAdd(&cnt[hg_order_bucket(cost[base + k])], 1u);
    __syncthreads();
    for (uint32_t b = t; b < 1024u; b += 64u)  // this workgroup's share of bucket b
        if (cnt[b]) pos[b] += atomicAdd(&sc->claim[b], cnt[b]);
    __syncthreads();
    uint32_t bad = 0;
    for (uint32_t k = t; k < kOrderTilesPerGroup && base + k < n; k += 64u) {
        const uint32_t i = base + k;
        const uint32_t p = atomicAdd(&pos[hg_order_bucket(cost[i])], 1u);
        if (p < n) order[p] = i;  // always, while the costs hold still during the sort
        else ++bad;
        cost[i] = 0ull;
    }
#if HG_CHECK_EXEC
    if (bad && faults) atomicAdd(faults, (unsigned long long)bad);
#else
    (void)bad;
    (void)faults;
#endif
    __syncthreads();
    // the last workgroup out clears the histogram and the claims (every other one has read them: release / acquire)
    uint32_t last = 0;
    if (t == 0)
        last = __hip_atomic_fetch_add(&sc->done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
    last = __builtin_amdgcn_readfirstlane(last);
    if (last) {
        for (uint32_t b = t; b < 1024u; b += 64u) {
            __hip_atomic_store(&sc->hist[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&sc->claim[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (t == 0) __hip_atomic_store(&sc->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#if HG_CHECK_EXEC
// HG_CHECK_EXEC builds: the order must be a permutation of [0, n).  seen[] (n words, zero) counts each tile's places;
// the second kernel counts tiles placed other than once into *faults and zeroes seen[] again.
__global__ __launch_bounds__(64) void hg_order_verify_mark(const uint32_t* __restrict__ order, uint32_t n,
                                                           uint32_t* __restrict__ seen,
                                                           unsigned long long* __restrict__ faults) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = order[i];
    if (v < n) atomicAdd(&seen[v], 1u);
    else atomicAdd(faults, 1ull);
}
// HG_CHECK_EXEC builds: words that every use leaves zeroed (the sort's histogram / claims / done count, a queue
// launch's heads and exit count) must read zero when the next use starts; each that does not counts into *faults
__global__ __launch_bounds__(64) void hg_check_zeroed(const uint32_t* __restrict__ p, uint32_t n,
                                                      unsigned long long* __restrict__ faults) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n && p[i] != 0u) atomicAdd(faults, 1ull);
}
__global__ __launch_bounds__(64) void hg_order_verify_count(uint32_t n, uint32_t* __restrict__ seen,
                                                            unsigned long long* __restrict__ faults) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    if (seen[i] != 1u) atomicAdd(faults, 1ull);
    seen[i] = 0u;
}
#endif

// HG_CHECK_EXEC builds only (nothing otherwise): count the nonzero words of p[0, n) into *faults
void hg_launch_check_zeroed(const uint32_t* p, uint32_t n, unsigned long long* faults, hipStream_t stream) {
#if HG_CHECK_EXEC
    hipLaunchKernelGGL(hg_check_zeroed, dim3((n + 63u) / 64u), dim3(64), 0, stream, p, n, faults);
#else
    (void)p, (void)n, (void)faults, (void)stream;
#endif
}

size_t hg_order_scratch_bytes(uint32_t n) {
    return sizeof(HgOrderScratch) + (HG_CHECK_EXEC ? size_t(n) * sizeof(uint32_t) : 0);
}

// scratch: hg_order_scratch_bytes(n) bytes, zeroed when allocated; faults: hg_counters.order_faults (check builds)
hipError_t hg_launch_order_tiles(unsigned long long* cost, uint32_t* order, uint32_t n, void* scratch,
                                 unsigned long long* faults, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    HgOrderScratch* sc = static_cast<HgOrderScratch*>(scratch);
    const dim3 g{(n + kOrderTilesPerGroup - 1) / kOrderTilesPerGroup};
    if (faults) hg_launch_check_zeroed(static_cast<const uint32_t*>(scratch), 2049u, faults, stream);
    hipLaunchKernelGGL(hg_order_hist, g, dim3(64), 0, stream, cost, n, sc);
    hipLaunchKernelGGL(hg_order_scatter, g, dim3(64), 0, stream, cost, order, n, sc, faults);
#if HG_CHECK_EXEC
    uint32_t* seen = reinterpret_cast<uint32_t*>(sc + 1);
    hipLaunchKernelGGL(hg_order_verify_mark, dim3((n + 63) / 64), dim3(64), 0, stream, order, n, seen, faults);
    hipLaunchKernelGGL(hg_order_verify_count, dim3((n + 63) / 64), dim3(64), 0, stream, n, seen, faults);
#endif
    return hipGetLastError();
}
