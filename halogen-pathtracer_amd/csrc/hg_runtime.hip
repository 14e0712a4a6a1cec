// hg_runtime.hip — implementation of the C-ABI in include/halogen_abi.h (context, uploads, dispatch,
// readback, counters).  Stands in for the ComputeBuffer / RTHandle / DispatchCompute / Blit calls of
// Assets/Scripts/Render Features/HalogenRenderPass.cs (RP:237-508).
//
// Error model: every entry point returns HG_OK or a negative HG_E_* code and never aborts; the text of
// the last error is kept per context (hg_last_error).  There is no CPU fallback: a missing GPU or a HIP
// failure is an error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "halogen_abi.h"
#include "hg_fmath.h"
#include "hg_layout.h"
#include "hg_ctx.h"
#include "hg_tiling.h"
#include "hg_interval.h"
#include "hg_pack.h"
#include "hg_atrous.h"
#include "hg_scene_pack.h"
#include "hg_pair_guard.h"
#include "hg_plan.h"

hipError_t hg_launch_mega(const HgKernelParams& kp, int block, bool counters, hipStream_t stream);
hipError_t hg_launch_mega_regen(const HgKernelParams& kp, int block, bool counters, hipStream_t stream);
hipError_t hg_launch_mega_stream(const HgKernelParams& kp, int block, bool counters, hipStream_t stream,
                                 bool server = false);
hipError_t hg_launch_server_frame(float4* acc, const float4* colors, uint32_t n_slots, int32_t frame_count,
                                  const uint32_t* done, uint32_t target, uint64_t timeout_ticks,
                                  const unsigned long long* exitw, uint32_t* lost, unsigned long long* err,
                                  uint32_t epoch, hipStream_t stream);
hipError_t hg_launch_blend_frames(const HgKernelParams& kp, const uint32_t* lost, hipStream_t stream);
hipError_t hg_launch_order_tiles(unsigned long long* cost, uint32_t* order, uint32_t n, void* scratch,
                                 unsigned long long* faults, hipStream_t stream);
size_t hg_order_scratch_bytes(uint32_t n);
int64_t hg_selftest_rcp_all(int64_t* tested);

namespace {

using EventPair = std::pair<hipEvent_t, hipEvent_t>;
using EventGuard = HgPairGuard<EventPair>;  // a timing pair that goes back to free_events unless handed on

// hg_scene_pack.h packs with HIP's vector types here and with its own plain structs under g++ (its tests): the same bytes
#ifdef HG_VECTOR_SHIM
#error "hg_scene_pack.h defined its float4 / uint2 shim in a HIP translation unit"
#endif
static_assert(sizeof(float4) == HG_FLOAT4_BYTES && alignof(float4) == HG_FLOAT4_BYTES, "float4 differs from the shim");
static_assert(sizeof(uint2) == HG_UINT2_BYTES && alignof(uint2) == HG_UINT2_BYTES, "uint2 differs from the shim");
static_assert(sizeof(HgDevMesh) == 144 && alignof(HgDevMesh) == 16, "HgDevMesh is 144 B (hg_layout.h)");

}  // namespace

namespace {

int fail(hg_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HG_HIP(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail((ctx), HG_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

int set_device(hg_ctx* c) {
    HG_HIP(c, hipSetDevice(c->device));
    return HG_OK;
}

void release(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

int upload(hg_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    size_t alloc = std::max<size_t>(bytes, 16);  // the reference allocates >= 1 element (RP:544)
    if (b.bytes != alloc) {
        release(b);
        hipError_t e = hipMalloc(&b.p, alloc);
        if (e != hipSuccess) return fail(c, HG_E_NOMEM, "hipMalloc(%zu) failed: %s", alloc, hipGetErrorString(e));
        b.bytes = alloc;
    }
    if (bytes) HG_HIP(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return HG_OK;
}

int drain_events(hg_ctx* c) {
    if (c->pending.empty() && c->pending_trace.empty()) return HG_OK;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    for (auto& pr : c->pending) {
        float ms = 0.0f;
        HG_HIP(c, hipEventElapsedTime(&ms, pr.first, pr.second));
        c->counters.kernel_ms += double(ms);
        c->free_events.push_back(pr);
    }
    // the launches' intervals relative to the first one pushed (which need not be the first to start: offsets can be
    // negative; the trace streams' events share the device clock); the batch ends at a synchronisation, so batches do
    // not overlap one another
    std::vector<std::pair<double, double>> iv;
    iv.reserve(c->pending_trace.size());
    for (auto& pr : c->pending_trace) {
        float ms = 0.0f, a = 0.0f;
        HG_HIP(c, hipEventElapsedTime(&ms, pr.first, pr.second));
        HG_HIP(c, hipEventElapsedTime(&a, c->pending_trace.front().first, pr.first));
        iv.emplace_back(double(a), double(a) + double(ms));
        c->counters.trace_ms += double(ms);
        c->counters.trace_launches++;
    }
    const double covered = hg_interval_union(std::move(iv));
    c->counters.trace_busy_ms += covered;
    for (auto& pr : c->pending_trace) c->free_events.push_back(pr);
    c->pending.clear();
    c->pending_trace.clear();
    return HG_OK;
}

int event_pair(hg_ctx* c, EventGuard& g) {
    EventPair ev;
    if (!c->free_events.empty()) {
        ev = c->free_events.back();
        c->free_events.pop_back();
    } else {
        HG_HIP(c, hipEventCreate(&ev.first));
        HG_HIP(c, hipEventCreate(&ev.second));
    }
    g.hold(ev);
    return HG_OK;
}

int ensure(hg_ctx* c, DevBuf& b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (b.bytes >= bytes) return HG_OK;
    release(b);
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(c, HG_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    b.bytes = bytes;
    return HG_OK;
}

// The same in uncached device memory (MTYPE UC: no L2 holds its lines, so writes from one XCD are seen by loads from
// any other without cache maintenance): the render server's colour ring and frame counts, written by persistent
// waves and read by the gate and blend kernels while those waves still run
int ensure_uncached(hg_ctx* c, DevBuf& b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (b.bytes >= bytes) return HG_OK;
    release(b);
    hipError_t e = hipExtMallocWithFlags(&b.p, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess)
        return fail(c, HG_E_NOMEM, "hipExtMallocWithFlags(%zu, uncached) failed: %s", bytes, hipGetErrorString(e));
    b.bytes = bytes;
    return HG_OK;
}

double host_seconds() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the render server (hg_ctx::Server; device side hg_mega.hip kServer) ------------------------------------------
// The server closes itself after HG_OPT_SERVER_IDLE_US with nothing posted (the close handshake, hg_mega.hip sv_close:
// no host clock is involved in whether a post is taken).  A frame's gate gives up after 30 s, or at once when every
// wave of the server has left with the frame's count short: the frame is lost (reported, the accumulator invalid).
constexpr uint64_t kGateTimeoutTicks = 30ull * 100000000ull;  // 100-MHz s_memrealtime
// HG_OPT_SERVER_GATE_US, else HALOGEN_SERVER_GATE_TIMEOUT_MS (diagnostics: a shorter bound turns a stuck frame into an
// error fast), else 30 s
uint64_t gate_timeout_ticks(const hg_ctx* c) {
    if (c->sv.gate_us >= 0) return uint64_t(c->sv.gate_us) * 100ull;
    static const uint64_t t = [] {
        const char* e = std::getenv("HALOGEN_SERVER_GATE_TIMEOUT_MS");
        const long long ms = e ? std::atoll(e) : 0;
        return ms > 0 ? uint64_t(ms) * 100000ull : kGateTimeoutTicks;
    }();
    return t;
}

// HALOGEN_SERVER_TRACE=1: every server start, stop, post and refusal on stderr (diagnostics)
void sv_trace(const char* fmt, ...) {
    static const bool on = std::getenv("HALOGEN_SERVER_TRACE") != nullptr;
    if (!on) return;
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "[hg server %.6f] ", host_seconds());
    std::vfprintf(stderr, fmt, ap);
    std::fputc('\n', stderr);
    va_end(ap);
}

// A lost server frame, as its gate reported it in the host's lost-frame word (HG_SV_LOST | the accumulator epoch of the
// frame): the accumulator is invalid if the frame belongs to the current accumulation (a clear, a checkpoint load or a
// reallocation since has discarded it otherwise)
void server_note_lost(hg_ctx* c) {
    if (!c->sv.host) return;
    const unsigned long long w = __atomic_exchange_n(&c->sv.host[HG_SV_HOST_LOST], 0ull, __ATOMIC_SEQ_CST);
    if (!(w & HG_SV_LOST)) return;
    c->frames_lost++;
    sv_trace("a frame of accumulator epoch %u was lost (current epoch %u)", uint32_t(w), c->acc_epoch);
    if (uint32_t(w) == c->acc_epoch) c->acc_lost = true;
}
// The error of every entry point that renders into or reads the accumulator while it is invalid
int lost_check(hg_ctx* c) {
    server_note_lost(c);
    if (!c->acc_lost) return HG_OK;
    return fail(c, HG_E_FRAME_LOST, "a render server frame was lost (its gate gave up before the frame completed): the "
                                    "accumulation is invalid until hg_clear_accumulation or hg_set_accumulation");
}
// A new accumulation (clear, checkpoint load, reallocation), on the context stream after everything before it: lost
// frames before it no longer matter, and the blends after it run again
int reset_lost(hg_ctx* c) {
    server_note_lost(c);
    c->acc_epoch++;
    c->acc_lost = false;
    HG_HIP(c, hipMemsetAsync(c->lost.p, 0, sizeof(uint32_t), c->stream));
    return HG_OK;
}

// Stop the server: set the stop flag, the waves drain every frame posted and leave; wait (bounded) for the kernel.
int server_stop(hg_ctx* c) {
    hg_ctx::Server& S = c->sv;
    if (!S.running) return HG_OK;
    // the stop word carries the frames the host asked for: frames posted ahead of the calls (server_speculate) and not
    // yet claimed are abandoned (the waves' view drops to it, hg_mega.hip sv_view)
    __atomic_store_n(&S.host[HG_SV_HOST_POST], static_cast<unsigned long long>(S.committed) | HG_SV_STOP, __ATOMIC_SEQ_CST);
    const double t0 = host_seconds();
    sv_trace("stop: %u frames committed, %u posted", S.committed, S.posted);
    hipError_t q;
    while ((q = hipStreamQuery(S.stream)) == hipErrorNotReady) {
        if (host_seconds() - t0 > 60.0) {
            (void)hipGetLastError();
            return fail(c, HG_E_HIP, "render server did not stop within 60 s");
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    (void)hipGetLastError();  // hipErrorNotReady is a status here
    S.running = false;
    sv_trace("stopped after %.3f ms (%s)", (host_seconds() - t0) * 1e3, hipGetErrorString(q));
#if HG_SV_DIAG_TIMES
    {  // (analysis builds) per frame: first claim and last count on the device clock (10 ns), host post time
        std::vector<unsigned long long> d(512);
        if (hipMemcpy(d.data(), static_cast<char*>(S.ctl.p) + HG_SV_DIAG_WORD * 4u, d.size() * 8u,
                      hipMemcpyDeviceToHost) == hipSuccess) {
            const unsigned long long t00 = ~d[0];
            for (uint32_t k = 0; k < std::min<uint32_t>(S.posted, 256u); ++k)
                sv_trace("frame %u: posted %+.3f ms (host), first claim %+.3f ms, last count %+.3f ms (device)", k,
                         (S.post_s[k] - S.post_s[0]) * 1e3, double(~d[2 * k] - t00) * 1e-5,
                         double(d[2 * k + 1] - t00) * 1e-5);
        }
    }
#endif
    if (q != hipSuccess) return fail(c, HG_E_HIP, "render server: %s", hipGetErrorString(q));
    return HG_OK;
}

// Wait for every stream of the context: the context stream and both trace streams (before device buffers that a
// trace in flight may read are changed or freed); the render server is stopped first
int quiesce(hg_ctx* c) {
    if (int rc = server_stop(c)) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    if (c->rb_stream) HG_HIP(c, hipStreamSynchronize(c->rb_stream));
    for (hg_ctx::TraceLane& L : c->lanes)
        if (L.stream) HG_HIP(c, hipStreamSynchronize(L.stream));
    return HG_OK;
}

// Grow a trace stream's buffer; only when that buffer is not in use (quiesce first if it must move)
int ensure_quiet(hg_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= std::max<size_t>(bytes, 16)) return HG_OK;
    if (int rc = quiesce(c)) return rc;
    return ensure(c, b, bytes);
}

// The cost order of a trace stream or of the render server (`o`: its tile_cost, tile_order, order_scratch and stream).
// Two steps, because a call grows every trace stream's buffers before it queues its first chunk and sorts per chunk.
// Grow: with `grow` (ensure, or ensure_quiet while traces may be in flight); the sort's scratch is zeroed once, when
// allocated (each use leaves it zeroed).
template <class Owner>
int cost_order_ensure(hg_ctx* c, Owner& o, uint32_t tiles, int (*grow)(hg_ctx*, DevBuf&, size_t)) {
    const size_t tb = size_t(tiles) * sizeof(uint32_t);
    if (int rc = grow(c, o.tile_cost, 2 * tb)) return rc;
    if (int rc = grow(c, o.tile_order, tb)) return rc;
    const size_t osb = hg_order_scratch_bytes(tiles);
    if (o.order_scratch.bytes >= osb) return HG_OK;
    if (int rc = grow(c, o.order_scratch, osb)) return rc;
    if (hipMemsetAsync(o.order_scratch.p, 0, o.order_scratch.bytes, o.stream) != hipSuccess)
        return fail(c, HG_E_HIP, "hipMemsetAsync(order scratch) failed");
    return HG_OK;
}
// Use: sort the recorded costs into the order (`sort`), or zero the costs before their first records
template <class Owner>
hipError_t cost_order_run(hg_ctx* c, Owner& o, uint32_t tiles, bool sort) {
    unsigned long long* cost = static_cast<unsigned long long*>(o.tile_cost.p);
    if (!sort) return hipMemsetAsync(cost, 0, size_t(tiles) * sizeof(unsigned long long), o.stream);
    return hg_launch_order_tiles(cost, static_cast<uint32_t*>(o.tile_order.p), tiles, o.order_scratch.p,
                                 static_cast<unsigned long long*>(c->counters_dev.p) + 18, o.stream);
}

int alloc_target(hg_ctx* c) {
    if (int rc = quiesce(c)) return rc;
    c->tiles_x = (c->W + HG_TILE - 1) / HG_TILE;
    c->tiles_y = (c->H + HG_TILE - 1) / HG_TILE;
    const int64_t total = int64_t(c->tiles_x) * c->tiles_y;
    c->n_local_tiles = total > c->rank ? int32_t((total - c->rank + c->n_ranks - 1) / c->n_ranks) : 0;
    for (hg_ctx::TraceLane& L : c->lanes) {
        L.tile_cost_valid = false;
        L.tile_order_valid = false;
        L.frames_since_order = 0;
    }
    c->sv.tile_cost_valid = false;  // (its buffer may be reallocated, or hold the old tiling's costs)
    if (int rc = reset_lost(c)) return rc;
    const size_t bytes = size_t(c->n_local_tiles) * 64 * sizeof(float4);
    c->rb_pending = 0;  // quiesced: begun readbacks are complete, and their images die with the old size or tiling
    c->rb_next = 0;
    release(c->acc);
    if (bytes) {
        hipError_t e = hipMalloc(&c->acc.p, bytes);
        if (e != hipSuccess) return fail(c, HG_E_NOMEM, "hipMalloc(accumulation %zu) failed", bytes);
        c->acc.bytes = bytes;
        HG_HIP(c, hipMemsetAsync(c->acc.p, 0, bytes, c->stream));
    }
    return HG_OK;
}


}  // namespace

extern "C" {

namespace {
// A trace stream (HG_LANE_STREAMS).  Plain streams share HIP's pool of GPU_MAX_HW_QUEUES (4) hardware queues with every
// other stream of the process; two trace streams on one queue serialise their launches.
hipError_t create_lane_stream(const hg_ctx* c, int lane, hipStream_t* s) {
    if (lane < HG_TRACE_LANES_BIG) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    std::vector<uint32_t> mask(size_t((c->n_cu + 31) / 32), 0u);
    for (int i = 0; i < c->n_cu; ++i) mask[size_t(i) / 32] |= 1u << (i % 32);
    // (CU-masked streams are blocking with respect to the legacy null stream, unlike the plain ones.)  Where the
    // runtime refuses CU masks, a plain stream: the same results, only the queue sharing above comes back.
    if (hipExtStreamCreateWithCUMask(s, uint32_t(mask.size()), mask.data()) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
}  // namespace

int hg_abi_version(void) { return HG_ABI_VERSION; }

int hg_create(int device, hg_ctx** out) {
    if (!out) return HG_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return HG_E_HIP;
    if (device < 0 || device >= n) return HG_E_INVALID;
    hg_ctx* c = new hg_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->call_done[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->call_done[1], hipEventDisableTiming) != hipSuccess ||
        hipMalloc(&c->counters_dev.p, 32 * sizeof(unsigned long long)) != hipSuccess) {
        delete c;
        return HG_E_HIP;
    }
    c->counters_dev.bytes = 32 * sizeof(unsigned long long);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        delete c;
        return HG_E_HIP;
    }
    c->n_cu = prop.multiProcessorCount;
    if (ensure_uncached(c, c->lost, 128) != HG_OK || hipMemset(c->lost.p, 0, 128) != hipSuccess ||
        hipMemset(c->counters_dev.p, 0, c->counters_dev.bytes) != hipSuccess) {
        hg_destroy(c);
        return HG_E_HIP;
    }
    for (int li = 0; li < HG_TRACE_LANES; ++li) {
        hg_ctx::TraceLane& L = c->lanes[li];
        if (create_lane_stream(c, li, &L.stream) != hipSuccess ||
            hipEventCreateWithFlags(&L.traced, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.blended, hipEventDisableTiming) != hipSuccess) {
            hg_destroy(c);
            return HG_E_HIP;
        }
    }
    *out = c;
    return HG_OK;
}

void hg_destroy(hg_ctx* c) {
    if (!c) return;
    c->pending_frames = 0;  // held frames are discarded: nothing can observe them after this call
    (void)hipSetDevice(c->device);
    (void)server_stop(c);
    sv_trace("destroy: server stopped");
    if (std::getenv("HALOGEN_SERVER_TRACE")) {
        unsigned long long w[4] = {};
        if (c->sv.ctl.p && hipMemcpyAsync(w, static_cast<char*>(c->sv.ctl.p) + HG_SV_EXIT_WORD * 4u, sizeof w,
                                          hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
            hipStreamSynchronize(c->stream) == hipSuccess)
            sv_trace("destroy: server waves out %llu of %llu", w[0] & 0xFFFFFFFFull, w[0] >> 32);
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    sv_trace("destroy: context stream idle");
    for (hg_ctx::TraceLane& L : c->lanes)
        if (L.stream) (void)hipStreamSynchronize(L.stream);
    for (DevBuf* b : {&c->spheres, &c->meshes, &c->materials, &c->nodes, &c->leaves, &c->tris, &c->normals, &c->cube,
                      &c->acc, &c->counters_dev, &c->spill, &c->lost, &c->query_in, &c->query_out, &c->guide0,
                      &c->guide1, &c->denoise_work[0], &c->denoise_work[1]})
        release(*b);
    auto destroy_lanes = [c] {
        for (hg_ctx::TraceLane& L : c->lanes) {
            for (DevBuf* b : {&L.frame_color, &L.spill, &L.tile_cost, &L.tile_order, &L.order_scratch, &L.queue})
                release(*b);
            if (L.traced) (void)hipEventDestroy(L.traced);
            if (L.blended) (void)hipEventDestroy(L.blended);
            sv_trace("destroy: lane stream %p", static_cast<void*>(L.stream));
            if (L.stream) (void)hipStreamDestroy(L.stream);
        }
        sv_trace("destroy: trace streams destroyed");
    };
    // (analysis builds, HG_DIAG_TEARDOWN: HALOGEN_DIAG_TEARDOWN=server_first[,bufs_last][,host_last][,events_last]
    // destroys the server's stream before the trace streams, the order that hung in round 5, and defers the named
    // server resources past every stream destroy: tools/gpu_teardown.sh)
    bool server_first = false, bufs_last = false, host_last = false, events_last = false;
#if HG_DIAG_TEARDOWN
    if (const char* td = std::getenv("HALOGEN_DIAG_TEARDOWN")) {
        server_first = std::strstr(td, "server_first") != nullptr;
        bufs_last = std::strstr(td, "bufs_last") != nullptr;
        host_last = std::strstr(td, "host_last") != nullptr;
        events_last = std::strstr(td, "events_last") != nullptr;
    }
#endif
    hg_ctx::Server& S = c->sv;
    auto server_bufs = [&S] {
        for (DevBuf* b : {&S.ctl, &S.done, &S.ring, &S.spill, &S.tile_cost, &S.tile_order, &S.order_scratch}) release(*b);
        sv_trace("destroy: server buffers freed");
    };
    auto server_events = [&S] {
        for (hipEvent_t& e : S.blended)
            if (e) (void)hipEventDestroy(e);
        if (S.exited) (void)hipEventDestroy(S.exited);
        sv_trace("destroy: server events destroyed");
    };
    auto server_host = [&S] {
        if (S.host) (void)hipHostFree(S.host);
        sv_trace("destroy: server host word freed");
    };
    auto destroy_server = [&] {
        if (S.stream) (void)hipStreamSynchronize(S.stream);
        sv_trace("destroy: server stream idle");
        if (!bufs_last) server_bufs();
        if (!events_last) server_events();
        if (!host_last) server_host();
        if (S.stream) (void)hipStreamDestroy(S.stream);
        sv_trace("destroy: server stream destroyed");
    };
    // The server's stream after the trace streams: destroyed before them, the next hipStreamDestroy of a plain trace
    // stream hung in round 5 (DESIGN.md section 4.7 has what the analysis build found)
    if (server_first) destroy_server();
    destroy_lanes();
    if (!server_first) destroy_server();
    if (bufs_last) server_bufs();
    if (events_last) server_events();
    if (host_last) server_host();
    if (c->rb_stream) (void)hipStreamSynchronize(c->rb_stream);
    release(c->image);
    for (int k = 0; k < HG_READBACK_MAX; ++k) {
        release(c->rb_image[k]);
        if (c->rb_untiled[k]) (void)hipEventDestroy(c->rb_untiled[k]);
        if (c->image_host[k]) (void)hipHostFree(c->image_host[k]);
        if (c->image_copied[k]) (void)hipEventDestroy(c->image_copied[k]);
    }
    if (c->rb_stream) (void)hipStreamDestroy(c->rb_stream);
    for (auto& pr : c->pending_trace) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : c->pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : c->free_events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t e : c->call_done)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    sv_trace("destroy: done");
    delete c;
}

const char* hg_last_error(const hg_ctx* c) { return c ? c->err.c_str() : "null context"; }

int hg_upload_scene(hg_ctx* c, const HalogenSphere* spheres, int32_t n_spheres, const HalogenMeshData* meshes,
                    int32_t n_meshes, const PackedHalogenMaterial* materials, int32_t n_materials,
                    const HalogenTriangle* tris, int32_t n_tris, const BVHEntry* blas, int32_t n_nodes) {
    return hg_upload_scene_gen(c, 0, spheres, n_spheres, meshes, n_meshes, materials, n_materials, tris, n_tris, blas,
                               n_nodes);
}

namespace {

int fail(hg_ctx* c, const HgPackError& err) { return fail(c, err.code, "%s", err.text.c_str()); }

// The bookkeeping of an upload whose device copies are on the stream: the retained host copies the next upload compares
// against (made while the device copies run), the mesh table a partial re-upload starts from, counters and counts
int commit_scene(hg_ctx* c, const HgSceneIn& in, HgScenePack& pack, HgUploadDecision d, uint64_t geometry_generation) {
    const bool partial = d.kind == HG_UPLOAD_PARTIAL;
    for (int k = 0; k < (partial ? 3 : 5); ++k) copy_bytes(c->scene_copy[k], in.src(k), in.bytes(k));
    HG_HIP(c, hipStreamSynchronize(c->stream));  // host staging vectors die at return
    c->dev_meshes.swap(pack.dm);
    c->scene_uploads++;
    if (partial) {
        c->scene_uploads_partial++;
        c->scene_uploads_vouched += d.vouched ? 1u : 0u;
    } else {
        c->stack_depth = pack.stack_depth;
        c->n_tris = in.n_tris;
        c->n_nodes = in.n_nodes;
    }
    c->geometry_gen = geometry_generation;
    c->n_spheres = in.n_spheres;
    c->n_meshes = in.n_meshes;
    c->n_materials = in.n_materials;
    c->has_scene = true;
    return HG_OK;
}

}  // namespace

// Decision, validation and layout are hg_scene_pack.h's (no HIP; tested on the CPU); here the device and the context.
// A rejection of the spheres, or of anything in a partial re-upload, leaves the previous scene in place; a rejection in
// the mesh / BLAS checks of a full rebuild leaves the context without a scene.
int hg_upload_scene_gen(hg_ctx* c, uint64_t geometry_generation, const HalogenSphere* spheres, int32_t n_spheres,
                        const HalogenMeshData* meshes, int32_t n_meshes, const PackedHalogenMaterial* materials,
                        int32_t n_materials, const HalogenTriangle* tris, int32_t n_tris, const BVHEntry* blas,
                        int32_t n_nodes) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (n_spheres < 0 || n_meshes < 0 || n_materials < 0 || n_tris < 0 || n_nodes < 0)
        return fail(c, HG_E_INVALID, "negative count");
    if ((n_spheres && !spheres) || (n_meshes && !meshes) || (n_materials && !materials) || (n_tris && !tris) ||
        (n_nodes && !blas))
        return fail(c, HG_E_INVALID, "null array with non-zero count");
    const HgSceneIn in{spheres, n_spheres, meshes, n_meshes, materials, n_materials, tris, n_tris, blas, n_nodes};
    HgPackError err;
    if (hg_scene_check_limits(in, err)) return fail(c, err);
    const HgUploadDecision d = hg_upload_decide(c->has_scene, c->scene_copy, c->geometry_gen, c->dev_meshes.size(), in,
                                                geometry_generation);
    if (d.kind == HG_UPLOAD_SKIP) {
        c->scene_uploads_skipped++;
        c->scene_uploads_vouched += d.vouched ? 1u : 0u;
        // (compared equal: the caller's generation now names the device's geometry, so the next upload under it is
        // vouched for; without this, a first tagged upload of an untagged scene never let the next ones skip the
        // compare)
        c->geometry_gen = geometry_generation;
        return HG_OK;
    }
    c->guides_valid = false;  // the device scene changes: the guide images (hg_update_guides) are another scene's
    const bool partial = d.kind == HG_UPLOAD_PARTIAL;
    HgScenePack pack;
    if (hg_pack_spheres_materials(in, pack, err)) return fail(c, err);
    if (partial && hg_pack_mesh_table(in, c->dev_meshes, pack, err)) return fail(c, err);
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;  // no trace in flight reads the buffers replaced below
    c->has_scene = false;
    if (!partial) {
        for (auto& v : c->scene_copy) v.clear();
        if (hg_pack_geometry(in, pack, err)) return fail(c, err);
    }
    int rc;
    if ((rc = upload(c, c->spheres, pack.sph.data(), pack.sph.size() * sizeof(float4)))) return rc;
    if ((rc = upload(c, c->materials, pack.mat.data(), pack.mat.size() * sizeof(float4)))) return rc;
    if ((rc = upload(c, c->meshes, pack.dm.data(), pack.dm.size() * sizeof(HgDevMesh)))) return rc;
    if (!partial) {
        if ((rc = upload(c, c->nodes, pack.rec.data(), pack.rec.size() * sizeof(float4)))) return rc;
        if ((rc = upload(c, c->leaves, pack.leaf.data(), pack.leaf.size() * sizeof(uint2)))) return rc;
        if ((rc = upload(c, c->tris, pack.t9.data(), pack.t9.size() * sizeof(float)))) return rc;
        if ((rc = upload(c, c->normals, pack.nrm.data(), pack.nrm.size() * sizeof(float4)))) return rc;
    }
    return commit_scene(c, in, pack, d, geometry_generation);
}

int hg_upload_cubemap(hg_ctx* c, int32_t face_size, int32_t n_mips, const float* texels, size_t n_floats) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (face_size <= 0 || n_mips <= 0 || n_mips > HG_MAX_CUBE_MIPS || !texels)
        return fail(c, HG_E_INVALID, "bad cubemap shape");
    uint64_t need = 0;
    for (int m = 0; m < n_mips; ++m) {
        c->cube_mip_offset[m] = uint32_t(need / 4);
        const uint64_t s = std::max(1, face_size >> m);
        need += 6ull * s * s * 4ull;
    }
    if (need != n_floats) return fail(c, HG_E_INVALID, "cubemap has %zu floats, expected %llu", n_floats,
                                      (unsigned long long)need);
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;
    if (int rc = upload(c, c->cube, texels, n_floats * sizeof(float))) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    c->cube_size = face_size;
    c->cube_mips = n_mips;
    return HG_OK;
}

int hg_set_params(hg_ctx* c, const hg_params* p) {
    if (!c || !p) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (p->samplesPerPixel < 1) return fail(c, HG_E_INVALID, "samplesPerPixel must be >= 1");
    if (!(p->screenParameters.x >= 1.0f) || !(p->screenParameters.y >= 1.0f))
        return fail(c, HG_E_INVALID, "screenParameters must be >= 1");
    c->params = *p;
    c->has_params = true;
    return HG_OK;
}

int hg_resize(hg_ctx* c, int32_t width, int32_t height) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (width <= 0 || height <= 0 || int64_t(width) * height > (int64_t(1) << 31))
        return fail(c, HG_E_INVALID, "bad target size %dx%d", width, height);
    if (int rc = set_device(c)) return rc;
    c->W = width;
    c->H = height;
    c->guides_valid = false;  // (hg_update_guides: the guide images are the old size's)
    return alloc_target(c);
}

int hg_set_tiling(hg_ctx* c, int32_t rank, int32_t n_ranks) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(c, HG_E_INVALID, "bad tiling %d/%d", rank, n_ranks);
    if (int rc = set_device(c)) return rc;
    c->rank = rank;
    c->n_ranks = n_ranks;
    return c->W > 0 ? alloc_target(c) : HG_OK;
}

int hg_clear_accumulation(hg_ctx* c) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = set_device(c)) return rc;
    if (c->acc.p) HG_HIP(c, hipMemsetAsync(c->acc.p, 0, c->acc.bytes, c->stream));
    return reset_lost(c);
}

}  // extern "C"

namespace {

// Validation of an hg_render call against the context's state (at the call, so that errors come from the call itself)
int render_check(hg_ctx* c, int32_t n_frames) {
    if (!c->has_scene) return fail(c, HG_E_NOSCENE, "hg_upload_scene not called");
    if (!c->has_params) return fail(c, HG_E_INVALID, "hg_set_params not called");
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (n_frames < 0) return fail(c, HG_E_INVALID, "n_frames < 0");
    const hg_params& p = c->params;
    if (int32_t(p.screenParameters.x) != c->W || int32_t(p.screenParameters.y) != c->H)
        return fail(c, HG_E_INVALID, "screenParameters (%g,%g) != target %dx%d", p.screenParameters.x,
                    p.screenParameters.y, c->W, c->H);
    const int32_t ns = int32_t(p.bufferCounts.x), nm = int32_t(p.bufferCounts.y);
    if (ns < 0 || ns > c->n_spheres || nm < 0 || nm > c->n_meshes)
        return fail(c, HG_E_INVALID, "bufferCounts (%d,%d) exceed uploaded (%d,%d)", ns, nm, c->n_spheres, c->n_meshes);
    return HG_OK;
}

// The server can take the frame of FrameCount `fc` next: running, started with these parameters and options, `fc`
// continuing its chain, room left in its lifetime's unit numbering, not closing (sv_close) and its kernel still resident
bool server_continues(hg_ctx* c, int32_t fc) {
    const hg_ctx::Server& S = c->sv;
    if (!S.running) return false;
    hg_params p = c->params;
    p.frameCount = S.params.frameCount;
    if (std::memcmp(&p, &S.params, sizeof p) != 0 || int64_t(fc) != int64_t(S.params.frameCount) + int64_t(S.committed) ||
        S.kernel_variant != c->kernel || S.descent_t != c->descent_t || S.posted >= S.cap ||
        __atomic_load_n(&S.host[HG_SV_HOST_CLOSING], __ATOMIC_SEQ_CST) != 0ull)
        return false;
    const hipError_t q = hipStreamQuery(S.stream);
    (void)hipGetLastError();
    return q == hipErrorNotReady;
}

// Launch the server for the frames from FrameCount `fc`: kp is the launch's parameter block as render_now built it.  HG_E_UNSUPPORTED when the device gives no stream with a hardware queue of its own (the server's
// gates on the context stream must never queue behind it): the caller launches per call instead.
// HALOGEN_SERVER_SERIAL=1: every gate waits for its server lifetime's end (a profiling aid for profilers that run one
// kernel at a time; the frames are then blended only after the lifetime closes, on idle or at a stop)
bool server_serial() {
    static const bool on = [] {
        const char* e = std::getenv("HALOGEN_SERVER_SERIAL");
        return e && std::atoi(e) == 1;
    }();
    return on;
}

int server_start(hg_ctx* c, const HgKernelParams& kp_in, int32_t fc) {
    hg_ctx::Server& S = c->sv;
    if (!S.stream) {
        std::vector<uint32_t> mask(size_t((c->n_cu + 31) / 32), 0u);
        for (int i = 0; i < c->n_cu; ++i) mask[size_t(i) / 32] |= 1u << (i % 32);
        if (hipExtStreamCreateWithCUMask(&S.stream, uint32_t(mask.size()), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            S.stream = nullptr;
            c->server_on = 0;
            return HG_E_UNSUPPORTED;
        }
        for (hipEvent_t& e : S.blended) HG_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HG_HIP(c, hipEventCreateWithFlags(&S.exited, hipEventDisableTiming));
        // coherent (fine-grained) pinned memory: the pollers' system-scope loads of the post word read host memory
        // itself (measured the same as the default pinned memory, tools/sweeps/sweep_r05_server.txt; this is the
        // memory type whose coherence the loads rely on)
        HG_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&S.host), 256, hipHostMallocMapped | hipHostMallocCoherent));
        for (int k = 0; k < 4; ++k) S.host[k] = 0ull;
    }
    const uint32_t tiles = uint32_t(c->n_local_tiles);
    // waves per SIMD: HG_SV_WAVES, the kernel's occupancy (HALOGEN_SERVER_WAVES overrides, 1..HG_STREAM_WAVES, for A/B)
    static const uint32_t sv_waves = [] {
        const char* e = std::getenv("HALOGEN_SERVER_WAVES");
        const int v = e ? std::atoi(e) : 0;
        return uint32_t(v >= 1 && v <= HG_STREAM_WAVES ? v : HG_SV_WAVES);
    }();
    const HgServerPlan P = hg_plan_server(c->n_cu, tiles, kp_in.stack_depth, int(sv_waves));  // ring, grid, spill, divide
    const uint32_t ring = P.ring, grid = P.grid;
    const size_t per_frame = P.per_frame, spill_bytes = P.spill_bytes;
    // the last lifetime's gates and blends on the context stream read its ring and counts: everything below runs after
    // them (an event, no host wait) unless a buffer must move (then the context stream is drained first)
    if (S.ring.bytes < size_t(ring) * per_frame || S.done.bytes < size_t(ring) * 128u)
        HG_HIP(c, hipStreamSynchronize(c->stream));
    int rc = ensure_uncached(c, S.ring, size_t(ring) * per_frame);
    if (!rc) rc = ensure_uncached(c, S.done, size_t(ring) * 128u);
    if (!rc) rc = ensure_uncached(c, S.ctl, HG_SV_CTL_BYTES);  // (polled by scalar loads: hg_mega.hip sv_sload)
    if (!rc && spill_bytes) rc = ensure(c, S.spill, spill_bytes);
    // the cost order only with HG_SV_COST_ORDER: the server's frames overlap, so no frame's end waits on its longest
    // tiles, and raster order keeps a claim's consecutive tiles together (HG_SV_COST_ORDER in hg_tunables.h)
    const bool ordered = c->tile_order_on && HG_SV_COST_ORDER;
    if (!rc && ordered) rc = cost_order_ensure(c, S, tiles, ensure);
    if (rc) return rc;
    // The counts and heads are zeroed on the context stream: after the last lifetime's gates and blends, and before
    // this lifetime's gates, which are queued there too (zeroed on the server's stream instead, a new gate could read
    // the last lifetime's count of its ring slot before the zeroing and pass at once)
    HG_HIP(c, hipMemsetAsync(S.ctl.p, 0, HG_SV_CTL_BYTES, c->stream));
    HG_HIP(c, hipMemsetAsync(S.done.p, 0, size_t(ring) * 128u, c->stream));
    {
        EventGuard ev(c->free_events);  // (given back at once: the wait holds what it needs of the event)
        if (int r = event_pair(c, ev)) return r;
        HG_HIP(c, hipEventRecord(ev.pair.first, c->stream));
        HG_HIP(c, hipStreamWaitEvent(S.stream, ev.pair.first, 0));
    }
    HgKernelParams kp = kp_in;
    kp.tile_order = nullptr;
    kp.tile_cost = nullptr;
    if (ordered) {  // the cost order of the last lifetime's frames, or none yet
        kp.tile_cost = static_cast<unsigned long long*>(S.tile_cost.p);
        HG_HIP(c, cost_order_run(c, S, tiles, S.tile_cost_valid));
        if (S.tile_cost_valid) kp.tile_order = static_cast<const uint32_t*>(S.tile_order.p);
        S.tile_cost_valid = true;
    }
    kp.frame_color = static_cast<float4*>(S.ring.p);
    kp.frames_done = static_cast<uint32_t*>(S.done.p);
    kp.queue = static_cast<uint32_t*>(S.ctl.p);
    kp.resident_waves = P.slots;
    kp.wave_units = 1;
    kp.spill = spill_bytes ? static_cast<uint32_t*>(S.spill.p) : nullptr;
    kp.spill_stride = grid * 64u;
    kp.first_frame = fc;
    kp.n_frames = 1;
    kp.frame_split = 1;
    kp.accumulate = 1;
    void* post = nullptr;
    HG_HIP(c, hipHostGetDevicePointer(&post, S.host, 0));
    kp.sv_post = static_cast<const unsigned long long*>(post);
    kp.sv_ring = ring;
    kp.sv_frames_cap = P.frames_cap;
    kp.sv_idle_ticks = uint32_t(std::min<uint64_t>(uint64_t(S.idle_us) * 100ull, 0xFFFFFFFFull));
    kp.sv_div_magic = P.div_magic;
    kp.sv_div_shift = P.div_shift;
    // (the lost-frame word is not reset: a gate of the last lifetime may still report into it)
    __atomic_store_n(&S.host[HG_SV_HOST_POST], 0ull, __ATOMIC_SEQ_CST);
    __atomic_store_n(&S.host[HG_SV_HOST_CLOSING], 0ull, __ATOMIC_SEQ_CST);
    __atomic_store_n(&S.host[HG_SV_HOST_CLOSED], 0ull, __ATOMIC_SEQ_CST);
    HG_HIP(c, hg_launch_mega_stream(kp, 64, c->counters_on != 0, S.stream, true));
    if (server_serial()) HG_HIP(c, hipEventRecord(S.exited, S.stream));
    S.running = true;
    S.ring_n = ring;
    S.posted = 0;
    S.committed = 0;
    S.cap = kp.sv_frames_cap;
    for (uint32_t k = 0; k < HG_SV_RING; ++k) {
        S.uses[k] = 0;
        S.blend_valid[k] = false;
    }
    S.params = c->params;
    S.params.frameCount = fc;
    S.kernel_variant = c->kernel;
    S.descent_t = c->descent_t;
    S.kp = kp;
    c->server_launches++;
    sv_trace("start: FrameCount %d, %u tiles, ring %u, grid %u", fc, tiles, ring, grid);
    return HG_OK;
}

// Post frame k = S.posted to the server: the host's half of the close handshake (hg_mega.hip sv_close).  Raise the post
// word, then read the closing word.  Not raised: the post is taken (a wave that closes later reads the post word after
// this store).  Raised: the post is taken only if the closing wave's read of the post word included it (the close
// word); else HG_E_UNSUPPORTED, nothing posted: the caller restarts the server and posts there.  The ring slot must be
// free (its frame ring_n back blended).
int server_post_frame(hg_ctx* c) {
    hg_ctx::Server& S = c->sv;
    const uint32_t k = S.posted, s = k & (S.ring_n - 1u);
    __atomic_store_n(&S.host[HG_SV_HOST_POST], static_cast<unsigned long long>(k + 1u), __ATOMIC_SEQ_CST);
    if (__atomic_load_n(&S.host[HG_SV_HOST_CLOSING], __ATOMIC_SEQ_CST) != 0ull) {
        // the closing wave publishes the post word it read right after reading it (bounded wait: a wave that raised
        // the closing word is running its next few instructions)
        unsigned long long fin;
        const double t0 = host_seconds();
        while (!((fin = __atomic_load_n(&S.host[HG_SV_HOST_CLOSED], __ATOMIC_SEQ_CST)) & HG_SV_CLOSED)) {
            if (host_seconds() - t0 > 10.0) return fail(c, HG_E_HIP, "render server: the closing wave never published");
            std::this_thread::yield();
        }
        if (uint32_t(fin) < k + 1u) {
            c->server_refused++;
            sv_trace("post %u: refused (the server closed at %u frames)", k, uint32_t(fin));
            return HG_E_UNSUPPORTED;
        }
        sv_trace("post %u: taken by a closing server", k);
    }
    S.uses[s]++;
    S.posted = k + 1u;
#if HG_SV_DIAG_TIMES
    if (k < 256u) S.post_s[k] = host_seconds();
#endif
    return HG_OK;
}

// The frame the host asks for next (FrameCount = first + committed): posted now, unless it was posted ahead
// (server_speculate), then its gate + blend on the context stream (in frame order, like every other blend).  Frames run
// at most ring_n ahead of their blends (the host waits for the blend of the frame ring_n back before reusing its ring
// slot).  HG_E_UNSUPPORTED: the post was refused (a closing server), nothing queued.
int server_commit(hg_ctx* c) {
    hg_ctx::Server& S = c->sv;
    const uint32_t k = S.committed, s = k & (S.ring_n - 1u);
    if (k == S.posted) {
        if (S.blend_valid[s]) {
            sv_trace("post %u: waiting for the blend of frame %u", k, k - S.ring_n);
            HG_HIP(c, hipEventSynchronize(S.blended[s]));
        }
        if (int rc = server_post_frame(c)) return rc;
    }
    const uint32_t tiles = uint32_t(c->n_local_tiles), n_slots = tiles * 64u;
    void* err = nullptr;
    HG_HIP(c, hipHostGetDevicePointer(&err, S.host + HG_SV_HOST_LOST, 0));
    if (server_serial()) HG_HIP(c, hipStreamWaitEvent(c->stream, S.exited, 0));
    HG_HIP(c, hg_launch_server_frame(static_cast<float4*>(c->acc.p),
                                     static_cast<const float4*>(S.ring.p) + size_t(s) * n_slots, n_slots,
                                     S.kp.first_frame + int32_t(k), static_cast<const uint32_t*>(S.done.p) + 32u * s,
                                     S.uses[s] * tiles, gate_timeout_ticks(c),
                                     reinterpret_cast<const unsigned long long*>(static_cast<const uint32_t*>(S.ctl.p) +
                                                                                 HG_SV_EXIT_WORD),
                                     static_cast<uint32_t*>(c->lost.p), static_cast<unsigned long long*>(err),
                                     c->acc_epoch, c->stream));
    HG_HIP(c, hipEventRecord(S.blended[s], c->stream));
    S.blend_valid[s] = true;
    S.committed = k + 1u;
    c->server_frames++;
    sv_trace("committed %u (slot %u, target %u)", k, s, S.uses[s] * tiles);
    return HG_OK;
}

// Frames traced ahead of the host's calls (HG_OPT_SERVER_AHEAD, with the counters off): the next frames of the same
// parameters and FrameCount chain are posted without a gate or blend, never waiting (a ring slot whose blend has not
// run stops it).  A call that continues the chain commits them (server_commit); anything else stops the server and
// abandons those not yet claimed.  The host's display of frame k then waits only for frame k's gate, blend and copy:
// frame k + 1 is already being traced.  Same images (a frame is blended only when the host asks for it).
void server_speculate(hg_ctx* c) {
    hg_ctx::Server& S = c->sv;
    if (c->sv_ahead <= 0 || c->counters_on) return;
    const uint32_t ahead = std::min<uint32_t>(uint32_t(c->sv_ahead), S.ring_n - 2u);
    while (S.posted < S.committed + ahead && S.posted < S.cap) {
        const uint32_t s = S.posted & (S.ring_n - 1u);
        if (S.blend_valid[s]) {
            const hipError_t q = hipEventQuery(S.blended[s]);
            (void)hipGetLastError();  // hipErrorNotReady is a status here
            if (q != hipSuccess) return;
        }
        if (server_post_frame(c) != HG_OK) return;  // (refused: the next call restarts the server)
        c->server_ahead_posts++;
    }
}

// n_frames frames from FrameCount = params.frameCount through the server (started or restarted as needed).  A first
// HG_E_UNSUPPORTED (no stream of its own) falls back to launches; nothing was posted then.  A post refused by a closing
// server restarts it (bounded: a server closes only after HG_OPT_SERVER_IDLE_US with nothing posted).
int server_render(hg_ctx* c, const HgKernelParams& kp, int32_t n_frames) {
    for (int32_t f = 0; f < n_frames; ++f) {
        const int32_t fc = c->params.frameCount + f;
        for (int attempt = 0;; ++attempt) {
            if (c->sv.running && !server_continues(c, fc))
                if (int rc = server_stop(c)) return rc;
            if (!c->sv.running) {
                const int rc = server_start(c, kp, fc);
                if (rc == HG_E_UNSUPPORTED && f > 0) return fail(c, HG_E_HIP, "render server: restart failed");
                if (rc) return rc;
            }
            const int rc = server_commit(c);
            if (rc != HG_E_UNSUPPORTED) {
                if (rc) return rc;
                break;
            }
            if (attempt >= 64) return fail(c, HG_E_HIP, "render server: 64 fresh servers in a row refused a post");
        }
    }
    server_speculate(c);
    return HG_OK;
}

// The host runs ahead of the GPU: the render call before the previous one has not finished on the device.  Then the
// render server pays: it removes the drain at each frame's end.  A host that waits for every frame (a display at once,
// or one frame behind) never runs ahead; the server serves it when it traces ahead of the calls (server_chain).
bool host_ahead(hg_ctx* c) {
    const int k = int(c->calls & 1u);  // recorded by the call before last
    if (!c->call_done_valid[k]) return false;
    const hipError_t q = hipEventQuery(c->call_done[k]);
    (void)hipGetLastError();  // hipErrorNotReady is a status here
    return q == hipErrorNotReady;
}
// The call continues a chain of at least two calls (same parameters, FrameCount continuing) and the server may trace
// ahead of it (HG_OPT_SERVER_AHEAD, counters off): the frames the host waits for are then already in flight
bool server_chain(hg_ctx* c, int32_t n_frames) {
    hg_params q = c->params;
    q.frameCount = 0;
    const bool cont = c->chain_len > 0 && c->params.frameCount == c->chain_next &&
                      std::memcmp(&q, &c->chain_params, sizeof q) == 0;
    c->chain_len = cont ? c->chain_len + 1 : 1;
    c->chain_params = q;
    c->chain_next = c->params.frameCount + n_frames;
    return c->sv_ahead > 0 && !c->counters_on && c->chain_len >= 2;
}
// After a render call's work is queued: its completion event, for host_ahead
void note_call(hg_ctx* c) {
    const int k = int(c->calls & 1u);
    c->call_done_valid[k] = hipEventRecord(c->call_done[k], c->stream) == hipSuccess;
    c->calls++;
}

// The camera part of a launch's parameter block (everything camera_ray reads, hg_device.h) from the uniforms
void set_camera(HgKernelParams& kp, const hg_params& p) {
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) kp.cam[r * 4 + k] = p.camLocalToWorld.m[k * 4 + r];
    kp.W = p.screenParameters.x;
    kp.H = p.screenParameters.y;
    kp.Wu = uint32_t(p.screenParameters.x);
    kp.Hu = uint32_t(p.screenParameters.y);
    kp.vw = p.viewParameters.x;
    kp.vh = p.viewParameters.y;
    kp.near_ = p.viewParameters.z;
    kp.far_ = p.viewParameters.w;
    // tan(radians(focalConeAngle)) * ViewParameters.z (:998), once per launch with the shared spec
    kp.focal_disc_radius = hg_tanf(p.focalConeAngle * HG_DEG2RAD) * p.viewParameters.z;
    kp.psx = (p.viewParameters.x * 2.0f) / p.screenParameters.x;  // get_ray_jitter :986
    kp.psy = (p.viewParameters.y * 2.0f) / p.screenParameters.y;
    kp.filter_radius = p.filterRadius;
    kp.focal_dist = p.focalPlaneDistance;
}

// The scene part of a launch's parameter block: the uploaded arrays, the stack depth and the descent threshold
void set_scene(HgKernelParams& kp, const hg_ctx* c, uint32_t descent_t) {
    kp.stack_depth = c->stack_depth;
    kp.descent_t = descent_t;
    kp.spheres = static_cast<const float4*>(c->spheres.p);
    kp.meshes = static_cast<const HgDevMesh*>(c->meshes.p);
    kp.materials = static_cast<const float4*>(c->materials.p);
    kp.nodes = static_cast<const float4*>(c->nodes.p);
    kp.leaves = static_cast<const uint2*>(c->leaves.p);
    kp.tris = static_cast<const float*>(c->tris.p);
    kp.normals = static_cast<const float4*>(c->normals.p);
}

// The pixels of this rank's local tiles that lie in the image: f(accumulator slot, image pixel) (hg_tiling.h)
template <class F>
void for_local_pixels(const hg_ctx* c, F&& f) {
    hg_for_local_pixels(uint32_t(c->W), uint32_t(c->H), uint32_t(c->n_local_tiles), uint32_t(c->rank),
                        uint32_t(c->n_ranks), f);
}

// What the launch plan (hg_plan.h) reads of the context, its uniforms and the call
HgPlanIn plan_input(const hg_ctx* c, int32_t n_frames) {
    const hg_params& p = c->params;
    return HgPlanIn{c->n_cu,        c->n_local_tiles, c->W,          c->H,          c->stack_depth,     c->n_meshes,
                    c->kernel,      c->block,         c->frame_split, c->wave_units, c->queue_fill,      c->descent_t,
                    c->tile_order_on, c->coalesce,    c->n_ranks,    p.halogenDebugMode, p.maxBounces, p.samplesPerPixel,
                    n_frames};
}

// The parameter block of a render call planned as P; the chunks set their own frames and their trace stream's buffers
HgKernelParams kernel_params(const hg_ctx* c, const HgCallPlan& P, int32_t n_frames, int32_t accumulate) {
    const hg_params& p = c->params;
    HgKernelParams kp{};
    set_camera(kp, p);
    kp.Hu = uint32_t(c->H);
    kp.spp = p.samplesPerPixel;
    kp.max_bounces = p.maxBounces;
    kp.max_diff = p.maxDiffuseBounces;
    kp.max_glossy = p.maxGlossyBounces;
    kp.max_trans = p.maxTransmissionBounces;
    kp.debug_mode = p.halogenDebugMode;
    kp.tri_range = p.triangleDebugDisplayRange;
    kp.box_range = p.boxDebugDisplayRange;
    kp.default_mip = p.defaultHDRIMipLevel;
    kp.use_cube = (p.useEnvironmentCubemap > 0 && c->cube_mips > 0) ? 1 : 0;
    kp.n_spheres = int32_t(p.bufferCounts.x);
    kp.n_meshes = int32_t(p.bufferCounts.y);
    kp.first_frame = accumulate ? p.frameCount : 1;
    kp.n_frames = n_frames;
    kp.accumulate = accumulate ? 1 : 0;
    kp.frame_split = 1;
    kp.tiles_x = c->tiles_x;
    kp.rank = c->rank;
    kp.n_ranks = c->n_ranks;
    kp.n_local_tiles = c->n_local_tiles;
    kp.cube_size = c->cube_size;
    kp.cube_mips = c->cube_mips;
    std::memcpy(kp.cube_mip_offset, c->cube_mip_offset, sizeof kp.cube_mip_offset);
    set_scene(kp, c, P.descent_t);
    kp.stream_deep = P.stream_deep;
    kp.spill_stride = P.spill_stride;
    kp.cube = static_cast<const float4*>(c->cube.p);
    kp.acc = static_cast<float4*>(c->acc.p);
    kp.counters = c->counters_on ? static_cast<unsigned long long*>(c->counters_dev.p) : nullptr;
    return kp;
}

int launch_failed(hg_ctx* c, hipError_t e) {
    return fail(c, HG_E_HIP, "megakernel launch failed: %s", hipGetErrorString(e));
}

// Trace pipeline, step 1: the trace streams' buffers for a call planned as P, grown only while idle.  The streams
// beyond HG_TRACE_LANES_BIG trace short chunks only: they get buffers when the call has such a chunk (P.short_chunks)
int ensure_lanes(hg_ctx* c, const HgCallPlan& P) {
    for (int li = 0; li < HG_TRACE_LANES; ++li) {
        hg_ctx::TraceLane& L = c->lanes[li];
        if (li >= HG_TRACE_LANES_BIG && !P.short_chunks) continue;
        const int fmax = li < HG_TRACE_LANES_BIG ? P.big_frames : P.short_frames;
        int rc = ensure_quiet(c, L.frame_color, P.per_frame * size_t(fmax));
        if (!rc && P.spill_bytes) rc = ensure_quiet(c, L.spill, P.spill_bytes);
        if (!rc && P.ordered) rc = cost_order_ensure(c, L, uint32_t(c->n_local_tiles), ensure_quiet);
        // the queue heads are zeroed once, when allocated (each use leaves them zeroed)
        if (!rc && P.stream_k && L.queue.bytes < HG_QUEUE_BYTES) {
            rc = ensure_quiet(c, L.queue, HG_QUEUE_BYTES);
            if (!rc && hipMemsetAsync(L.queue.p, 0, L.queue.bytes, L.stream) != hipSuccess)
                rc = fail(c, HG_E_HIP, "hipMemsetAsync(queue) failed");
        }
        if (rc) return rc;
    }
    return HG_OK;
}

// Step 2: the trace stream of a chunk.  Short chunks take every stream in turn, or the first one whose last trace and
// blend are done (HG_OPT_LANE_PICK: its queue stays warm); long ones the first HG_TRACE_LANES_BIG in turn
hg_ctx::TraceLane& pick_lane(hg_ctx* c, bool short_stream) {
    int li = -1;
    if (!short_stream) {
        li = c->next_lane_big;
        c->next_lane_big = (c->next_lane_big + 1) % HG_TRACE_LANES_BIG;
        return c->lanes[li];
    }
    if (c->lane_pick) {
        for (int j = 0; j < HG_TRACE_LANES && li < 0; ++j)
            if (!c->lanes[j].blend_pending || hipEventQuery(c->lanes[j].blended) == hipSuccess) li = j;
        (void)hipGetLastError();  // hipErrorNotReady is a status here
    }
    if (li < 0) {
        li = c->next_lane;
        c->next_lane = (c->next_lane + 1) % HG_TRACE_LANES;
    }
    return c->lanes[li];
}

// Traces in flight on the trace streams other than L (hg_queue_waves sizes a queue launch by it)
int traces_in_flight(hg_ctx* c, const hg_ctx::TraceLane& L) {
    int busy = 0;
    for (const hg_ctx::TraceLane& O : c->lanes)
        if (&O != &L && O.blend_pending && hipEventQuery(O.traced) == hipErrorNotReady) ++busy;
    (void)hipGetLastError();  // hipErrorNotReady is a status here, not an error for the launch check
    return busy;
}

// Step 3: one chunk (kc: its frames) on trace stream L in the shape K: wait for the stream's buffers, sort, trace on
// L.stream; blend in frame order on the context stream; record the events that order the next chunk.  call_start: the
// call's timing event, for its first chunk (the launch starts there).
int launch_chunk(hg_ctx* c, hg_ctx::TraceLane& L, HgKernelParams& kc, const HgCallPlan& P, const HgChunkPlan& K,
                 hipEvent_t call_start) {
    const uint32_t tiles = uint32_t(c->n_local_tiles);
    const uint32_t slots = uint32_t(hg_wave_slots(c->n_cu, HG_STREAM_WAVES));
    kc.frame_split = K.frame_split;
    kc.frame_color = static_cast<float4*>(L.frame_color.p);
    kc.spill = P.spill_bytes ? static_cast<uint32_t*>(L.spill.p) : nullptr;
    kc.queue = K.queue ? static_cast<uint32_t*>(L.queue.p) : nullptr;
    kc.resident_waves = K.queue && HG_QUEUE_WAVES_DIV > 1 ? hg_queue_waves(slots, traces_in_flight(c, L)) : slots;
    kc.wave_units = K.wave_units;
    kc.tile_order = nullptr;
    kc.tile_cost = P.ordered ? static_cast<unsigned long long*>(L.tile_cost.p) : nullptr;
    hipError_t e = hipSuccess;
    // this stream's buffers are free once the blend of its previous chunk has read them
    if (L.blend_pending) e = hipStreamWaitEvent(L.stream, L.blended, 0);
    if (e == hipSuccess && call_start) e = hipEventRecord(call_start, L.stream);
    if (e == hipSuccess && P.ordered) {
        // Cost order, per trace stream: the stream sorts its own costs into its own order buffer (the traces adding
        // those costs and reading that order run on the same stream, so none is in flight during the sort), once
        // HG_ORDER_MIN_FRAMES frames were traced on it since its last sort: 64-frame launches every time, the
        // reference's 1-frame launches every 16th frame per stream.  Costs not yet valid are zeroed instead.
        const bool sort =
            L.tile_cost_valid && (!L.tile_order_valid || L.frames_since_order >= int64_t(HG_ORDER_MIN_FRAMES));
        if (sort || !L.tile_cost_valid) {
            e = cost_order_run(c, L, tiles, sort);
            L.tile_order_valid = sort && e == hipSuccess;
            L.frames_since_order = 0;
        }
        if (L.tile_order_valid) kc.tile_order = static_cast<const uint32_t*>(L.tile_order.p);
        L.tile_cost_valid = e == hipSuccess;
        L.frames_since_order += kc.n_frames;
    }
    EventGuard tev(c->free_events);  // the chunk's own timing pair (HG_OPT_TIMING)
    if (e == hipSuccess && c->timing) {
        if (int rc = event_pair(c, tev)) return rc;
        e = hipEventRecord(tev.pair.first, L.stream);
    }
    if (e == hipSuccess)
        e = P.stream_k ? hg_launch_mega_stream(kc, P.block, c->counters_on != 0, L.stream)
                       : hg_launch_mega_regen(kc, P.block, c->counters_on != 0, L.stream);
    if (tev.held()) {  // a pair goes to drain_events only with both ends recorded
        if (e == hipSuccess) e = hipEventRecord(tev.pair.second, L.stream);
        if (e == hipSuccess) tev.hand_to(c->pending_trace);
    }
    if (e == hipSuccess) e = hipEventRecord(L.traced, L.stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, L.traced, 0);
    if (e == hipSuccess)  // in frame order, on the context stream
        e = hg_launch_blend_frames(kc, static_cast<const uint32_t*>(c->lost.p), c->stream);
    if (e == hipSuccess) e = hipEventRecord(L.blended, c->stream);
    L.blend_pending = e == hipSuccess;
    return e == hipSuccess ? HG_OK : launch_failed(c, e);
}

// A pipelined call: its chunks traced on the trace streams and blended on the context stream
int launch_pipelined(hg_ctx* c, const HgPlanIn& in, const HgCallPlan& P, const HgKernelParams& kp, hipEvent_t start) {
    if (int rc = ensure_lanes(c, P)) return rc;
    HgKernelParams kc = kp;
    int rc = HG_OK;
    for (int done = 0; done < in.n_frames && !rc; done += kc.n_frames) {  // chunks at frame boundaries change nothing
        kc.n_frames = std::min(in.n_frames - done, P.chunk_max);
        kc.first_frame = kp.accumulate ? kp.first_frame + done : 1;
        const HgChunkPlan K = hg_plan_chunk(in, P, kc.n_frames);
        rc = launch_chunk(c, pick_lane(c, K.short_stream), kc, P, K, done == 0 ? start : nullptr);
    }
    if (rc)  // a sort or a queue launch that failed part way may have left its words non-zero
        for (hg_ctx::TraceLane& L : c->lanes) {
            if (L.queue.p) (void)hipMemsetAsync(L.queue.p, 0, L.queue.bytes, L.stream);
            if (L.order_scratch.p) (void)hipMemsetAsync(L.order_scratch.p, 0, L.order_scratch.bytes, L.stream);
            L.tile_cost_valid = L.tile_order_valid = false;
        }
    return rc;
}

// After a call's work is queued on the context stream: the end of its timing pair (now drain_events'), its completion
// event, the counts, and FrameCount++ per accumulated frame (RP:347)
int finish_call(hg_ctx* c, EventGuard& ev, int32_t n_frames, int32_t accumulate) {
    HG_HIP(c, hipEventRecord(ev.pair.second, c->stream));
    note_call(c);
    ev.hand_to(c->pending);
    c->counters.launches++;
    if (c->pending.size() + c->pending_trace.size() > 4096)
        if (int rc = drain_events(c)) return rc;
    if (accumulate) c->params.frameCount += n_frames;
    return HG_OK;
}

// One launch of n_frames frames from FrameCount = params.frameCount (which it advances when accumulating): check,
// plan (hg_plan.h), parameter block, then the render server or a launch of the planned shape, then the book-keeping
int render_now(hg_ctx* c, int32_t n_frames, int32_t accumulate) {
    if (int rc = render_check(c, n_frames)) return rc;
    if (n_frames == 0) return HG_OK;
    if (int rc = set_device(c)) return rc;
    const HgPlanIn in = plan_input(c, n_frames);
    const HgCallPlan P = hg_plan_call(in);
    HgKernelParams kp = kernel_params(c, P, n_frames, accumulate);
    EventGuard ev(c->free_events);  // the call's timing pair
    if (int rc = event_pair(c, ev)) return rc;
    HG_HIP(c, hipEventRecord(ev.pair.first, c->stream));
    if (P.status) return fail(c, P.status, "target too large: %lld work units", (long long)c->n_local_tiles);
    if (P.spill_bytes && !P.pipelined) {
        if (int rc = ensure_quiet(c, c->spill, P.spill_bytes)) return rc;
        kp.spill = static_cast<uint32_t*>(c->spill.p);
    }
    c->counters.last_kernel = P.last_kernel;
    // the reference's one frame per call: posted to the render server (persistent trace waves)
    const bool chain = accumulate && server_chain(c, n_frames);
    if (c->server_on && P.stream_k && P.pipelined && accumulate && n_frames <= HG_QUEUE_MAX_FRAMES &&
        c->n_local_tiles > 0 && (c->server_on == 2 || host_ahead(c) || chain)) {
        const int rc = server_render(c, kp, n_frames);
        if (rc == HG_OK) return finish_call(c, ev, n_frames, accumulate);
        if (rc != HG_E_UNSUPPORTED) return rc;
    } else if (c->sv.running) {  // another kind of launch needs the GPU's wave slots
        if (int rc = server_stop(c)) return rc;
    }
    if (P.pipelined) {
        if (int rc = launch_pipelined(c, in, P, kp, ev.pair.first)) return rc;
    } else if (P.regen) {  // a regenerating launch that blends in the kernel (make noitems): on the context stream
        HgKernelParams kc = kp;
        for (int done = 0; done < n_frames; done += kc.n_frames) {
            kc.n_frames = std::min(n_frames - done, P.chunk_max);
            kc.first_frame = accumulate ? kp.first_frame + done : 1;
            kc.frame_split = std::min(P.split, kc.n_frames);
            const hipError_t e = hg_launch_mega_regen(kc, P.block, c->counters_on != 0, c->stream);
            if (e != hipSuccess) return launch_failed(c, e);
        }
    } else {
        const hipError_t e = hg_launch_mega(kp, P.block, c->counters_on != 0, c->stream);
        if (e != hipSuccess) return launch_failed(c, e);
    }
    return finish_call(c, ev, n_frames, accumulate);
}

}  // namespace

bool hg_ctx_lost(hg_ctx* c) {
    server_note_lost(c);
    return c->acc_lost;
}

int hg_ctx_flush(hg_ctx* c) {
    if (!c || c->pending_frames == 0) return HG_OK;
    const int32_t n = c->pending_frames, acc = c->pending_acc;
    c->pending_frames = 0;
    return render_now(c, n, acc);
}

// The accumulator (this rank's tiles, tile-major) as a row-major image in a display format (hg_pack.h); pixels of
// other ranks' tiles are 0.  One thread per pixel: the stores are contiguous (16 / 8 / 4 B per pixel), the loads are 8
// consecutive float4 per tile row.  64-thread workgroups (see launch_untile).
template <int kFmt, bool kRows>
__global__ __launch_bounds__(64) void hg_untile_image(void* __restrict__ image, const float4* __restrict__ acc,
                                                       int32_t W, int32_t H, int32_t tiles_x, int32_t rank,
                                                       int32_t n_ranks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= uint32_t(W) * uint32_t(H)) return;
    float4 v;
    if constexpr (kRows) {  // the source is already a row-major image (the multi-GPU gather's assembled image)
        v = acc[i];
    } else {
        const HgPixelSource s = hg_pixel_source(i % uint32_t(W), i / uint32_t(W), uint32_t(tiles_x), uint32_t(n_ranks));
        v = s.rank == uint32_t(rank) ? acc[size_t(s.local_tile) * 64u + s.lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (kFmt == HG_DISPLAY_RGBA32F) {
        static_cast<float4*>(image)[i] = v;
    } else if constexpr (kFmt == HG_DISPLAY_RGBA16F) {
        uint32_t h[2];
        hg_pack_rgba16f(v.x, v.y, v.z, v.w, h);
        static_cast<uint2*>(image)[i] = make_uint2(h[0], h[1]);
    } else {
        static_cast<uint32_t*>(image)[i] = hg_pack_r11g11b10(v.x, v.y, v.z);
    }
}

namespace {

size_t display_bpp(int32_t format) {
    return format == HG_DISPLAY_RGBA32F ? 16 : format == HG_DISPLAY_RGBA16F ? 8 : format == HG_DISPLAY_R11G11B10F ? 4 : 0;
}

template <bool kRows>
void launch_untile(hg_ctx* c, void* dst, int32_t format, const float4* src) {
    // one-wave workgroups with few registers: a display readback's untile runs beside the persistent trace waves of the
    // next frames (which hold most wave slots), as the lean blend does, instead of waiting for a CU to drain
    const size_t pixels = size_t(c->W) * size_t(c->H);
    const dim3 g(uint32_t((pixels + 63) / 64)), b(64);
    if (format == HG_DISPLAY_RGBA16F)
        hipLaunchKernelGGL((hg_untile_image<HG_DISPLAY_RGBA16F, kRows>), g, b, 0, c->stream, dst, src, c->W, c->H,
                           c->tiles_x, c->rank, c->n_ranks);
    else if (format == HG_DISPLAY_R11G11B10F)
        hipLaunchKernelGGL((hg_untile_image<HG_DISPLAY_R11G11B10F, kRows>), g, b, 0, c->stream, dst, src, c->W, c->H,
                           c->tiles_x, c->rank, c->n_ranks);
    else
        hipLaunchKernelGGL((hg_untile_image<HG_DISPLAY_RGBA32F, kRows>), g, b, 0, c->stream, dst, src, c->W, c->H,
                           c->tiles_x, c->rank, c->n_ranks);
}

// Enqueue on the context stream: the accumulator untiled (or, with `rows`, a row-major float4 image of the target's
// size converted) into `target` (c->image unless given; grown as needed) in `format`.  Returns its size in bytes.
int untile_async(hg_ctx* c, size_t* bytes, int32_t format = HG_DISPLAY_RGBA32F, const float4* rows = nullptr,
                 DevBuf* target = nullptr) {
    DevBuf& img = target ? *target : c->image;
    const size_t pixels = size_t(c->W) * size_t(c->H);
    *bytes = pixels * display_bpp(format);
    if (img.bytes < *bytes) {  // everything that might read the old image is ordered before on the context stream
        HG_HIP(c, hipStreamSynchronize(c->stream));
        if (int rc = ensure(c, img, *bytes)) return rc;
    }
    if (rows) launch_untile<true>(c, img.p, format, rows);
    else launch_untile<false>(c, img.p, format, static_cast<const float4*>(c->acc.p));
    HG_HIP(c, hipGetLastError());
    return HG_OK;
}

}  // namespace

// The display readback of hg_readback_begin_format, from the accumulator (rows == nullptr) or from a row-major float4
// image of the target's size on the context's device (the comm's assembled image, hg_comm_readback_begin)
int hg_ctx_display_begin(hg_ctx* c, const void* rows, int32_t format) {
    if (int rc = hg_ctx_flush(c)) return rc;
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (!display_bpp(format)) return fail(c, HG_E_INVALID, "unknown display format %d", format);
    if (c->rb_pending >= c->rb_depth)
        return fail(c, HG_E_INVALID, "%d readbacks outstanding (HG_OPT_READBACK_DEPTH): call hg_readback_end first",
                    c->rb_pending);
    if (int rc = set_device(c)) return rc;
    const int k = c->rb_next;  // not outstanding: at most rb_depth are, and k is the slot after the newest
    // HG_OPT_READBACK_STREAM 2 (zero copy): the untile kernel writes the display image straight into the slot's pinned
    // host image (mapped, fine-grained: its stores cross PCIe as they retire), no copy; the copy event is recorded
    // after the kernel on the context stream
    if (c->rb_side == 2) {
        const size_t bytes = size_t(c->W) * size_t(c->H) * display_bpp(format);
        if (c->image_host_cap[k] < bytes || !c->image_host_mapped[k]) {
            if (c->image_host[k]) {
                HG_HIP(c, hipEventSynchronize(c->image_copied[k]));  // (its last copy was ended: returns at once)
                HG_HIP(c, hipHostFree(c->image_host[k]));
            }
            c->image_host[k] = nullptr;
            c->image_host_cap[k] = 0;
            hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&c->image_host[k]), bytes,
                                         hipHostMallocMapped | hipHostMallocCoherent);
            if (e != hipSuccess) return fail(c, HG_E_NOMEM, "hipHostMalloc(%zu, mapped) failed: %s", bytes, hipGetErrorString(e));
            c->image_host_cap[k] = bytes;
            c->image_host_mapped[k] = true;
            if (!c->image_copied[k]) HG_HIP(c, hipEventCreateWithFlags(&c->image_copied[k], hipEventDisableTiming));
        }
        void* dptr = nullptr;
        HG_HIP(c, hipHostGetDevicePointer(&dptr, c->image_host[k], 0));
        if (rows) launch_untile<true>(c, dptr, format, static_cast<const float4*>(rows));
        else launch_untile<false>(c, dptr, format, static_cast<const float4*>(c->acc.p));
        HG_HIP(c, hipGetLastError());
        HG_HIP(c, hipEventRecord(c->image_copied[k], c->stream));
        c->image_host_bytes[k] = bytes;
        c->image_host_format[k] = format;
        c->rb_next = (k + 1) % c->rb_depth;
        c->rb_pending++;
        return HG_OK;
    }
    // HG_OPT_READBACK_STREAM 1: the slot's own device image, copied on the side stream, so the context stream (the next
    // frames' blends) does not wait for the copy; 0: c->image, copied on the context stream
    const bool side = c->rb_side != 0;
    if (side && !c->rb_stream) {
        // the copy stream on a hardware queue of its own (a plain stream shares one with a trace lane and waits behind
        // its traces: depth 2 1,285 -> 1,642 Mpaths/s, sweep_r04_rbq)
        HG_HIP(c, create_lane_stream(c, HG_TRACE_LANES, &c->rb_stream));
        for (int j = 0; j < HG_READBACK_MAX; ++j)
            HG_HIP(c, hipEventCreateWithFlags(&c->rb_untiled[j], hipEventDisableTiming));
    }
    size_t bytes = 0;
    DevBuf* dimg = side ? &c->rb_image[k] : &c->image;
    if (int rc = untile_async(c, &bytes, format, static_cast<const float4*>(rows), dimg)) return rc;
    if (c->image_host_cap[k] < bytes) {
        if (c->image_host[k]) {
            HG_HIP(c, hipEventSynchronize(c->image_copied[k]));  // (its last copy was ended, so this returns at once)
            HG_HIP(c, hipHostFree(c->image_host[k]));
        }
        c->image_host[k] = nullptr;
        c->image_host_cap[k] = 0;
        c->image_host_mapped[k] = false;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&c->image_host[k]), bytes, 0);
        if (e != hipSuccess) return fail(c, HG_E_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        c->image_host_cap[k] = bytes;
        if (!c->image_copied[k]) HG_HIP(c, hipEventCreateWithFlags(&c->image_copied[k], hipEventDisableTiming));
    }
    if (side) {
        HG_HIP(c, hipEventRecord(c->rb_untiled[k], c->stream));
        HG_HIP(c, hipStreamWaitEvent(c->rb_stream, c->rb_untiled[k], 0));
        HG_HIP(c, hipMemcpyAsync(c->image_host[k], dimg->p, bytes, hipMemcpyDeviceToHost, c->rb_stream));
        HG_HIP(c, hipEventRecord(c->image_copied[k], c->rb_stream));
    } else {
        HG_HIP(c, hipMemcpyAsync(c->image_host[k], dimg->p, bytes, hipMemcpyDeviceToHost, c->stream));
        HG_HIP(c, hipEventRecord(c->image_copied[k], c->stream));
    }
    c->image_host_bytes[k] = bytes;
    c->image_host_format[k] = format;
    c->rb_next = (k + 1) % c->rb_depth;
    c->rb_pending++;
    return HG_OK;
}

// The copy event of the oldest outstanding display readback (nullptr when none is outstanding)
hipEvent_t hg_ctx_display_oldest(const hg_ctx* c) {
    if (c->rb_pending <= 0) return nullptr;
    return c->image_copied[(c->rb_next - c->rb_pending + c->rb_depth) % c->rb_depth];
}

extern "C" {

int hg_readback_begin_format(hg_ctx* c, int32_t format) {
    if (!c) return HG_E_INVALID;
    return hg_ctx_display_begin(c, nullptr, format);
}

int hg_readback_begin(hg_ctx* c) { return hg_readback_begin_format(c, HG_DISPLAY_RGBA32F); }

int hg_readback_end_data(hg_ctx* c, const void** data, size_t* n_bytes, int32_t* format) {
    if (!c || !data) return HG_E_INVALID;
    if (c->rb_pending <= 0) return fail(c, HG_E_INVALID, "no readback outstanding: call hg_readback_begin first");
    if (int rc = set_device(c)) return rc;
    const int k = (c->rb_next - c->rb_pending + c->rb_depth) % c->rb_depth;  // the oldest begun
    HG_HIP(c, hipEventSynchronize(c->image_copied[k]));
    c->rb_pending--;
    *data = c->image_host[k];
    if (n_bytes) *n_bytes = c->image_host_bytes[k];
    if (format) *format = c->image_host_format[k];
    return lost_check(c);  // (the image is handed out either way: the accumulation through the last frame blended)
}

int hg_readback_end(hg_ctx* c, const float** rgba, size_t* n_floats) {
    if (!c || !rgba) return HG_E_INVALID;
    if (c->rb_pending <= 0) return fail(c, HG_E_INVALID, "no readback outstanding: call hg_readback_begin first");
    const int k = (c->rb_next - c->rb_pending + c->rb_depth) % c->rb_depth;
    if (c->image_host_format[k] != HG_DISPLAY_RGBA32F)
        return fail(c, HG_E_INVALID, "the oldest readback is in display format %d: use hg_readback_end_data",
                    c->image_host_format[k]);
    const void* data = nullptr;
    size_t bytes = 0;
    if (int rc = hg_readback_end_data(c, &data, &bytes, nullptr)) return rc;
    *rgba = static_cast<const float*>(data);
    if (n_floats) *n_floats = bytes / sizeof(float);
    return HG_OK;
}

int hg_pack_display(const float* rgba, size_t n_pixels, int32_t format, void* out) {
    if ((n_pixels && (!rgba || !out)) || !display_bpp(format)) return HG_E_INVALID;
    for (size_t i = 0; i < n_pixels; ++i) {
        const float* v = rgba + 4 * i;
        if (format == HG_DISPLAY_RGBA32F) {
            std::memcpy(static_cast<float*>(out) + 4 * i, v, 16);
        } else if (format == HG_DISPLAY_RGBA16F) {
            hg_pack_rgba16f(v[0], v[1], v[2], v[3], static_cast<uint32_t*>(out) + 2 * i);
        } else {
            static_cast<uint32_t*>(out)[i] = hg_pack_r11g11b10(v[0], v[1], v[2]);
        }
    }
    return HG_OK;
}

int hg_render(hg_ctx* c, int32_t n_frames, int32_t accumulate) {
    if (!c) return HG_E_INVALID;
    if (int rc = render_check(c, n_frames)) return rc;
    if (int rc = lost_check(c)) return rc;
    if (n_frames == 0) return HG_OK;
    accumulate = accumulate ? 1 : 0;
    if (c->pending_frames > 0 && (accumulate != c->pending_acc || int64_t(c->pending_frames) + n_frames > INT32_MAX))
        if (int rc = hg_ctx_flush(c)) return rc;
    if (c->coalesce <= 1 && c->pending_frames == 0) return render_now(c, n_frames, accumulate);
    // held: the frames follow the held ones (FrameCount advances at the launch; nothing reads it before, every other
    // entry point flushes first)
    c->pending_acc = accumulate;
    c->pending_frames += n_frames;
    return c->pending_frames >= hg_hold_window(plan_input(c, c->pending_frames)) ? hg_ctx_flush(c) : HG_OK;
}

int hg_synchronize(hg_ctx* c) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;
    if (int rc = drain_events(c)) return rc;
    return lost_check(c);
}

int32_t hg_local_tile_count(const hg_ctx* c) { return c ? c->n_local_tiles : 0; }

int hg_readback(hg_ctx* c, float* rgba, size_t n_floats) {
    if (!c || !rgba) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (n_floats < size_t(c->W) * size_t(c->H) * 4) return fail(c, HG_E_INVALID, "readback buffer too small");
    if (int rc = set_device(c)) return rc;
    if (c->n_ranks == 1) {  // the whole image: untiled on the device, one copy into the caller's memory
        size_t bytes = 0;
        if (int rc = untile_async(c, &bytes)) return rc;
        HG_HIP(c, hipMemcpyAsync(rgba, c->image.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HG_HIP(c, hipStreamSynchronize(c->stream));
        if (int rc = drain_events(c)) return rc;
        return lost_check(c);  // (the image is written either way: the accumulation through the last frame blended)
    }
    // this rank's pixels only (the others are left untouched): the tiles are repacked on the host
    std::vector<float4> tiles(size_t(c->n_local_tiles) * 64);
    if (!tiles.empty())
        HG_HIP(c, hipMemcpyAsync(tiles.data(), c->acc.p, tiles.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = drain_events(c)) return rc;
    for_local_pixels(c, [&](size_t slot, size_t pixel) { std::memcpy(rgba + pixel * 4, &tiles[slot], sizeof(float4)); });
    return lost_check(c);
}

int hg_set_accumulation(hg_ctx* c, const float* rgba, size_t n_floats, int32_t frame_count) {
    if (!c || !rgba) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (n_floats < size_t(c->W) * size_t(c->H) * 4) return fail(c, HG_E_INVALID, "accumulation image too small");
    if (frame_count < 1) return fail(c, HG_E_INVALID, "frame_count must be >= 1 (FrameCount starts at 1, RP:152)");
    if (int rc = set_device(c)) return rc;
    // the tile-major repack of hg_readback, inverted; slots of an edge tile outside the image hold 0, as after a clear
    std::vector<float4> tiles(size_t(c->n_local_tiles) * 64, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for_local_pixels(c, [&](size_t slot, size_t pixel) { std::memcpy(&tiles[slot], rgba + pixel * 4, sizeof(float4)); });
    if (!tiles.empty())
        HG_HIP(c, hipMemcpyAsync(c->acc.p, tiles.data(), tiles.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (int rc = reset_lost(c)) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));  // the staging vector dies at return
    c->params.frameCount = frame_count;
    return drain_events(c);
}

int hg_copy_tiles_device(hg_ctx* c, void* dst, size_t n_bytes) {
    if (!c || !dst) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    const size_t need = size_t(c->n_local_tiles) * 64 * sizeof(float4);
    if (n_bytes < need) return fail(c, HG_E_INVALID, "destination too small (%zu < %zu)", n_bytes, need);
    if (int rc = set_device(c)) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));  // every render kernel retired before the copy engine reads acc
    if (need) HG_HIP(c, hipMemcpyAsync(dst, c->acc.p, need, hipMemcpyDeviceToDevice, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = drain_events(c)) return rc;
    return lost_check(c);
}

int hg_get_counters(const hg_ctx* cc, hg_counters* out) {
    hg_ctx* c = const_cast<hg_ctx*>(cc);
    if (!c || !out) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = server_stop(c)) return rc;  // (its waves add their counts when they leave)
    HG_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = drain_events(c)) return rc;
    unsigned long long v[32];
    HG_HIP(c, hipMemcpy(v, c->counters_dev.p, sizeof v, hipMemcpyDeviceToHost));
    *out = c->counters;
    out->paths = v[0];
    out->rays = v[1];
    out->tri_tests = v[2];
    out->aabb_tests = v[3];
    out->mesh_visits = v[4];
    out->sphere_tests = v[5];
    out->hits = v[6];
    out->node_rounds = v[7];
    out->tri_rounds = v[8];
    out->trace_cycles = v[9];
    out->shade_cycles = v[10];
    for (int k = 0; k < 4; ++k) out->shade_detail[k] = v[11 + k];
    out->shade_rounds = v[15];
    out->primary_misses = v[16];
    out->exec_fallbacks = v[17];
    out->order_faults = v[18];
    out->scene_uploads = c->scene_uploads;
    out->scene_uploads_skipped = c->scene_uploads_skipped;
    out->scene_uploads_partial = c->scene_uploads_partial;
    out->scene_uploads_vouched = c->scene_uploads_vouched;
    out->server_launches = c->server_launches;
    out->server_frames = c->server_frames;
    server_note_lost(c);
    out->server_refused = c->server_refused;
    out->server_ahead = c->server_ahead_posts;
    out->frames_lost = c->frames_lost;
    return HG_OK;
}

int hg_reset_counters(hg_ctx* c) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = server_stop(c)) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = drain_events(c)) return rc;
    HG_HIP(c, hipMemset(c->counters_dev.p, 0, c->counters_dev.bytes));
    c->counters = hg_counters{};
    return HG_OK;
}

int64_t hg_selftest(hg_ctx* c, int32_t test, int64_t* tested) {
    if (!c) return HG_E_INVALID;
    if (int rc = set_device(c)) return rc;
    if (test == HG_SELFTEST_BUILD) {  // compile-time checks of this build (no device work)
        if (tested) *tested = 0;
        return (HG_CHECK_EXEC ? HG_BUILD_CHECK_EXEC : 0) | (HG_REGEN_ITEMS ? 0 : HG_BUILD_NO_REGEN_ITEMS);
    }
    if (test != HG_SELFTEST_RCP) return fail(c, HG_E_INVALID, "unknown self-test %d", test);
    const int64_t r = hg_selftest_rcp_all(tested);
    if (r < 0) return fail(c, HG_E_HIP, "self-test failed to run");
    return r;
}

int hg_set_option(hg_ctx* c, int32_t option, int32_t value) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (c->sv.running) {  // every option changes what the server's waves were launched with
        if (int rc = set_device(c)) return rc;
        if (int rc = server_stop(c)) return rc;
    }
    switch (option) {
        case HG_OPT_KERNEL:
            if (value == HG_KERNEL_WAVEFRONT || value == HG_KERNEL_MEGA_POOL)
                return fail(c, HG_E_UNSUPPORTED, "kernel variant %d was measured, rejected and removed (DESIGN.md section 10)",
                            value);
            if (value != HG_KERNEL_MEGA && value != HG_KERNEL_MEGA_REGEN && value != HG_KERNEL_MEGA_STREAM &&
                value != HG_KERNEL_AUTO)
                return fail(c, HG_E_INVALID, "unknown kernel variant %d", value);
            c->kernel = value;
            return HG_OK;
        case HG_OPT_BLOCK:
            if (value != 64 && value != 128 && value != 256) return fail(c, HG_E_INVALID, "block must be 64/128/256");
            c->block = value;
            return HG_OK;
        case HG_OPT_COUNTERS:
            c->counters_on = value ? 1 : 0;
            return HG_OK;
        case HG_OPT_TIMING:
            c->timing = value ? 1 : 0;
            return HG_OK;
        case HG_OPT_REFILL:  // the wavefront pipeline's dequeue threshold
            return fail(c, HG_E_UNSUPPORTED, "HG_OPT_REFILL: the wavefront pipeline was removed (DESIGN.md section 10)");
        case HG_OPT_DESCENT_T:
            if (value < -1 || value > 64) return fail(c, HG_E_INVALID, "descent threshold must be -1 (auto)..64");
            c->descent_t = value;
            return HG_OK;
        case HG_OPT_TILE_ORDER:
            c->tile_order_on = value ? 1 : 0;
            for (hg_ctx::TraceLane& L : c->lanes) L.tile_cost_valid = L.tile_order_valid = false;
            return HG_OK;
        case HG_OPT_COALESCE:
            if (value < 1 || value > 65535) return fail(c, HG_E_INVALID, "coalesce window must be 1..65535 frames");
            c->coalesce = value;
            return HG_OK;
        case HG_OPT_READBACK_DEPTH:
            if (value < 1 || value > HG_READBACK_MAX)
                return fail(c, HG_E_INVALID, "readback depth must be 1..%d", HG_READBACK_MAX);
            if (c->rb_pending) return fail(c, HG_E_INVALID, "readbacks outstanding: end them before changing the depth");
            c->rb_depth = value;
            c->rb_next = 0;
            return HG_OK;
        case HG_OPT_READBACK_STREAM:
            if (c->rb_pending) return fail(c, HG_E_INVALID, "readbacks outstanding: end them before changing the stream");
            if (value < 0 || value > 2) return fail(c, HG_E_INVALID, "HG_OPT_READBACK_STREAM %d: expected 0, 1 or 2", value);
            c->rb_side = value;
            return HG_OK;
        case HG_OPT_FRAME_SPLIT:
            if (value < 0 || value > 4096) return fail(c, HG_E_INVALID, "frame split must be 0 (auto)..4096");
            c->frame_split = value;
            return HG_OK;
        case HG_OPT_LANE_PICK:
            c->lane_pick = value ? 1 : 0;
            return HG_OK;
        case HG_OPT_SERVER:
            if (value < 0 || value > 2) return fail(c, HG_E_INVALID, "HG_OPT_SERVER %d: expected 0, 1 or 2", value);
            c->server_on = value;
            return HG_OK;
        case HG_OPT_QUEUE_FILL:
            if (value < 0 || value > 64) return fail(c, HG_E_INVALID, "queue fill threshold must be 0 (off)..64 rounds");
            c->queue_fill = value;
            return HG_OK;
        case HG_OPT_SERVER_AHEAD:
            if (value < 0 || value > HG_SV_RING - 2) return fail(c, HG_E_INVALID, "server ahead must be 0..%d", HG_SV_RING - 2);
            c->sv_ahead = value;
            return HG_OK;
        case HG_OPT_SERVER_IDLE_US:
            if (value < 0 || value > 40000000) return fail(c, HG_E_INVALID, "server idle time must be 0..40000000 us");
            c->sv.idle_us = value;
            return HG_OK;
        case HG_OPT_SERVER_GATE_US:
            c->sv.gate_us = value;  // (< 0: the default)
            return HG_OK;
        case HG_OPT_WAVE_UNITS:
            if (value < 0 || value > HG_WAVE_UNITS_LIMIT)
                return fail(c, HG_E_INVALID, "wave units must be 0 (auto)..%d", HG_WAVE_UNITS_LIMIT);
            c->wave_units = value;
            return HG_OK;
        default:
            return fail(c, HG_E_INVALID, "unknown option %d", option);
    }
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// Ray queries (hg_trace_rays, hg_trace_rays_device, hg_camera_rays; kernels in hg_query.hip)
// ---------------------------------------------------------------------------------------------------------------------
uint32_t hg_query_threads(uint32_t n);
uint32_t hg_query_lds_stack();
hipError_t hg_launch_query(const HgKernelParams& kp, const void* rays, void* hits, uint32_t n, bool any,
                           hipStream_t stream);
hipError_t hg_launch_camera_rays(const HgKernelParams& kp, uint32_t frame, const void* pixels, void* rays, uint32_t n,
                                 hipStream_t stream);

namespace {

constexpr int64_t kQueryChunk = int64_t(1) << 20;  // records per launch (and per staging buffer)

// What every entry point but hg_render does first, as far as hg_synchronize takes it: the held frames launched, the
// render server stopped, every stream of the context idle
int query_begin(hg_ctx* c) {
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = set_device(c)) return rc;
    return quiesce(c);
}

// The parameter block of a query launch of `threads` threads: the uploaded scene (all of it: no bufferCounts, no
// tiling), far = +inf, the lockstep kernel's descent threshold; nothing of the target, the uniforms or the counters
int query_params(hg_ctx* c, uint32_t threads, HgKernelParams& kp) {
    kp = HgKernelParams{};
    kp.far_ = HG_INF;
    kp.n_spheres = c->n_spheres;
    kp.n_meshes = c->n_meshes;
    set_scene(kp, c, hg_descent_t(c->descent_t, c->stack_depth, HG_KERNEL_MEGA));
    kp.spill_stride = threads;
    const uint32_t lds_part = hg_query_lds_stack();
    if (kp.stack_depth > lds_part) {  // one spill column per thread (the context is idle: the buffer may move)
        if (int rc = ensure(c, c->spill, size_t(threads) * (kp.stack_depth - lds_part) * sizeof(uint32_t))) return rc;
        kp.spill = static_cast<uint32_t*>(c->spill.p);
    }
    return HG_OK;
}

int query_args(hg_ctx* c, const void* in, int64_t n, int32_t mode, const void* out) {
    if (n < 0) return fail(c, HG_E_INVALID, "negative ray count");
    if (mode != HG_RAYS_CLOSEST && mode != HG_RAYS_ANY) return fail(c, HG_E_INVALID, "unknown ray query mode %d", mode);
    if (!in || !out) return fail(c, HG_E_INVALID, "null array with a non-zero ray count");
    if (!c->has_scene) return fail(c, HG_E_NOSCENE, "hg_upload_scene not called");
    return HG_OK;
}

// n rays at device pointers, in launches of at most kQueryChunk; the context is idle (query_begin) and the caller waits
// for the stream
int query_launch(hg_ctx* c, const void* d_rays, int64_t n, int32_t mode, void* d_hits) {
    HgKernelParams kp;
    if (int rc = query_params(c, hg_query_threads(uint32_t(std::min(n, kQueryChunk))), kp)) return rc;
    for (int64_t at = 0; at < n; at += kQueryChunk) {
        const uint32_t m = uint32_t(std::min(n - at, kQueryChunk));
        HG_HIP(c, hg_launch_query(kp, static_cast<const hg_ray*>(d_rays) + at, static_cast<hg_ray_hit*>(d_hits) + at, m,
                                  mode == HG_RAYS_ANY, c->stream));
    }
    return HG_OK;
}

}  // namespace

extern "C" {

int hg_trace_rays_device(hg_ctx* c, const void* d_rays, int64_t n, int32_t mode, void* d_hits) {
    if (!c) return HG_E_INVALID;
    if (n == 0) return HG_OK;
    if (int rc = query_args(c, d_rays, n, mode, d_hits)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_rays) | reinterpret_cast<uintptr_t>(d_hits)) & 15u)
        return fail(c, HG_E_INVALID, "device ray / hit arrays must be 16-byte aligned");
    if (int rc = query_begin(c)) return rc;
    if (int rc = query_launch(c, d_rays, n, mode, d_hits)) return rc;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

int hg_trace_rays(hg_ctx* c, const hg_ray* rays, int64_t n, int32_t mode, hg_ray_hit* hits) {
    if (!c) return HG_E_INVALID;
    if (n == 0) return HG_OK;
    if (int rc = query_args(c, rays, n, mode, hits)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        const hg_ray& r = rays[i];
        if (!(std::isfinite(r.origin.x) && std::isfinite(r.origin.y) && std::isfinite(r.origin.z)))
            return fail(c, HG_E_INVALID, "ray %lld: origin is not finite", (long long)i);
        if (!(std::isfinite(r.direction.x) && std::isfinite(r.direction.y) && std::isfinite(r.direction.z)))
            return fail(c, HG_E_INVALID, "ray %lld: direction is not finite", (long long)i);
        if (r.direction.x == 0.0f && r.direction.y == 0.0f && r.direction.z == 0.0f)
            return fail(c, HG_E_INVALID, "ray %lld: zero direction", (long long)i);
        if (std::isnan(r.t_max)) return fail(c, HG_E_INVALID, "ray %lld: t_max is NaN", (long long)i);
    }
    if (int rc = query_begin(c)) return rc;
    const size_t cap = size_t(std::min(n, kQueryChunk));
    if (int rc = ensure(c, c->query_in, cap * sizeof(hg_ray))) return rc;
    if (int rc = ensure(c, c->query_out, cap * sizeof(hg_ray_hit))) return rc;
    for (int64_t at = 0; at < n; at += kQueryChunk) {  // in stream order: a chunk's copies and launch reuse the staging
        const size_t m = size_t(std::min(n - at, kQueryChunk));
        HG_HIP(c, hipMemcpyAsync(c->query_in.p, rays + at, m * sizeof(hg_ray), hipMemcpyHostToDevice, c->stream));
        if (int rc = query_launch(c, c->query_in.p, int64_t(m), mode, c->query_out.p)) return rc;
        HG_HIP(c, hipMemcpyAsync(hits + at, c->query_out.p, m * sizeof(hg_ray_hit), hipMemcpyDeviceToHost, c->stream));
    }
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

int hg_camera_rays(hg_ctx* c, const hg_params* p, int32_t frame_count, const int32_t* pixels_xy, int64_t n,
                   hg_ray* rays) {
    if (!c) return HG_E_INVALID;
    if (n == 0) return HG_OK;
    if (n < 0) return fail(c, HG_E_INVALID, "negative pixel count");
    if (!p || !pixels_xy || !rays) return fail(c, HG_E_INVALID, "null params or array with a non-zero pixel count");
    const float Wf = p->screenParameters.x, Hf = p->screenParameters.y;
    if (!(Wf >= 1.0f && Hf >= 1.0f && Wf <= 65536.0f && Hf <= 65536.0f))
        return fail(c, HG_E_INVALID, "screenParameters (%g,%g) out of range", Wf, Hf);
    const int32_t W = int32_t(Wf), H = int32_t(Hf);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t x = pixels_xy[2 * i], y = pixels_xy[2 * i + 1];
        if (x < 0 || x >= W || y < 0 || y >= H)
            return fail(c, HG_E_INVALID, "pixel %lld: (%d,%d) outside the %dx%d screen", (long long)i, x, y, W, H);
    }
    if (int rc = query_begin(c)) return rc;
    HgKernelParams kp{};
    set_camera(kp, *p);
    const size_t cap = size_t(std::min(n, kQueryChunk));
    if (int rc = ensure(c, c->query_in, cap * 2 * sizeof(int32_t))) return rc;
    if (int rc = ensure(c, c->query_out, cap * sizeof(hg_ray))) return rc;
    for (int64_t at = 0; at < n; at += kQueryChunk) {
        const size_t m = size_t(std::min(n - at, kQueryChunk));
        HG_HIP(c, hipMemcpyAsync(c->query_in.p, pixels_xy + 2 * at, m * 2 * sizeof(int32_t), hipMemcpyHostToDevice,
                                 c->stream));
        HG_HIP(c, hg_launch_camera_rays(kp, uint32_t(frame_count), c->query_in.p, c->query_out.p, uint32_t(m), c->stream));
        HG_HIP(c, hipMemcpyAsync(rays + at, c->query_out.p, m * sizeof(hg_ray), hipMemcpyDeviceToHost, c->stream));
    }
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// Denoised display (hg_update_guides, hg_readback_guides, hg_readback_begin_denoised; kernels in hg_denoise.hip, the
// filter's arithmetic in hg_atrous.h)
// ---------------------------------------------------------------------------------------------------------------------
uint32_t hg_guides_threads(uint32_t n);
hipError_t hg_launch_guides(const HgKernelParams& kp, uint32_t frame, void* guide0, void* guide1, uint32_t first,
                            uint32_t n, hipStream_t stream);
hipError_t hg_launch_denoise(const void* acc, const void* guide0, const void* guide1, void* const work[2], int32_t W,
                             int32_t H, int32_t tiles_x, const hg_denoise_params& p, hipStream_t stream,
                             const void** result);

extern "C" {

int hg_update_guides(hg_ctx* c, const hg_params* p, int32_t frame_count) {
    if (!c) return HG_E_INVALID;
    if (!p) return fail(c, HG_E_INVALID, "null params");
    if (!c->has_scene) return fail(c, HG_E_NOSCENE, "hg_upload_scene not called");
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (!(p->screenParameters.x == float(c->W) && p->screenParameters.y == float(c->H)))
        return fail(c, HG_E_INVALID, "screenParameters (%g,%g) are not the target's size %dx%d", p->screenParameters.x,
                    p->screenParameters.y, c->W, c->H);
    if (int rc = query_begin(c)) return rc;
    // the context is idle: the four images may move
    c->guides_valid = false;
    const size_t pixels = size_t(c->W) * size_t(c->H);
    for (DevBuf* b : {&c->guide0, &c->guide1, &c->denoise_work[0], &c->denoise_work[1]})
        if (int rc = ensure(c, *b, pixels * sizeof(float4))) return rc;
    // the closest-hit query's parameter block (the whole uploaded scene, far = +inf) with the caller's camera
    HgKernelParams kp;
    if (int rc = query_params(c, hg_guides_threads(uint32_t(std::min<size_t>(pixels, size_t(kQueryChunk)))), kp)) return rc;
    const float far_ = kp.far_;
    set_camera(kp, *p);
    kp.far_ = far_;
    for (size_t at = 0; at < pixels; at += size_t(kQueryChunk)) {  // in stream order: the launches share the spill buffer
        const uint32_t m = uint32_t(std::min(pixels - at, size_t(kQueryChunk)));
        HG_HIP(c, hg_launch_guides(kp, uint32_t(frame_count), c->guide0.p, c->guide1.p, uint32_t(at), m, c->stream));
    }
    HG_HIP(c, hipStreamSynchronize(c->stream));
    c->guides_valid = true;
    return HG_OK;
}

int hg_readback_guides(hg_ctx* c, float* guide0, float* guide1, size_t n_floats_each) {
    if (!c) return HG_E_INVALID;
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (!c->guides_valid) return fail(c, HG_E_INVALID, "no guide images for this scene and target: call hg_update_guides");
    const size_t bytes = size_t(c->W) * size_t(c->H) * sizeof(float4);
    if (n_floats_each * sizeof(float) < bytes) return fail(c, HG_E_INVALID, "guide buffer too small");
    if (int rc = set_device(c)) return rc;
    if (guide0) HG_HIP(c, hipMemcpyAsync(guide0, c->guide0.p, bytes, hipMemcpyDeviceToHost, c->stream));
    if (guide1) HG_HIP(c, hipMemcpyAsync(guide1, c->guide1.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
}

int hg_readback_begin_denoised(hg_ctx* c, int32_t format, const hg_denoise_params* p) {
    if (!c) return HG_E_INVALID;
    if (!p) return fail(c, HG_E_INVALID, "null denoise params");
    if (!hg_atrous_params_ok(*p))
        return fail(c, HG_E_INVALID,
                    "bad denoise params: iterations %d (1..%d), sigmas %g %g %g (off, or in [1e-4, 1e4]), demodulate %d, "
                    "flags %u", p->iterations, HG_ATROUS_MAX_ITERATIONS, p->sigma_color, p->sigma_normal, p->sigma_depth,
                    p->demodulate, p->flags);
    if (int rc = hg_ctx_flush(c)) return rc;
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (!display_bpp(format)) return fail(c, HG_E_INVALID, "unknown display format %d", format);
    if (c->n_ranks > 1)
        return fail(c, HG_E_UNSUPPORTED, "denoised display of a tiled context (rank %d of %d): a rank's share has no "
                    "neighbours", c->rank, c->n_ranks);
    if (int64_t(c->W) * c->H > HG_ATROUS_MAX_PIXELS)
        return fail(c, HG_E_UNSUPPORTED, "denoised display of more than 2^28 pixels (%dx%d)", c->W, c->H);
    if (!c->guides_valid) return fail(c, HG_E_INVALID, "no guide images for this scene and target: call hg_update_guides");
    if (c->rb_pending >= c->rb_depth)
        return fail(c, HG_E_INVALID, "%d readbacks outstanding (HG_OPT_READBACK_DEPTH): call hg_readback_end first",
                    c->rb_pending);
    if (int rc = set_device(c)) return rc;
    // on the context stream, after every frame rendered so far (the server keeps tracing: nothing here waits)
    void* const work[2] = {c->denoise_work[0].p, c->denoise_work[1].p};
    const void* denoised = nullptr;
    HG_HIP(c, hg_launch_denoise(c->acc.p, c->guide0.p, c->guide1.p, work, c->W, c->H, c->tiles_x, *p, c->stream, &denoised));
    return hg_ctx_display_begin(c, denoised, format);
}

}  // extern "C"
