// hg_render.hip — rendering: the host half of the render server (hg_ctx::Server; device side hg_mega.hip kServer, hg_server.h), the
// trace pipeline (chunks traced on the trace streams, blended in frame order on the context stream), render_now, which
// launches what the plan of hg_plan.h decides, and hg_render / hg_ctx_flush, which hold and release frames.  Stands in
// for the DispatchCompute / Blit calls of Assets/Scripts/Render Features/HalogenRenderPass.cs (RP:237-508).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "hg_fmath.h"
#include "hg_rt.h"
#include "hg_launch.h"
#include "hg_plan.h"

namespace hgrt {

static double host_seconds() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
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
    // yet claimed are abandoned (the waves' view drops to it, hg_server.h sv_view)
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

// The camera part of a launch's parameter block (everything camera_ray reads, hg_dev_shade.h) from the uniforms
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
    kp.cull = static_cast<const float4*>(c->cull.p);
    kp.n_cull = hg_cull_count(c->cull_table, kp.n_meshes);  // (the caller has set kp.n_meshes)
    kp.materials = static_cast<const float4*>(c->materials.p);
    kp.n_materials = c->n_materials;
    kp.nodes = static_cast<const float4*>(c->nodes.p);
    kp.leaves = static_cast<const uint2*>(c->leaves.p);
    kp.tris = static_cast<const float*>(c->tris.p);
    kp.normals = static_cast<const float4*>(c->normals.p);
}

namespace {

// ---- the render server (hg_ctx::Server; device side hg_mega.hip kServer, hg_server.h) ------------------------------------------
// The server closes itself after HG_OPT_SERVER_IDLE_US with nothing posted (the close handshake, hg_server.h sv_close:
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

// Grow a trace stream's buffer; only when that buffer is not in use (quiesce first if it must move)
int ensure_quiet(hg_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= std::max<size_t>(bytes, 16)) return HG_OK;
    if (int rc = quiesce(c)) return rc;
    return ensure(c, b, bytes);
}

// The cost order of a trace stream (its tile_cost, tile_order and order_scratch).  Two steps, because a call grows every
// trace stream's buffers before it queues its first chunk and sorts per chunk.  Grow, only while the buffers are not
// in use: the sort's scratch is zeroed once, when allocated (each use leaves it zeroed).
int cost_order_ensure(hg_ctx* c, hg_ctx::TraceLane& L, uint32_t tiles) {
    const size_t tb = size_t(tiles) * sizeof(uint32_t);
    if (int rc = ensure_quiet(c, L.tile_cost, 2 * tb)) return rc;
    if (int rc = ensure_quiet(c, L.tile_order, tb)) return rc;
    const size_t osb = hg_order_scratch_bytes(tiles);
    if (L.order_scratch.bytes >= osb) return HG_OK;
    if (int rc = ensure_quiet(c, L.order_scratch, osb)) return rc;
    if (hipMemsetAsync(L.order_scratch.p, 0, L.order_scratch.bytes, L.stream) != hipSuccess)
        return fail(c, HG_E_HIP, "hipMemsetAsync(order scratch) failed");
    return HG_OK;
}
// Use: sort the recorded costs into the order (`sort`), or zero the costs before their first records
hipError_t cost_order_run(hg_ctx* c, hg_ctx::TraceLane& L, uint32_t tiles, bool sort) {
    unsigned long long* cost = static_cast<unsigned long long*>(L.tile_cost.p);
    if (!sort) return hipMemsetAsync(cost, 0, size_t(tiles) * sizeof(unsigned long long), L.stream);
    return hg_launch_order_tiles(cost, static_cast<uint32_t*>(L.tile_order.p), tiles, L.order_scratch.p,
                                 static_cast<unsigned long long*>(c->counters_dev.p) + 18, L.stream);
}

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

// Launch the server for the frames from FrameCount `fc`: kp is the launch's parameter block as render_now built it.
// HG_E_UNSUPPORTED when the device gives no stream with a hardware queue of its own (the server's
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
        if (create_masked_stream(c, &S.stream) != hipSuccess) {
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
    if (!rc) rc = ensure_uncached(c, S.ctl, HG_SV_CTL_BYTES);  // (polled by scalar loads: hg_dev_wave.h sv_sload)
    if (!rc && spill_bytes) rc = ensure(c, S.spill, spill_bytes);
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
    // raster order, no cost records: the server's frames overlap, so no frame's end waits on its longest tiles, and
    // raster order keeps a claim's consecutive tiles together (the cost order was measured and removed)
    HgKernelParams kp = kp_in;
    kp.tile_order = nullptr;
    kp.tile_cost = nullptr;
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

// Post frame k = S.posted to the server: the host's half of the close handshake (hg_server.h sv_close).  Raise the post
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
        if (!rc && P.ordered) rc = cost_order_ensure(c, L, uint32_t(c->n_local_tiles));
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

}  // namespace hgrt

using namespace hgrt;

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

extern "C" {

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

}  // extern "C"
