// hg_rt.h — what the runtime's translation units (hg_runtime.hip, hg_render.hip, hg_display.hip, hg_query.hip,
// hg_denoise.hip, hg_refit.hip, hg_lbvh.hip, hg_deform.hip, hg_comm.hip) share over a context: private to libhalogen_hip.so, none of it in the C-ABI.  The
// helpers are in namespace hgrt (each is defined in the file named beside it); the hg_ctx_* functions are the
// context's services to hg_comm.hip and to each other.
#pragma once
#include "hg_ctx.h"
#include "hg_pair_guard.h"
#include "hg_tiling.h"

// Launch the held frames of a context, if any (hg_render.hip; every entry point but hg_render calls it first)
int hg_ctx_flush(hg_ctx* c);
// The context's accumulation is invalid (a render server frame was lost; reads the gates' report first) (hg_render.hip)
bool hg_ctx_lost(hg_ctx* c);
// Enqueue a display readback (hg_readback_begin_format) from the accumulator (rows == nullptr) or from a row-major
// float4 image of the target's size on the context's device; and the copy event of the oldest outstanding one
// (hg_display.hip)
int hg_ctx_display_begin(hg_ctx* c, const void* rows, int32_t format);
hipEvent_t hg_ctx_display_oldest(const hg_ctx* c);

namespace hgrt {

using EventPair = std::pair<hipEvent_t, hipEvent_t>;
using EventGuard = HgPairGuard<EventPair>;  // a timing pair that goes back to free_events unless handed on

// ---- hg_runtime.hip ----
// Keep the text as the context's last error; returns `code`
int fail(hg_ctx* c, int code, const char* fmt, ...);

#define HG_HIP(ctx, call)                                                                                    \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return hgrt::fail((ctx), HG_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

int set_device(hg_ctx* c);
// Device buffers of a context: free; (re)allocate to exactly the size and copy on the context stream; grow, in plain
// or in uncached device memory.  At least 16 bytes each.
void release(DevBuf& b);
int upload(hg_ctx* c, DevBuf& b, const void* src, size_t bytes);
int ensure(hg_ctx* c, DevBuf& b, size_t bytes);
int ensure_uncached(hg_ctx* c, DevBuf& b, size_t bytes);
// Wait for every stream of the context (the render server is stopped first)
int quiesce(hg_ctx* c);
// Timing: the elapsed times of the launches queued so far into the counters (waits for the context stream); a timing
// pair from the free list
int drain_events(hg_ctx* c);
int event_pair(hg_ctx* c, EventGuard& g);
// A stream with an all-CU mask (a hardware queue of its own); and a trace stream, which is one beyond the first
// HG_TRACE_LANES_BIG lanes, or a plain stream where the runtime refuses CU masks
hipError_t create_masked_stream(const hg_ctx* c, hipStream_t* s);
hipError_t create_lane_stream(const hg_ctx* c, int lane, hipStream_t* s);

// The pixels of this rank's local tiles that lie in the image: f(accumulator slot, image pixel) (hg_tiling.h)
template <class F>
void for_local_pixels(const hg_ctx* c, F&& f) {
    hg_for_local_pixels(uint32_t(c->W), uint32_t(c->H), uint32_t(c->n_local_tiles), uint32_t(c->rank),
                        uint32_t(c->n_ranks), f);
}

// ---- hg_render.hip ----
void sv_trace(const char* fmt, ...);  // HALOGEN_SERVER_TRACE=1: the server's starts, stops, posts on stderr
int server_stop(hg_ctx* c);
void server_note_lost(hg_ctx* c);
int lost_check(hg_ctx* c);
int reset_lost(hg_ctx* c);
// The camera and the scene part of a launch's parameter block
void set_camera(HgKernelParams& kp, const hg_params& p);
void set_scene(HgKernelParams& kp, const hg_ctx* c, uint32_t descent_t);

// ---- hg_display.hip ----
size_t display_bpp(int32_t format);  // bytes per pixel of a display format, 0 for an unknown one
// What every display begin checks first: a target, a known format, a free slot in the ring
int display_check(hg_ctx* c, int32_t format);

// ---- hg_query.hip ----
constexpr int64_t kQueryChunk = int64_t(1) << 20;  // records per launch (and per staging buffer)
int query_begin(hg_ctx* c);
int query_params(hg_ctx* c, uint32_t threads, HgKernelParams& kp);

// ---- hg_refit.hip ----
// Forget the refit plans of the device scene and free their device lists (a full upload lays the records out anew)
void refit_reset(hg_ctx* c);
// Everything hg_refit_mesh* checks before the first device write.  On success: the tree (its plan built and cached on
// first use; every other tree's plan is cached too) and the meshes refitted together.  Then the refit itself, from
// n_tris HalogenTriangle on the device (4-byte aligned), for a context that is quiesced (hg_lbvh.hip runs both too)
int refit_check(hg_ctx* c, int32_t mesh_index, const void* tris, int32_t n_tris, hg_ctx::RefitTree*& tree,
                std::vector<int32_t>& instances);
int refit_device(hg_ctx* c, hg_ctx::RefitTree& tree, const std::vector<int32_t>& instances, const void* d_tris,
                 int32_t n_tris, uint64_t geometry_generation);

// ---- hg_deform.hip ----
// After a rebuild of the tree at `tri_offset`: if an index list is bound to it (hg_set_mesh_vertices), permute it on the
// context stream by the rebuild's order (d_order: n_tris uint32 on the device), so it stays in the tree's triangle order
int deform_follow_order(hg_ctx* c, uint32_t tri_offset, const uint32_t* d_order, uint32_t n_tris);

}  // namespace hgrt
