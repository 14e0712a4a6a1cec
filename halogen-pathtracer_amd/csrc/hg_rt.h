// hg_rt.h — what the runtime's translation units (hg_runtime.hip, hg_render.hip, hg_display.hip, hg_query.hip,
// hg_denoise.hip, hg_refit.hip, hg_lbvh.hip, hg_deform.hip, hg_comm.hip) share over a context: private to
// libhalogen_hip.so, none of it in the C-ABI.  The helpers are in namespace hgrt (each is defined in the file named
// beside it); the hg_ctx_* functions are the context's services to hg_comm.hip and to each other.
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
// Keep the text as the context's last error; returns `code`.  Or a refusal of the host-only headers, as it stands
int fail(hg_ctx* c, int code, const char* fmt, ...);
int fail(hg_ctx* c, const HgPackError& err);

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

// ---- mesh updates: hg_refit.hip, hg_lbvh.hip, hg_deform.hip ----
constexpr int kTriWords = 18;  // floats of a HalogenTriangle
static_assert(sizeof(HalogenTriangle) == 72, "the kernels move a triangle as 18 floats");

// One update of one mesh of the device scene: what the ten entry points hg_refit_mesh, hg_rebuild_mesh,
// hg_rebuild_mesh_sah, hg_deform_mesh, hg_skin_mesh and their _device forms fill in
struct MeshUpdate {
    const char* who;  // the entry point, for its messages
    int32_t mesh_index;
    enum Source { kTriangles, kVertices, kBones } source;
    const void* a;  // `count` 72-byte triangles | vertex positions | row-major 3 x 4 bone matrices
    const void* b;  // nullptr                   | vertex normals   | nullptr
    int32_t count;
    bool device;    // a, b and order are device pointers (else host pointers)
    int32_t how;    // HG_DEFORM_REFIT, HG_DEFORM_REBUILD (leaf_size) or HG_DEFORM_REBUILD_SAH (node_cost); no flag bits
    int32_t leaf_size;
    float node_cost;
    void* order;  // optional: where a rebuild's order goes
    uint64_t generation;
    // HG_DEFORM_NORMALS (vertices, bones): the vertex normals are recomputed from the moved faces; b is nullptr
    bool recompute_normals = false;
};
// The one path of them all (hg_refit.hip; its header has the steps)
int update_mesh(hg_ctx* c, const MeshUpdate& u);
// Forget the trees of the device scene, their device lists and the vertex bindings (a full upload lays the records out
// anew) (hg_refit.hip)
void refit_reset(hg_ctx* c);
// The two kinds of build of a rebuild, for a quiesced context, from n triangles on the device: the new records' refs
// into the scene's nodes from slot.rec_min on and, compact, into c->lbvh.refs; the triangles in the new order into
// c->lbvh.tris; the order into c->lbvh.index_sorted and d_order (optional).  By surface area: refuses, before the first
// write to the scene, a tree whose n_records do not fit the slot (hg_lbvh.hip)
int build_lbvh_device(hg_ctx* c, uint32_t tri_offset, const HgMeshTrees::Slot& slot, uint32_t L, uint32_t K,
                      const void* d_tris, uint32_t n, void* d_order);
int build_sah_device(hg_ctx* c, int32_t mesh_index, uint32_t tri_offset, const HgMeshTrees::Slot& slot, float node_cost,
                     const void* d_tris, uint32_t n, void* d_order, uint32_t& n_records);
// An update whose source is vertices or a bone palette: the checks of the source (the binding first), and the source as
// the binding's triangles in c->refit_in on the context stream (hg_deform.hip)
int vertex_source_check(hg_ctx* c, const MeshUpdate& u, hg_ctx::VertexBinding*& b);
int vertex_source_device(hg_ctx* c, const MeshUpdate& u, hg_ctx::VertexBinding& b);
void release_binding(hg_ctx::VertexBinding& b);
// After a rebuild of the tree at `tri_offset`: if an index list is bound to it (hg_set_mesh_vertices), permute it on the
// context stream by the rebuild's order (d_order: n_tris uint32 on the device), so it stays in the tree's triangle order
// (hg_deform.hip)
int deform_follow_order(hg_ctx* c, uint32_t tri_offset, const uint32_t* d_order, uint32_t n_tris);

}  // namespace hgrt
