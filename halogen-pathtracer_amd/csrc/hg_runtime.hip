// hg_runtime.hip — the context behind the C-ABI of include/halogen_abi.h: create / destroy, device buffers, scene and
// cubemap upload, params / resize / tiling / clear, options, counters, self-test, synchronize.  Rendering is
// hg_render.hip's, display readback hg_display.hip's, ray queries hg_query.hip's, the denoised display
// hg_denoise.hip's, the refit of a deforming mesh hg_refit.hip's; what they share is declared in hg_rt.h.  Stands in for the ComputeBuffer / RTHandle calls of
// Assets/Scripts/Render Features/HalogenRenderPass.cs (RP:237-508).
//
// Error model: every entry point returns HG_OK or a negative HG_E_* code and never aborts; the text of
// the last error is kept per context (hg_last_error).  There is no CPU fallback: a missing GPU or a HIP
// failure is an error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hg_rt.h"
#include "hg_launch.h"
#include "hg_interval.h"
#include "hg_scene_pack.h"

// hg_scene_pack.h packs with HIP's vector types here and with its own plain structs under g++ (its tests): the same bytes
#ifdef HG_VECTOR_SHIM
#error "hg_scene_pack.h defined its float4 / uint2 shim in a HIP translation unit"
#endif
static_assert(sizeof(float4) == HG_FLOAT4_BYTES && alignof(float4) == HG_FLOAT4_BYTES, "float4 differs from the shim");
static_assert(sizeof(uint2) == HG_UINT2_BYTES && alignof(uint2) == HG_UINT2_BYTES, "uint2 differs from the shim");
static_assert(sizeof(HgDevMesh) == 144 && alignof(HgDevMesh) == 16, "HgDevMesh is 144 B (hg_layout.h)");

namespace hgrt {

int fail(hg_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

int fail(hg_ctx* c, const HgPackError& err) { return fail(c, err.code, "%s", err.text.c_str()); }

int set_device(hg_ctx* c) {
    HG_HIP(c, hipSetDevice(c->device));
    return HG_OK;
}

void release(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

// `b` freed and allocated again with `bytes` bytes, in plain or in uncached device memory
static int reallocate(hg_ctx* c, DevBuf& b, size_t bytes, bool uncached) {
    release(b);
    const hipError_t e = uncached ? hipExtMallocWithFlags(&b.p, bytes, hipDeviceMallocUncached) : hipMalloc(&b.p, bytes);
    if (e != hipSuccess)
        return fail(c, HG_E_NOMEM, uncached ? "hipExtMallocWithFlags(%zu, uncached) failed: %s" : "hipMalloc(%zu) failed: %s",
                    bytes, hipGetErrorString(e));
    b.bytes = bytes;
    return HG_OK;
}

int upload(hg_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    const size_t alloc = std::max<size_t>(bytes, 16);  // the reference allocates >= 1 element (RP:544)
    if (b.bytes != alloc)
        if (int rc = reallocate(c, b, alloc, false)) return rc;
    if (bytes) HG_HIP(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return HG_OK;
}

int ensure(hg_ctx* c, DevBuf& b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    return b.bytes >= bytes ? HG_OK : reallocate(c, b, bytes, false);
}

// The same in uncached device memory (MTYPE UC: no L2 holds its lines, so writes from one XCD are seen by loads from
// any other without cache maintenance): the render server's colour ring and frame counts, written by persistent
// waves and read by the gate and blend kernels while those waves still run
int ensure_uncached(hg_ctx* c, DevBuf& b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    return b.bytes >= bytes ? HG_OK : reallocate(c, b, bytes, true);
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

// A stream with an all-CU mask: a hardware queue of its own.  (Plain streams share HIP's pool of GPU_MAX_HW_QUEUES (4)
// hardware queues with every other stream of the process; CU-masked streams are blocking with respect to the legacy
// null stream, unlike the plain ones.)
hipError_t create_masked_stream(const hg_ctx* c, hipStream_t* s) {
    std::vector<uint32_t> mask(size_t((c->n_cu + 31) / 32), 0u);
    for (int i = 0; i < c->n_cu; ++i) mask[size_t(i) / 32] |= 1u << (i % 32);
    const hipError_t e = hipExtStreamCreateWithCUMask(s, uint32_t(mask.size()), mask.data());
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

// A trace stream (HG_LANE_STREAMS): two trace streams on one hardware queue serialise their launches.  Where the
// runtime refuses CU masks, a plain stream: the same results, only the queue sharing comes back.
hipError_t create_lane_stream(const hg_ctx* c, int lane, hipStream_t* s) {
    if (lane >= HG_TRACE_LANES_BIG && create_masked_stream(c, s) == hipSuccess) return hipSuccess;
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

}  // namespace hgrt

using namespace hgrt;

namespace {

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
    if (int rc = reset_lost(c)) return rc;
    const size_t bytes = size_t(c->n_local_tiles) * 64 * sizeof(float4);
    c->rb.reset();  // quiesced: begun readbacks are complete, and their images die with the old size or tiling
    release(c->acc);
    if (bytes) {
        hipError_t e = hipMalloc(&c->acc.p, bytes);
        if (e != hipSuccess) return fail(c, HG_E_NOMEM, "hipMalloc(accumulation %zu) failed", bytes);
        c->acc.bytes = bytes;
        HG_HIP(c, hipMemsetAsync(c->acc.p, 0, bytes, c->stream));
    }
    return HG_OK;
}

// The HIP objects a context has from the start: its stream, events, counters, lost-frame word and trace streams
bool create_objects(hg_ctx* c) {
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->call_done[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->call_done[1], hipEventDisableTiming) != hipSuccess ||
        hipMalloc(&c->counters_dev.p, 32 * sizeof(unsigned long long)) != hipSuccess)
        return false;
    c->counters_dev.bytes = 32 * sizeof(unsigned long long);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return false;
    c->n_cu = prop.multiProcessorCount;
    if (ensure_uncached(c, c->lost, 128) != HG_OK || hipMemset(c->lost.p, 0, 128) != hipSuccess ||
        hipMemset(c->counters_dev.p, 0, c->counters_dev.bytes) != hipSuccess)
        return false;
    for (int li = 0; li < HG_TRACE_LANES; ++li) {
        hg_ctx::TraceLane& L = c->lanes[li];
        if (create_lane_stream(c, li, &L.stream) != hipSuccess ||
            hipEventCreateWithFlags(&L.traced, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.blended, hipEventDisableTiming) != hipSuccess)
            return false;
    }
    return true;
}

}  // namespace

extern "C" {

int hg_abi_version(void) { return HG_ABI_VERSION; }

int hg_create(int device, hg_ctx** out) {
    if (!out) return HG_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return HG_E_HIP;
    if (device < 0 || device >= n) return HG_E_INVALID;
    hg_ctx* c = new hg_ctx();
    c->device = device;
    if (!create_objects(c)) {  // (hg_destroy takes a half-built context: nothing made so far leaks)
        hg_destroy(c);
        return HG_E_HIP;
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
    for (DevBuf* b : {&c->spheres, &c->meshes, &c->cull, &c->materials, &c->nodes, &c->leaves, &c->tris, &c->normals, &c->cube,
                      &c->acc, &c->counters_dev, &c->spill, &c->lost, &c->query_in, &c->query_out, &c->guide0,
                      &c->guide1, &c->denoise_work[0], &c->denoise_work[1], &c->refit_in, &c->refit_raw, &c->lbvh.points,
                      &c->lbvh.partial, &c->lbvh.bounds, &c->lbvh.codes, &c->lbvh.index, &c->lbvh.codes_sorted,
                      &c->lbvh.index_sorted, &c->lbvh.sort_temp, &c->lbvh.tris, &c->lbvh.refs, &c->lbvh.topo,
                      &c->lbvh.live, &c->lbvh.new_index, &c->lbvh.scan_temp, &c->deform_positions, &c->deform_normals,
                      &c->deform_bones})
        release(*b);
    refit_reset(c);
    // The trace streams first, the server's stream after them: destroyed before them, the next hipStreamDestroy of a
    // plain trace stream hung in round 5 (DESIGN.md section 4.7 has what the analysis found)
    for (hg_ctx::TraceLane& L : c->lanes) {
        for (DevBuf* b : {&L.frame_color, &L.spill, &L.tile_cost, &L.tile_order, &L.order_scratch, &L.queue})
            release(*b);
        if (L.traced) (void)hipEventDestroy(L.traced);
        if (L.blended) (void)hipEventDestroy(L.blended);
        sv_trace("destroy: lane stream %p", static_cast<void*>(L.stream));
        if (L.stream) (void)hipStreamDestroy(L.stream);
    }
    sv_trace("destroy: trace streams destroyed");
    hg_ctx::Server& S = c->sv;
    if (S.stream) (void)hipStreamSynchronize(S.stream);
    sv_trace("destroy: server stream idle");
    for (DevBuf* b : {&S.ctl, &S.done, &S.ring, &S.spill}) release(*b);
    sv_trace("destroy: server buffers freed");
    for (hipEvent_t& e : S.blended)
        if (e) (void)hipEventDestroy(e);
    if (S.exited) (void)hipEventDestroy(S.exited);
    sv_trace("destroy: server events destroyed");
    if (S.host) (void)hipHostFree(S.host);
    sv_trace("destroy: server host word freed");
    if (S.stream) (void)hipStreamDestroy(S.stream);
    sv_trace("destroy: server stream destroyed");
    if (c->rb_stream) (void)hipStreamSynchronize(c->rb_stream);
    release(c->image);
    for (hg_ctx::DisplaySlot& d : c->slots) {
        release(d.image);
        if (d.untiled) (void)hipEventDestroy(d.untiled);
        if (d.host) (void)hipHostFree(d.host);
        if (d.copied) (void)hipEventDestroy(d.copied);
    }
    if (c->rb_stream) (void)hipStreamDestroy(c->rb_stream);
    for (auto* list : {&c->pending_trace, &c->pending, &c->free_events})
        for (auto& pr : *list) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
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

// The bookkeeping of an upload whose device copies are on the stream: the retained host copies the next upload compares
// against (made while the device copies run), the mesh table a partial re-upload starts from, counters and counts
int commit_scene(hg_ctx* c, const HgSceneIn& in, HgScenePack& pack, HgUploadDecision d, uint64_t geometry_generation) {
    const bool partial = d.kind == HG_UPLOAD_PARTIAL;
    for (int k = 0; k < (partial ? 3 : 5); ++k) copy_bytes(c->scene_copy[k], in.src(k), in.bytes(k));
    HG_HIP(c, hipStreamSynchronize(c->stream));  // host staging vectors die at return
    c->dev_meshes.swap(pack.dm);
    c->cull_table.q.swap(pack.cull.q);
    c->cull_table.n = pack.cull.n;
    c->scene_uploads++;
    if (partial) {
        c->scene_uploads_partial++;
        c->scene_uploads_vouched += d.vouched ? 1u : 0u;
    } else {
        c->stack_depth = pack.stack_depth;
        c->n_nodes = in.n_nodes;
        // what a mesh update reads of this layout (hg_mesh_trees.h); the caller's arrays describe the device again
        refit_reset(c);
        c->trees.reset(pack.rec, pack.leaf, in.n_tris);
        const size_t bytes[4] = {pack.rec.size() * sizeof(float4), pack.leaf.size() * sizeof(uint2),
                                 pack.t9.size() * sizeof(float), pack.nrm.size() * sizeof(float4)};
        std::memcpy(c->geometry_bytes, bytes, sizeof bytes);
        hg_root_pairs(in, c->root_pairs);
        c->geometry_stale = false;
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
    const bool stale = c->geometry_stale;  // refitted since the last full upload (hg_refit.hip)
    const HgUploadDecision d = hg_upload_decide_refit(c->has_scene, stale, c->scene_copy, c->geometry_gen,
                                                      c->dev_meshes.size(), c->trees.n_tris, c->n_nodes, in,
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
    if (partial && (stale ? hg_pack_mesh_table_kept(in, c->dev_meshes, c->root_pairs, pack, err)
                          : hg_pack_mesh_table(in, c->dev_meshes, pack, err)))
        return fail(c, err);
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
    if ((rc = upload(c, c->cull, pack.cull.q.data(), pack.cull.q.size() * sizeof(float4)))) return rc;
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
    const uint64_t need = hg_cube_mip_offsets(face_size, n_mips, c->cube_mip_offset);
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

int hg_synchronize(hg_ctx* c) {
    if (!c) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = quiesce(c)) return rc;
    if (int rc = drain_events(c)) return rc;
    return lost_check(c);
}

int32_t hg_local_tile_count(const hg_ctx* c) { return c ? c->n_local_tiles : 0; }

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
            if (c->rb.pending) return fail(c, HG_E_INVALID, "readbacks outstanding: end them before changing the depth");
            c->rb.set_depth(value);
            return HG_OK;
        case HG_OPT_READBACK_STREAM:
            if (c->rb.pending) return fail(c, HG_E_INVALID, "readbacks outstanding: end them before changing the stream");
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
