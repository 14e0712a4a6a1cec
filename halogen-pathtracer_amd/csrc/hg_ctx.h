// hg_ctx.h — the context object behind the C-ABI's opaque hg_ctx (private to libhalogen_hip.so; the functions over it
// that its translation units share are declared in hg_rt.h).  What of it is host logic with a header of its own, tested
// on the CPU: the tree bookkeeping of the mesh updates (hg_mesh_trees.h), the display slot ring (hg_slot_ring.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "halogen_abi.h"
#include "hg_mesh_trees.h"
#include "hg_slot_ring.h"

struct DevBuf {  // a device allocation owned by a context
    void* p = nullptr;
    size_t bytes = 0;
};

struct hg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // scene
    bool has_scene = false;
    DevBuf spheres, meshes, materials, nodes, leaves, tris, normals;
    int32_t n_spheres = 0, n_meshes = 0, n_materials = 0, n_nodes = 0;  // (the triangle count: trees.n_tris)
    uint32_t stack_depth = 2;
    // the caller's arrays of the last upload (spheres, meshes, materials, triangles, BVH entries), byte for byte: an
    // identical re-upload (the reference re-uploads on every camera move) is detected and skipped
    std::vector<uint8_t> scene_copy[5];
    std::vector<HgDevMesh> dev_meshes;  // the device mesh table of the last upload (partial re-uploads start from it)
    // the cull table of dev_meshes (hg_cull.h) as it lies in `cull`, uploaded wherever the mesh table is
    DevBuf cull;
    HgCullTable cull_table;
    uint64_t scene_uploads = 0, scene_uploads_skipped = 0, scene_uploads_partial = 0, scene_uploads_vouched = 0;
    uint64_t geometry_gen = 0;  // hg_upload_scene_gen: the caller's geometry generation of the last upload (0: none)
    // Mesh updates (hg_refit_mesh, hg_rebuild_mesh[_sah], hg_deform_mesh, hg_skin_mesh: one path, update_mesh of
    // hg_refit.hip).  `trees` is the host's picture of the device scene's topology, kept by every full upload and by
    // every rebuild, with every check an update makes against it (hg_mesh_trees.h); refit_lists holds, per tree under
    // trees' key, its plan's records on the device once a refit used them (a rebuild hands the list on to the new tree).
    // Beside them: the bytes of the four geometry arrays and the local boxes of each mesh root's two children (a refit
    // replaces its meshes').  geometry_stale: an update changed the device since the last full upload, so scene_copy[3]
    // and [4] no longer describe it (hg_upload_decide_refit).
    HgMeshTrees trees;
    std::map<uint64_t, DevBuf> refit_lists;
    size_t geometry_bytes[4] = {};  // nodes, leaves, triangles, normals as uploaded (the buffers hold at least 16 B)
    std::vector<HgRootPair> root_pairs;
    bool geometry_stale = false;
    // the triangles of an update on the device where the caller's are not (staged from the host, or packed from
    // vertices); one raw box (6 floats) per record of a tree
    DevBuf refit_in, refit_raw;
    uint64_t scene_refits = 0;
    // The rebuilds' device scratch (hg_lbvh.hip), grown on demand
    struct Lbvh {
        DevBuf points, partial, bounds;       // key points (3 floats each); per-workgroup and final pmin / pmax
        DevBuf codes, index, codes_sorted, index_sorted, sort_temp;
        DevBuf tris, refs;                    // the triangles in the new order; the compact (refA, refB) per record
        // hg_rebuild_mesh_sah: the L = 1 tree (an HgLbvhNode per internal node), its live flags, their exclusive scan
        DevBuf topo, live, new_index, scan_temp;
    } lbvh;
    uint64_t scene_rebuilds = 0;
    // Deform from vertices (hg_set_mesh_vertices, hg_deform_mesh, hg_skin_mesh; hg_deform.hip).  Per bound tree, by its
    // triangle offset like trees.slots, until the next full upload: the mesh's index list on the device in the tree's
    // current triangle order (every rebuild of the tree permutes it into `spare` and swaps the two), and, once
    // hg_set_mesh_skin gave them, the rest pose, the influences and the vertices the last hg_skin_mesh* produced.
    struct VertexBinding {
        DevBuf indices, spare;  // n_tris int3 each
        int32_t n_tris = 0, n_vertices = 0;
        DevBuf rest_positions, rest_normals, bone_indices, weights;  // 3 floats, 3 floats, 4 uint16, 4 floats per vertex
        DevBuf positions, normals;                                   // the skinned vertices
        int32_t n_bones = 0;  // 0: no skin
        bool skinned = false;  // positions / normals hold a pose
        // hg_set_mesh_vertices_opt(HG_BIND_ADJACENCY), for HG_DEFORM_NORMALS (csrc/hg_normals.h): the list as it was
        // bound, which no rebuild permutes; the inverted index over it (n_vertices + 1 offsets, 3 * n_tris face ids);
        // the face pass's output (3 floats a triangle) and the vertex pass's for the deform forms (3 floats a vertex;
        // the skin forms' goes to `normals`)
        bool adjacency = false;
        DevBuf frozen, adj_offsets, adj_faces, face_normals, vertex_normals;
    };
    std::map<uint32_t, VertexBinding> vertex_bindings;
    DevBuf deform_positions, deform_normals, deform_bones;  // the host-pointer forms' vertices and palette

    // cubemap
    DevBuf cube;
    int32_t cube_size = 0, cube_mips = 0;
    uint32_t cube_mip_offset[HG_MAX_CUBE_MIPS] = {};

    // params
    bool has_params = false;
    hg_params params{};

    // target
    int32_t W = 0, H = 0, rank = 0, n_ranks = 1, tiles_x = 0, tiles_y = 0, n_local_tiles = 0;
    DevBuf acc;

    DevBuf spill;  // traversal stack entries beyond the LDS part, per thread, of launches on the context stream
    // Ray queries (hg_trace_rays, hg_camera_rays): device staging of one launch's input records (rays / pixels) and
    // output records (hits / rays) of the host-pointer forms; grown on demand, reused, freed by hg_destroy
    DevBuf query_in, query_out;
    // Trace pipeline (hg_render): the regenerating / streaming kernels trace each launch chunk on one of HG_TRACE_LANES
    // side streams, in turn, into that stream's own frame-colour buffer; the chunk's in-order blend into the accumulator
    // runs on `stream`.  So a chunk's tail overlaps the next chunk's trace, and everything else on `stream` (readback,
    // clear, gather) stays ordered after the blends.  Per trace stream: its buffers and the events that order them.
    struct TraceLane {
        hipStream_t stream = nullptr;
        hipEvent_t traced = nullptr;   // after this stream's last trace (the blend on `stream` waits for it)
        hipEvent_t blended = nullptr;  // after the blend of this stream's last chunk (its buffers are free again)
        bool blend_pending = false;    // `blended` was recorded and the next trace here must wait for it
        DevBuf frame_color;            // this chunk's per-frame colours ([slot][frame], fc_index)
        DevBuf spill;                  // traversal stack entries beyond the LDS part, one column per thread
        // Cost order: this stream's traces add their wave times to tile_cost and its sorts read and clear them, all in
        // this stream's order.  (One buffer shared by both streams let a sort read costs that the other stream's trace
        // was still adding to: the counting sort's two passes then disagreed and wrote out of range.)
        DevBuf tile_cost;              // per local tile, wave-clock cost since this stream's last sort
        DevBuf tile_order;             // the cost order this stream's launches read
        DevBuf order_scratch;          // hg_order.hip: histogram and claims (zeroed at allocation, left zeroed)
        DevBuf queue;                  // kQueue launches: the 8 unit heads + exit count (zeroed at allocation; the
                                       // last wave of each launch zeroes them again)
        bool tile_cost_valid = false;  // tile_cost holds costs for this tiling
        bool tile_order_valid = false;
        int64_t frames_since_order = 0;  // frames traced on this stream since its last sort
    };
    static_assert(HG_TRACE_LANES_BIG >= 1 && HG_TRACE_LANES_BIG <= HG_TRACE_LANES, "HG_TRACE_LANES_BIG out of range");
    TraceLane lanes[HG_TRACE_LANES];
    int next_lane = 0;     // chunks of at most HG_QUEUE_MAX_FRAMES frames: every lane in turn
    int next_lane_big = 0;  // longer chunks: lanes [0, HG_TRACE_LANES_BIG) in turn

    // The render server (hg_mega.hip kServer and hg_server.h): launches of the reference's one frame per call
    // (at most HG_QUEUE_MAX_FRAMES frames, accumulating, streaming kernel) post their frames to persistent trace waves
    // that outlive the call, instead of launching; each frame's blend runs on `stream` behind a gate on its completion
    // count.  Stopped (the waves drain what was posted and leave) by every entry point that changes what the waves
    // read, by another kind of launch, and when its parameters or FrameCount chain do not continue.
    struct Server {
        hipStream_t stream = nullptr;  // CU-masked: a hardware queue of its own (never ahead of `stream`'s gates)
        bool running = false;
        DevBuf ctl;         // heads, mirror, ticket (HG_SV_CTL_BYTES), zeroed before each launch
        DevBuf done;        // per ring slot a completion count on its own 128-B line, zeroed before each launch
        DevBuf ring;        // colour ring: ring_n frames of n_local_tiles * 64 float4
        DevBuf spill;
        unsigned long long* host = nullptr;  // pinned, coherent: the host words HG_SV_HOST_* (hg_layout.h)
        uint32_t ring_n = 0, posted = 0, cap = 0;
        uint32_t committed = 0;  // frames the host asked for (gate + blend queued); posted - committed were posted ahead
        uint32_t uses[HG_SV_RING] = {};     // frames posted to each ring slot in this lifetime
        hipEvent_t blended[HG_SV_RING] = {};  // after the blend of each ring slot's last frame
        // HALOGEN_SERVER_SERIAL=1 (a profiling aid, tools/pmc_server.sh): the gates wait for the lifetime's end (this
        // event, after the server kernel), so a profiler that runs one kernel at a time (rocprofv3 --pmc) never runs a
        // gate before the server it waits for
        hipEvent_t exited = nullptr;
        bool blend_valid[HG_SV_RING] = {};
        hg_params params{};   // the parameters it was started with (frameCount: its first frame)
        int32_t kernel_variant = 0, descent_t = 0;
        HgKernelParams kp{};  // the launch's parameters (the blends read acc / ring / first_frame)
        int32_t idle_us = HG_SV_IDLE_US;  // HG_OPT_SERVER_IDLE_US
        int64_t gate_us = -1;             // HG_OPT_SERVER_GATE_US (< 0: the default, 30 s)
#if HG_SV_DIAG_TIMES
        double post_s[256] = {};  // (analysis builds) host clock of each post
#endif
    } sv;
    int32_t server_on = 1;  // HG_OPT_SERVER
    uint64_t server_launches = 0, server_frames = 0;
    uint64_t server_refused = 0;  // posts that met a closing server (the close handshake), re-posted to a new one
    // HG_OPT_SERVER_AHEAD: frames the server traces ahead of the host's calls (counters off), and the call chain that
    // engages the server without a host running ahead: consecutive accumulating calls with the same parameters, each
    // continuing the last one's FrameCount
    int32_t sv_ahead = HG_SV_AHEAD;
    uint64_t server_ahead_posts = 0;
    hg_params chain_params{};
    int32_t chain_next = 0, chain_len = 0;
    // Lost frames (a server frame's gate gave up, hg_server_gate): the gate raises `lost` (uncached device memory), and
    // every later blend into the accumulator is skipped; the host marks the accumulator invalid (acc_lost) when it reads
    // the gate's host word and the frame belongs to the current accumulation (acc_epoch: advanced by every clear,
    // checkpoint load and reallocation, which also reset both).  While acc_lost, hg_render and every readback / copy /
    // gather of the accumulator return HG_E_FRAME_LOST.
    DevBuf lost;
    uint32_t acc_epoch = 0;
    bool acc_lost = false;
    uint64_t frames_lost = 0;
    // The server serves only a host that runs ahead: each render call records call_done[calls & 1] on `stream` after
    // its frames' blends, so at a call the event of the call before last tells whether the GPU still works on it
    hipEvent_t call_done[2] = {};
    bool call_done_valid[2] = {};
    uint64_t calls = 0;

    // counters / timing
    DevBuf counters_dev;
    hg_counters counters{};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending, free_events, pending_trace;

    // device / options
    int n_cu = 0;
    int32_t kernel = HG_KERNEL_AUTO, block = 128, counters_on = 1, timing = 0;
    int32_t frame_split = 0;  // 0: automatic (see hg_render)
    int32_t wave_units = 0;   // HG_OPT_WAVE_UNITS, 0: automatic (see hg_render)
    int32_t lane_pick = HG_LANE_PICK;  // HG_OPT_LANE_PICK: 1-frame chunks on the first idle trace stream (1) or in turn (0)
    int32_t descent_t = -1;   // < 0: automatic from the BLAS depth
    int32_t tile_order_on = HG_TILE_ORDER;  // HG_OPT_TILE_ORDER
    int32_t queue_fill = HG_QUEUE_FILL;     // HG_OPT_QUEUE_FILL
    // Render coalescing (HG_OPT_COALESCE): hg_render is asynchronous, so consecutive calls with the same parameters are
    // held and launched as one multi-frame launch once `coalesce` frames are pending, or as soon as anything reads or
    // changes the context's state (every other entry point flushes first: hg_ctx_flush).  Same frames, same order,
    // same image; 1 = every call launches at once.
    int32_t coalesce = HG_COALESCE;
    int32_t pending_frames = 0, pending_acc = 0;

    // Display readback (hg_display.hip: hg_readback, hg_readback_begin[_format] / _end[_data]): the accumulator untiled on
    // the device into a row-major image in the display format, which ends up in the next of rb.depth slots (a ring)
    struct DisplaySlot {
        void* host = nullptr;  // the pinned host image the caller reads
        size_t cap = 0;        // its allocated bytes
        size_t bytes = 0;      // bytes of the readback it holds
        int32_t format = 0;
        bool mapped = false;   // allocated mapped + fine-grained (HG_OPT_READBACK_STREAM 2 untiles straight into it)
        hipEvent_t copied = nullptr;   // after the readback's last write to `host`
        DevBuf image;                  // HG_OPT_READBACK_STREAM 1: the slot's own device image, copied on rb_stream
        hipEvent_t untiled = nullptr;  // ... after the untile into it (the copy on rb_stream waits for it)
    };
    DevBuf image;  // HG_OPT_READBACK_STREAM 0 and hg_readback: the one device image, copied on `stream`
    DisplaySlot slots[HG_READBACK_MAX];
    HgSlotRing rb;                    // HG_OPT_READBACK_DEPTH; the slot the next begin fills, begun readbacks not yet ended
    int rb_side = HG_READBACK_SIDE;   // HG_OPT_READBACK_STREAM
    hipStream_t rb_stream = nullptr;  // created at the first begin that copies on it

    // Denoised display (hg_update_guides, hg_readback_begin_denoised; kernels in hg_denoise.hip): the guide images
    // (row-major W x H float4: normal + t, albedo + kind) and the filter's two colour images, all allocated by
    // hg_update_guides (the context is idle there), so a denoised begin allocates nothing beside a running server.
    // guides_valid: they belong to this target size and this device scene (hg_resize and a rebuilding upload clear it)
    DevBuf guide0, guide1, denoise_work[2];
    bool guides_valid = false;
};
