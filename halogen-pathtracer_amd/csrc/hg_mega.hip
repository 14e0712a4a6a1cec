// hg_mega.hip — the megakernels of the hot path: the streaming kernel (default for deep BLAS), the regenerating
// kernel (default otherwise) and the lockstep kernel (HG_KERNEL_MEGA: debug views, large-maxBounces fallback).
//
// Reference: Assets/Scripts/Halogen Shaders/HalgoenCompute.compute, kernel HalogenCompute (:1015-1063) with
// the accumulation blit (AccumulationShader.shader:27-34) fused as its epilogue.  One wave64 = one 8x8 pixel
// tile; the BLAS stack lives in LDS ([depth][lane]).  The lockstep kernel below is the simplest faithful form:
// each lane runs all n_frames frames of its pixel back to back.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hg_device.h"
#include "hg_launch.h"
#include "hg_sched.h"
#include "hg_server.h"

using namespace hgd;

// The counting instantiations' epilogue: the wave's sums go to hg_counters.  kPhases: the wave-clock phase split and the
// shading rounds of the regenerating and streaming kernels (the lockstep kernel has neither).
template <bool kPhases>
__device__ __forceinline__ void flush_counters(const HgKernelParams& kp, uint32_t lane, uint32_t paths, const Counters& c,
                                               uint64_t cyc_trav = 0, uint64_t cyc_shade = 0) {
    // every ray transforms into every mesh and prefilters every sphere: those counts follow from c.rays
    const uint32_t v[9] = {paths, c.rays, c.tri, c.aabb, c.rays * uint32_t(kp.n_meshes),
                           c.rays * uint32_t(kp.n_spheres), c.hits, c.node_rounds, c.tri_rounds};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const uint32_t s = wave_sum(v[k]);
        if (lane == 0 && s) atomicAdd(kp.counters + k, (unsigned long long)s);
    }
    if (kPhases) {
        if (lane == 0) {
            atomicAdd(kp.counters + 9, (unsigned long long)cyc_trav);
            atomicAdd(kp.counters + 10, (unsigned long long)cyc_shade);
        }
        const uint32_t sr = wave_sum(c.shade_rounds);
        if (lane == 0 && sr) atomicAdd(kp.counters + 15, (unsigned long long)sr);
    }
    const uint32_t pm = wave_sum(c.primary_miss);
    if (lane == 0 && pm) atomicAdd(kp.counters + 16, (unsigned long long)pm);
}

// kDebug: the debug views (HalogenDebugMode 1-5) get their own instantiation so the production kernel's register
// allocation does not pay for trace_ray_debug.
template <bool kCounters, bool kDebug>
__global__ __launch_bounds__(256, HG_LOCK_WAVES) void hg_trace_kernel(const HgKernelParams kp) {
    const uint32_t lane = threadIdx.x & 63u;
    const int local_tile = int(blockIdx.x) * int(blockDim.x >> 6) + int(threadIdx.x >> 6);
    HgTileRect rect;
    tile_rect(kp, local_tile, rect);
    const uint32_t px = rect.x0 + (lane & 7u), py = rect.y0 + (lane >> 3);
    const bool active = local_tile < kp.n_local_tiles && px < kp.Wu && py < kp.Hu;
    Counters c{0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t paths = 0;
    if (active) {
        const MegaStack stk{threadIdx.x, blockDim.x, kp.spill + blockIdx.x * blockDim.x + threadIdx.x,
                            kp.spill_stride};
        const size_t slot = size_t(local_tile) * 64 + lane;
        // HalogenCompute :1023-1033
        const float ndcx = (float(px) / kp.W) * 2.0f - 1.0f;
        const float ndcy = (float(py) / kp.H) * 2.0f - 1.0f;
        const uint32_t pixel_id = pcg_hash(px + py * kp.Wu);
        for (int f = 0; f < kp.n_frames; ++f) {
            const int32_t fc = kp.accumulate ? kp.first_frame + f : 1;
            Sampler smp{uint32_t(fc), pixel_id, 0u};
            MediumStack ms{0ull, 0};
            f3 color = mk(0, 0, 0);
            for (uint32_t s = 0; s < kp.spp; ++s) {
                const Ray r = camera_ray(kp, smp, ndcx, ndcy);
                paths++;
                if (!kDebug) color = color + trace_ray(kp, smp, ms, r, c, stk);
                else color = color + trace_ray_debug(kp, smp, ms, r, c, stk);
            }
            const float sppf = float(kp.spp);
            color = mk(color.x / sppf, color.y / sppf, color.z / sppf);
            // read-modify-write per frame: 32 B, keeps 4 VGPRs free while tracing
            kp.acc[slot] = kp.accumulate ? blend_frame(kp.acc[slot], color, float(fc)) : frame_alone(color);
        }
    }
    if (kCounters) flush_counters<false>(kp, lane, paths, c);
}

size_t hg_mega_lds_bytes(uint32_t stack_depth, int block) {
    return size_t(stack_depth < HG_MEGA_LDS_STACK ? stack_depth : HG_MEGA_LDS_STACK) * size_t(block) *
           sizeof(uint32_t);
}

// Regenerating variant (HG_KERNEL_MEGA_REGEN): each loop iteration runs ONE bounce (get_ray_intersection + one
// body of trace_ray's loop, :887-945) for every lane; a lane whose path ended starts its next sample / frame right
// away (blending a finished frame into the accumulator), so lanes never idle until the longest path of their wave
// ends — at the price of desynchronised bounce depths (less coherent node fetches).  Path state is packed to keep
// the traversal's register budget: bounceTypes[3] + the bounce index in one word (host guarantees maxBounces <=
// HG_REGEN_MAX_BOUNCES), frame + sample index in another (n_frames, spp < 2^16, host-chunked), the pixel's ndc /
// accumulator slot recomputed at each regeneration.
// Per-lane path state parked in LDS (RowVec3 / RowVec4 rows, hg_dev_stack.h): the throughput, radiance and sample sum
// are touched once per bounce, so they stay out of the registers the traversal needs.
constexpr uint32_t kRegenLdsState = 9;  // words per lane: throughput, radiance, sample sum
// Streaming kernel: one more word per lane (row 9, unused since the round-2 LDS accumulator was retired: the leaf-share
// rows stay 64-bit aligned at row 10).
constexpr uint32_t kStreamLdsState = 10;
// Streaming kernel LDS rows (one wave per workgroup, RowVec / RowStack): throughput 0-2, path colour 3-5, sample sum
// 6-8, the distributed leaf test 10-12, the traversal stack from row 13.
constexpr uint32_t kRowThr = 0, kRowCol = 3, kRowSum = HG_ROW_SUM, kRowLeaf = kStreamLdsState;
constexpr uint32_t kRowStack = kRowLeaf + kLeafShareWords;
constexpr uint32_t kRegenRowStack = kRegenLdsState;  // regenerating kernel: rows 0-8 as above, the stack from row 9

// RayColor / SamplesPerPixel (:1060); x / 1 == x exactly (NaN and signed zeros included), so spp 1 skips the divisions
__device__ __forceinline__ f3 sample_mean(const HgKernelParams& kp, f3 sum) {
    if (kp.spp == 1) return sum;
    const float sppf = float(kp.spp);
    return mk(sum.x / sppf, sum.y / sppf, sum.z / sppf);
}

// The wave's copy of the material table (mat_f4, hg_dev_records.h), made once the lanes' rows are initialised: at spp 1 the
// table may lie in the sample-sum rows (hg_layout.h hg_wave_lds_plan), which no lane writes or reads after that
// initialisation (sample_mean above and the one_sample branches of the shading loops: the sum of one sample is the
// sample).  The render server's waves copy once per lifetime: every upload, a partial one included, stops the server
// before it replaces a buffer (hg_upload_scene_gen's quiesce, hg_runtime.hip), as the mesh copy already relies on.
template <bool kMatLds>
__device__ __forceinline__ void mat_lds_begin(const HgKernelParams& kp, uint32_t lane) {
    if constexpr (kMatLds) {
        wave_lds_sync();
        mat_lds_fill(kp, lane);
        wave_lds_sync();
    }
}

template <bool kCounters, bool kMeshLds, bool kMatLds>
__global__ __launch_bounds__(HG_STREAM_LB, HG_MEGA_WAVES) void hg_trace_regen_kernel(const HgKernelParams kp) {
    const uint32_t lane = threadIdx.x & 63u;
    if (kMeshLds) {  // the wave's copy of the mesh records (mesh_f4, hg_dev_records.h)
        mesh_lds_fill(kp, lane);
        wave_lds_sync();
    }
    // wave -> (tile, frame chunk): with frame_split == 1 the wave index is the tile
    // one wave per workgroup (launched with 64 threads): wave = workgroup; LDS rows as the streaming kernel's
    const uint32_t gw = blockIdx.x;
    const uint32_t nlt = uint32_t(kp.n_local_tiles), split = uint32_t(kp.frame_split);
    int local_tile;
    uint32_t chunk;
    wave_unit(kp, gw, nlt, split, local_tile, chunk);
    tile_cost_begin(kp, lane, local_tile, chunk < split);
    const uint32_t f_begin = hg_chunk_begin(chunk, uint32_t(kp.n_frames), split);
    const uint32_t f_end = hg_chunk_begin(chunk + 1u, uint32_t(kp.n_frames), split);
    const RowStack<HG_MEGA_LDS_STACK, kRegenRowStack> stk{lane, kp.spill + blockIdx.x * 64u + lane, kp.spill_stride};
    const RowVec3<kRowThr> s_thr{lane};
    const RowVec3<kRowCol> s_col{lane};
    const RowVec3<kRowSum> s_sum{lane};
    bool work;
    uint32_t px, py;
    {
        HgTileRect rect;
        tile_rect(kp, local_tile, rect);
        px = rect.x0 + (lane & 7u);
        py = rect.y0 + (lane >> 3);
        work = chunk < split && px < kp.Wu && py < kp.Hu && f_end > f_begin;
    }
    Counters c{0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t paths = 0;
    uint32_t fs = f_begin << 16;  // frame index << 16 | sample index
    uint32_t bounce = 0;          // diffuse | glossy << 8 | transmission << 16 | bounce index << 24
    Sampler smp{kp.accumulate ? uint32_t(kp.first_frame) + f_begin : 1u, pcg_hash(px + py * kp.Wu), 0u};
    MediumStack ms{0ull, 0};
    Ray ray{mk(0, 0, 0), mk(0, 0, 1)};
    float acc_rough = 0.0f;
#if HG_REGEN_ITEMS
    const TileItems items(kp, local_tile, chunk < split, f_begin, f_end, lane);
    uint32_t pix = lane;  // the item's pixel within the tile (x + 8 y)
    if (lane < items.n_items) {  // item `lane`
        uint32_t f;
        items.get(lane, pix, f);
        px = items.tx0 + (pix & 7u);
        py = items.ty0 + (pix >> 3);
        fs = f << 16;
        smp = Sampler{kp.accumulate ? uint32_t(kp.first_frame) + f : 1u, pcg_hash(px + py * kp.Wu), 0u};
    }
    work = lane < items.n_items;
#else
    const uint32_t pix = lane;
#endif
    if (work) {
        ray = camera_ray(kp, smp, (float(px) / kp.W) * 2.0f - 1.0f, (float(py) / kp.H) * 2.0f - 1.0f);  // :1023-1033
        paths++;
        s_thr.set(mk(1, 1, 1));
        s_col.set(mk(0, 0, 0));
        s_sum.set(mk(0, 0, 0));
    }
    mat_lds_begin<kMatLds>(kp, lane);
    uint64_t cyc_trav = 0, cyc_shade = 0;  // wave clock (s_memtime) per phase, counting instantiation only
    while (__any(work)) {
        const uint64_t t0 = kCounters ? wave_clock() : 0;
        const bool was_work = work;
        uint64_t t1 = 0;
        if (work) {
            __builtin_amdgcn_s_setprio(HG_TRAVERSE_PRIO);
            const Hit hit = intersect<kMeshLds>(kp, ray, c, stk);
            __builtin_amdgcn_s_setprio(0);
            if (kCounters) t1 = wave_clock();
            c.shade_rounds += wave_once();
            bool alive = false;
            f3 thr = s_thr.get(), col = s_col.get();
            if (hit.t < kp.far_) {  // :898-936
                c.hits++;
                const Mat mt = load_mat<kMatLds>(kp, hit.mat);
                col = col + xyz(mt.emis_rough) * thr;
                uint32_t bt = 0;
                const f3 att = evaluate_hit<kMatLds>(kp, smp, ms, ray, hit, mt, bt);
                bounce += 1u << (8u * bt);
                thr = thr * att;
                acc_rough += mt.emis_rough.w * thr.x;
                const float rr = smp.get1(ID_RR);
                smp.offset += BOUNCE_INC;
                const float contribution = hg_fmaxf(hg_fmaxf(thr.x, thr.y), thr.z);
                if (!(rr > contribution)) {
                    thr = thr * rcp_exact(contribution);
                    bounce += 1u << 24;
                    alive = (bounce >> 24) <= kp.max_bounces && !((bounce & 0xFFu) > kp.max_diff ||
                                                                 ((bounce >> 8) & 0xFFu) > kp.max_glossy ||
                                                                 ((bounce >> 16) & 0xFFu) > kp.max_trans);
                }
            } else {  // :941
                c.primary_miss += bounce == 0u;  // the path's camera ray (no bounce recorded yet)
                col = col + sample_sky(kp, ray.d, sky_level(kp, acc_rough)) * thr;
            }
            if (!alive) {
                // RayColor += trace_ray(...); spp 1: 0 + col == col (col starts at +0 and only has terms added: never -0)
                const bool one_sample = kp.spp == 1;
                f3 sum = one_sample ? col : s_sum.get() + col;
                ++fs;
                bool next = (fs & 0xFFFFu) < kp.spp;  // next sample: statics persist (:188-189)
                if (!next) {
                    const f3 color = sample_mean(kp, sum);
                    const size_t slot_i = size_t(uint32_t(local_tile)) * 64u + pix;
                    // this frame's colour, blended later in frame order: every launch of the trace pipeline (the runtime
                    // passes a colour buffer exactly then, and blends after every chunk of it, a 1-frame chunk included)
                    if (HG_REGEN_ITEMS || kp.frame_color != nullptr) {
                        fc_store(kp.frame_color + fc_index(kp, fs >> 16, slot_i),
                                 make_float4(color.x, color.y, color.z, 1.0f));
                    } else {
                        float4* slot = kp.acc + slot_i;
                        *slot = kp.accumulate ? blend_frame(*slot, color, float(smp.frame)) : frame_alone(color);
                    }
                    fs = (fs & 0xFFFF0000u) + 0x10000u;
#if HG_REGEN_ITEMS
                    const uint32_t k = wave_take();
                    if (k < items.n_items) {  // the next (pixel, frame) item: statics reset as for a dispatch
                        uint32_t f;
                        items.get(k, pix, f);
                        next = true;
                        sum = mk(0, 0, 0);
                        fs = f << 16;
                        smp = Sampler{kp.accumulate ? uint32_t(kp.first_frame) + f : 1u,
                                      pcg_hash(items.tx0 + (pix & 7u) + (items.ty0 + (pix >> 3)) * kp.Wu), 0u};
                        ms = MediumStack{0ull, 0};
                    }
#else
                    if ((fs >> 16) < f_end) {  // next frame = next dispatch: statics reset
                        next = true;
                        sum = mk(0, 0, 0);
                        smp.frame = kp.accumulate ? uint32_t(kp.first_frame) + (fs >> 16) : 1u;
                        smp.offset = 0;
                        ms = MediumStack{0ull, 0};
                    }
#endif
                }
                if (!one_sample) s_sum.set(sum);
                if (next) {
#if HG_REGEN_ITEMS
                    const uint32_t qx = items.tx0 + (pix & 7u), qy = items.ty0 + (pix >> 3);
#else
                    HgTileRect rect;
                    tile_rect(kp, local_tile, rect);
                    const uint32_t qx = rect.x0 + (pix & 7u), qy = rect.y0 + (pix >> 3);
#endif
                    ray = camera_ray(kp, smp, (float(qx) / kp.W) * 2.0f - 1.0f, (float(qy) / kp.H) * 2.0f - 1.0f);
                    thr = mk(1, 1, 1);
                    col = mk(0, 0, 0);
                    acc_rough = 0.0f;
                    bounce = 0;
                    paths++;
                } else {
                    work = false;
                }
            }
            s_thr.set(thr);
            s_col.set(col);
        }
        if (kCounters) {  // t1 was read inside the divergent branch: take it from a lane that ran it
            const uint64_t t2 = wave_clock();
            const int src = __ffsll((unsigned long long)__ballot(was_work)) - 1;
            const uint64_t t1u = (uint64_t(__shfl(uint32_t(t1 >> 32), src)) << 32) | __shfl(uint32_t(t1), src);
            cyc_trav += t1u - t0;
            cyc_shade += t2 - t1u;
        }
    }
    record_tile_cost(lane);
    if (kCounters) flush_counters<true>(kp, lane, paths, c, cyc_trav, cyc_shade);
}

// Runtime flags -> template arguments: with_flags(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{},
// ...), so a launcher names its kernel once and exactly the combinations it can be called with are instantiated.
template <class F>
static void with_flags(F&& f) {
    f();
}
template <class F, class... Rest>
static void with_flags(F&& f, bool b, Rest... rest) {
    if (b) with_flags([&](auto... k) { f(std::true_type{}, k...); }, rest...);
    else with_flags([&](auto... k) { f(std::false_type{}, k...); }, rest...);
}

hipError_t hg_launch_mega_regen(const HgKernelParams& kp_in, int block, bool counters, hipStream_t stream) {
    (void)block;  // one wave per workgroup (the kernel's LDS rows assume it)
    block = 64;
    const int64_t grid = int64_t(kp_in.n_local_tiles) * kp_in.frame_split;
    if (grid == 0) return hipSuccess;
    const uint32_t lds_depth = kp_in.stack_depth < HG_MEGA_LDS_STACK ? kp_in.stack_depth : HG_MEGA_LDS_STACK;
    const size_t lds = size_t(kRegenRowStack + lds_depth) * 64u * sizeof(uint32_t);
    HgKernelParams kp = kp_in;
    // which of the mesh records and the material table the waves keep in LDS, and where (hg_layout.h)
    const HgWaveLdsPlan lp = hg_wave_lds_plan(lds, kp.n_meshes, HG_MAT_LDS_REGEN ? kp.n_materials : 0, kp.spp, HG_REGEN_LDS_BUDGET);
    kp.mesh_lds_word = lp.mesh_word;
    kp.mat_lds_word = lp.mat_word;
    const dim3 g{uint32_t(grid)}, b{uint32_t(block)};
    with_flags(
        [&](auto C, auto M, auto T) {
            hipLaunchKernelGGL((hg_trace_regen_kernel<decltype(C)::value, decltype(M)::value, decltype(T)::value>), g, b,
                               lp.bytes, stream, kp);
        },
        counters, lp.mesh_lds, lp.mat_lds);
    return hipGetLastError();
}


// Streaming variant (HG_KERNEL_MEGA_STREAM): the regenerating kernel with a resumable traversal.  Lanes advance
// their traversal one while-while round at a time; once at most HG_STREAM_TMIN lanes are still traversing (and
// some have finished), the finished lanes shade their hit and start their next ray while the stragglers keep
// their traversal state, so the wave's lanes stay busy instead of waiting for the slowest ray of every bounce.
// Every frame's colour goes to frame_color (item scheduling), blended in frame order by hg_blend_frames.  kQueue: the
// persistent work-queue form above (launches of few frames).
// kServer (with kQueue): the render server's persistent form above.
template <bool kCounters, bool kMeshLds, bool kMatLds, bool kQueue, bool kDeep, bool kServer>
__global__ __launch_bounds__(HG_STREAM_LB, HG_STREAM_WAVES) void hg_trace_stream_kernel(const HgKernelParams kp) {
    static_assert(!kServer || kQueue, "the render server is a queue launch");
    // shade once at most kTmin lanes still traverse; reshade while at least kReshade need it (compile-time: as kernel
    // parameters they cost 8 B of scratch)
    constexpr uint32_t kTmin = kDeep ? HG_STREAM_TMIN_DEEP : HG_STREAM_TMIN;
    constexpr uint32_t kReshade = kDeep ? HG_STREAM_RESHADE_DEEP : HG_STREAM_RESHADE;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nlt = uint32_t(kp.n_local_tiles), split = uint32_t(kp.frame_split);
    const uint32_t n_units = nlt * split;  // kQueue: (tile, frame chunk) units of the queue
    int local_tile = 0;
    uint32_t chunk = 0, f_begin = 0, f_end = 0, u_first = 0;
    if constexpr (kQueue) {
        if (lane == 0) {
            lds_put(hg_next_item, 0u);
            for (uint32_t u = 0; u < 2u; ++u) {
                lds_put(hg_qu[u].base, 0u);
                lds_put(hg_qu[u].end, 0u);
            }
            lds_put(hg_q_cur, 0u);
            lds_put(hg_q_dry, 0u);
            lds_put(hg_q_need, 1u);  // (both units empty: the first loop top pulls two)
            hg_wave_cost[threadIdx.x >> 6] = nullptr;
            if constexpr (kServer) sv_init(kp);
        }
    } else {
        // wave -> (tile, frame chunk), as in hg_trace_regen_kernel
        // one wave per workgroup (launched with 64 threads): wave = workgroup
        const uint32_t gw = blockIdx.x;
        u_first = gw * (kp.wave_units > 1u ? kp.wave_units : 1u);  // (more than one unit only without a frame split)
        wave_unit(kp, u_first, nlt, split, local_tile, chunk);
        tile_cost_begin(kp, lane, local_tile, chunk < split);
        f_begin = hg_chunk_begin(chunk, uint32_t(kp.n_frames), split);
        f_end = hg_chunk_begin(chunk + 1u, uint32_t(kp.n_frames), split);
    }
    const RowStack<HG_STREAM_LDS_STACK, kRowStack> stk{lane, kp.spill + blockIdx.x * 64u + lane, kp.spill_stride};
    const RowVec3<kRowThr> s_thr{lane};
    const RowVec3<kRowCol> s_col{lane};
    const RowVec3<kRowSum> s_sum{lane};
    const LeafShare ls{kRowLeaf * 64u};
    const uint32_t nm = uint32_t(kp.n_meshes);
    if (kMeshLds) {  // the wave's copy of the mesh records (mesh_f4, hg_dev_records.h)
        mesh_lds_fill(kp, lane);
        wave_lds_sync();
    }
    bool work = false;
    uint32_t px = 0u, py = 0u;
    Counters c{0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t paths = 0;
    uint32_t fs = f_begin << 16;  // frame index << 16 | sample index
    uint32_t bounce = 0;          // diffuse | glossy << 8 | transmission << 16 | bounce index << 24
    Sampler smp{kp.accumulate ? uint32_t(kp.first_frame) + f_begin : 1u, pcg_hash(px + py * kp.Wu), 0u};
    MediumStack ms{0ull, 0};
    Ray ray{mk(0, 0, 0), mk(0, 0, 1)};
    float acc_rough = 0.0f;
    Trav tv;
    tv.mi = nm;
    uint32_t slot = 0;  // the lane's item: kQueue its accumulator slot (local tile * 64 + pixel), else v (UnitItems)
    bool dry = false;   // kQueue, wave-uniform: the queue has no unit left
    const UnitItems items = kQueue ? UnitItems() : UnitItems(kp, u_first, local_tile, chunk < split, f_begin, f_end, lane);
    if constexpr (kQueue) {
        wave_lds_sync();  // hg_q / hg_next_item initialised (lane 0); every lane takes its first item in the loop
    } else {
        if (lane < items.n_items) {  // item `lane`
            uint32_t f;
            items.get(kp, lane, slot, f);
            items.pixel(slot, px, py);
            fs = f << 16;
            smp = Sampler{kp.accumulate ? uint32_t(kp.first_frame) + f : 1u, pcg_hash(px + py * kp.Wu), 0u};
        }
        work = lane < items.n_items;
        if (work) {
            ray = camera_ray(kp, smp, (float(px) / kp.W) * 2.0f - 1.0f, (float(py) / kp.H) * 2.0f - 1.0f);  // :1023-1033
            paths++;
            s_thr.set(mk(1, 1, 1));
            s_col.set(mk(0, 0, 0));
            s_sum.set(mk(0, 0, 0));
            trav_begin<kMeshLds>(kp, ray, tv, c);
        }
    }
    mat_lds_begin<kMatLds>(kp, lane);
    uint64_t cyc_trav = 0, cyc_shade = 0;  // wave clock (s_memtime) per phase, counting instantiation only
    __builtin_amdgcn_s_setprio(HG_TRAVERSE_PRIO);  // traversal waits on memory: its waves issue first
    for (;;) {  // (kServer: once per stretch of posted work; the others: once)
        if constexpr (kServer) {  // (no path in flight: the state starts afresh, so none of it is live across the wait)
            work = false;
            ray = Ray{mk(0, 0, 0), mk(0, 0, 1)};
            tv = Trav{};
            tv.mi = nm;
            smp = Sampler{0u, 0u, 0u};
            ms = MediumStack{0ull, 0};
            fs = bounce = slot = 0u;
            acc_rough = 0.0f;
        }
        for (;;) {
            // ---- kQueue: the wave refills a spent unit, and idle lanes (the wave's start; lanes whose take found both
            // units spent) become fresh: they take their item in the shading pass below
            if constexpr (kServer) {
                wave_lds_sync();
                if (lane == 0u) lds_put(hg_q_empty, sv_refill(kp) ? 1u : 0u);
                wave_lds_sync();
                if (!work && __builtin_amdgcn_readfirstlane(lds_get(hg_q_empty)) == 0u) {
                    work = true;
                    bounce = kFreshLane;
                    tv.mi = nm;
                }
            } else if (kQueue && !dry) {
                wave_lds_sync();
                if (__builtin_amdgcn_readfirstlane(lds_get(hg_q_need)) != 0u) {  // (an idle lane implies a take past it)
                    if (lane == 0u) {
                        lds_put(hg_q_need, 0u);
                        lds_put(hg_q_empty, queue_refill(kp, n_units, split) ? 1u : 0u);
                    }
                    wave_lds_sync();
                    dry = __builtin_amdgcn_readfirstlane(lds_get(hg_q_empty)) != 0u;
                }
                if (!work && !dry) {
                    work = true;
                    bounce = kFreshLane;
                    tv.mi = nm;
                }
            }
            if (!__any(work)) break;
            // ---- traversal rounds until few lanes are left traversing
            if (kCounters) cyc_trav -= wave_clock();
            for (;;) {
                const bool act = work && tv.mi < nm;
                const uint64_t am = wave_ballot(act);
                // (work includes act: some lane waits to shade iff the work mask differs)
                if (am == 0ull || (uint32_t(__builtin_popcountll(am)) <= kTmin && wave_ballot(work) != am)) break;
                trav_step<kMeshLds>(kp, ray, tv, c, stk, act, ls);
            }
            if (kCounters) {
                const uint64_t t = wave_clock();
                cyc_trav += t;
                cyc_shade -= t;
            }
            __builtin_amdgcn_s_setprio(0);
            // ---- finished lanes: shade, then start their next ray (a ray with nothing to traverse shades again)
            // (rays that finish at once — everything culled — shade again in this loop while at least
            // HG_STREAM_RESHADE lanes need it, otherwise in the next shading phase)
            for (uint32_t it = 0;; ++it) {
                const uint32_t n_sh = wave_count(work && tv.mi >= nm);
                if (n_sh == 0u || (it > 0u && n_sh < kReshade)) break;
                if (work && tv.mi >= nm) {
                c.shade_rounds += wave_once();
                const bool fresh = kQueue && bounce == kFreshLane;  // no path yet: straight to the take below
                bool alive = false;
                f3 thr = s_thr.get(), col = s_col.get();
                if (!fresh) {
                const Hit hit = trav_hit<kMeshLds>(kp, ray, tv);
                if (hit.t < kp.far_) {  // :898-936
                    c.hits++;
                    const Mat mt = load_mat<kMatLds>(kp, hit.mat);
                    col = col + xyz(mt.emis_rough) * thr;
                    uint32_t bt = 0;
                    const f3 att = evaluate_hit<kMatLds>(kp, smp, ms, ray, hit, mt, bt);
                    bounce += 1u << (8u * bt);
                    thr = thr * att;
                    acc_rough += mt.emis_rough.w * thr.x;
                    const float rr = smp.get1(ID_RR);
                    smp.offset += BOUNCE_INC;
                    const float contribution = hg_fmaxf(hg_fmaxf(thr.x, thr.y), thr.z);
                    if (!(rr > contribution)) {
                        thr = thr * rcp_exact(contribution);
                        bounce += 1u << 24;
                        alive = (bounce >> 24) <= kp.max_bounces && !((bounce & 0xFFu) > kp.max_diff ||
                                                                     ((bounce >> 8) & 0xFFu) > kp.max_glossy ||
                                                                     ((bounce >> 16) & 0xFFu) > kp.max_trans);
                    }
                } else {  // :941
                    c.primary_miss += bounce == 0u;  // the path's camera ray (no bounce recorded yet)
                    col = col + sample_sky(kp, ray.d, sky_level(kp, acc_rough)) * thr;
                }
                }
                if (!alive) {
                    // RayColor += trace_ray(...); spp 1: the sum is the path's colour (0 + col == col bit for bit: col
                    // is never -0, it starts at +0 and only has terms added)
                    const bool one_sample = kp.spp == 1;
                    f3 sum = one_sample ? col : s_sum.get() + col;
                    ++fs;
                    bool next = !fresh && (fs & 0xFFFFu) < kp.spp;  // next sample: statics persist (:188-189)
                    if (!next) {
                        const f3 color = sample_mean(kp, sum);
                        const size_t slot_i = kQueue ? size_t(slot) : size_t(items.slot(slot));
                        // this frame's colour, blended later in frame order (hg_blend_frames*; the server's gate + blend)
                        if constexpr (kServer) {
                            if (!fresh) {
                                const uint32_t k = smp.frame - uint32_t(kp.first_frame);  // the server's frame index
                                // (the ring is uncached memory: the gate and blend on another XCD read what this wrote)
                                fc_store(kp.frame_color + size_t(k & lds_get(hg_sv.mask)) * (lds_get(hg_sv.nlt) * 64u) + slot_i,
                                         make_float4(color.x, color.y, color.z, 1.0f));
                                atomicAdd(&hg_sv.win_done[k & 3u], 1u);  // (LDS) one more item of frame k finished
                            }
                        } else if (!fresh) {
                            fc_store(kp.frame_color + fc_index(kp, fs >> 16, slot_i), make_float4(color.x, color.y, color.z, 1.0f));
                        }
                        fs = (fs & 0xFFFF0000u) + 0x10000u;
                        if constexpr (kQueue) {
                            uint32_t f = 0, hx = 0, hy = 0;
                            if (queue_item(wave_take(), slot, f, hx, hy)) {  // the unit's next item: statics reset
                                next = true;
                                sum = mk(0, 0, 0);
                                fs = kServer ? 0u : f << 16;  // (the server's frame index is smp.frame - first_frame)
                                smp = Sampler{kp.accumulate ? uint32_t(kp.first_frame) + f : 1u, pcg_hash(hx + hy * kp.Wu),
                                              0u};
                                ms = MediumStack{0ull, 0};
                            }
                        } else {
                            const uint32_t k = wave_take();
                            if (k < items.n_items) {  // the next (pixel, frame) item: statics reset as for a dispatch
                                uint32_t f, hx, hy;
                                items.get(kp, k, slot, f);
                                items.pixel(slot, hx, hy);
                                next = true;
                                sum = mk(0, 0, 0);
                                fs = f << 16;
                                smp = Sampler{kp.accumulate ? uint32_t(kp.first_frame) + f : 1u, pcg_hash(hx + hy * kp.Wu),
                                              0u};
                                ms = MediumStack{0ull, 0};
                            }
                        }
                    }
                    if (!one_sample) s_sum.set(sum);
                    if (next) {
                        {
                            uint32_t qx, qy;
                            if constexpr (kQueue) slot_pixel(kp, slot, qx, qy);
                            else items.pixel(slot, qx, qy);
                            ray = camera_ray(kp, smp, (float(qx) / kp.W) * 2.0f - 1.0f, (float(qy) / kp.H) * 2.0f - 1.0f);
                        }
                        thr = mk(1, 1, 1);
                        col = mk(0, 0, 0);
                        acc_rough = 0.0f;
                        bounce = 0;
                        paths++;
                        alive = true;
                    } else {
                        work = false;
                    }
                }
                s_thr.set(thr);
                s_col.set(col);
                if (alive) trav_begin<kMeshLds>(kp, ray, tv, c);
                }
            }
            __builtin_amdgcn_s_setprio(HG_TRAVERSE_PRIO);
            if (kCounters) cyc_shade += wave_clock();
        }
        if constexpr (!kServer) {
            break;
        } else {
            // no path in flight and no item to hand out: wait for the host's next frame (polling the host word), or
            // leave.  Outside the tracing loop, where no path state is live (its registers stay the tracing loop's).
            wave_lds_sync();
            if (lane == 0u) lds_put(hg_q_empty, sv_wait(kp));
            wave_lds_sync();
            if (__builtin_amdgcn_readfirstlane(lds_get(hg_q_empty)) != 0u) break;
        }
    }
    if constexpr (kQueue) record_tile_cost(lane);
    else items.record_cost(kp, lane);
    if constexpr (kServer) {  // waves out | grid << 32 (the gates: a frame still short once all left is lost)
        if (lane == 0u) {
            // after this wave's frame counts (its last sv_flush) have completed in memory
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __builtin_amdgcn_s_waitcnt(0);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __hip_atomic_store(kp.queue + HG_SV_EXIT_WORD + 1u, gridDim.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(kp.queue + HG_SV_EXIT_WORD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (kQueue && !kServer) {
        // The last wave out resets the queue heads for the next launch on this stream (no memset launch per queue
        // launch: a blit kernel waited for a CU that the other streams' persistent waves held).  A wave leaves only
        // once its pulls found the queue dry, and it pulls no more after that: every head atomic of the launch has
        // returned before the last wave's increment of the exit count.  Relaxed: an agent-scope acquire / release is
        // a write-back / invalidate of the XCD's whole L2 on gfx950, per wave leaving (strict C3 +1.3 %, a display
        // one frame behind +3.4 % without it; DESIGN.md section 10 lever 13); the next launch on this stream starts
        // after this one's end.
        if (lane == 0u) {
            const uint32_t out = __hip_atomic_fetch_add(kp.queue + HG_QUEUE_DONE_WORD, 1u, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
            if (out == gridDim.x - 1u) {
                for (uint32_t h = 0; h < 8u; ++h)
                    __hip_atomic_store(kp.queue + 32u * h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(kp.queue + HG_QUEUE_DONE_WORD, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (kCounters) flush_counters<true>(kp, lane, paths, c, cyc_trav, cyc_shade);
}

hipError_t hg_launch_mega_stream(const HgKernelParams& kp_in, int block, bool counters, hipStream_t stream, bool server) {
    (void)block;  // one wave per workgroup (the kernel's LDS rows assume it)
    int64_t grid = int64_t(kp_in.n_local_tiles) * kp_in.frame_split;
    const bool queue = kp_in.queue != nullptr;  // the runtime passes a queue for launches of few frames
    if (queue) grid = grid < int64_t(kp_in.resident_waves) ? grid : int64_t(kp_in.resident_waves);  // persistent waves
    else if (kp_in.wave_units > 1u && kp_in.frame_split == 1)  // wave_units tiles per wave (UnitItems)
        grid = (grid + kp_in.wave_units - 1) / kp_in.wave_units;
    if (grid == 0) return hipSuccess;
    const uint32_t lds_depth = kp_in.stack_depth < HG_STREAM_LDS_STACK ? kp_in.stack_depth : HG_STREAM_LDS_STACK;
    const size_t lds = size_t(kRowStack + lds_depth) * 64u * sizeof(uint32_t);
    HgKernelParams kp = kp_in;
    // which of the mesh records and the material table the waves keep in LDS, and where (hg_layout.h)
    const HgWaveLdsPlan lp = hg_wave_lds_plan(lds, kp.n_meshes, HG_MAT_LDS_STREAM ? kp.n_materials : 0, kp.spp, HG_WAVE_LDS_BUDGET);
    kp.mesh_lds_word = lp.mesh_word;
    kp.mat_lds_word = lp.mat_word;
    const dim3 g{uint32_t(grid)}, b{64u};
    const size_t sh = lp.bytes;
    // the last wave of the previous launch zeroed the heads and the exit count
    if (HG_CHECK_EXEC && queue && !server && kp.counters)
        hg_launch_check_zeroed(static_cast<const uint32_t*>(kp.queue), uint32_t(HG_QUEUE_BYTES / 4u), kp.counters + 18, stream);
    // D: deep BLAS (kp.stream_deep), the kDeep thresholds.  The server is a queue launch.
    if (server)
        with_flags(
            [&](auto C, auto M, auto T, auto D) {
                hipLaunchKernelGGL((hg_trace_stream_kernel<decltype(C)::value, decltype(M)::value, decltype(T)::value, true,
                                                           decltype(D)::value, true>),
                                   g, b, sh, stream, kp);
            },
            counters, lp.mesh_lds, lp.mat_lds, kp.stream_deep != 0);
    else
        with_flags(
            [&](auto C, auto M, auto T, auto Q, auto D) {
                hipLaunchKernelGGL((hg_trace_stream_kernel<decltype(C)::value, decltype(M)::value, decltype(T)::value,
                                                           decltype(Q)::value, decltype(D)::value, false>),
                                   g, b, sh, stream, kp);
            },
            counters, lp.mesh_lds, lp.mat_lds, queue, kp.stream_deep != 0);
    return hipGetLastError();
}


// Launcher used by the runtime (hg_render.hip)
hipError_t hg_launch_mega(const HgKernelParams& kp, int block, bool counters, hipStream_t stream) {
    const int tiles_per_block = block / 64;
    const int grid = (kp.n_local_tiles + tiles_per_block - 1) / tiles_per_block;
    if (grid == 0) return hipSuccess;
    const size_t lds = hg_mega_lds_bytes(kp.stack_depth, block);
    with_flags(
        [&](auto C, auto D) {
            hipLaunchKernelGGL((hg_trace_kernel<decltype(C)::value, decltype(D)::value>), dim3(uint32_t(grid)), dim3(block),
                               lds, stream, kp);
        },
        counters, kp.debug_mode != 0);
    return hipGetLastError();
}
