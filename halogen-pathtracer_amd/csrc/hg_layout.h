// hg_layout.h — device-side data layout of the Halogen scene in HBM (private to libhalogen_hip.so).
//
// The ABI structs (include/halogen_abi.h) are the reference's AoS C# layouts.  hg_upload_scene repacks
// them once (hg_scene_pack.h) into the layout below, chosen for the gfx950 traversal loop:
//
//   node records   64 B per INNER BLAS entry, CHILD-PAIR form: a record holds the boxes of the entry's two
//                  children and their node refs, so popping an inner node costs exactly one 64-B record fetch
//                  (4 x dwordx4) and the reference's re-read of the popped node (HalgoenCompute.compute:405)
//                  disappears.  Leaf entries have no record.  Records are numbered in depth-first pre-order of
//                  sibling pairs: two inner siblings sit at records 2k and 2k + 1 (one 128-B line; a zero pad
//                  record is inserted where the pair would start odd) and a subtree's records are contiguous.
//   node ref       uint32, decided at upload from triangleCount, so the kernel never has to read a node to
//                  know what it is.  Bit 31 clear: the record number of an inner entry.  Bit 31 set: a leaf;
//                  a leaf of 1..15 triangles whose first triangle is below 2^27 is INLINE, HG_LEAF_BIT |
//                  count << 27 | global first triangle (no memory access to find its triangles; never equal
//                  to HG_NONE); any other leaf has count bits 0 and indexes the leaf table.
//   leaf table     the escape for larger leaves, 8 B each: (global first triangle, triangle count).
//   triangles      36 B per triangle, packed (v0.xyz, e1.xyz, e2.xyz), where e1 = v1 - v0 and e2 = v2 - v0 are the
//                  reference's own first two subtractions (:312-313) done once on the host with the same IEEE
//                  operation; a leaf's triangles sit on 2-3 cache lines.
//   normals        48 B per triangle (n0, n1 - n0, n2 - n0), read once per accepted hit.
//   meshes         144 B per mesh (HgDevMesh): full worldToLocal (16 floats, Unity column-major), root ref,
//                  triangle offset, material index, the exact-cull boxes.
//   cull table     32 B per entry, one or two entries per cullable mesh below 64 (hg_cull.h): the exact-cull boxes
//                  again, contiguous, which is all a ray start reads of the meshes.
//   spheres        48 B: (centre, radius), (cornerA, material bits), (cornerB, 0).
//   materials      80 B: albedo; (specular.rgb, metallic); (emissive.rgb*intensity, roughness);
//                  (absorption.xyz, ior); (priority, medium id, roughness^2, 0).
//   accumulation   float4 per pixel, TILE-MAJOR: 8x8 tiles of 1 KiB, local tile t holds global tile
//                  rank + t*n_ranks, pixel (lx,ly) at lx + 8*ly — one wave writes one contiguous KiB.
//
// The measured-and-rejected experiments of rounds 1-4 (wavefront pipeline, path pool, LDS node cache, quad /
// deduplicated node fetch, ray sort, path migration, packed-pair and stream triangle layouts, ...) were removed from
// the sources in round 5; their designs and numbers stay in DESIGN.md section 10 and in git history.
#pragma once
#include <stdint.h>

#include "hg_tunables.h"

struct alignas(16) HgDevMesh {
    float w2l[16];  // Unity column-major: column c = w2l[4c .. 4c+3]
    uint32_t root_ref;
    uint32_t tri_offset;
    uint32_t material;
    uint32_t cullable;  // 1: the root is an inner node and cull_* hold its children's padded world boxes
    // World-space boxes of the root's two children, padded far beyond every float rounding of the reference's
    // local-space test (hg_scene_pack.h: mesh_cull_boxes).  If a ray certainly misses both (or meets them only
    // beyond its current closest hit), the reference's traversal of this mesh would test exactly those two
    // boxes, push nothing and find nothing — so the mesh is skipped and only its 2 AABB tests are counted.
    float4 cull_a_lo, cull_a_hi, cull_b_lo, cull_b_hi;
};

// The cull table (hg_cull.h): what a ray start reads of the boxes above, 32 B per entry: (lo.xyz, tag), (hi.xyz, 0).
// tag: the mesh index, and HG_CULL_MORE when the next entry belongs to the same mesh.
#define HG_CULL_MAX_MESHES 64u
#define HG_CULL_MESH_MASK 0x3Fu
#define HG_CULL_MORE 0x80000000u

// Everything the trace kernel needs, passed by value as the kernel argument.
struct HgKernelParams {
    // camera (rows 0..2 of CamLocalToWorldMatrix, row-major: cam[r*4+c] = M(r,c))
    float cam[12];
    float W, H;
    uint32_t Wu, Hu;
    float vw, vh, near_, far_;
    float focal_disc_radius;  // tan(radians(focalConeAngle)) * near, evaluated on the host with hg_fmath.h
    float psx, psy;           // (vw*2)/W, (vh*2)/H
    float filter_radius, focal_dist;
    uint32_t spp, max_bounces, max_diff, max_glossy, max_trans;
    uint32_t debug_mode, tri_range, box_range;
    int32_t default_mip;
    int32_t use_cube;
    int32_t n_spheres, n_meshes;
    int32_t first_frame, n_frames, accumulate;
    // frame-parallel split (regenerating kernel): frame_split waves share each tile, wave k tracing frames
    // [k*n_frames/split, (k+1)*n_frames/split) into frame_color (fc_index); hg_blend_frames_* (hg_blend.hip) then applies the
    // accumulation blend in frame order.  frame_split == 1: the kernel blends into acc itself.
    int32_t frame_split;
    float4* __restrict__ frame_color;  // render server: a ring of sv_ring frames, frame k at [(k & (sv_ring-1)) * slots]
    // render server (kServer): per ring slot a completion count on its own 128-B line (word 32 s), advanced by
    // n_local_tiles for every frame of that slot; the context stream's gate waits for it (hg_server_gate)
    uint32_t* __restrict__ frames_done;
    // cost-ordered dispatch (regen / stream kernels): wave w traces local tile tile_order[w % n_local_tiles] (null:
    // tile w % n_local_tiles) and adds its wave-clock cost to tile_cost[tile] (null: not recorded).  Any permutation
    // gives the same image: tiles are independent and each tile's frames keep their order.
    unsigned long long* __restrict__ tile_cost;  // s_memtime cycles per tile
    const uint32_t* __restrict__ tile_order;
    // HG_STREAM_QUEUE: 8 unit heads (one per XCD, 128 B apart: queue[32 h]), zeroed before each streaming launch, and
    // the number of persistent waves (one per resident wave slot of the GPU)
    uint32_t* __restrict__ queue;
    uint32_t resident_waves;
    // streaming launches without the queue and without a frame split: each wave traces wave_units consecutive units
    // of the cost order (1: one tile per wave), its lanes taking their items one after another (UnitItems, hg_sched.h)
    uint32_t wave_units;
    // render server: the host words in pinned host memory (HG_SV_HOST_*; [0] the post word, frames posted | stop << 32)
    const unsigned long long* __restrict__ sv_post;
    uint32_t sv_ring;        // colour ring slots (a power of two)
    uint32_t sv_frames_cap;  // frames the server may trace in its lifetime (n_local_tiles * frames < 2^31)
    uint32_t sv_idle_ticks;  // nothing posted for this long (100-MHz s_memrealtime ticks): a wave closes the server
    uint32_t sv_div_magic, sv_div_shift;  // unit -> frame: u / n_local_tiles = umulhi(u, magic) >> shift (u < 2^31)
    // tiling
    int32_t tiles_x, rank, n_ranks, n_local_tiles;
    uint32_t stack_depth;  // LDS traversal stack entries per lane
    uint32_t mesh_lds_word;  // the mesh records' LDS copy starts at this word (hg_wave_lds_plan below)
    uint32_t descent_t;    // relaxed while-while threshold (hg_dev_trav.h isect_meshes), 0 = classic while-while
    uint32_t stream_deep;  // streaming kernel: the deep-BLAS shading thresholds (HG_STREAM_TMIN_DEEP / _RESHADE_DEEP)
    uint32_t mat_lds_word;  // the material table's LDS copy starts at this word (kMatLds launches; hg_wave_lds_plan)
    uint32_t* __restrict__ spill;  // per-lane traversal stack entries beyond the LDS part (rarely touched)
    uint32_t spill_stride;          // = threads of the launch grid
    // cubemap
    int32_t cube_size, cube_mips;
    uint32_t cube_mip_offset[HG_MAX_CUBE_MIPS];  // in float4 texels
    // scene
    int32_t n_materials;  // records of `materials` (what a wave copies into its LDS)
    uint32_t n_cull;      // entries of `cull` that belong to meshes below n_meshes
    const float4* __restrict__ spheres;
    const HgDevMesh* __restrict__ meshes;
    const float4* __restrict__ cull;  // the cull table, 2 float4 per entry, an even number of entries allocated
    const float4* __restrict__ materials;
    const float4* __restrict__ nodes;
    const uint2* __restrict__ leaves;
    const float* __restrict__ tris;  // 9 floats per triangle: v0, e1, e2
    const float4* __restrict__ normals;
    const float4* __restrict__ cube;
    // outputs
    float4* __restrict__ acc;
    unsigned long long* __restrict__ counters;  // 32 x u64: 0-6 hg_counters' first 7 fields, 7-15 wave-level
                                                // rounds / clocks, 16 primary misses (hg_runtime.hip hg_get_counters)
};

#define HG_NONE 0xFFFFFFFFu
#define HG_SPHERE_BIT 0x80000000u

// ---- the dynamic LDS of a one-wave workgroup of the regenerating and streaming kernels (hg_mega.hip) ----------------
// `rows` of 64 words come first: the lane's throughput (rows 0-2), path colour (3-5) and sample sum (6-8), then, in the
// streaming kernel, a spare row and the leaf-share words, then the traversal stack's LDS entries.  Two read-only tables
// that are the same for every wave may follow, each copied by the wave once at its start:
//   mesh records   HG_MESH_LDS_F4 float4 per mesh, after the rows, when they fit the budget;
//   materials      HG_MAT_F4 float4 per material.  At spp 1 the kernels only initialise the sample-sum rows, before
//                  the copy (hg_mega.hip mat_lds_begin), and never read or write them again (the sum of one sample
//                  is the sample: sample_mean and the `one_sample` branches), so a table of at most
//                  HG_SUM_ROWS_BYTES lives there and the launch needs no more LDS than without it.  Otherwise it
//                  goes behind the mesh records (behind the rows, when those stay in global memory) if the budget
//                  still allows; else the kernels read it from global memory.
// The rows are never shortened and the mesh records are placed first, so the material table never displaces either.
// A budget of 0 keeps both tables in global memory.
#define HG_MAT_F4 5  // float4 per material record
#define HG_ROW_SUM 6u  // first of the three sample-sum rows, both kernels
#define HG_SUM_ROWS_BYTES (3u * 64u * 4u)

struct HgWaveLdsPlan {
    uint32_t mesh_word, mat_word;  // first LDS word of each table (mat_word: only with mat_lds)
    uint32_t bytes;                // dynamic LDS bytes of the launch
    bool mesh_lds, mat_lds;        // which tables the waves copy into LDS
    bool mat_in_sum_rows;          // the material table lies in the sample-sum rows
};

inline HgWaveLdsPlan hg_wave_lds_plan(size_t rows_bytes, int32_t n_meshes, int32_t n_materials, uint32_t spp,
                                      size_t budget) {
    HgWaveLdsPlan p{uint32_t(rows_bytes / 4u), 0u, uint32_t(rows_bytes), false, false, false};
    if (budget == 0) return p;
    size_t end = rows_bytes;
    const size_t mesh_bytes = n_meshes > 0 ? size_t(n_meshes) * HG_MESH_LDS_F4 * 16u : 0;
    if (mesh_bytes && end + mesh_bytes <= budget) {
        p.mesh_lds = true;
        end += mesh_bytes;
    }
    const size_t mat_bytes = n_materials > 0 ? size_t(n_materials) * HG_MAT_F4 * 16u : 0;
    if (mat_bytes && spp == 1u && mat_bytes <= HG_SUM_ROWS_BYTES &&
        rows_bytes >= size_t(HG_ROW_SUM) * 256u + HG_SUM_ROWS_BYTES) {
        p.mat_lds = p.mat_in_sum_rows = true;
        p.mat_word = HG_ROW_SUM * 64u;
    } else if (mat_bytes && end + mat_bytes <= budget) {
        p.mat_lds = true;
        p.mat_word = uint32_t(end / 4u);
        end += mat_bytes;
    }
    p.bytes = uint32_t(end);
    return p;
}
