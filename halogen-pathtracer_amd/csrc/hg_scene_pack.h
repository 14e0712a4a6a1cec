// hg_scene_pack.h — what hg_upload_scene does before anything reaches the device: the decision (skip / partial / full),
// the validation of the caller's arrays and the layout of the device scene (hg_layout.h).  Plain functions of plain
// arrays and nothing of HIP, so plain g++ compiles this header: tests/test_scene_pack.py and host/asan_scene_pack.cpp
// (AddressSanitizer + UBSan) run it with no GPU.  hg_runtime.hip keeps the HIP calls and the context's bookkeeping.
// Also here: what changes in those decisions once a mesh was refitted on the device (hg_refit.hip), tested by
// tests/test_refit.py and host/asan_refit.cpp.
//
// An error is the HG_E_* code plus its text (HgPackError); hg_runtime.hip hands both to fail().
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "halogen_abi.h"
#include "hg_tunables.h"

// hg_layout.h names float4 and uint2 and leaves them to its includer.  Without HIP's vector types: plain structs of
// their size and alignment (hg_runtime.hip asserts that HIP's agree).
#ifndef HIP_INCLUDE_HIP_AMD_DETAIL_HIP_VECTOR_TYPES_H
#define HG_VECTOR_SHIM 1
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(8) uint2 { uint32_t x, y; };
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
#endif
#define HG_FLOAT4_BYTES 16
#define HG_UINT2_BYTES 8
static_assert(sizeof(float4) == HG_FLOAT4_BYTES && alignof(float4) == HG_FLOAT4_BYTES, "float4 is 16 B, 16-B aligned");
static_assert(sizeof(uint2) == HG_UINT2_BYTES && alignof(uint2) == HG_UINT2_BYTES, "uint2 is 8 B, 8-B aligned");

#include "hg_host_pool.h"
#include "hg_layout.h"
#include "hg_cull.h"
#include "hg_refit.h"
#include "hg_refit_plan.h"

constexpr uint32_t kMaxStack = 64;  // LDS stack entries per lane; BLAS depth must be <= kMaxStack - 2
constexpr int kHostThreads = 16;    // host threads of hg_upload_scene's compare / repack (the GPU box's CPU share)
static_assert(HG_REFIT_MAX_DEPTH == kMaxStack - 2, "hg_refit_blas accepts the depths hg_pack_geometry accepts");

// The traversal stack entries per lane for a scene whose deepest BLAS entry is `max_depth` levels below its root
inline uint32_t hg_stack_depth(uint32_t max_depth) { return std::max<uint32_t>(2u, (max_depth + 2 + 1) & ~1u); }

struct HgPackError {
    int code = HG_OK;
    std::string text;
};

inline int hg_pack_fail(HgPackError& err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err.code = code;
    err.text = buf;
    return code;
}

// The caller's five arrays, in the order of hg_ctx::scene_copy (spheres, meshes, materials, triangles, BLAS entries)
struct HgSceneIn {
    const HalogenSphere* spheres;
    int32_t n_spheres;
    const HalogenMeshData* meshes;
    int32_t n_meshes;
    const PackedHalogenMaterial* materials;
    int32_t n_materials;
    const HalogenTriangle* tris;
    int32_t n_tris;
    const BVHEntry* blas;
    int32_t n_nodes;
    const void* src(int k) const {
        const void* p[5] = {spheres, meshes, materials, tris, blas};
        return p[k];
    }
    size_t bytes(int k) const {
        const size_t b[5] = {size_t(n_spheres) * sizeof(HalogenSphere), size_t(n_meshes) * sizeof(HalogenMeshData),
                             size_t(n_materials) * sizeof(PackedHalogenMaterial),
                             size_t(n_tris) * sizeof(HalogenTriangle), size_t(n_nodes) * sizeof(BVHEntry)};
        return b[k];
    }
};

// The host staging of the device scene (hg_layout.h).  A partial pack fills sph, mat, dm and cull only.
struct HgScenePack {
    std::vector<float4> sph, mat;
    std::vector<HgDevMesh> dm;
    HgCullTable cull;  // of dm (hg_cull.h): every function that fills dm ends by deriving it
    std::vector<float4> rec;
    std::vector<uint2> leaf;
    std::vector<float> t9;  // (v0, e1, e2) of tri_load, packed per triangle
    std::vector<float4> nrm;
    uint32_t stack_depth = 2;
};

inline float4 f4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
inline float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline float bits(int32_t i) { float f; std::memcpy(&f, &i, 4); return f; }

// Padded world-space boxes of a mesh root's two children (for the exact mesh skip, hg_dev_isect.h mesh_live_mask).
// The local box corners go through the double-precision inverse of the float worldToLocal the kernel uses;
// the pad (1e-3 of the box size + 1e-4 of the coordinate magnitude + 1e-5) exceeds by orders of magnitude
// the float rounding of the reference's local-space slab test (~1e-7 relative), so "misses the padded box"
// implies "the reference's ray_AABB_test returns INF (or a tEntry beyond the closest hit)".
inline bool invert4(const double a[16], double out[16]) {
    double inv[16];
    inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] +
             a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
    inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] -
             a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
    inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] +
             a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
    inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] -
              a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
    inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] -
             a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
    inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] +
             a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
    inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] -
             a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
    inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] +
              a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
    inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] +
             a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
    inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] -
             a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
    inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] +
              a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
    inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] -
              a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
    inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] -
             a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
    inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] +
             a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
    inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] -
              a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
    inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] +
              a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
    const double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
    if (!(std::fabs(det) > 1e-30) || !std::isfinite(det)) return false;
    for (int i = 0; i < 16; ++i) out[i] = inv[i] / det;
    return true;
}

inline bool world_box(const double l2w[16], const BVHEntry& e, float4& lo, float4& hi) {
    const float c[2][3] = {{e.boundingCornerA.x, e.boundingCornerA.y, e.boundingCornerA.z},
                           {e.boundingCornerB.x, e.boundingCornerB.y, e.boundingCornerB.z}};
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int k = 0; k < 8; ++k) {
        const double p[3] = {c[k & 1][0], c[(k >> 1) & 1][1], c[(k >> 2) & 1][2]};
        for (int r = 0; r < 3; ++r) {  // column-major: M(r,col) = l2w[col*4 + r]
            const double w = l2w[r] * p[0] + l2w[4 + r] * p[1] + l2w[8 + r] * p[2] + l2w[12 + r];
            if (!std::isfinite(w)) return false;
            mn[r] = std::min(mn[r], w);
            mx[r] = std::max(mx[r], w);
        }
    }
    double size = 0.0, mag = 0.0;
    for (int r = 0; r < 3; ++r) {
        size = std::max(size, mx[r] - mn[r]);
        mag = std::max({mag, std::fabs(mn[r]), std::fabs(mx[r])});
    }
    const double pad = 1e-3 * size + 1e-4 * mag + 1e-5;
    lo = make_float4(float(mn[0] - pad), float(mn[1] - pad), float(mn[2] - pad), 0.0f);
    hi = make_float4(float(mx[0] + pad), float(mx[1] + pad), float(mx[2] + pad), 0.0f);
    return true;
}

inline bool mesh_cull_boxes(const hg_mat4& w2l, const BVHEntry& A, const BVHEntry& B, HgDevMesh& dm) {
    double a[16], l2w[16];
    for (int i = 0; i < 16; ++i) a[i] = w2l.m[i];
    if (!invert4(a, l2w)) return false;
    return world_box(l2w, A, dm.cull_a_lo, dm.cull_a_hi) && world_box(l2w, B, dm.cull_b_lo, dm.cull_b_hi);
}

// A mesh record's exact-cull boxes (its root's two children in world space) and cullable flag, from its matrix; all
// zero when not cullable, so a partial re-upload leaves no field of the previous matrix behind
inline void set_cull_boxes(const HalogenMeshData& m, const BVHEntry* blas, HgDevMesh& dm) {
    dm.cullable = 0;
    dm.cull_a_lo = dm.cull_a_hi = dm.cull_b_lo = dm.cull_b_hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t off = m.accelerationBufferOffset;
    if (blas[off].triangleCount != 0) return;
    const BVHEntry& A = blas[off + blas[off].indexA];
    const BVHEntry& B = blas[off + blas[off].indexA + 1];
    if (mesh_cull_boxes(m.worldToLocal, A, B, dm)) dm.cullable = 1;
    else dm.cull_a_lo = dm.cull_a_hi = dm.cull_b_lo = dm.cull_b_hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// The child-pair record layout (hg_dev_records.h node_pair): q0 = (A.lo, refA), q1 = (A.hi, refB), q2 = (B.lo, -), q3 = (B.hi, -)
inline void put_pair(float4* r, const BVHEntry& A, const BVHEntry& B, uint32_t ra, uint32_t rb) {
    r[0] = f4(A.boundingCornerA.x, A.boundingCornerA.y, A.boundingCornerA.z, bits(ra));
    r[1] = f4(A.boundingCornerB.x, A.boundingCornerB.y, A.boundingCornerB.z, bits(rb));
    r[2] = f4(B.boundingCornerA.x, B.boundingCornerA.y, B.boundingCornerA.z, 0.0f);
    r[3] = f4(B.boundingCornerB.x, B.boundingCornerB.y, B.boundingCornerB.z, 0.0f);
}

// fn(begin, end) over [0, n) in contiguous chunks on the persistent host pool (hg_host_pool.h), at most `max_threads`
// chunks of at least `grain` items
template <class F>
void parallel_for(size_t n, size_t grain, int max_threads, F fn) {
    HgHostPool& pool = HgHostPool::get();
    const size_t t = std::max<size_t>(1, std::min<size_t>({size_t(max_threads), size_t(pool.threads()),
                                                           (n + grain - 1) / std::max<size_t>(grain, 1)}));
    if (t <= 1) {
        fn(size_t(0), n);
        return;
    }
    const size_t chunk = (n + t - 1) / t;
    pool.run(t, [&](size_t k) {
        const size_t b = std::min(n, k * chunk), e = std::min(n, b + chunk);
        if (b < e) fn(b, e);
    });
}

// Byte equality of two buffers, compared in parallel chunks (the scene's triangle array is 63 MB at C3)
inline bool same_bytes(const void* a, const void* b, size_t n) {
    if (n == 0) return true;
    std::atomic<bool> diff{false};
    parallel_for(n, size_t(4) << 20, kHostThreads, [&](size_t lo, size_t hi) {
        constexpr size_t step = size_t(1) << 20;
        for (size_t i = lo; i < hi && !diff.load(std::memory_order_relaxed); i += step)
            if (std::memcmp(static_cast<const char*>(a) + i, static_cast<const char*>(b) + i, std::min(step, hi - i)))
                diff.store(true, std::memory_order_relaxed);
    });
    return !diff.load();
}

inline void copy_bytes(std::vector<uint8_t>& dst, const void* src, size_t n) {
    dst.resize(n);
    if (n == 0) return;
    parallel_for(n, size_t(4) << 20, kHostThreads, [&](size_t lo, size_t hi) {
        std::memcpy(dst.data() + lo, static_cast<const char*>(src) + lo, hi - lo);
    });
}

inline int hg_scene_check_limits(const HgSceneIn& in, HgPackError& err) {
    // the traversal addresses nodes / triangles with 32-bit byte offsets (hg_dev_records.h ld_off)
    if (in.n_nodes >= (1 << 26) || in.n_tris >= (1 << 28))
        return hg_pack_fail(err, HG_E_UNSUPPORTED,
                            "scene too large: %d BLAS entries (max 2^26-1), %d triangles (max 2^28-1)", in.n_nodes,
                            in.n_tris);
    if (in.n_materials > 255)
        return hg_pack_fail(err, HG_E_UNSUPPORTED,
                            "at most 255 materials (medium stack packs material indices in bytes)");
    return HG_OK;
}

// hg_upload_cubemap's mip table: mip m of the [mip][face][y][x][4] chain starts at float4 texel mip_offset[m]; returns the
// floats of the whole chain (n_mips <= HG_MAX_CUBE_MIPS).  Also called by the test-only probe (hg_devprobe.hip).
inline uint64_t hg_cube_mip_offsets(int32_t face_size, int32_t n_mips, uint32_t* mip_offset) {
    uint64_t need = 0;
    for (int m = 0; m < n_mips; ++m) {
        mip_offset[m] = uint32_t(need / 4);
        const uint64_t s = std::max(1, face_size >> m);
        need += 6ull * s * s * 4ull;
    }
    return need;
}

// ---- the upload decision ----------------------------------------------------------------------------------------------
enum HgUploadKind { HG_UPLOAD_SKIP, HG_UPLOAD_PARTIAL, HG_UPLOAD_FULL };
struct HgUploadDecision {
    HgUploadKind kind;
    bool vouched;  // the caller's geometry generation stood in for the compare of the triangles and BVH entries
};

// What an upload of `in` under `generation` has to do, given the last upload: `copy` its retained arrays, `last_gen` its
// generation, `n_dev_meshes` the length of its device mesh table (has_scene false: there is none, a full rebuild).
//
// Skip: an upload of exactly the arrays already on the device changes nothing: the reference re-uploads every buffer
// on each camera move (ClearAccumulation sets ObjectBuffersDirty, RP:262-268, 296-299), and the drop-in keeps that
// call pattern.  Compared byte for byte against the retained host copies of the last upload (in parallel; ~3 ms
// for C3's 80 MB), it skips the validation, the repack, the copies, the quiesce and the cost-order reset.
// Partial: the triangles and the BVH entries are the last upload's and every mesh keeps its buffer offsets (objects
// moved, or materials / spheres changed): the node records, leaves, triangles and normals on the device stay; only
// the mesh table (world->local matrices, materials, exact-cull boxes), spheres and materials are rebuilt and copied.
// Same device contents as a full upload of these arrays.
inline HgUploadDecision hg_upload_decide(bool has_scene, const std::vector<uint8_t> (&copy)[5], uint64_t last_gen,
                                         size_t n_dev_meshes, const HgSceneIn& in, uint64_t generation) {
    // A caller-kept geometry generation equal to the last upload's vouches for the triangles and BVH entries (the C# /
    // C++ / Python passes bump it when RayTracingManager's mesh registry changes): no compare of those 78 MB (C3).
    const bool vouched = has_scene && generation != 0 && generation == last_gen;
    if (!has_scene) return {HG_UPLOAD_FULL, vouched};
    bool same[5];
    for (int k = 0; k < 5; ++k) same[k] = copy[k].size() == in.bytes(k);
    for (int k = 0; k < 3; ++k)
        same[k] = same[k] && (!in.bytes(k) || !std::memcmp(copy[k].data(), in.src(k), in.bytes(k)));
    for (int k = 3; k < 5; ++k) same[k] = same[k] && (vouched || same_bytes(copy[k].data(), in.src(k), in.bytes(k)));
    if (same[0] && same[1] && same[2] && same[3] && same[4]) return {HG_UPLOAD_SKIP, vouched};
    bool partial = same[3] && same[4] && size_t(in.n_meshes) == n_dev_meshes && copy[1].size() == in.bytes(1);
    for (int mi = 0; partial && mi < in.n_meshes; ++mi) {
        const HalogenMeshData& o = reinterpret_cast<const HalogenMeshData*>(copy[1].data())[mi];
        partial = o.triangleBufferOffset == in.meshes[mi].triangleBufferOffset &&
                  o.accelerationBufferOffset == in.meshes[mi].accelerationBufferOffset;
    }
    return {partial ? HG_UPLOAD_PARTIAL : HG_UPLOAD_FULL, vouched};
}

// ---- the tables: spheres, materials and the matrix-dependent mesh fields (both kinds of upload) ------------------------
inline int hg_pack_spheres_materials(const HgSceneIn& in, HgScenePack& out, HgPackError& err) {
    // ---- spheres
    std::vector<float4>& sph = out.sph;
    sph.assign(size_t(in.n_spheres) * 3, f4(0, 0, 0, 0));
    for (int i = 0; i < in.n_spheres; ++i) {
        const HalogenSphere& s = in.spheres[i];
        if (s.materialIndex >= uint32_t(in.n_materials))
            return hg_pack_fail(err, HG_E_INVALID, "sphere %d: materialIndex %u out of range", i, s.materialIndex);
        sph[3 * i] = f4(s.center.x, s.center.y, s.center.z, s.radius);
        sph[3 * i + 1] = f4(s.boundingCornerA.x, s.boundingCornerA.y, s.boundingCornerA.z, bits(s.materialIndex));
        sph[3 * i + 2] = f4(s.boundingCornerB.x, s.boundingCornerB.y, s.boundingCornerB.z, 0.0f);
    }
    // ---- materials
    std::vector<float4>& mat = out.mat;
    mat.assign(size_t(in.n_materials) * 5, f4(0, 0, 0, 0));
    for (int i = 0; i < in.n_materials; ++i) {
        const PackedHalogenMaterial& m = in.materials[i];
        mat[5 * i] = f4(m.albedo.x, m.albedo.y, m.albedo.z, m.albedo.w);
        mat[5 * i + 1] = f4(m.specularAlbedo.x, m.specularAlbedo.y, m.specularAlbedo.z, m.metallic);
        // emissive.rgb * emissive.a (:901) and roughness^2 (:699) are the kernel's own operations done once here
        mat[5 * i + 2] = f4(m.emissive.x * m.emissive.w, m.emissive.y * m.emissive.w, m.emissive.z * m.emissive.w,
                            m.roughness);
        mat[5 * i + 3] = f4(m.rayMedium.absorption.x, m.rayMedium.absorption.y, m.rayMedium.absorption.z,
                            m.rayMedium.indexOfRefraction);
        mat[5 * i + 4] = f4(bits(m.rayMedium.priority), bits(m.rayMedium.materialID), m.roughness * m.roughness, 0.0f);
    }
    return HG_OK;
}

inline int check_mesh_material(const HgSceneIn& in, int mi, HgPackError& err) {
    if (in.meshes[mi].materialIndex >= uint32_t(in.n_materials))
        return hg_pack_fail(err, HG_E_INVALID, "mesh %d: materialIndex %u out of range", mi,
                            in.meshes[mi].materialIndex);
    return HG_OK;
}

// The fields of a mesh record that follow the mesh's matrix and material (root_ref and tri_offset follow the geometry);
// the mesh's tree has been validated
inline void fill_mesh_record(const HalogenMeshData& m, const BVHEntry* blas, HgDevMesh& dm) {
    std::memcpy(dm.w2l, m.worldToLocal.m, sizeof dm.w2l);
    dm.material = m.materialIndex;
    set_cull_boxes(m, blas, dm);
}

// A partial upload's mesh table: the last upload's (`prev`, whose trees and offsets are these meshes') with every
// matrix-dependent field rebuilt
inline int hg_pack_mesh_table(const HgSceneIn& in, const std::vector<HgDevMesh>& prev, HgScenePack& out,
                              HgPackError& err) {
    std::vector<HgDevMesh>& dm = out.dm;
    dm = prev;
    for (int mi = 0; mi < in.n_meshes; ++mi) {
        if (int rc = check_mesh_material(in, mi, err)) return rc;
        fill_mesh_record(in.meshes[mi], in.blas, dm[mi]);
    }
    hg_cull_table(dm.data(), dm.size(), out.cull);
    return HG_OK;
}

// ---- after a refit (hg_refit_mesh, hg_refit.hip) ------------------------------------------------------------------------
// The local boxes of every mesh root's two children, as the caller's BVH entries hold them (a full upload keeps them on
// the context; a refit replaces those of the meshes it refitted)
inline void hg_root_pairs(const HgSceneIn& in, std::vector<HgRootPair>& out) {
    out.assign(size_t(in.n_meshes), HgRootPair{});
    for (int mi = 0; mi < in.n_meshes; ++mi) {
        const uint32_t off = in.meshes[mi].accelerationBufferOffset;
        if (in.blas[off].triangleCount != 0) continue;
        const BVHEntry* ab = &in.blas[off + in.blas[off].indexA];
        for (int k = 0; k < 2; ++k) {
            std::memcpy(&out[size_t(mi)].box[6 * k], &ab[k].boundingCornerA, 12);
            std::memcpy(&out[size_t(mi)].box[6 * k + 3], &ab[k].boundingCornerB, 12);
        }
    }
}

// set_cull_boxes from kept root-child boxes instead of the caller's BVH entries; `prev` tells whether the root is inner
inline void set_cull_boxes_kept(const HalogenMeshData& m, const HgRootPair& kept, HgDevMesh& dm) {
    const bool inner = !(dm.root_ref & HG_LEAF_BIT);
    dm.cullable = 0;
    dm.cull_a_lo = dm.cull_a_hi = dm.cull_b_lo = dm.cull_b_hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!inner) return;
    BVHEntry ab[2] = {};
    for (int k = 0; k < 2; ++k) {
        std::memcpy(&ab[k].boundingCornerA, &kept.box[6 * k], 12);
        std::memcpy(&ab[k].boundingCornerB, &kept.box[6 * k + 3], 12);
    }
    if (mesh_cull_boxes(m.worldToLocal, ab[0], ab[1], dm)) dm.cullable = 1;
    else dm.cull_a_lo = dm.cull_a_hi = dm.cull_b_lo = dm.cull_b_hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// hg_pack_mesh_table for a context whose geometry was refitted: the caller's BVH entries are not read
inline int hg_pack_mesh_table_kept(const HgSceneIn& in, const std::vector<HgDevMesh>& prev,
                                   const std::vector<HgRootPair>& kept, HgScenePack& out, HgPackError& err) {
    std::vector<HgDevMesh>& dm = out.dm;
    dm = prev;
    for (int mi = 0; mi < in.n_meshes; ++mi) {
        if (int rc = check_mesh_material(in, mi, err)) return rc;
        const HalogenMeshData& m = in.meshes[mi];
        std::memcpy(dm[size_t(mi)].w2l, m.worldToLocal.m, sizeof dm[size_t(mi)].w2l);
        dm[size_t(mi)].material = m.materialIndex;
        set_cull_boxes_kept(m, kept[size_t(mi)], dm[size_t(mi)]);
    }
    hg_cull_table(dm.data(), dm.size(), out.cull);
    return HG_OK;
}

// hg_upload_decide for a context that may have been refitted.  `stale`: a refit changed the device's triangles and
// boxes since the last full upload, so the retained copies of the triangles and BVH entries (copy[3], copy[4]) no
// longer describe the device and nothing may be compared against them.  Then an upload is vouched only when its
// generation is non-zero and the refit's, and the triangle count, the node count and every mesh's two offsets are the
// device's: it decides skip or partial from the three small tables alone.  Every other upload after a refit is a full
// upload from the caller's arrays (which the caller kept current, hg_refit_blas): never skip, never partial.
inline HgUploadDecision hg_upload_decide_refit(bool has_scene, bool stale, const std::vector<uint8_t> (&copy)[5],
                                               uint64_t last_gen, size_t n_dev_meshes, int32_t dev_tris,
                                               int32_t dev_nodes, const HgSceneIn& in, uint64_t generation) {
    if (!has_scene || !stale) return hg_upload_decide(has_scene, copy, last_gen, n_dev_meshes, in, generation);
    bool vouched = generation != 0 && generation == last_gen && in.n_tris == dev_tris && in.n_nodes == dev_nodes &&
                   size_t(in.n_meshes) == n_dev_meshes && copy[1].size() == in.bytes(1);
    for (int mi = 0; vouched && mi < in.n_meshes; ++mi) {
        const HalogenMeshData& o = reinterpret_cast<const HalogenMeshData*>(copy[1].data())[mi];
        vouched = o.triangleBufferOffset == in.meshes[mi].triangleBufferOffset &&
                  o.accelerationBufferOffset == in.meshes[mi].accelerationBufferOffset;
    }
    if (!vouched) return {HG_UPLOAD_FULL, false};
    bool same = true;
    for (int k = 0; k < 3; ++k)
        same = same && copy[k].size() == in.bytes(k) && (!in.bytes(k) || !std::memcmp(copy[k].data(), in.src(k), in.bytes(k)));
    return {same ? HG_UPLOAD_SKIP : HG_UPLOAD_PARTIAL, true};
}

// ---- the geometry of a full rebuild: triangles, BLAS validation, device layout, mesh table -----------------------------
inline int hg_pack_geometry(const HgSceneIn& in, HgScenePack& out, HgPackError& err) {
    const HalogenMeshData* meshes = in.meshes;
    const HalogenTriangle* tris = in.tris;
    const BVHEntry* blas = in.blas;
    const int32_t n_meshes = in.n_meshes, n_tris = in.n_tris, n_nodes = in.n_nodes;
    // ---- triangles (independent per triangle: parallel)
    const size_t nt = size_t(n_tris);
    std::vector<float>& t9 = out.t9;
    std::vector<float4>& nrm = out.nrm;
    t9.assign(nt * 9, 0.0f);
    nrm.assign(nt * 3, f4(0, 0, 0, 0));
    parallel_for(nt, 32768, kHostThreads, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; ++t) {
            const HalogenTriangle& h = tris[t];
            const float e1x = h.pointB.x - h.pointA.x, e1y = h.pointB.y - h.pointA.y, e1z = h.pointB.z - h.pointA.z;
            const float e2x = h.pointC.x - h.pointA.x, e2y = h.pointC.y - h.pointA.y, e2z = h.pointC.z - h.pointA.z;
            const float v[9] = {h.pointA.x, h.pointA.y, h.pointA.z, e1x, e1y, e1z, e2x, e2y, e2z};
            std::memcpy(&t9[9 * t], v, sizeof v);
            nrm[3 * t] = f4(h.normalA.x, h.normalA.y, h.normalA.z, 0.0f);
            nrm[3 * t + 1] = f4(h.normalB.x - h.normalA.x, h.normalB.y - h.normalA.y, h.normalB.z - h.normalA.z, 0.0f);
            nrm[3 * t + 2] = f4(h.normalC.x - h.normalA.x, h.normalC.y - h.normalA.y, h.normalC.z - h.normalA.z, 0.0f);
        }
    });
    // ---- BLAS, pass 1: validate every mesh's tree by DFS (ranges, depth, sharing between meshes)
    std::vector<int64_t> owner(size_t(n_nodes), -1);  // (accOffset << 32 | triOffset) that produced the entry
    std::vector<HgDevMesh>& dm = out.dm;
    dm.assign(static_cast<size_t>(n_meshes), HgDevMesh{});
    uint32_t max_depth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> dfs;
    for (int mi = 0; mi < n_meshes; ++mi) {
        const HalogenMeshData& m = meshes[mi];
        if (int rc = check_mesh_material(in, mi, err)) return rc;
        const uint32_t off = m.accelerationBufferOffset, toff = m.triangleBufferOffset;
        if (off >= uint32_t(n_nodes))
            return hg_pack_fail(err, HG_E_INVALID, "mesh %d: accelerationBufferOffset out of range", mi);
        const int64_t key = (int64_t(off) << 32) | int64_t(toff);
        dfs.assign(1, {off, 0u});
        while (!dfs.empty()) {
            auto [g, depth] = dfs.back();
            dfs.pop_back();
            if (depth + 2 > kMaxStack)
                return hg_pack_fail(err, HG_E_UNSUPPORTED, "mesh %d: BLAS deeper than %u levels (or cyclic)", mi,
                                    kMaxStack - 2);
            max_depth = std::max(max_depth, depth);
            if (owner[g] != -1 && owner[g] != key)
                return hg_pack_fail(err, HG_E_UNSUPPORTED, "BLAS entry %u shared by meshes with different offsets", g);
            owner[g] = key;
            const BVHEntry& e = blas[g];
            if (e.triangleCount > 0) {
                if (uint64_t(toff) + e.indexA + e.triangleCount > uint64_t(n_tris))
                    return hg_pack_fail(err, HG_E_INVALID, "mesh %d: leaf %u references triangles out of range", mi, g);
            } else {
                const uint64_t a = uint64_t(off) + e.indexA;
                if (a + 1 >= uint64_t(n_nodes))
                    return hg_pack_fail(err, HG_E_INVALID, "mesh %d: node %u has children out of range", mi, g);
                dfs.push_back({uint32_t(a + 1), depth + 1});
                dfs.push_back({uint32_t(a), depth + 1});
            }
        }
    }
    // ---- BLAS, pass 2: device layout.  Inner nodes get a child-pair record (both children's boxes + refs, 64 B),
    // leaves an entry of the leaf table.  Records are numbered in depth-first pre-order of sibling pairs: the two
    // children of a node sit in one 128-B line (the far sibling, popped later, is usually still cached) and a
    // subtree's records are contiguous.  Traversal follows refs only, so visit order and results are unchanged.
    std::vector<uint32_t> dref(size_t(n_nodes), HG_NONE);  // device ref of each reference BVH entry
    std::vector<float4>& rec = out.rec;
    std::vector<uint2>& leaf = out.leaf;
    rec.clear();
    leaf.clear();
    rec.reserve(size_t(n_nodes) * 4 + 8);
    auto new_record = [&]() {
        rec.resize(rec.size() + 4, f4(0, 0, 0, 0));
        return uint32_t(rec.size() / 4 - 1);
    };
    std::vector<uint32_t> expand;
    for (int mi = 0; mi < n_meshes; ++mi) {
        const HalogenMeshData& m = meshes[mi];
        const uint32_t off = m.accelerationBufferOffset, toff = m.triangleBufferOffset;
        auto ref_for = [&](uint32_t g, bool with_sibling_pad) -> uint32_t {  // assigns a device ref on first use
            if (dref[g] != HG_NONE) return dref[g];
            const BVHEntry& e = blas[g];
            if (e.triangleCount > 0) {
                const uint64_t first = uint64_t(toff) + e.indexA;
                if (e.triangleCount <= HG_LEAF_INLINE_MAX && first < HG_LEAF_PAYLOAD) {  // never encodes HG_NONE
                    dref[g] = HG_LEAF_BIT | (e.triangleCount << HG_LEAF_CNT_SHIFT) | uint32_t(first);
                } else {
                    if (leaf.size() > HG_LEAF_PAYLOAD) return HG_NONE;  // reported below
                    dref[g] = HG_LEAF_BIT | uint32_t(leaf.size());
                    leaf.push_back(make_uint2(uint32_t(first), e.triangleCount));
                }
            } else {
                if (with_sibling_pad && (rec.size() / 4) % 2 == 1) new_record();  // pair starts on an even record
                dref[g] = new_record();
                expand.push_back(g);
            }
            return dref[g];
        };
        const uint32_t root = ref_for(off, false);
        if (root == HG_NONE) return hg_pack_fail(err, HG_E_UNSUPPORTED, "too many large BLAS leaves");
        while (!expand.empty()) {
            const uint32_t g = expand.back();
            expand.pop_back();
            const uint32_t a = off + blas[g].indexA;
            const bool both_new = dref[a] == HG_NONE && dref[a + 1] == HG_NONE && blas[a].triangleCount == 0 &&
                                  blas[a + 1].triangleCount == 0;
            const size_t mark = expand.size();
            const uint32_t ra = ref_for(a, both_new);
            const uint32_t rb = ref_for(a + 1, false);
            if (ra == HG_NONE || rb == HG_NONE)
                return hg_pack_fail(err, HG_E_UNSUPPORTED, "too many large BLAS leaves");
            if (expand.size() == mark + 2) std::swap(expand[mark], expand[mark + 1]);  // expand child A first
            const BVHEntry& A = blas[a];
            const BVHEntry& B = blas[a + 1];
            put_pair(&rec[4 * size_t(dref[g])], A, B, ra, rb);
        }
        dm[mi].root_ref = root;
        dm[mi].tri_offset = toff;
        fill_mesh_record(m, blas, dm[mi]);
    }
    if (rec.size() / 4 >= (size_t(1) << 26))
        return hg_pack_fail(err, HG_E_UNSUPPORTED, "BLAS too large: %zu device node records", rec.size() / 4);
    if (rec.empty()) new_record();
    if (leaf.empty()) leaf.push_back(make_uint2(0, 0));
    hg_cull_table(dm.data(), dm.size(), out.cull);
    out.stack_depth = hg_stack_depth(max_depth);
    return HG_OK;
}
