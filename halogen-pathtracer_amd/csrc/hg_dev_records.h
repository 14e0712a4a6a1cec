// hg_dev_records.h — per-lane path state and the accessors of the uploaded records: materials, meshes, triangles,
// leaves, child pairs and frame colours (part of hg_device.h).
#pragma once
#include <hip/hip_runtime.h>

#include "hg_dev_math.h"
#include "hg_layout.h"

namespace hgd {

// ---------------------------------------------------------------------------------------------------
// Per-lane path state
// ---------------------------------------------------------------------------------------------------
struct Counters {
    uint32_t rays, tri, aabb, node_rounds, tri_rounds, hits;  // *_rounds: wave-level loop iterations (one lane counts)
    uint32_t shade_rounds;
    uint32_t primary_miss;  // camera rays that hit nothing
};

// bounceTypes[3] of trace_ray (:887) kept as three named registers (a runtime-indexed array would go to
// scratch memory on gfx950)
struct Bounces {
    uint32_t diffuse, glossy, transmission;
    __device__ __forceinline__ void bump(uint32_t t) {
        diffuse += t == 0u;
        glossy += t == 1u;
        transmission += t == 2u;
    }
};

struct Ray {
    f3 o, d;
};

struct Hit {
    float t;
    float orient;
    f3 pos, n;
    uint32_t mat;
};
// "no hit yet": the closest distance seeded with t (+inf for a path's ray, t_max for a query), everything else 0
__device__ __forceinline__ Hit hit_none(float t) { return Hit{t, 0.0f, mk(0, 0, 0), mk(0, 0, 0), 0u}; }

// nested-dielectric stack (:188-189): 8 material indices packed one byte each in a u64 (the medium of a
// stack entry is always the internal medium of a material, so its index identifies it completely)
struct MediumStack {
    uint64_t s;
    int sp;
    __device__ __forceinline__ uint32_t get(int i) const { return uint32_t(s >> (8 * i)) & 0xFFu; }
};

// material record accessors
struct Mat {
    float4 albedo, spec_metal, emis_rough, absorb_ior, prio_id_r2;
};
extern __shared__ __attribute__((aligned(16))) uint32_t hg_lds_stack[];  // (the wave's dynamic LDS, hg_dev_stack.h)
// float4 k of material m.  kLds: from the wave's LDS copy of the table at word kp.mat_lds_word (mat_lds_fill;
// hg_layout.h hg_wave_lds_plan decides where it lies and whether a launch has one), else from global memory.
template <bool kLds = false>
__device__ __forceinline__ float4 mat_f4(const HgKernelParams& kp, uint32_t m, uint32_t k) {
    if constexpr (kLds) return reinterpret_cast<const float4*>(hg_lds_stack + kp.mat_lds_word)[m * HG_MAT_F4 + k];
    else return kp.materials[HG_MAT_F4 * m + k];
}
// copy the material table into the wave's LDS (one wave per workgroup)
__device__ __forceinline__ void mat_lds_fill(const HgKernelParams& kp, uint32_t lane) {
    float4* mt = reinterpret_cast<float4*>(hg_lds_stack + kp.mat_lds_word);
    const uint32_t nf4 = uint32_t(kp.n_materials) * HG_MAT_F4;
    for (uint32_t i = lane; i < nf4; i += 64u) mt[i] = kp.materials[i];
}
template <bool kMatLds = false>
__device__ __forceinline__ Mat load_mat(const HgKernelParams& kp, uint32_t m) {
    return Mat{mat_f4<kMatLds>(kp, m, 0), mat_f4<kMatLds>(kp, m, 1), mat_f4<kMatLds>(kp, m, 2), mat_f4<kMatLds>(kp, m, 3),
               mat_f4<kMatLds>(kp, m, 4)};
}
template <bool kMatLds = false>
__device__ __forceinline__ int32_t mat_priority(const HgKernelParams& kp, uint32_t m) {
    return __float_as_int(mat_f4<kMatLds>(kp, m, 4).x);
}

// The wave's LDS copy of the mesh records (HG_MESH_LDS): mesh m's first HG_MESH_LDS_F4 float4 (w2l columns, header)
// at float4 index m * HG_MESH_LDS_F4 from word kp.mesh_lds_word (after the kernel's stack rows, hg_mega.hip).
template <bool kLds>
__device__ __forceinline__ float4 mesh_f4(const HgKernelParams& kp, uint32_t m, uint32_t k) {
    if constexpr (kLds) return reinterpret_cast<const float4*>(hg_lds_stack + kp.mesh_lds_word)[m * HG_MESH_LDS_F4 + k];
    else return reinterpret_cast<const float4*>(kp.meshes + m)[k];
}
// copy every mesh record's first HG_MESH_LDS_F4 float4 into the wave's LDS (one wave per workgroup)
__device__ __forceinline__ void mesh_lds_fill(const HgKernelParams& kp, uint32_t lane) {
    float4* mt = reinterpret_cast<float4*>(hg_lds_stack + kp.mesh_lds_word);
    const uint32_t nf4 = uint32_t(kp.n_meshes) * HG_MESH_LDS_F4;
    for (uint32_t i = lane; i < nf4; i += 64u) {
        const uint32_t m = i / HG_MESH_LDS_F4;
        mt[i] = reinterpret_cast<const float4*>(kp.meshes + m)[i - m * HG_MESH_LDS_F4];
    }
}

// base + 32-bit byte offset: lets the compiler use the scalar-base + VGPR-offset load form (upload keeps every
// scene array below 4 GiB, hg_runtime.hip)
template <class T>
__device__ __forceinline__ T ld_off(const T* base, uint32_t byte_off) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}

// Frame colour of launch frame f (0 .. n_frames-1) for accumulator slot `slot`: [slot][frame], one pixel's frames
// contiguous (hg_blend_frames* read the same layout)
__device__ __forceinline__ size_t fc_slot_frame(size_t slot, uint32_t f, uint32_t n_frames) {
    return slot * size_t(n_frames) + f;
}
// Frame colours are written once by the trace and read once by the blend: both go through the non-temporal hint, so
// the 2.1 GB a 64-frame C3 launch writes is not kept in L2 ahead of the BVH lines (+0.2..0.6 %, sweep_r03_n)
__device__ __forceinline__ void fc_store(float4* p, float4 v) {
    __builtin_nontemporal_store(v.x, &p->x);
    __builtin_nontemporal_store(v.y, &p->y);
    __builtin_nontemporal_store(v.z, &p->z);
    __builtin_nontemporal_store(v.w, &p->w);
}
__device__ __forceinline__ float4 fc_load(const float4* p) {
    return make_float4(__builtin_nontemporal_load(&p->x), __builtin_nontemporal_load(&p->y),
                       __builtin_nontemporal_load(&p->z), __builtin_nontemporal_load(&p->w));
}
__device__ __forceinline__ size_t fc_index(const HgKernelParams& kp, uint32_t f, size_t slot) {
    return fc_slot_frame(slot, f, uint32_t(kp.n_frames));
}
// The accumulation blend of one frame's colour, acc*(1-w) + c*w with w = 1/FrameCount (AccumulationShader.shader:33),
// and what a launch that does not accumulate stores instead.  Every blend of the library is this one: the lockstep
// kernel's in place and the frame-order blends of hg_blend.hip, the same operations in the same order.
__device__ __forceinline__ float4 blend_frame(float4 a, f3 c, float frame_count) {
    const float w = rcp_exact(frame_count);
    const float k = 1.0f - w;
    return make_float4(a.x * k + c.x * w, a.y * k + c.y * w, a.z * k + c.z * w, a.w * k + 1.0f * w);
}
__device__ __forceinline__ float4 frame_alone(f3 c) { return make_float4(c.x, c.y, c.z, 1.0f); }

// Triangle ti's Moller-Trumbore operands from its packed 36-B record (v0, e1, e2): a = (v0, e1.x), b = (e1.yz, e2.xy),
// cz = e2.z, as two 4-B-aligned 16-B loads and one 4-B load.  (The three SoA streams of rounds 1-2 put a leaf's
// triangles on 3-5 lines instead of 2-3: L1 misses -20 % with this record; 48-B padded records lost 0.3-5.7 %; the
// non-temporal hint on these loads lost 10 %, a leaf's triangles are re-read by the next rounds and waves.)
__device__ __forceinline__ void tri_load(const HgKernelParams& kp, uint32_t ti, float4& a, float4& b, float& cz) {
    typedef float hg_v4u __attribute__((ext_vector_type(4), aligned(4)));  // 4-B aligned 16-B loads
    const char* p = reinterpret_cast<const char*>(kp.tris) + ti * 36u;
    const hg_v4u va = *reinterpret_cast<const hg_v4u*>(p), vb = *reinterpret_cast<const hg_v4u*>(p + 16);
    a = make_float4(va.x, va.y, va.z, va.w);
    b = make_float4(vb.x, vb.y, vb.z, vb.w);
    cz = *reinterpret_cast<const float*>(p + 32);
}

// Load of scene data the kernel never writes (mesh records, spheres) through the constant address space: a
// wave-uniform address then compiles to a scalar load (s_load_dwordx4, scalar cache) even after the kernel's own
// global stores, where a generic load must stay a vector load (one full memory latency per mesh / sphere).
typedef float hg_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ldc(const float4* base, uint32_t i) {
    typedef const __attribute__((address_space(4))) hg_v4f* cptr;
    const hg_v4f v = ((cptr)(uintptr_t)base)[i];
    return make_float4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ uint2 leaf_range(const HgKernelParams& kp, uint32_t ref) {
    const uint32_t cnt = (ref >> HG_LEAF_CNT_SHIFT) & HG_LEAF_INLINE_MAX;
    if (__builtin_expect(cnt != 0u, 1)) return make_uint2(ref & HG_LEAF_PAYLOAD, cnt);
    return ld_off(kp.leaves, (ref & HG_LEAF_PAYLOAD) << 3);
}

// A child-pair record (hg_runtime.hip, BLAS pass 2): both children's boxes and refs in 64 B, 56 of them used:
// q0 = (A.lo, refA), q1 = (A.hi, refB), q2 = (B.lo, -), q3 = (B.hi, -).  (The coordinate-by-coordinate form for packed
// FP32 box tests cost 8-16 B of scratch and lost 1-2.4 %)
struct NodePair {
    float4 q0, q1, q2, q3;
};
__device__ __forceinline__ NodePair node_pair(const HgKernelParams& kp, uint32_t node) {
    const uint32_t ro = node << 6;
    return NodePair{ld_off(kp.nodes, ro), ld_off(kp.nodes, ro + 16), ld_off(kp.nodes, ro + 32), ld_off(kp.nodes, ro + 48)};
}
__device__ __forceinline__ uint32_t pair_ref_a(const NodePair& r) { return __float_as_uint(r.q0.w); }
__device__ __forceinline__ uint32_t pair_ref_b(const NodePair& r) { return __float_as_uint(r.q1.w); }

}  // namespace hgd
