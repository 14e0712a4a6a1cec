// hg_devprobe.hip — TEST INFRASTRUCTURE ONLY (make devprobe -> halogen/devprobe/libhg_devprobe.so; never linked into
// libhalogen_hip.so).  One elementwise entry point that evaluates the device building blocks of hg_device.h
// (20-23: hg_dev_math.h, hg_dev_sampler.h; 30-33: hg_dev_isect.h; 50-51: hg_dev_sky.h; 52-58: hg_dev_shade.h),
// hg_fmath.h and hg_pack.h themselves — the functions the megakernels call, not restatements — on caller-supplied
// inputs, so tests/test_gpu_device_units.py can put each next to its CPU-oracle counterpart (oracle/hg_oracle.c
// hgo_fmath and the hgo_*_batch exports) bit for bit.
//
// hg_devprobe(fn, in, in_bytes, out, out_bytes, n): element i reads kIn[fn] words at in + i * kIn[fn] and writes
// kOut[fn] words at out + i * kOut[fn] (host pointers; 4-byte words, float or uint32 bits):
//   0..11  hg_fmath.h, the codes of hgo_fmath: 0 sin, 1 cos, 2 acos, 3 tan, 4 log, 5 exp, 6 round, 7 rnorm, 8 asin,
//          9 / 10 sin / cos of hg_sincosf, 11 acos_fused                              in: x                  out: y
//   12/13  hg_fminf / hg_fmaxf                                                       in: a, b               out: y
//   20     hgd::rcp_exact                                                            in: x                  out: 1/x
//   21     hgd::pcg_hash                                                             in: v                  out: hash
//   22     hgd::Sampler::get1                                in: frame, pixel, offset, id                   out: u
//   23     hgd::Sampler::get2                                in: frame, pixel, offset, id                   out: a, b
//   30     hgd::ray_aabb                                     in: A, B, o, inv (12 floats)                   out: t
//   31/32  hgd::tri_accept<false> / <true>                   in: lo, ld, best_t, record v0 e1 e2 (16)       out: accept, t, U, V, front
//   33     hgd::isect_spheres, n_spheres = 1                 in: o, d, t, far_, the sphere's 3 float4 (20)  out: ref, t
//   40     hg_pack_r11g11b10                                 in: r, g, b                                    out: word
//   41     hg_pack_rgba16f                                   in: r, g, b, a                                 out: 2 words
// The shading half (tests/test_gpu_shading_units.py; the oracle's side: hgo_sky_batch ... hgo_evaluate_hit_batch):
//   50 T   hgd::sample_sky (with cube_adjacent)              in: direction, level (int)                      out: rgb
//   51     hgd::sky_level                                    in: default_mip (int), acc_rough               out: level
//   52     hgd::lambert                                      in: n, rv                                      out: direction
//   53     hgd::reflect                                      in: i, n                                       out: direction
//   54     hgd::schlick_adjusted                             in: n1, n2, normal, incident, min, max (10)    out: value
//   55     hgd::refract_tir                                  in: incident, normal, n1, n2 (8)               out: direction, tir
//   56 T   hgd::medium_push / medium_pop                     in: sp, stack bytes lo, hi, 16 ops (19)        out: 16 x stack (144)
//          an op is kind << 30 | value: kind 1 push material `value`, 2 pop id `value`, 0 nothing; a stack is sp and
//          medium_of(kp, get(i)).id of each entry below sp (0xFFFFFFFF above), 9 words, given after every op
//   57 T   hgd::evaluate_hit (with material_brdf)            in: frame, pixel, offset; sp, stack bytes lo, hi; ray o, d;
//          hit t, orient, pos, n, mat (21)                   out: att, ray.o, ray.d, bt_out, stack (19)
//   58     hgd::inv_blackman_harris                          in: x                                          out: y
// T: needs tables in device memory and so the second entry point, hg_devprobe_tables(fn, in, ..., n, materials,
// n_materials, cube_texels, n_cube_floats, cube_face_size, cube_mips): the material table is packed from the
// PackedHalogenMaterial array with hg_pack_spheres_materials (hg_scene_pack.h) as hg_upload_scene packs it (56, 57;
// 1..255 materials), the cubemap's mip table is hg_upload_cubemap's hg_cube_mip_offsets (50); either may be null when
// fn does not read it.  HgKernelParams holds only what these functions read.  Material indices (stack bytes below sp,
// pushed materials, the hit's) must be below n_materials and sp within 0..8: checked on the host.
// Returns the HIP status (0 = hipSuccess); hipErrorInvalidValue for an unknown fn, a buffer too small for n, a missing
// table or an element that fails the checks above.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "hg_device.h"
#include "hg_fmath.h"
#include "hg_pack.h"
#include "hg_scene_pack.h"

namespace {

__host__ __device__ constexpr uint32_t words_in(int fn) {
    return (fn >= 0 && fn <= 11) || fn == 20 || fn == 21 ? 1u
           : fn == 12 || fn == 13                        ? 2u
           : fn == 22 || fn == 23                        ? 4u
           : fn == 30                                    ? 12u
           : fn == 31 || fn == 32                        ? 16u
           : fn == 33                                    ? 20u
           : fn == 40                                    ? 3u
           : fn == 41 || fn == 50                        ? 4u
           : fn == 51                                    ? 2u
           : fn == 52 || fn == 53                        ? 6u
           : fn == 54                                    ? 10u
           : fn == 55                                    ? 8u
           : fn == 56                                    ? 19u
           : fn == 57                                    ? 21u
           : fn == 58                                    ? 1u
                                                         : 0u;
}
__host__ __device__ constexpr uint32_t words_out(int fn) {
    return (fn >= 0 && fn <= 13) || fn == 20 || fn == 21 || fn == 22 || fn == 30 || fn == 40 ? 1u
           : fn == 23 || fn == 33 || fn == 41                                                  ? 2u
           : fn == 31 || fn == 32                                                              ? 5u
           : fn == 51 || fn == 54 || fn == 58                                                  ? 1u
           : fn == 50 || fn == 52 || fn == 53                                                  ? 3u
           : fn == 55                                                                          ? 4u
           : fn == 56                                                                          ? 144u
           : fn == 57                                                                          ? 19u
                                                                                               : 0u;
}
__host__ __device__ constexpr bool needs_cube(int fn) { return fn == 50; }
__host__ __device__ constexpr bool needs_materials(int fn) { return fn == 56 || fn == 57; }
constexpr int kProbeMaterials = 256;  // the device table's length: every byte of a medium stack indexes inside it

__device__ float fmath_eval(int fn, float v) {
    float r, o;
    switch (fn) {
        case 0: return hg_sinf(v);
        case 1: return hg_cosf(v);
        case 2: return hg_acosf(v);
        case 3: return hg_tanf(v);
        case 4: return hg_logf(v);
        case 5: return hg_expf(v);
        case 6: return hg_roundf(v);
        case 7: return hg_rnorm(v);
        case 9: hg_sincosf(v, &r, &o); return r;
        case 10: hg_sincosf(v, &o, &r); return r;
        case 11: return hg_acosf_fused(v);
        default: return hg_asinf(v);
    }
}

template <bool kFlat>
__device__ void tri_probe(const float* e, uint32_t* o) {
    const float4 a = make_float4(e[7], e[8], e[9], e[10]), b = make_float4(e[11], e[12], e[13], e[14]);
    float t, U, V;
    bool front;
    const bool acc = hgd::tri_accept<kFlat>(hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5]), a, b, e[15], e[6], t,
                                            U, V, front);
    o[0] = acc ? 1u : 0u;
    o[1] = __float_as_uint(t);
    o[2] = __float_as_uint(U);
    o[3] = __float_as_uint(V);
    o[4] = front ? 1u : 0u;
}

__global__ __launch_bounds__(256) void hg_devprobe_kernel(int fn, const uint32_t* __restrict__ in,
                                                          uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* ui = in + i * words_in(fn);
    const float* e = reinterpret_cast<const float*>(ui);
    uint32_t* o = out + i * words_out(fn);
    if (fn >= 0 && fn <= 11) {
        o[0] = __float_as_uint(fmath_eval(fn, e[0]));
    } else if (fn == 12 || fn == 13) {
        o[0] = __float_as_uint(fn == 12 ? hg_fminf(e[0], e[1]) : hg_fmaxf(e[0], e[1]));
    } else if (fn == 20) {
        o[0] = __float_as_uint(hgd::rcp_exact(e[0]));
    } else if (fn == 21) {
        o[0] = hgd::pcg_hash(ui[0]);
    } else if (fn == 22 || fn == 23) {
        const hgd::Sampler s{ui[0], ui[1], ui[2]};
        if (fn == 22) {
            o[0] = __float_as_uint(s.get1(ui[3]));
        } else {
            float a, b;
            s.get2(ui[3], a, b);
            o[0] = __float_as_uint(a);
            o[1] = __float_as_uint(b);
        }
    } else if (fn == 30) {
        o[0] = __float_as_uint(hgd::ray_aabb(hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5]),
                                             hgd::mk(e[6], e[7], e[8]), hgd::mk(e[9], e[10], e[11])));
    } else if (fn == 31) {
        tri_probe<false>(e, o);
    } else if (fn == 32) {
        tri_probe<true>(e, o);
    } else if (fn == 33) {
        HgKernelParams kp = {};
        kp.n_spheres = 1;
        kp.far_ = e[7];
        kp.spheres = reinterpret_cast<const float4*>(e + 8);  // 80-B elements: 16-B aligned
        const hgd::Ray ray{hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5])};
        float t = e[6];
        o[0] = hgd::isect_spheres(kp, ray, t);
        o[1] = __float_as_uint(t);
    } else if (fn == 40) {
        o[0] = hg_pack_r11g11b10(e[0], e[1], e[2]);
    } else if (fn == 41) {
        hg_pack_rgba16f(e[0], e[1], e[2], e[3], o);
    }
}

__device__ void put_f3(uint32_t* o, hgd::f3 v) {
    o[0] = __float_as_uint(v.x);
    o[1] = __float_as_uint(v.y);
    o[2] = __float_as_uint(v.z);
}
// sp and the id of each entry below it (0xFFFFFFFF above), 9 words
__device__ void put_stack(const HgKernelParams& kp, const hgd::MediumStack& ms, uint32_t* o) {
    o[0] = uint32_t(ms.sp);
    for (int i = 0; i < 8; ++i) o[1 + i] = i < ms.sp ? hgd::medium_of(kp, ms.get(i)).id : 0xFFFFFFFFu;
}

// fn 50..58: the shading half, over the tables of kp
__global__ __launch_bounds__(256) void hg_devprobe_shading_kernel(int fn, HgKernelParams kp,
                                                                  const uint32_t* __restrict__ in,
                                                                  uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* ui = in + i * words_in(fn);
    const float* e = reinterpret_cast<const float*>(ui);
    uint32_t* o = out + i * words_out(fn);
    if (fn == 50) {
        put_f3(o, hgd::sample_sky(kp, hgd::mk(e[0], e[1], e[2]), int(ui[3])));
    } else if (fn == 51) {
        kp.default_mip = int32_t(ui[0]);
        o[0] = uint32_t(hgd::sky_level(kp, e[1]));
    } else if (fn == 52) {
        put_f3(o, hgd::lambert(hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5])));
    } else if (fn == 53) {
        put_f3(o, hgd::reflect(hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5])));
    } else if (fn == 54) {
        o[0] = __float_as_uint(hgd::schlick_adjusted(e[0], e[1], hgd::mk(e[2], e[3], e[4]), hgd::mk(e[5], e[6], e[7]),
                                                     e[8], e[9]));
    } else if (fn == 55) {
        bool tir = false;
        put_f3(o, hgd::refract_tir(hgd::mk(e[0], e[1], e[2]), hgd::mk(e[3], e[4], e[5]), e[6], e[7], tir));
        o[3] = tir ? 1u : 0u;
    } else if (fn == 56) {
        hgd::MediumStack ms{uint64_t(ui[1]) | (uint64_t(ui[2]) << 32), int(ui[0])};
        for (int k = 0; k < 16; ++k) {
            const uint32_t kind = ui[3 + k] >> 30, val = ui[3 + k] & 0x3FFFFFFFu;
            if (kind == 1u) hgd::medium_push(kp, ms, val);
            else if (kind == 2u) hgd::medium_pop(kp, ms, val);
            put_stack(kp, ms, o + 9 * k);
        }
    } else if (fn == 57) {
        const hgd::Sampler smp{ui[0], ui[1], ui[2]};
        hgd::MediumStack ms{uint64_t(ui[4]) | (uint64_t(ui[5]) << 32), int(ui[3])};
        hgd::Ray ray{hgd::mk(e[6], e[7], e[8]), hgd::mk(e[9], e[10], e[11])};
        const hgd::Hit hit{e[12], e[13], hgd::mk(e[14], e[15], e[16]), hgd::mk(e[17], e[18], e[19]), ui[20]};
        const hgd::Mat mt = hgd::load_mat(kp, hit.mat);
        uint32_t bt = 0xFFFFFFFFu;
        put_f3(o, hgd::evaluate_hit(kp, smp, ms, ray, hit, mt, bt));
        put_f3(o + 3, ray.o);
        put_f3(o + 6, ray.d);
        o[9] = bt;
        put_stack(kp, ms, o + 10);
    } else if (fn == 58) {
        o[0] = __float_as_uint(hgd::inv_blackman_harris(e[0]));
    }
}

// the elements' stacks and material indices stay inside the table (fn 56, 57)
bool elements_in_range(int fn, const uint32_t* in, int64_t n, uint32_t n_materials) {
    const uint32_t wi = words_in(fn), at = fn == 56 ? 0u : 3u;  // (sp, lo, hi) at word `at`
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t* e = in + i * wi;
        const uint32_t sp = e[at];
        if (sp > 8u) return false;
        const uint64_t s = uint64_t(e[at + 1]) | (uint64_t(e[at + 2]) << 32);
        for (uint32_t k = 0; k < sp; ++k)
            if (((s >> (8 * k)) & 0xFFu) >= n_materials) return false;
        if (fn == 56) {
            for (int k = 0; k < 16; ++k)
                if ((e[3 + k] >> 30) == 1u && (e[3 + k] & 0x3FFFFFFFu) >= n_materials) return false;
                else if ((e[3 + k] >> 30) == 3u) return false;
        } else if (e[20] >= n_materials) {
            return false;
        }
    }
    return true;
}

int run_probe(int fn, const void* in, size_t in_bytes, void* out, size_t out_bytes, int64_t n,
              const PackedHalogenMaterial* materials, int32_t n_materials, const float* cube_texels,
              size_t n_cube_floats, int32_t cube_face_size, int32_t cube_mips) {
    const size_t wi = words_in(fn), wo = words_out(fn);
    if (wi == 0 || wo == 0 || n < 0 || (n > 0 && (!in || !out))) return int(hipErrorInvalidValue);
    if (n > (int64_t(1) << 28)) return int(hipErrorInvalidValue);  // the grid below stays far inside 2^31 workgroups
    const size_t nb_in = size_t(n) * wi * 4, nb_out = size_t(n) * wo * 4;
    if (in_bytes < nb_in || out_bytes < nb_out) return int(hipErrorInvalidValue);
    HgKernelParams kp = {};
    std::vector<float4> mat(size_t(kProbeMaterials) * 5, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    if (needs_materials(fn)) {
        if (!materials || n_materials < 1 || n_materials >= kProbeMaterials) return int(hipErrorInvalidValue);
        HgSceneIn scene = {};
        scene.materials = materials;
        scene.n_materials = n_materials;
        HgScenePack pack;
        HgPackError err;
        if (hg_pack_spheres_materials(scene, pack, err) != HG_OK) return int(hipErrorInvalidValue);
        std::copy(pack.mat.begin(), pack.mat.end(), mat.begin());
        if (!elements_in_range(fn, static_cast<const uint32_t*>(in), n, uint32_t(n_materials)))
            return int(hipErrorInvalidValue);
    }
    if (needs_cube(fn)) {
        if (!cube_texels || cube_face_size <= 0 || cube_mips <= 0 || cube_mips > HG_MAX_CUBE_MIPS)
            return int(hipErrorInvalidValue);
        if (hg_cube_mip_offsets(cube_face_size, cube_mips, kp.cube_mip_offset) != n_cube_floats)
            return int(hipErrorInvalidValue);
        kp.use_cube = 1;
        kp.cube_size = cube_face_size;
        kp.cube_mips = cube_mips;
    }
    if (n == 0) return int(hipSuccess);
    uint32_t *d_in = nullptr, *d_out = nullptr;
    float4 *d_mat = nullptr, *d_cube = nullptr;
    hipError_t rc = hipMalloc(&d_in, nb_in);
    if (rc == hipSuccess) rc = hipMalloc(&d_out, nb_out);
    if (rc == hipSuccess) rc = hipMemcpy(d_in, in, nb_in, hipMemcpyHostToDevice);
    if (rc == hipSuccess && needs_materials(fn)) {
        rc = hipMalloc(&d_mat, mat.size() * sizeof(float4));
        if (rc == hipSuccess) rc = hipMemcpy(d_mat, mat.data(), mat.size() * sizeof(float4), hipMemcpyHostToDevice);
        kp.materials = d_mat;
    }
    if (rc == hipSuccess && needs_cube(fn)) {
        rc = hipMalloc(&d_cube, n_cube_floats * sizeof(float));
        if (rc == hipSuccess) rc = hipMemcpy(d_cube, cube_texels, n_cube_floats * sizeof(float), hipMemcpyHostToDevice);
        kp.cube = d_cube;
    }
    if (rc == hipSuccess) {
        const unsigned groups = unsigned((n + 255) / 256);  // whole workgroups; the kernels check i < n
        if (fn >= 50)
            hipLaunchKernelGGL(hg_devprobe_shading_kernel, dim3(groups), dim3(256), 0, 0, fn, kp, d_in, d_out, n);
        else
            hipLaunchKernelGGL(hg_devprobe_kernel, dim3(groups), dim3(256), 0, 0, fn, d_in, d_out, n);
        rc = hipGetLastError();
    }
    if (rc == hipSuccess) rc = hipDeviceSynchronize();
    if (rc == hipSuccess) rc = hipMemcpy(out, d_out, nb_out, hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (d_mat) (void)hipFree(d_mat);
    if (d_cube) (void)hipFree(d_cube);
    return int(rc);
}

}  // namespace

extern "C" int hg_devprobe(int fn, const void* in, size_t in_bytes, void* out, size_t out_bytes, int64_t n) {
    if (needs_cube(fn) || needs_materials(fn)) return int(hipErrorInvalidValue);
    return run_probe(fn, in, in_bytes, out, out_bytes, n, nullptr, 0, nullptr, 0, 0, 0);
}

extern "C" int hg_devprobe_tables(int fn, const void* in, size_t in_bytes, void* out, size_t out_bytes, int64_t n,
                                  const PackedHalogenMaterial* materials, int32_t n_materials, const float* cube_texels,
                                  size_t n_cube_floats, int32_t cube_face_size, int32_t cube_mips) {
    return run_probe(fn, in, in_bytes, out, out_bytes, n, materials, n_materials, cube_texels, n_cube_floats,
                     cube_face_size, cube_mips);
}
