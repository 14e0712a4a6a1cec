// hg_skin.h — linear-blend skinning of one vertex (hg_skin_vertices, hg_skin_mesh, hg_skin_mesh_device;
// include/halogen_abi.h) and the host-side checks of a vertex binding, one definition for the device kernel
// (hg_deform.hip) and the host twin (hg_host_mesh.cpp).  Not in the reference.
//
// The contract, in the order the arithmetic is done (fp32, no contraction: both sides build with -ffp-contract=off):
//   bone        12 floats, a row-major 3 x 4 matrix: rows of (x y z t).
//   blend       per element M = ((w0 * B0 + w1 * B1) + w2 * B2) + w3 * B3, B_k the bone the vertex's k-th index names.
//               The weights are used as given: no renormalisation, and a zero weight is still multiplied.
//   position    p'[r] = ((M[r][0] * x + M[r][1] * y) + M[r][2] * z) + M[r][3]
//   normal      n'[r] = (M[r][0] * nx + M[r][1] * ny) + M[r][2] * nz: the 3 x 3 block itself, not its inverse transpose,
//               which is right for rigid and uniformly scaled bones: what real-time skinning does.  Then
//               d = (n'[0] * n'[0] + n'[1] * n'[1]) + n'[2] * n'[2]; if d > 0, n' *= hg_rnorm(d); otherwise n' stays.
// Inputs and results are assumed finite (NaN payloads are outside the contract); bone indices are checked where they are
// bound (hg_skin_first_bad_bone), never here.
#pragma once
#include <stdint.h>

#include "hg_fmath.h"

#define HG_SKIN_BONE_FLOATS 12
#define HG_SKIN_INFLUENCES 4

// bones: the palette; idx, w: the vertex's four bone indices and weights; p, n: its rest position and normal
HG_FN void hg_skin_vertex(const float* bones, const uint16_t idx[4], const float w[4], const float p[3], const float n[3],
                          float out_p[3], float out_n[3]) {
    const float* b0 = bones + uint32_t(idx[0]) * HG_SKIN_BONE_FLOATS;
    const float* b1 = bones + uint32_t(idx[1]) * HG_SKIN_BONE_FLOATS;
    const float* b2 = bones + uint32_t(idx[2]) * HG_SKIN_BONE_FLOATS;
    const float* b3 = bones + uint32_t(idx[3]) * HG_SKIN_BONE_FLOATS;
    float m[HG_SKIN_BONE_FLOATS];
    for (int e = 0; e < HG_SKIN_BONE_FLOATS; ++e) m[e] = ((w[0] * b0[e] + w[1] * b1[e]) + w[2] * b2[e]) + w[3] * b3[e];
    for (int r = 0; r < 3; ++r) {
        const float* q = m + 4 * r;
        out_p[r] = ((q[0] * p[0] + q[1] * p[1]) + q[2] * p[2]) + q[3];
        out_n[r] = (q[0] * n[0] + q[1] * n[1]) + q[2] * n[2];
    }
    const float d = (out_n[0] * out_n[0] + out_n[1] * out_n[1]) + out_n[2] * out_n[2];
    if (d > 0.0f) {
        const float s = hg_rnorm(d);
        out_n[0] *= s;
        out_n[1] *= s;
        out_n[2] *= s;
    }
}

// What hg_set_mesh_vertices checks of the caller's index list before anything is bound: the position (in 0 .. 3 *
// n_triangles) of the first index outside [0, n_vertices), or -1
static inline int64_t hg_skin_first_bad_index(const int32_t* indices, int64_t n_triangles, int32_t n_vertices) {
    for (int64_t i = 0; i < 3 * n_triangles; ++i)
        if (indices[i] < 0 || indices[i] >= n_vertices) return i;
    return -1;
}

// What hg_set_mesh_skin and hg_skin_vertices check: the position (in 0 .. 4 * n_vertices) of the first bone index that
// is not below n_bones, or -1
static inline int64_t hg_skin_first_bad_bone(const uint16_t* bone_indices, int64_t n_vertices, int32_t n_bones) {
    for (int64_t i = 0; i < HG_SKIN_INFLUENCES * n_vertices; ++i)
        if (int32_t(bone_indices[i]) >= n_bones) return i;
    return -1;
}
