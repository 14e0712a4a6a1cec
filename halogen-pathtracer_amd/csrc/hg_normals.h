// hg_normals.h — area-weighted vertex normals of a mesh from its positions and its index list (hg_vertex_normals,
// HG_DEFORM_NORMALS; include/halogen_abi.h), one definition for the two device kernels (hg_deform.hip) and the host
// twin (hg_host_mesh.cpp), and the host-side builder of the inverted index both sum through.  No HIP in it.  Not in the
// reference.
//
// The contract, in the order the arithmetic is done (fp32, no contraction: both sides build with -ffp-contract=off):
//   face normal    of a triangle whose corners name the vertices a, b, c: e1 = b - a, e2 = c - a,
//                  f = (e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x): two products
//                  and one subtraction per component.  Unnormalised: the sum below weights a face by its area.
//   vertex normal  of vertex v: s = +0; s += f(t) once for every corner of every triangle that names v (a triangle that
//                  names v twice is added twice), the corners taken in ascending order of the triangle's index triple
//                  (i0, i1, i2) as listed.  Ties have identical triples and hence identical f: their order cannot
//                  matter.  d = (s.x * s.x + s.y * s.y) + s.z * s.z; if d > 0, n = s * hg_rnorm(d); otherwise
//                  n = (0, 0, 0): an unreferenced vertex, a vertex with only zero-area faces, a sum that cancels.
// The order by triple makes the result a function of the positions and of the SET of triangles: a rebuild permutes the
// list on the host and on the device, and a sum in list order would leave the two a last bit apart afterwards.
// The sum goes through an inverted index (the adjacency): offsets[n_vertices + 1] and faces[3 * n_triangles], the face
// ids of vertex v at faces[offsets[v] .. offsets[v + 1]) in the order above.  Built once per index list, on the host.
// Positions are assumed finite (NaN payloads are outside the contract); indices are checked where they are bound
// (hg_skin_first_bad_index), never here.  Angle weighting is out of scope: it needs acos of a quotient of rounded
// lengths, and the lists of one vertex are never split (that would change the order of the sum).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "hg_fmath.h"

// The most triangles an adjacency is built for: 3 * n_triangles corners must fit the int32 offsets
#define HG_NORMALS_MAX_TRIANGLES (INT32_MAX / 3)

// a, b, c: the positions of the triangle's three corners
HG_FN void hg_face_normal(const float a[3], const float b[3], const float c[3], float f[3]) {
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    f[0] = e1y * e2z - e1z * e2y;
    f[1] = e1z * e2x - e1x * e2z;
    f[2] = e1x * e2y - e1y * e2x;
}

// The normal of the vertex whose face ids are faces[begin .. end), from the face normals (3 floats a face)
HG_FN void hg_vertex_normal(const float* face_normals, const int32_t* faces, int32_t begin, int32_t end, float n[3]) {
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int32_t j = begin; j < end; ++j) {
        const float* f = face_normals + (size_t)(uint32_t)faces[j] * 3;
        sx += f[0];
        sy += f[1];
        sz += f[2];
    }
    const float d = (sx * sx + sy * sy) + sz * sz;
    if (d > 0.0f) {
        const float r = hg_rnorm(d);
        n[0] = sx * r;
        n[1] = sy * r;
        n[2] = sz * r;
    } else {
        n[0] = n[1] = n[2] = 0.0f;
    }
}

// The adjacency of an index list whose every index is in [0, n_vertices) and whose n_triangles is at most
// HG_NORMALS_MAX_TRIANGLES: a counting sort of the corners by vertex, then each vertex's range sorted by the triple of
// its triangle (equal triples by face id, so the arrays themselves are a function of the list).
// offsets: n_vertices + 1; faces: 3 * n_triangles.
static inline void hg_normals_build_adjacency(const int32_t* indices, int32_t n_triangles, int32_t n_vertices,
                                              int32_t* offsets, int32_t* faces) {
    for (int64_t v = 0; v <= n_vertices; ++v) offsets[v] = 0;
    const int64_t n_corners = 3 * (int64_t)n_triangles;
    for (int64_t i = 0; i < n_corners; ++i) offsets[(int64_t)indices[i] + 1]++;
    for (int64_t v = 0; v < n_vertices; ++v) offsets[v + 1] += offsets[v];
    // (fill from the front: offsets[v] is moved to its range's end and put back below)
    for (int64_t i = 0; i < n_corners; ++i) faces[offsets[indices[i]]++] = (int32_t)(i / 3);
    for (int64_t v = n_vertices; v > 0; --v) offsets[v] = offsets[v - 1];
    offsets[0] = 0;
    for (int64_t v = 0; v < n_vertices; ++v) {
        if (offsets[v + 1] - offsets[v] < 2) continue;
        std::sort(faces + offsets[v], faces + offsets[v + 1], [indices](int32_t x, int32_t y) {
            const int32_t* p = indices + (int64_t)x * 3;
            const int32_t* q = indices + (int64_t)y * 3;
            if (p[0] != q[0]) return p[0] < q[0];
            if (p[1] != q[1]) return p[1] < q[1];
            if (p[2] != q[2]) return p[2] < q[2];
            return x < y;
        });
    }
}
