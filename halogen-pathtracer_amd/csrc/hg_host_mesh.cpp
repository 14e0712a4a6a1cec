// hg_host_mesh.cpp — a mesh's data on the host (product code): the triangle list the reference packs in C#
//   RayTracingMesh.UpdateTriangleList   Assets/Scripts/RayTracingMesh.cs:70-87   -> hg_pack_triangles
// and the host twins of the device's mesh updates (hg_deform.hip, hg_refit.hip): skinning, vertex normals, refit.  The
// twins compile the arithmetic of the contracts (hg_skin.h, hg_normals.h, hg_refit.h) the device kernels compile.
// Compiled with -ffp-contract=off.
#include <cstdint>
#include <utility>
#include <vector>

#include "halogen_abi.h"
#include "hg_normals.h"
#include "hg_refit.h"
#include "hg_skin.h"

extern "C" int hg_pack_triangles(const float* V, const float* N, int32_t n_vertices, const int32_t* idx,
                                 int32_t n_tris, HalogenTriangle* out) {
    if (!V || !N || !idx || !out || n_tris < 0) return HG_E_INVALID;
    for (int64_t t = 0; t < n_tris; ++t) {
        int32_t i0 = idx[3 * t], i1 = idx[3 * t + 1], i2 = idx[3 * t + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices)
            return HG_E_INVALID;
        HalogenTriangle& h = out[t];
        h.pointA = {V[3 * i0], V[3 * i0 + 1], V[3 * i0 + 2]};
        h.pointB = {V[3 * i1], V[3 * i1 + 1], V[3 * i1 + 2]};
        h.pointC = {V[3 * i2], V[3 * i2 + 1], V[3 * i2 + 2]};
        h.normalA = {N[3 * i0], N[3 * i0 + 1], N[3 * i0 + 2]};
        h.normalB = {N[3 * i1], N[3 * i1 + 1], N[3 * i1 + 2]};
        h.normalC = {N[3 * i2], N[3 * i2 + 1], N[3 * i2 + 2]};
    }
    return HG_OK;
}

// hg_skin_vertices: the host twin of the device skin kernel (hg_deform.hip), over the contract of hg_skin.h.  Everything
// is validated before the first vertex is written.
extern "C" int hg_skin_vertices(const float* rest_positions, const float* rest_normals, const uint16_t* bone_indices,
                                const float* weights, int32_t n_vertices, const float* bones, int32_t n_bones,
                                float* out_positions, float* out_normals) {
    if (!rest_positions || !rest_normals || !bone_indices || !weights || !bones || !out_positions || !out_normals)
        return HG_E_INVALID;
    if (n_vertices <= 0 || n_bones < 1 || n_bones > 65536) return HG_E_INVALID;
    if (hg_skin_first_bad_bone(bone_indices, n_vertices, n_bones) >= 0) return HG_E_INVALID;
    for (int64_t v = 0; v < n_vertices; ++v)
        hg_skin_vertex(bones, bone_indices + 4 * v, weights + 4 * v, rest_positions + 3 * v, rest_normals + 3 * v,
                       out_positions + 3 * v, out_normals + 3 * v);
    return HG_OK;
}

// hg_vertex_normals: the host twin of a deform with HG_DEFORM_NORMALS (hg_deform.hip), over the contract of
// hg_normals.h: the adjacency, every face's normal, every vertex's sum through the adjacency.  Everything is validated
// before the first normal is written.
extern "C" int hg_vertex_normals(const float* positions, int32_t n_vertices, const int32_t* indices, int32_t n_triangles,
                                 float* out_normals) {
    if (!positions || !indices || !out_normals) return HG_E_INVALID;
    if (n_vertices < 1 || n_triangles < 1 || n_triangles > HG_NORMALS_MAX_TRIANGLES) return HG_E_INVALID;
    if (hg_skin_first_bad_index(indices, n_triangles, n_vertices) >= 0) return HG_E_INVALID;
    std::vector<int32_t> offsets(size_t(n_vertices) + 1), faces(size_t(n_triangles) * 3);
    hg_normals_build_adjacency(indices, n_triangles, n_vertices, offsets.data(), faces.data());
    std::vector<float> face_normals(size_t(n_triangles) * 3);
    for (int64_t t = 0; t < n_triangles; ++t)
        hg_face_normal(positions + size_t(indices[3 * t]) * 3, positions + size_t(indices[3 * t + 1]) * 3,
                       positions + size_t(indices[3 * t + 2]) * 3, face_normals.data() + 3 * t);
    for (int64_t v = 0; v < n_vertices; ++v)
        hg_vertex_normal(face_normals.data(), faces.data(), offsets[size_t(v)], offsets[size_t(v) + 1], out_normals + 3 * v);
    return HG_OK;
}

// hg_refit_blas: the host twin of the device refit (hg_refit.hip), over the contract of hg_refit.h.  Bottom-up from the
// root (entry 0): a leaf's raw box from its triangles, an inner entry's the union of its children's; then every reached
// entry's stored box (the root's without the pad).  Everything is validated before the first box is written: ranges,
// depth (as hg_upload_scene accepts it) and cycles.  Entries reached along two paths are computed once.
extern "C" int hg_refit_blas(const HalogenTriangle* tris, int32_t n_tris, BVHEntry* nodes, int32_t n_nodes) {
    if (!nodes || n_nodes <= 0 || n_tris < 0 || (n_tris && !tris)) return HG_E_INVALID;
    enum : uint8_t { kNew = 0, kOpen = 1, kDone = 2 };
    std::vector<uint8_t> state(size_t(n_nodes), kNew);
    std::vector<HgRawBox> raw;
    raw.resize(size_t(n_nodes));
    std::vector<std::pair<uint32_t, uint32_t>> stack{{0u, 0u}};  // (entry, depth)
    while (!stack.empty()) {
        const auto [g, depth] = stack.back();
        const BVHEntry& e = nodes[g];
        if (state[g] == kNew) {
            if (depth > HG_REFIT_MAX_DEPTH) return HG_E_UNSUPPORTED;  // deeper than the traversal's stack, or cyclic
            if (e.triangleCount > 0) {
                if (uint64_t(e.indexA) + e.triangleCount > uint64_t(n_tris)) return HG_E_INVALID;
                HgRawBox b = hg_refit_empty();
                for (uint32_t i = 0; i < e.triangleCount; ++i) hg_refit_add_triangle(b, tris[size_t(e.indexA) + i]);
                raw[g] = b;
                state[g] = kDone;
                stack.pop_back();
                continue;
            }
            if (uint64_t(e.indexA) + 1 >= uint64_t(n_nodes)) return HG_E_INVALID;
            state[g] = kOpen;
            for (uint32_t child : {e.indexA + 1, e.indexA}) {
                if (state[child] == kOpen) return HG_E_UNSUPPORTED;  // a cycle
                if (state[child] == kNew) stack.push_back({child, depth + 1});
            }
        } else {
            stack.pop_back();
            if (state[g] != kOpen) continue;
            raw[g] = hg_refit_union(raw[e.indexA], raw[e.indexA + 1]);
            state[g] = kDone;
        }
    }
    for (int32_t g = 0; g < n_nodes; ++g) {
        if (state[size_t(g)] != kDone) continue;
        float mn[3], mx[3];
        if (g == 0 && hg_refit_root_is_current_padded(raw[0], nodes[0])) continue;  // (hg_refit.h: the root)
        hg_refit_stored(raw[size_t(g)], g != 0, mn, mx);
        nodes[g].boundingCornerA = {mn[0], mn[1], mn[2]};
        nodes[g].boundingCornerB = {mx[0], mx[1], mx[2]};
    }
    return HG_OK;
}
