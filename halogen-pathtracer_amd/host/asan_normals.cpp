// asan_normals.cpp — the host side of recomputed vertex normals under AddressSanitizer + UBSan (make asan_normals;
// tests/test_normals.py): the adjacency builder and the arithmetic of csrc/hg_normals.h and the twin hg_vertex_normals
// (hg_host_mesh.cpp), on random and adversarial index lists.  Arrays are sized exactly: a read or write past either end
// is an error here.  Whatever the input, every call must return a code, and a refused call must have written nothing.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "expect.h"
#include "halogen_abi.h"
#include "hg_normals.h"

// The adjacency of `idx` is what the header promises: every corner once, under its vertex, in triple order
static void check_adjacency(const std::vector<int32_t>& idx, int nt, int nv) {
    std::vector<int32_t> offsets(size_t(nv) + 1, -7), faces(size_t(nt) * 3, -7);
    hg_normals_build_adjacency(idx.data(), nt, nv, offsets.data(), faces.data());
    EXPECT(offsets[0] == 0 && offsets[size_t(nv)] == 3 * nt);
    std::vector<int> seen(size_t(nt), 0);
    for (int v = 0; v < nv; ++v) {
        EXPECT(offsets[size_t(v)] <= offsets[size_t(v) + 1]);
        for (int32_t j = offsets[size_t(v)]; j < offsets[size_t(v) + 1]; ++j) {
            const int32_t f = faces[size_t(j)];
            EXPECT(f >= 0 && f < nt);
            if (f < 0 || f >= nt) return;
            const int32_t* t = &idx[size_t(f) * 3];
            EXPECT(t[0] == v || t[1] == v || t[2] == v);
            seen[size_t(f)]++;
            if (j > offsets[size_t(v)]) {
                const int32_t* p = &idx[size_t(faces[size_t(j) - 1]) * 3];
                EXPECT(std::lexicographical_compare(p, p + 3, t, t + 3) || std::equal(p, p + 3, t));
            }
        }
    }
    for (int s : seen) EXPECT(s == 3);
}

static void check_twin(const std::vector<float>& P, const std::vector<int32_t>& idx, int nt, int nv, std::mt19937& rng) {
    std::vector<float> N(size_t(nv) * 3, -7.0f);
    EXPECT(hg_vertex_normals(P.data(), nv, idx.data(), nt, N.data()) == HG_OK);
    for (int v = 0; v < nv; ++v) {
        const float* n = &N[size_t(v) * 3];
        const float d = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        EXPECT(d == 0.0f || std::fabs(d - 1.0f) < 1e-5f);
    }
    // any order of the triangles: the same bits
    std::vector<int> perm(size_t(nt), 0);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<int32_t> shuffled(idx.size());
    for (int t = 0; t < nt; ++t) std::memcpy(&shuffled[size_t(t) * 3], &idx[size_t(perm[size_t(t)]) * 3], 12);
    std::vector<float> N2(N.size(), -7.0f);
    EXPECT(hg_vertex_normals(P.data(), nv, shuffled.data(), nt, N2.data()) == HG_OK);
    EXPECT(!std::memcmp(N.data(), N2.data(), N.size() * sizeof(float)));
    // refusals: nothing written
    const std::vector<float> keep = N;
    EXPECT(hg_vertex_normals(nullptr, nv, idx.data(), nt, N.data()) == HG_E_INVALID);
    EXPECT(hg_vertex_normals(P.data(), nv, nullptr, nt, N.data()) == HG_E_INVALID);
    EXPECT(hg_vertex_normals(P.data(), nv, idx.data(), nt, nullptr) == HG_E_INVALID);
    EXPECT(hg_vertex_normals(P.data(), 0, idx.data(), nt, N.data()) == HG_E_INVALID);
    EXPECT(hg_vertex_normals(P.data(), -1, idx.data(), nt, N.data()) == HG_E_INVALID);
    EXPECT(hg_vertex_normals(P.data(), nv, idx.data(), 0, N.data()) == HG_E_INVALID);
    EXPECT(hg_vertex_normals(P.data(), nv, idx.data(), -1, N.data()) == HG_E_INVALID);
    EXPECT(hg_vertex_normals(P.data(), nv, idx.data(), INT32_MAX, N.data()) == HG_E_INVALID);  // (refused by the count)
    const int32_t wrong[4] = {nv, -1, INT32_MAX, INT32_MIN};
    for (int32_t w : wrong) {
        std::vector<int32_t> bad = idx;
        bad[rng() % bad.size()] = w;
        EXPECT(hg_vertex_normals(P.data(), nv, bad.data(), nt, N.data()) == HG_E_INVALID);
    }
    EXPECT(N == keep);
}

int main() {
    std::mt19937 rng(1357);
    std::uniform_real_distribution<float> unit(-1.0f, 1.0f);
    for (int round = 0; round < 8; ++round) {
        const int nv = round == 0 ? 1 : round == 1 ? 3 : round == 2 ? 255 : 257 + 613 * round;
        const int nt = round == 0 ? 1 : round == 1 ? 1 : 2 * nv + 1;
        std::vector<float> P(size_t(nv) * 3);
        for (float& x : P) x = 10.0f * unit(rng);
        std::uniform_int_distribution<int32_t> vert(0, nv - 1);
        std::vector<int32_t> idx(size_t(nt) * 3);
        for (int32_t& i : idx) i = vert(rng);
        if (round == 1) idx = {0, 1, 2};  // a single triangle
        if (round >= 2) {
            idx[0] = idx[1] = idx[2] = nv - 1;                       // a triangle naming the last vertex three times
            std::memcpy(&idx[3], &idx[6], 12);                        // a duplicated triangle
            std::memcpy(&idx[size_t(nt - 1) * 3], &idx[6], 12);       // ... and again at the end
            idx[9] = idx[10];                                         // a zero-area triangle
        }
        check_adjacency(idx, nt, nv);
        check_twin(P, idx, nt, nv, rng);
        // all corners on one vertex
        std::vector<int32_t> one(size_t(nt) * 3, nv / 2);
        check_adjacency(one, nt, nv);
        check_twin(P, one, nt, nv, rng);
        std::vector<float> N(size_t(nv) * 3, -7.0f);
        EXPECT(hg_vertex_normals(P.data(), nv, one.data(), nt, N.data()) == HG_OK);
        for (float x : N) EXPECT(x == 0.0f);
        // a fan round vertex 0: one long list, the others short
        if (nv >= 3) {
            std::vector<int32_t> fan(size_t(nv - 2) * 3);
            for (int t = 0; t < nv - 2; ++t) {
                fan[size_t(t) * 3] = 0;
                fan[size_t(t) * 3 + 1] = t + 1;
                fan[size_t(t) * 3 + 2] = t + 2;
            }
            check_adjacency(fan, nv - 2, nv);
            check_twin(P, fan, nv - 2, nv, rng);
        }
    }
    // the shared arithmetic directly: a right triangle in the xy plane has the normal (0, 0, area * 2)
    const float a[3] = {0, 0, 0}, b[3] = {2, 0, 0}, c[3] = {0, 3, 0};
    float f[3];
    hg_face_normal(a, b, c, f);
    EXPECT(f[0] == 0.0f && f[1] == 0.0f && f[2] == 6.0f);
    const int32_t faces[2] = {0, 0};
    float n[3];
    hg_vertex_normal(f, faces, 0, 2, n);
    EXPECT(n[0] == 0.0f && n[1] == 0.0f && n[2] == 1.0f);
    hg_vertex_normal(f, faces, 1, 1, n);  // an empty list
    EXPECT(n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f);
    if (failures) return 1;
    std::printf("asan_normals ok\n");
    return 0;
}
