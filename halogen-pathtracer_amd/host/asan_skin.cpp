// asan_skin.cpp — the host side of a deform from vertices under AddressSanitizer + UBSan (make asan_skin;
// tests/test_skin.py): the skinning twin hg_skin_vertices (hg_host_mesh.cpp) and the checks hg_set_mesh_vertices and
// hg_set_mesh_skin make of the caller's lists before anything is bound (csrc/hg_skin.h), on random and edge input.
// Arrays are sized exactly, so a read or write past either end is an error here.  Whatever the input, every call must
// return a code, and a refused call must have written nothing.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "expect.h"
#include "halogen_abi.h"
#include "hg_skin.h"

int main() {
    std::mt19937 rng(2468);
    std::uniform_real_distribution<float> unit(-1.0f, 1.0f), weight(0.0f, 1.5f);
    for (int round = 0; round < 8; ++round) {
        const int nv = round == 0 ? 1 : round == 1 ? 255 : 257 + 613 * round;
        const int nb = round == 0 ? 1 : round == 1 ? 4 : round == 2 ? 65536 : 3 + 40 * round;
        std::uniform_int_distribution<int> bone(0, nb - 1);
        std::vector<float> P(size_t(nv) * 3), N(size_t(nv) * 3), W(size_t(nv) * 4), B(size_t(nb) * 12);
        std::vector<uint16_t> I(size_t(nv) * 4);
        for (float& x : P) x = 10.0f * unit(rng);
        for (float& x : N) x = unit(rng);
        for (float& x : W) x = weight(rng);
        for (float& x : B) x = 2.0f * unit(rng);
        for (uint16_t& i : I) i = uint16_t(bone(rng));
        // edges: a zero normal, zero and denormal weights, one bone four times, the last bone, a large translation
        N[0] = N[1] = N[2] = 0.0f;
        W[0] = 0.0f;
        W[1] = 1e-41f;
        I[0] = I[1] = I[2] = I[3] = uint16_t(nb - 1);
        B[size_t(nb - 1) * 12 + 3] = 1e6f;
        std::vector<float> oP(P.size(), -7.0f), oN(N.size(), -7.0f);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), W.data(), nv, B.data(), nb, oP.data(), oN.data()) == HG_OK);
        for (float x : oP) EXPECT(std::isfinite(x));
        for (int v = 0; v < nv; ++v) {
            const float* n = &oN[size_t(v) * 3];
            const float d = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
            EXPECT(d == 0.0f || std::fabs(d - 1.0f) < 1e-5f);
        }
        EXPECT(oN[0] == 0.0f && oN[1] == 0.0f && oN[2] == 0.0f);  // the zero normal stays
        // one vertex through the shared function directly: the same bits as the array form
        float p1[3], n1[3];
        const int last = nv - 1;
        hg_skin_vertex(B.data(), &I[size_t(last) * 4], &W[size_t(last) * 4], &P[size_t(last) * 3], &N[size_t(last) * 3], p1, n1);
        EXPECT(!std::memcmp(p1, &oP[size_t(last) * 3], 12) && !std::memcmp(n1, &oN[size_t(last) * 3], 12));
        // refusals: nothing written
        std::vector<float> keepP = oP, keepN = oN;
        std::vector<uint16_t> bad = I;
        bad[size_t(rng() % uint32_t(nv)) * 4 + rng() % 4] = uint16_t(nb);  // (65536 bones: wraps to 0, a valid index)
        const int want = nb == 65536 ? HG_OK : HG_E_INVALID;
        EXPECT(hg_skin_vertices(P.data(), N.data(), bad.data(), W.data(), nv, B.data(), nb, oP.data(), oN.data()) == want);
        if (want != HG_OK) EXPECT(oP == keepP && oN == keepN);
        keepP = oP;
        keepN = oN;
        EXPECT(hg_skin_first_bad_bone(I.data(), nv, nb) == -1);
        if (nb < 65536) EXPECT(hg_skin_first_bad_bone(bad.data(), nv, nb) >= 0);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), W.data(), 0, B.data(), nb, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), W.data(), -1, B.data(), nb, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), W.data(), nv, B.data(), 0, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), W.data(), nv, B.data(), 65537, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(nullptr, N.data(), I.data(), W.data(), nv, B.data(), nb, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), nullptr, I.data(), W.data(), nv, B.data(), nb, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), N.data(), nullptr, W.data(), nv, B.data(), nb, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), nullptr, nv, B.data(), nb, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), W.data(), nv, nullptr, nb, oP.data(), oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), W.data(), nv, B.data(), nb, nullptr, oN.data()) == HG_E_INVALID);
        EXPECT(hg_skin_vertices(P.data(), N.data(), I.data(), W.data(), nv, B.data(), nb, oP.data(), nullptr) == HG_E_INVALID);
        EXPECT(oP == keepP && oN == keepN);

        // the index list of a binding: a valid list passes, every kind of bad index is found where it is
        const int nt = 2 * nv + 1;
        std::uniform_int_distribution<int32_t> vert(0, nv - 1);
        std::vector<int32_t> idx(size_t(nt) * 3);
        for (int32_t& i : idx) i = vert(rng);
        idx[0] = idx[1] = idx[2] = nv - 1;  // a triangle naming the last vertex three times
        EXPECT(hg_skin_first_bad_index(idx.data(), nt, nv) == -1);
        EXPECT(hg_skin_first_bad_index(idx.data(), 0, nv) == -1);
        const int32_t wrong[4] = {nv, -1, INT32_MAX, INT32_MIN};
        for (int32_t w : wrong) {
            std::vector<int32_t> b2 = idx;
            const size_t at = rng() % b2.size();
            b2[at] = w;
            EXPECT(hg_skin_first_bad_index(b2.data(), nt, nv) == int64_t(at));
        }
    }
    if (failures) return 1;
    std::printf("asan_skin ok\n");
    return 0;
}
