// hg_host_denoise.cpp — hg_denoise_host: the host twin of hg_readback_begin_denoised's filter (product code; no
// device work).  The arithmetic is hg_atrous.h's, the same functions the device kernels compile; every pixel is
// computed sequentially by one thread, so the row split below changes no bit.  Compiled with -ffp-contract=off.
#include <cstdint>
#include <cstring>
#include <vector>

#include "halogen_abi.h"
#include "hg_atrous.h"
#include "hg_host_pool.h"

extern "C" int hg_denoise_host(const float* rgba, const float* guide0, const float* guide1, int32_t width,
                               int32_t height, const hg_denoise_params* p, float* out_rgba) {
    if (!rgba || !guide0 || !guide1 || !p || !out_rgba) return HG_E_INVALID;
    if (width <= 0 || height <= 0 || int64_t(width) * height > (int64_t(1) << 31)) return HG_E_INVALID;
    if (!hg_atrous_params_ok(*p)) return HG_E_INVALID;
    const size_t W = size_t(width), pixels = W * size_t(height);
    std::vector<float> work[2] = {std::vector<float>(pixels * 4), std::vector<float>(pixels * 4)};
    HgHostPool& pool = HgHostPool::get();
    pool.run(size_t(height), [&](size_t y) {  // the untile's place: the colour, demodulated
        for (size_t i = y * W; i < (y + 1) * W; ++i) {
            float c[4] = {rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]};
            if (p->demodulate) hg_atrous_demodulate(c, guide1 + 4 * i);
            std::memcpy(&work[0][4 * i], c, sizeof c);
        }
    });
    int at = 0;
    for (int32_t it_i = 0; it_i < p->iterations; ++it_i, at ^= 1) {
        const HgAtrousIter it = hg_atrous_iter(*p, it_i);
        const bool remod = p->demodulate && it_i == p->iterations - 1;
        const float* src = work[at].data();
        float* dst = work[at ^ 1].data();
        pool.run(size_t(height), [&](size_t y) {
            for (int32_t x = 0; x < width; ++x) {
                float out[4];
                hg_atrous_pixel(it, width, height, x, int32_t(y),
                                [&](int32_t qx, int32_t qy, float c[3], float g[4]) {
                                    const size_t q = size_t(qy) * W + size_t(qx);
                                    std::memcpy(c, src + 4 * q, 3 * sizeof(float));
                                    std::memcpy(g, guide0 + 4 * q, 4 * sizeof(float));
                                },
                                out);
                const size_t i = y * W + size_t(x);
                out[3] = src[4 * i + 3];
                if (remod) hg_atrous_remodulate(out, guide1 + 4 * i);
                std::memcpy(dst + 4 * i, out, sizeof out);
            }
        });
    }
    std::memcpy(out_rgba, work[at].data(), pixels * 4 * sizeof(float));
    return HG_OK;
}
