// hg_display.hip — display readback (hg_readback, hg_readback_begin[_format] / _end[_data], hg_pack_display): the
// accumulator untiled on the device into a row-major image in a display format (hg_pack.h) and brought to the host,
// at once or through a ring of slots (hg_ctx::DisplaySlot, hg_slot_ring.h) that lets readbacks stay outstanding while
// the next frames render.  Stands in for the Blit to the camera target of HalogenRenderPass.cs (RP:237-508).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "hg_rt.h"
#include "hg_pack.h"

// The accumulator (this rank's tiles, tile-major) as a row-major image in a display format (hg_pack.h); pixels of
// other ranks' tiles are 0.  One thread per pixel: the stores are contiguous (16 / 8 / 4 B per pixel), the loads are 8
// consecutive float4 per tile row.  64-thread workgroups (see launch_untile).
template <int kFmt, bool kRows>
__global__ __launch_bounds__(64) void hg_untile_image(void* __restrict__ image, const float4* __restrict__ acc,
                                                       int32_t W, int32_t H, int32_t tiles_x, int32_t rank,
                                                       int32_t n_ranks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= uint32_t(W) * uint32_t(H)) return;
    float4 v;
    if constexpr (kRows) {  // the source is already a row-major image (the multi-GPU gather's assembled image)
        v = acc[i];
    } else {
        const HgPixelSource s = hg_pixel_source(i % uint32_t(W), i / uint32_t(W), uint32_t(tiles_x), uint32_t(n_ranks));
        v = s.rank == uint32_t(rank) ? acc[size_t(s.local_tile) * 64u + s.lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (kFmt == HG_DISPLAY_RGBA32F) {
        static_cast<float4*>(image)[i] = v;
    } else if constexpr (kFmt == HG_DISPLAY_RGBA16F) {
        uint32_t h[2];
        hg_pack_rgba16f(v.x, v.y, v.z, v.w, h);
        static_cast<uint2*>(image)[i] = make_uint2(h[0], h[1]);
    } else {
        static_cast<uint32_t*>(image)[i] = hg_pack_r11g11b10(v.x, v.y, v.z);
    }
}

namespace hgrt {

size_t display_bpp(int32_t format) {
    return format == HG_DISPLAY_RGBA32F ? 16 : format == HG_DISPLAY_RGBA16F ? 8 : format == HG_DISPLAY_R11G11B10F ? 4 : 0;
}

int display_check(hg_ctx* c, int32_t format) {
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (!display_bpp(format)) return fail(c, HG_E_INVALID, "unknown display format %d", format);
    if (c->rb.full())
        return fail(c, HG_E_INVALID, "%d readbacks outstanding (HG_OPT_READBACK_DEPTH): call hg_readback_end first",
                    c->rb.pending);
    return HG_OK;
}

}  // namespace hgrt

using namespace hgrt;

namespace {

// Enqueue on the context stream: `src` (the accumulator, or with kRows a row-major float4 image of the target's size)
// as a row-major image in `format` at `dst`
template <bool kRows>
int launch_untile(hg_ctx* c, void* dst, int32_t format, const float4* src) {
    // one-wave workgroups with few registers: a display readback's untile runs beside the persistent trace waves of the
    // next frames (which hold most wave slots), as the lean blend does, instead of waiting for a CU to drain
    const size_t pixels = size_t(c->W) * size_t(c->H);
    const dim3 g(uint32_t((pixels + 63) / 64)), b(64);
    if (format == HG_DISPLAY_RGBA16F)
        hipLaunchKernelGGL((hg_untile_image<HG_DISPLAY_RGBA16F, kRows>), g, b, 0, c->stream, dst, src, c->W, c->H,
                           c->tiles_x, c->rank, c->n_ranks);
    else if (format == HG_DISPLAY_R11G11B10F)
        hipLaunchKernelGGL((hg_untile_image<HG_DISPLAY_R11G11B10F, kRows>), g, b, 0, c->stream, dst, src, c->W, c->H,
                           c->tiles_x, c->rank, c->n_ranks);
    else
        hipLaunchKernelGGL((hg_untile_image<HG_DISPLAY_RGBA32F, kRows>), g, b, 0, c->stream, dst, src, c->W, c->H,
                           c->tiles_x, c->rank, c->n_ranks);
    HG_HIP(c, hipGetLastError());
    return HG_OK;
}

// A device image an untile writes, grown to `bytes`: everything that might read the old image is ordered before on the
// context stream
int ensure_image(hg_ctx* c, DevBuf& img, size_t bytes) {
    if (img.bytes >= bytes) return HG_OK;
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return ensure(c, img, bytes);
}

// The slot's pinned host image, of at least `bytes` bytes; with `mapped`, one the device can write (mapped,
// fine-grained: HG_OPT_READBACK_STREAM 2).  A mapped image serves the copy modes too.  The slot is not outstanding, so
// the last write to the image it replaces was waited for at that readback's end.
int slot_host_image(hg_ctx* c, hg_ctx::DisplaySlot& s, size_t bytes, bool mapped) {
    if (s.cap >= bytes && (s.mapped || !mapped)) return HG_OK;
    if (s.host) {
        HG_HIP(c, hipEventSynchronize(s.copied));  // (returns at once)
        HG_HIP(c, hipHostFree(s.host));
    }
    s.host = nullptr;
    s.cap = 0;
    s.mapped = false;
    const hipError_t e = hipHostMalloc(&s.host, bytes, mapped ? hipHostMallocMapped | hipHostMallocCoherent : 0);
    if (e != hipSuccess)
        return fail(c, HG_E_NOMEM, "hipHostMalloc(%zu%s) failed: %s", bytes, mapped ? ", mapped" : "", hipGetErrorString(e));
    s.cap = bytes;
    s.mapped = mapped;
    if (!s.copied) HG_HIP(c, hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    return HG_OK;
}

}  // namespace

// The display readback of hg_readback_begin_format, from the accumulator (rows == nullptr) or from a row-major float4
// image of the target's size on the context's device (the comm's assembled image, hg_comm_readback_begin).  By
// HG_OPT_READBACK_STREAM: 0 untiles into c->image and copies on the context stream; 1 untiles into the slot's own
// device image and copies on the side stream, so the context stream (the next frames' blends) does not wait for the
// copy; 2 (zero copy) untiles straight into the slot's host image, whose stores cross PCIe as they retire.
int hg_ctx_display_begin(hg_ctx* c, const void* rows, int32_t format) {
    if (int rc = hg_ctx_flush(c)) return rc;
    if (int rc = display_check(c, format)) return rc;
    if (int rc = set_device(c)) return rc;
    const int mode = c->rb_side;
    if (mode == 1 && !c->rb_stream) {
        // the copy stream on a hardware queue of its own (a plain stream shares one with a trace lane and waits behind
        // its traces: depth 2 1,285 -> 1,642 Mpaths/s, sweep_r04_rbq)
        HG_HIP(c, create_lane_stream(c, HG_TRACE_LANES, &c->rb_stream));
        for (hg_ctx::DisplaySlot& d : c->slots) HG_HIP(c, hipEventCreateWithFlags(&d.untiled, hipEventDisableTiming));
    }
    hg_ctx::DisplaySlot& s = c->slots[c->rb.next];  // not outstanding: the slot after the newest
    const size_t bytes = size_t(c->W) * size_t(c->H) * display_bpp(format);
    if (int rc = slot_host_image(c, s, bytes, mode == 2)) return rc;
    void* dst = nullptr;
    if (mode == 2) {
        HG_HIP(c, hipHostGetDevicePointer(&dst, s.host, 0));
    } else {
        DevBuf& img = mode == 1 ? s.image : c->image;
        if (int rc = ensure_image(c, img, bytes)) return rc;
        dst = img.p;
    }
    if (int rc = rows ? launch_untile<true>(c, dst, format, static_cast<const float4*>(rows))
                      : launch_untile<false>(c, dst, format, static_cast<const float4*>(c->acc.p)))
        return rc;
    if (mode == 1) {
        HG_HIP(c, hipEventRecord(s.untiled, c->stream));
        HG_HIP(c, hipStreamWaitEvent(c->rb_stream, s.untiled, 0));
        HG_HIP(c, hipMemcpyAsync(s.host, dst, bytes, hipMemcpyDeviceToHost, c->rb_stream));
        HG_HIP(c, hipEventRecord(s.copied, c->rb_stream));
    } else {
        if (mode == 0) HG_HIP(c, hipMemcpyAsync(s.host, dst, bytes, hipMemcpyDeviceToHost, c->stream));
        HG_HIP(c, hipEventRecord(s.copied, c->stream));
    }
    s.bytes = bytes;
    s.format = format;
    c->rb.begin();
    return HG_OK;
}

// The copy event of the oldest outstanding display readback (nullptr when none is outstanding)
hipEvent_t hg_ctx_display_oldest(const hg_ctx* c) {
    return c->rb.pending > 0 ? c->slots[c->rb.oldest()].copied : nullptr;
}

extern "C" {

int hg_readback_begin_format(hg_ctx* c, int32_t format) {
    if (!c) return HG_E_INVALID;
    return hg_ctx_display_begin(c, nullptr, format);
}

int hg_readback_begin(hg_ctx* c) { return hg_readback_begin_format(c, HG_DISPLAY_RGBA32F); }

int hg_readback_end_data(hg_ctx* c, const void** data, size_t* n_bytes, int32_t* format) {
    if (!c || !data) return HG_E_INVALID;
    if (c->rb.pending <= 0) return fail(c, HG_E_INVALID, "no readback outstanding: call hg_readback_begin first");
    if (int rc = set_device(c)) return rc;
    const hg_ctx::DisplaySlot& s = c->slots[c->rb.oldest()];
    HG_HIP(c, hipEventSynchronize(s.copied));
    c->rb.end();
    *data = s.host;
    if (n_bytes) *n_bytes = s.bytes;
    if (format) *format = s.format;
    return lost_check(c);  // (the image is handed out either way: the accumulation through the last frame blended)
}

int hg_readback_end(hg_ctx* c, const float** rgba, size_t* n_floats) {
    if (!c || !rgba) return HG_E_INVALID;
    if (c->rb.pending <= 0) return fail(c, HG_E_INVALID, "no readback outstanding: call hg_readback_begin first");
    const int32_t oldest = c->slots[c->rb.oldest()].format;
    if (oldest != HG_DISPLAY_RGBA32F)
        return fail(c, HG_E_INVALID, "the oldest readback is in display format %d: use hg_readback_end_data", oldest);
    const void* data = nullptr;
    size_t bytes = 0;
    if (int rc = hg_readback_end_data(c, &data, &bytes, nullptr)) return rc;
    *rgba = static_cast<const float*>(data);
    if (n_floats) *n_floats = bytes / sizeof(float);
    return HG_OK;
}

int hg_pack_display(const float* rgba, size_t n_pixels, int32_t format, void* out) {
    if ((n_pixels && (!rgba || !out)) || !display_bpp(format)) return HG_E_INVALID;
    for (size_t i = 0; i < n_pixels; ++i) {
        const float* v = rgba + 4 * i;
        if (format == HG_DISPLAY_RGBA32F) {
            std::memcpy(static_cast<float*>(out) + 4 * i, v, 16);
        } else if (format == HG_DISPLAY_RGBA16F) {
            hg_pack_rgba16f(v[0], v[1], v[2], v[3], static_cast<uint32_t*>(out) + 2 * i);
        } else {
            static_cast<uint32_t*>(out)[i] = hg_pack_r11g11b10(v[0], v[1], v[2]);
        }
    }
    return HG_OK;
}

int hg_readback(hg_ctx* c, float* rgba, size_t n_floats) {
    if (!c || !rgba) return HG_E_INVALID;
    if (int rc = hg_ctx_flush(c)) return rc;
    if (c->W <= 0) return fail(c, HG_E_NOTARGET, "hg_resize not called");
    if (n_floats < size_t(c->W) * size_t(c->H) * 4) return fail(c, HG_E_INVALID, "readback buffer too small");
    if (int rc = set_device(c)) return rc;
    if (c->n_ranks == 1) {  // the whole image: untiled on the device, one copy into the caller's memory
        const size_t bytes = size_t(c->W) * size_t(c->H) * sizeof(float4);
        if (int rc = ensure_image(c, c->image, bytes)) return rc;
        if (int rc = launch_untile<false>(c, c->image.p, HG_DISPLAY_RGBA32F, static_cast<const float4*>(c->acc.p))) return rc;
        HG_HIP(c, hipMemcpyAsync(rgba, c->image.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HG_HIP(c, hipStreamSynchronize(c->stream));
        if (int rc = drain_events(c)) return rc;
        return lost_check(c);  // (the image is written either way: the accumulation through the last frame blended)
    }
    // this rank's pixels only (the others are left untouched): the tiles are repacked on the host
    std::vector<float4> tiles(size_t(c->n_local_tiles) * 64);
    if (!tiles.empty())
        HG_HIP(c, hipMemcpyAsync(tiles.data(), c->acc.p, tiles.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = drain_events(c)) return rc;
    for_local_pixels(c, [&](size_t slot, size_t pixel) { std::memcpy(rgba + pixel * 4, &tiles[slot], sizeof(float4)); });
    return lost_check(c);
}

}  // extern "C"
