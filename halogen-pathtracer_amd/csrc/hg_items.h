// hg_items.h — the integer arithmetic that decides which lane traces which pixel of which frame, one definition for
// device and host code (nothing of HIP here: tests/test_item_mapping.py compiles it with g++).
//
// A launch's work is cut into units (a local tile x a chunk of the launch's frames); a unit's (pixel, frame) items are
// numbered pixel-major and handed to the lanes of a wave one after another (hg_sched.h, hg_server.h).  Everything here
// is 32-bit, as the kernels compute it: the host guarantees tiles, frames and items of a launch below 2^31.
#pragma once
#include <stdint.h>

#include "hg_tiling.h"
#include "hg_tunables.h"

HG_HD uint32_t hg_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// ---- tile rectangle --------------------------------------------------------------------------------------------
struct HgTileRect {
    uint32_t x0, y0;  // image pixel of the tile's lane 0 (hg_tile_origin, in 32 bits)
    uint32_t tw, th;  // its width and height inside the W x H image (hg_tile_extent)
};
// The part of a tile starting at `origin` that lies inside an image `size` wide (or high): min(8, size - origin), 0
// when the tile starts outside
HG_HD uint32_t hg_tile_extent(uint32_t size, uint32_t origin) {
    return hg_umin(uint32_t(HG_TILE), size - hg_umin(size, origin));
}
// The rectangle of global tile g = hg_global_tile(local tile, rank, ranks).  I is the integer type of the division:
// uint32_t, or int where a kernel's prologue has divided signed since before item scheduling (the two compile to
// different instructions; they agree for every tile of an image).
template <class I>
HG_HD I hg_global_tile(I local_tile, I rank, I n_ranks) {
    return rank + local_tile * n_ranks;
}
// (Results through references, not a returned struct: inlined into a kernel, these compile to the instructions that the
// arithmetic written out in place compiled to, in the same order.)
template <class I>
HG_HD void hg_global_tile_origin(I g, I tiles_x, uint32_t& x0, uint32_t& y0) {  // hg_tile_origin, in 32 bits
    const I ty = g / tiles_x;
    x0 = uint32_t(g - ty * tiles_x) * HG_TILE;
    y0 = uint32_t(ty) * HG_TILE;
}
template <class I>
HG_HD void hg_global_tile_rect(I g, I tiles_x, uint32_t W, uint32_t H, HgTileRect& r) {
    hg_global_tile_origin(g, tiles_x, r.x0, r.y0);
    r.tw = hg_tile_extent(W, r.x0);
    r.th = hg_tile_extent(H, r.y0);
}
HG_HD HgTileRect hg_tile_rect(uint32_t local_tile, uint32_t rank, uint32_t n_ranks, uint32_t tiles_x, uint32_t W,
                              uint32_t H) {
    HgTileRect r;
    hg_global_tile_rect<uint32_t>(hg_global_tile(local_tile, rank, n_ranks), tiles_x, W, H, r);
    return r;
}

// ---- items of one unit -----------------------------------------------------------------------------------------
struct HgItem {
    uint32_t i, f;  // the item's valid pixel (0 .. tw * th - 1) and its frame within the unit's nf frames
};
// Item k of a unit of nf frames, pixel-major: pixel k / nf, frame k mod nf (a wave's lanes trace one pixel's frames).
// A power-of-two nf (every chunk of the default 64-frame launches) takes a shift and a mask; use_shift = false (the
// CPU test) forces the division for such an nf too.
HG_HD HgItem hg_item_split(uint32_t k, uint32_t nf, bool use_shift = true) {
    uint32_t i, f;
    if (use_shift && (nf & (nf - 1u)) == 0u) {
        const uint32_t lg = uint32_t(__builtin_ctz(nf));
        i = k >> lg;
        f = k & (nf - 1u);
    } else {
        i = k / nf;
        f = k - i * nf;
    }
    return HgItem{i, f};
}
// Valid pixel i of a tile whose tw x th rectangle (nv = tw * th pixels) lies inside the image -> its pixel within the
// tile, x + 8 y
HG_HD uint32_t hg_item_pixel(uint32_t i, uint32_t tw, uint32_t nv) {
    return nv == 64u ? i : (i % tw) + 8u * (i / tw);
}

// ---- items of a wave's several units (UnitItems, whole tiles only) ---------------------------------------------
struct HgUnitItem {
    uint32_t j, pix, f;  // the unit, the pixel within its tile, the frame within the nf frames
};
// The units' items are numbered one unit after another, 64 * nf each: item k -> its unit (HgItem::i) and its number
// within the unit (HgItem::f)
HG_HD HgItem hg_unit_split(uint32_t k, uint32_t nf, bool use_shift = true) {
    uint32_t j, kk;
    if (use_shift && (nf & (nf - 1u)) == 0u) {
        const uint32_t lg = 6u + uint32_t(__builtin_ctz(nf));
        j = k >> lg;
        kk = k & ((1u << lg) - 1u);
    } else {
        j = k / (64u * nf);
        kk = k - j * (64u * nf);
    }
    return HgItem{j, kk};
}
HG_HD HgUnitItem hg_unit_item(uint32_t k, uint32_t nf, bool use_shift = true) {
    const HgItem u = hg_unit_split(k, nf, use_shift);
    const HgItem it = hg_item_split(u.f, nf, use_shift);
    return HgUnitItem{u.i, hg_item_pixel(it.i, 8u, 64u), it.f};
}

// ---- frame chunks ----------------------------------------------------------------------------------------------
// Chunk c of `split` covers the launch's frames [hg_chunk_begin(c), hg_chunk_begin(c + 1))
HG_HD uint32_t hg_chunk_begin(uint32_t chunk, uint32_t n_frames, uint32_t split) {
    return uint32_t((uint64_t(chunk) * n_frames) / split);
}

// ---- wave -> unit ----------------------------------------------------------------------------------------------
// Wave (or queue unit) gw of a launch of nlt tiles x split chunks: its position in the launch's tile order (the kernel
// reads tile_order[pos]; >= nlt: past the end) and its frame chunk (>= split: no work).  Tile-index order is
// chunk-major (tile gw mod nlt, chunk gw / nlt).  Cost order is tile-major (position gw / split, chunk gw mod split),
// so a tile's chunks run side by side and the most expensive tiles' chunks all start first; there waves past the last
// unit get chunk = split.
HG_HD uint32_t hg_wave_unit_pos(uint32_t gw, uint32_t nlt, uint32_t split, bool cost_order) {
    return cost_order ? gw / split : gw % nlt;
}
HG_HD uint32_t hg_wave_unit_chunk(uint32_t gw, uint32_t nlt, uint32_t split, bool cost_order) {
    if (cost_order) return gw / split < nlt ? gw % split : split;
    return gw / nlt;
}

// ---- the render server's run placement ---------------------------------------------------------------------------
// Unit i of a server frame (head i % 8, the XCD whose waves pull it first) -> its place in the frame's tiles: head h
// takes runs h, h + 8, ... of HG_SV_TILE_RUN consecutive tiles, so a wave's and a CU's consecutive units are
// neighbours; the tail past the last whole round of 8 runs stays in place.
HG_HD uint32_t hg_sv_run_place(uint32_t i, uint32_t nlt) {
    constexpr uint32_t B = HG_SV_TILE_RUN;
    if (i < (nlt / (8u * B)) * (8u * B)) {
        const uint32_t h = i & 7u, n = i >> 3;
        i = (n / B) * (8u * B) + h * B + n % B;
    }
    return i;
}

// ---- cost order ------------------------------------------------------------------------------------------------
// The bucket of a tile's wave-clock cost: 1024 log-scale buckets, 16 per octave, bucket 0 the most expensive
HG_HD uint32_t hg_order_bucket(unsigned long long c) {
    if (c < 2ull) return 1023u;
    const uint32_t e = 63u - uint32_t(__builtin_clzll(c));                          // 1..63
    const uint32_t m = uint32_t(e >= 4u ? (c >> (e - 4u)) : (c << (4u - e))) & 15u;  // the 4 bits after the leading 1
    return 1023u - (e * 16u + m);
}
