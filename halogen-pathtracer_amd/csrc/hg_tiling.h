// hg_tiling.h — the image tiling of the multi-GPU path, one definition for device and host code.
//
// The image is cut into 8x8 tiles numbered row-major (g = ty * tiles_x + tx).  Rank r of n owns the tiles g with
// g % n == r, stored in its accumulator as local tile l = g / n (tile-major, pixel (x & 7) + 8 (y & 7) of a tile at
// float4 l * 64 + lane; hg_layout.h).  The gather moves every rank's local tiles into slab r of the root's staging
// buffer ([rank][slab_tiles][64] float4, slab_tiles = rank 0's count, the largest).  hg_assemble_image (hg_comm.hip)
// and its host twin hg_comm_assemble_host (the torch-gather path of halogen/distributed.py and the CPU tests) both
// read the image through hg_pixel_source, so the two gathers cannot disagree on where a pixel lives.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_HD __host__ __device__ __forceinline__
#else
#define HG_HD inline
#endif

// tiles owned by `rank` of n when the image has `total` tiles (ragged: the first total % n ranks hold one more)
HG_HD int64_t hg_rank_tiles(int64_t total, int32_t rank, int32_t n) {
    return total > rank ? (total - rank + n - 1) / n : 0;
}

struct HgPixelSource {
    uint32_t rank;        // owner rank of the pixel's tile
    uint32_t local_tile;  // the tile's index in that rank's accumulator / slab
    uint32_t lane;        // the pixel within the tile, (x & 7) + 8 (y & 7)
};

// Where image pixel (x, y) lives among the ranks' tiles
HG_HD HgPixelSource hg_pixel_source(uint32_t x, uint32_t y, uint32_t tiles_x, uint32_t n_ranks) {
    const uint32_t g = (y >> 3) * tiles_x + (x >> 3);
    return HgPixelSource{g % n_ranks, g / n_ranks, (x & 7u) + 8u * (y & 7u)};
}

struct HgTileOrigin {
    uint32_t x, y;  // image pixel of the tile's lane 0 (an edge tile may reach beyond the image)
};

// The inverse: where local tile `local_tile` of `rank` lies in the image (global tile rank + local_tile * n_ranks)
HG_HD HgTileOrigin hg_tile_origin(uint32_t local_tile, uint32_t rank, uint32_t n_ranks, uint32_t tiles_x) {
    const uint64_t g = uint64_t(rank) + uint64_t(local_tile) * n_ranks;
    return HgTileOrigin{uint32_t(g % tiles_x) * 8u, uint32_t(g / tiles_x) * 8u};
}

// Visit the pixels inside the W x H image of a rank's n_local_tiles local tiles: f(accumulator slot, image pixel),
// slot = local_tile * 64 + lane, pixel = y * W + x.  Slots of an edge tile beyond the image are not visited.
template <class F>
inline void hg_for_local_pixels(uint32_t W, uint32_t H, uint32_t n_local_tiles, uint32_t rank, uint32_t n_ranks, F&& f) {
    const uint32_t tiles_x = (W + 7u) / 8u;
    for (uint32_t lt = 0; lt < n_local_tiles; ++lt) {
        const HgTileOrigin o = hg_tile_origin(lt, rank, n_ranks, tiles_x);
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t x = o.x + (l & 7u), y = o.y + (l >> 3);
            if (x < W && y < H) f(size_t(lt) * 64u + l, size_t(y) * W + x);
        }
    }
}

// float4 index of a pixel source in the [rank][slab_tiles][64] staging layout
HG_HD size_t hg_slab_index(const HgPixelSource& s, uint32_t slab_tiles) {
    return (size_t(s.rank) * slab_tiles + s.local_tile) * 64u + s.lane;
}
