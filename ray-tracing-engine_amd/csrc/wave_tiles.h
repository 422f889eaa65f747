// wave_tiles.h: the wave-tile list of a frame (rt_api.cpp ensure_tiles; host only, no device code, so that
// tools/wave_tiles_host_check.cpp can build it alone).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace rtl {

struct TileKey {
  uint32_t w = 0, h = 0, rank = 0, world = 0, tile = 0, sshift = 0;
  uint32_t fine = 0, sshiftFine = 0;  // the last `fine` coarse tiles stand in the list as their items at sshiftFine (wave_tiles)
  bool operator==(const TileKey& o) const {
    return w == o.w && h == o.h && rank == o.rank && world == o.world && tile == o.tile && sshift == o.sshift &&
           fine == o.fine && sshiftFine == o.sshiftFine;
  }
};

// A wave integrates (64 >> sshift) pixels x (1 << sshift) samples at a time.  Pixel
// footprint of one wave for sshift = 0..6: 8x8, 8x4, 4x4, 4x2, 2x2, 2x1, 1x1.
inline void wave_tile_shape(uint32_t sshift, uint32_t& tw, uint32_t& th) {
  static const uint32_t W[7] = {8, 8, 4, 4, 2, 2, 1}, H[7] = {8, 4, 4, 2, 2, 1, 1};
  tw = W[sshift], th = H[sshift];
}

// f(x8, y8) for each 8x8-pixel granule rank `rank` of `world` owns, row-major — the order ensure_tiles
// renders them in and the order of the packed exchange buffer.
template <class F>
void owned_granules(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t tile, F f) {
  if (tile == 0) tile = 8;
  if (world == 0) world = 1;
  const uint32_t gx = (w + 7) / 8, gy = (h + 7) / 8;
  for (uint32_t y8 = 0; y8 < gy; ++y8)
    for (uint32_t x8 = 0; x8 < gx; ++x8)
      if (world <= 1 || (x8 * 8 / tile + y8 * 8 / tile) % world == rank) f(x8, y8);
}

// the wave tiles inside each owned granule, row-major, so that consecutive waves touch neighbouring pixels
// The fine tail (k.fine > 0, k.sshiftFine > k.sshift): the last k.fine coarse tiles leave the list and their pixels come
// back behind all coarse items as items at sshiftFine, row-major within each coarse tile, in the coarse tiles' order —
// shorter items for the end of a launch whose waves draw from a counter (rt_kernels.h RenderArgs::fineFrom).
// *fineFrom: the index of the first fine item, or the list's length.
inline std::vector<uint32_t> wave_tiles(const TileKey& k, uint32_t* fineFrom = nullptr) {
  std::vector<uint32_t> tiles;
  uint32_t tw, th;
  wave_tile_shape(k.sshift, tw, th);
  owned_granules(k.w, k.h, k.rank, k.world, k.tile, [&](uint32_t x8, uint32_t y8) {
    for (uint32_t y = y8 * 8; y < y8 * 8 + 8 && y < k.h; y += th)
      for (uint32_t x = x8 * 8; x < x8 * 8 + 8 && x < k.w; x += tw) tiles.push_back(x | (y << 16));
  });
  uint32_t from = (uint32_t)tiles.size();
  if (k.fine && k.sshiftFine > k.sshift) {
    const uint32_t f = std::min<uint32_t>(k.fine, from);
    const std::vector<uint32_t> split(tiles.end() - f, tiles.end());
    tiles.resize(from -= f);
    uint32_t fw, fh;
    wave_tile_shape(k.sshiftFine, fw, fh);
    for (const uint32_t t : split) {
      const uint32_t x0 = t & 0xffffu, y0 = t >> 16;
      for (uint32_t y = y0; y < y0 + th && y < k.h; y += fh)
        for (uint32_t x = x0; x < x0 + tw && x < k.w; x += fw) tiles.push_back(x | (y << 16));
    }
  }
  if (fineFrom) *fineFrom = from;
  return tiles;
}

}  // namespace rtl
