// wave_tiles_host_check.cpp — the wave-tile list builder (csrc/wave_tiles.h) as a stand-alone program: host only, no GPU, no
// Python; tests/test_wave_tiles_host.py builds it with the sanitizers and runs it.  From the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iray-tracing-engine_amd/csrc \
//       tools/wave_tiles_host_check.cpp -o wave_tiles_host_check && ./wave_tiles_host_check
// For every frame size, shard, coarse and fine shift and number of split tiles it checks that
//  * every in-image pixel the rank owns is covered exactly once, and no other pixel at all,
//  * the coarse items are the first of the plain list, in its order; the fine items come last, row-major within each split
//    coarse tile, in the coarse tiles' order,
//  * fineFrom and the two counts are what the split says (F = 0: the plain list; F beyond the list: every tile split; a fine
//    shift that is not above the coarse one: no tail).
#include <cstdio>
#include <vector>

#include "wave_tiles.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                                                                   \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      if (failures < 20) fprintf(stderr, "line %d: %s  [%ux%u rank %u/%u s %u -> %u F %u]\n", __LINE__, #cond, k.w, k.h, k.rank, k.world, k.sshift, k.sshiftFine, k.fine); \
      ++failures;                                                                                                      \
    }                                                                                                                  \
  } while (0)

void check(const rtl::TileKey& k) {
  rtl::TileKey plainKey = k;
  plainKey.fine = 0, plainKey.sshiftFine = 0;
  uint32_t plainFrom = 12345u;
  const std::vector<uint32_t> plain = rtl::wave_tiles(plainKey, &plainFrom);
  EXPECT(plainFrom == plain.size());
  uint32_t from = 12345u;
  const std::vector<uint32_t> got = rtl::wave_tiles(k, &from);
  EXPECT(rtl::wave_tiles(k) == got);  // (the index is optional)
  const bool tail = k.fine && k.sshiftFine > k.sshift;
  const uint32_t split = tail ? std::min<uint32_t>(k.fine, (uint32_t)plain.size()) : 0u;
  EXPECT(from == plain.size() - split && from <= got.size());
  if (from > got.size()) return;
  if (!split) EXPECT(got == plain);
  for (uint32_t i = 0; i < from; ++i) EXPECT(got[i] == plain[i]);
  // the fine items, as the definition says them
  uint32_t tw, th, fw = 0, fh = 0;
  rtl::wave_tile_shape(k.sshift, tw, th);
  if (tail) rtl::wave_tile_shape(k.sshiftFine, fw, fh);
  std::vector<uint32_t> want;
  for (uint32_t i = from; i < plain.size(); ++i) {
    const uint32_t x0 = plain[i] & 0xffffu, y0 = plain[i] >> 16;
    for (uint32_t y = y0; y < y0 + th; y += fh)
      for (uint32_t x = x0; x < x0 + tw; x += fw)
        if (x < k.w && y < k.h) want.push_back(x | (y << 16));
  }
  EXPECT(std::vector<uint32_t>(got.begin() + from, got.end()) == want);
  // coverage: every owned in-image pixel once, nothing else
  std::vector<uint8_t> cover((size_t)k.w * k.h, 0), owned((size_t)k.w * k.h, 0);
  rtl::owned_granules(k.w, k.h, k.rank, k.world, k.tile, [&](uint32_t x8, uint32_t y8) {
    for (uint32_t y = y8 * 8; y < y8 * 8 + 8 && y < k.h; ++y)
      for (uint32_t x = x8 * 8; x < x8 * 8 + 8 && x < k.w; ++x) owned[(size_t)y * k.w + x] = 1;
  });
  for (uint32_t i = 0; i < got.size(); ++i) {
    const uint32_t w = i < from ? tw : fw, h = i < from ? th : fh, x0 = got[i] & 0xffffu, y0 = got[i] >> 16;
    EXPECT(x0 < k.w && y0 < k.h);  // (an item starts inside the image)
    for (uint32_t y = y0; y < y0 + h && y < k.h; ++y)
      for (uint32_t x = x0; x < x0 + w && x < k.w; ++x) ++cover[(size_t)y * k.w + x];
  }
  bool once = true;
  for (size_t i = 0; i < cover.size(); ++i) once = once && cover[i] == owned[i];
  EXPECT(once);
}

}  // namespace

int main() {
  const uint32_t sizes[][2] = {{8, 8}, {1, 1}, {33, 19}, {64, 64}, {7, 30}, {21, 8}, {70, 3}};  // (widths and heights no footprint divides)
  uint32_t cases = 0;
  for (const auto& sz : sizes)
    for (uint32_t world = 1; world <= 3; ++world)
      for (uint32_t rank = 0; rank < world; ++rank)
        for (uint32_t s = 0; s <= 6; ++s)
          for (uint32_t sf = 0; sf <= 6; ++sf)
            for (const uint32_t fine : {0u, 1u, 2u, 5u, 100000u, ~0u}) {
              rtl::TileKey k;
              k.w = sz[0], k.h = sz[1], k.rank = rank, k.world = world, k.tile = world == 3 ? 16 : 8, k.sshift = s;
              k.fine = fine, k.sshiftFine = sf;
              check(k);
              ++cases;
            }
  printf("%u cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
