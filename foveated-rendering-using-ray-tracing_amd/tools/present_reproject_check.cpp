// present_reproject_check.cpp — the reprojected present's rule (present_splat_place, present_splat_key,
// present_resolve_word, present_warp_texel in csrc/fr_math.h: the functions fr_present_reproject_pack and the kernels
// run) driven alone on the host under AddressSanitizer and UndefinedBehaviorSanitizer: positions and matrices that
// are huge, tiny, NaN and +-Inf, every array behind a checked index. What it shows: a place that is accepted lies
// inside the output, the float -> int conversions are only reached in range, and the resolve and the fallback read
// inside their images only. Runs without a device: make reproject-check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/fr_math.h"

using namespace fr;

int main() {
  std::mt19937 rng(12345);
  std::uniform_real_distribution<float> unit(-1.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-45f, 1e-38f, 1e30f, -1e30f, 3.4e38f, -3.4e38f, inf, -inf, nan, 0.5f, 7.0f};
  const int nspecial = (int)(sizeof(special) / sizeof(special[0]));
  const int sizes[][4] = {{1, 1, 1, 1}, {7, 5, 7, 5}, {64, 4, 64, 4}, {33, 17, 16, 9}, {259, 3, 259, 3}};
  unsigned long long landed = 0, cracks = 0, fallbacks = 0;
  for (const auto& sz : sizes) {
    const int W = sz[0], H = sz[1], ow = sz[2], oh = sz[3];
    for (int round = 0; round < 200; round++) {
      float vp[16], h[9];
      for (float& v : vp) v = unit(rng) * (round % 3 == 0 ? 1.0f : 4.0f);
      for (float& v : h) v = unit(rng) * 2.0f;
      if (round % 5 == 1) vp[rng() % 16] = special[rng() % nspecial];  // (the enqueues refuse these; the rule must not trip)
      if (round % 7 == 2) h[rng() % 9] = special[rng() % nspecial];
      if (round % 4 == 0) { h[0] = (float)W / ow; h[1] = 0; h[2] = 0; h[3] = 0; h[4] = (float)H / oh; h[5] = 0; h[6] = 0; h[7] = 0; h[8] = 1; }
      std::vector<f4> src((size_t)W * H), pos((size_t)W * H);
      for (size_t k = 0; k < src.size(); k++) {
        src[k] = mk4(unit(rng), unit(rng) * 2.0f, unit(rng), 1.0f);
        pos[k] = mk4(unit(rng) * 8.0f, unit(rng) * 8.0f, unit(rng) * 8.0f, 1.0f);
        if (rng() % 6 == 0) (&pos[k].x)[rng() % 3] = special[rng() % nspecial];
        if (rng() % 9 == 0) pos[k] = mk4(0.0f, 0.0f, 0.0f, 1.0f);
        if (rng() % 11 == 0) src[k].x = special[rng() % nspecial];
      }
      std::vector<uint64_t> keys((size_t)ow * oh, PRESENT_KEY_EMPTY);
      for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++) {
          int ox = -1, oy = -1;
          uint32_t depth = 0;
          if (!present_splat_place(pos.at((size_t)j * W + i), vp, ow, oh, &ox, &oy, &depth)) continue;
          if (ox < 0 || ox >= ow || oy < 0 || oy >= oh) { std::printf("a place outside the output: %d %d\n", ox, oy); return 1; }
          if (depth == 0 || depth > 0x7F800000u) { std::printf("a depth that is not a positive float: %08x\n", depth); return 1; }
          const uint64_t key = present_splat_key(depth, present_texel(src.at((size_t)j * W + i), (round & 1) != 0));
          uint64_t& k = keys.at((size_t)oy * ow + ox);
          if (key < k) k = key;
          landed++;
        }
      const auto key = [&](int i, int row) {
        if (i < 0 || i >= ow || row < 0 || row >= oh) { std::printf("a key read outside the output\n"); std::abort(); }
        return keys.at((size_t)row * ow + i);
      };
      const auto fetch = [&](int i, int row) {
        if (i < 0 || i >= W || row < 0 || row >= H) { std::printf("a tap outside the source\n"); std::abort(); }
        return src.at((size_t)row * W + i);
      };
      for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
          uint32_t w = 0;
          const uint64_t c = key(x, y);
          if (present_resolve_word(c, key, ow, oh, x, y, &w)) {
            cracks += c == PRESENT_KEY_EMPTY;
          } else {
            w = present_warp_texel(fetch, W, H, h, x, y, (round & 1) != 0);
            fallbacks++;
          }
          if ((w >> 24) != 0xFFu) { std::printf("alpha is not 255\n"); return 1; }
        }
    }
  }
  if (!landed || !cracks || !fallbacks) { std::printf("a zone of the rule did not occur\n"); return 1; }
  std::printf("present_reproject_check: %llu texels landed, %llu cracks closed, %llu fallback texels: ok\n", landed, cracks, fallbacks);
  return 0;
}
