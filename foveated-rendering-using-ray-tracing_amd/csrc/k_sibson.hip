// k_sibson.hip — SibsonInterpolation  FR/SibsonInterpolation.cpp:28-53, FR/shader/sibsonFS.glsl:16-49
// GL texture fetches at texel centres are integer texel loads; off-centre GL_LINEAR taps use fr::bilinear_repeat.
#include <hip/hip_runtime.h>
#include <cmath>
#include "fr_device.h"
#include "k_launch.h"
#include "k_image.h"

namespace fr {

// (sqrt_le_bound, fr_math.h: the disc test "sqrtf(r2) > d" of Sibson is "r2 > sqrt_le_bound(d)".)

// ------------------------------------------------------------------------------------------
// Sibson / nearest-natural-neighbour (sibsonFS.glsl:16-49, the active "#if 1" branch).
// ------------------------------------------------------------------------------------------
FR_DEV f3 rgb_at(const char* base, uint32_t texel) {  // 12-byte load of texel .xyz, 32-bit byte offset
  return *reinterpret_cast<const f3*>(base + (texel << 4));
}

// The taps of a row that pass the reference's tests (w in [0, 1) and distance <= d) are one
// contiguous run of the row's w sequence: w grows strictly (w += 1/W), so "w in [0, 1)" is an
// interval of it, and r2 = fl(fl(dx^2) + dy^2) with dx = fl(frag.x - w) does not increase up to
// w = frag.x and does not decrease after (every step is a monotone rounded operation), so
// "r2 <= r2max" is an interval too. A row therefore skips to its first valid tap and stops at the
// first invalid one after it; the taps it adds and their order are the reference's.
// WRAP = false: every tap of the pixel has 0 <= i0 and i1 <= W - 1 (the kernel checks it per wave),
// so the horizontal REPEAT wrap is not evaluated.
template <bool WRAP>
FR_DEV void sibson_pixel(const f4* __restrict__ coord, const f4* __restrict__ color, f4* __restrict__ out, int W,
                         int H, f2 screen, int x, int y) {
  const f2 frag = frag_uv(x, y, screen);
  const f4 closest = coord[(size_t)y * W + x];
  const float cdx = closest.x - frag.x, cdy = closest.y - frag.y;
  const float d2 = cdx * cdx + cdy * cdy;
  const float d = sqrtf(d2);  // distance(closest.st, FragCoord.st)
  // distance(FragCoord, reference) > d  <=>  r2 > r2max (exact, see sqrt_le_bound)
  const float r2max = sqrt_le_bound(d);
  const char* cbase = reinterpret_cast<const char*>(color);
  f4 inc = mk4(0, 0, 0, 0);
  const f2 min_box = mk2(frag.x - d, frag.y - d);
  const f2 max_box = mk2(frag.x + d, frag.y + d);
  const f2 increment = mk2(1.0f / screen.x, 1.0f / screen.y);
  for (float h = min_box.y; h < max_box.y; h += increment.y) {
    if (h < 0.0f || h >= 1.0f) continue;
    const float dy = frag.y - h;
    const float dy2 = dy * dy;
    float w = min_box.x;
    // skip to the row's first valid tap
    while (w < max_box.x) {
      const float dx = frag.x - w;
      if (w >= 0.0f && w < 1.0f && dx * dx + dy2 <= r2max) break;
      w += increment.x;
    }
    if (!(w < max_box.x)) continue;
    // GL_LINEAR rows for this h: ty in [-0.5, H - 0.5) -> j0 in [-1, H-1], REPEAT wrap
    const float ty = h * screen.y - 0.5f;
    const float fy0 = floorf(ty);
    float b = ty - fy0;
    b = floorf(b * 256.0f + 0.5f) * (1.0f / 256.0f);
    int j0 = (int)fy0;
    int j1 = j0 + 1 == H ? 0 : j0 + 1;
    j0 = j0 < 0 ? H - 1 : j0;
    const uint32_t o0 = (uint32_t)j0 * (uint32_t)W, o1 = (uint32_t)j1 * (uint32_t)W;
    const float nb = 1.0f - b;
    // colour rows as RGB (alpha is never read); consecutive taps of a row share a texel column,
    // so the previous tap's right column is reused instead of re-read (same values, half the loads).
    // Two column pairs alternate as left / right (the loop is unrolled by two: no register moves).
    int prev_i1 = -1;
    f3 A0 = mk3(0.0f), A1 = mk3(0.0f), B0 = mk3(0.0f), B1 = mk3(0.0f);
    auto tap = [&](f3& L0, f3& L1, f3& R0, f3& R1) {  // one tap at w; true while the next one is valid
      const float tx = w * screen.x - 0.5f;
      const float fx0 = floorf(tx);
      float a = tx - fx0;
      a = floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f);
      int i0 = (int)fx0;
      int i1 = i0 + 1;
      if (WRAP) {
        i1 = i1 == W ? 0 : i1;
        i0 = i0 < 0 ? W - 1 : i0;
      }
      if (i0 != prev_i1) {
        L0 = rgb_at(cbase, o0 + (uint32_t)i0);
        L1 = rgb_at(cbase, o1 + (uint32_t)i0);
      }
      R0 = rgb_at(cbase, o0 + (uint32_t)i1);
      R1 = rgb_at(cbase, o1 + (uint32_t)i1);
      const float na = 1.0f - a;
      const float w00 = na * nb, w10 = a * nb, w01 = na * b, w11 = a * b;
      const f3 c = L0 * w00 + R0 * w10 + L1 * w01 + R1 * w11;
      inc = inc + mk4(c.x, c.y, c.z, 1.0f);
      prev_i1 = i1;
      w += increment.x;
      if (!(w < max_box.x) || !(w < 1.0f)) return false;
      const float dx = frag.x - w;
      return !(dx * dx + dy2 > r2max);
    };
    while (tap(A0, A1, B0, B1) && tap(B0, B1, A0, A1)) {
    }
  }
  f4 o;
  if (inc.w > 0.0f) {
    o = mk4(inc.x / inc.w, inc.y / inc.w, inc.z / inc.w, 1.0f);
  } else {
    // no tap (a seed pixel, d = 0): texture2D(colorTex, closest.st), closest.st is a texel centre
    uint32_t cx = f2u_sat(closest.x * screen.x), cy = f2u_sat(closest.y * screen.y);
    cx = min(cx, (uint32_t)W - 1); cy = min(cy, (uint32_t)H - 1);
    o = color[(size_t)cy * W + cx];
  }
  out[(size_t)y * W + x] = o;
}

// The work of a pixel grows with d^2 (d = distance to its seed) and d runs from 0 to the cell
// radius inside every Voronoi cell, so the lanes of a wave over a spatial block idle much of the
// time. Each block ranks the pixels of a SIB_TILE x SIB_TILE tile by radius (LDS counting sort on
// one-pixel buckets) and its waves take 64 consecutive pixels of that order: similar trip counts
// per wave, still inside one tile (the colour window stays in L1/L2). Measured at 4K: 32x32 tiles
// 1.43-1.48 ms, 16x16 1.52; finer buckets (quarter, half pixel) are slower (they scatter the
// pixels of a wave over the tile). Every pixel is still computed by one
// lane with the reference's loop order: bit-identical results.
#ifndef SIB_TILE
#define SIB_TILE 32
#endif
#define SIB_THREADS (SIB_TILE * SIB_TILE)
#define SIB_BUCKETS 128
#ifndef SIB_BUCKETS_PER_PX
#define SIB_BUCKETS_PER_PX 1.0f
#endif

__global__ __launch_bounds__(SIB_THREADS) void k_sibson(const f4* __restrict__ coord, const f4* __restrict__ color,
                                                        f4* __restrict__ out, int W, int H, f2 screen) {
  __shared__ uint32_t bucket[SIB_BUCKETS];
  __shared__ uint16_t order[SIB_THREADS];
  __shared__ uint8_t keys[SIB_THREADS];
  const int tid = threadIdx.x;
  const int bx0 = blockIdx.x * SIB_TILE, by0 = blockIdx.y * SIB_TILE;
  for (int i = tid; i < SIB_BUCKETS; i += SIB_THREADS) bucket[i] = 0;
  __syncthreads();
  const int x = bx0 + (tid % SIB_TILE), y = by0 + (tid / SIB_TILE);
  int key = -1;
  if (x < W && y < H) {
    const f2 frag = frag_uv(x, y, screen);
    const f4 c = coord[(size_t)y * W + x];
    const float dx = c.x - frag.x, dy = c.y - frag.y;
    const float r = sqrtf(dx * dx + dy * dy) * fmaxf(screen.x, screen.y) * SIB_BUCKETS_PER_PX;
    key = r < (float)(SIB_BUCKETS - 1) ? (int)r : SIB_BUCKETS - 1;
    keys[tid] = (uint8_t)key;
    atomicAdd(&bucket[key], 1u);
  }
  __syncthreads();
  if (tid < 64) {  // exclusive scan of the bucket counts (one wave, two buckets per lane)
    const uint32_t v0 = bucket[2 * tid], v1 = bucket[2 * tid + 1];
    uint32_t incl = v0 + v1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (tid >= o) incl += t;
    }
    bucket[2 * tid] = incl - v0 - v1;
    bucket[2 * tid + 1] = incl - v1;
  }
  __syncthreads();
  if (key >= 0) order[atomicAdd(&bucket[key], 1u)] = (uint16_t)tid;
  __syncthreads();
  const int n = (int)bucket[SIB_BUCKETS - 1];  // after the scatter: end of the last bucket = pixels in the tile
  if (tid >= n) return;
  const int p = order[tid];
  const int px = bx0 + (p % SIB_TILE), py = by0 + (p / SIB_TILE);
  // taps span tx in [px - d W, px + d W) (texel units); d W <= r / SIB_BUCKETS_PER_PX, with 2 px of slack
  const int pkey = keys[p];
  const float rx = (float)(pkey + 1) / SIB_BUCKETS_PER_PX + 2.0f;
  const bool border = (float)px - rx < 0.0f || (float)px + rx + 1.0f >= (float)W || pkey == SIB_BUCKETS - 1;
  if (__ballot(border)) sibson_pixel<true>(coord, color, out, W, H, screen, px, py);
  else sibson_pixel<false>(coord, color, out, W, H, screen, px, py);
}

void launch_sibson(const f4* coord, const f4* color, f4* out, int W, int H, hipStream_t stream) {
  dim3 grid((W + SIB_TILE - 1) / SIB_TILE, (H + SIB_TILE - 1) / SIB_TILE);
  hipLaunchKernelGGL(k_sibson, grid, dim3(SIB_THREADS), 0, stream, coord, color, out, W, H, mk2((float)W, (float)H));
}

// ------------------------------------------------------------------------------------------
// Sibson, run form (fr_config.sibson_mode 0, the default). The taps of a row form one contiguous
// run (above) and sit one texel apart, so the GL_LINEAR taps of a run all share the horizontal
// weight a of its first tap and walk consecutive texel columns: the run's sum is
//   nb (na S0[I, I+n) + a S0[I+1, I+n+1)) + b (na S1[I, I+n) + a S1[I+1, I+n+1))
// with S_j[p, q) the sum of colour row j over columns p..q-1, read from per-row prefix sums. A row
// then costs a membership walk of its taps (a few VALU per tap, exact: the reference's positions
// and distance tests) plus eight prefix loads, instead of four texel loads and a bilinear blend
// per tap. Which taps count is exact; the sum differs from the per-tap form in rounding (the
// summation order) and where the accumulated positions drift across a 1/256 weight step inside a
// run (|a_k - a| <= 1/256 on the few taps that straddle a colour change): ~1e-6 on the image,
// checked against the oracle in tests/test_gpu_parity.py. Rows whose taps need the horizontal
// REPEAT wrap (the image's left and right borders) take the per-tap form.
//
// Prefix layout: row j, column i in [0, W]: P[j (W + 1) + i] = sum of the row's colours from the
// start of i's 64-column block up to i - 1 (values stay small: fp32 keeps ~1e-6 of a colour), and
// T[j NB + B] = block B's total, NB = ceil((W + 1) / 64); then S_j[p, q) = P[q] - P[p] + T[p/64 ..
// q/64 - 1].
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sibson_prefix(const f4* __restrict__ color, f4* __restrict__ P,
                                                      f4* __restrict__ T, int W, int NB) {
  const int lane = threadIdx.x;
  const int j = blockIdx.y, B = blockIdx.x;
  const int col = B * 64 + lane;
  f3 v = mk3(0.0f);
  if (col < W) v = xyz(color[(size_t)j * W + col]);
  f3 incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float tx = __shfl_up(incl.x, o, 64), ty = __shfl_up(incl.y, o, 64), tz = __shfl_up(incl.z, o, 64);
    if (lane >= o) incl = incl + mk3(tx, ty, tz);
  }
  if (col <= W) P[(size_t)j * (W + 1) + col] = mk4(incl - v, 0.0f);
  if (lane == 63) T[(size_t)j * NB + B] = mk4(incl, 0.0f);
}

FR_DEV f3 sib_rowsum(const f4* __restrict__ Pj, const f4* __restrict__ Tj, int p, int q) {
  f3 s = xyz(Pj[q]) - xyz(Pj[p]);
  for (int B = p >> 6; B < (q >> 6); B++) s = s + xyz(Tj[B]);
  return s;
}

// A row's run in closed form. The reference's tap positions are w_{k+1} = fl(w_k + 1/W) from
// w_0 = min_box.x. While they stay in one binade [2^e, 2^(e+1)) every w_k is a multiple of that
// binade's ulp u, and fl(w + inc) - w is inc rounded to a multiple of u: the same step delta for
// every k (a rounding tie alternates it; the first two steps then differ and the pixel walks its
// rows instead). So w_k = w_0 + k delta exactly (one fma, exact), and a row's run [k0, k1] follows
// from a chord estimate corrected by the reference's own per-tap test: O(1) per row instead of a
// walk over its taps. The x-extent (w_0, delta, the taps K inside the box, the tap nearest frag.x)
// is the same for every row of a pixel and is set up once. Pixels whose box is not inside one
// positive binade below 1 (left and right borders, binade edges) walk their rows.
struct SibRows {
  bool closed;
  float w0, delta, inv;
  int K, kbest;  // taps k < K lie in the box; kbest minimises the horizontal distance
  // multi: a box that crosses one binade edge of the tap positions (x = 0.5, 0.25, ... of the screen): its
  // taps in up to three runs of equal steps, tap k at fma(k - ks, ds, vs) for the last s with ks <= k
  // (sib_axis_build's segments); the rows' runs then come from the same four exact tests (sib_row_run_multi)
  bool multi;
};
struct SibMulti {  // (built only where a row loop needs it: sib_rows_multi)
  float w0, delta, inv;
  int K, kbest;
  int k1, k2;
  float v1, d1, v2, d2;
};

FR_DEV float sib_wk(const SibRows& r, int k) { return __builtin_fmaf((float)k, r.delta, r.w0); }
FR_DEV float sib_wk_multi(const SibMulti& r, int k) {
  return k >= r.k2 ? __builtin_fmaf((float)(k - r.k2), r.d2, r.v2)
                   : k >= r.k1 ? __builtin_fmaf((float)(k - r.k1), r.d1, r.v1) : __builtin_fmaf((float)k, r.delta, r.w0);
}
// an estimate (within a tap) of the index of the tap at position p
FR_DEV float sib_k_est(const SibMulti& r, float p) {
  return p >= r.v2 ? (float)r.k2 + (p - r.v2) * __builtin_amdgcn_rcpf(r.d2)
                   : p >= r.v1 ? (float)r.k1 + (p - r.v1) * __builtin_amdgcn_rcpf(r.d1) : (p - r.w0) * r.inv;
}

FR_DEV int sib_binade_steps(float v, float delta);
FR_DEV int sib_count_below(float v, float delta, float lim);
FR_DEV bool sib_same_binade(float a, float b);

// The multi-segment form of a box inside (0, 1) whose taps need two or three segments (sib_axis_build's
// rule); false when they need more (the pixel walks its rows, or goes to k_sibson_wide).
FR_DEV bool sib_rows_multi(SibMulti& r, float fx, float w0, float wmax, float inc) {
  // segment s of sib_axis_build: start tap k, start v, step d; the next one starts at the tap after its last
  auto segment = [&](float v, int& m, float& d) {
    const float v1 = v + inc, v2 = v1 + inc;
    const float delta = v1 - v;
    m = 0;
    if (v != 0.0f && sib_same_binade(v, v2) && v2 - v1 == delta && delta > 0.0f) {
      m = min(sib_binade_steps(v, delta), sib_count_below(v, delta, wmax) - 1);
      if (m >= 1 && __builtin_fmaf((float)(m - 1), delta, v) + inc != __builtin_fmaf((float)m, delta, v)) m--;
    }
    d = delta > 0.0f ? delta : inc;
    return __builtin_fmaf((float)m, delta, v) + inc;  // the reference's step from the segment's last tap
  };
  int m0, m1 = 0, m2 = 0;
  float d0, d1 = inc, d2 = inc;
  const float va = segment(w0, m0, d0);
  int K = m0 + 1, k1 = K, k2 = K;
  float v1 = INFINITY, v2 = INFINITY;
  if (va < wmax) {
    v1 = va;
    const float vb = segment(v1, m1, d1);
    K += m1 + 1;
    k2 = K;
    if (vb < wmax) {
      v2 = vb;
      const float vc = segment(v2, m2, d2);
      K += m2 + 1;
      if (vc < wmax) return false;  // more than three segments
    }
  }
  r.w0 = w0; r.delta = d0; r.inv = __builtin_amdgcn_rcpf(d0);
  r.K = K; r.kbest = 0;
  r.k1 = k1; r.v1 = v1; r.d1 = d1;
  r.k2 = k2; r.v2 = v2; r.d2 = d2;
  const int kc = min(max((int)floorf(sib_k_est(r, fx)), 0), K - 1);
  float best = INFINITY;
  for (int j = max(kc - 2, 0); j <= min(kc + 2, K - 1); j++) {
    const float dx = fx - sib_wk_multi(r, j);
    if (dx * dx < best) { best = dx * dx; r.kbest = j; }
  }
  // dx^2 falls, then rises along the taps: climb to the minimum whatever the estimate was
  auto dx2 = [&](int j) { const float dx = fx - sib_wk_multi(r, j); return dx * dx; };
  while (r.kbest + 1 < K && dx2(r.kbest + 1) < dx2(r.kbest)) r.kbest++;
  while (r.kbest > 0 && dx2(r.kbest - 1) < dx2(r.kbest)) r.kbest--;
  return true;
}

FR_DEV SibRows sib_rows_setup(float fx, float w0, float wmax, float inc) {
  SibRows r;
  r.closed = false;
  r.multi = false;
  r.w0 = w0; r.delta = inc; r.inv = 0.0f; r.K = 0; r.kbest = 0;
  if (!(w0 > 0.0f) || !(wmax < 1.0f)) return r;
  if ((__float_as_uint(w0) >> 23) != (__float_as_uint(wmax) >> 23)) {
    SibMulti m;
    r.multi = sib_rows_multi(m, fx, w0, wmax, inc);
    return r;
  }
  const float w1 = w0 + inc;
  const float delta = w1 - w0;  // exact (Sterbenz)
  if ((w1 + inc) - w1 != delta) return r;
  r.closed = true;
  r.delta = delta;
  r.inv = __builtin_amdgcn_rcpf(delta);  // estimates only: every bound is corrected by exact tests
  int K = max((int)ceilf((wmax - w0) * r.inv), 0);
  while (sib_wk(r, K) < wmax) K++;
  while (K > 0 && !(sib_wk(r, K - 1) < wmax)) K--;
  r.K = K;
  if (K == 0) return r;
  const int kc = min(max((int)floorf((fx - w0) * r.inv), 0), K - 1);
  float best = INFINITY;
  for (int k = max(kc - 1, 0); k <= min(kc + 2, K - 1); k++) {
    const float dx = fx - sib_wk(r, k);
    if (dx * dx < best) { best = dx * dx; r.kbest = k; }
  }
  return r;
}

// The run [k0, k1] of the row with vertical term dy2; false: no tap of the row is in the disc. In the
// closed form dx_k = fx - w_k, and r2 = fl(fl(dx_k^2) + dy2) grows with |dx_k|, so the run is the taps with
// |dx_k| <= X for the row's half chord X. X is estimated as sqrt(r2max - dy2) in fp32: its error (a few
// ulps of r2max, spread over X) is far below the tap spacing delta for every radius the buckets allow, so
// the estimated ends ceil((fx - X - w0) / delta) and floor((fx + X - w0) / delta) are each off by at most
// one tap. The reference's own test at the estimate and its neighbour settles each end: four exact tests
// per row, no walk. (kbest, the tap nearest fx, decides whether the row has any tap.)
FR_DEV bool sib_row_run(const SibRows& r, float fx, float dy2, float r2max, int& k0, int& k1) {
  auto inside = [&](int k) {
    const float dx = fx - sib_wk(r, k);
    return dx * dx + dy2 <= r2max;
  };
  if (r.K == 0 || !inside(r.kbest)) return false;  // the nearest tap is out: all are
  const float chord = __builtin_amdgcn_sqrtf(fmaxf(r2max - dy2, 0.0f));
  const float c = fx - r.w0;
  // estimates clamped to [0, kbest] and [kbest, K - 1]; inside(kbest) holds, so a failed test at an
  // estimate other than kbest moves it one tap towards kbest
  const int a = min(max((int)ceilf((c - chord) * r.inv), 0), r.kbest);
  const int b = max(min((int)floorf((c + chord) * r.inv), r.K - 1), r.kbest);
  k0 = (a > 0 && inside(a - 1)) ? a - 1 : (inside(a) ? a : a + 1);
  k1 = (b < r.K - 1 && inside(b + 1)) ? b + 1 : (inside(b) ? b : b - 1);
  return true;
}

// sib_row_run for a multi-segment box: the same estimates (from the segment holding the chord's end) and the
// same exact tests, on the piecewise tap positions.
FR_DEV bool sib_row_run_multi(const SibMulti& r, float fx, float dy2, float r2max, int& k0, int& k1) {
  auto inside = [&](int k) {
    const float dx = fx - sib_wk_multi(r, k);
    return dx * dx + dy2 <= r2max;
  };
  if (r.K == 0 || !inside(r.kbest)) return false;
  const float chord = __builtin_amdgcn_sqrtf(fmaxf(r2max - dy2, 0.0f));
  int a = min(max((int)ceilf(sib_k_est(r, fx - chord)), 0), r.kbest);
  int b = max(min((int)floorf(sib_k_est(r, fx + chord)), r.K - 1), r.kbest);
  // (the estimate at a segment junction can be off by more than a tap: walk, exactly, towards the ends)
  while (a > 0 && inside(a - 1)) a--;
  while (!inside(a)) a++;
  while (b < r.K - 1 && inside(b + 1)) b++;
  while (!inside(b)) b--;
  k0 = a;
  k1 = b;
  return true;
}

// One pixel in run form. row.sum<INTERIOR>(j0, i0, n, w, a, b) returns the bilinear sum of the row's n taps:
// unwrapped texel row j0 in [-1, H-1] (and j0 + 1), first tap's texel column i0 in [-1, W-1] at
// position w, its 8-bit horizontal weight a, the row's vertical weight b.
//
// INTERIOR (the whole wave's boxes lie inside the image with a margin, and every pixel has the closed
// form: the usual case) drops the checks that cannot fire there: rows outside [0, 1), the texel-row
// wrap, the walk, and the per-tap border rows. The box margins: [1, W - 3] texels horizontally (the
// run's texel columns i0 .. i0 + n - 1 follow its taps to within a texel), [1, H - 2] vertically.
template <bool INTERIOR, class RowSum>
FR_DEV f4 sibson_rows_loop(const f4* __restrict__ color, int W, int H, f2 screen, f2 frag, f4 closest, float d,
                           const SibRows& rows, RowSum&& row) {
  const float r2max = sqrt_le_bound(d);
  f4 inc = mk4(0, 0, 0, 0);
  const f2 min_box = mk2(frag.x - d, frag.y - d);
  const f2 max_box = mk2(frag.x + d, frag.y + d);
  const f2 increment = mk2(1.0f / screen.x, 1.0f / screen.y);
  int k0 = -1, k1 = -1;  // the previous row's run (closed form)
  SibMulti multi;
  if (!INTERIOR && rows.multi) sib_rows_multi(multi, frag.x, min_box.x, max_box.x, increment.x);
  for (float h = min_box.y; h < max_box.y; h += increment.y) {
    if (!INTERIOR && (h < 0.0f || h >= 1.0f)) continue;
    const float dy = frag.y - h;
    const float dy2 = dy * dy;
    float w;
    int n;
    if (INTERIOR || rows.closed) {
      if (!sib_row_run(rows, frag.x, dy2, r2max, k0, k1)) continue;
      w = sib_wk(rows, k0);
      n = k1 - k0 + 1;
    } else if (rows.multi) {  // (the walk's run, found by its ends)
      if (!sib_row_run_multi(multi, frag.x, dy2, r2max, k0, k1)) continue;
      w = sib_wk_multi(multi, k0);
      n = k1 - k0 + 1;
    } else {
      w = min_box.x;
      while (w < max_box.x) {  // the row's first valid tap
        const float dx = frag.x - w;
        if (w >= 0.0f && w < 1.0f && dx * dx + dy2 <= r2max) break;
        w += increment.x;
      }
      if (!(w < max_box.x)) continue;
      // the run: taps while still inside the box, the texture and the disc
      n = 1;
      for (float w2 = w + increment.x; w2 < max_box.x && w2 < 1.0f; w2 += increment.x) {
        const float dx = frag.x - w2;
        if (dx * dx + dy2 > r2max) break;
        n++;
      }
    }
    const float ty = h * screen.y - 0.5f;
    const float fy0 = floorf(ty);
    float b = ty - fy0;
    b = floorf(b * 256.0f + 0.5f) * (1.0f / 256.0f);
    const float tx = w * screen.x - 0.5f;
    const float fx0 = floorf(tx);
    float a = tx - fx0;
    a = floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f);
    const f3 c = row.template sum<INTERIOR>((int)fy0, (int)fx0, n, w, a, b);
    inc = inc + mk4(c.x, c.y, c.z, (float)n);
  }
  if (inc.w > 0.0f) return mk4(inc.x / inc.w, inc.y / inc.w, inc.z / inc.w, 1.0f);
  uint32_t cx = f2u_sat(closest.x * screen.x), cy = f2u_sat(closest.y * screen.y);
  cx = min(cx, (uint32_t)W - 1); cy = min(cy, (uint32_t)H - 1);
  return color[(size_t)cy * W + cx];
}

FR_DEV float sib_radius(f2 frag, f4 closest) {  // distance(closest.st, FragCoord.st)
  const float cdx = closest.x - frag.x, cdy = closest.y - frag.y;
  return sqrtf(cdx * cdx + cdy * cdy);
}

template <class RowSum>
FR_DEV f4 sibson_pixel_runs(const f4* __restrict__ color, int W, int H, f2 screen, f2 frag, f4 closest, float d,
                            const SibRows& rows, RowSum&& row) {
  const bool interior = rows.closed && (frag.x - d) * screen.x >= 1.0f && (frag.x + d) * screen.x <= screen.x - 3.0f &&
                        (frag.y - d) * screen.y >= 1.0f && (frag.y + d) * screen.y <= screen.y - 2.0f;
  if (__ballot(interior) == __ballot(true))
    return sibson_rows_loop<true>(color, W, H, screen, frag, closest, d, rows, row);
  return sibson_rows_loop<false>(color, W, H, screen, frag, closest, d, rows, row);
}

// Row sums from the global per-row prefix arrays; rows whose taps wrap horizontally (the image's
// left and right borders) are summed per tap with the REPEAT wrap, as sibson_pixel does.
struct SibGlobalRows {
  const f4* __restrict__ color;
  const f4* __restrict__ P;
  const f4* __restrict__ T;
  int W, H, NB;
  float sx;
  // The run form of n taps from texel column i0 (columns i0 .. i0 + n, inside the row) on texel rows j0, j1.
  FR_DEV f3 prefix_sum(int j0, int j1, int i0, int n, float a, float b) const {
    // 32-bit element offsets from the kernel-argument bases (scalar base + vector offset loads)
    const char* Pb = reinterpret_cast<const char*>(P);
    const uint32_t e0 = (uint32_t)j0 * (uint32_t)(W + 1) + (uint32_t)i0;
    const uint32_t e1 = (uint32_t)j1 * (uint32_t)(W + 1) + (uint32_t)i0;
    const uint32_t un = (uint32_t)n;
    // the eight prefix loads first, all in flight together (sib_rowsum's T loop between them made
    // four dependent round trips of every row); then the block totals of a run that crosses a
    // 64-column block boundary, added in sib_rowsum's order: the same sums bit for bit
    const f3 a0 = rgb_at(Pb, e0), b0 = rgb_at(Pb, e0 + 1), c0 = rgb_at(Pb, e0 + un), d0 = rgb_at(Pb, e0 + un + 1);
    const f3 a1 = rgb_at(Pb, e1), b1 = rgb_at(Pb, e1 + 1), c1 = rgb_at(Pb, e1 + un), d1 = rgb_at(Pb, e1 + un + 1);
    f3 s0 = c0 - a0, t0 = d0 - b0, s1 = c1 - a1, t1 = d1 - b1;
    const int bA = i0 >> 6, eA = (i0 + n) >> 6, bB = (i0 + 1) >> 6, eB = (i0 + n + 1) >> 6;
    if (bA != eB) {
      // the two runs' blocks [bA, eA) and [bB, eB) overlap (bB <= bA + 1, eB <= eA + 1): each block total
      // is loaded once, for both, and added in increasing block order as before
      const char* Tb = reinterpret_cast<const char*>(T);
      const uint32_t t0r = (uint32_t)j0 * (uint32_t)NB, t1r = (uint32_t)j1 * (uint32_t)NB;
      for (int B = bA; B < eB; B++) {
        const f3 u0 = rgb_at(Tb, t0r + B), u1 = rgb_at(Tb, t1r + B);
        if (B < eA) { s0 = s0 + u0; s1 = s1 + u1; }
        if (B >= bB) { t0 = t0 + u0; t1 = t1 + u1; }
      }
    }
    const float na = 1.0f - a;
    const f3 r0 = s0 * na + t0 * a;
    const f3 r1 = s1 * na + t1 * a;
    return r0 * (1.0f - b) + r1 * b;
  }
  template <bool INTERIOR>
  FR_DEV f3 sum(int j0, int i0, int n, float w, float a, float b) const {
    const int j1 = INTERIOR || j0 + 1 != H ? j0 + 1 : 0;
    j0 = INTERIOR || j0 >= 0 ? j0 : H - 1;
    const float nb = 1.0f - b;
    if (INTERIOR || (i0 >= 0 && i0 + n <= W - 1)) return prefix_sum(j0, j1, i0, n, a, b);
    const char* cbase = reinterpret_cast<const char*>(color);
    const uint32_t o0 = (uint32_t)j0 * (uint32_t)W, o1 = (uint32_t)j1 * (uint32_t)W;
    const float inc = 1.0f / sx;
    f3 acc = mk3(0.0f);
    if (n > 4 && i0 >= 0 && i0 < W - 1) {
      // A long run whose texel span reaches the last column (the run form's columns i0 .. i0 + n - 1 drift
      // a column past the taps' own near the border): its taps up to column W - 2 from the prefix sums, the
      // last ones (whose right texel wraps) per tap at w + t / W. Walking all n taps here (hundreds, for the
      // wide discs of an off-centre gaze) held every wave with such a row for hundreds of loads.
      const int n1 = W - 1 - i0;
      acc = prefix_sum(j0, j1, i0, n1, a, b);
      w = __builtin_fmaf((float)n1, inc, w);
      n -= n1;
    }
    for (int k = 0; k < n; k++, w += inc) {
      const float txk = w * sx - 0.5f;
      const float fxk = floorf(txk);
      float ak = txk - fxk;
      ak = floorf(ak * 256.0f + 0.5f) * (1.0f / 256.0f);
      int l0 = (int)fxk;
      const int l1 = l0 + 1 == W ? 0 : l0 + 1;
      l0 = l0 < 0 ? W - 1 : l0;
      const f3 L0 = rgb_at(cbase, o0 + (uint32_t)l0), L1 = rgb_at(cbase, o1 + (uint32_t)l0);
      const f3 R0 = rgb_at(cbase, o0 + (uint32_t)l1), R1 = rgb_at(cbase, o1 + (uint32_t)l1);
      const float nak = 1.0f - ak;
      acc = acc + (L0 * (nak * nb) + R0 * (ak * nb) + L1 * (nak * b) + R1 * (ak * b));
    }
    return acc;
  }
};

// The run form over radius-ranked 16x16 tiles (fr_config.sibson_mode 0). 16x16 measured 1.06 ms at
// 4K against 1.19 for 32x32; staging the tiles' colour windows in LDS with their row prefix sums
// measured no faster than the global prefix arrays (1.06 against 1.07 ms): the row loads are not
// what bounds the kernel, the per-row membership arithmetic is.
#define SIBR_TILE 16
#define SIBR_THREADS (SIBR_TILE * SIBR_TILE)
#ifndef SIBR_WAVES
#define SIBR_WAVES 6  // waves per SIMD (80 VGPRs, 10 spilled): round 6 0.742 -> 0.708 ms against 7 (72 VGPRs, 15 spilled; spill stores
                      // were 82 MB of the kernel's 242 MB written); round 2: 7 beat the then unconstrained 75 VGPRs, 8 1.24 ms
#endif
#define SIBR_ATTR __attribute__((amdgpu_waves_per_eu(SIBR_WAVES, SIBR_WAVES)))

// Pixels whose box has no closed form (it crosses a binade edge of the tap positions: x = 0.5, 0.25, ...
// of the screen, or the image border) and spans more than 2 SIBW_MIN_HALF taps go to `wide` for
// k_sibson_wide instead of walking their taps row by row here: wide[0] / wide[1] count the discs of at
// most / more than 2 SIBW_BIG_HALF rows, listed from wide[2] upwards / from wide[2 + N - 1] downwards.
#define SIBW_MIN_HALF 12.0f
#define SIBW_BIG_HALF 64.0f
#ifndef SIBS_HALF
// d * H > SIBS_HALF: k_sibson_strip's pixels (more than 64 rows; 2 x 64 / 48 / 32 rows measured 3.83 / 3.78 / 3.70
// ms at the 180-degree gaze, 2.89 / 2.75 / 2.61 at 90, 1.42 / 1.30 / 1.20 at 45, the centred frame unchanged; 2 x 24
// within noise of 2 x 32, 2 x 16 slower on the centred frame: 0.78 against 0.74 ms; 2 x 24 with five cost classes:
// 1.11 / 2.53 / 3.71 ms at 45 / 90 / 180 degrees, centred 0.735)
#define SIBS_HALF 24.0f
#endif

// k_sibson_strip's work buffer, in uint32 words: [0] the strip count, [1] unused, the strip lists, one flag bit
// per strip, the texel-row range the big discs read (min, max), then per list its strip count and its claim
// counter (a 128-B line each). A strip is listed once, by the first of its pixels k_sibson_runs finds big, in
// list SIBS_CLS x c + xs % 8: c its cost class (that pixel's disc height: the strip's widest disc sets its trip
// count, and its neighbours' are alike), xs its 64-column band. Blocks claim the costliest class first, the
// lists of their own XCD (blockIdx % 8) first within a class (the blocks sharing an L2 take the same bands, whose
// vertically neighbouring discs read the same prefix rows): the long strips start first, and the launch does
// not end on one.
#ifndef SIBS_CLS
#define SIBS_CLS 5  // (4 classes, without the one at 64 half-rows: 45 / 90 / 180 degrees 1.20 / 2.64 / 3.75 ms against
                    // 1.17 / 2.58 / 3.71 with 5, profiles/r05_sibson/cl5_*)
#endif
#define SIBS_LISTS (8 * SIBS_CLS)
FR_DEV int sibs_cost_class(float half_rows) {  // d * H of the strip's first big pixel -> 0 (costliest) ..
  // classes at 320, 192, 112 (and 64 with SIBS_CLS 5) half-rows; the last class holds the rest
  const int c = half_rows >= 320.0f ? 0 : half_rows >= 192.0f ? 1 : half_rows >= 112.0f ? 2 : half_rows >= 64.0f ? 3 : 4;
  return min(c, SIBS_CLS - 1);
}
struct StripLayout {
  uint32_t s64, n, cap, list, flags, rows, xcnt, xclaim, total;
  __host__ __device__ StripLayout(int W, int H) {
    s64 = (uint32_t)((W + 63) / 64);
    n = s64 * (uint32_t)H;
    cap = ((s64 + 7) / 8) * (uint32_t)H;  // a list's most strips
    list = 2;
    flags = list + SIBS_LISTS * cap;
    rows = flags + (n + 31) / 32;
    xcnt = (rows + 2 + 31) & ~31u;
    xclaim = xcnt + SIBS_LISTS * 32;
    total = xclaim + SIBS_LISTS * 32;
  }
};

// The pixel's seed (closest.st): from the JFA result `coord`, or (STATE) from the final 8-byte JFA state itself,
// decoded exactly as k_jfa_final_prefix writes coord.xy (the same two values, bit for bit; half the bytes).
template <bool STATE>
FR_DEV f2 sib_seed(const f4* __restrict__ coord, const u2* __restrict__ state, int W, int x, int y, f2 screen) {
  const uint32_t p = (uint32_t)y * (uint32_t)W + (uint32_t)x;
  if (!STATE) {
    const f4 c = coord[p];
    return mk2(c.x, c.y);
  }
  const u2 s = state[p];
  return mk2(jfa_seeded(s.x) ? jfa_coord(s.x) : ((float)x + 0.5f) / screen.x, jfa_coord(s.y));
}

// Traffic (round 6): every pixel's seed is read once, in raster order (the radius ranking needs it), and kept
// in LDS for the lane that takes the pixel in ranked order (which re-read coord before). Tiles are handed to the
// XCDs in super-tiles (below), so the prefix rows neighbouring tiles share are fetched into one L2.
// (Measured and not kept, round 6: the tiles in raster order or in one contiguous band per XCD (xcd_tile) instead of
// super-tiles; the results staged in LDS at their raster slot and stored row by row, instead of each lane storing
// its pixel in radius order; the seeds read from JFA_COORD while the final JFA state is at hand.)
template <bool STATE>
__global__ __launch_bounds__(SIBR_THREADS) SIBR_ATTR void k_sibson_runs(const f4* __restrict__ coord,
                                                              const u2* __restrict__ state,
                                                              const f4* __restrict__ color,
                                                              const f4* __restrict__ P, const f4* __restrict__ T,
                                                              f4* __restrict__ out, uint32_t* __restrict__ wide,
                                                              uint32_t* __restrict__ strips, int W, int H, int NB,
                                                              f2 screen, float strip_half, int mid, uint32_t tiles_x,
                                                              uint32_t tiles_y) {
  __shared__ uint32_t bucket[SIB_BUCKETS];
  __shared__ uint16_t order[SIBR_THREADS];
  __shared__ f4 slot[SIBR_THREADS];      // raster slot: the pixel's (seed.x, seed.y, d)
  __shared__ uint8_t done[SIBR_THREADS];  // cleared and never read (left from the LDS-staged store). Measured without
                                          // it: Sibson alone 0.711 ms against 0.708 with it, the latter's spread
                                          // 0.3 %: no gain to show, so it stays (MEASUREMENTS.md, JFA reuse)
  const int tid = threadIdx.x;
  // super-tiles of 4 x 4 tiles: the 16 blocks of one super-tile are dispatched to one XCD one after another (block b
  // runs on XCD b % 8), so the prefix rows its tiles share are fetched into one L2; consecutive super-tiles of the
  // raster order go to different XCDs, so every XCD's work spreads over the whole image (horizontal bands per XCD
  // load the XCDs unevenly: the fovea's discs are small, the periphery's large). 1-D grid; blocks past the image exit.
  const uint32_t sgx = (tiles_x + 3) / 4;
  const uint32_t b = blockIdx.x, sup = (b / 128) * 8 + (b % 8), sub = (b / 8) % 16;
  const uint32_t tx = (sup % sgx) * 4 + (sub % 4), ty = (sup / sgx) * 4 + (sub / 4);
  if (tx >= tiles_x || ty >= tiles_y) return;
  const int bx0 = (int)tx * SIBR_TILE, by0 = (int)ty * SIBR_TILE;
  for (int i = tid; i < SIB_BUCKETS; i += SIBR_THREADS) bucket[i] = 0;
  done[tid] = 0;
  __syncthreads();
  const int x = bx0 + (tid % SIBR_TILE), y = by0 + (tid / SIBR_TILE);
  int key = -1;
  if (x < W && y < H) {
    const f2 frag = frag_uv(x, y, screen);
    const f2 c = sib_seed<STATE>(coord, state, W, x, y, screen);
    const float d = sib_radius(frag, mk4(c.x, c.y, 0.0f, 0.0f));
    slot[tid] = mk4(c.x, c.y, d, 0.0f);
    const float r = d * fmaxf(screen.x, screen.y);
    key = r < (float)(SIB_BUCKETS - 1) ? (int)r : SIB_BUCKETS - 1;
    atomicAdd(&bucket[key], 1u);
  }
  __syncthreads();
  if (tid < 64) {
    const uint32_t v0 = bucket[2 * tid], v1 = bucket[2 * tid + 1];
    uint32_t incl = v0 + v1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (tid >= o) incl += t;
    }
    bucket[2 * tid] = incl - v0 - v1;
    bucket[2 * tid + 1] = incl - v1;
  }
  __syncthreads();
  if (key >= 0) order[atomicAdd(&bucket[key], 1u)] = (uint16_t)tid;
  __syncthreads();
  const int n = (int)bucket[SIB_BUCKETS - 1];
  // lanes past the tile's pixel count take part in the wave-wide steps below with nothing to do (no early
  // exit before them: the big discs' row range is reduced over the whole wave)
  const bool live = tid < n;
  const int p = live ? order[tid] : 0;
  const int px = bx0 + (p % SIBR_TILE), py = by0 + (p / SIBR_TILE);
  const f2 frag = frag_uv(px, py, screen);
  const f4 sd = slot[p];
  const f4 closest = mk4(sd.x, sd.y, 0.0f, 0.0f);
  const float d = sd.z;
  const SibRows rows = sib_rows_setup(frag.x, frag.x - d, frag.x + d, 1.0f / screen.x);
  // k_sibson_strip's pixels (its own test): the big discs, and with `mid` the other wide discs too
  const bool big = live && (d * screen.y > strip_half || (mid && !rows.closed && d * screen.x > SIBW_MIN_HALF));
  const bool go = live && !big && !rows.closed && !rows.multi && d * screen.x > SIBW_MIN_HALF;
  const bool large = d * screen.y > SIBW_BIG_HALF;  // (without the strip kernel) k_sibson_wide<64>'s list
  const int lane = tid & 63;
  if (__ballot(big)) {
    // the texel rows the big discs read (k_sibson_rowp builds the whole-row prefixes of those only): a
    // disc of tap rows h in [y - d, y + d) reads texel rows floor(h H - 0.5) and the next; a disc near the
    // top or bottom edge also reads the wrapped row, so it asks for every row
    const float lo = (frag.y - d) * screen.y, hi = (frag.y + d) * screen.y;
    const bool edge = lo < 2.0f || hi > screen.y - 3.0f;
    int ylo = big ? (edge ? 0 : (int)floorf(lo) - 2) : INT_MAX, yhi = big ? (edge ? H - 1 : (int)ceilf(hi) + 2) : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ylo = min(ylo, __shfl_xor(ylo, o, 64)); yhi = max(yhi, __shfl_xor(yhi, o, 64)); }
    const StripLayout L(W, H);
    const uint32_t S64 = L.s64;
    uint32_t* flags = strips + L.flags;
    uint32_t* rowr = strips + L.rows;
    if (lane == __ffsll((unsigned long long)__ballot(big)) - 1) {
      atomicMin(&rowr[0], (uint32_t)max(ylo, 0));
      atomicMax(&rowr[1], (uint32_t)min(yhi, H - 1));
    }
    if (big) {  // this pixel's strip (64 pixels of its row) goes to k_sibson_strip's list, once
      const uint32_t strip = (uint32_t)py * S64 + (uint32_t)(px >> 6);
      if (!(atomicOr(&flags[strip >> 5], 1u << (strip & 31)) & (1u << (strip & 31)))) {
        const uint32_t lst = (uint32_t)sibs_cost_class(d * screen.y) * 8u + ((uint32_t)(px >> 6) & 7u);
        strips[L.list + lst * L.cap + atomicAdd(&strips[L.xcnt + lst * 32], 1u)] = strip;
        atomicAdd(&strips[0], 1u);
      }
    }
  }
  const uint32_t N = (uint32_t)W * (uint32_t)H;
#pragma unroll
  for (int list = 0; list < 2; list++) {  // the other wide discs (no closed form, more than 2 SIBW_MIN_HALF taps)
    const bool mine = go && large == (list == 1);
    const uint64_t bal = __ballot(mine);
    if (!bal) continue;
    const int leader = __ffsll((unsigned long long)bal) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&wide[list], (uint32_t)__popcll(bal));
    base = __shfl(base, leader, 64);
    const uint32_t at = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (mine) wide[list == 0 ? 2 + at : 2 + N - 1 - at] = (uint32_t)py * (uint32_t)W + (uint32_t)px;
  }
  if (live && !big && !go) {
    const f4 r = sibson_pixel_runs(color, W, H, screen, frag, closest, d, rows, SibGlobalRows{color, P, T, W, H, NB, screen.x});
    out[(size_t)py * W + px] = r;
  }
}

// ------------------------------------------------------------------------------------------
// Sibson, wide discs (run form). The log-polar mask of an off-centre gaze leaves holes hundreds of
// texels wide (scripts/gaze_probe.py: discs of up to 1,137 rows at 4K), and a pixel there whose box
// crosses a binade edge of its tap positions has no single-step closed form: sibson_rows_loop would
// walk its taps row by row, O(d^2) per pixel (150-430 ms per 4K frame at such gazes). Here each such
// pixel gets a wave:
// - the reference's tap positions along each axis (v_{k+1} = fl(v_k + 1/W) from min_box, while
//   v < max_box) as a table of segments: runs of equal steps inside one binade, v_k = v_s + (k - k_s)
//   delta exactly (built once per pixel, in LDS, the same for every lane);
// - the pixel's rows spread over the lanes; a row's run of valid taps from the chord estimate,
//   settled by the reference's own test, and summed per segment from the row prefix sums (the run
//   form's rounding-level approximation, as in sibson_rows_loop);
// - the lanes' partial sums added with shuffles.
// ------------------------------------------------------------------------------------------
#define SIBW_SEGS 64      // a 4K box needs at most 28
#define SIBW_WAVES 4      // waves per block
#define SIBW_BLOCKS 1024  // 4 waves per SIMD (99 VGPRs)

FR_DEV bool sib_same_binade(float a, float b) { return (__float_as_uint(a) >> 23) == (__float_as_uint(b) >> 23); }

// The largest m >= 0 with v + j delta (exact) in v's binade (sign and exponent) for every j <= m.
FR_DEV int sib_binade_steps(float v, float delta) {
  const uint32_t bits = __float_as_uint(v);
  // positive v: below 2^(E+1); negative v: at most -2^E
  const float edge = v > 0.0f ? __uint_as_float(((bits >> 23) + 1u) << 23) : __uint_as_float(bits & 0xFF800000u);
  int m = (int)fminf(fmaxf(floorf((edge - v) * __builtin_amdgcn_rcpf(delta)), 0.0f), 1.0e8f);  // estimate
  while (m > 0 && !sib_same_binade(__builtin_fmaf((float)m, delta, v), v)) m--;
  while (sib_same_binade(__builtin_fmaf((float)(m + 1), delta, v), v)) m++;
  return m;
}

// The number of j >= 0 with v + j delta < lim (v < lim), for j inside v's binade (exact there).
FR_DEV int sib_count_below(float v, float delta, float lim) {
  int j = (int)fminf(fmaxf(ceilf((lim - v) * __builtin_amdgcn_rcpf(delta)), 1.0f), 1.0e8f);  // estimate
  while (j > 1 && !(__builtin_fmaf((float)(j - 1), delta, v) < lim)) j--;
  while (__builtin_fmaf((float)j, delta, v) < lim) j++;
  return j;
}

// One axis' tap table: segment s holds taps k[s] .. k[s+1]-1 at v[s] + (tap - k[s]) d[s].
struct SibAxis {
  int* k;
  float* v;
  float* d;
  int ns, K;  // segments; taps (v_k < vmax for k < K); K < 0: more than SIBW_SEGS segments
};

// for (v = v0; v < vmax; v += inc): the reference's loop, one segment per run of equal steps. Within a
// binade every v is a multiple of its ulp u, so fl(v + inc) - v is inc rounded to a multiple of u: the
// same step for every tap (a rounding tie fixes its parity after one step: the first two steps are
// compared, and a segment whose first two differ keeps one tap). Only the last step inside the binade
// can round at the next binade's spacing: it is checked with the reference's own addition.
FR_DEV void sib_axis_build(SibAxis& A, float v0, float vmax, float inc, bool store) {
  int k = 0, ns = 0;
  float v = v0;
  while (v < vmax) {
    if (ns == SIBW_SEGS) { A.K = -1; A.ns = ns; return; }
    const float v1 = v + inc, v2 = v1 + inc;
    const float delta = v1 - v;
    int m = 0;
    if (v != 0.0f && sib_same_binade(v, v2) && v2 - v1 == delta && delta > 0.0f) {
      m = min(sib_binade_steps(v, delta), sib_count_below(v, delta, vmax) - 1);
      if (m >= 1 && __builtin_fmaf((float)(m - 1), delta, v) + inc != __builtin_fmaf((float)m, delta, v)) m--;
    }
    if (store) { A.k[ns] = k; A.v[ns] = v; A.d[ns] = delta; }
    ns++;
    k += m + 1;
    v = __builtin_fmaf((float)m, delta, v) + inc;  // the reference's step from the segment's last tap
  }
  if (store) A.k[ns] = k;
  A.ns = ns;
  A.K = k;
}

FR_DEV int sib_seg_of(const SibAxis& A, int k) {  // the segment holding tap k (0 <= k < K)
  int lo = 0, hi = A.ns - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.k[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}
FR_DEV float sib_tap(const SibAxis& A, int k) {
  const int s = sib_seg_of(A, k);
  return __builtin_fmaf((float)(k - A.k[s]), A.d[s], A.v[s]);
}
// The first tap at or after position p (exact), in [0, K].
FR_DEV int sib_first_ge(const SibAxis& A, float p) {
  int lo = 0, hi = A.ns - 1;  // the last segment starting at or before p (estimate)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.v[mid] <= p) lo = mid; else hi = mid - 1;
  }
  int k = A.k[lo];
  if (A.v[lo] < p) k += (int)fminf(fmaxf(ceilf((p - A.v[lo]) * __builtin_amdgcn_rcpf(A.d[lo])), 0.0f), 1.0e8f);
  k = min(max(k, A.k[lo]), A.k[lo + 1]);
  while (k > 0 && !(sib_tap(A, k - 1) < p)) k--;
  while (k < A.K && sib_tap(A, k) < p) k++;
  return k;
}

// LDS written by lane 0 and read by the wave's other lanes (each wave has its own tables)
FR_DEV void sib_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Measured and not kept (4K, 180-degree gaze, 27-29 ms here): a contiguous chunk of rows per lane with
// segment cursors instead of binary searches (47 ms: the rows outside the image and the long equator
// runs fall on a few lanes), block totals from a per-row prefix over the blocks, and both tables built
// in one lane-parallel pass (27 ms, but 139-151 VGPRs and 0.5-0.6 instead of 0.35-0.45 ms on a
// centred-gaze frame). The kernel is bound by its scattered 12-byte prefix loads: a wave's 64 lanes
// read 64 different rows, one cache line per lane and load.
template <int SIBW_LANES, int LIST>
__global__ __launch_bounds__(64 * SIBW_WAVES) void k_sibson_wide(const f4* __restrict__ coord,
                                                                 const f4* __restrict__ color,
                                                                 const f4* __restrict__ P, const f4* __restrict__ T,
                                                                 f4* __restrict__ out,
                                                                 const uint32_t* __restrict__ wide, int W, int H,
                                                                 int NB, f2 screen, const u2* __restrict__ state,
                                                                 int coord_owed) {
  constexpr int SIBW_PER_WAVE = 64 / SIBW_LANES;
  __shared__ int skk[SIBW_WAVES * SIBW_PER_WAVE][2][SIBW_SEGS + 1];
  __shared__ float svv[SIBW_WAVES * SIBW_PER_WAVE][2][SIBW_SEGS], sdd[SIBW_WAVES * SIBW_PER_WAVE][2][SIBW_SEGS];
  // SIBW_PER_WAVE pixels per wave, SIBW_LANES lanes each: 16 for the discs of at most 128 rows (a
  // centred-gaze frame's wide pixels have 20-40 rows: a whole wave per pixel left half of it idle and paid
  // the table build once per 64 lanes; Sibson 0.93 -> 0.79 ms alone at 4K), 64 for the larger ones (16
  // lanes each measured 34 -> 47 ms at the 180-degree gaze: four discs of unequal size per wave)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int grp = lane / SIBW_LANES, gl = lane % SIBW_LANES;
  const int slot = wv * SIBW_PER_WAVE + grp;
  int(*sk)[SIBW_SEGS + 1] = skk[slot];
  float(*sv)[SIBW_SEGS] = svv[slot];
  float(*sd)[SIBW_SEGS] = sdd[slot];
  const uint32_t count = wide[LIST];
  const uint32_t N = (uint32_t)W * (uint32_t)H;
  const SibGlobalRows row{color, P, T, W, H, NB, screen.x};
  // every wave leaves after the list's end
  for (uint32_t base = (blockIdx.x * SIBW_WAVES + wv) * SIBW_PER_WAVE; base < count;
       base += gridDim.x * SIBW_WAVES * SIBW_PER_WAVE) {
    // a group past the list's end recomputes the wave's first pixel and writes nothing (the loop and the
    // shuffles stay uniform over the wave)
    const bool mine = base + grp < count;
    const uint32_t at = mine ? base + grp : base;
    const uint32_t p = wide[LIST == 0 ? 2 + at : 2 + N - 1 - at];
    const int x = (int)(p % (uint32_t)W), y = (int)(p / (uint32_t)W);
    const f2 frag = frag_uv(x, y, screen);
    // (coord_owed: JFA_COORD not written, the seeds from the final JFA state)
    const f2 cs = coord_owed ? sib_seed<true>(coord, state, W, x, y, screen) : sib_seed<false>(coord, state, W, x, y, screen);
    const f4 closest = mk4(cs.x, cs.y, 0.0f, 0.0f);
    const float d = sib_radius(frag, closest);
    const float r2max = sqrt_le_bound(d);
    SibAxis X{sk[0], sv[0], sd[0], 0, 0}, Y{sk[1], sv[1], sd[1], 0, 0};
    sib_axis_build(X, frag.x - d, frag.x + d, 1.0f / screen.x, gl == 0);
    sib_axis_build(Y, frag.y - d, frag.y + d, 1.0f / screen.y, gl == 0);
    sib_wave_sync();
    f4 acc = mk4(0, 0, 0, 0);
    if (X.K < 0 || Y.K < 0) {  // more segments than the table holds (not reached for W, H < 2^16): walk
      if (gl == 0 && mine) {
        const SibRows walk{false, 0.0f, 0.0f, 0.0f, 0, 0};
        out[p] = sibson_rows_loop<false>(color, W, H, screen, frag, closest, d, walk, row);
      }
      sib_wave_sync();
      continue;
    }
    // taps inside [0, 1) horizontally, and the one nearest frag.x (the disc's runs contain it)
    const int kz = sib_first_ge(X, 0.0f), ko = sib_first_ge(X, 1.0f);
    int kbest = min(sib_first_ge(X, frag.x), X.K - 1);
    if (kbest > 0) {
      const float a = frag.x - sib_tap(X, kbest - 1), b = frag.x - sib_tap(X, kbest);
      if (a * a < b * b) kbest--;
    }
    auto inside = [&](int k, float dy2) {
      const float dx = frag.x - sib_tap(X, k);
      return dx * dx + dy2 <= r2max;
    };
    for (int j = gl; j < Y.K && X.K > 0 && kz < ko; j += SIBW_LANES) {
      const float h = sib_tap(Y, j);
      if (h < 0.0f || h >= 1.0f) continue;
      const float dy = frag.y - h;
      const float dy2 = dy * dy;
      if (!inside(kbest, dy2)) continue;  // the nearest tap is out: all are
      const float chord = __builtin_amdgcn_sqrtf(fmaxf(r2max - dy2, 0.0f));
      int k0 = min(sib_first_ge(X, frag.x - chord), kbest);
      if (inside(k0, dy2)) { while (k0 > 0 && inside(k0 - 1, dy2)) k0--; }
      else { do k0++; while (!inside(k0, dy2)); }
      int k1 = max(sib_first_ge(X, frag.x + chord) - 1, kbest);
      k1 = min(k1, X.K - 1);
      if (inside(k1, dy2)) { while (k1 < X.K - 1 && inside(k1 + 1, dy2)) k1++; }
      else { do k1--; while (!inside(k1, dy2)); }
      k0 = max(k0, kz);
      k1 = min(k1, ko - 1);
      if (k0 > k1) continue;
      const float ty = h * screen.y - 0.5f;
      const float fy0 = floorf(ty);
      float b = ty - fy0;
      b = floorf(b * 256.0f + 0.5f) * (1.0f / 256.0f);
      const int j0 = (int)fy0;
      auto texel = [&](float w, int& i, float& a) {
        const float tx = w * screen.x - 0.5f;
        const float fx0 = floorf(tx);
        a = tx - fx0;
        a = floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f);
        i = (int)fx0;
      };
      f3 c = mk3(0.0f);
      int ri = 0, rn = 0;  // the pending run, merged across segment edges where the columns and weight continue
      float ra = 0.0f, rw = 0.0f;
      for (int k = k0; k <= k1;) {  // one part per segment the run crosses
        const int s = sib_seg_of(X, k);
        const int kend = min(k1, X.k[s + 1] - 1);
        int n = kend - k + 1;
        float w = __builtin_fmaf((float)(k - X.k[s]), X.d[s], X.v[s]);
        int i0;
        float a;
        texel(w, i0, a);
        if (i0 < 0) {  // the left border tap (texel column -1 wraps): on its own
          c = c + row.template sum<false>(j0, i0, 1, w, a, b);
          n--;
          w = __builtin_fmaf((float)(k + 1 - X.k[s]), X.d[s], X.v[s]);
          texel(w, i0, a);
        }
        if (n > 0) {
          const float wl = __builtin_fmaf((float)(kend - X.k[s]), X.d[s], X.v[s]);
          int il;
          float al;
          texel(wl, il, al);
          if (il >= W - 1) {  // the right border tap (its right column wraps): on its own
            c = c + row.template sum<false>(j0, il, 1, wl, al, b);
            n--;
          }
        }
        if (n > 0) {
          if (rn > 0 && i0 == ri + rn && a == ra) {
            rn += n;
          } else {
            if (rn > 0) c = c + row.template sum<false>(j0, ri, rn, rw, ra, b);
            ri = i0; rn = n; ra = a; rw = w;
          }
        }
        k = kend + 1;
      }
      if (rn > 0) c = c + row.template sum<false>(j0, ri, rn, rw, ra, b);
      acc = acc + mk4(c.x, c.y, c.z, (float)(k1 - k0 + 1));
    }
#pragma unroll
    for (int o = SIBW_LANES / 2; o > 0; o >>= 1) {
      acc.x += __shfl_xor(acc.x, o, 64);
      acc.y += __shfl_xor(acc.y, o, 64);
      acc.z += __shfl_xor(acc.z, o, 64);
      acc.w += __shfl_xor(acc.w, o, 64);
    }
    if (gl == 0 && mine) {
      f4 o;
      if (acc.w > 0.0f) {
        o = mk4(acc.x / acc.w, acc.y / acc.w, acc.z / acc.w, 1.0f);
      } else {
        uint32_t cx = f2u_sat(closest.x * screen.x), cy = f2u_sat(closest.y * screen.y);
        cx = min(cx, (uint32_t)W - 1); cy = min(cy, (uint32_t)H - 1);
        o = color[(size_t)cy * W + cx];
      }
      out[p] = o;
    }
    sib_wave_sync();  // the tables are rebuilt for the next pixel
  }
}

// ------------------------------------------------------------------------------------------
// Sibson, big discs (more than 2 SIBS_HALF rows, closed form or not): a wave per 64-pixel strip of an
// image row, a lane per pixel. k_sibson_wide gives each such pixel a wave whose lanes take its rows, so
// each prefix load of a wave touches 64 different image rows (64 cache lines); this was 16-34 ms of
// Sibson at the 90-180 degree probe gazes, whose log-polar masks leave holes hundreds of texels wide.
// Here the lanes are neighbouring pixels of one row, aligned on their first texel row: in every step of
// the loop they sum a run of the same image row (or one of two, with the bilinear pair) at neighbouring
// columns, so their prefix loads share cache lines. Each lane still follows its own pixel exactly as
// k_sibson_wide does:
// - its tap rows are the reference's own loop, h += 1/H from min_box.y, one per step;
// - its tap columns come from its own segment table (sib_axis_build's segments, only those holding taps
//   in [0, 1): at most 13 for a 4K box; a pixel needing more than SIBS_SEGS goes to k_sibson_wide);
// - a row's run is settled by the reference's test at its ends and summed per segment from whole-row
//   prefix sums (k_sibson_rowp: eight loads per row whatever the run's length, where k_sibson_wide adds
//   the run's block totals one by one).
// The sums are those of k_sibson_wide up to rounding (the whole-row prefixes' last bits, averaged over
// the disc's taps).
// ------------------------------------------------------------------------------------------
#define SIBS_SEGS 16
#ifndef SIBS_WAVES
#define SIBS_WAVES 4  // waves per block, all on one strip (a power of two)
#endif
#ifndef SIBS_OCC
#define SIBS_OCC 4
#endif

// G[j][i] = the sum of row j's colours in columns 0 .. i-1 (i = 0 .. W): the block prefix P plus the block
// totals before it. A block per row; nothing to do when k_sibson_runs listed no strip. Sums of that size lose
// more bits than P's block-local ones (an ulp of the row's total, ~2^-24 of W colours), which a big disc's
// average over more than 2 SIBS_HALF rows of runs divides by its tap count.
#define SIBG_THREADS 256
#define SIBG_MAX_BLOCKS 1024  // W < 65472 (launch_sibson_runs keeps k_sibson_wide for wider frames)
__global__ __launch_bounds__(SIBG_THREADS) void k_sibson_rowp(const f4* __restrict__ P, const f4* __restrict__ T,
                                                              f4* __restrict__ G, const uint32_t* __restrict__ strips,
                                                              int W, int NB) {
  __shared__ float tt[3][SIBG_MAX_BLOCKS];
  if (strips[0] == 0) return;
  const int tid = threadIdx.x, j = blockIdx.x;
  const uint32_t* rows = strips + StripLayout(W, gridDim.x).rows;  // (a block per image row)
  if ((uint32_t)j < rows[0] || (uint32_t)j > rows[1]) return;  // no big disc reads this row
  if (tid < 64) {  // the exclusive prefix of the row's block totals, 64 blocks at a time
    f3 carry = mk3(0.0f);
    for (int B0 = 0; B0 < NB; B0 += 64) {
      const int B = B0 + tid;
      const f3 v = B < NB ? xyz(T[(size_t)j * NB + B]) : mk3(0.0f);
      f3 incl = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float tx = __shfl_up(incl.x, o, 64), ty = __shfl_up(incl.y, o, 64), tz = __shfl_up(incl.z, o, 64);
        if (tid >= o) incl = incl + mk3(tx, ty, tz);
      }
      if (B < NB) {
        const f3 e = carry + (incl - v);
        tt[0][B] = e.x; tt[1][B] = e.y; tt[2][B] = e.z;
      }
      carry = carry + mk3(__shfl(incl.x, 63, 64), __shfl(incl.y, 63, 64), __shfl(incl.z, 63, 64));
    }
  }
  __syncthreads();
  const size_t row = (size_t)j * (W + 1);
  for (int i = tid; i <= W; i += SIBG_THREADS) {
    const int B = i >> 6;
    G[row + i] = mk4(xyz(P[row + i]) + mk3(tt[0][B], tt[1][B], tt[2][B]), 0.0f);
  }
}

// A lane's tap table in LDS, segment s at [s * 64 + lane] (conflict-free when the lanes read the same s).
// A segment's step is its first one, fl(v + inc) - v (sib_axis_build's delta), recomputed rather than
// stored: two tables per lane instead of three, which leaves the LDS for 4 waves per SIMD.
struct SibLaneAxis {
  int* k;     // SIBS_SEGS + 1 entries: the first tap of each stored segment, then the end of the last one
  float* v;   // SIBS_SEGS
  float inc;  // 1 / W
  int ns;     // stored segments (-1: more than SIBS_SEGS hold taps in [0, 1))
  FR_DEV int K(int s) const { return k[s * 64]; }
  FR_DEV float V(int s) const { return v[s * 64]; }
  FR_DEV float D(int s) const { const float x = V(s); return (x + inc) - x; }
};

// sib_axis_build's segments, keeping those with a tap in [0, 1) (the only taps a row sums).
FR_DEV void sls_build(SibLaneAxis& A, float v0, float vmax, float inc) {
  int k = 0, ns = 0;
  float v = v0;
  while (v < vmax && v < 1.0f) {
    const float v1 = v + inc, v2 = v1 + inc;
    const float delta = v1 - v;
    int m = 0;
    if (v != 0.0f && sib_same_binade(v, v2) && v2 - v1 == delta && delta > 0.0f) {
      m = min(sib_binade_steps(v, delta), sib_count_below(v, delta, vmax) - 1);
      if (m >= 1 && __builtin_fmaf((float)(m - 1), delta, v) + inc != __builtin_fmaf((float)m, delta, v)) m--;
    }
    const float last = __builtin_fmaf((float)m, delta, v);
    if (last >= 0.0f) {
      if (ns == SIBS_SEGS) { A.ns = -1; return; }
      A.k[ns * 64] = k; A.v[ns * 64] = v;
      ns++;
    }
    k += m + 1;
    v = last + inc;  // the reference's step from the segment's last tap
  }
  A.k[ns * 64] = k;
  A.ns = ns;
}

FR_DEV int sls_seg_of(const SibLaneAxis& A, int k) {  // the stored segment holding tap k
  int lo = 0, hi = A.ns - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.K(mid) <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}
FR_DEV float sls_tap(const SibLaneAxis& A, int k) {
  const int s = sls_seg_of(A, k);
  return __builtin_fmaf((float)(k - A.K(s)), A.D(s), A.V(s));
}
// The first stored tap at or after position p, in [A.K(0), A.K(ns)].
FR_DEV int sls_first_ge(const SibLaneAxis& A, float p) {
  int lo = 0, hi = A.ns - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.V(mid) <= p) lo = mid; else hi = mid - 1;
  }
  int k = A.K(lo);
  if (A.V(lo) < p) k += (int)fminf(fmaxf(ceilf((p - A.V(lo)) * __builtin_amdgcn_rcpf(A.D(lo))), 0.0f), 1.0e8f);
  k = min(max(k, A.K(lo)), A.K(lo + 1));
  const int k_lo = A.K(0), k_hi = A.K(A.ns);
  while (k > k_lo && !(sls_tap(A, k - 1) < p)) k--;
  while (k < k_hi && sls_tap(A, k) < p) k++;
  return k;
}

// One stored segment of a lane's table held in registers: taps [k0, k1) at v + (k - k0) d. tap() moves it
// to the segment holding k (a neighbouring one, in practice) and returns the tap's position.
struct SibCursor {
  int s = 0, k0 = 0, k1 = 0;
  float v = 0.0f, d = 0.0f, vn = 0.0f;  // vn: the next stored segment's start (+inf after the last)
  FR_DEV void load(const SibLaneAxis& A, int seg) {
    s = seg; k0 = A.K(seg); k1 = A.K(seg + 1); v = A.V(seg); d = (v + A.inc) - v;
    vn = seg + 1 < A.ns ? A.V(seg + 1) : INFINITY;
  }
  FR_DEV float at(int k) const { return __builtin_fmaf((float)(k - k0), d, v); }
  FR_DEV float tap(const SibLaneAxis& A, int k) {
    if (k < k0 || k >= k1) {  // (rare: one range test on the common path, the walk only when it fails)
      while (k < k0) load(A, s - 1);
      while (k >= k1) load(A, s + 1);
    }
    return at(k);
  }
  // The tap at or just after position p, estimated from the segment holding p (within a tap or two of
  // sls_first_ge's exact answer; the caller settles it), in [A.K(0), A.K(ns)].
  FR_DEV int near(const SibLaneAxis& A, float p) {
    if ((s > 0 && p < v) || p >= vn) {  // (registers only: no table read unless the segment changes)
      while (s > 0 && p < v) load(A, s - 1);
      while (p >= vn) load(A, s + 1);
    }
    int k = k0;
    if (v < p) k += (int)fminf(ceilf((p - v) * __builtin_amdgcn_rcpf(d)), 1.0e8f);
    return min(k, k1);
  }
  // sls_first_ge from the cursor's segment: the first stored tap at or after p, in [A.K(0), A.K(ns)]
  FR_DEV int first_ge(const SibLaneAxis& A, float p) {
    while (s > 0 && p < v) load(A, s - 1);
    while (s < A.ns - 1 && p >= A.V(s + 1)) load(A, s + 1);
    int k = k0;
    if (v < p) k += (int)fminf(fmaxf(ceilf((p - v) * __builtin_amdgcn_rcpf(d)), 0.0f), 1.0e8f);
    k = min(max(k, k0), k1);
    const int k_lo = A.K(0), k_hi = A.K(A.ns);
    while (k > k_lo && !(tap(A, k - 1) < p)) k--;
    while (k < k_hi && tap(A, k) < p) k++;
    return k;
  }
};

// Row sums from the whole-row prefix sums G: eight loads per row whatever the run's length (P and T take a
// block total per 64 columns the run crosses); border taps by SibGlobalRows' per-tap path.
struct SibStripRows {
  SibGlobalRows g;
  const f4* __restrict__ G;
  FR_DEV f3 sum(int j0, int i0, int n, float w, float a, float b) const {
    const int W = g.W, H = g.H;
    if (!(i0 >= 0 && i0 + n <= W - 1)) return g.template sum<false>(j0, i0, n, w, a, b);
    const int j1 = j0 + 1 != H ? j0 + 1 : 0;
    j0 = j0 >= 0 ? j0 : H - 1;
    const char* Gb = reinterpret_cast<const char*>(G);
    const uint32_t e0 = (uint32_t)j0 * (uint32_t)(W + 1) + (uint32_t)i0;
    const uint32_t e1 = (uint32_t)j1 * (uint32_t)(W + 1) + (uint32_t)i0;
    const uint32_t un = (uint32_t)n;
    const f3 a0 = rgb_at(Gb, e0), b0 = rgb_at(Gb, e0 + 1), c0 = rgb_at(Gb, e0 + un), d0 = rgb_at(Gb, e0 + un + 1);
    const f3 a1 = rgb_at(Gb, e1), b1 = rgb_at(Gb, e1 + 1), c1 = rgb_at(Gb, e1 + un), d1 = rgb_at(Gb, e1 + un + 1);
    const float na = 1.0f - a, nb = 1.0f - b;
    const f3 r0 = (c0 - a0) * na + (d0 - b0) * a;
    const f3 r1 = (c1 - a1) * na + (d1 - b1) * a;
    return r0 * nb + r1 * b;
  }
};

// GL_LINEAR's texel column and 8-bit weight of tap position w (sibsonFS.glsl's texture() at the tap)
FR_DEV void sib_texel(float w, float sx, int& i, float& a) {
  const float tx = w * sx - 0.5f;
  const float fx0 = floorf(tx);
  a = tx - fx0;
  a = floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f);
  i = (int)fx0;
}

// Per lane and stored segment, the texel column and weight of its first tap and the last segment of
// its class (the following segments whose first taps continue the columns at the same weight: a run's pieces in
// them merge, as k_sibson_wide merges them), tabled with the segments; a row then takes one step per class it crosses
// instead of one per segment, without recomputing positions and texels at each segment edge.

// A block of SIBS_WAVES waves takes one strip at a time: wave 0 builds the lanes' tables (LDS, shared), and
// the waves split the strip's tap rows by iteration (wave w takes iterations w, w + SIBS_WAVES, ...; every
// wave steps each lane's h through all of them, the reference's sequence). Their partial sums meet in LDS
// and are added in wave order. With a wave per strip, a frame with few big discs waited on one wave's
// hundreds of dependent row steps (48 us for the centred gaze's few strips), and the waves that drew the
// widest strips set the end of the launch.
__global__ __launch_bounds__(64 * SIBS_WAVES) __attribute__((amdgpu_waves_per_eu(SIBS_OCC))) void k_sibson_strip(
    const f4* __restrict__ coord, const f4* __restrict__ color, const f4* __restrict__ P, const f4* __restrict__ T,
    const f4* __restrict__ G, f4* __restrict__ out, uint32_t* __restrict__ strips, uint32_t* __restrict__ wide, int W,
    int H, int NB, f2 screen, float strip_half, int mid, const u2* __restrict__ state, int coord_owed) {
  __shared__ int skk[(SIBS_SEGS + 1) * 64];
  __shared__ float svv[SIBS_SEGS * 64];
  __shared__ int sns[64];
  __shared__ int sci[SIBS_SEGS * 64];    // first tap's texel column
  __shared__ float sca[SIBS_SEGS * 64];  // first tap's weight
  __shared__ int sce[SIBS_SEGS * 64];    // the class's last segment
  __shared__ f4 sacc[SIBS_WAVES - 1][64];
  __shared__ uint32_t sclaim;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  SibLaneAxis X{skk + lane, svv + lane, 1.0f / screen.x, 0};
  const StripLayout L(W, H);
  uint32_t lst_next = 0;  // (wave 0's: the claim order's next list, SIBS_LISTS when all are claimed)
  const int S64 = (W + 63) / 64;
  const uint32_t N = (uint32_t)W * (uint32_t)H;
  const SibStripRows row{SibGlobalRows{color, P, T, W, H, NB, screen.x}, G};
  const float inc_x = 1.0f / screen.x, inc_y = 1.0f / screen.y;
  // Strips are claimed one at a time from the lists' counters (StripLayout): their costs differ by ~10x (the
  // widest disc of the strip sets its trip count).
  for (;;) {  // every block leaves once every list is claimed
    if (wv == 0) {
      // Class by class, this block's XCD first within a class. Wave 0's lanes look at the lists ahead in that
      // order at once and the claims skip the exhausted ones (a claim counter only grows, so a stale read can
      // only send a claim to an exhausted list, which the atomic then reports): a block leaves after one
      // round trip when nothing is left, not after one atomic per list.
      uint32_t at = 0xFFFFFFFFu;
      while (lst_next < SIBS_LISTS) {
        const uint32_t pos = lst_next + (uint32_t)lane;
        const uint32_t lp = (pos & ~7u) | ((blockIdx.x + pos) & 7u);
        const bool avail = pos < SIBS_LISTS && strips[L.xclaim + lp * 32] < strips[L.xcnt + lp * 32];
        const unsigned long long m = __ballot(avail);
        if (!m) { lst_next = SIBS_LISTS; break; }
        lst_next += (uint32_t)__ffsll(m) - 1u;
        const uint32_t lst = (lst_next & ~7u) | ((blockIdx.x + lst_next) & 7u);
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(&strips[L.xclaim + lst * 32], 1u);
        k = (uint32_t)__shfl((int)k, 0, 64);
        if (k < strips[L.xcnt + lst * 32]) { at = L.list + lst * L.cap + k; break; }
        lst_next++;
      }
      if (lane == 0) sclaim = at;
    }
    __syncthreads();  // (also: the previous strip's tables and partial sums are no longer read)
    const uint32_t s = sclaim;
    if (s == 0xFFFFFFFFu) break;  // block-uniform
    const uint32_t strip = strips[s];
    const int y = (int)(strip / (uint32_t)S64), x = (int)(strip % (uint32_t)S64) * 64 + lane;
    const uint32_t p = (uint32_t)y * (uint32_t)W + (uint32_t)min(x, W - 1);
    const f2 frag = frag_uv(min(x, W - 1), y, screen);
    const f2 cs = coord_owed ? sib_seed<true>(coord, state, W, min(x, W - 1), y, screen)
                             : sib_seed<false>(coord, state, W, min(x, W - 1), y, screen);
    const f4 closest = mk4(cs.x, cs.y, 0.0f, 0.0f);
    const float d = sib_radius(frag, closest);
    bool own = x < W && (d * screen.y > strip_half ||  // k_sibson_runs' test: this lane writes the pixel
                         (mid && d * screen.x > SIBW_MIN_HALF && !sib_rows_setup(frag.x, frag.x - d, frag.x + d, inc_x).closed));
    if (wv == 0 && own) {
      sls_build(X, frag.x - d, frag.x + d, inc_x);
      int ns_word = X.ns;
      if (X.ns < 0) {  // more segments than the table holds: k_sibson_wide's list of large discs
        const uint32_t at = atomicAdd(&wide[1], 1u);
        wide[2 + N - 1 - at] = p;
      }
      if (X.ns > 0) {
        for (int t = 0; t < X.ns; t++) sib_texel(X.V(t), screen.x, sci[t * 64 + lane], sca[t * 64 + lane]);
        sce[(X.ns - 1) * 64 + lane] = X.ns - 1;
        for (int t = X.ns - 2; t >= 0; t--) {
          const bool cont = sci[(t + 1) * 64 + lane] == sci[t * 64 + lane] + (X.K(t + 1) - X.K(t)) &&
                            sca[(t + 1) * 64 + lane] == sca[t * 64 + lane];
          sce[t * 64 + lane] = cont ? sce[(t + 1) * 64 + lane] : t;
        }
        // the border taps (on their own, per tap): the first stored tap if its texel column is -1, the last
        // if its right texel column wraps (at most one tap each: the taps are 1/W apart)
        int il;
        float al;
        sib_texel(__builtin_fmaf((float)(X.K(X.ns) - 1 - X.K(X.ns - 1)), X.D(X.ns - 1), X.V(X.ns - 1)), screen.x, il, al);
        ns_word |= (sci[lane] < 0 ? 1 << 16 : 0) | (il >= W - 1 ? 1 << 17 : 0);
      }
      sns[lane] = ns_word;
    }
    __syncthreads();  // the tables
    const int ns_word = own ? sns[lane] : 0;
    X.ns = ns_word < 0 ? -1 : (ns_word & 0xFFFF);
    own = own && X.ns >= 0;
    const bool lborder = ns_word > 0 && (ns_word & (1 << 16)), rborder = ns_word > 0 && (ns_word & (1 << 17));
    bool mine = own && X.ns > 0;  // ... and walks its tap rows (no tap in [0, 1): the reference's fallback colour)
    const float r2max = sqrt_le_bound(d);
    // taps in [0, 1) horizontally; the valid one nearest frag.x (every row's run contains it, if any)
    int kz = 0, ko = 0, kbest = 0;
    if (mine) {
      kz = sls_first_ge(X, 0.0f);
      ko = sls_first_ge(X, 1.0f);
      kbest = sls_first_ge(X, frag.x);
      if (kbest > kz) {
        const float a = frag.x - sls_tap(X, kbest - 1), b = kbest < ko ? frag.x - sls_tap(X, kbest) : INFINITY;
        if (kbest >= ko || a * a < b * b) kbest--;
      }
      kbest = min(max(kbest, kz), ko - 1);
      mine = kz < ko;
    }
    // the lanes start on the texel row of their first tap row (the wave's loads then share rows)
    const float hmax = frag.y + d;
    float h = frag.y - d;
    const int t0 = mine ? (int)floorf(h * screen.y - 0.5f) : INT_MAX;
    int tmin = t0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tmin = min(tmin, __shfl_xor(tmin, o, 64));
    const int start = mine ? t0 - tmin : 0;
    // Segment cursors in registers for the run's two ends (they move to a neighbouring segment only a few
    // times per pixel, as the chord grows and shrinks): a tap position is one fma, not a table search.
    SibCursor cl, cr;
    float dxb2 = 0.0f;  // the nearest tap's dx^2: a row has taps in the disc iff dxb2 + dy2 <= r2max
    if (mine) {
      cl.load(X, sls_seg_of(X, kbest));
      cr = cl;
      const float dxb = frag.x - cl.at(kbest);
      dxb2 = dxb * dxb;
    }
    auto inside = [&](SibCursor& c, int k, float dy2) {
      const float dx = frag.x - c.tap(X, k);
      return dx * dx + dy2 <= r2max;
    };
    f4 acc = mk4(0, 0, 0, 0);
    // One pass of the loop per SIBS_WAVES iterations (tap rows): every wave steps each lane's h through all of
    // them (the reference's sequence) and takes the row of iteration base + wv.
    for (int base = 0; __ballot(mine && h < hmax); base += SIBS_WAVES) {
      float hr = 0.0f;
      bool have = false;
#pragma unroll
      for (int q = 0; q < SIBS_WAVES; q++) {
        if (mine && h < hmax && base + q >= start) {
          if (q == wv) { hr = h; have = true; }
          h += inc_y;  // the reference's step (sibsonFS.glsl:30)
        }
      }
      if (!have || hr < 0.0f || hr >= 1.0f) continue;
      const float dy = frag.y - hr;
      const float dy2 = dy * dy;
      if (!(dxb2 + dy2 <= r2max)) continue;  // (inside(kbest))
      const float chord = __builtin_amdgcn_sqrtf(fmaxf(r2max - dy2, 0.0f));
      // the run's ends from the chord (within a tap or two), settled by the reference's test
      int k0 = min(max(cl.near(X, frag.x - chord), kz), kbest);
      int k1 = max(min(cr.near(X, frag.x + chord) - 1, ko - 1), kbest);
      if (inside(cl, k0, dy2)) { while (k0 > kz && inside(cl, k0 - 1, dy2)) k0--; }
      else { do k0++; while (!inside(cl, k0, dy2)); }
      if (inside(cr, k1, dy2)) { while (k1 < ko - 1 && inside(cr, k1 + 1, dy2)) k1++; }
      else { do k1--; while (!inside(cr, k1, dy2)); }
      cl.tap(X, k0);  // (the cursors rest on the run's ends)
      const float ty = hr * screen.y - 0.5f;
      const float fy0 = floorf(ty);
      float b = ty - fy0;
      b = floorf(b * 256.0f + 0.5f) * (1.0f / 256.0f);
      const int j0 = (int)fy0;
      f3 c = mk3(0.0f);
      acc.w += (float)(k1 - k0 + 1);  // (the row's tap count, added first: k0, k1 are consumed below)
      const bool rpeel = rborder && k1 == ko - 1;
      if (lborder && k0 == kz) {  // the left border tap (texel column -1 wraps): on its own
        const float w = cl.at(k0);
        int i;
        float a;
        sib_texel(w, screen.x, i, a);
        c = c + row.g.template sum<false>(j0, i, 1, w, a, b);
        k0++;
      }
      if (rpeel) k1--;
      if (k0 <= k1) {
        const float w0 = cl.tap(X, k0);
        int ri;
        float ra;
        sib_texel(w0, screen.x, ri, ra);
        float rw = w0;
        cr.tap(X, k1);
        const int s1 = cr.s;
        int rn = (cl.s == s1 ? k1 + 1 : cl.k1) - k0;
        for (int t = cl.s + 1; t <= s1;) {  // one step per class the run crosses
          const int It = sci[t * 64 + lane];
          const float At = sca[t * 64 + lane];
          const int Kt = X.K(t);
          if (!(It == ri + rn && At == ra)) {
            c = c + row.sum(j0, ri, rn, rw, ra, b);
            ri = It; ra = At; rw = X.V(t); rn = 0;
          }
          const int te = min(sce[t * 64 + lane], s1);
          rn += (te == s1 ? k1 + 1 : X.K(te + 1)) - Kt;
          t = te + 1;
        }
        c = c + row.sum(j0, ri, rn, rw, ra, b);
      }
      if (rpeel) {  // the right border tap (its right texel column wraps): on its own
        const float w = cr.tap(X, ko - 1);
        int i;
        float a;
        sib_texel(w, screen.x, i, a);
        c = c + row.g.template sum<false>(j0, i, 1, w, a, b);
      }
      acc.x += c.x; acc.y += c.y; acc.z += c.z;
    }
    if (wv > 0) sacc[wv - 1][lane] = acc;
    __syncthreads();  // the partial sums
    if (wv == 0 && own) {
#pragma unroll
      for (int w = 0; w < SIBS_WAVES - 1; w++) acc = acc + sacc[w][lane];
      f4 o;
      if (acc.w > 0.0f) {
        o = mk4(acc.x / acc.w, acc.y / acc.w, acc.z / acc.w, 1.0f);
      } else {
        uint32_t cx = f2u_sat(closest.x * screen.x), cy = f2u_sat(closest.y * screen.y);
        cx = min(cx, (uint32_t)W - 1); cy = min(cy, (uint32_t)H - 1);
        o = color[(size_t)cy * W + cx];
      }
      out[p] = o;
    }
  }
}

int sibson_prefix_blocks(int W) { return (W + 1 + 63) / 64; }

// Resets the Sibson work lists for a pass: wide[0..1] and strips[0..1] (counts), the strip flags, the texel-row
// range (min = 0xFFFFFFFF, max = 0) and the per-list counters (StripLayout: [flags, total) is flags, rows, buckets).
__global__ __launch_bounds__(256) void k_sibson_clear(uint32_t* __restrict__ wide, uint32_t* __restrict__ strips,
                                                      uint32_t flags, uint32_t rows, uint32_t total) {
  const uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 < 2) { wide[i0] = 0; strips[i0] = 0; }
  for (uint32_t i = flags + i0; i < total; i += gridDim.x * blockDim.x) strips[i] = i == rows ? 0xFFFFFFFFu : 0u;
}

// k_sibson_strip's work buffers: strips (StripLayout); G: W + 1 entries per row.
size_t sibson_strip_words(int W, int H) { return StripLayout(W, H).total; }
size_t sibson_rowp_texels(int W, int H) { return (size_t)(W + 1) * H; }

// state: the final state of the JumpFlooding run that wrote the prefix sums (prefix_fresh); coord_owed: that run did
// not write JFA_COORD (launch_jfa, outputs = false).
void launch_sibson_runs(const f4* coord, const u2* state, const f4* color, f4* P, f4* T, f4* G, uint32_t* wide,
                        uint32_t* strips, f4* out, int W, int H, bool prefix_fresh, bool strip, int strip_mid,
                        bool coord_owed, hipStream_t stream) {
  const int NB = sibson_prefix_blocks(W);
  strip = strip && NB <= SIBG_MAX_BLOCKS;
  const float strip_half = strip ? SIBS_HALF : INFINITY;  // (FOVRT_SIB_STRIP=0: k_sibson_wide for every wide disc)
  // mid (fr_ctx::sib_strip_mid): the wide discs without a closed form of at most 2 SIBS_HALF rows go to the strips too
  const int mid = strip ? strip_mid : 0;
  const f2 screen = mk2((float)W, (float)H);
  if (!prefix_fresh)  // (k_jfa_final_prefix wrote P and T with the colours)
    hipLaunchKernelGGL(k_sibson_prefix, dim3(NB, H), dim3(64), 0, stream, color, P, T, W, NB);
  const StripLayout L(W, H);
  // the lists' counters, the strip flags, the row range and the claim counters, in one launch (five
  // hipMemsetAsync calls were seven fill launches of ~5 us each, back to back on the JFA -> Sibson chain)
  hipLaunchKernelGGL(k_sibson_clear, dim3(std::min<uint32_t>((L.total - L.flags + 255) / 256, 64u)), dim3(256), 0, stream,
                     wide, strips, L.flags, L.rows, L.total);
  const uint32_t tiles_x = (uint32_t)(W + SIBR_TILE - 1) / SIBR_TILE, tiles_y = (uint32_t)(H + SIBR_TILE - 1) / SIBR_TILE;
  const uint32_t supers = ((tiles_x + 3) / 4) * ((tiles_y + 3) / 4);  // (k_sibson_runs: 16 blocks per super-tile)
  dim3 grid(((supers + 7) / 8) * 8 * 16);
  const bool fresh = state && prefix_fresh;
  const int owed = fresh && coord_owed ? 1 : 0;  // (JFA_COORD is written whenever the prefix sums are not fresh)
  if (fresh || owed)
    hipLaunchKernelGGL(k_sibson_runs<true>, grid, dim3(SIBR_THREADS), 0, stream, coord, state, color, P, T, out, wide,
                       strips, W, H, NB, screen, strip_half, mid, tiles_x, tiles_y);
  else
    hipLaunchKernelGGL(k_sibson_runs<false>, grid, dim3(SIBR_THREADS), 0, stream, coord, state, color, P, T, out, wide,
                       strips, W, H, NB, screen, strip_half, mid, tiles_x, tiles_y);
  hipLaunchKernelGGL((k_sibson_wide<16, 0>), dim3(SIBW_BLOCKS), dim3(64 * SIBW_WAVES), 0, stream, coord, color, P, T,
                     out, wide, W, H, NB, screen, state, owed);
  // the big discs, then those of them whose tap table overflowed (appended to the second list)
  if (strip) {
    hipLaunchKernelGGL(k_sibson_rowp, dim3(H), dim3(SIBG_THREADS), 0, stream, P, T, G, strips, W, NB);
    // (5 waves per SIMD measured slower: 96 VGPRs with spills, 90 / 180 degrees 5.3 / 5.6 against 4.7 / 4.2 ms)
    hipLaunchKernelGGL(k_sibson_strip, dim3(256 * SIBS_OCC * 4 / SIBS_WAVES), dim3(64 * SIBS_WAVES), 0, stream, coord, color, P, T, G, out,
                       strips, wide, W, H, NB, screen, strip_half, mid, state, owed);
  }
  hipLaunchKernelGGL((k_sibson_wide<64, 1>), dim3(SIBW_BLOCKS), dim3(64 * SIBW_WAVES), 0, stream, coord, color, P, T,
                     out, wide, W, H, NB, screen, state, owed);
}

}  // namespace fr
