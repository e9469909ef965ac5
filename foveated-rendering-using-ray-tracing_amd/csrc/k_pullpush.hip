// k_pullpush.hip — PullPushInterpolation  FR/PullPushInterpolation.cpp:48-238, pullFS/pushFS/pullpushFinal.glsl
#include <hip/hip_runtime.h>
#include <cmath>
#include "fr_device.h"
#include "k_launch.h"

namespace fr {

// ------------------------------------------------------------------------------------------
// PullPush on the reference's 1.5S x S atlases (S = 2^ceil(log2(max(W,H))), input zero-padded).
// Only the level regions are dispatched; the pull atlas' full-resolution region is the (padded)
// input itself and is read in place. The push atlas keeps the reference's cross-frame state.
// In-dispatch read/write overlaps of the reference (pushFS reads row 0 of the level it writes,
// and column S-1 of the full-resolution region during the last dispatch) are resolved with
// snapshot semantics: reads see the atlas as it was when the dispatch began.
// ------------------------------------------------------------------------------------------
struct PPArgs {
  const f4* in;  // W x H
  f4* pull;      // 1.5S x S
  f4* push;      // 1.5S x S
  f4* snap;      // scratch: per level c (1..e-1) 2^(c-1)+1 texels at snap_off[c]; level e: S/2+2 texels
  f4* out;       // W x H
  int W, H, S, e, AW;  // AW = 1.5 S
};

FR_DEV f4 pp_in(const PPArgs& a, int x, int y) {
  if (x < a.W && y < a.H) return a.in[(size_t)y * a.W + x];
  return mk4(0, 0, 0, 0);
}
// imageLoad(pullTex, xy): out of range -> 0; full-resolution region == padded input.
FR_DEV f4 pp_pull(const PPArgs& a, int x, int y) {
  if (x < 0 || y < 0 || x >= a.AW || y >= a.S) return mk4(0, 0, 0, 0);
  if (x < a.S) return pp_in(a, x, y);
  return a.pull[(size_t)y * a.AW + x];
}

// pullFS.glsl:48-75 for one texel: the children with alpha > 0 in offset order (0,0) (1,0) (1,1)
// (0,1), summed, divided by the summed alpha; alpha = any child.
FR_DEV f4 pull_combine(const f4 (&ch)[4]) {
  int hitCount = 0;
  f4 f = mk4(0, 0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (ch[i].w > 0.0f) { f = f + ch[i]; hitCount++; }
  if (hitCount > 0) f = f / f.w;
  return mk4(f.x, f.y, f.z, hitCount > 0 ? 1.0f : 0.0f);
}

// Pull levels sl-1 .. sl-L (L <= 6) from level sl over 2^L x 2^L tiles of level sl: a block reduces
// its tile through LDS and writes every level's texels to the atlas (the push stage reads them).
// Every texel is pull_combine of its four children, as in one launch per level, so the atlas is bit-identical;
// the 12 dependent launches of the 4K pyramid become 2 (levels 11..6 over 64x64 input tiles, then 5..0).
__global__ __launch_bounds__(256) void k_pull_tiles(PPArgs a, int sl, int L) {
  __shared__ f4 buf0[32 * 32];
  __shared__ f4 buf1[16 * 16];
  const int T = 1 << L;
  const int tx0 = blockIdx.x * T, ty0 = blockIdx.y * T;  // tile origin at level sl
  int n = T >> 1;
  {  // level sl - 1 from the atlas (or the padded input)
    const int s = sl - 1;
    for (int i = threadIdx.x; i < n * n; i += 256) {
      const int lx = i % n, ly = i / n;
      const int cx = tx0 + 2 * lx, cy = ty0 + 2 * ly;
      f4 ch[4];
      const int ox[4] = {0, 1, 1, 0}, oy[4] = {0, 0, 1, 1};
#pragma unroll
      for (int k = 0; k < 4; k++)
        ch[k] = (sl == a.e) ? pp_in(a, cx + ox[k], cy + oy[k])
                            : a.pull[(size_t)((1 << sl) - 1 + cy + oy[k]) * a.AW + a.S + cx + ox[k]];
      const f4 v = pull_combine(ch);
      buf0[i] = v;
      a.pull[(size_t)((1 << s) - 1 + (ty0 >> 1) + ly) * a.AW + a.S + (tx0 >> 1) + lx] = v;
    }
  }
  __syncthreads();
  f4* src = buf0;
  f4* dst = buf1;
  for (int l = 2; l <= L; l++) {
    const int m = n >> 1, s = sl - l;
    for (int i = threadIdx.x; i < m * m; i += 256) {
      const int lx = i % m, ly = i / m;
      const f4 ch[4] = {src[(2 * ly) * n + 2 * lx], src[(2 * ly) * n + 2 * lx + 1], src[(2 * ly + 1) * n + 2 * lx + 1],
                        src[(2 * ly + 1) * n + 2 * lx]};
      const f4 v = pull_combine(ch);
      dst[i] = v;
      a.pull[(size_t)((1 << s) - 1 + (ty0 >> l) + ly) * a.AW + a.S + (tx0 >> l) + lx] = v;
    }
    __syncthreads();
    f4* t = src; src = dst; dst = t;
    n = m;
  }
}

FR_DEV int snap_offset(int c) {  // sum_{k=1}^{c-1} (2^(k-1) + 1)
  return ((1 << (c - 1)) - 1) + (c - 1);
}

// Snapshot of the push-atlas texels that a later dispatch of this frame both reads and writes:
// row 0 of every level c in 1..e-1 (x in [0, 2^(c-1)]), stored consecutively, then the
// full-resolution column S-1, rows [S/2-2, S-1].
__global__ void k_push_snapshot(PPArgs a) {
  const int levels = snap_offset(a.e), total = levels + a.S / 2 + 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (i < levels) {
      int c = 1;
      while (snap_offset(c + 1) <= i) c++;
      a.snap[i] = a.push[(size_t)((1 << c) - 1) * a.AW + a.S + (i - snap_offset(c))];
    } else {
      const int y = a.S / 2 - 2 + (i - levels);
      a.snap[i] = (y >= 0) ? a.push[(size_t)y * a.AW + (a.S - 1)] : mk4(0, 0, 0, 0);
    }
  }
}


// imageLoad(destTex, q) during push level c with snapshot semantics.
FR_DEV f4 pp_push_read(const PPArgs& a, int c, int x, int y) {
  if (x < 0 || y < 0 || x >= a.AW || y >= a.S) return mk4(0, 0, 0, 0);
  if (c < a.e) {
    if (y == (1 << c) - 1 && x >= a.S && x <= a.S + (1 << (c - 1))) return a.snap[snap_offset(c) + (x - a.S)];
  } else {
    if (x == a.S - 1 && y >= a.S / 2 - 2) return a.snap[snap_offset(a.e) + (y - (a.S / 2 - 2))];
  }
  return a.push[(size_t)y * a.AW + x];
}

__constant__ int c_pp_off[9][2] = {{1, -1}, {1, 0}, {1, 1}, {0, -1}, {0, 0}, {0, 1}, {-1, -1}, {-1, 0}, {-1, 1}};
__constant__ float c_pp_w[9] = {1.0f / 16.0f, 1.0f / 8.0f, 1.0f / 16.0f, 1.0f / 8.0f, 1.0f / 4.0f,
                                1.0f / 8.0f, 1.0f / 16.0f, 1.0f / 8.0f, 1.0f / 16.0f};

FR_DEV f4 push_texel(const PPArgs& a, int c, int lx, int ly, int X, int Y) {
  f4 next = (c == a.e) ? pp_in(a, X, Y) : a.pull[(size_t)Y * a.AW + X];
  if (next.w > 0.0f) return next;
  const int qx = a.S + lx / 2, qy = (1 << (c - 1)) - 1 + ly / 2;
  int find_idx = 0;
  for (int i = 0; i < 9; i++) {
    f4 fc = pp_pull(a, qx + c_pp_off[i][0], qy + c_pp_off[i][1]);
    if (fc.w > 0.0f) { find_idx = i; break; }
  }
  f4 f = mk4(0, 0, 0, 0);
  for (int i = 0; i < 9; i++) {
    int k = (i + find_idx) % 9;
    f = f + c_pp_w[i] * pp_push_read(a, c, qx + c_pp_off[k][0], qy + c_pp_off[k][1]);
  }
  return f;
}

// Push level c (1 <= c < e) at (S, 2^c - 1).
__global__ void k_push_level(PPArgs a, int c) {
  const int n = 1 << c;
  const int total = n * n;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int lx = t % n, ly = t / n;
    const int X = a.S + lx, Y = n - 1 + ly;
    a.push[(size_t)Y * a.AW + X] = push_texel(a, c, lx, ly, X, Y);
  }
}

// Push level c on 64x4-texel tiles with the parents' pull and push texels (level c-1, a 34x4
// window) staged in LDS: each parent is read by up to 36 texels of the tile. Only parents inside
// the level c-1 region are staged; that region is complete before the dispatch and never written
// by it, so LDS holds exactly what imageLoad would return. Reads outside it (other levels, the
// column x = S-1, the snapshot rows) take the generic path. FINAL: level e fused with
// pullpushFinal (the cropped output plus the column x = S-1 the next frame reads).
// FINAL launches cover only the texels it writes: the W x H image (col_x0 < 0) or the 64-wide
// tile column holding x = S-1 (col_x0 = S - 64).
template <bool FINAL>
__global__ __launch_bounds__(256) void k_push_tile(PPArgs a, int c, int col_x0) {
  __shared__ f4 lpull[34 * 4];
  __shared__ f4 lpush[34 * 4];
  const int n = 1 << c, half = n >> 1;
  const int lx0 = (FINAL && col_x0 >= 0) ? col_x0 : blockIdx.x * 64, ly0 = blockIdx.y * 4;
  const int px0 = lx0 / 2 - 1, py0 = ly0 / 2 - 1;
  for (int i = threadIdx.x; i < 34 * 4; i += 256) {
    const int wx = px0 + i % 34, wy = py0 + i / 34;
    if (wx >= 0 && wx < half && wy >= 0 && wy < half) {
      const size_t q = (size_t)(half - 1 + wy) * a.AW + a.S + wx;
      lpull[i] = a.pull[q];
      lpush[i] = a.push[q];
    }
  }
  __syncthreads();
  const int lx = lx0 + (threadIdx.x & 63), ly = ly0 + (threadIdx.x >> 6);
  const int X = FINAL ? lx : a.S + lx, Y = FINAL ? ly : n - 1 + ly;
  bool in_img = false, col = false;
  if (FINAL) {
    in_img = lx < a.W && ly < a.H;
    col = lx == a.S - 1 && ly < a.S;
    if (!in_img && !col) return;
  } else if (lx >= n || ly >= n) {
    return;
  }
  f4 v = FINAL ? pp_in(a, X, Y) : a.pull[(size_t)Y * a.AW + X];
  if (!(v.w > 0.0f)) {
    const int qx = lx / 2, qy = ly / 2;  // parent, level-local
    int find_idx = 0;
    // c_pp_off[k] = (1 - k / 3, k % 3 - 1) and c_pp_w as immediates: no per-lane loads of the
    // constant tables at the rotated (lane-dependent) index; the same texels and weights
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int px = qx + 1 - i / 3, py = qy + i % 3 - 1;
      const f4 fc = (px >= 0 && px < half && py >= 0 && py < half) ? lpull[(py - py0) * 34 + (px - px0)]
                                                                    : pp_pull(a, a.S + px, half - 1 + py);
      if (fc.w > 0.0f) { find_idx = i; break; }
    }
    constexpr float wt[9] = {1.0f / 16.0f, 1.0f / 8.0f, 1.0f / 16.0f, 1.0f / 8.0f, 1.0f / 4.0f,
                             1.0f / 8.0f, 1.0f / 16.0f, 1.0f / 8.0f, 1.0f / 16.0f};
    f4 f = mk4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int k = i + find_idx >= 9 ? i + find_idx - 9 : i + find_idx;
      const int kd = (k * 11) >> 5;  // k / 3 for k < 9
      const int px = qx + 1 - kd, py = qy + (k - 3 * kd) - 1;
      const f4 pv = (px >= 0 && px < half && py >= 0 && py < half) ? lpush[(py - py0) * 34 + (px - px0)]
                                                                    : pp_push_read(a, c, a.S + px, half - 1 + py);
      f = f + wt[i] * pv;
    }
    v = f;
  }
  if (FINAL) {
    if (in_img) a.out[(size_t)ly * a.W + lx] = v;
    if (col) a.push[(size_t)ly * a.AW + lx] = v;
  } else {
    a.push[(size_t)Y * a.AW + X] = v;
  }
}

__global__ void k_push_level0(PPArgs a) { a.push[a.S] = a.pull[a.S]; }

int pp_size(int W, int H) {
  int S = 1;
  while (S < W || S < H) S *= 2;
  return S;
}
size_t pp_snap_count(int S) {
  int e = 0;
  while ((1 << e) < S) e++;
  return (size_t)((1 << (e - 1)) - 1 + (e - 1)) + (size_t)(S / 2 + 2) + 64;
}

void launch_pullpush(const f4* in, f4* pull, f4* push, f4* snap, f4* out, int W, int H, hipStream_t stream) {
  PPArgs a;
  a.in = in; a.pull = pull; a.push = push; a.snap = snap; a.out = out;
  a.W = W; a.H = H; a.S = pp_size(W, H); a.AW = a.S + a.S / 2;
  a.e = 0;
  while ((1 << a.e) < a.S) a.e++;
  if (a.e <= 1) {
    // S = 1 and S = 2: the reference's push loop never writes the full-resolution region. It moves
    // writeOffset to (0, 0) after step--, when the NEXT dispatch is the last one; at e = 1 the only
    // dispatch still writes at (S, 1), and at e = 0 there is none (PullPushInterpolation.cpp:163-198).
    // pullpushFinal then copies out what the cleared atlas holds: zeros, for any input.
    hipMemsetAsync(out, 0, (size_t)W * H * sizeof(f4), stream);
    return;
  }
  for (int sl = a.e; sl > 0;) {
    const int L = std::min(6, sl);
    const int tiles = 1 << (sl - L);
    hipLaunchKernelGGL(k_pull_tiles, dim3(tiles, tiles), dim3(256), 0, stream, a, sl, L);
    sl -= L;
  }
  hipLaunchKernelGGL(k_push_snapshot, dim3((pp_snap_count(a.S) + 255) / 256), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(k_push_level0, dim3(1), dim3(1), 0, stream, a);
  for (int c = 1; c < a.e; c++) {
    const int n = 1 << c;
    int total = n * n;
    int blocks = std::min((total + 255) / 256, 4096);
    if (n >= 64) hipLaunchKernelGGL(k_push_tile<false>, dim3(n / 64, n / 4), dim3(256), 0, stream, a, c, -1);
    else hipLaunchKernelGGL(k_push_level, dim3(blocks), dim3(256), 0, stream, a, c);
  }
  // the final level: the image region, then the 64-wide tile column holding x = S-1, which the
  // next frame reads (a texel both launches write gets the same value from each: the final level
  // reads the column through the snapshot, never through the texels being written)
  hipLaunchKernelGGL(k_push_tile<true>, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, stream, a, a.e, -1);
  hipLaunchKernelGGL(k_push_tile<true>, dim3(1, (a.S + 3) / 4), dim3(256), 0, stream, a, a.e, std::max(a.S - 64, 0));
}

}  // namespace fr
