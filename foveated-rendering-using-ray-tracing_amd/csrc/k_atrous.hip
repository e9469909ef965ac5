// k_atrous.hip — ATrous               FR/ATrous.cpp:47-132, FR/shader/atFS.glsl:40-90
#include <hip/hip_runtime.h>
#include <cmath>
#include "fr_device.h"
#include "k_launch.h"

namespace fr {

// ------------------------------------------------------------------------------------------
// A-Trous (atFS.glsl:40-90): 5x5 B3 kernel, colour / normal / position edge stopping.
// ------------------------------------------------------------------------------------------
__constant__ float c_at_kernel[25] = {
    1.f / 256.f, 1.f / 64.f, 3.f / 128.f, 1.f / 64.f, 1.f / 256.f, 1.f / 64.f, 1.f / 16.f, 3.f / 32.f, 1.f / 16.f,
    1.f / 64.f,  3.f / 128.f, 3.f / 32.f, 9.f / 64.f, 3.f / 32.f, 3.f / 128.f, 1.f / 64.f, 1.f / 16.f, 3.f / 32.f,
    1.f / 16.f,  1.f / 64.f, 1.f / 256.f, 1.f / 64.f, 3.f / 128.f, 1.f / 64.f, 1.f / 256.f};

// GLSL exp() as the reference's GL driver evaluates it: the hardware base-2 exponential of
// x * log2(e) (v_exp_f32), not the libm-accurate expf. A-Trous is a tolerance stage.
FR_DEV float gl_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504f); }

// One atFS pass over a 16x16 block. TILE: position / normal / colour of the block plus its
// 2*stepWidth halo are staged in LDS once (each texel is read by up to 25 pixels). c_phi, n_phi,
// p_phi and stepWidth^2 are powers of two (always so in ATrous::render: 1, 2^-k, 1, 4^k; launch_atrous
// launches nothing otherwise), so the divisions are exact multiplications by the reciprocal:
// bit-identical, without the division sequence.
FR_DEV float at_dot(f4 t) {
  return __builtin_fmaf(t.w, t.w, __builtin_fmaf(t.z, t.z, __builtin_fmaf(t.y, t.y, t.x * t.x)));
}

template <bool TILE>
__global__ __launch_bounds__(256) void k_atrous(const f4* __restrict__ pos, const f4* __restrict__ nrm,
                                                const f4* __restrict__ col, f4* __restrict__ out, int W, int H,
                                                float c_phi, float n_phi, float p_phi, float stepWidth) {
  extern __shared__ f4 at_lds[];
  const int sw = (int)stepWidth;
  const int halo = 2 * sw, tw = 16 + 2 * halo;
  const int bx0 = blockIdx.x * 16, by0 = blockIdx.y * 16;
  f4* lp = at_lds;
  f4* ln = at_lds + tw * tw;
  f4* lc = at_lds + 2 * tw * tw;
  if (TILE) {
    for (int i = threadIdx.x; i < tw * tw; i += 256) {
      const int gx = bx0 - halo + i % tw, gy = by0 - halo + i / tw;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
        const size_t q = (size_t)gy * W + gx;
        lp[i] = pos[q]; ln[i] = nrm[q]; lc[i] = col[q];
      }
    }
    __syncthreads();
  }
  const int x = bx0 + (threadIdx.x & 15);
  const int y = by0 + (threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const size_t p = (size_t)y * W + x;
  const int lme = ((threadIdx.x >> 4) + halo) * tw + (threadIdx.x & 15) + halo;
  const f4 pval = TILE ? lp[lme] : pos[p], nval = TILE ? ln[lme] : nrm[p], cval = TILE ? lc[lme] : col[p];
  const float inv_c = 1.0f / c_phi, inv_n = 1.0f / n_phi, inv_p = 1.0f / p_phi, inv_sw2 = 1.0f / (stepWidth * stepWidth);
  f4 sum = mk4(0, 0, 0, 0);
  float cum_w = 0.0f;
#pragma unroll
  for (int i = 0; i < 25; i++) {
    const int ox = (i % 5) - 2, oy = 2 - (i / 5);  // offset[i] = (-2..2, +2..-2) row by row
    const int tx = x + ox * sw, ty = y + oy * sw;
    if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;
    const size_t q = (size_t)ty * W + tx;
    const int lq = lme + oy * sw * tw + ox * sw;
    // w = min(e^-a, 1) * min(e^-b, 1) * min(e^-c, 1) with a, b, c >= 0 (squared distances over
    // positive phis): one exponential of the sum, each term clamped at 0 (which also keeps the
    // reference's weight 1 for a NaN term, fminf(e^NaN, 1) = 1). GLSL exp is itself the hardware
    // exp2 approximation, so this stays within the stage's 2e-6 tolerance. The dot
    // products and the weighted sums are FMA chains and the tap weight times the kernel weight is
    // formed once: ulp-level rounding differences from atFS's order, 0.29 -> 0.225 ms at 4K.
    f4 ctmp = TILE ? lc[lq] : col[q];
    f4 t = cval - ctmp;
    float dist2 = at_dot(t);
    const float ec = fmaxf(dist2 * inv_c, 0.0f);
    f4 ntmp = TILE ? ln[lq] : nrm[q];
    t = nval - ntmp;
    dist2 = fmaxf(at_dot(t) * inv_sw2, 0.0f);
    const float en = fmaxf(dist2 * inv_n, 0.0f);
    f4 ptmp = TILE ? lp[lq] : pos[q];
    t = pval - ptmp;
    dist2 = at_dot(t);
    const float ep = fmaxf(dist2 * inv_p, 0.0f);
    const float wk = gl_exp(-(ec + en + ep)) * c_at_kernel[i];
    sum = mk4(__builtin_fmaf(ctmp.x, wk, sum.x), __builtin_fmaf(ctmp.y, wk, sum.y), __builtin_fmaf(ctmp.z, wk, sum.z),
              __builtin_fmaf(ctmp.w, wk, sum.w));
    cum_w += wk;
  }
  out[p] = sum / cum_w;
}

// atFS at stepWidth 1 (ATrous::render's first pass, the only one at the default iteration count)
// with two vertically adjacent pixels per thread over a 16x32 block: the two 5x5 footprints share
// 4 of their 6 texel rows, so each thread reads 6x5 position / normal / colour texels from LDS for
// both pixels (45 ds_read_b128 per pixel instead of 75). Each pixel accumulates its own taps in
// atFS order (rows from oy = +2 down to -2, ox ascending) with k_atrous's arithmetic, so the output
// is bit-identical to k_atrous<true>. Interior blocks (every tap inside the image) run
// without bounds tests.
FR_DEV float at_weight(f4 cval, f4 nval, f4 pval, f4 ctmp, f4 ntmp, f4 ptmp, float inv_c, float inv_n, float inv_p,
                       float kern) {
  f4 t = cval - ctmp;
  float dist2 = at_dot(t);
  const float ec = fmaxf(dist2 * inv_c, 0.0f);
  t = nval - ntmp;
  dist2 = fmaxf(at_dot(t), 0.0f);  // stepWidth^2 = 1
  const float en = fmaxf(dist2 * inv_n, 0.0f);
  t = pval - ptmp;
  dist2 = at_dot(t);
  const float ep = fmaxf(dist2 * inv_p, 0.0f);
  return gl_exp(-(ec + en + ep)) * kern;
}

template <bool CHECK>
FR_DEV void atrous_rows2(const f4* lp, const f4* ln, const f4* lc, int u, int v, int x, int y, int W, int H, float inv_c,
                         float inv_n, float inv_p, f4& outA, f4& outB) {
  constexpr int TW = 20;
  const int la = v * TW + u, lb = la + TW;
  const f4 cA = lc[la], nA = ln[la], pA = lp[la];
  const f4 cB = lc[lb], nB = ln[lb], pB = lp[lb];
  f4 sA = mk4(0, 0, 0, 0), sB = mk4(0, 0, 0, 0);
  float wA = 0.0f, wB = 0.0f;
#pragma unroll 1  // a row at a time: fully unrolled, the compiler hoists the loads of several rows
                  // and defers the accumulation chains (over 200 VGPRs, one wave per SIMD)
  for (int r = 0; r < 6; r++) {  // tile row v + 3 - r: B's oy = 2 - r, A's oy = 3 - r
#pragma unroll
    for (int ox = -2; ox <= 2; ox++) {
      const int lq = la + (3 - r) * TW + ox;
      const f4 c = lc[lq], n = ln[lq], p = lp[lq];
      const bool colok = !CHECK || (x + ox >= 0 && x + ox < W);
      if (r >= 1) {
        const int oy = 3 - r;
        if (colok && (!CHECK || (y + oy >= 0 && y + oy < H))) {
          const float wk = at_weight(cA, nA, pA, c, n, p, inv_c, inv_n, inv_p, c_at_kernel[(2 - oy) * 5 + ox + 2]);
          sA = mk4(__builtin_fmaf(c.x, wk, sA.x), __builtin_fmaf(c.y, wk, sA.y), __builtin_fmaf(c.z, wk, sA.z),
                   __builtin_fmaf(c.w, wk, sA.w));
          wA += wk;
        }
      }
      if (r <= 4) {
        const int oy = 2 - r;
        if (colok && (!CHECK || (y + 1 + oy >= 0 && y + 1 + oy < H))) {
          const float wk = at_weight(cB, nB, pB, c, n, p, inv_c, inv_n, inv_p, c_at_kernel[(2 - oy) * 5 + ox + 2]);
          sB = mk4(__builtin_fmaf(c.x, wk, sB.x), __builtin_fmaf(c.y, wk, sB.y), __builtin_fmaf(c.z, wk, sB.z),
                   __builtin_fmaf(c.w, wk, sB.w));
          wB += wk;
        }
      }
    }
  }
  outA = sA / wA;
  outB = sB / wB;
}

__global__ __launch_bounds__(256) void k_atrous_rows2(const f4* __restrict__ pos, const f4* __restrict__ nrm,
                                                      const f4* __restrict__ col, f4* __restrict__ out, int W, int H,
                                                      float c_phi, float n_phi, float p_phi, int xcd) {
  constexpr int TW = 20, TH = 36;
  __shared__ f4 lp[TW * TH], ln[TW * TH], lc[TW * TH];
  // xcd: the blocks of one XCD take one band of tile rows, so a tile's halo texels are mostly in the
  // L2 that fetched its neighbours' (round-robin order: every 8th tile per XCD, each halo from HBM)
  const uint32_t tile = xcd ? xcd_tile(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y) : blockIdx.y * gridDim.x + blockIdx.x;
  const int ox0 = (int)(tile % gridDim.x) * 16 - 2, oy0 = (int)(tile / gridDim.x) * 32 - 2;
  for (int i = threadIdx.x; i < TW * TH; i += 256) {
    const int gx = ox0 + i % TW, gy = oy0 + i / TW;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t q = (size_t)gy * W + gx;
      lp[i] = pos[q]; ln[i] = nrm[q]; lc[i] = col[q];
    }
  }
  __syncthreads();
  const int u = 2 + (threadIdx.x & 15), v = 2 + 2 * (threadIdx.x >> 4);
  const int x = ox0 + u, y = oy0 + v;
  if (x >= W || y >= H) return;
  const bool interior = ox0 >= 0 && oy0 >= 0 && ox0 + TW <= W && oy0 + TH <= H;  // block-uniform
  const float inv_c = 1.0f / c_phi, inv_n = 1.0f / n_phi, inv_p = 1.0f / p_phi;
  f4 a, b;
  if (interior) atrous_rows2<false>(lp, ln, lc, u, v, x, y, W, H, inv_c, inv_n, inv_p, a, b);
  else atrous_rows2<true>(lp, ln, lc, u, v, x, y, W, H, inv_c, inv_n, inv_p, a, b);
  out[(size_t)y * W + x] = a;
  if (y + 1 < H) out[(size_t)(y + 1) * W + x] = b;
}

static bool pow2f(float v) {
  int e;
  return v > 0.0f && std::isfinite(v) && std::frexp(v, &e) == 0.5f;
}

// false, with nothing launched: a phi or stepWidth^2 that is not a power of two (the kernels multiply by reciprocals)
bool launch_atrous(const f4* pos, const f4* nrm, const f4* col, f4* out, int W, int H, float c_phi, float n_phi,
                   float p_phi, float stepWidth, bool rows2, int xcd, hipStream_t stream) {
  dim3 grid((W + 15) / 16, (H + 15) / 16);
  const bool pw = pow2f(c_phi) && pow2f(n_phi) && pow2f(p_phi) && pow2f(stepWidth * stepWidth) &&
                  pow2f(1.0f / c_phi) && pow2f(1.0f / n_phi) && pow2f(1.0f / p_phi) &&
                  pow2f(1.0f / (stepWidth * stepWidth));
  if (!pw) return false;
  const int sw = (int)stepWidth;
  // rows2 = false (fr_ctx::atrous_rows2): k_atrous for the stepWidth-1 pass too (A/B of the two-row kernel)
  if (rows2 && stepWidth == 1.0f) {
    dim3 g2((W + 15) / 16, (H + 31) / 32);
    hipLaunchKernelGGL(k_atrous_rows2, g2, dim3(256), 0, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, xcd);
    return true;
  }
  const int tw = 16 + 4 * sw;
  const size_t lds = (size_t)3 * tw * tw * sizeof(f4);
  if (sw >= 1 && lds <= 64 * 1024)
    hipLaunchKernelGGL((k_atrous<true>), grid, dim3(256), lds, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, stepWidth);
  else  // (a halo beyond 64 KB of LDS: stepWidth >= 8)
    hipLaunchKernelGGL((k_atrous<false>), grid, dim3(256), 0, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, stepWidth);
  return true;
}

}  // namespace fr
