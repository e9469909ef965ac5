// k_image.hip — the image-space half of the hot path on gfx950 (HBM-bandwidth bound, no MFMA):
//   sampling_step (entry 1)        FR/cuda/samplingStep.cu:72-239 + shared_helper_funcs.h:60-300,376-412
//   warp_sort compaction (entry 2) FR/cuda/warpSort.cu:67-169 -> wave ballot + scan (ray_count bit-exact)
//   JumpFlooding                   FR/JumpFlooding.cpp:60-140, FR/shader/cpFS.glsl, FR/shader/jfFS.glsl
//   SibsonInterpolation            FR/SibsonInterpolation.cpp:28-53, FR/shader/sibsonFS.glsl:16-49
//   PullPushInterpolation          FR/PullPushInterpolation.cpp:48-238, pullFS/pushFS/pullpushFinal.glsl
//   ATrous                         FR/ATrous.cpp:47-132, FR/shader/atFS.glsl:40-90
// GL texture fetches at texel centres are integer texel loads; off-centre GL_LINEAR taps (Sibson)
// use fr::bilinear_repeat. JFA propagates a 32-bit seed index (+2 alpha flags) instead of two
// RGBA32F textures: the reference's coord/colour pair is a pure function of the seed pixel.
#include <hip/hip_runtime.h>
#include <cmath>
#include "fr_device.h"

namespace fr {

// ------------------------------------------------------------------------------------------
// Entry 1: sampling_step. Blocks of 16x16 pixels (4 waves of 16x4); each wave publishes its
// 64-bit usingRay ballot, which entry 2 scans into the active list in tile order.
// ------------------------------------------------------------------------------------------
__constant__ float c_gx[9] = {-1.0f, -0.0f, +1.0f, -2.0f, +0.0f, +2.0f, -1.0f, -0.0f, +1.0f};
__constant__ float c_gy[9] = {-1.0f, -2.0f, -1.0f, -0.0f, +0.0f, +0.0f, +1.0f, +2.0f, +1.0f};
// uint2 offset[9] = {(-1,+1), (0,+1), ...}: every "(a, b)" is a comma expression, so the nine
// scalars {1,1,1,0,0,0,-1,-1,-1} fill the uint2 array flat (shared_helper_funcs.h:20-24, PTX
// FR/cuda/samplingStep.ptx:16).
__constant__ uint32_t c_off[9][2] = {{1u, 1u}, {1u, 0u}, {0u, 0u}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0xFFFFFFFFu, 0u},
                                     {0u, 0u}, {0u, 0u}, {0u, 0u}, {0u, 0u}};
__constant__ uint8_t c_mask25[4][4] = {{1, 1, 0, 0}, {1, 1, 0, 0}, {1, 1, 1, 1}, {1, 1, 1, 1}};
__constant__ uint8_t c_mask50[4][4] = {{1, 1, 0, 0}, {1, 1, 0, 0}, {0, 0, 1, 1}, {0, 0, 1, 1}};
__constant__ uint8_t c_mask75[4][4] = {{1, 1, 0, 0}, {1, 1, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

enum MaskMode { MASK_SALIENCY = 0, MASK_LOGPOLAR = 1, MASK_UNIFORM2X2 = 2, MASK_ALL = 3, MASK_LOGPOLAR_SIGNED = 4 };

FR_DEV bool masked_sampling(uint32_t x, uint32_t y, float sample_dist, float intensity) {
  bool isSample = false;
  const float r0 = 0.07f, r1 = r0 * 1.5f, r2 = r0 * 2.0f;
  const uint32_t mx = x % 4u, my = y % 4u;
  if (0 <= sample_dist && sample_dist < r0) isSample = true;
  else if (r0 < sample_dist && sample_dist <= r1) isSample = c_mask25[mx][my];
  else if (r1 < sample_dist && sample_dist <= r2) isSample = c_mask50[mx][my];
  const float g0 = 0.01f, g1 = 0.4f, g2 = 0.6f;
  if (g0 < intensity && intensity < g1) isSample = isSample | (bool)c_mask75[mx][my];
  else if (g1 <= intensity && intensity < g2) isSample = isSample | (bool)c_mask50[mx][my];
  else if (g2 <= intensity) isSample = isSample | (bool)c_mask25[mx][my];
  else isSample = isSample | ((x % 8u) == 0 && (y % 8u) == 0);
  return isSample;
}

FR_DEV uint32_t i2u(int32_t v) { return (uint32_t)v; }

// L = log of the largest centre-to-corner distance (shared_helper_funcs.h:380-384, :396-400): the
// same for every pixel of a frame, so the host computes it once (log_polar_L) and passes it in.
FR_HD float log_polar_L(f2 center, f2 bs) {
  float l1 = length(center);
  float l2 = length(bs - center);
  float l3 = length(mk2(center.x, bs.y - center.y));
  float l4 = length(mk2(bs.x - center.x, center.y));
  return fr_log(fmaxf(fmaxf(l1, l2), fmaxf(l3, l4)));
}

FR_DEV u2 forward_log_polar(u2 xy, f2 center, f2 bs, float L) {
  f2 xp = mk2((float)xy.x, (float)xy.y) - center;
  u2 uv;
  uv.x = i2u(f2i_sat(fr_pow(fr_log(length(xp)) / L, 4.0f) * bs.x));
  uv.y = i2u(f2i_sat((fr_atan2(xp.y, xp.x) + ((2.0f * kPi) * (xp.y < 0.0f ? 1.0f : 0.0f))) * (bs.y / (2.0f * kPi))));
  return uv;
}

FR_DEV u2 inverse_log_polar(u2 uv, f2 center, f2 bs, float L) {
  u2 xy{0xFFFFFFFFu, 0xFFFFFFFFu};  // make_uint2(-1.0f): pinned to the wrap-around value
  if ((float)uv.x >= bs.x || (float)uv.y >= bs.y) return xy;
  float B = (2.0f * kPi) / bs.y;
  float K = fr_pow((float)uv.x / bs.x, 1.0f / 4.0f);
  float e = fr_exp(L * K);
  xy.x = i2u(f2i_sat(e * fr_cos(B * (float)uv.y) + center.x));
  xy.y = i2u(f2i_sat(e * fr_sin(B * (float)uv.y) + center.y));
  return xy;
}

// Entry-2 input: per wave and per primary-hit class (0 refraction, 1 reflection, 2 diffuse, 3 miss,
// from the G-buffer) the 64-bit usingRay ballot, and per 16x16 block the per-class counts. The
// active list is built class-major so that waves of the megakernel hold paths of similar length.
FR_DEV void publish_ballots(bool on, int cls, unsigned long long* __restrict__ words, uint32_t* __restrict__ counts) {
  __shared__ uint32_t cnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t nb = (size_t)gridDim.x * gridDim.y;
  const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; c++) {
    unsigned long long m = __ballot(on && cls == c);
    if (lane == 0) {
      words[(b * 4 + wv) * 4 + c] = m;
      atomicAdd(&cnt[c], (uint32_t)__popcll(m));
    }
  }
  __syncthreads();
  if (threadIdx.x < 4) counts[threadIdx.x * nb + b] = cnt[threadIdx.x];
}

// The saliency features are functions of the 4x4 cell origin (samplingStep.cu:186-219): the 16
// cells of a 16x16 block are evaluated once each and shared via LDS (the same expressions as
// per pixel, so every pixel sees the same values). The 4 x 16 Sobel sums (diffuse gx, gy, normal
// gx, gy; gradient(), shared_helper_funcs.h) are one per lane of wave 0, with all nine taps of a lane requested at once; wave 1
// evaluates the per-cell rest. (One lane evaluating a whole cell serialised 36 tap loads.)
// Called by all 256 threads of the block (two barriers); cellf / cellg are the block's LDS.
FR_DEV void saliency_cells(const FrameUniforms& U, const DevScene& sc, const f4* __restrict__ diffuse,
                           const f4* __restrict__ normal, const f4* __restrict__ depth, float (&cellf)[16][8],
                           float (&cellg)[4][16]) {
  const int W = U.width, H = U.height;
  const f2 screenf = U.screen;
  if (threadIdx.x < 64) {
    const int cell = threadIdx.x & 15, g = threadIdx.x >> 4;
    const uint32_t sx = blockIdx.x * 16 + 4 * (cell & 3), sy = blockIdx.y * 16 + 4 * (cell >> 2);
    if ((int)sx < W && (int)sy < H) {
      const f4* buf = g < 2 ? diffuse : normal;
      const float* gw = (g & 1) ? c_gy : c_gx;
      f4 tap[9];
      bool in[9];
#pragma unroll
      for (int i = 0; i < 9; i++) {
        const uint32_t kx = sx + c_off[i][0] * 4u, ky = sy + c_off[i][1] * 4u;
        in[i] = !((float)kx >= screenf.x || (float)ky >= screenf.y);
        tap[i] = buf[in[i] ? (size_t)ky * W + kx : (size_t)sy * W + sx];
      }
      float result = 0.0f;  // grad_comp's sum in tap order as fma(mean, g[i], sum) (samplingStep.ptx:355-359)
#pragma unroll
      for (int i = 0; i < 9; i++)
        result = in[i] ? __builtin_fmaf((tap[i].x + tap[i].y + tap[i].z) / 3.0f, gw[i], result) : result;
      cellg[g][cell] = result;
    }
  } else if (threadIdx.x < 80) {
    const int cell = threadIdx.x & 15;
    const uint32_t sx = blockIdx.x * 16 + 4 * (cell & 3), sy = blockIdx.y * 16 + 4 * (cell >> 2);
    if ((int)sx < W && (int)sy < H) {
      f4 rgba = diffuse[(size_t)sy * W + sx];
      float R = rgba.x - (rgba.y + rgba.z) / 2.0f;
      float G = rgba.y - (rgba.x + rgba.z) / 2.0f;
      float Bc = rgba.z - (rgba.x + rgba.y) / 2.0f;
      float Y = (rgba.x + rgba.y) / 2.0f - fabsf(rgba.x - rgba.y) / 2.0f - rgba.z;
      float L = (rgba.x + rgba.y + rgba.z) / 3.0f;
      // depth_buffer[make_uint2(gaze)] (samplingStep.cu:197, shared_helper_funcs.h:94): the saturating conversion is the
      // reference's; the clamp to the last row / column is ours (a cursor on the window's top edge
      // gives gaze.y = H, off-window cursors give any value; the reference reads out of bounds)
      const uint32_t gzx = min(f2u_sat(U.gaze.x), (uint32_t)W - 1), gzy = min(f2u_sat(U.gaze.y), (uint32_t)H - 1);
      float theta = lengthc(sc.bbox_max - sc.bbox_min) * 0.005f;  // samplingStep.ptx:785-795
      float focal = depth[(size_t)gzy * W + gzx].x;
      float dep = depth[(size_t)sy * W + sx].x - focal;
      float dep2 = dep * dep;
      float dd = 0.4f * theta;
      float* f = cellf[cell];
      f[0] = R - G;                      // rgbyl.x
      f[1] = Bc - Y;                     // rgbyl.y
      f[2] = L;                          // rgbyl.z
      f[4] = 1.0f / (dd * sqrtf(2.0f * kPi)) * fr_exp(-dep2 / (dd * dd)) * (1.0f * theta);  // s_depth
      f[5] = normal[(size_t)sy * W + sx].w;                                                // s_shadow
    }
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const float gx = cellg[0][threadIdx.x], gy = cellg[1][threadIdx.x];
    const float ngx = cellg[2][threadIdx.x], ngy = cellg[3][threadIdx.x];
    cellf[threadIdx.x][3] = cuda_atanf(gy / gx);  // s_orientation: CUDA's atanf (samplingStep.ptx:748-784)
    cellf[threadIdx.x][6] = len2c(ngx, ngy);      // s_normal_grad (:1117-1119)
  }
  __syncthreads();
}

// A pixel's saliency from its cell's features and its reprojected position (WEIGHT.xy).
FR_DEV float pixel_saliency(const float (&cellf)[16][8], int x, int y, f2 query_uv) {
  const float* f = cellf[((y & 15) >> 2) * 4 + ((x & 15) >> 2)];
  const f3 rgbyl = mk3(f[0], f[1], f[2]);
  const float s_orientation = f[3], s_depth = f[4], s_shadow = f[5], s_normal_grad = f[6];
  float velocity = len2c((float)x - query_uv.x, (float)y - query_uv.y) * 0.5f;  // samplingStep.ptx:1120-1128
  if (query_uv.x < 0.0f && query_uv.y < 0.0f) velocity = 0.0f;
  const float m = -0.4f, Am = 20.0f;
  float va = (velocity / Am) * (velocity / Am);
  float s_velocity = __builtin_fmaf(fr_exp(-va / (m * m)), 1.0f / (m * sqrtf(2.0f * kPi)), 1.0f);  // :1147
  float saliency = (__builtin_fmaf(rgbyl.x + rgbyl.y, 0.5f, rgbyl.z) + s_orientation) / 3.0f;      // :1150-1153
  saliency = fmaxf(saliency, s_normal_grad);
  saliency *= s_depth;
  saliency = fmaxf(saliency, s_velocity) * s_shadow;
  return saliency;
}

// The `extra` heat map of a saliency, with CUDA's cosf / sinf (samplingStep.ptx:1288-1600).
FR_DEV f4 heat_map(float saliency) {
  return mk4(cuda_cosf(saliency * kPi_2 - kPi_2), cuda_sinf(saliency * kPi) * 1.5f, cuda_cosf(saliency * kPi_2), 1.0f);
}

template <bool LOCAL>  // LOCAL: a tile-local front (fr_set_front_local); the whole-screen instance carries none of it
__global__ __launch_bounds__(256) void k_sampling(FrameUniforms U, DevScene sc, const f4* __restrict__ position,
                                                  const f4* __restrict__ depth, const f4* __restrict__ depth_cache,
                                                  f4* __restrict__ weight, const f4* __restrict__ normal,
                                                  const f4* __restrict__ diffuse, f4* __restrict__ extra,
                                                  uint8_t* __restrict__ mask, const uint8_t* __restrict__ gclass,
                                                  unsigned long long* __restrict__ words, uint32_t* __restrict__ counts,
                                                  int write_extra, const uint8_t* __restrict__ lp_cache,
                                                  uint32_t* __restrict__ bcount) {
  const int W = U.width, H = U.height;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = blockIdx.x * 16 + (lane & 15);
  const int y = blockIdx.y * 16 + wv * 4 + (lane >> 4);
  const f2 screenf = U.screen;
  if (LOCAL && !shard_owns(U, blockIdx.x * 16, blockIdx.y * 16)) {
    // tile-local front: another rank's block (its G-buffer may not exist here) is inactive; its ballot
    // words, class counts, unfolded count and mask bytes are zero
    const size_t nb = (size_t)gridDim.x * gridDim.y, b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x < 16) words[b * 16 + threadIdx.x] = 0ull;
    else if (threadIdx.x < 20) counts[(threadIdx.x - 16) * nb + b] = 0u;
    else if (threadIdx.x == 20 && bcount) bcount[b] = 0u;
    if (x < W && y < H) mask[(size_t)y * W + x] = 0;
    return;
  }
  // Only the saliency mask and an `extra` stored here read the saliency features. write_extra is 0 when the
  // context leaves the heat map to k_extra (written when something reads EXTRA) or never writes it: with a
  // log-polar, uniform or full mask the cell phase, its two barriers and its 36 B of tap loads per pixel are
  // then skipped (block-uniform branch).
  const bool saliency_used = U.mask_mode == MASK_SALIENCY || write_extra;
  __shared__ float cellf[16][8];
  __shared__ float cellg[4][16];
  if (saliency_used) saliency_cells(U, sc, diffuse, normal, depth, cellf, cellg);
  bool usingRay = false, unfolded = false;
  int cls = 3;
  if (x < W && y < H) {
    const size_t p = (size_t)y * W + x;
    cls = gclass[p];
    f4 pos = position[p];
    f4 wgt = weight[p];
    f2 query_uv = mk2(wgt.x, wgt.y);
    float isValid = 0.0f;
    if (query_uv.x > -1.0f && query_uv.y > -1.0f) {
      if ((0 <= query_uv.x && query_uv.x < screenf.x - 0.5f) && (0 <= query_uv.y && query_uv.y < screenf.y - 0.5f)) {
        uint32_t qx = f2u_sat(fr_round(query_uv.x)), qy = f2u_sat(fr_round(query_uv.y));
        f4 prev_depth = depth_cache[(size_t)qy * W + qx];
        float diff = prev_depth.x - lengthc(xyz(pos) - U.prev_eye);  // samplingStep.ptx:258-273
        isValid = fabsf(diff) < sc.scene_epsilon ? 1.0f : 0.0f;
      }
    }
    const float saliency = saliency_used ? pixel_saliency(cellf, x, y, query_uv) : 0.0f;

    switch (U.mask_mode) {
      case MASK_SALIENCY:
        usingRay = masked_sampling((uint32_t)x, (uint32_t)y,  // gaze_dist (samplingStep.ptx:276-288)
                                   len2c((float)x - U.gaze.x, (float)y - U.gaze.y) / len2c(screenf.x, screenf.y), saliency);
        break;
      case MASK_LOGPOLAR:
      case MASK_LOGPOLAR_SIGNED: usingRay = lp_cache[p] != 0; break;  // k_logpolar_mask
      case MASK_UNIFORM2X2: usingRay = (x % 2 == 0) && (y % 2 == 0); break;
      default: usingRay = true;
    }
    if (bcount) unfolded = usingRay;
    usingRay = usingRay && shard_owns(U, x, y);  // tile sharding: this rank traces its own tiles only
    weight[p] = mk4(query_uv.x, query_uv.y, isValid, 0.0f);
    if (write_extra) extra[p] = heat_map(saliency);
    mask[p] = usingRay ? 1 : 0;
  }
  publish_ballots(usingRay, cls, words, counts);
  if (bcount) {
    // tile sharding: this block's active pixels before the ownership fold (a 16x16 block lies in one
    // tile); k_owner_counts sums them per owner, so every rank knows every rank's active count
    __shared__ uint32_t nb;
    if (threadIdx.x == 0) nb = 0;
    __syncthreads();
    const unsigned long long m = __ballot(unfolded);
    if ((threadIdx.x & 63) == 0) atomicAdd(&nb, (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) bcount[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = nb;
  }
}

// The heat map a k_sampling launch left unwritten (context.cpp, materialize_extra_now): the same cell phase and
// per-pixel expressions over that launch's inputs (its uniforms, DIFFUSE, NORMAL, DEPTH and WEIGHT.xy, which
// the sampling does not change), so EXTRA is what that launch would have stored, bit for bit.
__global__ __launch_bounds__(256) void k_extra(FrameUniforms U, DevScene sc, const f4* __restrict__ depth,
                                               const f4* __restrict__ weight, const f4* __restrict__ normal,
                                               const f4* __restrict__ diffuse, f4* __restrict__ extra) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = blockIdx.x * 16 + (lane & 15);
  const int y = blockIdx.y * 16 + wv * 4 + (lane >> 4);
  __shared__ float cellf[16][8];
  __shared__ float cellg[4][16];
  saliency_cells(U, sc, diffuse, normal, depth, cellf, cellg);
  if (x < U.width && y < U.height) {
    const size_t p = (size_t)y * U.width + x;
    const f4 wgt = weight[p];
    extra[p] = heat_map(pixel_saliency(cellf, x, y, mk2(wgt.x, wgt.y)));
  }
}

void launch_extra(const FrameUniforms& U, const DevScene& sc, const f4* depth, const f4* weight, const f4* normal,
                  const f4* diffuse, f4* extra, hipStream_t stream) {
  dim3 grid((U.width + 15) / 16, (U.height + 15) / 16);
  hipLaunchKernelGGL(k_extra, grid, dim3(256), 0, stream, U, sc, depth, weight, normal, diffuse, extra);
}

// Per-owner sums of the unfolded block counts (one block; owners < FR_MAX_SHARD_RANKS).
__global__ __launch_bounds__(256) void k_owner_counts(FrameUniforms U, const uint32_t* __restrict__ bcount,
                                                      uint32_t* __restrict__ owner_counts) {
  __shared__ uint32_t acc[64];
  if (threadIdx.x < 64) acc[threadIdx.x] = 0;
  __syncthreads();
  const int gx = (U.width + 15) / 16, gy = (U.height + 15) / 16;
  uint32_t local = 0;
  int cur = -1;
  for (int b = threadIdx.x; b < gx * gy; b += blockDim.x) {
    const int bx = b % gx, by = b / gx;
    const int o = shard_owner(U, shard_tile_of(U, bx * 16, by * 16));
    if (o != cur) {
      if (cur >= 0 && local) atomicAdd(&acc[cur], local);
      cur = o;
      local = 0;
    }
    local += bcount[b];
  }
  if (cur >= 0 && local) atomicAdd(&acc[cur], local);
  __syncthreads();
  if (threadIdx.x < 64) owner_counts[threadIdx.x] = acc[threadIdx.x];
}

void launch_owner_counts(const FrameUniforms& U, const uint32_t* bcount, uint32_t* owner_counts, hipStream_t stream) {
  hipLaunchKernelGGL(k_owner_counts, dim3(1), dim3(256), 0, stream, U, bcount, owner_counts);
}

// The log-polar mask (samplingStep.cu:180-182) is a pure function of the pixel, the gaze and the
// screen size: it is evaluated by k_logpolar_mask only when one of those (or the mode) changes and
// read by k_sampling from then on.

// The inverse map depends on (u, v) only, and (u, v) takes ceil(W / 4) ceil(H / 4) values for W H pixels:
// k_logpolar_inv evaluates inverse_log_polar once per (u, v) into lp_inv (its four transcendentals), and
// k_logpolar_mask looks each pixel's up there instead, with the same result bit for bit (4K: 0.52 M
// evaluations against 8.3 M; the forward map's three stay per pixel).
size_t logpolar_inv_words(int W, int H) {
  return 2 * (size_t)ceilf((float)W * 0.25f) * (size_t)ceilf((float)H * 0.25f);
}
__global__ __launch_bounds__(256) void k_logpolar_inv(FrameUniforms U, float lpL, int nu, int nv, u2* __restrict__ inv) {
  const f2 bs = U.screen * 0.25f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nu * nv; i += gridDim.x * blockDim.x)
    inv[i] = inverse_log_polar(u2{(uint32_t)(i % nu), (uint32_t)(i / nu)}, U.gaze, bs, lpL);
}
FR_DEV uint32_t logpolar_on_tab(const FrameUniforms& U, f2 bs, float lpL, uint32_t x, uint32_t y, int nu,
                                const u2* __restrict__ inv) {
  u2 li{x, y};
  u2 uv = forward_log_polar(li, U.gaze, bs, lpL);
  // (inverse_log_polar's range test, then its value for this (u, v))
  const u2 xy = (float)uv.x >= bs.x || (float)uv.y >= bs.y ? u2{0xFFFFFFFFu, 0xFFFFFFFFu} : inv[(size_t)uv.y * nu + uv.x];
  f2 dv = U.mask_mode == MASK_LOGPOLAR ? mk2((float)(li.x - xy.x), (float)(li.y - xy.y))
                                       : mk2((float)(int32_t)(li.x - xy.x), (float)(int32_t)(li.y - xy.y));
  return length(dv) < sqrtf(length(mk2(1.5f, 1.5f))) ? 1u : 0u;
}

// 16 consecutive mask bytes per lane, one 16-byte store (a byte store per lane wrote ~24 B of HBM per
// pixel: WRITE_SIZE 199 MB for the 8.3 MB 4K mask).
__global__ __launch_bounds__(256) void k_logpolar_mask(FrameUniforms U, float lpL, int nu, const u2* __restrict__ inv,
                                                       uint8_t* __restrict__ lp) {
  const size_t N = (size_t)U.width * U.height;
  const f2 bs = U.screen * 0.25f;
  const uint32_t W = (uint32_t)U.width;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g * 16 < N; g += (size_t)gridDim.x * blockDim.x) {
    const size_t p0 = g * 16;
    uint32_t x = (uint32_t)(p0 % W), y = (uint32_t)(p0 / W);
    if (p0 + 16 <= N) {
      // one pixel at a time (the f64 transcendentals need most of the registers: an unrolled body spilled
      // 336 B per lane to scratch), the bytes gathered in two 64-bit words
      unsigned long long lo = 0, hi = 0;
#pragma unroll 1
      for (int b = 0; b < 16; b++) {
        const unsigned long long bit = (unsigned long long)logpolar_on_tab(U, bs, lpL, x, y, nu, inv) << (8 * (b & 7));
        if (b < 8) lo |= bit; else hi |= bit;
        if (++x == W) { x = 0; y++; }
      }
      *reinterpret_cast<uint4*>(lp + p0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    } else {
      for (size_t p = p0; p < N; p++) {
        lp[p] = (uint8_t)logpolar_on_tab(U, bs, lpL, x, y, nu, inv);
        if (++x == W) { x = 0; y++; }
      }
    }
  }
}

void launch_sampling(const FrameUniforms& U, const DevScene& sc, const f4* position, const f4* depth,
                     const f4* depth_cache, f4* weight, const f4* normal, const f4* diffuse, f4* extra, uint8_t* mask,
                     const uint8_t* gclass, unsigned long long* words, uint32_t* counts, int write_extra,
                     uint8_t* lp_cache, uint32_t* lp_inv, bool lp_refresh, uint32_t* bcount, hipStream_t stream) {
  if (lp_refresh) {
    const size_t N = (size_t)U.width * U.height;
    const float lpL = log_polar_L(U.gaze, U.screen * 0.25f);
    const int nu = (int)ceilf((float)U.width * 0.25f), nv = (int)ceilf((float)U.height * 0.25f);
    u2* inv = reinterpret_cast<u2*>(lp_inv);
    hipLaunchKernelGGL(k_logpolar_inv, dim3((unsigned)std::min((nu * nv + 255) / 256, 8192)), dim3(256), 0, stream, U,
                       lpL, nu, nv, inv);
    hipLaunchKernelGGL(k_logpolar_mask, dim3((unsigned)std::min<size_t>((N / 16 + 256) / 256, 8192)), dim3(256), 0,
                       stream, U, lpL, nu, inv, lp_cache);
  }
  dim3 grid((U.width + 15) / 16, (U.height + 15) / 16);
  hipLaunchKernelGGL(U.front_need ? k_sampling<true> : k_sampling<false>, grid, dim3(256), 0, stream, U, sc, position, depth, depth_cache, weight, normal,
                     diffuse, extra, mask, gclass, words, counts, write_extra, lp_cache, bcount);
}

// ------------------------------------------------------------------------------------------
// Entry 2: compaction (warpSort.cu:67-169 -> ballots + a two-level exclusive scan). The list is
// class-major (refraction, reflection, diffuse, miss), tile order inside a class;
// ray_count = number of active pixels (warpSort.cu:76-82, step 30).
// ------------------------------------------------------------------------------------------
// One-wave scans: every block is a single wave64, so the scans never wait for a whole CU's worth of
// free wave slots (1024-thread blocks sat ~0.6 ms behind the reconstruction kernels of the previous
// frame in the pipelined loop, on the frame's critical path).
#define SCAN_TILE 1024
#define SCAN_PER_LANE (SCAN_TILE / 64)

FR_DEV uint32_t wave_inclusive_scan(uint32_t x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

// Exclusive prefix of each count inside its SCAN_TILE tile; tile_sum[tile] = the tile's total.
__global__ __launch_bounds__(64) void k_scan_tiles(const uint32_t* __restrict__ counts, uint32_t n,
                                                   uint32_t* __restrict__ local_prefix, uint32_t* __restrict__ tile_sum) {
  const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_LANE;
  uint32_t v[SCAN_PER_LANE];
  uint32_t sum = 0;
#pragma unroll
  for (int k = 0; k < SCAN_PER_LANE; k++) {
    v[k] = base + k < n ? counts[base + k] : 0u;
    sum += v[k];
  }
  const uint32_t incl = wave_inclusive_scan(sum);
  uint32_t run = incl - sum;
#pragma unroll
  for (int k = 0; k < SCAN_PER_LANE; k++) {
    if (base + k < n) local_prefix[base + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 63) tile_sum[blockIdx.x] = incl;
}

// Tile totals -> exclusive tile prefixes, and ray_count = the grand total (one wave).
__global__ __launch_bounds__(64) void k_scan_top(uint32_t* __restrict__ tile_sum, uint32_t ntiles,
                                                 uint32_t* __restrict__ ray_count) {
  const uint32_t per = (ntiles + 63) / 64, base = threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t k = 0; k < per; k++) sum += base + k < ntiles ? tile_sum[base + k] : 0u;
  const uint32_t incl = wave_inclusive_scan(sum);
  uint32_t run = incl - sum;
  for (uint32_t k = 0; k < per; k++) {
    if (base + k < ntiles) {
      const uint32_t t = tile_sum[base + k];
      tile_sum[base + k] = run;  // becomes the tile prefix
      run += t;
    }
  }
  if (threadIdx.x == 63) *ray_count = incl;
}

__global__ __launch_bounds__(256) void k_scatter(const unsigned long long* __restrict__ words,
                                                 const uint32_t* __restrict__ local_prefix,
                                                 const uint32_t* __restrict__ tile_prefix, int W,
                                                 uint32_t* __restrict__ active, uint32_t* __restrict__ ray_count) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t nb = (size_t)gridDim.x * gridDim.y;
  const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  // ray_count[c] (c = 1, 2, 3) = the start of class c in the class-major list, for the megakernel's
  // work queue (per-class ranges, the refraction class's chunk size)
  if (b == 0 && threadIdx.x < 3) {
    const size_t ci = (threadIdx.x + 1) * nb;
    ray_count[threadIdx.x + 1] = local_prefix[ci] + tile_prefix[ci / SCAN_TILE];
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const unsigned long long m = words[(b * 4 + wv) * 4 + c];
    if (!((m >> lane) & 1ull)) continue;
    const size_t ci = c * nb + b;
    uint32_t pos = local_prefix[ci] + tile_prefix[ci / SCAN_TILE];
    for (int w2 = 0; w2 < wv; w2++) pos += (uint32_t)__popcll(words[(b * 4 + w2) * 4 + c]);
    pos += (uint32_t)__popcll(m & below);
    const int x = blockIdx.x * 16 + (lane & 15);
    const int y = blockIdx.y * 16 + wv * 4 + (lane >> 4);
    active[pos] = (uint32_t)y * W + x;
  }
}

// Rebuild the wave ballots from a host-written mask (tests / external samplers).
__global__ __launch_bounds__(256) void k_mask_words(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ gclass,
                                                    int W, int H, unsigned long long* __restrict__ words,
                                                    uint32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = blockIdx.x * 16 + (lane & 15);
  const int y = blockIdx.y * 16 + wv * 4 + (lane >> 4);
  bool on = x < W && y < H && mask[(size_t)y * W + x] != 0;
  int cls = (x < W && y < H) ? gclass[(size_t)y * W + x] : 3;
  publish_ballots(on, cls, words, counts);
}

void launch_mask_words(const uint8_t* mask, const uint8_t* gclass, int W, int H, unsigned long long* words,
                       uint32_t* counts, hipStream_t stream) {
  dim3 grid((W + 15) / 16, (H + 15) / 16);
  hipLaunchKernelGGL(k_mask_words, grid, dim3(256), 0, stream, mask, gclass, W, H, words, counts);
}

size_t compaction_tiles(int W, int H) {
  size_t nb = (size_t)((W + 15) / 16) * ((H + 15) / 16);
  return (4 * nb + SCAN_TILE - 1) / SCAN_TILE;
}

void launch_compaction(int W, int H, const unsigned long long* words, const uint32_t* counts, uint32_t* local_prefix,
                       uint32_t* tile_sum, uint32_t* ray_count, uint32_t* active, hipStream_t stream) {
  dim3 grid((W + 15) / 16, (H + 15) / 16);
  const uint32_t n = 4 * grid.x * grid.y;
  const uint32_t ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(64), 0, stream, counts, n, local_prefix, tile_sum);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(64), 0, stream, tile_sum, ntiles, ray_count);
  hipLaunchKernelGGL(k_scatter, grid, dim3(256), 0, stream, words, local_prefix, tile_sum, W, active, ray_count);
}

// ------------------------------------------------------------------------------------------
// JumpFlooding. The state of a seeded pixel (alpha >= 1) is its current seed's coord texel (sx, sy) =
// ((x + 0.5) / W, (y + 0.5) / H) (cpFS.glsl: gl_FragCoord.st / screenSize) as two fp32 words with their
// (always clear) sign bits set, exactly the values the reference's coordTex holds; an unseeded pixel's
// .x is +inf (its .y its own sy). One 8-byte word per pixel replaces the reference's two RGBA32F textures
// per pass, and a candidate needs no table or texture gather. An unseeded or out-of-image candidate has
// an infinite distance, so no candidate needs a flag test (jfFS skips both: "a < 1" and outside [0, 1)).
// The alpha > 0 case of cpFS (.a in (0, 1)) only sets the current pixel's starting distance, which jfFS
// ignores while .a < 1: it needs no state. The seed's pixel is recovered exactly as floor(sx * W)
// (sx*W = x + 0.5 within 2^-8 for W < 2^15).
// ------------------------------------------------------------------------------------------
#define JFA_FLAG 0x80000000u
#define JFA_UNSEEDED 0x7F800000u  // +inf in .x

FR_DEV f2 frag_uv(uint32_t x, uint32_t y, f2 screen) { return mk2(((float)x + 0.5f) / screen.x, ((float)y + 0.5f) / screen.y); }
FR_DEV float jfa_coord(uint32_t w) { return fabsf(__uint_as_float(w)); }  // coordinates are > 0: |x| clears the flag
FR_DEV bool jfa_seeded(uint32_t wx) { return wx != JFA_UNSEEDED; }

__global__ void k_jfa_init(const f4* __restrict__ in, u2* __restrict__ state, int W, int H, f2 screen) {
  // 32-bit pixel indices (fr_create keeps W H below 2^26): one 32-bit division per pixel, not a 64-bit one
  const uint32_t N = (uint32_t)W * (uint32_t)H;
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x) {
    const float a = in[p].w;
    const uint32_t y = p / (uint32_t)W;
    const f2 uv = frag_uv(p - y * (uint32_t)W, y, screen);
    state[p] = a >= 1.0f ? u2{__float_as_uint(uv.x) | JFA_FLAG, __float_as_uint(uv.y) | JFA_FLAG}
                         : u2{JFA_UNSEEDED, __float_as_uint(uv.y)};
  }
}

// (sqrt_le_bound: fr_math.h.)

// One jfFS pass at `step` (FR/shader/jfFS.glsl:12-58). The reference walks the 8 neighbours in
// order and takes one when the pixel is not yet seeded or when distance() (sqrt of the fp32 sum of
// squares) is strictly smaller. That is: among the current seed (if seeded) and the valid neighbours
// in tap order, the first one whose sqrtf(d2) is minimal. sqrtf is monotone, so the minimum is
// sqrtf(min d2), and an element reaches it iff d2 <= sqrt_le_bound(sqrtf(min d2)): one sqrt per
// pixel and pass instead of one per improving candidate, same result bit for bit.
// A seeded state carries the sign bit on both words, so |s| - m = -(s + m) exactly (rounding is
// symmetric) and its d2 is (s.x + m.x)^2 + (s.y + m.y)^2 on the raw words, bit for bit; an unseeded or
// out-of-image candidate (.x = +inf) has d2 = +inf, never below a seeded one's.
typedef float jfa_v2 __attribute__((ext_vector_type(2)));
FR_DEV u2 jfa_pick(const u2 (&nb)[9], f2 me) {
  float d2[9];
  float dmin = INFINITY;
  const jfa_v2 m = {me.x, me.y};
#pragma unroll
  for (int i = 0; i < 9; i++) {
    // (dx, dy) and their squares as packed pairs (v_pk_add_f32 / v_pk_mul_f32: the same IEEE operations, two
    // per instruction; a pass is VALU-bound)
    const jfa_v2 c = {__uint_as_float(nb[i].x), __uint_as_float(nb[i].y)};
    const jfa_v2 dd = c + m;
    const jfa_v2 sq = dd * dd;
    d2[i] = sq.x + sq.y;
    dmin = fminf(dmin, d2[i]);
  }
  u2 r = nb[0];
  if (dmin != INFINITY) {  // (nothing seeded around: unchanged)
    const float bound = sqrt_le_bound(sqrtf(dmin));
#pragma unroll
    for (int i = 8; i >= 0; i--)
      if (d2[i] <= bound) r = nb[i];
  }
  return r;
}

// jfa_pick with the validity of the candidates' rows above and below (up: nb[1..3], down: nb[6..8]) known to
// be the same on every lane of the wave (k_jfa_step's rows are): an invalid row's three candidates are neither
// evaluated nor selected (they would be +inf: the result is jfa_pick's, bit for bit). At 4K the step-2048 pass
// has one valid row of three for 95 % of its pixels, the step-1024 pass two of three.
FR_DEV u2 jfa_pick_rows(const u2 (&nb)[9], f2 me, bool up, bool down) {
  float d2[9];
  float dmin = INFINITY;
  const jfa_v2 m = {me.x, me.y};
  auto dist = [&](int i) {
    const jfa_v2 c = {__uint_as_float(nb[i].x), __uint_as_float(nb[i].y)};
    const jfa_v2 dd = c + m;
    const jfa_v2 sq = dd * dd;
    d2[i] = sq.x + sq.y;
    dmin = fminf(dmin, d2[i]);
  };
  dist(0); dist(4); dist(5);
  if (up) { dist(1); dist(2); dist(3); }
  if (down) { dist(6); dist(7); dist(8); }
  u2 r = nb[0];
  if (dmin != INFINITY) {
    const float bound = sqrt_le_bound(sqrtf(dmin));
    if (down) {
      if (d2[8] <= bound) r = nb[8];
      if (d2[7] <= bound) r = nb[7];
      if (d2[6] <= bound) r = nb[6];
    }
    if (d2[5] <= bound) r = nb[5];
    if (d2[4] <= bound) r = nb[4];
    if (up) {
      if (d2[3] <= bound) r = nb[3];
      if (d2[2] <= bound) r = nb[2];
      if (d2[1] <= bound) r = nb[1];
    }
    if (d2[0] <= bound) r = nb[0];
  }
  return r;
}

// JFA_SKIP: rows outside the image neither loaded nor evaluated (wave-uniform tests), in the passes of fewer than 4
// rows per thread only (the large steps, whose rows mostly fall outside). In the 4-row passes, where nearly every row
// is inside, the per-row branches kept the 18 loads from issuing together: steps 30 -> 36 us, the JFA stage 0.54 ->
// 0.64 ms; in the step-2048 pass 63 -> 48 us (r06l, profiles/r06_jfa/).
#ifndef JFA_SKIP
#define JFA_SKIP 1
#endif

// A thread computes JFA_ROWS pixels of one column, `step` rows apart: pixel (x, y) reads rows
// y - step, y, y + step, so JFA_ROWS such pixels share their rows and read JFA_ROWS + 2 of them
// instead of 3 JFA_ROWS. A pass is bound by these re-reads (the 66 MB state at 4K is served from
// the Infinity Cache): 3 -> 1.5 row reads per pixel. Rows are grouped by residue: group g holds
// rows base + k step, base = (g / step) JFA_ROWS step + g % step. The pixel's own texel centre
// comes from a table (ftab: ((x + 0.5) / W) for x < W, then ((y + 0.5) / H), correctly rounded on
// the host) instead of two divisions.
// JFA_ROWS = min(4, ceil(H / step)): the large steps have fewer rows to share.
template <int JFA_ROWS>
__global__ __launch_bounds__(256) void k_jfa_step(const u2* __restrict__ src, u2* __restrict__ dst, int W, int H,
                                                  int step, const float* __restrict__ ftab, int xcd) {
  // xcd: the blocks of one XCD take one contiguous run of the row-major block order, so a block's left and
  // right taps (x -+ step, the neighbouring blocks for steps below 512) and its groups' shared rows are
  // mostly in the L2 that fetched them for its neighbours (round-robin order puts them on other XCDs)
  const uint32_t t = xcd ? xcd_tile(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y) : blockIdx.y * gridDim.x + blockIdx.x;
  const int x = (int)(t % gridDim.x) * 64 + (threadIdx.x & 63);
  // (g, hence base and every row's validity, is the same on all lanes of a wave)
  const int g = __builtin_amdgcn_readfirstlane((int)(t / gridDim.x) * 4 + (threadIdx.x >> 6));
  const int base = (g / step) * (JFA_ROWS * step) + g % step;
  if (x >= W || base >= H) return;
  const bool inl = x - step >= 0, inr = x + step < W;
  const int xl = inl ? x - step : x, xr = inr ? x + step : x;
  // rows base + (m - 1) step, m = 0 .. JFA_ROWS + 1: the states at x - step, x, x + step
  u2 L[JFA_ROWS + 2], C[JFA_ROWS + 2], R[JFA_ROWS + 2];
  bool in[JFA_ROWS + 2];
  // 32-bit byte offsets from the kernel-argument base (the 4K state is 66 MB): scalar-base loads
  const char* sb = reinterpret_cast<const char*>(src);
  auto ld = [&](uint32_t e) { return *reinterpret_cast<const u2*>(sb + e * 8u); };
#pragma unroll
  for (int m = 0; m < JFA_ROWS + 2; m++) {
    const int yr = base + (m - 1) * step;
    in[m] = yr >= 0 && yr < H;
#if JFA_SKIP
    if (JFA_ROWS < 4 && !in[m]) {  // (wave-uniform)
      L[m] = C[m] = R[m] = u2{JFA_UNSEEDED, 0u};
      continue;
    }
#endif
    const uint32_t row = (uint32_t)(in[m] ? yr : base) * (uint32_t)W;
    L[m] = ld(row + (uint32_t)xl);
    C[m] = ld(row + (uint32_t)x);
    R[m] = ld(row + (uint32_t)xr);
    // taps outside the image are no candidates (jfFS skips them): an unseeded state in their place
    L[m].x = in[m] && inl ? L[m].x : JFA_UNSEEDED;
    C[m].x = in[m] ? C[m].x : JFA_UNSEEDED;
    R[m].x = in[m] && inr ? R[m].x : JFA_UNSEEDED;
  }
#pragma unroll
  for (int k = 0; k < JFA_ROWS; k++) {
    const int y = base + k * step;
    if (y < H) {
      // the current seed first, then the neighbours in jfFS order (-,-) (0,-) (+,-) (-,0) (+,0) (-,+) (0,+) (+,+)
      const u2 nb[9] = {C[k + 1], L[k], C[k], R[k], L[k + 1], R[k + 1], L[k + 2], C[k + 2], R[k + 2]};
      *reinterpret_cast<u2*>(reinterpret_cast<char*>(dst) + ((uint32_t)y * (uint32_t)W + (uint32_t)x) * 8u) =
          (JFA_SKIP && JFA_ROWS < 4) ? jfa_pick_rows(nb, mk2(ftab[x], ftab[W + y]), in[k], in[k + 2])
                                     : jfa_pick(nb, mk2(ftab[x], ftab[W + y]));
    }
  }
}

int jfa_rows(int H, int step) { return std::min(4, (H + step - 1) / step); }
int jfa_row_groups(int H, int step) {
  // groups of jfa_rows rows `step` apart covering 0 .. H-1 (bands of jfa_rows * step rows)
  const int band = jfa_rows(H, step) * step;
  return ((H + band - 1) / band) * step;
}

__global__ void k_jfa_final(const u2* __restrict__ state, const f4* __restrict__ in, f4* __restrict__ coord,
                            f4* __restrict__ color, int W, int H, f2 screen) {
  const size_t N = (size_t)W * H;
  for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
    const u2 s = state[p];
    // (a pixel no seed reached keeps its own texel: cpFS's coord)
    const float sx = jfa_seeded(s.x) ? jfa_coord(s.x) : ((float)(p % (size_t)W) + 0.5f) / screen.x;
    const float sy = jfa_coord(s.y);
    const uint32_t ix = min((uint32_t)floorf(sx * screen.x), (uint32_t)W - 1);
    const uint32_t iy = min((uint32_t)floorf(sy * screen.y), (uint32_t)H - 1);
    const f4 c = in[(size_t)iy * W + ix];
    coord[p] = mk4(sx, sy, 0.0f, c.w);
    color[p] = c;
  }
}

// k_jfa_final for the Sibson run form: one wave per 64 columns of a row writes the JFA outputs and,
// from the colours it just gathered, the row's block prefix sums P and block totals T that
// k_sibson_prefix would compute (the same scan, the same sums), saving that kernel's re-read of the colour.
// OUT = false: JFA_COORD is not written here (Sibson reads the seeds from the state); the context writes it with
// k_jfa_coord only when something asks for it (133 MB of stores per 4K frame saved). JFA_COLOR is written: Sibson's
// border taps and seed fallbacks read it. (Computing those as in[seed pixel] instead made k_sibson_runs 0.66 -> 0.84 ms:
// each border tap then waits on a state load, a division and a dependent colour load.)
template <bool OUT>
__global__ __launch_bounds__(64) void k_jfa_final_prefix(const u2* __restrict__ state, const f4* __restrict__ in,
                                                         f4* __restrict__ coord, f4* __restrict__ color,
                                                         f4* __restrict__ P, f4* __restrict__ T, int W, int H, int NB,
                                                         f2 screen) {
  const int lane = threadIdx.x;
  const int j = blockIdx.y, B = blockIdx.x;
  const int col = B * 64 + lane;
  f3 v = mk3(0.0f);
  if (col < W) {
    const size_t p = (size_t)j * W + col;
    const u2 s = state[p];
    // (a pixel no seed reached keeps its own texel: cpFS's coord)
    const float sx = jfa_seeded(s.x) ? jfa_coord(s.x) : ((float)col + 0.5f) / screen.x;
    const float sy = jfa_coord(s.y);
    const uint32_t ix = min((uint32_t)floorf(sx * screen.x), (uint32_t)W - 1);
    const uint32_t iy = min((uint32_t)floorf(sy * screen.y), (uint32_t)H - 1);
    const f4 c = in[(size_t)iy * W + ix];
    if (OUT) coord[p] = mk4(sx, sy, 0.0f, c.w);
    color[p] = c;
    v = xyz(c);
  }
  f3 incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float tx = __shfl_up(incl.x, o, 64), ty = __shfl_up(incl.y, o, 64), tz = __shfl_up(incl.z, o, 64);
    if (lane >= o) incl = incl + mk3(tx, ty, tz);
  }
  if (col <= W) P[(size_t)j * (W + 1) + col] = mk4(incl - v, 0.0f);
  if (lane == 63) T[(size_t)j * NB + B] = mk4(incl, 0.0f);
}

int jfa_max_step(int W, int H) {
  int m = 1;
  while (m * 2 < W || m * 2 < H) m *= 2;  // FR/JumpFlooding.cpp:33-34
  return m;
}

int sibson_prefix_blocks(int W);
const u2* launch_jfa(const f4* in, u2* stateA, u2* stateB, f4* coord, f4* color, const float* ftab, int W, int H,
                     f4* sibP, f4* sibT, bool outputs, hipStream_t stream) {
  const size_t N = (size_t)W * H;
  int blocks = (int)std::min<size_t>((N + 255) / 256, 8192);
  f2 screen = mk2((float)W, (float)H);
  static const int xcd = [] { const char* v = getenv("FOVRT_JFA_XCD"); return v ? atoi(v) : 1; }();
  // (Measured and not kept: the first pass forming the seeds' states from the input's alpha itself, without
  // k_jfa_init: 138-154 us for that pass against 62 + 33 us for the pass and the init, its 16-byte texel
  // reads per tap doubling the pass's traffic.)
  hipLaunchKernelGGL(k_jfa_init, dim3(blocks), dim3(256), 0, stream, in, stateA, W, H, screen);
  u2* a = stateA;
  u2* b = stateB;
  // (Measured and not kept: steps 8, 4, 2, 1 fused in one launch over 64x32 tiles with a 15-texel halo in
  // LDS, 151 us against 4 x 31 us. A pass is VALU-bound, ~130 instructions per pixel, not HBM-bound, and the
  // halos add 29 % of pixel work.)
  for (int step = jfa_max_step(W, H); step >= 1; step /= 2) {
    dim3 grid((W + 63) / 64, (jfa_row_groups(H, step) + 3) / 4);
    auto k = jfa_rows(H, step) == 4 ? k_jfa_step<4> : jfa_rows(H, step) == 3 ? k_jfa_step<3>
           : jfa_rows(H, step) == 2 ? k_jfa_step<2> : k_jfa_step<1>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, stream, a, b, W, H, step, ftab, xcd);
    std::swap(a, b);
  }
  if (sibP) {
    const int NB = sibson_prefix_blocks(W);
    hipLaunchKernelGGL(outputs ? k_jfa_final_prefix<true> : k_jfa_final_prefix<false>, dim3(NB, H), dim3(64), 0, stream,
                       a, in, coord, color, sibP, sibT, W, H, NB, screen);
  } else {
    hipLaunchKernelGGL(k_jfa_final, dim3(blocks), dim3(256), 0, stream, a, in, coord, color, W, H, screen);
  }
  return a;  // the final state (k_sibson_runs reads its seeds from it)
}

// JFA_COORD of a JumpFlooding run whose final pass did not write it (launch_jfa, outputs = false): k_jfa_final's
// coord from the final state, with the seed colour's alpha from JFA_COLOR (which that pass wrote)
__global__ void k_jfa_coord(const u2* __restrict__ state, const f4* __restrict__ color, f4* __restrict__ coord, int W,
                            int H, f2 screen) {
  const size_t N = (size_t)W * H;
  for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
    const u2 s = state[p];
    const float sx = jfa_seeded(s.x) ? jfa_coord(s.x) : ((float)(p % (size_t)W) + 0.5f) / screen.x;
    coord[p] = mk4(sx, jfa_coord(s.y), 0.0f, color[p].w);
  }
}
void launch_jfa_coord(const u2* state, const f4* color, f4* coord, int W, int H, hipStream_t stream) {
  const size_t N = (size_t)W * H;
  hipLaunchKernelGGL(k_jfa_coord, dim3((unsigned)std::min<size_t>((N + 255) / 256, 8192)), dim3(256), 0, stream, state,
                     color, coord, W, H, mk2((float)W, (float)H));
}


// (sqrt_le_bound, above: the disc test "sqrtf(r2) > d" of Sibson is "r2 > sqrt_le_bound(d)".)

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
// in LDS for the lane that takes the pixel in ranked order (which re-read coord before); the results go back
// to LDS at their raster slot and the block stores its tile row by row (a wave's lanes had stored 16-B texels
// scattered over the tile in radius order: 2.07x the output's bytes written). Tiles are handed to the XCDs in
// contiguous bands (xcd_tile), so the prefix rows neighbouring tiles share are fetched into one L2.
#ifndef SIBR_XCD
#define SIBR_XCD 2
#endif
#ifndef SIBR_LDS_STORE
#define SIBR_LDS_STORE 0
#endif
#ifndef SIBR_STATE
#define SIBR_STATE 1
#endif
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
  __shared__ f4 slot[SIBR_THREADS];      // raster slot: the pixel's (seed.x, seed.y, d), then its result
  __shared__ uint8_t done[SIBR_THREADS];  // the slot holds a result to store
  const int tid = threadIdx.x;
#if SIBR_XCD == 2
  // super-tiles of 4 x 4 tiles: the 16 blocks of one super-tile are dispatched to one XCD one after another (block b
  // runs on XCD b % 8), so the prefix rows its tiles share are fetched into one L2; consecutive super-tiles of the
  // raster order go to different XCDs, so every XCD's work spreads over the whole image (horizontal bands per XCD
  // load the XCDs unevenly: the fovea's discs are small, the periphery's large). 1-D grid; blocks past the image exit.
  const uint32_t sgx = (tiles_x + 3) / 4;
  const uint32_t b = blockIdx.x, sup = (b / 128) * 8 + (b % 8), sub = (b / 8) % 16;
  const uint32_t tx = (sup % sgx) * 4 + (sub % 4), ty = (sup / sgx) * 4 + (sub / 4);
  if (tx >= tiles_x || ty >= tiles_y) return;
  const int bx0 = (int)tx * SIBR_TILE, by0 = (int)ty * SIBR_TILE;
#else
  const uint32_t t = SIBR_XCD ? xcd_tile(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y) : blockIdx.y * gridDim.x + blockIdx.x;
  const int bx0 = (int)(t % gridDim.x) * SIBR_TILE, by0 = (int)(t / gridDim.x) * SIBR_TILE;
#endif
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
#if SIBR_LDS_STORE
    slot[p] = r;
    done[p] = 1;
#else
    out[(size_t)py * W + px] = r;
#endif
  }
#if SIBR_LDS_STORE
  __syncthreads();
  if (done[tid]) out[(size_t)y * W + x] = slot[tid];
#endif
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
                        uint32_t* strips, f4* out, int W, int H, bool prefix_fresh, bool strip, bool coord_owed,
                        hipStream_t stream) {
  const int NB = sibson_prefix_blocks(W);
  strip = strip && NB <= SIBG_MAX_BLOCKS;
  const float strip_half = strip ? SIBS_HALF : INFINITY;  // (FOVRT_SIB_STRIP=0: k_sibson_wide for every wide disc)
  // mid: the wide discs without a closed form of at most 2 SIBS_HALF rows go to the strips too
  static const int mid_env = [] { const char* v = getenv("FOVRT_SIB_STRIP_MID"); return v ? atoi(v) : 0; }();
  const int mid = strip ? mid_env : 0;
  const f2 screen = mk2((float)W, (float)H);
  if (!prefix_fresh)  // (k_jfa_final_prefix wrote P and T with the colours)
    hipLaunchKernelGGL(k_sibson_prefix, dim3(NB, H), dim3(64), 0, stream, color, P, T, W, NB);
  const StripLayout L(W, H);
  // the lists' counters, the strip flags, the row range and the claim counters, in one launch (five
  // hipMemsetAsync calls were seven fill launches of ~5 us each, back to back on the JFA -> Sibson chain)
  hipLaunchKernelGGL(k_sibson_clear, dim3(std::min<uint32_t>((L.total - L.flags + 255) / 256, 64u)), dim3(256), 0, stream,
                     wide, strips, L.flags, L.rows, L.total);
  const uint32_t tiles_x = (uint32_t)(W + SIBR_TILE - 1) / SIBR_TILE, tiles_y = (uint32_t)(H + SIBR_TILE - 1) / SIBR_TILE;
#if SIBR_XCD == 2
  const uint32_t supers = ((tiles_x + 3) / 4) * ((tiles_y + 3) / 4);
  dim3 grid(((supers + 7) / 8) * 8 * 16);
#else
  dim3 grid(tiles_x, tiles_y);
#endif
  const bool fresh = state && prefix_fresh;
  const int owed = fresh && coord_owed ? 1 : 0;  // (JFA_COORD is written whenever the prefix sums are not fresh)
  if ((SIBR_STATE && fresh) || owed)
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

// Pull level s (size 2^s at (S, 2^s - 1)) from level s+1 (or the input when s+1 == e).
__global__ void k_pull_level(PPArgs a, int s) {
  const int n = 1 << s;
  const int total = n * n;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int lx = t % n, ly = t / n;
    const int ox[4] = {0, 1, 1, 0}, oy[4] = {0, 0, 1, 1};
    int hitCount = 0;
    f4 f = mk4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int cx = 2 * lx + ox[i], cy = 2 * ly + oy[i];
      f4 r = (s + 1 == a.e) ? pp_in(a, cx, cy) : a.pull[(size_t)((1 << (s + 1)) - 1 + cy) * a.AW + a.S + cx];
      if (r.w > 0.0f) { f = f + r; hitCount++; }
    }
    if (hitCount > 0) f = f / f.w;
    f = mk4(f.x, f.y, f.z, hitCount > 0 ? 1.0f : 0.0f);
    a.pull[(size_t)((1 << s) - 1 + ly) * a.AW + a.S + lx] = f;
  }
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
// Same texel arithmetic as k_pull_level (pull_combine), so the atlas is bit-identical; the 12
// dependent launches of the 4K pyramid become 2 (levels 11..6 over 64x64 input tiles, then 5..0).
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
  if (a.e == 0) {  // 1x1 screen: pull/push degenerate to a copy
    hipMemcpyAsync(out, in, sizeof(f4), hipMemcpyDeviceToDevice, stream);
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
// 2*stepWidth halo are staged in LDS once (each texel is read by up to 25 pixels). POW2: c_phi,
// n_phi, p_phi and stepWidth^2 are powers of two (always so in ATrous::render: 1, 2^-k, 1, 4^k), so
// the divisions are exact multiplications by the reciprocal: bit-identical, without the division
// sequence.
FR_DEV float at_dot(f4 t) {
  return __builtin_fmaf(t.w, t.w, __builtin_fmaf(t.z, t.z, __builtin_fmaf(t.y, t.y, t.x * t.x)));
}

template <bool TILE, bool POW2>
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
    const float ec = fmaxf(POW2 ? dist2 * inv_c : dist2 / c_phi, 0.0f);
    f4 ntmp = TILE ? ln[lq] : nrm[q];
    t = nval - ntmp;
    dist2 = fmaxf(POW2 ? at_dot(t) * inv_sw2 : at_dot(t) / (stepWidth * stepWidth), 0.0f);
    const float en = fmaxf(POW2 ? dist2 * inv_n : dist2 / n_phi, 0.0f);
    f4 ptmp = TILE ? lp[lq] : pos[q];
    t = pval - ptmp;
    dist2 = at_dot(t);
    const float ep = fmaxf(POW2 ? dist2 * inv_p : dist2 / p_phi, 0.0f);
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
// is bit-identical to k_atrous<true, POW2>. Interior blocks (every tap inside the image) run
// without bounds tests.
template <bool POW2>
FR_DEV float at_weight(f4 cval, f4 nval, f4 pval, f4 ctmp, f4 ntmp, f4 ptmp, float inv_c, float inv_n, float inv_p,
                       float c_phi, float n_phi, float p_phi, float kern) {
  f4 t = cval - ctmp;
  float dist2 = at_dot(t);
  const float ec = fmaxf(POW2 ? dist2 * inv_c : dist2 / c_phi, 0.0f);
  t = nval - ntmp;
  dist2 = fmaxf(at_dot(t), 0.0f);  // stepWidth^2 = 1
  const float en = fmaxf(POW2 ? dist2 * inv_n : dist2 / n_phi, 0.0f);
  t = pval - ptmp;
  dist2 = at_dot(t);
  const float ep = fmaxf(POW2 ? dist2 * inv_p : dist2 / p_phi, 0.0f);
  return gl_exp(-(ec + en + ep)) * kern;
}

template <bool POW2, bool CHECK>
FR_DEV void atrous_rows2(const f4* lp, const f4* ln, const f4* lc, int u, int v, int x, int y, int W, int H, float inv_c,
                         float inv_n, float inv_p, float c_phi, float n_phi, float p_phi, f4& outA, f4& outB) {
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
          const float wk = at_weight<POW2>(cA, nA, pA, c, n, p, inv_c, inv_n, inv_p, c_phi, n_phi, p_phi,
                                           c_at_kernel[(2 - oy) * 5 + ox + 2]);
          sA = mk4(__builtin_fmaf(c.x, wk, sA.x), __builtin_fmaf(c.y, wk, sA.y), __builtin_fmaf(c.z, wk, sA.z),
                   __builtin_fmaf(c.w, wk, sA.w));
          wA += wk;
        }
      }
      if (r <= 4) {
        const int oy = 2 - r;
        if (colok && (!CHECK || (y + 1 + oy >= 0 && y + 1 + oy < H))) {
          const float wk = at_weight<POW2>(cB, nB, pB, c, n, p, inv_c, inv_n, inv_p, c_phi, n_phi, p_phi,
                                           c_at_kernel[(2 - oy) * 5 + ox + 2]);
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

template <bool POW2>
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
  if (interior) atrous_rows2<POW2, false>(lp, ln, lc, u, v, x, y, W, H, inv_c, inv_n, inv_p, c_phi, n_phi, p_phi, a, b);
  else atrous_rows2<POW2, true>(lp, ln, lc, u, v, x, y, W, H, inv_c, inv_n, inv_p, c_phi, n_phi, p_phi, a, b);
  out[(size_t)y * W + x] = a;
  if (y + 1 < H) out[(size_t)(y + 1) * W + x] = b;
}

static bool pow2f(float v) {
  int e;
  return v > 0.0f && std::isfinite(v) && std::frexp(v, &e) == 0.5f;
}

void launch_atrous(const f4* pos, const f4* nrm, const f4* col, f4* out, int W, int H, float c_phi, float n_phi,
                   float p_phi, float stepWidth, hipStream_t stream) {
  dim3 grid((W + 15) / 16, (H + 15) / 16);
  const bool pw = pow2f(c_phi) && pow2f(n_phi) && pow2f(p_phi) && pow2f(stepWidth * stepWidth) &&
                  pow2f(1.0f / c_phi) && pow2f(1.0f / n_phi) && pow2f(1.0f / p_phi) &&
                  pow2f(1.0f / (stepWidth * stepWidth));
  const int sw = (int)stepWidth;
  // FOVRT_ATROUS_ROWS2=0: k_atrous for the stepWidth-1 pass too (A/B of the two-row kernel)
  static const bool rows2 = [] {
    const char* v = getenv("FOVRT_ATROUS_ROWS2");
    return !v || atoi(v) != 0;
  }();
  static const int xcd = [] {
    const char* v = getenv("FOVRT_ATROUS_XCD");
    return v ? atoi(v) != 0 : 1;
  }();
  if (rows2 && stepWidth == 1.0f) {
    dim3 g2((W + 15) / 16, (H + 31) / 32);
    if (pw) hipLaunchKernelGGL((k_atrous_rows2<true>), g2, dim3(256), 0, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, xcd);
    else hipLaunchKernelGGL((k_atrous_rows2<false>), g2, dim3(256), 0, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, xcd);
    return;
  }
  const int tw = 16 + 4 * sw;
  const size_t lds = (size_t)3 * tw * tw * sizeof(f4);
  const bool tile = sw >= 1 && lds <= 64 * 1024;
  if (tile && pw)
    hipLaunchKernelGGL((k_atrous<true, true>), grid, dim3(256), lds, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, stepWidth);
  else if (tile)
    hipLaunchKernelGGL((k_atrous<true, false>), grid, dim3(256), lds, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, stepWidth);
  else if (pw)
    hipLaunchKernelGGL((k_atrous<false, true>), grid, dim3(256), 0, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, stepWidth);
  else
    hipLaunchKernelGGL((k_atrous<false, false>), grid, dim3(256), 0, stream, pos, nrm, col, out, W, H, c_phi, n_phi, p_phi, stepWidth);
}

// ------------------------------------------------------------------------------------------
// LogPolarTransform (FR/Log_Polar_Transform.cpp:40-106; shader/logPolarCPFS.glsl,
// shader/ilogPolarCPFS.glsl): the forward pass stores, at the log-polar texel uv = Forward(xy),
// the input sampled (GL_LINEAR, REPEAT) at the round trip Inverse(uv) / screen; the inverse pass
// gives every pixel the log-polar texel of its own Forward(xy). Both dispatch (W/32)*32 x (H/32)*32
// invocations (glDispatchCompute(W/32, H/32) with 32x32 groups); other texels keep their value.
// Every invocation that stores to a texel uv stores in(Inverse(uv)), so the forward pass's
// concurrent stores agree and the result is deterministic. GLSL PI = 3.141592, screen-sized
// distances to the corners, bufferSize = 0.25 * screen, ivec2 (truncating) coordinates.
// ------------------------------------------------------------------------------------------
struct LPArgs {
  f2 screen, buf, gaze;
  float L;
  int W, H, nx, ny;  // dispatched extent
};
#define LP_PI 3.141592f

FR_DEV void lp_forward(const LPArgs& p, int x, int y, int& u, int& v) {
  const f2 xp = mk2((float)x - p.gaze.x, (float)y - p.gaze.y);
  u = f2i_sat(fr_pow(fr_log(length(xp)) / p.L, 4.0f) * p.buf.x);
  v = f2i_sat((fr_atan2(xp.y, xp.x) + ((2.0f * LP_PI) * (xp.y < 0.0f ? 1.0f : 0.0f))) * (p.buf.y / (2.0f * LP_PI)));
}

FR_DEV void lp_inverse(const LPArgs& p, int u, int v, int& x, int& y) {
  x = y = -1;
  if ((float)u < 0.0f || (float)u >= p.buf.x * 2.0f || (float)v < 0.0f || (float)v >= p.buf.y * 2.0f) return;
  const float B = (2.0f * LP_PI) / p.buf.y;
  const float K = fr_pow((float)u / p.buf.x, 1.0f / 4.0f);
  const float e = fr_exp(p.L * K);
  x = f2i_sat(e * fr_cos(B * (float)v) + p.gaze.x);
  y = f2i_sat(e * fr_sin(B * (float)v) + p.gaze.y);
}

__global__ void k_logpolar_forward(LPArgs p, const f4* __restrict__ in, f4* __restrict__ fwd) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 32 + (threadIdx.x >> 5);
  if (x >= p.nx || y >= p.ny) return;
  int u, v, sx, sy;
  lp_forward(p, x, y, u, v);
  lp_inverse(p, u, v, sx, sy);
  const f4 data = bilinear_repeat([&](int i, int j) { return in[(size_t)j * p.W + i]; }, p.W, p.H,
                                  (float)sx / p.screen.x, (float)sy / p.screen.y);
  if (u >= 0 && u < p.W && v >= 0 && v < p.H) fwd[(size_t)v * p.W + u] = data;  // imageStore drops the rest
}

__global__ void k_logpolar_inverse(LPArgs p, const f4* __restrict__ fwd, f4* __restrict__ inv) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 32 + (threadIdx.x >> 5);
  if (x >= p.nx || y >= p.ny) return;
  int u, v;
  lp_forward(p, x, y, u, v);
  inv[(size_t)y * p.W + x] = (u >= 0 && u < p.W && v >= 0 && v < p.H) ? fwd[(size_t)v * p.W + u] : mk4(0, 0, 0, 0);
}

void launch_logpolar(const f4* in, f4* fwd, f4* inv, int W, int H, f2 gaze, hipStream_t stream) {
  LPArgs p;
  p.screen = mk2((float)W, (float)H);
  p.buf = mk2((float)W * 0.25f, (float)H * 0.25f);
  p.gaze = gaze;
  const float l1 = length(gaze), l2 = length(p.screen - gaze);
  const float l3 = length(mk2(gaze.x, p.screen.y - gaze.y)), l4 = length(mk2(p.screen.x - gaze.x, gaze.y));
  p.L = fr_log(fmaxf(fmaxf(l1, l2), fmaxf(l3, l4)));
  p.W = W; p.H = H;
  p.nx = (W / 32) * 32; p.ny = (H / 32) * 32;
  if (p.nx == 0 || p.ny == 0) return;
  dim3 grid(W / 32, H / 32);
  hipLaunchKernelGGL(k_logpolar_forward, grid, dim3(1024), 0, stream, p, in, fwd);
  hipLaunchKernelGGL(k_logpolar_inverse, grid, dim3(1024), 0, stream, p, fwd, inv);
}

// ------------------------------------------------------------------------------------------
// Final composite (the reference's side-by-side display of renderAll, FR/main.cpp:26-113, for the
// stereo configuration): nviews W x H images -> one (nviews * W) x H image, view v in columns
// [v W, (v+1) W).
// ------------------------------------------------------------------------------------------
__global__ void k_composite(const f4* __restrict__ views, int nviews, int W, int H, f4* __restrict__ out) {
  const size_t N = (size_t)W * H * nviews;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < N; i += (size_t)gridDim.x * blockDim.x) {
    const size_t ow = (size_t)W * nviews;
    const size_t y = i / ow, X = i % ow;
    const size_t v = X / W, x = X % W;
    out[i] = views[(v * H + y) * W + x];
  }
}

void launch_composite(const f4* views, int nviews, int W, int H, f4* out, hipStream_t stream) {
  const size_t N = (size_t)W * H * nviews;
  hipLaunchKernelGGL(k_composite, dim3((unsigned)std::min<size_t>((N + 255) / 256, 16384)), dim3(256), 0, stream,
                     views, nviews, W, H, out);
}

// ------------------------------------------------------------------------------------------
// Tile sharding: pack this rank's tiles of an RGBA32F buffer into a contiguous slab (tile-major,
// T*T slots per tile, owned tiles in increasing order) and unpack another rank's slab into place.
// ------------------------------------------------------------------------------------------
FR_DEV bool shard_slot(const FrameUniforms& U, int rank, int x, int y, size_t& slot) {
  const int T = U.shard_tile;
  const uint32_t m = U.shard_map[shard_tile_of(U, x, y)];
  if ((int)(m >> 24) != rank) return false;
  slot = (size_t)(m & 0xFFFFFFu) * T * T + (size_t)(y % T) * T + (x % T);
  return true;
}

__global__ void k_shard_pack(FrameUniforms U, const f4* __restrict__ buf, f4* __restrict__ slab) {
  const size_t N = (size_t)U.width * U.height;
  for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
    size_t slot;
    if (shard_slot(U, U.shard_rank, (int)(p % U.width), (int)(p / U.width), slot)) slab[slot] = buf[p];
  }
}

__global__ void k_shard_unpack(FrameUniforms U, int rank, const f4* __restrict__ slab, f4* __restrict__ buf) {
  const size_t N = (size_t)U.width * U.height;
  for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
    size_t slot;
    if (shard_slot(U, rank, (int)(p % U.width), (int)(p / U.width), slot)) buf[p] = slab[slot];
  }
}

void launch_shard_pack(const FrameUniforms& U, const f4* buf, f4* slab, hipStream_t stream) {
  const size_t N = (size_t)U.width * U.height;
  hipLaunchKernelGGL(k_shard_pack, dim3((unsigned)std::min<size_t>((N + 255) / 256, 8192)), dim3(256), 0, stream, U,
                     buf, slab);
}

void launch_shard_unpack(const FrameUniforms& U, int rank, const f4* slab, f4* buf, hipStream_t stream) {
  const size_t N = (size_t)U.width * U.height;
  hipLaunchKernelGGL(k_shard_unpack, dim3((unsigned)std::min<size_t>((N + 255) / 256, 8192)), dim3(256), 0, stream,
                     U, rank, slab, buf);
}

}  // namespace fr
