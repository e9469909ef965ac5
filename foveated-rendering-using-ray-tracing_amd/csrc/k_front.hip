// k_front.hip — the front stages of a frame, image space, on gfx950 (HBM-bandwidth bound, no MFMA):
//   sampling_step (entry 1)        FR/cuda/samplingStep.cu:72-239 + shared_helper_funcs.h:60-300,376-412
//   the EXTRA heat map, the owner counts of a sharded frame, the log-polar mask
//   warp_sort compaction (entry 2) FR/cuda/warpSort.cu:67-169 -> wave ballot + scan (ray_count bit-exact)
#include <hip/hip_runtime.h>
#include <cmath>
#include "fr_device.h"
#include "k_launch.h"

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
// DEVBOX: the scene box comes from device memory (dev_box: min, max; GeoUpdateState::box or ::xbox), where an
// enqueued geometry update (fr_update_geometry_enqueue) leaves it and the host no longer knows it; else from
// sc.bbox_min / bbox_max as the host passed them (dev_box is not read). Same bytes either way.
template <bool DEVBOX>
FR_DEV void saliency_cells(const FrameUniforms& U, const DevScene& sc, const float* __restrict__ dev_box,
                           const f4* __restrict__ diffuse, const f4* __restrict__ normal,
                           const f4* __restrict__ depth, float (&cellf)[16][8], float (&cellg)[4][16]) {
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
      const f3 bmin = DEVBOX ? mk3(dev_box[0], dev_box[1], dev_box[2]) : sc.bbox_min;
      const f3 bmax = DEVBOX ? mk3(dev_box[3], dev_box[4], dev_box[5]) : sc.bbox_max;
      float theta = lengthc(bmax - bmin) * 0.005f;  // samplingStep.ptx:785-795
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

// LOCAL: a tile-local front (fr_set_front_local); the whole-screen instance carries none of it.
// MOTION: this frame's G-buffer ran its motion form (fr_set_motion_reprojection): WEIGHT.z holds the distance of the
// reprojected point, where it was a frame ago, from the previous eye, and the history depth is tested against that.
// DEVBOX: saliency_cells' (a context that has enqueued a geometry update).
template <bool LOCAL, bool MOTION, bool DEVBOX>
__global__ __launch_bounds__(256) void k_sampling(FrameUniforms U, DevScene sc, const f4* __restrict__ position,
                                                  const f4* __restrict__ depth, const f4* __restrict__ depth_cache,
                                                  f4* __restrict__ weight, const f4* __restrict__ normal,
                                                  const f4* __restrict__ diffuse, f4* __restrict__ extra,
                                                  uint8_t* __restrict__ mask, const uint8_t* __restrict__ gclass,
                                                  unsigned long long* __restrict__ words, uint32_t* __restrict__ counts,
                                                  int write_extra, const uint8_t* __restrict__ lp_cache,
                                                  uint32_t* __restrict__ bcount,
                                                  const float* __restrict__ dev_box) {
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
  if (saliency_used) saliency_cells<DEVBOX>(U, sc, dev_box, diffuse, normal, depth, cellf, cellg);
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
        float diff = prev_depth.x - (MOTION ? wgt.z : lengthc(xyz(pos) - U.prev_eye));  // samplingStep.ptx:258-273
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

// The heat map a k_sampling launch left unwritten (ctx_frame.cpp, fr_ctx::extra): the same cell phase and
// per-pixel expressions over that launch's inputs (its uniforms, DIFFUSE, NORMAL, DEPTH and WEIGHT.xy, which
// the sampling does not change), so EXTRA is what that launch would have stored, bit for bit.
template <bool DEVBOX>
__global__ __launch_bounds__(256) void k_extra(FrameUniforms U, DevScene sc, const f4* __restrict__ depth,
                                               const f4* __restrict__ weight, const f4* __restrict__ normal,
                                               const f4* __restrict__ diffuse, f4* __restrict__ extra,
                                               const float* __restrict__ dev_box) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = blockIdx.x * 16 + (lane & 15);
  const int y = blockIdx.y * 16 + wv * 4 + (lane >> 4);
  __shared__ float cellf[16][8];
  __shared__ float cellg[4][16];
  saliency_cells<DEVBOX>(U, sc, dev_box, diffuse, normal, depth, cellf, cellg);
  if (x < U.width && y < U.height) {
    const size_t p = (size_t)y * U.width + x;
    const f4 wgt = weight[p];
    extra[p] = heat_map(pixel_saliency(cellf, x, y, mk2(wgt.x, wgt.y)));
  }
}

void launch_extra(const FrameUniforms& U, const DevScene& sc, const f4* depth, const f4* weight, const f4* normal,
                  const f4* diffuse, f4* extra, const float* dev_box, hipStream_t stream) {
  dim3 grid((U.width + 15) / 16, (U.height + 15) / 16);
  auto k = dev_box ? k_extra<true> : k_extra<false>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, stream, U, sc, depth, weight, normal, diffuse, extra, dev_box);
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

// The eccentricity mask (FR_MASK_ECCENTRIC, ecc_sampled in fr_device.h) into the context's cached mask, which
// k_sampling then reads as it reads the log-polar one. k_logpolar_mask's store: 16 mask bytes per lane in one 16-byte
// store, a scalar tail. Bit operations, two products and a sum per pixel: no transcendentals, no LDS. r2 is read
// once, from the controller's record when the context holds a ray budget (r2_dev), else from the argument.
__global__ __launch_bounds__(256) void k_ecc_mask(f2 gaze, const float* __restrict__ r2_dev, float r2_host,
                                                  uint32_t floor_ranks, uint32_t W, size_t N, uint8_t* __restrict__ lp) {
  const float r2 = r2_dev ? *r2_dev : r2_host;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g * 16 < N; g += (size_t)gridDim.x * blockDim.x) {
    const size_t p0 = g * 16;
    uint32_t x = (uint32_t)(p0 % W), y = (uint32_t)(p0 / W);
    if (p0 + 16 <= N) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int b = 0; b < 16; b++) {
        w[b >> 2] |= (ecc_sampled(x, y, gaze, r2, floor_ranks) ? 1u : 0u) << (8 * (b & 3));
        if (++x == W) { x = 0; y++; }
      }
      *reinterpret_cast<uint4*>(lp + p0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (size_t p = p0; p < N; p++) {
        lp[p] = ecc_sampled(x, y, gaze, r2, floor_ranks) ? 1 : 0;
        if (++x == W) { x = 0; y++; }
      }
    }
  }
}

void launch_ecc_mask(f2 gaze, const FovState* st, float r2, uint32_t floor_ranks, int W, int H, uint8_t* lp_cache,
                     hipStream_t stream) {
  const size_t N = (size_t)W * H;
  hipLaunchKernelGGL(k_ecc_mask, dim3((unsigned)std::min<size_t>((N / 16 + 256) / 256, 8192)), dim3(256), 0, stream, gaze,
                     st ? &st->r2 : nullptr, r2, floor_ranks, (uint32_t)W, N, lp_cache);
}

// The ray budget's controller (the rule is beside fr_set_foveation in include/fovrt.h), one lane, ahead of the mask
// generation on the stream of the front stages. reset: the first launch after fr_set_foveation starts from r2_0 and
// reads no count. count: the ray count of the compaction that followed the previous sampling launch, or NULL when
// there was none (r2 is kept).
__global__ __launch_bounds__(64) void k_fov_control(FovState* __restrict__ st, const uint32_t* __restrict__ count, int reset,
                                                    float r2_0, uint32_t budget, float tolerance, float r2_max) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (reset) {
    st->r2 = r2_0;
    st->last_count = 0u;
    st->adjusted = 0u;
    st->held = 0u;
  } else if (count) {
    const uint32_t n = *count;
    bool held;
    st->r2 = fov_next_r2(st->r2, n, budget, tolerance, r2_max, &held);
    st->last_count = n;
    if (held) st->held++; else st->adjusted++;
  }
}

void launch_fov_control(FovState* st, const uint32_t* count, bool reset, float r2_0, uint32_t budget, float tolerance,
                        float r2_max, hipStream_t stream) {
  hipLaunchKernelGGL(k_fov_control, dim3(1), dim3(64), 0, stream, st, count, reset ? 1 : 0, r2_0, budget, tolerance, r2_max);
}

// A caller's sampling mask (FR_MASK_CALLER) into the context's copy: a 16-byte load, every byte normalised to 0 / 1,
// a 16-byte store; a scalar tail. src is 16-byte aligned (fr_set_sampling_mask refuses other device pointers).
FR_DEV uint32_t bytes_to_01(uint32_t w) { return ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u) >> 7; }
// (src may be dst: a host mask is copied into place first; every lane reads its bytes before it writes them)
__global__ __launch_bounds__(256) void k_mask_take(const uint8_t* src, uint8_t* dst, size_t N) {
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g * 16 < N; g += (size_t)gridDim.x * blockDim.x) {
    const size_t p0 = g * 16;
    if (p0 + 16 <= N) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + p0);
      *reinterpret_cast<uint4*>(dst + p0) = make_uint4(bytes_to_01(v.x), bytes_to_01(v.y), bytes_to_01(v.z), bytes_to_01(v.w));
    } else {
      for (size_t p = p0; p < N; p++) dst[p] = src[p] != 0 ? 1 : 0;
    }
  }
}

void launch_mask_take(const uint8_t* src, uint8_t* dst, int W, int H, hipStream_t stream) {
  const size_t N = (size_t)W * H;
  hipLaunchKernelGGL(k_mask_take, dim3((unsigned)std::min<size_t>((N / 16 + 256) / 256, 8192)), dim3(256), 0, stream, src,
                     dst, N);
}

void launch_sampling(const FrameUniforms& U, const DevScene& sc, const f4* position, const f4* depth,
                     const f4* depth_cache, f4* weight, const f4* normal, const f4* diffuse, f4* extra, uint8_t* mask,
                     const uint8_t* gclass, unsigned long long* words, uint32_t* counts, int write_extra,
                     uint8_t* lp_cache, uint32_t* lp_inv, bool lp_refresh, uint32_t* bcount, bool motion,
                     const float* dev_box, hipStream_t stream) {
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
  auto pick = [&](auto local) {
    constexpr bool L = decltype(local)::value;
    return dev_box ? (motion ? k_sampling<L, true, true> : k_sampling<L, false, true>)
                      : (motion ? k_sampling<L, true, false> : k_sampling<L, false, false>);
  };
  auto k = U.front_need ? pick(std::true_type{}) : pick(std::false_type{});
  hipLaunchKernelGGL(k, grid, dim3(256), 0, stream, U, sc, position, depth, depth_cache, weight, normal, diffuse, extra,
                     mask, gclass, words, counts, write_extra, lp_cache, bcount, dev_box);
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

}  // namespace fr
