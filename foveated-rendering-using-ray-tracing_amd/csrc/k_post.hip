// k_post.hip — what follows the reconstruction: LogPolarTransform, the multi-view composite, and the shard
// pack / unpack of a multi-GPU group.
#include <hip/hip_runtime.h>
#include <cmath>
#include "fr_device.h"
#include "k_launch.h"

namespace fr {

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
