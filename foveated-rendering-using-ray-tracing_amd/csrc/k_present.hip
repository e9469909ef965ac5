// k_present.hip — present: one RGBA32F image to packed 8-bit texels (fr_present_enqueue, fr_present_enqueue_device).
// The rule is present_unorm8 / present_texel in fr_math.h, the text fr_present_pack runs on the host. The kernel is
// bound by memory (20 B moved per texel, a dozen operations): no LDS, no atomics, a grid sized to the image, one lane
// per four consecutive texels of one output row (four 16-byte loads, one 16-byte store), so a wave reads 4 KiB and
// writes 1 KiB of one row, both contiguous.
#include <hip/hip_runtime.h>

#include "fr_device.h"
#include "k_launch.h"

namespace fr {

#define PRESENT_BX 64  // lanes along a row: one wave per block row
#define PRESENT_BY 4   // rows per block

// lanes = ceil(W / 4). Output row r is image row r, or H - 1 - r (top_down); out is tight, W words per row. A lane
// whose four texels are all inside the row writes them with one 16-byte store when W is a multiple of four (ALIGNED:
// every row of `out`, itself 16-byte aligned, then starts on a 16-byte boundary) and with word stores otherwise; the
// last lane of a row whose width is no multiple of four writes the W & 3 texels that are left. (Two instances, not a
// branch on W & 3: the compiler sank the fourth word's store out of both arms and left 12 + 4 bytes in each. The
// alpha float is never used, so the loads come out as 12 bytes of each 16-byte texel.)
template <bool ALIGNED>
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_pack(const f4* __restrict__ src, int W, int H, int lanes,
                                                                         bool bgra, bool top_down,
                                                                         uint32_t* __restrict__ out) {
  const int j = (int)(blockIdx.x * PRESENT_BX + threadIdx.x);
  const int r = (int)(blockIdx.y * PRESENT_BY + threadIdx.y);
  if (j >= lanes || r >= H) return;
  const int x = 4 * j;
  const int sr = top_down ? H - 1 - r : r;
  const f4* in = src + (size_t)sr * W + x;
  uint32_t* o = out + (size_t)r * W + x;
  if (x + 4 <= W) {
    const f4 t0 = in[0], t1 = in[1], t2 = in[2], t3 = in[3];
    const uint4 q = make_uint4(present_texel(t0, bgra), present_texel(t1, bgra), present_texel(t2, bgra),
                               present_texel(t3, bgra));
    if (ALIGNED) {
      *reinterpret_cast<uint4*>(o) = q;
    } else {
      o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    }
  } else {
    for (int k = 0; x + k < W; k++) o[k] = present_texel(in[k], bgra);
  }
}

// format: FR_PRESENT_RGBA8 (0) or FR_PRESENT_BGRA8 (1), FR_PRESENT_TOP_DOWN (0x100) or-ed in; the callers have checked
// it and the size (1..32767 each way, so the grid's y extent is at most 8192). out: W * H words, 16-byte aligned.
void launch_present_pack(const f4* src, int W, int H, int format, void* out, hipStream_t stream) {
  const int lanes = (W + 3) / 4;
  const dim3 grid((unsigned)((lanes + PRESENT_BX - 1) / PRESENT_BX), (unsigned)((H + PRESENT_BY - 1) / PRESENT_BY));
  const bool bgra = (format & 0xFF) == 1, top_down = (format & 0x100) != 0;
  if ((W & 3) == 0)
    hipLaunchKernelGGL(k_present_pack<true>, grid, dim3(PRESENT_BX, PRESENT_BY), 0, stream, src, W, H, lanes, bgra, top_down,
                       static_cast<uint32_t*>(out));
  else
    hipLaunchKernelGGL(k_present_pack<false>, grid, dim3(PRESENT_BX, PRESENT_BY), 0, stream, src, W, H, lanes, bgra, top_down,
                       static_cast<uint32_t*>(out));
}

// k_present_warp: the same output side on an ow x oh image, each texel sampled from the W x H source through a
// homography by present_warp_texel (fr_math.h), the function fr_present_warp_pack runs on the host. Everything the call
// gives travels by value in the kernel arguments (the coefficients sit in scalar registers), so the launch is ordered
// by its stream alone and keeps nothing of the caller's alive. Input side: plain per-lane 16-byte gathers, no LDS. For
// the maps this is made for (a timewarp, a crop, a scale) a lane's four points lie along one source row or close to
// it and neighbouring lanes read neighbouring texels, so the taps a wave shares come out of L1 / L2; a tap of weight
// zero is never loaded (the identity reads what k_present_pack reads). No atomics, no scratch.
struct WarpArgs {
  float h[9];
  int W, H, ow, oh, lanes;  // lanes = ceil(ow / 4)
  bool bgra, top_down;
};

template <bool ALIGNED>
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_warp(const f4* __restrict__ src, const WarpArgs a,
                                                                         uint32_t* __restrict__ out) {
  const int j = (int)(blockIdx.x * PRESENT_BX + threadIdx.x);
  const int r = (int)(blockIdx.y * PRESENT_BY + threadIdx.y);
  if (j >= a.lanes || r >= a.oh) return;
  const int x = 4 * j;
  const int y = a.top_down ? a.oh - 1 - r : r;
  const int W = a.W;
  // (present_warp_texel calls it with 0 <= i < W and 0 <= row < H only)
  const auto fetch = [src, W](int i, int row) { return src[(size_t)row * W + i]; };
  uint32_t* o = out + (size_t)r * a.ow + x;
  if (x + 4 <= a.ow) {
    const uint4 q = make_uint4(present_warp_texel(fetch, W, a.H, a.h, x, y, a.bgra),
                               present_warp_texel(fetch, W, a.H, a.h, x + 1, y, a.bgra),
                               present_warp_texel(fetch, W, a.H, a.h, x + 2, y, a.bgra),
                               present_warp_texel(fetch, W, a.H, a.h, x + 3, y, a.bgra));
    if (ALIGNED) {
      *reinterpret_cast<uint4*>(o) = q;
    } else {
      o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    }
  } else {
    for (int k = 0; x + k < a.ow; k++) o[k] = present_warp_texel(fetch, W, a.H, a.h, x + k, y, a.bgra);
  }
}

// As launch_present_pack, with the homography h[9] and the output size (1 <= ow <= W, 1 <= oh <= H, checked by the
// callers with the coefficients); out: ow * oh words, 16-byte aligned.
void launch_present_warp(const f4* src, int W, int H, int format, const float* h, int ow, int oh, void* out,
                         hipStream_t stream) {
  WarpArgs a;
  for (int k = 0; k < 9; k++) a.h[k] = h[k];
  a.W = W; a.H = H; a.ow = ow; a.oh = oh; a.lanes = (ow + 3) / 4;
  a.bgra = (format & 0xFF) == 1; a.top_down = (format & 0x100) != 0;
  const dim3 grid((unsigned)((a.lanes + PRESENT_BX - 1) / PRESENT_BX), (unsigned)((oh + PRESENT_BY - 1) / PRESENT_BY));
  if ((ow & 3) == 0)
    hipLaunchKernelGGL(k_present_warp<true>, grid, dim3(PRESENT_BX, PRESENT_BY), 0, stream, src, a, static_cast<uint32_t*>(out));
  else
    hipLaunchKernelGGL(k_present_warp<false>, grid, dim3(PRESENT_BX, PRESENT_BY), 0, stream, src, a, static_cast<uint32_t*>(out));
}

// k_present_blend: k_present_pack's shape (lanes, rows, stores, the tail lane) over the virtual image of
// present_blend_fetch (fr_math.h), the function fr_present_blend_pack runs on the host: each texel is `inner` inside
// the gaze's disc, `outer` beyond the ring, their smoothstep mix between. The blend travels by value in the kernel
// arguments. A texel reads `inner` only where s < 1 and `outer` only where s > 0, behind branches on s: a wave that
// lies wholly inside the disc or wholly beyond the ring (one row of 256 texels: all of them outside a ring zone)
// skips the other source's loads and moves the pack's 20 B per texel, and the division of the ramp is behind the
// ring's branch. A lane forms its four weights first and issues its loads together. No LDS, no atomics, no scratch.
template <bool ALIGNED>
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_blend(const f4* __restrict__ inner,
                                                                          const f4* __restrict__ outer, int W, int H,
                                                                          int lanes, bool bgra, bool top_down,
                                                                          const PresentBlend blend,
                                                                          uint32_t* __restrict__ out) {
  const int j = (int)(blockIdx.x * PRESENT_BX + threadIdx.x);
  const int r = (int)(blockIdx.y * PRESENT_BY + threadIdx.y);
  if (j >= lanes || r >= H) return;
  const int x = 4 * j;
  const int sr = top_down ? H - 1 - r : r;
  // (called with 0 <= i < W and row = sr < H only)
  const auto fi = [inner, W](int i, int row) { return inner[(size_t)row * W + i]; };
  const auto fo = [outer, W](int i, int row) { return outer[(size_t)row * W + i]; };
  uint32_t* o = out + (size_t)r * W + x;
  if (x + 4 <= W) {
    // present_blend_fetch's steps, each for the four texels: the weights, then every load, then the mixes
    const f4* in = inner + (size_t)sr * W + x;
    const f4* ou = outer + (size_t)sr * W + x;
    const float s0 = present_blend_weight(x, sr, blend), s1 = present_blend_weight(x + 1, sr, blend),
                s2 = present_blend_weight(x + 2, sr, blend), s3 = present_blend_weight(x + 3, sr, blend);
    const f4 z = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    f4 a0 = z, a1 = z, a2 = z, a3 = z, b0 = z, b1 = z, b2 = z, b3 = z;
    if (s0 < 1.0f) a0 = in[0];
    if (s1 < 1.0f) a1 = in[1];
    if (s2 < 1.0f) a2 = in[2];
    if (s3 < 1.0f) a3 = in[3];
    if (s0 > 0.0f) b0 = ou[0];
    if (s1 > 0.0f) b1 = ou[1];
    if (s2 > 0.0f) b2 = ou[2];
    if (s3 > 0.0f) b3 = ou[3];
    const uint4 q = make_uint4(present_texel(present_blend_mix(a0, b0, s0), bgra), present_texel(present_blend_mix(a1, b1, s1), bgra),
                               present_texel(present_blend_mix(a2, b2, s2), bgra), present_texel(present_blend_mix(a3, b3, s3), bgra));
    if (ALIGNED) {
      *reinterpret_cast<uint4*>(o) = q;
    } else {
      o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    }
  } else {
    for (int k = 0; x + k < W; k++) o[k] = present_texel(present_blend_fetch(fi, fo, x + k, sr, blend), bgra);
  }
}

// k_present_blend_warp: k_present_warp whose fetch is the blended one, so the blend is evaluated at each source tap,
// before the bilinear filter.
template <bool ALIGNED>
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_blend_warp(const f4* __restrict__ inner,
                                                                               const f4* __restrict__ outer,
                                                                               const WarpArgs a, const PresentBlend blend,
                                                                               uint32_t* __restrict__ out) {
  const int j = (int)(blockIdx.x * PRESENT_BX + threadIdx.x);
  const int r = (int)(blockIdx.y * PRESENT_BY + threadIdx.y);
  if (j >= a.lanes || r >= a.oh) return;
  const int x = 4 * j;
  const int y = a.top_down ? a.oh - 1 - r : r;
  const int W = a.W;
  // (present_warp_texel calls it with 0 <= i < W and 0 <= row < H only)
  const auto fi = [inner, W](int i, int row) { return inner[(size_t)row * W + i]; };
  const auto fo = [outer, W](int i, int row) { return outer[(size_t)row * W + i]; };
  const auto fetch = [&fi, &fo, &blend](int i, int row) { return present_blend_fetch(fi, fo, i, row, blend); };
  uint32_t* o = out + (size_t)r * a.ow + x;
  if (x + 4 <= a.ow) {
    const uint4 q = make_uint4(present_warp_texel(fetch, W, a.H, a.h, x, y, a.bgra),
                               present_warp_texel(fetch, W, a.H, a.h, x + 1, y, a.bgra),
                               present_warp_texel(fetch, W, a.H, a.h, x + 2, y, a.bgra),
                               present_warp_texel(fetch, W, a.H, a.h, x + 3, y, a.bgra));
    if (ALIGNED) {
      *reinterpret_cast<uint4*>(o) = q;
    } else {
      o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    }
  } else {
    for (int k = 0; x + k < a.ow; k++) o[k] = present_warp_texel(fetch, W, a.H, a.h, x + k, y, a.bgra);
  }
}

// As launch_present_pack (h NULL) or launch_present_warp over the blend of two W x H sources; inner and outer may be
// the same image.
void launch_present_blend(const f4* inner, const f4* outer, int W, int H, int format, const PresentBlend& blend,
                          const float* h, int ow, int oh, void* out, hipStream_t stream) {
  const bool bgra = (format & 0xFF) == 1, top_down = (format & 0x100) != 0;
  const int lanes = (ow + 3) / 4;
  const dim3 grid((unsigned)((lanes + PRESENT_BX - 1) / PRESENT_BX), (unsigned)((oh + PRESENT_BY - 1) / PRESENT_BY));
  const dim3 block(PRESENT_BX, PRESENT_BY);
  uint32_t* o = static_cast<uint32_t*>(out);
  if (!h) {  // ow x oh is W x H
    if ((W & 3) == 0)
      hipLaunchKernelGGL(k_present_blend<true>, grid, block, 0, stream, inner, outer, W, H, lanes, bgra, top_down, blend, o);
    else
      hipLaunchKernelGGL(k_present_blend<false>, grid, block, 0, stream, inner, outer, W, H, lanes, bgra, top_down, blend, o);
    return;
  }
  WarpArgs a;
  for (int k = 0; k < 9; k++) a.h[k] = h[k];
  a.W = W; a.H = H; a.ow = ow; a.oh = oh; a.lanes = lanes;
  a.bgra = bgra; a.top_down = top_down;
  if ((ow & 3) == 0)
    hipLaunchKernelGGL(k_present_blend_warp<true>, grid, block, 0, stream, inner, outer, a, blend, o);
  else
    hipLaunchKernelGGL(k_present_blend_warp<false>, grid, block, 0, stream, inner, outer, a, blend, o);
}

}  // namespace fr
