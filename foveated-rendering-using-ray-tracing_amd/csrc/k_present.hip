// k_present.hip — present: one RGBA32F image to packed 8-bit texels (fr_present_enqueue, fr_present_enqueue_device),
// through a homography, and over the blend of two images. The rules are present_texel, present_warp_texel and
// present_blend_fetch in fr_math.h, the text the fr_present_*_pack functions run on the host. Every kernel here has
// the output side of k_present.h: a grid sized to the output, one lane per four consecutive texels of one output row,
// one 16-byte store per full lane. No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include "k_launch.h"
#include "k_present.h"

namespace fr {

// The pack is bound by memory (20 B moved per texel, a dozen operations): four 16-byte loads, issued together, and one
// 16-byte store per lane, so a wave reads 4 KiB and writes 1 KiB of one row, both contiguous. (The alpha float is never
// used, so the loads come out as 12 bytes of each 16-byte texel.)
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_pack(const f4* __restrict__ src, int W, int H, int lanes,
                                                                         bool bgra, bool top_down,
                                                                         uint32_t* __restrict__ out) {
  const PresentLane l = present_lane(W, H, lanes, top_down, out);
  if (!l.in) return;
  const f4* in = src + (size_t)l.y * W + l.x;
  if (l.full) {
    const f4 t0 = in[0], t1 = in[1], t2 = in[2], t3 = in[3];
    present_store(l.o, make_uint4(present_texel(t0, bgra), present_texel(t1, bgra), present_texel(t2, bgra),
                                  present_texel(t3, bgra)));
  } else {
    for (int k = 0; l.x + k < W; k++) l.o[k] = present_texel(in[k], bgra);
  }
}

// out: W * H words, 16-byte aligned.
void launch_present_pack(const f4* src, int W, int H, int format, void* out, hipStream_t stream) {
  const int lanes = (W + 3) / 4;
  const PresentFormat f = present_format(format);
  hipLaunchKernelGGL(k_present_pack, present_grid(lanes, H), present_block(), 0, stream, src, W, H, lanes, f.bgra,
                     f.top_down, static_cast<uint32_t*>(out));
}

// k_present_warp: each texel of the ow x oh output sampled from the W x H source through a homography by
// present_warp_texel. Everything the call gives travels by value in the kernel arguments (the coefficients sit in
// scalar registers), so the launch is ordered by its stream alone and keeps nothing of the caller's alive. Input side:
// plain per-lane 16-byte gathers. For the maps this is made for (a timewarp, a crop, a scale) a lane's four points lie
// along one source row or close to it and neighbouring lanes read neighbouring texels, so the taps a wave shares come
// out of L1 / L2; a tap of weight zero is never loaded (the identity reads what k_present_pack reads).
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_warp(const f4* __restrict__ src, const WarpArgs a,
                                                                         uint32_t* __restrict__ out) {
  // (present_lane's steps in place, which keeps the instructions this kernel was measured with: through the descriptor
  // its identity fell outside the earlier build's windows in the one session that timed it, MEASUREMENTS.md "Present,
  // folded")
  const int j = (int)(blockIdx.x * PRESENT_BX + threadIdx.x);
  const int r = (int)(blockIdx.y * PRESENT_BY + threadIdx.y);
  if (j >= a.lanes || r >= a.oh) return;
  const int x = 4 * j;
  const int y = a.top_down ? a.oh - 1 - r : r;
  const int W = a.W;
  // (present_warp_texel calls it with 0 <= i < W and 0 <= row < H only)
  const auto fetch = [src, W](int i, int row) { return src[(size_t)row * W + i]; };
  const auto texel = [&](int xx) { return present_warp_texel(fetch, W, a.H, a.h, xx, y, a.bgra); };
  uint32_t* o = out + (size_t)r * a.ow + x;
  if (x + 4 <= a.ow) {
    present_store(o, make_uint4(texel(x), texel(x + 1), texel(x + 2), texel(x + 3)));
  } else {
    for (int k = 0; x + k < a.ow; k++) o[k] = texel(x + k);
  }
}

// As launch_present_pack, with the homography h[9] and the output size (1 <= ow <= W, 1 <= oh <= H, checked by the
// callers with the coefficients); out: ow * oh words, 16-byte aligned.
void launch_present_warp(const f4* src, int W, int H, int format, const float* h, int ow, int oh, void* out,
                         hipStream_t stream) {
  const WarpArgs a = warp_args(h, W, H, ow, oh, format);
  hipLaunchKernelGGL(k_present_warp, present_grid(a.lanes, oh), present_block(), 0, stream, src, a,
                     static_cast<uint32_t*>(out));
}

// k_present_blend: the pack over the virtual image of present_blend_fetch: each texel is `inner` inside the gaze's
// disc, `outer` beyond the ring, their smoothstep mix between. The blend travels by value in the kernel arguments. A
// texel reads `inner` only where s < 1 and `outer` only where s > 0, behind branches on s: a wave that lies wholly
// inside the disc or wholly beyond the ring (one row of 256 texels: all of them outside a ring zone) skips the other
// source's loads and moves the pack's 20 B per texel, and the division of the ramp is behind the ring's branch. A lane
// forms its four weights first and issues its loads together: the four-texel body is present_blend_fetch's steps
// written out, not four calls of it, which waits between the texels.
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_blend(const f4* __restrict__ inner,
                                                                          const f4* __restrict__ outer, int W, int H,
                                                                          int lanes, bool bgra, bool top_down,
                                                                          const PresentBlend blend,
                                                                          uint32_t* __restrict__ out) {
  const PresentLane l = present_lane(W, H, lanes, top_down, out);
  if (!l.in) return;
  const int x = l.x, sr = l.y;
  if (l.full) {
    // the weights, then every load, then the mixes
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
    present_store(l.o, make_uint4(present_texel(present_blend_mix(a0, b0, s0), bgra), present_texel(present_blend_mix(a1, b1, s1), bgra),
                                  present_texel(present_blend_mix(a2, b2, s2), bgra), present_texel(present_blend_mix(a3, b3, s3), bgra)));
  } else {
    // (called with 0 <= i < W and row = sr < H only)
    const auto fi = [inner, W](int i, int row) { return inner[(size_t)row * W + i]; };
    const auto fo = [outer, W](int i, int row) { return outer[(size_t)row * W + i]; };
    for (int k = 0; x + k < W; k++) l.o[k] = present_texel(present_blend_fetch(fi, fo, x + k, sr, blend), bgra);
  }
}

// k_present_blend_warp: k_present_warp whose fetch is the blended one, so the blend is evaluated at each source tap,
// before the bilinear filter.
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_blend_warp(const f4* __restrict__ inner,
                                                                               const f4* __restrict__ outer,
                                                                               const WarpArgs a, const PresentBlend blend,
                                                                               uint32_t* __restrict__ out) {
  const PresentLane l = present_lane(a.ow, a.oh, a.lanes, a.top_down, out);
  if (!l.in) return;
  const int W = a.W;
  // (present_warp_texel calls it with 0 <= i < W and 0 <= row < H only)
  const auto fi = [inner, W](int i, int row) { return inner[(size_t)row * W + i]; };
  const auto fo = [outer, W](int i, int row) { return outer[(size_t)row * W + i]; };
  const auto fetch = [&fi, &fo, &blend](int i, int row) { return present_blend_fetch(fi, fo, i, row, blend); };
  const auto texel = [&](int x) { return present_warp_texel(fetch, W, a.H, a.h, x, l.y, a.bgra); };
  if (l.full) {
    present_store(l.o, make_uint4(texel(l.x), texel(l.x + 1), texel(l.x + 2), texel(l.x + 3)));
  } else {
    for (int k = 0; l.x + k < a.ow; k++) l.o[k] = texel(l.x + k);
  }
}

// As launch_present_pack (h NULL: ow x oh is W x H) or launch_present_warp over the blend of two W x H sources; inner
// and outer may be the same image.
void launch_present_blend(const f4* inner, const f4* outer, int W, int H, int format, const PresentBlend& blend,
                          const float* h, int ow, int oh, void* out, hipStream_t stream) {
  const int lanes = (ow + 3) / 4;
  const dim3 grid = present_grid(lanes, oh), block = present_block();
  uint32_t* o = static_cast<uint32_t*>(out);
  if (h) {
    hipLaunchKernelGGL(k_present_blend_warp, grid, block, 0, stream, inner, outer, warp_args(h, W, H, ow, oh, format), blend, o);
    return;
  }
  const PresentFormat f = present_format(format);
  hipLaunchKernelGGL(k_present_blend, grid, block, 0, stream, inner, outer, W, H, lanes, f.bgra, f.top_down, blend, o);
}

}  // namespace fr
