// k_present_reproject.hip — the reprojected present (fr_present_enqueue_reprojected, _device): every texel of a W x H
// image moves to where the display camera sees its world-space hit point (POSITION), the nearest one wins a place,
// and the places nothing reaches take the fallback homography's texel. The rule is present_splat_place /
// present_resolve_word / present_warp_texel in fr_math.h, the text fr_present_reproject_pack runs on the host.
// Three launches on one in-order stream over a key image of the context: a clear of ow * oh keys to all ones, the
// scatter k_present_splat, and k_present_resolve, which has k_present_pack's output side. Everything the call gives
// travels by value in the kernels' arguments. No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "k_launch.h"
#include "k_present.h"

namespace fr {

struct SplatArgs {
  float vp[16];
  int W, H, ow, oh;
  bool bgra;
};

// One lane per source texel: a wave takes 64 consecutive texels of one row, 1 KiB of pos and 1 KiB of src, both
// contiguous, both loads issued before either is looked at. The scatter is one 64-bit unsigned minimum per texel that
// lands; its return value is dropped, so it is the form that sends nothing back. The minimum does not depend on the
// order of arrival, so the key image has one right content. For the motions this is made for (a head's 12 ms) the
// texels of a wave land on neighbouring keys of one or two rows: a wave's atomics cover a few contiguous 64-byte
// segments and few lanes share a key (several to one only where the display camera is farther away or a surface is
// seen at a flatter angle). ox, oy are inside the ow x oh output by present_splat_place's test, and ow * oh <= W * H
// keys are allocated.
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_splat(const f4* __restrict__ src,
                                                                              const f4* __restrict__ pos, const SplatArgs a,
                                                                              unsigned long long* __restrict__ keys) {
  const int i = (int)(blockIdx.x * PRESENT_BX + threadIdx.x);
  const int j = (int)(blockIdx.y * PRESENT_BY + threadIdx.y);
  if (i >= a.W || j >= a.H) return;
  const size_t at = (size_t)j * a.W + i;
  const f4 p = pos[at];
  const f4 t = src[at];
  int ox, oy;
  uint32_t depth;
  if (!present_splat_place(p, a.vp, a.ow, a.oh, &ox, &oy, &depth)) return;
  const unsigned long long key = present_splat_key(depth, present_texel(t, a.bgra));
  (void)atomicMin(keys + ((size_t)oy * a.ow + ox), key);
}

// The output side of k_present.h on the ow x oh output, written out. A full lane loads its four keys (32 contiguous bytes) together,
// before the first of them is looked at; a texel reads its four neighbours only where its own key is empty (one of the
// lane's own where it is one), and the source through the fallback homography only where the crack rule fails as well.
__global__ __launch_bounds__(PRESENT_BX* PRESENT_BY) void k_present_resolve(const f4* __restrict__ src,
                                                                            const unsigned long long* __restrict__ keys,
                                                                            const WarpArgs a, uint32_t* __restrict__ out) {
  // (present_lane's steps in place: through the descriptor the compiler took one more scalar register)
  const int j = (int)(blockIdx.x * PRESENT_BX + threadIdx.x);
  const int r = (int)(blockIdx.y * PRESENT_BY + threadIdx.y);
  if (j >= a.lanes || r >= a.oh) return;
  const int x = 4 * j;
  const int y = a.top_down ? a.oh - 1 - r : r;
  const int W = a.W, ow = a.ow;
  // (present_resolve_word calls it with 0 <= i < ow and 0 <= row < oh only, present_warp_texel with 0 <= i < W and
  // 0 <= row < H only)
  const auto key = [keys, ow](int i, int row) { return (uint64_t)keys[(size_t)row * ow + i]; };
  const auto fetch = [src, W](int i, int row) { return src[(size_t)row * W + i]; };
  const auto texel = [&](uint64_t c, int xx) {
    uint32_t w;
    if (present_resolve_word(c, key, ow, a.oh, xx, y, &w)) return w;
    return present_warp_texel(fetch, W, a.H, a.h, xx, y, a.bgra);
  };
  uint32_t* o = out + (size_t)r * ow + x;
  if (x + 4 <= ow) {
    const unsigned long long* kc = keys + (size_t)y * ow + x;
    const uint64_t c0 = kc[0], c1 = kc[1], c2 = kc[2], c3 = kc[3];
    // (the left and right neighbours inside the lane's span are the keys it holds)
    const auto own = [&](int i, int row) {
      if (row != y) return key(i, row);
      const int k = i - x;
      return k == 0 ? c0 : k == 1 ? c1 : k == 2 ? c2 : k == 3 ? c3 : key(i, row);
    };
    const auto texel4 = [&](uint64_t c, int xx) {
      uint32_t w;
      if (present_resolve_word(c, own, ow, a.oh, xx, y, &w)) return w;
      return present_warp_texel(fetch, W, a.H, a.h, xx, y, a.bgra);
    };
    present_store(o, make_uint4(texel4(c0, x), texel4(c1, x + 1), texel4(c2, x + 2), texel4(c3, x + 3)));
  } else {
    for (int k = 0; x + k < ow; k++) o[k] = texel(key(x + k, y), x + k);
  }
}

// format as launch_present_pack; the callers have checked the sizes (1 <= ow <= W <= 32767, 1 <= oh <= H <= 32767), vp
// and h. keys: W * H keys, 8-byte aligned; out: ow * oh words, 16-byte aligned.
void launch_present_reproject(const f4* src, const f4* pos, int W, int H, int format, const float* vp, const float* h,
                              int ow, int oh, unsigned long long* keys, void* out, hipStream_t stream) {
  if (hipMemsetAsync(keys, 0xFF, (size_t)ow * oh * sizeof(unsigned long long), stream) != hipSuccess) return;
  const WarpArgs a = warp_args(h, W, H, ow, oh, format);
  SplatArgs s;
  for (int k = 0; k < 16; k++) s.vp[k] = vp[k];
  s.W = W; s.H = H; s.ow = ow; s.oh = oh; s.bgra = a.bgra;
  hipLaunchKernelGGL(k_present_splat, present_grid(W, H), present_block(), 0, stream, src, pos, s, keys);
  hipLaunchKernelGGL(k_present_resolve, present_grid(a.lanes, oh), present_block(), 0, stream, src, keys, a,
                     static_cast<uint32_t*>(out));
}

}  // namespace fr
