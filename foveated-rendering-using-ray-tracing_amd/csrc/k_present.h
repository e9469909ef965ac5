// k_present.h — what the present kernels (k_present.hip, k_present_reproject.hip) share: the block shape, the format,
// the arguments of a warped kernel, and the output side of a lane.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fovrt.h"
#include "fr_device.h"

namespace fr {

#define PRESENT_BX 64  // lanes along a row: one wave per block row
#define PRESENT_BY 4   // rows per block

inline dim3 present_block() { return dim3(PRESENT_BX, PRESENT_BY); }
// The grid over `across` lanes a row and `rows` rows. The callers have checked the sizes (1..32767 each way), so its y
// extent is at most 8192.
inline dim3 present_grid(int across, int rows) {
  return dim3((unsigned)((across + PRESENT_BX - 1) / PRESENT_BX), (unsigned)((rows + PRESENT_BY - 1) / PRESENT_BY));
}

// format: FR_PRESENT_RGBA8 or FR_PRESENT_BGRA8, FR_PRESENT_TOP_DOWN or-ed in (fr_present_enable has checked it).
struct PresentFormat {
  bool bgra, top_down;
};
inline PresentFormat present_format(int format) {
  return {(format & ~FR_PRESENT_TOP_DOWN) == FR_PRESENT_BGRA8, (format & FR_PRESENT_TOP_DOWN) != 0};
}

// What a kernel that samples the W x H source through a homography into ow x oh texels takes, by value.
struct WarpArgs {
  float h[9];
  int W, H, ow, oh, lanes;  // lanes = ceil(ow / 4)
  bool bgra, top_down;
};
inline WarpArgs warp_args(const float* h, int W, int H, int ow, int oh, int format) {
  const PresentFormat f = present_format(format);
  WarpArgs a;
  for (int k = 0; k < 9; k++) a.h[k] = h[k];
  a.W = W; a.H = H; a.ow = ow; a.oh = oh; a.lanes = (ow + 3) / 4;
  a.bgra = f.bgra; a.top_down = f.top_down;
  return a;
}

// The output side of a lane: four consecutive texels of one output row, x .. x + 3 of image row y, at o. Output row r
// is image row r, or oh - 1 - r (top_down); out is tight, ow words per row. in: the lane has texels at all; full: all
// four lie inside the row, else the lane is the last of a row whose width is no multiple of four and writes the ow & 3
// texels that are left, o[0] .. o[ow - 1 - x].
struct PresentLane {
  int x, y;
  uint32_t* o;
  bool in, full;
};
__device__ inline PresentLane present_lane(int ow, int oh, int lanes, bool top_down, uint32_t* out) {
  const int j = (int)(blockIdx.x * PRESENT_BX + threadIdx.x);
  const int r = (int)(blockIdx.y * PRESENT_BY + threadIdx.y);
  PresentLane l;
  l.in = j < lanes && r < oh;
  l.x = 4 * j;
  l.y = top_down ? oh - 1 - r : r;
  l.o = out + (size_t)r * ow + l.x;
  l.full = l.x + 4 <= ow;
  return l;
}

// A full lane's store. The compiler forms one 16-byte store from the four word stores; a row that does not start on a
// 16-byte boundary (ow no multiple of four) takes the same instruction, which needs word alignment only.
__device__ inline void present_store(uint32_t* o, uint4 q) {
  o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
}

}  // namespace fr
