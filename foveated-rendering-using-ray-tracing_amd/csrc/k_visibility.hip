// k_visibility.hip — per-model visibility (fr_set_model_visibility): the positions the tree writers read while a
// model is hidden.
//
// Visibility is applied where the tree is written, not where it is traversed. k_hide turns the true positions P into
// the collapsed positions C(P, visible) of include/fovrt.h: a triangle of a hidden model takes its first corner for
// all three (the bits are copied), every other triangle is copied. A refit or a build over C gives hidden triangles
// point boxes and a TriGeo with a zero normal, which fails the triangle test of every ray: the traversal kernels
// need no mask.
//
// One launch, a pure stream of 36 B in and 36 B out per triangle. A block owns a tile of 256 whole triangles, 2304
// floats or exactly 576 float4, so tiles start on 16-byte boundaries: 16-byte global loads and stores, coalesced,
// although a triangle is 36 bytes. The model boundaries and the hidden bits are kernel arguments (scalar operands,
// no load). A block whose triangles all lie in visible models (a block-uniform test on scalars, and the common case)
// stores what it loaded. The others pass the tile through LDS, where the lane that owns a hidden triangle overwrites
// corners 1 and 2 of its entry with corner 0's three words (entries are 9 words apart: odd, so the lanes of a wave
// fall on distinct banks). No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <string>

#include "fr_device.h"
#include "k_launch.h"

namespace fr {
namespace {

constexpr int kTile = FR_HIDE_TILE;   // triangles per block, one per lane
constexpr int kVec = kTile * 9 / 4;   // the tile as float4
constexpr int kPer = (kVec + kTile - 1) / kTile;  // float4 a lane moves
static_assert(kTile * 9 % 4 == 0, "a tile is a whole number of float4");

// float4 number `vec` of an array of nfl floats. The input holds exactly nfl floats: the last float4 is read word by
// word where it is partial (the words past the end are 0).
FR_DEV float4 load_vec(const float* __restrict__ pos, size_t vec, size_t nfl) {
  const size_t f = 4 * vec;
  if (f + 4 <= nfl) return *reinterpret_cast<const float4*>(pos + f);
  float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < 4; k++)
    if (f + k < nfl) w[k] = pos[f + k];
  return make_float4(w[0], w[1], w[2], w[3]);
}

// out holds 9 nt floats padded to whole float4 (pose_array_bytes; what it holds in the padding is never read).
__global__ __launch_bounds__(kTile) void k_hide(const float* __restrict__ pos, float4* __restrict__ out, int nt,
                                                const HideArgs a) {
  __shared__ float4 tile[kVec];
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * kTile, t1 = min(t0 + kTile, nt);
  const size_t nfl = 9 * (size_t)nt, nvec = (nfl + 3) / 4;
  const size_t v0 = (size_t)blockIdx.x * kVec;
  // does a hidden model reach into [t0, t1)? (scalars only)
  bool any = false;
#pragma unroll
  for (int i = 0; i < FR_POSE_MAX_MODELS; i++)
    any |= ((a.hidden >> i) & 1u) && a.first_tri[i] < t1 && a.first_tri[i + 1] > t0;
  float4 v[kPer];
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    const int lv = tid + k * kTile;
    if (lv < kVec && v0 + lv < nvec) v[k] = load_vec(pos, v0 + lv, nfl);
  }
  if (!any) {
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      const int lv = tid + k * kTile;
      if (lv < kVec && v0 + lv < nvec) out[v0 + lv] = v[k];
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    const int lv = tid + k * kTile;
    if (lv < kVec && v0 + lv < nvec) tile[lv] = v[k];
  }
  __syncthreads();
  const int tri = t0 + tid;
  int m = 0;
#pragma unroll
  for (int i = 1; i < FR_POSE_MAX_MODELS; i++) m += tri >= a.first_tri[i] ? 1 : 0;
  if (tri < t1 && ((a.hidden >> m) & 1u)) {
    float* e = reinterpret_cast<float*>(tile) + 9 * tid;
    const float x = e[0], y = e[1], z = e[2];
    e[3] = x; e[4] = y; e[5] = z;
    e[6] = x; e[7] = y; e[8] = z;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    const int lv = tid + k * kTile;
    if (lv < kVec && v0 + lv < nvec) out[v0 + lv] = tile[lv];
  }
}

}  // namespace

// The kernel arguments of a mask: first_tri holds the nmodels (<= FR_POSE_MAX_MODELS) first triangles; bit k of
// `visible` clear hides model k (bits at or above nmodels are ignored).
HideArgs hide_args(const int* first_tri, int nmodels, int nt, uint32_t visible) {
  HideArgs a;
  for (int i = 0; i <= FR_POSE_MAX_MODELS; i++) a.first_tri[i] = i < nmodels ? first_tri[i] : nt;
  const uint32_t valid = nmodels >= 32 ? 0xFFFFFFFFu : (1u << nmodels) - 1u;
  a.hidden = ~visible & valid;
  return a;
}

// pos (9 nt floats) -> out (pose_array_bytes(nt)), in stream order (nothing waits).
bool gpu_hide_enqueue(const HideArgs& a, const f3* pos, f3* out, int nt, hipStream_t s, std::string& err) {
  if (nt <= 0) return true;
  hipLaunchKernelGGL(k_hide, dim3((nt + kTile - 1) / kTile), dim3(kTile), 0, s, reinterpret_cast<const float*>(pos),
                     reinterpret_cast<float4*>(out), nt, a);
  if (hipGetLastError() != hipSuccess) {
    err = "visibility: launch failure";
    return false;
  }
  return true;
}

}  // namespace fr
