// k_pose.hip — the scene's models posed by matrix on the device (fr_model_pose_enable, fr_set_model_transforms).
//
// The scene is a triangle soup assembled from rigid models, each a contiguous triangle range. A pose is one 3 x 4
// matrix per model over the rest geometry (the positions and normals captured by fr_model_pose_enable); k_pose
// writes the posed positions and normals into two staging arrays of the layout every geometry update reads (9
// floats per triangle), and the existing update path takes them from there. The rule has one right answer in
// bytes (include/fovrt.h): fp32, every operation rounded on its own, no fma:
//   p'.c = ((M[c][0] p.x + M[c][1] p.y) + M[c][2] p.z) + M[c][3]
//   n'.c = (K[c][0] n.x + K[c][1] n.y) + K[c][2] n.z                K = cofactors of A = det A^-T
// and a model at the identity takes its rest bits (the arithmetic would turn a -0 into +0). The products and
// sums are written with the _rn intrinsics, which the compiler does not contract; the cofactors come from the
// host (pose_args below, compiled with contraction off), so host and device cannot disagree about them.
//
// One launch, one thread per corner. The matrices, cofactors, identity flags and model boundaries are kernel
// arguments. A block moves its 256 corners (768 floats of each array) through LDS: 16-byte global loads and stores,
// coalesced, although a corner is 12 bytes; the lanes read and write their own three words of the tile (stride 3
// words: no bank conflict). A lane finds its model by comparing its triangle with the 15 boundaries (scalar
// operands) and loads its model's matrix from the kernel arguments by that index: one address per wave, except in
// the few waves that hold a model edge, where every lane still takes its own model's.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "fr_device.h"
#include "k_launch.h"

namespace fr {
namespace {

constexpr int kBlock = 256;           // corners per block
constexpr int kVec = kBlock * 3 / 4;  // the block's floats of one array, as float4

FR_DEV float row3(const float* r, f3 v) {
  return __fadd_rn(__fadd_rn(__fmul_rn(r[0], v.x), __fmul_rn(r[1], v.y)), __fmul_rn(r[2], v.z));
}

// One corner in place: p, n its three words of the position and the normal tile.
FR_DEV void pose_corner(const float* M, const float* K, float* p, float* n) {
  const f3 P = mk3(p[0], p[1], p[2]), N = mk3(n[0], n[1], n[2]);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    p[c] = __fadd_rn(row3(M + 4 * c, P), M[4 * c + 3]);
    n[c] = row3(K + 3 * c, N);
  }
}

// The arrays hold 3 ncorners floats, padded to whole float4 (the allocation covers the padding; what the
// staging arrays hold there is never read).
__global__ __launch_bounds__(kBlock) void k_pose(const float4* __restrict__ rest_pos, const float4* __restrict__ rest_nrm,
                                                 float4* __restrict__ out_pos, float4* __restrict__ out_nrm,
                                                 int ncorners, const PoseArgs a) {
  __shared__ float4 sp[kVec], sn[kVec];
  const int tid = threadIdx.x;
  const size_t nvec = (3 * (size_t)ncorners + 3) / 4;
  const size_t vec = (size_t)blockIdx.x * kVec + tid;
  const bool mover = tid < kVec && vec < nvec;
  float4 vp, vn;
  if (mover) {
    vp = rest_pos[vec];
    vn = rest_nrm[vec];
  }
  // The lane's model and its matrix, fetched while the tile is on its way. The boundaries are scalar operands; the
  // matrix is indexed per lane, which the compiler turns into loads from the kernel-argument segment (one address
  // per wave, except in a wave that holds a model edge).
  const int corner = blockIdx.x * kBlock + tid;
  int m = 0;
#pragma unroll
  for (int i = 1; i < FR_POSE_MAX_MODELS; i++) m += corner / 3 >= a.first_tri[i] ? 1 : 0;
  const bool posed = corner < ncorners && !((a.identity >> m) & 1u);
  float M[12], K[9];
  if (posed) {
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = a.M[m][k];
#pragma unroll
    for (int k = 0; k < 9; k++) K[k] = a.K[m][k];
  }
  if (mover) {
    sp[tid] = vp;
    sn[tid] = vn;
  }
  __syncthreads();
  if (posed) pose_corner(M, K, reinterpret_cast<float*>(sp) + 3 * tid, reinterpret_cast<float*>(sn) + 3 * tid);
  __syncthreads();
  if (mover) {
    out_pos[vec] = sp[tid];
    out_nrm[vec] = sn[tid];
  }
}

// The normals d_shade holds (n0 / n1 / n2 .xyz), as 9 floats per triangle.
__global__ void k_expand_normals(const TriShade* __restrict__ shade, int nt, f3* __restrict__ nrm) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  nrm[3 * t] = xyz(shade[t].n0);
  nrm[3 * t + 1] = xyz(shade[t].n1);
  nrm[3 * t + 2] = xyz(shade[t].n2);
}

bool launched(const char* what, std::string& err) {
  if (hipGetLastError() != hipSuccess) {
    err = std::string(what) + ": launch failure";
    return false;
  }
  return true;
}

}  // namespace

size_t pose_array_bytes(int nt) { return ((9 * (size_t)nt + 3) / 4) * sizeof(float4); }

// The kernel arguments of a pose: m holds nmodels (<= FR_POSE_MAX_MODELS) matrices of 12 floats, first_tri the
// nmodels first triangles. NULL when the pose is acceptable, else what is wrong with it: a float that is not
// finite, or a model whose determinant (the rule of include/fovrt.h, fp32) is not finite or not positive.
const char* pose_args(PoseArgs* a, const float* m, int nmodels, const int* first_tri) {
#pragma clang fp contract(off)
  static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  a->identity = 0;
  for (int i = 0; i < FR_POSE_MAX_MODELS; i++) a->first_tri[i] = i < nmodels ? first_tri[i] : INT_MAX;
  for (int i = 0; i < nmodels * 12; i++)
    if (!std::isfinite(m[i])) return "matrix entry not finite";
  for (int i = 0; i < FR_POSE_MAX_MODELS; i++) {
    const float* M = i < nmodels ? m + 12 * i : kIdentity;
    bool same = true;
    for (int k = 0; k < 12; k++) {
      a->M[i][k] = M[k];
      same &= M[k] == kIdentity[k];
    }
    if (same) a->identity |= 1u << i;
    auto A = [&](int r, int c) { return M[4 * r + c]; };
    float* K = a->K[i];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
        const float p = A(r1, c1) * A(r2, c2);
        const float q = A(r1, c2) * A(r2, c1);
        K[3 * r + c] = p - q;
      }
    const float d0 = A(0, 0) * K[0], d1 = A(0, 1) * K[1], d2 = A(0, 2) * K[2];
    const float s = d0 + d1;
    const float det = s + d2;
    if (!std::isfinite(det)) return "determinant not finite";
    if (!(det > 0.0f)) return "determinant not positive (a mirrored or flattened model)";
  }
  return nullptr;
}

// rest -> staged, in stream order (nothing waits).
bool gpu_pose_enqueue(const PoseArgs& a, const f3* rest_pos, const f3* rest_nrm, f3* out_pos, f3* out_nrm, int nt,
                      hipStream_t s, std::string& err) {
  const int ncorners = 3 * nt;
  if (ncorners <= 0) return true;
  hipLaunchKernelGGL(k_pose, dim3((ncorners + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                     reinterpret_cast<const float4*>(rest_pos), reinterpret_cast<const float4*>(rest_nrm),
                     reinterpret_cast<float4*>(out_pos), reinterpret_cast<float4*>(out_nrm), ncorners, a);
  return launched("pose", err);
}

// The rest geometry: pos and shade's normals as they are now, in stream order.
bool gpu_pose_capture_enqueue(const f3* pos, const TriShade* shade, f3* rest_pos, f3* rest_nrm, int nt, hipStream_t s,
                              std::string& err) {
  if (nt <= 0) return true;
  if (hipMemcpyAsync(rest_pos, pos, 9 * (size_t)nt * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    err = "pose: device copy failed";
    return false;
  }
  hipLaunchKernelGGL(k_expand_normals, dim3((nt + kBlock - 1) / kBlock), dim3(kBlock), 0, s, shade, nt, rest_nrm);
  return launched("pose capture", err);
}

}  // namespace fr
