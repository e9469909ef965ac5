// k_normals.hip — shading normals that follow moving geometry (fr_update_geometry, fr_set_normals,
// fr_recompute_normals).
//
// The scene is a triangle soup: corner c = 3 t + k of triangle t. The smooth-vertex weld (scene.cpp,
// build_normal_groups) names the corners that are one vertex; it is fixed for the life of the scene and lives
// here as CSR (per vertex: its corners in ascending order). The recomputed normal of a vertex has one right
// answer in bytes, because the order of its sum is part of the rule:
//   acc = (0, 0, 0); for the corners c of the vertex, ascending: acc += cross(p1 - p0, p2 - p0) of triangle c / 3
//   d = dot(acc, acc); FLT_MIN <= d < inf: every corner of the vertex takes acc * (1 / sqrtf(d))
//   else each corner takes its own triangle's cross, normalised the same way when its dot is in that range,
//   else the corner keeps the normal it has.
// fp32, unfused (fr_math.h's cross and dot; the build passes -ffp-contract=off), no atomics. Three launches:
// one cross per triangle, one lane per vertex walking its run, one lane per triangle writing n0 / n1 / n2 .xyz
// of its TriShade (every .w and all of t stay: texture coordinates and flags live there). Corners of triangles
// without FR_SHADE_HAS_NORMALS have vertex -1 and are never written.
//
// Also here: the finiteness check of a caller's normals in device memory and their scatter into TriShade.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <string>
#include "fr_device.h"
#include "k_launch.h"

namespace fr {
namespace {

constexpr int kBlock = 256;

FR_DEV bool normalisable(float d) { return d >= FLT_MIN && d < INFINITY; }

// GATED (every kernel that writes): the form of an enqueued update (fr_update_geometry_enqueue). *reject
// (GeoUpdateState::reject, one uniform load per kernel) != 0: the update was rejected on the device and the kernel
// writes nothing. The plain instances never read the pointer.
template <bool GATED>
__global__ void k_face_cross(const f3* __restrict__ pos, int nt, f3* __restrict__ face,
                             const uint32_t* __restrict__ reject) {
  if (GATED && *reject) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  const f3 p0 = pos[3 * t], p1 = pos[3 * t + 1], p2 = pos[3 * t + 2];
  face[t] = cross(p1 - p0, p2 - p0);
}

// vnrm[v] = (normal, 1), or (0, 0, 0, 0): the corners of v fall back on their own triangles.
template <bool GATED>
__global__ void k_vertex_normals(const int32_t* __restrict__ off, const int32_t* __restrict__ corners, int nv,
                                 const f3* __restrict__ face, f4* __restrict__ vnrm,
                                 const uint32_t* __restrict__ reject) {
  if (GATED && *reject) return;
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  f3 acc = mk3(0.0f);
  for (int i = off[v], e = off[v + 1]; i < e; i++) acc = acc + face[corners[i] / 3];
  const float d = dot(acc, acc);
  vnrm[v] = normalisable(d) ? mk4(acc * (1.0f / sqrtf(d)), 1.0f) : mk4(0.0f, 0.0f, 0.0f, 0.0f);
}

FR_DEV void store_xyz(f4* dst, f3 n) {
  dst->x = n.x;
  dst->y = n.y;
  dst->z = n.z;
}

template <bool GATED>
__global__ void k_scatter_recomputed(const int32_t* __restrict__ corner_vertex, int nt, const f4* __restrict__ vnrm,
                                     const f3* __restrict__ face, TriShade* __restrict__ shade,
                                     const uint32_t* __restrict__ reject) {
  if (GATED && *reject) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  f4* const dst[3] = {&shade[t].n0, &shade[t].n1, &shade[t].n2};
  for (int k = 0; k < 3; k++) {
    const int v = corner_vertex[3 * t + k];
    if (v < 0) continue;
    const f4 n = vnrm[v];
    if (n.w != 0.0f) { store_xyz(dst[k], xyz(n)); continue; }
    const f3 f = face[t];
    const float d = dot(f, f);
    if (normalisable(d)) store_xyz(dst[k], f * (1.0f / sqrtf(d)));
  }
}

// A caller's normals (9 floats per triangle, device memory): *bad != 0 when a corner that has a vertex holds a
// float that is not finite.
__global__ void k_check_normals(const float* __restrict__ nrm, const int32_t* __restrict__ corner_vertex, size_t ncorners,
                                uint32_t* __restrict__ bad) {
  bool b = false;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncorners; c += (size_t)gridDim.x * blockDim.x)
    if (corner_vertex[c] >= 0) b |= !(isfinite(nrm[3 * c]) && isfinite(nrm[3 * c + 1]) && isfinite(nrm[3 * c + 2]));
  if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

template <bool GATED>
__global__ void k_scatter_given(const int32_t* __restrict__ corner_vertex, int nt, const float* __restrict__ nrm,
                                TriShade* __restrict__ shade, const uint32_t* __restrict__ reject) {
  if (GATED && *reject) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  f4* const dst[3] = {&shade[t].n0, &shade[t].n1, &shade[t].n2};
  for (int k = 0; k < 3; k++) {
    const size_t c = 3 * (size_t)t + k;
    if (corner_vertex[c] >= 0) store_xyz(dst[k], mk3(nrm[3 * c], nrm[3 * c + 1], nrm[3 * c + 2]));
  }
}

// The normals of an enqueued update out of place (fr_set_geometry_overlap): src's TriShade records into dst, which
// is two updates old, with the new normals on the way. One lane per 16-B word of a record (n0, n1, n2, t), so
// consecutive lanes load and store consecutive words; words 0..2 are corner k's (normal, texture coordinate), whose
// .xyz take k_scatter_given's or k_scatter_recomputed's value where those kernels write, and src's where they do not.
// NRM_COPY (FR_NORMALS_KEEP), and every rejected update (*reject != 0, one uniform load): the plain copy. Writing
// nothing is no option: dst would bring back the normals from before the previous update.
enum { NRM_COPY, NRM_GIVEN, NRM_RECOMPUTED };
template <int MODE>
__global__ void k_normals_to(const TriShade* __restrict__ src, TriShade* __restrict__ dst,
                             const int32_t* __restrict__ corner_vertex, int nt, const float* __restrict__ nrm,
                             const f4* __restrict__ vnrm, const f3* __restrict__ face,
                             const uint32_t* __restrict__ reject) {
  const bool copy = MODE == NRM_COPY || *reject != 0u;
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 4 * (size_t)nt) return;
  f4 w = reinterpret_cast<const f4*>(src)[q];
  const int k = (int)(q & 3);
  if (!copy && k < 3) {
    const size_t t = q >> 2, c = 3 * t + k;
    const int v = corner_vertex[c];
    if (v >= 0) {
      if (MODE == NRM_GIVEN) {
        store_xyz(&w, mk3(nrm[3 * c], nrm[3 * c + 1], nrm[3 * c + 2]));
      } else {
        const f4 n = vnrm[v];
        if (n.w != 0.0f) {
          store_xyz(&w, xyz(n));
        } else {
          const f3 f = face[t];
          const float d = dot(f, f);
          if (normalisable(d)) store_xyz(&w, f * (1.0f / sqrtf(d)));
        }
      }
    }
  }
  reinterpret_cast<f4*>(dst)[q] = w;
}

template <typename T>
hipError_t alloc(T** p, size_t n) {
  return hipMalloc((void**)p, (n > 0 ? n : 1) * sizeof(T));
}

int blocks(size_t n) { return (int)((n + kBlock - 1) / kBlock); }

}  // namespace

// The weld on the device and the scratch of a recompute, made once per context (no allocation in an update).
struct NormalsWork {
  int nt = 0, nv = 0;
  int32_t *corner_vertex = nullptr, *off = nullptr, *corners = nullptr;
  f3* face = nullptr;
  f4* vnrm = nullptr;
  uint32_t* bad = nullptr;
  uint32_t* host = nullptr;  // pinned: the check's flag
};

void normals_work_free(NormalsWork* w) {
  if (!w) return;
  for (void* p : {(void*)w->corner_vertex, (void*)w->off, (void*)w->corners, (void*)w->face, (void*)w->vnrm,
                  (void*)w->bad})
    if (p) hipFree(p);
  if (w->host) hipHostFree(w->host);
  delete w;
}

// corner_vertex: 3 nt ids (-1: no vertex); off: nv + 1 offsets into corners (off[nv] entries). One launch from
// this module on s (the check over no corners), so that its code object is loaded at context creation rather than
// in the first update (HIP loads a module at its first launch).
bool normals_work_create(NormalsWork** out, const int32_t* corner_vertex, const int32_t* off, const int32_t* corners,
                         int nt, int nv, hipStream_t s, std::string& err) {
  NormalsWork* w = new NormalsWork();
  w->nt = nt;
  w->nv = nv;
  const size_t nc = 3 * (size_t)nt, nrun = (size_t)off[nv];
  if (alloc(&w->corner_vertex, nc) || alloc(&w->off, (size_t)nv + 1) || alloc(&w->corners, nrun) ||
      alloc(&w->face, (size_t)nt) || alloc(&w->vnrm, (size_t)nv) || alloc(&w->bad, 1) ||
      hipHostMalloc((void**)&w->host, sizeof(uint32_t)) != hipSuccess) {
    err = "normals: device allocation failed";
    normals_work_free(w);
    return false;
  }
  if (hipMemcpy(w->corner_vertex, corner_vertex, nc * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(w->off, off, ((size_t)nv + 1) * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(w->corners, corners, nrun * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
    err = "normals: device copy failed";
    normals_work_free(w);
    return false;
  }
  hipLaunchKernelGGL(k_check_normals, dim3(1), dim3(64), 0, s, (const float*)nullptr, w->corner_vertex, (size_t)0, w->bad);
  if (hipGetLastError() != hipSuccess) {
    err = "normals: launch failed";
    normals_work_free(w);
    return false;
  }
  *out = w;
  return true;
}

static bool finish(hipStream_t s, const char* what, std::string& err) {
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) {
    err = std::string(what) + ": kernel failure";
    return false;
  }
  return true;
}

static bool launched(const char* what, std::string& err) {
  if (hipGetLastError() != hipSuccess) {
    err = std::string(what) + ": launch failure";
    return false;
  }
  return true;
}

// Each of the three calls below has an enqueue half, which launches and returns, and the call itself, which also
// waits. reject: NULL, or the device verdict word of an enqueued update (the gated kernels).

// The rule above over pos (3 vertices per triangle, device) into shade's normals.
bool gpu_recompute_normals_enqueue(NormalsWork* w, const f3* pos, TriShade* shade, const uint32_t* reject, hipStream_t s,
                                   std::string& err) {
  if (!w) { err = "normals: no workspace"; return false; }
  if (w->nv > 0) {
    auto fc = reject ? k_face_cross<true> : k_face_cross<false>;
    auto vn = reject ? k_vertex_normals<true> : k_vertex_normals<false>;
    auto sr = reject ? k_scatter_recomputed<true> : k_scatter_recomputed<false>;
    hipLaunchKernelGGL(fc, dim3(blocks(w->nt)), dim3(kBlock), 0, s, pos, w->nt, w->face, reject);
    hipLaunchKernelGGL(vn, dim3(blocks(w->nv)), dim3(kBlock), 0, s, w->off, w->corners, w->nv, w->face, w->vnrm, reject);
    hipLaunchKernelGGL(sr, dim3(blocks(w->nt)), dim3(kBlock), 0, s, w->corner_vertex, w->nt, w->vnrm, w->face, shade,
                       reject);
  }
  return launched("normals recompute", err);
}

bool gpu_recompute_normals(NormalsWork* w, const f3* pos, TriShade* shade, hipStream_t s, std::string& err) {
  return gpu_recompute_normals_enqueue(w, pos, shade, nullptr, s, err) && finish(s, "normals recompute", err);
}

// Every float of nrm (device, 9 per triangle) on a corner that has a vertex is finite: *flag (device; NULL: the
// workspace's own word, which gpu_check_normals reads back) stays 0.
bool gpu_check_normals_enqueue(NormalsWork* w, const float* nrm, uint32_t* flag, hipStream_t s, std::string& err) {
  if (!w) { err = "normals: no workspace"; return false; }
  if (!flag) flag = w->bad;
  const size_t nc = 3 * (size_t)w->nt;
  hipMemsetAsync(flag, 0, sizeof(uint32_t), s);
  hipLaunchKernelGGL(k_check_normals, dim3(blocks(nc) < 2048 ? blocks(nc) : 2048), dim3(kBlock), 0, s, nrm,
                     w->corner_vertex, nc, flag);
  return launched("normals check", err);
}

bool gpu_check_normals(NormalsWork* w, const float* nrm, bool* finite, hipStream_t s, std::string& err) {
  if (!gpu_check_normals_enqueue(w, nrm, nullptr, s, err)) return false;
  hipMemcpyAsync(w->host, w->bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  if (!finish(s, "normals check", err)) {
    err += " (is the pointer device memory of ntris x 9 floats?)";
    return false;
  }
  *finite = *w->host == 0;
  return true;
}

// nrm (device, 9 floats per triangle) into shade's normals, on the corners that have a vertex.
bool gpu_scatter_normals_enqueue(NormalsWork* w, const float* nrm, TriShade* shade, const uint32_t* reject, hipStream_t s,
                                 std::string& err) {
  if (!w) { err = "normals: no workspace"; return false; }
  if (w->nv > 0) {
    auto sg = reject ? k_scatter_given<true> : k_scatter_given<false>;
    hipLaunchKernelGGL(sg, dim3(blocks(w->nt)), dim3(kBlock), 0, s, w->corner_vertex, w->nt, nrm, shade, reject);
  }
  return launched("normals scatter", err);
}

// The normals of an enqueued update out of place (k_normals_to): src's records into dst with the caller's normals
// (nrm: device, 9 floats per triangle), the recomputed ones (pos: the positions now in place), or src's own (both
// NULL). reject: the device verdict word, never NULL. No wait.
bool gpu_normals_to_enqueue(NormalsWork* w, const float* nrm, const f3* pos, const TriShade* src, TriShade* dst,
                            const uint32_t* reject, hipStream_t s, std::string& err) {
  if (!w || !reject) { err = "normals: no workspace"; return false; }
  const int G = blocks(4 * (size_t)w->nt);
  const int32_t* cv = w->corner_vertex;
  if (w->nv == 0 || (!nrm && !pos)) {
    hipLaunchKernelGGL(k_normals_to<NRM_COPY>, dim3(G), dim3(kBlock), 0, s, src, dst, cv, w->nt, nrm, w->vnrm, w->face, reject);
  } else if (nrm) {
    hipLaunchKernelGGL(k_normals_to<NRM_GIVEN>, dim3(G), dim3(kBlock), 0, s, src, dst, cv, w->nt, nrm, w->vnrm, w->face, reject);
  } else {
    hipLaunchKernelGGL(k_face_cross<true>, dim3(blocks(w->nt)), dim3(kBlock), 0, s, pos, w->nt, w->face, reject);
    hipLaunchKernelGGL(k_vertex_normals<true>, dim3(blocks(w->nv)), dim3(kBlock), 0, s, w->off, w->corners, w->nv, w->face,
                       w->vnrm, reject);
    hipLaunchKernelGGL(k_normals_to<NRM_RECOMPUTED>, dim3(G), dim3(kBlock), 0, s, src, dst, cv, w->nt, nrm, w->vnrm, w->face,
                       reject);
  }
  return launched("normals (out of place)", err);
}

bool gpu_scatter_normals(NormalsWork* w, const float* nrm, TriShade* shade, hipStream_t s, std::string& err) {
  return gpu_scatter_normals_enqueue(w, nrm, shade, nullptr, s, err) && finish(s, "normals scatter", err);
}

}  // namespace fr
