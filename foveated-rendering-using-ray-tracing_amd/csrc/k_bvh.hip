// k_bvh.hip — the GPU BVH builder: a linear BVH (Morton order, Karras 2012
// hierarchy) built on the device and collapsed into the engine's four-wide nodes, so that a scene
// whose triangles move can be re-indexed every frame without a host round trip.
//
// The output has exactly the layout the host binned-SAH builder (scene.cpp) produces and the
// traversal (k_trace.hip) relies on:
//   - BvhNode: four SoA child slabs, inflated by the host's inflate_lo/hi, empty slots +-inf/-1;
//   - the inner children of a node are contiguous (one traversal stack entry per level);
//   - the leaf children of a node own one contiguous triangle range (the union-span leaf test);
//   - leaves hold at most two triangles; TriGeo is computed with the host's operations.
// Traversal results do not depend on the tree (closest hit ties -> lowest primitive index, shadow
// transmittance in f64), so a frame rendered over this BVH equals the host-built one.
//
// Steps: primitive boxes + centroid bounds -> 30-bit Morton codes -> radix sort (hipCUB) -> Karras
// binary hierarchy -> bottom-up boxes (one atomic per internal node) -> level-synchronous collapse
// into four-wide nodes (the host's rule: open the largest-area inner entry until four) -> per-node
// leaf triangle counts, exclusive scan, triangle relayout.
//
// Also here, for geometry that moves without regrouping: the refit of an existing four-wide tree of either
// builder (gpu_refit_bvh: same topology, new boxes and leaf triangles), the tree's SAH cost (gpu_bvh_cost) and
// the check of positions handed over in device memory (gpu_check_positions). Each has an enqueue half that
// launches and returns; an update enqueued in stream order (fr_update_geometry_enqueue) uses those alone, with
// the refit's gated kernels and the take-over of the positions by verdict (gpu_take_over_positions).
// The build has an enqueue form as well (fr_rebuild_bvh_enqueue: gpu_build_bvh_enqueue, gpu_collapse_marked_enqueue): a
// fixed launch schedule whose verdict and numbers stay in device memory (RebuildState), and the refit has forms
// that take the node count of such a tree from there. A conditional build (fr_rebuild_bvh_enqueue_if) puts the cost
// and a one-lane decision ahead of that schedule (gpu_rebuild_decide_enqueue) and the new tree's cost behind it
// (gpu_rebuild_rebase_enqueue); a build the device declines runs the schedule over an empty level 0.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "fr_device.h"
#include "k_launch.h"

namespace fr {
namespace {

constexpr int kLeafMax = 2;  // triangles per leaf (the host builder's default)

FR_DEV uint32_t expand_bits(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

// float <-> unsigned with the same order (for atomicMin / atomicMax on floats)
FR_DEV uint32_t ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FR_DEV float unord(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

FR_DEV float inflate_lo_d(float v) { return v - (1e-5f + 4e-7f * fabsf(v)); }  // scene.cpp inflate_lo
FR_DEV float inflate_hi_d(float v) { return v + (1e-5f + 4e-7f * fabsf(v)); }

FR_DEV float area_of(f4 lo, f4 hi) {
  const float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
  if (dx < 0) return 0.0f;
  return 2.0f * (dx * dy + dy * dz + dz * dx);
}

FR_DEV float wave_min(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
FR_DEV float wave_max(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Primitive boxes and the centroid bounds (cb[0..2] = min, cb[3..5] = max, order-mapped).
__global__ void k_prim_boxes(const f3* __restrict__ pos, int n, f4* __restrict__ blo, f4* __restrict__ bhi,
                             uint32_t* __restrict__ cb) {
  f3 cmin = mk3(INFINITY), cmax = mk3(-INFINITY);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const f3 a = pos[3 * i], b = pos[3 * i + 1], c = pos[3 * i + 2];
    const f3 lo = mk3(fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z));
    const f3 hi = mk3(fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z));
    blo[i] = mk4(lo, 0.0f);
    bhi[i] = mk4(hi, 0.0f);
    const f3 ce = (lo + hi) * 0.5f;
    cmin = mk3(fminf(cmin.x, ce.x), fminf(cmin.y, ce.y), fminf(cmin.z, ce.z));
    cmax = mk3(fmaxf(cmax.x, ce.x), fmaxf(cmax.y, ce.y), fmaxf(cmax.z, ce.z));
  }
  const float r[6] = {wave_min(cmin.x), wave_min(cmin.y), wave_min(cmin.z),
                      wave_max(cmax.x), wave_max(cmax.y), wave_max(cmax.z)};
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 3; k++) atomicMin(&cb[k], ord(r[k]));
    for (int k = 3; k < 6; k++) atomicMax(&cb[k], ord(r[k]));
  }
}

__global__ void k_morton(const f4* __restrict__ blo, const f4* __restrict__ bhi, int n, const uint32_t* __restrict__ cb,
                         uint32_t* __restrict__ codes, int32_t* __restrict__ ids) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f3 cmin = mk3(unord(cb[0]), unord(cb[1]), unord(cb[2]));
  const f3 cmax = mk3(unord(cb[3]), unord(cb[4]), unord(cb[5]));
  const f4 lo = blo[i], hi = bhi[i];
  const f3 ce = (xyz(lo) + xyz(hi)) * 0.5f;
  auto q = [](float c, float a, float b) {
    const float e = b - a;
    const float t = e > 0.0f ? (c - a) / e : 0.5f;
    return (uint32_t)fminf(fmaxf(t * 1024.0f, 0.0f), 1023.0f);
  };
  codes[i] = (expand_bits(q(ce.x, cmin.x, cmax.x)) << 2) | (expand_bits(q(ce.y, cmin.y, cmax.y)) << 1) |
             expand_bits(q(ce.z, cmin.z, cmax.z));
  ids[i] = i;
}

// Karras' delta with the index as the tie-breaker of equal codes.
FR_DEV int kdelta(const uint32_t* __restrict__ codes, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint32_t a = codes[i], b = codes[j];
  if (a == b) return 32 + __clz((uint32_t)(i ^ j));
  return __clz(a ^ b);
}

// Internal node i of the binary tree (ids: internal [0, n-1), leaf k -> n-1+k).
__global__ void k_karras(const uint32_t* __restrict__ codes, int n, int2* __restrict__ child, int* __restrict__ parent,
                         int2* __restrict__ range) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const int d = kdelta(codes, n, i, i + 1) - kdelta(codes, n, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = kdelta(codes, n, i, i - d);
  int lmax = 2;
  while (kdelta(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
  int l = 0;
  for (int t = lmax / 2; t >= 1; t /= 2)
    if (kdelta(codes, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = kdelta(codes, n, i, j);
  int s = 0, t = l;
  do {
    t = (t + 1) >> 1;
    if (kdelta(codes, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int gamma = i + s * d + min(d, 0);
  const int first = min(i, j), last = max(i, j);
  const int left = first == gamma ? n - 1 + gamma : gamma;
  const int right = last == gamma + 1 ? n - 1 + gamma + 1 : gamma + 1;
  child[i] = int2{left, right};
  parent[left] = i;
  parent[right] = i;
  range[i] = int2{first, last};
  if (i == 0) parent[0] = -1;
}

FR_DEV f4 load_agent(const f4* p) {
  const float* q = reinterpret_cast<const float*>(p);
  return mk4(__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
             __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
             __hip_atomic_load(q + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0.0f);
}

// Bottom-up boxes: a leaf walks to the root; the first arrival at a node stops, the second (which
// then sees both children) writes the union and continues.
__global__ void k_boxes_up(int n, const int32_t* __restrict__ ids, const f4* __restrict__ blo, const f4* __restrict__ bhi,
                           const int* __restrict__ parent, const int2* __restrict__ child, f4* nlo, f4* nhi,
                           uint32_t* __restrict__ arrivals) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  int node = parent[n - 1 + k];
  while (node >= 0) {
    if (__hip_atomic_fetch_add(&arrivals[node], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const int2 c = child[node];
    f4 lo = mk4(INFINITY, INFINITY, INFINITY, 0.0f), hi = mk4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    for (int side = 0; side < 2; side++) {
      const int e = side ? c.y : c.x;
      f4 a, b;
      if (e >= n - 1) { a = blo[ids[e - (n - 1)]]; b = bhi[ids[e - (n - 1)]]; }
      else { a = load_agent(nlo + e); b = load_agent(nhi + e); }
      lo = mk4(fminf(lo.x, a.x), fminf(lo.y, a.y), fminf(lo.z, a.z), 0.0f);
      hi = mk4(fmaxf(hi.x, b.x), fmaxf(hi.y, b.y), fmaxf(hi.z, b.z), 0.0f);
    }
    float* pl = reinterpret_cast<float*>(nlo + node);
    float* ph = reinterpret_cast<float*>(nhi + node);
    for (int q = 0; q < 3; q++) {
      __hip_atomic_store(pl + q, (&lo.x)[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ph + q, (&hi.x)[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    node = parent[node];
  }
}

struct CollapseItem {
  int bin;   // binary node id
  int slot;  // its four-wide node
  int need;  // traversal stack entries on the path to it
};

struct BinTree {
  int n;
  const int2* child;
  const int2* range;
  const f4 *nlo, *nhi, *blo, *bhi;
  const int32_t* ids;
  FR_DEV bool is_leaf(int e) const { return e >= n - 1 || range[e].y - range[e].x + 1 <= kLeafMax; }
  FR_DEV int first(int e) const { return e >= n - 1 ? e - (n - 1) : range[e].x; }
  FR_DEV int size(int e) const { return e >= n - 1 ? 1 : range[e].y - range[e].x + 1; }
  FR_DEV f4 lo(int e) const { return e >= n - 1 ? blo[ids[e - (n - 1)]] : nlo[e]; }
  FR_DEV f4 hi(int e) const { return e >= n - 1 ? bhi[ids[e - (n - 1)]] : nhi[e]; }
};

// The same questions of a MarkedTree (k_launch.h; the device SAH builder's): a leaf is marked, not recognised by
// its size, and holds any number of triangles.
struct MarkedBinTree {
  const int2* child;
  const int2* range;
  const f4 *nlo, *nhi;
  FR_DEV bool is_leaf(int e) const { return child[e].x < 0; }
  FR_DEV int first(int e) const { return range[e].x; }
  FR_DEV int size(int e) const { return range[e].y - range[e].x; }
  FR_DEV f4 lo(int e) const { return nlo[e]; }
  FR_DEV f4 hi(int e) const { return nhi[e]; }
};

// One level of the collapse: every item becomes a four-wide node; its inner children are allocated
// contiguously and become the next level's items. Leaf entries keep their sorted-order range for
// now (k_emit_leaves relays them out). Tree: BinTree (the LBVH) or MarkedBinTree.
// GATED: the form of an enqueued build, whose binary tree may have failed on the device (*stop != 0: its root may
// then be a leaf, which the collapse does not handle) and writes nothing then. The plain instances never read it.
template <class Tree, bool GATED = false>
__global__ void k_collapse(Tree T, const CollapseItem* __restrict__ cur, const uint32_t* __restrict__ ncur,
                           CollapseItem* __restrict__ next, uint32_t* __restrict__ nnext, uint32_t* __restrict__ node_ctr,
                           BvhNode* __restrict__ nodes, uint32_t* __restrict__ max_stack, uint32_t* __restrict__ levels,
                           const uint32_t* __restrict__ stop) {
  if (GATED && *stop) return;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nc = *ncur;
  if (i == 0 && nc) atomicAdd(levels, 1u);
  if (i >= nc) return;
  const CollapseItem it = cur[i];
  int e[4];
  int ne = 2;
  e[0] = T.child[it.bin].x;
  e[1] = T.child[it.bin].y;
  while (ne < 4) {  // open the inner entry of largest area (scene.cpp collapse)
    int best = -1;
    float ba = -1.0f;
    for (int k = 0; k < ne; k++)
      if (!T.is_leaf(e[k])) {
        const float a = area_of(T.lo(e[k]), T.hi(e[k]));
        if (a > ba) { ba = a; best = k; }
      }
    if (best < 0) break;
    const int2 c = T.child[e[best]];
    for (int k = best; k + 1 < ne; k++) e[k] = e[k + 1];
    e[ne - 1] = c.x;
    e[ne] = c.y;
    ne++;
  }
  int inner = 0;
  for (int k = 0; k < ne; k++) inner += !T.is_leaf(e[k]);
  const int need = it.need + (inner > 1 ? 1 : 0);
  atomicMax(max_stack, (uint32_t)need);
  const int base = inner ? (int)atomicAdd(node_ctr, (uint32_t)inner) : 0;
  BvhNode nd;
  float* LX = &nd.lox.x; float* HX = &nd.hix.x;
  float* LY = &nd.loy.x; float* HY = &nd.hiy.x;
  float* LZ = &nd.loz.x; float* HZ = &nd.hiz.x;
  int r = 0;
  for (int k = 0; k < 4; k++) {
    if (k >= ne) {
      LX[k] = LY[k] = LZ[k] = INFINITY;
      HX[k] = HY[k] = HZ[k] = -INFINITY;
      nd.child[k] = 0;
      nd.count[k] = -1;
      continue;
    }
    const f4 lo = T.lo(e[k]), hi = T.hi(e[k]);
    LX[k] = inflate_lo_d(lo.x); HX[k] = inflate_hi_d(hi.x);
    LY[k] = inflate_lo_d(lo.y); HY[k] = inflate_hi_d(hi.y);
    LZ[k] = inflate_lo_d(lo.z); HZ[k] = inflate_hi_d(hi.z);
    if (T.is_leaf(e[k])) {
      nd.child[k] = T.first(e[k]);
      nd.count[k] = T.size(e[k]);
    } else {
      nd.child[k] = base + r;
      nd.count[k] = 0;
      next[atomicAdd(nnext, 1u)] = CollapseItem{e[k], base + r, need};
      r++;
    }
  }
  nodes[it.slot] = nd;
}

// DEVN (here and below): the form of an enqueued build or update, whose node count is in device memory (*nn_dev,
// one uniform load); the grid then covers the capacity `nn` (one node per triangle). The plain instances never
// read the pointer. k_leaf_counts<true> writes every entry of the capacity (0 past the tree: the scan runs over all).
template <bool DEVN>
__global__ void k_leaf_counts(const BvhNode* __restrict__ nodes, int nn, uint32_t* __restrict__ cnt,
                              const uint32_t* __restrict__ nn_dev) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  if (DEVN && i >= (int)*nn_dev) { cnt[i] = 0u; return; }
  uint32_t s = 0;
  for (int k = 0; k < 4; k++) s += nodes[i].count[k] > 0 ? (uint32_t)nodes[i].count[k] : 0u;
  cnt[i] = s;
}

// TriGeo of primitive p with the host's operations (scene.cpp: e0 = p1 - p0, e1 = p0 - p2, n = cross(e1, e0),
// unfused); the builder's leaves and the refit share it.
FR_DEV void store_tri_geo(const f3* __restrict__ pos, int p, TriGeo* __restrict__ out) {
  const f3 p0 = pos[3 * p], p1 = pos[3 * p + 1], p2 = pos[3 * p + 2];
  const f3 e0 = p1 - p0, e1 = p0 - p2, nn3 = cross(e1, e0);
  out->a = mk4(p0.x, p0.y, p0.z, e0.x);
  out->b = mk4(e0.y, e0.z, e1.x, e1.y);
  out->c = mk4(e1.z, nn3.x, nn3.y, nn3.z);
}

// Leaf children of node i -> one contiguous range starting at off[i].
template <bool DEVN>
__global__ void k_emit_leaves(BvhNode* __restrict__ nodes, int nn, const uint32_t* __restrict__ off,
                              const int32_t* __restrict__ ids, const f3* __restrict__ pos, TriGeo* __restrict__ tri,
                              int32_t* __restrict__ prim, const uint32_t* __restrict__ nn_dev) {
  if (DEVN) nn = min(nn, (int)*nn_dev);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  uint32_t o = off[i];
  for (int k = 0; k < 4; k++) {
    const int cnt = nodes[i].count[k];
    if (cnt <= 0) continue;
    const int first = nodes[i].child[k];
    nodes[i].child[k] = (int)o;
    for (int j = 0; j < cnt; j++, o++) {
      const int p = ids[first + j];
      prim[o] = p;
      store_tri_geo(pos, p, &tri[o]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Refit: new boxes and leaf triangles for an existing four-wide tree (either builder's); child, count,
// prim and the node order stay.
// ---------------------------------------------------------------------------------------------
// GATED (all three kernels): the form of an enqueued update (fr_update_geometry_enqueue), whose verdict is in
// device memory. *reject (GeoUpdateState::reject, one uniform load per kernel) != 0: the update was rejected on the
// device and the kernel writes nothing. The plain instances never read the pointer.
template <bool GATED>
__global__ void k_refit_tris(const f3* __restrict__ pos, const int32_t* __restrict__ prim, int n, TriGeo* __restrict__ tri,
                             const uint32_t* __restrict__ reject) {
  if (GATED && *reject) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) store_tri_geo(pos, prim[j], &tri[j]);
}

// Parent links (node, not slot) from the nodes themselves, and the arrival counters back to zero.
template <bool GATED, bool DEVN = false>
__global__ void k_refit_links(const BvhNode* __restrict__ nodes, int nn, int* __restrict__ parent,
                              uint32_t* __restrict__ arrivals, const uint32_t* __restrict__ reject,
                              const uint32_t* __restrict__ nn_dev) {
  if (GATED && *reject) return;
  if (DEVN) nn = min(nn, (int)*nn_dev);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  arrivals[i] = 0u;
  if (i == 0) parent[0] = -1;
  for (int k = 0; k < 4; k++)
    if (nodes[i].count[k] == 0) parent[nodes[i].child[k]] = i;
}

FR_DEV void store_agent(f4* p, f3 v) {
  float* q = reinterpret_cast<float*>(p);
  __hip_atomic_store(q, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q + 2, v.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Bottom-up boxes over the four-wide tree, k_boxes_up's scheme: a node without inner slots starts a walk; a
// thread that finishes a node arrives at its parent, and the last of the parent's inner children to arrive
// (which then sees every child's raw box) goes on with the parent. nlo / nhi hold the raw (uninflated) box of
// each node; a slot stores inflate(raw). Nobody waits: a walk that is not the last arrival ends.
template <bool GATED, bool DEVN = false>
__global__ void k_refit_up(BvhNode* nodes, int nn, const f3* __restrict__ pos, const int32_t* __restrict__ prim,
                           const int* __restrict__ parent, uint32_t* __restrict__ arrivals, f4* nlo, f4* nhi,
                           const uint32_t* __restrict__ reject, const uint32_t* __restrict__ nn_dev) {
  if (GATED && *reject) return;
  if (DEVN) nn = min(nn, (int)*nn_dev);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  int node = i;
  {
    const int* cnt = nodes[i].count;
    if (cnt[0] == 0 || cnt[1] == 0 || cnt[2] == 0 || cnt[3] == 0) return;
  }
  for (;;) {
    BvhNode* nd = nodes + node;
    float* LX = &nd->lox.x; float* HX = &nd->hix.x;
    float* LY = &nd->loy.x; float* HY = &nd->hiy.x;
    float* LZ = &nd->loz.x; float* HZ = &nd->hiz.x;
    f3 nlo3 = mk3(INFINITY), nhi3 = mk3(-INFINITY);
    for (int k = 0; k < 4; k++) {
      const int cnt = nd->count[k], ch = nd->child[k];
      if (cnt < 0) continue;  // an empty slot stays +inf / -inf / child 0
      f3 lo = mk3(INFINITY), hi = mk3(-INFINITY);
      if (cnt == 0) {
        lo = xyz(load_agent(nlo + ch));
        hi = xyz(load_agent(nhi + ch));
      } else {
        for (int j = 0; j < cnt; j++) {
          const int p = prim[ch + j];
          for (int v = 0; v < 3; v++) {
            const f3 q = pos[3 * p + v];
            lo = mk3(fminf(lo.x, q.x), fminf(lo.y, q.y), fminf(lo.z, q.z));
            hi = mk3(fmaxf(hi.x, q.x), fmaxf(hi.y, q.y), fmaxf(hi.z, q.z));
          }
        }
      }
      LX[k] = inflate_lo_d(lo.x); HX[k] = inflate_hi_d(hi.x);
      LY[k] = inflate_lo_d(lo.y); HY[k] = inflate_hi_d(hi.y);
      LZ[k] = inflate_lo_d(lo.z); HZ[k] = inflate_hi_d(hi.z);
      nlo3 = mk3(fminf(nlo3.x, lo.x), fminf(nlo3.y, lo.y), fminf(nlo3.z, lo.z));
      nhi3 = mk3(fmaxf(nhi3.x, hi.x), fmaxf(nhi3.y, hi.y), fmaxf(nhi3.z, hi.z));
    }
    const int up = parent[node];
    if (up < 0) return;
    store_agent(nlo + node, nlo3);
    store_agent(nhi + node, nhi3);
    const int* pc = nodes[up].count;
    const uint32_t inner = (uint32_t)(pc[0] == 0) + (uint32_t)(pc[1] == 0) + (uint32_t)(pc[2] == 0) + (uint32_t)(pc[3] == 0);
    if (__hip_atomic_fetch_add(&arrivals[up], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u != inner) return;
    node = up;
  }
}

// ---------------------------------------------------------------------------------------------
// Refit out of place (fr_set_geometry_overlap): the same three kernels reading one tree (src) and writing another
// (dst), which no frame in flight reads. dst is two updates old, or a replaced tree of another topology, so nothing
// of it is kept: every node is written whole (the new boxes around src's child / count; an empty slot's boxes are
// src's), tri[j] is rebuilt and prim copied. The accepted result is the in-place refit's, byte for byte. A rejected
// update (*reject != 0, one uniform load per kernel) cannot write nothing here: the same launches then copy src's
// nodes and triangles verbatim. 16-B loads and stores throughout (a node is eight of them, a TriGeo three).
// ---------------------------------------------------------------------------------------------
__global__ void k_refit_tris_to(const f3* __restrict__ pos, const int32_t* __restrict__ prim,
                                const TriGeo* __restrict__ src, int n, TriGeo* __restrict__ dst,
                                int32_t* __restrict__ prim_dst, const uint32_t* __restrict__ reject) {
  const uint32_t rej = *reject;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int p = prim[j];
  prim_dst[j] = p;
  if (rej) {
    const TriGeo g = src[j];
    dst[j].a = g.a; dst[j].b = g.b; dst[j].c = g.c;
  } else {
    store_tri_geo(pos, p, &dst[j]);
  }
}

// k_refit_links over src. Rejected: the copy of the nodes instead, one 16-B word per lane, consecutive lanes
// consecutive words (the grid's nn lanes take eight words each).
template <bool DEVN>
__global__ void k_refit_links_to(const BvhNode* __restrict__ src, int nn, int* __restrict__ parent,
                                 uint32_t* __restrict__ arrivals, BvhNode* __restrict__ dst,
                                 const uint32_t* __restrict__ reject, const uint32_t* __restrict__ nn_dev) {
  if (DEVN) nn = min(nn, (int)*nn_dev);
  if (*reject) {
    const f4* s4 = reinterpret_cast<const f4*>(src);
    f4* d4 = reinterpret_cast<f4*>(dst);
    const size_t n4 = (size_t)nn * 8, first = (size_t)blockIdx.x * blockDim.x * 8 + threadIdx.x;
    for (int k = 0; k < 8; k++) {
      const size_t q = first + (size_t)k * blockDim.x;
      if (q < n4) d4[q] = s4[q];
    }
    return;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  arrivals[i] = 0u;
  if (i == 0) parent[0] = -1;
  for (int k = 0; k < 4; k++)
    if (src[i].count[k] == 0) parent[src[i].child[k]] = i;
}

// k_refit_up's walk over src's topology; the thread that finishes a node stores it whole into dst.
template <bool DEVN>
__global__ void k_refit_up_to(const BvhNode* __restrict__ src, BvhNode* __restrict__ dst, int nn,
                              const f3* __restrict__ pos, const int32_t* __restrict__ prim,
                              const int* __restrict__ parent, uint32_t* __restrict__ arrivals, f4* nlo, f4* nhi,
                              const uint32_t* __restrict__ reject, const uint32_t* __restrict__ nn_dev) {
  if (*reject) return;
  if (DEVN) nn = min(nn, (int)*nn_dev);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  int node = i;
  {
    const int* cnt = src[i].count;
    if (cnt[0] == 0 || cnt[1] == 0 || cnt[2] == 0 || cnt[3] == 0) return;
  }
  for (;;) {
    BvhNode nd = src[node];
    float* LX = &nd.lox.x; float* HX = &nd.hix.x;
    float* LY = &nd.loy.x; float* HY = &nd.hiy.x;
    float* LZ = &nd.loz.x; float* HZ = &nd.hiz.x;
    f3 nlo3 = mk3(INFINITY), nhi3 = mk3(-INFINITY);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int cnt = nd.count[k], ch = nd.child[k];
      if (cnt < 0) continue;  // an empty slot keeps src's +inf / -inf / child 0
      f3 lo = mk3(INFINITY), hi = mk3(-INFINITY);
      if (cnt == 0) {
        lo = xyz(load_agent(nlo + ch));
        hi = xyz(load_agent(nhi + ch));
      } else {
        for (int j = 0; j < cnt; j++) {
          const int p = prim[ch + j];
          for (int v = 0; v < 3; v++) {
            const f3 q = pos[3 * p + v];
            lo = mk3(fminf(lo.x, q.x), fminf(lo.y, q.y), fminf(lo.z, q.z));
            hi = mk3(fmaxf(hi.x, q.x), fmaxf(hi.y, q.y), fmaxf(hi.z, q.z));
          }
        }
      }
      LX[k] = inflate_lo_d(lo.x); HX[k] = inflate_hi_d(hi.x);
      LY[k] = inflate_lo_d(lo.y); HY[k] = inflate_hi_d(hi.y);
      LZ[k] = inflate_lo_d(lo.z); HZ[k] = inflate_hi_d(hi.z);
      nlo3 = mk3(fminf(nlo3.x, lo.x), fminf(nlo3.y, lo.y), fminf(nlo3.z, lo.z));
      nhi3 = mk3(fmaxf(nhi3.x, hi.x), fmaxf(nhi3.y, hi.y), fmaxf(nhi3.z, hi.z));
    }
    dst[node] = nd;
    const int up = parent[node];
    if (up < 0) return;
    store_agent(nlo + node, nlo3);
    store_agent(nhi + node, nhi3);
    const int* pc = src[up].count;
    const uint32_t inner = (uint32_t)(pc[0] == 0) + (uint32_t)(pc[1] == 0) + (uint32_t)(pc[2] == 0) + (uint32_t)(pc[3] == 0);
    if (__hip_atomic_fetch_add(&arrivals[up], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u != inner) return;
    node = up;
  }
}

// SAH cost terms: part[i] = sum over node i's non-empty slots of area(stored box) * (1 for an inner slot, count
// for a leaf slot); *root_area = the area of the union of node 0's slot boxes. DEVN: every entry of the capacity is
// written (0 past the tree, and a root area of 0 for a tree without a node: the sum runs over all). GATE (the cost
// of a tree a conditional build has just made): NULL, or the build's verdict word; nothing is read of a destination
// that a failed or skipped build left (the terms are 0 then, and k_rebuild_rebase does not look at the sum).
template <bool DEVN>
__global__ void k_cost_terms(const BvhNode* __restrict__ nodes, int nn, float* __restrict__ part,
                             float* __restrict__ root_area, const uint32_t* __restrict__ nn_dev,
                             const uint32_t* __restrict__ gate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  if (DEVN && (i >= (int)*nn_dev || (gate && *gate))) {
    part[i] = 0.0f;
    if (i == 0) *root_area = 0.0f;
    return;
  }
  const BvhNode nd = nodes[i];
  const float* LX = &nd.lox.x; const float* HX = &nd.hix.x;
  const float* LY = &nd.loy.x; const float* HY = &nd.hiy.x;
  const float* LZ = &nd.loz.x; const float* HZ = &nd.hiz.x;
  float s = 0.0f;
  f4 ulo = mk4(INFINITY, INFINITY, INFINITY, 0.0f), uhi = mk4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
  for (int k = 0; k < 4; k++) {
    if (nd.count[k] < 0) continue;
    const f4 lo = mk4(LX[k], LY[k], LZ[k], 0.0f), hi = mk4(HX[k], HY[k], HZ[k], 0.0f);
    s += area_of(lo, hi) * (nd.count[k] > 0 ? (float)nd.count[k] : 1.0f);
    ulo = mk4(fminf(ulo.x, lo.x), fminf(ulo.y, lo.y), fminf(ulo.z, lo.z), 0.0f);
    uhi = mk4(fmaxf(uhi.x, hi.x), fmaxf(uhi.y, hi.y), fmaxf(uhi.z, hi.z), 0.0f);
  }
  part[i] = s;
  if (i == 0) *root_area = area_of(ulo, uhi);
}

// A caller's device positions before they are taken over: cb[0..5] = the box of all vertices (order-mapped, as
// in k_prim_boxes), cb[6] != 0 when a coordinate is not finite.
__global__ void k_check_positions(const float* __restrict__ xyz, size_t nverts, uint32_t* __restrict__ cb) {
  f3 lo = mk3(INFINITY), hi = mk3(-INFINITY);
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nverts; i += (size_t)gridDim.x * blockDim.x) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    bad |= !(isfinite(x) && isfinite(y) && isfinite(z));
    lo = mk3(fminf(lo.x, x), fminf(lo.y, y), fminf(lo.z, z));
    hi = mk3(fmaxf(hi.x, x), fmaxf(hi.y, y), fmaxf(hi.z, z));
  }
  const float r[6] = {wave_min(lo.x), wave_min(lo.y), wave_min(lo.z), wave_max(hi.x), wave_max(hi.y), wave_max(hi.z)};
  const bool any_bad = __any(bad);
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 3; k++) atomicMin(&cb[k], ord(r[k]));
    for (int k = 3; k < 6; k++) atomicMax(&cb[k], ord(r[k]));
    if (any_bad) atomicOr(&cb[6], 1u);
  }
}

// The take-over of an enqueued update (fr_update_geometry_enqueue), after both checks: one lane per vertex (12 B,
// consecutive lanes consecutive vertices). dst (the context's spare array, which the host makes the current one
// whatever the verdict) gets the caller's positions when the update is accepted and the current ones otherwise.
// The verdict is cb[6] (k_check_positions) and *bad_nrm (k_check_normals; NULL: no normals were given), two
// uniform loads. Lane 0 of block 0 publishes it for the gated kernels that follow (st->reject), counts it, and on
// an accepted update writes the scene box from the check's result (k_check_positions' order-mapped min / max, so
// the bytes a synchronous update reads back). flags bit 0: first enqueue of the context, the device box is seeded
// with the host's (seed_lo / seed_hi) first; bit 1: an owed EXTRA heat map reads the box in place, which is kept
// for it in st->xbox before the new one lands.
__global__ void k_take_over(const f3* __restrict__ xyz, const f3* __restrict__ cur, size_t nverts, f3* __restrict__ dst,
                            const uint32_t* __restrict__ cb, const uint32_t* __restrict__ bad_nrm,
                            GeoUpdateState* __restrict__ st, int flags, f3 seed_lo, f3 seed_hi) {
  const uint32_t rej = (cb[6] ? 1u : 0u) | (bad_nrm && *bad_nrm ? 2u : 0u);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nverts) dst[i] = rej ? cur[i] : xyz[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (flags & 1) {
      st->box[0] = seed_lo.x; st->box[1] = seed_lo.y; st->box[2] = seed_lo.z;
      st->box[3] = seed_hi.x; st->box[4] = seed_hi.y; st->box[5] = seed_hi.z;
    }
    if (flags & 2)
      for (int k = 0; k < 6; k++) st->xbox[k] = st->box[k];
    st->reject = rej;
    if (rej) {
      st->rejected++;
      if (rej & 1u) st->rejected_pos++;
      if (rej & 2u) st->rejected_nrm++;
    } else {
      st->applied++;
      for (int k = 0; k < 6; k++) st->box[k] = unord(cb[k]);
    }
  }
}

template <typename T>
hipError_t alloc(T** p, size_t n) {
  return hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T));
}

}  // namespace

// Scratch of the builder, kept by the context between rebuilds (no allocation, no hipFree, which would
// synchronise the whole device, in a rebuild once it exists).
struct BvhWork {
  int cap = 0;
  f4 *blo = nullptr, *bhi = nullptr, *nlo = nullptr, *nhi = nullptr;
  uint32_t *cb = nullptr, *codes = nullptr, *codes_s = nullptr, *arrivals = nullptr, *ctr = nullptr, *cnt = nullptr,
           *off = nullptr;
  int32_t *ids = nullptr, *ids_s = nullptr;
  int2 *child = nullptr, *range = nullptr;
  int* parent = nullptr;
  CollapseItem *qa = nullptr, *qb = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  uint32_t* host = nullptr;  // pinned, 8 words: the builder's counters; the position check's box and flag; the cost's sums
};

void bvh_work_free(BvhWork* w) {
  if (!w) return;
  for (void* p : {(void*)w->blo, (void*)w->bhi, (void*)w->nlo, (void*)w->nhi, (void*)w->cb, (void*)w->codes,
                  (void*)w->codes_s, (void*)w->ids, (void*)w->ids_s, (void*)w->child, (void*)w->range, (void*)w->parent,
                  (void*)w->arrivals, (void*)w->ctr, (void*)w->qa, (void*)w->qb, (void*)w->cnt, (void*)w->off, w->tmp})
    if (p) hipFree(p);
  if (w->host) hipHostFree(w->host);
  delete w;
}

static bool bvh_work_reserve(BvhWork*& w, int n, hipStream_t s, std::string& err) {
  if (w && w->cap >= n) return true;
  bvh_work_free(w);
  w = new BvhWork();
  if (alloc(&w->blo, n) || alloc(&w->bhi, n) || alloc(&w->nlo, n) || alloc(&w->nhi, n) || alloc(&w->cb, 8) ||
      alloc(&w->codes, n) || alloc(&w->codes_s, n) || alloc(&w->ids, n) || alloc(&w->ids_s, n) || alloc(&w->child, n) ||
      alloc(&w->range, n) || alloc(&w->parent, 2 * n) || alloc(&w->arrivals, n) || alloc(&w->ctr, 8) ||
      alloc(&w->qa, n) || alloc(&w->qb, n) || alloc(&w->cnt, n) || alloc(&w->off, n) ||
      hipHostMalloc((void**)&w->host, 8 * sizeof(uint32_t)) != hipSuccess) {
    err = "GPU BVH builder: device allocation failed";
    bvh_work_free(w);
    w = nullptr;
    return false;
  }
  size_t sort_bytes = 0, scan_bytes = 0, sum_bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, w->codes, w->codes_s, w->ids, w->ids_s, n, 0, 30, s);
  hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, w->cnt, w->off, n, s);
  hipcub::DeviceReduce::Sum(nullptr, sum_bytes, (float*)nullptr, (float*)nullptr, n, s);  // gpu_bvh_cost
  w->tmp_bytes = std::max(std::max(sort_bytes, scan_bytes), sum_bytes);
  if (hipMalloc(&w->tmp, w->tmp_bytes) != hipSuccess) {
    err = "GPU BVH builder: scratch allocation failed";
    bvh_work_free(w);
    w = nullptr;
    return false;
  }
  w->cap = n;
  return true;
}

bool bvh_work_prepare(BvhWork** w, int n, hipStream_t s, std::string& err) { return bvh_work_reserve(*w, n, s, err); }

// One launch from this module (k_build_init on the workspace), so that its code object is loaded at
// context creation rather than in the first rebuild.
__global__ void k_build_init(uint32_t* __restrict__ cb, CollapseItem* __restrict__ qa, uint32_t* __restrict__ ctr);
bool bvh_builder_warm(BvhWork* w, hipStream_t s, std::string& err) {
  if (!w) return true;
  hipLaunchKernelGGL(k_build_init, dim3(1), dim3(64), 0, s, w->cb, w->qa, w->ctr);
  if (hipGetLastError() != hipSuccess) { err = "GPU BVH builder: launch failed"; return false; }
  return true;
}

// The builder's small initial values in one launch (they were three pageable host-to-device copies, which
// go through the runtime's staging path: the first rebuilds of a context took 6-15 ms instead of 0.8-2).
// cb: the scene box accumulators (min: +bits, max: 0; then the position check's flag); qa[0]: the root item;
// ctr: node_ctr, max_stack, ncur, nnext, levels.
__global__ void k_build_init(uint32_t* __restrict__ cb, CollapseItem* __restrict__ qa, uint32_t* __restrict__ ctr) {
  const int t = threadIdx.x;
  if (t < 8) cb[t] = t < 3 ? 0xFFFFFFFFu : 0u;
  if (t < 5) ctr[t] = t == 0 || t == 2 ? 1u : 0u;
  if (t == 0) qa[0] = CollapseItem{0, 0, 0};
}

template <class Tree, class Phase>
static bool collapse_and_emit(BvhWork& w, Tree T, const int32_t* ids, const f3* pos, int n, const TreeArrays& t,
                              int* num_nodes, int* max_stack, int* depth, hipStream_t s, std::string& err, Phase&& phase);

// Builds the four-wide BVH of n triangles (pos: 3 vertices per triangle, device) into the caller's
// arrays t (device, n entries each) with the workspace *work (created or grown here, kept
// by the caller). Returns false with err set on failure. num_nodes, max_stack and depth (levels of
// the four-wide tree below the root) describe the result. The collapse runs its levels in batches of
// launches that skip themselves once the level queue is empty, with one host read per batch.
bool gpu_build_bvh(BvhWork** work, const f3* pos, int n, const TreeArrays& t, int* num_nodes, int* max_stack, int* depth,
                   hipStream_t s, std::string& err) {
  if (n < 3) { err = "GPU BVH builder needs at least 3 triangles"; return false; }
  // FOVRT_BVH_PHASES=1: host time of each phase (each followed by a stream sync) on stderr, a diagnostic
  static const bool phases = [] { const char* v = getenv("FOVRT_BVH_PHASES"); return v && atoi(v) != 0; }();
  // (host time, and the GPU time between events recorded at the phase boundaries)
  auto t_last = std::chrono::steady_clock::now();
  hipEvent_t ev_last = nullptr;
  auto phase = [&](const char* name) {
    if (!phases) return;
    using clk = std::chrono::steady_clock;
    const auto a0 = clk::now();
    hipEvent_t ev = nullptr;
    hipEventCreate(&ev);
    const auto a1 = clk::now();
    hipEventRecord(ev, s);
    const auto a2 = clk::now();
    hipStreamSynchronize(s);
    const auto t = clk::now();
    auto ms = [](clk::time_point x, clk::time_point y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
    if (!strcmp(name, "entry"))
      fprintf(stderr, "bvh entry api: create %.3f record %.3f sync %.3f ms\n", ms(a0, a1), ms(a1, a2), ms(a2, t));
    float gms = 0.0f;
    if (ev_last) { hipEventElapsedTime(&gms, ev_last, ev); hipEventDestroy(ev_last); }
    fprintf(stderr, "bvh phase %-10s %8.3f ms host %8.3f ms gpu\n", name,
            std::chrono::duration<double, std::milli>(t - t_last).count(), gms);
    t_last = t;
    ev_last = ev;
    if (!strcmp(name, "emit")) { hipEventDestroy(ev_last); ev_last = nullptr; }
  };
  phase("entry");
  if (!bvh_work_reserve(*work, n, s, err)) return false;
  BvhWork& w = **work;
  hipLaunchKernelGGL(k_build_init, dim3(1), dim3(64), 0, s, w.cb, w.qa, w.ctr);
  const int B = 256, G = (n + B - 1) / B;
  hipLaunchKernelGGL(k_prim_boxes, dim3(std::min(G, 2048)), dim3(B), 0, s, pos, n, w.blo, w.bhi, w.cb);
  hipLaunchKernelGGL(k_morton, dim3(G), dim3(B), 0, s, w.blo, w.bhi, n, w.cb, w.codes, w.ids);
  phase("morton");
  size_t tb = w.tmp_bytes;
  hipcub::DeviceRadixSort::SortPairs(w.tmp, tb, w.codes, w.codes_s, w.ids, w.ids_s, n, 0, 30, s);
  phase("sort");
  hipLaunchKernelGGL(k_karras, dim3(G), dim3(B), 0, s, w.codes_s, n, w.child, w.parent, w.range);
  hipMemsetAsync(w.arrivals, 0, (size_t)n * sizeof(uint32_t), s);
  hipLaunchKernelGGL(k_boxes_up, dim3(G), dim3(B), 0, s, n, w.ids_s, w.blo, w.bhi, w.parent, w.child, w.nlo, w.nhi,
                     w.arrivals);
  phase("karras");
  BinTree T{n, w.child, w.range, w.nlo, w.nhi, w.blo, w.bhi, w.ids_s};
  return collapse_and_emit(w, T, w.ids_s, pos, n, t, num_nodes, max_stack, depth, s, err, phase);
}

BvhWorkView bvh_work_view(BvhWork* w) { return BvhWorkView{w->blo, w->bhi, w->cb}; }

bool gpu_prim_boxes_enqueue(BvhWork* work, const f3* pos, int n, hipStream_t s, std::string& err) {
  if (!work || n < 1 || n > work->cap) { err = "GPU BVH builder: no workspace for these triangles"; return false; }
  BvhWork& w = *work;
  hipLaunchKernelGGL(k_build_init, dim3(1), dim3(64), 0, s, w.cb, w.qa, w.ctr);
  const int B = 256, G = (n + B - 1) / B;
  hipLaunchKernelGGL(k_prim_boxes, dim3(std::min(G, 2048)), dim3(B), 0, s, pos, n, w.blo, w.bhi, w.cb);
  if (hipGetLastError() != hipSuccess) { err = "GPU BVH builder: launch failure"; return false; }
  return true;
}

bool gpu_collapse_marked(BvhWork* work, const MarkedTree& T, const int32_t* ids, const f3* pos, int n, const TreeArrays& t,
                         int* num_nodes, int* max_stack, int* depth, hipStream_t s, std::string& err) {
  if (!work || n < 3 || n > work->cap) { err = "GPU BVH builder: no workspace for these triangles"; return false; }
  // (qa[0], ctr: k_build_init ran in gpu_prim_boxes_enqueue, and nothing since has touched them)
  return collapse_and_emit(*work, MarkedBinTree{T.child, T.range, T.lo, T.hi}, ids, pos, n, t, num_nodes, max_stack,
                           depth, s, err, [](const char*) {});
}

// The four-wide part of a build: the collapse of the binary tree T, whose leaves own ranges of ids, then the leaf
// scan and the triangle relayout. The collapse runs its levels in batches of launches that skip themselves once
// the level queue is empty, with one host read per batch.
template <class Tree, class Phase>
static bool collapse_and_emit(BvhWork& w, Tree T, const int32_t* ids, const f3* pos, int n, const TreeArrays& t,
                              int* num_nodes, int* max_stack, int* depth, hipStream_t s, std::string& err, Phase&& phase) {
  const int B = 256, G = (n + B - 1) / B;
  size_t tb = w.tmp_bytes;
  // (qa[0] = the root item and ctr = {1, 0, 1, 0, 0}: k_build_init)
  const int kBatch = 8;
  int launched = 0;
  CollapseItem *qa = w.qa, *qb = w.qb;
  for (;;) {
    for (int b = 0; b < kBatch; b++) {
      hipMemsetAsync(w.ctr + 3, 0, sizeof(uint32_t), s);
      // a level holds at most n items (one per inner node of the binary tree)
      hipLaunchKernelGGL(k_collapse<Tree>, dim3(G), dim3(B), 0, s, T, qa, w.ctr + 2, qb, w.ctr + 3, w.ctr, t.nodes,
                         w.ctr + 1, w.ctr + 4, nullptr);
      hipMemcpyAsync(w.ctr + 2, w.ctr + 3, sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
      std::swap(qa, qb);
    }
    launched += kBatch;
    hipMemcpyAsync(w.host, w.ctr, 5 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) { err = "GPU BVH builder: kernel failure"; return false; }
    if (w.host[2] == 0) break;
    if (launched >= 64) { err = "GPU BVH builder: collapse did not terminate"; return false; }
  }
  phase("collapse");
  *num_nodes = (int)w.host[0];
  *max_stack = (int)w.host[1];
  *depth = (int)w.host[4] - 1;
  const int nn = *num_nodes, GN = (nn + B - 1) / B;
  hipLaunchKernelGGL(k_leaf_counts<false>, dim3(GN), dim3(B), 0, s, t.nodes, nn, w.cnt, nullptr);
  tb = w.tmp_bytes;
  hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.cnt, w.off, nn, s);
  phase("scan");
  hipLaunchKernelGGL(k_emit_leaves<false>, dim3(GN), dim3(B), 0, s, t.nodes, nn, w.off, ids, pos, t.tri, t.prim, nullptr);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) {
    err = "GPU BVH builder: kernel failure";
    return false;
  }
  phase("emit");
  return true;
}

// ---------------------------------------------------------------------------------------------
// The enqueue form of a build (fr_rebuild_bvh_enqueue): the same kernels on a fixed launch schedule, nothing read
// back. What the host loop learnt from the counters stays on the device, in the context's RebuildState.
// ---------------------------------------------------------------------------------------------
// The level counters of the collapse: level L's launch reads level[L] and counts its inner children into
// level[L + 1], so no counter is reset or copied between launches.
// conditional (here and below): the build is fr_rebuild_bvh_enqueue_if's and rs->fail holds k_rebuild_decide's word;
// a skipped build starts from an empty level 0, so every collapse launch finds nothing. An unconditional build never
// reads the word a previous build left there.
__global__ void k_rebuild_begin(RebuildState* __restrict__ rs, int conditional) {
  const uint32_t root = conditional && (rs->fail & FR_REBUILD_SKIP) ? 0u : 1u;
  for (int t = threadIdx.x; t <= FR_REBUILD_LEVELS; t += blockDim.x) rs->level[t] = t == 0 ? root : 0u;
}

// The decision of a conditional build (fr_rebuild_bvh_enqueue_if; include/fovrt.h states the rule), one lane, after
// the cost terms of the tree in use and their sum (sums[0]; sums[1]: the root's area). nodes: the tree's node count
// (host_nodes when the host knows it, >= 0; else *nn_dev). The word it leaves in rs->fail is FR_REBUILD_SKIP or 0.
__global__ void k_rebuild_decide(RebuildState* __restrict__ rs, const float* __restrict__ sums, int host_nodes,
                                 const uint32_t* __restrict__ nn_dev, float ratio, int base_stale) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  rs->fail = FR_REBUILD_SKIP;
  const uint32_t nodes = host_nodes >= 0 ? (uint32_t)host_nodes : *nn_dev;
  if (nodes == 0u) return;
  const float sum = sums[0], root = sums[1];
  if (!(root > 0.0f)) return;
  const float cost = (float)(1.0 + (double)sum / (double)root);  // gpu_bvh_cost's
  if (!isfinite(cost)) return;
  rs->last_cost = cost;
  // (a baseline of 0 was never adopted: an earlier evaluation of this tree found nothing to score)
  if (base_stale || !(rs->base_cost > 0.0f)) { rs->base_cost = cost; return; }
  if (cost > ratio * rs->base_cost) rs->fail = 0u;
}

// After a conditional build, one lane: the cost of a tree it built (the terms' sum as above, over the new tree) is
// the baseline from now on. A failed or skipped build leaves the baseline alone.
__global__ void k_rebuild_rebase(RebuildState* __restrict__ rs, const float* __restrict__ sums) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || rs->fail) return;
  const float sum = sums[0], root = sums[1];
  if (!(root > 0.0f)) return;
  const float cost = (float)(1.0 + (double)sum / (double)root);
  if (!isfinite(cost)) return;
  rs->base_cost = rs->last_cost = cost;
}

// The verdict, one lane, after the last collapse launch. sah_fail: the SAH builder's failure word (NULL: the LBVH);
// ctr: node_ctr, max_stack, -, -, levels (k_build_init, k_collapse); levels: the collapse launches made. The built
// tree's numbers go to *out; rs->emit_nodes gates the leaf kernels. A skipped build keeps its word and emits nothing.
__global__ void k_rebuild_verdict(RebuildState* __restrict__ rs, const uint32_t* __restrict__ sah_fail,
                                  const uint32_t* __restrict__ ctr, int levels, TreeDesc* __restrict__ out,
                                  int conditional) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (conditional && (rs->fail & FR_REBUILD_SKIP)) {
    rs->fail = FR_REBUILD_SKIP;
    rs->emit_nodes = 0u;
    return;
  }
  uint32_t f = 0u;
  if (sah_fail && *sah_fail) f |= FR_REBUILD_FAIL_SAH;
  if (!f && ctr[1] > (uint32_t)FR_BVH_STACK) f |= FR_REBUILD_FAIL_STACK;
  if (!f && rs->level[levels] != 0u) f |= FR_REBUILD_FAIL_COLLAPSE;
  rs->fail = f;
  rs->emit_nodes = f ? 0u : ctr[0];
  if (!f) *out = TreeDesc{ctr[0], ctr[1], ctr[4] - 1u, 0u};
}

// The last kernel of an enqueued build. A failed build (rs->fail) has partly written the destination: the tree in
// use (src_*) is copied over it, whole, with its record (host_desc when the host knows that tree's numbers,
// host_nodes >= 0; *src_desc when it has not seen that tree either): 16-B words, consecutive lanes consecutive
// words, a grid-stride loop. A skipped build wrote nothing there, and the destination becomes the scene's all the
// same: the same copy. Lane 0 of block 0 counts the verdict (a skip in `skipped`, not in `failed`).
__global__ void k_rebuild_keep(RebuildState* __restrict__ rs, const BvhNode* __restrict__ src_nodes,
                               const TriGeo* __restrict__ src_tri, const int32_t* __restrict__ src_prim, int host_nodes,
                               TreeDesc host_desc, const TreeDesc* __restrict__ src_desc, int n,
                               BvhNode* __restrict__ dst_nodes, TriGeo* __restrict__ dst_tri,
                               int32_t* __restrict__ dst_prim, TreeDesc* __restrict__ dst_desc, int conditional) {
  const uint32_t f = rs->fail;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (!f) {
    if (lead) {
      rs->built++;
      if (conditional) rs->cond_built++;
    }
    return;
  }
  const TreeDesc d = host_nodes >= 0 ? host_desc : *src_desc;
  const size_t nn = min((size_t)d.nodes, (size_t)n);
  const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const f4* s4 = reinterpret_cast<const f4*>(src_nodes);
  f4* d4 = reinterpret_cast<f4*>(dst_nodes);
  for (size_t q = first; q < nn * 8; q += stride) d4[q] = s4[q];
  s4 = reinterpret_cast<const f4*>(src_tri);
  d4 = reinterpret_cast<f4*>(dst_tri);
  for (size_t q = first; q < (size_t)n * 3; q += stride) d4[q] = s4[q];
  for (size_t q = first; q < (size_t)n; q += stride) dst_prim[q] = src_prim[q];
  if (lead) {
    *dst_desc = d;
    if (f & FR_REBUILD_SKIP) { rs->skipped++; return; }
    rs->failed++;
    if (conditional) rs->cond_failed++;
    if (f & FR_REBUILD_FAIL_SAH) rs->failed_sah++;
    if (f & FR_REBUILD_FAIL_STACK) rs->failed_stack++;
    if (f & FR_REBUILD_FAIL_COLLAPSE) rs->failed_collapse++;
  }
}

static_assert(sizeof(BvhNode) == 8 * sizeof(f4) && sizeof(TriGeo) == 3 * sizeof(f4), "k_rebuild_keep copies 16-B words");

// collapse_and_emit without the host: `levels` collapse launches (level L holds at most min(4^L, n) items), the
// verdict, the leaf kernels over the capacity with the node count from the device, and the keep kernel.
// (qa[0] = the root item and ctr = {1, 0, 1, 0, 0}: k_build_init.) sah_fail: see k_rebuild_verdict; it also gates
// the collapse, whose binary tree's root is a leaf after a failure there.
template <class Tree>
static bool collapse_and_emit_enqueue(BvhWork& w, Tree T, const int32_t* ids, const f3* pos, int n, int levels,
                                      const uint32_t* sah_fail, const RebuildTarget& t, hipStream_t s, std::string& err) {
  const int B = 256, G = (n + B - 1) / B;
  RebuildState* rs = t.rs;
  CollapseItem *qa = w.qa, *qb = w.qb;
  auto collapse = sah_fail ? k_collapse<Tree, true> : k_collapse<Tree, false>;
  for (int L = 0; L < levels; L++) {
    const long long items = L < 15 ? std::min<long long>(1ll << (2 * L), n) : n;
    const int GL = (int)((items + B - 1) / B);
    hipLaunchKernelGGL(collapse, dim3(GL), dim3(B), 0, s, T, qa, rs->level + L, qb, rs->level + L + 1, w.ctr, t.dst.nodes,
                       w.ctr + 1, w.ctr + 4, sah_fail);
    std::swap(qa, qb);
  }
  hipLaunchKernelGGL(k_rebuild_verdict, dim3(1), dim3(64), 0, s, rs, sah_fail, w.ctr, levels, t.desc, t.conditional);
  hipLaunchKernelGGL(k_leaf_counts<true>, dim3(G), dim3(B), 0, s, t.dst.nodes, n, w.cnt, &rs->emit_nodes);
  size_t tb = w.tmp_bytes;
  hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.cnt, w.off, n, s);
  hipLaunchKernelGGL(k_emit_leaves<true>, dim3(G), dim3(B), 0, s, t.dst.nodes, n, w.off, ids, pos, t.dst.tri, t.dst.prim,
                     &rs->emit_nodes);
  const int GK = (int)std::min<long long>(((long long)n * 8 + B - 1) / B, 2048);
  hipLaunchKernelGGL(k_rebuild_keep, dim3(GK), dim3(B), 0, s, rs, t.src.nodes, t.src.tri, t.src.prim, t.src_host_nodes,
                     t.src_host_desc, t.src_desc, n, t.dst.nodes, t.dst.tri, t.dst.prim, t.desc, t.conditional);
  if (hipGetLastError() != hipSuccess) { err = "GPU BVH builder: launch failure"; return false; }
  return true;
}

bool gpu_collapse_marked_enqueue(BvhWork* work, const MarkedTree& T, const int32_t* ids, const f3* pos, int n, int levels,
                                 const uint32_t* sah_fail, const RebuildTarget& t, hipStream_t s, std::string& err) {
  if (!work || n < 3 || n > work->cap || levels < 1 || levels > FR_REBUILD_LEVELS || !sah_fail) {
    err = "GPU BVH builder: no workspace for these triangles";
    return false;
  }
  return collapse_and_emit_enqueue(*work, MarkedBinTree{T.child, T.range, T.lo, T.hi}, ids, pos, n, levels, sah_fail, t, s,
                                   err);
}

bool gpu_rebuild_begin_enqueue(RebuildState* rs, int conditional, hipStream_t s, std::string& err) {
  hipLaunchKernelGGL(k_rebuild_begin, dim3(1), dim3(128), 0, s, rs, conditional);
  if (hipGetLastError() != hipSuccess) { err = "GPU BVH builder: launch failure"; return false; }
  return true;
}

// gpu_build_bvh in stream order: the same launches up to the binary tree (they never read anything back), then
// collapse_and_emit_enqueue with today's bound of 64 collapse launches. The workspace must exist (fr_create's).
bool gpu_build_bvh_enqueue(BvhWork* work, const f3* pos, int n, const RebuildTarget& t, hipStream_t s, std::string& err) {
  if (!work || n < 3 || n > work->cap) { err = "GPU BVH builder: no workspace for these triangles"; return false; }
  BvhWork& w = *work;
  if (!gpu_rebuild_begin_enqueue(t.rs, t.conditional, s, err)) return false;
  hipLaunchKernelGGL(k_build_init, dim3(1), dim3(64), 0, s, w.cb, w.qa, w.ctr);
  const int B = 256, G = (n + B - 1) / B;
  hipLaunchKernelGGL(k_prim_boxes, dim3(std::min(G, 2048)), dim3(B), 0, s, pos, n, w.blo, w.bhi, w.cb);
  hipLaunchKernelGGL(k_morton, dim3(G), dim3(B), 0, s, w.blo, w.bhi, n, w.cb, w.codes, w.ids);
  size_t tb = w.tmp_bytes;
  hipcub::DeviceRadixSort::SortPairs(w.tmp, tb, w.codes, w.codes_s, w.ids, w.ids_s, n, 0, 30, s);
  hipLaunchKernelGGL(k_karras, dim3(G), dim3(B), 0, s, w.codes_s, n, w.child, w.parent, w.range);
  hipMemsetAsync(w.arrivals, 0, (size_t)n * sizeof(uint32_t), s);
  hipLaunchKernelGGL(k_boxes_up, dim3(G), dim3(B), 0, s, n, w.ids_s, w.blo, w.bhi, w.parent, w.child, w.nlo, w.nhi,
                     w.arrivals);
  BinTree T{n, w.child, w.range, w.nlo, w.nhi, w.blo, w.bhi, w.ids_s};
  return collapse_and_emit_enqueue(w, T, w.ids_s, pos, n, FR_REBUILD_LEVELS, nullptr, t, s, err);
}

// Refits the four-wide tree t.nodes[0, num_nodes) (either builder's) over new positions, in place: every slot box
// and tri[j] for every leaf-order j are rewritten, child / count / prim are not. num_nodes == 0 (the whole scene
// is one leaf): tri only. Three launches whatever the depth, no allocation; the scratch is *work's nlo / nhi
// (raw node boxes), parent and arrivals, which hold one entry per triangle (a tree has at most as many nodes).
// gpu_refit_bvh_enqueue launches them and returns (reject: NULL, or the device verdict word of an enqueued update,
// which selects the gated kernels); gpu_refit_bvh also waits for them.
// nodes_dev (the enqueue forms; NULL: num_nodes is the tree's): the tree's node count in device memory, for a tree
// the host has not seen (fr_rebuild_bvh_enqueue). num_nodes is ignored then and the grids cover the capacity, n.
bool gpu_refit_bvh_enqueue(BvhWork* work, const f3* pos, int n, const TreeArrays& t, int num_nodes,
                           const uint32_t* reject, const uint32_t* nodes_dev, hipStream_t s, std::string& err) {
  if (nodes_dev) num_nodes = n;
  if (!work || n < 1 || n > work->cap || num_nodes < 0 || num_nodes > work->cap || (nodes_dev && !reject)) {
    err = "GPU BVH refit: no workspace for this tree";
    return false;
  }
  BvhWork& w = *work;
  const int B = 256;
  auto tris = reject ? k_refit_tris<true> : k_refit_tris<false>;
  auto links = nodes_dev ? k_refit_links<true, true> : reject ? k_refit_links<true> : k_refit_links<false>;
  auto up = nodes_dev ? k_refit_up<true, true> : reject ? k_refit_up<true> : k_refit_up<false>;
  hipLaunchKernelGGL(tris, dim3((n + B - 1) / B), dim3(B), 0, s, pos, t.prim, n, t.tri, reject);
  if (num_nodes > 0) {
    const int GN = (num_nodes + B - 1) / B;
    hipLaunchKernelGGL(links, dim3(GN), dim3(B), 0, s, t.nodes, num_nodes, w.parent, w.arrivals, reject, nodes_dev);
    hipLaunchKernelGGL(up, dim3(GN), dim3(B), 0, s, t.nodes, num_nodes, pos, t.prim, w.parent, w.arrivals, w.nlo, w.nhi,
                       reject, nodes_dev);
  }
  if (hipGetLastError() != hipSuccess) {
    err = "GPU BVH refit: launch failure";
    return false;
  }
  return true;
}

// The refit of an enqueued update out of place (k_refit_*_to): from the tree in use (src) over `pos` into the
// arrays no frame in flight reads (dst, room for num_nodes nodes and n triangles), whole. reject: the device
// verdict word, never NULL. The same scratch, the same three launches, no wait.
bool gpu_refit_bvh_to_enqueue(BvhWork* work, const f3* pos, int n, const TreeArrays& src, int num_nodes,
                              const TreeArrays& dst, const uint32_t* reject, const uint32_t* nodes_dev, hipStream_t s,
                              std::string& err) {
  if (nodes_dev) num_nodes = n;
  if (!work || !reject || n < 1 || n > work->cap || num_nodes < 0 || num_nodes > work->cap) {
    err = "GPU BVH refit: no workspace for this tree";
    return false;
  }
  BvhWork& w = *work;
  const int B = 256;
  hipLaunchKernelGGL(k_refit_tris_to, dim3((n + B - 1) / B), dim3(B), 0, s, pos, src.prim, src.tri, n, dst.tri, dst.prim,
                     reject);
  if (num_nodes > 0) {
    const int GN = (num_nodes + B - 1) / B;
    hipLaunchKernelGGL(nodes_dev ? k_refit_links_to<true> : k_refit_links_to<false>, dim3(GN), dim3(B), 0, s, src.nodes,
                       num_nodes, w.parent, w.arrivals, dst.nodes, reject, nodes_dev);
    hipLaunchKernelGGL(nodes_dev ? k_refit_up_to<true> : k_refit_up_to<false>, dim3(GN), dim3(B), 0, s, src.nodes,
                       dst.nodes, num_nodes, pos, src.prim, w.parent, w.arrivals, w.nlo, w.nhi, reject, nodes_dev);
  }
  if (hipGetLastError() != hipSuccess) {
    err = "GPU BVH refit: launch failure";
    return false;
  }
  return true;
}

bool gpu_refit_bvh(BvhWork* work, const f3* pos, int n, const TreeArrays& t, int num_nodes, hipStream_t s,
                   std::string& err) {
  if (!gpu_refit_bvh_enqueue(work, pos, n, t, num_nodes, nullptr, nullptr, s, err)) return false;
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) {
    err = "GPU BVH refit: kernel failure";
    return false;
  }
  return true;
}

// SAH cost of the tree: 1 + (sum over non-empty slots of area(stored box) * (1 | leaf count)) / area(root), the
// root being the union of node 0's slot boxes. One f32 term per node, summed by hipCUB (a tree reduction: its
// error does not grow with the node count as an atomic accumulation's would), the division in f64 on the host.
bool gpu_bvh_cost(BvhWork* work, const BvhNode* nodes, int num_nodes, float* cost, hipStream_t s, std::string& err) {
  if (!work || num_nodes < 1 || num_nodes > work->cap) { err = "GPU BVH cost: no workspace for this tree"; return false; }
  BvhWork& w = *work;
  const int B = 256;
  float* part = reinterpret_cast<float*>(w.codes);
  float* sums = reinterpret_cast<float*>(w.ctr + 5);  // sum, root area
  hipLaunchKernelGGL(k_cost_terms<false>, dim3((num_nodes + B - 1) / B), dim3(B), 0, s, nodes, num_nodes, part, sums + 1,
                     nullptr, nullptr);
  size_t tb = w.tmp_bytes;
  hipcub::DeviceReduce::Sum(w.tmp, tb, part, sums, num_nodes, s);
  hipMemcpyAsync(w.host + 5, w.ctr + 5, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) {
    err = "GPU BVH cost: kernel failure";
    return false;
  }
  float sum, root;
  memcpy(&sum, w.host + 5, sizeof(float));
  memcpy(&root, w.host + 6, sizeof(float));
  if (!(root > 0.0f)) { err = "GPU BVH cost: the root box has no area"; return false; }
  *cost = (float)(1.0 + (double)sum / (double)root);
  return true;
}

// The cost in stream order, for a conditional build (fr_rebuild_bvh_enqueue_if): gpu_bvh_cost's terms and sum into the
// same scratch, nothing read back. nodes_dev (NULL: num_nodes is the tree's): the node count in device memory; the
// grid and the sum then cover the capacity, n. gate: k_cost_terms'.
static void cost_enqueue(BvhWork& w, const BvhNode* nodes, int num_nodes, int n, const uint32_t* nodes_dev,
                         const uint32_t* gate, hipStream_t s) {
  const int B = 256, len = nodes_dev ? n : num_nodes;
  float* part = reinterpret_cast<float*>(w.codes);
  float* sums = reinterpret_cast<float*>(w.ctr + 5);
  hipLaunchKernelGGL(nodes_dev ? k_cost_terms<true> : k_cost_terms<false>, dim3((len + B - 1) / B), dim3(B), 0, s, nodes,
                     len, part, sums + 1, nodes_dev, gate);
  size_t tb = w.tmp_bytes;
  hipcub::DeviceReduce::Sum(w.tmp, tb, part, sums, len, s);
}

// The decision of a conditional build, ahead of its schedule: the cost of the tree in use (num_nodes, or nodes_dev for
// a tree the host has not seen) and k_rebuild_decide, which leaves the verdict word in rs->fail. No wait.
bool gpu_rebuild_decide_enqueue(BvhWork* work, RebuildState* rs, const BvhNode* nodes, int num_nodes, int n,
                                const uint32_t* nodes_dev, float ratio, bool base_stale, hipStream_t s,
                                std::string& err) {
  if (!work || n < 1 || n > work->cap || num_nodes < 0 || num_nodes > work->cap) {
    err = "GPU BVH cost: no workspace for this tree";
    return false;
  }
  BvhWork& w = *work;
  if (nodes_dev || num_nodes > 0) cost_enqueue(w, nodes, num_nodes, n, nodes_dev, nullptr, s);
  hipLaunchKernelGGL(k_rebuild_decide, dim3(1), dim3(64), 0, s, rs, reinterpret_cast<const float*>(w.ctr + 5),
                     nodes_dev ? -1 : num_nodes, nodes_dev, ratio, base_stale ? 1 : 0);
  if (hipGetLastError() != hipSuccess) { err = "GPU BVH cost: launch failure"; return false; }
  return true;
}

// Behind a conditional build: the cost of the tree it made (t.dst.nodes, whose node count is t.desc's) becomes the
// baseline (k_rebuild_rebase). After a failed or skipped build the terms are not read and nothing changes. No wait.
bool gpu_rebuild_rebase_enqueue(BvhWork* work, const RebuildTarget& t, int n, hipStream_t s, std::string& err) {
  if (!work || n < 1 || n > work->cap) { err = "GPU BVH cost: no workspace for this tree"; return false; }
  BvhWork& w = *work;
  cost_enqueue(w, t.dst.nodes, n, n, &t.desc->nodes, &t.rs->fail, s);
  hipLaunchKernelGGL(k_rebuild_rebase, dim3(1), dim3(64), 0, s, t.rs, reinterpret_cast<const float*>(w.ctr + 5));
  if (hipGetLastError() != hipSuccess) { err = "GPU BVH cost: launch failure"; return false; }
  return true;
}

// Checks n triangles of device positions (any device pointer the caller owns) in one pass: *finite, and
// box[0..2] = min, box[3..5] = max over all vertices. One kernel, one small copy back.
// gpu_check_positions_enqueue launches the check and leaves its result on the device (the workspace's cb words,
// which k_take_over reads); gpu_check_positions also copies it back and waits.
bool gpu_check_positions_enqueue(BvhWork* work, const float* xyz, int n, hipStream_t s, std::string& err) {
  if (!work || n < 1) { err = "GPU position check: no workspace"; return false; }
  BvhWork& w = *work;
  hipLaunchKernelGGL(k_build_init, dim3(1), dim3(64), 0, s, w.cb, w.qa, w.ctr);
  const int B = 256;
  const size_t nverts = (size_t)n * 3;
  const int G = (int)std::min<size_t>((nverts + B - 1) / B, 2048);
  hipLaunchKernelGGL(k_check_positions, dim3(G), dim3(B), 0, s, xyz, nverts, w.cb);
  if (hipGetLastError() != hipSuccess) { err = "GPU position check: launch failure"; return false; }
  return true;
}

// The take-over of an enqueued update (k_take_over), after gpu_check_positions_enqueue and, with given normals,
// the normals check into st->bad_nrm (bad_nrm then, else NULL). No wait.
bool gpu_take_over_positions(BvhWork* work, const f3* xyz, const f3* cur, int n, f3* dst, const uint32_t* bad_nrm,
                             GeoUpdateState* st, int flags, f3 seed_lo, f3 seed_hi, hipStream_t s, std::string& err) {
  if (!work || n < 1) { err = "GPU position take-over: no workspace"; return false; }
  const int B = 256;
  const size_t nverts = (size_t)n * 3;
  hipLaunchKernelGGL(k_take_over, dim3((unsigned)((nverts + B - 1) / B)), dim3(B), 0, s, xyz, cur, nverts, dst,
                     work->cb, bad_nrm, st, flags, seed_lo, seed_hi);
  if (hipGetLastError() != hipSuccess) { err = "GPU position take-over: launch failure"; return false; }
  return true;
}

bool gpu_check_positions(BvhWork* work, const float* xyz, int n, bool* finite, float box[6], hipStream_t s,
                         std::string& err) {
  if (!gpu_check_positions_enqueue(work, xyz, n, s, err)) return false;
  BvhWork& w = *work;
  hipMemcpyAsync(w.host, w.cb, 7 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) {
    err = "GPU position check: kernel failure (is the pointer device memory of ntris x 9 floats?)";
    return false;
  }
  *finite = w.host[6] == 0;
  for (int k = 0; k < 6; k++) {
    const uint32_t u = w.host[k];
    const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;  // unord
    memcpy(&box[k], &b, sizeof(float));
  }
  return true;
}

}  // namespace fr
