// k_bvh_sah.hip — the device binned-SAH builder (fr_config.bvh_builder = 2): scene.cpp's Builder at its defaults
// (leaf 2, 16 bins, the widest centroid axis, depth 30), restated for the device so that the tree is the host's.
//
// Why the trees can be equal: every quantity that decides a split is a min, a max or an integer count, exact in
// any order; the rest (bin index, areas, costs) is fp32 arithmetic evaluated per node in the host's order, and
// both sides are built with -ffp-contract=off. What is free is the order in which the nodes of a level take their
// indices and the order of the triangles inside a leaf (include/fovrt.h, bvh_builder, states the rule).
//
// The binary tree is built top down, one level per round of launches (at most 30 rounds; level order comes from
// the launches alone, no kernel waits for another block). The nodes of a level are the consecutive ids the level
// above allocated. `ids` holds the primitives of every node as one range, in ascending primitive order (the
// partition is stable), so "the n/2 lowest primitive indices" of the equal-centroid rule is the first half.
//   small nodes (<= 64 triangles): one wave per node does everything (k_sah_small): centroid bounds by wave
//     reduction, bins in LDS, candidate k by lane k, the partition by ballot, in place;
//   large nodes: one lane per triangle. k_sah_bin bins into the node's global slot (a block whose first triangle's
//     node covers most of it accumulates in LDS and flushes once); k_sah_select runs the fifteen candidates, one
//     lane per node, and makes the children; k_sah_flags + a hipCUB scan + k_sah_move_read / k_sah_move_write are
//     the stable partition (read everything, then write: in place), and the move also gathers the children's
//     centroid bounds.
// A child's box is the union of the bins on its side: the union of its triangles' boxes.
// The four-wide part is k_bvh.hip's (gpu_collapse_marked): collapse, leaf scan, triangle relayout.
// gpu_build_bvh_sah reads the counters back once per eight levels and stops when a level made no node;
// gpu_build_bvh_sah_enqueue (fr_rebuild_bvh_enqueue) launches every level and reads nothing back.
//
// Not the host's: a node with ex > 0 none of whose candidates has a finite cost (coordinates around 1e19) fails
// the build (the host falls back to a median there), and the host's FOVRT_BVH_* tuning variables are not read.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdint>
#include <string>
#include "fr_device.h"
#include "k_launch.h"

namespace fr {
namespace {

constexpr int kLeaf = 2, kBins = 16, kMaxDepth = 30;  // scene.cpp Builder's defaults
constexpr int kSmall = 64;                            // a node of at most this many triangles is one wave's
// A large node's slot, in words: cnt[16], lo[3][16], hi[3][16] (order-mapped), then the node's centroid bounds
// (min[3], max[3], order-mapped) and the chosen split.
constexpr int kBinWords = 7 * kBins, kSlotCb = kBinWords, kSlotK = kBinWords + 6, kSlotWords = 120;
// counters: nodes allocated; the level's nodes [first, end); large nodes of this level and of the next; failure
enum { C_NODES = 0, C_FIRST, C_END, C_BIG_CUR, C_BIG_NEXT, C_FAIL, C_WORDS = 8 };

FR_DEV uint32_t ord(float f) {  // k_bvh.hip's: float <-> unsigned with the same order
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FR_DEV float unord(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

FR_DEV float area_of(f3 lo, f3 hi) {  // scene.cpp Box::area
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
FR_DEV f3 min3(f3 a, f3 b) { return mk3(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)); }
FR_DEV f3 max3(f3 a, f3 b) { return mk3(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z)); }

struct SahDev {
  int n, node_cap, slot_cap;
  const f4 *blo, *bhi;  // primitive boxes (the LBVH workspace's)
  int32_t* ids;         // position -> primitive
  int32_t* node_of;     // position -> the last large node that moved it (large nodes only look at their own)
  uint32_t *flag, *scan;
  int32_t *tmp_id, *tmp_dst;
  int2 *rng, *kid;  // node -> [b, e) of ids; children ({-1, -1}: a leaf)
  f4 *nlo, *nhi;    // node -> raw box
  int32_t* bslot;   // node -> its slot when it is large and will be split, else -1
  uint32_t* ctr;
};

// How a node is split: 0 binned on `axis`, 1 equal centroids (first half / second half), 2 not at all (the extent
// is not a number or not finite)
struct Axis {
  int axis, mode;
  float lo, ex;
};
FR_DEV Axis axis_of(f3 cmin, f3 cmax) {
  const f3 ext = cmax - cmin;
  Axis a;
  a.axis = ext.x > ext.y ? (ext.x > ext.z ? 0 : 2) : (ext.y > ext.z ? 1 : 2);
  a.lo = a.axis == 0 ? cmin.x : a.axis == 1 ? cmin.y : cmin.z;
  a.ex = a.axis == 0 ? ext.x : a.axis == 1 ? ext.y : ext.z;
  a.mode = a.ex > 0.0f ? (a.ex < INFINITY ? 0 : 2) : (a.ex == 0.0f ? 1 : 2);
  return a;
}
// the bin of a triangle (rank: its place in the node's range, size: the node's triangles)
FR_DEV int bin_of(const Axis& a, f3 ce, int rank, int size) {
  if (a.mode != 0) return rank < size / 2 ? 0 : 1;
  const float key = a.axis == 0 ? ce.x : a.axis == 1 ? ce.y : ce.z;
  const int k = (int)((key - a.lo) / a.ex * kBins);
  return k < 0 ? 0 : (k >= kBins ? kBins - 1 : k);
}

FR_DEV void slot_init(uint32_t* S) {
  for (int t = 0; t < kSlotWords; t++) S[t] = t < kBins ? 0u : (t < 4 * kBins ? 0xFFFFFFFFu : (t < kBinWords ? 0u : (t < kSlotCb + 3 ? 0xFFFFFFFFu : 0u)));
}

// A node that cannot be split (no finite candidate, or a bound that cannot be reached was): the failure flag, and
// the node stays a leaf, which every later kernel handles.
FR_DEV int fail_node(const SahDev& D, int node) {
  atomicOr(&D.ctr[C_FAIL], 1u);
  D.kid[node] = int2{-1, -1};
  return -1;
}

// One lane: the two children of `node` (depth: its level), left of nl triangles with box [llo, lhi], right with the
// rest and [rlo, rhi]. *cbase: the left child's id (the right one follows).
FR_DEV bool make_children(const SahDev& D, int node, int depth, int nl, f3 llo, f3 lhi, f3 rlo, f3 rhi,
                          uint32_t* next_slots, int* cbase) {
  const int c = (int)atomicAdd(&D.ctr[C_NODES], 2u);
  if (c + 2 > D.node_cap) { fail_node(D, node); return false; }  // (cannot happen: at most 2n - 1 nodes)
  const int2 r = D.rng[node];
  for (int side = 0; side < 2; side++) {
    const int ch = c + side;
    const int2 cr = side ? int2{r.x + nl, r.y} : int2{r.x, r.x + nl};
    const int sz = cr.y - cr.x;
    const bool leaf = sz <= kLeaf || depth + 1 >= kMaxDepth;
    D.rng[ch] = cr;
    D.kid[ch] = leaf ? int2{-1, -1} : int2{0, 0};
    D.nlo[ch] = side ? mk4(rlo, 0.0f) : mk4(llo, 0.0f);
    D.nhi[ch] = side ? mk4(rhi, 0.0f) : mk4(lhi, 0.0f);
    int slot = -1;
    if (!leaf && sz > kSmall) {
      slot = (int)atomicAdd(&D.ctr[C_BIG_NEXT], 1u);
      if (slot >= D.slot_cap) {  // (cannot happen: the large nodes of a level are disjoint ranges of > kSmall)
        atomicOr(&D.ctr[C_FAIL], 1u);
        D.kid[ch] = int2{-1, -1};
        slot = -1;
      } else {
        slot_init(next_slots + (size_t)slot * kSlotWords);
      }
    }
    D.bslot[ch] = slot;
  }
  D.kid[node] = int2{c, c + 1};
  *cbase = c;
  return true;
}

// Candidate k (1..15) of a node from its bins, the host's: l over the bins < k, r over the bins >= k, each the union
// of its non-empty bins; INFINITY when a side is empty or the cost is not a number.
FR_DEV float candidate(const uint32_t* bins, int k, f3* llo, f3* lhi, f3* rlo, f3* rhi, int* nl_out) {
  f3 ll = mk3(INFINITY), lh = mk3(-INFINITY), rl = mk3(INFINITY), rh = mk3(-INFINITY);
  int nl = 0, nr = 0;
#pragma unroll
  for (int j = 0; j < kBins; j++) {
    const int c = (int)bins[j];
    if (!c) continue;
    const f3 lo = mk3(unord(bins[kBins + j]), unord(bins[2 * kBins + j]), unord(bins[3 * kBins + j]));
    const f3 hi = mk3(unord(bins[4 * kBins + j]), unord(bins[5 * kBins + j]), unord(bins[6 * kBins + j]));
    if (j < k) { ll = min3(ll, lo); lh = max3(lh, hi); nl += c; }
    else { rl = min3(rl, lo); rh = max3(rh, hi); nr += c; }
  }
  *llo = ll; *lhi = lh; *rlo = rl; *rhi = rh; *nl_out = nl;
  if (!nl || !nr) return INFINITY;
  const float c = area_of(ll, lh) * (float)nl + area_of(rl, rh) * (float)nr;
  return c < INFINITY ? c : INFINITY;
}

// One lane: the split of `node` (depth: its level) from its bins, and its two children. Returns the chosen k
// (left: bins < k), or -1 after fail_node. *cbase: the left child's id, *nl: the left child's triangles.
FR_DEV int split_node(const SahDev& D, int node, int depth, const uint32_t* bins, int mode, uint32_t* next_slots,
                      int* cbase, int* nl_out) {
  int cnt[kBins];
#pragma unroll
  for (int k = 0; k < kBins; k++) cnt[k] = (int)bins[k];
  auto blo = [&](int k) { return mk3(unord(bins[kBins + k]), unord(bins[2 * kBins + k]), unord(bins[3 * kBins + k])); };
  auto bhi = [&](int k) { return mk3(unord(bins[4 * kBins + k]), unord(bins[5 * kBins + k]), unord(bins[6 * kBins + k])); };
  int best_k = -1;
  if (mode == 1) {
    best_k = 1;
  } else if (mode == 0) {
    // r over bins >= k for every k, then l over bins < k growing with k: the host's unions, which are the same
    // min / max in any order
    float ra[kBins];
    int rn[kBins];
    {
      f3 lo = mk3(INFINITY), hi = mk3(-INFINITY);
      int nr = 0;
#pragma unroll
      for (int k = kBins - 1; k >= 1; k--) {
        if (cnt[k]) { lo = min3(lo, blo(k)); hi = max3(hi, bhi(k)); nr += cnt[k]; }
        ra[k] = area_of(lo, hi);
        rn[k] = nr;
      }
    }
    f3 lo = mk3(INFINITY), hi = mk3(-INFINITY);
    int nl = 0;
    float best = INFINITY;
#pragma unroll
    for (int k = 1; k < kBins; k++) {
      if (cnt[k - 1]) { lo = min3(lo, blo(k - 1)); hi = max3(hi, bhi(k - 1)); nl += cnt[k - 1]; }
      if (!nl || !rn[k]) continue;
      const float c = area_of(lo, hi) * (float)nl + ra[k] * (float)rn[k];
      if (c < best) { best = c; best_k = k; }
    }
  }
  if (best_k <= 0) return fail_node(D, node);
  f3 llo = mk3(INFINITY), lhi = mk3(-INFINITY), rlo = mk3(INFINITY), rhi = mk3(-INFINITY);
  int nl = 0;
#pragma unroll
  for (int k = 0; k < kBins; k++) {
    if (!cnt[k]) continue;
    if (k < best_k) { llo = min3(llo, blo(k)); lhi = max3(lhi, bhi(k)); nl += cnt[k]; }
    else { rlo = min3(rlo, blo(k)); rhi = max3(rhi, bhi(k)); }
  }
  if (!make_children(D, node, depth, nl, llo, lhi, rlo, rhi, next_slots, cbase)) return -1;
  *nl_out = nl;
  return best_k;
}

// The root, its slot (the centroid bounds are k_prim_boxes') and the counters. verdict: NULL, or the word of a
// conditional build (RebuildState::fail); a skipped one starts without a root, so every level finds nothing.
__global__ void k_sah_init(SahDev D, const uint32_t* __restrict__ cb, uint32_t* __restrict__ slots0,
                           const uint32_t* __restrict__ verdict) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (verdict && (*verdict & FR_REBUILD_SKIP)) {
    for (int k = 0; k < C_WORDS; k++) D.ctr[k] = 0u;
    return;
  }
  D.rng[0] = int2{0, D.n};
  D.kid[0] = int2{0, 0};
  D.nlo[0] = mk4(0.0f, 0.0f, 0.0f, 0.0f);
  D.nhi[0] = mk4(0.0f, 0.0f, 0.0f, 0.0f);
  const bool big = D.n > kSmall;
  D.bslot[0] = big ? 0 : -1;
  if (big) {
    slot_init(slots0);
    for (int k = 0; k < 6; k++) slots0[kSlotCb + k] = cb[k];
  }
  for (int k = 0; k < C_WORDS; k++) D.ctr[k] = 0u;
  D.ctr[C_NODES] = 1u;
  D.ctr[C_BIG_NEXT] = big ? 1u : 0u;
}

// The next level: the nodes allocated since the last call.
__global__ void k_sah_level(uint32_t* __restrict__ ctr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ctr[C_FIRST] = ctr[C_END];
  ctr[C_END] = ctr[C_NODES];
  ctr[C_BIG_CUR] = ctr[C_BIG_NEXT];
  ctr[C_BIG_NEXT] = 0u;
}

// Small nodes of the level, one wave each (a grid-stride loop over the level's nodes).
__global__ void __launch_bounds__(256) k_sah_small(SahDev D, int depth) {
  __shared__ uint32_t sb[4][kBinWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int first = (int)D.ctr[C_FIRST], end = (int)D.ctr[C_END];
  const int nw = gridDim.x * 4;
  uint32_t* B = sb[wv];
  for (int node = first + blockIdx.x * 4 + wv; node < end; node += nw) {
    const int2 r = D.rng[node];
    const int sz = r.y - r.x;
    if (D.kid[node].x < 0 || sz > kSmall) continue;  // a leaf, or a large node
    const bool act = lane < sz;
    const int id = act ? D.ids[r.x + lane] : 0;
    const f3 lo = act ? xyz(D.blo[id]) : mk3(INFINITY), hi = act ? xyz(D.bhi[id]) : mk3(-INFINITY);
    const f3 ce = (lo + hi) * 0.5f;
    const f3 cmin = mk3(wave_min(act ? ce.x : INFINITY), wave_min(act ? ce.y : INFINITY), wave_min(act ? ce.z : INFINITY));
    const f3 cmax = mk3(wave_max(act ? ce.x : -INFINITY), wave_max(act ? ce.y : -INFINITY), wave_max(act ? ce.z : -INFINITY));
    const Axis A = axis_of(cmin, cmax);
    const int bin = bin_of(A, ce, lane, sz);
    for (int t = lane; t < kBinWords; t += 64) B[t] = t < kBins ? 0u : (t < 4 * kBins ? 0xFFFFFFFFu : 0u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (act) {
      atomicAdd(&B[bin], 1u);
      atomicMin(&B[kBins + bin], ord(lo.x)); atomicMin(&B[2 * kBins + bin], ord(lo.y)); atomicMin(&B[3 * kBins + bin], ord(lo.z));
      atomicMax(&B[4 * kBins + bin], ord(hi.x)); atomicMax(&B[5 * kBins + bin], ord(hi.y)); atomicMax(&B[6 * kBins + bin], ord(hi.z));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the fifteen candidates, lane k's is k; the host takes them in order and keeps the first of strictly smaller
    // cost: the smallest cost, and among equal ones the lowest k. Equal centroids: k = 1 (bins 0 and 1 are the halves).
    f3 llo, lhi, rlo, rhi;
    int nl = 0;
    const int kc = lane >= 1 && lane < kBins ? lane : 1;
    float cost = candidate(B, kc, &llo, &lhi, &rlo, &rhi, &nl);
    if (lane < 1 || lane >= kBins) cost = INFINITY;
    int k = -1;
    if (A.mode == 1) {
      k = 1;
    } else if (A.mode == 0) {
      const float best = wave_min(cost);
      if (best < INFINITY) k = __ffsll((long long)__ballot(cost == best)) - 1;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int ok = 1, cbase = 0;
    if (lane == (k > 0 ? k : 0))
      ok = k > 0 ? (int)make_children(D, node, depth, nl, llo, lhi, rlo, rhi, nullptr, &cbase) : fail_node(D, node) + 1;
    if (k <= 0 || !__shfl(ok, k, 64)) continue;
    nl = __shfl(nl, k, 64);
    // the stable partition, in place: every lane has read its primitive
    const bool left = act && bin < k;
    const unsigned long long lm = __ballot(left);
    const int lrank = __popcll(lm & ((1ull << lane) - 1ull));
    if (act) D.ids[r.x + (left ? lrank : nl + lane - lrank)] = id;
  }
}

// Large nodes: the bins of the level, one lane per position.
__global__ void __launch_bounds__(256) k_sah_bin(SahDev D, uint32_t* __restrict__ slots) {
  __shared__ uint32_t sb[kBinWords];
  __shared__ int s_node;
  if (D.ctr[C_BIG_CUR] == 0u) return;
  const int first = (int)D.ctr[C_FIRST], end = (int)D.ctr[C_END];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int node = i < D.n ? D.node_of[i] : -1;
  const int slot = node >= first && node < end ? D.bslot[node] : -1;
  if (threadIdx.x == 0) s_node = slot >= 0 ? node : -1;
  if (threadIdx.x < kBinWords) sb[threadIdx.x] = threadIdx.x < kBins ? 0u : (threadIdx.x < 4 * kBins ? 0xFFFFFFFFu : 0u);
  __syncthreads();
  const int n0 = s_node;  // the block's first node accumulates in LDS
  if (slot >= 0) {
    uint32_t* S = slots + (size_t)slot * kSlotWords;
    const int2 r = D.rng[node];
    const int id = D.ids[i];
    const f3 lo = xyz(D.blo[id]), hi = xyz(D.bhi[id]);
    const f3 ce = (lo + hi) * 0.5f;
    const Axis A = axis_of(mk3(unord(S[kSlotCb]), unord(S[kSlotCb + 1]), unord(S[kSlotCb + 2])),
                           mk3(unord(S[kSlotCb + 3]), unord(S[kSlotCb + 4]), unord(S[kSlotCb + 5])));
    const int bin = bin_of(A, ce, i - r.x, r.y - r.x);
    D.flag[i] = (uint32_t)bin;
    if (node == n0) {
      atomicAdd(&sb[bin], 1u);
      atomicMin(&sb[kBins + bin], ord(lo.x)); atomicMin(&sb[2 * kBins + bin], ord(lo.y)); atomicMin(&sb[3 * kBins + bin], ord(lo.z));
      atomicMax(&sb[4 * kBins + bin], ord(hi.x)); atomicMax(&sb[5 * kBins + bin], ord(hi.y)); atomicMax(&sb[6 * kBins + bin], ord(hi.z));
    } else {
      atomicAdd(&S[bin], 1u);
      atomicMin(&S[kBins + bin], ord(lo.x)); atomicMin(&S[2 * kBins + bin], ord(lo.y)); atomicMin(&S[3 * kBins + bin], ord(lo.z));
      atomicMax(&S[4 * kBins + bin], ord(hi.x)); atomicMax(&S[5 * kBins + bin], ord(hi.y)); atomicMax(&S[6 * kBins + bin], ord(hi.z));
    }
  }
  __syncthreads();
  if (n0 >= 0 && threadIdx.x < kBinWords) {
    uint32_t* S0 = slots + (size_t)D.bslot[n0] * kSlotWords;
    const int t = threadIdx.x;
    const uint32_t v = sb[t];
    // (min / max: an atomic only where it can change the bound, which an earlier read decides safely)
    if (t < kBins) { if (v) atomicAdd(&S0[t], v); }
    else if (t < 4 * kBins) { if (v < __hip_atomic_load(&S0[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&S0[t], v); }
    else if (v > __hip_atomic_load(&S0[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&S0[t], v);
  }
}

// Large nodes: the split and the children, one lane per node of the level.
__global__ void k_sah_select(SahDev D, int depth, uint32_t* __restrict__ slots, uint32_t* __restrict__ next_slots) {
  if (D.ctr[C_BIG_CUR] == 0u) return;
  const int first = (int)D.ctr[C_FIRST], end = (int)D.ctr[C_END];
  for (int node = first + blockIdx.x * blockDim.x + threadIdx.x; node < end; node += gridDim.x * blockDim.x) {
    const int slot = D.bslot[node];
    if (slot < 0) continue;
    uint32_t* S = slots + (size_t)slot * kSlotWords;
    const Axis A = axis_of(mk3(unord(S[kSlotCb]), unord(S[kSlotCb + 1]), unord(S[kSlotCb + 2])),
                           mk3(unord(S[kSlotCb + 3]), unord(S[kSlotCb + 4]), unord(S[kSlotCb + 5])));
    int cbase, nl;
    S[kSlotK] = (uint32_t)split_node(D, node, depth, S, A.mode, next_slots, &cbase, &nl);
  }
}

// Large nodes: bin -> "goes left", the scan's input (0 everywhere else).
__global__ void k_sah_flags(SahDev D, const uint32_t* __restrict__ slots) {
  if (D.ctr[C_BIG_CUR] == 0u) return;  // (nobody reads the scan of such a level)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n) return;
  uint32_t f = 0u;
  if (D.ctr[C_BIG_CUR] != 0u) {
    const int first = (int)D.ctr[C_FIRST], end = (int)D.ctr[C_END];
    const int node = D.node_of[i];
    const int slot = node >= first && node < end ? D.bslot[node] : -1;
    if (slot >= 0) {
      const int k = (int)slots[(size_t)slot * kSlotWords + kSlotK];
      f = k > 0 && (int)D.flag[i] < k ? 1u : 0u;
    }
  }
  D.flag[i] = f;
}

// Large nodes: where every triangle goes (tmp_dst, -1: nowhere), what it is (tmp_id) and its new node (flag), and
// the centroid bounds of the large children, one reduction per wave and child.
__global__ void __launch_bounds__(256) k_sah_move_read(SahDev D, const uint32_t* __restrict__ slots,
                                                       uint32_t* __restrict__ next_slots) {
  if (D.ctr[C_BIG_CUR] == 0u) return;
  const int first = (int)D.ctr[C_FIRST], end = (int)D.ctr[C_END];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int node = i < D.n ? D.node_of[i] : -1;
  const int slot = node >= first && node < end ? D.bslot[node] : -1;
  const bool moves = slot >= 0 && (int)slots[(size_t)(slot < 0 ? 0 : slot) * kSlotWords + kSlotK] > 0;
  int cs = -1;
  f3 ce = mk3(0.0f);
  if (moves) {
    const int2 r = D.rng[node], kids = D.kid[node];
    const int nl = D.rng[kids.x].y - D.rng[kids.x].x;
    const int lrank = (int)(D.scan[i] - D.scan[r.x]);
    const bool left = D.flag[i] != 0u;
    const int id = D.ids[i];
    const int child = left ? kids.x : kids.y;
    D.tmp_id[i] = id;
    D.tmp_dst[i] = left ? r.x + lrank : r.x + nl + (i - r.x) - lrank;
    D.flag[i] = (uint32_t)child;
    cs = D.bslot[child];
    if (cs >= 0) ce = (xyz(D.blo[id]) + xyz(D.bhi[id])) * 0.5f;
  } else if (i < D.n) {
    D.tmp_dst[i] = -1;
  }
  unsigned long long todo = __ballot(cs >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int ls = __shfl(cs, leader, 64);
    const bool mine = cs == ls;
    const float r[6] = {wave_min(mine ? ce.x : INFINITY), wave_min(mine ? ce.y : INFINITY), wave_min(mine ? ce.z : INFINITY),
                        wave_max(mine ? ce.x : -INFINITY), wave_max(mine ? ce.y : -INFINITY), wave_max(mine ? ce.z : -INFINITY)};
    if (lane == leader) {
      uint32_t* S = next_slots + (size_t)ls * kSlotWords + kSlotCb;
      // (a bound only moves one way: a value an earlier read does not beat cannot beat the current one either)
      for (int k = 0; k < 3; k++)
        if (ord(r[k]) < __hip_atomic_load(&S[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&S[k], ord(r[k]));
      for (int k = 3; k < 6; k++)
        if (ord(r[k]) > __hip_atomic_load(&S[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&S[k], ord(r[k]));
    }
    todo &= ~__ballot(mine);
  }
}

__global__ void k_sah_move_write(SahDev D) {
  if (D.ctr[C_BIG_CUR] == 0u) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n) return;
  const int dst = D.tmp_dst[i];
  if (dst < 0) return;
  D.ids[dst] = D.tmp_id[i];
  D.node_of[dst] = (int32_t)D.flag[i];
}

__global__ void k_sah_ids(int32_t* __restrict__ ids, int32_t* __restrict__ node_of, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ids[i] = i;
  node_of[i] = 0;
}

template <typename T>
hipError_t alloc(T** p, size_t n) {
  return hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T));
}

size_t slot_cap_of(int n) { return (size_t)n / (kSmall + 1) + 1; }

}  // namespace

// The builder's scratch, made once per context (a rebuild allocates nothing): sah_work_bytes(n) in all, about
// 143 bytes per triangle (24 per position, 104 per triangle for its two binary nodes, 15 of bin slots), and the
// scan's few KB.
struct SahWork {
  int cap = 0;
  int32_t *ids = nullptr, *node_of = nullptr, *tmp_id = nullptr, *tmp_dst = nullptr, *bslot = nullptr;
  uint32_t *flag = nullptr, *scan = nullptr, *ctr = nullptr, *slots[2] = {nullptr, nullptr};
  int2 *rng = nullptr, *kid = nullptr;
  f4 *nlo = nullptr, *nhi = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  uint32_t* host = nullptr;  // pinned: the counters
};

size_t sah_work_bytes(int n) {
  const size_t N = (size_t)std::max(n, 1);
  return N * 6 * 4 + 2 * N * (8 + 8 + 16 + 16 + 4) + 2 * slot_cap_of(n) * kSlotWords * 4 + C_WORDS * 4;
}

void sah_work_free(SahWork* w) {
  if (!w) return;
  for (void* p : {(void*)w->ids, (void*)w->node_of, (void*)w->tmp_id, (void*)w->tmp_dst, (void*)w->bslot, (void*)w->flag,
                  (void*)w->scan, (void*)w->ctr, (void*)w->slots[0], (void*)w->slots[1], (void*)w->rng, (void*)w->kid,
                  (void*)w->nlo, (void*)w->nhi, w->tmp})
    if (p) hipFree(p);
  if (w->host) hipHostFree(w->host);
  delete w;
}

bool sah_work_create(SahWork** out, int n, hipStream_t s, std::string& err) {
  SahWork* w = new SahWork();
  const size_t N = (size_t)std::max(n, 1), SC = slot_cap_of(n) * kSlotWords;
  if (alloc(&w->ids, N) || alloc(&w->node_of, N) || alloc(&w->tmp_id, N) || alloc(&w->tmp_dst, N) || alloc(&w->flag, N) ||
      alloc(&w->scan, N) || alloc(&w->bslot, 2 * N) || alloc(&w->rng, 2 * N) || alloc(&w->kid, 2 * N) ||
      alloc(&w->nlo, 2 * N) || alloc(&w->nhi, 2 * N) || alloc(&w->slots[0], SC) || alloc(&w->slots[1], SC) ||
      alloc(&w->ctr, C_WORDS) || hipHostMalloc((void**)&w->host, C_WORDS * sizeof(uint32_t)) != hipSuccess) {
    err = "GPU SAH builder: device allocation failed";
    sah_work_free(w);
    return false;
  }
  hipcub::DeviceScan::ExclusiveSum(nullptr, w->tmp_bytes, w->flag, w->scan, n, s);
  if (hipMalloc(&w->tmp, std::max<size_t>(w->tmp_bytes, 1)) != hipSuccess) {
    err = "GPU SAH builder: scratch allocation failed";
    sah_work_free(w);
    return false;
  }
  w->cap = n;
  *out = w;
  return true;
}

bool gpu_build_bvh_sah(SahWork* sw, BvhWork* work, const f3* pos, int n, const TreeArrays& t, int* num_nodes,
                       int* max_stack, int* depth, bool* unsupported, hipStream_t s, std::string& err) {
  *unsupported = false;
  if (n < 3) { err = "GPU BVH builder needs at least 3 triangles"; return false; }
  if (!sw || !work || n > sw->cap) { err = "GPU SAH builder: no workspace for these triangles"; return false; }
  if (!gpu_prim_boxes_enqueue(work, pos, n, s, err)) return false;
  const BvhWorkView v = bvh_work_view(work);
  SahWork& w = *sw;
  SahDev D{n, 2 * n, (int)slot_cap_of(n), v.blo, v.bhi, w.ids, w.node_of, w.flag, w.scan, w.tmp_id, w.tmp_dst,
           w.rng, w.kid, w.nlo, w.nhi, w.bslot, w.ctr};
  const int B = 256, G = (n + B - 1) / B;
  hipLaunchKernelGGL(k_sah_ids, dim3(G), dim3(B), 0, s, w.ids, w.node_of, n);
  hipLaunchKernelGGL(k_sah_init, dim3(1), dim3(64), 0, s, D, v.cb, w.slots[0], nullptr);
  // Levels in batches with one read of the counters per batch. A level without large nodes has none below it:
  // from the batch after the read that shows it, only the small nodes' kernel runs.
  const int kBatch = 8;
  bool big = n > kSmall;
  for (int level = 0; level < kMaxDepth;) {
    for (int b = 0; b < kBatch && level < kMaxDepth; b++, level++) {
      uint32_t *cur = w.slots[level & 1], *next = w.slots[(level + 1) & 1];
      hipLaunchKernelGGL(k_sah_level, dim3(1), dim3(64), 0, s, w.ctr);
      // (at most min(2^level, n) nodes at a level; the waves stride over them)
      const long long cap_nodes = level < 30 ? std::min<long long>(1ll << level, n) : n;
      const int GS = (int)std::min<long long>((cap_nodes + 3) / 4, 4096);
      hipLaunchKernelGGL(k_sah_small, dim3(GS), dim3(B), 0, s, D, level);
      if (!big) continue;
      hipLaunchKernelGGL(k_sah_bin, dim3(G), dim3(B), 0, s, D, cur);
      const int GN = (int)std::min<long long>((cap_nodes + B - 1) / B, 1024);
      hipLaunchKernelGGL(k_sah_select, dim3(GN), dim3(B), 0, s, D, level, cur, next);
      hipLaunchKernelGGL(k_sah_flags, dim3(G), dim3(B), 0, s, D, cur);
      size_t tb = w.tmp_bytes;
      hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.flag, w.scan, n, s);
      hipLaunchKernelGGL(k_sah_move_read, dim3(G), dim3(B), 0, s, D, cur, next);
      hipLaunchKernelGGL(k_sah_move_write, dim3(G), dim3(B), 0, s, D);
    }
    hipMemcpyAsync(w.host, w.ctr, C_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) {
      err = "GPU SAH builder: kernel failure";
      return false;
    }
    if (w.host[C_FAIL]) {
      *unsupported = true;
      err = "GPU SAH builder: a node has no finite SAH candidate (coordinates too large); the host builder's median "
            "fallback is not implemented on the device";
      return false;
    }
    if (w.host[C_NODES] == w.host[C_END]) break;  // the last level made no node
    if (w.host[C_BIG_NEXT] == 0) big = false;
  }
  return gpu_collapse_marked(work, MarkedTree{w.kid, w.rng, w.nlo, w.nhi}, w.ids, pos, n, t, num_nodes, max_stack, depth,
                             s, err);
}

// The build in stream order: every level of the depth bound is launched, with the large nodes' kernels whenever the
// scene can have a large node at all. Each kernel reads its level's range and C_BIG_CUR from ctr, so a level past the
// last one, or one without large nodes, finds nothing. C_FAIL stays on the device: it gates the collapse and feeds
// the verdict (k_bvh.hip). A conditional build the device skipped (t.conditional, RebuildState::fail) starts without
// a root: every level is such a level.
bool gpu_build_bvh_sah_enqueue(SahWork* sw, BvhWork* work, const f3* pos, int n, const RebuildTarget& t, hipStream_t s,
                               std::string& err) {
  if (n < 3) { err = "GPU BVH builder needs at least 3 triangles"; return false; }
  if (!sw || !work || n > sw->cap) { err = "GPU SAH builder: no workspace for these triangles"; return false; }
  if (!gpu_rebuild_begin_enqueue(t.rs, t.conditional, s, err) || !gpu_prim_boxes_enqueue(work, pos, n, s, err)) return false;
  const BvhWorkView v = bvh_work_view(work);
  SahWork& w = *sw;
  SahDev D{n, 2 * n, (int)slot_cap_of(n), v.blo, v.bhi, w.ids, w.node_of, w.flag, w.scan, w.tmp_id, w.tmp_dst,
           w.rng, w.kid, w.nlo, w.nhi, w.bslot, w.ctr};
  const int B = 256, G = (n + B - 1) / B;
  hipLaunchKernelGGL(k_sah_ids, dim3(G), dim3(B), 0, s, w.ids, w.node_of, n);
  hipLaunchKernelGGL(k_sah_init, dim3(1), dim3(64), 0, s, D, v.cb, w.slots[0], t.conditional ? &t.rs->fail : nullptr);
  const bool big = n > kSmall;
  for (int level = 0; level < kMaxDepth; level++) {
    uint32_t *cur = w.slots[level & 1], *next = w.slots[(level + 1) & 1];
    hipLaunchKernelGGL(k_sah_level, dim3(1), dim3(64), 0, s, w.ctr);
    const long long cap_nodes = std::min<long long>(1ll << level, n);
    const int GS = (int)std::min<long long>((cap_nodes + 3) / 4, 4096);
    hipLaunchKernelGGL(k_sah_small, dim3(GS), dim3(B), 0, s, D, level);
    // (splits are uneven, so no level is known on the host to be free of large nodes: each of these leaves at once
    // on the device when C_BIG_CUR is 0)
    if (!big) continue;
    hipLaunchKernelGGL(k_sah_bin, dim3(G), dim3(B), 0, s, D, cur);
    const int GN = (int)std::min<long long>((cap_nodes + B - 1) / B, 1024);
    hipLaunchKernelGGL(k_sah_select, dim3(GN), dim3(B), 0, s, D, level, cur, next);
    hipLaunchKernelGGL(k_sah_flags, dim3(G), dim3(B), 0, s, D, cur);
    size_t tb = w.tmp_bytes;
    hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.flag, w.scan, n, s);
    hipLaunchKernelGGL(k_sah_move_read, dim3(G), dim3(B), 0, s, D, cur, next);
    hipLaunchKernelGGL(k_sah_move_write, dim3(G), dim3(B), 0, s, D);
  }
  if (hipGetLastError() != hipSuccess) { err = "GPU SAH builder: launch failure"; return false; }
  return gpu_collapse_marked_enqueue(work, MarkedTree{w.kid, w.rng, w.nlo, w.nhi}, w.ids, pos, n, kMaxDepth,
                                     w.ctr + C_FAIL, t, s, err);
}

}  // namespace fr
