// k_jfa.hip — JumpFlooding            FR/JumpFlooding.cpp:60-140, FR/shader/cpFS.glsl, FR/shader/jfFS.glsl
// JFA propagates the seed's texel centre (8 bytes per pixel) instead of two RGBA32F textures: the reference's
// coord/colour pair is a pure function of the seed pixel. The passes run only when the seed set differs from the
// previous launch's (a still camera and gaze leave it as it was); the colours are gathered every launch.
#include <hip/hip_runtime.h>
#include <cmath>
#include "fr_device.h"
#include "k_launch.h"
#include "k_image.h"

namespace fr {

// ------------------------------------------------------------------------------------------
// JumpFlooding. The state of a seeded pixel (alpha >= 1) is its current seed's coord texel (sx, sy) =
// ((x + 0.5) / W, (y + 0.5) / H) (cpFS.glsl: gl_FragCoord.st / screenSize) as two fp32 words with their
// (always clear) sign bits set, exactly the values the reference's coordTex holds; an unseeded pixel's
// .x is +inf (its .y its own sy). One 8-byte word per pixel replaces the reference's two RGBA32F textures
// per pass, and a candidate needs no table or texture gather. An unseeded or out-of-image candidate has
// an infinite distance, so no candidate needs a flag test (jfFS skips both: "a < 1" and outside [0, 1)).
// The alpha > 0 case of cpFS (.a in (0, 1)) only sets the current pixel's starting distance, which jfFS
// ignores while .a < 1: it needs no state. The seed's pixel is recovered exactly as floor(sx * W)
// (sx*W = x + 0.5 within 2^-8 for W < 2^15).
//
// Reuse. The state carries nothing of the colours, so the final state is a function of the seed set {p : alpha >= 1}
// and of W, H alone. k_jfa_init keeps that set as a bitmap (`seeds`: one 64-bit wave ballot per 64 consecutive
// pixels, zero bits past W H) and compares each word with the one the previous launch left. Every launch has a
// generation number (the host counts them); a launch that finds a word changed, or that the host forces, raises
// ctl[JFA_CTL_CHANGED] to its generation (an atomic max: nothing ever resets the word, so no block races with a reset).
// The passes of a launch whose generation is not in that word leave at once: the fixed buffer F still holds the final
// state of the last launch that changed the set, which is the state they would compute, bit for bit. For F to survive
// such a launch nothing but a pass that runs writes it: k_jfa_init writes G, the passes go G -> H -> G ..., and the
// last one writes F. The colours enter in the final kernels only, which run every launch and count the launches whose
// passes were skipped in ctl[JFA_CTL_SKIPPED]. The host never learns the outcome: it forces the first launch of a
// context, the one after fr_restore, and every launch when FOVRT_JFA_REUSE=0.
// ------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_jfa_init(const f4* __restrict__ in, u2* __restrict__ state,
                                                  unsigned long long* __restrict__ seeds, uint32_t* ctl, uint32_t gen,
                                                  int force, int W, int H, f2 screen) {
  // 32-bit pixel indices (fr_create keeps W H below 2^26): one 32-bit division per pixel, not a 64-bit one
  const uint32_t N = (uint32_t)W * (uint32_t)H;
  const uint32_t lane = threadIdx.x & 63u;
  // a wave always takes one whole bitmap word: 64 pixels from a multiple of 64 (the block is 4 waves and the stride
  // a multiple of 256), the last word's lanes past N with nothing to load or store and a zero bit
  int changed = 0;
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p - lane < N; p += gridDim.x * blockDim.x) {
    bool seed = false;
    if (p < N) {
      const float a = in[p].w;
      const uint32_t y = p / (uint32_t)W;
      const f2 uv = frag_uv(p - y * (uint32_t)W, y, screen);
      seed = a >= 1.0f;
      state[p] = seed ? u2{__float_as_uint(uv.x) | JFA_FLAG, __float_as_uint(uv.y) | JFA_FLAG}
                      : u2{JFA_UNSEEDED, __float_as_uint(uv.y)};
    }
    const unsigned long long bits = __ballot(seed);
    if (lane == 0) {
      const uint32_t w = p >> 6;
      changed |= seeds[w] != bits;
      seeds[w] = bits;
    }
  }
  // One atomic from a forced launch; else at most one per block that met a changed word, and none once the mark is
  // seen. (Measured and not kept: one per changed word, all on one address: 0.10 ms more for a 4K launch whose every
  // word changed, and the panning frame 1 % slower than without the bitmap; MEASUREMENTS.md.)
  if (force) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&ctl[JFA_CTL_CHANGED], gen);
  } else if (__syncthreads_or(changed) && threadIdx.x == 0 &&
             __atomic_load_n(&ctl[JFA_CTL_CHANGED], __ATOMIC_RELAXED) != gen) {
    atomicMax(&ctl[JFA_CTL_CHANGED], gen);
  }
}

// (sqrt_le_bound: fr_math.h.)

// One jfFS pass at `step` (FR/shader/jfFS.glsl:12-58). The reference walks the 8 neighbours in
// order and takes one when the pixel is not yet seeded or when distance() (sqrt of the fp32 sum of
// squares) is strictly smaller. That is: among the current seed (if seeded) and the valid neighbours
// in tap order, the first one whose sqrtf(d2) is minimal. sqrtf is monotone, so the minimum is
// sqrtf(min d2), and an element reaches it iff d2 <= sqrt_le_bound(sqrtf(min d2)): one sqrt per
// pixel and pass instead of one per improving candidate, same result bit for bit.
// A seeded state carries the sign bit on both words, so |s| - m = -(s + m) exactly (rounding is
// symmetric) and its d2 is (s.x + m.x)^2 + (s.y + m.y)^2 on the raw words, bit for bit; an unseeded or
// out-of-image candidate (.x = +inf) has d2 = +inf, never below a seeded one's.
typedef float jfa_v2 __attribute__((ext_vector_type(2)));
FR_DEV u2 jfa_pick(const u2 (&nb)[9], f2 me) {
  float d2[9];
  float dmin = INFINITY;
  const jfa_v2 m = {me.x, me.y};
#pragma unroll
  for (int i = 0; i < 9; i++) {
    // (dx, dy) and their squares as packed pairs (v_pk_add_f32 / v_pk_mul_f32: the same IEEE operations, two
    // per instruction; a pass is VALU-bound)
    const jfa_v2 c = {__uint_as_float(nb[i].x), __uint_as_float(nb[i].y)};
    const jfa_v2 dd = c + m;
    const jfa_v2 sq = dd * dd;
    d2[i] = sq.x + sq.y;
    dmin = fminf(dmin, d2[i]);
  }
  u2 r = nb[0];
  if (dmin != INFINITY) {  // (nothing seeded around: unchanged)
    const float bound = sqrt_le_bound(sqrtf(dmin));
#pragma unroll
    for (int i = 8; i >= 0; i--)
      if (d2[i] <= bound) r = nb[i];
  }
  return r;
}

// jfa_pick with the validity of the candidates' rows above and below (up: nb[1..3], down: nb[6..8]) known to
// be the same on every lane of the wave (k_jfa_step's rows are): an invalid row's three candidates are neither
// evaluated nor selected (they would be +inf: the result is jfa_pick's, bit for bit). At 4K the step-2048 pass
// has one valid row of three for 95 % of its pixels, the step-1024 pass two of three.
FR_DEV u2 jfa_pick_rows(const u2 (&nb)[9], f2 me, bool up, bool down) {
  float d2[9];
  float dmin = INFINITY;
  const jfa_v2 m = {me.x, me.y};
  auto dist = [&](int i) {
    const jfa_v2 c = {__uint_as_float(nb[i].x), __uint_as_float(nb[i].y)};
    const jfa_v2 dd = c + m;
    const jfa_v2 sq = dd * dd;
    d2[i] = sq.x + sq.y;
    dmin = fminf(dmin, d2[i]);
  };
  dist(0); dist(4); dist(5);
  if (up) { dist(1); dist(2); dist(3); }
  if (down) { dist(6); dist(7); dist(8); }
  u2 r = nb[0];
  if (dmin != INFINITY) {
    const float bound = sqrt_le_bound(sqrtf(dmin));
    if (down) {
      if (d2[8] <= bound) r = nb[8];
      if (d2[7] <= bound) r = nb[7];
      if (d2[6] <= bound) r = nb[6];
    }
    if (d2[5] <= bound) r = nb[5];
    if (d2[4] <= bound) r = nb[4];
    if (up) {
      if (d2[3] <= bound) r = nb[3];
      if (d2[2] <= bound) r = nb[2];
      if (d2[1] <= bound) r = nb[1];
    }
    if (d2[0] <= bound) r = nb[0];
  }
  return r;
}

// Rows outside the image are neither loaded nor evaluated (wave-uniform tests), in the passes of fewer than 4
// rows per thread only (the large steps, whose rows mostly fall outside). In the 4-row passes, where nearly every row
// is inside, the per-row branches kept the 18 loads from issuing together: steps 30 -> 36 us, the JFA stage 0.54 ->
// 0.64 ms; in the step-2048 pass 63 -> 48 us (r06l, profiles/r06_jfa/).

// A thread computes JFA_ROWS pixels of one column, `step` rows apart: pixel (x, y) reads rows
// y - step, y, y + step, so JFA_ROWS such pixels share their rows and read JFA_ROWS + 2 of them
// instead of 3 JFA_ROWS. A pass is bound by these re-reads (the 66 MB state at 4K is served from
// the Infinity Cache): 3 -> 1.5 row reads per pixel. Rows are grouped by residue: group g holds
// rows base + k step, base = (g / step) JFA_ROWS step + g % step. The pixel's own texel centre
// comes from a table (ftab: ((x + 0.5) / W) for x < W, then ((y + 0.5) / H), correctly rounded on
// the host) instead of two divisions.
// JFA_ROWS = min(4, ceil(H / step)): the large steps have fewer rows to share.
template <int JFA_ROWS>
__global__ __launch_bounds__(256) void k_jfa_step(const u2* __restrict__ src, u2* __restrict__ dst, int W, int H,
                                                  int step, const float* __restrict__ ftab, int xcd,
                                                  const uint32_t* __restrict__ ctl, uint32_t gen) {
  // the seed set is the previous launch's (k_jfa_init): F holds this launch's final state already. One scalar load
  // and a wave-uniform branch ahead of everything else.
  if (ctl[JFA_CTL_CHANGED] != gen) return;
  // xcd: the blocks of one XCD take one contiguous run of the row-major block order, so a block's left and
  // right taps (x -+ step, the neighbouring blocks for steps below 512) and its groups' shared rows are
  // mostly in the L2 that fetched them for its neighbours (round-robin order puts them on other XCDs)
  const uint32_t t = xcd ? xcd_tile(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y) : blockIdx.y * gridDim.x + blockIdx.x;
  const int x = (int)(t % gridDim.x) * 64 + (threadIdx.x & 63);
  // (g, hence base and every row's validity, is the same on all lanes of a wave)
  const int g = __builtin_amdgcn_readfirstlane((int)(t / gridDim.x) * 4 + (threadIdx.x >> 6));
  const int base = (g / step) * (JFA_ROWS * step) + g % step;
  if (x >= W || base >= H) return;
  const bool inl = x - step >= 0, inr = x + step < W;
  const int xl = inl ? x - step : x, xr = inr ? x + step : x;
  // rows base + (m - 1) step, m = 0 .. JFA_ROWS + 1: the states at x - step, x, x + step
  u2 L[JFA_ROWS + 2], C[JFA_ROWS + 2], R[JFA_ROWS + 2];
  bool in[JFA_ROWS + 2];
  // 32-bit byte offsets from the kernel-argument base (the 4K state is 66 MB): scalar-base loads
  const char* sb = reinterpret_cast<const char*>(src);
  auto ld = [&](uint32_t e) { return *reinterpret_cast<const u2*>(sb + e * 8u); };
#pragma unroll
  for (int m = 0; m < JFA_ROWS + 2; m++) {
    const int yr = base + (m - 1) * step;
    in[m] = yr >= 0 && yr < H;
    if (JFA_ROWS < 4 && !in[m]) {  // (wave-uniform)
      L[m] = C[m] = R[m] = u2{JFA_UNSEEDED, 0u};
      continue;
    }
    const uint32_t row = (uint32_t)(in[m] ? yr : base) * (uint32_t)W;
    L[m] = ld(row + (uint32_t)xl);
    C[m] = ld(row + (uint32_t)x);
    R[m] = ld(row + (uint32_t)xr);
    // taps outside the image are no candidates (jfFS skips them): an unseeded state in their place
    L[m].x = in[m] && inl ? L[m].x : JFA_UNSEEDED;
    C[m].x = in[m] ? C[m].x : JFA_UNSEEDED;
    R[m].x = in[m] && inr ? R[m].x : JFA_UNSEEDED;
  }
#pragma unroll
  for (int k = 0; k < JFA_ROWS; k++) {
    const int y = base + k * step;
    if (y < H) {
      // the current seed first, then the neighbours in jfFS order (-,-) (0,-) (+,-) (-,0) (+,0) (-,+) (0,+) (+,+)
      const u2 nb[9] = {C[k + 1], L[k], C[k], R[k], L[k + 1], R[k + 1], L[k + 2], C[k + 2], R[k + 2]};
      *reinterpret_cast<u2*>(reinterpret_cast<char*>(dst) + ((uint32_t)y * (uint32_t)W + (uint32_t)x) * 8u) =
          JFA_ROWS < 4 ? jfa_pick_rows(nb, mk2(ftab[x], ftab[W + y]), in[k], in[k + 2])
                       : jfa_pick(nb, mk2(ftab[x], ftab[W + y]));
    }
  }
}

int jfa_rows(int H, int step) { return std::min(4, (H + step - 1) / step); }
int jfa_row_groups(int H, int step) {
  // groups of jfa_rows rows `step` apart covering 0 .. H-1 (bands of jfa_rows * step rows)
  const int band = jfa_rows(H, step) * step;
  return ((H + band - 1) / band) * step;
}

// a launch whose passes were skipped, counted by one thread of its final kernel (fr_jfa_reuse_count)
FR_DEV void jfa_count_skipped(uint32_t* ctl, uint32_t gen) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && ctl[JFA_CTL_CHANGED] != gen)
    atomicAdd(&ctl[JFA_CTL_SKIPPED], 1u);
}

__global__ void k_jfa_final(const u2* __restrict__ state, const f4* __restrict__ in, f4* __restrict__ coord,
                            f4* __restrict__ color, int W, int H, f2 screen, uint32_t* ctl, uint32_t gen) {
  jfa_count_skipped(ctl, gen);
  const size_t N = (size_t)W * H;
  for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
    const u2 s = state[p];
    // (a pixel no seed reached keeps its own texel: cpFS's coord)
    const float sx = jfa_seeded(s.x) ? jfa_coord(s.x) : ((float)(p % (size_t)W) + 0.5f) / screen.x;
    const float sy = jfa_coord(s.y);
    const uint32_t ix = min((uint32_t)floorf(sx * screen.x), (uint32_t)W - 1);
    const uint32_t iy = min((uint32_t)floorf(sy * screen.y), (uint32_t)H - 1);
    const f4 c = in[(size_t)iy * W + ix];
    coord[p] = mk4(sx, sy, 0.0f, c.w);
    color[p] = c;
  }
}

// k_jfa_final for the Sibson run form: one wave per 64 columns of a row writes the JFA outputs and,
// from the colours it just gathered, the row's block prefix sums P and block totals T that
// k_sibson_prefix would compute (the same scan, the same sums), saving that kernel's re-read of the colour.
// OUT = false: JFA_COORD is not written here (Sibson reads the seeds from the state); the context writes it with
// k_jfa_coord only when something asks for it (133 MB of stores per 4K frame saved). JFA_COLOR is written: Sibson's
// border taps and seed fallbacks read it. (Computing those as in[seed pixel] instead made k_sibson_runs 0.66 -> 0.84 ms:
// each border tap then waits on a state load, a division and a dependent colour load.)
template <bool OUT>
__global__ __launch_bounds__(64) void k_jfa_final_prefix(const u2* __restrict__ state, const f4* __restrict__ in,
                                                         f4* __restrict__ coord, f4* __restrict__ color,
                                                         f4* __restrict__ P, f4* __restrict__ T, int W, int H, int NB,
                                                         f2 screen, uint32_t* ctl, uint32_t gen) {
  jfa_count_skipped(ctl, gen);
  const int lane = threadIdx.x;
  const int j = blockIdx.y, B = blockIdx.x;
  const int col = B * 64 + lane;
  f3 v = mk3(0.0f);
  if (col < W) {
    const size_t p = (size_t)j * W + col;
    const u2 s = state[p];
    // (a pixel no seed reached keeps its own texel: cpFS's coord)
    const float sx = jfa_seeded(s.x) ? jfa_coord(s.x) : ((float)col + 0.5f) / screen.x;
    const float sy = jfa_coord(s.y);
    const uint32_t ix = min((uint32_t)floorf(sx * screen.x), (uint32_t)W - 1);
    const uint32_t iy = min((uint32_t)floorf(sy * screen.y), (uint32_t)H - 1);
    const f4 c = in[(size_t)iy * W + ix];
    if (OUT) coord[p] = mk4(sx, sy, 0.0f, c.w);
    color[p] = c;
    v = xyz(c);
  }
  f3 incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float tx = __shfl_up(incl.x, o, 64), ty = __shfl_up(incl.y, o, 64), tz = __shfl_up(incl.z, o, 64);
    if (lane >= o) incl = incl + mk3(tx, ty, tz);
  }
  if (col <= W) P[(size_t)j * (W + 1) + col] = mk4(incl - v, 0.0f);
  if (lane == 63) T[(size_t)j * NB + B] = mk4(incl, 0.0f);
}

int jfa_max_step(int W, int H) {
  int m = 1;
  while (m * 2 < W || m * 2 < H) m *= 2;  // FR/JumpFlooding.cpp:33-34
  return m;
}

// st.F: the final state, of this launch or retained (see the head of this file); st.G, st.H: the passes' ping-pong.
const u2* launch_jfa(const f4* in, const JfaState& st, uint32_t gen, bool force, f4* coord, f4* color,
                     const float* ftab, int W, int H, f4* sibP, f4* sibT, bool outputs, int xcd, hipStream_t stream) {
  const size_t N = (size_t)W * H;
  int blocks = (int)std::min<size_t>((N + 255) / 256, 8192);
  f2 screen = mk2((float)W, (float)H);
  // (Measured and not kept: the first pass forming the seeds' states from the input's alpha itself, without
  // k_jfa_init: 138-154 us for that pass against 62 + 33 us for the pass and the init, its 16-byte texel
  // reads per tap doubling the pass's traffic.)
  hipLaunchKernelGGL(k_jfa_init, dim3(blocks), dim3(256), 0, stream, in, st.G, st.seeds, st.ctl, gen, force ? 1 : 0, W,
                     H, screen);
  u2* a = st.G;
  u2* b = st.H;
  // (Measured and not kept: steps 8, 4, 2, 1 fused in one launch over 64x32 tiles with a 15-texel halo in
  // LDS, 151 us against 4 x 31 us. A pass is VALU-bound, ~130 instructions per pixel, not HBM-bound, and the
  // halos add 29 % of pixel work.)
  for (int step = jfa_max_step(W, H); step >= 1; step /= 2) {
    dim3 grid((W + 63) / 64, (jfa_row_groups(H, step) + 3) / 4);
    auto k = jfa_rows(H, step) == 4 ? k_jfa_step<4> : jfa_rows(H, step) == 3 ? k_jfa_step<3>
           : jfa_rows(H, step) == 2 ? k_jfa_step<2> : k_jfa_step<1>;
    // the last pass writes F, whichever of G and H it reads
    hipLaunchKernelGGL(k, grid, dim3(256), 0, stream, a, step == 1 ? st.F : b, W, H, step, ftab, xcd, st.ctl, gen);
    std::swap(a, b);
  }
  if (sibP) {
    const int NB = sibson_prefix_blocks(W);
    hipLaunchKernelGGL(outputs ? k_jfa_final_prefix<true> : k_jfa_final_prefix<false>, dim3(NB, H), dim3(64), 0, stream,
                       st.F, in, coord, color, sibP, sibT, W, H, NB, screen, st.ctl, gen);
  } else {
    hipLaunchKernelGGL(k_jfa_final, dim3(blocks), dim3(256), 0, stream, st.F, in, coord, color, W, H, screen, st.ctl,
                       gen);
  }
  return st.F;  // the final state (k_sibson_runs reads its seeds from it)
}

// JFA_COORD of a JumpFlooding run whose final pass did not write it (launch_jfa, outputs = false): k_jfa_final's
// coord from the final state, with the seed colour's alpha from JFA_COLOR (which that pass wrote)
__global__ void k_jfa_coord(const u2* __restrict__ state, const f4* __restrict__ color, f4* __restrict__ coord, int W,
                            int H, f2 screen) {
  const size_t N = (size_t)W * H;
  for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
    const u2 s = state[p];
    const float sx = jfa_seeded(s.x) ? jfa_coord(s.x) : ((float)(p % (size_t)W) + 0.5f) / screen.x;
    coord[p] = mk4(sx, jfa_coord(s.y), 0.0f, color[p].w);
  }
}
void launch_jfa_coord(const u2* state, const f4* color, f4* coord, int W, int H, hipStream_t stream) {
  const size_t N = (size_t)W * H;
  hipLaunchKernelGGL(k_jfa_coord, dim3((unsigned)std::min<size_t>((N + 255) / 256, 8192)), dim3(256), 0, stream, state,
                     color, coord, W, H, mk2((float)W, (float)H));
}

}  // namespace fr
