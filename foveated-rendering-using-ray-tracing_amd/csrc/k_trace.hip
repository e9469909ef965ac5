// k_trace.hip — software ray tracing for gfx950: BVH traversal, the G-buffer trace (entry 0) and the
// foveated path-trace megakernel (entry 3) with the reference's three materials.
//
// Reference programs restated here:
//   g_buffer_trace            FR/cuda/g_buffer_trace_camera.cu:84-151
//   ray-0 closest hit         FR/cuda/g_diffuse.cu:67-144,   miss g_miss FR/cuda/gradientbg.cu:45-51
//   ray_trace                 FR/cuda/fov_path_trace_camera.cu:72-176
//   diffuse CH / shadow AH    FR/cuda/diffuse.cu:65-148, 226-241
//   reflection CH / AH        FR/cuda/reflection.cu:71-169, 239-253
//   refraction CH / AH        FR/cuda/refraction.cu:59-153
//   envmap_miss               FR/cuda/gradientbg.cu:57-66
//   mesh_intersect_refine     FR/cuda/triangle_mesh.cu:57-105 (+ intersection_refinement.h)
//
// MI355X design: no RT cores, so traversal is a wave64 software loop over a 4-wide BVH whose 128-B nodes
// carry the boxes of all four children (eight 16-B loads, two 64-B lines per visit) with a per-lane stack
// in LDS; triangles are pre-differenced (three 16-B loads). OptiX's recursive rtTrace is replaced by an explicit,
// output-equivalent work list: children whose results the parent never reads are not traced
// (diffuse/mirror parents read only child.reflectance, so grand-children and
// refraction sub-trees below them are dead work in the reference). Closest-hit ties resolve to the
// lowest primitive index and the transparent-shadow product is accumulated in f64, so results are
// independent of BVH shape and traversal order.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "fr_device.h"
#include "k_launch.h"

namespace fr {

#ifndef TRACE_BLOCK
#define TRACE_BLOCK 128  // 64 / 192 / 256 measured slower (256: 179.6 against 190.0 fps)
#endif
#define BVH_STACK FR_BVH_STACK
#define ITEM_STACK 24

// Diagnostic build (-DFR_STAMPS): wave-level cycle stamps (s_memtime) of the megakernel's phases,
// summed per wave and added to DevStats::pad (fr_stats.diag). Never part of a measured build.
#ifdef FR_STAMPS
FR_DEV uint64_t stamp() {
  uint64_t t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define STAMP(v) const uint64_t v = stamp()
#define STAMP_ADD(acc, v) acc += stamp() - v
#else
#define STAMP(v)
#define STAMP_ADD(acc, v)
#endif

struct Hit {
  float t, beta, gamma;
  int leaf, prim;
};

struct Stack {
  int32_t* base;  // LDS column of this lane: entries at base[k * TRACE_BLOCK]
};

FR_DEV void cswap(float& ka, int& va, float& kb, int& vb) {
  const bool s = kb < ka;
  const float tk = s ? kb : ka; kb = s ? ka : kb; ka = tk;
  const int tv = s ? vb : va; vb = s ? va : vb; va = tv;
}

// optix::intersect_triangle (branchless form) as triangle_mesh.ptx:361-430 computes it: the crosses
// unfused (n precomputed by the host), n.d / beta / gamma / t as the contracted dot, e2 = rcp(n.d) (p0 - o).
FR_DEV bool tri_test(const TriGeo& g, f3 o, f3 d, float tmin, float tmax, float& t, float& beta, float& gamma) {
  f3 p0 = mk3(g.a.x, g.a.y, g.a.z);
  f3 e0 = mk3(g.a.w, g.b.x, g.b.y);
  f3 e1 = mk3(g.b.z, g.b.w, g.c.x);
  f3 n = mk3(g.c.y, g.c.z, g.c.w);
  f3 e2 = (1.0f / dotc(n, d)) * (p0 - o);
  f3 i = cross(d, e2);
  beta = dotc(e1, i);
  gamma = dotc(e0, i);
  t = dotc(n, e2);
  return (t < tmax) & (t > tmin) & (beta >= 0.0f) & (gamma >= 0.0f) & (beta + gamma <= 1.0f);
}

// 1 / d, with +-2^100 for a component whose reciprocal overflows (d = +-0 or denormal). With inv = +-inf,
// lo inv - o inv is inf - inf = NaN for one plane and -inf for the other when lo < 0 < o (or the mirror
// case), and the slab test then culls a box the axis-parallel ray runs through; the finite stand-in
// keeps both planes' signs right (every product is exact: a power of two times a float).
FR_DEV float safe_rcp(float v) {
  const float r = 1.0f / v;
  return fabsf(r) == INFINITY ? copysignf(0x1p100f, r) : r;
}
FR_DEV f3 safe_inv(f3 d) { return mk3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z)); }

FR_DEV f3 shading_normal_of(const DevScene& sc, const TriShade& s, float beta, float gamma, f3 ng_normalized) {
  int flags = (int)fbits(s.t.w);
  if (!(flags & FR_SHADE_HAS_NORMALS)) return ng_normalized;
  f3 n0 = xyz(s.n0), n1 = xyz(s.n1), n2 = xyz(s.n2);
  // fma(w, n0, fma(b, n1, g n2)) (triangle_mesh.ptx:478-488)
  return normalizec(fma3(1.0f - beta - gamma, n0, fma3(beta, n1, gamma * n2)));
}

// The single traversal routine of the engine.
//   any_hit == false: closest hit in (tmin, tmax), ties -> lowest primitive index (rtTrace, ray types 0/1).
//   any_hit == true : shadow query (ray type 2): the first opaque hit returns 0 (diffuse.cu:226-231,
//                     reflection.cu:239-244); every refractive hit multiplies 1 - schlick(|n.d|, 5)
//                     (refraction.cu:144-153). The product is kept in f64 so it does not depend on
//                     the order in which the BVH delivers the hits.
// fresnel_schlick(c, 5, 0, 1) with the power rounded once: x^5 in f64 (x^2 is exact there, the two further products
// round at 2^-53), then to fp32. The platform's powf, which fresnel_schlick uses, is off by a last bit now and then,
// and 1 - schlick magnifies that bit where the power is near 1: on rays whose direction is not a unit vector the
// transmittance then misses the restatement (glibc's powf, which is this value) by up to 94 ulp. The masked queries,
// which are held to that restatement on such rays, take this form; the frame's shadow rays and the unmasked queries
// keep the one they have, instruction for instruction.
FR_DEV float schlick5_rounded_once(float cos_theta) {
  const double x = (double)fmaxf(0.0f, 1.0f - cos_theta);
  const double x2 = x * x;
  return fmaxf(0.0f, fminf(__builtin_fmaf(1.0f, (float)(x2 * x2 * x), 0.0f), 1.0f));
}

template <bool POW_ONCE = false>
FR_DEV void take_hit(const DevScene& sc, int j, const TriGeo& g, f3 d, bool any_hit, float t, float b, float gm,
                     Hit& best, double& atten, bool& done) {
  if (!any_hit) {
    // best.prim is loaded lazily (-2: not yet known): only an exact tie in t needs it here, and
    // trav_step resolves it when the query completes
    bool take = t < best.t;
    if (!take && t == best.t) {
      const int prim = sc.tri_prim[j];
      if (best.prim == -2) best.prim = sc.tri_prim[best.leaf];
      take = prim < best.prim;
      if (take) best.prim = prim;
    } else if (take) {
      best.prim = -2;
    }
    if (take) {
      best.t = t; best.beta = b; best.gamma = gm; best.leaf = j;
    }
  } else {
    const TriShade s = sc.shade[sc.tri_prim[j]];
    int flags = (int)fbits(s.t.w);
    if (sc.mats[flags & 0xff].type != MATL_REFRACTION) { atten = 0.0; done = true; return; }
    f3 ng = normalizec(mk3(g.c.y, g.c.z, g.c.w));
    // world_shading_normal = normalize(rtTransformNormal(.., shading_normal)) (refraction.cu:146): the
    // attribute normalised a second time (identity transform)
    f3 ns = normalizec(shading_normal_of(sc, s, b, gm, ng));
    float nDi = fabsf(dotc(ns, d));
    atten *= (double)(1.0f - (POW_ONCE ? schlick5_rounded_once(nDi) : fresnel_schlick(nDi, 5.0f, 0.0f, 1.0f)));
  }
}

// MASKED (ray queries with per-ray model masks): a candidate tri_test accepts is dropped when the bit of its
// triangle's model is clear in `mask`, before take_hit sees it, so an excluded model neither wins, ties, blocks nor
// attenuates; the primitive-map load is paid on accepted candidates only; a refractive crossing it keeps takes the
// power of its Schlick term rounded once (schlick5_rounded_once). The frame's kernels and the unmasked
// queries instantiate MASKED = false, which is the code without the arm.
template <bool MASKED = false>
FR_DEV void test_tri(const DevScene& sc, int j, const TriGeo& g, f3 o, f3 d, float tmin, float tmax, bool any_hit,
                     Hit& best, double& atten, bool& done, uint32_t mask = 0, const RayModels* rm = nullptr) {
  float t, b, gm;
  if (tri_test(g, o, d, tmin, tmax, t, b, gm)) {
    if (MASKED && !((mask >> ray_model_of(*rm, sc.tri_prim[j])) & 1u)) return;
    take_hit<MASKED>(sc, j, g, d, any_hit, t, b, gm, best, atten, done);
  }
}


// Slab tests of the four children of a node (SoA slabs, child k in component k): the entry distance of
// each child box, or +inf when the ray misses it within [tmin, tmax].
// A plane is t = lo * inv - o * inv, one fused op (6 % off the shading stage against (lo - o) * inv). The
// rounding differs from (lo - o) * inv by far less than the boxes' inflation (1e-5 + 4e-7 |v|), so culling
// stays conservative; an axis-parallel ray has inv = +-2^100 (safe_rcp), so its planes on that axis are
// huge values of the right signs: no constraint inside the slab, a miss outside.
// The near / far plane of each axis is picked by the ray's direction: for inv >= 0 the lo plane is the
// near one (lo <= hi, and fma is monotone), else the hi plane. So the loads fetch the near and far slabs
// directly (per-lane offsets 0 / 16 into the node's lo / hi pair), and a child costs one max3 and one min3
// instead of a min and a max per axis (megakernel 3.18 -> 3.07 ms at 4K bunny, 2.07 -> 1.94 ms at 4K
// vokselia). inv is never NaN or infinite, so the keys are those of the min / max form bit for bit (an
// empty slot, planes +-inf, is a miss here and a hit there; its count of -1 excludes it either way).
// The near / far slabs of a node for this ray's direction signs, and its child words (eight 16-B loads).
struct NodeSlabs {
  f4 nx, fx, ny, fy, nz, fz;
  int4 ch, ct;
};
FR_DEV NodeSlabs load_node(const DevScene& sc, int node, f3 inv) {
  const char* base = reinterpret_cast<const char*>(sc.nodes);
  const uint32_t off = (uint32_t)node * (uint32_t)sizeof(BvhNode);
  const uint32_t sx = (__float_as_uint(inv.x) >> 27) & 16u, sy = (__float_as_uint(inv.y) >> 27) & 16u,
                 sz = (__float_as_uint(inv.z) >> 27) & 16u;
  auto ld = [&](uint32_t o4) { return *reinterpret_cast<const f4*>(base + (size_t)(off + o4)); };
  NodeSlabs n;
  n.nx = ld(sx); n.fx = ld(sx ^ 16u); n.ny = ld(32u + sy); n.fy = ld(32u + (sy ^ 16u));
  n.nz = ld(64u + sz); n.fz = ld(64u + (sz ^ 16u));
  n.ch = *reinterpret_cast<const int4*>(base + (size_t)(off + 96u));
  n.ct = *reinterpret_cast<const int4*>(base + (size_t)(off + 112u));
  return n;
}
FR_DEV void slab4_keys(const NodeSlabs& N, f3 o, f3 inv, float tmin, float tmax, float key[4], int32_t child[4],
                       int32_t count[4]) {
  const f4 nx = N.nx, fx = N.fx, ny = N.ny, fy = N.fy, nz = N.nz, fz = N.fz;
  const int4 ch = N.ch, ct = N.ct;
  const float oix = -o.x * inv.x, oiy = -o.y * inv.y, oiz = -o.z * inv.z;
  // the 24 plane distances as packed pairs (children 0-1 and 2-3 of one slab: v_pk_fma_f32, the same IEEE fma
  // per element), 12 instructions instead of 24
  const v2f ix = v2s(inv.x), iy = v2s(inv.y), iz = v2s(inv.z), ox = v2s(oix), oy = v2s(oiy), oz = v2s(oiz);
  auto pl = [](float a, float b, v2f i, v2f oi) { return __builtin_elementwise_fma(v2(a, b), i, oi); };
  const v2f nx01 = pl(nx.x, nx.y, ix, ox), nx23 = pl(nx.z, nx.w, ix, ox), fx01 = pl(fx.x, fx.y, ix, ox),
            fx23 = pl(fx.z, fx.w, ix, ox);
  const v2f ny01 = pl(ny.x, ny.y, iy, oy), ny23 = pl(ny.z, ny.w, iy, oy), fy01 = pl(fy.x, fy.y, iy, oy),
            fy23 = pl(fy.z, fy.w, iy, oy);
  const v2f nz01 = pl(nz.x, nz.y, iz, oz), nz23 = pl(nz.z, nz.w, iz, oz), fz01 = pl(fz.x, fz.y, iz, oz),
            fz23 = pl(fz.z, fz.w, iz, oz);
  const float TN[3][4] = {{nx01.x, nx01.y, nx23.x, nx23.y}, {ny01.x, ny01.y, ny23.x, ny23.y},
                          {nz01.x, nz01.y, nz23.x, nz23.y}};
  const float TF[3][4] = {{fx01.x, fx01.y, fx23.x, fx23.y}, {fy01.x, fy01.y, fy23.x, fy23.y},
                          {fz01.x, fz01.y, fz23.x, fz23.y}};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float n = fmaxf(fmaxf(TN[0][k], TN[1][k]), fmaxf(TN[2][k], tmin));
    const float f = fminf(fminf(TF[0][k], TF[1][k]), fminf(TF[2][k], tmax));
    key[k] = n <= f ? n : INFINITY;
  }
  child[0] = ch.x; child[1] = ch.y; child[2] = ch.z; child[3] = ch.w;
  count[0] = ct.x; count[1] = ct.y; count[2] = ct.z; count[3] = ct.w;
}
FR_DEV void slab4_dir(const DevScene& sc, int node, f3 o, f3 inv, float tmin, float tmax, float key[4],
                      int32_t child[4], int32_t count[4]) {
  slab4_keys(load_node(sc, node, inv), o, inv, tmin, tmax, key, child, count);
}

// Does the ray reach any child box of the root (LDS copy)? When it does not, the query's traversal
// would end at its first node visit with nothing found: a miss, or attenuation 1 for a shadow ray.
// One child at a time (rolled loop), so that the test holds few registers in the shading pass; the
// planes are evaluated as slab4_dir does (min / max form: the same entry and exit distances), so a miss
// here is a miss of every child at the first node visit.
FR_DEV bool root_hit(const BvhNode& root, f3 o, f3 inv, float tmin, float tmax) {
  const float oix = -o.x * inv.x, oiy = -o.y * inv.y, oiz = -o.z * inv.z;
  const float* b = &root.lox.x;
  bool hit = false;
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    const float x0 = __builtin_fmaf(b[k], inv.x, oix), x1 = __builtin_fmaf(b[4 + k], inv.x, oix);
    const float y0 = __builtin_fmaf(b[8 + k], inv.y, oiy), y1 = __builtin_fmaf(b[12 + k], inv.y, oiy);
    const float z0 = __builtin_fmaf(b[16 + k], inv.z, oiz), z1 = __builtin_fmaf(b[20 + k], inv.z, oiz);
    const float n = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), tmin));
    const float f = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), tmax));
    hit |= n <= f;
  }
  return hit;
}

// Resumable traversal: the state of one query between node visits, so the megakernel can step
// all lanes' traversals together and shade the ones that finished (a lane never waits for the
// slowest traversal of its wave before it is refilled).
struct TravState {
  Hit best;
  double atten;  // any-hit product (f64: independent of the order the BVH delivers the hits)
  f3 inv;
  int node, sp;  // node to visit next (-1: none), stack depth
  int tlo, thi;  // triangles of the last visited node still to test (one pair per step)
};

FR_DEV void trav_begin(TravState& ts, f3 d, float tmax) {
  ts.atten = 1.0;
  ts.best.t = tmax; ts.best.leaf = -1; ts.best.prim = -1; ts.best.beta = 0; ts.best.gamma = 0;
  ts.inv = safe_inv(d);
  ts.node = 0;
  ts.sp = 0;
  ts.tlo = ts.thi = 0;
}

// Leaf-step form: a step visits a node only when the previous node's triangles are all tested, and
// tests at most one pair of triangles; the inner children are scheduled at the visit (culled by the
// best t known then, which is conservative). A lane with a long triangle span no longer holds its
// wave for several pair iterations while the other lanes wait.
FR_DEV void visit_loaded(const NodeSlabs& N, Stack st, TravState& ts, f3 o, float tmin) {
  {
    float key[4];
    int32_t child[4], count[4];
    slab4_keys(N, o, ts.inv, tmin, ts.best.t, key, child, count);
    int lo = 0x7FFFFFFF, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (key[k] != INFINITY && count[k] > 0) {
        lo = min(lo, child[k]);
        hi = max(hi, child[k] + count[k]);
      }
    }
    ts.tlo = lo;
    ts.thi = hi;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (count[k] != 0) key[k] = INFINITY;
    int c0 = child[0], c1 = child[1], c2 = child[2], c3 = child[3];
    float k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3];
    cswap(k0, c0, k1, c1);
    cswap(k2, c2, k3, c3);
    cswap(k0, c0, k2, c2);
    cswap(k1, c1, k3, c3);
    cswap(k1, c1, k2, c2);
    if (k0 != INFINITY) {
      const int nrem = (k1 != INFINITY) + (k2 != INFINITY) + (k3 != INFINITY);
      if (nrem) {
        const int base = min(min(c1, nrem > 1 ? c2 : c1), nrem > 2 ? c3 : c1);
        const uint32_t e = ((uint32_t)base << 8) | ((uint32_t)nrem << 6) | (uint32_t)(c1 - base) |
                           ((uint32_t)(c2 - base) & 3u) << 2 | ((uint32_t)(c3 - base) & 3u) << 4;
        st.base[ts.sp * TRACE_BLOCK] = (int32_t)e;
        ts.sp++;
      }
      ts.node = c0;
    } else if (ts.sp == 0) {
      ts.node = -1;
    } else {
      const uint32_t e = (uint32_t)st.base[(ts.sp - 1) * TRACE_BLOCK];
      ts.node = (int)(e >> 8) + (int)(e & 3u);
      const uint32_t n = (e >> 6) & 3u;
      if (n == 1) ts.sp--;
      else st.base[(ts.sp - 1) * TRACE_BLOCK] = (int32_t)((e & ~0xFFu) | ((n - 1) << 6) | ((e & 0x3Fu) >> 2));
    }
  }
}

FR_DEV void visit_node(const DevScene& sc, Stack st, TravState& ts, f3 o, float tmin) {
  visit_loaded(load_node(sc, ts.node, ts.inv), st, ts, o, tmin);
}

template <bool MASKED = false>
FR_DEV bool trav_step(const DevScene& sc, Stack st, TravState& ts, f3 o, f3 d, float tmin, float tmax, bool any_hit,
                      uint32_t mask = 0, const RayModels* rm = nullptr) {
  if (ts.tlo >= ts.thi) visit_node(sc, st, ts, o, tmin);
  if (ts.tlo < ts.thi) {
    const int j = ts.tlo;
    const bool two = j + 1 < ts.thi;
    const TriGeo g0 = sc.tri_geo[j];
    const TriGeo g1 = sc.tri_geo[two ? j + 1 : j];
    bool done = false;
    test_tri<MASKED>(sc, j, g0, o, d, tmin, tmax, any_hit, ts.best, ts.atten, done, mask, rm);
    if (done) return true;
    if (two) {
      test_tri<MASKED>(sc, j + 1, g1, o, d, tmin, tmax, any_hit, ts.best, ts.atten, done, mask, rm);
      if (done) return true;
    }
    ts.tlo = j + 2;
  }
  if (ts.tlo >= ts.thi && ts.node < 0) {
    if (ts.best.prim == -2) ts.best.prim = sc.tri_prim[ts.best.leaf];
    return true;
  }
  return false;
}

// Closed traversal (G-buffer): closest hit in (tmin, tmax), ties -> lowest primitive index
// (rtTrace, ray types 0/1); any_hit: the shadow query of ray type 2 (diffuse.cu:226-231,
// reflection.cu:239-244, refraction.cu:144-153).
FR_DEV void traverse(const DevScene& sc, Stack st, f3 o, f3 d, float tmin, float tmax, bool any_hit, Hit& best,
                     float& atten_out) {
  TravState ts;
  trav_begin(ts, d, tmax);
  while (!trav_step(sc, st, ts, o, d, tmin, tmax, any_hit)) {
  }
  best = ts.best;
  atten_out = (float)ts.atten;
}

// (float)b / 255.0f for a byte b, exactly: the reciprocal product corrected by one fma (checked for all 256
// values; tests/test_cpu_textures.py), 3 VALU instead of an IEEE division.
FR_DEV float unorm8(uint32_t b) {
  const float x = (float)b;
  const float inv = 1.0f / 255.0f;
  const float r = x * inv;
  return __builtin_fmaf(__builtin_fmaf(-r, 255.0f, x), inv, r);
}

// One texel of a packed texture, decoded to the RGBA32F value the host loader produced.
FR_DEV f4 tex_texel(uint32_t t, int kind) {
  if (kind == FR_TEX_UNORM8) return mk4(unorm8(t & 255u), unorm8((t >> 8) & 255u), unorm8((t >> 16) & 255u), unorm8(t >> 24));
  const uint32_t e = t >> 24;  // RGBE: m * 2^(e - 136), e = 0 black (load_hdr)
  const float f = e ? __builtin_amdgcn_ldexpf(1.0f, (int)e - 136) : 0.0f;
  return mk4((float)(t & 255u) * f, (float)((t >> 8) & 255u) * f, (float)((t >> 16) & 255u) * f, 1.0f);
}

FR_DEV f4 tex_sample(const DevTexture& t, float u, float v) {
  const int w = t.w;
  if (t.kind == FR_TEX_F32) {
    const f4* data = t.data;
    return bilinear_repeat([&](int x, int y) { return data[(size_t)y * w + x]; }, t.w, t.h, u, v);
  }
  const uint32_t* packed = t.packed;
  const int kind = t.kind;
  return bilinear_repeat([&](int x, int y) { return tex_texel(packed[(size_t)y * w + x], kind); }, t.w, t.h, u, v);
}

// The closest-hit programs' view of a hit. They read the intersection attributes through
// normalize(rtTransformNormal(RT_OBJECT_TO_WORLD, .)) (g_diffuse.cu:69-70, diffuse.cu:67-68,
// reflection.cu:73-74, refraction.cu:70): under the identity transform that is the attribute (itself a
// normalised vector, triangle_mesh.cu:70-79) normalised once more, which moves it by an ulp now and then;
// the PTX keeps both normalisations (FR/cuda/diffuse.ptx:160-180). refine_and_offset_hitpoint takes the
// attribute itself (triangle_mesh.cu:95-101).
struct SurfaceHit {
  f3 ng;        // world_geometric_normal
  f3 ns;        // world_shading_normal
  f3 front;     // front_hit_point
  f2 uv;        // texcoord.xy
  int mat;
};

FR_DEV SurfaceHit surface(const DevScene& sc, const Hit& h, f3 o, f3 d) {
  SurfaceHit s;
  const TriGeo g = sc.tri_geo[h.leaf];
  f3 n = mk3(g.c.y, g.c.z, g.c.w);
  const f3 ng_attr = normalizec(n);
  const TriShade sh = sc.shade[h.prim];
  int flags = (int)fbits(sh.t.w);
  s.mat = flags & 0xff;
  s.ng = normalizec(ng_attr);
  s.ns = (flags & FR_SHADE_HAS_NORMALS) ? normalizec(shading_normal_of(sc, sh, h.beta, h.gamma, ng_attr)) : s.ng;
  if (flags & FR_SHADE_HAS_UV) {  // fma(w, t0, fma(b, t1, g t2)) (triangle_mesh.ptx:508-521)
    const float w = 1.0f - h.beta - h.gamma;
    s.uv = mk2(__builtin_fmaf(w, sh.n0.w, __builtin_fmaf(h.beta, sh.n2.w, h.gamma * sh.t.y)),
               __builtin_fmaf(w, sh.n1.w, __builtin_fmaf(h.beta, sh.t.x, h.gamma * sh.t.z)));
  } else {
    s.uv = mk2(0.0f, 0.0f);
  }
  f3 back;
  refine_and_offset(fma3(h.t, d, o), d, ng_attr, mk3(g.a.x, g.a.y, g.a.z), back, s.front);
  return s;
}

FR_DEV f3 kd_of(const DevScene& sc, int mat, f2 uv) {
  const DevTexture& t = sc.texs[sc.mats[mat].tex];
  f4 c = tex_sample(t, uv.x / 1.0f, uv.y / 1.0f);  // Kd_map_scale = (1,1)
  return xyz(c);
}

// CUDA's atan2f / acosf / sinf (gradientbg.ptx:102-212)
FR_DEV f3 envmap_miss(const DevScene& sc, f3 d) {
  float theta = cuda_atan2f(d.x, d.z);
  float phi = kPi * 0.5f - cuda_acosf(d.y);
  float u = (theta + kPi) * (0.5f * k1_Pi);
  float v = 0.5f * (1.0f + cuda_sinf(phi));
  return xyz(tex_sample(sc.texs[sc.envmap], u, v)) * 2.0f;
}

// Ray-segment counters live in LDS (ds_add per event, one global atomic per block at exit), so they
// cost the megakernel no VGPRs.
enum CounterId { C_PRIMARY = 0, C_SHADOW, C_BOUNCE, C_MIRROR, C_REFR, C_REFL, C_TRUNC, C_OVERFLOW, C_COUNT };
struct Counters {
  uint32_t* lds;
  FR_DEV void inc(int k) const { atomicAdd(&lds[k], 1u); }
};

struct Item {
  f3 o, d, w;
  int depth;
  float importance;
};
// The refraction work items waiting on a lane (its explicit recursion stack), in
// a per-context device buffer, item k of every lane of the launch contiguous (k-major), 64 B per item,
// so a push or a pop moves one half cache line with three 16-B accesses. (Measured and not kept: a private
// array. The compiler puts it in scratch, where dword j of item k of the 64 lanes of a wave share one
// 256-B row, so one lane's push or pop touched 11 different cache lines (1,072 B of scratch per lane).)
struct ItemStack {
  f4* base;         // item 0 of this lane
  uint32_t stride;  // f4 between consecutive items of one lane (4 x the launch's lanes)
  FR_DEV void put(int k, const Item& x) const {
    f4* p = base + (size_t)k * stride;
    p[0] = mk4(x.o.x, x.o.y, x.o.z, x.d.x);
    p[1] = mk4(x.d.y, x.d.z, x.w.x, x.w.y);
    p[2] = mk4(x.w.z, __int_as_float(x.depth), x.importance, 0.0f);
  }
  FR_DEV Item get(int k) const {
    const f4* p = base + (size_t)k * stride;
    const f4 a = p[0], b = p[1], c = p[2];
    return Item{mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), mk3(b.z, b.w, c.x), __float_as_int(c.y), c.z};
  }
};

struct ItemState {  // what of the current work item stays live after its closest hit
  f3 w;
  int depth;
  float importance;
};

// Light sample geometry shared by the diffuse and reflection programs (diffuse.cu:94-103).
struct LightSample {
  float Ldist, nDl, LnDl;
  f3 L;
};
// light_position + v1 z1 + v2 z2 as fma(z2, v2, fma(z1, v1, light_position)) (diffuse.ptx:672-679)
FR_DEV LightSample light_sample(const DevScene& sc, f3 ff, f3 hp, float z1, float z2) {
  LightSample ls;
  const f3 light_pos = fma3(z2, sc.light_v2, fma3(z1, sc.light_v1, sc.light_position));
  ls.Ldist = lengthc(light_pos - hp);
  ls.L = normalizec(light_pos - hp);
  ls.nDl = dotc(ff, ls.L);
  ls.LnDl = dotc(sc.light_normal, ls.L);
  return ls;
}
FR_DEV float light_weight(const DevScene& sc, float nDl, float LnDl, float Ldist) {
  return nDl * LnDl * sc.light_area / (kPi * Ldist * Ldist);
}

enum Phase : int { PH_ITEM = 0, PH_PARENT_SHADOW = 1, PH_CHILD = 2, PH_CHILD_SHADOW = 3 };
enum Kind : int { K_DIFFUSE = 0, K_REFLECTION = 1 };

// A sample's radiance is the sum of its refraction-tree leaves' contributions (path_shade adds one
// step's contributions at a time). Two forms, chosen per frame size by the host (fx_below, k_shade_paths
// and k_shade_resolve agree on it; a function of W, H and spp only, so a tile-sharded rank and the
// one-GPU frame of the same view pick the same form and compose bit for bit):
//  - fp32 (large frames): the sample's lane sums them in the oracle's depth-first order and stores the
//    value (16-B record in samples);
//  - 32.32 fixed point (frames of fewer than SHADE_FX_FRAME pixel-samples W H spp per lane of the grid,
//    whose launches are small at the usual ~10 % density: 1080p at 4 spp): each step's fp32 sum is
//    rounded to fixed point and added as an integer. Integer sums do not depend on their order, so the
//    value is the same whichever lanes trace the tree's work items: the launch's tail hands pending items
//    to idle lanes of the same wave (k_shade_paths). The sample's lane stores its share (32-B record in
//    samples: x, y, z, flags); a lane that took over items adds its share to the slot's 32-B record in
//    help with no-return atomics, and the owner marks its record (FX_HELPED) so that k_shade_resolve adds
//    the help record and re-zeroes it. Non-finite contributions set flags (bits 0/1/2 NaN, 4/5/6 +inf,
//    8/9/10 -inf per component). A sum that leaves the int64 range (contributions near 2^30 each) sets
//    the flag of its sign instead of wrapping: radiance is never negative here, so any overflow of a
//    partial sum (the lane's own, the helpers' atomics, the owner + help total) is one of the true sum.
//    Contributions that large need a light power near 1e11 in these scenes; the fp32 form keeps them
//    finite, so the two forms differ only there.
#define FX_ONE 4294967296.0
#define FX_LIMIT 1073741824.0f  // |contribution| >= 2^30 counts as an overflow to +-inf
#define FX_NONFINITE 0xFFFu
#define FX_HELPED (1u << 16)    // the owner handed items to other lanes
#define FX_HELPER (1u << 17)    // this lane's share belongs to another lane's sample
#ifndef SHADE_FX_FRAME
#define SHADE_FX_FRAME 64       // W H spp per lane below which a frame uses the fixed-point form
#endif
struct SampleSum {
  long long v[3];  // fixed point, or the fp32 sums' bits in the low words
  uint32_t flags;
  FR_DEV void clear() { v[0] = v[1] = v[2] = 0; flags = 0; }
  FR_DEV f3 as_float() const {
    return mk3(__uint_as_float((uint32_t)v[0]), __uint_as_float((uint32_t)v[1]), __uint_as_float((uint32_t)v[2]));
  }
  FR_DEV void set_float(f3 x) {
    v[0] = __float_as_uint(x.x); v[1] = __float_as_uint(x.y); v[2] = __float_as_uint(x.z);
  }
  FR_DEV void add(f3 x) {
    const float c[3] = {x.x, x.y, x.z};
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (fabsf(c[k]) < FX_LIMIT) {
        const long long d = (long long)((double)c[k] * FX_ONE);
        if (__builtin_add_overflow(v[k], d, &v[k])) flags |= d > 0 ? 16u << k : 256u << k;
      } else {
        flags |= c[k] != c[k] ? 1u << k : (c[k] > 0.0f ? 16u << k : 256u << k);
      }
    }
  }
  FR_DEV void flush(f4* samples, unsigned long long* help, uint32_t slot, bool fx) const {
    if (!fx) {
      samples[slot] = mk4(as_float(), 0.0f);
      return;
    }
    if (!(flags & FX_HELPER)) {
      ulonglong2* r = reinterpret_cast<ulonglong2*>(samples) + (size_t)slot * 2;
      r[0] = make_ulonglong2((unsigned long long)v[0], (unsigned long long)v[1]);
      r[1] = make_ulonglong2((unsigned long long)v[2], (unsigned long long)(flags & (FX_NONFINITE | FX_HELPED)));
      return;
    }
    unsigned long long* rec = help + (size_t)slot * 4;
    uint32_t ovf = 0;
#pragma unroll
    for (int k = 0; k < 3; k++)
      if (v[k]) {
        const long long old = (long long)atomicAdd(rec + k, (unsigned long long)v[k]);
        long long sum;
        if (__builtin_add_overflow(old, v[k], &sum)) ovf |= v[k] > 0 ? 16u << k : 256u << k;
      }
    if ((flags & FX_NONFINITE) | ovf) atomicOr(rec + 3, (unsigned long long)((flags & FX_NONFINITE) | ovf));
  }
};
FR_DEV float fx_comp(long long v, unsigned long long fl, int k) {
  const bool nan = (fl >> k) & 1, pinf = (fl >> (4 + k)) & 1, ninf = (fl >> (8 + k)) & 1;
  if (nan || (pinf && ninf)) return __builtin_nanf("");
  if (pinf) return INFINITY;
  if (ninf) return -INFINITY;
  return (float)((double)v * (1.0 / FX_ONE));
}
// The value of sample slot `slot`; in the fixed-point form it re-zeroes the help record it read.
FR_DEV f3 sample_value(const f4* samples, unsigned long long* help, uint32_t slot, bool fx) {
  if (!fx) return xyz(samples[slot]);
  const ulonglong2* r = reinterpret_cast<const ulonglong2*>(samples) + (size_t)slot * 2;
  const ulonglong2 r0 = r[0], r1 = r[1];
  long long v0 = (long long)r0.x, v1 = (long long)r0.y, v2 = (long long)r1.x;
  unsigned long long fl = r1.y;
  if (fl & FX_HELPED) {
    ulonglong2* h = reinterpret_cast<ulonglong2*>(help + (size_t)slot * 4);
    const ulonglong2 h0 = h[0], h1 = h[1];
    const long long hv[3] = {(long long)h0.x, (long long)h0.y, (long long)h1.x};
    if (__builtin_add_overflow(v0, hv[0], &v0)) fl |= hv[0] > 0 ? 16u : 256u;
    if (__builtin_add_overflow(v1, hv[1], &v1)) fl |= hv[1] > 0 ? 32u : 512u;
    if (__builtin_add_overflow(v2, hv[2], &v2)) fl |= hv[2] > 0 ? 64u : 1024u;
    fl |= h1.y;
    h[0] = make_ulonglong2(0ull, 0ull);
    h[1] = make_ulonglong2(0ull, 0ull);
  }
  return mk3(fx_comp(v0, fl, 0), fx_comp(v1, fl, 1), fx_comp(v2, fl, 2));
}

// Per-lane state of one camera-sample path between two traversals.
struct PathState {
  int n;             // refraction work items on the stack
  ItemState it;      // current work item
  SampleSum total;   // this lane's share of the sample's radiance
  f3 qo, qd;         // pending query (also the current item's ray while phase == PH_ITEM)
  float qtmax;
  bool qany;
  int phase;
  bool diffuse_kind, want_child;
  f3 Kd, pres, cdir, front;
  float pm, nDl, LnDl, Ldist, phong;
  uint32_t cseed, seed;
};

FR_DEV void path_begin(PathState& ps, f3 o, f3 d, uint32_t seed, Counters cnt) {
  ps.n = 0;
  ps.it = ItemState{mk3(1.0f), 0, 1.0f};
  ps.total.clear();
  ps.qo = o; ps.qd = d; ps.qtmax = INFINITY; ps.qany = false;
  ps.phase = PH_ITEM;
  ps.diffuse_kind = true; ps.want_child = false;
  ps.Kd = ps.pres = ps.cdir = ps.front = mk3(0.0f);
  ps.pm = 1.0f; ps.nDl = ps.LnDl = ps.Ldist = 0.0f; ps.phong = -1.0f;
  ps.cseed = 0; ps.seed = seed;
  cnt.inc(C_PRIMARY);
}

// One camera sample of ray_trace (fov_path_trace_camera.cu:121-164): the value rtTrace leaves in
// prd.result for a type-1 ray. The reference recursion is executed as a state machine around ONE
// traversal call site; path_shade consumes the result of the pending query (closest hit h, or the
// any-hit attenuation), sets up the next query, and returns true once the sample's radiance
// (added to ps.total by path_shade) is complete:
//   PH_ITEM          closest hit of a work item (the camera ray or a refraction/reflection child of a
//                    refractive surface); refraction nodes push their children, other hits shade;
//   PH_PARENT_SHADOW the light sample of a diffuse / reflection surface;
//   PH_CHILD         the closest hit of its bounce (diffuse) or mirror (reflection) child, of which the
//                    parent reads only `.reflectance` (diffuse.cu:142, reflection.cu:144);
//   PH_CHILD_SHADOW  that child's light sample when it landed on a diffuse surface.
// Contributions are summed over the leaves of the refraction tree with their path weights, in the
// same depth-first order for every schedule, so a sample's value does not depend on which lane or
// when it is computed.
FR_DEV bool path_shade_step(const DevScene& sc, const FrameUniforms& U, PathState& ps, const ItemStack& items, Counters cnt,
                            const Hit& h, float atten, f3& total) {
  int& n = ps.n;
  ItemState& it = ps.it;
  f3& qo = ps.qo;
  f3& qd = ps.qd;
  float& qtmax = ps.qtmax;
  bool& qany = ps.qany;
  int& phase = ps.phase;
  bool& diffuse_kind = ps.diffuse_kind;
  bool& want_child = ps.want_child;
  f3& Kd = ps.Kd;
  f3& pres = ps.pres;
  f3& cdir = ps.cdir;
  f3& front = ps.front;
  float& pm = ps.pm;
  float& nDl = ps.nDl;
  float& LnDl = ps.LnDl;
  float& Ldist = ps.Ldist;
  float& phong = ps.phong;
  uint32_t& cseed = ps.cseed;
  const uint32_t seed = ps.seed;
  const f3 cutoff = mk3(0.34f, 0.55f, 0.85f);  // refraction material cutoff_color (FR/PathTracer.cpp:749)
  {
    bool pop = false;
    if (phase == PH_ITEM) {
      if (h.leaf < 0) {
        total += it.w * envmap_miss(sc, qd);
        pop = true;
      } else {
        SurfaceHit s = surface(sc, h, qo, qd);
        const int type = sc.mats[s.mat].type;
        Kd = kd_of(sc, s.mat, s.uv);
        if (type == MATL_REFRACTION) {  // refraction.cu:59-142; beer = exp(log(1) * t) = 1
          const f3 hp = fma3(h.t, qd, qo);  // refraction.ptx:279-281
          const f3 nrm = s.ns;
          const f3 i = qd;
          const f3 wk = it.w * Kd;
          float reflection = 1.0f;
          if (it.depth < U.refraction_max_depth) {
            // The last child pushed here would be popped right away, so it is continued from registers
            // and only an earlier sibling goes through the item stack (same depth-first order, and the
            // same ITEM_STACK accounting on the virtual depth n + pushed).
            int pushed = 0;
            Item child;
            f3 tdir;
            if (refract(tdir, i, nrm, 1.4f)) {
              float cos_theta = dotc(i, nrm);
              if (cos_theta < 0.0f) cos_theta = -cos_theta;
              else cos_theta = dotc(tdir, nrm);
              reflection = fresnel_schlick(cos_theta, 3.0f, 0.1f, 1.0f);
              float importance = it.importance * (1.0f - reflection) * luminance(mk3(1.0f));
              if (importance > 0.01f) {
                if (n < ITEM_STACK) { child = Item{hp, tdir, wk * ((1.0f - reflection) * mk3(1.0f)), it.depth + 1, importance}; pushed = 1; cnt.inc(C_REFR); }
                else cnt.inc(C_OVERFLOW);
              } else {
                total += wk * ((1.0f - reflection) * mk3(1.0f) * cutoff);
              }
            }
            f3 r = reflect(i, nrm);
            float importance = it.importance * reflection * luminance(mk3(1.0f));
            if (importance > 0.01f) {
              if (n + pushed < ITEM_STACK) {
                if (pushed) items.put(n++, child);
                child = Item{hp, r, wk * (reflection * mk3(1.0f)), it.depth + 1, importance};
                pushed = 1;
                cnt.inc(C_REFL);
              } else {
                cnt.inc(C_OVERFLOW);
              }
            } else {
              total += wk * (reflection * mk3(1.0f) * cutoff);
            }
            if (pushed) {
              it = ItemState{child.w, child.depth, child.importance};
              qo = child.o; qd = child.d; qtmax = INFINITY; qany = false;
              phase = PH_ITEM;
              return false;
            }
          } else {
            cnt.inc(C_TRUNC);
          }
          pop = true;
        } else {
          const f3 ff = faceforward_neg(s.ns, qd, s.ng);
          uint32_t sd = seed;
          const float z1 = rnd(sd);
          const float z2 = rnd(sd);
          front = s.front;
          LightSample ls = light_sample(sc, ff, front, z1, z2);
          nDl = ls.nDl; LnDl = ls.LnDl; Ldist = ls.Ldist;
          cseed = sd;
          diffuse_kind = type == MATL_DIFFUSE;
          if (diffuse_kind) {  // diffuse.cu:65-148
            pm = 1.0f;
            want_child = it.depth < U.diffuse_max_depth - 1;
            if (want_child) cdir = onb_inverse_transform(ff, cosine_sample_hemisphere(z1, z2));
          } else {  // reflection.cu:71-169
            f3 H = normalizec(ls.L - qd);
            float nDh = dotc(ff, H);
            phong = nDh > 0.0f ? fx_pow(nDh, 88.0f) : -1.0f;
            const float rn = 0.05f;  // reflectivity_n (FR/PathTracer.cpp:730)
            pm = fresnel_schlick(-dotc(ff, qd), 5.0f, rn, 1.0f);
            float importance = it.importance * luminance(mk3(pm));
            want_child = importance > 0.01f && it.depth < U.reflection_max_depth;
            if (want_child) cdir = reflect(qd, ff);
          }
          phase = PH_PARENT_SHADOW;
          if (nDl > 0.0f && LnDl > 0.0f) {
            cnt.inc(C_SHADOW);
            qo = front; qd = ls.L; qtmax = Ldist; qany = true;
            return false;
          }
          atten = 0.0f;  // no light sample: fall through
        }
      }
    }
    if (!pop && phase == PH_PARENT_SHADOW) {
      f3 S = mk3(0.0f);
      if (nDl > 0.0f && LnDl > 0.0f && atten > 0.0f) {
        const float weight = light_weight(sc, nDl, LnDl, Ldist);
        if (diffuse_kind) {
          S += sc.light_emission * weight * mk3(atten);
        } else {
          f3 Lc = sc.light_emission * weight * mk3(atten);
          S += Kd * nDl * Lc;  // fma(Kd nDl, Lc, 0) (reflection.ptx:386-391)
          if (phong >= 0.0f) S = fma3(Lc * mk3(1.0f), mk3(phong), S);  // Ks = (1,1,1), phong_exp = 88 (:558-561)
        }
      }
      pres = Kd * S;
      if (want_child) {
        cnt.inc(diffuse_kind ? C_BOUNCE : C_MIRROR);
        qo = front; qd = cdir; qtmax = INFINITY; qany = false;
        phase = PH_CHILD;
        return false;
      }
      total += it.w * pres;
      pop = true;
    } else if (!pop && phase == PH_CHILD) {
      bool lit = false;
      if (h.leaf >= 0) {
        SurfaceHit s = surface(sc, h, qo, qd);
        if (sc.mats[s.mat].type == MATL_DIFFUSE) {
          const f3 ff = faceforward_neg(s.ns, qd, s.ng);
          uint32_t sd = cseed;
          const float z1 = rnd(sd);
          const float z2 = rnd(sd);
          Kd = kd_of(sc, s.mat, s.uv);
          LightSample ls = light_sample(sc, ff, s.front, z1, z2);
          nDl = ls.nDl; LnDl = ls.LnDl; Ldist = ls.Ldist;
          if (nDl > 0.0f && LnDl > 0.0f) {
            cnt.inc(C_SHADOW);
            qo = s.front; qd = ls.L; qtmax = Ldist; qany = true;
            phase = PH_CHILD_SHADOW;
            lit = true;
          }
        }
      }
      if (lit) return false;
      total += it.w * (pres + mk3(pm) * mk3(0.0f));
      pop = true;
    } else if (!pop && phase == PH_CHILD_SHADOW) {
      f3 S = mk3(0.0f);
      if (atten > 0.0f) S += sc.light_emission * light_weight(sc, nDl, LnDl, Ldist) * mk3(atten);
      // the parent's result + child.reflectance (diffuse.ptx, pm = 1) / fma(r, child.reflectance, result)
      // (reflection.ptx:833-835)
      total += it.w * fma3(mk3(pm), Kd * S, pres);
      pop = true;
    }
    // next work item
    if (n == 0) return true;
    const Item nx = items.get(--n);
    it = ItemState{nx.w, nx.depth, nx.importance};
    qo = nx.o; qd = nx.d; qtmax = INFINITY; qany = false;
    phase = PH_ITEM;
    return false;
  }
}

// One shading step. fp32 form: the step adds to the running sum, in the order the oracle does.
// Fixed-point form: the step's contributions are summed in fp32 from zero, then added once.
FR_DEV bool path_shade(const DevScene& sc, const FrameUniforms& U, PathState& ps, const ItemStack& items, Counters cnt,
                       const Hit& h, float atten, bool fx) {
  f3 c = fx ? mk3(0.0f) : ps.total.as_float();
  const bool done = path_shade_step(sc, U, ps, items, cnt, h, atten, c);
  if (fx) ps.total.add(c);
  else ps.total.set_float(c);
  return done;
}

FR_DEV Hit trace_closest(const DevScene& sc, Stack st, f3 o, f3 d, float tmin, float tmax) {
  Hit h;
  float a;
  traverse(sc, st, o, d, tmin, tmax, false, h, a);
  return h;
}

FR_DEV void counters_begin(uint32_t* lds) {
  if (threadIdx.x < C_COUNT) lds[threadIdx.x] = 0;
  __syncthreads();
}
FR_DEV void counters_end(DevStats* stats, uint32_t* lds, bool gbuf) {
  __syncthreads();
  if (threadIdx.x < C_COUNT) {
    unsigned long long v = lds[threadIdx.x];
    if (v) {
      unsigned long long* dst;
      switch (threadIdx.x) {
        case C_PRIMARY: dst = gbuf ? &stats->gbuffer_primary : &stats->primary; break;
        case C_SHADOW: dst = &stats->shadow; break;
        case C_BOUNCE: dst = &stats->diffuse_bounce; break;
        case C_MIRROR: dst = &stats->mirror; break;
        case C_REFR: dst = &stats->refraction; break;
        case C_REFL: dst = &stats->reflection; break;
        case C_TRUNC: dst = &stats->truncated; break;
        default: dst = &stats->bvh_overflow; break;
      }
      atomicAdd(dst, v);
    }
  }
}

// Entry 0 traces one camera ray per pixel: the segment count is W * H, added once per launch (65K
// blocks each adding to one counter serialise on its L2 channel: ~0.5 ms at 4K).
FR_DEV void gbuffer_count(DevStats* stats, const FrameUniforms& U) {
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicAdd(&stats->gbuffer_primary, U.front_need ? (unsigned long long)U.front_pixels : (unsigned long long)U.width * U.height);
}

// The point (w, beta, gamma) of triangle k over the positions P (3 per triangle, scene order): fma(w, p0, fma(b, p1,
// g p2)), the form surface() gives the texture coordinates.
FR_DEV f3 tri_blend(const f3* __restrict__ P, int k, float w, float b, float g) {
  const f3* p = P + 3 * (size_t)k;
  return fma3(w, p[0], fma3(b, p[1], g * p[2]));
}

// The G-buffer outputs of one pixel's primary hit (g_diffuse.cu:67-144, g_miss gradientbg.cu:45-51).
// MOTION (fr_set_motion_reprojection, the first G-buffer after a position update): the reprojection starts from where
// the hit point was when the previous G-buffer traced its triangle (prev_pos: those positions; cur_pos: the ones this
// launch traces), and WEIGHT.z carries that point's distance from the previous eye for this frame's k_sampling. A
// triangle that did not move has delta = 0 exactly and gets the plain form's reprojection bits.
template <bool MOTION>
FR_DEV void gbuffer_store(const DevScene& sc, const FrameUniforms& U, bool on, int x, int y, f3 o, f3 d, const Hit& h,
                          f4* __restrict__ position, f4* __restrict__ normal, f4* __restrict__ depth,
                          f4* __restrict__ diffuse, f4* __restrict__ weight, uint8_t* __restrict__ gclass,
                          const f3* __restrict__ cur_pos, const f3* __restrict__ prev_pos) {
  const int W = U.width;
  if (on) {
    f3 origin = mk3(0.0f), nrm = mk3(0.0f), result = mk3(0.0f);
    float radiance = 0.0f, dv = 0.0f, prev_dist = 0.0f;
    f2 reproj = mk2(-1.0f, -1.0f);
    int cls = 3;  // primary-hit class for the class-major active list: 0 refr, 1 refl, 2 diffuse, 3 miss
    if (h.leaf >= 0) {
      SurfaceHit s = surface(sc, h, o, d);
      const int type = sc.mats[s.mat].type;
      cls = type == MATL_REFRACTION ? 0 : (type == MATL_REFLECTION ? 1 : 2);
      f3 ff = faceforward_neg(s.ns, d, s.ng);
      f3 hp = s.front;
      origin = hp;
      f3 Kd = kd_of(sc, s.mat, s.uv);
      result = mk3(0.0f) + mk3(1.0f) * Kd;
      nrm = s.ng;
      dv = lengthc(hp - U.eye);
      // compute_reprojection as g_diffuse.ptx:659-689: contracted rows, rcp(w) * row, fma(ndc, W, W) * 0.5
      f3 hp_prev = hp;
      if (MOTION) {
        const float w = 1.0f - h.beta - h.gamma;
        const f3 delta = tri_blend(prev_pos, h.prim, w, h.beta, h.gamma) - tri_blend(cur_pos, h.prim, w, h.beta, h.gamma);
        if (!(delta.x == 0.0f && delta.y == 0.0f && delta.z == 0.0f)) hp_prev = hp + delta;
        prev_dist = lengthc(hp_prev - U.prev_eye);
      }
      f4 p_cs = mul(U.prev_vp, mk4(hp_prev, 1.0f));
      const float iw = 1.0f / p_cs.w;
      reproj = mk2(__builtin_fmaf(p_cs.x * iw, U.screen.x, U.screen.x) * 0.5f,
                   __builtin_fmaf(p_cs.y * iw, U.screen.y, U.screen.y) * 0.5f);
      // shadow flag: light corner + v1 + v2 (g_diffuse.cu:115-143); the traced shadow ray's result is
      // never read (inShadow is never set), so only the two facing tests are observable.
      const f3 light_pos = sc.light_position + sc.light_v1 + sc.light_v2;
      const f3 L = normalizec(light_pos - hp);
      const float nDl = dotc(ff, L);
      const float LnDl = dotc(sc.light_normal, L);
      radiance = (nDl > 0.0f && LnDl > 0.0f) ? 1.0f : 0.0f;
    }
    size_t idx = (size_t)y * W + x;
    position[idx] = mk4(origin, 1.0f);
    normal[idx] = mk4(__builtin_fmaf(nrm.x, 0.5f, 0.5f), __builtin_fmaf(nrm.y, 0.5f, 0.5f),  // g_buffer_trace_camera.ptx:633-635
                      __builtin_fmaf(nrm.z, 0.5f, 0.5f), radiance);
    depth[idx] = mk4(dv, dv, dv, 1.0f);
    diffuse[idx] = mk4(result, 1.0f);
    weight[idx] = mk4(reproj.x, reproj.y, MOTION ? prev_dist : 0.0f, 1.0f);
    gclass[idx] = (uint8_t)cls;
  }
}

// ---------------------------------------------------------------------------------------------
// Entry 0: G-buffer. One lane per pixel, 8x8-pixel tiles per wave (coherent primary rays).
// ---------------------------------------------------------------------------------------------
// LOCAL: a tile-local front (U.front_need set; fr_set_front_local); the whole-screen instance carries none of it.
// MOTION: gbuffer_store's motion form (cur_pos / prev_pos: 18 more scattered dword loads on the hit lanes, no LDS); the
// plain instances read neither pointer.
template <bool LOCAL, bool MOTION>
__global__ __launch_bounds__(TRACE_BLOCK) void k_gbuffer(DevScene sc, FrameUniforms U, f4* __restrict__ position,
                                                         f4* __restrict__ normal, f4* __restrict__ depth,
                                                         f4* __restrict__ diffuse, f4* __restrict__ weight,
                                                         uint8_t* __restrict__ gclass, DevStats* stats,
                                                         const f3* __restrict__ cur_pos,
                                                         const f3* __restrict__ prev_pos) {
  __shared__ int32_t lds_stack[BVH_STACK * TRACE_BLOCK];
  Stack st{&lds_stack[threadIdx.x]};
  const int W = U.width, H = U.height;
  gbuffer_count(stats, U);
  const int tiles_x = (W + 7) >> 3;
  const int wave = (blockIdx.x * TRACE_BLOCK + threadIdx.x) >> 6;
  // a tile-local front: only the tiles this rank's sampling reads (wave = its 8x8 tile's index)
  if (LOCAL && wave < tiles_x * ((H + 7) >> 3) && !U.front_need[wave] && wave != gaze_tile8(U)) return;
  const int lane = threadIdx.x & 63;
  const int x = (wave % tiles_x) * 8 + (lane & 7);
  const int y = (wave / tiles_x) * 8 + (lane >> 3);
  const bool on = x < W && y < H;
  // camera ray (g_buffer_trace_camera.cu:95-100), traversed node by node in a wave-uniform loop
  // fma(x / W, 2, -1), the contracted rows, rcp(w) * row, normalize (g_buffer_trace_camera.ptx:507-566)
  const f2 screenf = U.screen;
  f4 tmp = mk4(__builtin_fmaf((float)x / screenf.x, 2.0f, -1.0f), __builtin_fmaf((float)y / screenf.y, 2.0f, -1.0f),
               -1.0f, 1.0f);
  tmp = mul(U.inv_vp, tmp);
  const f3 nearPos = div_rcp(xyz(tmp), tmp.w);
  const f3 o = U.eye;
  const f3 d = normalizec(nearPos - U.eye);
  TravState ts;
  trav_begin(ts, d, INFINITY);
  bool tracing = on;
  while (__ballot(tracing)) {
    if (tracing && trav_step(sc, st, ts, o, d, sc.scene_epsilon, INFINITY, false)) tracing = false;
  }
  gbuffer_store<MOTION>(sc, U, on, x, y, o, d, ts.best, position, normal, depth, diffuse, weight, gclass, cur_pos,
                        prev_pos);
}

// ---------------------------------------------------------------------------------------------
// Entry 3: foveated shading over the compacted active list (fov_path_trace_camera.cu:96-186).
//
// The work unit is one camera sample: slot = k * spp + j is sample j of active pixel k, and j maps
// to the reference's loop counter s = spp - j (its do{}while(--samples_per_pixel) order). Sample
// paths differ wildly in length (a miss ends after one traversal, a GI path through the glass
// bunny runs dozens), so a lane that finishes takes the next slot instead of idling until its
// wave's longest path ends: k_shade_paths is persistent, every wave keeps a wave-local queue of
// 64 slots and refills it from chunk counters sharded by XCD (chunk g = j * 8 + shard, one counter
// per 128-byte line, blockIdx & 7 = the XCD the block runs on; an exhausted shard steals from the
// next). Each finished sample is written to samples[slot]; k_shade_resolve then reduces a pixel's
// samples in the reference's order ((0 + r_spp) + r_spp-1) + ..., tone-maps and updates the
// temporal history. A sample's value does not depend on the lane or time it ran, so the result is
// the same for every schedule.
// ---------------------------------------------------------------------------------------------
#define SHADE_SHARDS 8
#define SHADE_SHARD_STRIDE 32  // uint32 words between shard counters (128 B)
#define SHADE_REFR_CTR 16      // word 16 of a shard's line: k_shade_resolve zeroes it with the chunk counter; nothing claims from it
// (Measured and not kept: the refraction class of a large launch claimed slot by slot from that counter. It removed the
// late starts the sample trace showed, but the pipelined 4K frame got no faster: 237.2 against 242.8 fps over five
// interleaved runs each, and two modes, 229-247 fps, instead of one.)

#ifndef SHADE_CHUNK
#define SHADE_CHUNK 64
#endif


FR_DEV f4 history_of(const FrameUniforms& U, const f4* __restrict__ weight, const f4* __restrict__ history_cache,
                     uint32_t p) {
  f4 cw = weight[p];
  f4 c = mk4(0, 0, 0, 0);
  if (cw.z > 0.0f) {
    uint32_t qx = f2u_sat(fr_round(cw.x)), qy = f2u_sat(fr_round(cw.y));
    c = history_cache[(size_t)qy * U.width + qx];
  }
  return c;
}

// Per active pixel, the sample-independent part of ray_trace's camera ray (fov_path_trace_camera.cu:
// 110-136): the seed is re-derived for every sample from (pixel, frame), so all spp samples of a pixel
// draw the same r1, r2 and continue from the same seed. k_sample_setup evaluates
// it once per pixel (tea16, the history gather, the two draws, the NDC pixel position) instead of once
// per sample inside the megakernel's refill.
// hvalid (the early form, ctx_frame.cpp frame_half): instead of history_cache's .w, the bit k_carry_history of the
// previous frame computed for it (.w > 0 of the history that frame wrote, which is this frame's history_cache), so the
// setup needs neither that frame's k_shade_resolve nor the history buffer: it runs with the frame's front stages.
__global__ void k_sample_setup(FrameUniforms U, const uint32_t* __restrict__ active, const uint32_t* __restrict__ ray_count,
                               const f4* __restrict__ weight, const f4* __restrict__ history_cache,
                               const unsigned long long* __restrict__ hvalid, f4* __restrict__ aux,
                               uint32_t* __restrict__ aux_seed) {
  const uint32_t count = *ray_count;
  const int W = U.width;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
    const uint32_t p = active[k];
    const uint32_t px = p % W, py = p / W;
    bool valid;
    if (hvalid) {  // history_of's source pixel, its validity bit
      const f4 cw = weight[p];
      valid = false;
      if (cw.z > 0.0f) {
        const uint32_t q = f2u_sat(fr_round(cw.y)) * (uint32_t)W + f2u_sat(fr_round(cw.x));
        valid = (hvalid[q >> 6] >> (q & 63u)) & 1ull;
      }
    } else {
      valid = history_of(U, weight, history_cache, p).w > 0.0f;
    }
    uint32_t seed = tea16((uint32_t)W * py + px, valid ? U.frame : 0u);
    const f2 pixel = mk2(__builtin_fmaf((float)px / U.screen.x, 2.0f, -1.0f),  // fov_path_trace_camera.ptx:509-512
                         __builtin_fmaf((float)py / U.screen.y, 2.0f, -1.0f));
    const float r1 = rnd(seed);
    const float r2 = rnd(seed);
    aux[k] = mk4(pixel.x, pixel.y, r1, r2);
    aux_seed[k] = seed;
  }
}

// Camera ray of sample slot (fov_path_trace_camera.cu:110-136): jitter and direction from the pixel's
// k_sample_setup values.
FR_DEV void path_init(const FrameUniforms& U, const f4 a, const uint32_t seed, uint32_t slot, PathState& ps,
                      Counters cnt) {
  const int spp = U.spp;
  const int sq = U.sqrt_spp;
  // fr_create admits spp 1, 2, 4, 8 only (sqrt_spp 1, 1, 2, 2): shifts and masks, no integer division
  const uint32_t k = slot >> __builtin_ctz((uint32_t)spp);
  const int s = spp - (int)(slot - k * (uint32_t)spp);
  const f2 pixel = mk2(a.x, a.y);
  const f2 jitter_scale = mk2(1.0f / U.screen.x / (float)sq, 1.0f / U.screen.y / (float)sq);
  const uint32_t jx = (uint32_t)s & (uint32_t)(sq - 1);
  const uint32_t jy = (uint32_t)s >> __builtin_ctz((uint32_t)sq);
  const float r1 = a.z, r2 = a.w;
  // pixel + jitter * jitter_scale as fma (fov_path_trace_camera.ptx:525-528), then as entry 0's ray
  f2 jitter = mk2((float)jx - r1, (float)jy - r2);
  f2 dd = mk2(__builtin_fmaf(jitter.x, jitter_scale.x, pixel.x), __builtin_fmaf(jitter.y, jitter_scale.y, pixel.y));
  f4 tmp = mul(U.inv_vp, mk4(dd.x, dd.y, -1.0f, 1.0f));
  f3 nearPos = div_rcp(xyz(tmp), tmp.w);
  f3 dir = normalizec(nearPos - U.eye);
  path_begin(ps, U.eye, dir, seed, cnt);
}

FR_DEV uint32_t lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Index of the r-th set bit (r < popcount(m)) of m: binary search on the popcounts of the low halves.
FR_DEV uint32_t nth_set_bit(unsigned long long m, uint32_t r) {
  uint32_t pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const uint32_t c = (uint32_t)__popcll(m & ((1ull << w) - 1ull));
    if (r >= c) { r -= c; m >>= w; pos += w; }
  }
  return pos;
}

enum LaneState : int { L_IDLE = 0, L_TRAV = 1, L_READY = 2 };

// Diagnostic build: every query the megakernel issues is appended to g_rec (o|tmax, d|any), the
// input of the standalone traversal probe (fr_diag_trace_queries).
#ifdef FR_STAMPS
__device__ f4* g_rec = nullptr;
__device__ uint32_t g_rec_n = 0;
__device__ uint32_t g_rec_cap = 0;
FR_DEV void record_query(f3 o, f3 d, float tmax, bool any) {
  if (!g_rec) return;
  const uint32_t i = atomicAdd(&g_rec_n, 1u);
  if (i < g_rec_cap) {
    g_rec[2 * (size_t)i] = mk4(o, tmax);
    g_rec[2 * (size_t)i + 1] = mk4(d, any ? 1.0f : 0.0f);
  }
}
#define RECORD_QUERY(ps) record_query(ps.qo, ps.qd, ps.qtmax, ps.qany)
#else
#define RECORD_QUERY(ps)
#endif

// Diagnostic build: per sample slot (queries, traversal steps, start, end) and per wave (start, the
// moment its refill found no fresh work, end, samples), times from s_memrealtime (100 MHz, low 32
// bits): the critical path of the megakernel (fr_diag_sample_trace, scripts/sample_trace.py).
#ifdef FR_STAMPS
__device__ uint32_t* g_srec = nullptr;
__device__ uint32_t g_srec_cap = 0;
__device__ uint32_t* g_wrec = nullptr;
__device__ uint32_t g_wrec_cap = 0;
FR_DEV uint32_t rtime() { return (uint32_t)__builtin_amdgcn_s_memrealtime(); }
#define DIAG(x) x
#else
#define DIAG(x)
#endif

#ifndef TRAV_UNROLL
// traversal steps per wave-wide ballot (round 2: 1 / 2 / 3 / 4 gave 182.2 / 186.6 / 189.7 / 189.1 fps; round 5, on
// the PTX-faithful code, six interleaved pairs: 2 against 3, 4,448 against 4,421 Mrays/s, megakernel serialised
// 3.105 against 3.140 ms; 4: 4,391; profiles/r05_mkab/tu_*)
#define TRAV_UNROLL 2
#endif
#ifndef SHADE_FIRST_STEP
// Every new query is first tested against the root's child boxes (LDS copy) in the shading pass:
// about half of the queries (shadow rays that clear the scene, rays that leave it) end there, and
// their lanes shade again before the next traversal loop instead of spending a whole loop (run until
// its slowest lane is done) on one node visit. The traversal itself is unchanged.
#define SHADE_FIRST_STEP 1
#endif
#ifndef SHADE_WAVES
#define SHADE_WAVES 3  // waves per SIMD the register allocation must allow (3: 168 VGPRs; measured best of 2-5)
#endif
#ifndef SHADE_EXIT_T
// Early exit from the traversal loop: once at most SHADE_EXIT_T lanes still traverse (after SHADE_EXIT_S passes) and
// some lane is answered, the answered lanes shade and refill while the rest keep their traversal state for the next
// loop. Only in launches of the sample-sum form whose refraction class (primary hits on glass) is at least
// 1 / SHADE_EXIT_REFR of the samples: there a few lanes deep inside a glass tree hold the wave's other lanes for
// dozens of steps. Measured (round 6, interleaved bench pairs, profiles/r06_trav_exit_*): 4K bunny (8.1 % refraction)
// +0.9 to +2.6 % fps, megakernel serialised 3.14 -> 3.03 ms; without the gate 4K vokselia GI 3 (2.5 %) -5 % and 1080p
// bunny (fixed-point form) -4 %, where the extra shading passes cost more than the idle lanes. T = 4 .. 12 measured
// alike on the 4K bunny, 16 neutral, 32 worse; a minimum pass count (16 / 32 / 64) did not separate the workloads.
#define SHADE_EXIT_T 8
#endif
#ifndef SHADE_EXIT_S
#define SHADE_EXIT_S 0
#endif
#ifndef SHADE_EXIT_REFR
#define SHADE_EXIT_REFR 20
#endif
__global__ __launch_bounds__(TRACE_BLOCK) __attribute__((amdgpu_waves_per_eu(SHADE_WAVES, SHADE_WAVES))) void k_shade_paths(DevScene sc, FrameUniforms U,
                                                             const uint32_t* __restrict__ active,
                                                             const uint32_t* __restrict__ ray_count,
                                                             const f4* __restrict__ weight,
                                                             const f4* __restrict__ history_cache,
                                                             uint32_t* __restrict__ chunk_ctr,
                                                             f4* __restrict__ samples, DevStats* stats,
                                                             const f4* __restrict__ aux,
                                                             const uint32_t* __restrict__ aux_seed,
                                                             uint32_t chunk_refr_fixed, uint32_t xcd_bands,
                                                             unsigned long long* __restrict__ help, uint32_t fx_below,
                                                             f4* __restrict__ item_store) {
  __shared__ int32_t lds_stack[BVH_STACK * TRACE_BLOCK];
  __shared__ uint32_t lds_cnt[C_COUNT];
  __shared__ BvhNode lds_root;
  Stack st{&lds_stack[threadIdx.x]};
  if (threadIdx.x < 32) reinterpret_cast<float*>(&lds_root)[threadIdx.x] = reinterpret_cast<const float*>(sc.nodes)[threadIdx.x];
  counters_begin(lds_cnt);
  Counters cnt{lds_cnt};
  const ItemStack items{item_store + (size_t)(blockIdx.x * TRACE_BLOCK + threadIdx.x) * 4, gridDim.x * TRACE_BLOCK * 4u};
  const uint32_t spp_shift = __builtin_ctz((uint32_t)U.spp);
  const uint32_t total = ray_count[0] * (uint32_t)U.spp;
  // The refraction class (the head of the class-major list: the long sample trees through the glass)
  // is handed out in chunks of chunk_refr, the rest in chunks of SHADE_CHUNK. A launch of fewer than
  // 8 samples per lane (1080p) ends with its longest trees: smaller chunks then spread that class over
  // all waves, so its trees start at once instead of waiting behind their wave's busy lanes (64-slot
  // chunks: the last ones started up to 2 ms late). A larger launch keeps whole 64-slot chunks: the
  // long trees stay in few waves and the others retire early, which leaves the CUs to the frame's
  // other kernels (spreading there: 4K bunny 207 -> 193 fps, 4K vokselia 8 spp 178 -> 170 fps). Below one
  // sample per lane (a tile-sharded rank with a few tiles) the chunks are the smallest, 8 slots: with 64,
  // one wave took a foveal tile's refraction trees alone (2.3 ms for 14.7 K pixels).
  const uint32_t nrefr = min(ray_count[1] * (uint32_t)U.spp, total);
  // the fixed-point form and its tail handoff (SampleSum): launches below fx_below samples
  const bool fx = total < fx_below;
  const uint32_t lanes = gridDim.x * TRACE_BLOCK;
  const uint32_t chunk_refr = chunk_refr_fixed ? chunk_refr_fixed
                              : total < 8 * lanes
                                  ? min(max(nrefr / (lanes / 64), 8u), (uint32_t)SHADE_CHUNK) & ~((uint32_t)U.spp - 1u)
                                  : SHADE_CHUNK;
  const uint32_t nsmall = (nrefr + chunk_refr - 1) / chunk_refr;
  const uint32_t nchunks = nsmall + (total - nrefr + SHADE_CHUNK - 1) / SHADE_CHUNK;
  // xcd_bands (the default): class c's slots [cb[c], cb[c + 1]); shard (XCD) s takes the s-th eighth of
  // every class, classes in list order: an XCD's rays come from one band of each class's tile-ordered
  // range (coherent geometry in its L2), and every XCD starts with its share of the refraction class.
  // Else chunk g goes to shard g % 8 (interleaved).
  uint32_t cb[5];
  cb[0] = 0; cb[4] = total;
#pragma unroll
  for (int c = 1; c < 4; c++) cb[c] = min(ray_count[c] * (uint32_t)U.spp, total);
  cb[1] = nrefr;
  auto part = [&](int c, uint32_t s) {  // start of shard s's part of class c (a multiple of spp)
    const uint32_t len = (cb[c + 1] - cb[c]) >> spp_shift;
    return cb[c] + (uint32_t)(((uint64_t)len * s / SHADE_SHARDS) << spp_shift);
  };
  const uint32_t lane = threadIdx.x & 63;
  const float tmin = sc.scene_epsilon;
  const bool exit_early = SHADE_EXIT_T > 0 && (SHADE_EXIT_REFR == 0 || (!fx && (uint64_t)nrefr * SHADE_EXIT_REFR >= total));
  // wave-uniform queue state
  uint32_t shard = blockIdx.x & (SHADE_SHARDS - 1);
  uint32_t shards_left = SHADE_SHARDS;
  uint32_t q_next = 0, q_end = 0;
  // per-lane state: IDLE (no sample) -> TRAV (query in flight) -> READY (query answered, to shade)
  int ls = L_IDLE;
  uint32_t slot = 0;
  PathState ps;
  TravState ts;
  uint64_t trav_cycles = 0, step_cycles = 0, refill_cycles = 0, total_cycles = 0;
#ifdef FR_STAMPS
  uint32_t n_visits = 0, n_wave_steps = 0;
  uint32_t d_q = 0, d_steps = 0, d_t0 = 0, w_done = 0;
  const uint32_t w_begin = rtime();
  uint32_t w_dry = 0;
#endif
  STAMP(t_begin);
  while (true) {
    STAMP(t_refill);
    // Every idle lane takes a slot while the queue has any: the wave's pending range first, then
    // further chunks (one chunk per pass left idle lanes waiting a traversal loop).
    unsigned long long idle = __ballot(ls == L_IDLE);
    while (idle && (q_next < q_end || shards_left)) {
      if (q_next >= q_end) {
        // interleaved, not one contiguous range per XCD: the class-major list would put the refraction
        // class (the longest paths) on one XCD (measured 173 vs 183 fps)
        if (xcd_bands) {
        bool found = false;
        uint32_t j = 0;
        if (lane == 0) j = atomicAdd(&chunk_ctr[shard * SHADE_SHARD_STRIDE], 1u);
        j = __builtin_amdgcn_readfirstlane(j);
#pragma unroll
        for (int c = 0; c < 4; c++) {  // constant bounds: unrolled, cb[] stays in registers
          const uint32_t b = part(c, shard), e = part(c, shard + 1);
          const uint32_t ch = c == 0 ? chunk_refr : SHADE_CHUNK;
          const uint32_t n = (e - b + ch - 1) / ch;
          if (!found && j < n) {
            q_next = b + j * ch;
            q_end = min(q_next + ch, e);
            found = true;
          }
          if (!found) j -= n;
        }
        if (!found) {
          shard = (shard + 1) & (SHADE_SHARDS - 1);
          shards_left--;
        }
        } else {
        uint32_t j = 0;
        if (lane == 0) j = atomicAdd(&chunk_ctr[shard * SHADE_SHARD_STRIDE], 1u);
        j = __builtin_amdgcn_readfirstlane(j);
        const uint32_t g = j * SHADE_SHARDS + shard;
        if (g < nsmall) {
          q_next = g * chunk_refr;
          q_end = min(q_next + chunk_refr, nrefr);
        } else if (g < nchunks) {
          q_next = nrefr + (g - nsmall) * SHADE_CHUNK;
          q_end = min(q_next + SHADE_CHUNK, total);
        } else {
          shard = (shard + 1) & (SHADE_SHARDS - 1);
          shards_left--;
        }
        }
        continue;
      }
      const uint32_t take = min((uint32_t)__popcll(idle), q_end - q_next);
      if (ls == L_IDLE) {
        const uint32_t r = lanes_below(idle);
        if (r < take) {
          slot = q_next + r;
          path_init(U, aux[slot >> spp_shift], aux_seed[slot >> spp_shift], slot, ps, cnt);
          trav_begin(ts, ps.qd, ps.qtmax);
          RECORD_QUERY(ps);
          DIAG(d_q = 1; d_steps = 0; d_t0 = rtime());
          ls = L_TRAV;
        }
      }
      q_next += take;
      idle = __ballot(ls == L_IDLE);
    }
    const bool more = q_next < q_end || shards_left;  // wave-uniform: idle lanes can still be fed
    DIAG(if (!more && !w_dry) w_dry = rtime());
    if (fx && !more) {
      // The queue is dry: an idle lane takes the top pending work item (a refraction or reflection child
      // waiting on the item stack) of a busy lane of its wave, so the rest of a long sample tree is traced
      // by several lanes at once. The k-th idle lane pairs with the k-th lane holding items. The seed is
      // the sample's (ps.seed does not advance), so the item shades as it would on its owner's lane.
      const unsigned long long idle = __ballot(ls == L_IDLE);
      const unsigned long long donors = __ballot(ls != L_IDLE && ps.n > 0);
      if (idle && donors) {
        const uint32_t npair = min((uint32_t)__popcll(idle), (uint32_t)__popcll(donors));
        Item x = Item{mk3(0.0f), mk3(0.0f), mk3(0.0f), 0, 0.0f};
        if (ls != L_IDLE && ps.n > 0 && lanes_below(donors) < npair) {
          x = items.get(--ps.n);
          ps.total.flags |= FX_HELPED;
        }
        const bool taker = ls == L_IDLE && lanes_below(idle) < npair;
        const int src = taker ? (int)nth_set_bit(donors, lanes_below(idle)) : (int)lane;
        auto sh = [&](float v) { return __shfl(v, src, 64); };
        const f3 o = mk3(sh(x.o.x), sh(x.o.y), sh(x.o.z)), d = mk3(sh(x.d.x), sh(x.d.y), sh(x.d.z));
        const f3 w = mk3(sh(x.w.x), sh(x.w.y), sh(x.w.z));
        const int depth = __shfl(x.depth, src, 64);
        const float importance = sh(x.importance);
        const uint32_t xslot = (uint32_t)__shfl((int)slot, src, 64), xseed = (uint32_t)__shfl((int)ps.seed, src, 64);
        if (taker) {
          slot = xslot;
          ps.n = 0;
          ps.total.clear();
          ps.total.flags = FX_HELPER;
          ps.it = ItemState{w, depth, importance};
          ps.qo = o; ps.qd = d; ps.qtmax = INFINITY; ps.qany = false;
          ps.phase = PH_ITEM;
          ps.diffuse_kind = true; ps.want_child = false;
          ps.seed = xseed;
          trav_begin(ts, ps.qd, ps.qtmax);
          RECORD_QUERY(ps);
          DIAG(d_q = 1; d_steps = 0; d_t0 = rtime());
          ls = L_TRAV;
        }
      }
    }
    STAMP_ADD(refill_cycles, t_refill);
    if (!__ballot(ls != L_IDLE)) {
      if (!more) break;
      continue;
    }
    STAMP(t_tr);
    // Lanes whose new query was answered at the root shade again before any traversal.
    const bool traverse = !SHADE_FIRST_STEP || !__ballot(ls == L_READY);
    // Step every in-flight traversal node by node until all are answered; a lane whose query is
    // answered waits for the wave (measured: shading a few lanes at a time costs more than it saves,
    // also when the loop is left once 32/44/52 of 64 lanes are answered: +6 % stage time; and this
    // wave-uniform loop beats the per-lane form of the same schedule).
    for (uint32_t pass = 0; traverse && __ballot(ls == L_TRAV) &&
                            (!exit_early || pass < SHADE_EXIT_S || __popcll(__ballot(ls == L_TRAV)) > SHADE_EXIT_T ||
                             !__ballot(ls == L_READY));
         pass++) {
#ifdef FR_STAMPS
      n_wave_steps++;
      if (ls == L_TRAV) n_visits++;
#endif
#pragma unroll
      for (int u = 0; u < TRAV_UNROLL; u++)
        if (ls == L_TRAV) {
          DIAG(d_steps++);
          if (trav_step(sc, st, ts, ps.qo, ps.qd, tmin, ps.qtmax, ps.qany)) ls = L_READY;
        }
    }
    STAMP_ADD(trav_cycles, t_tr);
    STAMP(t_step);
    if (ls == L_READY) {
      const bool fin = path_shade(sc, U, ps, items, cnt, ts.best, (float)ts.atten, fx);
      if (fin) {
        ps.total.flush(samples, help, slot, fx);
        ls = L_IDLE;
#ifdef FR_STAMPS
        if (g_srec && slot < g_srec_cap) {
          g_srec[4 * (size_t)slot] = d_q; g_srec[4 * (size_t)slot + 1] = d_steps;
          g_srec[4 * (size_t)slot + 2] = d_t0; g_srec[4 * (size_t)slot + 3] = rtime();
        }
        w_done++;
#endif
      } else {
        trav_begin(ts, ps.qd, ps.qtmax);
        RECORD_QUERY(ps);
        DIAG(d_q++);
        ls = L_TRAV;
        // answered at the root: a miss (closest hit) or attenuation 1 (shadow); shaded in the next
        // pass, which runs before the next traversal loop
        if (SHADE_FIRST_STEP && !root_hit(lds_root, ps.qo, ts.inv, tmin, ps.qtmax)) ls = L_READY;
      }
    }
    STAMP_ADD(step_cycles, t_step);
  }
  STAMP_ADD(total_cycles, t_begin);
#ifdef FR_STAMPS
  if (lane == 0) {
    atomicAdd(&stats->pad[0], (unsigned long long)total_cycles);
    atomicAdd(&stats->pad[1], (unsigned long long)refill_cycles);
    atomicAdd(&stats->pad[2], (unsigned long long)step_cycles);
    atomicAdd(&stats->pad[3], (unsigned long long)trav_cycles);
    atomicAdd(&stats->pad[5], (unsigned long long)n_wave_steps);
  }
  atomicAdd(&stats->pad[4], (unsigned long long)n_visits);
  {
    const uint32_t wid = (blockIdx.x * TRACE_BLOCK + threadIdx.x) >> 6;
    const uint32_t w_end = rtime();
    uint32_t tot = w_done;
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    if (lane == 0 && g_wrec && wid < g_wrec_cap) {
      g_wrec[4 * (size_t)wid] = w_begin; g_wrec[4 * (size_t)wid + 1] = w_dry ? w_dry : w_end;
      g_wrec[4 * (size_t)wid + 2] = w_end; g_wrec[4 * (size_t)wid + 3] = tot;
    }
  }
#endif
  counters_end(stats, lds_cnt, false);
}

// Reduction, tone mapping and history of every active pixel (fov_path_trace_camera.cu:166-186).
// It also re-arms the work-queue counters of k_shade_paths for the next launch (they are zero at
// allocation), which spares a memset launch on the frame's critical path.
__global__ void k_shade_resolve(FrameUniforms U, const uint32_t* __restrict__ active,
                                const uint32_t* __restrict__ ray_count, const f4* __restrict__ weight,
                                const f4* __restrict__ history_cache, const f4* __restrict__ samples,
                                f4* __restrict__ history_buffer, f4* __restrict__ shading,
                                uint32_t* __restrict__ chunk_ctr, unsigned long long* __restrict__ help,
                                uint32_t fx_below, f4* __restrict__ radiance) {
  if (blockIdx.x == 0 && threadIdx.x < SHADE_SHARDS) {
    chunk_ctr[threadIdx.x * SHADE_SHARD_STRIDE] = 0;
    chunk_ctr[threadIdx.x * SHADE_SHARD_STRIDE + SHADE_REFR_CTR] = 0;
  }
  const uint32_t count = *ray_count;
  const int spp = U.spp;
  const bool fx = count * (uint32_t)spp < fx_below;  // the form k_shade_paths used (SampleSum)
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
    const uint32_t p = active[k];
    const f4 c_history = history_of(U, weight, history_cache, p);
    f3 total = mk3(0.0f);
    for (int j = 0; j < spp; j++) total = total + sample_value(samples, help, k * (uint32_t)spp + j, fx);
    total = total / (float)spp;
    f3 tm = uncharted2_tonemapping(total);
    if (radiance) radiance[k] = mk4(tm, 1.0f);  // (a sharded rank's part for the others: k_shard_pack_active)
    f4 fin = mk4(tm, 1.0f) + c_history;
    history_buffer[p] = fin;
    shading[p] = color_to_accumulated(fin);
  }
}

// Sparse form of the SHADING gather: a tracing rank sends only the pixels it traced (its active list: the
// pixel index and the pixel's (tone-mapped radiance, 1), 20 B each, ~10 % of its tiles); a receiving rank
// (which carries the history of every other pixel itself) adds the reprojected history from its own
// complete history, as k_shade_resolve does, and scatters them. The sender's history at the reprojection
// source is not used: a tile-edge pixel's reprojection can round to a neighbour in another rank's tiles
// (a still camera too), whose history the sender does not hold.
__global__ void k_shard_pack_active(const uint32_t* __restrict__ active, const uint32_t* __restrict__ ray_count,
                                    const f4* __restrict__ radiance, f4* __restrict__ vals, uint32_t* __restrict__ idx) {
  const uint32_t n = *ray_count;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    vals[k] = radiance[k];
    idx[k] = active[k];
  }
}
__global__ void k_shard_unpack_active(FrameUniforms U, const f4* __restrict__ vals, const uint32_t* __restrict__ idx,
                                      uint32_t n, uint32_t npix, const f4* __restrict__ weight,
                                      const f4* __restrict__ history_cache, f4* __restrict__ history_buffer,
                                      f4* __restrict__ shading) {
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const uint32_t p = idx[k];
    if (p >= npix) continue;  // a slab from another resolution (or garbage) never writes out of bounds
    const f4 fin = vals[k] + history_of(U, weight, history_cache, p);  // (k_shade_resolve's sum)
    history_buffer[p] = fin;
    shading[p] = color_to_accumulated(fin);
  }
}
void launch_shard_pack_active(const uint32_t* active, const uint32_t* ray_count, uint32_t capacity, const f4* radiance,
                              f4* vals, uint32_t* idx, hipStream_t stream) {
  if (!capacity) return;
  hipLaunchKernelGGL(k_shard_pack_active, dim3((unsigned)std::min<size_t>((capacity + 255) / 256, 4096)), dim3(256), 0,
                     stream, active, ray_count, radiance, vals, idx);
}
void launch_shard_unpack_active(const FrameUniforms& U, const f4* vals, const uint32_t* idx, uint32_t n, uint32_t npix,
                                const f4* weight, const f4* history_cache, f4* history_buffer, f4* shading,
                                hipStream_t stream) {
  if (!n) return;
  hipLaunchKernelGGL(k_shard_unpack_active, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0,
                     stream, U, vals, idx, n, npix, weight, history_cache, history_buffer, shading);
}

// History validity rings of a still-camera group (group.cpp, exchange). A pixel's seed depends on whether
// the history at its reprojection source is valid (k_sample_setup: .w > 0). Under a still camera that
// source is the pixel itself or a neighbour one rounding step away, so a pure tracer (whose history holds
// only its own tiles) misses the validity of the pixels just outside its tiles, which their owners hold.
// Each rank packs the bits (history .w > 0, after its frame) of the FR_VRING-pixel ring inside each of its
// tiles; a pure tracer writes them into its history's .w (1 or 0) before its next frame, so the seeds and
// its own carried validity follow the one-GPU frame's. Ring pixel k of a tile of side T: k < R T the top
// rows, then the bottom rows, the left columns, the right columns (k / T = the row or column's depth).
FR_DEV bool vring_pixel(int t, int k, int W, int H, int T, int& x, int& y) {
  const int ntx = (W + T - 1) / T;
  const int x0 = (t % ntx) * T, y0 = (t / ntx) * T;
  const int side = k / (FR_VRING * T), r = (k % (FR_VRING * T)) / T, c = k % T;
  switch (side) {
    case 0: x = x0 + c; y = y0 + r; break;
    case 1: x = x0 + c; y = y0 + T - 1 - r; break;
    case 2: x = x0 + r; y = y0 + c; break;
    default: x = x0 + T - 1 - r; y = y0 + c; break;
  }
  return x < W && y < H;
}
__global__ void k_vring_pack(const f4* __restrict__ hist, int W, int H, int T, const int32_t* __restrict__ tiles,
                             int ntiles, uint32_t* __restrict__ out) {
  const int wpt = FR_VRING * T / 8;  // 4 R T bits per tile
  for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < ntiles * wpt; w += gridDim.x * blockDim.x) {
    const int t = tiles[w / wpt], k0 = (w % wpt) * 32;
    uint32_t bits = 0;
    for (int b = 0; b < 32; b++) {
      int x, y;
      if (vring_pixel(t, k0 + b, W, H, T, x, y) && hist[(size_t)y * W + x].w > 0.0f) bits |= 1u << b;
    }
    out[w] = bits;
  }
}
__global__ void k_vring_unpack(const uint32_t* __restrict__ in, int W, int H, int T, const int32_t* __restrict__ tiles,
                               int ntiles, f4* __restrict__ hist) {
  const int per = 4 * FR_VRING * T;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ntiles * per; i += gridDim.x * blockDim.x) {
    int x, y;
    if (!vring_pixel(tiles[i / per], i % per, W, H, T, x, y)) continue;
    const uint32_t bit = (in[i / 32] >> (i % 32)) & 1u;
    reinterpret_cast<float*>(hist + (size_t)y * W + x)[3] = bit ? 1.0f : 0.0f;
  }
}
void launch_vring_pack(const f4* hist, int W, int H, int T, const int32_t* tiles, int ntiles, uint32_t* out,
                       hipStream_t stream) {
  if (ntiles <= 0) return;
  const int n = ntiles * (FR_VRING * T / 8);
  hipLaunchKernelGGL(k_vring_pack, dim3((unsigned)std::min((n + 255) / 256, 4096)), dim3(256), 0, stream, hist, W, H, T,
                     tiles, ntiles, out);
}
void launch_vring_unpack(const uint32_t* in, int W, int H, int T, const int32_t* tiles, int ntiles, f4* hist,
                         hipStream_t stream) {
  if (ntiles <= 0) return;
  const int n = ntiles * 4 * FR_VRING * T;
  hipLaunchKernelGGL(k_vring_unpack, dim3((unsigned)std::min((n + 255) / 256, 4096)), dim3(256), 0, stream, in, W, H,
                     T, tiles, ntiles, hist);
}

// Inactive pixels of entry 3 (fov_path_trace_camera.cu:102-108): carry the reprojected history.
// hvalid (latency mode, a one-view frame, not tile-sharded): per pixel, whether the history this frame writes there has .w > 0 (an
// active pixel's is k_shade_resolve's 1 + c.w, an inactive one's the carried c.w), one bit per pixel from the wave's
// ballot: the next frame's early k_sample_setup reads it instead of waiting for this frame's resolve.
template <bool LOCAL>
__global__ void k_carry_history(FrameUniforms U, const uint8_t* __restrict__ mask, const f4* __restrict__ weight,
                                const f4* __restrict__ history_cache, f4* __restrict__ history_buffer,
                                f4* __restrict__ shading, unsigned long long* __restrict__ hvalid) {
  const size_t N = (size_t)U.width * U.height;
  for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
    if (!LOCAL && hvalid) {  // (every lane of the wave takes part in the ballot: 64 consecutive pixels, the first 64-aligned)
      const bool act = mask[p] != 0;
      const f4 c = history_of(U, weight, history_cache, (uint32_t)p);
      const unsigned long long bits = __ballot(act ? 1.0f + c.w > 0.0f : c.w > 0.0f);
      if ((threadIdx.x & 63) == 0) hvalid[p >> 6] = bits;
      if (act) continue;
      history_buffer[p] = c;
      shading[p] = color_to_accumulated(c);
      continue;
    }
    if (mask[p]) continue;
    if (LOCAL && !shard_owns(U, (int)(p % (uint32_t)U.width), (int)(p / (uint32_t)U.width))) continue;  // not this rank's pixel
    f4 cw = weight[p];
    f4 c = mk4(0, 0, 0, 0);
    if (cw.z > 0.0f) {
      uint32_t qx = f2u_sat(fr_round(cw.x)), qy = f2u_sat(fr_round(cw.y));
      c = history_cache[(size_t)qy * U.width + qx];
    }
    history_buffer[p] = c;
    shading[p] = color_to_accumulated(c);
  }
}

#ifdef FR_STAMPS
// ---------------------------------------------------------------------------------------------
// Traversal probe (diagnostic build only): the megakernel's recorded query stream, traced by a
// persistent kernel whose lanes take the next query of their wave's chunk as soon as their own is
// answered. queries[2i] = (o, tmax), queries[2i+1] = (d, any); hits[i] = (t, beta, gamma, leaf),
// or (atten, 0, 0, -1) of a shadow query. It measures what traversal alone costs outside the
// megakernel. KIND 0: mixed stream; 1: closest-hit only; 2: shadow only.
// ---------------------------------------------------------------------------------------------
#ifndef TQ_WAVES
#define TQ_WAVES 5
#endif
#define TQ_CHUNK 64
template <int KIND>
__global__ __launch_bounds__(TRACE_BLOCK) __attribute__((amdgpu_waves_per_eu(TQ_WAVES, TQ_WAVES))) void k_trace_queries(
    DevScene sc, const f4* __restrict__ queries, uint32_t n, f4* __restrict__ hits, uint32_t* __restrict__ ctr) {
  __shared__ int32_t lds_stack[BVH_STACK * TRACE_BLOCK];
  Stack st{&lds_stack[threadIdx.x]};
  const float tmin = sc.scene_epsilon;
  uint32_t q_next = 0, q_end = 0;  // wave-uniform chunk
  bool more = true;                // the stream may still have chunks
  int qi = -1;                     // this lane's query
  f3 o, d;
  float tmax;
  bool any = false;
  TravState ts;
  while (true) {
    unsigned long long need = __ballot(qi < 0);
    while (need && more) {
      if (q_next >= q_end) {
        uint32_t j = 0;
        if ((threadIdx.x & 63) == 0) j = atomicAdd(ctr, 1u);
        j = __builtin_amdgcn_readfirstlane(j);
        q_next = j * TQ_CHUNK;
        q_end = min(q_next + TQ_CHUNK, n);
        if (q_next >= n) { more = false; break; }
      }
      if (qi < 0) {
        const uint32_t i = q_next + lanes_below(need);
        if (i < q_end) {
          qi = (int)i;
          const f4 a = queries[2 * (size_t)i], b = queries[2 * (size_t)i + 1];
          o = mk3(a.x, a.y, a.z); tmax = a.w;
          d = mk3(b.x, b.y, b.z); any = KIND == 0 ? b.w != 0.0f : KIND == 2;
          trav_begin(ts, d, tmax);
        }
      }
      q_next = min(q_next + (uint32_t)__popcll(need), q_end);
      need = __ballot(qi < 0);
    }
    if (!__ballot(qi >= 0)) break;
    if (qi >= 0 && trav_step(sc, st, ts, o, d, tmin, tmax, any)) {
      hits[qi] = any ? mk4((float)ts.atten, 0.0f, 0.0f, __int_as_float(-1))
                     : mk4(ts.best.t, ts.best.beta, ts.best.gamma, __int_as_float(ts.best.leaf));
      qi = -1;
    }
  }
}

void launch_trace_queries(const DevScene& sc, const f4* queries, uint32_t n, f4* hits, uint32_t* ctr,
                          hipStream_t stream, int kind) {
  hipMemsetAsync(ctr, 0, sizeof(uint32_t), stream);
  auto k = kind == 1 ? k_trace_queries<1> : kind == 2 ? k_trace_queries<2> : k_trace_queries<0>;
  hipLaunchKernelGGL(k, dim3(256 * 4 * TQ_WAVES / (TRACE_BLOCK / 64)), dim3(TRACE_BLOCK), 0, stream, sc, queries, n,
                     hits, ctr);
}

void diag_record_queries(f4* buf, uint32_t cap, hipStream_t stream) {
  const uint32_t zero = 0;
  hipMemcpyToSymbolAsync(HIP_SYMBOL(g_rec), &buf, sizeof(buf), 0, hipMemcpyHostToDevice, stream);
  hipMemcpyToSymbolAsync(HIP_SYMBOL(g_rec_cap), &cap, sizeof(cap), 0, hipMemcpyHostToDevice, stream);
  hipMemcpyToSymbolAsync(HIP_SYMBOL(g_rec_n), &zero, sizeof(zero), 0, hipMemcpyHostToDevice, stream);
}
void diag_sample_trace(uint32_t* srec, uint32_t scap, uint32_t* wrec, uint32_t wcap, hipStream_t stream) {
  hipMemcpyToSymbolAsync(HIP_SYMBOL(g_srec), &srec, sizeof(srec), 0, hipMemcpyHostToDevice, stream);
  hipMemcpyToSymbolAsync(HIP_SYMBOL(g_srec_cap), &scap, sizeof(scap), 0, hipMemcpyHostToDevice, stream);
  hipMemcpyToSymbolAsync(HIP_SYMBOL(g_wrec), &wrec, sizeof(wrec), 0, hipMemcpyHostToDevice, stream);
  hipMemcpyToSymbolAsync(HIP_SYMBOL(g_wrec_cap), &wcap, sizeof(wcap), 0, hipMemcpyHostToDevice, stream);
}
uint32_t diag_recorded_queries(hipStream_t stream) {
  uint32_t n = 0;
  hipMemcpyFromSymbolAsync(&n, HIP_SYMBOL(g_rec_n), sizeof(n), 0, hipMemcpyDeviceToHost, stream);
  hipStreamSynchronize(stream);
  return n;
}
#endif

// ---------------------------------------------------------------------------------------------
// Ray queries (fr_trace_rays, include/fovrt.h): a caller's batch of rays against the scene, over trav_begin /
// trav_step as every other ray of the engine. The shape is k_trace_queries': a persistent grid, a wave claims
// chunks of RQ_CHUNK rays with one atomic on a counter of the record, a lane whose ray is answered takes the chunk's
// next ray by its rank among the idle lanes, and a lane never waits for another wave. Against it: 32-B fr_ray
// records (two 16-B loads) with their own tmin, the degenerate-ray rule ahead of trav_begin (no traversal ever
// runs on NaN slabs), the scene's triangle index instead of the leaf's, the miss record (+inf, 0, 0, -1), and one
// template arm per kind (KIND 0: closest hit, 16-B fr_ray_hit records; KIND 1: transmittance, one float each; KIND 2:
// the closest hit as row 0 of 80-B fr_ray_surface records, which k_ray_surface completes) and per masking.
// The batch's chunks are split into FR_RAYQ_SHARDS contiguous runs with a counter each, 128 B apart; a wave starts
// on the run of its block's XCD (blockIdx & 7) and moves to the next run when its own is exhausted, for good: a
// run never refills. With one counter the 8.29 M camera rays of a 4K frame took 1.61 ms whatever their order, 12.5 ns
// per claim (129,600 same-address atomics, which the XCDs' L2s cannot combine); MEASUREMENTS.md, "Ray queries".
// Launch bounds and waves per SIMD are k_trace_queries' (not retuned).
// ---------------------------------------------------------------------------------------------
#ifndef RQ_WAVES
#define RQ_WAVES 5
#endif
#define RQ_CHUNK 64
// Answered without traversal: a NaN among the eight floats, an origin or a direction that is not finite, the
// direction (0, 0, 0), and an empty window (tmin >= tmax). (fabsf(NaN) < inf is false, so the finiteness tests
// catch the NaNs of origin and direction; !(tmin < tmax) those of the window.)
FR_DEV bool ray_degenerate(f4 a, f4 b) {
  const bool finite = fabsf(a.x) < INFINITY && fabsf(a.y) < INFINITY && fabsf(a.z) < INFINITY &&
                      fabsf(b.x) < INFINITY && fabsf(b.y) < INFINITY && fabsf(b.z) < INFINITY;
  const bool zero = b.x == 0.0f && b.y == 0.0f && b.z == 0.0f;
  return !finite || zero || !(a.w < b.w);
}
// KIND 2 (FR_RAYS_SURFACE): the closest hit written as row 0 of an 80-B fr_ray_surface record, with the hit's leaf
// index (-1: a miss) left in the record's word 7 for k_ray_surface, which overwrites it with the model.
#define RS_ROWS 5  // 16-B rows of an fr_ray_surface record
template <int KIND>
FR_DEV void ray_answer(void* __restrict__ out, uint32_t i, const TravState* ts) {
  if (KIND == 0) {
    const bool hit = ts && ts->best.leaf >= 0;
    static_cast<f4*>(out)[i] = hit ? mk4(ts->best.t, ts->best.beta, ts->best.gamma, __int_as_float(ts->best.prim))
                                   : mk4(INFINITY, 0.0f, 0.0f, __int_as_float(-1));
  } else if (KIND == 2) {
    const bool hit = ts && ts->best.leaf >= 0;
    f4* rec = static_cast<f4*>(out) + (size_t)RS_ROWS * i;
    rec[0] = hit ? mk4(ts->best.t, ts->best.beta, ts->best.gamma, __int_as_float(ts->best.prim))
                 : mk4(INFINITY, 0.0f, 0.0f, __int_as_float(-1));
    reinterpret_cast<int32_t*>(rec)[7] = hit ? ts->best.leaf : -1;
  } else {
    static_cast<float*>(out)[i] = ts ? (float)ts->atten : 1.0f;
  }
}
// MASKED: masks[i] selects the models ray i sees (test_tri); a ray whose mask selects no model of the scene is
// answered without traversal, as a degenerate ray is. The unmasked instantiations never read masks or rm.
template <int KIND, bool MASKED>
__global__ __launch_bounds__(TRACE_BLOCK) __attribute__((amdgpu_waves_per_eu(RQ_WAVES, RQ_WAVES))) void k_ray_queries(
    DevScene sc, const f4* __restrict__ rays, uint32_t n, void* __restrict__ out, RayQueryState* __restrict__ rq,
    const uint32_t* __restrict__ masks, const RayModels rm) {
  __shared__ int32_t lds_stack[BVH_STACK * TRACE_BLOCK];
  Stack st{&lds_stack[threadIdx.x]};
  uint32_t q_next = 0, q_end = 0;  // wave-uniform chunk
  bool more = true;                // the batch may still have chunks
  const uint32_t chunks = (n + RQ_CHUNK - 1) / RQ_CHUNK;
  uint32_t shard = blockIdx.x % FR_RAYQ_SHARDS, tried = 0;  // the run this wave claims from; runs found exhausted
  int qi = -1;                     // this lane's ray
  f3 o, d;
  float tmin, tmax;
  uint32_t mask = 0;               // MASKED: this lane's ray's models
  TravState ts;
  while (true) {
    unsigned long long need = __ballot(qi < 0);
    while (need && more) {
      if (q_next >= q_end) {
        // the next chunk of this wave's run, or of the first later run that still has one
        bool got = false;
        while (tried < FR_RAYQ_SHARDS) {
          const uint32_t lo = (uint32_t)((uint64_t)chunks * shard / FR_RAYQ_SHARDS),
                         hi = (uint32_t)((uint64_t)chunks * (shard + 1) / FR_RAYQ_SHARDS);
          uint32_t j = 0;
          if ((threadIdx.x & 63) == 0) j = atomicAdd(&rq->next_chunk[shard * FR_RAYQ_SHARD_STRIDE], 1u);
          j = __builtin_amdgcn_readfirstlane(j);
          // (j <= a run's chunks + the grid's waves, chunks <= 2^24: no sum or product here reaches 2^32)
          if (j < hi - lo) {
            q_next = (lo + j) * RQ_CHUNK;
            q_end = min(q_next + RQ_CHUNK, n);
            got = true;
            break;
          }
          shard = (shard + 1) % FR_RAYQ_SHARDS;
          tried++;
        }
        if (!got) { more = false; break; }
      }
      if (qi < 0) {
        const uint32_t i = q_next + lanes_below(need);
        if (i < q_end) {
          const f4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
          if (MASKED) mask = masks[i] & rm.valid;
          if (ray_degenerate(a, b) || (MASKED && mask == 0)) {
            ray_answer<KIND>(out, i, nullptr);  // (the lane stays idle and takes another ray of the chunk)
          } else {
            qi = (int)i;
            o = mk3(a.x, a.y, a.z); tmin = a.w;
            d = mk3(b.x, b.y, b.z); tmax = b.w;
            trav_begin(ts, d, tmax);
          }
        }
      }
      q_next = min(q_next + (uint32_t)__popcll(need), q_end);
      need = __ballot(qi < 0);
    }
    if (!__ballot(qi >= 0)) break;
    if (qi >= 0 && trav_step<MASKED>(sc, st, ts, o, d, tmin, tmax, KIND == 1, mask, &rm)) {
      ray_answer<KIND>(out, (uint32_t)qi, &ts);
      qi = -1;
    }
  }
}

// The surface at the hits k_ray_queries<2> found (FR_RAYS_SURFACE): one lane per ray reads its ray, row 0 of its
// record and the leaf index in word 7, and writes rows 1 to 4 as the closest-hit programs see the hit: surface() and
// kd_of(), the G-buffer's and the megakernel's, unchanged. A separate launch keeps the traversal kernel's registers
// and occupancy, and the divergent fetches of shading record, material and texels are made by full waves rather
// than by the lanes of a traversing wave that happen to finish. A lane stores its four rows as four 16-B stores,
// 64 consecutive bytes of its own record: the record's 80-B stride leaves no wider store aligned, and a stage
// through LDS to make the wave's stores contiguous would add 5 KB of LDS and two barriers per block to a kernel
// whose time is the texel and shading-record fetches (MEASUREMENTS.md, "Ray queries: surface and masks").
#define RS_BLOCK 256
__global__ __launch_bounds__(RS_BLOCK) void k_ray_surface(DevScene sc, const f4* __restrict__ rays, uint32_t n, f4* out,
                                                          const RayModels rm) {
  const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
  if (i >= n) return;
  f4* rec = out + (size_t)RS_ROWS * i;
  const f4 r0 = rec[0];
  const int leaf = reinterpret_cast<const int32_t*>(rec)[7];
  if (leaf < 0) {  // a miss, a degenerate ray or an empty mask: model -1, every other word 0
    rec[1] = mk4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    rec[2] = rec[3] = rec[4] = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const f4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
  const f3 o = mk3(a.x, a.y, a.z), d = mk3(b.x, b.y, b.z);
  Hit h;
  h.t = r0.x; h.beta = r0.y; h.gamma = r0.z; h.leaf = leaf; h.prim = __float_as_int(r0.w);
  const SurfaceHit s = surface(sc, h, o, d);
  const f3 kd = kd_of(sc, s.mat, s.uv);
  const int flags = (int)fbits(sc.shade[h.prim].t.w);
  const TriGeo g = sc.tri_geo[leaf];
  // refine_and_offset's side test, on the attribute normal
  const int back = dotc(normalizec(mk3(g.c.y, g.c.z, g.c.w)), d) > 0.0f ? 1 : 0;
  const int word = s.mat | sc.mats[s.mat].type << 8 | (flags & (FR_SHADE_HAS_NORMALS | FR_SHADE_HAS_UV)) << 8 | back << 18;
  rec[1] = mk4(s.front.x, s.front.y, s.front.z, __int_as_float(ray_model_of(rm, h.prim)));
  rec[2] = mk4(s.ng.x, s.ng.y, s.ng.z, s.uv.x);
  rec[3] = mk4(s.ns.x, s.ns.y, s.ns.z, s.uv.y);
  rec[4] = mk4(kd.x, kd.y, kd.z, __int_as_float(word));
}

// Resident blocks of k_ray_queries: RQ_WAVES waves per SIMD, 4 SIMDs per CU, 256 CUs (12 KB of LDS per block).
static uint32_t ray_query_resident_blocks() { return 256u * 4u * RQ_WAVES / (TRACE_BLOCK / 64); }

// kind: 0 closest hit (out: n records of 16 B), 1 transmittance (out: n floats), 2 surface (out: n records of 80 B;
// k_ray_surface follows on the same stream). masks: NULL, or n words (bit k: model k takes part). The counter of `rq`
// is zeroed in stream order ahead of the kernel. max_blocks: the context's cap on the grid (FOVRT_RAYQ_BLOCKS), 0 = none.
void launch_ray_queries(const DevScene& sc, const void* rays, const uint32_t* masks, uint32_t n, int kind, void* out,
                        RayQueryState* rq, const RayModels& rm, uint32_t max_blocks, hipStream_t stream) {
  if (n == 0) return;
  uint32_t blocks = std::min((n + TRACE_BLOCK - 1) / TRACE_BLOCK, ray_query_resident_blocks());
  if (max_blocks) blocks = std::min(blocks, max_blocks);
  (void)hipMemsetAsync(rq, 0, sizeof(RayQueryState), stream);
  auto k = masks ? (kind == 1 ? k_ray_queries<1, true> : kind == 2 ? k_ray_queries<2, true> : k_ray_queries<0, true>)
                 : (kind == 1 ? k_ray_queries<1, false> : kind == 2 ? k_ray_queries<2, false> : k_ray_queries<0, false>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(TRACE_BLOCK), 0, stream, sc, static_cast<const f4*>(rays), n, out, rq, masks,
                     rm);
  if (kind == 2)
    hipLaunchKernelGGL(k_ray_surface, dim3((n + RS_BLOCK - 1) / RS_BLOCK), dim3(RS_BLOCK), 0, stream, sc,
                       static_cast<const f4*>(rays), n, static_cast<f4*>(out), rm);
}

// ---------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------
void launch_gbuffer(const DevScene& sc, const FrameUniforms& U, f4* position, f4* normal, f4* depth, f4* diffuse,
                    f4* weight, uint8_t* gclass, DevStats* stats, const f3* cur_pos, const f3* prev_pos,
                    hipStream_t stream) {
  int tiles = ((U.width + 7) / 8) * ((U.height + 7) / 8);
  int threads = tiles * 64;
  int blocks = (threads + TRACE_BLOCK - 1) / TRACE_BLOCK;
  // the motion form when the caller gives both position arrays (ctx_frame.cpp, enqueue_geometry)
  const bool motion = cur_pos && prev_pos;
  auto k = U.front_need ? (motion ? k_gbuffer<true, true> : k_gbuffer<true, false>)
                        : (motion ? k_gbuffer<false, true> : k_gbuffer<false, false>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(TRACE_BLOCK), 0, stream, sc, U, position, normal, depth, diffuse, weight,
                     gclass, stats, cur_pos, prev_pos);
}

// Grid of k_shade_paths: persistent, as many resident blocks as the register budget allows (SHADE_WAVES
// waves per SIMD, 4 SIMDs per CU, TRACE_BLOCK / 64 waves per block, 256 CUs). per_cu: the context's blocks per CU
// (fr_ctx::shade_blocks_per_cu, at most shade_max_blocks_per_cu).
int shade_max_blocks_per_cu() { return 4 * SHADE_WAVES / (TRACE_BLOCK / 64); }
static int shade_blocks(const FrameUniforms& U, uint32_t max_active, int per_cu) {
  size_t slots = (size_t)max_active * U.spp;
  return (int)std::min<size_t>((slots + TRACE_BLOCK - 1) / TRACE_BLOCK, (size_t)256 * per_cu);
}

// Does a W x H frame at spp (max_active = W H) use the fixed-point sums and the tail handoff (SampleSum)?
// handoff: 0 never, 1 below SHADE_FX_FRAME pixel-samples per lane of the grid, 2 always.
static bool shade_fx_frame(int spp, uint32_t max_active, uint32_t handoff, int per_cu) {
  if (handoff == 0) return false;
  if (handoff >= 2) return true;
  FrameUniforms U{};
  U.spp = spp;
  const uint64_t lanes = (uint64_t)shade_blocks(U, max_active, per_cu) * TRACE_BLOCK;
  return (uint64_t)max_active * (uint64_t)spp < (uint64_t)SHADE_FX_FRAME * lanes;
}

// Sample slots that can use the fixed-point form (32-B records in samples, 32-B help records).
size_t shade_fx_slots(uint32_t max_active, int spp, uint32_t handoff, int per_cu) {
  return shade_fx_frame(spp, max_active, handoff, per_cu) ? (size_t)max_active * spp : 0;
}

// The kernels' threshold: launches of fewer samples use the fixed-point form (all or none).
static uint32_t shade_fx_below(const FrameUniforms& U, uint32_t max_active, uint32_t handoff, int per_cu) {
  return shade_fx_frame(U.spp, max_active, handoff, per_cu) ? 0xFFFFFFFFu : 0u;
}

void launch_shade_paths(const DevScene& sc, const FrameUniforms& U, const uint32_t* active, const uint32_t* ray_count,
                        uint32_t max_active, const f4* weight, const f4* history_cache, uint32_t* chunk_ctr,
                        f4* samples, unsigned long long* help, DevStats* stats, f4* aux, uint32_t* aux_seed,
                        uint32_t chunk_refr, uint32_t xcd_bands, uint32_t handoff, int per_cu, f4* item_store,
                        hipStream_t stream) {
  if (max_active == 0) return;
  const int blocks = shade_blocks(U, max_active, per_cu);
  // chunk_refr: a fixed refraction-class chunk (fr_ctx, FOVRT_SHADE_CHUNK_REFR), 0 = adaptive
  const uint32_t cr = chunk_refr ? std::min(std::max(chunk_refr & ~((uint32_t)U.spp - 1u), (uint32_t)U.spp), (uint32_t)SHADE_CHUNK) : 0u;
  const uint32_t fxb = shade_fx_below(U, max_active, handoff, per_cu);
  hipLaunchKernelGGL(k_shade_paths, dim3(blocks), dim3(TRACE_BLOCK), 0, stream, sc,
                     U, active, ray_count, weight, history_cache, chunk_ctr, samples, stats, aux, aux_seed, cr,
                     xcd_bands, help, fxb, item_store);
}

// The megakernel's item stacks (ItemStack): the largest grid's lanes x ITEM_STACK items of 64 B.
size_t shade_item_store_f4(int per_cu) {
  FrameUniforms U{};
  U.spp = 1;
  return (size_t)shade_blocks(U, 0xFFFFFFFFu, per_cu) * TRACE_BLOCK * ITEM_STACK * 4;
}

void launch_sample_setup(const FrameUniforms& U, const uint32_t* active, const uint32_t* ray_count, uint32_t max_active,
                         const f4* weight, const f4* history_cache, const unsigned long long* hvalid, f4* aux,
                         uint32_t* aux_seed, hipStream_t stream) {
  if (max_active == 0) return;
  hipLaunchKernelGGL(k_sample_setup, dim3((unsigned)std::min<size_t>((max_active + 255) / 256, 4096)), dim3(256), 0,
                     stream, U, active, ray_count, weight, history_cache, hvalid, aux, aux_seed);
}

void launch_shade_resolve(const FrameUniforms& U, const uint32_t* active, const uint32_t* ray_count,
                          uint32_t max_active, const f4* weight, const f4* history_cache, const f4* samples,
                          unsigned long long* help, f4* history_buffer, f4* shading, uint32_t* chunk_ctr,
                          uint32_t handoff, int per_cu, f4* radiance, hipStream_t stream) {
  if (max_active == 0) return;
  int rblocks = (int)std::min<size_t>((max_active + 255) / 256, 4096);
  hipLaunchKernelGGL(k_shade_resolve, dim3(rblocks), dim3(256), 0, stream, U, active, ray_count, weight,
                     history_cache, samples, history_buffer, shading, chunk_ctr, help,
                     shade_fx_below(U, max_active, handoff, per_cu), radiance);
}

size_t shade_counter_words() { return SHADE_SHARDS * SHADE_SHARD_STRIDE; }

void launch_carry_history(const FrameUniforms& U, const uint8_t* mask, const f4* weight, const f4* history_cache,
                          f4* history_buffer, f4* shading, unsigned long long* hvalid, hipStream_t stream) {
  size_t N = (size_t)U.width * U.height;
  int blocks = (int)std::min<size_t>((N + 255) / 256, 8192);
  hipLaunchKernelGGL(U.front_need ? k_carry_history<true> : k_carry_history<false>, dim3(blocks), dim3(256), 0, stream, U, mask, weight, history_cache,
                     history_buffer, shading, hvalid);
}

}  // namespace fr
