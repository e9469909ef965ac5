// sah_host_check — the host side of the device SAH builder's reference under the host sanitizers: fr_scene_create
// and the test hook fr__scene_rebuild_over (the host builder's tree over any geometry) on a few cases, with its own
// main, linked against the sanitizer build of the library (make asan-sah-check). No device is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fovrt.h"

extern "C" {
int fr__scene_bvh(fr_scene* sc, const void** nodes, int* num_nodes, const void** tri_geo, const int32_t** prim,
                  int* num_leaf_tris);
int fr__scene_rebuild_over(fr_scene* sc, const float* xyz, size_t ntris);
}

static int fails = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } \
  } while (0)

struct Tree {
  std::vector<unsigned char> nodes;
  std::vector<int32_t> prim;
};

static Tree tree_of(fr_scene* sc, int ntris) {
  const void *nodes = nullptr, *tri = nullptr;
  const int32_t* prim = nullptr;
  int nn = 0, nl = 0;
  CHECK(fr__scene_bvh(sc, &nodes, &nn, &tri, &prim, &nl) == FR_OK);
  CHECK(nl == ntris && nn >= 1 && nn <= ntris);
  Tree t;
  t.nodes.assign((const unsigned char*)nodes, (const unsigned char*)nodes + (size_t)nn * 128);
  t.prim.assign(prim, prim + nl);
  std::vector<int> seen((size_t)ntris, 0);
  for (int p : t.prim) {
    CHECK(p >= 0 && p < ntris);
    if (p >= 0 && p < ntris) seen[(size_t)p]++;
  }
  for (int s : seen) CHECK(s == 1);
  return t;
}

int main() {
  fr_config cfg;
  fr_config_default(&cfg);
  cfg.scene = 1;
  cfg.texture_mode = 1;
  cfg.detail = 1;
  fr_scene* sc = nullptr;
  CHECK(fr_scene_create(&cfg, &sc) == FR_OK && sc);
  if (!sc) return 1;
  fr_scene_arrays a;
  CHECK(fr_scene_get_arrays(sc, &a) == FR_OK);
  const int n = a.num_tris;
  const std::vector<float> rest(a.pos, a.pos + (size_t)n * 9);
  const Tree t0 = tree_of(sc, n);

  // the rest positions again: the scene's own tree, byte for byte
  CHECK(fr__scene_rebuild_over(sc, rest.data(), (size_t)n) == 0);
  const Tree t1 = tree_of(sc, n);
  CHECK(t1.nodes == t0.nodes && t1.prim == t0.prim);

  // case 1: a smooth deformation
  std::vector<float> pos = rest;
  for (size_t v = 0; v < (size_t)n * 3; v++) pos[3 * v + 1] += 0.2f * sinf(3.0f * rest[3 * v]);
  CHECK(fr__scene_rebuild_over(sc, pos.data(), (size_t)n) == 0);
  const Tree t2 = tree_of(sc, n);
  CHECK(t2.nodes != t0.nodes);

  // case 2: every triangle the same one (equal centroids at every node)
  for (size_t i = 0; i < (size_t)n; i++) memcpy(&pos[9 * i], &rest[0], 9 * sizeof(float));
  CHECK(fr__scene_rebuild_over(sc, pos.data(), (size_t)n) == 0);
  tree_of(sc, n);

  // case 3: a geometric comb on one line, which reaches the depth limit (leaves of more than two triangles)
  std::fill(pos.begin(), pos.end(), 0.0f);
  for (size_t i = 0; i < (size_t)n; i++) {
    const float x = ldexpf(8.0f, -(int)(i % 125));
    pos[9 * i] = pos[9 * i + 3] = pos[9 * i + 6] = x;
    pos[9 * i + 4] = 1e-3f;
    pos[9 * i + 8] = 1e-3f;
  }
  CHECK(fr__scene_rebuild_over(sc, pos.data(), (size_t)n) == 0);
  tree_of(sc, n);

  // refused: a wrong count, a non-finite coordinate; the tree stays
  const Tree t3 = tree_of(sc, n);
  CHECK(fr__scene_rebuild_over(sc, pos.data(), (size_t)n - 1) == FR_E_INVALID);
  pos[5] = INFINITY;
  CHECK(fr__scene_rebuild_over(sc, pos.data(), (size_t)n) == FR_E_INVALID);
  const Tree t4 = tree_of(sc, n);
  CHECK(t4.nodes == t3.nodes && t4.prim == t3.prim);

  CHECK(fr_scene_destroy(sc) == FR_OK);
  printf(fails ? "sah_host_check: %d failures\n" : "sah_host_check ok (%d)\n", fails);
  return fails ? 1 : 0;
}
