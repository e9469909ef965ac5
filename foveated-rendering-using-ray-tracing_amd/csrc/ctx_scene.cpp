// ctx_scene.cpp — the scene's description on the host: the model table, the smooth-vertex groups and the export of a
// context's scene (fr_scene_export, which first brings the host mirrors up to date), and the host-only fr_scene object
// with its test hooks, which shares the three fillers below with them.
#include <cmath>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

void fri::box_of(const f3* v, size_t n, f3* lo, f3* hi) {
  *lo = mk3(INFINITY);
  *hi = mk3(-INFINITY);
  for (size_t i = 0; i < n; i++) {
    *lo = mk3(fminf(lo->x, v[i].x), fminf(lo->y, v[i].y), fminf(lo->z, v[i].z));
    *hi = mk3(fmaxf(hi->x, v[i].x), fmaxf(hi->y, v[i].y), fmaxf(hi->z, v[i].z));
  }
}

// The models are the contiguous triangle ranges add_mesh recorded (scene.cpp), in scene order.
int fri::model_info(const HostScene& s, int i, const char** name, int* first_tri, int* ntris) {
  if (i < 0 || i >= (int)s.model_tri_count.size()) return FR_E_INVALID;
  int first = 0;
  for (int k = 0; k < i; k++) first += s.model_tri_count[k];
  if (name) *name = s.model_names[i].c_str();
  if (first_tri) *first_tri = first;
  if (ntris) *ntris = s.model_tri_count[i];
  return FR_OK;
}

static int copy_groups(const NormalGroups& g, int32_t* corner_vertex, size_t ncorners, int* nverts) {
  if (corner_vertex) {
    if (ncorners != g.corner_vertex.size()) return FR_E_INVALID;
    memcpy(corner_vertex, g.corner_vertex.data(), ncorners * sizeof(int32_t));
  }
  if (nverts) *nverts = g.num_verts;
  return FR_OK;
}

static void fill_arrays(const HostScene& s, const Bvh& bvh, f3 emission, std::vector<int32_t>& mat_pairs,
                        std::vector<int32_t>& tex_dims, std::vector<const float*>& tex_ptrs, fr_scene_arrays* o) {
  memset(o, 0, sizeof(*o));
  o->num_tris = s.num_tris();
  o->pos = &s.pos[0].x; o->nrm = &s.nrm[0].x; o->uv = &s.uv[0].x; o->flags = s.flags.data();
  mat_pairs.clear();
  for (auto& m : s.mats) { mat_pairs.push_back(m.type); mat_pairs.push_back(m.tex); }
  o->num_materials = (int)s.mats.size();
  o->materials = mat_pairs.data();
  tex_dims.clear(); tex_ptrs.clear();
  for (auto& t : s.texs) { tex_dims.push_back(t.w); tex_dims.push_back(t.h); tex_ptrs.push_back(&t.data[0].x); }
  o->num_textures = (int)s.texs.size();
  o->tex_dims = tex_dims.data();
  o->tex_data = tex_ptrs.data();
  o->envmap = s.envmap;
  const f3 L[5] = {s.light_position, s.light_v1, s.light_v2, s.light_normal, emission};
  for (int i = 0; i < 5; i++) { o->light[3 * i] = L[i].x; o->light[3 * i + 1] = L[i].y; o->light[3 * i + 2] = L[i].z; }
  o->bbox[0] = s.bbox_min.x; o->bbox[1] = s.bbox_min.y; o->bbox[2] = s.bbox_min.z;
  o->bbox[3] = s.bbox_max.x; o->bbox[4] = s.bbox_max.y; o->bbox[5] = s.bbox_max.z;
  o->bvh_nodes = tree_nodes(bvh);
  o->bvh_depth = bvh.max_depth;
  o->bvh_max_stack = bvh.max_stack;
}

struct fr_scene {
  HostScene scene;
  Bvh bvh;
  NormalGroups groups;
  std::string err;
  std::vector<const float*> tex_ptrs;
  std::vector<int32_t> tex_dims, mat_pairs;
};

extern "C" {

int fr_model_count(fr_ctx* c, int* n) {
  if (!c || !n) return FR_E_INVALID;
  *n = (int)c->scene.model_tri_count.size();
  return FR_OK;
}

int fr_model_info(fr_ctx* c, int i, const char** name, int* first_tri, int* ntris) {
  if (!c) return FR_E_INVALID;
  if (model_info(c->scene, i, name, first_tri, ntris)) return fail(c, FR_E_INVALID, "fr_model_info: no such model");
  return FR_OK;
}

int fr_normal_groups(fr_ctx* c, int32_t* corner_vertex, size_t ncorners, int* nverts) {
  if (!c) return FR_E_INVALID;
  if (copy_groups(c->groups, corner_vertex, ncorners, nverts))
    return fail(c, FR_E_INVALID, "fr_normal_groups: ncorners is not 3 per triangle");
  return FR_OK;
}

int fr_scene_export(fr_ctx* c, fr_scene_arrays* o) {
  if (!c || !o) return FR_E_INVALID;
  if (int rc = tree_numbers(c)) return rc;
  if (c->geo_read.pending && (c->pos_mirror_stale || c->box_mirror_stale || c->nrm_mirror_stale)) {
    // enqueued updates may still be running: the copies below (null stream) do not wait for the context stream
    // (nor for front_stream, where an overlapped update runs: the context stream waits for that one first)
    hipSetDevice(c->cfg.device);
    join_update(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (c->pos_mirror_stale) {  // positions last came from device memory (fr_update_positions): fetch them now
    hipSetDevice(c->cfg.device);
    HIP_TRY(c, hipMemcpy(c->scene.pos.data(), c->d_pos, c->scene.pos.size() * sizeof(f3), hipMemcpyDeviceToHost));
    c->pos_mirror_stale = false;
  }
  if (c->box_mirror_stale) {  // an enqueued update left the scene box on the device (fr_update_geometry_enqueue)
    hipSetDevice(c->cfg.device);
    float box[6];
    HIP_TRY(c, hipMemcpy(box, c->geo->box, sizeof(box), hipMemcpyDeviceToHost));
    c->scene.bbox_min = c->dsc.bbox_min = mk3(box[0], box[1], box[2]);
    c->scene.bbox_max = c->dsc.bbox_max = mk3(box[3], box[4], box[5]);
    c->box_mirror_stale = false;
  }
  if (c->nrm_mirror_stale) {  // normals were last written on the device: they are d_shade's n0 / n1 / n2 .xyz
    hipSetDevice(c->cfg.device);
    std::vector<TriShade> shade(c->scene.flags.size());
    HIP_TRY(c, hipMemcpy(shade.data(), c->d_shade, shade.size() * sizeof(TriShade), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < shade.size(); i++) {
      c->scene.nrm[3 * i] = xyz(shade[i].n0);
      c->scene.nrm[3 * i + 1] = xyz(shade[i].n1);
      c->scene.nrm[3 * i + 2] = xyz(shade[i].n2);
    }
    c->nrm_mirror_stale = false;
  }
  fill_arrays(c->scene, c->bvh, c->dsc.light_emission, c->mat_pairs, c->tex_dims, c->tex_ptrs, o);
  return FR_OK;
}

int fr_scene_create(const fr_config* cfg_in, fr_scene** out) {
  if (!out) return fail(nullptr, FR_E_INVALID, "out is NULL");
  *out = nullptr;
  fr_config cfg;
  if (cfg_in) cfg = *cfg_in; else fr_config_default(&cfg);
  if (cfg.scene < 0 || cfg.scene > 2) return fail(nullptr, FR_E_INVALID, "bad scene preset");
  if (cfg.mesh_mode < 0 || cfg.mesh_mode > 2) return fail(nullptr, FR_E_INVALID, "bad mesh_mode");
  fr_scene* sc = new fr_scene();
  std::string err;
  if (!build_preset_scene(cfg.scene, cfg.asset_dir ? cfg.asset_dir : "assets", cfg.texture_mode, cfg.light_power,
                          cfg.detail, sc->scene, err, cfg.mesh_mode)) {
    delete sc;
    return fail(nullptr, FR_E_IO, "scene: " + err);
  }
  build_bvh(sc->scene, sc->bvh);
  build_normal_groups(sc->scene, sc->groups);
  *out = sc;
  return FR_OK;
}

int fr_scene_get_arrays(fr_scene* sc, fr_scene_arrays* o) {
  if (!sc || !o) return FR_E_INVALID;
  fill_arrays(sc->scene, sc->bvh, sc->scene.light_emission, sc->mat_pairs, sc->tex_dims, sc->tex_ptrs, o);
  return FR_OK;
}

int fr_scene_normal_groups(fr_scene* sc, int32_t* corner_vertex, size_t ncorners, int* nverts) {
  if (!sc) return FR_E_INVALID;
  return copy_groups(sc->groups, corner_vertex, ncorners, nverts);
}

int fr_scene_model_count(fr_scene* sc, int* n) {
  if (!sc || !n) return FR_E_INVALID;
  *n = (int)sc->scene.model_tri_count.size();
  return FR_OK;
}

int fr_scene_model_info(fr_scene* sc, int i, const char** name, int* first_tri, int* ntris) {
  if (!sc) return FR_E_INVALID;
  return model_info(sc->scene, i, name, first_tri, ntris);
}

// Test hook (not part of include/fovrt.h): the host-built tree of an fr_scene (pointers into it, valid until
// fr_scene_destroy): num_nodes BvhNode, then num_leaf_tris TriGeo and leaf-order primitive indices.
int fr__scene_bvh(fr_scene* sc, const void** nodes, int* num_nodes, const void** tri_geo, const int32_t** prim,
                  int* num_leaf_tris) {
  if (!sc || !nodes || !num_nodes || !tri_geo || !prim || !num_leaf_tris) return FR_E_INVALID;
  *nodes = sc->bvh.nodes.data();
  *num_nodes = (int)sc->bvh.nodes.size();
  *tri_geo = sc->bvh.tri_geo.data();
  *prim = sc->bvh.tri_prim.data();
  *num_leaf_tris = (int)sc->bvh.tri_prim.size();
  return FR_OK;
}

// Test hook (not part of include/fovrt.h): replaces the positions of an fr_scene (xyz: ntris x 9 floats, finite;
// ntris the scene's) and its box, and builds its tree over them with the host builder, as fr_scene_create did over
// the preset's. The host builder's tree for any geometry, without a device: the reference of the device SAH
// builder. Returns a negative status, or the number of splits that took the median fallback although the node's
// centroids differ on the split axis (the one case in which the device builder fails instead; 0 on geometry of
// ordinary size). Pointers fr__scene_bvh and fr_scene_get_arrays gave before the call are stale after it.
int fr__scene_rebuild_over(fr_scene* sc, const float* xyz, size_t ntris) {
  if (!sc || !xyz || ntris != (size_t)sc->scene.num_tris()) return FR_E_INVALID;
  for (size_t i = 0; i < ntris * 9; i++)
    if (!std::isfinite(xyz[i])) return FR_E_INVALID;
  memcpy(sc->scene.pos.data(), xyz, ntris * 9 * sizeof(float));
  box_of(sc->scene.pos.data(), ntris * 3, &sc->scene.bbox_min, &sc->scene.bbox_max);
  int medians = 0;
  build_bvh(sc->scene, sc->bvh, &medians);
  return medians;
}

int fr_scene_destroy(fr_scene* sc) {
  if (!sc) return FR_E_INVALID;
  delete sc;
  return FR_OK;
}

}  // extern "C"
