// ctx_create.cpp — fr_ctx's life and plain state: fr_create (scene upload, texture packing, every buffer allocated
// once), fr_destroy, the error text and the setters that only store a value. With the other ctx_*.cpp the host-side
// counterpart of PathTracer (FR/PathTracer.cpp) and of the GL pass classes: zero host copies between stages (the
// reference's PBO->texture copies, FR/PathTracer.cpp:253-305, disappear).
#include <cmath>
#include <cstdlib>

#include "ctx_internal.h"

using namespace fr;
using fri::fail;

static thread_local std::string g_create_error;

int fri::fail(fr_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg; else g_create_error = msg;
  return code;
}

extern "C" {

const char* fr_version(void) { return "fovrt 0.2 (gfx950)"; }
int fr_abi_version(void) { return FOVRT_ABI_VERSION; }

int fr_config_default(fr_config* c) {
  if (!c) return FR_E_INVALID;
  memset(c, 0, sizeof(*c));
  c->abi_version = FOVRT_ABI_VERSION;
  c->width = 1024; c->height = 1024;
  c->scene = FR_SCENE_BUNNY;
  c->mask_mode = FR_MASK_SALIENCY;
  c->spp = 1;
  c->diffuse_max_depth = 1;
  c->refraction_max_depth = 16;
  c->light_power = 810.0f;
  c->optimize = 1;
  c->atrous_iterations = 1;
  c->write_extra = 1;
  return FR_OK;  // (device 0, texture_mode, detail and mesh_mode 0, asset_dir NULL: the memset)
}

const char* fr_last_error(fr_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// The densest exact storage of a host texture (DevTexture): FR_TEX_UNORM8 when every channel of every
// texel is (float)b / 255.0f, FR_TEX_RGBE when every texel is m * 2^(e - 136) with alpha 1 (load_hdr's
// decoding), else FR_TEX_F32. Each candidate is decoded back here with the loaders' own formulas and
// must reproduce every float bit for bit.
static int pack_texture(const HostTexture& t, std::vector<uint32_t>& out) {
  const size_t n = t.data.size();
  auto same = [](float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; };
  out.resize(n);
  bool unorm = true;
  for (size_t i = 0; i < n && unorm; i++) {
    const float v[4] = {t.data[i].x, t.data[i].y, t.data[i].z, t.data[i].w};
    uint32_t word = 0;
    for (int c = 0; c < 4; c++) {
      const long b = std::lrint((double)v[c] * 255.0);
      if (b < 0 || b > 255 || !same((float)b / 255.0f, v[c])) { unorm = false; break; }
      word |= (uint32_t)b << (8 * c);
    }
    out[i] = word;
  }
  if (unorm) return FR_TEX_UNORM8;
  for (size_t i = 0; i < n; i++) {
    const float v[3] = {t.data[i].x, t.data[i].y, t.data[i].z};
    if (!same(t.data[i].w, 1.0f)) return FR_TEX_F32;
    const float M = std::max(v[0], std::max(v[1], v[2]));
    uint32_t word = 0;
    if (M > 0.0f) {
      int ex = 0;
      std::frexp(M, &ex);
      const int k = ex - 8, e = k + 136;  // M / 2^k in [128, 256)
      if (e < 1 || e > 255) return FR_TEX_F32;
      const float f = std::ldexp(1.0f, e - 136);
      for (int c = 0; c < 3; c++) {
        const float m = std::ldexp(v[c], -k);
        if (!(m >= 0.0f && m <= 255.0f) || m != std::floor(m) || !same((float)(int)m * f, v[c])) return FR_TEX_F32;
        word |= (uint32_t)m << (8 * c);
      }
      word |= (uint32_t)e << 24;
    } else if (!(same(v[0], 0.0f) && same(v[1], 0.0f) && same(v[2], 0.0f))) {
      return FR_TEX_F32;
    }
    out[i] = word;
  }
  return FR_TEX_RGBE;
}

// The FOVRT_* environment knobs of a context, read once per fr_create; the kernels' launchers take them as arguments.
// (Read where they act instead: the host BVH builder's in scene.cpp, FOVRT_BVH_PHASES in k_bvh.hip, FOVRT_DIAG_DUMP
// in fr_diag_trace_queries, and once per process FOVRT_LAT_OVERLAP in wait_for_previous_frame (ctx_frame.cpp) and
// FOVRT_GROUP_VRING in group.cpp.)
static void read_env_knobs(fr_ctx* c) {
  if (const char* v = getenv("FOVRT_SHADE_CHUNK_REFR")) c->chunk_refr = (uint32_t)std::max(0, atoi(v));
  if (const char* v = getenv("FOVRT_SHADE_XCD_BANDS")) c->xcd_bands = atoi(v) != 0;
  if (const char* v = getenv("FOVRT_SHADE_HANDOFF")) c->handoff = (uint32_t)std::min(std::max(atoi(v), 0), 2);
  if (const char* v = getenv("FOVRT_TEX_PACKING")) c->tex_packing = atoi(v) != 0;  // A/B knob: 0 = RGBA32F textures
  if (const char* v = getenv("FOVRT_JFA_LAZY_OUTPUTS")) c->lazy_jfa_outputs = atoi(v) != 0;  // A/B knob
  if (const char* v = getenv("FOVRT_EARLY_SETUP")) c->early_setup = atoi(v) != 0;            // A/B knob
  if (const char* v = getenv("FOVRT_EXTRA_LAZY")) c->extra_lazy = atoi(v) != 0;  // A/B knob: 0 = every sampling writes EXTRA
  if (const char* v = getenv("FOVRT_SIB_STRIP")) c->sib_strip = atoi(v) != 0;      // A/B knob: 0 = k_sibson_wide for the big discs
  // FOVRT_SLOTS: frame slots of the pipelined loop (2 or 3; A/B knob)
  if (const char* v = getenv("FOVRT_SLOTS")) c->nslots = std::max(2, std::min(fr_ctx::MAX_SLOTS, atoi(v)));
  {  // FOVRT_SHADE_BLOCKS_PER_CU: tuning knob (fewer leaves room for concurrent kernels)
    const char* v = getenv("FOVRT_SHADE_BLOCKS_PER_CU");
    const int full = fr::shade_max_blocks_per_cu();
    c->shade_blocks_per_cu = v ? std::max(1, std::min(full, atoi(v))) : full;
  }
  if (const char* v = getenv("FOVRT_JFA_XCD")) c->jfa_xcd = atoi(v);
  if (const char* v = getenv("FOVRT_JFA_REUSE")) c->jfa_reuse = atoi(v) != 0;  // A/B knob: 0 = every JFA runs its passes
  if (const char* v = getenv("FOVRT_SIB_STRIP_MID")) c->sib_strip_mid = atoi(v);
  if (const char* v = getenv("FOVRT_ATROUS_ROWS2")) c->atrous_rows2 = atoi(v) != 0;
  if (const char* v = getenv("FOVRT_ATROUS_XCD")) c->atrous_xcd = atoi(v) != 0;
  // FOVRT_RAYQ_BLOCKS: a cap on k_ray_queries' grid (0, the default: none), so that a test's few hundred rays make
  // one wave take several chunks
  if (const char* v = getenv("FOVRT_RAYQ_BLOCKS")) c->rayq_blocks = (uint32_t)std::max(0, atoi(v));
}

// The context's events that can be timed (plain hipEventCreate): the stage timing, the ordering events inside a frame
// and latency mode's schedule. fr_create makes them, fr_destroy destroys them.
static std::vector<hipEvent_t*> timed_events(fr_ctx* c) {
  fr_ctx::StageEvents& t = c->tev;
  std::vector<hipEvent_t*> v = {&t.begin, &t.geometry, &t.sampling, &t.optimize, &t.shading, &t.end, &t.paths_begin,
                                &t.paths_end, &t.chain2_begin, &t.pullpush, &t.atrous, &t.chain1_begin, &t.jfa,
                                &t.sibson, &t.stage_begin, &t.stage_end, &c->ev_carry_fork, &c->ev_carry_done,
                                &c->ev_recon_fork, &c->ev_chain2_done, &c->ev_stream_join};
  for (auto& s : c->lat.ev)
    for (hipEvent_t* e : {&s.front_begin, &s.front_end, &s.jfa_end, &s.recon_end}) v.push_back(e);
  return v;
}

int fr_create(const fr_config* cfg_in, fr_ctx** out) {
  if (!out) return fail(nullptr, FR_E_INVALID, "out is NULL");
  *out = nullptr;
  fr_config cfg;
  if (cfg_in) cfg = *cfg_in; else fr_config_default(&cfg);
  if (cfg.abi_version != FOVRT_ABI_VERSION)
    return fail(nullptr, FR_E_INVALID, "fr_config.abi_version != FOVRT_ABI_VERSION (initialise it with fr_config_default)");
  if (cfg.width <= 0 || cfg.height <= 0 || cfg.width > 32767 || cfg.height > 32767)
    return fail(nullptr, FR_E_INVALID, "width/height out of range (1..32767)");
  if (!(cfg.spp == 1 || cfg.spp == 2 || cfg.spp == 4 || cfg.spp == 8))
    return fail(nullptr, FR_E_UNSUPPORTED, "spp must be 1, 2, 4 or 8");
  // (the two steered modes, FR_MASK_ECCENTRIC and FR_MASK_CALLER, are entered with fr_set_mask_mode: a context is
  // created in one of the five reference modes, as it always was)
  if (cfg.mask_mode < 0 || cfg.mask_mode > 4) return fail(nullptr, FR_E_INVALID, "bad mask_mode");
  if (cfg.mesh_mode < 0 || cfg.mesh_mode > 2) return fail(nullptr, FR_E_INVALID, "bad mesh_mode");
  if (cfg.scene < 0 || cfg.scene > 2) return fail(nullptr, FR_E_INVALID, "bad scene preset");
  if (cfg.refraction_max_depth < 0 || cfg.refraction_max_depth > 100) return fail(nullptr, FR_E_INVALID, "bad refraction_max_depth");
  if (cfg.sibson_mode < 0 || cfg.sibson_mode > 1) return fail(nullptr, FR_E_INVALID, "bad sibson_mode");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, FR_E_HIP, "no HIP device available");
  if (cfg.device < 0 || cfg.device >= ndev) return fail(nullptr, FR_E_INVALID, "device ordinal out of range");

  fr_ctx* c = new fr_ctx();
  c->cfg = cfg;
  c->asset_dir = cfg.asset_dir ? cfg.asset_dir : "assets";
  c->cfg.asset_dir = nullptr;
  c->W = cfg.width; c->H = cfg.height;
  auto bail = [&](int code) { g_create_error = c->err; fr_destroy(c); return code; };
  if (hipSetDevice(cfg.device) != hipSuccess) { c->err = "hipSetDevice failed"; return bail(FR_E_HIP); }
  // (this order: five streams share four hardware queues by default)
  for (hipStream_t* st : {&c->stream, &c->atrous_stream, &c->sibson_stream, &c->carry_stream, &c->front_stream}) {
    if (hipStreamCreateWithPriority(st, hipStreamNonBlocking, 0) != hipSuccess) {
      c->err = "stream create failed";
      return bail(FR_E_HIP);
    }
  }
  for (hipEvent_t* e : timed_events(c)) hipEventCreate(e);
  hipEventCreateWithFlags(&c->front_done.ev, hipEventDisableTiming);
  for (auto& f : c->trace_done) hipEventCreateWithFlags(&f.ev, hipEventDisableTiming);
  for (auto& f : c->recon_done) hipEventCreateWithFlags(&f.ev, hipEventDisableTiming);
  for (auto& f : c->jfa_done) hipEventCreateWithFlags(&f.ev, hipEventDisableTiming);
  for (auto& e : c->ev_counts) hipEventCreateWithFlags(&e, hipEventDisableTiming);
  hipEventCreateWithFlags(&c->geo_read.ev, hipEventDisableTiming);
  for (auto& f : c->set_read) hipEventCreateWithFlags(&f.ev, hipEventDisableTiming);
  hipEventCreateWithFlags(&c->update_done.ev, hipEventDisableTiming);
  hipEventCreateWithFlags(&c->rays_done.ev, hipEventDisableTiming);
  hipEventCreateWithFlags(&c->mask_taken.ev, hipEventDisableTiming);
  hipEventCreateWithFlags(&c->mask_read.ev, hipEventDisableTiming);
  read_env_knobs(c);

  std::string err;
  if (!build_preset_scene(cfg.scene, c->asset_dir, cfg.texture_mode, cfg.light_power, cfg.detail, c->scene, err,
                          cfg.mesh_mode)) {
    c->err = "scene: " + err;
    return bail(FR_E_IO);
  }
  if (cfg.bvh_builder < 0 || cfg.bvh_builder > 2) { c->err = "bad bvh_builder"; return bail(FR_E_INVALID); }
  if (cfg.bvh_builder == 0) {
    build_bvh(c->scene, c->bvh);
    if (c->bvh.max_stack > FR_BVH_STACK) {
      c->err = "BVH needs a traversal stack deeper than FR_BVH_STACK";
      return bail(FR_E_UNSUPPORTED);
    }
  }
  const HostScene& s = c->scene;
  const int nt = s.num_tris();
  std::vector<TriShade> shade(nt);
  for (int i = 0; i < nt; i++) {
    TriShade& t = shade[i];
    f3 n0 = s.nrm[3 * i], n1 = s.nrm[3 * i + 1], n2 = s.nrm[3 * i + 2];
    f2 t0 = s.uv[3 * i], t1 = s.uv[3 * i + 1], t2 = s.uv[3 * i + 2];
    t.n0 = mk4(n0, t0.x); t.n1 = mk4(n1, t0.y); t.n2 = mk4(n2, t1.x);
    t.t = mk4(t1.y, t2.x, t2.y, bitsf((uint32_t)s.flags[i]));
  }
  auto up = [&](auto** dst, const auto& vec) -> bool {
    using T = typename std::remove_reference<decltype(vec)>::type::value_type;
    if (dalloc((T**)dst, vec.size()) != hipSuccess) return false;
    return hipMemcpy(*dst, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(&c->d_shade, shade) || !up(&c->d_pos, s.pos) || dalloc(&c->spare_pos, s.pos.size()) != hipSuccess) {
    c->err = "device allocation (scene) failed";
    return bail(FR_E_NOMEM);
  }
  // the record of enqueued updates (fr_update_geometry_enqueue allocates nothing)
  if (dalloc(&c->geo, 1) != hipSuccess || hipMemset(c->geo, 0, sizeof(fr::GeoUpdateState)) != hipSuccess ||
      hipHostMalloc((void**)&c->h_geo, sizeof(fr::GeoUpdateState)) != hipSuccess) {
    c->err = "device allocation (scene) failed";
    return bail(FR_E_NOMEM);
  }
  // the record of enqueued rebuilds (fr_rebuild_bvh_enqueue allocates nothing either)
  if (dalloc(&c->rb, 1) != hipSuccess || hipHostMalloc((void**)&c->h_rb, sizeof(fr::RebuildState)) != hipSuccess) {
    c->err = "device allocation (scene) failed";
    return bail(FR_E_NOMEM);
  }
  // the record of the ray budget (fr_set_foveation allocates nothing), and the parameters a context starts from
  if (dalloc(&c->fov_st, 1) != hipSuccess || hipHostMalloc((void**)&c->h_fov, sizeof(fr::FovState)) != hipSuccess) {
    c->err = "device allocation (scene) failed";
    return bail(FR_E_NOMEM);
  }
  fri::foveation_init(c);
  // the record of ray queries (fr_trace_rays allocates nothing)
  if (dalloc(&c->rq, 1) != hipSuccess) {
    c->err = "device allocation (scene) failed";
    return bail(FR_E_NOMEM);
  }
  {  // the weld and the recompute's scratch exist from the start: an update of the normals allocates nothing
    build_normal_groups(s, c->groups);
    std::string werr;
    if (!normals_work_create(&c->nrm_work, c->groups.corner_vertex.data(), c->groups.vert_off.data(),
                             c->groups.vert_corners.data(), nt, c->groups.num_verts, c->stream, werr)) {
      c->err = werr;
      return bail(FR_E_NOMEM);
    }
  }
  // The tree arrays hold one entry per triangle (room for any device-built tree), and the GPU builder's
  // spare arrays and scratch exist from the start: fr_rebuild_bvh allocates nothing (hipMalloc / hipFree
  // in a rebuild cost ~10-20 ms and synchronise the device).
  {
    const size_t cap = (size_t)std::max(nt, 1);
    if (!fri::tree_alloc(&c->tree, std::max(cap, c->bvh.nodes.size()), cap) || !fri::tree_alloc(&c->spare, cap, cap)) {
      c->err = "device allocation (scene) failed";
      return bail(FR_E_NOMEM);
    }
    c->tree_full_cap = c->bvh.nodes.size() <= cap;
    std::string werr;
    if (nt >= 3 && !bvh_work_prepare(&c->bvh_work, nt, c->stream, werr)) { c->err = werr; return bail(FR_E_NOMEM); }
    // the device SAH builder's scratch, on its contexts alone (the others' footprint does not move); the build
    // below is also that module's first launch
    if (cfg.bvh_builder == 2 && nt >= 3 && !sah_work_create(&c->sah_work, nt, c->stream, werr)) {
      c->err = werr;
      return bail(FR_E_NOMEM);
    }
  }
  if (cfg.bvh_builder == 0) {
    if (hipMemcpy(c->tree.nodes, c->bvh.nodes.data(), c->bvh.nodes.size() * sizeof(BvhNode), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->tree.tri, c->bvh.tri_geo.data(), c->bvh.tri_geo.size() * sizeof(TriGeo), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->tree.prim, c->bvh.tri_prim.data(), c->bvh.tri_prim.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
      c->err = "device copy (scene) failed";
      return bail(FR_E_HIP);
    }
  } else if (int rc = fri::gpu_rebuild(c, c->d_pos)) {
    return bail(rc);
  }
  // The host-built tree's arrays go now, right after their upload, not in the first rebuild. Freeing them
  // (tens of MB, the upload's DMA source) there cost that rebuild 2-6 ms of munmap, and the next GPU
  // submission waited another 7-20 ms before its first kernel started (rocprofv3: the GPU idle with the
  // work queued; profiles/r05_rebuild): the first two rebuilds of every context took 9 and 21 ms
  // (BENCH_r04 bvh.rebuild_ms) instead of 0.8. Here the cost lands in fr_create, which synchronises.
  if (cfg.bvh_builder == 0) {
    c->bvh.host_nodes = (int)c->bvh.nodes.size();
    std::vector<BvhNode>().swap(c->bvh.nodes);
    std::vector<TriGeo>().swap(c->bvh.tri_geo);
    std::vector<int32_t>().swap(c->bvh.tri_prim);
  }
  if (nt >= 3) {
    // the GPU builder's code object is loaded now (HIP loads a module at its first launch: 3-5 ms)
    std::string werr;
    if (!bvh_builder_warm(c->bvh_work, c->stream, werr)) { c->err = werr; return bail(FR_E_HIP); }
  }
  // (the uploads above are synchronous hipMemcpy calls; the builder warm-up ran on c->stream: wait for this
  // context's stream only, not for other contexts or groups rendering on the device)
  if (hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "stream synchronisation (scene) failed"; return bail(FR_E_HIP); }
  DevScene& d = c->dsc;
  memset(&d, 0, sizeof(d));
  fri::point_dsc(c);
  d.root_count = 0; d.num_tris = nt;
  c->d_tex.resize(s.texs.size(), nullptr);
  std::vector<DevTexture> htex(s.texs.size());
  for (size_t i = 0; i < s.texs.size(); i++) {
    std::vector<uint32_t> packed;
    const int kind = c->tex_packing ? pack_texture(s.texs[i], packed) : FR_TEX_F32;
    htex[i] = DevTexture{nullptr, nullptr, s.texs[i].w, s.texs[i].h, kind};
    if (kind == FR_TEX_F32) {
      f4* p = nullptr;
      if (!up(&p, s.texs[i].data)) { c->err = "device allocation (texture) failed"; return bail(FR_E_NOMEM); }
      c->d_tex[i] = p;
      htex[i].data = p;
    } else {
      uint32_t* p = nullptr;
      if (!up(&p, packed)) { c->err = "device allocation (texture) failed"; return bail(FR_E_NOMEM); }
      c->d_tex[i] = p;
      htex[i].packed = p;
    }
  }
  if (!up(&c->d_mats, s.mats) || !up(&c->d_texs, htex)) { c->err = "device allocation (materials) failed"; return bail(FR_E_NOMEM); }
  d.mats = c->d_mats;
  d.texs = c->d_texs;
  d.envmap = s.envmap;
  d.light_position = s.light_position; d.light_v1 = s.light_v1; d.light_v2 = s.light_v2;
  d.light_normal = s.light_normal; d.light_emission = s.light_emission;
  d.light_area = lengthc(cross(s.light_v1, s.light_v2));  // as diffuse.ptx:725-736 computes A (contracted length)
  d.bbox_min = s.bbox_min; d.bbox_max = s.bbox_max;
  d.scene_epsilon = 1.e-3f;

  const size_t N = (size_t)c->W * c->H;
  for (int i = 0; i < P_COUNT; i++)
    if (dalloc(&c->img[i], N) != hipSuccess) { c->err = "device allocation (images) failed"; return bail(FR_E_NOMEM); }
  const size_t nblocks = (size_t)((c->W + 15) / 16) * ((c->H + 15) / 16);
  const size_t nwords = nblocks * 16;  // 4 waves x 4 classes per 16x16 block
  c->pp_S = pp_size(c->W, c->H);
  const size_t atlas = (size_t)c->pp_S * (c->pp_S + c->pp_S / 2);
  if (compaction_tiles(c->W, c->H) > 1024) { c->err = "screen too large for the compaction scan"; return bail(FR_E_UNSUPPORTED); }
  for (int k = 0; k < c->nslots; k++)
    if (dalloc(&c->mask_p[k], N) != hipSuccess || dalloc(&c->ray_count_p[k], 4) != hipSuccess ||
        dalloc(&c->active_p[k], N) != hipSuccess) {
      c->err = "device allocation (work buffers) failed";
      return bail(FR_E_NOMEM);
    }
  c->mask = c->mask_p[0]; c->ray_count = c->ray_count_p[0]; c->active = c->active_p[0];
  for (int k = 0; k < fr_ctx::MAX_SLOTS; k++)
    if (dalloc(&c->owner_counts_p[k], FR_MAX_SHARD_RANKS) != hipSuccess) {
      c->err = "device allocation (work buffers) failed";
      return bail(FR_E_NOMEM);
    }
  if (dalloc(&c->bcount, nblocks) != hipSuccess ||
      hipHostMalloc((void**)&c->h_counts, sizeof(uint32_t) * fr_ctx::MAX_SLOTS * FR_MAX_SHARD_RANKS) != hipSuccess) {
    c->err = "allocation (shard counts) failed";
    return bail(FR_E_NOMEM);
  }
  memset(c->h_counts, 0, sizeof(uint32_t) * fr_ctx::MAX_SLOTS * FR_MAX_SHARD_RANKS);
  if (dalloc(&c->gclass, N) != hipSuccess || dalloc(&c->lp_cache, N) != hipSuccess ||
      dalloc(&c->lp_inv, logpolar_inv_words(c->W, c->H)) != hipSuccess || dalloc(&c->words, nwords) != hipSuccess ||
      dalloc(&c->counts, 4 * nblocks) != hipSuccess || dalloc(&c->offsets, 4 * nblocks) != hipSuccess ||
      dalloc(&c->tiles, 1024) != hipSuccess || dalloc(&c->jfa.G, N) != hipSuccess || dalloc(&c->jfa.H, N) != hipSuccess ||
      dalloc(&c->jfa.F, N) != hipSuccess || dalloc(&c->jfa.seeds, jfa_seed_words(c->W, c->H)) != hipSuccess ||
      dalloc(&c->jfa.ctl, JFA_CTL_WORDS) != hipSuccess ||
      dalloc(&c->pull, atlas) != hipSuccess || dalloc(&c->push, atlas) != hipSuccess ||
      dalloc(&c->snap, pp_snap_count(c->pp_S)) != hipSuccess || dalloc(&c->stats, 1) != hipSuccess ||
      dalloc(&c->shade_ctr, shade_counter_words()) != hipSuccess || dalloc(&c->samples, std::max(N * cfg.spp, 2 * shade_fx_slots((uint32_t)N, cfg.spp, c->handoff, c->shade_blocks_per_cu))) != hipSuccess ||
      dalloc(&c->sample_help, std::max<size_t>(4 * shade_fx_slots((uint32_t)N, cfg.spp, c->handoff, c->shade_blocks_per_cu), 1)) != hipSuccess ||
      dalloc(&c->aux_p[0], N) != hipSuccess || dalloc(&c->aux_seed_p[0], N) != hipSuccess ||
      dalloc(&c->aux_p[1], N) != hipSuccess || dalloc(&c->aux_seed_p[1], N) != hipSuccess ||
      dalloc(&c->hvalid, N / 64 + 1) != hipSuccess ||
      hipMalloc((void**)&c->item_store, shade_item_store_f4(c->shade_blocks_per_cu) * sizeof(f4)) != hipSuccess ||
      (cfg.sibson_mode == 0 && (dalloc(&c->sib_prefix, (size_t)(c->W + 1) * c->H) != hipSuccess ||
                                dalloc(&c->sib_blocks, (size_t)sibson_prefix_blocks(c->W) * c->H) != hipSuccess ||
                                hipMalloc((void**)&c->sib_wide, ((size_t)c->W * c->H + 2) * sizeof(uint32_t)) != hipSuccess ||
                                hipMalloc((void**)&c->sib_strips, sibson_strip_words(c->W, c->H) * sizeof(uint32_t)) != hipSuccess ||
                                dalloc(&c->sib_rowp, sibson_rowp_texels(c->W, c->H)) != hipSuccess))) {
    c->err = "device allocation (work buffers) failed";
    return bail(FR_E_NOMEM);
  }
  c->aux = c->aux_p[0];
  c->aux_seed = c->aux_seed_p[0];
  {  // texel centres in texture coordinates, IEEE-correctly-rounded division as in the kernels
    std::vector<float> ft((size_t)c->W + c->H);
    for (int x = 0; x < c->W; x++) ft[x] = ((float)x + 0.5f) / (float)c->W;
    for (int y = 0; y < c->H; y++) ft[(size_t)c->W + y] = ((float)y + 0.5f) / (float)c->H;
    if (!up(&c->ftab, ft)) { c->err = "device allocation (work buffers) failed"; return bail(FR_E_NOMEM); }
  }
  // Default camera: the preset pose, prev = current.
  FrameUniforms& U = c->U;
  memset(&U, 0, sizeof(U));
  U.width = c->W; U.height = c->H;
  U.screen = mk2((float)c->W, (float)c->H);
  U.diffuse_max_depth = cfg.diffuse_max_depth;
  U.reflection_max_depth = 4;
  U.refraction_max_depth = cfg.refraction_max_depth;
  U.spp = cfg.spp;
  U.sqrt_spp = (int)floor(sqrt((double)cfg.spp) + 1e-9);
  U.mask_mode = cfg.mask_mode;
  U.shard_rank = 0; U.shard_count = 1; U.shard_tile = 128; U.shard_tiles_x = (c->W + 127) / 128; U.shard_map = nullptr;
  U.front_need = nullptr; U.front_pixels = 0;
  {
    fr_camera_pose pose;
    float eye[3], tgt[3], upv[3] = {0, 1, 0};
    fr_preset_camera(cfg.scene, eye, tgt);
    memcpy(pose.pos, eye, sizeof(eye));
    pose.rot[0] = 1; pose.rot[1] = pose.rot[2] = pose.rot[3] = 0;
    pose.fovy_deg = 45.0f; pose.znear = 0.1f; pose.zfar = 500.1f;
    pose.aspect = (float)c->W / (float)c->H;
    fr_camera_look_at(&pose, tgt, upv);
    fr_camera cam;
    fr_camera_uniforms(&pose, &pose, c->W, c->H, &cam);
    fr_set_camera(c, &cam);
  }
  if (hipDeviceSynchronize() != hipSuccess) { c->err = "device sync failed"; return bail(FR_E_HIP); }
  *out = c;
  return FR_OK;
}

int fr_destroy(fr_ctx* c) {
  if (!c) return FR_E_INVALID;
  hipSetDevice(c->cfg.device);
  const hipStream_t streams[5] = {c->stream, c->atrous_stream, c->sibson_stream, c->carry_stream, c->front_stream};
  for (hipStream_t s : streams) if (s) hipStreamSynchronize(s);
  fri::present_destroy(c);  // (waits for the present stream first)
  auto fr = [](void* p) { if (p) hipFree(p); };
  fri::tree_free(&c->tree); fri::tree_free(&c->spare);
  fr(c->d_shade); fr(c->d_pos); fr(c->spare_pos); fr(c->prev_pos); fr(c->shade_back); fr(c->vis_pos);
  fr(c->pose_rest_pos); fr(c->pose_rest_nrm); fr(c->pose_stage_pos); fr(c->pose_stage_nrm);
  if (c->bvh_work) bvh_work_free(c->bvh_work);
  if (c->sah_work) sah_work_free(c->sah_work);
  if (c->nrm_work) normals_work_free(c->nrm_work);
  for (auto p : c->d_tex) fr(p);
  fr(c->d_mats); fr(c->d_texs);
  for (auto p : c->img) fr(p);
  for (int k = 0; k < fr_ctx::MAX_SLOTS; k++) { fr(c->mask_p[k]); fr(c->ray_count_p[k]); fr(c->active_p[k]); fr(c->owner_counts_p[k]); }
  fr(c->bcount); fr(c->shard_map); fr(c->front_need); fr(c->shade_radiance);
  if (c->h_counts) hipHostFree(c->h_counts);
  fr(c->geo);
  if (c->h_geo) hipHostFree(c->h_geo);
  fr(c->rb);
  if (c->h_rb) hipHostFree(c->h_rb);
  fr(c->rq); fr(c->rq_area);
  fr(c->fov_st); fr(c->cmask);
  if (c->h_fov) hipHostFree(c->h_fov);
  if (c->mask_taken.ev) hipEventDestroy(c->mask_taken.ev);
  if (c->mask_read.ev) hipEventDestroy(c->mask_read.ev);
  if (c->rays_done.ev) hipEventDestroy(c->rays_done.ev);
  if (c->geo_read.ev) hipEventDestroy(c->geo_read.ev);
  for (auto& f : c->set_read) if (f.ev) hipEventDestroy(f.ev);
  if (c->update_done.ev) hipEventDestroy(c->update_done.ev);
  for (auto e : c->ev_counts) if (e) hipEventDestroy(e);
  fr(c->gclass); fr(c->lp_cache); fr(c->lp_inv); fr(c->words); fr(c->counts); fr(c->offsets); fr(c->tiles); fr(c->shade_ctr); fr(c->samples); fr(c->sample_help); fr(c->aux_p[0]); fr(c->aux_p[1]); fr(c->aux_seed_p[0]); fr(c->aux_seed_p[1]); fr(c->hvalid); fr(c->item_store); fr(c->jfa.G); fr(c->jfa.H); fr(c->jfa.F); fr(c->jfa.seeds); fr(c->jfa.ctl); fr(c->ftab);
  fr(c->pull); fr(c->push); fr(c->snap); fr(c->stats); fr(c->sib_prefix); fr(c->sib_blocks); fr(c->sib_wide); fr(c->sib_strips); fr(c->sib_rowp);
  for (hipEvent_t* e : timed_events(c)) if (*e) hipEventDestroy(*e);
  if (c->front_done.ev) hipEventDestroy(c->front_done.ev);
  for (auto& f : c->trace_done) if (f.ev) hipEventDestroy(f.ev);
  for (auto& f : c->recon_done) if (f.ev) hipEventDestroy(f.ev);
  for (auto& f : c->jfa_done) if (f.ev) hipEventDestroy(f.ev);
  for (auto& q : c->kt_ev)
    for (auto e : q) if (e) hipEventDestroy(e);
  for (auto& q : c->fc_ev)
    for (auto e : q) if (e) hipEventDestroy(e);
  if (c->fc_ref) hipEventDestroy(c->fc_ref);
  for (hipStream_t s : streams) if (s) hipStreamDestroy(s);
  delete c;
  return FR_OK;
}

int fr_set_camera(fr_ctx* c, const fr_camera* cam) {
  if (!c || !cam) return FR_E_INVALID;
  FrameUniforms& U = c->U;
  memcpy(U.inv_vp.m, cam->inv_vp, sizeof(U.inv_vp.m));
  memcpy(U.prev_vp.m, cam->prev_vp, sizeof(U.prev_vp.m));
  U.eye = mk3(cam->eye[0], cam->eye[1], cam->eye[2]);
  U.prev_eye = mk3(cam->prev_eye[0], cam->prev_eye[1], cam->prev_eye[2]);
  if (!std::isfinite(cam->gaze[0]) || !std::isfinite(cam->gaze[1])) return fail(c, FR_E_INVALID, "fr_set_camera: gaze not finite");
  U.gaze = mk2(cam->gaze[0], cam->gaze[1]);
  return FR_OK;
}

int fr_set_light_power(fr_ctx* c, float power) {
  if (!c) return FR_E_INVALID;
  c->dsc.light_emission = mk3(power);
  c->light_pending = true;
  return FR_OK;
}

int fr_set_diffuse_max_depth(fr_ctx* c, int depth) {
  if (!c || depth < 0) return FR_E_INVALID;
  c->U.diffuse_max_depth = depth;
  return FR_OK;
}

int fr_reset_accumulation(fr_ctx* c) {
  if (!c) return FR_E_INVALID;
  c->accum = 0;
  return FR_OK;
}

int fr_accum_frame(fr_ctx* c, uint32_t* f) {
  if (!c || !f) return FR_E_INVALID;
  *f = c->accum;
  return FR_OK;
}

// Test hook (not part of include/fovrt.h): pack_texture on n RGBA32F texels; returns the FR_TEX_* kind
// and writes the packed words (n of them) for the packed kinds.
int fr__pack_texture(const float* rgba, int n, uint32_t* out) {
  if (!rgba || n < 0 || !out) return -1;
  HostTexture t;
  t.w = n; t.h = 1;
  t.data.resize((size_t)n);
  memcpy(t.data.data(), rgba, sizeof(f4) * (size_t)n);
  std::vector<uint32_t> packed;
  const int kind = pack_texture(t, packed);
  if (kind != FR_TEX_F32) memcpy(out, packed.data(), sizeof(uint32_t) * (size_t)n);
  return kind;
}

}  // extern "C"
