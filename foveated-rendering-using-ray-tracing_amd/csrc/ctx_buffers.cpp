// ctx_buffers.cpp — the caller's side of the image buffers: views, reads, writes and copies (the lazy outputs JFA_COORD
// and EXTRA are written when a call names them or what they read), small read-backs, snapshot / restore.
#include <algorithm>
#include <array>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

// ---- Snapshot / restore of the temporal state (deterministic multi-frame golden tests) ----
// What a frame carries into the next one: the history and depth ping-pong pairs (FR/PathTracer.cpp:226-238),
// the pull / push atlases and the push pass's snapshot texels (the push reads the previous frame's atlas,
// FR/PullPushInterpolation.cpp:57-58), the m_accumFrame counter with its pending light reset, the light
// emission, and the camera / gaze uniforms of the last update. Everything else a frame reads it writes first.
// Layout: a fixed header, then the buffers in the order below (cache before current of each pair).
namespace {
constexpr uint32_t kSnapMagic = 0x4E535246u;  // "FRSN"
constexpr uint32_t kSnapVersion = 1;
struct SnapHeader {
  uint32_t magic, version;
  int32_t width, height, pp_S, spp, scene, mask_mode;
  uint32_t accum, light_pending;
  float light_emission[3];
  int32_t diffuse_max_depth;
  float inv_vp[16], prev_vp[16], eye[3], prev_eye[3], gaze[2];
  uint64_t payload_bytes;
};
struct SnapPart {
  void* dev;
  size_t bytes;
};
std::array<SnapPart, 7> snap_parts(fr_ctx* c) {
  const size_t img = (size_t)c->W * c->H * sizeof(f4);
  const size_t atlas = (size_t)c->pp_S * (c->pp_S + c->pp_S / 2) * sizeof(f4);
  return {{{c->img[c->hist_cache], img}, {c->img[c->hist_cur], img}, {c->img[c->depth_cache], img},
           {c->img[c->depth_cur], img}, {c->pull, atlas}, {c->push, atlas},
           {c->snap, pp_snap_count(c->pp_S) * sizeof(f4)}}};
}
size_t snap_total(fr_ctx* c) {
  size_t n = sizeof(SnapHeader);
  for (const SnapPart& p : snap_parts(c)) n += p.bytes;
  return n;
}
}  // namespace

extern "C" {

static int buffer_view(fr_ctx* c, int id, fr_buffer_view* v) {
  if (!c || !v) return FR_E_INVALID;
  join_recon(c);  // later work on the context stream is ordered after the reconstruction
  const size_t N = (size_t)c->W * c->H;
  int p;
  if (id == FR_BUF_THREAD) *v = fr_buffer_view{c->active, (int)N, 1, N * 4, N * 4, FR_FMT_U32};
  else if (id == FR_BUF_MASK) *v = fr_buffer_view{c->mask, c->W, c->H, (size_t)c->W, N, FR_FMT_U8};
  else if (id == FR_BUF_GCLASS) *v = fr_buffer_view{c->gclass, c->W, c->H, (size_t)c->W, N, FR_FMT_U8};
  else if (resolve(c, id, &p)) return fail(c, FR_E_INVALID, "unknown buffer id");
  else *v = fr_buffer_view{c->img[p], c->W, c->H, (size_t)c->W * sizeof(f4), N * sizeof(f4), FR_FMT_RGBA32F};
  return FR_OK;
}

int fr_copy_buffer(fr_ctx* c, int id, void* dst, size_t bytes) {
  fr_buffer_view v;
  if (int rc = buffer_view(c, id, &v)) return rc;
  if (!dst || bytes > v.bytes) return fail(c, FR_E_INVALID, "copy_buffer: size");
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, hipMemcpyAsync(dst, v.device_ptr, bytes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

int fr_composite_views(fr_ctx* c, const void* views, int nviews, void* out, size_t out_bytes) {
  if (!c || !views || !out || nviews < 1) return FR_E_INVALID;
  const size_t need = (size_t)nviews * c->W * c->H * sizeof(f4);
  if (out_bytes < need) return fail(c, FR_E_INVALID, "fr_composite_views: output smaller than nviews * W * H * 16");
  join_recon(c);
  hipSetDevice(c->cfg.device);
  launch_composite((const f4*)views, nviews, c->W, c->H, (f4*)out, c->stream);
  if (int rc = check_launch(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

int fr_synchronize(fr_ctx* c) {
  if (!c) return FR_E_INVALID;
  join_recon(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return present_sync(c);  // (a context that presents: the packs and copies to the host enqueued so far as well)
}

int fr_ray_count(fr_ctx* c, uint32_t* n) {
  if (!c || !n) return FR_E_INVALID;
  join_recon(c);
  HIP_TRY(c, hipMemcpyAsync(n, c->ray_count, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

int fr_gaze_target(fr_ctx* c, float xyz[3]) {
  // gaze_target[0] = position_buffer[make_uint2(gaze)] (samplingStep.cu:184)
  if (!c || !xyz) return FR_E_INVALID;
  join_recon(c);
  // same texel as the sampling kernel's focal-depth read: saturating conversion, clamped to the screen
  const uint32_t gx = std::min(f2u_sat(c->U.gaze.x), (uint32_t)c->W - 1), gy = std::min(f2u_sat(c->U.gaze.y), (uint32_t)c->H - 1);
  f4 v;
  HIP_TRY(c, hipMemcpyAsync(&v, c->img[P_pos(c)] + (size_t)gy * c->W + gx, sizeof(f4), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  xyz[0] = v.x; xyz[1] = v.y; xyz[2] = v.z;
  return FR_OK;
}

int fr_get_buffer(fr_ctx* c, int id, fr_buffer_view* v) {
  bool owed = c && c->jfa_coord_owed && (id == FR_BUF_JFA_COLOR || id == FR_BUF_JFA_COORD);
  // a view of EXTRA: from now on every sampling writes it (the caller reads through the pointer without a call).
  // A view of something the owed heat map reads: the caller may write through it, so EXTRA is written first.
  int p;
  if (c && c->extra.owed && (id == FR_BUF_EXTRA || (resolve(c, id, &p) == FR_OK && c->extra.reads(p)))) {
    c->extra.settle(c);
    owed = true;
  }
  const int rc = buffer_view(c, id, v);
  if (rc == FR_OK && id == FR_BUF_EXTRA) c->extra_lazy = false;
  // a view handed out after its image was written on demand: that write is complete when the call returns (the
  // caller may read through the pointer on any stream)
  if (rc == FR_OK && owed) HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the caller may write the JFA outputs through the view: Sibson then derives its seeds and row prefix sums
  // from them again instead of from the JFA run's own state
  if (rc == FR_OK && (id == FR_BUF_JFA_COLOR || id == FR_BUF_JFA_COORD)) retire_sibson_prefix(c);
  // ... and the history: the next frame's sample setup then reads it, not the validity bits of what the last frame left
  if (rc == FR_OK && (id == FR_BUF_HISTORY || id == FR_BUF_HISTORY_CACHE)) c->hvalid_fresh = false;
  return rc;
}

int fr_read_buffer(fr_ctx* c, int id, void* host, size_t bytes) {
  fr_buffer_view v;
  if (int rc = buffer_view(c, id, &v)) return rc;
  if (!host || bytes > v.bytes) return fail(c, FR_E_INVALID, "read_buffer: size");
  HIP_TRY(c, hipMemcpyAsync(host, v.device_ptr, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

int fr_write_buffer(fr_ctx* c, int id, const void* host, size_t bytes) {
  fr_buffer_view v;
  if (c && c->extra.owed) {
    // a whole EXTRA from the caller replaces the owed heat map; a write of something the heat map reads comes after it
    int p;
    if (id == FR_BUF_EXTRA && host && bytes == (size_t)c->W * c->H * sizeof(f4)) c->extra.owed = false;
    else if (id != FR_BUF_EXTRA && resolve(c, id, &p) == FR_OK && c->extra.reads(p)) c->extra.settle(c);
  }
  if (int rc = buffer_view(c, id, &v)) return rc;
  if (!host || bytes > v.bytes) return fail(c, FR_E_INVALID, "write_buffer: size");
  HIP_TRY(c, hipMemcpyAsync(v.device_ptr, host, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // Sibson's row prefix sums (and the JFA state it reads its seeds from) no longer match these
  if (id == FR_BUF_JFA_COLOR || id == FR_BUF_JFA_COORD) retire_sibson_prefix(c);
  if (id == FR_BUF_HISTORY || id == FR_BUF_HISTORY_CACHE) c->hvalid_fresh = false;
  if (id == FR_BUF_MASK) {
    // a host-written mask must also drive the compaction: rebuild the wave ballots from it
    c->compacted = false;
    c->mask_dirty = true;
  }
  return FR_OK;
}

int fr_snapshot_bytes(fr_ctx* c, size_t* bytes) {
  if (!c || !bytes) return FR_E_INVALID;
  *bytes = snap_total(c);
  return FR_OK;
}

int fr_snapshot(fr_ctx* c, void* host, size_t bytes) {
  if (!c) return FR_E_INVALID;
  const size_t need = snap_total(c);
  if (!host || bytes < need) return fail(c, FR_E_INVALID, "snapshot: buffer smaller than fr_snapshot_bytes");
  if (int rc = tree_numbers(c)) return rc;  // (behind an enqueued rebuild: the host's copy of the tree's numbers)
  join_recon(c);
  hipSetDevice(c->cfg.device);
  SnapHeader h{};
  h.magic = kSnapMagic; h.version = kSnapVersion;
  h.width = c->W; h.height = c->H; h.pp_S = c->pp_S; h.spp = c->U.spp; h.scene = c->cfg.scene;
  h.mask_mode = c->U.mask_mode;
  h.accum = c->accum; h.light_pending = c->light_pending ? 1u : 0u;
  h.light_emission[0] = c->dsc.light_emission.x; h.light_emission[1] = c->dsc.light_emission.y;
  h.light_emission[2] = c->dsc.light_emission.z;
  h.diffuse_max_depth = c->U.diffuse_max_depth;
  memcpy(h.inv_vp, &c->U.inv_vp, sizeof(h.inv_vp));
  memcpy(h.prev_vp, &c->U.prev_vp, sizeof(h.prev_vp));
  memcpy(h.eye, &c->U.eye, sizeof(h.eye));
  memcpy(h.prev_eye, &c->U.prev_eye, sizeof(h.prev_eye));
  memcpy(h.gaze, &c->U.gaze, sizeof(h.gaze));
  h.payload_bytes = need - sizeof(SnapHeader);
  char* out = static_cast<char*>(host);
  memcpy(out, &h, sizeof(h));
  size_t off = sizeof(h);
  for (const SnapPart& p : snap_parts(c)) {
    HIP_TRY(c, hipMemcpyAsync(out + off, p.dev, p.bytes, hipMemcpyDeviceToHost, c->stream));
    off += p.bytes;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

int fr_restore(fr_ctx* c, const void* host, size_t bytes) {
  if (!c) return FR_E_INVALID;
  const size_t need = snap_total(c);
  if (!host || bytes < need) return fail(c, FR_E_INVALID, "restore: buffer smaller than fr_snapshot_bytes");
  SnapHeader h;
  memcpy(&h, host, sizeof(h));
  if (h.magic != kSnapMagic || h.version != kSnapVersion) return fail(c, FR_E_INVALID, "restore: not a fovrt snapshot");
  if (h.width != c->W || h.height != c->H || h.pp_S != c->pp_S || h.spp != c->U.spp || h.scene != c->cfg.scene ||
      h.payload_bytes != need - sizeof(SnapHeader))
    return fail(c, FR_E_INVALID, "restore: snapshot of another configuration (size, spp or scene differ)");
  c->extra.settle(c);  // the depth pair is overwritten below: an owed EXTRA is written from the old one first
  join_recon(c);
  hipSetDevice(c->cfg.device);
  // The next Sibson derives its seeds and row prefix sums from the JFA outputs again: a JFA_COORD the last JumpFlooding
  // still owes is written now, from that run's final state (a restore touches neither JFA output), ahead of the
  // synchronize below.
  retire_sibson_prefix(c);
  const char* in = static_cast<const char*>(host);
  size_t off = sizeof(h);
  for (const SnapPart& p : snap_parts(c)) {
    HIP_TRY(c, hipMemcpyAsync(p.dev, in + off, p.bytes, hipMemcpyHostToDevice, c->stream));
    off += p.bytes;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->accum = h.accum;
  c->light_pending = h.light_pending != 0;
  c->dsc.light_emission = mk3(h.light_emission[0], h.light_emission[1], h.light_emission[2]);
  c->U.diffuse_max_depth = h.diffuse_max_depth;
  c->U.mask_mode = h.mask_mode;
  memcpy(&c->U.inv_vp, h.inv_vp, sizeof(h.inv_vp));
  memcpy(&c->U.prev_vp, h.prev_vp, sizeof(h.prev_vp));
  memcpy(&c->U.eye, h.eye, sizeof(h.eye));
  memcpy(&c->U.prev_eye, h.prev_eye, sizeof(h.prev_eye));
  memcpy(&c->U.gaze, h.gaze, sizeof(h.gaze));
  c->lp_gaze = f2{-1e30f, -1e30f};  // the log-polar mask cache is recomputed for the restored gaze
  c->lp_mode = -1;
  c->jfa_force = true;  // a snapshot carries no JFA state: the next JumpFlooding runs its passes, not what this context retained
  c->hvalid_fresh = false;
  c->moved = false;  // a snapshot carries no previous positions: the next G-buffer reprojects as over still geometry
  return FR_OK;
}

}  // extern "C"
