// ctx_shard.cpp — tile sharding of one view over several contexts: the plan (which rank owns which tile), the
// tile-local front stages, and the slabs ranks exchange (whole tiles, or the active pixels only).
#include <algorithm>
#include <cmath>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

// The checks and the launch of fr_shard_unpack_active and its enqueue form (join: after the pending reconstruction).
static int unpack_active(fr_ctx* c, const void* slab, size_t slab_bytes, uint32_t capacity, uint32_t count, bool join) {
  if (!c || !slab) return FR_E_INVALID;
  if (count > capacity) return fail(c, FR_E_INVALID, "fr_shard_unpack_active: count above capacity");
  if (slab_bytes < (size_t)capacity * 20) return fail(c, FR_E_INVALID, "fr_shard_unpack_active: slab smaller than 20 * capacity");
  if (join) join_recon(c);
  hipSetDevice(c->cfg.device);
  const f4* vals = (const f4*)slab;
  const uint32_t* idx = (const uint32_t*)((const char*)slab + (size_t)capacity * sizeof(f4));
  launch_shard_unpack_active(c->U, vals, idx, count, (uint32_t)((size_t)c->W * c->H), c->img[P_wgt(c)],
                             c->img[c->hist_cur], c->img[c->hist_cache], c->img[P_shd(c)], c->stream);
  c->hvalid_fresh = false;
  return FR_OK;
}

extern "C" {

int fr_shard_unpack_active_enqueue(fr_ctx* c, const void* slab, size_t slab_bytes, uint32_t capacity, uint32_t count) {
  if (int rc = unpack_active(c, slab, slab_bytes, capacity, count, false)) return rc;
  // the unpack reads the slot's WEIGHT: the front stages of frame + nslots (front_stream waits for trace_done[slot])
  // may overwrite it only after this launch
  c->trace_done[c->slot].record(c->stream);
  return check_launch(c);
}

int fr_shard_plan(int W, int H, int tile, int count, const float* weights, uint8_t* owner, size_t ntiles) {
  if (W <= 0 || H <= 0 || tile < 16 || tile % 16 || count < 1 || count > FR_MAX_SHARD_RANKS || !owner)
    return fail(nullptr, FR_E_INVALID, "fr_shard_plan: need W, H > 0, tile a multiple of 16, 1 <= count <= 64");
  const size_t nt = (size_t)((W + tile - 1) / tile) * ((H + tile - 1) / tile);
  if (ntiles != nt) return fail(nullptr, FR_E_INVALID, "fr_shard_plan: ntiles != ceil(W/tile) * ceil(H/tile)");
  std::vector<double> w(count, 1.0);
  double sum = count;
  if (weights) {
    sum = 0.0;
    for (int r = 0; r < count; r++) {
      if (!(weights[r] >= 0.0f) || !std::isfinite(weights[r])) return fail(nullptr, FR_E_INVALID, "fr_shard_plan: bad weight");
      w[r] = weights[r];
      sum += w[r];
    }
    if (sum <= 0.0) return fail(nullptr, FR_E_INVALID, "fr_shard_plan: all weights are 0");
  }
  // smooth weighted round robin (raster order): every step each rank earns its weight, the richest
  // rank (lowest rank on ties) takes the tile and pays the total
  std::vector<double> cur(count, 0.0);
  for (size_t t = 0; t < nt; t++) {
    int best = -1;
    for (int r = 0; r < count; r++) {
      if (w[r] <= 0.0) continue;
      cur[r] += w[r];
      if (best < 0 || cur[r] > cur[best]) best = r;
    }
    cur[best] -= sum;
    owner[t] = (uint8_t)best;
  }
  return FR_OK;
}

// The 8x8 tiles a tile-local front computes: an owned 16x16 block's saliency cells (origins 4 px apart)
// read taps 4 px beyond their origin, so block b's stencil covers pixels [16b - 4, 16b + 16] on each
// axis. The left half of block k is read by blocks k-1 and k, the right half by k and k+1.
static int update_front_need(fr_ctx* c) {
  if (!c->front_local) {
    c->U.front_need = nullptr;
    return FR_OK;
  }
  const int tx8 = (c->W + 7) / 8, ty8 = (c->H + 7) / 8;
  const int bx = (c->W + 15) / 16, by = (c->H + 15) / 16;
  const int T = c->U.shard_tile;
  auto owned = [&](int X, int Y) {
    if (X < 0 || Y < 0 || X >= bx || Y >= by) return false;
    return c->shard_owner[(size_t)((Y * 16) / T) * c->U.shard_tiles_x + (X * 16) / T] == c->U.shard_rank;
  };
  c->front_need_h.assign((size_t)tx8 * ty8, 0);
  c->front_need_px = 0;
  for (int j = 0; j < ty8; j++)
    for (int i = 0; i < tx8; i++) {
      const int X = i >> 1, Y = j >> 1, dx = (i & 1) ? 1 : -1, dy = (j & 1) ? 1 : -1;
      const bool need = owned(X, Y) || owned(X + dx, Y) || owned(X, Y + dy) || owned(X + dx, Y + dy);
      if (!need) continue;
      c->front_need_h[(size_t)j * tx8 + i] = 1;
      c->front_need_px += (uint32_t)(std::min(8, c->W - i * 8) * std::min(8, c->H - j * 8));
    }
  if (!c->front_need) HIP_TRY(c, hipMalloc((void**)&c->front_need, c->front_need_h.size()));
  HIP_TRY(c, hipMemcpy(c->front_need, c->front_need_h.data(), c->front_need_h.size(), hipMemcpyHostToDevice));
  c->U.front_need = c->front_need;
  return FR_OK;
}

int fr_set_shard_plan(fr_ctx* c, int rank, int count, int tile, const uint8_t* owner, size_t ntiles) {
  if (!c) return FR_E_INVALID;
  if (count < 1 || count > FR_MAX_SHARD_RANKS || rank < 0 || rank >= count || tile < 16 || tile % 16 || tile > 4096)
    return fail(c, FR_E_INVALID, "fr_set_shard: need 0 <= rank < count <= 64 and tile a multiple of 16 in 16..4096");
  const int tx = (c->W + tile - 1) / tile, ty = (c->H + tile - 1) / tile;
  const size_t nt = (size_t)tx * ty;
  if (count > 1 && (!owner || ntiles != nt))
    return fail(c, FR_E_INVALID, "fr_set_shard_plan: owner must hold ceil(W/tile) * ceil(H/tile) entries");
  std::vector<uint32_t> map(nt, 0);
  std::vector<uint32_t> next(count, 0);
  if (count > 1)
    for (size_t t = 0; t < nt; t++) {
      if (owner[t] >= count) return fail(c, FR_E_INVALID, "fr_set_shard_plan: owner out of range");
      map[t] = (uint32_t)owner[t] << 24 | next[owner[t]]++;
    }
  c->extra.settle(c);  // a sharded context's unpack calls write the images an owed EXTRA reads
  if (int rc = quiesce(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->front_stream));
  // the new map is complete before the old one goes: a failed allocation or copy leaves the previous
  // plan (map, owners, uniforms) in force
  uint32_t* new_map = nullptr;
  if (count > 1) {
    // a sharded rank's traced radiance (k_shade_resolve, active order): what it sends (fr_shard_pack_active)
    if (!c->shade_radiance && dalloc(&c->shade_radiance, (size_t)c->W * c->H) != hipSuccess) {
      c->shade_radiance = nullptr;
      return fail(c, FR_E_NOMEM, "fr_set_shard_plan: device allocation failed, previous plan kept");
    }
    if (hipMalloc((void**)&new_map, nt * sizeof(uint32_t)) != hipSuccess)
      return fail(c, FR_E_NOMEM, "fr_set_shard_plan: device allocation failed, previous plan kept");
    if (hipMemcpy(new_map, map.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
      hipFree(new_map);
      return fail(c, FR_E_HIP, "fr_set_shard_plan: device copy failed, previous plan kept");
    }
  }
  if (c->shard_map) hipFree(c->shard_map);
  c->shard_map = new_map;
  c->shard_owner.clear();
  if (count > 1) c->shard_owner.assign(owner, owner + nt);
  // counts of the previous plan are stale (fr_shard_counts refuses until a front stage ran under this one)
  for (bool& v : c->counts_valid) v = false;
  memset(c->h_counts, 0, sizeof(uint32_t) * fr_ctx::MAX_SLOTS * FR_MAX_SHARD_RANKS);
  c->U.shard_rank = rank;
  c->U.shard_count = count;
  c->U.shard_tile = tile;
  c->U.shard_tiles_x = tx;
  c->U.shard_map = c->shard_map;
  c->compacted = false;
  if (count == 1) c->front_local = false;
  return update_front_need(c);
}

int fr_set_front_local(fr_ctx* c, int on) {
  if (!c) return FR_E_INVALID;
  if (on != 0 && on != 1) return fail(c, FR_E_INVALID, "fr_set_front_local: on is 0 or 1");
  if (on && c->U.shard_count <= 1) return fail(c, FR_E_STATE, "fr_set_front_local: needs a shard plan with count > 1");
  if ((bool)on == c->front_local) return FR_OK;
  if (int rc = quiesce(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->front_stream));
  c->front_local = on != 0;
  c->compacted = false;
  return update_front_need(c);
}

int fr_set_shard_ex(fr_ctx* c, int rank, int count, int tile, int first_tracer) {
  if (!c) return FR_E_INVALID;
  if (first_tracer < 0 || (count > 1 && first_tracer >= count) || (count == 1 && first_tracer != 0))
    return fail(c, FR_E_INVALID, "fr_set_shard_ex: need 0 <= first_tracer < count (at least one tracing rank)");
  if (count < 1 || tile < 16 || tile % 16) return fail(c, FR_E_INVALID, "fr_set_shard: need count >= 1 and tile a multiple of 16");
  const size_t nt = (size_t)((c->W + tile - 1) / tile) * ((c->H + tile - 1) / tile);
  std::vector<uint8_t> owner(nt);
  for (size_t t = 0; t < nt; t++) owner[t] = (uint8_t)(first_tracer + t % (size_t)(count - first_tracer));
  return fr_set_shard_plan(c, rank, count, tile, owner.data(), nt);
}
int fr_set_shard(fr_ctx* c, int rank, int count, int tile) { return fr_set_shard_ex(c, rank, count, tile, 0); }

int fr_shard_counts(fr_ctx* c, uint32_t* counts, int n) {
  if (!c || !counts || n < 1) return FR_E_INVALID;
  if (c->U.shard_count <= 1) return fail(c, FR_E_STATE, "fr_shard_counts: call fr_set_shard with count > 1 first");
  if (!c->counts_valid[c->slot])
    return fail(c, FR_E_STATE, "fr_shard_counts: no front stage has run under the current shard plan");
  HIP_TRY(c, hipEventSynchronize(c->ev_counts[c->slot]));
  for (int r = 0; r < n; r++) counts[r] = r < c->U.shard_count ? c->h_counts[(size_t)c->slot * FR_MAX_SHARD_RANKS + r] : 0;
  return FR_OK;
}

int fr_shard_texels(fr_ctx* c, size_t* texels) {
  if (!c || !texels) return FR_E_INVALID;
  const int T = c->U.shard_count > 1 ? c->U.shard_tile : 0;
  if (!T) { *texels = (size_t)c->W * c->H; return FR_OK; }
  // the largest tile count of any rank (slabs of every rank have one size)
  std::vector<size_t> per(c->U.shard_count, 0);
  for (uint8_t o : c->shard_owner) per[o]++;
  size_t mx = 0;
  for (size_t v : per) mx = std::max(mx, v);
  *texels = std::max<size_t>(mx, 1) * (size_t)T * T;
  return FR_OK;
}

static int shard_io(fr_ctx* c, int id, int rank, void* slab, size_t bytes, bool pack) {
  if (!c || !slab) return FR_E_INVALID;
  if (c->U.shard_count <= 1) return fail(c, FR_E_STATE, "fr_shard_*: call fr_set_shard with count > 1 first");
  if (rank < 0 || rank >= c->U.shard_count) return fail(c, FR_E_INVALID, "fr_shard_unpack: bad source rank");
  join_recon(c);
  int p;
  if (resolve(c, id, &p)) return fail(c, FR_E_INVALID, "fr_shard_*: buffer is not an RGBA32F image");
  size_t texels = 0;
  fr_shard_texels(c, &texels);
  if (bytes < texels * sizeof(f4)) return fail(c, FR_E_INVALID, "fr_shard_*: slab smaller than fr_shard_texels * 16");
  hipSetDevice(c->cfg.device);
  if (pack) launch_shard_pack(c->U, c->img[p], (f4*)slab, c->stream);
  else launch_shard_unpack(c->U, rank, (const f4*)slab, c->img[p], c->stream);
  if (int rc = check_launch(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}
int fr_shard_pack(fr_ctx* c, int id, void* slab, size_t bytes) {
  return shard_io(c, id, c ? c->U.shard_rank : 0, slab, bytes, true);
}
int fr_shard_unpack(fr_ctx* c, int id, int src_rank, const void* slab, size_t bytes) {
  return shard_io(c, id, src_rank, const_cast<void*>(slab), bytes, false);
}

int fr_shard_pack_active(fr_ctx* c, void* slab, size_t slab_bytes, uint32_t capacity, uint32_t* count) {
  if (!c || !slab || !count) return FR_E_INVALID;
  if (c->U.shard_count <= 1) return fail(c, FR_E_STATE, "fr_shard_*: call fr_set_shard with count > 1 first");
  if (slab_bytes < (size_t)capacity * 20) return fail(c, FR_E_INVALID, "fr_shard_pack_active: slab smaller than 20 * capacity");
  join_recon(c);
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, hipMemcpyAsync(count, c->ray_count, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*count > capacity) return fail(c, FR_E_INVALID, "fr_shard_pack_active: capacity below the active pixel count");
  f4* vals = (f4*)slab;
  uint32_t* idx = (uint32_t*)((char*)slab + (size_t)capacity * sizeof(f4));
  launch_shard_pack_active(c->active, c->ray_count, capacity, c->shade_radiance, vals, idx, c->stream);
  if (int rc = check_launch(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

int fr_shard_unpack_active(fr_ctx* c, const void* slab, size_t slab_bytes, uint32_t capacity, uint32_t count) {
  if (int rc = unpack_active(c, slab, slab_bytes, capacity, count, true)) return rc;
  if (int rc = check_launch(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

}  // extern "C"
