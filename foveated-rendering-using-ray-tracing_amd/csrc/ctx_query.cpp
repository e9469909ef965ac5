// ctx_query.cpp — ray queries: a caller's batch of rays against the scene as of the call's place in the stream order
// (fr_trace_rays, fr_trace_rays_enqueue, their masked forms, fr_rays_consumed, fr_ray_query_reserve[_kind]; the
// kernels are k_ray_queries and k_ray_surface in k_trace.hip). A query reads the scene (tree, leaf triangles,
// primitive map, shading records, materials, textures) and the caller's rays and masks, and writes the caller's
// results and the context's query record (rq); it touches no image buffer, no temporal state, no counter of fr_stats
// and no JFA state.
#include <climits>
#include <cstdint>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

static_assert(sizeof(fr_ray) == 32 && sizeof(fr_ray_hit) == 16, "the kernel reads 32-B rays and writes 16-B hits");
static_assert(sizeof(fr_ray_surface) == 80 && offsetof(fr_ray_surface, model) == 28 && offsetof(fr_ray_surface, ng) == 32 &&
                  offsetof(fr_ray_surface, v) == 60 && offsetof(fr_ray_surface, surface) == 76,
              "k_ray_surface writes five 16-B rows");
static_assert(FR_MAX_MODELS == FR_POSE_MAX_MODELS, "the query kernels' arguments hold FR_MAX_MODELS boundaries");

#define FR_RAYS_MAX ((size_t)1 << 30)

static bool kind_ok(int kind) {
  return kind == FR_RAYS_CLOSEST || kind == FR_RAYS_TRANSMITTANCE || kind == FR_RAYS_SURFACE;
}
static size_t out_stride(int kind) {
  return kind == FR_RAYS_CLOSEST ? sizeof(fr_ray_hit) : kind == FR_RAYS_SURFACE ? sizeof(fr_ray_surface) : sizeof(float);
}
// Bytes of the staging area a host batch of n rays takes: rays, results, masks, in that order.
static size_t area_bytes(size_t n, int kind, bool masked) {
  return n * (sizeof(fr_ray) + out_stride(kind) + (masked ? sizeof(uint32_t) : 0));
}

// What every form refuses before anything is enqueued (n > 0; device: the arrays are device memory). surface_ok: the
// masked calls, which know FR_RAYS_SURFACE; fr_trace_rays and fr_trace_rays_enqueue keep their two kinds.
static int check_query_args(fr_ctx* c, const std::string& name, const void* rays, const uint32_t* masks, size_t n,
                            int kind, const void* out, bool device, bool surface_ok) {
  if (!kind_ok(kind) || (kind == FR_RAYS_SURFACE && !surface_ok)) return fail(c, FR_E_INVALID, name + ": bad kind");
  if (n > FR_RAYS_MAX) return fail(c, FR_E_INVALID, name + ": more than 2^30 rays");
  if (n == 0) return FR_OK;
  if (!rays || !out) return fail(c, FR_E_INVALID, name + ": rays or out is NULL");
  const uintptr_t r = reinterpret_cast<uintptr_t>(rays), o = reinterpret_cast<uintptr_t>(out),
                  m = reinterpret_cast<uintptr_t>(masks);
  if (device && ((r & 15u) || (o & (kind == FR_RAYS_TRANSMITTANCE ? 3u : 15u)) || (m & 3u)))
    return fail(c, FR_E_INVALID, name + ": a device pointer is not aligned (rays, hits and surface records: 16 bytes, "
                                        "transmittance and masks: 4)");
  if (r < o + n * out_stride(kind) && o < r + n * sizeof(fr_ray))
    return fail(c, FR_E_INVALID, name + ": rays and out overlap");
  if (masks && m < o + n * out_stride(kind) && o < m + n * sizeof(uint32_t))
    return fail(c, FR_E_INVALID, name + ": masks and out overlap");
  if ((masks || kind == FR_RAYS_SURFACE) && c->scene.model_tri_count.size() > FR_MAX_MODELS)
    return fail(c, FR_E_UNSUPPORTED, name + ": the scene has more than FR_MAX_MODELS models");
  return FR_OK;
}

// The scene's model boundaries as the query kernels take them (unused slots: INT_MAX, as PoseArgs).
static RayModels ray_models(fr_ctx* c) {
  RayModels rm;
  const size_t nm = std::min<size_t>(c->scene.model_tri_count.size(), FR_MAX_MODELS);
  for (size_t i = 0; i < FR_MAX_MODELS; i++) {
    rm.first_tri[i] = INT_MAX;
    if (i < nm) model_info(c->scene, (int)i, nullptr, &rm.first_tri[i], nullptr);
  }
  rm.valid = nm >= 32 ? 0xFFFFFFFFu : (1u << nm) - 1u;
  return rm;
}

// The launch, on the context stream, over the scene current at the call (dsc, as frames take it).
static int launch_query(fr_ctx* c, const void* rays, const uint32_t* masks, size_t n, int kind, void* out) {
  launch_ray_queries(c->dsc, rays, masks, (uint32_t)n, kind, out, c->rq, ray_models(c), c->rayq_blocks, c->stream);
  return check_launch(c);
}

// Grows the staging area to `bytes` (never shrinks it); rays: the request, for the error text.
static int reserve_area(fr_ctx* c, const std::string& name, size_t bytes) {
  if (int rc = quiesce(c)) return rc;  // (a query may still read the staging area about to be replaced)
  if (bytes <= c->rq_bytes) return FR_OK;
  void* na = nullptr;
  if (hipMalloc(&na, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, FR_E_NOMEM, name + ": device allocation failed (the reservation stays at " +
                                   std::to_string(c->rq_cap) + " rays)");
  }
  if (c->rq_area) hipFree(c->rq_area);
  c->rq_area = na; c->rq_bytes = bytes; c->rq_cap = bytes / area_bytes(1, FR_RAYS_CLOSEST, false);
  return FR_OK;
}

int fr_ray_query_reserve(fr_ctx* c, size_t max_rays) {
  if (!c) return FR_E_INVALID;
  if (max_rays > FR_RAYS_MAX) return fail(c, FR_E_INVALID, "fr_ray_query_reserve: more than 2^30 rays");
  return reserve_area(c, "fr_ray_query_reserve", area_bytes(max_rays, FR_RAYS_CLOSEST, false));
}

int fr_ray_query_reserve_kind(fr_ctx* c, size_t max_rays, int kind, int masked) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_ray_query_reserve_kind";
  if (max_rays > FR_RAYS_MAX) return fail(c, FR_E_INVALID, name + ": more than 2^30 rays");
  if (!kind_ok(kind)) return fail(c, FR_E_INVALID, name + ": bad kind");
  if (masked != 0 && masked != 1) return fail(c, FR_E_INVALID, name + ": masked is 0 or 1");
  return reserve_area(c, name, area_bytes(max_rays, kind, masked != 0));
}

static int trace_now(fr_ctx* c, const std::string& name, const void* rays, const uint32_t* masks, size_t n, int where,
                     int kind, void* out, bool surface_ok) {
  if (where != FR_MEM_HOST && where != FR_MEM_DEVICE) return fail(c, FR_E_INVALID, name + ": bad where");
  const bool device = where == FR_MEM_DEVICE;
  if (int rc = check_query_args(c, name, rays, masks, n, kind, out, device, surface_ok)) return rc;
  if (n == 0) return FR_OK;
  if (!device) {
    // the two first kinds without masks: the test fr_ray_query_reserve's callers know; otherwise the batch's bytes
    if (kind != FR_RAYS_SURFACE && !masks) {
      if (n > c->rq_cap)
        return fail(c, FR_E_INVALID, name + ": a host batch of " + std::to_string(n) + " rays exceeds the reservation of " +
                                         std::to_string(c->rq_cap) + " (fr_ray_query_reserve)");
    } else if (area_bytes(n, kind, masks != nullptr) > c->rq_bytes) {
      return fail(c, FR_E_INVALID, name + ": a host batch of " + std::to_string(n) + " rays takes " +
                                       std::to_string(area_bytes(n, kind, masks != nullptr)) + " bytes, the reservation holds " +
                                       std::to_string(c->rq_bytes) + " (fr_ray_query_reserve_kind)");
    }
  }
  if (int rc = quiesce(c)) return rc;
  if (device) {
    if (int rc = launch_query(c, rays, masks, n, kind, out)) return rc;
  } else {
    char* const d_rays = static_cast<char*>(c->rq_area);
    char* const d_out = d_rays + n * sizeof(fr_ray);
    uint32_t* const d_masks = masks ? reinterpret_cast<uint32_t*>(d_out + n * out_stride(kind)) : nullptr;
    HIP_TRY(c, hipMemcpyAsync(d_rays, rays, n * sizeof(fr_ray), hipMemcpyHostToDevice, c->stream));
    if (masks) HIP_TRY(c, hipMemcpyAsync(d_masks, masks, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_query(c, d_rays, d_masks, n, kind, d_out)) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, d_out, n * out_stride(kind), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

int fr_trace_rays(fr_ctx* c, const void* rays, size_t n, int where, int kind, void* out) {
  if (!c) return FR_E_INVALID;
  return trace_now(c, "fr_trace_rays", rays, nullptr, n, where, kind, out, false);
}

int fr_trace_rays_masked(fr_ctx* c, const void* rays, const uint32_t* masks, size_t n, int where, int kind, void* out) {
  if (!c) return FR_E_INVALID;
  return trace_now(c, "fr_trace_rays_masked", rays, masks, n, where, kind, out, true);
}

// The query in stream order: enqueued on the context stream, behind every update, pose, refit and rebuild made or
// enqueued before the call (in place they are earlier work of this stream; overlapped they run on front_stream, and
// join_update makes this stream wait for the last of them), and ahead of every one after it (in place: later work of
// this stream; overlapped: the update that will overwrite the set read here, two updates on, waits for set_read).
// It does not go through join_recon and leaves stream_dirty alone. That is safe because the query reads only the
// scene arrays and the caller's rays and masks, and writes only the caller's results and rq: the reconstruction
// streams read and write images, which the query never touches, so there is nothing of theirs to wait for; and the
// front stages of the next pipelined frame, which start on front_stream without waiting for this stream while
// stream_dirty is clear, read and write images, masks, counts and the scene, none of which the query writes. rq is
// only ever touched on this stream. So a query between two pipelined frames changes neither frame's schedule.
static int trace_enqueue(fr_ctx* c, const std::string& name, const void* rays, const uint32_t* masks, size_t n, int kind,
                         void* out, void* ready_event, bool surface_ok) {
  if (int rc = check_query_args(c, name, rays, masks, n, kind, out, true, surface_ok)) return rc;
  if (c->group_refs > 0 || c->U.shard_count > 1)
    return fail(c, FR_E_UNSUPPORTED, name + ": the context is a rank of a group or sharded (use fr_trace_rays)");
  if (n == 0) return FR_OK;
  hipSetDevice(c->cfg.device);
  join_update(c);
  if (ready_event) HIP_TRY(c, hipStreamWaitEvent(c->stream, static_cast<hipEvent_t>(ready_event), 0));
  if (int rc = launch_query(c, rays, masks, n, kind, out)) return rc;
  HIP_TRY(c, c->rays_done.record(c->stream));
  // overlapped updates: the query read the set in use; the update after the next one writes it
  HIP_TRY(c, mark_set_read(c));
  return FR_OK;
}

int fr_trace_rays_enqueue(fr_ctx* c, const void* rays, size_t n, int kind, void* out, void* ready_event) {
  if (!c) return FR_E_INVALID;
  return trace_enqueue(c, "fr_trace_rays_enqueue", rays, nullptr, n, kind, out, ready_event, false);
}

int fr_trace_rays_masked_enqueue(fr_ctx* c, const void* rays, const uint32_t* masks, size_t n, int kind, void* out,
                                 void* ready_event) {
  if (!c) return FR_E_INVALID;
  return trace_enqueue(c, "fr_trace_rays_masked_enqueue", rays, masks, n, kind, out, ready_event, true);
}

int fr_rays_consumed(fr_ctx* c, void* stream) {
  if (!c) return FR_E_INVALID;
  if (!c->rays_done.pending) return FR_OK;
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, c->rays_done.peek(static_cast<hipStream_t>(stream)));
  return FR_OK;
}
