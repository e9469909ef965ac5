// ctx_query.cpp — ray queries: a caller's batch of rays against the scene as of the call's place in the stream order
// (fr_trace_rays, fr_trace_rays_enqueue, fr_rays_consumed, fr_ray_query_reserve; the kernel is k_ray_queries in
// k_trace.hip). A query reads the scene (tree, leaf triangles, primitive map, shading records, materials) and the
// caller's rays, and writes the caller's results and the context's query record (rq); it touches no image buffer,
// no temporal state, no counter of fr_stats and no JFA state.
#include <cstdint>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

static_assert(sizeof(fr_ray) == 32 && sizeof(fr_ray_hit) == 16, "the kernel reads 32-B rays and writes 16-B hits");

#define FR_RAYS_MAX ((size_t)1 << 30)

static size_t out_stride(int kind) { return kind == FR_RAYS_CLOSEST ? sizeof(fr_ray_hit) : sizeof(float); }

// What both forms refuse before anything is enqueued (n > 0; device: the arrays are device memory).
static int check_query_args(fr_ctx* c, const std::string& name, const void* rays, size_t n, int kind, const void* out,
                            bool device) {
  if (kind != FR_RAYS_CLOSEST && kind != FR_RAYS_TRANSMITTANCE) return fail(c, FR_E_INVALID, name + ": bad kind");
  if (n > FR_RAYS_MAX) return fail(c, FR_E_INVALID, name + ": more than 2^30 rays");
  if (n == 0) return FR_OK;
  if (!rays || !out) return fail(c, FR_E_INVALID, name + ": rays or out is NULL");
  const uintptr_t r = reinterpret_cast<uintptr_t>(rays), o = reinterpret_cast<uintptr_t>(out);
  if (device && ((r & 15u) || (o & (kind == FR_RAYS_CLOSEST ? 15u : 3u))))
    return fail(c, FR_E_INVALID, name + ": a device pointer is not aligned (rays and hits: 16 bytes, transmittance: 4)");
  if (r < o + n * out_stride(kind) && o < r + n * sizeof(fr_ray))
    return fail(c, FR_E_INVALID, name + ": rays and out overlap");
  return FR_OK;
}

// The launch, on the context stream, over the scene current at the call (dsc, as frames take it).
static int launch_query(fr_ctx* c, const void* rays, size_t n, int kind, void* out) {
  launch_ray_queries(c->dsc, rays, (uint32_t)n, kind == FR_RAYS_TRANSMITTANCE ? 1 : 0, out, c->rq, c->rayq_blocks,
                     c->stream);
  return check_launch(c);
}

int fr_ray_query_reserve(fr_ctx* c, size_t max_rays) {
  if (!c) return FR_E_INVALID;
  if (max_rays > FR_RAYS_MAX) return fail(c, FR_E_INVALID, "fr_ray_query_reserve: more than 2^30 rays");
  if (int rc = quiesce(c)) return rc;  // (a query may still read the staging area about to be replaced)
  if (max_rays <= c->rq_cap) return FR_OK;
  void *nr = nullptr, *no = nullptr;
  if (hipMalloc(&nr, max_rays * sizeof(fr_ray)) != hipSuccess || hipMalloc(&no, max_rays * sizeof(fr_ray_hit)) != hipSuccess) {
    (void)hipGetLastError();
    if (nr) hipFree(nr);
    return fail(c, FR_E_NOMEM, "fr_ray_query_reserve: device allocation failed (the reservation stays at " +
                                   std::to_string(c->rq_cap) + " rays)");
  }
  if (c->rq_rays) hipFree(c->rq_rays);
  if (c->rq_out) hipFree(c->rq_out);
  c->rq_rays = nr; c->rq_out = no; c->rq_cap = max_rays;
  return FR_OK;
}

int fr_trace_rays(fr_ctx* c, const void* rays, size_t n, int where, int kind, void* out) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_trace_rays";
  if (where != FR_MEM_HOST && where != FR_MEM_DEVICE) return fail(c, FR_E_INVALID, name + ": bad where");
  const bool device = where == FR_MEM_DEVICE;
  if (int rc = check_query_args(c, name, rays, n, kind, out, device)) return rc;
  if (n == 0) return FR_OK;
  if (!device && n > c->rq_cap)
    return fail(c, FR_E_INVALID, name + ": a host batch of " + std::to_string(n) + " rays exceeds the reservation of " +
                                     std::to_string(c->rq_cap) + " (fr_ray_query_reserve)");
  if (int rc = quiesce(c)) return rc;
  if (device) {
    if (int rc = launch_query(c, rays, n, kind, out)) return rc;
  } else {
    HIP_TRY(c, hipMemcpyAsync(c->rq_rays, rays, n * sizeof(fr_ray), hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_query(c, c->rq_rays, n, kind, c->rq_out)) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, c->rq_out, n * out_stride(kind), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

// The query in stream order: enqueued on the context stream, behind every update, pose, refit and rebuild made or
// enqueued before the call (in place they are earlier work of this stream; overlapped they run on front_stream, and
// join_update makes this stream wait for the last of them), and ahead of every one after it (in place: later work of
// this stream; overlapped: the update that will overwrite the set read here, two updates on, waits for set_read).
// It does not go through join_recon and leaves stream_dirty alone. That is safe because the query reads only the
// scene arrays and the caller's rays, and writes only the caller's results and rq: the reconstruction streams read
// and write images, which the query never touches, so there is nothing of theirs to wait for; and the front stages
// of the next pipelined frame, which start on front_stream without waiting for this stream while stream_dirty is
// clear, read and write images, masks, counts and the scene, none of which the query writes. rq is only ever
// touched on this stream. So a query between two pipelined frames changes neither frame's schedule.
int fr_trace_rays_enqueue(fr_ctx* c, const void* rays, size_t n, int kind, void* out, void* ready_event) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_trace_rays_enqueue";
  if (int rc = check_query_args(c, name, rays, n, kind, out, true)) return rc;
  if (c->group_refs > 0 || c->U.shard_count > 1)
    return fail(c, FR_E_UNSUPPORTED, name + ": the context is a rank of a group or sharded (use fr_trace_rays)");
  if (n == 0) return FR_OK;
  hipSetDevice(c->cfg.device);
  join_update(c);
  if (ready_event) HIP_TRY(c, hipStreamWaitEvent(c->stream, static_cast<hipEvent_t>(ready_event), 0));
  if (int rc = launch_query(c, rays, n, kind, out)) return rc;
  HIP_TRY(c, c->rays_done.record(c->stream));
  // overlapped updates: the query read the set in use; the update after the next one writes it
  HIP_TRY(c, mark_set_read(c));
  return FR_OK;
}

int fr_rays_consumed(fr_ctx* c, void* stream) {
  if (!c) return FR_E_INVALID;
  if (!c->rays_done.pending) return FR_OK;
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, c->rays_done.peek(static_cast<hipStream_t>(stream)));
  return FR_OK;
}
