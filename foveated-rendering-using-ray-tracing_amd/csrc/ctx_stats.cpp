// ctx_stats.cpp — what a context reports about itself: ray statistics, the live kernel timing and frame clock rings
// (harvested in ctx_frame.cpp when they wrap), test hooks, and the FR_STAMPS probes of the diagnostic build.
#include <algorithm>
#include <cstdio>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

extern "C" {

int fr_get_stats(fr_ctx* c, fr_stats* s) {
  if (!c || !s) return FR_E_INVALID;
  DevStats d;
  HIP_TRY(c, hipMemcpyAsync(&d, c->stats, sizeof(d), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  s->gbuffer_primary = d.gbuffer_primary; s->primary = d.primary; s->shadow = d.shadow;
  s->diffuse_bounce = d.diffuse_bounce; s->mirror = d.mirror; s->refraction = d.refraction;
  s->reflection = d.reflection; s->truncated = d.truncated; s->overflow = d.bvh_overflow;
  for (int i = 0; i < 6; i++) s->diag[i] = d.pad[i];
  s->segments = d.gbuffer_primary + d.primary + d.shadow + d.diffuse_bounce + d.mirror + d.refraction + d.reflection;
  return FR_OK;
}

int fr_jfa_reuse_count(fr_ctx* c, uint32_t* skipped) {
  if (!c || !skipped) return FR_E_INVALID;
  join_recon(c);  // (the frame's JumpFlooding runs on the reconstruction stream)
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, hipMemcpyAsync(skipped, c->jfa.ctl + JFA_CTL_SKIPPED, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

// Test hook (not part of include/fovrt.h): the host build of the bound JFA and Sibson use.
float fr__sqrt_le_bound(float s) { return sqrt_le_bound(s); }

// Diagnostic hook (not part of include/fovrt.h): the last Sibson pass's list counts: strips (k_sibson_strip),
// wide[0] and wide[1] (k_sibson_wide's two lists).
int fr__sibson_counts(fr_ctx* c, uint32_t* out3) {
  if (!c || !out3 || !c->sib_strips) return FR_E_INVALID;
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, hipDeviceSynchronize());
  HIP_TRY(c, hipMemcpy(out3, c->sib_strips, sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(out3 + 1, c->sib_wide, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return FR_OK;
}

int fr_kernel_timing(fr_ctx* c, int enable) {
  if (!c) return FR_E_INVALID;
  if (enable && !c->kt_ev[0][0])
    for (auto& q : c->kt_ev)
      for (auto& e : q) HIP_TRY(c, hipEventCreate(&e));
  c->kt_on = enable != 0;
  c->kt_next = c->kt_pending = 0;
  c->kt_frames = 0;
  c->kt_stage_ms = c->kt_kernel_ms = 0.0;
  return FR_OK;
}

int fr_frame_clock(fr_ctx* c, int enable) {
  if (!c) return FR_E_INVALID;
  hipSetDevice(c->cfg.device);
  if (enable && !c->fc_ref) {
    HIP_TRY(c, hipEventCreate(&c->fc_ref));
    for (auto& q : c->fc_ev)
      for (auto& e : q) HIP_TRY(c, hipEventCreate(&e));
  }
  if (c->fc_pending) HIP_TRY(c, hipDeviceSynchronize());  // nothing recorded stays in flight across a reset
  c->fc_on = enable != 0;
  c->fc_next = c->fc_pending = 0;
  c->fc_cur = -1;
  c->fc_prev_end = -1.0;
  c->fc_latency.clear();
  c->fc_interval.clear();
  if (c->fc_on) HIP_TRY(c, hipEventRecord(c->fc_ref, c->stream));
  return FR_OK;
}

int fr_frame_clock_read(fr_ctx* c, float* latency_ms, float* interval_ms, int cap, int* n_latency, int* n_interval) {
  if (!c || cap < 0 || (cap > 0 && (!latency_ms || !interval_ms)) || !n_latency || !n_interval) return FR_E_INVALID;
  hipSetDevice(c->cfg.device);
  for (; c->fc_pending > 0; c->fc_pending--)
    fc_harvest(c, (c->fc_next - c->fc_pending + fr_ctx::FC_RING) % fr_ctx::FC_RING);
  *n_latency = (int)std::min<size_t>(c->fc_latency.size(), (size_t)cap);
  *n_interval = (int)std::min<size_t>(c->fc_interval.size(), (size_t)cap);
  if (*n_latency) memcpy(latency_ms, c->fc_latency.data(), sizeof(float) * *n_latency);
  if (*n_interval) memcpy(interval_ms, c->fc_interval.data(), sizeof(float) * *n_interval);
  return FR_OK;
}

int fr_kernel_times(fr_ctx* c, fr_stage_times* out) {
  if (!c || !out) return FR_E_INVALID;
  for (; c->kt_pending > 0; c->kt_pending--)
    kt_harvest(c, (c->kt_next - c->kt_pending + fr_ctx::KT_RING) % fr_ctx::KT_RING);
  out->frames = c->kt_frames;
  out->shading_ms = c->kt_stage_ms;
  out->shade_paths_ms = c->kt_kernel_ms;
  return FR_OK;
}

int fr_reset_stats(fr_ctx* c) {
  if (!c) return FR_E_INVALID;
  HIP_TRY(c, hipMemsetAsync(c->stats, 0, sizeof(DevStats), c->stream));
  return FR_OK;
}

#ifdef FR_STAMPS
// Diagnostic probe (libfovrt_diag.so only, not part of the ABI): one shading launch (geometry /
// sampling / optimize must have run) with per-sample records (queries, traversal steps, start, end;
// s_memrealtime ticks) and per-wave records (start, refill dry, end, samples), copied to the host.
extern "C" int fr_diag_sample_trace(fr_ctx* c, uint32_t* srec, uint32_t scap, uint32_t* wrec, uint32_t wcap) {
  if (!c || !srec || !wrec) return FR_E_INVALID;
  join_recon(c);
  hipSetDevice(c->cfg.device);
  uint32_t *ds = nullptr, *dw = nullptr;
  HIP_TRY(c, hipMalloc(&ds, (size_t)scap * 16));
  HIP_TRY(c, hipMalloc(&dw, (size_t)wcap * 16));
  hipMemsetAsync(ds, 0, (size_t)scap * 16, c->stream);
  hipMemsetAsync(dw, 0, (size_t)wcap * 16, c->stream);
  diag_sample_trace(ds, scap, dw, wcap, c->stream);
  int rc = enqueue_shading(c);
  diag_sample_trace(nullptr, 0, nullptr, 0, c->stream);
  hipStreamSynchronize(c->stream);
  if (!rc) {
    HIP_TRY(c, hipMemcpy(srec, ds, (size_t)scap * 16, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(wrec, dw, (size_t)wcap * 16, hipMemcpyDeviceToHost));
  }
  hipFree(ds);
  hipFree(dw);
  return rc;
}

// Diagnostic probe (libfovrt_diag.so only, not part of the ABI): records every query of one shading
// launch (geometry / sampling / optimize must have run), then traces the recorded stream with
// k_trace_queries. out = {queries, best ms of 5 runs, shadow queries, ms of the stream partitioned by
// kind, ms of its closest-hit part (specialised kernel), ms of its shadow part (specialised kernel)}.
extern "C" int fr_diag_trace_queries(fr_ctx* c, float* out) {
  if (!c || !out) return FR_E_INVALID;
  join_recon(c);
  hipSetDevice(c->cfg.device);
  const uint32_t cap = 48u << 20;
  f4 *rec = nullptr, *hits = nullptr;
  uint32_t* ctr = nullptr;
  HIP_TRY(c, hipMalloc(&rec, (size_t)cap * 32));
  HIP_TRY(c, hipMalloc(&hits, (size_t)cap * 16));
  HIP_TRY(c, hipMalloc(&ctr, 4));
  diag_record_queries(rec, cap, c->stream);
  if (int rc = enqueue_shading(c)) return rc;
  uint32_t n = std::min(diag_recorded_queries(c->stream), cap);
  diag_record_queries(nullptr, 0, c->stream);
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  // best of 5 runs of fn() on the context stream
  auto timeit = [&](auto fn) {
    float best = 1e30f;
    for (int r = 0; r < 5; r++) {
      hipEventRecord(a, c->stream);
      fn();
      hipEventRecord(b, c->stream);
      hipStreamSynchronize(c->stream);
      float ms = 0;
      hipEventElapsedTime(&ms, a, b);
      best = std::min(best, ms);
    }
    return best;
  };
  const float t_mixed = timeit([&] { launch_trace_queries(c->dsc, rec, n, hits, ctr, c->stream, 0); });
  // the same stream partitioned by kind (closest-hit first, then shadow; order within a kind kept)
  std::vector<f4> d((size_t)n * 2), part;
  HIP_TRY(c, hipMemcpy(d.data(), rec, (size_t)n * 32, hipMemcpyDeviceToHost));
  part.reserve(d.size());
  for (int pass = 0; pass < 2; pass++)
    for (uint32_t i = 0; i < n; i++)
      if ((d[2 * (size_t)i + 1].w != 0.0f) == (pass == 1)) { part.push_back(d[2 * (size_t)i]); part.push_back(d[2 * (size_t)i + 1]); }
  size_t shadow = 0;
  for (uint32_t i = 0; i < n; i++) shadow += d[2 * (size_t)i + 1].w != 0.0f;
  if (const char* path = getenv("FOVRT_DIAG_DUMP")) {  // every 16th query (o, tmax, d, any) for offline BVH studies
    if (FILE* f = fopen(path, "wb")) {
      for (uint32_t i = 0; i < n; i += 16) fwrite(&d[2 * (size_t)i], sizeof(f4), 2, f);
      fclose(f);
    }
  }
  const uint32_t nc = n - (uint32_t)shadow;
  HIP_TRY(c, hipMemcpy(rec, part.data(), (size_t)n * 32, hipMemcpyHostToDevice));
  const float t_sorted = timeit([&] { launch_trace_queries(c->dsc, rec, n, hits, ctr, c->stream, 0); });
  const float t_closest = timeit([&] { launch_trace_queries(c->dsc, rec, nc, hits, ctr, c->stream, 1); });
  const float t_shadow =
      timeit([&] { launch_trace_queries(c->dsc, rec + 2 * (size_t)nc, (uint32_t)shadow, hits, ctr, c->stream, 2); });
  out[3] = t_sorted;
  out[4] = t_closest;
  out[5] = t_shadow;
  out[0] = (float)n;
  out[1] = t_mixed;
  out[2] = (float)shadow;
  hipEventDestroy(a);
  hipEventDestroy(b);
  hipFree(rec);
  hipFree(hits);
  hipFree(ctr);
  return check_launch(c);
}
#endif

}  // extern "C"
