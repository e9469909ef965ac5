// ctx_foveation.cpp — foveation control: the mask mode at run time, the eccentricity mask's parameters with the ray
// budget's status, the host statement of that mask, and a caller's own sampling mask in stream order. The kernels
// (k_ecc_mask, k_fov_control, k_mask_take) are in k_front.hip; the sampling launch that uses all of it is
// enqueue_sampling in ctx_frame.cpp.
#include <cmath>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

namespace {
// What fr_set_foveation refuses whatever the context (NULL: fine, else why not).
const char* bad_foveation(const fr_foveation& f, int W, int H) {
  if (!std::isfinite(f.radius_px) || !(f.radius_px > 0.0f)) return "radius_px must be finite and > 0";
  if (f.floor_ranks < 1 || f.floor_ranks > 64) return "floor_ranks must be in 1..64";
  if (!(f.tolerance >= 0.0f && f.tolerance < 1.0f)) return "tolerance must be in [0, 1)";
  if ((uint64_t)f.ray_budget > (uint64_t)W * (uint64_t)H) return "ray_budget exceeds W * H";
  return nullptr;
}
bool sized(int W, int H) { return W > 0 && H > 0 && W <= 32767 && H <= 32767; }
}  // namespace

namespace fri {
void foveation_init(fr_ctx* c) {
  fr_foveation_default(c->W, c->H, &c->fov);
  c->fov_r2 = c->fov.radius_px * c->fov.radius_px;
  c->fov_used_r2 = c->fov_r2;
}

int foveation_check(fr_ctx* c) {
  if (c->U.mask_mode == FR_MASK_CALLER && !c->cmask_set)
    return fail(c, FR_E_STATE, "mask mode FR_MASK_CALLER: no mask was submitted (fr_set_sampling_mask)");
  if (c->U.mask_mode == FR_MASK_ECCENTRIC && c->fov.ray_budget > 0 && (c->group_refs > 0 || c->U.shard_count > 1))
    return fail(c, FR_E_UNSUPPORTED, "a ray budget on a rank of a group or a sharded context");
  return FR_OK;
}
}  // namespace fri

extern "C" {

int fr_foveation_default(int width, int height, fr_foveation* f) {
  if (!f || !sized(width, height)) return FR_E_INVALID;
  const float w = (float)width, h = (float)height;
  const float ww = w * w, hh = h * h;
  f->radius_px = 0.07f * sqrtf(ww + hh);
  f->floor_ranks = 1;
  f->ray_budget = 0;
  f->tolerance = 0.02f;
  return FR_OK;
}

int fr_foveation_mask(int width, int height, const float gaze[2], float r2, int floor_ranks, uint8_t* mask, uint32_t* count) {
  if (!sized(width, height) || !gaze || !std::isfinite(gaze[0]) || !std::isfinite(gaze[1]) || !std::isfinite(r2) ||
      r2 < 0.0f || floor_ranks < 1 || floor_ranks > 64)
    return FR_E_INVALID;
  const f2 g = mk2(gaze[0], gaze[1]);
  uint32_t n = 0;
  for (uint32_t y = 0; y < (uint32_t)height; y++)
    for (uint32_t x = 0; x < (uint32_t)width; x++) {
      const bool on = ecc_sampled(x, y, g, r2, (uint32_t)floor_ranks);
      if (mask) mask[(size_t)y * width + x] = on ? 1 : 0;
      n += on ? 1u : 0u;
    }
  if (count) *count = n;
  return FR_OK;
}

int fr_set_foveation(fr_ctx* c, const fr_foveation* f) {
  if (!c) return FR_E_INVALID;
  if (!f) return fail(c, FR_E_INVALID, "fr_set_foveation: NULL parameters");
  if (const char* why = bad_foveation(*f, c->W, c->H)) return fail(c, FR_E_INVALID, std::string("fr_set_foveation: ") + why);
  if (f->ray_budget > 0) {
    if (c->group_refs > 0 || c->U.shard_count > 1)
      return fail(c, FR_E_UNSUPPORTED, "fr_set_foveation: a ray budget on a rank of a group or a sharded context");
    if (!c->cfg.optimize)
      return fail(c, FR_E_UNSUPPORTED, "fr_set_foveation: a ray budget on a context created with optimize = 0");
  }
  c->fov = *f;
  c->fov_r2 = f->radius_px * f->radius_px;
  c->fov_dirty = true;
  c->fov_reset = true;
  return FR_OK;
}

int fr_get_foveation(fr_ctx* c, fr_foveation* f) {
  if (!c || !f) return FR_E_INVALID;
  *f = c->fov;
  return FR_OK;
}

int fr_foveation_status(fr_ctx* c, float* r2, uint32_t* last_count, uint64_t* adjusted, uint64_t* held) {
  if (!c) return FR_E_INVALID;
  if (int rc = quiesce(c)) return rc;
  FovState s{c->fov_reset ? c->fov_r2 : c->fov_used_r2, 0u, 0u, 0u};
  if (c->fov_on_device && !c->fov_reset) {
    HIP_TRY(c, hipMemcpyAsync(c->h_fov, c->fov_st, sizeof(FovState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    s = *c->h_fov;
  }
  if (r2) *r2 = s.r2;
  if (last_count) *last_count = s.last_count;
  if (adjusted) *adjusted = s.adjusted;
  if (held) *held = s.held;
  return FR_OK;
}

int fr_set_mask_mode(fr_ctx* c, int mode) {
  if (!c) return FR_E_INVALID;
  if (mode < FR_MASK_SALIENCY || mode > FR_MASK_CALLER) return fail(c, FR_E_INVALID, "fr_set_mask_mode: mode outside 0..6");
  c->U.mask_mode = mode;
  c->lp_mode = -1;
  return FR_OK;
}

int fr_get_mask_mode(fr_ctx* c, int* mode) {
  if (!c || !mode) return FR_E_INVALID;
  *mode = c->U.mask_mode;
  return FR_OK;
}

int fr_sampling_mask_enable(fr_ctx* c, int on) {
  if (!c) return FR_E_INVALID;
  if (on != 0 && on != 1) return fail(c, FR_E_INVALID, "fr_sampling_mask_enable: on is 0 or 1");
  if (int rc = quiesce(c)) return rc;
  if (on && !c->cmask) {
    if (dalloc(&c->cmask, (size_t)c->W * c->H) != hipSuccess) {
      (void)hipGetLastError();
      if (c->cmask) hipFree(c->cmask);
      c->cmask = nullptr;
      return fail(c, FR_E_NOMEM, "fr_sampling_mask_enable: device allocation failed");
    }
  }
  c->cmask_on = on != 0;
  return FR_OK;
}

// What both set calls refuse before anything is written.
static int check_mask_args(fr_ctx* c, const std::string& name, const void* mask, size_t bytes, bool device) {
  if (!mask) return fail(c, FR_E_INVALID, name + ": mask is NULL");
  if (bytes != (size_t)c->W * c->H) return fail(c, FR_E_INVALID, name + ": bytes != W * H");
  if (device && (reinterpret_cast<uintptr_t>(mask) & 15u))
    return fail(c, FR_E_INVALID, name + ": the device pointer is not 16-byte aligned");
  if (!c->cmask_on) return fail(c, FR_E_STATE, name + ": caller masks are not enabled (fr_sampling_mask_enable)");
  return FR_OK;
}

int fr_set_sampling_mask(fr_ctx* c, const void* mask, size_t bytes, int where) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_sampling_mask";
  if (where != FR_MEM_HOST && where != FR_MEM_DEVICE) return fail(c, FR_E_INVALID, name + ": bad where");
  if (int rc = check_mask_args(c, name, mask, bytes, where == FR_MEM_DEVICE)) return rc;
  if (int rc = quiesce(c)) return rc;
  const uint8_t* src = static_cast<const uint8_t*>(mask);
  if (where == FR_MEM_HOST) {  // the bytes land in the copy and are normalised in place
    HIP_TRY(c, hipMemcpyAsync(c->cmask, mask, bytes, hipMemcpyHostToDevice, c->stream));
    src = c->cmask;
  }
  launch_mask_take(src, c->cmask, c->W, c->H, c->stream);
  if (int rc = check_launch(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->cmask_set = true;
  return FR_OK;
}

// The copy in stream order, on the stream of the front stages: behind the front stages of every frame enqueued so far
// (the last reader of the copy there is that stream's k_sampling) and ahead of the next frame's. Work on the context
// stream outside a pipelined frame (a stage call's sampling may read the copy too) is joined as a frame's front stages
// join it, when stream_dirty says there is some; the flag is the frame's to clear.
int fr_set_sampling_mask_enqueue(fr_ctx* c, const void* mask, size_t bytes, void* ready_event) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_sampling_mask_enqueue";
  if (int rc = check_mask_args(c, name, mask, bytes, true)) return rc;
  if (c->group_refs > 0 || c->U.shard_count > 1)
    return fail(c, FR_E_UNSUPPORTED, name + ": the context is a rank of a group or sharded (use fr_set_sampling_mask)");
  hipSetDevice(c->cfg.device);
  if (c->stream_dirty) stream_join(c, c->front_stream);
  if (ready_event) HIP_TRY(c, hipStreamWaitEvent(c->front_stream, static_cast<hipEvent_t>(ready_event), 0));
  launch_mask_take(static_cast<const uint8_t*>(mask), c->cmask, c->W, c->H, c->front_stream);
  if (int rc = check_launch(c)) return rc;
  HIP_TRY(c, c->mask_read.record(c->front_stream));
  HIP_TRY(c, c->mask_taken.record(c->front_stream));
  c->cmask_set = true;
  return FR_OK;
}

int fr_sampling_mask_consumed(fr_ctx* c, void* stream) {
  if (!c) return FR_E_INVALID;
  if (!c->mask_read.pending) return FR_OK;
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, c->mask_read.peek(static_cast<hipStream_t>(stream)));
  return FR_OK;
}

}  // extern "C"
