// ctx_present.cpp — present: a reconstructed image as packed 8-bit texels, in host memory through a ring of pinned
// images (fr_present_enable, fr_present_enqueue, fr_present_acquire, fr_present_release) or in the caller's device
// memory (fr_present_enqueue_device, fr_present_done), in stream order; and the rule on the host (fr_present_pack).
// The kernel is k_present_pack (k_present.hip); the ring's bookkeeping is PresentRing (present_ring.h).
// fr_present_enqueue_warped and fr_present_enqueue_warped_device are the same two calls with k_present_warp in the
// pack's place (a homography between the image and the texels: late reprojection, crop, scale), and
// fr_present_warp_pack is that rule on the host; the ordering below is theirs unchanged. A warped slot carries
// ow * oh * 4 bytes to the host, no more. fr_present_enqueue_blended and fr_present_enqueue_blended_device are the same
// again over a virtual image that mixes two of the images around a gaze point (k_present_blend, k_present_blend_warp;
// fr_present_blend_pack on the host): the present stream waits as for one image, and the fence of each source is
// recorded behind the kernel. fr_present_enqueue_reprojected and fr_present_enqueue_reprojected_device are the warped
// calls with three launches in the kernel's place (launch_present_reproject, k_present_reproject.hip: a clear of the
// context's key image, a scatter of the source by the frame slot's POSITION, a resolve that falls back to the
// homography), and fr_present_reproject_pack is that rule on the host. They read POSITION beside the source, so the
// slot's present_read_shd is recorded behind them whatever the source is: POSITION's next writers (the front stages of
// the frame that takes the slot next; a stage call, a write or a restore through join_recon) wait for it already.
//
// Ordering. A present reads one of the images a frame's last stages write (SIBSON on sibson_stream, PULLPUSH and the
// A-Trous pair on atrous_stream, the slot's SHADING on the context stream; stage calls and fr_write_buffer write all
// of them on the context stream). The pack runs on present.stream, which first waits for
//  - the context stream as of the call (ev_fork): every stage call, write and timed frame before it, and the trace
//    half of every pipelined frame before it, whose resolve wrote SHADING;
//  - recon_done of every slot whose flag is still up: both chains of every reconstruction enqueued before the call
//    (sibson_stream is in order, so the last record covers the earlier ones; a flag that is down was consumed by the
//    context stream, by join_recon, or by front_stream ahead of a front_done the context stream has taken: either way
//    ev_fork covers it).
// It takes no fence down and leaves stream_dirty alone, so the frames around it keep their schedule. Whoever writes
// the image next waits for the pack's read: present_read / present_read_shd (ctx_internal.h), recorded here, waited
// for at a frame's reconstruction fork, in enqueue_geometry and in join_recon (ctx_frame.cpp). The copy to the host
// reads the staging image, which nothing but this stream touches, so nothing of a frame ever waits for a copy.
#include <cmath>
#include <cstdint>
#include <vector>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

namespace {
bool format_ok(int format) { return (format & ~FR_PRESENT_TOP_DOWN) == FR_PRESENT_RGBA8 || (format & ~FR_PRESENT_TOP_DOWN) == FR_PRESENT_BGRA8; }
size_t image_bytes(const fr_ctx* c) { return (size_t)c->W * c->H * 4; }

// The physical image a presentable id names at the call; -1 for any other id.
int presentable(fr_ctx* c, int id) {
  switch (id) {
    case FR_BUF_SHADING: return P_shd(c);
    case FR_BUF_SIBSON: return P_SIBSON;
    case FR_BUF_PULLPUSH: return P_PULLPUSH;
    case FR_BUF_ATROUS: return c->atrous_out;
    default: return -1;
  }
}

void free_slots(fr_ctx::Present& P) {
  for (int i = 0; i < PresentRing::MAX_SLOTS; i++) {
    if (P.stage[i]) hipFree(P.stage[i]);
    if (P.host[i]) hipHostFree(P.host[i]);
    P.stage[i] = P.host[i] = nullptr;
  }
  P.made = 0;
}

// A warp as the host rule and both warped enqueues take it: nine finite coefficients and an output no larger than the
// W x H source either way (0, 0: the source's size). *ow, *oh: the size to produce.
bool warp_ok(const fr_present_warp* warp, int W, int H, int* ow, int* oh) {
  if (!warp) return false;
  for (float v : warp->h) if (!std::isfinite(v)) return false;
  const bool whole = warp->out_width == 0 && warp->out_height == 0;
  *ow = whole ? W : warp->out_width;
  *oh = whole ? H : warp->out_height;
  return *ow >= 1 && *ow <= W && *oh >= 1 && *oh <= H;
}

// A blend as the host rule and both blended enqueues take it: finite gaze and radii, 0 <= inner <= outer, and a finite
// outer * outer. *b: the blend as the kernels take it, the squared radii one fp32 product each.
bool blend_ok(const fr_present_blend* blend, PresentBlend* b) {
  if (!blend) return false;
  const float r0 = blend->inner_radius_px, r1 = blend->outer_radius_px;
  if (!std::isfinite(blend->gaze[0]) || !std::isfinite(blend->gaze[1]) || !std::isfinite(r0) || !std::isfinite(r1)) return false;
  if (!(r0 >= 0.0f && r0 <= r1)) return false;
  const float r0sq = r0 * r0, r1sq = r1 * r1;
  if (!std::isfinite(r1sq)) return false;
  *b = PresentBlend{blend->gaze[0], blend->gaze[1], r0sq, r1sq};
  return true;
}
// A reprojection as the host rule and both reprojected enqueues take it: sixteen finite coefficients and a fallback
// that is a warp.
bool reproject_ok(const fr_present_reproject* rp, int W, int H, int* ow, int* oh) {
  if (!rp) return false;
  for (float v : rp->vp) if (!std::isfinite(v)) return false;
  return warp_ok(&rp->fallback, W, H, ow, oh);
}
const char* const kBadReproject =
    ": the reprojection is NULL, has a non-finite coefficient, or its fallback has one or an output size outside 1..W x 1..H";

const char* const kReprojectOff = ": reprojected presents are not enabled (fr_present_reproject_enable)";
const char* const kBadBlend =
    ": the blend is NULL, has a non-finite gaze or radius, a negative radius, inner > outer, or an outer radius whose "
    "square is not finite";

// What a present packs: one image, or (blended) the virtual image that mixes `phys` (inner) and `outer` by `blend`.
struct Source {
  int phys = -1, outer = -1;
  bool blended = false;
  PresentBlend blend{};
};

// The stream, the events and the fences, once; then the images of slots made .. slots - 1. All or nothing.
bool make_ring(fr_ctx* c, int slots) {
  fr_ctx::Present& P = c->present;
  bool ok = true;
  if (!P.stream) {
    ok = hipStreamCreateWithPriority(&P.stream, hipStreamNonBlocking, 0) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&P.ev_fork, hipEventDisableTiming) == hipSuccess;
    for (auto& e : P.ev)
      ok = ok && hipEventCreate(&e.begin) == hipSuccess && hipEventCreate(&e.packed) == hipSuccess &&
           hipEventCreate(&e.done) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->present_read.ev, hipEventDisableTiming) == hipSuccess;
    for (Fence& f : c->present_read_shd) ok = ok && hipEventCreateWithFlags(&f.ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->present_dev.ev, hipEventDisableTiming) == hipSuccess;
  }
  for (int i = P.made; ok && i < slots; i++) {
    ok = hipMalloc(&P.stage[i], image_bytes(c)) == hipSuccess && hipHostMalloc(&P.host[i], image_bytes(c), hipHostMallocDefault) == hipSuccess;
    if (ok) P.made = i + 1;
  }
  if (!ok) (void)hipGetLastError();
  return ok;
}

// What both enqueue forms refuse before anything is enqueued. src: the image to pack, resolved here from buffer_id, or
// (blend given: blended, with its parameters checked by the caller) the two images from the blend's ids.
int check_enqueue(fr_ctx* c, const std::string& name, int buffer_id, const fr_present_blend* blend, Source* src) {
  src->phys = presentable(c, blend ? blend->inner_buffer : buffer_id);
  src->outer = blend ? presentable(c, blend->outer_buffer) : src->phys;
  if (src->phys < 0 || src->outer < 0)
    return fail(c, FR_E_INVALID, name + ": the buffer is not FR_BUF_SHADING, FR_BUF_SIBSON, FR_BUF_PULLPUSH or FR_BUF_ATROUS");
  if (c->group_refs > 0 || c->U.shard_count > 1)
    return fail(c, FR_E_UNSUPPORTED, name + ": the context is a rank of a group or sharded");
  if (c->present.ring.n == 0) return fail(c, FR_E_STATE, name + ": presenting is not enabled (fr_present_enable)");
  return FR_OK;
}

// The present stream behind what wrote the image (the head of this file), then the pack into dst, then the fence
// its next writer waits for: of each source, when the present blends two. begin / packed: a slot's timing events, or
// NULL. warp: NULL for the plain pack, else the checked homography with its output size ow x oh (the kernels take warp
// and blend by value: nothing is read after the call). rp: the checked reprojection, whose fallback `warp` then is.
int enqueue_pack(fr_ctx* c, const Source& src, const fr_present_reproject* rp, const fr_present_warp* warp, int ow, int oh,
                 void* dst, hipEvent_t begin, hipEvent_t packed) {
  fr_ctx::Present& P = c->present;
  HIP_TRY(c, hipEventRecord(P.ev_fork, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(P.stream, P.ev_fork, 0));
  for (const Fence& f : c->recon_done) HIP_TRY(c, f.peek(P.stream));
  if (begin) HIP_TRY(c, hipEventRecord(begin, P.stream));
  if (rp)
    launch_present_reproject(c->img[src.phys], c->img[P_pos(c)], c->W, c->H, P.format, rp->vp, warp->h, ow, oh, P.keys, dst,
                             P.stream);
  else if (src.blended)
    launch_present_blend(c->img[src.phys], c->img[src.outer], c->W, c->H, P.format, src.blend, warp ? warp->h : nullptr, ow, oh,
                         dst, P.stream);
  else if (warp)
    launch_present_warp(c->img[src.phys], c->W, c->H, P.format, warp->h, ow, oh, dst, P.stream);
  else
    launch_present_pack(c->img[src.phys], c->W, c->H, P.format, dst, P.stream);
  if (int rc = check_launch(c)) return rc;
  if (packed) HIP_TRY(c, hipEventRecord(packed, P.stream));
  const int shd = P_shd(c);
  if (rp || src.phys == shd || src.outer == shd) HIP_TRY(c, c->present_read_shd[c->slot].record(P.stream));
  if (src.phys != shd || src.outer != shd) HIP_TRY(c, c->present_read.record(P.stream));
  return FR_OK;
}

// fr_present_enqueue (warp NULL), fr_present_enqueue_warped and (blended: the sources are the blend's, buffer_id is not
// used) fr_present_enqueue_blended: into the next free slot and on to its pinned image. reproject:
// fr_present_enqueue_reprojected, the warp is rp's fallback.
int enqueue_host(fr_ctx* c, const std::string& name, int buffer_id, const fr_present_blend* blend, bool blended,
                 const fr_present_warp* warp, bool warped, uint64_t* ticket, const fr_present_reproject* rp = nullptr,
                 bool reproject = false) {
  if (!c || !ticket) return FR_E_INVALID;
  int ow = c->W, oh = c->H;
  if (reproject) {
    if (!reproject_ok(rp, c->W, c->H, &ow, &oh)) return fail(c, FR_E_INVALID, name + kBadReproject);
    warp = &rp->fallback;
  } else if (warped && !warp_ok(warp, c->W, c->H, &ow, &oh))
    return fail(c, FR_E_INVALID, name + ": the warp is NULL, has a non-finite coefficient or an output size outside 1..W x 1..H");
  Source src;
  if ((src.blended = blended) && !blend_ok(blend, &src.blend)) return fail(c, FR_E_INVALID, name + kBadBlend);
  if (int rc = check_enqueue(c, name, buffer_id, blended ? blend : nullptr, &src)) return rc;
  fr_ctx::Present& P = c->present;
  if (reproject && !P.reproject) return fail(c, FR_E_STATE, name + kReprojectOff);
  uint64_t t = 0;
  const int s = P.ring.enqueue(&t);
  if (s < 0) return fail(c, FR_E_STATE, name + ": every slot of the ring is held (fr_present_release)");
  hipSetDevice(c->cfg.device);
  // (the slot's last copy is earlier work of the present stream: the pack overwrites the staging image behind it)
  int rc = enqueue_pack(c, src, reproject ? rp : nullptr, warped || reproject ? warp : nullptr, ow, oh, P.stage[s],
                        P.ev[s].begin, P.ev[s].packed);
  if (rc == FR_OK && hipMemcpyAsync(P.host[s], P.stage[s], (size_t)ow * oh * 4, hipMemcpyDeviceToHost, P.stream) != hipSuccess)
    rc = fail(c, FR_E_HIP, name + ": the copy to the host could not be enqueued");
  if (rc == FR_OK && hipEventRecord(P.ev[s].done, P.stream) != hipSuccess) rc = fail(c, FR_E_HIP, name + ": event record failed");
  if (rc != FR_OK) {
    P.ring.release(s);
    return rc;
  }
  *ticket = t;
  return FR_OK;
}

// fr_present_enqueue_device (warp NULL), fr_present_enqueue_warped_device and (blended) fr_present_enqueue_blended_device:
// straight into the caller's memory. reproject: fr_present_enqueue_reprojected_device, the warp is rp's fallback.
int enqueue_device(fr_ctx* c, const std::string& name, int buffer_id, const fr_present_blend* blend, bool blended,
                   const fr_present_warp* warp, bool warped, void* device_dst, size_t bytes,
                   const fr_present_reproject* rp = nullptr, bool reproject = false) {
  if (!c) return FR_E_INVALID;
  int ow = c->W, oh = c->H;
  if (reproject) {
    if (!reproject_ok(rp, c->W, c->H, &ow, &oh)) return fail(c, FR_E_INVALID, name + kBadReproject);
    warp = &rp->fallback;
  } else if (warped && !warp_ok(warp, c->W, c->H, &ow, &oh))
    return fail(c, FR_E_INVALID, name + ": the warp is NULL, has a non-finite coefficient or an output size outside 1..W x 1..H");
  if (!device_dst || (reinterpret_cast<uintptr_t>(device_dst) & 15u))
    return fail(c, FR_E_INVALID, name + ": device_dst is NULL or not 16-byte aligned");
  if (bytes != (size_t)ow * oh * 4) return fail(c, FR_E_INVALID, name + ": bytes != the output's width * height * 4");
  Source src;
  if ((src.blended = blended) && !blend_ok(blend, &src.blend)) return fail(c, FR_E_INVALID, name + kBadBlend);
  if (int rc = check_enqueue(c, name, buffer_id, blended ? blend : nullptr, &src)) return rc;
  if (reproject && !c->present.reproject) return fail(c, FR_E_STATE, name + kReprojectOff);
  hipSetDevice(c->cfg.device);
  if (int rc = enqueue_pack(c, src, reproject ? rp : nullptr, warped || reproject ? warp : nullptr, ow, oh, device_dst, nullptr,
                            nullptr))
    return rc;
  HIP_TRY(c, c->present_dev.record(c->present.stream));
  return FR_OK;
}
}  // namespace

namespace fri {
void present_join(fr_ctx* c) {
  c->present_read.peek(c->stream);
  for (const Fence& f : c->present_read_shd) f.peek(c->stream);
}

int present_sync(fr_ctx* c) {
  if (!c->present.stream) return FR_OK;
  HIP_TRY(c, hipStreamSynchronize(c->present.stream));
  c->present_read.pending = false;
  for (Fence& f : c->present_read_shd) f.pending = false;
  return FR_OK;
}

void present_destroy(fr_ctx* c) {
  fr_ctx::Present& P = c->present;
  if (P.stream) hipStreamSynchronize(P.stream);
  free_slots(P);
  if (P.keys) hipFree(P.keys);
  for (auto& e : P.ev)
    for (hipEvent_t v : {e.begin, e.packed, e.done}) if (v) hipEventDestroy(v);
  if (P.ev_fork) hipEventDestroy(P.ev_fork);
  // (the stream has drained, so no record of a fence is in flight: the flags go down with their events)
  if (c->present_read.ev) hipEventDestroy(c->present_read.ev);
  for (Fence& f : c->present_read_shd) if (f.ev) hipEventDestroy(f.ev);
  if (c->present_dev.ev) hipEventDestroy(c->present_dev.ev);
  c->present_read = c->present_dev = Fence{};
  for (Fence& f : c->present_read_shd) f = Fence{};
  if (P.stream) hipStreamDestroy(P.stream);
  P = fr_ctx::Present{};
}
}  // namespace fri

extern "C" {

int fr_present_pack(const float* rgba, int width, int height, int format, uint8_t* out) {
  if (!rgba || !out || width < 1 || height < 1 || width > 32767 || height > 32767 || !format_ok(format)) return FR_E_INVALID;
  const bool bgra = (format & ~FR_PRESENT_TOP_DOWN) == FR_PRESENT_BGRA8, top_down = (format & FR_PRESENT_TOP_DOWN) != 0;
  for (int r = 0; r < height; r++) {
    const float* in = rgba + (size_t)(top_down ? height - 1 - r : r) * width * 4;
    uint8_t* o = out + (size_t)r * width * 4;
    for (int x = 0; x < width; x++) {
      const uint32_t w = present_texel(mk4(in[4 * x], in[4 * x + 1], in[4 * x + 2], in[4 * x + 3]), bgra);
      o[4 * x] = (uint8_t)w; o[4 * x + 1] = (uint8_t)(w >> 8); o[4 * x + 2] = (uint8_t)(w >> 16); o[4 * x + 3] = (uint8_t)(w >> 24);
    }
  }
  return FR_OK;
}

int fr_present_warp_pack(const float* rgba, int width, int height, int format, const fr_present_warp* warp, uint8_t* out) {
  if (!rgba || !out || width < 1 || height < 1 || width > 32767 || height > 32767 || !format_ok(format)) return FR_E_INVALID;
  int ow, oh;
  if (!warp_ok(warp, width, height, &ow, &oh)) return FR_E_INVALID;
  const bool bgra = (format & ~FR_PRESENT_TOP_DOWN) == FR_PRESENT_BGRA8, top_down = (format & FR_PRESENT_TOP_DOWN) != 0;
  const auto fetch = [rgba, width](int i, int row) {
    const float* t = rgba + ((size_t)row * width + i) * 4;
    return mk4(t[0], t[1], t[2], t[3]);
  };
  for (int r = 0; r < oh; r++) {
    const int y = top_down ? oh - 1 - r : r;
    uint8_t* o = out + (size_t)r * ow * 4;
    for (int x = 0; x < ow; x++) {
      const uint32_t w = present_warp_texel(fetch, width, height, warp->h, x, y, bgra);
      o[4 * x] = (uint8_t)w; o[4 * x + 1] = (uint8_t)(w >> 8); o[4 * x + 2] = (uint8_t)(w >> 16); o[4 * x + 3] = (uint8_t)(w >> 24);
    }
  }
  return FR_OK;
}

int fr_present_enable(fr_ctx* c, int slots, int format) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_present_enable";
  if (slots < 0 || slots > PresentRing::MAX_SLOTS) return fail(c, FR_E_INVALID, name + ": slots outside 0..8");
  if (slots > 0 && !format_ok(format)) return fail(c, FR_E_INVALID, name + ": unknown format");
  if (c->W > 32767 || c->H > 32767) return fail(c, FR_E_UNSUPPORTED, name + ": a screen above 32767 pixels a side");
  fr_ctx::Present& P = c->present;
  if (slots == P.ring.n && (slots == 0 || format == P.format)) return FR_OK;  // nothing changes
  if (int rc = quiesce(c)) return rc;
  if (int rc = present_sync(c)) return rc;
  if (!P.ring.all_free()) return fail(c, FR_E_STATE, name + ": a ticket of the ring in place is not released");
  if (slots > 0 && !make_ring(c, slots)) {
    present_destroy(c);
    return fail(c, FR_E_NOMEM, name + ": allocation failed (nothing is kept, presenting is off)");
  }
  if (slots > 0) P.format = format;
  P.ring.reset(slots);
  return FR_OK;
}

int fr_present_enqueue(fr_ctx* c, int buffer_id, uint64_t* ticket) {
  return enqueue_host(c, "fr_present_enqueue", buffer_id, nullptr, false, nullptr, false, ticket);
}

int fr_present_enqueue_warped(fr_ctx* c, int buffer_id, const fr_present_warp* warp, uint64_t* ticket) {
  return enqueue_host(c, "fr_present_enqueue_warped", buffer_id, nullptr, false, warp, true, ticket);
}

int fr_present_acquire(fr_ctx* c, uint64_t ticket, int wait, const void** host) {
  if (!c || !host) return FR_E_INVALID;
  const std::string name = "fr_present_acquire";
  fr_ctx::Present& P = c->present;
  if (P.ring.n == 0) return fail(c, FR_E_STATE, name + ": presenting is not enabled (fr_present_enable)");
  const int s = P.ring.find(ticket);
  if (s < 0) return fail(c, FR_E_INVALID, name + ": unknown or released ticket");
  if (P.ring.state[s] != PresentRing::HELD) {
    hipSetDevice(c->cfg.device);
    const hipError_t e = wait ? hipEventSynchronize(P.ev[s].done) : hipEventQuery(P.ev[s].done);
    if (e == hipErrorNotReady) return FR_PRESENT_PENDING;
    if (e != hipSuccess) return fail(c, FR_E_HIP, name + ": " + hipGetErrorString(e));
    P.ring.acquired(s);
  }
  *host = P.host[s];
  return FR_OK;
}

int fr_present_release(fr_ctx* c, uint64_t ticket) {
  if (!c) return FR_E_INVALID;
  fr_ctx::Present& P = c->present;
  if (P.ring.n == 0) return fail(c, FR_E_STATE, "fr_present_release: presenting is not enabled (fr_present_enable)");
  const int s = P.ring.find(ticket);
  if (s < 0) return fail(c, FR_E_INVALID, "fr_present_release: unknown or released ticket");
  P.ring.release(s);
  return FR_OK;
}

int fr_present_times(fr_ctx* c, uint64_t ticket, float* pack_ms, float* copy_ms) {
  if (!c) return FR_E_INVALID;
  fr_ctx::Present& P = c->present;
  if (P.ring.n == 0) return fail(c, FR_E_STATE, "fr_present_times: presenting is not enabled (fr_present_enable)");
  const int s = P.ring.find(ticket);
  if (s < 0) return fail(c, FR_E_INVALID, "fr_present_times: unknown or released ticket");
  if (P.ring.state[s] != PresentRing::HELD) return fail(c, FR_E_STATE, "fr_present_times: the ticket is not acquired");
  hipSetDevice(c->cfg.device);
  float a = 0.0f, b = 0.0f;
  HIP_TRY(c, hipEventElapsedTime(&a, P.ev[s].begin, P.ev[s].packed));
  HIP_TRY(c, hipEventElapsedTime(&b, P.ev[s].packed, P.ev[s].done));
  if (pack_ms) *pack_ms = a;
  if (copy_ms) *copy_ms = b;
  return FR_OK;
}

int fr_present_enqueue_device(fr_ctx* c, int buffer_id, void* device_dst, size_t bytes) {
  return enqueue_device(c, "fr_present_enqueue_device", buffer_id, nullptr, false, nullptr, false, device_dst, bytes);
}

int fr_present_enqueue_warped_device(fr_ctx* c, int buffer_id, const fr_present_warp* warp, void* device_dst, size_t bytes) {
  return enqueue_device(c, "fr_present_enqueue_warped_device", buffer_id, nullptr, false, warp, true, device_dst, bytes);
}

int fr_present_blend_default(fr_ctx* c, fr_present_blend* blend) {
  if (!c || !blend) return FR_E_INVALID;
  blend->inner_buffer = FR_BUF_SIBSON;
  blend->outer_buffer = FR_BUF_ATROUS;
  blend->gaze[0] = c->U.gaze.x;
  blend->gaze[1] = c->U.gaze.y;
  blend->inner_radius_px = c->fov.radius_px;
  blend->outer_radius_px = 2.0f * blend->inner_radius_px;
  return FR_OK;
}

int fr_present_blend_pack(const float* inner, const float* outer, int width, int height, int format,
                          const fr_present_blend* blend, const fr_present_warp* warp, uint8_t* out) {
  if (!inner || !outer || !out || width < 1 || height < 1 || width > 32767 || height > 32767 || !format_ok(format))
    return FR_E_INVALID;
  int ow = width, oh = height;
  if (warp && !warp_ok(warp, width, height, &ow, &oh)) return FR_E_INVALID;
  PresentBlend b;
  if (!blend_ok(blend, &b)) return FR_E_INVALID;
  const bool bgra = (format & ~FR_PRESENT_TOP_DOWN) == FR_PRESENT_BGRA8, top_down = (format & FR_PRESENT_TOP_DOWN) != 0;
  const auto texel = [width](const float* img) {
    return [img, width](int i, int row) {
      const float* t = img + ((size_t)row * width + i) * 4;
      return mk4(t[0], t[1], t[2], t[3]);
    };
  };
  const auto fi = texel(inner), fo = texel(outer);
  const auto fetch = [&fi, &fo, &b](int i, int row) { return present_blend_fetch(fi, fo, i, row, b); };
  for (int r = 0; r < oh; r++) {
    const int y = top_down ? oh - 1 - r : r;
    uint8_t* o = out + (size_t)r * ow * 4;
    for (int x = 0; x < ow; x++) {
      const uint32_t w = warp ? present_warp_texel(fetch, width, height, warp->h, x, y, bgra) : present_texel(fetch(x, y), bgra);
      o[4 * x] = (uint8_t)w; o[4 * x + 1] = (uint8_t)(w >> 8); o[4 * x + 2] = (uint8_t)(w >> 16); o[4 * x + 3] = (uint8_t)(w >> 24);
    }
  }
  return FR_OK;
}

int fr_present_enqueue_blended(fr_ctx* c, const fr_present_blend* blend, const fr_present_warp* warp, uint64_t* ticket) {
  return enqueue_host(c, "fr_present_enqueue_blended", 0, blend, true, warp, warp != nullptr, ticket);
}

int fr_present_enqueue_blended_device(fr_ctx* c, const fr_present_blend* blend, const fr_present_warp* warp, void* device_dst,
                                      size_t bytes) {
  return enqueue_device(c, "fr_present_enqueue_blended_device", 0, blend, true, warp, warp != nullptr, device_dst, bytes);
}

int fr_present_reproject_pack(const float* rgba, const float* position, int width, int height, int format,
                              const fr_present_reproject* rp, uint8_t* out) {
  if (!rgba || !position || !out || width < 1 || height < 1 || width > 32767 || height > 32767 || !format_ok(format))
    return FR_E_INVALID;
  int ow, oh;
  if (!reproject_ok(rp, width, height, &ow, &oh)) return FR_E_INVALID;
  const bool bgra = (format & ~FR_PRESENT_TOP_DOWN) == FR_PRESENT_BGRA8, top_down = (format & FR_PRESENT_TOP_DOWN) != 0;
  const auto texel = [width](const float* img) {
    return [img, width](int i, int row) {
      const float* t = img + ((size_t)row * width + i) * 4;
      return mk4(t[0], t[1], t[2], t[3]);
    };
  };
  const auto fetch = texel(rgba), fpos = texel(position);
  std::vector<uint64_t> keys((size_t)ow * oh, PRESENT_KEY_EMPTY);  // the clear
  for (int j = 0; j < height; j++)                                   // the splat
    for (int i = 0; i < width; i++) {
      int ox, oy;
      uint32_t depth;
      if (!present_splat_place(fpos(i, j), rp->vp, ow, oh, &ox, &oy, &depth)) continue;
      const uint64_t key = present_splat_key(depth, present_texel(fetch(i, j), bgra));
      uint64_t& k = keys[(size_t)oy * ow + ox];
      if (key < k) k = key;
    }
  const auto key = [&keys, ow](int i, int row) { return keys[(size_t)row * ow + i]; };
  for (int r = 0; r < oh; r++) {  // the resolve
    const int y = top_down ? oh - 1 - r : r;
    uint8_t* o = out + (size_t)r * ow * 4;
    for (int x = 0; x < ow; x++) {
      uint32_t w;
      if (!present_resolve_word(key(x, y), key, ow, oh, x, y, &w)) w = present_warp_texel(fetch, width, height, rp->fallback.h, x, y, bgra);
      o[4 * x] = (uint8_t)w; o[4 * x + 1] = (uint8_t)(w >> 8); o[4 * x + 2] = (uint8_t)(w >> 16); o[4 * x + 3] = (uint8_t)(w >> 24);
    }
  }
  return FR_OK;
}

int fr_present_reproject_enable(fr_ctx* c, int on) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_present_reproject_enable";
  fr_ctx::Present& P = c->present;
  if (!on) {
    P.reproject = false;
    return FR_OK;
  }
  if (P.ring.n == 0) return fail(c, FR_E_STATE, name + ": presenting is not enabled (fr_present_enable)");
  if (!P.keys) {
    if (int rc = quiesce(c)) return rc;
    if (int rc = present_sync(c)) return rc;
    hipSetDevice(c->cfg.device);
    void* k = nullptr;
    if (hipMalloc(&k, (size_t)c->W * c->H * sizeof(unsigned long long)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, FR_E_NOMEM, name + ": allocation failed (nothing is kept, reprojected presents are off)");
    }
    P.keys = static_cast<unsigned long long*>(k);
  }
  P.reproject = true;
  return FR_OK;
}

int fr_present_enqueue_reprojected(fr_ctx* c, int buffer_id, const fr_present_reproject* rp, uint64_t* ticket) {
  return enqueue_host(c, "fr_present_enqueue_reprojected", buffer_id, nullptr, false, nullptr, false, ticket, rp, true);
}

int fr_present_enqueue_reprojected_device(fr_ctx* c, int buffer_id, const fr_present_reproject* rp, void* device_dst,
                                          size_t bytes) {
  return enqueue_device(c, "fr_present_enqueue_reprojected_device", buffer_id, nullptr, false, nullptr, false, device_dst,
                        bytes, rp, true);
}

int fr_present_done(fr_ctx* c, void* stream) {
  if (!c) return FR_E_INVALID;
  if (c->present.ring.n == 0) return fail(c, FR_E_STATE, "fr_present_done: presenting is not enabled (fr_present_enable)");
  if (!c->present_dev.pending) return FR_OK;
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, c->present_dev.peek(static_cast<hipStream_t>(stream)));
  return FR_OK;
}

}  // extern "C"
