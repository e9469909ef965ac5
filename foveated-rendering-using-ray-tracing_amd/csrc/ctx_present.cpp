// ctx_present.cpp — present: a reconstructed image as packed 8-bit texels, in stream order. Every form goes to host
// memory through a ring of pinned images (fr_present_enable, fr_present_enqueue*, fr_present_acquire,
// fr_present_release; the ring's bookkeeping is PresentRing, present_ring.h; a slot carries ow * oh * 4 bytes to the
// host, no more) or into the caller's device memory (fr_present_enqueue*_device, fr_present_done). One checked Request
// (check_request) says what to pack, enqueue_pack launches it, and each form's rule runs on the host as well.
//
//   form         kernels (k_present.hip, k_present_reproject.hip)         reads                        host rule
//   Plain        k_present_pack                                           one image                    fr_present_pack
//   Warped       k_present_warp (late reprojection, crop, scale)          one image                    fr_present_warp_pack
//   Blended      k_present_blend; k_present_blend_warp with a warp        two, mixed around a gaze     fr_present_blend_pack
//   Reprojected  a clear of the key image, k_present_splat, _resolve      one image and POSITION       fr_present_reproject_pack
//
// The fence recorded behind the kernels is present_read_shd of the frame slot for a source that is the slot's SHADING
// and present_read for any other; Blended records the fence of each of its sources. Reprojected records
// present_read_shd whatever the source is: POSITION's next writers (the front stages of the frame that takes the slot
// next; a stage call, a write or a restore through join_recon) wait for it already.
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
#include "k_present.h"

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
const char* const kBadWarp = ": the warp is NULL, has a non-finite coefficient or an output size outside 1..W x 1..H";
const char* const kReprojectOff = ": reprojected presents are not enabled (fr_present_reproject_enable)";
const char* const kBadBlend =
    ": the blend is NULL, has a non-finite gaze or radius, a negative radius, inner > outer, or an outer radius whose "
    "square is not finite";
const char* const kRingOff = ": presenting is not enabled (fr_present_enable)";

enum class Form { Plain, Warped, Blended, Reprojected };

// A checked present: the physical image to pack, or (Blended) the two that `blend` mixes, `phys` inside; h: the
// homography (Warped, Reprojected: the fallback; Blended: when a warp was given), else NULL; vp: Reprojected only;
// ow x oh: the output. h and vp point into the caller's structs: the launches copy them, nothing is read after the call.
struct Request {
  Form form = Form::Plain;
  int phys = -1, outer = -1;
  PresentBlend blend{};
  const float *h = nullptr, *vp = nullptr;
  int ow = 0, oh = 0;
};
struct DeviceDst { void* ptr; size_t bytes; };  // where a device form writes; the host forms have none

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

// What every enqueue refuses before anything is enqueued, and *req from what it takes. The order of the refusals is
// part of the interface, the same for the eight entry points: 1. a NULL context or ticket (the callers, before this);
// 2. the reprojection (Reprojected) or the warp (Warped; Blended when one is given); 3. device forms only (dev):
// device_dst, then bytes; 4. the blend (Blended; buffer_id is not used, the images are the blend's); 5. the buffer
// ids; 6. a rank of a group, or sharded; 7. the ring is off; 8. reprojected presents are not enabled (Reprojected);
// 9. every slot of the ring is held (enqueue_host, after this).
int check_request(fr_ctx* c, const std::string& name, Form form, int buffer_id, const fr_present_blend* blend,
                  const fr_present_warp* warp, const fr_present_reproject* rp, const DeviceDst* dev, Request* req) {
  req->form = form;
  req->ow = c->W;
  req->oh = c->H;
  if (form == Form::Reprojected) {
    if (!reproject_ok(rp, c->W, c->H, &req->ow, &req->oh)) return fail(c, FR_E_INVALID, name + kBadReproject);
    req->vp = rp->vp;
    req->h = rp->fallback.h;
  } else if (form == Form::Warped || (form == Form::Blended && warp)) {
    if (!warp_ok(warp, c->W, c->H, &req->ow, &req->oh)) return fail(c, FR_E_INVALID, name + kBadWarp);
    req->h = warp->h;
  }
  if (dev) {
    if (!dev->ptr || (reinterpret_cast<uintptr_t>(dev->ptr) & 15u))
      return fail(c, FR_E_INVALID, name + ": device_dst is NULL or not 16-byte aligned");
    if (dev->bytes != (size_t)req->ow * req->oh * 4) return fail(c, FR_E_INVALID, name + ": bytes != the output's width * height * 4");
  }
  const bool blended = form == Form::Blended;
  if (blended && !blend_ok(blend, &req->blend)) return fail(c, FR_E_INVALID, name + kBadBlend);
  req->phys = presentable(c, blended ? blend->inner_buffer : buffer_id);
  req->outer = blended ? presentable(c, blend->outer_buffer) : req->phys;
  if (req->phys < 0 || req->outer < 0)
    return fail(c, FR_E_INVALID, name + ": the buffer is not FR_BUF_SHADING, FR_BUF_SIBSON, FR_BUF_PULLPUSH or FR_BUF_ATROUS");
  if (c->group_refs > 0 || c->U.shard_count > 1)
    return fail(c, FR_E_UNSUPPORTED, name + ": the context is a rank of a group or sharded");
  if (c->present.ring.n == 0) return fail(c, FR_E_STATE, name + kRingOff);
  if (form == Form::Reprojected && !c->present.reproject) return fail(c, FR_E_STATE, name + kReprojectOff);
  return FR_OK;
}

// The present stream behind what wrote the image (the head of this file), then the pack into dst, then the fence
// its next writer waits for (the table at the head of this file). begin / packed: a slot's timing events, or NULL.
int enqueue_pack(fr_ctx* c, const Request& req, void* dst, hipEvent_t begin, hipEvent_t packed) {
  fr_ctx::Present& P = c->present;
  HIP_TRY(c, hipEventRecord(P.ev_fork, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(P.stream, P.ev_fork, 0));
  for (const Fence& f : c->recon_done) HIP_TRY(c, f.peek(P.stream));
  if (begin) HIP_TRY(c, hipEventRecord(begin, P.stream));
  const f4* src = c->img[req.phys];
  switch (req.form) {
    case Form::Plain: launch_present_pack(src, c->W, c->H, P.format, dst, P.stream); break;
    case Form::Warped: launch_present_warp(src, c->W, c->H, P.format, req.h, req.ow, req.oh, dst, P.stream); break;
    case Form::Blended:
      launch_present_blend(src, c->img[req.outer], c->W, c->H, P.format, req.blend, req.h, req.ow, req.oh, dst, P.stream);
      break;
    case Form::Reprojected:
      launch_present_reproject(src, c->img[P_pos(c)], c->W, c->H, P.format, req.vp, req.h, req.ow, req.oh, P.keys, dst, P.stream);
      break;
  }
  if (int rc = check_launch(c)) return rc;
  if (packed) HIP_TRY(c, hipEventRecord(packed, P.stream));
  const int shd = P_shd(c);
  if (req.form == Form::Reprojected || req.phys == shd || req.outer == shd) HIP_TRY(c, c->present_read_shd[c->slot].record(P.stream));
  if (req.phys != shd || req.outer != shd) HIP_TRY(c, c->present_read.record(P.stream));
  return FR_OK;
}

// The host forms: into the next free slot and on to its pinned image.
int enqueue_host(fr_ctx* c, const std::string& name, Form form, int buffer_id, const fr_present_blend* blend,
                 const fr_present_warp* warp, const fr_present_reproject* rp, uint64_t* ticket) {
  if (!c || !ticket) return FR_E_INVALID;
  Request req;
  if (int rc = check_request(c, name, form, buffer_id, blend, warp, rp, nullptr, &req)) return rc;
  fr_ctx::Present& P = c->present;
  uint64_t t = 0;
  const int s = P.ring.enqueue(&t);
  if (s < 0) return fail(c, FR_E_STATE, name + ": every slot of the ring is held (fr_present_release)");
  hipSetDevice(c->cfg.device);
  // (the slot's last copy is earlier work of the present stream: the pack overwrites the staging image behind it)
  int rc = enqueue_pack(c, req, P.stage[s], P.ev[s].begin, P.ev[s].packed);
  if (rc == FR_OK && hipMemcpyAsync(P.host[s], P.stage[s], (size_t)req.ow * req.oh * 4, hipMemcpyDeviceToHost, P.stream) != hipSuccess)
    rc = fail(c, FR_E_HIP, name + ": the copy to the host could not be enqueued");
  if (rc == FR_OK && hipEventRecord(P.ev[s].done, P.stream) != hipSuccess) rc = fail(c, FR_E_HIP, name + ": event record failed");
  if (rc != FR_OK) {
    P.ring.release(s);
    return rc;
  }
  *ticket = t;
  return FR_OK;
}

// The device forms: straight into the caller's memory, with the fence fr_present_done hands on.
int enqueue_device(fr_ctx* c, const std::string& name, Form form, int buffer_id, const fr_present_blend* blend,
                   const fr_present_warp* warp, const fr_present_reproject* rp, void* device_dst, size_t bytes) {
  if (!c) return FR_E_INVALID;
  const DeviceDst dev{device_dst, bytes};
  Request req;
  if (int rc = check_request(c, name, form, buffer_id, blend, warp, rp, &dev, &req)) return rc;
  hipSetDevice(c->cfg.device);
  if (int rc = enqueue_pack(c, req, device_dst, nullptr, nullptr)) return rc;
  HIP_TRY(c, c->present_dev.record(c->present.stream));
  return FR_OK;
}

// The slot of a ticket of the ring in place, for the calls that take one.
int slot_of(fr_ctx* c, const std::string& name, uint64_t ticket, int* s) {
  if (c->present.ring.n == 0) return fail(c, FR_E_STATE, name + kRingOff);
  *s = c->present.ring.find(ticket);
  if (*s < 0) return fail(c, FR_E_INVALID, name + ": unknown or released ticket");
  return FR_OK;
}

// What every host rule refuses: a NULL image or output, a size outside 1..32767, an unknown format.
bool rule_args_ok(int width, int height, int format, std::initializer_list<const void*> pointers) {
  for (const void* p : pointers) if (!p) return false;
  return width >= 1 && height >= 1 && width <= 32767 && height <= 32767 && format_ok(format);
}

// An RGBA32F image of `width` texels a row as the rules of fr_math.h fetch it.
auto image_fetch(const float* img, int width) {
  return [img, width](int i, int row) {
    const float* t = img + ((size_t)row * width + i) * 4;
    return mk4(t[0], t[1], t[2], t[3]);
  };
}

// The output side of every host rule: word(x, y) of image row y = r, or oh - 1 - r (top_down), as the four bytes of
// texel x of output row r.
template <class Word>
void pack_rows(int ow, int oh, bool top_down, uint8_t* out, Word word) {
  for (int r = 0; r < oh; r++) {
    const int y = top_down ? oh - 1 - r : r;
    uint8_t* o = out + (size_t)r * ow * 4;
    for (int x = 0; x < ow; x++) {
      const uint32_t w = word(x, y);
      o[4 * x] = (uint8_t)w; o[4 * x + 1] = (uint8_t)(w >> 8); o[4 * x + 2] = (uint8_t)(w >> 16); o[4 * x + 3] = (uint8_t)(w >> 24);
    }
  }
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
  if (!rule_args_ok(width, height, format, {rgba, out})) return FR_E_INVALID;
  const PresentFormat f = present_format(format);
  const auto fetch = image_fetch(rgba, width);
  pack_rows(width, height, f.top_down, out, [&](int x, int y) { return present_texel(fetch(x, y), f.bgra); });
  return FR_OK;
}

int fr_present_warp_pack(const float* rgba, int width, int height, int format, const fr_present_warp* warp, uint8_t* out) {
  if (!rule_args_ok(width, height, format, {rgba, out})) return FR_E_INVALID;
  int ow, oh;
  if (!warp_ok(warp, width, height, &ow, &oh)) return FR_E_INVALID;
  const PresentFormat f = present_format(format);
  const auto fetch = image_fetch(rgba, width);
  pack_rows(ow, oh, f.top_down, out, [&](int x, int y) { return present_warp_texel(fetch, width, height, warp->h, x, y, f.bgra); });
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
  return enqueue_host(c, "fr_present_enqueue", Form::Plain, buffer_id, nullptr, nullptr, nullptr, ticket);
}

int fr_present_enqueue_warped(fr_ctx* c, int buffer_id, const fr_present_warp* warp, uint64_t* ticket) {
  return enqueue_host(c, "fr_present_enqueue_warped", Form::Warped, buffer_id, nullptr, warp, nullptr, ticket);
}

int fr_present_acquire(fr_ctx* c, uint64_t ticket, int wait, const void** host) {
  if (!c || !host) return FR_E_INVALID;
  const std::string name = "fr_present_acquire";
  fr_ctx::Present& P = c->present;
  int s;
  if (int rc = slot_of(c, name, ticket, &s)) return rc;
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
  int s;
  if (int rc = slot_of(c, "fr_present_release", ticket, &s)) return rc;
  c->present.ring.release(s);
  return FR_OK;
}

int fr_present_times(fr_ctx* c, uint64_t ticket, float* pack_ms, float* copy_ms) {
  if (!c) return FR_E_INVALID;
  fr_ctx::Present& P = c->present;
  int s;
  if (int rc = slot_of(c, "fr_present_times", ticket, &s)) return rc;
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
  return enqueue_device(c, "fr_present_enqueue_device", Form::Plain, buffer_id, nullptr, nullptr, nullptr, device_dst, bytes);
}

int fr_present_enqueue_warped_device(fr_ctx* c, int buffer_id, const fr_present_warp* warp, void* device_dst, size_t bytes) {
  return enqueue_device(c, "fr_present_enqueue_warped_device", Form::Warped, buffer_id, nullptr, warp, nullptr, device_dst, bytes);
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
  if (!rule_args_ok(width, height, format, {inner, outer, out})) return FR_E_INVALID;
  int ow = width, oh = height;
  if (warp && !warp_ok(warp, width, height, &ow, &oh)) return FR_E_INVALID;
  PresentBlend b;
  if (!blend_ok(blend, &b)) return FR_E_INVALID;
  const PresentFormat f = present_format(format);
  const auto fi = image_fetch(inner, width), fo = image_fetch(outer, width);
  const auto fetch = [&fi, &fo, &b](int i, int row) { return present_blend_fetch(fi, fo, i, row, b); };
  pack_rows(ow, oh, f.top_down, out, [&](int x, int y) {
    return warp ? present_warp_texel(fetch, width, height, warp->h, x, y, f.bgra) : present_texel(fetch(x, y), f.bgra);
  });
  return FR_OK;
}

int fr_present_enqueue_blended(fr_ctx* c, const fr_present_blend* blend, const fr_present_warp* warp, uint64_t* ticket) {
  return enqueue_host(c, "fr_present_enqueue_blended", Form::Blended, 0, blend, warp, nullptr, ticket);
}

int fr_present_enqueue_blended_device(fr_ctx* c, const fr_present_blend* blend, const fr_present_warp* warp, void* device_dst,
                                      size_t bytes) {
  return enqueue_device(c, "fr_present_enqueue_blended_device", Form::Blended, 0, blend, warp, nullptr, device_dst, bytes);
}

int fr_present_reproject_pack(const float* rgba, const float* position, int width, int height, int format,
                              const fr_present_reproject* rp, uint8_t* out) {
  if (!rule_args_ok(width, height, format, {rgba, position, out})) return FR_E_INVALID;
  int ow, oh;
  if (!reproject_ok(rp, width, height, &ow, &oh)) return FR_E_INVALID;
  const PresentFormat f = present_format(format);
  const auto fetch = image_fetch(rgba, width), fpos = image_fetch(position, width);
  std::vector<uint64_t> keys((size_t)ow * oh, PRESENT_KEY_EMPTY);  // the clear
  for (int j = 0; j < height; j++)                                   // the splat
    for (int i = 0; i < width; i++) {
      int ox, oy;
      uint32_t depth;
      if (!present_splat_place(fpos(i, j), rp->vp, ow, oh, &ox, &oy, &depth)) continue;
      const uint64_t key = present_splat_key(depth, present_texel(fetch(i, j), f.bgra));
      uint64_t& k = keys[(size_t)oy * ow + ox];
      if (key < k) k = key;
    }
  const auto key = [&keys, ow](int i, int row) { return keys[(size_t)row * ow + i]; };
  pack_rows(ow, oh, f.top_down, out, [&](int x, int y) {  // the resolve
    uint32_t w;
    if (!present_resolve_word(key(x, y), key, ow, oh, x, y, &w)) w = present_warp_texel(fetch, width, height, rp->fallback.h, x, y, f.bgra);
    return w;
  });
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
  if (P.ring.n == 0) return fail(c, FR_E_STATE, name + kRingOff);
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
  return enqueue_host(c, "fr_present_enqueue_reprojected", Form::Reprojected, buffer_id, nullptr, nullptr, rp, ticket);
}

int fr_present_enqueue_reprojected_device(fr_ctx* c, int buffer_id, const fr_present_reproject* rp, void* device_dst,
                                          size_t bytes) {
  return enqueue_device(c, "fr_present_enqueue_reprojected_device", Form::Reprojected, buffer_id, nullptr, nullptr, rp, device_dst,
                        bytes);
}

int fr_present_done(fr_ctx* c, void* stream) {
  if (!c) return FR_E_INVALID;
  if (c->present.ring.n == 0) return fail(c, FR_E_STATE, std::string("fr_present_done") + kRingOff);
  if (!c->present_dev.pending) return FR_OK;
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, c->present_dev.peek(static_cast<hipStream_t>(stream)));
  return FR_OK;
}

}  // extern "C"
