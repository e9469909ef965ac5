// fovrt.hpp — header-only C++ facades over the fovrt C ABI (include/fovrt.h) that keep the reference's
// class names, method names and argument order, so a main.cpp-shaped frame loop
// (FR/main.cpp:152-358) drives the MI355X engine with only type changes:
//
//   reference (CUDA/OptiX + GL)                      here
//   ------------------------------------------------ -------------------------------------------------
//   GLuint (texture name)                            fovrt::Texture (a buffer id of the context)
//   tracer->m_context["gaze_target"] + rtBufferMap   tracer->gaze_target()
//   tracer->m_context["ray_count"] + rtBufferMap     tracer->ray_count()
//   const GLuint* query, GLuint64* elapsed, int* done  same parameters; query is ignored, elapsed is the
//                                                    pass time in ns (HIP events), done is set to 1
//   optix::Exception                                 fovrt::Error (thrown by the facade, never by the ABI)
//
// FR/ = "/root/reference/Foveated Rendering using Ray Tracing/". The facades own nothing on the device:
// the fr_ctx of the PathTracer owns every buffer, the pass objects only name its outputs.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fovrt.h"

namespace fovrt {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc, fr_ctx* ctx, const char* what) {
  if (rc != FR_OK) {
    const char* msg = fr_last_error(ctx);
    throw Error(rc, std::string(what) + ": " + (msg ? msg : "error"));
  }
}

// fr_present_pack: the present rule on the host, without a device; rgba holds width * height * 4 floats
inline std::vector<uint8_t> present_pack(const std::vector<float>& rgba, int width, int height, int format = FR_PRESENT_RGBA8) {
  if (width < 1 || height < 1 || rgba.size() != (size_t)width * height * 4) throw Error(FR_E_INVALID, "present_pack: size");
  std::vector<uint8_t> out(rgba.size());
  if (int rc = fr_present_pack(rgba.data(), width, height, format, out.data())) throw Error(rc, "present_pack: bad size or format");
  return out;
}

// fr_present_warp with its constructors: the homography of a warped present (the rule is in fovrt.h under "Present")
struct PresentWarp : fr_present_warp {
  PresentWarp() : fr_present_warp{{1, 0, 0, 0, 1, 0, 0, 0, 1}, 0, 0} {}
  static PresentWarp identity() { return PresentWarp(); }
  // the out_width x out_height texels whose lower left texel is (x0, y0), rows bottom-up
  static PresentWarp crop(int x0, int y0, int out_width, int out_height) {
    PresentWarp w;
    w.h[2] = (float)x0; w.h[5] = (float)y0;
    w.out_width = out_width; w.out_height = out_height;
    return w;
  }
  // the whole width x height image as out_width x out_height texels
  static PresentWarp scale(int width, int height, int out_width, int out_height) {
    PresentWarp w;
    w.h[0] = (float)width / (float)out_width; w.h[4] = (float)height / (float)out_height;
    w.out_width = out_width; w.out_height = out_height;
    return w;
  }
  // fr_present_warp_from_poses: the late reprojection from the rendered camera to the display camera
  static PresentWarp from_poses(const fr_camera_pose& rendered, const fr_camera_pose& display, int width, int height,
                                int out_width, int out_height, float ndc_depth = 1.0f) {
    PresentWarp w;
    if (int rc = fr_present_warp_from_poses(&rendered, &display, width, height, out_width, out_height, ndc_depth, &w))
      throw Error(rc, "present_warp_from_poses: bad size or depth, a singular matrix, or a corner behind the rendered camera");
    return w;
  }
};

// fr_present_warp_pack: the warped present rule on the host; the result holds out_width * out_height * 4 bytes
inline std::vector<uint8_t> present_warp_pack(const std::vector<float>& rgba, int width, int height, const fr_present_warp& warp,
                                              int format = FR_PRESENT_RGBA8) {
  if (width < 1 || height < 1 || rgba.size() != (size_t)width * height * 4) throw Error(FR_E_INVALID, "present_warp_pack: size");
  const bool whole = warp.out_width == 0 && warp.out_height == 0;
  const int ow = whole ? width : warp.out_width, oh = whole ? height : warp.out_height;
  if (ow < 1 || oh < 1 || ow > width || oh > height) throw Error(FR_E_INVALID, "present_warp_pack: output size");
  std::vector<uint8_t> out((size_t)ow * oh * 4);
  if (int rc = fr_present_warp_pack(rgba.data(), width, height, format, &warp, out.data())) throw Error(rc, "present_warp_pack: bad format or warp");
  return out;
}

// fr_present_blend: the two sources, the gaze and the two radii of a blended present (the rule is in fovrt.h under
// "Present"); PathTracer::present_blend_default gives a context's own
struct PresentBlend : fr_present_blend {
  PresentBlend() : fr_present_blend{FR_BUF_SIBSON, FR_BUF_ATROUS, {0, 0}, 0, 0} {}
  PresentBlend(float gx, float gy, float inner_radius, float outer_radius, int inner = FR_BUF_SIBSON, int outer = FR_BUF_ATROUS)
      : fr_present_blend{inner, outer, {gx, gy}, inner_radius, outer_radius} {}
};

// fr_present_blend_pack: the blended present rule on the host; warp nullptr: width * height * 4 bytes, else the
// warp's out_width * out_height * 4
inline std::vector<uint8_t> present_blend_pack(const std::vector<float>& inner, const std::vector<float>& outer, int width,
                                               int height, const fr_present_blend& blend, const fr_present_warp* warp = nullptr,
                                               int format = FR_PRESENT_RGBA8) {
  if (width < 1 || height < 1 || inner.size() != (size_t)width * height * 4 || outer.size() != inner.size())
    throw Error(FR_E_INVALID, "present_blend_pack: size");
  const bool whole = !warp || (warp->out_width == 0 && warp->out_height == 0);
  const int ow = whole ? width : warp->out_width, oh = whole ? height : warp->out_height;
  if (ow < 1 || oh < 1 || ow > width || oh > height) throw Error(FR_E_INVALID, "present_blend_pack: output size");
  std::vector<uint8_t> out((size_t)ow * oh * 4);
  if (int rc = fr_present_blend_pack(inner.data(), outer.data(), width, height, format, &blend, warp, out.data()))
    throw Error(rc, "present_blend_pack: bad format, blend or warp");
  return out;
}

// fr_present_reproject: the display camera's proj * view and the fallback homography of a reprojected present (the
// rule is in fovrt.h under "Present")
struct PresentReproject : fr_present_reproject {
  PresentReproject() : fr_present_reproject{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, PresentWarp()} {}
  // fr_present_reproject_from_poses: `rendered` is the pose the frame was traced with, `display` the one it is shown for
  static PresentReproject from_poses(const fr_camera_pose& rendered, const fr_camera_pose& display, int width, int height,
                                     int out_width, int out_height, float ndc_depth = 1.0f) {
    PresentReproject r;
    if (int rc = fr_present_reproject_from_poses(&rendered, &display, width, height, out_width, out_height, ndc_depth, &r))
      throw Error(rc, "present_reproject_from_poses: bad size or depth, a singular matrix, or a corner behind the rendered camera");
    return r;
  }
};

// fr_present_reproject_pack: the reprojected present rule on the host; the result holds the fallback's
// out_width * out_height * 4 bytes (0, 0: width * height * 4)
inline std::vector<uint8_t> present_reproject_pack(const std::vector<float>& rgba, const std::vector<float>& position, int width,
                                                   int height, const fr_present_reproject& rp, int format = FR_PRESENT_RGBA8) {
  if (width < 1 || height < 1 || rgba.size() != (size_t)width * height * 4 || position.size() != rgba.size())
    throw Error(FR_E_INVALID, "present_reproject_pack: size");
  const bool whole = rp.fallback.out_width == 0 && rp.fallback.out_height == 0;
  const int ow = whole ? width : rp.fallback.out_width, oh = whole ? height : rp.fallback.out_height;
  if (ow < 1 || oh < 1 || ow > width || oh > height) throw Error(FR_E_INVALID, "present_reproject_pack: output size");
  std::vector<uint8_t> out((size_t)ow * oh * 4);
  if (int rc = fr_present_reproject_pack(rgba.data(), position.data(), width, height, format, &rp, out.data()))
    throw Error(rc, "present_reproject_pack: bad format or reprojection");
  return out;
}

// A GL texture name of the reference = a buffer id of the context here.
struct Texture {
  int id = -1;
  constexpr Texture() = default;
  constexpr explicit Texture(int i) : id(i) {}
  constexpr operator int() const { return id; }
};

using vec3 = std::array<float, 3>;
using quat = std::array<float, 4>;  // (w, x, y, z) like glm::quat
using mat4 = std::array<float, 16>; // row-major, v' = M v

// Camera (FR/Camera.h, FR/Camera.cpp): the subset the frame loop uses, glm-compatible math.
class Camera {
 public:
  enum ProjMode { PM_Perspective, PM_Ortho_Height, PM_Ortho_Width, PM_Ortho };

  Camera() {
    pose_.pos[0] = pose_.pos[1] = pose_.pos[2] = 0.0f;
    pose_.rot[0] = 1.0f; pose_.rot[1] = pose_.rot[2] = pose_.rot[3] = 0.0f;
    pose_.fovy_deg = 45.0f; pose_.znear = 0.1f; pose_.zfar = 500.1f; pose_.aspect = 1.0f;
    prev_ = pose_;
  }
  void setScreen(float w, float h) { screen_[0] = w; screen_[1] = h; }          // FR/Camera.cpp:18-21
  void setViewport(float, float, float w, float h) { pose_.aspect = w / h; }  // :23-27 (aspect = w / h)
  void setProjectMode(ProjMode mode, float fov_deg, float n, float f) {
    if (mode != PM_Perspective) throw Error(FR_E_UNSUPPORTED, "only PM_Perspective is used by the frame loop");
    pose_.fovy_deg = fov_deg; pose_.znear = n; pose_.zfar = f;
  }
  void setPosition(const vec3& p) { for (int i = 0; i < 3; i++) pose_.pos[i] = p[i]; }
  void setRotation(const quat& q) { for (int i = 0; i < 4; i++) pose_.rot[i] = q[i]; }
  void setTarget(const vec3& t) { target_ = t; }  // FR/Camera.cpp: stores the target only
  void lookAt(const vec3& target, const vec3& up = {0.0f, 1.0f, 0.0f}) {  // FR/Camera.cpp:73-83
    check(fr_camera_look_at(&pose_, target.data(), up.data()), nullptr, "Camera::lookAt");
    target_ = target;
  }
  vec3 getPosition() const { return {pose_.pos[0], pose_.pos[1], pose_.pos[2]}; }
  vec3 getTarget() const { return target_; }
  quat getRotation() const { return {pose_.rot[0], pose_.rot[1], pose_.rot[2], pose_.rot[3]}; }
  mat4 getVMat() const { mat4 v, p; check(fr_camera_matrices(&pose_, v.data(), p.data()), nullptr, "getVMat"); return v; }
  mat4 getPMat() const { mat4 v, p; check(fr_camera_matrices(&pose_, v.data(), p.data()), nullptr, "getPMat"); return p; }
  void setPrevState() { prev_ = pose_; has_prev_ = true; }  // FR/Camera.cpp:234-241

  // the uniforms update_optix_variables derives (FR/PathTracer.cpp:774-820)
  fr_camera uniforms(int width, int height) const {
    fr_camera c;
    check(fr_camera_uniforms(&pose_, has_prev_ ? &prev_ : &pose_, width, height, &c), nullptr, "Camera uniforms");
    for (int i = 0; i < 3; i++) c.target[i] = target_[i];
    return c;
  }
  const fr_camera_pose& pose() const { return pose_; }

 private:
  fr_camera_pose pose_{};
  fr_camera_pose prev_{};
  bool has_prev_ = false;
  vec3 target_{0.0f, 0.0f, 0.0f};
  float screen_[2] = {0.0f, 0.0f};
};

class PathTracer;

// `tracer->m_accumFrame` reads the frame counter; `tracer->m_accumFrame = 0` resets accumulation
// (FR/main.cpp:248, the only assignment the reference makes).
class AccumFrame {
 public:
  explicit AccumFrame(fr_ctx* const* ctx) : ctx_(ctx) {}
  operator unsigned int() const {
    uint32_t f = 0;
    check(fr_accum_frame(*ctx_, &f), *ctx_, "m_accumFrame");
    return f;
  }
  AccumFrame& operator=(unsigned int v) {
    if (v != 0) throw Error(FR_E_UNSUPPORTED, "m_accumFrame can only be reset to 0");
    check(fr_reset_accumulation(*ctx_), *ctx_, "m_accumFrame = 0");
    return *this;
  }

 private:
  fr_ctx* const* ctx_;
};

// PathTracer (FR/PathTracer.h:10-110): the four launches, texture access and frame counter.
class PathTracer {
 public:
  enum TextureName { POSITION, NORMAL, DEPTH, DIFFUSE, WEIGHT, THREAD, HISTORY, SHADING, EXTRA };

  PathTracer() { fr_config_default(&cfg_); }  // cfg.abi_version = FOVRT_ABI_VERSION
  explicit PathTracer(const fr_config& cfg) : cfg_(cfg) {}
  PathTracer(const PathTracer&) = delete;
  PathTracer& operator=(const PathTracer&) = delete;
  virtual ~PathTracer() { if (ctx_) fr_destroy(ctx_); }

  bool initialize(int width, int height) {  // FR/PathTracer.cpp:41-78
    cfg_.width = width; cfg_.height = height;
    if (ctx_) { fr_destroy(ctx_); ctx_ = nullptr; }
    if (fr_create(&cfg_, &ctx_) != FR_OK) { error_ = fr_last_error(nullptr); ctx_ = nullptr; return false; }
    return true;
  }
  const std::string& initialize_error() const { return error_; }
  void init_camera(const Camera& camera) { update_optix_variables(camera); }  // :606-632
  void update_optix_variables(const Camera& camera) {                        // :774-820
    fr_camera c = camera.uniforms(cfg_.width, cfg_.height);
    check(fr_set_camera(ctx(), &c), ctx_, "update_optix_variables");
  }
  float geometry_launch() { float ms = 0; check(fr_geometry_launch(ctx(), &ms), ctx_, "geometry_launch"); return ms; }
  float sampling_launch() { float ms = 0; check(fr_sampling_launch(ctx(), &ms), ctx_, "sampling_launch"); return ms; }
  float optimize_launch() { float ms = 0; check(fr_optimize_launch(ctx(), &ms), ctx_, "optimize_launch"); return ms; }
  float shading_launch() { float ms = 0; check(fr_shading_launch(ctx(), &ms), ctx_, "shading_launch"); return ms; }

  Texture get_texture(TextureName name) const { return Texture((int)name); }  // :337-374

  vec3 gaze_target() {  // m_context["gaze_target"] (FR/main.cpp:278-287)
    vec3 g;
    check(fr_gaze_target(ctx(), g.data()), ctx_, "gaze_target");
    return g;
  }
  float rebuild_bvh() {  // the context's GPU builder (LBVH; binned SAH with bvh_builder 2) over the current triangles, wall ms
    float ms = 0.0f;
    check(fr_rebuild_bvh(ctx(), &ms), ctx_, "rebuild_bvh");
    return ms;
  }
  void set_positions(const float* xyz, size_t ntris) {  // moved vertices + GPU rebuild (fr_set_positions)
    check(fr_set_positions(ctx(), xyz, ntris), ctx_, "set_positions");
  }
  float refit_bvh() {  // same topology, new boxes and leaf triangles (fr_refit_bvh), wall ms
    float ms = 0.0f;
    check(fr_refit_bvh(ctx(), &ms), ctx_, "refit_bvh");
    return ms;
  }
  // moved vertices from host or device memory (FR_MEM_*), then a rebuild or a refit (FR_BVH_*)
  void update_positions(const void* xyz, size_t ntris, int where, int how) {
    check(fr_update_positions(ctx(), xyz, ntris, where, how), ctx_, "update_positions");
  }
  // update_positions plus the shading normals (FR_NORMALS_*): kept, given (nrm: 9 floats per triangle, the
  // memory kind of xyz) or recomputed from the new positions over the scene's smooth vertices
  void update_geometry(const void* xyz, const void* nrm, size_t ntris, int where, int how, int normals) {
    check(fr_update_geometry(ctx(), xyz, nrm, ntris, where, how, normals), ctx_, "update_geometry");
  }
  // update_geometry (device arrays, refit) in stream order, without waiting for the GPU. ready_event: a hipEvent_t
  // recorded after the arrays were produced, or nullptr; a bad array is rejected on the device
  // (geometry_update_status). The arrays stay untouched until geometry_consumed has ordered a stream behind the
  // update's reads of them.
  void update_geometry_enqueue(const void* xyz, const void* nrm, size_t ntris, int normals, void* ready_event = nullptr) {
    check(fr_update_geometry_enqueue(ctx(), xyz, nrm, ntris, normals, ready_event), ctx_, "update_geometry_enqueue");
  }
  void geometry_consumed(void* stream = nullptr) {  // stream: a hipStream_t (nullptr: the null stream); no host wait
    check(fr_geometry_consumed(ctx(), stream), ctx_, "geometry_consumed");
  }
  // enqueued updates (and enqueued poses) refit into a second tree and second normals beside the previous frame's
  // path trace (fr_set_geometry_overlap; off by default, 64 B per triangle at the first on; waits for pending work)
  void set_geometry_overlap(bool on) {
    check(fr_set_geometry_overlap(ctx(), on ? 1 : 0), ctx_, "set_geometry_overlap");
  }
  // enqueued updates applied / rejected on the device since the context was created (waits for pending work)
  void geometry_update_status(uint64_t* applied, uint64_t* rejected) {
    check(fr_geometry_update_status(ctx(), applied, rejected), ctx_, "geometry_update_status");
  }
  // fr_rebuild_bvh_enqueue: rebuild_bvh in stream order, without waiting for the GPU (compose it with an enqueued
  // update or pose). A build that fails on the device keeps the tree in use: bvh_rebuild_status counts it.
  void rebuild_bvh_enqueue() { check(fr_rebuild_bvh_enqueue(ctx()), ctx_, "rebuild_bvh_enqueue"); }
  void bvh_rebuild_status(uint64_t* built, uint64_t* failed) {
    check(fr_bvh_rebuild_status(ctx(), built, failed), ctx_, "bvh_rebuild_status");
  }
  // fr_rebuild_bvh_enqueue_if: rebuild_bvh_enqueue when the device finds the tree's SAH cost above ratio times its
  // baseline (the rule is in fovrt.h); set_rebuild_policy has the context make that call after every period-th
  // enqueued update or pose (period 0: off). bvh_rebuild_policy_status: conditional calls evaluated and skipped, the
  // cost evaluated last and the baseline (waits for pending work; any pointer may be null).
  void rebuild_bvh_enqueue_if(float ratio) {
    check(fr_rebuild_bvh_enqueue_if(ctx(), ratio), ctx_, "rebuild_bvh_enqueue_if");
  }
  void set_rebuild_policy(float ratio, int period) {
    check(fr_set_rebuild_policy(ctx(), ratio, period), ctx_, "set_rebuild_policy");
  }
  void bvh_rebuild_policy_status(uint64_t* evaluated, uint64_t* skipped, float* last_cost, float* base_cost) {
    check(fr_bvh_rebuild_policy_status(ctx(), evaluated, skipped, last_cost, base_cost), ctx_,
          "bvh_rebuild_policy_status");
  }
  // The scene's models (load_obj's meshes, FR/PathTracer.cpp:604-772): contiguous triangle ranges in scene order.
  struct Model {
    std::string name;
    int first_tri, ntris;
  };
  std::vector<Model> models() {
    int n = 0;
    check(fr_model_count(ctx(), &n), ctx_, "models");
    std::vector<Model> out(static_cast<size_t>(n));
    for (int i = 0; i < n; i++) {
      const char* name = nullptr;
      check(fr_model_info(ctx(), i, &name, &out[i].first_tri, &out[i].ntris), ctx_, "models");
      out[i].name = name;
    }
    return out;
  }
  // Ray queries (fr_trace_rays): a batch of rays against the scene as of the call's place in the stream order.
  // The host forms reserve the staging area on demand and wait for the answers; a miss is (inf, 0, 0, -1).
  void ray_query_reserve(size_t n) {
    check(fr_ray_query_reserve(ctx(), n), ctx_, "ray_query_reserve");
  }
  std::vector<fr_ray_hit> trace_rays(const std::vector<fr_ray>& rays) {
    std::vector<fr_ray_hit> out(rays.size());
    ray_query_reserve(rays.size());  // (allocates only when the request grows)
    check(fr_trace_rays(ctx(), rays.data(), rays.size(), FR_MEM_HOST, FR_RAYS_CLOSEST, out.data()), ctx_, "trace_rays");
    return out;
  }
  std::vector<float> trace_transmittance(const std::vector<fr_ray>& rays) {
    std::vector<float> out(rays.size());
    ray_query_reserve(rays.size());  // (allocates only when the request grows)
    check(fr_trace_rays(ctx(), rays.data(), rays.size(), FR_MEM_HOST, FR_RAYS_TRANSMITTANCE, out.data()), ctx_,
          "trace_transmittance");
    return out;
  }
  // device arrays (n fr_ray; n fr_ray_hit or n floats by kind), waiting for the answers
  void trace_rays(const void* rays, size_t n, int kind, void* out) {
    check(fr_trace_rays(ctx(), rays, n, FR_MEM_DEVICE, kind, out), ctx_, "trace_rays");
  }
  // ... and without waiting for the GPU; the arrays stay untouched until rays_consumed has ordered a stream (a
  // hipStream_t; nullptr: the null stream) behind the query
  void trace_rays_enqueue(const void* rays, size_t n, int kind, void* out, void* ready_event = nullptr) {
    check(fr_trace_rays_enqueue(ctx(), rays, n, kind, out, ready_event), ctx_, "trace_rays_enqueue");
  }
  void rays_consumed(void* stream = nullptr) { check(fr_rays_consumed(ctx(), stream), ctx_, "rays_consumed"); }
  // The surface at the hit (FR_RAYS_SURFACE) and per-ray model masks (fr_trace_rays_masked): masks holds one word
  // per ray, bit k set: model k of models() takes part in that ray; an empty masks vector is the unmasked query.
  void ray_query_reserve_kind(size_t n, int kind, bool masked) {
    check(fr_ray_query_reserve_kind(ctx(), n, kind, masked ? 1 : 0), ctx_, "ray_query_reserve_kind");
  }
  std::vector<fr_ray_surface> trace_surface(const std::vector<fr_ray>& rays, const std::vector<uint32_t>& masks = {}) {
    std::vector<fr_ray_surface> out(rays.size());
    trace_masked(rays, masks, FR_RAYS_SURFACE, out.data(), "trace_surface");
    return out;
  }
  std::vector<fr_ray_hit> trace_rays(const std::vector<fr_ray>& rays, const std::vector<uint32_t>& masks) {
    std::vector<fr_ray_hit> out(rays.size());
    trace_masked(rays, masks, FR_RAYS_CLOSEST, out.data(), "trace_rays");
    return out;
  }
  std::vector<float> trace_transmittance(const std::vector<fr_ray>& rays, const std::vector<uint32_t>& masks) {
    std::vector<float> out(rays.size());
    trace_masked(rays, masks, FR_RAYS_TRANSMITTANCE, out.data(), "trace_transmittance");
    return out;
  }
  // device arrays (masks: n words or nullptr), waiting for the answers, and in stream order
  void trace_rays(const void* rays, const uint32_t* masks, size_t n, int kind, void* out) {
    check(fr_trace_rays_masked(ctx(), rays, masks, n, FR_MEM_DEVICE, kind, out), ctx_, "trace_rays");
  }
  void trace_rays_enqueue(const void* rays, const uint32_t* masks, size_t n, int kind, void* out,
                          void* ready_event = nullptr) {
    check(fr_trace_rays_masked_enqueue(ctx(), rays, masks, n, kind, out, ready_event), ctx_, "trace_rays_enqueue");
  }
  // triangle indices (fr_ray_hit::prim) to model indices, the order of models(); -1 for a miss
  std::vector<int> model_of(const std::vector<int32_t>& prims) {
    const std::vector<Model> ms = models();
    std::vector<int> out(prims.size(), -1);
    for (size_t k = 0; k < prims.size(); k++)
      for (size_t i = 0; i < ms.size(); i++)
        if (prims[k] >= ms[i].first_tri && prims[k] < ms[i].first_tri + ms[i].ntris) out[k] = static_cast<int>(i);
    return out;
  }
  // Poses by matrix (fr_set_model_transforms): enable captures the current geometry as rest; m holds one row-major
  // 3 x 4 matrix per model (v' = A v + t over the rest geometry), posed on the device and taken as update_geometry
  // with given normals, or in stream order without waiting for the GPU (the enqueued form, always a refit).
  void enable_model_pose(bool on = true) { check(fr_model_pose_enable(ctx(), on ? 1 : 0), ctx_, "enable_model_pose"); }
  void set_model_transforms(const std::vector<std::array<float, 12>>& m, int how = FR_BVH_REFIT) {
    check(fr_set_model_transforms(ctx(), m.empty() ? nullptr : m[0].data(), m.size(), how), ctx_, "set_model_transforms");
  }
  void set_model_transforms_enqueue(const std::vector<std::array<float, 12>>& m) {
    check(fr_set_model_transforms_enqueue(ctx(), m.empty() ? nullptr : m[0].data(), m.size()), ctx_,
          "set_model_transforms_enqueue");
  }
  std::vector<std::array<float, 12>> model_transforms() {  // the pose last submitted
    int n = 0;
    check(fr_model_count(ctx(), &n), ctx_, "model_transforms");
    std::vector<std::array<float, 12>> m(static_cast<size_t>(n));
    check(fr_model_transforms(ctx(), n ? m[0].data() : nullptr, m.size()), ctx_, "model_transforms");
    return m;
  }
  // Per-model visibility (fr_set_model_visibility): bit k of `visible` clear hides model k of models() from every
  // frame and ray query, by a refit or a rebuild over the collapsed positions, or in stream order without waiting for
  // the GPU (the enqueued form, always a refit). model_visibility(): the mask last submitted, valid bits only.
  void enable_model_visibility(bool on = true) {
    check(fr_model_visibility_enable(ctx(), on ? 1 : 0), ctx_, "enable_model_visibility");
  }
  void set_model_visibility(uint32_t visible, int how = FR_BVH_REFIT) {
    check(fr_set_model_visibility(ctx(), visible, how), ctx_, "set_model_visibility");
  }
  void set_model_visibility_enqueue(uint32_t visible) {
    check(fr_set_model_visibility_enqueue(ctx(), visible), ctx_, "set_model_visibility_enqueue");
  }
  uint32_t model_visibility() {
    uint32_t v = 0;
    check(fr_model_visibility(ctx(), &v), ctx_, "model_visibility");
    return v;
  }
  // Foveation control (fr_set_mask_mode, fr_set_foveation, fr_set_sampling_mask). The mask mode changes at the next
  // sampling launch; FR_MASK_ECCENTRIC takes the parameters of set_foveation (ray_budget > 0: the device steers the
  // radius toward that many traced pixels, foveation_status waits and reports); FR_MASK_CALLER samples with the mask
  // last submitted: W * H bytes from host or device memory, or a device array in stream order without waiting for
  // the GPU (ready_event: a hipEvent_t or nullptr; the array stays untouched until sampling_mask_consumed has
  // ordered a stream behind the copy).
  void set_mask_mode(int mode) { check(fr_set_mask_mode(ctx(), mode), ctx_, "set_mask_mode"); }
  int mask_mode() {
    int m = 0;
    check(fr_get_mask_mode(ctx(), &m), ctx_, "mask_mode");
    return m;
  }
  fr_foveation foveation() {
    fr_foveation f;
    check(fr_get_foveation(ctx(), &f), ctx_, "foveation");
    return f;
  }
  void set_foveation(const fr_foveation& f) { check(fr_set_foveation(ctx(), &f), ctx_, "set_foveation"); }
  struct FoveationStatus { float r2; uint32_t last_count; uint64_t adjusted, held; };
  FoveationStatus foveation_status() {
    FoveationStatus s{};
    check(fr_foveation_status(ctx(), &s.r2, &s.last_count, &s.adjusted, &s.held), ctx_, "foveation_status");
    return s;
  }
  void enable_sampling_mask(bool on = true) { check(fr_sampling_mask_enable(ctx(), on ? 1 : 0), ctx_, "enable_sampling_mask"); }
  void set_sampling_mask(const std::vector<uint8_t>& mask) {
    check(fr_set_sampling_mask(ctx(), mask.data(), mask.size(), FR_MEM_HOST), ctx_, "set_sampling_mask");
  }
  void set_sampling_mask(const void* device_mask, size_t bytes) {
    check(fr_set_sampling_mask(ctx(), device_mask, bytes, FR_MEM_DEVICE), ctx_, "set_sampling_mask");
  }
  void set_sampling_mask_enqueue(const void* device_mask, size_t bytes, void* ready_event = nullptr) {
    check(fr_set_sampling_mask_enqueue(ctx(), device_mask, bytes, ready_event), ctx_, "set_sampling_mask_enqueue");
  }
  void sampling_mask_consumed(void* stream = nullptr) {
    check(fr_sampling_mask_consumed(ctx(), stream), ctx_, "sampling_mask_consumed");
  }
  // Present (fr_present_enable and the calls beside it): 8-bit frames in stream order. present() takes the buffer
  // (FR_BUF_SHADING, FR_BUF_SIBSON, FR_BUF_PULLPUSH or FR_BUF_ATROUS) as it stands at the call's place in the stream
  // order and returns its ticket without waiting for the GPU (Error with FR_E_STATE: every slot is held);
  // present_acquire gives the slot's pinned image, W * H * 4 bytes borrowed until present_release, or nullptr while
  // the frame is pending (wait = false only). present_to packs straight into device memory (16-byte aligned, W * H * 4
  // bytes); present_done orders a stream (a hipStream_t; nullptr: the null stream) behind the last such pack.
  void present_enable(int slots, int format = FR_PRESENT_RGBA8) {
    check(fr_present_enable(ctx(), slots, format), ctx_, "present_enable");
  }
  uint64_t present(int buffer) {
    uint64_t t = 0;
    check(fr_present_enqueue(ctx(), buffer, &t), ctx_, "present");
    return t;
  }
  const uint8_t* present_acquire(uint64_t ticket, bool wait = true) {
    const void* p = nullptr;
    const int rc = fr_present_acquire(ctx(), ticket, wait ? 1 : 0, &p);
    if (rc == FR_PRESENT_PENDING) return nullptr;
    check(rc, ctx_, "present_acquire");
    return static_cast<const uint8_t*>(p);
  }
  void present_release(uint64_t ticket) { check(fr_present_release(ctx(), ticket), ctx_, "present_release"); }
  struct PresentTimes { float pack_ms, copy_ms; };
  PresentTimes present_times(uint64_t ticket) {
    PresentTimes t{};
    check(fr_present_times(ctx(), ticket, &t.pack_ms, &t.copy_ms), ctx_, "present_times");
    return t;
  }
  void present_to(int buffer, void* device_dst, size_t bytes) {
    check(fr_present_enqueue_device(ctx(), buffer, device_dst, bytes), ctx_, "present_to");
  }
  void present_done(void* stream = nullptr) { check(fr_present_done(ctx(), stream), ctx_, "present_done"); }
  // The same through a homography (fr_present_enqueue_warped, fr_present_enqueue_warped_device): late reprojection,
  // crop, scale. The ticket's image, and `bytes` of the device form, are the warp's out_width * out_height * 4 bytes.
  uint64_t present_warped(int buffer, const fr_present_warp& warp) {
    uint64_t t = 0;
    check(fr_present_enqueue_warped(ctx(), buffer, &warp, &t), ctx_, "present_warped");
    return t;
  }
  void present_warped_to(int buffer, const fr_present_warp& warp, void* device_dst, size_t bytes) {
    check(fr_present_enqueue_warped_device(ctx(), buffer, &warp, device_dst, bytes), ctx_, "present_warped_to");
  }
  // A blended present (fr_present_enqueue_blended, fr_present_enqueue_blended_device): blend.inner_buffer around the
  // gaze, blend.outer_buffer in the periphery, their smoothstep mix between the radii; through `warp` when one is given.
  PresentBlend present_blend_default() {
    PresentBlend b;
    check(fr_present_blend_default(ctx(), &b), ctx_, "present_blend_default");
    return b;
  }
  uint64_t present_blended(const fr_present_blend& blend, const fr_present_warp* warp = nullptr) {
    uint64_t t = 0;
    check(fr_present_enqueue_blended(ctx(), &blend, warp, &t), ctx_, "present_blended");
    return t;
  }
  void present_blended_to(const fr_present_blend& blend, void* device_dst, size_t bytes, const fr_present_warp* warp = nullptr) {
    check(fr_present_enqueue_blended_device(ctx(), &blend, warp, device_dst, bytes), ctx_, "present_blended_to");
  }
  // A reprojected present (fr_present_reproject_enable, fr_present_enqueue_reprojected, _device): every texel moved to
  // where the display camera sees its POSITION, the fallback homography where nothing lands. After present_enable.
  void present_reproject_enable(bool on = true) {
    check(fr_present_reproject_enable(ctx(), on ? 1 : 0), ctx_, "present_reproject_enable");
  }
  uint64_t present_reprojected(int buffer, const fr_present_reproject& rp) {
    uint64_t t = 0;
    check(fr_present_enqueue_reprojected(ctx(), buffer, &rp, &t), ctx_, "present_reprojected");
    return t;
  }
  void present_reprojected_to(int buffer, const fr_present_reproject& rp, void* device_dst, size_t bytes) {
    check(fr_present_enqueue_reprojected_device(ctx(), buffer, &rp, device_dst, bytes), ctx_, "present_reprojected_to");
  }
  void set_normals(const void* nrm, size_t ntris, int where) {  // normals alone; positions and tree stay
    check(fr_set_normals(ctx(), nrm, ntris, where), ctx_, "set_normals");
  }
  float recompute_normals() {  // the normal rule over the current positions (fr_recompute_normals), wall ms
    float ms = 0.0f;
    check(fr_recompute_normals(ctx(), &ms), ctx_, "recompute_normals");
    return ms;
  }
  // history follows moving geometry: the G-buffer after a position update reprojects from the previous positions
  void set_motion_reprojection(bool on) {
    check(fr_set_motion_reprojection(ctx(), on ? 1 : 0), ctx_, "set_motion_reprojection");
  }
  // the smooth vertex of every corner 3 t + k (-1: the triangle has no normals); *nverts = their number
  std::vector<int32_t> normal_groups(int* nverts = nullptr) {
    fr_scene_arrays a;
    check(fr_scene_export(ctx(), &a), ctx_, "normal_groups");
    std::vector<int32_t> corner_vertex(3 * static_cast<size_t>(a.num_tris));
    check(fr_normal_groups(ctx(), corner_vertex.data(), corner_vertex.size(), nverts), ctx_, "normal_groups");
    return corner_vertex;
  }
  float bvh_sah_cost() {  // SAH cost of the tree in use (fr_bvh_sah_cost), lower is better
    float cost = 0.0f;
    check(fr_bvh_sah_cost(ctx(), &cost), ctx_, "bvh_sah_cost");
    return cost;
  }
  // cursorPosCallback (FR/gui.cpp:48-66): the cursor in window coordinates (y down); adjust_scale 1.25
  // in a window, 1 in full screen (g_fullScreen)
  void set_gaze(double xpos, double ypos, bool fullscreen = false) {
    check(fr_set_gaze(ctx(), xpos, ypos, fullscreen ? 1 : 0), ctx_, "set_gaze");
  }
  void reset_gaze() { check(fr_reset_gaze(ctx()), ctx_, "reset_gaze"); }  // framebufferSizeCallback (:32-35)
  unsigned int ray_count() {  // m_context["ray_count"] (FR/main.cpp:288-299)
    uint32_t n = 0;
    check(fr_ray_count(ctx(), &n), ctx_, "ray_count");
    return n;
  }

  // beyond the reference: whole-frame enqueue, buffer reads, statistics
  fr_frame_timing frame() { fr_frame_timing t{}; check(fr_frame(ctx(), &t), ctx_, "frame"); return t; }
  std::vector<float> read_rgba(Texture t) {
    std::vector<float> v((size_t)cfg_.width * cfg_.height * 4);
    check(fr_read_buffer(ctx(), t.id, v.data(), v.size() * sizeof(float)), ctx_, "read_rgba");
    return v;
  }
  fr_stats stats() { fr_stats s{}; check(fr_get_stats(ctx(), &s), ctx_, "stats"); return s; }
  // temporal state (history / depth pairs, pull-push atlases, m_accumFrame, camera) to host memory and back
  std::vector<uint8_t> snapshot() {
    size_t n = 0;
    check(fr_snapshot_bytes(ctx(), &n), ctx_, "snapshot");
    std::vector<uint8_t> v(n);
    check(fr_snapshot(ctx(), v.data(), v.size()), ctx_, "snapshot");
    return v;
  }
  void restore(const std::vector<uint8_t>& v) { check(fr_restore(ctx(), v.data(), v.size()), ctx_, "restore"); }
  // live per-launch HIP-event timing of the shading stage (off by default)
  void kernel_timing(bool on) { check(fr_kernel_timing(ctx(), on ? 1 : 0), ctx_, "kernel_timing"); }
  fr_stage_times kernel_times() { fr_stage_times t{}; check(fr_kernel_times(ctx(), &t), ctx_, "kernel_times"); return t; }
  // FR_PIPELINE_THROUGHPUT (frames back to back) or FR_PIPELINE_LATENCY (one trace half in flight)
  void set_pipeline_mode(int mode) { check(fr_set_pipeline_mode(ctx(), mode), ctx_, "set_pipeline_mode"); }
  // per-frame latency and display interval of pipelined frames (fr_frame_clock), in ms
  void frame_clock(bool on) { check(fr_frame_clock(ctx(), on ? 1 : 0), ctx_, "frame_clock"); }
  void frame_clock_read(std::vector<float>& latency_ms, std::vector<float>& interval_ms, int cap = 65536) {
    latency_ms.resize((size_t)cap);
    interval_ms.resize((size_t)cap);
    int nl = 0, ni = 0;
    check(fr_frame_clock_read(ctx(), latency_ms.data(), interval_ms.data(), cap, &nl, &ni), ctx_, "frame_clock_read");
    latency_ms.resize((size_t)nl);
    interval_ms.resize((size_t)ni);
  }
  fr_ctx* ctx() const {
    if (!ctx_) throw Error(FR_E_STATE, "PathTracer used before initialize()");
    return ctx_;
  }
  const fr_config& config() const { return cfg_; }

  AccumFrame m_accumFrame{&ctx_};

 private:
  // the host forms of the masked queries: reserve the staging area for the kind, then fr_trace_rays_masked
  void trace_masked(const std::vector<fr_ray>& rays, const std::vector<uint32_t>& masks, int kind, void* out,
                    const char* what) {
    if (!masks.empty() && masks.size() != rays.size()) throw std::invalid_argument("masks: one word per ray");
    ray_query_reserve_kind(rays.size(), kind, !masks.empty());  // (allocates only when the request grows)
    check(fr_trace_rays_masked(ctx(), rays.data(), masks.empty() ? nullptr : masks.data(), rays.size(), FR_MEM_HOST,
                               kind, out), ctx_, what);
  }
  fr_config cfg_{};
  fr_ctx* ctx_ = nullptr;
  std::string error_;
};

// GL pass classes (FR/JumpFlooding.h, FR/SibsonInterpolation.h, FR/PullPushInterpolation.h,
// FR/ATrous.h). They read the screen size from the tracer's context instead of g_screenSize.
namespace detail {
inline void finish(uint64_t ns, uint64_t* elapsed, int* done) {
  if (elapsed) *elapsed = ns;
  if (done) *done = 1;
}
}  // namespace detail

// GBuffer (FR/GBuffer.h:27-64): the reference constructs it and calls render() every frame
// (FR/main.cpp:153,255), but its constructor never builds the FBO, VAO or shader (FR/GBuffer.cpp:11-26)
// and nothing reads its textures; the G-buffer that feeds the path is OptiX entry 0
// (PathTracer::geometry_launch). The facade keeps those lines compiling: render() does no work and
// reports 0 ns, and the texture names are the "no texture" 0 of an unbuilt FBO.
class GBuffer {
 public:
  GBuffer() = default;
  void render(const unsigned* /*query*/ = nullptr, uint64_t* elapsed_time = nullptr, int* done = nullptr) {
    detail::finish(0, elapsed_time, done);
  }
  void BindBuffers() {}
  void resetFrameCount() {}
  void resetShader() {}
  void genScene() {}
  void loadMesh(const char*) {}
  void setupMesh() {}
  const Texture positionTex{};
  const Texture normalTex{};
  const Texture depthTex{};
  const unsigned fbo = 0;
};

class JumpFlooding {
 public:
  explicit JumpFlooding(PathTracer& t) : t_(t) {}
  void render(Texture rt, const unsigned* /*query*/ = nullptr, uint64_t* elapsed_time = nullptr, int* done = nullptr) {
    uint64_t ns = 0;
    check(fr_jfa_render(t_.ctx(), rt.id, &ns), t_.ctx(), "JumpFlooding::render");
    detail::finish(ns, elapsed_time, done);
  }
  void resetShader() {}
  const Texture coordTex{FR_BUF_JFA_COORD};
  const Texture colorTex{FR_BUF_JFA_COLOR};

 private:
  PathTracer& t_;
};

class LogPolarTransform {  // FR/Log_Polar_Transform.h
 public:
  explicit LogPolarTransform(PathTracer& t) : t_(t) {}
  void render(Texture pt, const unsigned* = nullptr, uint64_t* elapsed_time = nullptr, int* done = nullptr) {
    uint64_t ns = 0;
    check(fr_logpolar_render(t_.ctx(), pt.id, &ns), t_.ctx(), "LogPolarTransform::render");
    detail::finish(ns, elapsed_time, done);
  }
  void resetShader() {}
  const Texture logPolarTex{FR_BUF_LOGPOLAR};
  const Texture ilogPolarTex{FR_BUF_LOGPOLAR_INVERSE};

 private:
  PathTracer& t_;
};

class SibsonInterpolation {
 public:
  explicit SibsonInterpolation(PathTracer& t) : t_(t) {}
  void render(Texture coord, Texture color, const unsigned* = nullptr, uint64_t* elapsed_time = nullptr,
              int* done = nullptr) {
    if (coord.id != FR_BUF_JFA_COORD || color.id != FR_BUF_JFA_COLOR)
      throw Error(FR_E_INVALID, "SibsonInterpolation::render takes JumpFlooding's coordTex/colorTex");
    uint64_t ns = 0;
    check(fr_sibson_render(t_.ctx(), &ns), t_.ctx(), "SibsonInterpolation::render");
    detail::finish(ns, elapsed_time, done);
  }
  void resetShader() {}
  const Texture outputTex{FR_BUF_SIBSON};

 private:
  PathTracer& t_;
};

class PullPushInterpolation {
 public:
  explicit PullPushInterpolation(PathTracer& t) : t_(t) {}
  void render(Texture sparse, const unsigned* = nullptr, uint64_t* elapsed_time = nullptr, int* done = nullptr) {
    uint64_t ns = 0;
    check(fr_pullpush_render(t_.ctx(), sparse.id, &ns), t_.ctx(), "PullPushInterpolation::render");
    detail::finish(ns, elapsed_time, done);
  }
  void resetShader() {}
  const Texture outputTex{FR_BUF_PULLPUSH};

 private:
  PathTracer& t_;
};

class ATrous {
 public:
  explicit ATrous(PathTracer& t) : t_(t) {}
  // rtTex and frame are accepted and unused, as in atFS.glsl (FR/ATrous.cpp:47-132)
  void render(int count, Texture positionTex, Texture normalTex, Texture inColorTex, Texture /*rtTex*/ = Texture(),
              int /*frame*/ = 0, const unsigned* = nullptr, uint64_t* elapsed_time = nullptr, int* done = nullptr) {
    uint64_t ns = 0;
    check(fr_atrous_render(t_.ctx(), count, positionTex.id, normalTex.id, inColorTex.id, &ns), t_.ctx(),
          "ATrous::render");
    detail::finish(ns, elapsed_time, done);
  }
  const Texture colorTex{FR_BUF_ATROUS};

 private:
  PathTracer& t_;
};

// Multi-GPU group (fr_group_*): one object per process; ranks = the local tracers (in-process copies)
// or this process's tracer in an RCCL communicator.
class Group {
 public:
  Group(std::vector<PathTracer*> tracers, void* rccl_comm, const fr_group_config& cfg) {
    std::vector<fr_ctx*> c;
    for (PathTracer* t : tracers) c.push_back(t->ctx());
    check(fr_group_create(c.data(), (int)c.size(), rccl_comm, &cfg, &g_), nullptr, "fr_group_create");
    n_ = (int)c.size();
  }
  Group(const Group&) = delete;
  Group& operator=(const Group&) = delete;
  ~Group() { if (g_) fr_group_destroy(g_); }
  void frame() { check(fr_group_frame(g_, nullptr), nullptr, "fr_group_frame"); }
  std::vector<fr_frame_timing> frame_timed() {
    std::vector<fr_frame_timing> t((size_t)n_);
    check(fr_group_frame(g_, t.data()), nullptr, "fr_group_frame");
    return t;
  }
  void composite(void* device_out, size_t bytes) { check(fr_group_composite(g_, device_out, bytes), nullptr, "fr_group_composite"); }
  void synchronize() { check(fr_group_synchronize(g_), nullptr, "fr_group_synchronize"); }
  fr_group* handle() const { return g_; }

 private:
  fr_group* g_ = nullptr;
  int n_ = 0;
};

}  // namespace fovrt
