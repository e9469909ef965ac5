/* fovrt.h — C ABI of the MI355X-native foveated path-tracing + reconstruction engine.
 *
 * Drop-in boundary for the reference's hot path (ohseokkwon/Foveated-Rendering-using-Ray-Tracing).
 * Every entry point replaces one call of the reference's frame loop (FR/main.cpp:253-358); the
 * reference interface each one replaces is cited next to it ("FR/" = "Foveated Rendering using
 * Ray Tracing/"). Conventions:
 *   - every function returns FR_OK (0) or a negative fr_status; no exceptions cross the ABI;
 *   - fr_last_error(ctx) (or fr_last_error(NULL) after a failed fr_create) describes the failure;
 *   - the context owns all device memory (allocated in fr_create, freed in fr_destroy); per-frame
 *     calls never allocate; views returned by fr_get_buffer are borrowed and stay valid until the
 *     next call that writes that buffer, or fr_destroy;
 *   - one context per device, one host thread per context (calls are serialised, not re-entrant);
 *   - image buffers are row-major W x H with row 0 = bottom row (the OptiX launch index y and the
 *     GL texture t of the reference agree on this), RGBA32F unless the view says otherwise.
 */
#ifndef FOVRT_H
#define FOVRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: fr_config.abi_version; fr_set_gaze takes the cursor (cursorPosCallback) and fr_reset_gaze; the
 *    sparse shard calls take the slab size; fr_set_shard_plan / fr_shard_plan; the fr_group_* calls. */
#define FOVRT_ABI_VERSION 2

typedef enum fr_status {
  FR_OK = 0,
  FR_E_INVALID = -1,     /* bad argument / unknown buffer id */
  FR_E_HIP = -2,         /* HIP runtime error (no device, launch failure) */
  FR_E_NOMEM = -3,       /* device allocation failed */
  FR_E_IO = -4,          /* asset file missing or malformed */
  FR_E_STATE = -5,       /* call out of order (e.g. shading before sampling) */
  FR_E_UNSUPPORTED = -6  /* configuration outside what the engine implements */
} fr_status;

typedef enum fr_scene_preset {
  FR_SCENE_BOX = 0,      /* ground + refractive box               (configs[0]) */
  FR_SCENE_BUNNY = 1,    /* ground + box + bunny + reflective earth (configs[1], configs[2]) */
  FR_SCENE_VOKSELIA = 2  /* all five models of FR/PathTracer.cpp:582-595 */
} fr_scene_preset;

typedef enum fr_mask_mode {
  FR_MASK_SALIENCY = 0,   /* masked_sampling (FR/cuda/samplingStep.cu:222), the reference default */
  FR_MASK_LOGPOLAR = 1,   /* log-polar round trip (FR/cuda/samplingStep.cu:180-182) */
  FR_MASK_UNIFORM2X2 = 2, /* x%2==0 && y%2==0 (FR/PathTracer.cpp:526-533), non-foveated */
  FR_MASK_ALL = 3,        /* every pixel traced */
  FR_MASK_LOGPOLAR_SIGNED = 4,/* log-polar round trip with signed pixel differences: the 10% foveal
                               * density BASELINE.json quotes (the literal uint2 arithmetic of
                               * samplingStep.cu:182 wraps negative differences, halving it) */
  FR_MASK_ECCENTRIC = 5,      /* parametric eccentricity mask (fr_set_foveation): radius, floor, ray budget */
  FR_MASK_CALLER = 6          /* the caller's own mask (fr_set_sampling_mask) */
} fr_mask_mode;

typedef struct fr_config {
  int abi_version;            /* FOVRT_ABI_VERSION (fr_config_default sets it; fr_create rejects others) */
  int width, height;          /* FR/main.cpp:127-135 (argv W H), default 1024 x 1024 */
  int scene;                  /* fr_scene_preset */
  int mask_mode;              /* fr_mask_mode */
  int spp;                    /* 1, 2, 4 or 8 (reference: 1, FR/cuda/fov_path_trace_camera.cu:117) */
  int diffuse_max_depth;      /* g_diffuse_max_depth (FR/gui.cpp:26), default 1 */
  int refraction_max_depth;   /* min(refraction_maxdepth, max_depth) = 100 in the reference; default 16 */
  float light_power;          /* g_light_Power (FR/gui.cpp:21), default 810 */
  int optimize;               /* g_isOptimize (FR/gui.cpp:16): run the compaction (entry 2) */
  int atrous_iterations;      /* ATrous::render count (FR/main.cpp:355), default 1 */
  int write_extra;            /* write the saliency heat-map buffer (extra_buffer) */
  int device;                 /* HIP device ordinal */
  int texture_mode;           /* 0: reference assets from asset_dir (error if missing); 1: procedural */
  int detail;                 /* procedural mesh detail (0 = preset default) */
  int mesh_mode;              /* 0: the reference's .obj meshes where present under asset_dir, procedural
                               * stand-ins otherwise; 1: procedural only; 2: .obj required (FR_E_IO) */
  int bvh_builder;            /* 0: host binned SAH (default); 1: GPU LBVH (k_bvh.hip); 2: GPU binned SAH
                               * (k_bvh_sah.hip). The context's builder makes fr_create's tree and every later
                               * one (fr_rebuild_bvh, fr_set_positions, FR_BVH_REBUILD of fr_update_positions /
                               * fr_update_geometry / fr_set_model_transforms); a builder-0 context rebuilds with
                               * the LBVH. All three give identical frames.
                               *
                               * The tree of builder 2 is the tree of builder 0: one right answer, the rule
                               *   inputs    a triangle's box is the min / max of its vertices, its centroid
                               *             (lo + hi) * 0.5f;
                               *   leaves    a node of <= 2 triangles, or at depth >= 30 (the root: depth 0);
                               *   axis      over the node's centroid box, ext = hi - lo:
                               *             ext.x > ext.y ? (ext.x > ext.z ? 0 : 2) : (ext.y > ext.z ? 1 : 2);
                               *   bins      with ex = ext[axis] > 0, bin = (int)((key - lo) / ex * 16) clamped
                               *             to [0, 15]; a bin keeps its triangle count and the union of boxes;
                               *   split     for k = 1..15, l = union of bins < k, r = of bins >= k, skipped
                               *             when a side is empty; cost = l.area() * nl + r.area() * nr in fp32,
                               *             every operation rounded on its own (no fused multiply-add),
                               *             area = 2 * (dx*dy + dy*dz + dz*dx), 0 when dx < 0; the first k of
                               *             strictly smaller cost wins; left: the triangles of bins < k;
                               *   ex == 0   (all centroids equal) left: the n / 2 lowest primitive indices;
                               *   boxes     a child's box is the union of its triangles' boxes;
                               *   4-wide    the collapse, stack need, slot inflation and leaf layout of every
                               *             builder here.
                               * Equal: the hierarchy, every stored slot box bit for bit, every leaf's triangle
                               * set, the node count, bvh_depth, bvh_max_stack. Free: the index a node takes among
                               * the nodes of its level, and the order of the triangles inside one leaf. (Mins
                               * and maxes of +0 and -0 depend on the order; nothing stored does.)
                               * Not the host's: a node with ex > 0 none of whose candidates has a finite cost
                               * (coordinates around 1e19 and beyond) gets the median by (key, index) on the
                               * host; the device build fails with FR_E_UNSUPPORTED and leaves positions, tree
                               * and scene box as they were. The host's FOVRT_BVH_LEAF / _BINS / _SPLIT tuning
                               * variables do not reach the device: equality is with the host at its defaults.
                               * Scenes of fewer than 3 triangles behave as with builder 1. Scratch: 143 bytes
                               * per triangle, made by fr_create on builder-2 contexts only; a rebuild
                               * allocates nothing. */
  int sibson_mode;            /* 0 (default): run form, each row of a pixel's disc summed from per-row prefix
                               * sums (same taps as sibsonFS.glsl:30-44, rounding-level differences, ~1e-6);
                               * 1: per tap in the shader's order (bit-exact against the oracle) */
  const char* asset_dir;      /* directory holding CedarCity.hdr, grid.ppm, bunny/bunny.PPM, ... */
} fr_config;

/* Per-frame camera uniforms (PathTracer::update_optix_variables, FR/PathTracer.cpp:774-820).
 * Matrices are row-major "math" matrices: v' = M v. */
typedef struct fr_camera {
  float eye[3];
  float prev_eye[3];
  float inv_vp[16];   /* device "mvp"      = inverse(P * V)           (:786-787) */
  float prev_vp[16];  /* device "prev_mvp" = P * V of the previous frame (:789-790) */
  float up[3];
  float target[3];
  float gaze[2];      /* (g_gaze.x, H - g_gaze.y) */
} fr_camera;

/* glm-style camera pose (FR/Camera.cpp): position, unit quaternion (w, x, y, z), perspective. */
typedef struct fr_camera_pose {
  float pos[3];
  float rot[4];       /* glm::quat (w, x, y, z) */
  float fovy_deg;     /* 45 (FR/main.cpp:207) */
  float znear, zfar;  /* 0.1, 500.1 */
  float aspect;       /* viewport w / h */
} fr_camera_pose;

typedef enum fr_buffer_id {
  /* PathTracer::TextureName order (FR/PathTracer.h:13-31) */
  FR_BUF_POSITION = 0,
  FR_BUF_NORMAL = 1,
  FR_BUF_DEPTH = 2,
  FR_BUF_DIFFUSE = 3,
  FR_BUF_WEIGHT = 4,
  FR_BUF_THREAD = 5,        /* compacted active-pixel list (u32 pixel index, ray_count entries) */
  FR_BUF_HISTORY = 6,
  FR_BUF_SHADING = 7,
  FR_BUF_EXTRA = 8,
  /* reconstruction outputs (JumpFlooding / Sibson / PullPush / ATrous GL textures) */
  FR_BUF_JFA_COORD = 9,
  FR_BUF_JFA_COLOR = 10,
  FR_BUF_SIBSON = 11,
  FR_BUF_PULLPUSH = 12,
  FR_BUF_ATROUS = 13,
  /* temporal state (OptiX ping-pong partners) */
  FR_BUF_DEPTH_CACHE = 14,
  FR_BUF_HISTORY_CACHE = 15,
  FR_BUF_MASK = 16,         /* u8 usingRay per pixel */
  FR_BUF_LOGPOLAR = 17,     /* LogPolarTransform::logPolarTex  (forward image, W/4 x H/4 used) */
  FR_BUF_LOGPOLAR_INVERSE = 18, /* LogPolarTransform::ilogPolarTex */
  FR_BUF_GCLASS = 19,       /* u8 primary-hit class of the last G-buffer: 0 refraction, 1 reflection, 2 diffuse,
                             * 3 miss (the megakernel's class-major work order; diagnostics) */
  FR_BUF_COUNT = 20
} fr_buffer_id;

typedef enum fr_format { FR_FMT_RGBA32F = 0, FR_FMT_U32 = 1, FR_FMT_U8 = 2 } fr_format;

typedef struct fr_buffer_view {
  void* device_ptr;
  int width, height;   /* elements; THREAD: width = capacity, height = 1 */
  size_t pitch_bytes;  /* bytes per row */
  size_t bytes;        /* total bytes */
  int format;          /* fr_format */
} fr_buffer_view;

typedef struct fr_stats {
  uint64_t gbuffer_primary;   /* entry-0 camera rays */
  uint64_t primary;           /* entry-3 camera rays (ray_count * spp) */
  uint64_t shadow;            /* shadow rays (light samples) */
  uint64_t diffuse_bounce;    /* diffuse GI bounces */
  uint64_t mirror;            /* reflection-material mirror rays */
  uint64_t refraction;        /* refraction-material transmitted rays */
  uint64_t reflection;        /* refraction-material reflected rays */
  uint64_t truncated;         /* refraction nodes cut by refraction_max_depth */
  uint64_t overflow;          /* work items dropped (explicit stack full) */
  uint64_t segments;          /* sum of all traced ray segments */
  uint64_t diag[6];           /* diagnostic build (-DFR_STAMPS) only, else 0: megakernel cycle stamps
                                 [total, refill, shade, traversal], node visits, wave traversal steps */
} fr_stats;

typedef struct fr_frame_timing {
  /* stage names of PrintMSTimes (FR/main.cpp:260-358); milliseconds measured with HIP events */
  float geometry_ms, sampling_ms, optimize_ms, shading_ms;
  float jfa_ms, sibson_ms, pullpush_ms, atrous_ms;
  float total_ms;
  uint32_t ray_count;
  float shade_paths_ms; /* the path-trace megakernel alone (inside shading_ms) */
} fr_frame_timing;

typedef struct fr_ctx fr_ctx;

int fr_config_default(fr_config* cfg);
const char* fr_version(void);
int fr_abi_version(void);  /* FOVRT_ABI_VERSION of the library */

/* PathTracer::initialize(w, h) (FR/PathTracer.cpp:41-78) + the renderer constructors
 * (FR/main.cpp:152-159). */
int fr_create(const fr_config* cfg, fr_ctx** out);
int fr_destroy(fr_ctx* ctx);
const char* fr_last_error(fr_ctx* ctx);

/* Camera (FR/Camera.cpp): glm-compatible helpers. */
int fr_camera_look_at(fr_camera_pose* pose, const float target[3], const float up[3]);  /* :73-83 */
int fr_camera_matrices(const fr_camera_pose* pose, float view[16], float proj[16]);      /* :139-181, row-major */
int fr_camera_uniforms(const fr_camera_pose* cur, const fr_camera_pose* prev, int width, int height,
                       fr_camera* out);  /* update_optix_variables' host math, gaze = screen centre */
int fr_preset_camera(int scene, float eye[3], float target[3]);  /* FR/main.cpp:189-209 */

/* PathTracer::init_camera / update_optix_variables (FR/PathTracer.cpp:606-632, 774-820) */
int fr_set_camera(fr_ctx* ctx, const fr_camera* cam);
int fr_set_light_power(fr_ctx* ctx, float power);          /* g_light_changed path, :103-116 */
int fr_set_diffuse_max_depth(fr_ctx* ctx, int depth);      /* :800-806 */
int fr_reset_accumulation(fr_ctx* ctx);                    /* tracer->m_accumFrame = 0 (FR/main.cpp:248) */
int fr_accum_frame(fr_ctx* ctx, uint32_t* frame);          /* public m_accumFrame */

/* The four OptiX launches (FR/PathTracer.cpp:85-230). Synchronous; *ms = elapsed milliseconds. */
int fr_geometry_launch(fr_ctx* ctx, float* ms);   /* entry 0 g_buffer_trace */
int fr_sampling_launch(fr_ctx* ctx, float* ms);   /* entry 1 sampling_step */
int fr_optimize_launch(fr_ctx* ctx, float* ms);   /* entry 2 warp_sort x3 -> ray_count */
int fr_shading_launch(fr_ctx* ctx, float* ms);    /* entry 3 ray_trace + history/depth swaps */
int fr_ray_count(fr_ctx* ctx, uint32_t* count);   /* m_context["ray_count"] read-back (FR/main.cpp:288-299) */
int fr_gaze_target(fr_ctx* ctx, float xyz[3]);    /* m_context["gaze_target"] read-back (:278-287) */

/* GL reconstruction passes; *elapsed_ns like GL_TIME_ELAPSED (NULL allowed). */
int fr_jfa_render(fr_ctx* ctx, int in_buffer, uint64_t* elapsed_ns);            /* JumpFlooding::render */
int fr_sibson_render(fr_ctx* ctx, uint64_t* elapsed_ns);                        /* SibsonInterpolation::render */
int fr_pullpush_render(fr_ctx* ctx, int in_buffer, uint64_t* elapsed_ns);       /* PullPushInterpolation::render */
int fr_atrous_render(fr_ctx* ctx, int count, int pos_buffer, int nrm_buffer, int col_buffer,
                     uint64_t* elapsed_ns);                                     /* ATrous::render */

/* LogPolarTransform::render (FR/Log_Polar_Transform.cpp:40-106) of any RGBA32F buffer around the
 * current gaze: forward image -> FR_BUF_LOGPOLAR, round trip -> FR_BUF_LOGPOLAR_INVERSE. */
int fr_logpolar_render(fr_ctx* ctx, int in_buffer, uint64_t* elapsed_ns);
/* Final composite of nviews rendered views (e.g. the two eyes gathered to one GPU over RCCL):
 * device `views` = nviews consecutive W x H RGBA32F images -> device `out` = (nviews * W) x H,
 * view v in columns [v W, (v+1) W) (renderAll's side-by-side display, FR/main.cpp:26-113). */
int fr_composite_views(fr_ctx* ctx, const void* views, int nviews, void* out, size_t out_bytes);
/* Gaze input, the reference's GLFW callbacks. fr_set_gaze is cursorPosCallback (FR/gui.cpp:48-66): the
 * cursor (xpos, ypos) in window coordinates (y down) sets the Win32 POINT g_gaze = ((LONG)xpos,
 * (LONG)(ypos * adjust_scale)), adjust_scale = 1 in full screen (g_fullScreen) and 1.25 in a window
 * (:51-56); fr_reset_gaze is framebufferSizeCallback's g_gaze = (w / 2, h / 2) (:32-35). The kernels use
 * (g_gaze.x, H - g_gaze.y) (FR/PathTracer.cpp:795) from the next launch on; fr_set_camera's gaze
 * replaces it too. */
int fr_set_gaze(fr_ctx* ctx, double xpos, double ypos, int fullscreen);
int fr_reset_gaze(fr_ctx* ctx);

/* Foveation control: the sampling mask steered by the caller. Nothing here changes a context that does not use it: a
 * context in modes 0..4 that never makes these calls launches what it always launched.
 * fr_set_mask_mode replaces the mode fr_create took from fr_config.mask_mode (fr_create itself keeps accepting the
 * five reference modes 0..4 only: modes 5 and 6 are entered through this call). It is host state, as fr_set_gaze is:
 * it waits for nothing and takes effect at the next sampling launch (fr_sampling_launch, fr_frame, fr_trace_frame);
 * the cached mask of the log-polar and eccentricity modes is invalidated. Every mode 0..6 is accepted, anything else
 * is FR_E_INVALID. fr_get_mask_mode returns the mode in place. A snapshot carries the mode, as it always has; it carries
 * neither the parameters below, nor the controller's radius, nor a caller's mask: after fr_restore the context keeps
 * the ones it has.
 *
 * FR_MASK_ECCENTRIC: a pure function of the pixel, the gaze the kernels use (fr_set_gaze, fr_set_camera) and two
 * parameters, with one right answer in bytes. fp32, every operation rounded on its own, no fma; for pixel (x, y):
 *   xb = x & 7, yb = y & 7, a = xb ^ yb
 *   rank = sum over i = 0..2 of (2 * bit_i(a) + bit_i(yb)) << (2 * (2 - i))
 *          (an 8 x 8 ordered-dither permutation of 0..63; row y = 0: 0 32 8 40 2 34 10 42, row y = 1: 48 16 56 24 50 18 58 26)
 *   dx = (float)x - gaze.x;  dy = (float)y - gaze.y;  d2 = dx*dx + dy*dy              (two products, one sum)
 *   sampled  <=>  rank < floor_ranks  ||  (float)rank * d2 < 64.0f * r2
 * Inside the radius (d2 < r2) every pixel is sampled; outside it the density falls as r2 / d2 and the dither says
 * which pixels go. rank(0, 0) = 0, so the reference's 8 x 8 peripheral grid is always present; floor_ranks (1..64)
 * raises that floor to floor_ranks / 64. The ownership fold of a sharded context applies as in every other mode.
 * fr_foveation_default: radius_px = 0.07f * sqrtf((float)W*(float)W + (float)H*(float)H) (the reference's r0 of the
 * diagonal), floor_ranks = 1, ray_budget = 0, tolerance = 0.02f; a context starts from it. r2 = radius_px * radius_px,
 * one fp32 product on the host. fr_set_foveation is host state like fr_set_mask_mode; the mask is generated again
 * only when gaze, parameters or mode changed. FR_E_INVALID, with the parameters in place kept: a NULL argument, a
 * radius that is not finite or is <= 0, floor_ranks outside 1..64, a tolerance not in [0, 1), ray_budget > W * H.
 * fr_foveation_mask states the rule on the host, without a device, through the function the kernel runs: mask (W * H
 * bytes of 0 / 1, row y at y * W; may be NULL) and *count (the number sampled; may be NULL). A caller sizes a radius
 * for a wanted count with it. FR_E_INVALID: a size outside 1..32767, a NULL or non-finite gaze, an r2 that is not
 * finite or is < 0, floor_ranks outside 1..64.
 *
 * The ray budget (ray_budget = T > 0, mode 5 only): the radius follows the compaction's count on the device, in
 * stream order, with no host wait. r2_0 = radius_px * radius_px is what the first sampling launch after
 * fr_set_foveation uses. With n_k the ray count of the compaction that followed sampling launch k, launch k + 1 uses
 *   nf = (float)max(n_k, 1);  tf = (float)T
 *   |nf - tf| <= tolerance * tf            ->  r2_{k+1} = r2_k                                   (held)
 *   otherwise  ratio = min(max(tf / nf, 0.5f), 2.0f);
 *              r2_{k+1} = min(max(r2_k * ratio, 1.0f), (float)W*(float)W + (float)H*(float)H)   (adjusted)
 *   no compaction since launch k           ->  r2_{k+1} = r2_k
 * again fp32 with every operation rounded on its own. One lane decides, on the stream of the front stages ahead of
 * the mask generation, so stage calls and fr_frame in both pipeline modes walk the same trajectory; while a budget is
 * set the mask is generated at every sampling launch (the host does not know r2). The deadband keeps the mask still
 * once the count is on target: ring edges that moved every frame would discard history there. The count is concave
 * and increasing in r2 with a positive intercept (the floor grid), so r2 <- r2 * T / count(r2) approaches its fixed
 * point from one side. fr_foveation_status waits for the context's pending work, as fr_geometry_update_status does,
 * and returns the r2 the last mode-5 sampling launch used (r2_0 before the first), the count the controller read last
 * (0: none yet) and the launches that adjusted and that held since fr_set_foveation; any pointer may be NULL.
 * FR_E_UNSUPPORTED, parameters kept: ray_budget > 0 on a rank of a group or a sharded context (ranks with tile-local
 * fronts count different pixels and would diverge), and on a context created with fr_config.optimize = 0. A context
 * that becomes a rank or sharded with a budget in place has its next mode-5 sampling launch or frame refused the same
 * way, with nothing enqueued.
 *
 * FR_MASK_CALLER: the caller's mask, W * H bytes, a pixel sampled when its byte is not 0. The context keeps a 0 / 1
 * copy, made by the first fr_sampling_mask_enable(ctx, 1), which waits for the context's pending work and allocates
 * W * H bytes (FR_E_NOMEM: nothing is kept and the feature stays off); on = 0 makes the set calls return FR_E_STATE
 * until the next on = 1 and frees nothing. No other call of the feature allocates.
 * fr_set_sampling_mask takes the bytes from host (FR_MEM_HOST) or device memory (FR_MEM_DEVICE) and waits for the
 * context's pending work and for its own copy. fr_set_sampling_mask_enqueue takes device memory and copies in stream
 * order, behind the context's pending work and ahead of the next sampling launch: no host wait, no copy to the host,
 * no allocation. ready_event is as in fr_update_geometry_enqueue; the array must stay untouched until
 * fr_sampling_mask_consumed(ctx, stream) has made `stream` (a hipStream_t; 0 = the null stream) wait, on the device,
 * for the last enqueued copy's reads, as fr_geometry_consumed does for an update's. Device pointers are 16-byte
 * aligned. Every sampling launch in mode 6 uses the copy in place at its point of the stream order.
 * Equality: a frame whose mask came through either call equals, bit for bit, the stage calls with the same 0 / 1 mask
 * written by fr_write_buffer(FR_BUF_MASK) between fr_sampling_launch and fr_optimize_launch: MASK, WEIGHT, the count,
 * the active list, SHADING, the history and every reconstruction output.
 * Refused with nothing written: a NULL context or mask, bytes != W * H, a bad where, a misaligned device pointer
 * (FR_E_INVALID); the feature not enabled (FR_E_STATE); a sampling launch or frame in mode 6 before any mask was
 * submitted (FR_E_STATE, nothing of the frame enqueued); the enqueued form on a rank of a group or a sharded context
 * (FR_E_UNSUPPORTED: the synchronous form works there, and the caller gives every rank of a view the same mask, as
 * with cameras).
 * Not covered: a saliency-weighted eccentricity mask, a budget in milliseconds, the budget on groups and sharded
 * contexts, elliptical or per-eye foveae, parameters and masks inside a snapshot. */
typedef struct fr_foveation {
  float radius_px;      /* the foveal radius in pixels, > 0 */
  int floor_ranks;      /* 1..64: the peripheral floor density is floor_ranks / 64 */
  uint32_t ray_budget;  /* 0: none; T > 0: the device steers the radius toward T traced pixels */
  float tolerance;      /* the controller's deadband as a fraction of T, in [0, 1) */
} fr_foveation;
int fr_foveation_default(int width, int height, fr_foveation* f);
int fr_set_foveation(fr_ctx* ctx, const fr_foveation* f);
int fr_get_foveation(fr_ctx* ctx, fr_foveation* f);
int fr_foveation_mask(int width, int height, const float gaze[2], float r2, int floor_ranks, uint8_t* mask, uint32_t* count);
int fr_foveation_status(fr_ctx* ctx, float* r2, uint32_t* last_count, uint64_t* adjusted, uint64_t* held);
int fr_set_mask_mode(fr_ctx* ctx, int mode);
int fr_get_mask_mode(fr_ctx* ctx, int* mode);  /* (fr_mask_mode is the enum's name) */
int fr_sampling_mask_enable(fr_ctx* ctx, int on);
int fr_set_sampling_mask(fr_ctx* ctx, const void* mask, size_t bytes, int where);   /* FR_MEM_HOST | FR_MEM_DEVICE */
int fr_set_sampling_mask_enqueue(fr_ctx* ctx, const void* mask, size_t bytes, void* ready_event);
int fr_sampling_mask_consumed(fr_ctx* ctx, void* stream);

/* The whole main.cpp loop body (update -> 0 -> 1 -> 2 -> 3 -> JFA -> SI -> PPI -> AT). With timing == NULL
 * nothing is synchronised and consecutive frames pipeline: frame N's reconstruction (JFA -> Sibson and
 * pull-push -> A-Trous, on two internal streams) runs while frame N+1's trace half runs on the context
 * stream; POSITION / NORMAL / SHADING alternate between two buffers by frame parity for this. Every
 * other call (stage launches, buffer access, fr_synchronize) first orders itself after the pending
 * reconstruction, so results are those of the sequential loop. With timing != NULL the frame is
 * synchronised and per-stage HIP-event times are returned. */
int fr_frame(fr_ctx* ctx, fr_frame_timing* timing);
/* How untimed fr_frame calls overlap (the reference's loop is serial, FR/main.cpp:253-373, so its
 * gaze-to-image latency is its frame time):
 *   FR_PIPELINE_THROUGHPUT (default): the host enqueues frames back to back; frame N+1's front stages
 *     (entries 0-2) run beside frame N's path trace and frame N's reconstruction beside frame N+1's trace
 *     half, up to the context's frame slots in flight (highest frames per second, latency ~2-3 frames);
 *   FR_PIPELINE_LATENCY: one trace half in flight: fr_frame first waits (on the host) for the previous
 *     frame's path trace to finish, so the gaze the caller set just before the call is sampled when the
 *     GPU can start the frame; the previous frame's reconstruction overlaps this frame's front stages
 *     (G-buffer, sampling, compaction) and ends before its path trace starts (latency ~ 1.2 serial
 *     frames, throughput above the serial loop's).
 * Results are identical in both modes. */
#define FR_PIPELINE_THROUGHPUT 0
#define FR_PIPELINE_LATENCY 1
int fr_set_pipeline_mode(fr_ctx* ctx, int mode);
/* Which reconstruction chains fr_frame / fr_reconstruct_frame run on this context: bit 0 JumpFlooding ->
 * Sibson, bit 1 pull-push -> A-Trous (default 3, both; a group's split reconstruction sets 1 and 2 on
 * the two reconstruction ranks of a view). */
int fr_set_recon_chains(fr_ctx* ctx, int chains);
/* How entry 3 sums a camera sample's radiance: 0 fp32 in the oracle's depth-first order,
 * 1 (default) by frame size (fixed point below 64 pixel-samples per megakernel lane, fp32 above), 2 32.32
 * fixed point with the tail handoff (idle lanes take pending refraction items of busy ones; the value does
 * not depend on which lane traces an item). The forms differ by rounding only (<= 1e-4). Synchronises. */
int fr_set_sample_sum(fr_ctx* ctx, int mode);
int fr_trace_frame(fr_ctx* ctx, fr_frame_timing* timing);        /* update -> entries 0..3 only */
int fr_reconstruct_frame(fr_ctx* ctx, fr_frame_timing* timing);  /* JFA -> SI -> PPI -> AT only */
int fr_synchronize(fr_ctx* ctx);

/* Tile sharding of one view across ranks (BASELINE configs[3]): screen tiles of
 * tile x tile pixels, tile t = ty * ceil(W / tile) + tx traced by rank t % count (round robin, so
 * the dense foveal tiles spread over all ranks). Every rank computes the full G-buffer and sampling
 * mask and traces only its own tiles' active pixels; the compositing rank unpacks the other ranks'
 * tiles of SHADING and runs the reconstruction half. Exact for a static camera (history is
 * per-tile); with a moving camera also exchange HISTORY_CACHE the same way. count = 1 restores the
 * whole screen. Slabs are device buffers of fr_shard_texels() RGBA32F texels (T*T per owned tile,
 * owned tiles in increasing order); pack/unpack synchronise the context stream. (fr_group_* below
 * runs all of this, RCCL included, behind one call per frame.) */
int fr_set_shard(fr_ctx* ctx, int rank, int count, int tile);
/* Explicit tile owners: owner[t] (< count) traces tile t (ntiles = ceil(W/tile) * ceil(H/tile)). */
int fr_set_shard_plan(fr_ctx* ctx, int rank, int count, int tile, const uint8_t* owner, size_t ntiles);
/* Host only (no device): deals the ntiles tiles of a W x H screen over count ranks in proportion to
 * weights[0..count-1] (>= 0, not all 0) by smooth weighted round robin in raster order, so every rank
 * gets its share of the dense foveal tiles. weights NULL = equal. Writes owner[0..ntiles-1]. */
int fr_shard_plan(int width, int height, int tile, int count, const float* weights, uint8_t* owner, size_t ntiles);
/* Active pixels of every rank of the view in the last front stages (sampling + compaction), counted
 * on this rank from its own full mask: the pixels rank r traces and sends. Synchronises the front. */
int fr_shard_counts(fr_ctx* ctx, uint32_t* counts, int n);
/* Tile-local front stages for a tracing rank of a static camera (on = 1; needs count > 1 in the shard
 * plan): the G-buffer runs only on this rank's tiles plus the 4-pixel halo the saliency stencil reads
 * (and on the gaze pixel's 8x8 tile), and the sampling mask, compaction and the history carry only on
 * this rank's tiles. Its traced pixels are unchanged; every other pixel of its buffers is unspecified,
 * and fr_shard_counts reports 0 for the other ranks. The reprojection reads the previous frame at the
 * same pixel only while the camera is still, so a moving camera needs on = 0 (the default). A new shard
 * plan keeps the setting (and recomputes the tiles); a whole-screen plan turns it off. */
int fr_set_front_local(fr_ctx* ctx, int on);
/* The same with the tiles dealt over ranks first_tracer .. count-1 only (tile t to rank
 * first_tracer + t % (count - first_tracer)); ranks below first_tracer trace nothing. first_tracer = 1
 * leaves the view's compositing rank 0 to the G-buffer and the reconstruction half, which no other
 * rank can share (JFA's reach, the global pull-push pyramid). fr_set_shard = first_tracer 0. */
int fr_set_shard_ex(fr_ctx* ctx, int rank, int count, int tile, int first_tracer);
/* Sparse SHADING gather (SURVEY §8(e) "sparse variant"): a tracing rank packs only the pixels its last
 * trace half shaded, as capacity x 16 B of (tone-mapped radiance, 1) texels followed by capacity x 4 B of
 * pixel indices (slab_bytes >= 20 x capacity, else FR_E_INVALID); *count returns their number
 * (FR_E_INVALID when it exceeds capacity: size capacity from fr_ray_count). A receiving rank, after its own
 * trace half (which carries every other pixel's history), adds each entry's reprojected history from its
 * own history, as the shading resolve does, and scatters the sums into HISTORY_CACHE and SHADING (indices
 * outside the screen are skipped; the sender's own history is not used: a tile-edge pixel's reprojection
 * can round into another rank's tiles). ~10x less than the tile slabs at a 10 % mask. Exact for a
 * static camera when the compositing rank receives; with a moving camera when every rank receives
 * every other rank's pixels each frame (its reprojection then reads a complete history). Both
 * synchronise the context stream. */
int fr_shard_pack_active(fr_ctx* ctx, void* device_slab, size_t slab_bytes, uint32_t capacity, uint32_t* count);
int fr_shard_unpack_active(fr_ctx* ctx, const void* device_slab, size_t slab_bytes, uint32_t capacity,
                           uint32_t count);
/* fr_shard_unpack_active without the synchronisation: enqueued on the context stream after the work
 * already there (the slab must stay valid until that work has run, e.g. until fr_synchronize). */
int fr_shard_unpack_active_enqueue(fr_ctx* ctx, const void* device_slab, size_t slab_bytes, uint32_t capacity,
                                   uint32_t count);
int fr_shard_texels(fr_ctx* ctx, size_t* texels);
int fr_shard_pack(fr_ctx* ctx, int buffer_id, void* device_slab, size_t bytes);
int fr_shard_unpack(fr_ctx* ctx, int buffer_id, int src_rank, const void* device_slab, size_t bytes);

/* ---- Multi-GPU groups (SURVEY §8(b) Threading, §8(e)) --------------------------------------------
 * The reference is single-GPU; this is how frames shard over the GPUs of a node. A group is R ranks
 * (one fr_ctx each, all created with the same fr_config apart from .device) rendering V views (eyes) of
 * G = R / V ranks: rank r renders view r / G as view rank r % G (view v's camera is set on its ranks'
 * contexts with fr_set_camera as usual). In a view the screen tiles are dealt over the ranks by weight
 * (fr_shard_plan). Every rank runs the front stages (G-buffer, sampling mask, compaction) and traces its
 * own tiles' active pixels; each traced pixel (20 B: radiance texel + pixel index) goes to the view's
 * reconstruction ranks, which run JumpFlooding -> Sibson (view rank 0) and pull-push -> A-Trous (view
 * rank 1 with split_recon, else rank 0 as well); the composite is bit-identical to the one-GPU frame.
 * That gather is the path's only exchange (JFA's reach and the pull-push pyramid are global); it uses
 * RCCL ncclSend/ncclRecv over xGMI, sized on every rank from its own full mask (fr_shard_counts), so
 * there is no control collective and no host synchronisation beyond each rank's own front stages. With
 * moving_camera every rank receives every other rank's pixels instead (reprojection reads across
 * tiles). The optional composite gathers each view's A-Trous image to rank 0 (the stereo pair of
 * BASELINE configs[4], side by side, renderAll FR/main.cpp:26-113).
 * Ranks live either in one process (ctxs[0..n-1], any devices, rccl_comm NULL: device-to-device
 * copies; n = R) or one per process (n = 1, rccl_comm = an ncclComm_t of R ranks whose rank is this
 * context's: fr_rccl_comm_init, or the caller's own). */
#define FR_GROUP_MAX_VIEW_RANKS 16
typedef struct fr_group fr_group;
typedef struct fr_group_config {
  int views;               /* V >= 1, divides R */
  int tile;                /* screen tile edge, a multiple of 16 (default 128) */
  int split_recon;         /* 1 (default): the two reconstruction chains on view ranks 0 and 1 when G >= 2 */
  int moving_camera;       /* 1: every rank receives every other rank's traced pixels (default 0) */
  int composite;           /* 1: every frame, the views' A-Trous images side by side on rank 0 */
  float recon_cost[2];     /* the reconstruction work of view ranks 0 and 1 as a fraction of one frame's
                              trace work (default 0.5, 0.17: JFA + Sibson, pull-push + A-Trous at 4K);
                              the tiles are dealt so that every rank's total is level (water filling) */
  float weights[FR_GROUP_MAX_VIEW_RANKS];  /* explicit tracing weights per view rank; all 0 = from recon_cost */
  int sample_sum;          /* fr_set_sample_sum on every rank when G >= 2 (default 2: fixed point with the tail
                              handoff, which shortens a tracer's small launch; the view then equals a one-GPU
                              frame in that form); -1 leaves the contexts as they are */
  int front_local;         /* 1 (default): with a still camera, ranks that only trace run their front stages
                              on their own tiles plus halo (fr_set_front_local); ignored with moving_camera */
  int jfa_ranks;           /* view ranks that take JumpFlooding -> Sibson in turns, one frame each: view rank 0,
                              then 2, 3, ... (they all receive every traced pixel; the chain keeps no state
                              across frames). 0 (default) = auto: 2 when G >= 6 with split_recon, else 1 */
} fr_group_config;
int fr_group_config_default(fr_group_config* cfg);
/* RCCL bootstrap for callers without their own: rank 0 creates the 128-byte unique id, every rank
 * passes it (sent by any means) to fr_rccl_comm_init on its own device. */
int fr_rccl_unique_id(void* id128);
int fr_rccl_comm_init(const void* id128, int nranks, int rank, int device, void** comm);
int fr_rccl_comm_destroy(void* comm);
int fr_group_create(fr_ctx* const* ctxs, int n, void* rccl_comm, const fr_group_config* cfg, fr_group** out);
/* One frame of every local rank (update -> 0 -> 1 -> 2 -> 3, exchange, JFA -> SI and PPI -> AT on the
 * reconstruction ranks, the composite). timing == NULL: nothing is synchronised beyond the front stages'
 * counts, and consecutive frames pipeline. timing != NULL (n timings, one per local rank): the frame is
 * synchronised and each rank's stage times are returned (reconstruction stages 0 on other ranks). */
int fr_group_frame(fr_group* g, fr_frame_timing* timing);
/* Final composite (the group must have composite = 1): copies the last frame's (V * W) x H RGBA32F image
 * from rank 0 to device memory `out` of rank 0's device (bytes >= V * W * H * 16); synchronises. */
int fr_group_composite(fr_group* g, void* out, size_t bytes);
/* Roles of local rank i: *view, *view_rank, *chains (bit 0 JFA -> Sibson, bit 1 pull-push -> A-Trous
 * run here) and *tiles, the number of screen tiles it traces. */
int fr_group_rank_info(fr_group* g, int i, int* view, int* view_rank, int* chains, int* tiles);
/* Host only (no device): the tile plan fr_group_create would deal for one view of ranks_per_view ranks
 * (cfg NULL = fr_group_config_default): owner[t] = the view rank tracing tile t. */
int fr_group_plan(int width, int height, int ranks_per_view, const fr_group_config* cfg, uint8_t* owner, size_t ntiles);
/* Where the last frame's outputs of a view are: the global rank holding its JFA / Sibson images (the
 * rank whose turn it was, see jfa_ranks) and the one holding its pull-push / A-Trous images. */
int fr_group_output_ranks(fr_group* g, int view, int* jfa_rank, int* atrous_rank);
/* The tile plan of the views: owner[t] = the view rank that traces tile t (ntiles = ceil(W/tile) *
 * ceil(H/tile); all 0 when G = 1). */
int fr_group_tile_owners(fr_group* g, uint8_t* owner, size_t ntiles);
int fr_group_synchronize(fr_group* g);
int fr_group_destroy(fr_group* g);  /* the contexts trace the whole screen again */
const char* fr_group_last_error(void);  /* the failure of the calling thread's last fr_group_* / fr_rccl_* call */


/* GPU BVH builder (the reference's OptiX acceleration rebuild,
 * FR/PathTracer.cpp:590-602 rtAccelerationCreate(ctx, "Trbvh")). fr_rebuild_bvh re-indexes the
 * current triangles on the device (LBVH: Morton sort + Karras hierarchy, collapsed into the
 * engine's four-wide nodes); *ms = its wall time. fr_set_positions replaces the world-space
 * vertex positions (host array, 9 floats per triangle, the scene's triangle order) and rebuilds;
 * shading normals, texture coordinates and materials are kept. */
int fr_rebuild_bvh(fr_ctx* ctx, float* ms);
int fr_set_positions(fr_ctx* ctx, const float* xyz, size_t ntris);
/* fr_rebuild_bvh without host synchronisation: the tree is rebuilt over the current positions with the context's
 * builder (the LBVH on bvh_builder 0 and 1 contexts, the binned SAH on bvh_builder 2 ones), enqueued behind the
 * context's pending work; the call returns without waiting for the GPU. It synchronises no stream and no event,
 * copies nothing to the host that it waits for and allocates nothing; the builder runs a fixed schedule of
 * launches (every level its depth bound allows; those past the last find nothing to do). The update calls have no
 * rebuild form in stream order: a caller composes fr_update_geometry_enqueue or fr_set_model_transforms_enqueue
 * (which refit) with this call when it wants a new tree.
 * Equality: after a successful enqueued rebuild the tree, fr_scene_export's bvh_nodes / bvh_depth / bvh_max_stack,
 * fr_bvh_sah_cost and every later frame are what fr_rebuild_bvh called at the same point of the stream order
 * leaves (the tree is free only where bvh_builder says it is: node numbering within a level, order inside a leaf;
 * on a bvh_builder 2 context it is the host builder's tree over those positions). Positions, normals, scene box and
 * motion-reprojection state are untouched: like fr_rebuild_bvh the call is no position update.
 * Where it runs: on the context stream, or with fr_set_geometry_overlap on, on the stream of the front stages,
 * beside the previous frame's path trace. In both modes the build goes into the spare tree arrays, which become the
 * scene's when the call returns (overlapped: with the second array of shading records, brought up to date); frames
 * already enqueued keep the arrays they were given. Calls after it do not wait either: a later enqueued update or
 * pose refits the new tree, a later fr_frame(..., NULL) traces it, a later fr_rebuild_bvh_enqueue replaces it, none
 * of them with host knowledge of its node count.
 * Failure on the device: a bvh_builder 2 node with no finite SAH candidate (coordinates around 1e19), a tree whose
 * stack need exceeds FR_BVH_STACK, or a collapse that did not finish in the launches provided. The scene then
 * keeps the tree it had, bit for bit (a last kernel, gated on the verdict, copies the tree in use over the partly
 * written arrays, whole): the tree's numbers and every later frame are as if the call had not been made. Counters
 * on the device record each verdict: fr_bvh_rebuild_status waits for the context's pending work, as
 * fr_geometry_update_status does, and returns how many enqueued rebuilds built a tree and how many failed since
 * fr_create (either pointer may be NULL); when the failed count grew since its last call, fr_last_error says why.
 * Refused at once, nothing enqueued, scene untouched: a NULL context (FR_E_INVALID); a rank of a group or a
 * sharded context (FR_E_UNSUPPORTED); a scene of fewer than 3 triangles (fr_rebuild_bvh's answer); a context whose
 * tree in use is not yet a device-built one with a spare set beside it (FR_E_STATE: a bvh_builder 0 context
 * before its first fr_rebuild_bvh or FR_BVH_REBUILD update, which make the arrays; this call never allocates).
 * Every other call behaves as before and orders itself behind a pending rebuild; the synchronous ones
 * (fr_refit_bvh, fr_bvh_sah_cost, fr_scene_export, fr_snapshot, the synchronous updates) wait as they already do
 * and then learn the tree's numbers from the device. A context that never makes the call differs in nothing.
 * Not covered: groups and sharded contexts. */
int fr_rebuild_bvh_enqueue(fr_ctx* ctx);
int fr_bvh_rebuild_status(fr_ctx* ctx, uint64_t* built, uint64_t* failed);
/* fr_rebuild_bvh_enqueue when the device finds that the tree in use has grown: the stream, the fences, the swap of
 * the tree arrays, the refusals and the guarantees of that call (no wait, no copy to the host that anything waits
 * for, no allocation), and the decision is made on the device. Behind the context's pending work the SAH cost of the
 * tree in use is evaluated (fr_bvh_sah_cost's formula over the stored boxes; held to that call to 1e-4 relative, not
 * bit for bit: the sum may run over another length) and one lane decides:
 *   - the tree has no node, or its root area is not > 0, or the cost is not finite: skip, the baseline is untouched;
 *   - the baseline is stale (the tree in use came from fr_create, fr_rebuild_bvh, an FR_BVH_REBUILD update,
 *     fr_set_positions or the unconditional fr_rebuild_bvh_enqueue, or no baseline was ever adopted): the cost
 *     becomes the baseline, skip. The first evaluation of a tree adopts it;
 *   - cost > ratio * baseline (an fp32 product, strictly greater): build;
 *   - otherwise: skip.
 * A build is fr_rebuild_bvh_enqueue's, unchanged; after one that succeeded the new tree's cost is evaluated in stream
 * order and becomes the baseline. After one that failed on the device tree and baseline are as before and
 * fr_bvh_rebuild_status counts it as failed. A skipped build runs the same schedule of launches over an empty first
 * level (an LBVH context still sorts its codes) and ends as a failed one does, with the tree in use copied whole into
 * the arrays that become the scene's: tree, numbers and every later frame are as if the call had not been made. It
 * is counted as skipped, not as failed.
 * Refused at once, nothing enqueued: everything fr_rebuild_bvh_enqueue refuses, with the same codes; a ratio that is
 * not finite or is below 1 (FR_E_INVALID).
 * fr_set_rebuild_policy makes the context pose the question itself: with period > 0 it counts the updates and poses
 * that fr_update_geometry_enqueue and fr_set_model_transforms_enqueue accept on the host (whatever the device's later
 * verdict on them), from the call that set the policy, and after every period-th of them makes
 * fr_rebuild_bvh_enqueue_if(ctx, ratio) inside the same call: the context is equal to one whose caller makes those
 * calls by hand. Should that implicit call be refused (the context's state changed since), the update stays enqueued
 * and the update call returns the refusal. period 0 turns the policy off (the default; ratio is ignored then);
 * period < 0 is FR_E_INVALID, and with period > 0 the call is refused wherever fr_rebuild_bvh_enqueue_if would be.
 * fr_bvh_rebuild_policy_status waits as fr_bvh_rebuild_status does, for the same record: evaluated = conditional
 * calls since fr_create (built + failed + skipped of those alone), skipped, the cost evaluated last (after a build,
 * the new tree's) and the baseline. Any pointer may be NULL. fr_bvh_rebuild_status keeps counting every enqueued
 * build that built or failed, conditional or not. */
int fr_rebuild_bvh_enqueue_if(fr_ctx* ctx, float ratio);
int fr_set_rebuild_policy(fr_ctx* ctx, float ratio, int period);
int fr_bvh_rebuild_policy_status(fr_ctx* ctx, uint64_t* evaluated, uint64_t* skipped, float* last_cost,
                                 float* base_cost);
/* Moving geometry without giving up the tree. fr_refit_bvh keeps the topology of the tree in use (whichever
 * builder made it: the host SAH tree too) and recomputes every slot box bottom-up and every leaf triangle
 * from the current positions, in place; node count, depth and stack need do not change; *ms = its wall time.
 * fr_update_positions replaces the positions from host (FR_MEM_HOST) or device memory (FR_MEM_DEVICE: a
 * pointer the context's device can read, 9 floats per triangle) and then rebuilds (FR_BVH_REBUILD, the LBVH
 * of fr_rebuild_bvh) or refits (FR_BVH_REFIT). fr_set_positions is the HOST / REBUILD case. Every check
 * (triangle count, where, how, finite positions: FR_E_INVALID) runs before anything is written, device
 * positions are checked on the device, and a rebuild that fails (FR_E_UNSUPPORTED) leaves positions, tree and
 * scene box as they were. Device positions are not copied back: fr_scene_export fetches them when asked.
 * fr_bvh_sah_cost reports the quality of the tree in use, lower is better:
 *   1 + (sum over non-empty slots of area(slot box) * (1 for an inner slot | triangles of a leaf slot))
 *       / area(union of the root's slot boxes)
 * so a caller can compare a refitted tree with the same tree when it was built and rebuild when it has grown.
 * These calls wait for the context's pending work and for their own kernels (fr_update_geometry_enqueue below
 * is the update without host synchronisation). Not covered: groups (each rank's context is updated by its
 * caller). Shading normals are kept by these calls; fr_update_geometry below moves them with the positions. */
#define FR_BVH_REBUILD 0
#define FR_BVH_REFIT   1
#define FR_MEM_HOST    0
#define FR_MEM_DEVICE  1
int fr_refit_bvh(fr_ctx* ctx, float* ms);
int fr_update_positions(fr_ctx* ctx, const void* xyz, size_t ntris, int where, int how);
int fr_bvh_sah_cost(fr_ctx* ctx, float* cost);
/* Shading normals that follow the geometry. The scene is a triangle soup (corner c = 3 t + k of triangle t), so
 * its smooth vertices are derived once, from the scene as fr_create / fr_scene_create built it: two corners of
 * triangles that have normals (flags & 0x100) are one vertex when their rest positions and rest normals are
 * equal (all six floats by bits after adding +0.0f, so -0 equals +0). Vertices are numbered in order of their
 * first corner; corners of triangles without normals have vertex -1; a crease (equal positions, different
 * normals: a cube's faces) stays apart. The weld is fixed for the life of the scene: fr_normal_groups /
 * fr_scene_normal_groups copy it out (corner_vertex: 3 per triangle, or NULL; *nverts: the vertex count).
 * A recomputed normal has one right answer in bytes. fp32, unfused, no atomics, for a vertex v:
 *   acc = (0, 0, 0); over the corners c of v in ascending order: acc += cross(p1 - p0, p2 - p0) of triangle c / 3
 *   d = dot(acc, acc); if FLT_MIN <= d < inf every corner of v takes acc * (1.0f / sqrtf(d));
 *   otherwise each corner of v takes its own triangle's cross, normalised the same way when its dot is in that
 *   range; otherwise the corner keeps the normal it has.
 * fr_update_geometry is fr_update_positions (which is its FR_NORMALS_KEEP case) plus the normals: every check on
 * both arrays first, then positions, then the tree, then normals. FR_E_INVALID as for fr_update_positions, and
 * for a bad `normals` value, FR_NORMALS_GIVEN with nrm NULL and a given normal that is not finite on a triangle
 * that has normals (device arrays are checked on the device); a rejected update or a failed rebuild leaves
 * positions, tree, scene box and normals as they were. Given normals of triangles without normals are ignored:
 * neither checked nor written. Texture coordinates, flags and materials never change. fr_set_normals writes
 * given normals alone (positions and tree untouched); fr_recompute_normals applies the rule to the current
 * positions, *ms = its wall time. All of them wait for the context's pending work and for their own kernels,
 * and allocate nothing. fr_scene_export returns the current normals (fetched from the device when asked). */
#define FR_NORMALS_KEEP      0   /* fr_update_positions' behaviour */
#define FR_NORMALS_GIVEN     1   /* nrm: 9 floats per triangle, scene order, same memory kind as xyz */
#define FR_NORMALS_RECOMPUTE 2   /* the rule above, from the new positions */
int fr_update_geometry(fr_ctx* ctx, const void* xyz, const void* nrm, size_t ntris, int where, int how, int normals);
int fr_set_normals(fr_ctx* ctx, const void* nrm, size_t ntris, int where);
int fr_recompute_normals(fr_ctx* ctx, float* ms);
int fr_normal_groups(fr_ctx* ctx, int32_t* corner_vertex, size_t ncorners, int* nverts);
/* fr_update_geometry (device memory, refit) without host synchronisation: a caller who deforms the mesh before
 * every frame keeps the frame pipeline full. xyz is device memory the context's device can read, 9 floats per
 * triangle; nrm the same kind of array, required for FR_NORMALS_GIVEN and ignored otherwise. The tree is always
 * refitted (FR_BVH_REFIT; compose it with fr_rebuild_bvh_enqueue for a rebuild). The update is enqueued on the context stream
 * after the work already there and the call returns without waiting for the GPU: it synchronises no stream and no
 * event, copies nothing to the host and allocates nothing (what it needs is made by fr_create).
 * ready_event: a hipEvent_t the caller recorded after producing the arrays (the update's first read waits for it
 * on the device), or NULL when the arrays are already complete. The arrays must stay untouched until the update
 * has read them: fr_geometry_consumed(ctx, stream) makes `stream` (a hipStream_t; 0 = the null stream) wait, on
 * the device, for the last enqueued update's reads of the caller's arrays (an event recorded after the last kernel
 * that reads them), so work submitted to that stream afterwards may overwrite them. It does not block the host;
 * with no update enqueued it does nothing.
 * Rejected at once, with nothing enqueued: a NULL context (FR_E_INVALID); NULL xyz, a wrong triangle count, a
 * bad `normals` value, FR_NORMALS_GIVEN with nrm NULL (FR_E_INVALID, fr_last_error); a context that is a rank of a
 * group or has a shard plan of more than one rank (FR_E_UNSUPPORTED: groups stay "each rank's context is updated
 * by its caller", through the synchronous calls).
 * Checked on the device: the finiteness checks of fr_update_geometry run first, and everything of the update that
 * writes scene state reads their verdict from device memory: the taken-over positions, the leaf triangles, every
 * slot box, the normals and the scene box. An update with a position that is not finite, or with a given normal
 * that is not finite on a triangle that has normals, writes none of it: positions, tree, normals, scene box and
 * every later frame are as if the call had not been made, bit for bit (given normals of triangles without normals
 * are ignored, as above). Counters on the device record each verdict: fr_geometry_update_status waits for the
 * context's pending work, as fr_synchronize does, and returns how many enqueued updates were applied and how many
 * rejected since fr_create (either pointer may be NULL); when the rejected count grew since its last call,
 * fr_last_error says which array was not finite.
 * An accepted update equals the synchronous fr_update_geometry(xyz, nrm, ntris, FR_MEM_DEVICE, FR_BVH_REFIT,
 * normals) in every byte of positions, tree, normals and scene box and in every later frame. It counts as a
 * position update for fr_set_motion_reprojection (of several updates before one G-buffer the positions that
 * G-buffer traced are kept; after a rejected update prev equals cur and the frame is the plain one). The scene
 * box (the depth term of the saliency mask) stays in device memory from a context's first enqueued update on;
 * fr_scene_export fetches it, with positions and normals, when asked. The next pipelined frame's front stages
 * start after the update, so they no longer overlap the previous frame's path trace (the tree is refitted in
 * place; fr_set_geometry_overlap below gives the overlap back). Synchronous updates, fr_refit_bvh, fr_set_normals,
 * fr_recompute_normals, fr_snapshot and fr_restore keep their behaviour after enqueued updates (they wait for
 * pending work as always).
 * Not covered: groups and sharded contexts, host-memory arrays (a rebuild without synchronisation is
 * fr_rebuild_bvh_enqueue). */
int fr_update_geometry_enqueue(fr_ctx* ctx, const void* xyz, const void* nrm, size_t ntris, int normals,
                               void* ready_event);
int fr_geometry_consumed(fr_ctx* ctx, void* stream);
/* Enqueued updates beside the path trace (off by default). In place, an enqueued update sits on the context stream
 * between the path trace of the frame before it, which still reads tree and normals, and the front stages of the
 * frame after it. With overlap on, fr_update_geometry_enqueue and fr_set_model_transforms_enqueue refit into a
 * second tree and write a second array of shading records, which no frame in flight reads, on the stream of the
 * front stages; those arrays become the scene's when the call returns (frames already enqueued keep the ones they
 * were given), and the next frame's G-buffer, sampling and compaction follow the update beside the previous path
 * trace. Every word of the two calls' contracts holds: the checks, the verdict on the device (a rejected update
 * leaves the scene as it was, bit for bit), the counters, ready_event, fr_geometry_consumed,
 * fr_geometry_update_status, motion reprojection, the scene box, and bytes equal to the synchronous update's.
 * Every other call behaves as before and orders itself behind a pending update.
 * The first on = 1 makes the second set: the tree arrays fr_create made for fr_rebuild_bvh serve as the second
 * tree (a host-built tree of more nodes than triangles gets bigger ones), and 64 B per triangle are allocated and
 * copied for the shading records (FR_E_NOMEM: nothing is kept and the setting stays off). on = 0 returns to
 * updates in place and frees nothing. No update allocates. The call waits for the context's pending work.
 * FR_E_INVALID for a NULL context or on outside {0, 1}. With overlap off nothing differs from a context that never
 * made the call. Not covered: groups and sharded contexts (their enqueued updates stay FR_E_UNSUPPORTED). */
int fr_set_geometry_overlap(fr_ctx* ctx, int on);
int fr_geometry_update_status(fr_ctx* ctx, uint64_t* applied, uint64_t* rejected);
/* Ray queries: a caller's batch of rays against the scene, traced on the device by the traversal every other ray of
 * the engine uses. rays: n records of 32 B; the direction need not be normalised, t is in units of its length, and
 * tmax = +inf is allowed.
 * FR_RAYS_CLOSEST (out: n fr_ray_hit records): the hit of the reference's intersect_triangle with the smallest t in
 * the open interval (tmin, tmax), both ends strict; of equal t the lowest triangle index. prim is the scene's
 * triangle index (the order of fr_scene_export and fr_model_info, not the tree's leaf order); t, beta and gamma are
 * the bits of that triangle's own test. A miss is (t, beta, gamma, prim) = (+inf, 0, 0, -1): +inf, not the ray's tmax.
 * FR_RAYS_TRANSMITTANCE (out: n floats): the engine's shadow ray (ray type 2) over (tmin, tmax): 0 at the first
 * opaque triangle crossed; otherwise the product over every refractive triangle crossed of 1 - schlick(|n.d|, 5),
 * kept in f64 and rounded to fp32 once (so the order of the crossings changes at most the last bit); 1 when nothing
 * is crossed.
 * Degenerate rays are answered without traversal, as a miss or transmittance 1: a NaN among the eight floats, an
 * origin or a direction that is not finite, the direction (0, 0, 0), and tmin >= tmax.
 * Where the closest hit equals brute force over every triangle, bit for bit. The tree culls by slab planes
 * fma(lo, 1 / d, -o / d) against boxes inflated by 1e-5 + 4e-7 |v| per coordinate v. With u = 2^-24, 1 / d, o / d
 * and the fma each round once: the computed distance is ((lo - o) / d) (1 + e0) (1 + e2) - (o / d) e1 (1 + e0) (1 + e2)
 * with |e| <= u, off by at most (2 |lo - o| + |o|) u / |d_axis| to first order, which is a displacement of the plane
 * along its axis of at most (2 |lo - o| + |o|) u. With every origin coordinate inside the scene box grown on each
 * side by the box's longest edge L, and m the largest coordinate magnitude of the box, |o| <= m + L and
 * |lo - o| <= 2 L, so the displacement is at most (m + 5 L) u = 6e-8 (m + 5 L): below the inflation's constant 1e-5
 * while m + 5 L <= 160 units (the preset scenes: m = 10, L = 20, 6.6e-6), so a point of a triangle stays inside the
 * computed slabs of every box around it with a third of the inflation to spare. The direction's length must lie in
 * [1e-3, 1e3] so that no component of 1 / d or o / d leaves the normal range (2^100 stands for 1 / 0). That is as far
 * as the argument goes: it bounds the planes, not the hit. A hit's own t carries its test's rounding, about
 * 2^-22 (|n_x d_x| + |n_y d_y| + |n_z d_z|) / |n.d| of t, which grows at grazing incidence on triangles off the
 * axes; the guarantee covers a hit while that error times t |d| stays below half the inflation at the hit point. The
 * guaranteed domain is therefore narrower than "every ray from near the scene": a scene with m + 5 L <= 160, origins
 * in the grown box, lengths in [1e-3, 1e3], and hits within that bound.
 * Outside it the call still terminates (the tree is finite and every node is visited at most once) and every hit
 * returned is a true one, the bits of that triangle's own test inside the window; a grazing hit may be culled.
 * Which scene a query sees: tree, leaf triangles, primitive map, shading records and materials as of the call's
 * place in the stream order, after every update, pose, refit and rebuild made or enqueued before the call and before
 * every one after, in place and with fr_set_geometry_overlap on. A rebuild that failed or was skipped on the device
 * and an update rejected there leave the scene, and so the answers, as before.
 * fr_trace_rays waits for the context's pending work and for its own kernel. where (FR_MEM_HOST | FR_MEM_DEVICE)
 * applies to both rays and out. Host arrays go through a staging area of max_rays rays and results, which
 * fr_ray_query_reserve makes: it waits for pending work, allocates 48 B per ray at its first call and again only
 * when the request grows (FR_E_NOMEM keeps what was there); a host batch above the reservation is FR_E_INVALID
 * (fr_last_error names the reservation). Device arrays need no reservation. No query call allocates.
 * fr_trace_rays_enqueue takes device arrays only and enqueues the query on the context stream without waiting for
 * the GPU: it synchronises no stream and no event, copies nothing to the host and allocates nothing. ready_event is
 * as in fr_update_geometry_enqueue. rays and out must stay untouched until fr_rays_consumed(ctx, stream) has made
 * `stream` (a hipStream_t; 0 = the null stream) wait, on the device, for the last enqueued query's kernel: its reads
 * of rays and its writes of out. Work submitted to that stream afterwards may read the results and overwrite the
 * rays. It does not block the host; with no query enqueued it does nothing. The enqueued form joins no
 * reconstruction and leaves the frame pipeline's schedule as it was.
 * Refused at once, nothing enqueued, out untouched: a NULL context, NULL rays or out with n > 0, a bad kind or
 * where, n > 2^30, a device pointer not 16-byte aligned (out of FR_RAYS_TRANSMITTANCE: 4-byte), rays and out
 * overlapping (FR_E_INVALID); the enqueued form on a rank of a group or a sharded context (FR_E_UNSUPPORTED; the
 * synchronous form works there). n == 0 is FR_OK and enqueues nothing.
 * A query touches no image buffer, no temporal state, no counter of fr_stats: query rays are not counted, nothing of
 * the JumpFlooding reuse, and no schedule of another context.
 * Not covered by these two calls: groups in stream order; the surface at the hit and per-ray model masks are the
 * masked calls' (below). */
typedef struct fr_ray     { float origin[3]; float tmin; float dir[3]; float tmax; } fr_ray;      /* 32 B */
typedef struct fr_ray_hit { float t; float beta, gamma; int32_t prim; } fr_ray_hit;               /* 16 B */
#define FR_RAYS_CLOSEST       0   /* out: n fr_ray_hit */
#define FR_RAYS_TRANSMITTANCE 1   /* out: n floats */
int fr_ray_query_reserve(fr_ctx* ctx, size_t max_rays);
int fr_trace_rays(fr_ctx* ctx, const void* rays, size_t n, int where, int kind, void* out);
int fr_trace_rays_enqueue(fr_ctx* ctx, const void* rays, size_t n, int kind, void* out, void* ready_event);
int fr_rays_consumed(fr_ctx* ctx, void* stream);
/* Ray queries, second part: the surface at the hit, and per-ray model masks. fr_trace_rays_masked and
 * fr_trace_rays_masked_enqueue are fr_trace_rays and fr_trace_rays_enqueue with two additions; with masks == NULL and
 * one of the two kinds above they are those calls exactly. fr_trace_rays and fr_trace_rays_enqueue themselves keep
 * their two kinds and refuse FR_RAYS_SURFACE as a bad kind, as they always have.
 * FR_RAYS_SURFACE (out: n fr_ray_surface records of 80 B, five 16-byte rows; a device `out` is 16-byte aligned): the
 * FR_RAYS_CLOSEST answer followed by the closest-hit programs' view of that hit, as the G-buffer and the path trace
 * compute it. Every field has one right answer in bytes: fp32, the fmas written out below, dot products contracted
 * and normalize as the reference's PTX has them and as every kernel of the engine does.
 *   row 0          the fr_ray_hit FR_RAYS_CLOSEST returns for this ray: same window, tie rule and guaranteed domain.
 *   attribute normal  g = normalize(n), n the stored normal of the hit's leaf triangle (cross(p0 - p2, p1 - p0), each
 *                  product rounded), not a recomputation from positions.
 *   ng             normalize(g): the reference normalises the attribute a second time.
 *   ns             a = normalize(fma(w, n0, fma(beta, n1, gamma * n2))), w = 1 - beta - gamma, per component;
 *                  ns = normalize(a) for a triangle with flags & 0x100, else ns = ng.
 *   (u, v)         fma(w, t0, fma(beta, t1, gamma * t2)) per component when flags & 0x200, else (0, 0).
 *   point          the front point of refine_and_offset(fma(t, d, o), d, g, p0), p0 the leaf triangle's first vertex;
 *                  d as given, not normalised.
 *   kd             .xyz of the Kd texture lookup at (u, v): REPEAT wrap, bilinear with 8-bit fractions, the texture
 *                  of material m = flags & 0xff.
 *   model          the i with first_tri[i] <= prim < first_tri[i + 1] (fr_model_info).
 *   surface        m | type << 8 | (flags & 0x300) << 8 | back << 18: type the material's 0 (diffuse), 1
 *                  (reflection) or 2 (refraction); bits 16 and 17 say the triangle has normals and uv; back = 1 when
 *                  dot(g, d) > 0, the side test refine_and_offset makes.
 *   a miss, a degenerate ray, a mask that selects no model: row 0 is the miss record, model = -1, every other word 0.
 * For the camera ray of a pixel (tmin = the scene epsilon 1e-3, tmax = +inf) point equals POSITION.xyz,
 * fma(ng, 0.5, 0.5) equals NORMAL.xyz, kd equals DIFFUSE.xyz as values and the class of type equals GCLASS, after
 * fr_geometry_launch on the same scene.
 * masks: NULL, or n words, one per ray: bit k set means model k (fr_model_info's order) takes part in that ray. Bits
 * at or above the model count are ignored. A ray whose mask selects no model is answered without traversal, as a
 * degenerate ray is. FR_RAYS_CLOSEST and FR_RAYS_SURFACE then answer the closest hit among the triangles of the
 * selected models, with the tie rule among them; for FR_RAYS_TRANSMITTANCE an excluded model neither blocks nor
 * attenuates. The answers equal brute force over the selected models' triangles under the terms above (bit for bit in
 * the guaranteed domain; transmittance exactly 0 and 1, within one ulp between). With masks, the power of a
 * refractive crossing's Schlick term is rounded once ((1 - |ns.d|)^5 in f64, then to fp32), where the unmasked kind
 * and the frame's shadow rays take the platform's powf: a masked transmittance with every bit set and the unmasked one
 * agree in their exact zeros and ones and may differ in the last bits between. The unmasked kind therefore holds the
 * one-ulp bound against the restatement on unit directions only, where it was measured; on directions of other lengths
 * its answers have been seen up to 94 ulp away. Making the two forms one means changing the frame's shadow ray, and is
 * left as follow-up work. The tree is walked as without masks:
 * a candidate is dropped after its triangle test accepts it, so a mask never makes a query cheaper than its traversal.
 * Stream order, the scene a query sees, ready_event and fr_rays_consumed are as above; fr_rays_consumed also covers
 * the reads of masks. where applies to rays, masks and out alike.
 * Host staging: fr_ray_query_reserve(n) keeps meaning 48 B per ray, and a host batch of the first two kinds without
 * masks is accepted when n is within it. fr_ray_query_reserve_kind sizes the same area for max_rays rays of one kind:
 * 32 B per ray, plus the kind's result (16, 4 or 80 B), plus 4 B when masked; it grows the area only, waits for
 * pending work, and fails with FR_E_NOMEM keeping what was there. A host batch with masks or of FR_RAYS_SURFACE is
 * accepted when its bytes fit the area. No query call allocates.
 * Refused at once, nothing enqueued, out untouched (FR_E_INVALID): what the calls above refuse, with an 80-byte stride
 * in the overlap test of FR_RAYS_SURFACE; a device masks pointer not 4-byte aligned; masks overlapping out; a host
 * batch above the area. FR_E_UNSUPPORTED: the enqueued form on a rank of a group or a sharded context; masks or
 * FR_RAYS_SURFACE on a scene of more than FR_MAX_MODELS models.
 * Not covered: groups in stream order, per-ray windows beyond tmin / tmax, any-hit callbacks, instance transforms. */
typedef struct fr_ray_surface {
  float t, beta, gamma; int32_t prim;   /* row 0: the fr_ray_hit of FR_RAYS_CLOSEST */
  float point[3];       int32_t model;  /* row 1: front_hit_point; index into fr_model_info */
  float ng[3];          float   u;      /* row 2: world_geometric_normal; texcoord.x */
  float ns[3];          float   v;      /* row 3: world_shading_normal; texcoord.y */
  float kd[3];          int32_t surface;/* row 4: the Kd lookup at (u, v); material word */
} fr_ray_surface;                       /* 80 B */
#define FR_RAYS_SURFACE 2   /* out: n fr_ray_surface; the masked calls only */
int fr_ray_query_reserve_kind(fr_ctx* ctx, size_t max_rays, int kind, int masked);
int fr_trace_rays_masked(fr_ctx* ctx, const void* rays, const uint32_t* masks, size_t n, int where, int kind, void* out);
int fr_trace_rays_masked_enqueue(fr_ctx* ctx, const void* rays, const uint32_t* masks, size_t n, int kind, void* out,
                                 void* ready_event);
/* The scene's models, posed by matrix on the device. A scene is assembled from rigid models (ground, box, bunny,
 * earth, vokselia_spawn: PathTracer::load_obj's meshes with their transforms baked in), each a contiguous range of
 * the scene's triangles. The ranges partition [0, num_tris) in scene order: fr_model_count gives their number,
 * fr_model_info one model's name (borrowed, valid for the life of the context), first triangle and triangle
 * count (any of the three pointers may be NULL); FR_E_INVALID for a NULL context or an index outside the table.
 * A pose is one matrix per model, 12 floats each, row-major 3 x 4: M[r][0..3], v' = A v + t, relative to the rest
 * geometry (below). A posed array has one right answer in bytes. fp32, every operation rounded on its own, no
 * fma, for a corner (p, n) of a model whose matrix is not the identity:
 *   p'.c = ((M[c][0] p.x + M[c][1] p.y) + M[c][2] p.z) + M[c][3]                                    c = 0, 1, 2
 *   K[r][c] = A[r1][c1] A[r2][c2] - A[r1][c2] A[r2][c1]     (r1, r2) = ((r + 1) % 3, (r + 2) % 3), (c1, c2) likewise
 *   n'.c = (K[c][0] n.x + K[c][1] n.y) + K[c][2] n.z
 *   det = (A[0][0] K[0][0] + A[0][1] K[0][1]) + A[0][2] K[0][2]
 * K is the cofactor matrix, det times the inverse transpose, so with det > 0 a normal keeps the direction the
 * inverse transpose gives it; normals are not renormalised (the shader normalises where it reads them). A model
 * is at the identity when its 12 floats compare equal (==, so -0 counts as 0) to (1,0,0,0, 0,1,0,0, 0,0,1,0): it
 * takes its rest positions and rest normals bit for bit (the arithmetic would turn a -0 coordinate into +0).
 * Triangles without normals (flags & 0x100 clear) keep what they have, as in every update with given normals.
 * Rest geometry: fr_model_pose_enable(ctx, 1) waits for the context's pending work, allocates at its first call
 * four device arrays of 36 B per triangle (rest positions, rest normals, and the two arrays the posed geometry is
 * staged in; FR_E_NOMEM, with nothing kept), captures the current device positions and normals as rest and
 * resets the stored pose to identities. Calling it again captures again: that is how a mesh deformed through
 * fr_update_positions is posed. on = 0 makes the pose calls return FR_E_STATE until the next on = 1; it frees
 * nothing and changes nothing of the scene. A scene of more than FR_MAX_MODELS models: FR_E_UNSUPPORTED. No pose
 * call allocates.
 * fr_set_model_transforms computes X and N, the posed rest positions and normals, on the device (one kernel,
 * the matrices travel in its arguments: no copy, nothing of the caller's is read after the call returns) and then
 * is fr_update_geometry(X, N, ntris, FR_MEM_DEVICE, how, FR_NORMALS_GIVEN): every later frame, positions,
 * normals, tree, scene box and fr_bvh_sah_cost are byte for byte what that call leaves, a pose counts as a
 * position update for fr_set_motion_reprojection, and like it the call waits for the context's pending work.
 * fr_set_model_transforms_enqueue is the same against fr_update_geometry_enqueue(X, N, ntris, FR_NORMALS_GIVEN,
 * NULL): a refit in stream order with no host wait, which a caller without device code of their own can use
 * before every frame; consecutive poses need no event and no fr_geometry_consumed (the staged arrays belong to
 * the context). fr_model_transforms returns the pose last submitted (identities after an enable).
 * Refused at once, with nothing enqueued and the scene untouched: a NULL context or NULL m, nmodels other than
 * the model count, a bad `how`, a float of m that is not finite, a model whose det (the rule above) is not finite
 * or is <= 0 (a mirrored model flips the triangle winding, and with it the geometric normal refraction depends
 * on): FR_E_INVALID; posing not enabled: FR_E_STATE; for the enqueued form a rank of a group or a sharded
 * context: FR_E_UNSUPPORTED (the synchronous form works on a group's contexts one by one).
 * A finite pose can still overflow the positions. That is caught where fr_update_geometry catches an array that
 * is not finite: the synchronous call returns FR_E_INVALID, the enqueued one is rejected on the device and
 * counted by fr_geometry_update_status; both leave the scene untouched.
 * With fr_set_geometry_overlap on, the enqueued form poses, refits and writes the normals beside the previous
 * frame's path trace.
 * Not covered: per-model materials, instancing, a two-level tree, changed triangle counts, groups in stream order
 * (per-model visibility: below). */
#define FR_MAX_MODELS 16
int fr_model_count(fr_ctx* ctx, int* n);
int fr_model_info(fr_ctx* ctx, int i, const char** name, int* first_tri, int* ntris);
int fr_model_pose_enable(fr_ctx* ctx, int on);
int fr_set_model_transforms(fr_ctx* ctx, const float* m, size_t nmodels, int how);  /* FR_BVH_REFIT | FR_BVH_REBUILD */
int fr_set_model_transforms_enqueue(fr_ctx* ctx, const float* m, size_t nmodels);
int fr_model_transforms(fr_ctx* ctx, float* m, size_t nmodels);
/* Per-model visibility: models hidden from and shown to every frame and ray query, in stream order. Bit k of
 * `visible` clear means model k (fr_model_info's order) is hidden; bits at or above the model count are ignored and
 * read back clear; the default is every model visible. Visibility is applied where the tree is written, not where
 * it is traversed. The collapsed positions C(P, visible) are P, except that a triangle t of a hidden model takes
 * P[3t] for all three corners (the bits are copied): such a triangle has a zero normal and fails the triangle test
 * of every ray, and its box is a point. From the call on, at its place in the stream order, every tree writer reads
 * C(current positions, visible): the call's own refit or rebuild, fr_refit_bvh and fr_rebuild_bvh, fr_set_positions,
 * fr_update_positions, fr_update_geometry, fr_set_model_transforms, the enqueued forms of these,
 * fr_rebuild_bvh_enqueue, fr_rebuild_bvh_enqueue_if and the rebuild policy. The tree has one right answer in bytes:
 * the tree the same call makes without this feature over those positions. A hidden model costs a frame nothing.
 * Ray queries read the same tree: a hidden model neither wins, ties, blocks nor attenuates, in all three kinds,
 * masked or not (the effective mask is masks[i] & visible).
 * What does not change: the exported positions, normals, uv, flags and materials; the scene box the saliency mask
 * reads (the box of the true positions); the weld and fr_recompute_normals (true positions); the pose rest
 * geometry; motion reprojection (a visibility change is not a position update: the frame after it reprojects as
 * over still geometry); fr_geometry_update_status and the policy's update count. A snapshot does not carry it.
 * fr_model_visibility_enable(ctx, 1) waits for the context's pending work and allocates at its first call one
 * device position array of 36 B per triangle (FR_E_NOMEM, with nothing kept and the setting off); no other call of
 * this feature allocates. on = 0 makes the two set calls return FR_E_STATE until the next on = 1, is itself
 * FR_E_STATE while a model is hidden, and frees nothing. More than FR_MAX_MODELS models: FR_E_UNSUPPORTED.
 * fr_set_model_visibility waits as fr_refit_bvh does, then refits (FR_BVH_REFIT) or rebuilds with the context's
 * builder (FR_BVH_REBUILD) over C, also when the mask is the one in place; a failed rebuild leaves the tree and the
 * mask as they were. fr_set_model_visibility_enqueue is the refit in stream order, as fr_update_geometry_enqueue
 * with kept normals is: no host wait, no copy, no allocation; with fr_set_geometry_overlap on it refits into the
 * other set beside the previous frame's path trace. The mask changes at enqueue time: updates, poses and rebuilds
 * enqueued later use it. An enqueued update the device rejects while a model is hidden leaves the tree as it was.
 * Refused with nothing enqueued and tree and mask untouched: a NULL context or out-pointer, a bad `how`:
 * FR_E_INVALID; visibility not enabled: FR_E_STATE; the enqueued form on a rank of a group or a sharded context, or
 * without a refit workspace: FR_E_UNSUPPORTED (the synchronous form works on a group's contexts one by one).
 * fr_model_visibility returns the mask last submitted, valid bits only.
 * The rebuild policy: a tree written by either set call came by another route, so the next
 * fr_rebuild_bvh_enqueue_if adopts its cost as the baseline and skips (showing a model would otherwise look like a
 * tree that has grown). fr_bvh_sah_cost reports the tree in use, the point boxes of hidden triangles included.
 * Not covered: per-ray-class visibility (hidden from the camera but casting shadows), groups in stream order. */
#define FR_VISIBLE_ALL 0xffffffffu
int fr_model_visibility_enable(fr_ctx* ctx, int on);
int fr_set_model_visibility(fr_ctx* ctx, uint32_t visible, int how);   /* FR_BVH_REFIT | FR_BVH_REBUILD */
int fr_set_model_visibility_enqueue(fr_ctx* ctx, uint32_t visible);    /* refit, stream order */
int fr_model_visibility(fr_ctx* ctx, uint32_t* visible);               /* last submitted, & valid bits */
/* History that follows moving geometry (off by default). The G-buffer reprojects a hit point with the previous
 * camera, and the sampling stage accepts the history there only when the depth stored a frame ago equals the
 * point's distance from the previous eye: both assume the point stood still. With motion reprojection on, the
 * first G-buffer after a position update (fr_set_positions, fr_update_positions, fr_update_geometry) moves each
 * hit point back to where the same point of its triangle (same barycentrics) was when the previous G-buffer
 * traced it. fp32, every fma written out; for a hit (prim k, beta b, gamma g) over positions P (3 per triangle):
 *   w = 1.0f - b - g;  blend(P).c = fma(w, P[3k].c, fma(b, P[3k+1].c, g * P[3k+2].c))        c = x, y, z
 *   delta = blend(prev) - blend(cur);  hp_prev = delta == (0, 0, 0) ? hp : hp + delta         hp = POSITION
 *   WEIGHT = (reprojection of hp_prev, length(hp_prev - prev_eye), 1)
 * and that frame's sampling stage tests DEPTH_CACHE against WEIGHT.z instead of length(POSITION - prev_eye); it
 * still leaves WEIGHT = (qu, qv, valid, 0). A triangle whose nine floats did not change gets the bits it gets
 * today, as does every frame with no update since the last G-buffer and every frame with the feature off. prev
 * is the positions the most recent G-buffer traced: of several updates before one G-buffer the first one's
 * outgoing positions are kept. A rejected update or a failed rebuild changes nothing; fr_refit_bvh,
 * fr_rebuild_bvh, fr_set_normals and fr_recompute_normals neither. The first on = 1 allocates one more device
 * position array (36 B per triangle; FR_E_NOMEM); nothing is allocated per frame or per update (the arrays
 * rotate, no copy). on = 0 drops a pending motion (the positions then in place count as the ones the last G-buffer
 * traced), and so does fr_restore (a snapshot does not carry the previous positions: the frame after a restore
 * reprojects as over still geometry). FR_E_INVALID for a NULL
 * context or on outside {0, 1}. The call waits for the context's pending work. Not covered: a changed triangle
 * count, a sampling launch repeated for one G-buffer (the repeat runs the plain test), groups (each rank's
 * context is switched and updated by its caller). */
int fr_set_motion_reprojection(fr_ctx* ctx, int on);
/* Buffer access (PathTracer::get_texture, FR/PathTracer.cpp:337-374; rtBufferMap). */
int fr_get_buffer(fr_ctx* ctx, int id, fr_buffer_view* view);
int fr_read_buffer(fr_ctx* ctx, int id, void* host, size_t bytes);
int fr_write_buffer(fr_ctx* ctx, int id, const void* host, size_t bytes);
int fr_copy_buffer(fr_ctx* ctx, int id, void* device_dst, size_t bytes);  /* device-to-device, synchronous */
/* Snapshot / restore of the temporal state a frame hands to the next (the reference keeps it in
 * the history / depth ping-pong, FR/PathTracer.cpp:226-238, and in the push atlas carried across frames,
 * FR/PullPushInterpolation.cpp:57-58): HISTORY_CACHE / HISTORY, DEPTH_CACHE / DEPTH, the pull and push atlases
 * and the push snapshot texels, m_accumFrame (with a pending light reset), the light emission, the diffuse
 * depth and the last camera / gaze uniforms. fr_snapshot_bytes gives the size; fr_snapshot copies it to host
 * memory after all pending work; fr_restore loads it into a context of the same size, spp and scene
 * (FR_E_INVALID otherwise), so the next frame equals the one that followed the snapshot, bit for bit. */
int fr_snapshot_bytes(fr_ctx* ctx, size_t* bytes);
int fr_snapshot(fr_ctx* ctx, void* host, size_t bytes);
int fr_restore(fr_ctx* ctx, const void* host, size_t bytes);

/* Present: a reconstructed image as packed 8-bit texels, delivered in stream order without draining the context (the
 * reference's last step: renderAll draws the float textures into an 8-bit framebuffer, FR/main.cpp:26-113, which
 * saveBMP24 reads back as BGRA bytes, bottom row first, FR/gui.cpp:315-355). Nothing here changes a context that does
 * not use it: a context that never calls fr_present_enable creates the streams it created and enqueues what it enqueued.
 *
 * The rule, with one right answer in bytes. For a channel value x (fp32), every operation rounded on its own, no fma:
 *   v = (x != x) ? 0.0f : fminf(fmaxf(x, 0.0f), 1.0f)        NaN -> 0, -Inf -> 0, +Inf -> 1, -0 -> 0
 *   q = (uint8_t)(uint32_t)(v * 255.0f + 0.5f)               one product, one sum, truncation
 * GL's float -> UNORM8 conversion with round half up; k / 255 gives k. The stored values are display values already
 * (the tone map and its power are applied in the shading resolve), so there is no transfer curve. r, g and b are
 * converted, the alpha byte is always 255. FR_PRESENT_RGBA8: bytes r g b a per texel; FR_PRESENT_BGRA8: b g r a. Row 0
 * of the output is the bottom row, as in every buffer of the engine (BGRA8 is then the payload saveBMP24 writes);
 * with FR_PRESENT_TOP_DOWN or-ed into the format, output row r is image row H - 1 - r. The output is tight: W * 4
 * bytes per row, W * H * 4 in all. fr_present_pack states the rule on the host, without a device, through the function
 * the kernel runs (rgba: W * H * 4 floats); FR_E_INVALID: a NULL pointer, a size outside 1..32767, an unknown format.
 *
 * fr_present_enable(ctx, slots, format), slots 1..8: the first call waits for the context's pending work and makes
 * everything the feature needs: one more stream (the present stream), per slot a device staging image and a pinned
 * host image of W * H * 4 bytes with their events, and the fences that order later frames behind a present's read.
 * FR_E_NOMEM keeps nothing and leaves the feature off. A later call with other arguments waits, requires every ticket
 * to be released (FR_E_STATE otherwise) and remakes the ring (tickets keep counting); with the same arguments it does
 * nothing. slots = 0 turns the feature off under the same condition: the other calls then return FR_E_STATE; nothing
 * is freed before fr_destroy. No other call of the feature allocates.
 *
 * What a present sees: the buffer as it stands at the call's place in the stream order, behind every frame, stage call
 * and write made or enqueued before the call and ahead of every one after it. FR_BUF_SHADING, FR_BUF_SIBSON,
 * FR_BUF_PULLPUSH and FR_BUF_ATROUS are accepted and resolved at the call (SHADING is this frame's, ATROUS the last
 * A-Trous output). fr_present_enqueue makes no host wait and no copy to the host that anything waits for: the present
 * stream waits, on the device, for what writes the image, packs it into the next free slot's staging image and copies
 * that to the slot's pinned image; frames enqueued afterwards run meanwhile, and whatever overwrites the image next
 * waits for the pack's read only. *ticket counts from 1. When every slot is held (enqueued and not yet released) the
 * call returns FR_E_STATE and enqueues nothing: that is the backpressure.
 * fr_present_acquire(ctx, ticket, wait, &host): wait = 1 blocks until that slot's copy has landed, and on nothing else
 * (not on the context: later frames keep running); wait = 0 returns FR_PRESENT_PENDING or FR_OK. *host is the slot's
 * pinned image, borrowed until fr_present_release. Tickets are acquired and released in any order; a ticket may be
 * released without ever being acquired (the slot's next use is ordered behind its copy on the present stream); an
 * unknown or already released ticket is FR_E_INVALID. fr_present_times gives, for an acquired ticket, the pack
 * kernel's and the copy's time from the slot's events on the present stream (either pointer may be NULL; FR_E_STATE:
 * not acquired yet).
 * fr_present_enqueue_device is the same pack straight into the caller's device memory (16-byte aligned, bytes ==
 * W * H * 4): no slot, no host copy. fr_present_done(ctx, stream) makes `stream` (a hipStream_t; 0 = the null stream)
 * wait, on the device, for the last such pack, as fr_rays_consumed does for a query.
 * fr_synchronize and fr_destroy also wait for the present stream. A snapshot carries nothing of the ring, and
 * fr_restore leaves it alone.
 * Refused with nothing enqueued and nothing written: a NULL context or out-pointer, another buffer id, slots outside
 * 0..8, an unknown format, a wrong bytes, a misaligned or NULL device_dst (FR_E_INVALID); the feature not enabled, or
 * the ring full (FR_E_STATE); either enqueue on a rank of a group or on a sharded context (FR_E_UNSUPPORTED, as with
 * every other enqueued call).
 *
 * Present through a homography: late reprojection ("timewarp"), crop and scale, in the same place and the same order.
 * fr_present_enqueue_warped and fr_present_enqueue_warped_device are the two enqueue calls above with a projective map
 * between the image and the texels: the same buffers, resolved at the call; the same waits of the present stream; the
 * same fence behind the kernel's read; the same ring, tickets, acquire, release, times and fr_present_done. Plain and
 * warped presents may be mixed freely. The output is ow x oh texels, tight, 1 <= ow <= W and 1 <= oh <= H
 * (out_width = out_height = 0 means W x H), so a slot's images hold it; only ow * oh * 4 bytes are copied to the host,
 * and `bytes` of the device form must equal that. The warp is read during the call and travels in the kernel's
 * arguments: nothing of the caller's is kept.
 * The rule, with one right answer in bytes. S is the W x H source, row 0 at the bottom; h[0..8] is row-major and takes
 * the centre of an output texel to a source texel coordinate (texel i covers [i, i + 1), its centre is i + 0.5). For
 * output column x and output row r, y = r, or oh - 1 - r with FR_PRESENT_TOP_DOWN. All fp32, every operation rounded
 * on its own, no fma, '/' correctly rounded, subnormal results kept:
 *   px = (float)x + 0.5f                 py = (float)y + 0.5f
 *   u  = (h[0]*px + h[1]*py) + h[2]
 *   v  = (h[3]*px + h[4]*py) + h[5]
 *   w  = (h[6]*px + h[7]*py) + h[8]
 *   if !(w > 0)                                  -> border
 *   iw = 1.0f / w
 *   fx = u*iw - 0.5f                     fy = v*iw - 0.5f
 *   if !(fx >= -0.5f && fx < (float)W - 0.5f &&
 *        fy >= -0.5f && fy < (float)H - 0.5f)    -> border     (false for NaN and +-Inf)
 *   x0 = floorf(fx)   tx = fx - x0   xa = max((int)x0, 0)   xb = min((int)x0 + 1, W - 1)      (the same for y)
 *   row(j)   = (tx == 0) ? S[j][xa] : S[j][xa]*(1 - tx) + S[j][xb]*tx        per channel r, g, b
 *   value    = (ty == 0) ? row(ya) : row(ya)*(1 - ty) + row(yb)*ty
 *   byte     = the rule above of value;  alpha 255;  a border texel is 0, 0, 0, 255
 * A tap of weight 0 is not read. So the identity with ow x oh = W x H gives the plain present's bytes for every source
 * value, NaN and Inf next door included; h = [1 0 dx; 0 1 dy; 0 0 1] with integers dx, dy is an exact crop or shift
 * with border texels where it leaves the image; and where w <= 0 or the quotient overflows (a display camera turned
 * past the source's horizon) the texel is border. Within half a texel outside the source the edge texels repeat.
 * The two maps a caller writes by hand: the crop of ow x oh texels whose lower left texel is (x0, y0),
 * [1 0 x0; 0 1 y0; 0 0 1], and the scale of the whole image to ow x oh, [W/ow 0 0; 0 H/oh 0; 0 0 1].
 * fr_present_warp_pack states the rule on the host, without a device, through the function the kernel runs (out:
 * out_width * out_height * 4 bytes); FR_E_INVALID as fr_present_pack, and for a NULL warp, a non-finite coefficient or
 * an output size outside those limits.
 * fr_present_warp_from_poses (host only, f64 throughout, rounded once to fp32) builds the map for a late reprojection:
 * the output is out_width x out_height texels over the display camera's whole viewport, rows bottom-up; the source is
 * the width x height image the rendered camera produced; a texel centre maps to where the rendered camera sees the
 * point that lies on the display camera's ray at NDC depth ndc_depth (fr_camera_matrices' projection: z in [-1, 1],
 * +1 the far plane). With M = proj * view of fr_camera_matrices, that is S (M_r M_d^-1) restricted to z = ndc_depth
 * T, with T from output texel coordinates to the display camera's NDC and S from the rendered camera's NDC to source
 * texel coordinates, scaled so that h[8] = 1. With equal eye positions the map does not depend on ndc_depth (pure
 * rotation: exact for any scene depth); equal poses give [W/ow 0 0; 0 H/oh 0; 0 0 1] exactly, the identity for
 * out = width x height. FR_E_INVALID, with *warp untouched: a NULL pointer, a size outside 1..32767, a non-finite
 * depth, a singular or non-finite matrix, or an h[8] that cannot be normalised: before scaling, h[8] is the rendered
 * camera's clip w of output corner (0, 0) and must exceed 2^-20 * max(|h[6]| * out_width, |h[7]| * out_height, |h[8]|)
 * (at or below zero that corner lies on or behind the rendered camera's eye plane, and no positive scale exists).
 * Refused with nothing enqueued, nothing written and no ticket taken, beside the refusals above with their codes: a
 * NULL warp, a non-finite coefficient, an output size outside the limits, a wrong bytes, a NULL or misaligned
 * device_dst (FR_E_INVALID).
 *
 * Blended present: one image that is one reconstruction where the user looks and another in the periphery (the
 * reference draws SIBSON and ATROUS side by side, FR/main.cpp:26-113; a foveated display wants the sharp one at the
 * gaze, the denoised one around it, and no visible seam). fr_present_enqueue_blended and
 * fr_present_enqueue_blended_device are the enqueue calls above whose source is a virtual image: each of its texels
 * is a mix of two presentable buffers, weighted by the texel's squared distance from a gaze point. Everything after
 * that texel is what is described above: the 8-bit rule, formats and row orders, the ring, tickets, acquire, release,
 * times and fr_present_done; with a warp (NULL: none, the output is W x H) the virtual image is the S of the warped
 * rule, so the blend is evaluated at each source tap, before the bilinear filter. Plain, warped and blended presents
 * may be mixed freely.
 * The rule, with one right answer in bytes. fp32, every operation rounded on its own, no fma, '/' correctly rounded,
 * subnormal results kept. gaze is in fr_camera.gaze's coordinates (texels, row 0 at the bottom) and may lie off
 * screen; r0sq = inner_radius_px * inner_radius_px and r1sq = outer_radius_px * outer_radius_px, one fp32 product
 * each, formed on the host. For source texel (i, j):
 *   dx = (float)i - gaze[0]      dy = (float)j - gaze[1]      d2 = dx*dx + dy*dy
 *   d2 <= r0sq     -> s = 0
 *   !(d2 < r1sq)   -> s = 1      (d2 >= r1sq, +Inf included; and a d2 that is not a number, which fails both tests)
 *   otherwise         t = (d2 - r0sq) / (r1sq - r0sq)     a = 2.0f*t     b = 3.0f - a     c = t*t     s = c*b
 *   s == 0 -> texel = inner[j][i]          outer is not read
 *   s == 1 -> texel = outer[j][i]          inner is not read
 *   else      texel.c = inner.c*(1.0f - s) + outer.c*s          per channel r, g, b: two products, one sum
 * d2 is FR_MASK_ECCENTRIC's, so with inner_radius_px = fr_foveation.radius_px the disc that shows `inner` alone is the
 * disc that mask samples fully. s is the smoothstep of t and never exceeds 1. The select is on s itself, not on the
 * zone: inside the ramp s is exactly 0 where t is tiny (t*t underflows) and exactly 1 where t is within about 2^-13
 * of 1, and there too the source of weight zero is not read, so a NaN in it does not reach the texel. With a finite
 * gaze d2 is never NaN (it is +Inf where dx*dx overflows: s = 1); the rule gives a NaN d2 s = 1 all the same.
 * inner_radius_px == outer_radius_px is a hard edge at d2 <= r0sq. inner_buffer == outer_buffer is allowed.
 * fr_present_blend_default (host state only, waits for nothing) fills: inner_buffer = FR_BUF_SIBSON, outer_buffer =
 * FR_BUF_ATROUS, gaze = the gaze the kernels use from the next launch on (fr_set_camera, fr_set_gaze), inner_radius_px
 * = the radius_px fr_get_foveation returns, outer_radius_px = 2.0f * inner_radius_px (one fp32 product).
 * fr_present_blend_pack states the rule on the host, without a device, through the functions the kernels run (inner,
 * outer: width * height * 4 floats each; warp NULL: out holds width * height * 4 bytes, else out_width * out_height *
 * 4); it ignores the two buffer ids. FR_E_INVALID as fr_present_warp_pack (a NULL warp excepted) and as below.
 * The two enqueues resolve both buffers at the call, read the blend and the warp during the call (they travel in the
 * kernel's arguments: nothing of the caller's is kept), wait for nothing on the host and allocate nothing. The present
 * stream waits as for one image; behind the kernel the fence of each source is recorded, so the next writer of either
 * image waits for this read.
 * Refused with nothing enqueued, nothing written and no ticket taken: everything the enqueues above refuse, with the
 * same codes (a warp is checked only when one is given); a NULL blend, an inner_buffer or outer_buffer that is not
 * presentable, a non-finite gaze or radius, a negative radius, inner_radius_px > outer_radius_px, an outer_radius_px
 * whose fp32 square is not finite (FR_E_INVALID).
 *
 * Present with positional reprojection: a depth-aware splat of POSITION. The homography is exact for a rotation of the
 * head only; a translation is right at ndc_depth and wrong everywhere else, so near objects swim against far ones.
 * fr_present_enqueue_reprojected and fr_present_enqueue_reprojected_device are the two warped enqueue calls with the
 * frame's world-space hit points beside the image: every texel moves to where the display camera sees its hit point,
 * the nearest texel wins where several land in one place, and the homography fills where nothing lands (sky,
 * disocclusions). They are the warped enqueues in every respect of ordering: the same buffers, resolved at the call;
 * the same waits of the present stream; the same ring, tickets, acquire, release, times and fr_present_done; only
 * ow * oh * 4 bytes go to the host; rp is read during the call and travels in the kernels' arguments. POSITION is the
 * frame slot's at the call, as fr_read_buffer(FR_BUF_POSITION) would resolve it there; behind the kernels the fence
 * its next writer waits for is recorded beside the source's. Plain, warped, blended and reprojected presents may be
 * mixed freely.
 * The rule, with one right answer in bytes. fp32, every operation rounded on its own, no fma, '/' correctly rounded.
 * S is the W x H source image and P the W x H POSITION image, row 0 at the bottom; the output is ow x oh, 1 <= ow <= W
 * and 1 <= oh <= H (0, 0 means W x H): the fallback's output size. vp[0..15] is row-major and takes a world point to
 * the display camera's clip space. K is an ow x oh image of 64-bit keys; its row 0 is the bottom row, whatever the
 * output's row order.
 *   1. Clear. Every K[y][x] = 0xFFFFFFFFFFFFFFFF.
 *   2. Splat. For every source texel (i, j), with p = P[j][i]:
 *        if p.x == 0 && p.y == 0 && p.z == 0                      -> skip   (the G-buffer writes exactly 0, 0, 0, 1
 *                                                                           for a miss: sky has no depth)
 *        cx = ((vp[0]*p.x + vp[1]*p.y) + vp[2]*p.z) + vp[3]       cy alike from row 1, cw from row 3; row 2 is not used
 *        if !(cw > 0)                                             -> skip
 *        iw = 1.0f / cw
 *        sx = ((cx*iw)*0.5f + 0.5f) * (float)ow                   sy = ((cy*iw)*0.5f + 0.5f) * (float)oh
 *        if !(sx >= 0 && sx < (float)ow && sy >= 0 && sy < (float)oh)  -> skip   (false for NaN and +-Inf: non-finite
 *                                                                                positions fall out here)
 *        ox = (int)sx      oy = (int)sy
 *        q   = the packed 8-bit word of S[j][i] by the rule at the top, in the ring's format (byte 0 lowest)
 *        key = ((uint64)bits(cw) << 32) | q
 *        K[oy][ox] = min(K[oy][ox], key)                          as unsigned 64-bit
 *      cw > 0, so its bits order as its value: the nearest point wins; equal depths go to the smaller word. The
 *      minimum does not depend on the order of arrival, which is why the scatter has one right answer.
 *   3. Resolve. For output column x and output row r, y = r, or oh - 1 - r with FR_PRESENT_TOP_DOWN:
 *        K[y][x] is not all ones                                  -> the texel is its low word
 *        else, the crack rule: (left and right are both inside the image and both covered) or (below and above are
 *        both inside the image and both covered), in K as the splat left it
 *                                                                 -> the low word of the smallest key among the
 *                                                                    covered 4-neighbours
 *        else                                                     -> the warped rule's texel of the fallback
 *                                                                    homography at (x, y), unchanged, border texels
 *                                                                    included
 *      A one-texel crack opens wherever the display camera is closer than the rendered one.
 * fr_present_reproject_from_poses (host only, f64 throughout, rounded once to fp32): vp = proj * view of
 * fr_camera_matrices(display); fallback is what fr_present_warp_from_poses gives for the same arguments, with the same
 * refusals, *rp untouched on refusal. Equal poses give the rendered camera's vp and the exact scale or identity
 * fallback. The late-reprojection recipe: `rendered` is the pose the frame was traced with, `display` the pose sampled
 * just before the present.
 * fr_present_reproject_pack states the rule on the host, without a device, through the functions the kernels run
 * (rgba, position: width * height * 4 floats each; out: the output's width * height * 4 bytes), with K in a temporary
 * of its own; FR_E_INVALID as fr_present_warp_pack with the fallback as its warp, and for a NULL position or rp or a
 * non-finite vp coefficient.
 * fr_present_reproject_enable(ctx, 1): the first call waits for the context's pending work and allocates the key
 * image, W * H * 8 bytes; it needs fr_present_enable first (FR_E_STATE otherwise); FR_E_NOMEM keeps nothing and leaves
 * the feature off. on = 0 makes the two enqueues return FR_E_STATE and frees nothing before fr_destroy. No other call
 * of the feature allocates, and a context that never calls it creates the streams and enqueues the work it always did.
 * Refused with nothing enqueued, nothing written and no ticket taken: everything the warped enqueues refuse, with their
 * codes, the fallback being checked as a warp is; a NULL rp, a non-finite vp coefficient (FR_E_INVALID); the feature or
 * the ring not enabled, or the ring full (FR_E_STATE); a rank of a group or a sharded context (FR_E_UNSUPPORTED).
 *
 * Not covered: a transfer curve or dithering; NV12 / YUV and 10-bit outputs; the G-buffer channels and EXTRA; a
 * group's composite; the ring in a snapshot; of the warp: a
 * homography latched from device memory at kernel time; edge clamping beyond half a texel and filters other than
 * bilinear; lens distortion; outputs larger than the screen; groups; of the blend: radii latched on the device from
 * the ray budget controller's r2; elliptical or per-eye zones; more than two sources; curves other than smoothstep;
 * groups; of the positional reprojection: a blended source; splats larger than one texel or bilinear weights;
 * motion-vector (moving geometry) extrapolation; a second layer behind glass (POSITION is the primary hit, so what is
 * seen through the refractive box moves with the box's surface); outputs larger than the screen; groups; the key image
 * in a snapshot. */
#define FR_PRESENT_RGBA8    0
#define FR_PRESENT_BGRA8    1
#define FR_PRESENT_TOP_DOWN 0x100   /* or-ed into the format */
#define FR_PRESENT_PENDING  1       /* fr_present_acquire, wait = 0: not there yet */
int fr_present_pack(const float* rgba, int width, int height, int format, uint8_t* out);
int fr_present_enable(fr_ctx* ctx, int slots, int format);
int fr_present_enqueue(fr_ctx* ctx, int buffer_id, uint64_t* ticket);
int fr_present_acquire(fr_ctx* ctx, uint64_t ticket, int wait, const void** host);
int fr_present_release(fr_ctx* ctx, uint64_t ticket);
int fr_present_times(fr_ctx* ctx, uint64_t ticket, float* pack_ms, float* copy_ms);
int fr_present_enqueue_device(fr_ctx* ctx, int buffer_id, void* device_dst, size_t bytes);
int fr_present_done(fr_ctx* ctx, void* stream);
typedef struct fr_present_warp { float h[9]; int out_width, out_height; } fr_present_warp;   /* 0, 0 = W, H */
int fr_present_warp_pack(const float* rgba, int width, int height, int format, const fr_present_warp* warp, uint8_t* out);
int fr_present_warp_from_poses(const fr_camera_pose* rendered, const fr_camera_pose* display, int width, int height,
                               int out_width, int out_height, float ndc_depth, fr_present_warp* warp);
int fr_present_enqueue_warped(fr_ctx* ctx, int buffer_id, const fr_present_warp* warp, uint64_t* ticket);
int fr_present_enqueue_warped_device(fr_ctx* ctx, int buffer_id, const fr_present_warp* warp, void* device_dst, size_t bytes);
typedef struct fr_present_blend {
  int inner_buffer, outer_buffer;          /* any two of SHADING, SIBSON, PULLPUSH, ATROUS; may be equal */
  float gaze[2];                           /* finite; may lie off screen */
  float inner_radius_px, outer_radius_px;  /* finite, 0 <= inner <= outer, outer * outer finite in fp32 */
} fr_present_blend;
int fr_present_blend_default(fr_ctx* ctx, fr_present_blend* blend);
int fr_present_blend_pack(const float* inner, const float* outer, int width, int height, int format,
                          const fr_present_blend* blend, const fr_present_warp* warp /* NULL: plain */, uint8_t* out);
int fr_present_enqueue_blended(fr_ctx* ctx, const fr_present_blend* blend, const fr_present_warp* warp /* NULL: plain */,
                               uint64_t* ticket);
int fr_present_enqueue_blended_device(fr_ctx* ctx, const fr_present_blend* blend, const fr_present_warp* warp,
                                      void* device_dst, size_t bytes);
typedef struct fr_present_reproject {
  float vp[16];              /* world -> display clip, row-major */
  fr_present_warp fallback;  /* where nothing lands; its out size is the output's */
} fr_present_reproject;
int fr_present_reproject_from_poses(const fr_camera_pose* rendered, const fr_camera_pose* display, int width, int height,
                                    int out_width, int out_height, float ndc_depth, fr_present_reproject* rp);
int fr_present_reproject_pack(const float* rgba, const float* position, int width, int height, int format,
                              const fr_present_reproject* rp, uint8_t* out);
int fr_present_reproject_enable(fr_ctx* ctx, int on);
int fr_present_enqueue_reprojected(fr_ctx* ctx, int buffer_id, const fr_present_reproject* rp, uint64_t* ticket);
int fr_present_enqueue_reprojected_device(fr_ctx* ctx, int buffer_id, const fr_present_reproject* rp,
                                          void* device_dst, size_t bytes);

int fr_get_stats(fr_ctx* ctx, fr_stats* stats);
int fr_reset_stats(fr_ctx* ctx);
/* JumpFlooding launches of this context, in frames and stage calls alike, whose passes were skipped because the
 * device found the seed set {alpha >= 1} of the input equal to the previous launch's: their final state is the
 * retained one, bit for bit what the passes would compute, and JFA_COLOR, JFA_COORD and Sibson follow from it as
 * from any other. Counted on the device since fr_create (modulo 2^32); the call waits for the context's pending
 * work. The first launch of a context and the first after fr_restore always run their passes, and with
 * FOVRT_JFA_REUSE=0 in the environment of fr_create every launch does. FR_E_INVALID for a NULL argument. */
int fr_jfa_reuse_count(fr_ctx* ctx, uint32_t* skipped);

/* Live timing of entry 3 inside pipelined frames (no synchronisation added): after
 * fr_kernel_timing(ctx, 1) every shading stage records HIP events on the context stream around
 * itself and around the path-trace megakernel; fr_kernel_times returns the number of stages timed
 * since and their summed milliseconds (what rocprofv3 --kernel-trace reports for k_shade_paths).
 * fr_kernel_timing(ctx, 0) stops and clears. */
typedef struct fr_stage_times {
  uint32_t frames;
  double shading_ms;      /* carry_history + k_shade_paths + k_shade_resolve, summed */
  double shade_paths_ms;  /* k_shade_paths alone, summed */
} fr_stage_times;
int fr_kernel_timing(fr_ctx* ctx, int enable);
int fr_kernel_times(fr_ctx* ctx, fr_stage_times* out);

/* Frame clock of fr_frame (no synchronisation added beyond a ring of 16 frames): after
 * fr_frame_clock(ctx, 1) every fr_frame records a HIP event where its G-buffer may start (after the
 * waits for its frame slot) and one after both of its reconstruction chains. fr_frame_clock_read
 * returns, per frame since, the latency (start -> end: the gaze the frame samples to its finished
 * Sibson and A-Trous images, on the GPU) and the interval between consecutive frames' ends (the frame
 * time a display sees), in milliseconds; *n_latency / *n_interval receive the counts (at most cap each).
 * The reference's frame time is the serial sum of its stage timers (FR/main.cpp:368-373).
 * fr_frame_clock(ctx, 0) stops and clears. */
int fr_frame_clock(fr_ctx* ctx, int enable);
int fr_frame_clock_read(fr_ctx* ctx, float* latency_ms, float* interval_ms, int cap, int* n_latency, int* n_interval);

/* Scene inspection (host copies owned by the context; valid until fr_destroy). */
typedef struct fr_scene_arrays {
  int num_tris;
  const float* pos;      /* 9 floats per triangle (p0, p1, p2) */
  const float* nrm;      /* 9 floats per triangle */
  const float* uv;       /* 6 floats per triangle */
  const int32_t* flags;  /* material | 0x100 has_normals | 0x200 has_uv */
  int num_materials;
  const int32_t* materials;  /* (type, texture) pairs: 0 diffuse, 1 reflection, 2 refraction */
  int num_textures;
  const int32_t* tex_dims;   /* (w, h) pairs */
  const float* const* tex_data;  /* RGBA32F, row 0 = bottom */
  int envmap;
  float light[15];       /* position, v1, v2, normal, emission */
  float bbox[6];         /* min, max */
  int bvh_nodes, bvh_depth;  /* four-wide nodes, levels */
  int bvh_max_stack;        /* deepest traversal stack the tree can need (<= 24) */
} fr_scene_arrays;
int fr_scene_export(fr_ctx* ctx, fr_scene_arrays* out);

/* Host-only scene construction (no device needed): the same presets fr_create builds, for
 * inspection, asset checks and CPU-side validation. */
typedef struct fr_scene fr_scene;
int fr_scene_create(const fr_config* cfg, fr_scene** out);
int fr_scene_get_arrays(fr_scene* scene, fr_scene_arrays* out);
int fr_scene_normal_groups(fr_scene* scene, int32_t* corner_vertex, size_t ncorners, int* nverts);  /* fr_normal_groups */
int fr_scene_model_count(fr_scene* scene, int* n);  /* fr_model_count */
int fr_scene_model_info(fr_scene* scene, int i, const char** name, int* first_tri, int* ntris);  /* fr_model_info */
int fr_scene_destroy(fr_scene* scene);

#ifdef __cplusplus
}
#endif
#endif /* FOVRT_H */
