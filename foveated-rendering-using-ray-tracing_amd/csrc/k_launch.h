// k_launch.h — the host entry points of the kernel files (k_*.hip): launchers, workspaces and size helpers. Included
// by the file that defines each of them and, through ctx_internal.h, by every file that calls them. A declaration
// whose types drift from its definition does not build: another return type is an error in the .hip file, other
// parameter types declare an overload that nothing defines, which the link refuses (-z defs). Parameter names are
// the definitions'; two same-typed parameters in the wrong order are still for the reader to catch (so the three
// arrays of a tree travel as one TreeArrays, below).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "fr_device.h"

namespace fr {
// k_trace.hip
// (cur_pos, prev_pos: the positions this launch traces and the ones the previous launch traced, for the motion form;
// NULL for the plain one)
void launch_gbuffer(const DevScene& sc, const FrameUniforms& U, f4* position, f4* normal, f4* depth, f4* diffuse,
                    f4* weight, uint8_t* gclass, DevStats* stats, const f3* cur_pos, const f3* prev_pos,
                    hipStream_t stream);
void launch_shade_paths(const DevScene& sc, const FrameUniforms& U, const uint32_t* active, const uint32_t* ray_count,
                        uint32_t max_active, const f4* weight, const f4* history_cache, uint32_t* chunk_ctr,
                        f4* samples, unsigned long long* help, DevStats* stats, f4* aux, uint32_t* aux_seed,
                        uint32_t chunk_refr, uint32_t xcd_bands, uint32_t handoff, int per_cu, f4* item_store,
                        hipStream_t stream);
int shade_max_blocks_per_cu();
size_t shade_item_store_f4(int per_cu);
void launch_sample_setup(const FrameUniforms& U, const uint32_t* active, const uint32_t* ray_count, uint32_t max_active,
                         const f4* weight, const f4* history_cache, const unsigned long long* hvalid, f4* aux,
                         uint32_t* aux_seed, hipStream_t stream);
void launch_shade_resolve(const FrameUniforms& U, const uint32_t* active, const uint32_t* ray_count,
                          uint32_t max_active, const f4* weight, const f4* history_cache, const f4* samples,
                          unsigned long long* help, f4* history_buffer, f4* shading, uint32_t* chunk_ctr,
                          uint32_t handoff, int per_cu, f4* radiance, hipStream_t stream);
size_t shade_counter_words();
size_t shade_fx_slots(uint32_t max_active, int spp, uint32_t handoff, int per_cu);
void launch_carry_history(const FrameUniforms& U, const uint8_t* mask, const f4* weight, const f4* history_cache,
                          f4* history_buffer, f4* shading, unsigned long long* hvalid, hipStream_t stream);
void launch_shard_pack_active(const uint32_t* active, const uint32_t* ray_count, uint32_t capacity, const f4* radiance,
                              f4* vals, uint32_t* idx, hipStream_t stream);
void launch_shard_unpack_active(const FrameUniforms& U, const f4* vals, const uint32_t* idx, uint32_t n, uint32_t npix,
                                const f4* weight, const f4* history_cache, f4* history_buffer, f4* shading,
                                hipStream_t stream);
// the history validity rings of a still-camera group: FR_VRING pixels inside each tile
void launch_vring_pack(const f4* hist, int W, int H, int T, const int32_t* tiles, int ntiles, uint32_t* out,
                       hipStream_t stream);
void launch_vring_unpack(const uint32_t* in, int W, int H, int T, const int32_t* tiles, int ntiles, f4* hist,
                         hipStream_t stream);
// fr_trace_rays: n fr_ray records against sc; kind 0 closest hit (out: n fr_ray_hit), 1 transmittance (out: n floats),
// 2 surface (out: n fr_ray_surface; two launches); masks: NULL or n words, bit k: model k of rm takes part;
// max_blocks caps the grid (0: as many blocks as are resident)
void launch_ray_queries(const DevScene& sc, const void* rays, const uint32_t* masks, uint32_t n, int kind, void* out,
                        RayQueryState* rq, const RayModels& rm, uint32_t max_blocks, hipStream_t stream);
#ifdef FR_STAMPS
void launch_trace_queries(const DevScene& sc, const f4* queries, uint32_t n, f4* hits, uint32_t* ctr,
                          hipStream_t stream, int kind);
void diag_record_queries(f4* buf, uint32_t cap, hipStream_t stream);
uint32_t diag_recorded_queries(hipStream_t stream);
void diag_sample_trace(uint32_t* srec, uint32_t scap, uint32_t* wrec, uint32_t wcap, hipStream_t stream);
#endif

// k_front.hip
void launch_sampling(const FrameUniforms& U, const DevScene& sc, const f4* position, const f4* depth,
                     const f4* depth_cache, f4* weight, const f4* normal, const f4* diffuse, f4* extra, uint8_t* mask,
                     const uint8_t* gclass, unsigned long long* words, uint32_t* counts, int write_extra,
                     uint8_t* lp_cache, uint32_t* lp_inv, bool lp_refresh, uint32_t* bcount, bool motion,
                     const float* dev_box, hipStream_t stream);
// foveation control: the eccentricity mask into lp_cache (st: the ray budget's record, whose r2 the kernel then reads;
// NULL: r2), the budget's controller ahead of it, and the copy of a caller's mask (src 16-byte aligned) into dst
void launch_ecc_mask(f2 gaze, const FovState* st, float r2, uint32_t floor_ranks, int W, int H, uint8_t* lp_cache,
                     hipStream_t stream);
void launch_fov_control(FovState* st, const uint32_t* count, bool reset, float r2_0, uint32_t budget, float tolerance,
                        float r2_max, hipStream_t stream);
void launch_mask_take(const uint8_t* src, uint8_t* dst, int W, int H, hipStream_t stream);
void launch_extra(const FrameUniforms& U, const DevScene& sc, const f4* depth, const f4* weight, const f4* normal,
                  const f4* diffuse, f4* extra, const float* dev_box, hipStream_t stream);
size_t logpolar_inv_words(int W, int H);
void launch_owner_counts(const FrameUniforms& U, const uint32_t* bcount, uint32_t* owner_counts, hipStream_t stream);
void launch_mask_words(const uint8_t* mask, const uint8_t* gclass, int W, int H, unsigned long long* words,
                       uint32_t* counts, hipStream_t stream);
void launch_compaction(int W, int H, const unsigned long long* words, const uint32_t* counts, uint32_t* local_prefix,
                       uint32_t* tile_sum, uint32_t* ray_count, uint32_t* active, hipStream_t stream);
size_t compaction_tiles(int W, int H);

// k_post.hip
void launch_shard_pack(const FrameUniforms& U, const f4* buf, f4* slab, hipStream_t stream);
void launch_shard_unpack(const FrameUniforms& U, int rank, const f4* slab, f4* buf, hipStream_t stream);
void launch_logpolar(const f4* in, f4* fwd, f4* inv, int W, int H, f2 gaze, hipStream_t stream);
void launch_composite(const f4* views, int nviews, int W, int H, f4* out, hipStream_t stream);

// k_present.hip: src (W x H RGBA32F) to W * H packed 8-bit texels at out (16-byte aligned), by present_texel
// (fr_math.h); format: FR_PRESENT_RGBA8 or FR_PRESENT_BGRA8, FR_PRESENT_TOP_DOWN or-ed in (checked by the caller)
void launch_present_pack(const f4* src, int W, int H, int format, void* out, hipStream_t stream);
// The same through a homography (present_warp_texel, fr_math.h): h[9] row-major, output texel centres to source texel
// centres, copied into the kernel's arguments by the call; 1 <= ow <= W, 1 <= oh <= H; out: ow * oh words
void launch_present_warp(const f4* src, int W, int H, int format, const float* h, int ow, int oh, void* out,
                         hipStream_t stream);
// Either of the two over the virtual image present_blend_fetch (fr_math.h) makes of two W x H sources, which may be
// one image; the blend is copied into the kernel's arguments. h NULL: the plain form (ow x oh = W x H)
void launch_present_blend(const f4* inner, const f4* outer, int W, int H, int format, const PresentBlend& blend,
                          const float* h, int ow, int oh, void* out, hipStream_t stream);
// k_present_reproject.hip: the reprojected present (present_splat_place, present_resolve_word, fr_math.h). keys: room
// for W * H 64-bit keys, of which the first ow * oh are cleared, splatted into (every texel of src whose pos lands in
// the ow x oh output under vp[16], the smallest key winning) and resolved to ow * oh words at out; h[9]: the
// homography of the places nothing reaches. vp and h are copied into the kernels' arguments. Three launches on stream.
void launch_present_reproject(const f4* src, const f4* pos, int W, int H, int format, const float* vp, const float* h,
                              int ow, int oh, unsigned long long* keys, void* out, hipStream_t stream);

// k_jfa.hip, k_sibson.hip
// A context's JumpFlooding state: G, H the passes' ping-pong, F the final state (retained while the seed set stays),
// seeds the seed bitmap of the last launch (jfa_seed_words), ctl the JFA_CTL_* words. gen: the launch's generation
// (a context counts its launches from 1); force: run the passes whatever the bitmap says.
struct JfaState {
  u2 *G, *H, *F;
  unsigned long long* seeds;
  uint32_t* ctl;
};
enum { JFA_CTL_CHANGED = 0, JFA_CTL_SKIPPED = 1, JFA_CTL_WORDS = 2 };
inline size_t jfa_seed_words(int W, int H) { return ((size_t)W * H + 63) / 64; }
const u2* launch_jfa(const f4* in, const JfaState& st, uint32_t gen, bool force, f4* coord, f4* color,
                     const float* ftab, int W, int H, f4* sibP, f4* sibT, bool outputs, int xcd, hipStream_t stream);
void launch_jfa_coord(const u2* state, const f4* color, f4* coord, int W, int H, hipStream_t stream);
void launch_sibson(const f4* coord, const f4* color, f4* out, int W, int H, hipStream_t stream);
void launch_sibson_runs(const f4* coord, const u2* state, const f4* color, f4* P, f4* T, f4* G, uint32_t* wide,
                        uint32_t* strips, f4* out, int W, int H, bool prefix_fresh, bool strip, int strip_mid,
                        bool coord_owed, hipStream_t stream);
int sibson_prefix_blocks(int W);
size_t sibson_strip_words(int W, int H);
size_t sibson_rowp_texels(int W, int H);

// k_pullpush.hip, k_atrous.hip
void launch_pullpush(const f4* in, f4* pull, f4* push, f4* snap, f4* out, int W, int H, hipStream_t stream);
bool launch_atrous(const f4* pos, const f4* nrm, const f4* col, f4* out, int W, int H, float c_phi, float n_phi,
                   float p_phi, float stepWidth, bool rows2, int xcd, hipStream_t stream);
int pp_size(int W, int H);
size_t pp_snap_count(int S);

// k_bvh.hip
// The three device arrays of one four-wide tree: nodes, and the triangles and primitive indices in leaf order. A host
// type only: kernels keep their own parameter lists (and their const).
struct TreeArrays {
  BvhNode* nodes = nullptr;
  TriGeo* tri = nullptr;
  int32_t* prim = nullptr;
};
struct BvhWork;
bool gpu_build_bvh(BvhWork** work, const f3* pos, int n, const TreeArrays& t, int* num_nodes, int* max_stack, int* depth,
                   hipStream_t s, std::string& err);
void bvh_work_free(BvhWork* w);
bool bvh_work_prepare(BvhWork** w, int n, hipStream_t s, std::string& err);
bool bvh_builder_warm(BvhWork* w, hipStream_t s, std::string& err);
bool gpu_refit_bvh(BvhWork* work, const f3* pos, int n, const TreeArrays& t, int num_nodes, hipStream_t s,
                   std::string& err);
// (nodes_dev, here and below: NULL, or the node count in device memory of a tree the host has not seen)
bool gpu_refit_bvh_enqueue(BvhWork* work, const f3* pos, int n, const TreeArrays& t, int num_nodes,
                           const uint32_t* reject, const uint32_t* nodes_dev, hipStream_t s, std::string& err);
// the refit of an enqueued update out of place: from the tree in use into another set of arrays, whole
bool gpu_refit_bvh_to_enqueue(BvhWork* work, const f3* pos, int n, const TreeArrays& src, int num_nodes,
                              const TreeArrays& dst, const uint32_t* reject, const uint32_t* nodes_dev, hipStream_t s,
                              std::string& err);
bool gpu_check_positions_enqueue(BvhWork* work, const float* xyz, int n, hipStream_t s, std::string& err);
bool gpu_take_over_positions(BvhWork* work, const f3* xyz, const f3* cur, int n, f3* dst, const uint32_t* bad_nrm,
                             GeoUpdateState* st, int flags, f3 seed_lo, f3 seed_hi, hipStream_t s, std::string& err);
bool gpu_bvh_cost(BvhWork* work, const BvhNode* nodes, int num_nodes, float* cost, hipStream_t s, std::string& err);
bool gpu_check_positions(BvhWork* work, const float* xyz, int n, bool* finite, float box[6], hipStream_t s,
                         std::string& err);

// What another builder (k_bvh_sah.hip) shares with this one: the workspace's primitive boxes (blo / bhi, one per
// triangle), the centroid bounds k_prim_boxes leaves in cb[0..5] (order-mapped min / max), and the four-wide part.
struct BvhWorkView {
  const f4 *blo, *bhi;
  const uint32_t* cb;
};
BvhWorkView bvh_work_view(BvhWork* w);
// k_build_init and k_prim_boxes over pos (no wait)
bool gpu_prim_boxes_enqueue(BvhWork* work, const f3* pos, int n, hipStream_t s, std::string& err);
// A binary tree whose leaves are marked (child[e].x < 0) and own ids[range[e].x, range[e].y): any number of
// triangles, at any depth. lo / hi: the raw box of every node.
struct MarkedTree {
  const int2* child;
  const int2* range;
  const f4 *lo, *hi;
};
// The four-wide part of gpu_build_bvh over such a tree (root: node 0, not a leaf): collapse, leaf scan, triangle
// relayout, with the same kernels. Waits for the result.
bool gpu_collapse_marked(BvhWork* work, const MarkedTree& T, const int32_t* ids, const f3* pos, int n, const TreeArrays& t,
                         int* num_nodes, int* max_stack, int* depth, hipStream_t s, std::string& err);

// A build in stream order (fr_rebuild_bvh_enqueue): where it goes (dst, n entries each, and the record of its
// numbers), the context's record of such builds, and the tree in use (src), which a build that fails on the
// device copies over the destination (src_host_nodes >= 0: the host knows its numbers, src_host_desc; else src_desc).
// conditional: the build is fr_rebuild_bvh_enqueue_if's; gpu_rebuild_decide_enqueue has left FR_REBUILD_SKIP or 0 in
// rs->fail earlier on the stream, and a skipped build runs the same schedule over an empty level 0.
struct RebuildTarget {
  RebuildState* rs;
  TreeArrays dst, src;
  TreeDesc* desc;
  int src_host_nodes;
  TreeDesc src_host_desc;
  const TreeDesc* src_desc;
  int conditional;
};
// gpu_build_bvh / gpu_collapse_marked on a fixed launch schedule: no wait, no read-back, no allocation. The verdict
// and the tree's numbers stay on the device (t.rs, t.desc). levels: the collapse launches (the binary tree's depth
// bounds them); sah_fail: the device word that says the binary tree failed.
bool gpu_rebuild_begin_enqueue(RebuildState* rs, int conditional, hipStream_t s, std::string& err);
bool gpu_build_bvh_enqueue(BvhWork* work, const f3* pos, int n, const RebuildTarget& t, hipStream_t s, std::string& err);
bool gpu_collapse_marked_enqueue(BvhWork* work, const MarkedTree& T, const int32_t* ids, const f3* pos, int n, int levels,
                                 const uint32_t* sah_fail, const RebuildTarget& t, hipStream_t s, std::string& err);
// Around a conditional build: the SAH cost of the tree in use and the decision ahead of it (num_nodes, or nodes_dev;
// the rule is beside fr_rebuild_bvh_enqueue_if in include/fovrt.h), and behind it the cost of a tree it built, which
// becomes the baseline. gpu_bvh_cost's kernels and scratch; no wait, no read-back.
bool gpu_rebuild_decide_enqueue(BvhWork* work, RebuildState* rs, const BvhNode* nodes, int num_nodes, int n,
                                const uint32_t* nodes_dev, float ratio, bool base_stale, hipStream_t s,
                                std::string& err);
bool gpu_rebuild_rebase_enqueue(BvhWork* work, const RebuildTarget& t, int n, hipStream_t s, std::string& err);

// k_bvh_sah.hip: the device binned-SAH builder (fr_config.bvh_builder = 2), whose tree is the host builder's
struct SahWork;
bool sah_work_create(SahWork** out, int n, hipStream_t s, std::string& err);
void sah_work_free(SahWork* w);
size_t sah_work_bytes(int n);
// gpu_build_bvh's contract. *unsupported: the build met a node without a finite SAH candidate (see fovrt.h)
bool gpu_build_bvh_sah(SahWork* sw, BvhWork* work, const f3* pos, int n, const TreeArrays& t, int* num_nodes,
                       int* max_stack, int* depth, bool* unsupported, hipStream_t s, std::string& err);
// the same build in stream order: all 30 levels are launched (those past the last find nothing), see RebuildTarget
bool gpu_build_bvh_sah_enqueue(SahWork* sw, BvhWork* work, const f3* pos, int n, const RebuildTarget& t, hipStream_t s,
                               std::string& err);

// k_normals.hip: shading normals over moving geometry
struct NormalsWork;
bool normals_work_create(NormalsWork** out, const int32_t* corner_vertex, const int32_t* off, const int32_t* corners,
                         int nt, int nv, hipStream_t s, std::string& err);
void normals_work_free(NormalsWork* w);
bool gpu_recompute_normals(NormalsWork* w, const f3* pos, TriShade* shade, hipStream_t s, std::string& err);
bool gpu_check_normals(NormalsWork* w, const float* nrm, bool* finite, hipStream_t s, std::string& err);
bool gpu_scatter_normals(NormalsWork* w, const float* nrm, TriShade* shade, hipStream_t s, std::string& err);
// their enqueue halves (no wait; reject, flag: the device verdict word of an enqueued update, or NULL)
bool gpu_recompute_normals_enqueue(NormalsWork* w, const f3* pos, TriShade* shade, const uint32_t* reject, hipStream_t s,
                                   std::string& err);
bool gpu_check_normals_enqueue(NormalsWork* w, const float* nrm, uint32_t* flag, hipStream_t s, std::string& err);
bool gpu_scatter_normals_enqueue(NormalsWork* w, const float* nrm, TriShade* shade, const uint32_t* reject, hipStream_t s,
                                 std::string& err);
// the normals of an enqueued update out of place: src's records into dst with the given normals (nrm), the
// recomputed ones (pos), or src's own (both NULL)
bool gpu_normals_to_enqueue(NormalsWork* w, const float* nrm, const f3* pos, const TriShade* src, TriShade* dst,
                            const uint32_t* reject, hipStream_t s, std::string& err);

// k_pose.hip, model poses: a pose's kernel arguments (NULL, or why the pose is refused), the launch that writes the
// posed rest arrays into the staging arrays, the capture of the rest arrays, and the bytes of one such array
const char* pose_args(PoseArgs* a, const float* m, int nmodels, const int* first_tri);
bool gpu_pose_enqueue(const PoseArgs& a, const f3* rest_pos, const f3* rest_nrm, f3* out_pos, f3* out_nrm, int nt,
                      hipStream_t s, std::string& err);
bool gpu_pose_capture_enqueue(const f3* pos, const TriShade* shade, f3* rest_pos, f3* rest_nrm, int nt, hipStream_t s,
                              std::string& err);
size_t pose_array_bytes(int nt);

// k_visibility.hip, per-model visibility: a mask's kernel arguments, and the launch that writes the collapsed
// positions (pos with every triangle of a hidden model collapsed onto its first corner) into out, an array of
// pose_array_bytes(nt)
HideArgs hide_args(const int* first_tri, int nmodels, int nt, uint32_t visible);
bool gpu_hide_enqueue(const HideArgs& a, const f3* pos, f3* out, int nt, hipStream_t s, std::string& err);
}  // namespace fr
