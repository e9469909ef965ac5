// ctx_internal.h — the fr_ctx context (device memory, streams, frame slots) and the helpers shared by the C ABI in
// ctx_*.cpp (one file per concern) and the multi-GPU group in group.cpp. Not part of the public
// interface (include/fovrt.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/fovrt.h"
#include "fr_device.h"
#include "k_launch.h"
#include "present_ring.h"
#include "scene.h"

#define FR_MAX_SHARD_RANKS 64  // ranks per view (an owner is one byte of the tile map)

using fr::f2;
using fr::f3;
using fr::u2;
using fr::f4;
using fr::BvhNode;
using fr::TriGeo;
using fr::TriShade;
using fr::DevMaterial;
using fr::DevTexture;
using fr::DevScene;
using fr::DevStats;
using fr::FrameUniforms;
using fr::HostScene;
using fr::Bvh;

enum Phys {
  P_POSITION, P_NORMAL, P_DEPTH_A, P_DEPTH_B, P_DIFFUSE, P_WEIGHT, P_HIST_A, P_HIST_B, P_SHADING, P_EXTRA,
  P_JFA_COORD, P_JFA_COLOR, P_SIBSON, P_PULLPUSH, P_ATROUS_A, P_ATROUS_B, P_LOGPOLAR, P_LOGPOLAR_INV,
  // frame-slot copies of the buffers the reconstruction reads (POSITION, NORMAL, SHADING) and of
  // WEIGHT (read by the trace half's tail); slot 0 is the plain entry above
  P_POSITION_B, P_NORMAL_B, P_SHADING_B, P_WEIGHT_B,
  P_POSITION_C, P_NORMAL_C, P_SHADING_C, P_WEIGHT_C,
  P_COUNT
};

// An event with the flag that says a record of it may still be in flight. The owner creates and destroys `ev`
// (hipEventDisableTiming); a reader that needs the event whatever the flag (a host poll, a query) takes `ev`.
struct Fence {
  hipEvent_t ev = nullptr;
  bool pending = false;
  hipError_t record(hipStream_t s) { pending = true; return hipEventRecord(ev, s); }
  // s waits for the last record, if one is pending; the flag is cleared (consume: the next waiter has nothing to
  // wait for) or kept (peek: others still wait for the same record)
  hipError_t consume(hipStream_t s) {
    const hipError_t e = peek(s);
    pending = false;
    return e;
  }
  hipError_t peek(hipStream_t s) const { return pending ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
};

struct fr_ctx {
  fr_config cfg;
  std::string asset_dir;
  std::string err;
  int W = 0, H = 0;
  // The five streams, in creation order (all non-blocking, priority 0; a context that presents makes a sixth,
  // present.stream below). DESIGN.md §5 has the table of who records and who waits for each fence and ordering event.
  hipStream_t stream = nullptr;         // the context stream: entry 3, stage calls, updates
  hipStream_t atrous_stream = nullptr;  // reconstruction chain 2: pull-push -> A-Trous
  hipStream_t sibson_stream = nullptr;  // reconstruction chain 1: JFA -> Sibson
  hipStream_t carry_stream = nullptr;   // entry 3's carry of the inactive pixels, beside the megakernel
  // front stages of a pipelined frame (entries 0-2), beside the previous megakernel; overlapped updates between them
  hipStream_t front_stream = nullptr;
  // Invariant for front_stream: its front stages wait only for the slot fences (recon_done, trace_done), not for
  // earlier work on `stream`, although they overwrite shared buffers (gclass, DIFFUSE, EXTRA, depth,
  // ballots, counts, lp_cache). So every ABI call that enqueues on `stream` outside a pipelined frame
  // goes through join_recon, which sets stream_dirty, and the next pipelined frame's front stages then
  // wait for `stream` once (frame_half, ev_stream_join). fr_update_geometry_enqueue sets stream_dirty itself without
  // joining the reconstruction: its kernels touch positions, tree and normals, which only the trace half reads.

  // Frame pipelining: frame N's reconstruction (sibson_stream + atrous_stream) runs while later frames trace.
  // The buffers the reconstruction reads (POSITION, NORMAL, SHADING) rotate over `nslots` frame
  // slots (`slot` = the current frame's); a frame's front stages wait for the reconstruction that
  // last read their slot (recon_done). The front stages of a pipelined frame (G-buffer, sampling,
  // compaction) run on front_stream while the previous frame's megakernel still runs on `stream`: they
  // read nothing entry 3 writes. What entry 3's tail reads of them (WEIGHT, mask, active list, ray
  // count) rotates with the slot as well; the front of a frame waits for the trace half that last
  // read its slot (trace_done), and entry 3 of a frame waits for its own front (front_done).
  static constexpr int MAX_SLOTS = 3;
  int nslots = 3;
  int slot = 0;
  Fence front_done;             // front stream, after a pipelined frame's front stages
  Fence trace_done[MAX_SLOTS];  // context stream, after the last reader of the slot's WEIGHT / mask / active list
  Fence recon_done[MAX_SLOTS];  // sibson_stream, after both chains of the slot's reconstruction
  // latency mode: the end of the slot's JumpFlooding (sibson_stream; the host polls it, or trace_done when the chain
  // is not run here)
  Fence jfa_done[MAX_SLOTS];
  // Ordering inside a frame: plain events, each recorded and waited for unconditionally at one place (ctx_frame.cpp).
  hipEvent_t ev_carry_fork = nullptr;   // `stream` records before entry 3's kernels; carry_stream waits
  // carry_stream records after k_carry_history; `stream` waits before the resolve. Across frames: the front stream of
  // the NEXT frame waits for it before its early sample setup (latency mode), which reads the carry's validity bits.
  hipEvent_t ev_carry_done = nullptr;
  hipEvent_t ev_recon_fork = nullptr;   // `stream` records after the trace half; sibson_stream and atrous_stream wait
  hipEvent_t ev_chain2_done = nullptr;  // atrous_stream records after A-Trous; sibson_stream waits, then records recon_done
  // `stream` records, the front stream waits, when stream_dirty: something was enqueued on `stream` outside a
  // pipelined frame since the last one (the invariant above; no event of its own, so a plain flag)
  hipEvent_t ev_stream_join = nullptr;
  bool stream_dirty = true;
  // Stage timing of a timed frame (fr_frame_timing): each event ends the stage it is named after, on the stream that
  // ran it (`stream`; the chain events on their chain's stream). A timed frame records all of them, so untimed
  // frames never read them. stage_begin / stage_end: the pair around one stage call (timed()).
  struct StageEvents {
    hipEvent_t begin, geometry, sampling, optimize, shading, end;
    hipEvent_t paths_begin, paths_end;          // around k_shade_paths alone
    hipEvent_t chain2_begin, pullpush, atrous;  // atrous_stream
    hipEvent_t chain1_begin, jfa, sibson;       // sibson_stream
    hipEvent_t stage_begin, stage_end;
  } tev = {};
  // Latency mode's schedule (wait_for_previous_frame, ctx_frame.cpp): per slot, timing events at the front stages'
  // start and end, the JumpFlooding's end and the reconstruction's end (rec: all four were recorded, arm: this frame
  // records them); the last completed frame's front and Sibson (JFA end -> end) times.
  struct LatSchedule {
    struct { hipEvent_t front_begin, front_end, jfa_end, recon_end; } ev[MAX_SLOTS] = {};
    bool rec[MAX_SLOTS] = {}, arm = false;
    float front_ms = 0.0f, sib_ms = 0.0f;
    float front_hist[8] = {};  // the last frames' front-stage spans: their minimum is the uncontended one
    int front_n = 0;
  } lat;
  // Tile sharding (fr_set_shard_plan): tile -> (owner << 24 | index among the owner's tiles) on the
  // device (FrameUniforms::shard_map), and the owners on the host. With sharding on, the front stages
  // also count every rank's active pixels from the unfolded mask (bcount per 16x16 block ->
  // owner_counts_p[slot]) and copy them to pinned host memory (h_counts, ev_counts[slot]): a group
  // sizes its transfers from them without a collective (every rank computes the same full mask).
  uint32_t* shard_map = nullptr;
  f4* shade_radiance = nullptr;    // a sharded rank's traced pixels' (tone-mapped radiance, 1), active order
  std::vector<uint8_t> shard_owner;
  uint32_t* bcount = nullptr;
  uint32_t* owner_counts_p[MAX_SLOTS] = {};
  uint32_t* h_counts = nullptr;  // MAX_SLOTS x FR_MAX_SHARD_RANKS, pinned
  hipEvent_t ev_counts[MAX_SLOTS] = {};
  bool counts_valid[MAX_SLOTS] = {};  // a front stage under the current plan recorded ev_counts[slot]
  // Tile-local front stages (fr_set_front_local): per 8x8 pixel tile, does this rank's sampling read
  // it (front_need, device; FrameUniforms::front_need while on); front_need_px = their pixel count.
  bool front_local = false;
  uint8_t* front_need = nullptr;
  std::vector<uint8_t> front_need_h;
  uint32_t front_need_px = 0;
  int pipeline_mode = 0;            // FR_PIPELINE_THROUGHPUT / FR_PIPELINE_LATENCY (fr_set_pipeline_mode)
  int recon_chains = 3;             // reconstruction chains this context runs: 1 JFA -> Sibson, 2 pull-push -> A-Trous
  hipEvent_t recon_gate = nullptr;  // when set, chain 2 (pull-push -> A-Trous) waits for it (a group's
                                    // composite reads the last A-Trous image)
  uint8_t* mask_p[MAX_SLOTS] = {};
  uint32_t* active_p[MAX_SLOTS] = {};
  uint32_t* ray_count_p[MAX_SLOTS] = {};
  HostScene scene;
  Bvh bvh;
  // device scene: the tree in use, and the GPU builder's target arrays (adopt_spare swaps the two after a successful
  // build; tree_alloc / tree_free make and release either)
  fr::TreeArrays tree, spare;
  bool tree_full_cap = false;  // `tree` holds one entry per triangle (a device-built tree)
  f3* d_pos = nullptr;  // world-space vertices, 3 per triangle (the GPU builder's input)
  // fr_update_positions writes new positions here and swaps with d_pos once the update succeeded: the old
  // positions survive a failed rebuild on the device, without the host mirror
  f3* spare_pos = nullptr;
  // Motion reprojection (fr_set_motion_reprojection). prev_pos: the positions the most recent G-buffer launch traced
  // (allocated at the first on = 1; undefined while !moved, when d_pos are those positions). moved: d_pos changed
  // since that launch; the next G-buffer runs its motion form over (d_pos, prev_pos) and clears it. An update with
  // moved clear rotates d_pos -> prev_pos -> spare_pos -> d_pos instead of swapping d_pos and spare_pos, so spare_pos
  // stays free between updates and nothing is copied. motion_frame: the last G-buffer ran the motion form and left
  // a distance in WEIGHT.z for the sampling launch that follows it (which clears it).
  f3* prev_pos = nullptr;
  bool motion_on = false, moved = false, motion_frame = false;
  // scene.pos (the host mirror of d_pos) is behind: positions came from device memory and were not copied
  // back. fr_scene_export refreshes it; nothing else reads it.
  bool pos_mirror_stale = false;
  // Enqueued updates (fr_update_geometry_enqueue). geo: their record on the device (verdict, counters, the scene
  // box), made by fr_create; h_geo: its pinned copy for fr_geometry_update_status. Once a context has enqueued an
  // update the box lives in geo->box (dev_box points there, the saliency stage reads it; extra.box: the box an owed
  // EXTRA's sampling launch saw, geo->box or geo->xbox) and scene.bbox_min / bbox_max may be behind
  // (box_mirror_stale; fr_scene_export fetches it). geo_read: recorded on the context
  // stream after the last kernel that reads the caller's arrays of the last enqueued update; the caller's stream
  // waits for it (fr_geometry_consumed; never consumed: any number of streams may ask).
  // geo_rejected_seen: the rejected counts fr_geometry_update_status last reported (total, positions, normals).
  fr::GeoUpdateState* geo = nullptr;
  fr::GeoUpdateState* h_geo = nullptr;
  const float* dev_box = nullptr;
  Fence geo_read;
  bool box_mirror_stale = false;
  unsigned long long geo_rejected_seen[3] = {};
  // Enqueued rebuilds (fr_rebuild_bvh_enqueue). rb: their record on the device (verdict, counters, the numbers of
  // the two trees, the collapse's level counters), made by fr_create; h_rb: its pinned copy for fr_bvh_rebuild_status
  // and tree_numbers. tree_on_device: the tree in use was built by an enqueued rebuild the host has not looked at
  // since: its node count, stack need and depth are rb->tree[desc_cur], and bvh.gpu_nodes / max_stack / max_depth are
  // behind (beside pos_mirror_stale / box_mirror_stale: tree_numbers refreshes them, after a wait, for every host
  // reader; enqueued refits take the count from the device meanwhile). rb_failed_seen: the failed counts
  // fr_bvh_rebuild_status last reported (total, SAH, stack, collapse).
  fr::RebuildState* rb = nullptr;
  fr::RebuildState* h_rb = nullptr;
  bool tree_on_device = false;
  int desc_cur = 0;
  unsigned long long rb_failed_seen[4] = {};
  // Conditional rebuilds (fr_rebuild_bvh_enqueue_if). base_stale: rb->base_cost is not the cost of the tree in use when
  // it was built or adopted, because that tree came by another route (fr_create, gpu_rebuild, the unconditional
  // enqueued rebuild); the next conditional call hands the flag to its deciding kernel, which adopts the tree's cost.
  // The policy (fr_set_rebuild_policy): after every policy_period-th update or pose accepted by the enqueue calls
  // (policy_count, since the policy was set) the context makes the conditional call itself; period 0: off.
  bool base_stale = true;
  float policy_ratio = 0.0f;
  int policy_period = 0;
  int policy_count = 0;
  // Model poses (fr_model_pose_enable, fr_set_model_transforms). Four arrays of 9 floats per triangle, made by the
  // first enable: the rest geometry a pose is relative to (positions, and d_shade's normals expanded) and the
  // staging arrays k_pose writes and the update path then reads as a caller's device arrays. All four are read
  // and written on the context stream only. pose_m: the pose last submitted, 12 floats per model.
  f3 *pose_rest_pos = nullptr, *pose_rest_nrm = nullptr, *pose_stage_pos = nullptr, *pose_stage_nrm = nullptr;
  bool pose_on = false;
  std::vector<float> pose_m;
  // Per-model visibility (fr_model_visibility_enable, fr_set_model_visibility). vis_mask: the mask last submitted,
  // valid bits only for a context that has submitted one (FR_VISIBLE_ALL before). While a model is hidden every tree
  // writer reads vis_pos, the collapsed copy k_hide makes of the positions it was handed (tree_positions,
  // ctx_geometry.cpp), on the writer's own stream; with every model visible nothing reads or writes it. One array of
  // 36 B per triangle, made by the first enable (the ordering argument: above GeoEnqueue).
  f3* vis_pos = nullptr;
  bool vis_on = false;
  uint32_t vis_mask = FR_VISIBLE_ALL;
  // Overlapped updates (fr_set_geometry_overlap). While overlap_on, an enqueued update runs on front_stream and writes
  // the set no frame in flight reads: the spare tree arrays above and shade_back (made by the first on = 1, a copy of
  // d_shade), which then become the scene's (adopt_spare: a swap with `tree` and d_shade and a refresh of dsc;
  // frames already enqueued keep the dsc they were given). set_cur: which of the two sets is the scene's.
  // set_read[i]: recorded on the context stream after the last reader of set i there (entry 3; a G-buffer on the
  // context stream); front_stream waits for the other set's before the update's first write. update_done: recorded on
  // front_stream after the update's last kernel; the context stream waits for it before anything it runs outside a
  // pipelined frame (join_update, in join_recon), and a pipelined frame's front stages follow it on front_stream.
  bool overlap_on = false;
  TriShade* shade_back = nullptr;
  int set_cur = 0;
  Fence set_read[2];
  Fence update_done;
  // Ray queries (fr_trace_rays, ctx_query.cpp). rq: their record on the device (the chunk counter of k_ray_queries),
  // made by fr_create and zeroed in stream order ahead of every launch. rq_area: the staging area of host batches,
  // rq_bytes bytes (fr_ray_query_reserve: 48 B per ray; fr_ray_query_reserve_kind: 32 B, the kind's result and 4 B of
  // mask), laid out per call as rays, results, masks; rq_cap = rq_bytes / 48, the rays fr_ray_query_reserve's callers
  // were promised. rays_done: recorded on the context stream after the last enqueued query's kernel; the caller's
  // stream waits for it (fr_rays_consumed; never consumed: any number of streams may ask). rayq_blocks:
  // FOVRT_RAYQ_BLOCKS, a cap on the grid, 0 = none.
  fr::RayQueryState* rq = nullptr;
  void* rq_area = nullptr;
  size_t rq_bytes = 0;
  size_t rq_cap = 0;
  Fence rays_done;
  uint32_t rayq_blocks = 0;
  // Present (fr_present_enable, ctx_present.cpp): 8-bit frames to the host in stream order. Everything here is made by
  // the first enable and stays null on a context that never presents: present.stream, the sixth stream, runs the pack
  // kernel and the copy to the host and nothing else; per ring slot a device staging image, a pinned host image and
  // three timed events on that stream (begin: before the pack, packed: after it, done: after the copy; done is the
  // one fr_present_acquire waits for); ev_fork: the context stream records, the present stream waits (what a present
  // sees). ring: tickets and slot states, no HIP in it. made: slots that have their two images. keys: the W x H 64-bit
  // key image of the reprojected present (fr_present_reproject_enable makes it; null until then), used by the present
  // stream alone; reproject: those presents are on.
  // The fences of the other direction, recorded on the present stream after a pack and only ever peeked (several
  // streams wait for one record; fr_synchronize clears them): present_read after a pack of SIBSON, PULLPUSH or an
  // A-Trous image, for the next writers of those (sibson_stream and atrous_stream at a frame's fork, the context stream
  // in join_recon); present_read_shd[slot] after a pack of that slot's SHADING, for the front stages of the frame that
  // takes the slot next (entry 3 follows them) and join_recon; present_dev after a pack into the caller's memory, for
  // fr_present_done.
  struct Present {
    hipStream_t stream = nullptr;
    hipEvent_t ev_fork = nullptr;
    int format = 0;
    int made = 0;
    unsigned long long* keys = nullptr;
    bool reproject = false;
    fr::PresentRing ring;
    void* stage[fr::PresentRing::MAX_SLOTS] = {};
    void* host[fr::PresentRing::MAX_SLOTS] = {};
    struct { hipEvent_t begin, packed, done; } ev[fr::PresentRing::MAX_SLOTS] = {};
  } present;
  Fence present_read, present_read_shd[MAX_SLOTS], present_dev;
  int group_refs = 0;  // fr_group objects this context is a rank of (they update it through the synchronous calls)
  fr::BvhWork* bvh_work = nullptr;
  fr::SahWork* sah_work = nullptr;  // the device SAH builder's scratch (k_bvh_sah.hip): bvh_builder 2 contexts only
  // the smooth-vertex weld of the scene as fr_create built it (host), and on the device with the scratch of
  // a normal recompute (k_normals.hip); fixed for the life of the context
  fr::NormalGroups groups;
  fr::NormalsWork* nrm_work = nullptr;
  // scene.nrm (the host mirror of d_shade's normals) is behind: normals were written on the device.
  // fr_scene_export refreshes it; nothing else reads it.
  bool nrm_mirror_stale = false;
  TriShade* d_shade = nullptr;
  std::vector<void*> d_tex;
  bool tex_packing = true;  // textures in their densest exact storage (pack_texture); FOVRT_TEX_PACKING=0: RGBA32F
  bool sib_strip = true;    // Sibson's big discs by k_sibson_strip (default; FOVRT_SIB_STRIP=0: k_sibson_wide)
  DevMaterial* d_mats = nullptr;
  DevTexture* d_texs = nullptr;
  DevScene dsc;
  // image buffers
  f4* img[P_COUNT] = {};
  int depth_cur = P_DEPTH_A, depth_cache = P_DEPTH_B;
  int hist_cur = P_HIST_A, hist_cache = P_HIST_B;
  int atrous_out = P_ATROUS_A;
  uint8_t* mask = nullptr;  // mask_p[slot]
  uint8_t* gclass = nullptr;
  uint8_t* lp_cache = nullptr;  // log-polar mask for (lp_gaze, lp_mode); recomputed when either changes
  uint32_t* lp_inv = nullptr;   // the inverse log-polar map of every (u, v) of that gaze (k_logpolar_inv)
  f2 lp_gaze{-1e30f, -1e30f};
  int lp_mode = -1;
  // Foveation control (ctx_foveation.cpp). fov: the eccentricity mask's parameters (fr_set_foveation), fov_r2 their
  // squared radius; the mask shares lp_cache with the log-polar modes and fov_dirty says the parameters changed since it
  // was generated. The ray budget: fov_st its record on the device (made by fr_create; h_fov the pinned copy for
  // fr_foveation_status), fov_reset: the next mode-5 sampling launch starts the controller from fov_r2; fov_count: the
  // ray count of the compaction that followed the last sampling launch (NULL: none since); fov_on_device: the last
  // mode-5 launch took its r2 from fov_st (else fov_used_r2 is what it used).
  fr_foveation fov = {};
  float fov_r2 = 0.0f, fov_used_r2 = 0.0f;
  bool fov_dirty = true, fov_reset = true, fov_on_device = false;
  fr::FovState* fov_st = nullptr;
  fr::FovState* h_fov = nullptr;
  const uint32_t* fov_count = nullptr;
  // A caller's sampling mask (FR_MASK_CALLER). cmask: the context's 0 / 1 copy, W x H bytes, made by the first
  // fr_sampling_mask_enable(1); cmask_set: a mask was submitted. An enqueued copy runs on front_stream, ahead of the
  // next frame's front stages: mask_taken is recorded there after it (the context stream waits for it before anything
  // it runs outside a pipelined frame: join_update), and mask_read too, for the caller's stream
  // (fr_sampling_mask_consumed; never consumed).
  uint8_t* cmask = nullptr;
  bool cmask_on = false, cmask_set = false;
  Fence mask_taken, mask_read;
  unsigned long long* words = nullptr;
  uint32_t* counts = nullptr;
  uint32_t* offsets = nullptr;  // per (class, block) local prefix
  uint32_t* tiles = nullptr;
  uint32_t* ray_count = nullptr;  // ray_count_p[slot]
  uint32_t* active = nullptr;     // active_p[slot]
  uint32_t* shade_ctr = nullptr;  // sharded chunk counters of the shading work queue
  f4* samples = nullptr;          // one radiance value per (active pixel, camera sample): 16 B, or 32 B fixed point
  unsigned long long* sample_help = nullptr;  // fixed-point shares of the lanes that took over items, 32 B per sample
  f4* item_store = nullptr;     // the megakernel's refraction item stacks (shade_item_store_f4)
  f4* aux = nullptr;              // per active pixel: NDC position, r1, r2 (k_sample_setup): aux_p[aux_i]
  uint32_t* aux_seed = nullptr;   // per active pixel: the seed after the two draws: aux_seed_p[aux_i]
  // Early sample setup (frame_half, latency mode): a frame's k_sample_setup runs on the front stream right after its
  // compaction, into the other of two aux buffers, from the history validity bits (hvalid, one per pixel) the previous
  // frame's k_carry_history computed. hvalid_fresh: those bits describe HISTORY_CACHE as the next frame will read it
  // (cleared by anything else that writes the history).
  f4* aux_p[2] = {};
  uint32_t* aux_seed_p[2] = {};
  int aux_i = 0;
  unsigned long long* hvalid = nullptr;
  bool hvalid_fresh = false;
  bool setup_early = false;  // this frame's setup was enqueued by its front stages
  bool early_setup = true;   // FOVRT_EARLY_SETUP=0: every setup on the context stream before its megakernel
  // JFA state (seed coord texel + alpha flags): the passes' ping-pong G / H, the final state F, the seed bitmap and
  // the control words (k_jfa.hip). jfa_gen: launches so far; jfa_force: the next launch runs its passes whatever the
  // bitmap says (the first one, the one after fr_restore, one after a failed launch); jfa_reuse: FOVRT_JFA_REUSE=0
  // forces every launch.
  fr::JfaState jfa = {};
  uint32_t jfa_gen = 0;
  bool jfa_force = true;
  bool jfa_reuse = true;
  uint32_t chunk_refr = 0;  // fixed refraction-class chunk of the megakernel (FOVRT_SHADE_CHUNK_REFR), 0 adaptive
  uint32_t xcd_bands = 1;   // megakernel queue: per-XCD class bands (FOVRT_SHADE_XCD_BANDS=0: interleaved chunks)
  uint32_t handoff = 1;     // megakernel tail handoff (FOVRT_SHADE_HANDOFF): 0 never, 1 small launches, 2 always
  int shade_blocks_per_cu = 0;  // resident megakernel blocks per CU (FOVRT_SHADE_BLOCKS_PER_CU; default and most:
                                // shade_max_blocks_per_cu; fewer leave room for concurrent kernels)
  int jfa_xcd = 1;             // JFA steps in XCD-contiguous runs of the block order (FOVRT_JFA_XCD=0: round robin)
  int sib_strip_mid = 0;       // FOVRT_SIB_STRIP_MID=1: the mid-size wide discs go to k_sibson_strip too (helps
                               // 45-90 degree gazes, costs the centred one)
  bool atrous_rows2 = true;    // the stepWidth-1 A-Trous pass by k_atrous_rows2 (FOVRT_ATROUS_ROWS2=0: k_atrous)
  int atrous_xcd = 1;          // k_atrous_rows2's blocks in XCD-contiguous runs (FOVRT_ATROUS_XCD=0: round robin)
  float* ftab = nullptr;  // texel-centre coordinates ((x + 0.5) / W, x < W; then (y + 0.5) / H)
  f4 *pull = nullptr, *push = nullptr, *snap = nullptr;
  f4 *sib_prefix = nullptr, *sib_blocks = nullptr;  // Sibson run form: per-row block prefix sums + block totals
  uint32_t* sib_wide = nullptr;  // Sibson run form: wide-disc pixel lists (two counts, then W*H indices)
  uint32_t* sib_strips = nullptr;  // Sibson run form: k_sibson_strip's strip list and flags (sibson_strip_words)
  f4* sib_rowp = nullptr;          // Sibson strip kernel: whole-row prefix sums (sibson_rowp_texels)
  // the last JFA wrote them with JFA_COLOR. Set by enqueue_jfa alone and cleared by retire_sibson_prefix alone (when
  // JFA_COLOR / JFA_COORD are written or handed out, fr_get_buffer, and by fr_restore), which writes an owed JFA_COORD
  // first: Sibson reads its seeds from JFA_COORD whenever this is clear, so !sib_prefix_fresh implies !jfa_coord_owed
  bool sib_prefix_fresh = false;
  const u2* jfa_final = nullptr;  // that JFA's final state (the seeds k_sibson_runs reads while the prefix is fresh)
  // JumpFlooding leaves JFA_COORD unwritten (the run form reads the seeds from jfa_final): while jfa_coord_owed,
  // materialize_jfa writes it (k_jfa_coord, from jfa_final and JFA_COLOR) before anything reads it or writes JFA_COLOR.
  bool jfa_coord_owed = false;
  bool lazy_jfa_outputs = true;  // FOVRT_JFA_LAZY_OUTPUTS=0: every JumpFlooding writes JFA_COORD
  // k_sampling leaves the EXTRA heat map unwritten (nothing in a frame reads it): while extra.owed, extra.settle
  // writes it (k_extra) from what the owing launch saw, before anything reads EXTRA or overwrites one of those inputs
  // outside a frame: the launch's uniforms and scene (gaze, screen, bbox: copies, so later setters do not reach them),
  // DIFFUSE, and the physical buffers that were its DEPTH (the ping-pong swaps in enqueue_shading), NORMAL and WEIGHT
  // (its slot's; the sampling leaves WEIGHT.xy as they were). The next sampling replaces the debt. Inside a frame
  // nothing settles it: no caller can see EXTRA between a frame's G-buffer and its sampling. (ctx_frame.cpp)
  struct ExtraDebt {
    bool owed = false;
    FrameUniforms U;
    DevScene sc;
    const float* box = nullptr;  // the scene box the launch saw: dev_box then (NULL, geo->box), or geo->xbox
    int depth = P_DEPTH_A, nrm = P_NORMAL, wgt = P_WEIGHT;
    void record(const fr_ctx* c);  // what the sampling launch being enqueued sees
    bool reads(int phys) const;    // does the owed heat map read this physical buffer?
    void settle(fr_ctx* c);  // writes it: on the context stream, after the pending reconstruction and front stages
  } extra;
  bool extra_lazy = true;  // FOVRT_EXTRA_LAZY=0: every sampling writes EXTRA; also after fr_get_buffer(EXTRA) gave a view
  int pp_S = 0;
  DevStats* stats = nullptr;
  FrameUniforms U;
  uint32_t accum = 0;
  bool light_pending = false;
  bool compacted = false;
  bool mask_dirty = false;
  bool time_kernels = false;  // fr_frame with timing: also time the path-trace kernel alone
  // Live timing of entry 3 inside pipelined (untimed) frames: a ring of event quadruples recorded on
  // the context stream around carry_history / k_shade_paths / resolve (fr_kernel_timing); a slot is
  // harvested (its elapsed times summed) before it is reused and by fr_kernel_times.
  static constexpr int KT_RING = 32;
  hipEvent_t kt_ev[KT_RING][4] = {};
  bool kt_on = false;
  int kt_next = 0, kt_pending = 0;
  uint32_t kt_frames = 0;
  double kt_stage_ms = 0.0, kt_kernel_ms = 0.0;
  // Frame clock of pipelined frames (fr_frame_clock): per frame, an event where its G-buffer may start
  // (on the front stream, after the slot waits) and one after both reconstruction chains (sibson_stream).
  // latency = start -> end of one frame (gaze sample to finished image on the GPU), interval = end of
  // the previous frame -> end of this one. Harvested like kt_ev.
  static constexpr int FC_RING = 16;
  hipEvent_t fc_ev[FC_RING][2] = {};
  bool fc_on = false;
  int fc_next = 0, fc_pending = 0;
  hipEvent_t fc_ref = nullptr;  // recorded when the clock is enabled: every time is read against it
  double fc_prev_end = -1.0;    // the previous harvested frame's end (ms after fc_ref)
  int fc_cur = -1;              // the ring entry of the frame being enqueued
  bool fc_arm = false;          // frame_half: this enqueue_geometry starts a whole frame
  std::vector<float> fc_latency, fc_interval;
  // scene export copies
  std::vector<const float*> tex_ptrs;
  std::vector<int32_t> tex_dims, mat_pairs;
};

// Helpers shared by the ctx_*.cpp files and group.cpp (same semantics as the ABI calls they back). What a frame calls
// (frame_half and below) is defined in ctx_frame.cpp, so the per-frame host path stays in one translation unit.
namespace fri {
int fail(fr_ctx* c, int code, const std::string& msg);  // sets the error text (of fr_create when c is NULL)
int check_launch(fr_ctx* c);
// The context stream waits for every reconstruction still in flight (before any call that reads or
// writes what the reconstruction uses, or hands buffers to the caller). Calls join_update.
void join_recon(fr_ctx* c);
// The context stream waits for an overlapped update still in flight on front_stream (fr_set_geometry_overlap): it
// shares the update scratch, the staging arrays and geo with everything the context stream runs outside a frame.
void join_update(fr_ctx* c);
int quiesce(fr_ctx* c);  // join_recon, then the host waits for the context stream
// one frame half on the context; trace / recon as fr_trace_frame / fr_reconstruct_frame (recon runs the
// chains in c->recon_chains)
int frame_half(fr_ctx* c, fr_frame_timing* t, bool trace, bool recon);
int enqueue_shading(fr_ctx* c);  // entry 3 alone (the FR_STAMPS probes launch it)
int P_pos(const fr_ctx* c), P_shd(const fr_ctx* c), P_wgt(const fr_ctx* c);  // this frame slot's physical images
int resolve(fr_ctx* c, int id, int* phys);  // buffer id -> physical image, with the lazy outputs it names written
// Sibson's retained seeds and row prefix sums no longer describe the JFA outputs: clears sib_prefix_fresh, after
// writing a JFA_COORD that is still owed (every caller clears the flag through this)
void retire_sibson_prefix(fr_ctx* c);
void kt_harvest(fr_ctx* c, int i), fc_harvest(fr_ctx* c, int i);  // one ring entry of fr_kernel_timing / fr_frame_clock
// `waiter` waits for everything enqueued on the context stream so far (ev_stream_join). The caller keeps stream_dirty.
void stream_join(fr_ctx* c, hipStream_t waiter);
// While overlap_on: the context stream has just enqueued the last reader there of the scene's tree and normals.
inline hipError_t mark_set_read(fr_ctx* c) {
  return c->overlap_on ? c->set_read[c->set_cur].record(c->stream) : hipSuccess;
}
int gpu_rebuild(fr_ctx* c, const f3* pos);  // ctx_geometry.cpp
// The arrays of one tree (ctx_geometry.cpp), all or nothing: on failure what was made is freed, *t stays null and
// the sticky HIP error is cleared. tree_free releases them and nulls *t.
bool tree_alloc(fr::TreeArrays* t, size_t node_cap, size_t tri_cap);
void tree_free(fr::TreeArrays* t);
// The spare tree arrays become the scene's and the scene's the spare; with_shade: the shading records (d_shade /
// shade_back) and set_cur go with them. dsc's four pointers then name the scene's. (ctx_geometry.cpp)
void adopt_spare(fr_ctx* c, bool with_shade);
inline void point_dsc(fr_ctx* c) {  // dsc's pointers to the tree and the shading records in use
  c->dsc.nodes = c->tree.nodes; c->dsc.tri_geo = c->tree.tri; c->dsc.tri_prim = c->tree.prim; c->dsc.shade = c->d_shade;
}
inline int tree_nodes(const Bvh& b) {
  return b.gpu_nodes >= 0 ? b.gpu_nodes : b.host_nodes ? b.host_nodes : (int)b.nodes.size();
}
// Model i of the scene: the contiguous triangle range add_mesh recorded (ctx_scene.cpp). FR_E_INVALID: no such model.
int model_info(const HostScene& s, int i, const char** name, int* first_tri, int* ntris);
void box_of(const f3* v, size_t n, f3* lo, f3* hi);  // the box of n points (ctx_scene.cpp)
// The host's numbers of the tree in use (bvh.gpu_nodes / max_stack / max_depth) made current: while tree_on_device
// they are fetched from the device, behind the context's pending work (a wait). Every host reader of them goes
// through this first. (ctx_geometry.cpp)
int tree_numbers(fr_ctx* c);
// Foveation control (ctx_foveation.cpp). foveation_init: fr_create's parameters (fr_foveation_default). foveation_check:
// what a sampling launch refuses before anything of it or of its frame is enqueued (mode 6 without a mask; a ray
// budget on a context that has become a rank or sharded).
void foveation_init(fr_ctx* c);
int foveation_check(fr_ctx* c);
// Present (ctx_present.cpp). present_join: the context stream waits for every pack still reading a presentable image
// (join_recon calls it). present_sync: the host waits for the present stream, and the fences are cleared
// (fr_synchronize). present_destroy: fr_destroy's share. All three do nothing on a context that never presented.
void present_join(fr_ctx* c);
int present_sync(fr_ctx* c);
void present_destroy(fr_ctx* c);
}  // namespace fri
static_assert(sizeof(f3) == 3 * sizeof(float), "f3 must be three packed floats");

#define HIP_TRY(ctx, expr)                                                                                      \
  do {                                                                                                          \
    hipError_t e_ = (expr);                                                                                     \
    if (e_ != hipSuccess) return fri::fail(ctx, FR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <class T>
inline hipError_t dalloc(T** p, size_t count) {
  hipError_t e = hipMalloc((void**)p, count * sizeof(T) + 16);
  if (e != hipSuccess) return e;
  // The clear runs on the null stream, which is ordered against none of the context's streams (all non-blocking): the
  // host waits for it here, or it could land on top of what a stream writes into the new array next.
  e = hipMemset(*p, 0, count * sizeof(T) + 16);
  return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}
