// ctx_frame.cpp — what a frame enqueues: the four stage enqueues, the reconstruction enqueues, the frame driver
// (frame_half) with its latency schedule, and the stage-call entry points over them. Everything frame_half calls
// per frame is defined here, in one translation unit: other files reach it through fri::.
#include <immintrin.h>
#include <sched.h>

#include <chrono>
#include <cmath>
#include <functional>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

namespace {
// Host-side waits of the latency mode poll (a blocking wait woke the host up to milliseconds late). The spin
// pauses between queries, yields the core every 64 polls (RCCL proxy threads or other ranks' host threads may
// share it), and gives up after a deadline instead of spinning forever on an event that never completes.
constexpr float kPollDeadlineMs = 10000.0f;
inline void cpu_relax() { _mm_pause(); }
hipError_t poll_event(hipEvent_t ev, float deadline_ms) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t n = 1;; n++) {
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    if ((n & 63u) == 0) {
      if (std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count() > deadline_ms)
        return hipErrorNotReady;
      sched_yield();
    } else {
      cpu_relax();
    }
  }
}
float elapsed(hipEvent_t a, hipEvent_t b) {
  float ms = 0.0f;
  hipEventElapsedTime(&ms, a, b);
  return ms;
}
int slotted(const fr_ctx* c, int p0, int pb) { return c->slot == 0 ? p0 : pb + 4 * (c->slot - 1); }
int P_nrm(const fr_ctx* c) { return slotted(c, P_NORMAL, P_NORMAL_B); }
}  // namespace

namespace fri {
int P_pos(const fr_ctx* c) { return slotted(c, P_POSITION, P_POSITION_B); }
int P_shd(const fr_ctx* c) { return slotted(c, P_SHADING, P_SHADING_B); }
int P_wgt(const fr_ctx* c) { return slotted(c, P_WEIGHT, P_WEIGHT_B); }

int check_launch(fr_ctx* c) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, FR_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return FR_OK;
}

// Sums the elapsed times of ring slot i (its last event is synchronised first).
void kt_harvest(fr_ctx* c, int i) {
  hipEventSynchronize(c->kt_ev[i][3]);
  c->kt_stage_ms += elapsed(c->kt_ev[i][0], c->kt_ev[i][3]);
  c->kt_kernel_ms += elapsed(c->kt_ev[i][1], c->kt_ev[i][2]);
  c->kt_frames++;
}

// One frame of the frame clock (fr_frame_clock): its latency, and its interval after the previous frame.
void fc_harvest(fr_ctx* c, int i) {
  hipEventSynchronize(c->fc_ev[i][1]);
  const float s = elapsed(c->fc_ref, c->fc_ev[i][0]), e = elapsed(c->fc_ref, c->fc_ev[i][1]);
  c->fc_latency.push_back(e - s);
  if (c->fc_prev_end >= 0.0) c->fc_interval.push_back((float)(e - c->fc_prev_end));
  c->fc_prev_end = e;
}

void join_update(fr_ctx* c) {
  c->update_done.consume(c->stream);
  c->mask_taken.consume(c->stream);  // (an enqueued caller mask's copy runs on front_stream as well)
}

void join_recon(fr_ctx* c) {
  c->stream_dirty = true;  // the caller is about to enqueue on `stream` outside a pipelined frame
  for (Fence& f : c->recon_done) f.consume(c->stream);
  c->front_done.consume(c->stream);
  join_update(c);
  present_join(c);  // (what the caller enqueues may overwrite an image a present still reads)
}

int quiesce(fr_ctx* c) {
  join_recon(c);
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (Fence& f : c->set_read) f.pending = false;  // (recorded on `stream`: every reader of both sets has finished)
  return FR_OK;
}
}  // namespace fri

// fs: the stream of the front stages (entries 0-2): `stream`, or front_stream in a pipelined frame.
static int enqueue_geometry(fr_ctx* c, hipStream_t fs) {
  // a new frame: move to the next slot, once the reconstruction that read it has finished
  c->slot = (c->slot + 1) % c->nslots;
  c->setup_early = false;
  const int sl = c->slot;
  c->mask = c->mask_p[sl]; c->active = c->active_p[sl]; c->ray_count = c->ray_count_p[sl];
  c->recon_done[sl].consume(fs);  // entry 3 on `stream` waits for fs (front_done)
  if (fs != c->stream) c->trace_done[sl].consume(fs);
  // a present of the slot's SHADING still reading it: entry 3, which overwrites it (the carry and the resolve), waits
  // for these front stages
  c->present_read_shd[sl].peek(fs);
  if (c->lat.arm) hipEventRecord(c->lat.ev[sl].front_begin, fs);
  if (c->fc_arm) {  // fr_frame_clock: where this frame's G-buffer (the first stage to read the gaze) may start
    const int i = c->fc_next;
    if (c->fc_pending == fr_ctx::FC_RING) { fc_harvest(c, i); c->fc_pending--; }
    c->fc_cur = i;
    c->fc_next = (i + 1) % fr_ctx::FC_RING;
    c->fc_pending++;
    hipEventRecord(c->fc_ev[i][0], fs);
  }
  // frame = m_accumFrame++ ; a light change resets the counter afterwards (FR/PathTracer.cpp:99-116)
  c->U.frame = c->accum++;
  if (c->light_pending) { c->light_pending = false; c->accum = 0; }
  if (c->U.frame < 1) {  // d_buffer_init (g_buffer_trace_camera.cu:73-82)
    const size_t bytes = (size_t)c->W * c->H * sizeof(f4);
    hipMemsetAsync(c->img[c->hist_cur], 0, bytes, c->stream);
    hipMemsetAsync(c->img[c->hist_cache], 0, bytes, c->stream);
  }
  if (c->front_local) {  // the primaries this G-buffer traces: the needed tiles and the gaze pixel's
    const int t8 = gaze_tile8(c->U);
    const int tx8 = (c->W + 7) / 8;
    const uint32_t gw = (uint32_t)std::min(8, c->W - (t8 % tx8) * 8), gh = (uint32_t)std::min(8, c->H - (t8 / tx8) * 8);
    c->U.front_pixels = c->front_need_px + (c->front_need_h[t8] ? 0u : gw * gh);
  }
  // motion reprojection: the first G-buffer after a position update reprojects from the positions the previous
  // one traced, and leaves the sampling launch of this frame a distance in WEIGHT.z
  const bool motion = c->motion_on && c->moved;
  launch_gbuffer(c->dsc, c->U, c->img[P_pos(c)], c->img[P_nrm(c)], c->img[c->depth_cur], c->img[P_DIFFUSE],
                 c->img[P_wgt(c)], c->gclass, c->stats, motion ? c->d_pos : nullptr, motion ? c->prev_pos : nullptr,
                 fs);
  c->motion_frame = motion;
  c->moved = false;
  c->compacted = false;
  // (a G-buffer on front_stream is ordered before an overlapped update by the stream itself)
  if (fs == c->stream) mark_set_read(c);
  return check_launch(c);
}

static int enqueue_sampling(fr_ctx* c, hipStream_t fs) {
  c->mask_dirty = false;
  const bool lp = c->U.mask_mode == FR_MASK_LOGPOLAR || c->U.mask_mode == FR_MASK_LOGPOLAR_SIGNED;
  const bool lp_refresh = lp && (c->lp_mode != c->U.mask_mode || c->lp_gaze.x != c->U.gaze.x ||
                                 c->lp_gaze.y != c->U.gaze.y);
  if (lp_refresh) { c->lp_mode = c->U.mask_mode; c->lp_gaze = c->U.gaze; }
  // EXTRA on demand (fr_ctx::extra): the launch stores no heat map and, unless the saliency mask
  // reads them, evaluates no saliency features; what k_extra needs of it is recorded. A tile-local front and tile
  // sharding keep the eager form (their G-buffer inputs do not cover the screen).
  const bool lazy = c->extra_lazy && c->cfg.write_extra && !c->U.front_need && c->U.shard_count <= 1;
  // Foveation control: the eccentricity mask and a caller's mask reach k_sampling as the log-polar mask does, through
  // the mask it reads per pixel: a copy of the uniforms says MASK_LOGPOLAR and `cached` is the array to read. c->U keeps
  // the real mode (the snapshot header and the EXTRA debt read it). Modes 0..4 enter neither branch.
  FrameUniforms Uc = c->U;
  uint8_t* cached = c->lp_cache;
  if (c->U.mask_mode == FR_MASK_ECCENTRIC) {
    // With a ray budget the controller runs first (one lane; it reads the count the last compaction left, when there
    // was one since the last sampling launch) and the mask is generated at every launch from the r2 it leaves in
    // fov_st; without one only when gaze, parameters or mode changed.
    const bool budget = c->fov.ray_budget > 0;
    const float w = (float)c->W, h = (float)c->H;
    const float ww = w * w, hh = h * h;
    if (budget)
      launch_fov_control(c->fov_st, c->fov_count, c->fov_reset, c->fov_r2, c->fov.ray_budget, c->fov.tolerance, ww + hh, fs);
    if (budget || c->fov_dirty || c->lp_mode != FR_MASK_ECCENTRIC || c->lp_gaze.x != c->U.gaze.x ||
        c->lp_gaze.y != c->U.gaze.y) {
      launch_ecc_mask(c->U.gaze, budget ? c->fov_st : nullptr, c->fov_r2, (uint32_t)c->fov.floor_ranks, c->W, c->H,
                      c->lp_cache, fs);
      c->lp_mode = FR_MASK_ECCENTRIC; c->lp_gaze = c->U.gaze;
    }
    c->fov_dirty = false; c->fov_reset = false;
    c->fov_on_device = budget;
    c->fov_used_r2 = c->fov_r2;
    Uc.mask_mode = FR_MASK_LOGPOLAR;
  } else if (c->U.mask_mode == FR_MASK_CALLER) {
    cached = c->cmask;
    Uc.mask_mode = FR_MASK_LOGPOLAR;
  }
  c->fov_count = nullptr;
  launch_sampling(Uc, c->dsc, c->img[P_pos(c)], c->img[c->depth_cur], c->img[c->depth_cache], c->img[P_wgt(c)],
                  c->img[P_nrm(c)], c->img[P_DIFFUSE], c->img[P_EXTRA], c->mask, c->gclass, c->words, c->counts,
                  lazy ? 0 : c->cfg.write_extra, cached, c->lp_inv, lp_refresh,
                  c->U.shard_count > 1 ? c->bcount : nullptr, c->motion_frame, c->dev_box, fs);
  c->motion_frame = false;  // WEIGHT.z is the validity from here on: a repeated sampling launch runs the plain test
  if (c->cfg.write_extra) c->extra.owed = lazy;  // (write_extra = 0: EXTRA is never written, nothing is ever owed)
  if (lazy) c->extra.record(c);
  if (c->U.shard_count > 1) {
    // every rank's active count of this frame (fr_shard_counts, the group's transfer sizes), to pinned
    // host memory with its own event: reading it waits for this frame's front stages only
    launch_owner_counts(c->U, c->bcount, c->owner_counts_p[c->slot], fs);
    hipMemcpyAsync(c->h_counts + (size_t)c->slot * FR_MAX_SHARD_RANKS, c->owner_counts_p[c->slot],
                   sizeof(uint32_t) * FR_MAX_SHARD_RANKS, hipMemcpyDeviceToHost, fs);
    hipEventRecord(c->ev_counts[c->slot], fs);
    c->counts_valid[c->slot] = true;
  }
  c->compacted = false;
  return check_launch(c);
}

static int enqueue_optimize(fr_ctx* c, hipStream_t fs) {
  if (c->mask_dirty) {
    launch_mask_words(c->mask, c->gclass, c->W, c->H, c->words, c->counts, fs);
    c->mask_dirty = false;
  }
  launch_compaction(c->W, c->H, c->words, c->counts, c->offsets, c->tiles, c->ray_count, c->active, fs);
  c->compacted = true;
  c->fov_count = c->ray_count;  // what the ray budget's controller reads ahead of the next sampling launch
  return check_launch(c);
}

int fri::enqueue_shading(fr_ctx* c) {
  if (!c->compacted) {  // g_isOptimize = 0: the active list is still needed by this design
    if (int rc = enqueue_optimize(c, c->stream)) return rc;
  }
  c->front_done.consume(c->stream);  // a pipelined frame: entry 3 waits for its own front stages
  hipEvent_t* kt = nullptr;
  if (c->kt_on) {
    const int i = c->kt_next;
    if (c->kt_pending == fr_ctx::KT_RING) { kt_harvest(c, i); c->kt_pending--; }
    kt = c->kt_ev[i];
    c->kt_next = (i + 1) % fr_ctx::KT_RING;
    c->kt_pending++;
    hipEventRecord(kt[0], c->stream);
  }
  // this frame's sample setup: enqueued by its front stages into the other aux buffer (frame_half), or here
  if (c->setup_early) {
    c->aux_i ^= 1;
    c->aux = c->aux_p[c->aux_i];
    c->aux_seed = c->aux_seed_p[c->aux_i];
  }
  const bool early = c->setup_early;
  c->setup_early = false;
  // The inactive pixels' history carry (HBM-bound) touches no buffer k_shade_paths reads or writes:
  // it runs on carry_stream beside the latency-bound megakernel and joins before the resolve. In latency mode, with one
  // untiled view, it also writes the validity bits of the history this frame leaves (the next frame's early setup).
  const bool hv = c->pipeline_mode == FR_PIPELINE_LATENCY && c->early_setup && c->U.shard_count <= 1 && !c->U.front_need;
  hipEventRecord(c->ev_carry_fork, c->stream);
  hipStreamWaitEvent(c->carry_stream, c->ev_carry_fork, 0);
  launch_carry_history(c->U, c->mask, c->img[P_wgt(c)], c->img[c->hist_cache], c->img[c->hist_cur],
                       c->img[P_shd(c)], hv ? c->hvalid : nullptr, c->carry_stream);
  // (the next frame's early sample setup waits for this record as well: frame_half)
  hipEventRecord(c->ev_carry_done, c->carry_stream);
  const uint32_t N = (uint32_t)((size_t)c->W * c->H);
  if (!early)
    launch_sample_setup(c->U, c->active, c->ray_count, N, c->img[P_wgt(c)], c->img[c->hist_cache], nullptr, c->aux,
                        c->aux_seed, c->stream);
  if (c->time_kernels) hipEventRecord(c->tev.paths_begin, c->stream);
  if (kt) hipEventRecord(kt[1], c->stream);
  launch_shade_paths(c->dsc, c->U, c->active, c->ray_count, N, c->img[P_wgt(c)], c->img[c->hist_cache],
                     c->shade_ctr, c->samples, c->sample_help, c->stats, c->aux, c->aux_seed, c->chunk_refr,
                     c->xcd_bands, c->handoff, c->shade_blocks_per_cu, c->item_store, c->stream);
  if (c->time_kernels) hipEventRecord(c->tev.paths_end, c->stream);
  if (kt) hipEventRecord(kt[2], c->stream);
  hipStreamWaitEvent(c->stream, c->ev_carry_done, 0);
  launch_shade_resolve(c->U, c->active, c->ray_count, N, c->img[P_wgt(c)], c->img[c->hist_cache], c->samples,
                       c->sample_help, c->img[c->hist_cur], c->img[P_shd(c)], c->shade_ctr, c->handoff,
                       c->shade_blocks_per_cu, c->U.shard_count > 1 ? c->shade_radiance : nullptr, c->stream);
  if (kt) hipEventRecord(kt[3], c->stream);
  // this slot's WEIGHT / mask / active list are free for the front stages of frame + nslots after this
  c->trace_done[c->slot].record(c->stream);
  // overlapped updates: the megakernel was the last reader of the scene's tree and normals; the update after the
  // next one writes them (fr_set_geometry_overlap)
  mark_set_read(c);
  int rc = check_launch(c);
  // swapBuffer("history_cache", "history_buffer"); swapBuffer("depth_cache", "depth_buffer") (:226-227)
  std::swap(c->hist_cur, c->hist_cache);
  c->hvalid_fresh = hv;
  std::swap(c->depth_cur, c->depth_cache);
  return rc;
}

// JFA_COORD owed by the last JumpFlooding (launch_jfa with outputs = false), written on `s`, which the caller has
// ordered after that JumpFlooding (from its final state and JFA_COLOR: nothing but the next JumpFlooding or a write of
// JFA_COLOR changes those).
static void materialize_jfa(fr_ctx* c, hipStream_t s) {
  if (!c->jfa_coord_owed) return;
  launch_jfa_coord(c->jfa_final, c->img[P_JFA_COLOR], c->img[P_JFA_COORD], c->W, c->H, s);
  c->jfa_coord_owed = false;
}

// The one place outside enqueue_jfa that clears sib_prefix_fresh. launch_sibson_runs takes its seeds from JFA_COORD
// whenever the prefix sums are not fresh, so a JFA_COORD still owed is written first (on the context stream, after the
// pending reconstruction): !sib_prefix_fresh implies !jfa_coord_owed.
void fri::retire_sibson_prefix(fr_ctx* c) {
  if (c->jfa_coord_owed) {
    join_recon(c);
    hipSetDevice(c->cfg.device);
    materialize_jfa(c, c->stream);
  }
  c->sib_prefix_fresh = false;
}

// EXTRA owed by the last sampling: settled before anything reads it or, outside a frame, overwrites what k_extra reads
void fr_ctx::ExtraDebt::record(const fr_ctx* c) {
  U = c->U;
  sc = c->dsc;
  box = c->dev_box;
  depth = c->depth_cur;
  nrm = P_nrm(c);
  wgt = P_wgt(c);
}
void fr_ctx::ExtraDebt::settle(fr_ctx* c) {
  if (!owed) return;
  join_recon(c);
  hipSetDevice(c->cfg.device);
  launch_extra(U, sc, c->img[depth], c->img[wgt], c->img[nrm], c->img[P_DIFFUSE], c->img[P_EXTRA], box, c->stream);
  owed = false;
}
bool fr_ctx::ExtraDebt::reads(int phys) const {
  return owed && (phys == P_DIFFUSE || phys == depth || phys == nrm || phys == wgt);
}

int fri::resolve(fr_ctx* c, int id, int* phys) {
  // JFA_COORD read by a caller or a pass outside the frame chain, or JFA_COLOR about to be written: JFA_COORD is
  // written first when owed (on the context stream, after the pending reconstruction)
  if ((id == FR_BUF_JFA_COORD || id == FR_BUF_JFA_COLOR) && c->jfa_coord_owed) {
    join_recon(c);
    materialize_jfa(c, c->stream);
  }
  if (id == FR_BUF_EXTRA) c->extra.settle(c);  // the same for a read of EXTRA
  switch (id) {
    case FR_BUF_POSITION: *phys = P_pos(c); return FR_OK;
    case FR_BUF_NORMAL: *phys = P_nrm(c); return FR_OK;
    case FR_BUF_DEPTH: *phys = c->depth_cur; return FR_OK;
    case FR_BUF_DEPTH_CACHE: *phys = c->depth_cache; return FR_OK;
    case FR_BUF_DIFFUSE: *phys = P_DIFFUSE; return FR_OK;
    case FR_BUF_WEIGHT: *phys = P_wgt(c); return FR_OK;
    case FR_BUF_HISTORY: *phys = c->hist_cur; return FR_OK;
    case FR_BUF_HISTORY_CACHE: *phys = c->hist_cache; return FR_OK;
    case FR_BUF_SHADING: *phys = P_shd(c); return FR_OK;
    case FR_BUF_EXTRA: *phys = P_EXTRA; return FR_OK;
    case FR_BUF_JFA_COORD: *phys = P_JFA_COORD; return FR_OK;
    case FR_BUF_JFA_COLOR: *phys = P_JFA_COLOR; return FR_OK;
    case FR_BUF_SIBSON: *phys = P_SIBSON; return FR_OK;
    case FR_BUF_PULLPUSH: *phys = P_PULLPUSH; return FR_OK;
    case FR_BUF_ATROUS: *phys = c->atrous_out; return FR_OK;
    case FR_BUF_LOGPOLAR: *phys = P_LOGPOLAR; return FR_OK;
    case FR_BUF_LOGPOLAR_INVERSE: *phys = P_LOGPOLAR_INV; return FR_OK;
    default: return FR_E_INVALID;
  }
}

// JFA_COORD is written only when something asks for it (materialize_jfa: a caller's read, copy or view of a JFA
// output, a pass reading one, a write of JFA_COLOR). Sibson's run form takes the seeds from the final state and a frame
// reads nothing else of it: 133 MB less per 4K frame. (FOVRT_JFA_LAZY_OUTPUTS=0: always written.)
static int enqueue_jfa(fr_ctx* c, int in_buffer, hipStream_t stream = nullptr) {
  int p;
  if (resolve(c, in_buffer, &p)) return fail(c, FR_E_INVALID, "jfa: bad input buffer");
  const bool run_form = c->cfg.sibson_mode == 0;
  const bool lazy = run_form && c->lazy_jfa_outputs;
  if (!stream) stream = c->stream;
  // The launch's generation (k_jfa.hip). The passes run when the device finds the seed set changed, or when forced;
  // either way the final state is in jfa.F afterwards, so nothing below or later depends on which it was.
  if (++c->jfa_gen == 0) {  // wrapped: the device's word starts over with the count
    hipMemsetAsync(c->jfa.ctl + JFA_CTL_CHANGED, 0, sizeof(uint32_t), stream);
    c->jfa_gen = 1;
  }
  c->jfa_final = launch_jfa(c->img[p], c->jfa, c->jfa_gen, c->jfa_force || !c->jfa_reuse, c->img[P_JFA_COORD],
                            c->img[P_JFA_COLOR], c->ftab, c->W, c->H, run_form ? c->sib_prefix : nullptr,
                            run_form ? c->sib_blocks : nullptr, !lazy, c->jfa_xcd, stream);
  c->jfa_coord_owed = lazy;
  c->sib_prefix_fresh = run_form;
  const int rc = check_launch(c);
  c->jfa_force = rc != FR_OK;  // (a launch that failed may have left the bitmap ahead of the state)
  return rc;
}
static int enqueue_sibson(fr_ctx* c, hipStream_t stream = nullptr) {
  if (c->cfg.sibson_mode == 1) {  // per tap, bit-exact against the oracle (reads JFA_COORD)
    materialize_jfa(c, stream ? stream : c->stream);
    launch_sibson(c->img[P_JFA_COORD], c->img[P_JFA_COLOR], c->img[P_SIBSON], c->W, c->H, stream ? stream : c->stream);
  } else {  // run form (default): exact tap sets, rounding-level differences
    launch_sibson_runs(c->img[P_JFA_COORD], c->jfa_final, c->img[P_JFA_COLOR], c->sib_prefix, c->sib_blocks, c->sib_rowp, c->sib_wide,
                       c->sib_strips, c->img[P_SIBSON], c->W, c->H, c->sib_prefix_fresh, c->sib_strip, c->sib_strip_mid,
                       c->jfa_coord_owed,
                       stream ? stream : c->stream);
  }
  return check_launch(c);
}
static int enqueue_pullpush(fr_ctx* c, int in_buffer, hipStream_t stream = nullptr) {
  int p;
  if (resolve(c, in_buffer, &p)) return fail(c, FR_E_INVALID, "pullpush: bad input buffer");
  launch_pullpush(c->img[p], c->pull, c->push, c->snap, c->img[P_PULLPUSH], c->W, c->H, stream ? stream : c->stream);
  return check_launch(c);
}
static int enqueue_atrous(fr_ctx* c, int count, int pos, int nrm, int col, hipStream_t stream = nullptr) {
  if (!stream) stream = c->stream;
  int pp, pn, pc;
  if (count < 1 || resolve(c, pos, &pp) || resolve(c, nrm, &pn) || resolve(c, col, &pc))
    return fail(c, FR_E_INVALID, "atrous: bad arguments");
  if (pc == P_ATROUS_A || pc == P_ATROUS_B) return fail(c, FR_E_INVALID, "atrous: colour input aliases the output");
  float c_phi = 1.f, n_phi = 1.f, p_phi = 1.f;
  int sw = 1;
  // (phis and step widths stay powers of two below, which launch_atrous requires)
  const f4* in = c->img[pc];
  int out = P_ATROUS_B;
  for (int k = 0; k < count; k++) {  // FR/ATrous.cpp:90-113
    if (k) { c_phi *= 1.0f; n_phi *= 0.5f; p_phi *= 1.0f; sw *= 2; }
    out = out == P_ATROUS_A ? P_ATROUS_B : P_ATROUS_A;
    if (!launch_atrous(c->img[pp], c->img[pn], in, c->img[out], c->W, c->H, c_phi, n_phi, p_phi, (float)sw,
                       c->atrous_rows2, c->atrous_xcd, stream))
      return fail(c, FR_E_INVALID, "atrous: bad arguments");
    in = c->img[out];
  }
  c->atrous_out = out;
  return check_launch(c);
}

static int timed(fr_ctx* c, const std::function<int()>& f, float* ms) {
  hipSetDevice(c->cfg.device);
  join_recon(c);
  hipEventRecord(c->tev.stage_begin, c->stream);
  if (int rc = f()) return rc;
  hipEventRecord(c->tev.stage_end, c->stream);
  hipError_t e = hipEventSynchronize(c->tev.stage_end);
  if (e != hipSuccess) return fail(c, FR_E_HIP, std::string("stage failed: ") + hipGetErrorString(e));
  if (ms) *ms = elapsed(c->tev.stage_begin, c->tev.stage_end);
  return FR_OK;
}

// Latency mode, before a frame is enqueued: one frame ahead at most. The host waits until the previous frame's
// (slot prev's) JumpFlooding has ended (its path trace, when this context does not run that chain), then the caller
// samples the gaze and enqueues this frame, whose front stages (G-buffer, sampling, compaction) overlap the previous
// frame's Sibson and pull-push -> A-Trous; its path trace starts after them (frame_half).
// (polled: a blocking wait woke the host up to milliseconds late, and the GPU idled meanwhile)
static int wait_for_previous_frame(fr_ctx* c, int prev) {
  if (!c->jfa_done[prev].pending && !c->trace_done[prev].pending) return FR_OK;
  fr_ctx::LatSchedule& L = c->lat;
  hipEvent_t w = c->jfa_done[prev].pending ? c->jfa_done[prev].ev : c->trace_done[prev].ev;
  hipError_t e;
  if ((e = poll_event(w, kPollDeadlineMs)) != hipSuccess)
    return fail(c, FR_E_HIP, e == hipErrorNotReady ? std::string("frame failed: the previous frame did not complete within the poll deadline")
                                                    : std::string("frame failed: ") + hipGetErrorString(e));
  // Just in time: the front stages should end about when the previous frame's Sibson does (its path
  // trace waits for both). A completed frame's times estimate the two; when its Sibson took longer than
  // half its front stages, the host waits the difference more (an eye-tracked gaze's big discs: 2-5 ms of
  // Sibson against ~1.3 ms of front stages), so the gaze is sampled that much later.
  for (int k = 0; k < c->nslots; k++) {
    if (!L.rec[k] || hipEventQuery(L.ev[k].recon_end) != hipSuccess) continue;
    float f = 0.0f, sb = 0.0f;
    if (hipEventElapsedTime(&f, L.ev[k].front_begin, L.ev[k].front_end) == hipSuccess &&
        hipEventElapsedTime(&sb, L.ev[k].jfa_end, L.ev[k].recon_end) == hipSuccess) {
      // The front stages' span is the smallest of the last eight: a front stage that overlapped the
      // previous Sibson ran slower, and estimating from it started the next front stages earlier still (into
      // more of that Sibson: a feedback that held the eye-tracked circle's fronts at ~4 ms instead of ~1)
      L.front_hist[L.front_n++ & 7] = f;
      L.front_ms = f;
      for (int j = 1; j < std::min(8, L.front_n); j++)
        L.front_ms = std::min(L.front_ms, L.front_hist[(L.front_n - 1 - j) & 7]);
      L.sib_ms = sb;
    }
    L.rec[k] = false;
  }
  // Only half of the front stages' span is overlapped: the big discs' strip kernel fills every CU, and a
  // front stage started further into it ran ~4 ms instead of ~1, with its gaze sampled that much earlier
  // (eye-tracked circle latency p99 16.2 -> 12.6 ms at 142 fps; C3 p50 6.15 -> 5.81 ms; overlapping none:
  // p99 12.5 ms at 139 fps, the serial loop's rate). A short Sibson (no big discs: below kLatShortSibMs) takes the
  // whole span: the front stages then end with it without slowing down (4K bunny centred 186.0 -> 189.3 fps at
  // latency p50 5.72 -> 5.79 ms, 4K vokselia 233.1 -> 235.2 fps; profiles/r06_lat_overlap_*). FOVRT_LAT_OVERLAP:
  // one percentage for every frame instead (A/B knob).
  constexpr float kLatShortSibMs = 1.5f;
  static const float ovl_env = [] { const char* v = getenv("FOVRT_LAT_OVERLAP"); return v ? atoi(v) / 100.0f : -1.0f; }();
  const float ovl = ovl_env >= 0.0f ? ovl_env : L.sib_ms < kLatShortSibMs ? 1.0f : 0.5f;
  const float delay_ms = c->jfa_done[prev].pending ? L.sib_ms - ovl * L.front_ms : 0.0f;
  if (delay_ms > 0.05f) {
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count() < delay_ms &&
           hipEventQuery(c->recon_done[prev].ev) == hipErrorNotReady) {
      cpu_relax();
    }
  }
  c->jfa_done[prev].pending = false;  // polled by the host: no stream waits for it
  return FR_OK;
}

void fri::stream_join(fr_ctx* c, hipStream_t waiter) {
  hipEventRecord(c->ev_stream_join, c->stream);
  hipStreamWaitEvent(waiter, c->ev_stream_join, 0);
}

// Frame halves: the trace half (update -> entries 0..3) and the reconstruction half (JFA -> SI ->
// PPI -> AT). fr_frame runs both; a tile-sharded view runs the trace half on every rank and the
// reconstruction half on the rank that composites (after fr_shard_unpack of the other ranks' tiles).
int fri::frame_half(fr_ctx* c, fr_frame_timing* t, bool trace, bool recon) {
  if (!c) return FR_E_INVALID;
  hipSetDevice(c->cfg.device);
  const fr_ctx::StageEvents& T = c->tev;  // recorded by timed frames only (t)
  int rc;
  // fr_frame_clock: a frame that fails after enqueue_geometry reserved its ring entry gives the entry
  // back (it would never get its end event)
  struct FcGuard {
    fr_ctx* c;
    ~FcGuard() {
      if (c->fc_cur < 0) return;
      c->fc_next = c->fc_cur;
      c->fc_pending--;
      c->fc_cur = -1;
    }
  } fc_guard{c};
  if (t) {
    join_update(c);  // a timed frame's stages all run on `stream`: behind an overlapped update on front_stream
    hipEventRecord(T.begin, c->stream);
  }
  if (trace && (rc = foveation_check(c))) return rc;
  if (trace) {
    // untimed frames pipeline: the front stages go to front_stream and overlap the previous frame's
    // entry 3 (timed frames keep every stage on `stream`, one after the other)
    hipStream_t fs = t ? c->stream : c->front_stream;
    const bool latency = !t && c->pipeline_mode == FR_PIPELINE_LATENCY;
    const int prev = c->slot;  // the previous frame's slot
    if (latency && (rc = wait_for_previous_frame(c, prev))) return rc;
    // the front stages overwrite buffers (gclass, DIFFUSE, EXTRA, depth, ballots, counts, lp_cache) that
    // work enqueued on `stream` by other calls may still read: order them after it explicitly
    if (!t && c->stream_dirty) stream_join(c, fs);
    c->stream_dirty = false;
    c->fc_arm = c->fc_on && recon;  // whole frames only (a group's trace half has no end of its own)
    c->lat.arm = latency && recon;
    rc = enqueue_geometry(c, fs);
    c->fc_arm = false;
    if (rc) { c->lat.arm = false; return rc; }
    if (t) hipEventRecord(T.geometry, c->stream);
    if ((rc = enqueue_sampling(c, fs))) return rc;
    if (t) hipEventRecord(T.sampling, c->stream);
    if ((rc = enqueue_optimize(c, fs))) return rc;
    if (t) hipEventRecord(T.optimize, c->stream);
    if (latency && fs != c->stream && c->hvalid_fresh && c->U.shard_count <= 1 && !c->U.front_need && c->early_setup) {
      // Early sample setup (latency mode): from the validity bits of the previous frame's history instead of the
      // history itself, so it runs here with the front stages, and this frame's megakernel starts as
      // soon as the previous frame's reconstruction ends (the setup sat between them on the context stream, ~0.1 ms
      // on the CUs the reconstruction had just filled). Into the aux buffer the previous megakernel does not read.
      // (Throughput mode keeps the setup after the resolve: there the megakernel then started beside the previous
      // frame's reconstruction burst and ran 3.9 -> 4.1 ms, 240 -> 232 fps; profiles/r06_early_setup_ab.txt.)
      // Across frames: ev_carry_done still holds the PREVIOUS frame's record here (enqueue_shading below makes this
      // frame's), the carry that wrote those validity bits.
      hipStreamWaitEvent(fs, c->ev_carry_done, 0);
      const int o = c->aux_i ^ 1;
      launch_sample_setup(c->U, c->active, c->ray_count, (uint32_t)((size_t)c->W * c->H), c->img[P_wgt(c)], nullptr,
                          c->hvalid, c->aux_p[o], c->aux_seed_p[o], fs);
      if ((rc = check_launch(c))) return rc;
      c->setup_early = true;
    }
    if (!t) c->front_done.record(fs);
    if (c->lat.arm) hipEventRecord(c->lat.ev[c->slot].front_end, fs);
    // latency mode: this frame's path trace starts after the previous frame's reconstruction. The
    // megakernel fills every CU, so a reconstruction running beside it waited for it to end and then
    // delayed this frame's own reconstruction (pipelined latency p50 10-12 ms against a 5.6 ms frame).
    // (peek: the front stages of the frame that reuses slot prev still wait for it)
    if (latency) c->recon_done[prev].peek(c->stream);
    c->time_kernels = t != nullptr;
    rc = enqueue_shading(c);
    c->time_kernels = false;
    if (rc) return rc;
  } else if (t) {
    for (hipEvent_t e : {T.geometry, T.sampling, T.optimize, T.paths_begin, T.paths_end}) hipEventRecord(e, c->stream);
  }
  if (t) hipEventRecord(T.shading, c->stream);
  if (recon) {
    // The reconstruction of this frame's shading runs on its own streams, so the next frame's trace
    // half (on `stream`) overlaps it. Two independent chains read the shading: JFA -> Sibson
    // (sibson_stream) and pull-push -> A-Trous (atrous_stream; atFS binds the JFA texture but never reads it,
    // FR/shader/atFS.glsl:40-90). Both resolve their inputs now, at this frame's slot.
    // (a group's reconstruction rank may run only one of the chains: c->recon_chains)
    hipEventRecord(c->ev_recon_fork, c->stream);
    hipStreamWaitEvent(c->sibson_stream, c->ev_recon_fork, 0);
    hipStreamWaitEvent(c->atrous_stream, c->ev_recon_fork, 0);
    // a present still reading SIBSON, PULLPUSH or an A-Trous image (atrous_stream is ordered behind nothing else of
    // the previous frame's than its own chain)
    c->present_read.peek(c->sibson_stream);
    c->present_read.peek(c->atrous_stream);
    if (t) hipEventRecord(T.chain1_begin, c->sibson_stream);
    if ((c->recon_chains & 1) && (rc = enqueue_jfa(c, FR_BUF_SHADING, c->sibson_stream))) return rc;
    if (t) hipEventRecord(T.jfa, c->sibson_stream);
    if (c->pipeline_mode == FR_PIPELINE_LATENCY && (c->recon_chains & 1)) {
      c->jfa_done[c->slot].record(c->sibson_stream);
      if (c->lat.arm) hipEventRecord(c->lat.ev[c->slot].jfa_end, c->sibson_stream);
    }
    if ((c->recon_chains & 1) && (rc = enqueue_sibson(c, c->sibson_stream))) return rc;
    if (t) hipEventRecord(T.sibson, c->sibson_stream);
    if (c->recon_gate) hipStreamWaitEvent(c->atrous_stream, c->recon_gate, 0);
    if (t) hipEventRecord(T.chain2_begin, c->atrous_stream);
    if ((c->recon_chains & 2) && (rc = enqueue_pullpush(c, FR_BUF_SHADING, c->atrous_stream))) return rc;
    if (t) hipEventRecord(T.pullpush, c->atrous_stream);
    if ((c->recon_chains & 2) && (rc = enqueue_atrous(c, c->cfg.atrous_iterations, FR_BUF_POSITION, FR_BUF_NORMAL,
                                                      FR_BUF_PULLPUSH, c->atrous_stream))) return rc;
    if (t) hipEventRecord(T.atrous, c->atrous_stream);
    hipEventRecord(c->ev_chain2_done, c->atrous_stream);
    hipStreamWaitEvent(c->sibson_stream, c->ev_chain2_done, 0);
    c->recon_done[c->slot].record(c->sibson_stream);  // this slot's buffers are free again after this
    if (c->lat.arm && (c->recon_chains & 1)) {
      hipEventRecord(c->lat.ev[c->slot].recon_end, c->sibson_stream);
      c->lat.rec[c->slot] = true;
    }
    c->lat.arm = false;
    if (c->fc_cur >= 0) {  // fr_frame_clock: both chains of this frame are done
      hipEventRecord(c->fc_ev[c->fc_cur][1], c->sibson_stream);
      c->fc_cur = -1;
    }
    if (t) join_recon(c);
  }
  if (t) {
    hipEventRecord(T.end, c->stream);
    hipError_t e = hipEventSynchronize(T.end);
    if (e != hipSuccess) return fail(c, FR_E_HIP, std::string("frame failed: ") + hipGetErrorString(e));
    t->geometry_ms = elapsed(T.begin, T.geometry);
    t->sampling_ms = elapsed(T.geometry, T.sampling);
    t->optimize_ms = elapsed(T.sampling, T.optimize);
    t->shading_ms = elapsed(T.optimize, T.shading);
    t->jfa_ms = recon ? elapsed(T.chain1_begin, T.jfa) : 0.0f;
    t->sibson_ms = recon ? elapsed(T.jfa, T.sibson) : 0.0f;
    t->pullpush_ms = recon ? elapsed(T.chain2_begin, T.pullpush) : 0.0f;
    t->atrous_ms = recon ? elapsed(T.pullpush, T.atrous) : 0.0f;
    t->total_ms = elapsed(T.begin, T.end);
    t->shade_paths_ms = elapsed(T.paths_begin, T.paths_end);
    hipMemcpy(&t->ray_count, c->ray_count, 4, hipMemcpyDeviceToHost);
  }
  return FR_OK;
}

extern "C" {

int fr_geometry_launch(fr_ctx* c, float* ms) {
  if (!c) return FR_E_INVALID;
  c->extra.settle(c);  // the stage call overwrites DIFFUSE and DEPTH, and the caller may read EXTRA before the next sampling
  return timed(c, [&] { return enqueue_geometry(c, c->stream); }, ms);
}
int fr_sampling_launch(fr_ctx* c, float* ms) {
  if (!c) return FR_E_INVALID;
  if (int rc = foveation_check(c)) return rc;
  return timed(c, [&] { return enqueue_sampling(c, c->stream); }, ms);
}
int fr_optimize_launch(fr_ctx* c, float* ms) { if (!c) return FR_E_INVALID; return timed(c, [&] { return enqueue_optimize(c, c->stream); }, ms); }
int fr_shading_launch(fr_ctx* c, float* ms) { if (!c) return FR_E_INVALID; return timed(c, [&] { return enqueue_shading(c); }, ms); }

static int ns_timed(fr_ctx* c, std::function<int()> f, uint64_t* ns) {
  float ms = 0;
  int rc = timed(c, f, &ms);
  if (ns) *ns = (uint64_t)((double)ms * 1e6);
  return rc;
}
int fr_jfa_render(fr_ctx* c, int in_buffer, uint64_t* ns) { if (!c) return FR_E_INVALID; return ns_timed(c, [&] { return enqueue_jfa(c, in_buffer); }, ns); }
int fr_sibson_render(fr_ctx* c, uint64_t* ns) { if (!c) return FR_E_INVALID; return ns_timed(c, [&] { return enqueue_sibson(c); }, ns); }
int fr_pullpush_render(fr_ctx* c, int in_buffer, uint64_t* ns) { if (!c) return FR_E_INVALID; return ns_timed(c, [&] { return enqueue_pullpush(c, in_buffer); }, ns); }
static int enqueue_logpolar(fr_ctx* c, int in_buffer) {
  int p;
  if (resolve(c, in_buffer, &p)) return fail(c, FR_E_INVALID, "logpolar: bad input buffer");
  if (p == P_LOGPOLAR || p == P_LOGPOLAR_INV) return fail(c, FR_E_INVALID, "logpolar: input is one of its outputs");
  launch_logpolar(c->img[p], c->img[P_LOGPOLAR], c->img[P_LOGPOLAR_INV], c->W, c->H, c->U.gaze, c->stream);
  return check_launch(c);
}
int fr_logpolar_render(fr_ctx* c, int in_buffer, uint64_t* ns) {
  if (!c) return FR_E_INVALID;
  return ns_timed(c, [&] { return enqueue_logpolar(c, in_buffer); }, ns);
}

// g_gaze is a Win32 POINT (LONG x, y; FR/gui.h:14) and the cursor a double: the assignment truncates
// toward zero (clamped to the LONG range here, where C++ leaves it undefined)
static long to_long(double v) { return (long)std::max(-2147483648.0, std::min(2147483647.0, std::trunc(v))); }
static void set_g_gaze(fr_ctx* c, long gx, long gy) {
  // m_context["gaze"] = (float(g_gaze.x), float(g_screenSize.cy - g_gaze.y)) (FR/PathTracer.cpp:795); off-window
  // cursors are kept as given (the log-polar mask and the gaze distance are defined for any gaze); the two
  // texel reads at the gaze clamp to the screen (k_sampling, fr_gaze_target)
  c->U.gaze = mk2((float)gx, (float)((long)c->H - gy));
}
int fr_set_gaze(fr_ctx* c, double xpos, double ypos, int fullscreen) {
  // cursorPosCallback (FR/gui.cpp:48-66): adjust_scale = g_fullScreen ? 1 : 1.25 (:51-56);
  // g_gaze.x = xpos; g_gaze.y = ypos * adjust_scale (:65-66, and :59-60 on the first call)
  if (!c || !std::isfinite(xpos) || !std::isfinite(ypos)) return FR_E_INVALID;
  const float adjust_scale = fullscreen ? 1.0f : 1.25f;
  set_g_gaze(c, to_long(xpos), to_long(ypos * adjust_scale));
  return FR_OK;
}
int fr_reset_gaze(fr_ctx* c) {
  // framebufferSizeCallback (FR/gui.cpp:32-35): g_gaze = (w / 2, h / 2), integer division
  if (!c) return FR_E_INVALID;
  set_g_gaze(c, c->W / 2, c->H / 2);
  return FR_OK;
}

int fr_atrous_render(fr_ctx* c, int count, int pos, int nrm, int col, uint64_t* ns) {
  if (!c) return FR_E_INVALID;
  return ns_timed(c, [&] { return enqueue_atrous(c, count, pos, nrm, col); }, ns);
}

int fr_frame(fr_ctx* c, fr_frame_timing* t) { return frame_half(c, t, true, true); }
int fr_set_pipeline_mode(fr_ctx* c, int mode) {
  if (!c) return FR_E_INVALID;
  if (mode != FR_PIPELINE_THROUGHPUT && mode != FR_PIPELINE_LATENCY)
    return fail(c, FR_E_INVALID, "fr_set_pipeline_mode: FR_PIPELINE_THROUGHPUT (0) or FR_PIPELINE_LATENCY (1)");
  c->pipeline_mode = mode;
  return FR_OK;
}
int fr_set_sample_sum(fr_ctx* c, int mode) {
  if (!c) return FR_E_INVALID;
  if (mode < 0 || mode > 2) return fail(c, FR_E_INVALID, "fr_set_sample_sum: mode 0 (fp32), 1 (by frame size) or 2 (fixed point)");
  if ((uint32_t)mode == c->handoff) return FR_OK;
  join_recon(c);
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, hipDeviceSynchronize());
  // the fixed-point form keeps 32-B sample records and a 32-B help record per sample
  const size_t N = (size_t)c->W * c->H;
  const size_t need_s = std::max(N * c->cfg.spp, 2 * shade_fx_slots((uint32_t)N, c->cfg.spp, (uint32_t)mode, c->shade_blocks_per_cu));
  const size_t need_h = std::max<size_t>(4 * shade_fx_slots((uint32_t)N, c->cfg.spp, (uint32_t)mode, c->shade_blocks_per_cu), 1);
  const size_t have_s = std::max(N * c->cfg.spp, 2 * shade_fx_slots((uint32_t)N, c->cfg.spp, c->handoff, c->shade_blocks_per_cu));
  const size_t have_h = std::max<size_t>(4 * shade_fx_slots((uint32_t)N, c->cfg.spp, c->handoff, c->shade_blocks_per_cu), 1);
  if (need_s > have_s) {
    hipFree(c->samples); c->samples = nullptr;
    if (dalloc(&c->samples, need_s) != hipSuccess) return fail(c, FR_E_NOMEM, "fr_set_sample_sum: allocation failed");
  }
  if (need_h > have_h) {
    hipFree(c->sample_help); c->sample_help = nullptr;
    if (dalloc(&c->sample_help, need_h) != hipSuccess) return fail(c, FR_E_NOMEM, "fr_set_sample_sum: allocation failed");
  }
  c->handoff = (uint32_t)mode;
  return FR_OK;
}

int fr_set_recon_chains(fr_ctx* c, int chains) {
  if (!c) return FR_E_INVALID;
  if (chains < 0 || chains > 3) return fail(c, FR_E_INVALID, "fr_set_recon_chains: chains is a mask of bits 0 and 1");
  c->recon_chains = chains;
  return FR_OK;
}
int fr_trace_frame(fr_ctx* c, fr_frame_timing* t) { return frame_half(c, t, true, false); }
int fr_reconstruct_frame(fr_ctx* c, fr_frame_timing* t) { return frame_half(c, t, false, true); }

}  // extern "C"
