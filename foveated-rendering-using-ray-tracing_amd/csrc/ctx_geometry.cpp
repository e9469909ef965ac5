// ctx_geometry.cpp — the scene's geometry after fr_create: the tree (GPU rebuild, refit, SAH cost), position and
// normal updates (synchronous; in stream order, in place or overlapped into a second set), the models' poses by
// matrix, and the switches of motion reprojection and of overlapped updates. (The scene's description on the host, the
// model table and fr_scene_export among it: ctx_scene.cpp.)
#include <algorithm>
#include <chrono>
#include <cmath>

#include "ctx_internal.h"

using namespace fr;
using namespace fri;

bool fri::tree_alloc(TreeArrays* t, size_t node_cap, size_t tri_cap) {
  if (hipMalloc((void**)&t->nodes, node_cap * sizeof(BvhNode)) == hipSuccess &&
      hipMalloc((void**)&t->tri, tri_cap * sizeof(TriGeo)) == hipSuccess &&
      hipMalloc((void**)&t->prim, tri_cap * sizeof(int32_t)) == hipSuccess)
    return true;
  (void)hipGetLastError();
  tree_free(t);
  return false;
}

void fri::tree_free(TreeArrays* t) {
  for (void* p : {(void*)t->nodes, (void*)t->tri, (void*)t->prim})
    if (p) hipFree(p);
  *t = TreeArrays{};
}

void fri::adopt_spare(fr_ctx* c, bool with_shade) {
  std::swap(c->tree, c->spare);
  if (with_shade) {
    std::swap(c->d_shade, c->shade_back);
    c->set_cur ^= 1;
  }
  point_dsc(c);
}

// Per-model visibility: the valid bits of a mask, and the positions a tree writer reads. Every call that builds or
// refits the tree goes through tree_positions with the array it would read: with every model visible (every context
// that never hid one) that array itself comes back and nothing is launched; while a model is hidden k_hide writes its
// collapsed copy into vis_pos on `s`, the writer's stream, ahead of the writer (k_visibility.hip).
static uint32_t vis_valid(const fr_ctx* c) {
  const size_t nm = c->scene.model_tri_count.size();
  return nm >= 32 ? 0xFFFFFFFFu : (1u << nm) - 1u;
}
static int tree_positions(fr_ctx* c, const f3* pos, hipStream_t s, const f3** out) {
  *out = pos;
  if (!(~c->vis_mask & vis_valid(c)) || !c->vis_pos) return FR_OK;
  const int nm = (int)c->scene.model_tri_count.size(), nt = c->scene.num_tris();
  int first[FR_MAX_MODELS];
  for (int i = 0; i < nm; i++) model_info(c->scene, i, nullptr, &first[i], nullptr);
  std::string err;
  if (!gpu_hide_enqueue(hide_args(first, nm, nt, c->vis_mask), pos, c->vis_pos, nt, s, err)) return fail(c, FR_E_HIP, err);
  *out = c->vis_pos;
  return FR_OK;
}

// GPU build over `pos` (device; k_bvh.hip) into the spare arrays, which become the scene's tree when every
// step succeeded (the old tree becomes the spare). No allocation after the first rebuild, no read-back
// of the tree: the host keeps its node count, stack need and depth (fr_scene_export).
int fri::gpu_rebuild(fr_ctx* c, const f3* pos) {
  const int nt = c->scene.num_tris();
  const size_t cap = (size_t)std::max(nt, 1);
  if (!c->spare.nodes && !tree_alloc(&c->spare, cap, cap)) {  // (a failed re-allocation below left none)
    c->err = "GPU BVH: device allocation failed";
    return FR_E_NOMEM;
  }
  if (int rc = tree_positions(c, pos, c->stream, &pos)) return rc;
  int nn = 0, max_stack = 0, depth = 0;
  std::string err;
  // the context's builder: the LBVH, or on a bvh_builder 2 context the binned SAH of k_bvh_sah.hip
  bool unsupported = false;
  if (c->cfg.bvh_builder == 2
          ? !gpu_build_bvh_sah(c->sah_work, c->bvh_work, pos, nt, c->spare, &nn, &max_stack, &depth, &unsupported,
                               c->stream, err)
          : !gpu_build_bvh(&c->bvh_work, pos, nt, c->spare, &nn, &max_stack, &depth, c->stream, err)) {
    c->err = err;
    return unsupported ? FR_E_UNSUPPORTED : FR_E_HIP;
  }
  if (max_stack > FR_BVH_STACK) {
    c->err = "GPU BVH needs a traversal stack deeper than FR_BVH_STACK";
    return FR_E_UNSUPPORTED;
  }
  adopt_spare(c, false);
  if (!c->tree_full_cap) {
    // the replaced tree was sized for the host builder's node count (or there was none): the next spare
    // needs room for any device-built tree (at most one node per triangle)
    tree_free(&c->spare);
    c->tree_full_cap = true;
    // (a failure leaves no spare: allocated again next time; and no second tree: updates are in place until
    // fr_set_geometry_overlap makes one)
    if (!tree_alloc(&c->spare, cap, cap)) c->overlap_on = false;
  }
  Bvh b;
  b.root_count = 0; b.max_stack = max_stack; b.max_depth = depth;
  b.gpu_nodes = nn;
  b.host_nodes = 0;
  c->bvh = std::move(b);
  c->tree_on_device = false;  // (the host has just seen this tree's numbers)
  c->base_stale = true;       // (a conditional rebuild adopts this tree's cost first)
  return FR_OK;
}

// A device record behind the context's pending work, in its pinned copy (a wait).
static int fetch_record(fr_ctx* c, void* pinned, const void* dev, size_t bytes) {
  join_recon(c);
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, hipMemcpyAsync(pinned, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FR_OK;
}

// The record of enqueued rebuilds, and with it the numbers of the tree an enqueued rebuild left, if the host has not
// seen them.
static int fetch_rebuild_record(fr_ctx* c) {
  if (int rc = fetch_record(c, c->h_rb, c->rb, sizeof(fr::RebuildState))) return rc;
  if (!c->tree_on_device) return FR_OK;
  const fr::TreeDesc& d = c->h_rb->tree[c->desc_cur];
  c->bvh.gpu_nodes = (int)d.nodes;
  c->bvh.max_stack = (int)d.max_stack;
  c->bvh.max_depth = (int)d.depth;
  c->tree_on_device = false;
  return FR_OK;
}

int fri::tree_numbers(fr_ctx* c) {
  if (!c->tree_on_device) return FR_OK;
  return fetch_rebuild_record(c);
}

// Refit of the tree in use (either builder's) over `pos` (device), in place (k_bvh.hip). The caller has joined
// and synchronised the context stream.
static int gpu_refit(fr_ctx* c, const f3* pos) {
  if (int rc = tree_numbers(c)) return rc;
  if (int rc = tree_positions(c, pos, c->stream, &pos)) return rc;
  std::string err;
  const int nn = c->bvh.root_count > 0 ? 0 : tree_nodes(c->bvh);
  if (!gpu_refit_bvh(c->bvh_work, pos, c->scene.num_tris(), c->tree, nn, c->stream, err)) {
    c->err = err;
    return c->bvh_work ? FR_E_HIP : FR_E_UNSUPPORTED;
  }
  return FR_OK;
}

// The host's time of `body` on a quiet context (fr_rebuild_bvh, fr_refit_bvh, fr_recompute_normals).
template <class F>
static int host_timed(fr_ctx* c, float* ms, F body) {
  if (!c) return FR_E_INVALID;
  if (int rc = quiesce(c)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = body();
  if (ms) *ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

static int policy_after_update(fr_ctx* c);  // (fr_set_rebuild_policy, below the enqueued rebuild)

extern "C" {

int fr_rebuild_bvh(fr_ctx* c, float* ms) { return host_timed(c, ms, [&] { return gpu_rebuild(c, c->d_pos); }); }
int fr_refit_bvh(fr_ctx* c, float* ms) { return host_timed(c, ms, [&] { return gpu_refit(c, c->d_pos); }); }

int fr_bvh_sah_cost(fr_ctx* c, float* cost) {
  if (!c || !cost) return FR_E_INVALID;
  if (c->bvh.root_count > 0) { *cost = (float)c->bvh.root_count; return FR_OK; }  // one leaf: its triangles
  if (int rc = tree_numbers(c)) return rc;
  join_recon(c);
  hipSetDevice(c->cfg.device);
  std::string err;
  if (!gpu_bvh_cost(c->bvh_work, c->tree.nodes, tree_nodes(c->bvh), cost, c->stream, err))
    return fail(c, c->bvh_work ? FR_E_HIP : FR_E_UNSUPPORTED, err);
  return FR_OK;
}

// A caller's host normals: finite on every triangle that has normals (the others are ignored).
static bool host_normals_finite(const fr_ctx* c, const float* nrm) {
  const HostScene& s = c->scene;
  for (size_t t = 0; t < (size_t)s.num_tris(); t++) {
    if (!(s.flags[t] & FR_SHADE_HAS_NORMALS)) continue;
    for (size_t i = 9 * t; i < 9 * t + 9; i++)
      if (!std::isfinite(nrm[i])) return false;
  }
  return true;
}

// Normals from the caller's array into d_shade (the caller has joined and synchronised the context stream and
// checked the array). Host normals are staged in spare_pos, which is free between updates and of the right size.
static int write_given_normals(fr_ctx* c, const void* nrm, int where, const std::string& name) {
  const float* src = static_cast<const float*>(nrm);
  if (where == FR_MEM_HOST) {
    HIP_TRY(c, hipMemcpy(c->spare_pos, nrm, c->scene.pos.size() * sizeof(f3), hipMemcpyHostToDevice));
    src = &c->spare_pos[0].x;
  }
  std::string err;
  if (!gpu_scatter_normals(c->nrm_work, src, c->d_shade, c->stream, err)) return fail(c, FR_E_HIP, name + ": " + err);
  c->nrm_mirror_stale = true;  // refreshed by the next fr_scene_export
  return FR_OK;
}

static int recompute_normals(fr_ctx* c, const std::string& name) {
  std::string err;
  if (!gpu_recompute_normals(c->nrm_work, c->d_pos, c->d_shade, c->stream, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  c->nrm_mirror_stale = true;
  return FR_OK;
}

// The steps update_positions and fr_update_geometry_enqueue share. The arguments (enqueued: device memory, refit):
static int check_update_args(fr_ctx* c, const std::string& name, size_t ntris, int where, int how, const void* nrm,
                             int normals) {
  if (ntris != (size_t)c->scene.num_tris()) return fail(c, FR_E_INVALID, name + ": triangle count differs");
  if (where != FR_MEM_HOST && where != FR_MEM_DEVICE) return fail(c, FR_E_INVALID, name + ": bad memory kind");
  if (how != FR_BVH_REBUILD && how != FR_BVH_REFIT) return fail(c, FR_E_INVALID, name + ": bad update kind");
  if (normals != FR_NORMALS_KEEP && normals != FR_NORMALS_GIVEN && normals != FR_NORMALS_RECOMPUTE)
    return fail(c, FR_E_INVALID, name + ": bad normals kind");
  if (normals == FR_NORMALS_GIVEN && !nrm) return fail(c, FR_E_INVALID, name + ": FR_NORMALS_GIVEN without normals");
  return FR_OK;
}
// spare_pos, holding the new positions, becomes d_pos. Motion reprojection: spare_pos then holds the outgoing
// positions; if the last G-buffer traced them they become prev_pos (a three-pointer rotation, no copy); after an
// earlier update since that G-buffer prev_pos already holds what it traced and stays.
static void rotate_positions(fr_ctx* c) {
  std::swap(c->d_pos, c->spare_pos);
  if (c->motion_on && !c->moved) {
    std::swap(c->spare_pos, c->prev_pos);
    c->moved = true;
  }
}
// An owed EXTRA keeps the box its sampling launch saw: when that is geo->box, about to change, the debt moves to
// geo->xbox, and the caller enqueues the copy there ahead of the change (true).
static bool extra_keeps_box(fr_ctx* c) {
  if (!c->extra.owed || c->extra.box != c->geo->box) return false;
  c->extra.box = c->geo->xbox;
  return true;
}

// What fr_set_positions, fr_update_positions and fr_update_geometry share. Everything that can reject the update
// runs before anything of the scene is written: the new positions go to the spare device array, which becomes
// d_pos only when the tree over it exists (a failed rebuild leaves d_pos, the tree, the box and the mirror as
// they were). A caller's normals (FR_NORMALS_GIVEN) are checked with the positions, and the normals are written
// last, when positions and tree are in place: nothing after that point rejects the update.
static int update_positions(fr_ctx* c, const void* xyz, size_t ntris, int where, int how, const char* fn,
                            const void* nrm = nullptr, int normals = FR_NORMALS_KEEP) {
  const std::string name = fn;
  if (int rc = check_update_args(c, name, ntris, where, how, nrm, normals)) return rc;
  if (where == FR_MEM_HOST) {
    const float* h = static_cast<const float*>(xyz);
    for (size_t i = 0; i < ntris * 9; i++)
      if (!std::isfinite(h[i])) return fail(c, FR_E_INVALID, name + ": position not finite");
    if (normals == FR_NORMALS_GIVEN && !host_normals_finite(c, static_cast<const float*>(nrm)))
      return fail(c, FR_E_INVALID, name + ": normal not finite");
  }
  if (int rc = quiesce(c)) return rc;
  f3 lo = mk3(INFINITY), hi = mk3(-INFINITY);
  if (where == FR_MEM_DEVICE) {
    // finiteness and the scene box in one kernel over the caller's array, read back before d_pos changes
    bool finite = false;
    float box[6];
    std::string err;
    if (!gpu_check_positions(c->bvh_work, static_cast<const float*>(xyz), (int)ntris, &finite, box, c->stream, err))
      return fail(c, c->bvh_work ? FR_E_HIP : FR_E_UNSUPPORTED, name + ": " + err);
    if (!finite) return fail(c, FR_E_INVALID, name + ": position not finite");
    lo = mk3(box[0], box[1], box[2]);
    hi = mk3(box[3], box[4], box[5]);
    if (normals == FR_NORMALS_GIVEN) {
      if (!gpu_check_normals(c->nrm_work, static_cast<const float*>(nrm), &finite, c->stream, err))
        return fail(c, FR_E_HIP, name + ": " + err);
      if (!finite) return fail(c, FR_E_INVALID, name + ": normal not finite");
    }
  }
  const size_t bytes = ntris * 9 * sizeof(float);
  // (a device-to-device hipMemcpy returns before the copy ran, and the context stream is non-blocking: the
  // copy goes on the context stream, ahead of the kernels that read it)
  if (where == FR_MEM_HOST) HIP_TRY(c, hipMemcpy(c->spare_pos, xyz, bytes, hipMemcpyHostToDevice));
  else HIP_TRY(c, hipMemcpyAsync(c->spare_pos, xyz, bytes, hipMemcpyDeviceToDevice, c->stream));
  if (how == FR_BVH_REBUILD) {
    if (const int rc = gpu_rebuild(c, c->spare_pos)) return fail(c, rc, name + ": rebuild failed, scene unchanged: " + c->err);
  } else if (const int rc = gpu_refit(c, c->spare_pos)) {
    return fail(c, rc, name + ": " + c->err);
  }
  rotate_positions(c);
  if (where == FR_MEM_HOST) {
    memcpy(c->scene.pos.data(), xyz, bytes);
    c->pos_mirror_stale = false;
    box_of(c->scene.pos.data(), c->scene.pos.size(), &lo, &hi);
  } else {
    c->pos_mirror_stale = true;  // refreshed by the next fr_scene_export
  }
  // bbox_min / bbox_max (the depth-saliency theta of k_sampling) follow the geometry, as the
  // reference's scene AABB does at load time (FR/PathTracer.cpp:601-602,663)
  c->scene.bbox_min = c->dsc.bbox_min = lo;
  c->scene.bbox_max = c->dsc.bbox_max = hi;
  if (c->dev_box) {
    // the context has enqueued updates: the saliency stage reads the box from device memory, kept current here
    // (an owed EXTRA keeps the one its sampling launch saw)
    const float box[6] = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z};
    if (extra_keeps_box(c))
      HIP_TRY(c, hipMemcpyAsync(c->geo->xbox, c->geo->box, sizeof(box), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->geo->box, box, sizeof(box), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->box_mirror_stale = false;
  }
  // the normals last, over the positions and the tree now in place (spare_pos holds the replaced positions
  // and is free again)
  if (normals == FR_NORMALS_GIVEN) return write_given_normals(c, nrm, where, name);
  if (normals == FR_NORMALS_RECOMPUTE) return recompute_normals(c, name);
  return FR_OK;
}

int fr_set_positions(fr_ctx* c, const float* xyz, size_t ntris) {
  if (!c || !xyz) return FR_E_INVALID;
  return update_positions(c, xyz, ntris, FR_MEM_HOST, FR_BVH_REBUILD, "fr_set_positions");
}

int fr_update_positions(fr_ctx* c, const void* xyz, size_t ntris, int where, int how) {
  if (!c || !xyz) return FR_E_INVALID;
  return update_positions(c, xyz, ntris, where, how, "fr_update_positions");
}

int fr_update_geometry(fr_ctx* c, const void* xyz, const void* nrm, size_t ntris, int where, int how, int normals) {
  if (!c) return FR_E_INVALID;
  if (!xyz) return fail(c, FR_E_INVALID, "fr_update_geometry: positions are NULL");
  return update_positions(c, xyz, ntris, where, how, "fr_update_geometry", nrm, normals);
}

// fr_update_geometry (device memory, refit) in stream order (enqueue_update, below): every launch there goes on one
// stream, GeoEnqueue's, and nothing waits for the GPU (the enqueue halves of k_bvh.hip / k_normals.hip; no
// synchronisation, no copy to the host, no allocation). What the host learnt from the device in update_positions
// stays there: the verdict of the two checks is a device word that k_take_over publishes and every later kernel of
// the update reads, and the scene box goes from the check's result into geo->box, where the saliency stage reads it
// from now on.
// The three position arrays rotate there, at enqueue time and whatever the verdict, exactly as in update_positions;
// their contents follow in stream order (k_take_over fills the array that becomes d_pos with the caller's
// positions, or with the current ones when the update is rejected).
// In place (the default), the stream is the context stream. That is safe because every reader and writer
// of the three arrays, the tree and the normals is ordered on the context stream: the front stages of a pipelined
// frame run on front_stream, but entry 3 of that frame waits for them on the context stream (front_done) before this
// update is enqueued behind it, and the next frame's front stages wait for the context stream (stream_dirty).
// The reconstruction streams read none of it, so they are not joined.
// Overlapped (fr_set_geometry_overlap), the stream is front_stream, and tree and normals are written out of place,
// into the set no frame in flight reads, which becomes the scene's there (adopt_spare). The hazards:
//  - the set written was the scene's until the previous update: its last reader on the context stream is a
//    megakernel (or a G-buffer there), whose fence front_stream waits for (set_read); the G-buffers of pipelined
//    frames, the only other readers of it and of the position arrays, are earlier work of front_stream itself;
//  - the set read (the scene's) was written by the previous update, on front_stream, or by a synchronous call,
//    which the host waited for;
//  - the megakernel that reads the result waits for its own front stages (front_done), enqueued behind this update;
//  - the scratch of the checks, the refit and the normals, geo (verdict, counters, box, xbox) and the pose staging
//    arrays are shared with what the context stream runs outside a pipelined frame: all of that waits for the
//    update (update_done, consumed by join_recon), and the update waits for it where the front stages would
//    (stream_dirty: ev_stream_join). An owed EXTRA's k_extra, which reads geo->box or geo->xbox, is such work.
//  - two or three updates before one G-buffer alternate the sets; each waits for its own set's fence, so the second
//    one waits for the megakernel still reading the set it writes, and reads what the first wrote in stream order;
//  - after a synchronous rebuild the other set holds another topology: nothing of it is kept (every node, triangle
//    and leaf index is written);
//  - a failed frame's front stages without their entry 3 are earlier work of front_stream.
// (pose: fr_set_model_transforms_enqueue, whose k_pose produces xyz and nrm, the staging arrays, on the same stream)
// An enqueued rebuild (fr_rebuild_bvh_enqueue, enqueue_rebuild below) runs on the same stream under the same rules,
// and in both modes builds out of place, into the spare tree arrays, which the host makes the scene's at enqueue time:
//  - in place (context stream): the spare arrays' last readers are frames enqueued before the rebuild that retired
//    them; their entry 3 is earlier work of the context stream and waited for their front stages (front_done, consumed
//    by GeoEnqueue), and later front stages wait for the context stream (stream_dirty). Shading records and set_cur
//    stay: only the tree's pointers change, as in fr_rebuild_bvh;
//  - overlapped (front_stream): the set written is the one the fences above guard (set_read of the other set,
//    ev_stream_join), its shading records are brought along by gpu_normals_to_enqueue's copy, and tree and records
//    swap together with set_cur, so an update that follows finds the parity it assumes;
//  - the builders' scratch (bvh_work: boxes, codes, binary tree, queues, counters, the scan's; sah_work) and rb
//    (verdict, level counters, the trees' numbers) are shared with the checks, the refit, the cost and the
//    synchronous builders: all of it runs on the update's stream, and synchronous users wait through update_done
//    (join_recon) before they touch it;
//  - the tree's numbers: a refit enqueued behind the rebuild reads the node count from rb->tree[desc_cur] in stream
//    order (nodes_dev); a host reader waits and fetches them (tree_numbers); a frame needs none of them;
//  - a build that fails on the device reads the tree in use (the source of its last kernel's copy), which the
//    previous update or rebuild wrote earlier on this stream.
// Per-model visibility (fr_set_model_visibility_enqueue, and tree_positions inside the update and the rebuild) adds one
// array, vis_pos, and one kernel, k_hide, which writes it right ahead of the tree writer that reads it, on that
// writer's stream. One array is enough in both modes:
//  - every enqueued writer and reader of vis_pos (k_hide; the refit, gated or not, in place or out of place; the
//    builders' first kernels) runs on GeoEnqueue's stream, so they are serial there: a k_hide starts after the
//    previous tree writer has read what the previous k_hide wrote;
//  - the synchronous tree writers (gpu_rebuild, gpu_refit) run on the context stream behind quiesce, which waits for
//    update_done, so for everything front_stream has enqueued; and they finish before the host enqueues anything else
//    (both wait for their result), so a later k_hide on either stream finds vis_pos free;
//  - nothing else reads vis_pos: frames and ray queries read the tree, never the positions the tree was made from (the
//    motion form of the G-buffer reads d_pos and prev_pos, the true positions, and only for triangles a ray has hit,
//    which a hidden triangle never is);
//  - a change of mode (fr_set_geometry_overlap) waits for the context's pending work.
// k_hide reads the array the writer would read (d_pos; the array that becomes d_pos, behind k_take_over), which that
// writer's own fences already guard. The visibility call itself rotates no positions and writes no shading record in
// place; overlapped it brings the records along as the rebuild does (the KEEP copy) and swaps set and records together.
// The preamble of both (the caller has set the device): the stream, and the waits the notes above name.
struct GeoEnqueue {
  fr_ctx* c;
  const bool overlap;
  const hipStream_t s;
  explicit GeoEnqueue(fr_ctx* c_) : c(c_), overlap(c_->overlap_on), s(overlap ? c_->front_stream : c_->stream) {
    if (overlap) {
      if (c->stream_dirty) {
        stream_join(c, s);
        c->stream_dirty = false;  // the next frame's front stages follow this work on front_stream
      }
      c->set_read[c->set_cur ^ 1].consume(s);
    } else {
      c->stream_dirty = true;  // the next pipelined frame's front stages (front_stream) start after this work
      // (front stages whose entry 3 was never enqueued, after a failed frame: ordered before it as well)
      c->front_done.consume(c->stream);
    }
  }
  // whatever was enqueued of overlapped work, the context stream's next work outside a frame waits for it
  ~GeoEnqueue() { if (overlap) c->update_done.record(c->front_stream); }
};

static int enqueue_update(fr_ctx* c, const std::string& name, const void* xyz, const void* nrm, size_t ntris, int normals,
                          void* ready_event, const fr::PoseArgs* pose = nullptr) {
  if (!xyz) return fail(c, FR_E_INVALID, name + ": positions are NULL");
  if (int rc = check_update_args(c, name, ntris, FR_MEM_DEVICE, FR_BVH_REFIT, nrm, normals)) return rc;
  if (c->group_refs > 0 || c->U.shard_count > 1)
    return fail(c, FR_E_UNSUPPORTED, name + ": the context is a rank of a group or sharded (use " +
                                         (pose ? "fr_set_model_transforms)" : "fr_update_geometry)"));
  if (!c->bvh_work || !c->geo) return fail(c, FR_E_UNSUPPORTED, name + ": GPU BVH refit: no workspace for this tree");
  hipSetDevice(c->cfg.device);
  const GeoEnqueue g(c);
  const bool overlap = g.overlap;
  const hipStream_t s = g.s;
  if (ready_event) HIP_TRY(c, hipStreamWaitEvent(s, static_cast<hipEvent_t>(ready_event), 0));
  const int nt = (int)ntris;
  std::string err;
  if (pose && !gpu_pose_enqueue(*pose, c->pose_rest_pos, c->pose_rest_nrm, c->pose_stage_pos, c->pose_stage_nrm, nt, s, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  if (!gpu_check_positions_enqueue(c->bvh_work, static_cast<const float*>(xyz), nt, s, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  const bool given = normals == FR_NORMALS_GIVEN;
  if (given && !gpu_check_normals_enqueue(c->nrm_work, static_cast<const float*>(nrm), &c->geo->bad_nrm, s, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  // the box: seeded from the host's at the first enqueue; an owed EXTRA keeps the one its sampling launch saw
  const int flags = (c->dev_box ? 0 : 1) | (extra_keeps_box(c) ? 2 : 0);  // (2: k_take_over makes the copy)
  if (!gpu_take_over_positions(c->bvh_work, static_cast<const f3*>(xyz), c->d_pos, nt, c->spare_pos,
                               given ? &c->geo->bad_nrm : nullptr, c->geo, flags, c->scene.bbox_min, c->scene.bbox_max,
                               s, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  c->dev_box = c->geo->box;
  c->box_mirror_stale = true;
  if (!given) HIP_TRY(c, c->geo_read.record(s));  // xyz has been read
  const uint32_t* reject = &c->geo->reject;
  const int nn = c->bvh.root_count > 0 ? 0 : tree_nodes(c->bvh);
  // (behind an enqueued rebuild the host's count is stale: the refit takes the tree's from its device record)
  const uint32_t* nn_dev = c->tree_on_device ? &c->rb->tree[c->desc_cur].nodes : nullptr;
  // (a hidden model: k_hide behind k_take_over, over the array that becomes d_pos; after a rejected update that is the
  // current positions again, so it reproduces the collapsed ones the tree was made from, and the gated refit writes
  // nothing, as without it)
  const f3* tree_pos = nullptr;
  if (int rc = tree_positions(c, c->spare_pos, s, &tree_pos)) return rc;
  if (overlap ? !gpu_refit_bvh_to_enqueue(c->bvh_work, tree_pos, nt, c->tree, nn, c->spare, reject, nn_dev, s, err)
              : !gpu_refit_bvh_enqueue(c->bvh_work, tree_pos, nt, c->tree, nn, reject, nn_dev, s, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  rotate_positions(c);
  c->pos_mirror_stale = true;
  const bool recompute = normals == FR_NORMALS_RECOMPUTE;
  if (overlap) {
    // (FR_NORMALS_KEEP as well: the other set's normals are from before the previous update)
    if (!gpu_normals_to_enqueue(c->nrm_work, given ? static_cast<const float*>(nrm) : nullptr,
                                recompute ? c->d_pos : nullptr, c->d_shade, c->shade_back, reject, s, err))
      return fail(c, FR_E_HIP, name + ": " + err);
  } else if (given) {
    if (!gpu_scatter_normals_enqueue(c->nrm_work, static_cast<const float*>(nrm), c->d_shade, reject, s, err))
      return fail(c, FR_E_HIP, name + ": " + err);
  } else if (recompute) {
    if (!gpu_recompute_normals_enqueue(c->nrm_work, c->d_pos, c->d_shade, reject, s, err))
      return fail(c, FR_E_HIP, name + ": " + err);
  }
  if (given) HIP_TRY(c, c->geo_read.record(s));  // nrm has been read as well
  if (given || recompute) c->nrm_mirror_stale = true;
  if (overlap) adopt_spare(c, true);
  return FR_OK;
}

int fr_update_geometry_enqueue(fr_ctx* c, const void* xyz, const void* nrm, size_t ntris, int normals, void* ready_event) {
  if (!c) return FR_E_INVALID;
  if (int rc = enqueue_update(c, "fr_update_geometry_enqueue", xyz, nrm, ntris, normals, ready_event)) return rc;
  return policy_after_update(c);
}

int fr_geometry_consumed(fr_ctx* c, void* stream) {
  if (!c) return FR_E_INVALID;
  if (!c->geo_read.pending) return FR_OK;
  hipSetDevice(c->cfg.device);
  HIP_TRY(c, c->geo_read.peek(static_cast<hipStream_t>(stream)));
  return FR_OK;
}

int fr_geometry_update_status(fr_ctx* c, uint64_t* applied, uint64_t* rejected) {
  if (!c) return FR_E_INVALID;
  if (int rc = fetch_record(c, c->h_geo, c->geo, sizeof(fr::GeoUpdateState))) return rc;
  const fr::GeoUpdateState& g = *c->h_geo;
  if (applied) *applied = g.applied;
  if (rejected) *rejected = g.rejected;
  if (g.rejected > c->geo_rejected_seen[0]) {
    const bool pos = g.rejected_pos > c->geo_rejected_seen[1], nr = g.rejected_nrm > c->geo_rejected_seen[2];
    c->err = std::string("fr_update_geometry_enqueue: ") +
             (pos && nr ? "position not finite, normal not finite" : pos ? "position not finite" : "normal not finite") +
             " (update rejected on the device, scene unchanged)";
  }
  c->geo_rejected_seen[0] = g.rejected;
  c->geo_rejected_seen[1] = g.rejected_pos;
  c->geo_rejected_seen[2] = g.rejected_nrm;
  return FR_OK;
}

// What both enqueued rebuilds and fr_set_rebuild_policy refuse before anything is enqueued.
static int check_rebuild_state(fr_ctx* c, const std::string& name) {
  if (c->group_refs > 0 || c->U.shard_count > 1)
    return fail(c, FR_E_UNSUPPORTED, name + ": the context is a rank of a group or sharded (use fr_rebuild_bvh)");
  const int nt = c->scene.num_tris();
  if (nt < 3) return fail(c, FR_E_HIP, name + ": GPU BVH builder needs at least 3 triangles");
  const bool sah = c->cfg.bvh_builder == 2;
  if (!c->tree_full_cap || !c->spare.nodes || (!c->tree_on_device && c->bvh.gpu_nodes < 0) || !c->bvh_work || !c->rb ||
      !c->geo || (sah && !c->sah_work) || (c->overlap_on && !c->shade_back))
    return fail(c, FR_E_STATE, name + ": the tree in use is not yet a device-built one with a spare set beside it "
                                      "(call fr_rebuild_bvh once first; this call allocates nothing)");
  return FR_OK;
}
static int check_ratio(fr_ctx* c, const std::string& name, float ratio) {
  if (!std::isfinite(ratio) || ratio < 1.0f) return fail(c, FR_E_INVALID, name + ": ratio must be finite and at least 1");
  return FR_OK;
}

// fr_rebuild_bvh in stream order: the context's builder on its fixed launch schedule (gpu_build_bvh_enqueue,
// gpu_build_bvh_sah_enqueue), on the stream enqueue_update would use and behind the same fences: GeoEnqueue and the
// notes above it. The build goes into the spare tree arrays, which become the scene's here, whatever the verdict (a failed
// build ends with the tree in use copied over them, whole). Nothing waits, nothing is copied to the host, nothing is
// allocated: the new tree's numbers are the device record's until a host reader asks (tree_numbers).
// ratio: NULL, or the condition of fr_rebuild_bvh_enqueue_if (checked by the caller). The conditional form puts the
// decision ahead of the schedule and the new tree's cost behind it, on the same stream: the cost's scratch is the
// builders' (bvh_work's codes, counters and hipCUB storage), which the checks and the refit of an update enqueued
// earlier have finished with in stream order, and which the build's first kernels only write after the decision.
static int enqueue_rebuild(fr_ctx* c, const std::string& name, const float* ratio = nullptr) {
  if (int rc = check_rebuild_state(c, name)) return rc;
  const int nt = c->scene.num_tris();
  const bool sah = c->cfg.bvh_builder == 2;
  hipSetDevice(c->cfg.device);
  const GeoEnqueue g(c);
  const bool overlap = g.overlap;
  const hipStream_t s = g.s;
  fr::RebuildTarget t{};
  t.rs = c->rb;
  t.dst = c->spare;
  t.desc = &c->rb->tree[c->desc_cur ^ 1];
  t.src = c->tree;
  t.src_host_nodes = c->tree_on_device ? -1 : tree_nodes(c->bvh);
  t.src_host_desc = fr::TreeDesc{(uint32_t)std::max(t.src_host_nodes, 0), (uint32_t)c->bvh.max_stack,
                                 (uint32_t)c->bvh.max_depth, 0u};
  t.src_desc = &c->rb->tree[c->desc_cur];
  t.conditional = ratio ? 1 : 0;
  std::string err;
  if (ratio && !gpu_rebuild_decide_enqueue(c->bvh_work, c->rb, c->tree.nodes, std::max(t.src_host_nodes, 0), nt,
                                           c->tree_on_device ? &t.src_desc->nodes : nullptr, *ratio, c->base_stale, s, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  const f3* tree_pos = nullptr;  // (a hidden model: the build reads the collapsed positions)
  if (int rc = tree_positions(c, c->d_pos, s, &tree_pos)) return rc;
  if (sah ? !gpu_build_bvh_sah_enqueue(c->sah_work, c->bvh_work, tree_pos, nt, t, s, err)
          : !gpu_build_bvh_enqueue(c->bvh_work, tree_pos, nt, t, s, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  if (ratio && !gpu_rebuild_rebase_enqueue(c->bvh_work, t, nt, s, err)) return fail(c, FR_E_HIP, name + ": " + err);
  c->base_stale = !ratio;  // (the unconditional build installs a tree whose cost nobody has evaluated)
  // (overlapped: the other set's shading records are an update old; the tree's verdict does not touch them)
  if (overlap && !gpu_normals_to_enqueue(c->nrm_work, nullptr, nullptr, c->d_shade, c->shade_back, &c->geo->reject, s, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  adopt_spare(c, overlap);
  c->desc_cur ^= 1;
  c->bvh.root_count = 0;
  c->tree_on_device = true;
  return FR_OK;
}

int fr_rebuild_bvh_enqueue(fr_ctx* c) {
  if (!c) return FR_E_INVALID;
  return enqueue_rebuild(c, "fr_rebuild_bvh_enqueue");
}

int fr_rebuild_bvh_enqueue_if(fr_ctx* c, float ratio) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_rebuild_bvh_enqueue_if";
  if (int rc = check_rebuild_state(c, name)) return rc;
  if (int rc = check_ratio(c, name, ratio)) return rc;
  return enqueue_rebuild(c, name, &ratio);
}

int fr_set_rebuild_policy(fr_ctx* c, float ratio, int period) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_rebuild_policy";
  if (period < 0) return fail(c, FR_E_INVALID, name + ": period is negative");
  if (period > 0) {
    if (int rc = check_rebuild_state(c, name)) return rc;
    if (int rc = check_ratio(c, name, ratio)) return rc;
  }
  c->policy_ratio = ratio;
  c->policy_period = period;
  c->policy_count = 0;
  return FR_OK;
}

}  // extern "C"

// The policy's part of an enqueue call that has accepted its update or pose: every policy_period-th of them is
// followed by the conditional rebuild, as a caller would make it by hand.
static int policy_after_update(fr_ctx* c) {
  if (c->policy_period <= 0 || ++c->policy_count % c->policy_period != 0) return FR_OK;
  c->policy_count = 0;
  return enqueue_rebuild(c, "fr_set_rebuild_policy (the update is enqueued; the rebuild it owes)", &c->policy_ratio);
}

extern "C" {

int fr_bvh_rebuild_policy_status(fr_ctx* c, uint64_t* evaluated, uint64_t* skipped, float* last_cost, float* base_cost) {
  if (!c) return FR_E_INVALID;
  if (int rc = fetch_rebuild_record(c)) return rc;
  const fr::RebuildState& r = *c->h_rb;
  if (evaluated) *evaluated = r.cond_built + r.cond_failed + r.skipped;
  if (skipped) *skipped = r.skipped;
  if (last_cost) *last_cost = r.last_cost;
  if (base_cost) *base_cost = r.base_cost;
  return FR_OK;
}

int fr_bvh_rebuild_status(fr_ctx* c, uint64_t* built, uint64_t* failed) {
  if (!c) return FR_E_INVALID;
  if (int rc = fetch_rebuild_record(c)) return rc;
  const fr::RebuildState& r = *c->h_rb;
  if (built) *built = r.built;
  if (failed) *failed = r.failed;
  if (r.failed > c->rb_failed_seen[0]) {
    std::string why;
    auto add = [&](bool on, const char* text) { if (on) why += (why.empty() ? "" : "; ") + std::string(text); };
    add(r.failed_sah > c->rb_failed_seen[1], "GPU SAH builder: a node has no finite SAH candidate (coordinates too large)");
    add(r.failed_stack > c->rb_failed_seen[2], "GPU BVH needs a traversal stack deeper than FR_BVH_STACK");
    add(r.failed_collapse > c->rb_failed_seen[3], "GPU BVH builder: collapse did not terminate");
    c->err = "fr_rebuild_bvh_enqueue: " + why + " (build failed on the device, the scene keeps its tree)";
  }
  c->rb_failed_seen[0] = r.failed;
  c->rb_failed_seen[1] = r.failed_sah;
  c->rb_failed_seen[2] = r.failed_stack;
  c->rb_failed_seen[3] = r.failed_collapse;
  return FR_OK;
}

// Model poses (the models themselves: model_info, ctx_scene.cpp).
static_assert(FR_MAX_MODELS == FR_POSE_MAX_MODELS, "k_pose's kernel arguments hold FR_MAX_MODELS models");

int fr_model_pose_enable(fr_ctx* c, int on) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_model_pose_enable";
  if (on != 0 && on != 1) return fail(c, FR_E_INVALID, name + ": on is 0 or 1");
  if (!on) { c->pose_on = false; return FR_OK; }
  const size_t nm = c->scene.model_tri_count.size();
  if (nm > FR_MAX_MODELS) return fail(c, FR_E_UNSUPPORTED, name + ": the scene has more than FR_MAX_MODELS models");
  if (int rc = quiesce(c)) return rc;
  const int nt = c->scene.num_tris();
  if (!c->pose_stage_nrm) {
    f3** const arrays[4] = {&c->pose_rest_pos, &c->pose_rest_nrm, &c->pose_stage_pos, &c->pose_stage_nrm};
    const size_t bytes = pose_array_bytes(std::max(nt, 1));
    bool ok = true;
    // (cleared on the context stream, ahead of the capture below: the streams are non-blocking, so a clear on the
    // null stream is ordered against none of them and could land on top of the captured rest geometry)
    for (f3** p : arrays)
      ok = ok && hipMalloc((void**)p, bytes) == hipSuccess && hipMemsetAsync(*p, 0, bytes, c->stream) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      for (f3** p : arrays) { if (*p) hipFree(*p); *p = nullptr; }
      return fail(c, FR_E_NOMEM, name + ": device allocation (rest and staging arrays) failed");
    }
  }
  std::string err;
  if (!gpu_pose_capture_enqueue(c->d_pos, c->d_shade, c->pose_rest_pos, c->pose_rest_nrm, nt, c->stream, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->pose_m.assign(12 * nm, 0.0f);
  for (size_t i = 0; i < nm; i++) c->pose_m[12 * i] = c->pose_m[12 * i + 5] = c->pose_m[12 * i + 10] = 1.0f;
  c->pose_on = true;
  return FR_OK;
}

// What the two pose calls refuse before anything is enqueued, and the kernel arguments of an accepted pose.
static int check_pose(fr_ctx* c, const std::string& name, const float* m, size_t nmodels, fr::PoseArgs* args) {
  if (!m) return fail(c, FR_E_INVALID, name + ": matrices are NULL");
  if (!c->pose_on) return fail(c, FR_E_STATE, name + ": model poses are not enabled (fr_model_pose_enable)");
  const size_t nm = c->scene.model_tri_count.size();
  if (nmodels != nm) return fail(c, FR_E_INVALID, name + ": model count differs");
  int first[FR_MAX_MODELS];
  for (size_t i = 0; i < nm; i++) model_info(c->scene, (int)i, nullptr, &first[i], nullptr);
  if (const char* why = pose_args(args, m, (int)nm, first)) return fail(c, FR_E_INVALID, name + ": " + why);
  return FR_OK;
}

int fr_set_model_transforms(fr_ctx* c, const float* m, size_t nmodels, int how) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_model_transforms";
  fr::PoseArgs args;
  if (int rc = check_pose(c, name, m, nmodels, &args)) return rc;
  if (how != FR_BVH_REBUILD && how != FR_BVH_REFIT) return fail(c, FR_E_INVALID, name + ": bad update kind");
  if (int rc = quiesce(c)) return rc;
  const int nt = c->scene.num_tris();
  std::string err;
  if (!gpu_pose_enqueue(args, c->pose_rest_pos, c->pose_rest_nrm, c->pose_stage_pos, c->pose_stage_nrm, nt, c->stream, err))
    return fail(c, FR_E_HIP, name + ": " + err);
  if (int rc = update_positions(c, c->pose_stage_pos, (size_t)nt, FR_MEM_DEVICE, how, name.c_str(), c->pose_stage_nrm,
                                FR_NORMALS_GIVEN))
    return rc;
  c->pose_m.assign(m, m + 12 * nmodels);
  return FR_OK;
}

int fr_set_model_transforms_enqueue(fr_ctx* c, const float* m, size_t nmodels) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_model_transforms_enqueue";
  fr::PoseArgs args;
  if (int rc = check_pose(c, name, m, nmodels, &args)) return rc;
  if (int rc = enqueue_update(c, name, c->pose_stage_pos, c->pose_stage_nrm, (size_t)c->scene.num_tris(),
                              FR_NORMALS_GIVEN, nullptr, &args))
    return rc;
  c->pose_m.assign(m, m + 12 * nmodels);
  return policy_after_update(c);
}

int fr_model_transforms(fr_ctx* c, float* m, size_t nmodels) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_model_transforms";
  if (!m) return fail(c, FR_E_INVALID, name + ": matrices are NULL");
  if (!c->pose_on) return fail(c, FR_E_STATE, name + ": model poses are not enabled (fr_model_pose_enable)");
  if (12 * nmodels != c->pose_m.size()) return fail(c, FR_E_INVALID, name + ": model count differs");
  memcpy(m, c->pose_m.data(), c->pose_m.size() * sizeof(float));
  return FR_OK;
}

// Per-model visibility (the rule: include/fovrt.h; the positions a tree writer reads: tree_positions, above).
int fr_model_visibility_enable(fr_ctx* c, int on) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_model_visibility_enable";
  if (on != 0 && on != 1) return fail(c, FR_E_INVALID, name + ": on is 0 or 1");
  if (!on) {
    if (~c->vis_mask & vis_valid(c)) return fail(c, FR_E_STATE, name + ": a model is hidden (show every model first)");
    c->vis_on = false;
    return FR_OK;
  }
  if (c->scene.model_tri_count.size() > FR_MAX_MODELS)
    return fail(c, FR_E_UNSUPPORTED, name + ": the scene has more than FR_MAX_MODELS models");
  if (int rc = quiesce(c)) return rc;
  if (!c->vis_pos) {
    const size_t bytes = pose_array_bytes(std::max(c->scene.num_tris(), 1));
    // (cleared on the context stream, ahead of the copy below, for the reason given in fr_model_pose_enable)
    if (hipMalloc((void**)&c->vis_pos, bytes) != hipSuccess || hipMemsetAsync(c->vis_pos, 0, bytes, c->stream) != hipSuccess) {
      (void)hipGetLastError();
      if (c->vis_pos) hipFree(c->vis_pos);
      c->vis_pos = nullptr;
      return fail(c, FR_E_NOMEM, name + ": device allocation (collapsed positions) failed");
    }
    // k_hide's code object is loaded now (HIP loads a module at its first launch, 0.7 to 1 ms measured): one launch
    // with nothing hidden, a plain copy into the new array, so that no enqueued call pays for it
    const int nt = c->scene.num_tris();
    std::string err;
    if (!gpu_hide_enqueue(hide_args(nullptr, 0, nt, FR_VISIBLE_ALL), c->d_pos, c->vis_pos, nt, c->stream, err))
      return fail(c, FR_E_HIP, name + ": " + err);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->vis_on = true;
  return FR_OK;
}

int fr_set_model_visibility(fr_ctx* c, uint32_t visible, int how) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_model_visibility";
  if (how != FR_BVH_REBUILD && how != FR_BVH_REFIT) return fail(c, FR_E_INVALID, name + ": bad update kind");
  if (!c->vis_on) return fail(c, FR_E_STATE, name + ": model visibility is not enabled (fr_model_visibility_enable)");
  if (int rc = quiesce(c)) return rc;
  // the tree writers read the mask in place: it goes back when they fail (a failed rebuild leaves the tree it found)
  const uint32_t before = c->vis_mask;
  c->vis_mask = visible & vis_valid(c);
  if (const int rc = how == FR_BVH_REBUILD ? gpu_rebuild(c, c->d_pos) : gpu_refit(c, c->d_pos)) {
    c->vis_mask = before;
    return fail(c, rc, name + ": " + c->err);
  }
  c->base_stale = true;  // (a conditional rebuild adopts this tree's cost first: showing a model is not growth)
  return FR_OK;
}

// The refit of fr_set_model_visibility in stream order, under GeoEnqueue as an update is: k_hide, then the refit
// nothing gates (geo->accept is the verdict word where a kernel wants one), in place or, overlapped, into the other
// set with the shading records copied along. Positions do not rotate; nothing waits, is copied or allocated.
int fr_set_model_visibility_enqueue(fr_ctx* c, uint32_t visible) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_model_visibility_enqueue";
  if (!c->vis_on) return fail(c, FR_E_STATE, name + ": model visibility is not enabled (fr_model_visibility_enable)");
  if (c->group_refs > 0 || c->U.shard_count > 1)
    return fail(c, FR_E_UNSUPPORTED, name + ": the context is a rank of a group or sharded (use fr_set_model_visibility)");
  if (!c->bvh_work || !c->geo) return fail(c, FR_E_UNSUPPORTED, name + ": GPU BVH refit: no workspace for this tree");
  hipSetDevice(c->cfg.device);
  const GeoEnqueue g(c);
  const uint32_t before = c->vis_mask;
  c->vis_mask = visible & vis_valid(c);
  const f3* tree_pos = nullptr;
  if (int rc = tree_positions(c, c->d_pos, g.s, &tree_pos)) {
    c->vis_mask = before;
    return rc;
  }
  const int nt = c->scene.num_tris();
  const int nn = c->bvh.root_count > 0 ? 0 : tree_nodes(c->bvh);
  const uint32_t* accept = &c->geo->accept;
  const uint32_t* nn_dev = c->tree_on_device ? &c->rb->tree[c->desc_cur].nodes : nullptr;
  std::string err;
  if (g.overlap ? !gpu_refit_bvh_to_enqueue(c->bvh_work, tree_pos, nt, c->tree, nn, c->spare, accept, nn_dev, g.s, err) ||
                      !gpu_normals_to_enqueue(c->nrm_work, nullptr, nullptr, c->d_shade, c->shade_back, accept, g.s, err)
                : !gpu_refit_bvh_enqueue(c->bvh_work, tree_pos, nt, c->tree, nn, nn_dev ? accept : nullptr, nn_dev, g.s, err)) {
    c->vis_mask = before;
    return fail(c, FR_E_HIP, name + ": " + err);
  }
  if (g.overlap) adopt_spare(c, true);
  c->base_stale = true;
  return FR_OK;
}

int fr_model_visibility(fr_ctx* c, uint32_t* visible) {
  if (!c || !visible) return FR_E_INVALID;
  *visible = c->vis_mask & vis_valid(c);
  return FR_OK;
}

// Test hook (not part of include/fovrt.h): k_hide's tile, in triangles.
int fr__visibility_tile(void) { return FR_HIDE_TILE; }

int fr_set_motion_reprojection(fr_ctx* c, int on) {
  if (!c) return FR_E_INVALID;
  if (on != 0 && on != 1) return fail(c, FR_E_INVALID, "fr_set_motion_reprojection: on is 0 or 1");
  if (int rc = quiesce(c)) return rc;
  if (on && !c->prev_pos && dalloc(&c->prev_pos, c->scene.pos.size()) != hipSuccess) {
    (void)hipGetLastError();
    if (c->prev_pos) hipFree(c->prev_pos);
    c->prev_pos = nullptr;
    return fail(c, FR_E_NOMEM, "fr_set_motion_reprojection: device allocation (previous positions) failed");
  }
  c->motion_on = on != 0;
  if (!on) c->moved = false;  // a pending motion is dropped: the next G-buffer is the plain one
  return FR_OK;
}

// The second set of fr_set_geometry_overlap: the GPU builder's spare tree arrays (fr_create made them, with room for
// any device-built tree; a host-built tree of more nodes than that gets bigger ones, once) and a second TriShade
// array, copied from d_shade. On a quiet context. Either everything is made or nothing is kept.
static int make_second_set(fr_ctx* c, const std::string& name) {
  if (int rc = tree_numbers(c)) return rc;
  const size_t nt = (size_t)c->scene.num_tris(), cap = std::max<size_t>(nt, 1), nn = (size_t)tree_nodes(c->bvh);
  const bool first = !c->shade_back;
  const bool tree = !c->spare.nodes || (first && nn > cap);
  TreeArrays made;
  TriShade* shade = nullptr;
  bool ok = !tree || tree_alloc(&made, std::max(cap, nn), cap);
  if (ok && first)
    ok = dalloc(&shade, cap) == hipSuccess &&
         hipMemcpyAsync(shade, c->d_shade, nt * sizeof(TriShade), hipMemcpyDeviceToDevice, c->stream) == hipSuccess &&
         hipStreamSynchronize(c->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    tree_free(&made);
    if (shade) hipFree(shade);
    return fail(c, FR_E_NOMEM, name + ": device allocation (second tree and normals) failed");
  }
  if (tree) {
    tree_free(&c->spare);
    c->spare = made;
  }
  if (first) c->shade_back = shade;
  return FR_OK;
}

int fr_set_geometry_overlap(fr_ctx* c, int on) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_geometry_overlap";
  if (on != 0 && on != 1) return fail(c, FR_E_INVALID, name + ": on is 0 or 1");
  if (int rc = quiesce(c)) return rc;
  if (on)
    if (int rc = make_second_set(c, name)) return rc;
  c->overlap_on = on != 0;
  return FR_OK;
}

int fr_set_normals(fr_ctx* c, const void* nrm, size_t ntris, int where) {
  if (!c) return FR_E_INVALID;
  const std::string name = "fr_set_normals";
  if (!nrm) return fail(c, FR_E_INVALID, name + ": normals are NULL");
  if (ntris != (size_t)c->scene.num_tris()) return fail(c, FR_E_INVALID, name + ": triangle count differs");
  if (where != FR_MEM_HOST && where != FR_MEM_DEVICE) return fail(c, FR_E_INVALID, name + ": bad memory kind");
  if (where == FR_MEM_HOST && !host_normals_finite(c, static_cast<const float*>(nrm)))
    return fail(c, FR_E_INVALID, name + ": normal not finite");
  if (int rc = quiesce(c)) return rc;
  if (where == FR_MEM_DEVICE) {
    bool finite = false;
    std::string err;
    if (!gpu_check_normals(c->nrm_work, static_cast<const float*>(nrm), &finite, c->stream, err))
      return fail(c, FR_E_HIP, name + ": " + err);
    if (!finite) return fail(c, FR_E_INVALID, name + ": normal not finite");
  }
  return write_given_normals(c, nrm, where, name);
}

int fr_recompute_normals(fr_ctx* c, float* ms) {
  return host_timed(c, ms, [&] { return recompute_normals(c, "fr_recompute_normals"); });
}

// Test hook (not part of include/fovrt.h): the tree in use, whichever builder made it, copied to the host:
// fr_scene_export's bvh_nodes BvhNode, then num_tris TriGeo and num_tris leaf-order primitive indices.
int fr__bvh_read(fr_ctx* c, void* nodes, size_t nodes_bytes, void* tri_geo, size_t tri_bytes, int32_t* prim,
                 size_t prim_bytes) {
  if (!c || !nodes || !tri_geo || !prim) return FR_E_INVALID;
  if (int rc = tree_numbers(c)) return rc;
  const Bvh& b = c->bvh;
  const size_t nn = (size_t)tree_nodes(b);
  const size_t nt = (size_t)c->scene.num_tris();
  if (nodes_bytes < nn * sizeof(BvhNode) || tri_bytes < nt * sizeof(TriGeo) || prim_bytes < nt * sizeof(int32_t))
    return fail(c, FR_E_INVALID, "fr__bvh_read: buffer too small");
  if (int rc = quiesce(c)) return rc;
  HIP_TRY(c, hipMemcpy(nodes, c->tree.nodes, nn * sizeof(BvhNode), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(tri_geo, c->tree.tri, nt * sizeof(TriGeo), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(prim, c->tree.prim, nt * sizeof(int32_t), hipMemcpyDeviceToHost));
  return FR_OK;
}

// Test hook (not part of include/fovrt.h): the device addresses of the tree and the normals in use (a frame enqueued
// now reads them there). No wait.
int fr__scene_addresses(fr_ctx* c, const void** nodes, const void** shade) {
  if (!c || !nodes || !shade) return FR_E_INVALID;
  *nodes = c->tree.nodes;
  *shade = c->d_shade;
  return FR_OK;
}

}  // extern "C"
