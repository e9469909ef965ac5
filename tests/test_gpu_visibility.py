"""GPU suite for per-model visibility: fr_model_visibility_enable / fr_set_model_visibility /
fr_set_model_visibility_enqueue / fr_model_visibility.

The reference of a hidden model is the scene with every triangle of that model collapsed onto its first vertex
(ray_surface_cases.collapsed; tests/test_cpu_visibility.py holds the cases to what they claim). Trees are compared in
bytes with bvh_refit_np.refit_np over those positions and validated against them; frames with the oracle over the
collapsed arrays and the original scene box; stream order with a twin that makes the same sequence through the
synchronous calls; ray queries with the masked references at masks & visible. Scenes 0 and 1, procedural, detail 1;
frames at 100 x 70, queries at ray_cases.SIZE."""
import ctypes as C

import numpy as np
import pytest

import bvh_np
import pose_np as pn
import ray_cases as rc
import ray_surface_cases as rs
import trace_np as tn
import visibility_cases as vc
from bvh_canon_np import scene_rebuild_over
from bvh_refit_np import canonical_tree, refit_np
from helpers import equal_nan
from normals_np import recompute_np
from test_cpu_ray_surface import aimed
from test_cpu_rebuild_policy import mild
from test_gpu_bvh import mismatch_report, tree_bytes
from test_gpu_bvh_sah import assert_tree_is_hosts
from test_gpu_normals import assert_same_bits
from test_gpu_ray_queries import check_transmittance
from test_gpu_ray_surface import dev as dev_any, out_buf, query, records, report
from test_gpu_trace_edges import _default_schedule, _tn, check_front, check_gbuffer, shade_and_check  # noqa: F401
from test_gpu_update_enqueue import dev, settle

pytestmark = pytest.mark.gpu

F = np.float32
W, H = vc.W, vc.H
LBVH, SAH = 1, 2
ALL = vc.ALL


def mk(fovrt, scene, builder=0, w=W, h=H, visibility=True, motion=False, latency=False, overlap=False, pose=False, **kw):
    kw.setdefault("mask_mode", 4)
    kw.setdefault("spp", 2)
    t = fovrt.PathTracer(rc.config(fovrt, scene, w, h, builder, **kw))
    assert t.initialize(), t.last_error()
    if motion:
        t.set_motion_reprojection(True)
    if latency:
        t.set_pipeline_mode(fovrt.PIPELINE_LATENCY)
    if overlap:
        t.set_geometry_overlap(True)
    if pose:
        t.enable_model_pose()
    if visibility:
        t.enable_model_visibility()
    return t


def check_tree_over(fovrt, t, P, leaf_max=2):
    """The tree in use validated against positions P (the collapsed ones) and the context's own three numbers."""
    a = t.scene_arrays()
    nodes, tri, prim = bvh_np.read_tree(fovrt, t)
    return bvh_np.check_tree(nodes, tri, prim, P, a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"], leaf_max)


def untouched(t):
    a = t.scene_arrays()
    return {k: a[k].tobytes() for k in ("pos", "nrm", "bbox", "uv", "flags")}


def frame_ids(fovrt):
    TN = fovrt.TextureName
    return (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.WEIGHT, TN.MASK, TN.SHADING, TN.HISTORY_CACHE, TN.SIBSON,
            TN.ATROUS)


def assert_same_frames(fovrt, a, b, what):
    for tid in frame_ids(fovrt):
        x, y = a.read(tid), b.read(tid)
        assert equal_nan(x, y), (what, tid, mismatch_report(x, y))
    assert a.ray_count() == b.ray_count(), what


def gbuffer_with_weight(fovrt, t, uni):
    TN = fovrt.TextureName
    t.reset_accumulation()
    t.set_camera_uniforms(uni)
    t.geometry_launch()
    ids = (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.WEIGHT)
    return {name: t.read(tid) for name, tid in zip(("position", "normal", "depth", "diffuse", "weight"), ids)}


def assert_gbuffer_is_oracles(fovrt, oracle, t, arrays, ms, vis, uni, what, names=("position", "normal", "depth", "diffuse")):
    got = gbuffer_with_weight(fovrt, t, uni)
    want = oracle.gbuffer(oracle.OracleScene(rs.collapsed(arrays, ms, vis)), uni, W, H, 0)
    for k in names:
        assert equal_nan(got[k], want[k]), (what, k, mismatch_report(got[k], want[k]))


# ---------------------------------------------------------------------------------------------
# 1. Tree bytes; 2. untouched state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, LBVH, SAH])
@pytest.mark.parametrize("scene", [0, 1])
def test_refit_is_refit_np_over_the_collapsed_positions(fovrt_mod, scene, builder):
    """The bytes after fr_set_model_visibility(vis, FR_BVH_REFIT) are refit_np's of the tree before over C(P, vis). Back
    at FR_VISIBLE_ALL the tree is fr_refit_bvh's on a twin that never hid anything: in bytes on the host-built tree;
    two device builds number the nodes of a level freely (bvh_refit_np.canonical_tree), so there the twin is compared
    in canonical form and the context's own tree from before the first hide, refitted, in bytes."""
    t, twin = mk(fovrt_mod, scene, builder), mk(fovrt_mod, scene, builder, visibility=False)
    ms = t.models()
    a = t.scene_arrays()
    before_state = untouched(t)
    assert t.model_visibility() == vc.valid(ms)
    t.refit_bvh()
    own = tree_bytes(fovrt_mod, t)
    for vis in vc.tree_masks(ms):
        nodes0, _tri0, prim0 = bvh_np.read_tree(fovrt_mod, t)
        t.set_model_visibility(vis | 0xFFFF0000)  # the high bits are ignored and read back clear
        assert t.model_visibility() == vis
        nodes, tri, prim = bvh_np.read_tree(fovrt_mod, t)
        want_nodes, want_tri = refit_np(nodes0, prim0, vc.collapsed_pos(a, ms, vis))
        what = f"scene {scene} builder {builder} mask {vis:#x}"
        assert nodes.tobytes() == want_nodes.tobytes(), (what, "nodes")
        assert tri.tobytes() == want_tri.tobytes(), (what, "tri_geo")
        assert prim.tobytes() == prim0.tobytes(), (what, "prim")
        assert untouched(t) == before_state, what
        hidden = ~rs.selected(ms, vis)[prim]
        assert (tri[hidden, 9:12] == 0).all(), (what, "a hidden triangle keeps a normal")
    t.set_model_visibility(ALL)
    twin.refit_bvh()
    assert tree_bytes(fovrt_mod, t) == own
    if builder == 0:
        assert tree_bytes(fovrt_mod, t) == tree_bytes(fovrt_mod, twin)
    for x, y in zip(canonical_tree(*bvh_np.read_tree(fovrt_mod, t)), canonical_tree(*bvh_np.read_tree(fovrt_mod, twin))):
        assert x.tobytes() == y.tobytes()
    t.destroy(); twin.destroy()


@pytest.mark.parametrize("builder", [0, LBVH, SAH])
def test_rebuild_is_the_builders_tree_over_the_collapsed_positions(fovrt_mod, builder):
    """After FR_BVH_REBUILD the tree validates against C(P, vis) with the context's own numbers. The device LBVH's tree
    (builders 0 and 1 both rebuild with it) equals that of a twin handed the collapsed array through
    fr_update_positions(..., FR_BVH_REBUILD): in canonical form, since two device builds number the nodes of a level
    freely. The device SAH builder's tree is the host builder's over those positions (fr__scene_rebuild_over)."""
    scene = 1
    t, twin = mk(fovrt_mod, scene, builder), mk(fovrt_mod, scene, builder, visibility=False)
    ms = t.models()
    a = t.scene_arrays()
    before_state = untouched(t)
    host = fovrt_mod.Scene(rc.config(fovrt_mod, scene))
    v = vc.valid(ms)
    for vis in (vc.hiding(ms, ("bunny",)) & v, 2, 0, v):
        what = f"builder {builder} mask {vis:#x}"
        P = vc.collapsed_pos(a, ms, vis)
        t.set_model_visibility(vis, update="rebuild")
        assert t.model_visibility() == vis and untouched(t) == before_state, what
        if builder == SAH:
            assert scene_rebuild_over(fovrt_mod, host, P) >= 0
            leaf_max = max(2, int(bvh_np.scene_tree(fovrt_mod, host)[0]["count"].max()))
            check_tree_over(fovrt_mod, t, P, leaf_max)
            assert_tree_is_hosts(fovrt_mod, t, host, what)
        else:
            check_tree_over(fovrt_mod, t, P)
            # (a builder-0 context rebuilds with the device LBVH as well)
            twin.set_positions(P, update="rebuild")  # fr_update_positions(..., FR_BVH_REBUILD)
            ta, tb = bvh_np.read_tree(fovrt_mod, t), bvh_np.read_tree(fovrt_mod, twin)
            for name, x, y in zip(("nodes", "tri_geo", "prim"), canonical_tree(*ta), canonical_tree(*tb)):
                assert x.tobytes() == y.tobytes(), (what, name)
    t.destroy(); twin.destroy()


def test_facade_takes_names(fovrt_mod):
    t = mk(fovrt_mod, 1)
    ms = t.models()
    t.set_model_visibility(["ground", "box", "earth"])
    assert t.model_visibility() == vc.hiding(ms, ("bunny",)) & vc.valid(ms)
    t.set_model_visibility("box", update="rebuild")
    assert t.model_visibility() == 2
    with pytest.raises(ValueError):
        t.set_model_visibility(["teapot"])
    with pytest.raises(ValueError):
        t.set_model_visibility(ALL, update="rebuild", enqueue=True)
    t.set_model_visibility(ALL, enqueue=True)
    assert t.model_visibility() == vc.valid(ms)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Frames against the oracle over the collapsed arrays, with the original scene box
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["saliency", "logpolar"])
@pytest.mark.parametrize("scene,hide", [(s, h) for s in vc.FRAME_CASES for h in vc.FRAME_CASES[s]])
def test_frames_equal_the_oracle_over_the_collapsed_scene(fovrt_mod, oracle, scene, hide, mode):
    mask_mode = {"saliency": fovrt_mod.MASK_SALIENCY, "logpolar": fovrt_mod.MASK_LOGPOLAR}[mode]
    uni = vc.preset_uniforms(fovrt_mod, scene)
    for spp in (1, 4):
        t = mk(fovrt_mod, scene, mask_mode=mask_mode, spp=spp, diffuse_max_depth=3, refraction_max_depth=16)
        ms = t.models()
        vis = vc.hiding(ms, hide)
        arrays = t.scene_arrays()
        t.set_model_visibility(vis, enqueue=spp == 4)
        t.set_camera_uniforms(uni)
        c = rs.collapsed(arrays, ms, vis)
        assert c["bbox"].tobytes() == arrays["bbox"].tobytes()
        osc = oracle.OracleScene(c, refraction_max_depth=16, diffuse_max_depth=3)
        for frame in range(2):
            tag = (scene, hide, mode, spp, frame)
            t._frame = t.m_accumFrame
            t.geometry_launch()
            cls = check_gbuffer(t, oracle, osc, c, uni, W, H, frame, tag)
            if len(hide) == len(ms):
                assert (cls == 3).all(), (tag, "everything hidden is all sky")
            check_front(t, oracle, osc, uni, W, H, mask_mode, tag)
            shade_and_check(t, oracle, osc, uni, W, H, spp, str(tag))
        t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Composition with the other tree writers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
def test_every_tree_writer_reads_the_collapsed_positions(fovrt_mod, oracle, overlap):
    t = mk(fovrt_mod, 1, LBVH, overlap=overlap)
    ms = t.models()
    names = [m[0] for m in ms]
    vis = vc.hiding(ms, ("bunny",))
    uni = vc.preset_uniforms(fovrt_mod, 1)
    cv, nv = t.normal_groups()
    base = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    xyz = [dev(mild(base, f)) for f in (1, 2, 3)]
    settle()
    n = base.shape[0]
    t.set_model_visibility(vis)
    want_nrm = t.scene_arrays()["nrm"].reshape(-1, 3, 3).copy()

    def check(what, pos=None):
        a = t.scene_arrays()
        if pos is not None:
            assert a["pos"].tobytes() == np.ascontiguousarray(pos, F).tobytes(), (what, "positions")
        check_tree_over(fovrt_mod, t, vc.collapsed_pos(a, ms, vis))
        assert_same_bits(a["nrm"], want_nrm, what + ": normals")
        assert_gbuffer_is_oracles(fovrt_mod, oracle, t, a, ms, vis, uni, what)
        assert t.model_visibility() == vis & vc.valid(ms)

    check("hidden")
    for k, how in enumerate(("refit", "rebuild")):
        want_nrm = recompute_np(mild(base, k + 1), cv, nv, want_nrm)[0]
        t.set_positions_device(xyz[k].data_ptr(), n, update=how, normals="recompute")
        check(f"fr_update_geometry, {how}", mild(base, k + 1))
    want_nrm = recompute_np(mild(base, 3), cv, nv, want_nrm)[0]
    t.update_geometry_enqueue(xyz[2], normals="recompute")
    check("fr_update_geometry_enqueue", mild(base, 3))
    t.enable_model_pose()
    rest_pos, rest_nrm = mild(base, 3), want_nrm
    m = pn.identities(len(ms))
    m[names.index("bunny"), :, 3] = (0.25, 0.125, -0.5)
    m[names.index("earth"), :, 3] = (0.0, 0.1, 0.3)
    X, want_nrm = pn.pose_np(rest_pos, rest_nrm, ms, m, t.scene_arrays()["flags"])
    t.set_model_transforms(m, enqueue=True)
    check("fr_set_model_transforms_enqueue", X)
    t.rebuild_bvh_enqueue()
    check("fr_rebuild_bvh_enqueue", X)
    t.rebuild_bvh_enqueue_if(1.0)
    check("fr_rebuild_bvh_enqueue_if", X)
    t.refit_bvh()
    check("fr_refit_bvh", X)
    assert t.geometry_update_status() == (2, 0) and t.bvh_rebuild_status()[1] == 0
    t.destroy()


@pytest.mark.parametrize("overlap", [False, True])
def test_rejected_update_while_a_model_is_hidden_changes_nothing(fovrt_mod, overlap):
    a, b = mk(fovrt_mod, 1, overlap=overlap), mk(fovrt_mod, 1, overlap=overlap)
    ms = a.models()
    vis = vc.hiding(ms, ("bunny",))
    base = a.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    bad = mild(base, 1)
    bad[ms[2][1] + 7, 1, 2] = np.nan
    bad[3, 0, 0] = np.nan
    xd = dev(bad)
    settle()
    for t in (a, b):
        t.set_model_visibility(vis, enqueue=True)
        t.frame(timing=False)
    a.update_geometry_enqueue(xd, normals="recompute")
    assert a.geometry_update_status() == (0, 1)
    assert tree_bytes(fovrt_mod, a) == tree_bytes(fovrt_mod, b)
    assert untouched(a) == untouched(b)
    for t in (a, b):
        t.frame(timing=False)
    assert_same_frames(fovrt_mod, a, b, f"the frame after a rejected update, overlap={overlap}")
    a.destroy(); b.destroy()


def test_first_conditional_rebuild_after_a_visibility_change_adopts_the_baseline(fovrt_mod):
    """Scene 1, builder 2: hiding the ground halves the cost of the tree, so showing it again is growth by a factor of
    almost two; the conditional call that follows still skips, because a tree written by a visibility call came by
    another route, and takes that tree's cost for its baseline."""
    t = mk(fovrt_mod, 1, SAH)
    ms = t.models()
    tol = 1e-4  # the device's cost against fr_bvh_sah_cost (test_gpu_rebuild_policy's bar)
    t.rebuild_bvh_enqueue_if(1.2)
    e, s, last, base_all = t.bvh_rebuild_policy_status()
    assert (e, s) == (1, 1) and abs(base_all - t.bvh_sah_cost()) <= tol * base_all
    t.set_model_visibility(vc.hiding(ms, ("ground",)))
    t.rebuild_bvh_enqueue_if(1.2)
    e, s, last, base_hidden = t.bvh_rebuild_policy_status()
    assert (e, s) == (2, 2) and abs(base_hidden - t.bvh_sah_cost()) <= tol * base_hidden
    assert base_hidden * 1.2 < base_all, (base_hidden, base_all)
    t.set_model_visibility(ALL, enqueue=True)
    t.rebuild_bvh_enqueue_if(1.2)
    e, s, last, base = t.bvh_rebuild_policy_status()
    assert (e, s) == (3, 3), "showing a model looked like a tree that has grown"
    assert abs(base - base_all) <= tol * base_all and last == base
    assert t.bvh_rebuild_status() == (0, 0)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Stream order
# ---------------------------------------------------------------------------------------------
def pose_of(ms, k):
    names = [m[0] for m in ms]
    m = pn.identities(len(ms))
    m[names.index("bunny"), :, 3] = (0.25 * (k + 1), 0.125, -0.5 + 0.2 * k)
    m[names.index("earth"), :, 3] = (0.0, 0.1 * k, 0.3)
    return m


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("latency", [False, True])
def test_a_call_before_every_pipelined_frame(fovrt_mod, latency, overlap, motion):
    """hide, update, show, pose, hide two, rebuild: a enqueues each ahead of an untimed fr_frame; its twin makes the
    same sequence through the synchronous calls."""
    a = mk(fovrt_mod, 1, SAH, motion=motion, latency=latency, overlap=overlap, pose=True)
    b = mk(fovrt_mod, 1, SAH, motion=motion, latency=latency, pose=True)
    ms = a.models()
    base = a.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    xd = dev(mild(base, 1))
    settle()
    hide1, hide2 = vc.hiding(ms, ("bunny",)), vc.hiding(ms, ("box", "earth"))
    steps = [
        ("hide", lambda t, enq: t.set_model_visibility(hide1, enqueue=enq)),
        ("update", lambda t, enq: t.update_geometry_enqueue(xd, normals="recompute") if enq else
            t.set_positions_device(xd.data_ptr(), xd.shape[0], update="refit", normals="recompute")),
        ("show", lambda t, enq: t.set_model_visibility(ALL, enqueue=enq)),
        ("pose", lambda t, enq: t.set_model_transforms(pose_of(ms, 1), enqueue=enq)),
        ("hide two", lambda t, enq: t.set_model_visibility(hide2, enqueue=enq)),
        ("rebuild", lambda t, enq: t.rebuild_bvh_enqueue() if enq else t.rebuild_bvh()),
    ]
    for name, call in steps:
        call(a, True)
        a.frame(timing=False)
        call(b, False)
        b.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, f"{name}: latency={latency} overlap={overlap} motion={motion}")
    assert a.model_visibility() == b.model_visibility() == hide2 & vc.valid(ms)
    assert untouched(a) == untouched(b)
    for x, y in zip(canonical_tree(*bvh_np.read_tree(fovrt_mod, a)), canonical_tree(*bvh_np.read_tree(fovrt_mod, b))):
        assert x.tobytes() == y.tobytes()
    assert a.geometry_update_status() == (2, 0) and a.bvh_rebuild_status() == (1, 0)
    a.destroy(); b.destroy()


@pytest.mark.parametrize("overlap", [False, True])
def test_three_pairs_back_to_back_each_show_their_own_mask(fovrt_mod, overlap):
    """A context that enqueues k (visibility, frame) pairs with nothing between them ends on the twin's k-th frame,
    for k = 1, 2, 3: a frame's buffers are only the last frame's, so every prefix of the sequence runs on a context
    of its own."""
    twin = mk(fovrt_mod, 1)
    ms = twin.models()
    masks = [vc.hiding(ms, ("bunny",)), vc.hiding(ms, ("ground", "box")), vc.hiding(ms, ("earth",))]
    for k in range(3):
        twin.set_model_visibility(masks[k])
        twin.frame(timing=False)
        t = mk(fovrt_mod, 1, overlap=overlap)
        for j in range(k + 1):
            t.set_model_visibility(masks[j], enqueue=True)
            t.frame(timing=False)
        assert_same_frames(fovrt_mod, t, twin, f"{k + 1} pairs, overlap={overlap}")
        t.destroy()
    twin.destroy()


def test_weight_after_a_hide_is_the_plain_gbuffers(fovrt_mod, oracle):
    """Motion reprojection on, a position update traced, then a hide and no position update: the next G-buffer is
    the plain form over the collapsed scene, WEIGHT included (a visibility change is not a position update)."""
    t = mk(fovrt_mod, 1, motion=True)
    ms = t.models()
    uni = vc.preset_uniforms(fovrt_mod, 1)
    base = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    t.set_camera_uniforms(uni)
    t.set_positions(mild(base, 1), update="refit")
    t.geometry_launch()  # the motion form; the positions in place are now the ones the last G-buffer traced
    vis = vc.hiding(ms, ("bunny",))
    for enqueue in (True, False):
        t.set_model_visibility(vis, enqueue=enqueue)
        assert_gbuffer_is_oracles(fovrt_mod, oracle, t, t.scene_arrays(), ms, vis, uni, f"enqueue={enqueue}",
                                  names=("position", "normal", "depth", "diffuse", "weight"))
        vis = ALL
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 6. Ray queries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,hide", [(0, ("box",)), (1, ("bunny",)), (1, ("ground", "box"))])
def test_queries_see_what_frames_see(fovrt_mod, oracle, scene, hide):
    a, ms, r, masks, _plain, _brute = aimed(fovrt_mod, oracle, scene)
    cam = rc.camera_rows(fovrt_mod, {0: "box_close", 1: "bunny_close"}[scene])
    t = mk(fovrt_mod, scene, w=rc.SIZE[0], h=rc.SIZE[1])
    vis = vc.hiding(ms, hide)
    t.set_model_visibility(vis)
    nsc = tn.SceneNp(rs.collapsed(a, ms, vis))
    for rows, name in ((r, "aimed"), (cam, "camera")):
        every = np.full(len(rows), vis & vc.valid(ms), np.uint32)
        want = rs.masked_reference(oracle, a, ms, rows, every)
        for where in ("host", "device"):
            got = query(t, rows, where, "closest")
            assert rc.same_records(got, want), (name, where, report(got, want, rows))
        model = rs.model_of(ms, want["prim"])
        assert not np.isin(model, [i for i, m in enumerate(ms) if m[0] in hide]).any()
    both = masks & np.uint32(vis & vc.valid(ms))
    want = rs.masked_reference(oracle, a, ms, r, both)
    for where in ("host", "device"):
        got = query(t, r, where, "closest", masks)
        assert rc.same_records(got, want), (where, report(got, want, r))
    surf = rs.surface_np(nsc, r, want, ms)
    got = query(t, r, "device", "surface", masks)
    assert rc.same_records(got, surf), report(got, surf, r)
    # transmittance: the masked arm on the aimed set, the unmasked arm on unit directions (the shadow set)
    check_transmittance(query(t, r, "device", "transmittance", masks), rs.masked_np(a, ms, r, both, "shadow"))
    s = rc.shadow_rows(a)
    assert np.allclose(np.linalg.norm(s[:, 3:6].astype(np.float64), axis=1), 1.0, atol=1e-6)
    every = np.full(len(s), vis & vc.valid(ms), np.uint32)
    want_s = rs.masked_np(a, ms, s, every, "shadow")
    check_transmittance(query(t, s, "host", "transmittance"), want_s)
    check_transmittance(query(t, s, "device", "transmittance", rs.shadow_masks(ms, len(s))),
                        rs.masked_np(a, ms, s, rs.shadow_masks(ms, len(s)) & every, "shadow"))
    t.destroy()


@pytest.mark.parametrize("overlap", [False, True])
def test_three_enqueued_visibility_query_pairs_each_see_their_own_mask(fovrt_mod, oracle, overlap):
    a, ms, r, _masks, _plain, _brute = aimed(fovrt_mod, oracle, 1)
    r = r[::3]
    n = len(r)
    t = mk(fovrt_mod, 1, SAH, w=rc.SIZE[0], h=rc.SIZE[1], overlap=overlap)
    v = vc.valid(ms)
    masks = [vc.hiding(ms, ("bunny",)) & v, vc.hiding(ms, ("ground", "box")) & v, vc.hiding(ms, ("earth",)) & v]
    wants = [rs.masked_reference(oracle, a, ms, r, np.full(n, m, np.uint32)) for m in masks]
    assert not rc.same_records(wants[0], wants[1]) and not rc.same_records(wants[1], wants[2])
    rays = dev_any(rc.fr_rays(r))
    outs = [out_buf(n, "closest") for _ in masks]
    settle()
    for m, out in zip(masks, outs):
        t.set_model_visibility(m, enqueue=True)
        t.trace_rays_enqueue(rays, out, n=n, kind="closest")
    t.synchronize()
    for k, (out, want) in enumerate(zip(outs, wants)):
        assert rc.same_records(records(out, "closest"), want), (f"pair {k}", report(records(out, "closest"), want, r))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 7. Refusals write nothing
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_tree_and_mask_alone(fovrt_mod):
    lib = fovrt_mod.load_library()
    INVALID, STATE, UNSUPPORTED = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_STATE, fovrt_mod.FR_E_UNSUPPORTED
    REFIT, REBUILD = fovrt_mod.FR_BVH_REFIT, fovrt_mod.FR_BVH_REBUILD
    t, other = mk(fovrt_mod, 1, visibility=False), mk(fovrt_mod, 1)
    ms = t.models()
    hide = vc.hiding(ms, ("bunny",))
    v = C.c_uint32()

    def same(what, tree, mask):
        assert tree_bytes(fovrt_mod, t) == tree, what
        assert lib.fr_model_visibility(t._ctx, C.byref(v)) == 0 and v.value == mask, what

    tree = tree_bytes(fovrt_mod, t)
    every = vc.valid(ms)
    for how in (REFIT, REBUILD):
        assert lib.fr_set_model_visibility(t._ctx, hide, how) == STATE and "not enabled" in t.last_error()
    assert lib.fr_set_model_visibility_enqueue(t._ctx, hide) == STATE and "not enabled" in t.last_error()
    same("before enable", tree, every)
    assert lib.fr_model_visibility_enable(t._ctx, 2) == INVALID
    t.enable_model_visibility()
    for how in (2, -1):
        assert lib.fr_set_model_visibility(t._ctx, hide, how) == INVALID and "update kind" in t.last_error()
    assert lib.fr_model_visibility(t._ctx, None) == INVALID
    same("bad how", tree, every)
    t.set_model_visibility(hide)
    tree = tree_bytes(fovrt_mod, t)
    assert lib.fr_model_visibility_enable(t._ctx, 0) == STATE and "hidden" in t.last_error()
    same("off while a model is hidden", tree, hide & every)
    # a rank of an in-process group: the enqueued form is refused, the synchronous one works
    g = fovrt_mod.Group([t, other], views=1, tile=64)
    assert lib.fr_set_model_visibility_enqueue(t._ctx, every) == UNSUPPORTED and "group" in t.last_error()
    same("group", tree, hide & every)
    t.set_model_visibility(ALL)
    g.destroy()
    tree = tree_bytes(fovrt_mod, t)
    # a sharded context
    t.set_shard(0, 2, 32)
    assert lib.fr_set_model_visibility_enqueue(t._ctx, hide) == UNSUPPORTED and "sharded" in t.last_error()
    same("sharded", tree, every)
    # off: nothing hidden, so it is taken, and the set calls answer FR_E_STATE
    t.enable_model_visibility(False)
    assert lib.fr_set_model_visibility(t._ctx, hide, REFIT) == STATE
    assert lib.fr_set_model_visibility_enqueue(t._ctx, hide) == STATE
    same("after enable(0)", tree, every)
    t.destroy(); other.destroy()


def test_visibility_calls_allocate_nothing(fovrt_mod):
    import torch
    t = mk(fovrt_mod, 1, SAH, overlap=True)
    ms = t.models()
    masks = [vc.hiding(ms, (m[0],)) for m in ms]
    t.set_model_visibility(masks[0], enqueue=True)
    t.set_model_visibility(masks[1])
    t.set_model_visibility(masks[2], update="rebuild")
    t.synchronize()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()
    for m in masks * 3:
        t.set_model_visibility(m, enqueue=True)
    for m in masks:
        t.set_model_visibility(m)
        t.set_model_visibility(m, update="rebuild")
    t.enable_model_visibility()
    t.synchronize()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info() == before
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 8. Group
# ---------------------------------------------------------------------------------------------
def test_group_of_two_with_the_bunny_hidden_equals_the_single_context(fovrt_mod):
    import torch
    TN = fovrt_mod.TextureName
    w, h, tile = 200, 136, 64
    ranks, full = [mk(fovrt_mod, 1, w=w, h=h), mk(fovrt_mod, 1, w=w, h=h)], mk(fovrt_mod, 1, w=w, h=h)
    full.set_sample_sum(2)  # the group sums samples in fixed point
    cam = fovrt_mod.Camera.preset(1, w, h)
    g = fovrt_mod.Group(ranks, views=1, tile=tile, composite=True)
    ms = full.models()
    for t in ranks + [full]:
        t.set_model_visibility(vc.hiding(ms, ("bunny",)))
    for f in range(3):
        for t in ranks + [full]:
            t.update_optix_variables(cam)
        full.frame(timing=False)
        g.frame()
    g.synchronize()
    out = torch.empty(w * h * 4, dtype=torch.float32, device="cuda")
    g.composite(out.data_ptr(), out.numel() * 4)
    comp = out.cpu().numpy().reshape(h, w, 4)
    want = full.read(TN.ATROUS)
    assert equal_nan(comp, want), mismatch_report(comp, want)
    for t in ranks:
        assert equal_nan(t.read(TN.POSITION), full.read(TN.POSITION))
    shown = mk(fovrt_mod, 1, w=w, h=h, visibility=False)
    shown.update_optix_variables(cam)
    shown.geometry_launch()
    assert not equal_nan(shown.read(TN.POSITION), full.read(TN.POSITION)), "the bunny is not in the picture"
    g.destroy()
    for t in ranks + [full, shown]:
        t.destroy()
