"""GPU suite for motion reprojection (fr_set_motion_reprojection): the first G-buffer after a position update
reprojects each hit point from where its triangle was when the previous G-buffer traced it, and that frame's
sampling stage tests the history depth against that point.

The rule has one right answer in bytes: tests/motion_np.py restates it on trace_np's brute-force scene
(test_cpu_motion.py holds it to the plain restatements where nothing moved). The restatement of a case is computed
once and shared by the tests that need it. Everything else is compared with a context that has the feature off, or
with the CPU oracle over the new positions."""
import numpy as np
import pytest

import motion_np as mn
import trace_np as tn
from helpers import equal_nan
from test_gpu_bvh import GBUFFER, make_tracer, mismatch_report

pytestmark = pytest.mark.gpu

BOX_SIZE = (45, 29)    # partial 8x8 G-buffer tiles and partial 16x16 sampling blocks on both axes, several blocks
BUNNY_SIZE = (37, 27)  # (brute force over the reduced bunny's 9,106 triangles: ~4 ms a pixel)
MISS = np.array([-1, -1, 0, 1], np.float32)


def stages(t):
    t.geometry_launch(); t.sampling_launch(); t.optimize_launch(); t.shading_launch()


def tracer(fovrt, W, H, scene, builder=0, motion=True, **kw):
    t = make_tracer(fovrt, W, H, scene, builder, **kw)
    if motion:
        t.set_motion_reprojection(True)
    return t


_refs = {}


def reference(fovrt, t, scene, case, panned):
    """(prev, cur, uniforms of the two frames, the restatement of the second frame's G-buffer WEIGHT) of a case."""
    key = (scene, case, panned)
    if key not in _refs:
        arrays = t.scene_arrays()
        base = arrays["pos"].reshape(-1, 3, 3)
        W, H = BOX_SIZE if scene == 0 else BUNNY_SIZE
        if case == "sine":
            prev, cur = base.copy(), mn.sine(base, 1.0)
            uni1, uni2 = mn.cameras(fovrt, scene, W, H, panned)
        elif case == "translate":
            W, H = mn.TRANSLATE_SIZE
            prev, cur = mn.translate_case(base)
            uni1, uni2 = mn.cameras(fovrt, scene, W, H, False, shift=mn.TRANSLATE)
        else:
            prev, cur = mn.box_case(base, case)
            uni1, uni2 = mn.cameras(fovrt, scene, W, H, panned)
        arrays["pos"] = cur.reshape(-1, 9)
        ref = mn.motion_gbuffer_np(tn.SceneNp(arrays), prev, uni2, W, H, count_ties=(case == "tie"))
        for v in (prev, cur, *ref.values()):
            v.setflags(write=False)
        _refs[key] = (prev, cur, uni1, uni2, ref, arrays)
    return _refs[key]


def report(got, want):
    return mismatch_report(np.asarray(got), np.asarray(want))


# ---------------------------------------------------------------------------------------------
# 1. The rule, bit for bit
# ---------------------------------------------------------------------------------------------
RULE_CASES = [(0, "small"), (0, "far"), (0, "behind"), (0, "tie"), (1, "sine")]


@pytest.mark.parametrize("panned", [False, True], ids=["still", "panned"])
@pytest.mark.parametrize("scene,case", RULE_CASES)
def test_motion_gbuffer_and_sampling_match_the_restatement(fovrt_mod, oracle, scene, case, panned):
    TN = fovrt_mod.TextureName
    W, H = BOX_SIZE if scene == 0 else BUNNY_SIZE
    builder = int(panned)  # both builders, and both kinds of update, over the cases
    t = tracer(fovrt_mod, W, H, scene, builder)
    prev, cur, uni1, uni2, ref, arrays = reference(fovrt_mod, t, scene, case, panned)
    t.set_positions(prev, update="refit")
    t.set_camera_uniforms(uni1)
    stages(t)  # the frame before: its depth is the next frame's DEPTH_CACHE
    t.set_positions(cur, update="rebuild" if case in ("far", "sine") else "refit")
    t.set_camera_uniforms(uni2)
    frame = t.m_accumFrame
    t.geometry_launch()
    got = t.read(TN.WEIGHT)
    want = ref["weight"]
    hit = ref["prim"] >= 0
    moved_tri = (prev != cur).any((1, 2))
    moved = hit & moved_tri[np.maximum(ref["prim"], 0)]
    print(f"scene {scene} {case} panned {panned}: hit {int(hit.sum())} moved {int(moved.sum())} of {W * H}")
    assert hit.any() and (~hit).any() and moved.any()
    assert equal_nan(got, want), report(got, want)
    # the other G-buffer outputs do not know about the motion: the oracle's over the new positions
    osc = oracle.OracleScene(arrays)
    og = oracle.gbuffer(osc, uni2, W, H, frame)
    for name, tid in zip(GBUFFER, (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE)):
        assert equal_nan(t.read(tid), og[name]), (name, report(t.read(tid), og[name]))
    # a triangle that did not move and a miss carry the oracle's reprojection bits
    still = hit & ~moved
    if case != "sine":
        assert still.any()
    assert got[still][:, (0, 1, 3)].tobytes() == og["weight"][still][:, (0, 1, 3)].tobytes()
    assert (got[~hit] == MISS).all() and got[~hit].tobytes() == og["weight"][~hit].tobytes()
    if case == "far":  # every reprojection of the box left the screen
        assert ((want[moved][:, 0] >= W) | (want[moved][:, 0] < 0)).all()
    if case == "tie":  # the face the camera sees is doubled: the lowest primitive's motion is the one applied
        assert ref["ties"].any() and set(np.unique(ref["prim"][ref["ties"]])) <= {10, 11}
    depth_cache = t.read(TN.DEPTH_CACHE)
    t.sampling_launch()
    got2 = t.read(TN.WEIGHT)
    want2 = mn.motion_sampling_weight_np(want, depth_cache)
    assert equal_nan(got2, want2), report(got2, want2)
    os_ = oracle.sampling(osc, uni2, W, H, 1, og["position"], og["depth"], depth_cache, og["weight"], og["normal"],
                          og["diffuse"])["weight"]
    keep = still | ~hit
    assert got2[keep].tobytes() == os_[keep].tobytes()
    valid = got2[..., 2] > 0
    print(f"  valid: moved {int((valid & moved).sum())}/{int(moved.sum())} still {int((valid & still).sum())}/"
          f"{int(still.sum())}")
    if case in ("far", "behind"):
        assert not (valid & moved).any()
    # (how many moved pixels stay valid is the depth test's business: |difference| < 1e-3 against the depth stored at
    # the rounded reprojection, so on a slanted face only reprojections close to a pixel centre pass, as under a
    # camera pan; test_translated_scene_and_camera_keep_their_history is the case where all of them do)
    assert t.stats()["overflow"] == 0
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. The state machine
# ---------------------------------------------------------------------------------------------
def _nan(pos):
    bad = pos.copy()
    bad[bad.shape[0] // 2, 1, 2] = np.nan
    return bad


@pytest.mark.parametrize("variant", ["three_updates", "rejected_update", "device_refit"])
def test_previous_positions_are_the_last_gbuffers(fovrt_mod, variant):
    """Whatever happens between two G-buffers, prev is what the first one traced: A -> B -> C gives prev = A, a
    rejected update changes nothing, positions from device memory behave like the host's."""
    TN = fovrt_mod.TextureName
    W, H = BOX_SIZE
    t = tracer(fovrt_mod, W, H, 0)
    A, C, uni1, uni2, ref, _ = reference(fovrt_mod, t, 0, "small", False)
    B = mn.box_case(A, "far")[0]
    t.set_positions(A, update="refit")
    t.set_camera_uniforms(uni1)
    stages(t)
    if variant == "three_updates":
        t.set_positions(B, update="refit")
        t.set_positions(C, update="rebuild")
    elif variant == "rejected_update":
        t.set_positions(C, update="refit")
        for update in ("refit", "rebuild"):
            with pytest.raises(fovrt_mod.FovrtError) as e:
                t.set_positions(_nan(B), update=update)
            assert e.value.code == fovrt_mod.FR_E_INVALID
    else:
        import torch
        dev = torch.from_numpy(np.array(C, np.float32).reshape(-1, 9)).to("cuda:0")
        torch.cuda.synchronize()
        t.set_positions_device(dev.data_ptr(), C.shape[0], update="refit")
    t.set_camera_uniforms(uni2)
    t.geometry_launch()
    got = t.read(TN.WEIGHT)
    assert equal_nan(got, ref["weight"]), report(got, ref["weight"])
    depth_cache = t.read(TN.DEPTH_CACHE)
    t.sampling_launch()
    want2 = mn.motion_sampling_weight_np(ref["weight"], depth_cache)
    assert equal_nan(t.read(TN.WEIGHT), want2), report(t.read(TN.WEIGHT), want2)
    t.destroy()


FRAME_BUFFERS = ("POSITION", "NORMAL", "DEPTH", "DIFFUSE", "WEIGHT", "MASK", "GCLASS", "SHADING", "HISTORY_CACHE",
                 "DEPTH_CACHE", "EXTRA", "JFA_COLOR", "SIBSON", "PULLPUSH", "ATROUS")


def test_without_a_pending_update_the_frames_are_the_plain_ones(fovrt_mod):
    """A second G-buffer with no update, a motion dropped by on = 0, and three whole frames with the feature on
    and nothing moving: each equals a context with the feature off, bit for bit."""
    TN = fovrt_mod.TextureName
    W, H = BOX_SIZE
    on, off = tracer(fovrt_mod, W, H, 0), tracer(fovrt_mod, W, H, 0, motion=False)
    A, C, uni1, uni2, ref, _ = reference(fovrt_mod, on, 0, "small", False)
    gb = (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.WEIGHT, TN.GCLASS)

    def same(ids, what):
        for tid in ids:
            a, b = on.read(tid), off.read(tid)
            assert equal_nan(a, b), (what, tid, report(a, b))

    for t in (on, off):
        t.set_positions(A, update="refit")
        t.set_camera_uniforms(uni1)
        stages(t)
        t.set_positions(C, update="refit")
        t.set_camera_uniforms(uni2)
        stages(t)  # (with the feature on, the motion frame)
    assert not equal_nan(on.read(TN.WEIGHT), off.read(TN.WEIGHT))  # the box kept its history on one of them only
    for t in (on, off):  # no update since: the plain kernels on both
        t.geometry_launch()
    same(gb, "second G-buffer")
    for t in (on, off):
        t.sampling_launch()
    same(gb + (TN.MASK,), "second sampling")
    for t in (on, off):  # a pending motion dropped by on = 0
        t.optimize_launch(); t.shading_launch()
        t.set_positions(A, update="refit")
    on.set_motion_reprojection(False)
    on.set_motion_reprojection(True)
    for t in (on, off):
        t.geometry_launch()
    same(gb, "dropped motion")
    for t in (on, off):
        t.sampling_launch()
    same(gb + (TN.MASK,), "dropped motion, sampling")
    for t in (on, off):  # three whole frames, nothing moving
        t.optimize_launch(); t.shading_launch()
        for _ in range(3):
            t.frame(timing=False)
    same([getattr(TN, n) for n in FRAME_BUFFERS], "three frames")
    # and the entry's argument checks
    with pytest.raises(fovrt_mod.FovrtError) as e:
        on._check(fovrt_mod.load_library().fr_set_motion_reprojection(on._ctx, 2))
    assert e.value.code == fovrt_mod.FR_E_INVALID
    on.destroy(); off.destroy()


# ---------------------------------------------------------------------------------------------
# 3. It does what it is for
# ---------------------------------------------------------------------------------------------
def test_translated_scene_and_camera_keep_their_history(fovrt_mod):
    """The whole scene and the camera move by one vector between two frames: with the feature on the history
    survives on at least 99 % of the hit pixels (the restatement alone meets that: test_cpu_motion.py), with it off
    on fewer than half; and the frame that follows carries history exactly where the validity says so."""
    TN = fovrt_mod.TextureName
    W, H = mn.TRANSLATE_SIZE
    on, off = tracer(fovrt_mod, W, H, 0), tracer(fovrt_mod, W, H, 0, motion=False)
    before, after, uni1, uni2, ref, _ = reference(fovrt_mod, on, 0, "translate", False)
    hit = ref["prim"] >= 0
    out = {}
    for name, t in (("on", on), ("off", off)):
        t.set_positions(before, update="rebuild")
        t.set_camera_uniforms(uni1)
        t.frame(timing=False)
        depth_cache = t.read(TN.DEPTH_CACHE)
        hist = np.full((H, W, 4), 0.5, np.float32)
        hist[..., 3] = 1.0
        t.write(TN.HISTORY_CACHE, hist)  # every pixel has a history to lose
        t.set_positions(after, update="refit")
        t.set_camera_uniforms(uni2)
        t.frame(timing=False)
        out[name] = (t.read(TN.WEIGHT), t.read(TN.MASK), t.read(TN.HISTORY_CACHE), depth_cache)
    weight, mask, history, depth_cache = out["on"]
    want = mn.motion_sampling_weight_np(ref["weight"], depth_cache)
    frac = float((want[..., 2][hit] > 0).mean())
    print(f"hit {int(hit.sum())}, restatement valid {frac:.4f}")
    assert frac >= 0.99
    assert equal_nan(weight, want), report(weight, want)
    lost = float((out["off"][0][..., 2][hit] == 0).mean())
    print(f"feature off: invalid on {lost:.4f} of the hit pixels")
    assert lost > 0.5
    untraced = hit & (mask == 0)
    assert untraced.sum() > 20
    assert np.array_equal(history[..., 3][untraced] > 0, weight[..., 2][untraced] == 1)
    on.destroy(); off.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Pipelined frames and a group
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["throughput", "latency"])
def test_update_before_every_pipelined_frame(fovrt_mod, mode):
    TN = fovrt_mod.TextureName
    W, H = 160, 96
    a = tracer(fovrt_mod, W, H, 1, mask=4, spp=2)
    b = tracer(fovrt_mod, W, H, 1, mask=4, spp=2)
    if mode == "latency":
        a.set_pipeline_mode(fovrt_mod.PIPELINE_LATENCY)
    base = a.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    for f in range(6):
        pos = mn.sine(base, f)
        for t in (a, b):
            t.set_positions(pos, update="refit")
        a.frame(timing=False)
        stages(b)
        fovrt_mod.JumpFlooding(b).render(TN.SHADING)
        fovrt_mod.SibsonInterpolation(b).render()
        fovrt_mod.PullPushInterpolation(b).render(TN.SHADING)
        fovrt_mod.ATrous(b).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    for tid in (TN.SHADING, TN.HISTORY_CACHE, TN.WEIGHT, TN.SIBSON, TN.ATROUS):
        assert equal_nan(a.read(tid), b.read(tid)), (tid, report(a.read(tid), b.read(tid)))
    print(f"{mode}: valid history on {int((a.read(TN.WEIGHT)[..., 2] > 0).sum())} of {W * H} pixels")
    a.destroy(); b.destroy()


def test_group_of_two_equals_the_single_context(fovrt_mod):
    """One in-process group of two ranks, a still camera, the default tile-local front: every rank's context is
    switched on and updated by its caller, and the group's frames are the single context's."""
    TN = fovrt_mod.TextureName
    W, H, tile = 200, 136, 64
    mk = lambda: tracer(fovrt_mod, W, H, 1, mask=4, spp=2)
    ranks, full = [mk(), mk()], mk()
    full.set_sample_sum(2)  # the group sums samples in fixed point
    cam = fovrt_mod.Camera.preset(1, W, H)
    g = fovrt_mod.Group(ranks, views=1, tile=tile)
    base = full.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    for f in range(4):
        pos = mn.sine(base, f)
        for t in ranks + [full]:
            t.set_positions(pos, update="refit")
            t.update_optix_variables(cam)
        full.frame(timing=False)
        g.frame()
    g.synchronize()
    jfa_rank, at_rank = g.output_ranks(0)
    for r, t in enumerate(ranks):
        assert g.rank_info(r)["chains"]
        for tid in (TN.WEIGHT, TN.SHADING, TN.HISTORY_CACHE):
            assert equal_nan(t.read(tid), full.read(tid)), (r, tid, report(t.read(tid), full.read(tid)))
    assert equal_nan(ranks[jfa_rank].read(TN.SIBSON), full.read(TN.SIBSON))
    assert equal_nan(ranks[at_rank].read(TN.ATROUS), full.read(TN.ATROUS))
    g.destroy()
    for t in ranks + [full]:
        t.destroy()
