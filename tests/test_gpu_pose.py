"""GPU suite for model poses: fr_model_pose_enable / fr_set_model_transforms / fr_set_model_transforms_enqueue.

Two references, both in bytes. pose_np (numpy, one rounded operation at a time) says what the posed positions and
normals are; the calls that exist say what a context does with them: a posed context equals a second context that
is handed pose_np's arrays through fr_update_geometry or fr_update_geometry_enqueue. Small shapes throughout:
scene 0 is 14 triangles in 2 models (one wave, the model edge inside it), scene 1 at detail 1 has 4 models over
several blocks with no model edge on a block boundary; screens of 64 x 48."""
import ctypes as C

import numpy as np
import pytest

import bvh_np
import pose_np as pn
from bvh_refit_np import canonical_tree
from helpers import equal_nan
from test_gpu_bvh import GBUFFER, make_tracer, mismatch_report, tree_bytes
from test_gpu_normals import assert_same_bits, gbuffer
from test_gpu_update_enqueue import assert_same_state, dev, settle, state, sync_frame

pytestmark = pytest.mark.gpu

W, H = 64, 48
F = np.float32


def frame_bufs(fovrt):
    TN = fovrt.TextureName
    return (TN.POSITION, TN.NORMAL, TN.SHADING, TN.HISTORY_CACHE, TN.WEIGHT, TN.SIBSON, TN.ATROUS)


def mk(fovrt, scene=1, builder=0, motion=False, latency=False, pose=True):
    t = make_tracer(fovrt, W, H, scene, builder, mask=4, spp=2)
    if motion:
        t.set_motion_reprojection(True)
    if latency:
        t.set_pipeline_mode(fovrt.PIPELINE_LATENCY)
    if pose:
        t.enable_model_pose()
    return t


def rest(t):
    a = t.scene_arrays()
    return a["pos"].reshape(-1, 3, 3).copy(), a["nrm"].reshape(-1, 3, 3).copy(), a


def centre(pos, model):
    _, first, n = model
    p = pos[first:first + n].reshape(-1, 3).astype(np.float64)
    return 0.5 * (p.min(0) + p.max(0))


def matrix(kind, pos, model, f=0):
    """One model's matrix of a kind, for frame f."""
    if kind == "identity":
        return pn.identities(1)[0]
    if kind == "translate":  # A is the identity, the matrix is not
        return pn.about(np.eye(3), (0, 0, 0), (0.05 + 0.03 * f, 0.02 * f, -0.04))
    if kind == "wild":  # a rotation with a non-uniform scale, about the model's middle
        A = pn.rotation(1, 17.0 + 9.0 * f).astype(np.float64) @ pn.rotation(0, -8.0).astype(np.float64)
        return pn.about(A @ np.diag([1.1, 0.9, 1.05]), centre(pos, model), (0.0, 0.03, 0.0))
    if kind == "quarter":  # 90 degrees: exact zeros in A
        return pn.about(pn.rotation(2 if f % 2 == 0 else 1, 90.0), centre(pos, model), (0.01 * f, 0.0, 0.0))
    raise KeyError(kind)


KINDS = {
    "box_wild": {"ground": "identity", "box": "wild"},
    "box_quarter": {"ground": "translate", "box": "quarter"},
    "four": {"ground": "identity", "box": "translate", "bunny": "wild", "earth": "quarter"},
    "turning": {"ground": "identity", "box": "translate", "bunny": "wild", "earth": "identity"},
}


def pose(kinds, pos, models, f=0):
    return np.stack([matrix(KINDS[kinds][m[0]], pos, m, f) for m in models]).astype(F)


def assert_same_frames(fovrt, a, b, what):
    for tid in frame_bufs(fovrt):
        x, y = a.read(tid), b.read(tid)
        assert equal_nan(x, y), (what, tid, mismatch_report(x, y))


def assert_scene_is(t, X, N, what):
    a = t.scene_arrays()
    assert_same_bits(a["pos"], X, what + ": positions")
    assert_same_bits(a["nrm"], N, what + ": normals")


# ---------------------------------------------------------------------------------------------
# 0. The context's model table is the host scene's
# ---------------------------------------------------------------------------------------------
def test_context_model_table(fovrt_mod):
    t = mk(fovrt_mod, scene=1, pose=False)
    models = t.models()
    assert [m[0] for m in models] == ["ground", "box", "bunny", "earth"]
    assert models[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(models, models[1:]))
    assert models[-1][1] + models[-1][2] == t.scene_arrays()["flags"].shape[0]
    lib = fovrt_mod.load_library()
    name, n = C.c_char_p(), C.c_int()
    for i in (-1, 4):
        assert lib.fr_model_info(t._ctx, i, C.byref(name), None, C.byref(n)) == fovrt_mod.FR_E_INVALID
    # the shapes this suite relies on: a model edge inside a wave, several blocks, no edge on a block boundary
    assert len(models) == 4 and 3 * models[-1][1] > 2 * 256
    assert all((3 * first) % 64 != 0 for _, first, _ in models[1:])
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 1. Bytes of the rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,kinds", [(0, "box_wild"), (0, "box_quarter"), (1, "four")])
def test_posed_arrays_equal_numpy(fovrt_mod, scene, kinds):
    t = mk(fovrt_mod, scene)
    pos0, nrm0, a0 = rest(t)
    models = t.models()
    if scene == 0:
        assert models == [("ground", 0, 2), ("box", 2, 12)]
    assert np.array_equal(t.model_transforms(), pn.identities(len(models)))
    for f, enqueue in ((0, False), (1, True), (2, False)):  # every pose starts from rest
        m = pose(kinds, pos0, models, f)
        X, N = pn.pose_np(pos0, nrm0, models, m, a0["flags"])
        t.set_model_transforms(m, enqueue=enqueue)
        assert_scene_is(t, X, N, f"{kinds} frame {f}")
        assert t.model_transforms().tobytes() == m.tobytes()
        for (name, first, n), M in zip(models, m):
            same = X[first:first + n].tobytes() == pos0[first:first + n].tobytes()
            assert same == pn.is_identity(M), name  # the identity model keeps its rest bits, the others move
        got = t.scene_arrays()
        assert got["uv"].tobytes() == a0["uv"].tobytes() and got["flags"].tobytes() == a0["flags"].tobytes()
    bvh_np.check_tracer_tree(fovrt_mod, t)
    assert t.geometry_update_status() == (1, 0)
    # the (nmodels, 12) shape, and back to rest: every byte as it was
    t.set_model_transforms(pn.identities(len(models)).reshape(-1, 12))
    assert_scene_is(t, pos0, nrm0, "identities")
    t.destroy()


def test_identity_model_keeps_a_negative_zero(fovrt_mod):
    t = mk(fovrt_mod, 0, pose=False)
    pos0, nrm0, a0 = rest(t)
    models = t.models()
    pos0[0, 1, 1] = F(-0.0)  # a ground corner
    pos0[5, 2, 0] = F(-0.0)  # a box corner
    t.set_positions(pos0, update="refit")
    t.enable_model_pose()
    m = pose("box_wild", pos0, models)
    m[0, 1, 0] = F(-0.0)  # still the identity
    X, N = pn.pose_np(pos0, nrm0, models, m, a0["flags"])
    t.set_model_transforms(m)
    got = t.scene_arrays()["pos"].reshape(-1, 3, 3)
    assert_same_bits(got, X, "negative zero")
    assert np.signbit(got[0, 1, 1]) and got[0, 1, 1] == 0
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Equality with the existing update
# ---------------------------------------------------------------------------------------------
_oracle_ref = {}


def oracle_gbuffer(fovrt, oracle, arrays, X, N, scene, kinds):
    """The oracle's frame-0 G-buffer over (X, N) from the preset camera, once per pose."""
    key = (scene, kinds)
    if key not in _oracle_ref:
        osc = oracle.OracleScene(dict(arrays, pos=X.reshape(-1, 9), nrm=N.reshape(-1, 9)))
        uni = fovrt.Camera.preset(scene, W, H).uniforms(W, H)
        _oracle_ref[key] = (uni, oracle.gbuffer(osc, uni, W, H, 0))
    return _oracle_ref[key]


@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("scene,kinds", [(0, "box_wild"), (1, "four")])
def test_pose_equals_update_geometry(fovrt_mod, oracle, scene, kinds, builder):
    a, b = mk(fovrt_mod, scene, builder), mk(fovrt_mod, scene, builder, pose=False)
    pos0, nrm0, a0 = rest(a)
    models = a.models()
    ntris = pos0.shape[0]
    for f, how in ((0, "refit"), (1, "rebuild")):
        m = pose(kinds, pos0, models, f)
        X, N = pn.pose_np(pos0, nrm0, models, m, a0["flags"])
        dX, dN = dev(X), dev(N)
        settle()
        a.set_model_transforms(m, update=how)
        b.set_positions_device(dX.data_ptr(), ntris, update=how, normals=dN.data_ptr())
        what = f"scene {scene} builder {builder} {how}"
        assert_same_state(fovrt_mod, a, b, what, tree=False)
        ta, tb = bvh_np.read_tree(fovrt_mod, a), bvh_np.read_tree(fovrt_mod, b)
        # two device builds of the same triangles number the nodes of a level freely (bvh_refit_np.canonical_tree):
        # the host builder's refitted tree is compared as it is, every tree in its canonical form
        exact = builder == 0 and how == "refit"
        if exact:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(ta, tb)), what
        for name, x, y in zip(("nodes", "tri_geo", "prim"), canonical_tree(*ta), canonical_tree(*tb)):
            assert x.tobytes() == y.tobytes(), (what, name)
        ca, cb = a.bvh_sah_cost(), b.bvh_sah_cost()
        # (the cost is a float32 sum over the nodes in index order: the same bytes where the order is the same,
        # and within the rounding of two orders of n positive terms, n 2^-23 relative, where it is free)
        assert ca == cb if exact else abs(ca - cb) <= ta[0].shape[0] * 2.0 ** -23 * cb, (what, ca, cb)
        for k in range(2):
            a.frame(timing=False)
            b.frame(timing=False)
            assert_same_frames(fovrt_mod, a, b, f"{what} frame {k}")
        if how == "refit":
            uni, want = oracle_gbuffer(fovrt_mod, oracle, a0, X, N, scene, kinds)
            got = gbuffer(fovrt_mod, a, uni)
            for name in GBUFFER:
                assert equal_nan(got[name], want[name]), (what, name, mismatch_report(got[name], want[name]))
            gbuffer(fovrt_mod, b, uni)  # b goes the same way, so that the next frames still compare
    assert a.geometry_update_status() == (0, 0)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Stream order
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("latency", [False, True])
def test_pose_before_every_pipelined_frame(fovrt_mod, latency, motion):
    """a: a pose enqueued before each untimed fr_frame; b: synchronous poses and stage calls; c: pose_np's arrays
    through fr_update_geometry_enqueue."""
    a = mk(fovrt_mod, 1, motion=motion, latency=latency)
    b = mk(fovrt_mod, 1, motion=motion)
    c = mk(fovrt_mod, 1, motion=motion, latency=latency, pose=False)
    pos0, nrm0, a0 = rest(a)
    models = a.models()
    ms = [pose("turning", pos0, models, f) for f in range(4)]
    arrays = [pn.pose_np(pos0, nrm0, models, m, a0["flags"]) for m in ms]
    dXN = [(dev(X), dev(N)) for X, N in arrays]
    settle()
    what = f"latency={latency} motion={motion}"
    for f in range(4):
        a.set_model_transforms(ms[f], enqueue=True)
        a.frame(timing=False)
        b.set_model_transforms(ms[f], update="refit")
        sync_frame(fovrt_mod, b)
        c.update_geometry_enqueue(dXN[f][0], normals=dXN[f][1])
        c.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, f"{what} frame {f}: enqueued and synchronous poses")
        assert_same_frames(fovrt_mod, a, c, f"{what} frame {f}: enqueued pose and enqueued arrays")
    assert a.geometry_update_status() == (4, 0)
    assert b.geometry_update_status() == (0, 0)
    assert_same_state(fovrt_mod, a, b, what)
    assert_same_state(fovrt_mod, a, c, what)
    assert_scene_is(a, *arrays[3], what)
    a.destroy(); b.destroy(); c.destroy()


def test_pose_after_a_synchronous_update_starts_from_rest(fovrt_mod):
    a, b = mk(fovrt_mod, 1, motion=True), mk(fovrt_mod, 1, motion=True, pose=False)
    pos0, nrm0, a0 = rest(a)
    models = a.models()
    ms = [pose("turning", pos0, models, f) for f in range(2)]
    arrays = [pn.pose_np(pos0, nrm0, models, m, a0["flags"]) for m in ms]
    dXN = [(dev(X), dev(N)) for X, N in arrays]
    bent = pos0.copy()
    bent[..., 1] += F(0.05) * np.sin(F(3.0) * pos0[..., 0]).astype(F)
    settle()
    for t in (a, b):
        if t is a:
            t.set_model_transforms(ms[0], enqueue=True)
        else:
            t.update_geometry_enqueue(dXN[0][0], normals=dXN[0][1])
        t.frame(timing=False)
        t.set_positions(bent, update="refit")  # fr_update_positions: normals kept
        t.frame(timing=False)
        if t is a:
            t.set_model_transforms(ms[1], enqueue=True)
        else:
            t.update_geometry_enqueue(dXN[1][0], normals=dXN[1][1])
        t.frame(timing=False)
    assert_same_frames(fovrt_mod, a, b, "pose, update, pose")
    assert_same_state(fovrt_mod, a, b, "pose, update, pose")
    assert_scene_is(a, *arrays[1], "the second pose is over the rest geometry, not over the bent one")
    assert a.geometry_update_status() == (2, 0)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Recapture
# ---------------------------------------------------------------------------------------------
def test_enable_again_captures_the_deformed_mesh(fovrt_mod):
    t = mk(fovrt_mod, 1)
    pos0, nrm0, a0 = rest(t)
    models = t.models()
    _, first, n = models[2]
    assert models[2][0] == "bunny"
    bent = pos0.copy()
    bent[first:first + n, :, 1] += F(0.05) * np.sin(F(9.0) * pos0[first:first + n, :, 0]).astype(F)
    t.set_model_transforms(pose("four", pos0, models))  # a pose is in place when the mesh is deformed
    t.set_positions(bent, update="refit")
    t.enable_model_pose()
    assert np.array_equal(t.model_transforms(), pn.identities(len(models)))
    before = state(fovrt_mod, t)
    t.set_model_transforms(pn.identities(len(models)))
    assert state(fovrt_mod, t) == before, "an identity pose over the captured mesh changes no byte"
    # the captured normals are the ones in place: the first pose's
    nrm1 = np.frombuffer(before["nrm"], F).reshape(-1, 3, 3)
    assert nrm1.tobytes() == pn.pose_np(pos0, nrm0, models, pose("four", pos0, models), a0["flags"])[1].tobytes()
    m = np.stack([matrix("translate", bent, mod, 2) for mod in models]).astype(F)
    X, N = pn.pose_np(bent, nrm1, models, m, a0["flags"])
    t.set_model_transforms(m, enqueue=True)
    assert_scene_is(t, X, N, "translated, deformed")
    assert not np.array_equal(X[first:first + n], pn.pose_np(pos0, nrm0, models, m)[0][first:first + n])
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Refusals change nothing
# ---------------------------------------------------------------------------------------------
def overflowing(pos0, models):
    """Finite, det = 100, and the ground's |x| of 10 times 1e38 is past float32."""
    m = pn.identities(len(models))
    m[0] = np.array([[1e38, 0, 0, 0], [0, 1e-18, 0, 0], [0, 0, 1e-18, 0]], F)
    assert np.isfinite(m).all() and np.isfinite(pn.cofactors(m[0])[1]) and pn.cofactors(m[0])[1] > 0
    with np.errstate(all="ignore"):
        X, N = pn.pose_np(pos0, np.zeros_like(pos0), models, m)
    assert np.isinf(X).any() and np.isfinite(N).all()
    return m


def test_refused_poses_change_nothing(fovrt_mod):
    lib = fovrt_mod.load_library()
    INVALID, STATE, UNSUPPORTED = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_STATE, fovrt_mod.FR_E_UNSUPPORTED
    REFIT = fovrt_mod.FR_BVH_REFIT
    t, twin = mk(fovrt_mod, 1, pose=False), mk(fovrt_mod, 1, pose=False)
    pos0, _, _ = rest(t)
    models = t.models()
    nm = len(models)
    good = pose("four", pos0, models)

    def p(m):
        return None if m is None else m.ctypes.data_as(C.POINTER(C.c_float))

    def both(m, n, code, what, says):
        assert lib.fr_set_model_transforms(t._ctx, p(m), n, REFIT) == code, what
        assert says in t.last_error(), (what, t.last_error())
        assert lib.fr_set_model_transforms_enqueue(t._ctx, p(m), n) == code, what
        assert says in t.last_error(), (what, t.last_error())
        assert_same_state(fovrt_mod, t, twin, what)
        assert t.geometry_update_status() == twin.geometry_update_status(), what

    for x in (t, twin):
        x.frame(timing=False)
    out = np.empty((nm, 3, 4), F)
    both(good, nm, STATE, "before enable", "not enabled")
    assert lib.fr_model_transforms(t._ctx, p(out), nm) == STATE
    t.enable_model_pose()
    both(good, nm - 1, INVALID, "one model too few", "model count")
    both(np.concatenate([good, good[:1]]), nm + 1, INVALID, "one model too many", "model count")
    both(None, nm, INVALID, "NULL matrices", "NULL")
    bad = good.copy(); bad[2, 1, 3] = np.nan
    both(bad, nm, INVALID, "a NaN translation", "not finite")
    bad = good.copy(); bad[3, 0, 0] = np.inf
    both(bad, nm, INVALID, "an infinite entry", "not finite")
    bad = good.copy(); bad[1, :, :3] = np.diag([1.0, 0.0, 1.0])
    both(bad, nm, INVALID, "det = 0", "determinant not positive")
    bad = good.copy(); bad[1, :, :3] = np.diag([1.0, -1.0, 1.0])
    both(bad, nm, INVALID, "det < 0", "determinant not positive")
    for how in (2, -1):
        assert lib.fr_set_model_transforms(t._ctx, p(good), nm, how) == INVALID
        assert "update kind" in t.last_error()
        assert_same_state(fovrt_mod, t, twin, "bad how")
    assert lib.fr_model_transforms(t._ctx, p(out), nm - 1) == INVALID
    assert lib.fr_model_transforms(t._ctx, p(out), nm) == 0 and np.array_equal(out, pn.identities(nm))
    # rejected on the device: finite inputs to a checked path
    big = overflowing(pos0, models)
    for how in (REFIT, fovrt_mod.FR_BVH_REBUILD):
        assert lib.fr_set_model_transforms(t._ctx, p(big), nm, how) == INVALID
        assert "position not finite" in t.last_error(), t.last_error()
        assert_same_state(fovrt_mod, t, twin, "overflow, synchronous")
    assert lib.fr_set_model_transforms_enqueue(t._ctx, p(big), nm) == 0
    assert t.geometry_update_status() == (0, 1)
    assert_same_state(fovrt_mod, t, twin, "overflow, enqueued")
    for x in (t, twin):
        x.frame(timing=False)
    assert_same_frames(fovrt_mod, t, twin, "the frame after the refused poses")
    t.enable_model_pose(False)
    assert lib.fr_set_model_transforms(t._ctx, p(good), nm, REFIT) == STATE
    assert lib.fr_set_model_transforms_enqueue(t._ctx, p(good), nm) == STATE
    assert_same_state(fovrt_mod, t, twin, "after enable(0)")
    assert lib.fr_model_pose_enable(t._ctx, 2) == INVALID
    # a sharded context: the enqueued form is refused, the synchronous one works
    t.enable_model_pose()
    for x in (t, twin):
        x.set_shard(0, 2, 32)
    assert lib.fr_set_model_transforms_enqueue(t._ctx, p(good), nm) == UNSUPPORTED
    assert "sharded" in t.last_error()
    assert t.geometry_update_status() == (0, 1)
    assert_same_state(fovrt_mod, t, twin, "sharded")
    for x in (t, twin):
        x.frame(timing=False)
    assert_same_frames(fovrt_mod, t, twin, "the frame after the refusal on a sharded context")
    t.set_model_transforms(good)  # and a good pose is taken
    assert not np.array_equal(t.scene_arrays()["pos"], twin.scene_arrays()["pos"])
    t.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 6. No allocation per call
# ---------------------------------------------------------------------------------------------
def test_poses_allocate_nothing(fovrt_mod):
    import torch
    t = mk(fovrt_mod, 1)
    pos0, _, _ = rest(t)
    models = t.models()
    ms = [pose("turning", pos0, models, f) for f in range(10)]
    t.set_model_transforms(ms[0], enqueue=True)
    t.set_model_transforms(ms[1])
    t.set_model_transforms(ms[1], update="rebuild")
    t.synchronize()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()
    for m in ms:
        t.set_model_transforms(m, enqueue=True)
    for m in ms:
        t.set_model_transforms(m)
    t.synchronize()
    assert t.geometry_update_status() == (11, 0)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info() == before
    t.destroy()
