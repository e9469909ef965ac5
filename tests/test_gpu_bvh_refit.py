"""GPU suite for moving geometry without a rebuild: fr_refit_bvh / fr_update_positions / fr_bvh_sah_cost.

A refit has one right answer in bytes (bvh_refit_np.refit_np, held to bvh_np.check_tree by
test_cpu_bvh_refit.py): the tree in use with its topology kept, every slot box and every leaf triangle
recomputed. The trees are read back from the device (fr__bvh_read) and compared with it, on the trees of both
builders and on bvh_cases' adversarial geometry; what the traversal computes over them is compared with the CPU
oracle, whose G-buffers are the ones test_gpu_bvh.py computes (one shared cache).
"""
import numpy as np
import pytest

import bvh_cases
import bvh_np
from bvh_refit_np import canonical_tree, refit_np, sah_cost_np
from helpers import equal_nan
from test_gpu_bvh import GBUFFER, case_reference, make_tracer, mismatch_report, tree_bytes

pytestmark = pytest.mark.gpu

NUMBERS = ("bvh_nodes", "bvh_depth", "bvh_max_stack")


def numbers(t):
    a = t.scene_arrays()
    return {k: a[k] for k in NUMBERS}


def gbuffer(fovrt, t, uni):
    """Frame 0's G-buffer from the camera `uni`: {name: array}."""
    TN = fovrt.TextureName
    t.reset_accumulation()
    assert t.m_accumFrame == 0
    t.set_camera_uniforms(uni)
    t.geometry_launch()
    return {name: t.read(tid) for name, tid in zip(GBUFFER, (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE))}


def same_gbuffer(a, b):
    return all(equal_nan(a[k], b[k]) for k in GBUFFER)


def sine(base, f, amp=0.05):
    pos = base.copy()
    pos[..., 1] += np.float32(amp) * np.sin(np.float32(3.0) * base[..., 0] + np.float32(f)).astype(np.float32)
    return pos


# ---------------------------------------------------------------------------------------------
# 1. A refit over unchanged positions changes no byte
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [0, 1, 2])
@pytest.mark.parametrize("builder", [0, 1])
def test_refit_over_unchanged_positions_is_the_identity(fovrt_mod, builder, scene):
    t = make_tracer(fovrt_mod, 64, 48, scene, builder)
    before, out = tree_bytes(fovrt_mod, t), bvh_np.check_tracer_tree(fovrt_mod, t)
    assert t.refit_bvh() > 0.0
    after = tree_bytes(fovrt_mod, t)
    for name, a, b in zip(("nodes", "tri_geo", "prim"), before, after):
        assert a == b, name
    assert bvh_np.check_tracer_tree(fovrt_mod, t) == out
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Adversarial refits: the tree against refit_np, the G-buffer over it against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(bvh_cases.CASES))
@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("scene", [0, 1])
def test_adversarial_refit_tree_and_gbuffer(fovrt_mod, oracle, scene, builder, case):
    W, H = (32, 24) if case == "identical" else (64, 48)  # identical: every ray tests every triangle
    t = make_tracer(fovrt_mod, W, H, scene, builder)
    pos, ref = case_reference(fovrt_mod, oracle, t, scene, case, W, H)
    nodes0, _, prim0 = bvh_np.read_tree(fovrt_mod, t)
    before = numbers(t)
    t.set_positions(pos, update="refit")
    assert np.array_equal(t.scene_arrays()["pos"].reshape(-1, 3, 3), pos)
    nodes, tri, prim = bvh_np.read_tree(fovrt_mod, t)
    want_nodes, want_tri = refit_np(nodes0, prim0, pos)
    assert prim.tobytes() == prim0.tobytes()
    for name in ("child", "count", "lox", "hix", "loy", "hiy", "loz", "hiz"):
        assert nodes[name].tobytes() == want_nodes[name].tobytes(), name
    assert nodes.tobytes() == want_nodes.tobytes()
    assert tri.tobytes() == want_tri.tobytes()
    out = bvh_np.check_tracer_tree(fovrt_mod, t)
    print(f"scene {scene} builder {builder} {case}: {out}")
    assert numbers(t) == before
    for pose, (uni, g) in ref.items():
        got = gbuffer(fovrt_mod, t, uni)
        for name in GBUFFER:
            assert equal_nan(got[name], g[name]), (pose, name, mismatch_report(got[name], g[name]))
    assert t.stats()["overflow"] == 0
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Refits do not drift: back at the base positions the tree is the original one
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_refit_there_and_back_is_the_original_tree(fovrt_mod, builder):
    t = make_tracer(fovrt_mod, 64, 48, 1, builder)
    base = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    original = tree_bytes(fovrt_mod, t)
    for case in ("comb", "two_scales"):
        t.set_positions(bvh_cases.CASES[case](base, 0), update="refit")
        assert tree_bytes(fovrt_mod, t) != original
    t.set_positions(base, update="refit")
    assert tree_bytes(fovrt_mod, t) == original
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. A refit before every pipelined frame gives the frames a rebuild gives (frames do not depend on the tree)
# ---------------------------------------------------------------------------------------------
def test_refit_against_rebuild_before_every_pipelined_frame(fovrt_mod):
    TN = fovrt_mod.TextureName
    W, H = 160, 96
    a = make_tracer(fovrt_mod, W, H, 1, 0, mask=4, spp=2)
    b = make_tracer(fovrt_mod, W, H, 1, 0, mask=4, spp=2)
    base = a.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    before = numbers(a)
    for f in range(6):
        pos = sine(base, f)
        a.set_positions(pos, update="refit")
        b.set_positions(pos)
        a.frame(timing=False)
        b.geometry_launch(); b.sampling_launch(); b.optimize_launch(); b.shading_launch()
        fovrt_mod.JumpFlooding(b).render(TN.SHADING)
        fovrt_mod.SibsonInterpolation(b).render()
        fovrt_mod.PullPushInterpolation(b).render(TN.SHADING)
        fovrt_mod.ATrous(b).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    for tid in (TN.SHADING, TN.HISTORY_CACHE, TN.POSITION, TN.SIBSON, TN.ATROUS):
        assert equal_nan(a.read(tid), b.read(tid)), tid
    assert np.array_equal(a.scene_arrays()["pos"].reshape(-1, 3, 3), pos)
    assert numbers(a) == before  # the host SAH tree's, six refits later
    bvh_np.check_tracer_tree(fovrt_mod, a)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Positions from device memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update", ["rebuild", "refit"])
@pytest.mark.parametrize("builder", [0, 1])
def test_positions_from_device_memory(fovrt_mod, builder, update):
    import torch
    W, H = 64, 48
    a = make_tracer(fovrt_mod, W, H, 1, builder)
    b = make_tracer(fovrt_mod, W, H, 1, builder)
    base = a.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    pos = sine(base, 1.0, amp=0.2)
    n = pos.shape[0]
    dev = torch.from_numpy(pos.reshape(-1, 9)).to("cuda:0")
    torch.cuda.synchronize()
    nodes0, _, prim0 = bvh_np.read_tree(fovrt_mod, a)
    a.set_positions_device(dev.data_ptr(), n, update=update)
    b.set_positions(pos, update=update)
    # the twins' trees are the same tree; where the device LBVH made either (builder 1, a rebuild), equal up to
    # the node numbering its atomic counter handed out
    ta, tb = bvh_np.read_tree(fovrt_mod, a), bvh_np.read_tree(fovrt_mod, b)
    if builder == 0 and update == "refit":
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ta, tb))
    for name, x, y in zip(("nodes", "tri_geo", "prim"), canonical_tree(*ta), canonical_tree(*tb)):
        assert x.tobytes() == y.tobytes(), name
    if update == "refit":  # and the one right answer over this context's own tree
        want_nodes, want_tri = refit_np(nodes0, prim0, pos)
        assert ta[0].tobytes() == want_nodes.tobytes() and ta[1].tobytes() == want_tri.tobytes()
        assert ta[2].tobytes() == prim0.tobytes()
    uni = fovrt_mod.Camera.preset(1, W, H).uniforms(W, H)
    ga, gb = gbuffer(fovrt_mod, a, uni), gbuffer(fovrt_mod, b, uni)
    for name in GBUFFER:
        assert equal_nan(ga[name], gb[name]), (name, mismatch_report(ga[name], gb[name]))
    arrays = a.scene_arrays()  # the host mirror, fetched on demand
    assert np.array_equal(arrays["pos"].reshape(-1, 3, 3), pos)
    flat = pos.reshape(-1, 3)
    assert (np.asarray(arrays["bbox"]) == np.concatenate([flat.min(0), flat.max(0)])).all()
    assert (np.asarray(arrays["bbox"]) == np.asarray(b.scene_arrays()["bbox"])).all()
    bvh_np.check_tracer_tree(fovrt_mod, a)
    # a rejected update after device positions (no host mirror to fall back on) leaves them in place
    bad = dev.clone()
    bad[n // 3, 4] = float("inf")
    torch.cuda.synchronize()
    kept = tree_bytes(fovrt_mod, a)
    with pytest.raises(fovrt_mod.FovrtError) as e:
        a.set_positions_device(bad.data_ptr(), n, update=update)
    assert e.value.code == fovrt_mod.FR_E_INVALID
    assert tree_bytes(fovrt_mod, a) == kept
    assert np.array_equal(a.scene_arrays()["pos"].reshape(-1, 3, 3), pos)
    assert same_gbuffer(gbuffer(fovrt_mod, a, uni), ga)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 6. Rejected updates leave everything alone
# ---------------------------------------------------------------------------------------------
def _nan_positions(t):
    bad = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    bad[bad.shape[0] // 2, 1, 2] = np.nan
    return bad


def _reject_device_nan(fovrt, t, update):
    import torch
    bad = _nan_positions(t)
    dev = torch.from_numpy(bad.reshape(-1, 9)).to("cuda:0")
    torch.cuda.synchronize()
    t.set_positions_device(dev.data_ptr(), bad.shape[0], update=update)


def _reject_host_nan_refit(fovrt, t):
    t.set_positions(_nan_positions(t), update="refit")


def _reject_wrong_ntris(fovrt, t):
    pos = t.scene_arrays()["pos"].reshape(-1, 3, 3)
    t.set_positions(pos[:-1], update="refit")


def _reject_wrong_ntris_device(fovrt, t):
    import torch
    pos = t.scene_arrays()["pos"].reshape(-1, 9)
    dev = torch.from_numpy(pos.copy()).to("cuda:0")
    torch.cuda.synchronize()
    t.set_positions_device(dev.data_ptr(), pos.shape[0] - 1, update="rebuild")


def _reject_bad_how(fovrt, t):
    t.set_positions(t.scene_arrays()["pos"], update=2)


def _reject_bad_where(fovrt, t):
    import ctypes as C
    pos = np.ascontiguousarray(t.scene_arrays()["pos"], np.float32)
    t._check(fovrt.load_library().fr_update_positions(t._ctx, C.c_void_p(pos.ctypes.data), pos.size // 9, 2,
                                                      fovrt.FR_BVH_REFIT))


REJECTS = {"device_nan_refit": lambda f, t: _reject_device_nan(f, t, "refit"),
           "device_nan_rebuild": lambda f, t: _reject_device_nan(f, t, "rebuild"),
           "host_nan_refit": _reject_host_nan_refit, "wrong_ntris": _reject_wrong_ntris,
           "wrong_ntris_device": _reject_wrong_ntris_device, "bad_how": _reject_bad_how, "bad_where": _reject_bad_where}


@pytest.mark.parametrize("trigger", sorted(REJECTS))
@pytest.mark.parametrize("builder", [0, 1])
def test_rejected_updates_leave_everything_alone(fovrt_mod, builder, trigger):
    W, H = 64, 48
    t = make_tracer(fovrt_mod, W, H, 1, builder)
    uni = fovrt_mod.Camera.preset(1, W, H).uniforms(W, H)
    g0 = gbuffer(fovrt_mod, t, uni)
    tree0 = tree_bytes(fovrt_mod, t)
    a0 = t.scene_arrays()
    pos0, box0, num0 = a0["pos"].copy(), np.array(a0["bbox"]).copy(), numbers(t)
    with pytest.raises(fovrt_mod.FovrtError) as e:
        REJECTS[trigger](fovrt_mod, t)
    assert e.value.code == fovrt_mod.FR_E_INVALID
    assert tree_bytes(fovrt_mod, t) == tree0
    a1 = t.scene_arrays()
    assert a1["pos"].tobytes() == pos0.tobytes()
    assert np.array(a1["bbox"]).tobytes() == box0.tobytes()
    assert numbers(t) == num0
    bvh_np.check_tracer_tree(fovrt_mod, t)
    assert same_gbuffer(gbuffer(fovrt_mod, t, uni), g0)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 7. The SAH cost of the tree in use
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("scene", [0, 1])
def test_sah_cost_matches_numpy_and_grows_under_the_comb(fovrt_mod, scene, builder):
    """1e-4 relative: each area costs a few f32 ulps (6e-8 each), the f32 tree reduction over at most ~3e5
    positive terms about 25 * 2^-24 = 1.5e-6, the final float a half ulp; a wrong weight or a missed slot
    moves the cost by far more."""
    t = make_tracer(fovrt_mod, 64, 48, scene, builder)
    base = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()

    def both():
        got, want = t.bvh_sah_cost(), sah_cost_np(bvh_np.read_tree(fovrt_mod, t)[0])
        print(f"scene {scene} builder {builder}: cost {got!r}, numpy {want!r}")
        assert abs(got - want) <= 1e-4 * want, (got, want)
        return got

    before = both()
    assert both() == before  # the same tree, the same number (no atomics in arbitrary order)
    t.set_positions(bvh_cases.CASES["comb"](base, 0), update="refit")
    after = both()
    assert after > before, (before, after)
    t.destroy()
