"""GPU suite for shading normals that follow moving geometry: fr_update_geometry / fr_set_normals /
fr_recompute_normals.

A recompute has one right answer in bytes (normals_np.recompute_np over the weld test_cpu_normals.py holds to
numpy): the exported normals are compared with it on a smooth deformation, on bvh_cases' adversarial geometry
(triangles shuffled under the fixed weld, collapsed triangles) and on mirrored_pairs, which together take both
fallbacks of the rule. What the traversal computes over the new normals is compared with the CPU oracle over the
same arrays.
"""
import ctypes as C

import numpy as np
import pytest

import bvh_cases
import bvh_np
from bvh_refit_np import canonical_tree
from helpers import equal_nan, rmse_per_channel
from normals_np import mirrored_pairs, recompute_np, weld_np
from test_gpu_bvh import GBUFFER, make_tracer, mismatch_report, tree_bytes

pytestmark = pytest.mark.gpu

F = np.float32


def sine(base, f, amp=0.05):
    """test_gpu_bvh_refit.py's smooth deformation."""
    pos = base.copy()
    pos[..., 1] += F(amp) * np.sin(F(3.0) * base[..., 0] + F(f)).astype(F)
    return pos


CASES = dict(bvh_cases.CASES, sine=lambda base, seed: sine(base, 1.0), mirrored_pairs=mirrored_pairs)

_rest, _refs = {}, {}


def rest(t, scene):
    """The scene as built (shared, read-only): arrays, base positions, rest normals, weld."""
    if scene not in _rest:
        a = t.scene_arrays()
        cv, nv = weld_np(a["pos"], a["nrm"], a["flags"])
        for v in (a["pos"], a["nrm"], a["uv"], a["flags"], cv):
            v.setflags(write=False)
        _rest[scene] = (a, a["pos"].reshape(-1, 3, 3), a["nrm"].reshape(-1, 3, 3), cv, nv)
    return _rest[scene]


def reference(fovrt, oracle, t, scene, case, W, H, with_gbuffer=True):
    """(positions, numpy normals, fallback counts, {pose: (uniforms, frame-0 oracle G-buffer)}) of a case, once
    per (scene, case, size), shared by both builders and by the tests."""
    key = (scene, case, W, H)
    if key not in _refs or (with_gbuffer and _refs[key][3] is None):
        a, base, nrm0, cv, nv = rest(t, scene)
        pos = CASES[case](base, 0)
        nrm, counts = recompute_np(pos, cv, nv, nrm0)
        ref = None
        if with_gbuffer:
            arrays = dict(a, pos=pos.reshape(-1, 9), nrm=nrm.reshape(-1, 9))
            osc = oracle.OracleScene(arrays)
            ref = {}
            for name, cam in bvh_cases.poses(fovrt, scene, a["bbox"], W, H).items():
                uni = cam.uniforms(W, H)
                g = oracle.gbuffer(osc, uni, W, H, 0)
                for v in g.values():
                    v.setflags(write=False)
                ref[name] = (uni, g)
        pos.setflags(write=False)
        nrm.setflags(write=False)
        _refs[key] = (pos, nrm, counts, ref)
    return _refs[key]


def gbuffer(fovrt, t, uni):
    TN = fovrt.TextureName
    t.reset_accumulation()
    assert t.m_accumFrame == 0
    t.set_camera_uniforms(uni)
    t.geometry_launch()
    return {name: t.read(tid) for name, tid in zip(GBUFFER, (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE))}


def same_gbuffer(a, b):
    return all(equal_nan(a[k], b[k]) for k in GBUFFER)


def size_of(case):
    return (32, 24) if case == "identical" else (64, 48)  # identical: every ray tests every triangle


def nrm_of(t):
    return t.scene_arrays()["nrm"].reshape(-1, 3, 3)


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, F).reshape(-1, 3), np.ascontiguousarray(want, F).reshape(-1, 3)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    assert bad.size == 0, (what, f"{bad.size} corners differ; first {bad[:5].tolist()}: gpu {got[bad[0]]} "
                                 f"numpy {want[bad[0]]}")


# ---------------------------------------------------------------------------------------------
# 0. The context's weld is the host scene's
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [0, 1, 2])
def test_context_weld_equals_numpy(fovrt_mod, scene):
    t = make_tracer(fovrt_mod, 64, 48, scene, 0)
    _, _, _, cv, nv = rest(t, scene)
    got_cv, got_nv = t.normal_groups()
    assert got_nv == nv and np.array_equal(got_cv, cv)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 1. Recompute after a refit equals the numpy rule, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("scene", [0, 1])
def test_recompute_after_refit_equals_numpy(fovrt_mod, oracle, scene, builder, case):
    W, H = size_of(case)
    t = make_tracer(fovrt_mod, W, H, scene, builder)
    a = rest(t, scene)[0]
    pos, nrm, counts, _ = reference(fovrt_mod, oracle, t, scene, case, W, H, with_gbuffer=False)
    t.set_positions(pos, update="refit", normals="recompute")
    got = t.scene_arrays()
    print(f"scene {scene} builder {builder} {case}: corners (vertex, own triangle, kept) = {counts}")
    assert np.array_equal(got["pos"].reshape(-1, 3, 3), pos)
    assert_same_bits(got["nrm"], nrm, case)
    assert got["uv"].tobytes() == a["uv"].tobytes() and got["flags"].tobytes() == a["flags"].tobytes()
    t.destroy()


def test_cases_reach_both_fallbacks(fovrt_mod, oracle):
    """From numpy: the geometry of test 1 takes the vertex normal, the own triangle's and the kept one."""
    reached = np.zeros(3, np.int64)
    for scene in (0, 1):
        t = make_tracer(fovrt_mod, 32, 24, scene, 0)
        for case in sorted(CASES):
            reached += reference(fovrt_mod, oracle, t, scene, case, *size_of(case), with_gbuffer=False)[2]
        t.destroy()
    assert (reached > 0).all(), reached


def test_recompute_on_the_poles_and_across_models(fovrt_mod, oracle):
    """Scene 2: valence 64 at the sphere poles, five models under one weld."""
    t = make_tracer(fovrt_mod, 64, 48, 2, 0)
    a, base, nrm0, cv, nv = rest(t, 2)
    assert np.bincount(cv[cv >= 0]).max() == 64
    pos = sine(base, 1.0)
    want, counts = recompute_np(pos, cv, nv, nrm0)
    t.set_positions(pos, update="refit", normals="recompute")
    got = t.scene_arrays()
    assert_same_bits(got["nrm"], want, "scene 2 sine")
    assert got["uv"].tobytes() == a["uv"].tobytes() and got["flags"].tobytes() == a["flags"].tobytes()
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. The G-buffer over the recomputed normals against the oracle, every pixel, three poses
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sine", "degenerate_mix", "mirrored_pairs", "pairs"])
@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("scene", [0, 1])
def test_gbuffer_over_recomputed_normals_equals_oracle(fovrt_mod, oracle, scene, builder, case):
    W, H = size_of(case)
    t = make_tracer(fovrt_mod, W, H, scene, builder)
    pos, nrm, _, ref = reference(fovrt_mod, oracle, t, scene, case, W, H)
    t.set_positions(pos, update="refit", normals="recompute")
    for pose, (uni, g) in ref.items():
        got = gbuffer(fovrt_mod, t, uni)
        for name in GBUFFER:
            assert equal_nan(got[name], g[name]), (pose, name, mismatch_report(got[name], g[name]))
    assert t.stats()["overflow"] == 0
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Shading over a deformed pose with recomputed normals (the README's 1e-3 per-channel RMSE)
# ---------------------------------------------------------------------------------------------
def test_shading_over_recomputed_normals_within_tolerance(fovrt_mod, oracle):
    TN = fovrt_mod.TextureName
    W, H, spp, dmd = 64, 48, 4, 3
    t = make_tracer(fovrt_mod, W, H, 1, 0, mask=1, spp=spp, dmd=dmd)
    _, base, nrm0, cv, nv = rest(t, 1)
    pos = sine(base, 1.0, amp=0.2)
    t.set_positions(pos, update="refit", normals="recompute")
    arrays = t.scene_arrays()
    assert_same_bits(arrays["nrm"], recompute_np(pos, cv, nv, nrm0)[0], "sine 0.2")
    uni = fovrt_mod.Camera.preset(1, W, H).uniforms(W, H)
    t.set_camera_uniforms(uni)
    osc = oracle.OracleScene(arrays, refraction_max_depth=16, diffuse_max_depth=dmd)
    frame = t.m_accumFrame
    t.geometry_launch()
    t.sampling_launch()
    t.optimize_launch()
    mask, weight, hist_in = t.read(TN.MASK), t.read(TN.WEIGHT), t.read(TN.HISTORY_CACHE)
    t.shading_launch()
    got = t.read(TN.SHADING)
    ref = oracle.shading(osc, uni, W, H, frame, spp, mask, weight, hist_in)["shading"]
    rm = rmse_per_channel(got, ref)
    print(f"shading rmse {rm.tolist()}, {int(mask.sum())} traced pixels")
    assert mask.sum() > 0
    assert (rm <= 1e-3).all(), (rm, mismatch_report(got, ref))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Given normals, from host and from device memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_given_normals_from_host_and_device(fovrt_mod, oracle, builder):
    import torch
    TN = fovrt_mod.TextureName
    W, H, scene = 64, 48, 1
    r, h, d, u = (make_tracer(fovrt_mod, W, H, scene, builder) for _ in range(4))
    a = rest(r, scene)[0]
    pos, nrm, _, _ = reference(fovrt_mod, oracle, r, scene, "sine", W, H, with_gbuffer=False)
    n = pos.shape[0]
    uni = fovrt_mod.Camera.preset(scene, W, H).uniforms(W, H)
    r.set_positions(pos, update="refit", normals="recompute")
    want_g = gbuffer(fovrt_mod, r, uni)
    # set_positions, then set_normals from the host
    h.set_positions(pos, update="refit")
    assert_same_bits(nrm_of(h), a["nrm"], "kept")
    h.set_normals(nrm)
    # set_positions, then set_normals from device memory
    dev = torch.from_numpy(np.ascontiguousarray(nrm).reshape(-1, 9).copy()).to("cuda:0")
    dpos = torch.from_numpy(np.ascontiguousarray(pos).reshape(-1, 9).copy()).to("cuda:0")
    torch.cuda.synchronize()
    d.set_positions(pos, update="refit")
    d.set_normals_device(dev.data_ptr(), n)
    # both arrays in one fr_update_geometry, from device memory
    u.set_positions_device(dpos.data_ptr(), n, update="refit", normals=dev.data_ptr())
    for name, t in (("host", h), ("device", d), ("update_geometry", u)):
        assert_same_bits(nrm_of(t), nrm, name)
        got = gbuffer(fovrt_mod, t, uni)
        for k in GBUFFER:
            assert equal_nan(got[k], want_g[k]), (name, k, mismatch_report(got[k], want_g[k]))
    # and in one call from host memory
    u.set_positions(np.asarray(a["pos"]), update="rebuild", normals=np.asarray(a["nrm"]))
    assert_same_bits(nrm_of(u), a["nrm"], "host update_geometry")
    assert u.scene_arrays()["pos"].tobytes() == a["pos"].tobytes()
    # arbitrary finite normals change nrm alone
    rng = np.random.default_rng(7)
    wild = rng.uniform(-3, 3, nrm.shape).astype(F)
    tree0 = tree_bytes(fovrt_mod, h)
    h.set_normals(wild)
    got = h.scene_arrays()
    assert_same_bits(got["nrm"], wild, "arbitrary")
    assert got["uv"].tobytes() == a["uv"].tobytes() and got["flags"].tobytes() == a["flags"].tobytes()
    assert np.array_equal(got["pos"].reshape(-1, 3, 3), pos) and tree_bytes(fovrt_mod, h) == tree0
    g = gbuffer(fovrt_mod, h, uni)
    assert equal_nan(g["diffuse"], want_g["diffuse"])
    assert not equal_nan(g["normal"], want_g["normal"])
    for t in (r, h, d, u):
        t.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Rejected updates change nothing
# ---------------------------------------------------------------------------------------------
def _update_geometry(fovrt, t, xyz, nrm, ntris, where, how, normals):
    def ptr(v):
        if v is None:
            return None
        return C.c_void_p(v.ctypes.data if isinstance(v, np.ndarray) else v.data_ptr())
    t._check(fovrt.load_library().fr_update_geometry(t._ctx, ptr(xyz), ptr(nrm), ntris, where, how, normals))


def _poisoned(good, nan_at):
    bad = np.ascontiguousarray(good, F).reshape(-1, 9).copy()
    bad[nan_at] = np.nan
    return bad


def _device(v):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(v, F).reshape(-1, 9).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return d


def _reject(fovrt, t, pos, nrm, trigger, how):
    n = pos.shape[0]
    HOST, DEV, GIVEN = fovrt.FR_MEM_HOST, fovrt.FR_MEM_DEVICE, fovrt.FR_NORMALS_GIVEN
    pos9, nrm9 = pos.reshape(-1, 9), nrm.reshape(-1, 9)
    if trigger == "nan_normal_host":
        _update_geometry(fovrt, t, pos9, _poisoned(nrm, (n // 2, 4)), n, HOST, how, GIVEN)
    elif trigger == "nan_normal_device":
        _update_geometry(fovrt, t, _device(pos9), _device(_poisoned(nrm, (n // 2, 4))), n, DEV, how, GIVEN)
    elif trigger == "nan_position_host":
        _update_geometry(fovrt, t, _poisoned(pos, (n // 3, 7)), nrm9, n, HOST, how, GIVEN)
    elif trigger == "nan_position_device":
        _update_geometry(fovrt, t, _device(_poisoned(pos, (n // 3, 7))), _device(nrm9), n, DEV, how, GIVEN)
    elif trigger == "wrong_ntris":
        _update_geometry(fovrt, t, pos9, nrm9, n - 1, HOST, how, GIVEN)
    elif trigger == "bad_normals_value":
        _update_geometry(fovrt, t, pos9, nrm9, n, HOST, how, 3)
    elif trigger == "given_with_null":
        _update_geometry(fovrt, t, pos9, None, n, HOST, how, GIVEN)
    elif trigger == "given_with_null_device":
        _update_geometry(fovrt, t, _device(pos9), None, n, DEV, how, GIVEN)
    else:
        raise KeyError(trigger)


TRIGGERS = ("nan_normal_host", "nan_normal_device", "nan_position_host", "nan_position_device", "wrong_ntris",
            "bad_normals_value", "given_with_null", "given_with_null_device")


@pytest.mark.parametrize("builder", [0, 1])
def test_rejected_updates_change_nothing(fovrt_mod, oracle, builder):
    W, H, scene = 64, 48, 1
    t = make_tracer(fovrt_mod, W, H, scene, builder)
    _, base, nrm0, cv, nv = rest(t, scene)
    uni = fovrt_mod.Camera.preset(scene, W, H).uniforms(W, H)
    # a state no mirror holds: positions and normals last written on the device
    first = sine(base, 2.0, amp=0.1)
    dev = _device(first)
    t.set_positions_device(dev.data_ptr(), first.shape[0], update="refit", normals="recompute")
    g0, tree0, a0 = gbuffer(fovrt_mod, t, uni), tree_bytes(fovrt_mod, t), t.scene_arrays()
    pos, nrm, _, _ = reference(fovrt_mod, oracle, t, scene, "sine", W, H, with_gbuffer=False)
    for trigger in TRIGGERS:
        for how in (fovrt_mod.FR_BVH_REFIT, fovrt_mod.FR_BVH_REBUILD):
            with pytest.raises(fovrt_mod.FovrtError) as e:
                _reject(fovrt_mod, t, pos, nrm, trigger, how)
            assert e.value.code == fovrt_mod.FR_E_INVALID, (trigger, how, str(e.value))
            assert tree_bytes(fovrt_mod, t) == tree0, (trigger, how)
            a1 = t.scene_arrays()
            for k in ("pos", "nrm", "bbox", "uv", "flags"):
                assert np.asarray(a1[k]).tobytes() == np.asarray(a0[k]).tobytes(), (trigger, how, k)
            assert same_gbuffer(gbuffer(fovrt_mod, t, uni), g0), (trigger, how)
    # and the same arrays, unpoisoned, are taken
    _update_geometry(fovrt_mod, t, pos.reshape(-1, 9), nrm.reshape(-1, 9), pos.shape[0], fovrt_mod.FR_MEM_HOST,
                     fovrt_mod.FR_BVH_REFIT, fovrt_mod.FR_NORMALS_GIVEN)
    assert_same_bits(nrm_of(t), nrm, "accepted")
    bvh_np.check_tracer_tree(fovrt_mod, t)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 6. FR_NORMALS_KEEP is fr_update_positions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["refit", "rebuild"])
@pytest.mark.parametrize("builder", [0, 1])
def test_keep_is_update_positions(fovrt_mod, builder, how):
    TN = fovrt_mod.TextureName
    W, H, scene = 64, 48, 1
    a = make_tracer(fovrt_mod, W, H, scene, builder, mask=1, spp=2)
    b = make_tracer(fovrt_mod, W, H, scene, builder, mask=1, spp=2)
    base, nrm0 = rest(a, scene)[1:3]
    pos = sine(base, 1.0, amp=0.2)
    kind = a._update_kind(how)
    _update_geometry(fovrt_mod, a, pos.reshape(-1, 9), None, pos.shape[0], fovrt_mod.FR_MEM_HOST, kind,
                     fovrt_mod.FR_NORMALS_KEEP)
    b._check(fovrt_mod.load_library().fr_update_positions(b._ctx, C.c_void_p(pos.ctypes.data), pos.shape[0],
                                                          fovrt_mod.FR_MEM_HOST, kind))
    ta, tb = bvh_np.read_tree(fovrt_mod, a), bvh_np.read_tree(fovrt_mod, b)
    if builder == 0 and how == "refit":
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ta, tb))
    for name, x, y in zip(("nodes", "tri_geo", "prim"), canonical_tree(*ta), canonical_tree(*tb)):
        assert x.tobytes() == y.tobytes(), name
    for t in (a, b):
        assert_same_bits(nrm_of(t), nrm0, "kept")
        assert np.array_equal(t.scene_arrays()["pos"].reshape(-1, 3, 3), pos)
    uni = fovrt_mod.Camera.preset(scene, W, H).uniforms(W, H)
    for t in (a, b):
        t.set_camera_uniforms(uni)
        t.geometry_launch(); t.sampling_launch(); t.optimize_launch(); t.shading_launch()
    for tid in (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.MASK, TN.SHADING, TN.HISTORY_CACHE):
        assert equal_nan(a.read(tid), b.read(tid)), tid
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 7. No drift: normals are a function of the positions alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_recompute_does_not_drift(fovrt_mod, builder):
    scene = 1
    a = make_tracer(fovrt_mod, 64, 48, scene, builder)
    b = make_tracer(fovrt_mod, 64, 48, scene, builder)
    _, base, nrm0, cv, nv = rest(a, scene)
    assert b.recompute_normals() > 0.0
    direct = nrm_of(b)
    assert_same_bits(direct, recompute_np(base, cv, nv, nrm0)[0], "base")
    for f in (0.5, 2.5):
        a.set_positions(sine(base, f, amp=0.3), update="refit", normals="recompute")
        assert nrm_of(a).tobytes() != direct.tobytes()
    a.set_positions(base, update="refit", normals="recompute")
    assert_same_bits(nrm_of(a), direct, "there and back")
    assert a.recompute_normals() > 0.0
    assert_same_bits(nrm_of(a), direct, "twice")
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 8. An update with recompute before every pipelined frame: the ordering against frames in flight
# ---------------------------------------------------------------------------------------------
def test_recompute_before_every_pipelined_frame(fovrt_mod):
    TN = fovrt_mod.TextureName
    W, H, scene = 160, 96, 1
    a = make_tracer(fovrt_mod, W, H, scene, 0, mask=4, spp=2)
    b = make_tracer(fovrt_mod, W, H, scene, 0, mask=4, spp=2)
    _, base, nrm0, cv, nv = rest(a, scene)
    n = base.shape[0]
    nrm = nrm0
    for f in range(6):
        pos = sine(base, f)
        nrm = recompute_np(pos, cv, nv, nrm)[0]
        dev = _device(pos)
        a.set_positions_device(dev.data_ptr(), n, "refit", "recompute")
        b.set_positions(pos, update="refit")
        b.set_normals(nrm)
        a.frame(timing=False)
        b.geometry_launch(); b.sampling_launch(); b.optimize_launch(); b.shading_launch()
        fovrt_mod.JumpFlooding(b).render(TN.SHADING)
        fovrt_mod.SibsonInterpolation(b).render()
        fovrt_mod.PullPushInterpolation(b).render(TN.SHADING)
        fovrt_mod.ATrous(b).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    for tid in (TN.SHADING, TN.HISTORY_CACHE, TN.POSITION, TN.NORMAL, TN.SIBSON, TN.ATROUS):
        assert equal_nan(a.read(tid), b.read(tid)), tid
    assert_same_bits(nrm_of(a), nrm, "six updates")
    assert np.array_equal(a.scene_arrays()["pos"].reshape(-1, 3, 3), pos)
    a.destroy(); b.destroy()
