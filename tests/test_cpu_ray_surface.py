"""The cases of tests/ray_surface_cases.py are what they claim, on the references alone, before the GPU suite trusts
them: the collapsed-scene reference agrees with itself on three paths and never answers with an excluded triangle; the
aimed set sees through, loses and keeps hits in the numbers the masks need; surface_np reproduces the oracle's
G-buffer on camera rays; the masked transmittance set holds all three answers. And the host side of the ABI: the
record layout, the symbols, the facade's kinds, the refusals that need no context."""
import ctypes as C

import numpy as np
import pytest

import ray_cases as rc
import ray_surface_cases as rs
import trace_cases as tc
import trace_np as tn

_AIMED = {}


def aimed(fovrt, oracle, scene):
    """(arrays, models, rows, masks, unmasked brute-force records, masked brute-force records), computed once."""
    if scene not in _AIMED:
        a, ms = rc.scene_arrays(fovrt, scene), rs.models(fovrt, scene)
        r, masks = rs.aimed_rows(a, ms)
        plain = rc.hit_records(oracle.OracleScene(a).closest(r, brute=True))
        _AIMED[scene] = (a, ms, r, masks, plain, rs.masked_reference(oracle, a, ms, r, masks))
    return _AIMED[scene]


def test_symbols_and_record_sizes(fovrt_mod):
    lib = fovrt_mod.load_library()
    for s in ("fr_trace_rays_masked", "fr_trace_rays_masked_enqueue", "fr_ray_query_reserve_kind"):
        assert hasattr(lib, s) and s in fovrt_mod._SIGS, s
    assert fovrt_mod.FR_RAYS_SURFACE == 2
    assert C.sizeof(fovrt_mod.fr_ray_surface) == 80 and fovrt_mod.RAY_SURFACE_DTYPE.itemsize == 80
    assert fovrt_mod.RAY_SURFACE_DTYPE == rs.SURFACE_DTYPE
    for name, off in rs.OFFSETS.items():
        assert getattr(fovrt_mod.fr_ray_surface, name).offset == off, name
        assert fovrt_mod.RAY_SURFACE_DTYPE.fields[name][1] == off, name
    assert list(fovrt_mod.RAY_SURFACE_DTYPE.names) == list(rs.OFFSETS)


def test_facade_knows_the_surface_kind_and_masks(fovrt_mod):
    import inspect
    assert fovrt_mod.RAY_KINDS["surface"] == fovrt_mod.FR_RAYS_SURFACE
    assert fovrt_mod.PathTracer._ray_kind("surface") == 2 and fovrt_mod.PathTracer._ray_kind(2) == 2
    with pytest.raises(ValueError):
        fovrt_mod.PathTracer._ray_kind("normals")
    for m in ("trace_rays", "trace_rays_enqueue"):
        assert "masks" in inspect.signature(getattr(fovrt_mod.PathTracer, m)).parameters, m
    assert callable(fovrt_mod.PathTracer.ray_query_reserve_kind)


def test_null_context_is_refused(fovrt_mod):
    lib = fovrt_mod.load_library()
    rays = rc.fr_rays(rc.rows([[0, 1, 0]], [[0, -1, 0]]))
    masks = np.array([1], np.uint32)
    out = np.full(20, 7.0, np.float32)
    E = fovrt_mod.FR_E_INVALID
    p = C.c_void_p
    assert lib.fr_ray_query_reserve_kind(None, 16, 2, 1) == E
    for kind in (0, 1, 2):
        assert lib.fr_trace_rays_masked(None, p(rays.ctypes.data), p(masks.ctypes.data), 1, 0, kind,
                                        p(out.ctypes.data)) == E
        assert lib.fr_trace_rays_masked_enqueue(None, p(rays.ctypes.data), p(masks.ctypes.data), 1, kind,
                                                p(out.ctypes.data), None) == E
    assert (out == 7.0).all()


@pytest.mark.parametrize("scene", [0, 1])
def test_masked_references_agree_on_the_aimed_set(fovrt_mod, oracle, scene):
    a, ms, r, masks, plain, brute = aimed(fovrt_mod, oracle, scene)
    assert len(r) == 150 * len(ms) and len(ms) == (2, 4)[scene]
    assert rc.same_records(rs.masked_reference(oracle, a, ms, r, masks, brute=False), brute)
    assert rc.same_records(rs.masked_np(a, ms, r, masks), brute)
    hit = brute["prim"] >= 0
    model = rs.model_of(ms, brute["prim"])
    assert ((masks[hit] >> model[hit].astype(np.uint32)) & 1).all(), "an answer lies in an excluded model"
    # a ray whose unmasked hit is in a selected model keeps that record
    pm = rs.model_of(ms, plain["prim"])
    keep = (plain["prim"] >= 0) & (((masks >> np.maximum(pm, 0).astype(np.uint32)) & 1) == 1)
    assert keep.sum() >= 50 and rc.same_records(brute[keep], plain[keep])
    # bits above the model count change nothing
    high = masks | np.uint32(0xFFFF0000)
    assert rc.same_records(rs.masked_reference(oracle, a, ms, r, high), brute)


@pytest.mark.parametrize("scene", [0, 1])
def test_the_aimed_set_is_worth_its_name(fovrt_mod, oracle, scene):
    _a, ms, _r, masks, plain, brute = aimed(fovrt_mod, oracle, scene)
    through, per_model, lost, zero = rs.aimed_counts(ms, plain, brute, masks)
    print("aimed set, scene", scene, "see-through", through, per_model, "lost", lost, "zero masks", zero)
    if scene == 1:
        assert through >= 30 and min(per_model) >= 1 and lost >= 100 and zero >= 20
    else:
        assert through >= 8 and lost >= 40 and zero >= 20


@pytest.mark.parametrize("name", ["bunny_close", "box_close"])
def test_surface_np_equals_the_oracles_gbuffer(fovrt_mod, oracle, name):
    W, H = rc.SIZE
    scene = tc.VIEWS[name][0]
    a, ms = rc.scene_arrays(fovrt_mod, scene), rs.models(fovrt_mod, scene)
    uni = tc.camera(fovrt_mod, name, W, H).uniforms(W, H)
    r = rc.camera_rows(fovrt_mod, name)
    osc = oracle.OracleScene(a)
    hits = rc.hit_records(osc.closest(r, brute=True))
    rec = rs.surface_np(tn.SceneNp(a), r, hits, ms)
    g = oracle.gbuffer(osc, uni, W, H, 0)
    hit = hits["prim"] >= 0
    assert 50 <= hit.sum()
    pos, nrm, dif = (g[k].reshape(-1, 4)[hit] for k in ("position", "normal", "diffuse"))
    assert np.array_equal(rec["point"][hit], pos[:, :3])
    half = (rec["ng"][hit].astype(np.float64) * 0.5 + 0.5).astype(np.float32)  # (exact in f64: one rounding, as the fma)
    assert np.array_equal(half, nrm[:, :3])
    assert np.array_equal(rec["kd"][hit], dif[:, :3])
    assert (rec[~hit] == rs.miss_surface()).all()
    assert np.array_equal(rs.class_of_type(rec), tc.classes_np(a, hits["prim"]))
    assert ((rec["model"] >= 0) == hit).all()


def obj_refs(fovrt, oracle, directory, name):
    """(arrays, models, rows, brute-force hits, surface_np records) of an OBJ scene of ray_surface_cases."""
    sc = fovrt.Scene(rs.obj_scene_config(fovrt, directory, name))
    a, ms = sc.arrays(), sc.models()
    r = rs.obj_rows(fovrt, a)
    hits = rc.hit_records(oracle.OracleScene(a).closest(r, brute=True))
    return a, ms, r, hits, rs.surface_np(tn.SceneNp(a), r, hits, ms)


def check_obj_records(a, name, hits, rec):
    """The hits cover the ground's triangles (normals and uv) and the box's (flags as the scene's name says), both
    sides of each kind; a triangle without normals has ns = ng, one without uv has (u, v) = (0, 0)."""
    flags = np.asarray(a["flags"])
    assert (flags[:2] & 0x300).tolist() == [0x300] * 2 and (flags[2:] & 0x300).tolist() == [rs.OBJ_SCENES[name]] * 4
    hit = hits["prim"] >= 0
    got = (rec["surface"] >> 8) & 0x300
    assert np.array_equal(got[hit], flags[hits["prim"][hit]] & 0x300)
    back = (rec["surface"] >> 18) & 1
    for want, least in ((0x300, 10), (rs.OBJ_SCENES[name], 60)):
        sel = hit & (got == want)
        assert sel.sum() >= least and back[sel].any() and not back[sel].all(), (name, hex(want), int(sel.sum()))
    box = hit & (hits["prim"] >= 2)
    assert (rec["u"][box] == 0).all() and (rec["v"][box] == 0).all()
    assert len(np.unique(rec["kd"][box], axis=0)) == 1       # the one texel lookup at (0, 0)
    same = (rec["ns"] == rec["ng"]).all(axis=1)
    if name == "bare":
        assert same[box].all()
    else:
        assert not same[box].all()                           # the vertex normals differ from the face's
    return set(np.unique(got[hit]).tolist())


def test_surface_np_on_triangles_without_normals_and_uv(fovrt_mod, oracle, tmp_path):
    """The OBJ scenes: every flag combination occurs among the hits, and on the camera rays surface_np equals the
    oracle's G-buffer."""
    W, H = rc.SIZE
    seen = set()
    for name in rs.OBJ_SCENES:
        a, _ms, r, hits, rec = obj_refs(fovrt_mod, oracle, tmp_path, name)
        seen |= check_obj_records(a, name, hits, rec)
        g = oracle.gbuffer(oracle.OracleScene(a), rs.obj_camera(fovrt_mod).uniforms(W, H), W, H, 0)
        cam = slice(0, W * H)
        hit = hits["prim"][cam] >= 0
        assert (hits["prim"][cam] >= 2).sum() >= 40, name
        pos, nrm, dif = (g[k].reshape(-1, 4)[hit] for k in ("position", "normal", "diffuse"))
        assert np.array_equal(rec["point"][cam][hit], pos[:, :3]), name
        half = (rec["ng"][cam][hit].astype(np.float64) * 0.5 + 0.5).astype(np.float32)
        assert np.array_equal(half, nrm[:, :3]), name
        assert np.array_equal(rec["kd"][cam][hit], dif[:, :3]), name
    assert seen == {0x300, 0x100, 0}


@pytest.mark.parametrize("scene", [0, 1])
def test_masked_transmittance_set_holds_all_three_answers(fovrt_mod, scene):
    a, ms = rc.scene_arrays(fovrt_mod, scene), rs.models(fovrt_mod, scene)
    s = rc.shadow_rows(a)
    masks = rs.shadow_masks(ms, len(s))
    v = rs.masked_np(a, ms, s, masks, "shadow")
    plain = rc.shadow_np(tn.SceneNp(a), s)
    counts = (int((v == 0).sum()), int((v == 1).sum()), int(((v > 0) & (v < 1)).sum()))
    print("masked transmittance set, scene", scene, "(zero, one, between):", counts,
          "changed by the mask:", int((v != plain).sum()))
    assert min(counts) >= 20 and sum(counts) == len(s)
    assert np.array_equal(v[0::2], plain[0::2])
    assert (v[1::2] != plain[1::2]).sum() >= 10  # leaving the glass box out changes answers
