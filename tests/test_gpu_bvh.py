"""GPU suite for the BVH builders: the trees themselves, read back from the device (fr__bvh_read) and checked
by the numpy validator (bvh_np.check_tree), and what the traversal computes over them against the CPU oracle,
whose own tree test_cpu_bvh.py holds to its brute force on the same geometry.

The geometry is bvh_cases': equal Morton codes, dead centroid axes, zero-area triangles, hundreds of triangles
in one Morton cell, a one-sided hierarchy. fr_set_positions always rebuilds with the device LBVH (k_bvh.hip),
on contexts whose first tree either builder made.
"""
import numpy as np
import pytest

import bvh_cases
import bvh_np
from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan, rmse_per_channel

pytestmark = pytest.mark.gpu

GBUFFER = ("position", "normal", "depth", "diffuse")


def make_tracer(fovrt, W, H, scene, builder, mask=1, spp=1, dmd=1):
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=scene, mask_mode=mask, spp=spp, diffuse_max_depth=dmd,
                                      texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, detail=1, bvh_builder=builder))
    assert t.initialize()
    return t


def mismatch_report(a, b):
    bad = ~np.isclose(a, b, rtol=0, atol=0, equal_nan=True)
    if not bad.any():
        return "equal"
    idx = np.argwhere(bad)[:5]
    return f"{bad.sum()} of {bad.size} differ; first {idx.tolist()}: gpu {a[tuple(idx[0])]} oracle {b[tuple(idx[0])]}"


def tree_bytes(fovrt, t):
    return tuple(a.tobytes() for a in bvh_np.read_tree(fovrt, t))


# ---------------------------------------------------------------------------------------------
# Structure of the preset trees
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [0, 1, 2])
@pytest.mark.parametrize("builder", [0, 1])
def test_preset_tree_structure(fovrt_mod, builder, scene):
    t = make_tracer(fovrt_mod, 64, 48, scene, builder)
    out = bvh_np.check_tracer_tree(fovrt_mod, t)
    print(f"scene {scene} builder {builder}: {out}")
    if builder == 1:
        assert t.rebuild_bvh() > 0.0
        # the spare arrays' tree (the two swap); the same triangles give the same hierarchy, only the order in
        # which the nodes of a level take their indices is free
        assert bvh_np.check_tracer_tree(fovrt_mod, t) == out
    t.destroy()


# ---------------------------------------------------------------------------------------------
# Adversarial rebuilds: the tree after fr_set_positions, and the G-buffer over it from three poses
# ---------------------------------------------------------------------------------------------
_refs = {}


def case_reference(fovrt, oracle, t, scene, case, W, H):
    """(positions, {pose: (uniforms, frame-0 oracle G-buffer)}) of a case, computed once per (scene, case)
    and shared by the tests of both initial builders."""
    key = (scene, case, W, H)
    if key not in _refs:
        arrays = t.scene_arrays()
        base = arrays["pos"].reshape(-1, 3, 3)
        pos = bvh_cases.CASES[case](base, 0)
        cams = bvh_cases.poses(fovrt, scene, arrays["bbox"], W, H)
        arrays["pos"] = pos.reshape(-1, 9)
        osc = oracle.OracleScene(arrays)
        ref = {}
        for name, cam in cams.items():
            uni = cam.uniforms(W, H)
            g = oracle.gbuffer(osc, uni, W, H, 0)
            for v in g.values():
                v.setflags(write=False)
            ref[name] = (uni, g)
        pos.setflags(write=False)
        _refs[key] = (pos, ref)
    return _refs[key]


@pytest.mark.parametrize("case", sorted(bvh_cases.CASES))
@pytest.mark.parametrize("builder", [0, 1])
@pytest.mark.parametrize("scene", [0, 1])
def test_adversarial_rebuild_tree_and_gbuffer(fovrt_mod, oracle, scene, builder, case):
    TN = fovrt_mod.TextureName
    W, H = (32, 24) if case == "identical" else (64, 48)  # identical: every ray tests every triangle
    t = make_tracer(fovrt_mod, W, H, scene, builder)
    pos, ref = case_reference(fovrt_mod, oracle, t, scene, case, W, H)
    t.set_positions(pos)
    arrays = t.scene_arrays()
    assert np.array_equal(arrays["pos"].reshape(-1, 3, 3), pos)
    out = bvh_np.check_tracer_tree(fovrt_mod, t)
    print(f"scene {scene} builder {builder} {case}: {out}")
    for pose, (uni, g) in ref.items():
        t.reset_accumulation()  # frame 0, the frame of the shared reference
        assert t.m_accumFrame == 0
        t.set_camera_uniforms(uni)
        t.geometry_launch()
        hit = float((g["position"][..., :3] != 0).any(-1).mean())
        for name, tid in zip(GBUFFER, (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE)):
            got = t.read(tid)
            assert equal_nan(got, g[name]), (pose, name, hit, mismatch_report(got, g[name]))
    assert t.stats()["overflow"] == 0
    t.destroy()


# ---------------------------------------------------------------------------------------------
# Secondary rays over adversarial trees: shadow rays through doubled glass faces, bounces among
# zero-area triangles
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pairs", "degenerate_mix", "two_scales"])
def test_secondary_rays_over_adversarial_trees(fovrt_mod, oracle, case):
    TN = fovrt_mod.TextureName
    W, H, spp, dmd = 48, 32, 4, 3
    t = make_tracer(fovrt_mod, W, H, 0, 1, mask=3, spp=spp, dmd=dmd)
    pos = bvh_cases.CASES[case](t.scene_arrays()["pos"].reshape(-1, 3, 3), 0)
    t.set_positions(pos)
    bvh_np.check_tracer_tree(fovrt_mod, t)
    uni = fovrt_mod.Camera.preset(0, W, H).uniforms(W, H)
    t.set_camera_uniforms(uni)
    osc = oracle.OracleScene(t.scene_arrays(), refraction_max_depth=16, diffuse_max_depth=dmd)
    frame = t.m_accumFrame
    t.geometry_launch()
    t.sampling_launch()
    t.optimize_launch()
    mask, weight, hist_in = t.read(TN.MASK), t.read(TN.WEIGHT), t.read(TN.HISTORY_CACHE)
    assert mask.all()
    t.shading_launch()
    got = t.read(TN.SHADING)
    ref = oracle.shading(osc, uni, W, H, frame, spp, mask, weight, hist_in)["shading"]
    rm = rmse_per_channel(got, ref)
    st = t.stats()
    print(f"{case}: rmse {rm.tolist()} shadow {st['shadow']} refraction {st['refraction']}")
    assert (rm <= 1e-3).all(), (rm, mismatch_report(got, ref))
    assert st["overflow"] == 0 and st["shadow"] > 0
    # (two_scales' box-spanning triangle stands between this camera and what is left of the glass cube)
    assert st["refraction"] > 0 or case == "two_scales"
    t.destroy()


# ---------------------------------------------------------------------------------------------
# A rebuild before every pipelined frame: the double-buffered tree swaps while the previous frame's
# reconstruction is in flight
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_rebuild_before_every_pipelined_frame(fovrt_mod, builder):
    TN = fovrt_mod.TextureName
    W, H = 160, 96
    a = make_tracer(fovrt_mod, W, H, 1, builder, mask=4, spp=2)
    b = make_tracer(fovrt_mod, W, H, 1, builder, mask=4, spp=2)
    base = a.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    for f in range(6):
        pos = base.copy()
        pos[..., 1] += np.float32(0.05) * np.sin(np.float32(3.0) * base[..., 0] + np.float32(f)).astype(np.float32)
        a.set_positions(pos)
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
    bvh_np.check_tracer_tree(fovrt_mod, a)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# A rejected update leaves the tree alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_rejected_update_leaves_the_tree_alone(fovrt_mod, builder):
    t = make_tracer(fovrt_mod, 64, 48, 1, builder)
    before = tree_bytes(fovrt_mod, t)
    numbers = {k: t.scene_arrays()[k] for k in ("bvh_nodes", "bvh_depth", "bvh_max_stack")}
    bad = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    bad[bad.shape[0] // 2, 1, 2] = np.nan
    with pytest.raises(fovrt_mod.FovrtError) as e:
        t.set_positions(bad)
    assert e.value.code == fovrt_mod.FR_E_INVALID
    assert tree_bytes(fovrt_mod, t) == before
    assert {k: t.scene_arrays()[k] for k in numbers} == numbers
    bvh_np.check_tracer_tree(fovrt_mod, t)
    t.destroy()
