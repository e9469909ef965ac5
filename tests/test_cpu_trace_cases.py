"""The off-preset trace cases (tests/trace_cases.py) are what they claim, and the reference side is pinned on
them before the GPU suite trusts it: every view delivers its class mix on the oracle's G-buffer, the camera
rays have the zero components (and the slab test the finite stand-in for 1 / 0) they are there for, the oracle
and the second restatement (tests/trace_np.py) agree on the views, and the oracle runs every tiny shape."""
import numpy as np
import pytest

import trace_cases as tc
import trace_np as tn
from helpers import ASSET_DIR, TEXTURE_MODE

TOL = 1e-6  # test_cpu_trace_restatement's

_SCENES = {}


def scene_arrays(fovrt, scene):
    """The scene's arrays at detail 1, loaded once per session."""
    if scene not in _SCENES:
        _SCENES[scene] = fovrt.Scene(fovrt.Config(scene=scene, texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR,
                                                  detail=1)).arrays()
    return _SCENES[scene]


def _view(fovrt, oracle, name, W, H):
    a = scene_arrays(fovrt, tc.VIEWS[name][0])
    uni = tc.camera(fovrt, name, W, H).uniforms(W, H)
    return a, oracle.OracleScene(a), uni


def _face_normals(a, prim):
    P = np.asarray(a["pos"], np.float64).reshape(-1, 3, 3)[prim.astype(np.int64)]
    return np.cross(P[..., 1, :] - P[..., 0, :], P[..., 2, :] - P[..., 0, :])


@pytest.mark.parametrize("name", tc.VIEW_NAMES)
def test_view_delivers_its_class_mix(fovrt_mod, oracle, name):
    W, H = tc.VIEW_SIZE
    a, osc, uni = _view(fovrt_mod, oracle, name, W, H)
    cls, hits = tc.primary_classes(osc, a, uni, W, H)
    share = [float((cls == c).mean()) for c in range(4)]
    print(name, "shares (refraction, reflection, diffuse, miss):", np.round(share, 3))
    for c, (lo, hi) in tc.CONDITIONS[name].items():
        assert lo <= share[c] <= hi, (name, c, share)
    # the classes are those of the oracle's own entry 0: a miss writes reprojection -1 and position 0
    g = oracle.gbuffer(osc, uni, W, H, 0)
    assert np.array_equal(g["weight"][..., 0] == -1, cls == 3)
    if name in ("inside_box", "below"):  # the first hit is a back face on every pixel
        _eye, d = tc.camera_rays_np(uni, W, H)
        assert (np.einsum("hwk,hwk->hw", d.astype(np.float64), _face_normals(a, hits[..., 1])) > 0).all()
    if name == "below":  # ... which no light reaches: entry 0's lit flag is 0
        assert (g["normal"][..., 3] == 0).all()


def test_views_have_rays_with_zero_components(fovrt_mod, oracle):
    """Over the zero-component views at 64x48: rays with d.x == 0, with d.y == 0, with d.z == 0, one with two
    zero components, one negative zero. And the zeros reach the code they are there for: on a ray with a zero
    component whose origin is off 0 on that axis, a box that straddles 0 and the origin there (the ground's
    triangles under down_axis) is reached with the stand-in 2^100 and culled with the plain reciprocal, in the
    device's min / max slab form, so such a ray would lose the hit the oracle finds."""
    W, H = tc.VIEW_SIZE
    zeros = np.zeros(3, np.int64)
    two = negative = lost = 0
    for name in tc.ZERO_VIEWS:
        a, osc, uni = _view(fovrt_mod, oracle, name, W, H)
        eye, d = tc.camera_rays_np(uni, W, H)
        z = d == 0
        assert z.any(), name
        zeros += z.sum((0, 1))
        two += int((z.sum(-1) >= 2).sum())
        negative += int((z & np.signbit(d)).sum())
        hits = osc.closest(tc.closest_rays(eye, d)).reshape(H, W, 4)
        sel = z.any(-1) & (hits[..., 1] >= 0)
        P = np.asarray(a["pos"], np.float32).reshape(-1, 3, 3)[hits[..., 1][sel].astype(np.int64)]
        lo, hi = P.min(1), P.max(1)
        lo = lo - (np.float32(1e-5) + np.float32(4e-7) * np.abs(lo))  # the device's inflation of its boxes
        hi = hi + (np.float32(1e-5) + np.float32(4e-7) * np.abs(hi))
        ds = d[sel]
        safe = tc.box_reached_np(lo, hi, eye, tc.reciprocal_np(ds, True), 1e-3, np.inf)
        plain = tc.box_reached_np(lo, hi, eye, tc.reciprocal_np(ds, False), 1e-3, np.inf)
        assert safe.all(), name  # the hit triangle's own box is never culled
        lost += int((~plain).sum())
        print(name, "zero components (x, y, z):", z.sum((0, 1)), "hit rays among them:", int(sel.sum()),
              "lost with a plain reciprocal:", int((~plain).sum()))
    assert (zeros > 0).all(), zeros
    assert two > 0 and negative > 0, (two, negative)
    assert lost > 0


def _restate(oracle, a, uni, W, H, spp, dmd, refr, frames):
    osc = oracle.OracleScene(a, refraction_max_depth=refr, diffuse_max_depth=dmd)
    nsc = tn.SceneNp(a, refraction_max_depth=refr, diffuse_max_depth=dmd)
    hist = np.zeros((H, W, 4), np.float32)
    depth_cache = np.zeros((H, W, 4), np.float32)
    worst = 0.0
    for frame in range(frames):
        g_or = oracle.gbuffer(osc, uni, W, H, frame)
        g_np = tn.gbuffer_np(nsc, uni, W, H, frame)
        for k in g_or:
            assert np.array_equal(g_np[k], g_or[k], equal_nan=True), (frame, k)
        s = oracle.sampling(osc, uni, W, H, 3, g_or["position"], g_or["depth"], depth_cache, g_or["weight"],
                            g_or["normal"], g_or["diffuse"])
        sh_or = oracle.shading(osc, uni, W, H, frame, spp, s["mask"], s["weight"], hist)
        sh_np = tn.shade_np(nsc, uni, W, H, frame, spp, s["mask"], s["weight"], hist)
        for k in ("history", "shading"):
            err = np.abs(sh_np[k] - sh_or[k])
            assert np.isfinite(sh_or[k]).all() and (err <= TOL).all(), (frame, k, float(err.max()))
            worst = max(worst, float(err.max()))
        hist, depth_cache = sh_or["history"], g_or["depth"]
    return worst


@pytest.mark.parametrize("refr", [16, 100])
@pytest.mark.parametrize("name", tc.SCENE0_VIEWS)
def test_box_views_match_second_restatement(fovrt_mod, oracle, name, refr):
    """Every box-scene view at 16x12, 4 spp, GI depth 3, at the default refraction cap and the reference's own
    (100): the G-buffer bit for bit, shading within 1e-6."""
    W, H = 16, 12
    a = scene_arrays(fovrt_mod, 0)
    uni = tc.camera(fovrt_mod, name, W, H).uniforms(W, H)
    worst = _restate(oracle, a, uni, W, H, 4, 3, refr, frames=1)
    print(name, refr, "worst shading difference", worst)


@pytest.mark.parametrize("name", ["earth_close", "inside_bunny"])
def test_bunny_views_match_second_restatement(fovrt_mod, oracle, name):
    """The reflective sphere filling the screen, and the eye inside the glass bunny: 16x12 (fewer pixels than
    the preset's 20x14 restatement test), 4 spp, GI depth 3, one frame."""
    W, H = 16, 12
    a = scene_arrays(fovrt_mod, 1)
    uni = tc.camera(fovrt_mod, name, W, H).uniforms(W, H)
    worst = _restate(oracle, a, uni, W, H, 4, 3, 16, frames=1)
    print(name, "worst shading difference", worst)


@pytest.mark.parametrize("W,H", tc.TINY_SHAPES)
def test_oracle_runs_tiny_shapes(fovrt_mod, oracle, W, H):
    """Entries 0 to 3 of the oracle on every tiny shape, in every mask mode, over two frames (the second reads
    a depth cache and a history): finite shading, warp_sort's count equal to the mask sum, inactive pixels
    carrying their history."""
    a = scene_arrays(fovrt_mod, 1)
    uni = fovrt_mod.Camera.preset(1, W, H).uniforms(W, H)
    osc = oracle.OracleScene(a, refraction_max_depth=16, diffuse_max_depth=3)
    for mode in tc.MASK_MODES:
        hist = np.zeros((H, W, 4), np.float32)
        depth_cache = np.zeros((H, W, 4), np.float32)
        for frame in range(2):
            g = oracle.gbuffer(osc, uni, W, H, frame)
            s = oracle.sampling(osc, uni, W, H, mode, g["position"], g["depth"], depth_cache, g["weight"],
                                g["normal"], g["diffuse"])
            n, _ = oracle.warp_sort(s["mask"])
            assert n == int(s["mask"].sum()), (mode, frame)
            if mode == 3:
                assert n == W * H
            sh = oracle.shading(osc, uni, W, H, frame, 4, s["mask"], s["weight"], hist)
            assert np.isfinite(sh["shading"]).all() and np.isfinite(sh["history"]).all(), (mode, frame)
            assert set(np.unique(sh["shading"][..., 3]).tolist()) <= {0.0, 1.0}
            hist, depth_cache = sh["history"], g["depth"]
