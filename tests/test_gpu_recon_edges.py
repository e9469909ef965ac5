"""The reconstruction half (JFA -> Sibson, pull-push -> A-Trous) at the edges the parity suite leaves out:
A-Trous past the LDS-tiled step widths, on a G-buffer-shaped input, on non-finite texels and through its
A/B arms; pull-push below one tile and taller than wide; the whole chain on traced inputs; and more
than one A-Trous iteration in frames, snapshots, buffer copies and a group's composite.

The inputs and shape lists are tests/recon_cases.py's; tests/test_cpu_recon_cases.py holds the oracle
and the numpy restatements to each other on the same inputs."""
import copy

import numpy as np
import pytest

import recon_cases as rc
from helpers import (ASSET_DIR, TEXTURE_MODE, PullPushNp, atrous_np, equal_nan, logpolar_mask_np, rmse_per_channel,
                     sparse_image)

pytestmark = pytest.mark.gpu

SIB_RUN_MAX, SIB_RUN_RMSE = 4e-3, 5e-5  # the run form's bars (README, tests/test_gpu_parity.py)

TN = None


@pytest.fixture(scope="module", autouse=True)
def _tn(fovrt_mod):
    global TN
    TN = fovrt_mod.TextureName


def make_tracer(fovrt, W, H, scene=0, mask=3, spp=1, dmd=1, **kw):
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=scene, mask_mode=mask, spp=spp, diffuse_max_depth=dmd,
                                      texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, **kw))
    assert t.initialize()
    return t


def report(a, b):
    bad = ~np.isclose(a, b, rtol=0, atol=0, equal_nan=True)
    if not bad.any():
        return "equal"
    i = tuple(np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} differ; first {i}: {a[i]} against {b[i]}"


def device_atrous(fovrt_mod, t, count, pos, nrm, col):
    t.write(TN.POSITION, pos)
    t.write(TN.NORMAL, nrm)
    t.write(TN.PULLPUSH, col)
    fovrt_mod.ATrous(t).render(count, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    return t.read(TN.ATROUS)


@pytest.fixture(scope="module")
def atrous_inputs():
    """name -> (W, H) -> (pos, nrm, col), built once."""
    shapes = sorted(set(rc.ATROUS_DEEP_SHAPES + rc.ATROUS_STRUCT_SHAPES + rc.ATROUS_ARM_SHAPES))
    return {"gbuffer": {s: rc.gbuffer_case(*s, seed=s[0] + s[1]) for s in shapes},
            "noise": {s: rc.noise_case(*s, seed=s[0]) for s in rc.ATROUS_DEEP_SHAPES}}


_refs = {}


def atrous_refs(oracle, key, count, pos, nrm, col):
    """(oracle, numpy) for an input, computed once per module."""
    if (key, count) not in _refs:
        with np.errstate(invalid="ignore"):
            _refs[(key, count)] = (oracle.atrous(count, pos, nrm, col), atrous_np(count, pos, nrm, col))
    return _refs[(key, count)]


# ---------------------------------------------------------------------------------------------
# 1. Deep A-Trous: count 4 and 5 (step width 8 and 16) launch the untiled k_atrous<false, true>
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", rc.ATROUS_DEEP_COUNTS)
@pytest.mark.parametrize("W,H", rc.ATROUS_DEEP_SHAPES)
@pytest.mark.parametrize("kind", ["gbuffer", "noise"])
def test_atrous_deep_passes(fovrt_mod, oracle, atrous_inputs, kind, W, H, count):
    pos, nrm, col = atrous_inputs[kind][(W, H)]
    t = make_tracer(fovrt_mod, W, H)
    got = device_atrous(fovrt_mod, t, count, pos, nrm, col)
    ref, ref_np = atrous_refs(oracle, (kind, W, H), count, pos, nrm, col)
    e_o, e_n = np.abs(got - ref).max(), np.abs(got - ref_np).max()
    print(f"atrous deep {kind} {W}x{H} count {count}: oracle {e_o:.3g} numpy {e_n:.3g}")
    t.destroy()
    assert np.isfinite(got).all()
    assert e_o < rc.ATROUS_BAR_ORACLE
    assert e_n < rc.ATROUS_BAR_NP


# ---------------------------------------------------------------------------------------------
# 2. Structured input at the tiled passes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", rc.ATROUS_STRUCT_COUNTS)
@pytest.mark.parametrize("W,H", rc.ATROUS_STRUCT_SHAPES)
def test_atrous_structured_input(fovrt_mod, oracle, atrous_inputs, W, H, count):
    pos, nrm, col = atrous_inputs["gbuffer"][(W, H)]
    t = make_tracer(fovrt_mod, W, H)
    got = device_atrous(fovrt_mod, t, count, pos, nrm, col)
    ref, ref_np = atrous_refs(oracle, ("gbuffer", W, H), count, pos, nrm, col)
    e_o, e_n = np.abs(got - ref).max(), np.abs(got - ref_np).max()
    print(f"atrous structured {W}x{H} count {count}: oracle {e_o:.3g} numpy {e_n:.3g}")
    t.destroy()
    assert e_o < rc.ATROUS_BAR_ORACLE
    assert e_n < rc.ATROUS_BAR_NP


# ---------------------------------------------------------------------------------------------
# 3. Non-finite texels: the oracle's rule (tests/test_cpu_recon_cases.py), texel for texel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", rc.ATROUS_NONFINITE_COUNTS)
@pytest.mark.parametrize("W,H", rc.ATROUS_NONFINITE_SHAPES)
def test_atrous_nonfinite_texels(fovrt_mod, oracle, W, H, count):
    pos, nrm, col, _ = rc.nonfinite_case(W, H, seed=5)
    t = make_tracer(fovrt_mod, W, H)
    got = device_atrous(fovrt_mod, t, count, pos, nrm, col)
    t.destroy()
    ref = oracle.atrous(count, pos, nrm, col)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), report(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref))
    fin = np.isfinite(ref)
    assert fin.any() or (W, H, count) == (40, 24, 4)
    if fin.any():
        err = np.abs(got[fin] - ref[fin]).max()
        print(f"atrous nonfinite {W}x{H} count {count}: {int((~fin).sum())} non-finite values, oracle {err:.3g}")
        assert err < rc.ATROUS_BAR_ORACLE


# ---------------------------------------------------------------------------------------------
# 4. The A/B arms give the default's bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", ["FOVRT_ATROUS_ROWS2", "FOVRT_ATROUS_XCD"])
@pytest.mark.parametrize("W,H", rc.ATROUS_ARM_SHAPES)
def test_atrous_arms_bit_identical(fovrt_mod, atrous_inputs, monkeypatch, knob, W, H):
    """k_atrous_rows2 (two rows per thread) against k_atrous<true, true> at step width 1, and its
    XCD-contiguous block order against round robin."""
    pos, nrm, col = atrous_inputs["gbuffer"][(W, H)]
    base = make_tracer(fovrt_mod, W, H)
    monkeypatch.setenv(knob, "0")
    arm = make_tracer(fovrt_mod, W, H)
    monkeypatch.delenv(knob)
    for count in rc.ATROUS_ARM_COUNTS:
        a = device_atrous(fovrt_mod, base, count, pos, nrm, col)
        b = device_atrous(fovrt_mod, arm, count, pos, nrm, col)
        assert equal_nan(a, b), (count, report(a, b))
    base.destroy(); arm.destroy()


@pytest.mark.parametrize("kind", ["logpolar", 0.003])
def test_jfa_xcd_arm_bit_identical(fovrt_mod, monkeypatch, kind):
    W, H = 201, 130
    rng = np.random.default_rng(11)
    mask = logpolar_mask_np(W, H, W // 2, H - H // 2) if kind == "logpolar" else (rng.random((H, W)) < kind).astype(np.uint8)
    img = sparse_image(W, H, mask, seed=4)
    base = make_tracer(fovrt_mod, W, H, sibson_mode=1)
    monkeypatch.setenv("FOVRT_JFA_XCD", "0")
    arm = make_tracer(fovrt_mod, W, H, sibson_mode=1)
    monkeypatch.delenv("FOVRT_JFA_XCD")
    for t in (base, arm):
        t.write(TN.SHADING, img)
        fovrt_mod.JumpFlooding(t).render(TN.SHADING)
    for tid in (TN.JFA_COORD, TN.JFA_COLOR):
        assert equal_nan(base.read(tid), arm.read(tid)), tid
    base.destroy(); arm.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Pull-push below one tile, taller than wide, and at the degenerate atlases; thin JFA / Sibson
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", rc.PULLPUSH_SHAPES)
def test_pullpush_tiny_and_tall(fovrt_mod, oracle, W, H):
    """S < 64: k_pull_tiles with L < 6, every push level by k_push_level, the final column launch at
    x0 = 0. S <= 2: zeros, as the reference's host loop leaves them (test_cpu_recon_cases.py)."""
    t = make_tracer(fovrt_mod, W, H, sibson_mode=1)
    st, npst = oracle.PullPushState(W, H), PullPushNp(W, H)
    for k, img in enumerate(rc.pullpush_frames(W, H)):
        t.write(TN.SHADING, img)
        fovrt_mod.PullPushInterpolation(t).render(TN.SHADING)
        got = t.read(TN.PULLPUSH)
        ref = st.render(img)
        assert equal_nan(got, ref), (k, report(got, ref))
        assert equal_nan(got, npst.render(img)), k
    t.destroy()


@pytest.mark.parametrize("W,H", rc.JFA_THIN_SHAPES)
@pytest.mark.parametrize("density", [0.1, 1.0])
def test_jfa_and_sibson_thin_images(fovrt_mod, oracle, W, H, density):
    rng = np.random.default_rng(W * 131 + H)
    img = sparse_image(W, H, (rng.random((H, W)) < density).astype(np.uint8), seed=W + H)
    t = make_tracer(fovrt_mod, W, H, sibson_mode=1)
    t.write(TN.SHADING, img)
    fovrt_mod.JumpFlooding(t).render(TN.SHADING)
    coord, color = t.read(TN.JFA_COORD), t.read(TN.JFA_COLOR)
    rcoord, rcol = oracle.jfa(img)
    assert equal_nan(coord, rcoord), report(coord, rcoord)
    assert equal_nan(color, rcol), report(color, rcol)
    fovrt_mod.SibsonInterpolation(t).render()
    si, rs = t.read(TN.SIBSON), oracle.sibson(rcoord, rcol)
    assert equal_nan(si, rs), report(si, rs)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 6. The chain on traced inputs: every stage against its oracle function on the GPU's own upstream
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,mask", [(1, 4), (1, 0), (2, 4), (2, 0)])
def test_reconstruction_chain_on_traced_frames(fovrt_mod, oracle, scene, mask):
    W, H = 100, 70
    t = make_tracer(fovrt_mod, W, H, scene=scene, mask=mask, spp=4, dmd=3, sibson_mode=1)
    run = make_tracer(fovrt_mod, W, H, scene=scene, mask=mask, spp=4, dmd=3, sibson_mode=0)
    cam = fovrt_mod.Camera.preset(scene, W, H)
    if scene == 2:
        # The preset looks straight down at the map from 8 units up: no ray misses, and neighbours are never
        # more than 0.9 units apart. From 2.5 units up, looking along the ground, the top of the screen is sky
        # and the blocks hide ground several units behind them.
        cam.setPosition((cam.pos[0], 2.5, cam.pos[2]))
        cam.lookAt(np.asarray(cam.pos) + np.array([1.0, -0.15, 0.3], np.float32))
    st = oracle.PullPushState(W, H)
    for f in range(3):
        cam.setPrevState()
        cam.lookAt(np.asarray(cam.target) + np.array([0.01, 0.005, 0.0], np.float32))
        t.update_optix_variables(cam)
        t.geometry_launch(); t.sampling_launch(); t.optimize_launch(); t.shading_launch()
        sh, pos, nrm = t.read(TN.SHADING), t.read(TN.POSITION), t.read(TN.NORMAL)
        # JFA, per-tap Sibson: bit-exact
        fovrt_mod.JumpFlooding(t).render(TN.SHADING)
        coord, color = t.read(TN.JFA_COORD), t.read(TN.JFA_COLOR)
        rcoord, rcol = oracle.jfa(sh)
        assert equal_nan(coord, rcoord), (f, report(coord, rcoord))
        assert equal_nan(color, rcol), (f, report(color, rcol))
        fovrt_mod.SibsonInterpolation(t).render()
        rs = oracle.sibson(coord, color)
        si = t.read(TN.SIBSON)
        assert equal_nan(si, rs), (f, report(si, rs))
        # run form: same taps, inside its bars
        run.write(TN.JFA_COORD, coord)
        run.write(TN.JFA_COLOR, color)
        fovrt_mod.SibsonInterpolation(run).render()
        sf = run.read(TN.SIBSON)
        ok = np.isfinite(rs)
        assert np.array_equal(np.isfinite(sf), ok) and np.array_equal(sf[..., 3], rs[..., 3])
        d = np.where(ok, sf, 0) - np.where(ok, rs, 0)
        print(f"chain scene {scene} mask {mask} frame {f}: run form max {np.abs(d).max():.3g} "
              f"rmse {rmse_per_channel(d, np.zeros_like(d)).max():.3g}")
        assert np.abs(d).max() <= SIB_RUN_MAX
        assert (rmse_per_channel(d, np.zeros_like(d)) <= SIB_RUN_RMSE).all()
        # pull-push: bit-exact, one state carried over the frames
        fovrt_mod.PullPushInterpolation(t).render(TN.SHADING)
        pp = t.read(TN.PULLPUSH)
        rpp = st.render(sh)
        assert equal_nan(pp, rpp), (f, report(pp, rpp))
        # A-Trous on the real G-buffer and the pull-push image
        for count in (1, 3):
            fovrt_mod.ATrous(t).render(count, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
            got = t.read(TN.ATROUS)
            ref = oracle.atrous(count, pos, nrm, pp)
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
            fin = np.isfinite(ref)
            err = np.abs(got[fin] - ref[fin]).max()
            with np.errstate(invalid="ignore"):
                ref_np = atrous_np(count, pos, nrm, pp)
            fin_np = fin & np.isfinite(ref_np)
            err_np = np.abs(got[fin_np] - ref_np[fin_np]).max()
            print(f"chain scene {scene} mask {mask} frame {f} atrous count {count}: oracle {err:.3g} numpy {err_np:.3g} "
                  f"(colour max {np.abs(pp[np.isfinite(pp)]).max():.3g}, non-finite {int((~fin).sum())})")
            assert err < rc.ATROUS_BAR_ORACLE
            assert err_np < rc.ATROUS_BAR_NP
        # not vacuous: miss texels and a depth edge
        # (a missed ray: origin pinned to 0, normal 0 stored as 0 * 0.5 + 0.5, unlit)
        miss = (pos[..., :3] == 0).all(-1) & (nrm[..., :3] == 0.5).all(-1) & (nrm[..., 3] == 0)
        dd = np.sum((pos[:, 1:, :3].astype(np.float64) - pos[:, :-1, :3]) ** 2, -1)
        hit_pair = ~miss[:, 1:] & ~miss[:, :-1]
        med = float(np.median(dd[hit_pair]))  # an edge: neighbours 10 times further apart than the typical pair
        print(f"chain scene {scene} mask {mask} frame {f}: {int(miss.sum())} miss texels, neighbour distance^2 max "
              f"{dd[hit_pair].max():.4g} median {med:.4g}")
        assert miss.any() and dd[hit_pair].max() > 100 * med > 0, (int(miss.sum()), float(dd[hit_pair].max()), med)
    t.destroy(); run.destroy()


# ---------------------------------------------------------------------------------------------
# 7. More than one A-Trous iteration in frames: the output image alternates between two buffers
# ---------------------------------------------------------------------------------------------
def assert_atrous_image_is_the_iterated_filter(oracle, t, iters, img):
    """img is the oracle's `iters` passes over the context's own POSITION / NORMAL / PULLPUSH (within the bar):
    not the image an earlier pass left in the other buffer."""
    ref = oracle.atrous(iters, t.read(TN.POSITION), t.read(TN.NORMAL), t.read(TN.PULLPUSH))
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(img), fin)
    assert np.abs(img[fin] - ref[fin]).max() < rc.ATROUS_BAR_ORACLE, np.abs(img[fin] - ref[fin]).max()


FRAME_BUFFERS = ("SHADING", "JFA_COLOR", "SIBSON", "PULLPUSH", "ATROUS", "HISTORY_CACHE", "POSITION", "NORMAL",
                 "DEPTH_CACHE")


def _pan(cam):
    cam.setPrevState()
    cam.lookAt(np.asarray(cam.target) + np.array([0.01, 0.005, 0.0], np.float32))


@pytest.mark.parametrize("iters", [2, 3])
@pytest.mark.parametrize("mode", ["timed", "throughput", "latency"])
def test_frames_with_several_atrous_iterations(fovrt_mod, oracle, mode, iters):
    import torch
    W, H = 128, 96
    a = make_tracer(fovrt_mod, W, H, scene=1, mask=4, spp=4, dmd=3, atrous_iterations=iters)
    b = make_tracer(fovrt_mod, W, H, scene=1, mask=4, spp=4, dmd=3, atrous_iterations=iters)
    if mode == "latency":
        a.set_pipeline_mode(fovrt_mod.PIPELINE_LATENCY)
    cam = fovrt_mod.Camera.preset(1, W, H)
    for f in range(5):
        _pan(cam)
        a.update_optix_variables(cam)
        b.update_optix_variables(cam)
        a.frame(timing=mode == "timed")
        b.geometry_launch(); b.sampling_launch(); b.optimize_launch(); b.shading_launch()
        fovrt_mod.JumpFlooding(b).render(TN.SHADING)
        fovrt_mod.SibsonInterpolation(b).render()
        fovrt_mod.PullPushInterpolation(b).render(TN.SHADING)
        fovrt_mod.ATrous(b).render(iters, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    for name in FRAME_BUFFERS:
        tid = getattr(TN, name)
        assert equal_nan(a.read(tid), b.read(tid)), (name, report(a.read(tid), b.read(tid)))
    assert_atrous_image_is_the_iterated_filter(oracle, a, iters, a.read(TN.ATROUS))
    fovrt_mod.ATrous(b).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    assert not equal_nan(a.read(TN.ATROUS), b.read(TN.ATROUS))
    out = torch.empty(W * H * 4, dtype=torch.float32, device="cuda")
    a.copy_buffer(TN.ATROUS, out.data_ptr(), out.numel() * 4)
    assert equal_nan(out.cpu().numpy().reshape(H, W, 4), a.read(TN.ATROUS))
    a.destroy(); b.destroy()


@pytest.mark.parametrize("iters", [2, 3])
def test_snapshot_restore_with_several_atrous_iterations(fovrt_mod, oracle, iters):
    W, H = 128, 96
    mk = lambda: make_tracer(fovrt_mod, W, H, scene=1, mask=4, spp=4, dmd=3, atrous_iterations=iters)
    a, b = mk(), mk()
    cam = fovrt_mod.Camera.preset(1, W, H)
    cams = []
    for f in range(4):
        _pan(cam)
        cams.append(copy.deepcopy(cam))
    for f in range(3):
        a.update_optix_variables(cams[f])
        a.frame(timing=False)
    snap = a.snapshot()
    a.update_optix_variables(cams[3])
    a.frame(timing=False)
    want = {n: a.read(getattr(TN, n)) for n in ("ATROUS", "PULLPUSH", "SHADING")}
    b.restore(snap)  # a fresh context: its A-Trous has never run
    b.update_optix_variables(cams[3])
    b.frame(timing=False)
    for n, w in want.items():
        assert equal_nan(b.read(getattr(TN, n)), w), ("fresh context", n)
    assert_atrous_image_is_the_iterated_filter(oracle, b, iters, b.read(TN.ATROUS))
    a.restore(snap)
    a.update_optix_variables(cams[3])
    a.frame(timing=False)
    for n, w in want.items():
        assert equal_nan(a.read(getattr(TN, n)), w), ("same context", n)
    a.destroy(); b.destroy()


@pytest.mark.parametrize("iters", [2, 3])
def test_group_composite_with_several_atrous_iterations(fovrt_mod, oracle, iters):
    """Two in-process ranks, one view: the composite on rank 0 is the single context's A-Trous image."""
    import torch
    W, H, tile = 128, 96, 64
    mk = lambda: make_tracer(fovrt_mod, W, H, scene=1, mask=4, spp=4, dmd=3, atrous_iterations=iters)
    ranks, full = [mk(), mk()], mk()
    full.set_sample_sum(2)  # the group sums samples in fixed point
    cam = fovrt_mod.Camera.preset(1, W, H)
    g = fovrt_mod.Group(ranks, views=1, tile=tile, composite=True)
    for f in range(3):
        for t in ranks + [full]:
            t.update_optix_variables(cam)
        full.frame(timing=False)
        g.frame()
    g.synchronize()
    out = torch.empty(W * H * 4, dtype=torch.float32, device="cuda")
    g.composite(out.data_ptr(), out.numel() * 4)
    comp = out.cpu().numpy().reshape(H, W, 4)
    _, at_rank = g.output_ranks(0)
    want = full.read(TN.ATROUS)
    assert equal_nan(ranks[at_rank].read(TN.ATROUS), want), report(ranks[at_rank].read(TN.ATROUS), want)
    assert equal_nan(comp, want), report(comp, want)
    assert_atrous_image_is_the_iterated_filter(oracle, ranks[at_rank], iters, comp)
    g.destroy()
    for t in ranks + [full]:
        t.destroy()
