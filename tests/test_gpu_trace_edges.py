"""GPU suite for the trace half away from the preset cameras: entry 0 (k_gbuffer with GCLASS), the sampling mask,
the compaction into the class-major active list, and entry 3 (the megakernel k_shade_paths with k_shade_resolve)
against the CPU oracle, on the views, sizes and parameter sets of tests/trace_cases.py.

tests/test_cpu_trace_cases.py holds the cases to what they claim (class mixes with an empty class, one class
holding everything, rays with components of +-0) and pins the oracle on them against the second restatement.
Every stage runs on the GPU's own upstream buffers, as in test_gpu_parity.py. Integer work and the G-buffer are
held to bit equality; shading to the project's bars (per-channel RMSE <= 1e-3, max < 5e-2), in both sample-sum
forms: the fixed-point sums with the tail handoff that small launches take by default, and the fp32 running sums
(FOVRT_SHADE_HANDOFF=0) that 4K frames take."""
import numpy as np
import pytest

import trace_cases as tc
from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan, rmse_per_channel
from test_gpu_bvh import mismatch_report

pytestmark = pytest.mark.gpu

TN = None
GBUFFER = ("position", "normal", "depth", "diffuse", "weight")
COUNTERS = ("primary", "shadow", "mirror", "refraction", "reflection", "truncated")


@pytest.fixture(scope="module", autouse=True)
def _tn(fovrt_mod):
    global TN
    TN = fovrt_mod.TextureName


@pytest.fixture(autouse=True)
def _default_schedule(monkeypatch):
    for k in ("FOVRT_SHADE_HANDOFF", "FOVRT_SHADE_CHUNK_REFR", "FOVRT_SHADE_XCD_BANDS"):
        monkeypatch.delenv(k, raising=False)


def make_tracer(fovrt, W, H, scene, mask=3, spp=4, dmd=3, refr=16, builder=0, **kw):
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=scene, mask_mode=mask, spp=spp, diffuse_max_depth=dmd,
                                      refraction_max_depth=refr, texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR,
                                      detail=1, bvh_builder=builder, **kw))
    assert t.initialize()
    return t


def gbuffer_ids():
    return (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.WEIGHT)


def check_gbuffer(t, oracle, osc, arrays, uni, W, H, frame, tag):
    """After geometry_launch: the five outputs and GCLASS against the oracle. Returns the classes."""
    ref = oracle.gbuffer(osc, uni, W, H, frame)
    for name, tid in zip(GBUFFER, gbuffer_ids()):
        got = t.read(tid)
        assert equal_nan(got, ref[name]), (tag, name, mismatch_report(got, ref[name]))
    cls, _hits = tc.primary_classes(osc, arrays, uni, W, H)
    got = t.read(TN.GCLASS)
    assert np.array_equal(got, cls), (tag, "gclass", mismatch_report(got, cls))
    return cls


def check_front(t, oracle, osc, uni, W, H, mode, tag):
    """sampling_launch and optimize_launch on the device's G-buffer: MASK, WEIGHT, EXTRA, the count and the
    active list (the mask's pixels, class-major). Returns (mask, weight after sampling)."""
    inp = [t.read(v) for v in (TN.POSITION, TN.DEPTH, TN.DEPTH_CACHE, TN.WEIGHT, TN.NORMAL, TN.DIFFUSE)]
    gcls = t.read(TN.GCLASS)
    t.sampling_launch()
    ref = oracle.sampling(osc, uni, W, H, mode, *inp)
    mask, weight = t.read(TN.MASK), t.read(TN.WEIGHT)
    assert np.array_equal(mask, ref["mask"]), (tag, "mask", mismatch_report(mask, ref["mask"]))
    assert equal_nan(weight, ref["weight"]), (tag, "weight", mismatch_report(weight, ref["weight"]))
    extra = t.read(TN.EXTRA)
    assert equal_nan(extra, ref["extra"]), (tag, "extra", mismatch_report(extra, ref["extra"]))
    t.optimize_launch()
    check_list(t, oracle, mask, gcls, tag)
    return mask, weight


def check_list(t, oracle, mask, gcls, tag):
    n = t.ray_count()
    n_ref, _ = oracle.warp_sort(mask)
    assert n == n_ref == int(mask.sum()), (tag, n, n_ref, int(mask.sum()))
    lst = t.read(TN.THREAD)[:n]
    assert np.array_equal(np.sort(lst), np.flatnonzero(mask.reshape(-1))), (tag, "active list")
    order = gcls.reshape(-1)[lst].astype(np.int64)
    assert (np.diff(order) >= 0).all(), (tag, "the active list is not class-major", order[:64].tolist())


def shade_and_check(t, oracle, osc, uni, W, H, spp, tag, pool=None, classes=True):
    """shading_launch after the front stages, against the oracle on the device's own mask, WEIGHT and history:
    the bars, inactive history, alpha, overflow and the primary count. Returns (shading, figures)."""
    frame_stats = t.stats()
    mask, weight, hist_in, gcls = t.read(TN.MASK), t.read(TN.WEIGHT), t.read(TN.HISTORY_CACHE), t.read(TN.GCLASS)
    n = t.ray_count()
    assert n == int(mask.sum()), tag
    t.shading_launch()
    got, got_hist = t.read(TN.SHADING), t.read(TN.HISTORY_CACHE)
    ref = oracle.shading(osc, uni, W, H, t._frame, spp, mask, weight, hist_in)
    d = np.nan_to_num(got.astype(np.float64) - ref["shading"].astype(np.float64), nan=1.0)
    rm, mx = rmse_per_channel(got, ref["shading"]), float(np.abs(d).max())
    print(f"{tag}: active {n} rmse {rm[:3].max():.3g} max {mx:.3g}")
    if pool is not None:
        pool.append((d * d).reshape(-1, 4))
    else:
        assert (rm <= tc.SHADE_RMSE).all(), (tag, rm, mismatch_report(got, ref["shading"]))
    assert mx < tc.SHADE_MAX, (tag, mx, mismatch_report(got, ref["shading"]))
    if classes and pool is None:
        for c in range(4):
            sel = (mask == 1) & (gcls == c)
            if sel.sum() >= 16:
                crm = np.sqrt(np.mean(d[sel][:, :3] ** 2, 0))
                assert (crm <= tc.SHADE_RMSE).all(), (tag, "class", c, crm)
    inactive = mask == 0
    assert equal_nan(got_hist[inactive], ref["history"][inactive]), (tag, "inactive history")
    assert set(np.unique(got[..., 3]).tolist()) <= {0.0, 1.0}, tag
    st = t.stats()
    assert st["overflow"] == 0, (tag, st["overflow"])
    assert st["primary"] - frame_stats["primary"] == n * spp, (tag, st["primary"] - frame_stats["primary"], n * spp)
    return got, (float(rm[:3].max()), mx)


def front(t):
    """geometry, sampling and compaction; remembers the frame number entry 0 took."""
    t._frame = t.m_accumFrame
    t.geometry_launch()
    t.sampling_launch()
    t.optimize_launch()


def view(fovrt, name, W, H):
    cam = tc.camera(fovrt, name, W, H)
    return tc.VIEWS[name][0], cam, cam.uniforms(W, H)


# ---------------------------------------------------------------------------------------------
# a. Views: G-buffer, class, sampling and compaction, bit for bit
# ---------------------------------------------------------------------------------------------
FRONT_CASES = ([(n, W, H, 0) for n, W, H in tc.VIEW_CASES]
               + [(n,) + tc.VIEW_SIZE + (b,) for n in tc.ZERO_VIEWS + ["inside_box"] for b in (1, 2)])


@pytest.mark.parametrize("name,W,H,builder", FRONT_CASES)
def test_view_front_stages_bit_exact(fovrt_mod, oracle, name, W, H, builder):
    """Entry 0's five outputs and GCLASS, then MASK, WEIGHT, EXTRA, the count and the class-major active list in
    mask modes 0, 3 and 4 over two frames (the second has a depth cache). Builders 1 and 2 put other boxes in
    front of the slab test on the views whose rays have zero components, and around the eye inside the glass."""
    scene, _cam, uni = view(fovrt_mod, name, W, H)
    for mode in (0, 3, 4):
        t = make_tracer(fovrt_mod, W, H, scene, mask=mode, spp=1, dmd=1, builder=builder)
        t.set_camera_uniforms(uni)
        arrays = t.scene_arrays()
        osc = oracle.OracleScene(arrays)
        for frame in range(2):
            tag = (name, W, H, builder, mode, frame)
            t.geometry_launch()
            cls = check_gbuffer(t, oracle, osc, arrays, uni, W, H, frame, tag)
            if (W, H) == tc.VIEW_SIZE:
                for c, (lo, hi) in tc.CONDITIONS[name].items():
                    assert lo <= float((cls == c).mean()) <= hi, (tag, c)
            check_front(t, oracle, osc, uni, W, H, mode, tag)
            t.shading_launch()
        t.destroy()


# ---------------------------------------------------------------------------------------------
# b. Views: shading against the oracle, in both sample-sum forms
# ---------------------------------------------------------------------------------------------
# every pixel traced (the class mix is the view's); at 100x70 the saliency mask as well (inactive pixels)
SHADE_CASES = [(n, W, H, 3) for n, W, H in tc.VIEW_CASES] + [(n,) + tc.RAGGED_SIZE + (0,) for n in tc.RAGGED_VIEWS]


@pytest.mark.parametrize("name,W,H,mode", SHADE_CASES)
def test_view_shading_in_both_sample_sum_forms(fovrt_mod, oracle, monkeypatch, name, W, H, mode):
    """4 spp, GI depth 3, three frames: the default form (fixed-point sums, tail handoff) and the fp32 running
    sums (FOVRT_SHADE_HANDOFF=0, with the traversal loop's early exit where refraction is at least 1/20 of the
    samples), each against the oracle, and against each other inside test_megakernel_tail_handoff's bars."""
    spp = 4
    scene, _cam, uni = view(fovrt_mod, name, W, H)
    tracers = {}
    for form in ("default", "0"):
        if form == "0":
            monkeypatch.setenv("FOVRT_SHADE_HANDOFF", "0")
        t = make_tracer(fovrt_mod, W, H, scene, mask=mode, spp=spp, dmd=3)
        t.set_camera_uniforms(uni)
        tracers[form] = t
    osc = oracle.OracleScene(tracers["default"].scene_arrays(), refraction_max_depth=16, diffuse_max_depth=3)
    for frame in range(3):
        out = {}
        for form, t in tracers.items():
            front(t)
            out[form], _ = shade_and_check(t, oracle, osc, uni, W, H, spp, f"{name} {W}x{H} mask {mode} form {form} frame {frame}")
        a, b = out["default"], out["0"]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        rm, mx = rmse_per_channel(a, b), float(np.nanmax(np.abs(a - b)))
        print(f"{name} {W}x{H} mask {mode} frame {frame}: forms rmse {rm.max():.3g} max {mx:.3g}")
        assert (rm <= tc.FORMS_RMSE).all(), (name, frame, rm)
        assert mx <= tc.FORMS_MAX, (name, frame, mismatch_report(a, b))
    sa, sb = tracers["default"].stats(), tracers["0"].stats()
    for k in COUNTERS:
        assert sa[k] == sb[k], (name, k, sa[k], sb[k])
    for t in tracers.values():
        t.destroy()


@pytest.mark.parametrize("chunk,bands", [("64", "1"), ("4", "1"), ("0", "0"), ("64", "0")])
@pytest.mark.parametrize("name", ["box_close", "sky"])
def test_schedule_arms_on_extreme_mixes(fovrt_mod, monkeypatch, name, chunk, bands):
    """The megakernel's work queue with one class holding every sample (box_close: refraction) and with the
    three hit classes empty (sky), at 100x70: fixed refraction chunks and chunks interleaved over the XCDs
    schedule the same samples differently; SHADING, the history and the counters do not change."""
    W, H = tc.RAGGED_SIZE
    scene, _cam, uni = view(fovrt_mod, name, W, H)
    a = make_tracer(fovrt_mod, W, H, scene)
    monkeypatch.setenv("FOVRT_SHADE_CHUNK_REFR", chunk)
    monkeypatch.setenv("FOVRT_SHADE_XCD_BANDS", bands)
    b = make_tracer(fovrt_mod, W, H, scene)
    for t in (a, b):
        t.set_camera_uniforms(uni)
        for _ in range(2):
            front(t)
            t.shading_launch()
    gcls = a.read(TN.GCLASS)
    assert (gcls == (0 if name == "box_close" else 3)).all()
    assert a.ray_count() == b.ray_count() == W * H
    for tid in (TN.SHADING, TN.HISTORY_CACHE):
        assert equal_nan(a.read(tid), b.read(tid)), (name, tid, mismatch_report(a.read(tid), b.read(tid)))
    sa, sb = a.stats(), b.stats()
    for k in COUNTERS + ("overflow",):
        assert sa[k] == sb[k], (name, k, sa[k], sb[k])
    assert sa["primary"] == 2 * W * H * 4
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# c. Tiny and thin screens
# ---------------------------------------------------------------------------------------------
def test_tiny_and_thin_screens(fovrt_mod, oracle):
    """Every tiny shape on the bunny preset in mask modes 0 to 4, two frames (the second reads a depth cache and
    a history): the G-buffer, GCLASS, MASK, WEIGHT, EXTRA, the count and the class-major list bit for bit;
    every shaded pixel inside the maximum bar and inactive history exact. A single pixel's rounding must not
    decide the RMSE of a six-pixel screen, so the squared errors of all shapes, modes and frames are pooled
    into one per-channel RMSE, held to the same 1e-3."""
    pool = []
    for W, H in tc.TINY_SHAPES:
        uni = fovrt_mod.Camera.preset(1, W, H).uniforms(W, H)
        for mode in tc.MASK_MODES:
            t = make_tracer(fovrt_mod, W, H, 1, mask=mode)
            t.set_camera_uniforms(uni)
            arrays = t.scene_arrays()
            osc = oracle.OracleScene(arrays, refraction_max_depth=16, diffuse_max_depth=3)
            for frame in range(2):
                tag = (W, H, mode, frame)
                t._frame = t.m_accumFrame
                t.geometry_launch()
                check_gbuffer(t, oracle, osc, arrays, uni, W, H, frame, tag)
                check_front(t, oracle, osc, uni, W, H, mode, tag)
                shade_and_check(t, oracle, osc, uni, W, H, 4, f"tiny {W}x{H} mode {mode} frame {frame}", pool=pool)
            t.destroy()
    sq = np.concatenate(pool)
    rm = np.sqrt(sq.mean(0))
    print(f"tiny screens: {sq.shape[0]} pixels pooled, rmse {rm}")
    assert (rm <= tc.SHADE_RMSE).all(), rm


def test_one_active_pixel_fewer_samples_than_shards(fovrt_mod, oracle):
    """box_close at 3x2 with a host-written mask of one pixel: the launch has spp = 4 samples, fewer than the
    queue's eight shards, all of class 0."""
    W, H, spp = 3, 2, 4
    scene, _cam, uni = view(fovrt_mod, "box_close", W, H)
    t = make_tracer(fovrt_mod, W, H, scene)
    t.set_camera_uniforms(uni)
    osc = oracle.OracleScene(t.scene_arrays(), refraction_max_depth=16, diffuse_max_depth=3)
    m = np.zeros((H, W), np.uint8)
    m[1, 1] = 1
    pool = []
    for frame in range(2):
        t._frame = t.m_accumFrame
        t.geometry_launch()
        t.sampling_launch()
        t.write(TN.MASK, m)
        t.optimize_launch()
        assert t.ray_count() == 1 and t.read(TN.GCLASS)[1, 1] == 0
        assert t.read(TN.THREAD)[0] == W + 1
        shade_and_check(t, oracle, osc, uni, W, H, spp, f"one pixel frame {frame}", pool=pool)
    rm = np.sqrt(np.concatenate(pool).mean(0))
    assert (rm <= tc.SHADE_RMSE).all(), rm
    assert t.stats()["primary"] == 2 * spp


# ---------------------------------------------------------------------------------------------
# d. Parameters off their defaults, against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refr", tc.REFRACTION_DEPTHS)
@pytest.mark.parametrize("name", tc.REFRACTION_VIEWS)
def test_refraction_depth_caps(fovrt_mod, oracle, name, refr):
    """The refraction recursion capped at 2, either side of the device's item stack (24, 25) and at the
    reference's own 100, with the eye inside the glass box and in front of the glass bunny, against the oracle
    at the same cap. Where one more level gives the oracle more segments the cap is reached, and the device
    must count truncated nodes, and none where it is not.

    The segments are counted at diffuse depth 1. A diffuse bounce that hits glass makes the oracle trace the
    whole glass tree below it, as the reference does, although the diffuse program reads only the child's
    reflectance, which a refraction program never writes; the device ends such a bounce at its hit. Those
    trees reach caps the camera's own trees do not (inside_box at 24 and 25), and nothing the frame shows
    depends on them. Refraction draws no random numbers, so the camera's trees are the same at every diffuse
    depth."""
    W, H = tc.VIEW_SIZE
    spp = 4
    scene, _cam, uni = view(fovrt_mod, name, W, H)
    t = make_tracer(fovrt_mod, W, H, scene, refr=refr)
    t.set_camera_uniforms(uni)
    arrays = t.scene_arrays()
    osc = oracle.OracleScene(arrays, refraction_max_depth=refr, diffuse_max_depth=3)
    front(t)
    mask, weight, hist_in = t.read(TN.MASK), t.read(TN.WEIGHT), t.read(TN.HISTORY_CACHE)
    shade_and_check(t, oracle, osc, uni, W, H, spp, f"{name} refraction cap {refr}")
    segs = []
    for cap in (refr, refr + 1):
        camera_trees = oracle.OracleScene(arrays, refraction_max_depth=cap, diffuse_max_depth=1)
        oracle.shading(camera_trees, uni, W, H, 0, spp, mask, weight, hist_in)
        segs.append(camera_trees.segments())
    reached = segs[1] > segs[0]
    st = t.stats()
    print(f"{name} cap {refr}: oracle segments {segs}, cap reached {reached}, truncated {st['truncated']}")
    assert (st["truncated"] > 0) == reached, (segs, st["truncated"])
    if refr == 100:
        assert not reached  # the importance cutoff ends every tree before the reference's own cap
    t.destroy()


@pytest.mark.parametrize("dmd", tc.DIFFUSE_DEPTHS)
def test_diffuse_depth_at_create(fovrt_mod, oracle, dmd):
    W, H = tc.VIEW_SIZE
    scene, _cam, uni = view(fovrt_mod, "along_z", W, H)
    t = make_tracer(fovrt_mod, W, H, scene, dmd=dmd)
    t.set_camera_uniforms(uni)
    osc = oracle.OracleScene(t.scene_arrays(), refraction_max_depth=16, diffuse_max_depth=dmd)
    for frame in range(2):
        front(t)
        shade_and_check(t, oracle, osc, uni, W, H, 4, f"along_z diffuse depth {dmd} frame {frame}")
    assert (t.stats()["diffuse_bounce"] > 0) == (dmd > 1)
    t.destroy()


def test_diffuse_depth_changed_between_frames(fovrt_mod, oracle):
    """fr_set_diffuse_max_depth from 1 to 4 and then to 2: each frame shades at the depth set before it."""
    W, H = tc.VIEW_SIZE
    scene, _cam, uni = view(fovrt_mod, "along_z", W, H)
    t = make_tracer(fovrt_mod, W, H, scene, dmd=tc.DIFFUSE_DEPTH_SEQUENCE[0])
    t.set_camera_uniforms(uni)
    osc = oracle.OracleScene(t.scene_arrays(), refraction_max_depth=16, diffuse_max_depth=tc.DIFFUSE_DEPTH_SEQUENCE[0])
    bounces = []
    for frame, dmd in enumerate(tc.DIFFUSE_DEPTH_SEQUENCE):
        if frame:
            t.set_diffuse_max_depth(dmd)
            osc.set_params(16, dmd)
        before = t.stats()["diffuse_bounce"]
        front(t)
        shade_and_check(t, oracle, osc, uni, W, H, 4, f"along_z diffuse depth -> {dmd} frame {frame}")
        bounces.append(t.stats()["diffuse_bounce"] - before)
    assert bounces[0] == 0 and bounces[1] > bounces[2] > 0, bounces
    t.destroy()


@pytest.mark.parametrize("power", tc.LIGHT_POWERS)
def test_light_power_at_create_and_set(fovrt_mod, oracle, power):
    """light_power 100 at create; 0 set before the first frame (every direct term is exactly 0)."""
    W, H = tc.VIEW_SIZE
    scene, _cam, uni = view(fovrt_mod, "along_z", W, H)
    if power:
        t = make_tracer(fovrt_mod, W, H, scene, light_power=power)
    else:
        t = make_tracer(fovrt_mod, W, H, scene)
        t.set_light_power(power)
    t.set_camera_uniforms(uni)
    arrays = t.scene_arrays()
    assert (arrays["light"][12:15] == np.float32(power)).all()
    osc = oracle.OracleScene(arrays, refraction_max_depth=16, diffuse_max_depth=3)
    for frame in range(2):
        front(t)
        shade_and_check(t, oracle, osc, uni, W, H, 4, f"along_z light {power} frame {frame}")
    t.destroy()


def test_light_change_restarts_the_accumulation(fovrt_mod, oracle):
    """Three frames around fr_set_light_power(2000) (FR/PathTracer.cpp:99-116): the frame after the call shades
    with the old frame number and the new light, the counter then reads 0, and the frame after that starts from
    zeroed history."""
    W, H = tc.VIEW_SIZE
    scene, _cam, uni = view(fovrt_mod, "along_z", W, H)
    t = make_tracer(fovrt_mod, W, H, scene, mask=0)
    t.set_camera_uniforms(uni)
    osc = oracle.OracleScene(t.scene_arrays(), refraction_max_depth=16, diffuse_max_depth=3)
    for frame in range(4):
        if frame == 2:
            t.set_light_power(2000.0)
            arrays = t.scene_arrays()
            assert (arrays["light"][12:15] == np.float32(2000.0)).all()
            osc = oracle.OracleScene(arrays, refraction_max_depth=16, diffuse_max_depth=3)
        front(t)
        assert t._frame == (frame if frame < 3 else 0)
        assert t.m_accumFrame == (frame + 1 if frame < 2 else frame - 2)
        hist_in = t.read(TN.HISTORY_CACHE)
        assert (hist_in[..., 3] > 0).any() == (frame in (1, 2))
        if frame == 3:
            assert not hist_in.any()
        shade_and_check(t, oracle, osc, uni, W, H, 4, f"along_z light change frame {frame}")
    t.destroy()


@pytest.mark.parametrize("name", tc.PAN_VIEWS)
def test_moving_camera_pan_then_cut(fovrt_mod, oracle, name):
    """Three frames of a pan (setPrevState, then the target moves), then a cut to the sky pose, where no
    reprojection lands on a valid history: the G-buffer and the sampling stage bit for bit (the saliency mask
    reads the velocity), shading inside the bars, and WEIGHT's history flag as the oracle has it."""
    W, H = tc.VIEW_SIZE
    scene, cam, _uni = view(fovrt_mod, name, W, H)
    t = make_tracer(fovrt_mod, W, H, scene, mask=0)
    arrays = t.scene_arrays()
    osc = oracle.OracleScene(arrays, refraction_max_depth=16, diffuse_max_depth=3)
    _s, sky_eye, sky_target, sky_up = tc.view_pose(fovrt_mod, "sky")
    for frame in range(4):
        cam.setPrevState()
        if frame < 3:
            cam.lookAt(np.asarray(cam.target) + np.asarray(tc.PAN_STEP, np.float32))
        else:
            cam.setPosition(sky_eye)
            cam.lookAt(sky_target, sky_up)
        uni = cam.uniforms(W, H)
        t.set_camera_uniforms(uni)
        tag = (name, "pan" if frame < 3 else "cut", frame)
        t._frame = t.m_accumFrame
        t.geometry_launch()
        check_gbuffer(t, oracle, osc, arrays, uni, W, H, frame, tag)
        _mask, weight = check_front(t, oracle, osc, uni, W, H, 0, tag)
        if 0 < frame < 3 and name == "along_z":
            # the pan reprojects onto valid history (on street the depth under a reprojected pixel is never
            # within scene_epsilon of the hit's: every flag is 0 there, in the oracle as on the device)
            assert (weight[..., 2] > 0).any(), tag
        if frame == 3:
            assert not (weight[..., 2] > 0).any(), tag
        shade_and_check(t, oracle, osc, uni, W, H, 4, f"{name} moving camera frame {frame}")
    t.destroy()
