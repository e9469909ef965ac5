"""GPU suite for foveation control: the eccentricity mask (k_ecc_mask) in bytes against the numpy restatement, frames in
that mode against the CPU oracle, a caller's masks in stream order (k_mask_take) against the stage calls with
fr_write_buffer(FR_BUF_MASK), the ray budget's controller (k_fov_control) against the restatement's closed loop,
mode switches, refusals, a two-rank group and snapshot / restore.

Scenes 0 and 1, procedural detail 1, 100 x 70 unless said otherwise, 2 spp. A context is created in one of the
reference modes and enters modes 5 and 6 through set_mask_mode. A radius is given in pixels and squared by the host in
fp32, so every expected mask is the restatement's at fnp.radius_r2(radius)."""
import ctypes as C

import numpy as np
import pytest

import foveation_np as fnp
import trace_cases as tc
from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan, rmse_per_channel
from test_gpu_bvh import mismatch_report

pytestmark = pytest.mark.gpu

W, H = 100, 70
SPP = 2


def mk(fovrt, w=W, h=H, scene=1, mask=4, **kw):
    t = fovrt.PathTracer(fovrt.Config(width=w, height=h, scene=scene, mask_mode=mask, spp=SPP, diffuse_max_depth=1,
                                      texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, detail=1, **kw))
    assert t.initialize()
    return t


def uniforms(fovrt, scene, w, h, gaze):
    u = fovrt.Camera.preset(scene, w, h).uniforms(w, h)
    u.gaze[0], u.gaze[1] = float(gaze[0]), float(gaze[1])
    return u


def radius_of(r2):
    return np.float32(np.sqrt(np.float32(r2), dtype=np.float32))


def out_ids(fovrt):
    TN = fovrt.TextureName
    return (TN.MASK, TN.WEIGHT, TN.SHADING, TN.HISTORY_CACHE, TN.JFA_COLOR, TN.SIBSON, TN.PULLPUSH, TN.ATROUS)


def assert_same_outputs(fovrt, a, b, what, ids=None):
    TN = fovrt.TextureName
    for tid in ids or out_ids(fovrt):
        x, y = a.read(tid), b.read(tid)
        assert equal_nan(x, y), (what, tid, mismatch_report(x, y))
    n = a.ray_count()
    assert n == b.ray_count(), (what, "count")
    assert np.array_equal(a.read(TN.THREAD)[:n], b.read(TN.THREAD)[:n]), (what, "active list")


def check_list(fovrt, oracle, t, mask, tag):
    """The count and the active list of the compaction: the mask's pixels, class-major."""
    TN = fovrt.TextureName
    n = t.ray_count()
    n_ref, _ = oracle.warp_sort(mask)
    assert n == n_ref == int(mask.sum()), (tag, n, n_ref, int(mask.sum()))
    lst = t.read(TN.THREAD)[:n]
    assert np.array_equal(np.sort(lst), np.flatnonzero(mask.reshape(-1))), (tag, "active list")
    order = t.read(TN.GCLASS).reshape(-1)[lst].astype(np.int64)
    assert (np.diff(order) >= 0).all(), (tag, "the active list is not class-major")


def recon(fovrt, t):
    TN = fovrt.TextureName
    fovrt.JumpFlooding(t).render(TN.SHADING)
    fovrt.SibsonInterpolation(t).render()
    fovrt.PullPushInterpolation(t).render(TN.SHADING)
    fovrt.ATrous(t).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)


# ---------------------------------------------------------------------------------------------
# 1. The mask in bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", fnp.SCREENS)
def test_mask_in_bytes(fovrt_mod, oracle, w, h):
    """MASK after a mode-5 sampling launch equals numpy on every gaze, radius and floor of the CPU suite (7000 and 195
    pixels take the 16-byte body and the scalar tail, 1 x 1 the tail alone); WEIGHT and EXTRA are the oracle's at mode
    3; the count is the mask's sum and the active list its pixels, class-major. Two frames: the second reads a depth
    cache."""
    TN = fovrt_mod.TextureName
    t = mk(fovrt_mod, w, h, scene=1)
    t.set_mask_mode(fovrt_mod.MASK_ECCENTRIC)
    assert t.mask_mode() == 5
    osc = oracle.OracleScene(t.scene_arrays())
    for frame in range(2):
        first = True
        for gaze in fnp.GAZES:
            g = gaze or fnp.centre(w, h)
            uni = uniforms(fovrt_mod, 1, w, h, g)
            t.set_camera_uniforms(uni)
            if first:
                t.geometry_launch()
            inp = [t.read(v) for v in (TN.POSITION, TN.DEPTH, TN.DEPTH_CACHE, TN.WEIGHT, TN.NORMAL, TN.DIFFUSE)]
            for r2 in fnp.r2_values(w, h):
                rad = radius_of(r2)
                for fl in fnp.FLOORS:
                    tag = (w, h, frame, g, float(rad), fl)
                    t.set_foveation(radius_px=rad, floor_ranks=fl)
                    t.sampling_launch()
                    ref = fnp.mask(w, h, g, fnp.radius_r2(rad), fl)
                    got = t.read(TN.MASK)
                    assert np.array_equal(got, ref), (tag, mismatch_report(got, ref))
                    t.optimize_launch()
                    check_list(fovrt_mod, oracle, t, ref, tag)
            o = oracle.sampling(osc, uni, w, h, 3, *inp)
            wgt, extra = t.read(TN.WEIGHT), t.read(TN.EXTRA)
            assert equal_nan(wgt, o["weight"]), (w, h, frame, g, "weight", mismatch_report(wgt, o["weight"]))
            assert equal_nan(extra, o["extra"]), (w, h, frame, g, "extra", mismatch_report(extra, o["extra"]))
            first = False
        t.shading_launch()
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Frames against the oracle
# ---------------------------------------------------------------------------------------------
def test_frames_against_the_oracle(fovrt_mod, oracle):
    """Two consecutive mode-5 frames on scene 1 (the second reprojects the first): SHADING against oracle.shading over
    numpy's mask at the suite's bars, the inactive pixels' history exactly the oracle's."""
    TN = fovrt_mod.TextureName
    t = mk(fovrt_mod)
    t.set_mask_mode(5)
    g = (41.0, 30.5)
    uni = uniforms(fovrt_mod, 1, W, H, g)
    t.set_camera_uniforms(uni)
    osc = oracle.OracleScene(t.scene_arrays())
    ref_mask = fnp.mask(W, H, g, fnp.radius_r2(fovrt_mod.foveation_default(W, H)["radius_px"]), 1)
    assert 0.05 < ref_mask.mean() < 0.5
    for frame in range(2):
        fno = t.m_accumFrame
        t.geometry_launch(); t.sampling_launch(); t.optimize_launch()
        mask, weight, hist_in = t.read(TN.MASK), t.read(TN.WEIGHT), t.read(TN.HISTORY_CACHE)
        assert np.array_equal(mask, ref_mask), (frame, mismatch_report(mask, ref_mask))
        t.shading_launch()
        got, got_hist = t.read(TN.SHADING), t.read(TN.HISTORY_CACHE)
        ref = oracle.shading(osc, uni, W, H, fno, SPP, ref_mask, weight, hist_in)
        rm = rmse_per_channel(got, ref["shading"])
        mx = float(np.abs(np.nan_to_num(got.astype(np.float64) - ref["shading"], nan=1.0)).max())
        print(f"mode 5 frame {frame}: active {int(mask.sum())} rmse {rm[:3].max():.3g} max {mx:.3g}")
        assert (rm <= tc.SHADE_RMSE).all(), (frame, rm)
        assert mx < tc.SHADE_MAX, (frame, mx)
        inactive = ref_mask == 0
        assert equal_nan(got_hist[inactive], ref["history"][inactive]), (frame, "inactive history")
        if frame:
            assert (weight[..., 2] > 0).any(), "the second frame found no valid history"
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Caller masks
# ---------------------------------------------------------------------------------------------
def caller_masks(n, seed=5):
    """n masks with bytes from {0, 1, 2, 255}; the third is empty and the fifth full."""
    rng = np.random.default_rng(seed)
    ms = [rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(H, W), p=[0.7, 0.1, 0.1, 0.1]) for _ in range(n)]
    if n > 2:
        ms[2][:] = 0
    if n > 4:
        ms[4] = rng.choice(np.array([1, 2, 255], np.uint8), size=(H, W))
    return ms


def twin_frame(fovrt, b, m01):
    """The stage calls with the mask written between sampling and compaction: what a caller could do before."""
    TN = fovrt.TextureName
    b.geometry_launch(); b.sampling_launch()
    b.write(TN.MASK, m01)
    b.optimize_launch(); b.shading_launch()
    recon(fovrt, b)


@pytest.mark.parametrize("latency", [False, True])
def test_enqueued_caller_masks_equal_written_masks(fovrt_mod, latency):
    """Six pipelined frames with another mask enqueued before each from a producer stream that is still writing it
    when the call is made and overwrites the array right after sampling_mask_consumed, against a twin that gets the
    same masks (as 0 / 1, the form the context keeps) through fr_write_buffer between its stage calls: every output
    buffer, the count and the active list, after the empty mask, after the full one and at the end."""
    import torch
    masks = caller_masks(6)
    a, b = mk(fovrt_mod), mk(fovrt_mod, mask=3)
    a.enable_sampling_mask()
    a.set_mask_mode(fovrt_mod.MASK_CALLER)
    if latency:
        a.set_pipeline_mode(fovrt_mod.PIPELINE_LATENCY)
    src = [torch.from_numpy(m.reshape(-1).copy()).to("cuda:0") for m in masks]
    dev = torch.zeros(W * H, dtype=torch.uint8, device="cuda:0")
    ballast = torch.ones(1 << 24, dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    for f, m in enumerate(masks):
        with torch.cuda.stream(s):
            for _ in range(4):  # the producer is still busy when the call below is made
                ballast.mul_(1.0001)
            dev.copy_(src[f])
            ev = torch.cuda.Event()
            ev.record(s)
        a.set_sampling_mask(dev, enqueue=True, ready_event=ev)
        a.frame(timing=False)
        a.sampling_mask_consumed(s)
        with torch.cuda.stream(s):
            dev.fill_(255 if f % 2 else 0)  # free to overwrite: the copy has read it
        twin_frame(fovrt_mod, b, (m != 0).astype(np.uint8))
        if f in (2, 4, 5):
            assert_same_outputs(fovrt_mod, a, b, f"latency={latency} frame {f}")
            assert a.ray_count() == int((m != 0).sum())
    torch.cuda.synchronize()
    a.destroy(); b.destroy()


def test_synchronous_caller_masks_from_host_and_device(fovrt_mod):
    """fr_set_sampling_mask from host and from device memory ahead of pipelined frames gives the twin's frames; the
    copy the context keeps is 0 / 1."""
    import torch
    TN = fovrt_mod.TextureName
    masks = caller_masks(3, seed=9)
    hst, dvc, b = mk(fovrt_mod), mk(fovrt_mod), mk(fovrt_mod, mask=3)
    for t in (hst, dvc):
        t.enable_sampling_mask()
        t.set_mask_mode(6)
    for f, m in enumerate(masks):
        hst.set_sampling_mask(m)
        d = torch.from_numpy(m.reshape(-1).copy()).to("cuda:0")
        torch.cuda.synchronize()
        dvc.set_sampling_mask(d)
        hst.frame(timing=False); dvc.frame(timing=False)
        twin_frame(fovrt_mod, b, (m != 0).astype(np.uint8))
        assert_same_outputs(fovrt_mod, hst, b, f"host frame {f}")
        assert_same_outputs(fovrt_mod, dvc, b, f"device frame {f}")
        assert set(np.unique(hst.read(TN.MASK)).tolist()) <= {0, 1}
    # stage calls in mode 6 use the same copy
    hst.geometry_launch(); hst.sampling_launch()
    assert np.array_equal(hst.read(TN.MASK), (masks[-1] != 0).astype(np.uint8))
    for t in (hst, dvc, b):
        t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. The ray budget
# ---------------------------------------------------------------------------------------------
def bits(x):
    return np.float32(x).view(np.uint32)


@pytest.mark.parametrize("w,h,gaze,T,radius", fnp.LOOPS[:3])
def test_budget_walks_the_restatements_trajectory(fovrt_mod, w, h, gaze, T, radius):
    """Twelve launches through stage calls (status after each), fr_frame in throughput mode and fr_frame in latency
    mode (status once at the end, and the last frame's MASK): r2 in bits and the count of the numpy closed loop fed the
    device's own counts."""
    TN = fovrt_mod.TextureName
    uni = uniforms(fovrt_mod, 0, w, h, gaze)
    # stage calls
    t = mk(fovrt_mod, w, h, scene=0)
    t.set_mask_mode(5)
    t.set_camera_uniforms(uni)
    t.set_foveation(radius_px=radius, ray_budget=T)
    assert t.foveation_status() == {"r2": float(fnp.radius_r2(radius)), "last_count": 0, "adjusted": 0, "held": 0}
    t.geometry_launch()
    r2, counts, nheld = fnp.radius_r2(radius), [], 0
    for k in range(12):
        if k:
            r2, held = fnp.control(r2, counts[-1], T, 0.02, w, h)
            nheld += held
        t.sampling_launch(); t.optimize_launch()
        st = t.foveation_status()
        assert bits(st["r2"]) == bits(r2), (k, st, float(r2))
        assert st["last_count"] == (counts[-1] if k else 0) and st["held"] == nheld and st["adjusted"] == k - nheld, (k, st)
        ref = fnp.mask(w, h, gaze, r2, 1)
        counts.append(t.ray_count())
        assert counts[-1] == int(ref.sum()), (k, counts[-1], int(ref.sum()))
        assert np.array_equal(t.read(TN.MASK), ref), k
    assert fnp.in_band(counts[-1], T), counts
    loop = fnp.closed_loop(w, h, gaze, T, radius, 12, counts=counts)
    assert [c for _, c, _ in loop] == counts and bits(loop[-1][0]) == bits(r2)
    t.destroy()
    # pipelined frames, both modes: the same trajectory
    for mode in (fovrt_mod.PIPELINE_THROUGHPUT, fovrt_mod.PIPELINE_LATENCY):
        p = mk(fovrt_mod, w, h, scene=0)
        p.set_pipeline_mode(mode)
        p.set_mask_mode(5)
        p.set_camera_uniforms(uni)
        p.set_foveation(radius_px=radius, ray_budget=T)
        for k in range(12):
            p.frame(timing=False)
        st = p.foveation_status()
        assert bits(st["r2"]) == bits(r2) and st["last_count"] == counts[-2], (mode, st, float(r2), counts)
        assert st["held"] == nheld and st["adjusted"] == 11 - nheld, (mode, st)
        assert np.array_equal(p.read(TN.MASK), fnp.mask(w, h, gaze, r2, 1)), mode
        assert p.ray_count() == counts[-1]
        p.destroy()


def test_budget_follows_the_gaze_restarts_and_holds_without_a_compaction(fovrt_mod):
    """The gaze moved from the centre to the corner (3.5, 66.25) after launch 6 leaves part of the fovea off screen:
    the radius grows again. A second fr_set_foveation restarts from its radius. Two sampling launches with no
    compaction between them use the same r2."""
    TN = fovrt_mod.TextureName
    T = 1400
    t = mk(fovrt_mod, scene=0)
    t.set_mask_mode(5)
    gaze = (50.0, 35.0)
    t.set_camera_uniforms(uniforms(fovrt_mod, 0, W, H, gaze))
    t.set_foveation(radius_px=10.0, ray_budget=T)
    t.geometry_launch()
    r2, n, trail = fnp.radius_r2(10.0), None, []
    for k in range(14):
        if k == 7:
            gaze = (3.5, 66.25)
            t.set_camera_uniforms(uniforms(fovrt_mod, 0, W, H, gaze))
        if k:
            r2, _ = fnp.control(r2, n, T, 0.02, W, H)
        t.sampling_launch(); t.optimize_launch()
        assert bits(t.foveation_status()["r2"]) == bits(r2), k
        n = t.ray_count()
        assert n == int(fnp.mask(W, H, gaze, r2, 1).sum()), k
        trail.append((float(r2), n))
    assert fnp.in_band(trail[6][1], T) and not fnp.in_band(trail[7][1], T), trail
    assert trail[7][1] < T and trail[-1][0] > trail[6][0] and fnp.in_band(trail[-1][1], T), trail
    # a second fr_set_foveation restarts the controller from its radius: the count in place is not read
    t.set_foveation(radius_px=5.0, ray_budget=T, tolerance=0.05)
    t.sampling_launch()
    assert t.foveation_status() == {"r2": 25.0, "last_count": 0, "adjusted": 0, "held": 0}
    assert np.array_equal(t.read(TN.MASK), fnp.mask(W, H, gaze, np.float32(25.0), 1))
    # no compaction since that launch: r2 is kept and nothing is counted
    t.sampling_launch()
    assert t.foveation_status() == {"r2": 25.0, "last_count": 0, "adjusted": 0, "held": 0}
    t.optimize_launch()
    n = t.ray_count()
    t.sampling_launch()
    st = t.foveation_status()
    r2b, held = fnp.control(np.float32(25.0), n, T, 0.05, W, H)
    assert bits(st["r2"]) == bits(r2b) and st["last_count"] == n and (st["adjusted"], st["held"]) == (1 - held, int(held))
    # the budget taken away: the radius is the host's again
    t.set_foveation(radius_px=7.0, ray_budget=0)
    t.sampling_launch()
    assert t.foveation_status()["r2"] == 49.0
    assert np.array_equal(t.read(TN.MASK), fnp.mask(W, H, gaze, np.float32(49.0), 1))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Mode switches
# ---------------------------------------------------------------------------------------------
def test_mode_switches_on_one_context(fovrt_mod, oracle):
    """4 -> 5 -> 6 -> 4 -> 0 on one context: after each switch MASK and the count are that mode's reference (the
    oracle for the reference modes, numpy for 5, the submitted mask for 6); back in mode 4 the mask bytes are those
    of a context that never left it."""
    TN = fovrt_mod.TextureName
    g = (61.0, 22.0)
    uni = uniforms(fovrt_mod, 1, W, H, g)
    t, never = mk(fovrt_mod), mk(fovrt_mod)
    osc = oracle.OracleScene(t.scene_arrays())
    for x in (t, never):
        x.set_camera_uniforms(uni)
        x.geometry_launch()
    inp = [t.read(v) for v in (TN.POSITION, TN.DEPTH, TN.DEPTH_CACHE, TN.WEIGHT, TN.NORMAL, TN.DIFFUSE)]
    t.enable_sampling_mask()
    own = (np.random.default_rng(3).random((H, W)) < 0.2).astype(np.uint8) * 3
    t.set_sampling_mask(own)
    refs = {4: oracle.sampling(osc, uni, W, H, 4, *inp)["mask"], 0: oracle.sampling(osc, uni, W, H, 0, *inp)["mask"],
            5: fnp.mask(W, H, g, fnp.radius_r2(fovrt_mod.foveation_default(W, H)["radius_px"]), 1),
            6: (own != 0).astype(np.uint8)}
    assert len({r.tobytes() for r in refs.values()}) == 4
    never.sampling_launch()
    for i, mode in enumerate((4, 5, 6, 4, 0)):
        if i:
            t.set_mask_mode(mode)
        assert t.mask_mode() == mode
        t.sampling_launch()
        got = t.read(TN.MASK)
        assert np.array_equal(got, refs[mode]), (i, mode, mismatch_report(got, refs[mode]))
        t.optimize_launch()
        assert t.ray_count() == int(refs[mode].sum()), (i, mode)
        if mode == 4:
            assert np.array_equal(got, never.read(TN.MASK)), i
    t.destroy(); never.destroy()


# ---------------------------------------------------------------------------------------------
# 6. Refusals write nothing
# ---------------------------------------------------------------------------------------------
def code_of(fovrt, fn, *args):
    try:
        fn(*args)
    except fovrt.FovrtError as e:
        return e.code
    return 0


def test_refusals_write_nothing(fovrt_mod):
    """Every refusal of the feature, each with its code; afterwards mode, parameters, MASK and the next frame are a
    twin's that never made the calls."""
    import torch
    lib = fovrt_mod.load_library()
    INV, STATE, UNS = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_STATE, fovrt_mod.FR_E_UNSUPPORTED
    N = W * H
    a, b = mk(fovrt_mod), mk(fovrt_mod)
    for t in (a, b):
        t.set_mask_mode(5)
        t.set_foveation(radius_px=9.0, floor_ranks=2)
        t.frame(timing=False)
    par = a.foveation()
    for kw in (dict(radius_px=float("nan")), dict(radius_px=float("inf")), dict(radius_px=0.0), dict(radius_px=-1.0),
               dict(floor_ranks=0), dict(floor_ranks=65), dict(tolerance=-0.1), dict(tolerance=1.0),
               dict(tolerance=float("nan")), dict(ray_budget=N + 1)):
        assert code_of(fovrt_mod, lambda: a.set_foveation(**kw)) == INV, kw
    assert lib.fr_set_foveation(a._ctx, None) == INV
    for mode in (-1, 7, 100):
        assert code_of(fovrt_mod, a.set_mask_mode, mode) == INV
    good = torch.ones(N + 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    host = np.ones((H, W), np.uint8)
    # not enabled
    assert code_of(fovrt_mod, a.set_sampling_mask, host) == STATE
    assert code_of(fovrt_mod, lambda: a.set_sampling_mask(good, enqueue=True)) == STATE
    a.enable_sampling_mask()
    assert code_of(fovrt_mod, a.enable_sampling_mask, 2) == 0  # (bool(2): on)
    assert lib.fr_sampling_mask_enable(a._ctx, 2) == INV
    p = C.c_void_p(good.data_ptr())
    assert lib.fr_set_sampling_mask(a._ctx, None, N, 0) == INV
    assert lib.fr_set_sampling_mask_enqueue(a._ctx, None, N, None) == INV
    assert lib.fr_set_sampling_mask(a._ctx, p, N - 1, 1) == INV
    assert lib.fr_set_sampling_mask_enqueue(a._ctx, p, N + 1, None) == INV
    assert lib.fr_set_sampling_mask(a._ctx, p, N, 2) == INV
    assert lib.fr_set_sampling_mask(a._ctx, C.c_void_p(good.data_ptr() + 1), N, 1) == INV
    assert lib.fr_set_sampling_mask_enqueue(a._ctx, C.c_void_p(good.data_ptr() + 8), N, None) == INV
    a.enable_sampling_mask(False)
    assert code_of(fovrt_mod, a.set_sampling_mask, host) == STATE
    a.enable_sampling_mask()
    # mode 6 before any mask was submitted: the launch and the frame are refused whole
    a.set_mask_mode(6)
    acc = a.m_accumFrame
    assert code_of(fovrt_mod, a.sampling_launch) == STATE
    assert code_of(fovrt_mod, lambda: a.frame(timing=False)) == STATE
    assert code_of(fovrt_mod, lambda: a.frame(timing=True)) == STATE
    assert a.m_accumFrame == acc
    a.set_mask_mode(5)
    assert a.mask_mode() == b.mask_mode() == 5 and a.foveation() == par == b.foveation()
    assert_same_outputs(fovrt_mod, a, b, "after the refusals")
    for t in (a, b):
        t.frame(timing=False)
    assert_same_outputs(fovrt_mod, a, b, "the frame after the refusals")
    a.destroy(); b.destroy()
    # a sharded context: no budget, no enqueued mask (the synchronous one works)
    TN = fovrt_mod.TextureName
    a, b = mk(fovrt_mod), mk(fovrt_mod)
    for t in (a, b):
        t.set_mask_mode(5)
        t.set_shard(0, 2, 32)
    a.enable_sampling_mask()
    par = a.foveation()
    assert code_of(fovrt_mod, lambda: a.set_foveation(ray_budget=1000)) == UNS
    assert code_of(fovrt_mod, lambda: a.set_sampling_mask(good, enqueue=True)) == UNS
    assert a.foveation() == par
    a.set_sampling_mask(good)
    for t in (a, b):
        t.trace_frame(timing=False)
    for tid in (TN.MASK, TN.WEIGHT, TN.SHADING):
        assert equal_nan(a.read(tid), b.read(tid)), ("sharded", tid)
    a.destroy(); b.destroy()
    # a context without the compaction stage
    a = mk(fovrt_mod, optimize=0)
    a.set_mask_mode(5)
    par = a.foveation()
    assert code_of(fovrt_mod, lambda: a.set_foveation(ray_budget=1000)) == UNS
    assert a.foveation() == par
    a.set_foveation(radius_px=4.0)  # (without a budget the parameters are accepted)
    a.destroy()


# ---------------------------------------------------------------------------------------------
# 7. A group
# ---------------------------------------------------------------------------------------------
def test_two_rank_group_equals_one_context(fovrt_mod):
    """A two-rank in-process group in mode 5, the same parameters on both ranks: the reconstruction ranks' outputs
    equal the one-context frame's, as the group equality tests assert for the other modes."""
    TN = fovrt_mod.TextureName
    ranks, full = [mk(fovrt_mod), mk(fovrt_mod)], mk(fovrt_mod)
    full.set_sample_sum(2)  # a group sums samples in fixed point
    g0 = (30.0, 40.0)
    for t in ranks + [full]:
        t.set_mask_mode(5)
        t.set_foveation(radius_px=14.0, floor_ranks=2)
        t.set_camera_uniforms(uniforms(fovrt_mod, 1, W, H, g0))
    g = fovrt_mod.Group(ranks, views=1, tile=32)
    for f in range(3):
        full.frame(timing=False)
        g.frame(timing=False)
    g.synchronize()
    ref = fnp.mask(W, H, g0, fnp.radius_r2(14.0), 2)
    assert np.array_equal(full.read(TN.MASK), ref)
    jfa_rank, at_rank = g.output_ranks(0)
    for r in range(2):
        if g.rank_info(r)["chains"]:
            for tid in (TN.SHADING, TN.HISTORY_CACHE):
                assert equal_nan(ranks[r].read(tid), full.read(tid)), (r, tid)
    for tid in (TN.JFA_COLOR, TN.SIBSON):
        assert equal_nan(ranks[jfa_rank].read(tid), full.read(tid)), tid
    for tid in (TN.PULLPUSH, TN.ATROUS):
        assert equal_nan(ranks[at_rank].read(tid), full.read(tid)), tid
    # a rank of a group takes no budget
    assert code_of(fovrt_mod, lambda: ranks[0].set_foveation(ray_budget=500)) == fovrt_mod.FR_E_UNSUPPORTED
    g.destroy()
    for t in ranks + [full]:
        t.destroy()


# ---------------------------------------------------------------------------------------------
# 8. Snapshot
# ---------------------------------------------------------------------------------------------
def test_snapshot_and_restore_in_mode_5(fovrt_mod):
    """A snapshot carries the mode; the context keeps its parameters: the frame after fr_restore equals the frame
    that followed the snapshot, bit for bit."""
    t = mk(fovrt_mod)
    t.set_mask_mode(5)
    t.set_foveation(radius_px=11.0, floor_ranks=3)
    t.set_camera_uniforms(uniforms(fovrt_mod, 1, W, H, (70.0, 20.0)))
    for _ in range(2):
        t.frame(timing=False)
    snap = t.snapshot()
    t.frame(timing=False)
    ids = out_ids(fovrt_mod)
    want = [t.read(i) for i in ids]
    n = t.ray_count()
    t.frame(timing=False)
    t.restore(snap)
    assert t.mask_mode() == 5 and t.foveation()["floor_ranks"] == 3
    t.frame(timing=False)
    for i, w_ in zip(ids, want):
        assert equal_nan(t.read(i), w_), i
    assert t.ray_count() == n == int(fnp.mask(W, H, (70.0, 20.0), np.float32(121.0), 3).sum())
    t.destroy()
