"""EXTRA on demand: k_sampling leaves the heat map unwritten and the context writes it (k_extra, from what the
owing launch saw) when something reads EXTRA or is about to overwrite one of its inputs. Every comparison is bit
for bit, against a context that writes EXTRA in every sampling (FOVRT_EXTRA_LAZY=0) and, where the stage calls
expose the sampling's inputs, against the oracle's heat map.

Shapes: 100x70 (ragged 16x16 blocks on both axes, cells cut by the border) and 96x64 (whole blocks); every mask
mode, since the saliency mask keeps the cell phase inside k_sampling and the others drop it.

PathTracer.read() asks for a view of the buffer first, and a view of EXTRA turns the context eager for good
(the caller may read through the pointer at any time), so the buffers are read with fr_read_buffer directly.
"""
import numpy as np
import pytest

from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan

pytestmark = pytest.mark.gpu

SIZES = [(100, 70), (96, 64)]
MODES = [0, 1, 2, 3, 4]


def make_tracer(fovrt, W, H, mask, spp=1, dmd=1):
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=1, mask_mode=mask, spp=spp, diffuse_max_depth=dmd,
                                      refraction_max_depth=16, texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR))
    assert t.initialize()
    return t


def make_pair(fovrt, monkeypatch, W, H, mask, **kw):
    monkeypatch.setenv("FOVRT_EXTRA_LAZY", "0")
    eager = make_tracer(fovrt, W, H, mask, **kw)
    monkeypatch.delenv("FOVRT_EXTRA_LAZY")
    lazy = make_tracer(fovrt, W, H, mask, **kw)
    return eager, lazy


def raw_read(fovrt, t, buf, W, H):
    """fr_read_buffer without the view PathTracer.read() takes first."""
    out = np.empty((H, W), np.uint8) if int(buf) == int(fovrt.TextureName.MASK) else np.empty((H, W, 4), np.float32)
    t._check(fovrt._lib.fr_read_buffer(t._ctx, int(buf), out.ctypes.data, out.nbytes))
    return out


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("mask_mode", MODES)
def test_extra_on_demand_stage_calls(fovrt_mod, oracle, monkeypatch, W, H, mask_mode):
    TN = fovrt_mod.TextureName
    eager, lazy = make_pair(fovrt_mod, monkeypatch, W, H, mask_mode)
    both = (eager, lazy)
    rd = lambda t, b: raw_read(fovrt_mod, t, b, W, H)
    cam = fovrt_mod.Camera.preset(1, W, H)
    osc = oracle.OracleScene(lazy.scene_arrays())
    inputs = (TN.POSITION, TN.DEPTH, TN.DEPTH_CACHE, TN.WEIGHT, TN.NORMAL, TN.DIFFUSE)

    def uniforms(gx, gy):
        u = cam.uniforms(W, H)
        u.gaze[0], u.gaze[1] = gx, gy
        for t in both:
            t.set_camera_uniforms(u)
        return u

    def geometry_and_sampling(u):
        for t in both:
            t.geometry_launch()
        inp = [rd(lazy, b) for b in inputs]
        for t in both:
            t.sampling_launch()
        return oracle.sampling(osc, u, W, H, mask_mode, *inp)["extra"]

    def finish_frame():
        for t in both:
            t.optimize_launch()
            t.shading_launch()

    # geometry, sampling, read
    u = uniforms(0.3 * W, 0.7 * H)
    ref = geometry_and_sampling(u)
    e = rd(lazy, TN.EXTRA)
    assert same_bits(e, rd(eager, TN.EXTRA)) and equal_nan(e, ref), "after the stage calls"
    finish_frame()

    # sampling (second frame: a depth cache and reprojected positions exist), the gaze moved, then a stage-call
    # G-buffer from another camera: still the first launch's heat map (its gaze, DIFFUSE, DEPTH, NORMAL, WEIGHT)
    cam.setPrevState()
    cam.lookAt(np.asarray(cam.target) + np.array([0.02, 0.01, 0.0], np.float32))
    u = uniforms(0.6 * W, 0.4 * H)
    ref = geometry_and_sampling(u)
    cam.setPrevState()
    cam.lookAt(np.asarray(cam.target) + np.array([-0.05, 0.03, 0.0], np.float32))
    u = uniforms(0.1 * W, 0.2 * H)
    for t in both:
        t.geometry_launch()
    e = rd(lazy, TN.EXTRA)
    assert same_bits(e, rd(eager, TN.EXTRA)) and equal_nan(e, ref), "after a later G-buffer"

    # sampling, a new gaze alone, read
    for t in both:
        t.sampling_launch()
    for t in both:
        t.set_gaze(0.9 * W, 0.1 * H)
    assert same_bits(rd(lazy, TN.EXTRA), rd(eager, TN.EXTRA)), "after set_gaze"

    # sampling, then the caller overwrites an input
    for k, buf in enumerate((TN.DIFFUSE, TN.NORMAL, TN.DEPTH, TN.WEIGHT)):
        inp = [rd(lazy, b) for b in inputs]
        for t in both:
            t.sampling_launch()
        u = cam.uniforms(W, H)
        # the gaze set_gaze(0.9 W, 0.1 H) left: (LONG(x), H - LONG(1.25 y)) for a windowed cursor
        u.gaze[0], u.gaze[1] = np.float32(int(0.9 * W)), np.float32(H - int(0.1 * H * 1.25))
        ref = oracle.sampling(osc, u, W, H, mask_mode, *inp)["extra"]
        for t in both:
            t.write(buf, np.full((H, W, 4), 0.25 * k, np.float32))
        e = rd(lazy, TN.EXTRA)
        assert same_bits(e, rd(eager, TN.EXTRA)) and equal_nan(e, ref), ("after a write of", int(buf))
        for t in both:  # fresh inputs for the next round
            t.geometry_launch()

    # sampling, then the caller's own EXTRA: its bytes win
    mine = np.random.default_rng(5).random((H, W, 4), dtype=np.float32)
    for t in both:
        t.sampling_launch()
        t.write(TN.EXTRA, mine)
    assert same_bits(rd(lazy, TN.EXTRA), mine) and same_bits(rd(eager, TN.EXTRA), mine)
    eager.destroy()
    lazy.destroy()


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("mask_mode", MODES)
def test_extra_on_demand_frames(fovrt_mod, monkeypatch, W, H, mask_mode):
    import torch
    TN = fovrt_mod.TextureName
    eager, lazy = make_pair(fovrt_mod, monkeypatch, W, H, mask_mode, spp=2)
    both = (eager, lazy)
    rd = lambda t, b: raw_read(fovrt_mod, t, b, W, H)
    cam = fovrt_mod.Camera.preset(1, W, H)
    images = (TN.EXTRA, TN.SHADING, TN.SIBSON, TN.PULLPUSH, TN.ATROUS, TN.WEIGHT, TN.MASK)

    def frames(n, timing=False):
        for _ in range(n):
            cam.setPrevState()
            cam.lookAt(np.asarray(cam.target) + np.array([0.01, 0.005, 0.0], np.float32))
            for t in both:
                t.update_optix_variables(cam)
                t.set_gaze(0.3 * W, 0.6 * H / 1.25)
                t.frame(timing=timing)

    def check(what, bufs=images):
        for b in bufs:
            assert same_bits(rd(lazy, b), rd(eager, b)), (what, int(b))

    # pipelined frames with a moving camera and an off-centre gaze, then one timed (serial) frame
    frames(4)
    check("after four frames")
    frames(1, timing=True)
    check("after a timed frame")
    # frame, the gaze moved, read: the frame's gaze
    frames(1)
    for t in both:
        t.set_gaze(0.8 * W, 0.2 * H)
    check("after set_gaze", (TN.EXTRA,))
    # snapshot, more frames, restore (the depth pair is overwritten while EXTRA is owed), read, next frame
    frames(1)
    snaps = [t.snapshot() for t in both]
    frames(2)
    for t, s in zip(both, snaps):
        t.restore(s)
    check("after restore", (TN.EXTRA,))
    frames(1)
    check("the frame after restore")
    # a view of EXTRA: later frames' heat maps are in the buffer without another call asking for it
    views = [t.view(TN.EXTRA) for t in both]
    frames(2)
    out = [torch.empty(H * W * 4, dtype=torch.float32, device="cuda") for _ in both]
    for t, v, o in zip(both, views, out):
        t.synchronize()
        t.composite_views(v.device_ptr, 1, o.data_ptr(), o.numel() * 4)  # a plain copy from the pointer
    assert same_bits(out[1].cpu().numpy(), out[0].cpu().numpy()), "through the view"
    assert same_bits(out[1].cpu().numpy().reshape(H, W, 4), rd(eager, TN.EXTRA))
    eager.destroy()
    lazy.destroy()
