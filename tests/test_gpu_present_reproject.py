"""GPU suite for the reprojected present (k_present_splat, k_present_resolve: a depth-aware splat of POSITION): the
kernels in bytes against the numpy restatement on the shared case set, after traced frames, between pipelined frames
against a twin context that reads the float images after the same frame, sharing the ring with the other presents,
around other calls, the refusals, and a context that never enables the feature.

Scene 1 (the bunny preset), procedural detail 1, 100 x 70 unless a size is given, 2 spp. No test here synchronises a
presenting context between an enqueue and its acquire: the acquire is the only wait."""
import ctypes as C

import numpy as np
import pytest

import present_blend_np as pbn
import present_np as pnp
import present_reproject_cases as prc
import present_reproject_np as prn
import present_warp_np as pwn
from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan
from test_gpu_bvh import mismatch_report
from test_gpu_present import H, SPP, W, assert_same_state, mk, take
from test_gpu_present_warp import camera_states

pytestmark = pytest.mark.gpu


def ref(img, pos, rp, fmt):
    return prn.reproject(img, pos, rp.vp, rp.fallback.h, rp.fallback.out_width, rp.fallback.out_height, fmt)


def late(fovrt, cams, k, ow=W, oh=H):
    """Frame k's image shown for frame k + 1's pose."""
    return fovrt.PresentReproject.from_poses(cams[k], cams[k + 1], W, H, ow, oh)


# ---------------------------------------------------------------------------------------------
# 1. The kernels are the rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,ow,oh", prc.SCREENS)
def test_kernel_is_the_rule(fovrt_mod, w, h, ow, oh):
    """Every POSITION case and display pose of the shared set, POSITION and the four presentable buffers written with
    fr_write_buffer (ATROUS after one A-Trous pass, so that the image the view names is the pass's output), presented
    reprojected to the host and into a torch tensor: the bytes are present_reproject_np's in every format."""
    import torch
    TN = fovrt_mod.TextureName
    t = mk(fovrt_mod, w, h)
    fovrt_mod.ATrous(t).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    bufs = (TN.SIBSON, TN.PULLPUSH, TN.SHADING, TN.ATROUS)
    imgs = prc.sources(w, h)
    for b, img in zip(bufs, imgs):
        t.write(b, img)
    rps = prc.reprojections(fovrt_mod, w, h, ow, oh)
    positions = [prc.position(fovrt_mod, name, w, h) for name in prc.POSITIONS]
    n = ow * oh * 4
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    for f, fmt in enumerate(pnp.FORMATS):
        t.present_enable(3, fmt)
        t.present_reproject_enable()
        for i, (pname, pos) in enumerate(zip(prc.POSITIONS, positions)):
            t.write(TN.POSITION, pos)
            for j, (dname, rp) in enumerate(rps):
                b = (f + i + j) % 4
                want = ref(imgs[b], pos, rp, fmt)
                ticket = t.present_reprojected(bufs[b], rp)
                t.present_reprojected_to(bufs[b], rp, dst)
                take(t, ticket, want, (w, h, fmt, pname, dname, bufs[b], "host"))
                t.present_done(s)
                got = dst.cpu().numpy().reshape(want.shape)  # (on torch's current stream, behind the kernels)
                assert np.array_equal(got, want), (w, h, fmt, pname, dname, bufs[b], "device", mismatch_report(got, want))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Traced frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [1, 2])
def test_traced_frames(fovrt_mod, scene):
    """After a real frame of the scene's preset view, ATROUS and SHADING shown for a shifted and turned pose: the bytes
    are the restatement over what fr_read_buffer gives of POSITION and the source afterwards."""
    TN = fovrt_mod.TextureName
    t = fovrt_mod.PathTracer(fovrt_mod.Config(width=W, height=H, scene=scene, mask_mode=4, spp=SPP, diffuse_max_depth=1,
                                              texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, detail=1))
    assert t.initialize()
    cam = fovrt_mod.Camera.preset(scene, W, H)
    shown = pwn.turned(fovrt_mod, cam, 1, 1.5, (0.04, -0.02, 0.03))
    t.set_camera_uniforms(cam.uniforms(W, H))
    t.present_enable(2, pnp.BGRA8)
    t.present_reproject_enable()
    t.frame(timing=False)
    rp = fovrt_mod.PresentReproject.from_poses(cam, shown, W, H, W, H, 0.99)
    small = fovrt_mod.PresentReproject.from_poses(cam, shown, W, H, 61, 43, 0.99)
    tickets = [t.present_reprojected(TN.ATROUS, rp), t.present_reprojected(TN.SHADING, small)]
    pos = t.read(TN.POSITION)
    assert (pos[..., :3] != 0).any(-1).mean() > 0.3  # the view sees the scene
    want = [ref(t.read(TN.ATROUS), pos, rp, pnp.BGRA8), ref(t.read(TN.SHADING), pos, small, pnp.BGRA8)]
    covered, crack = prn.zones(prn.splat(t.read(TN.ATROUS), pos, rp.vp, W, H, pnp.BGRA8))
    assert covered.any() and (~covered & ~crack).any()  # both the splat and the fallback show
    take(t, tickets[0], want[0], (scene, "ATROUS"))
    take(t, tickets[1], want[1], (scene, "SHADING at 61 x 43"))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Pipelined frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latency,iters,overlap", [(False, 1, False), (True, 1, False), (False, 2, False),
                                                   (True, 2, False), (False, 1, True)])
def test_pipelined_frames(fovrt_mod, latency, iters, overlap):
    """Eight untimed frames with the camera and the gaze moved before each and a reprojected present after every frame,
    from that frame's pose to the next frame's: ATROUS on one context, SHADING at a smaller size on another; three
    slots, ticket k - 2 taken after ticket k is enqueued, no synchronize. Every image is the restatement over what a
    twin reads of POSITION and the source after the same frame, and after the eighth frame both presenting contexts are
    the twin, bit for bit. overlap: overlapped geometry updates with a pose enqueued before each frame."""
    TN = fovrt_mod.TextureName
    N = 8
    a, s, twin = (mk(fovrt_mod, latency=latency, atrous_iterations=iters) for _ in range(3))
    everyone = (a, s, twin)
    if overlap:
        from test_gpu_pose import pose, rest
        pos0, _nrm0, _ = rest(twin)
        models = twin.models()
        for t in everyone:
            t.enable_model_pose()
            t.set_geometry_overlap(True)
    fmt_a, fmt_s = pnp.BGRA8, pnp.RGBA8 | pnp.TOP_DOWN
    a.present_enable(3, fmt_a)
    s.present_enable(3, fmt_s)
    a.present_reproject_enable()
    s.present_reproject_enable()
    cams, unis = camera_states(fovrt_mod, N + 1)
    want_a, want_s, tick_a, tick_s = [], [], [], []
    for k in range(N):
        for t in everyone:
            t.set_camera_uniforms(unis[k])
            if overlap:
                t.set_model_transforms(pose("turning", pos0, models, k), enqueue=True)
        rp_a = late(fovrt_mod, cams, k, W - 4 * (k % 2), H - (k % 3))
        rp_s = late(fovrt_mod, cams, k, 64 + k, 41)
        a.frame(timing=False)
        tick_a.append(a.present_reprojected(TN.ATROUS, rp_a))
        s.frame(timing=False)
        tick_s.append(s.present_reprojected(TN.SHADING, rp_s))
        twin.frame(timing=False)
        pos = twin.read(TN.POSITION)
        want_a.append(ref(twin.read(TN.ATROUS), pos, rp_a, fmt_a))
        want_s.append(ref(twin.read(TN.SHADING), pos, rp_s, fmt_s))
        if k:  # consecutive images differ in bytes, or a present of the wrong frame would pass
            assert want_a[k].shape != want_a[k - 1].shape or not np.array_equal(want_a[k], want_a[k - 1]), k
            assert want_s[k].shape != want_s[k - 1].shape or not np.array_equal(want_s[k], want_s[k - 1]), k
        assert tick_a[k] == k + 1 and tick_s[k] == k + 1
        if k >= 2:
            take(a, tick_a[k - 2], want_a[k - 2], ("atrous", latency, iters, overlap, k - 2))
            take(s, tick_s[k - 2], want_s[k - 2], ("shading", latency, iters, overlap, k - 2))
    for k in (N - 2, N - 1):
        take(a, tick_a[k], want_a[k], ("atrous", latency, iters, overlap, k))
        take(s, tick_s[k], want_s[k], ("shading", latency, iters, overlap, k))
    assert_same_state(fovrt_mod, a, twin, "the context that presents ATROUS reprojected")
    assert_same_state(fovrt_mod, s, twin, "the context that presents SHADING reprojected")
    for t in everyone:
        t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Mixed use
# ---------------------------------------------------------------------------------------------
def test_shares_the_ring(fovrt_mod):
    """After each of two frames: ATROUS plain, SHADING warped, a blend, SIBSON reprojected (eight slots, nothing taken
    before the last is enqueued). Tickets count across the four kinds; times come back for a reprojected ticket; a
    full ring refuses the reprojected call and enqueues nothing."""
    TN = fovrt_mod.TextureName
    lib = fovrt_mod.load_library()
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    fmt = pnp.RGBA8
    t.present_enable(8, fmt)
    t.present_reproject_enable()
    cams, unis = camera_states(fovrt_mod, 3)
    crop = fovrt_mod.PresentWarp.crop(40, 30, 37, 25)
    blend = fovrt_mod.PresentBlend((47.0, 31.0), 12.0, 30.0, TN.SIBSON, TN.ATROUS)
    tickets, want = [], []
    for k in range(2):
        for x in (t, twin):
            x.set_camera_uniforms(unis[k])
            x.frame(timing=False)
        rp = late(fovrt_mod, cams, k, 96, 67)
        tickets += [t.present(TN.ATROUS), t.present_warped(TN.SHADING, crop), t.present_blended(blend),
                    t.present_reprojected(TN.SIBSON, rp)]
        sh, at, sib = twin.read(TN.SHADING), twin.read(TN.ATROUS), twin.read(TN.SIBSON)
        want += [pnp.pack(at, fmt), pwn.warp(sh, crop.h, 37, 25, fmt), pbn.pack(sib, at, (47.0, 31.0), 12.0, 30.0, fmt),
                 ref(sib, twin.read(TN.POSITION), rp, fmt)]
    assert tickets == list(range(1, 9))
    tk = C.c_uint64(99)
    keep = rp.c_struct()
    assert lib.fr_present_enqueue_reprojected(t._ctx, int(TN.ATROUS), C.byref(keep), C.byref(tk)) == fovrt_mod.FR_E_STATE
    assert tk.value == 99
    for x in (t, twin):
        x.set_camera_uniforms(unis[2])
        x.frame(timing=False)
    for i, (ticket, w_) in enumerate(zip(tickets, want)):
        got = t.present_acquire(ticket)
        assert got.shape == w_.shape and np.array_equal(got, w_), (i, mismatch_report(got, w_))
        if i % 4 == 3:
            times = t.present_times(ticket)
            assert times["pack_ms"] >= 0 and times["copy_ms"] >= 0
        t.present_release(ticket)
    assert_same_state(fovrt_mod, t, twin, "four kinds of present in one ring")
    t.destroy(); twin.destroy()


def test_around_other_calls(fovrt_mod):
    """Reprojected presents between stage calls, before and after fr_write_buffer(FR_BUF_POSITION), across
    fr_snapshot / fr_restore and after a timed frame: each sees the image and POSITION as they stand at its place in
    the stream order."""
    TN = fovrt_mod.TextureName
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    cams, unis = camera_states(fovrt_mod, 4)
    fmt = pnp.BGRA8 | pnp.TOP_DOWN
    t.present_enable(3, fmt)
    t.present_reproject_enable()
    rps = [late(fovrt_mod, cams, k) for k in range(3)]
    for x in (t, twin):
        x.set_camera_uniforms(unis[0])
        x.frame(timing=False)
    # between stage calls: the present sees the Sibson pass's image and the frame's POSITION, not the G-buffer stage
    # call that overwrites POSITION afterwards (the slot moves on, and the write below goes to the new slot's image)
    for x in (t, twin):
        fovrt_mod.JumpFlooding(x).render(TN.SHADING)
        fovrt_mod.SibsonInterpolation(x).render()
    pos0 = twin.read(TN.POSITION)
    first = ref(twin.read(TN.SIBSON), pos0, rps[0], fmt)
    tk = t.present_reprojected(TN.SIBSON, rps[0])
    for x in (t, twin):
        x.set_camera_uniforms(unis[1])
        x.geometry_launch()
    take(t, tk, first, "a reprojected present between a stage call and a G-buffer stage call")
    # before and after a write of POSITION
    pos1 = twin.read(TN.POSITION)
    assert not equal_nan(pos0, pos1)
    tk = t.present_reprojected(TN.SIBSON, rps[0])
    other = prc.position(fovrt_mod, prc.POSITIONS[1], W, H)
    for x in (t, twin):
        x.write(TN.POSITION, other)
    sib = twin.read(TN.SIBSON)
    before, after = ref(sib, pos1, rps[0], fmt), ref(sib, other, rps[0], fmt)
    assert not np.array_equal(before, after)
    take(t, tk, before, "a reprojected present before a write of POSITION")
    tk = t.present_reprojected(TN.SIBSON, rps[0])
    take(t, tk, after, "a reprojected present after a write of POSITION")
    # across snapshot / restore: the ticket enqueued before survives both, and the frame after equals the twin's
    for x in (t, twin):
        x.set_camera_uniforms(unis[1])
        x.frame(timing=False)
    want = ref(twin.read(TN.ATROUS), twin.read(TN.POSITION), rps[1], fmt)
    tk = t.present_reprojected(TN.ATROUS, rps[1])
    snaps = [x.snapshot() for x in (t, twin)]
    assert snaps[0] == snaps[1]
    for x, sn in zip((t, twin), snaps):
        x.set_camera_uniforms(unis[2])
        x.frame(timing=False)
        x.restore(sn)
    take(t, tk, want, "a reprojected present across snapshot and restore")
    tk = t.present_reprojected(TN.ATROUS, rps[1])
    take(t, tk, ref(twin.read(TN.ATROUS), twin.read(TN.POSITION), rps[1], fmt), "right after the restore")
    for x in (t, twin):
        x.set_camera_uniforms(unis[2])
        x.frame(timing=False)
    tk = t.present_reprojected(TN.ATROUS, rps[2])
    take(t, tk, ref(twin.read(TN.ATROUS), twin.read(TN.POSITION), rps[2], fmt), "the frame after the restore")
    # after a timed frame (every stage on the context stream, synchronised)
    for x in (t, twin):
        x.set_camera_uniforms(unis[0])
        x.frame(timing=True)
    tks = [t.present_reprojected(TN.ATROUS, rps[0]), t.present_reprojected(TN.SHADING, rps[0]), t.present(TN.SHADING)]
    pos = twin.read(TN.POSITION)
    take(t, tks[0], ref(twin.read(TN.ATROUS), pos, rps[0], fmt), "after a timed frame, ATROUS")
    take(t, tks[1], ref(twin.read(TN.SHADING), pos, rps[0], fmt), "after a timed frame, SHADING")
    take(t, tks[2], pnp.pack(twin.read(TN.SHADING), fmt), "after a timed frame, SHADING plain")
    assert_same_state(fovrt_mod, t, twin, "reprojected presents around other calls")
    t.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Refusals, and a context that never enables the feature
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(fovrt_mod):
    """Every refusal of the header's list for the enable and the two reprojected calls, each followed by a frame that
    equals the twin's; nothing is written to the destination and no ticket is taken; on a rank of a group both enqueues
    are FR_E_UNSUPPORTED."""
    import torch
    TN = fovrt_mod.TextureName
    lib = fovrt_mod.load_library()
    INV, STATE, UNS = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_STATE, fovrt_mod.FR_E_UNSUPPORTED
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    cams, unis = camera_states(fovrt_mod, 3)
    dst = torch.full((H * W * 4 + 64,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dp = dst.data_ptr()
    AT = int(TN.ATROUS)
    tk = C.c_uint64(99)
    state = {"k": 0}
    keep = []
    good = late(fovrt_mod, cams, 0)

    def rp(vp=None, hm=None, ow=W, oh=H):
        r = fovrt_mod.PresentReproject(good.vp if vp is None else vp,
                                       fovrt_mod.PresentWarp(good.fallback.h if hm is None else hm, ow, oh))
        keep.append(r.c_struct())
        return C.byref(keep[-1])

    def refused(code, what, fn, *args):
        assert fn(t._ctx, *args) == code, what
        assert tk.value == 99, what
        k = state["k"] = (state["k"] + 1) % 3
        for x in (t, twin):
            x.set_camera_uniforms(unis[k])
            x.frame(timing=False)
        for b in (TN.SHADING, TN.SIBSON, TN.ATROUS, TN.POSITION):
            assert equal_nan(t.read(b), twin.read(b)), (what, b)
        assert (dst.cpu().numpy() == 7).all(), what

    host, dev, enable = lib.fr_present_enqueue_reprojected, lib.fr_present_enqueue_reprojected_device, lib.fr_present_reproject_enable
    full = W * H * 4
    # before the ring is on: the enable and both enqueues
    refused(STATE, "enable before fr_present_enable", enable, 1)
    refused(STATE, "enqueue, no ring", host, AT, rp(), C.byref(tk))
    refused(STATE, "device enqueue, no ring", dev, AT, rp(), C.c_void_p(dp), full)
    t.present_enable(2, pnp.RGBA8)
    # the ring is on, the feature is not
    refused(STATE, "enqueue, not enabled", host, AT, rp(), C.byref(tk))
    refused(STATE, "device enqueue, not enabled", dev, AT, rp(), C.c_void_p(dp), full)
    t.present_reproject_enable()
    t.present_reproject_enable(False)
    refused(STATE, "enqueue, turned off", host, AT, rp(), C.byref(tk))
    refused(STATE, "device enqueue, turned off", dev, AT, rp(), C.c_void_p(dp), full)
    t.present_reproject_enable()
    refused(INV, "NULL ticket", host, AT, rp(), None)
    refused(INV, "NULL rp", host, AT, None, C.byref(tk))
    refused(INV, "NULL rp, device", dev, AT, None, C.c_void_p(dp), full)
    for k in (0, 6, 15):
        for bad in (np.nan, -np.inf):
            vp = good.vp.copy()
            vp[k] = bad
            refused(INV, ("vp", k, bad), host, AT, rp(vp=vp), C.byref(tk))
            refused(INV, ("vp, device", k, bad), dev, AT, rp(vp=vp), C.c_void_p(dp), full)
    for k in (0, 8):
        hm = good.fallback.h.copy()
        hm[k] = np.inf
        refused(INV, ("fallback coefficient", k), host, AT, rp(hm=hm), C.byref(tk))
        refused(INV, ("fallback coefficient, device", k), dev, AT, rp(hm=hm), C.c_void_p(dp), full)
    for ow, oh in ((W + 1, H), (W, H + 1), (0, H), (W, 0), (-1, H), (W, -4)):
        refused(INV, ("size", ow, oh), host, AT, rp(ow=ow, oh=oh), C.byref(tk))
        refused(INV, ("size, device", ow, oh), dev, AT, rp(ow=ow, oh=oh), C.c_void_p(dp), max(ow, 1) * max(oh, 1) * 4)
    for b in (TN.POSITION, TN.EXTRA, TN.MASK, 99, -1):
        refused(INV, ("buffer", b), host, int(b), rp(), C.byref(tk))
        refused(INV, ("device buffer", b), dev, int(b), rp(), C.c_void_p(dp), full)
    small = 40 * 30 * 4
    refused(INV, "bytes of the whole screen for a smaller output", dev, AT, rp(ow=40, oh=30), C.c_void_p(dp), full)
    refused(INV, "bytes short", dev, AT, rp(ow=40, oh=30), C.c_void_p(dp), small - 4)
    refused(INV, "bytes long", dev, AT, rp(ow=40, oh=30), C.c_void_p(dp), small + 4)
    refused(INV, "misaligned", dev, AT, rp(ow=40, oh=30), C.c_void_p(dp + 4), small)
    refused(INV, "NULL device_dst", dev, AT, rp(ow=40, oh=30), None, small)
    # the ring full
    held = [t.present(TN.ATROUS), t.present(TN.ATROUS)]
    refused(STATE, "the ring is full", host, AT, rp(), C.byref(tk))
    for ticket in held:
        t.present_release(ticket)
    # the feature still works afterwards, and no refusal took a ticket
    r40 = fovrt_mod.PresentReproject(good.vp, fovrt_mod.PresentWarp(good.fallback.h, 40, 30))
    ticket = t.present_reprojected(TN.ATROUS, r40)
    assert ticket == 3
    t.present_reprojected_to(TN.ATROUS, r40, dst[:small])
    want = ref(twin.read(TN.ATROUS), twin.read(TN.POSITION), r40, pnp.RGBA8)
    take(t, ticket, want, "after the refusals")
    t.present_done(torch.cuda.current_stream())
    got = dst.cpu().numpy()
    assert np.array_equal(got[:small].reshape(30, 40, 4), want) and (got[small:] == 7).all()  # ow * oh * 4 bytes, no more
    dst.fill_(7)
    torch.cuda.synchronize()
    # a rank of a group
    other = mk(fovrt_mod)
    g = fovrt_mod.Group([t, other], views=1, tile=32)
    assert host(t._ctx, AT, rp(), C.byref(tk)) == UNS and tk.value == 99
    assert dev(t._ctx, AT, rp(), C.c_void_p(dp), full) == UNS
    g.synchronize()
    assert (dst.cpu().numpy() == 7).all()
    g.destroy()
    t.destroy(); twin.destroy(); other.destroy()


def test_never_enabled_is_untouched(fovrt_mod):
    """A context that presents plain and warped images but never calls fr_present_reproject_enable: its frames, in
    both pipeline modes, are the twin's, its presents are right, and the reprojected call is refused."""
    TN = fovrt_mod.TextureName
    for latency in (False, True):
        t, twin = mk(fovrt_mod, latency=latency), mk(fovrt_mod, latency=latency)
        cams, unis = camera_states(fovrt_mod, 5)
        t.present_enable(3, pnp.RGBA8)
        for k in range(4):
            for x in (t, twin):
                x.set_camera_uniforms(unis[k])
                x.frame(timing=False)
            wp = fovrt_mod.PresentWarp.from_poses(cams[k], cams[k + 1], W, H)
            tks = [t.present(TN.SHADING), t.present_warped(TN.ATROUS, wp)]
            with pytest.raises(fovrt_mod.FovrtError):
                t.present_reprojected(TN.ATROUS, late(fovrt_mod, cams, k))
            take(t, tks[0], pnp.pack(twin.read(TN.SHADING), pnp.RGBA8), ("plain", latency, k))
            take(t, tks[1], pwn.warp(twin.read(TN.ATROUS), wp.h, W, H, pnp.RGBA8), ("warped", latency, k))
        assert_same_state(fovrt_mod, t, twin, ("never enabled", latency))
        t.destroy(); twin.destroy()
