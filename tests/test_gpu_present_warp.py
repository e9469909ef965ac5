"""GPU suite for the warped present (k_present_warp: a homography between the image and the 8-bit texels): the kernel in
bytes against the numpy restatement on the shared case set, warped presents between pipelined frames against a twin
context that reads the float image after the same frame, plain and warped presents sharing the ring and standing
around other calls, and the refusals.

Scene 1 (the bunny preset), procedural detail 1, 100 x 70 unless a size is given, 2 spp. No test here synchronises a
presenting context between an enqueue and its acquire: the acquire is the only wait."""
import ctypes as C

import numpy as np
import pytest

import present_np as pnp
import present_warp_np as pwn
from helpers import equal_nan
from test_gpu_bvh import mismatch_report
from test_gpu_present import H, W, assert_same_state, mk, take

pytestmark = pytest.mark.gpu


def PW(fovrt, h, ow=0, oh=0):
    return fovrt.PresentWarp(h, ow, oh)


def camera_states(fovrt, n, w=W, h=H):
    """n cameras and their uniforms, each moved and turned against the one before (and reprojecting from it), with a
    gaze that moves too: consecutive frames differ, and so do consecutive poses."""
    cams, unis, prev = [], [], None
    for k in range(n):
        cam = fovrt.Camera.preset(1, w, h)
        tgt = cam.target.copy()
        cam.setPosition(cam.pos + np.array([0.05 * k, 0.02 * k, -0.04 * k], np.float32))
        cam.lookAt(tgt + np.array([0.03 * k, -0.02 * k, 0.0], np.float32))
        cam.prev = prev
        prev = (cam.pos.copy(), cam.rot.copy(), cam.fovy, cam.znear, cam.zfar, cam.aspect)
        u = cam.uniforms(w, h)
        u.gaze[0], u.gaze[1] = float(18 + 9 * k), float(12 + 6 * k)
        cams.append(cam)
        unis.append(u)
    return cams, unis


def foveal_crop(fovrt, gaze, ow=33, oh=21, w=W, h=H):
    """The ow x oh texels around the gaze, kept inside the screen."""
    x0 = int(min(max(gaze[0] - ow // 2, 0), w - ow))
    y0 = int(min(max(gaze[1] - oh // 2, 0), h - oh))
    return fovrt.PresentWarp.crop(x0, y0, ow, oh)


# ---------------------------------------------------------------------------------------------
# 1. The kernel is the rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", pwn.SCREENS)
def test_kernel_is_the_rule(fovrt_mod, w, h):
    """The shared case set over the present suite's value set, written into each presentable buffer (ATROUS after one
    A-Trous pass, so that the image the view names is the pass's output), presented warped to the host and into a
    torch tensor: the bytes are present_warp_np's in every format, each case on a buffer that changes with the format;
    and the identity is the plain present's image of the same buffer."""
    import torch
    TN = fovrt_mod.TextureName
    t = mk(fovrt_mod, w, h)
    fovrt_mod.ATrous(t).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    bufs = (TN.SIBSON, TN.PULLPUSH, TN.SHADING, TN.ATROUS)
    imgs = [pwn.source(w, h, k) for k in range(4)]
    for b, img in zip(bufs, imgs):
        t.write(b, img)
    cases = pwn.cases(fovrt_mod, w, h)
    dst = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    for i, fmt in enumerate(pnp.FORMATS):
        t.present_enable(3, fmt)
        for j, (name, hm, ow, oh) in enumerate(cases):
            b = (i + j) % 4
            wp = PW(fovrt_mod, hm, ow, oh)
            ref = pwn.warp(imgs[b], hm, ow, oh, fmt)
            n = ref.size
            ticket = t.present_warped(bufs[b], wp)
            t.present_warped_to(bufs[b], wp, dst[:n])
            take(t, ticket, ref, (w, h, fmt, name, bufs[b], "host"))
            t.present_done(s)
            got = dst[:n].cpu().numpy().reshape(ref.shape)  # (on torch's current stream, behind the kernel)
            assert np.array_equal(got, ref), (w, h, fmt, name, bufs[b], "device", mismatch_report(got, ref))
        for b in range(4):
            plain, warped = t.present(bufs[b]), t.present_warped(bufs[b], fovrt_mod.PresentWarp.identity())
            ref = pnp.pack(imgs[b], fmt)
            take(t, plain, ref, (w, h, fmt, bufs[b], "plain"))
            take(t, warped, ref, (w, h, fmt, bufs[b], "identity"))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Pipelined frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latency,iters,overlap", [(False, 1, False), (True, 1, False), (False, 2, False),
                                                   (True, 2, False), (False, 1, True)])
def test_pipelined_frames(fovrt_mod, latency, iters, overlap):
    """Eight untimed frames with the camera and the gaze moved before each and a warped present after every frame:
    ATROUS reprojected from that frame's pose to the next frame's on one context, a foveal crop of SIBSON around the
    gaze on another; three slots, ticket k - 2 taken after ticket k is enqueued, no synchronize. Every image is
    present_warp_np over what a twin reads after the same frame, and after the eighth frame both presenting contexts
    are the twin, bit for bit. overlap: overlapped geometry updates with a pose enqueued before each frame."""
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
    cams, unis = camera_states(fovrt_mod, N + 1)
    want_a, want_s, tick_a, tick_s = [], [], [], []
    for k in range(N):
        for t in everyone:
            t.set_camera_uniforms(unis[k])
            if overlap:
                t.set_model_transforms(pose("turning", pos0, models, k), enqueue=True)
        late = fovrt_mod.PresentWarp.from_poses(cams[k], cams[k + 1], W, H, W - 4 * (k % 2), H - (k % 3))
        crop = foveal_crop(fovrt_mod, (unis[k].gaze[0], unis[k].gaze[1]))
        assert not np.array_equal(late.h, np.array(pwn.IDENTITY, np.float32))
        a.frame(timing=False)
        tick_a.append(a.present_warped(TN.ATROUS, late))
        s.frame(timing=False)
        tick_s.append(s.present_warped(TN.SIBSON, crop))
        twin.frame(timing=False)
        want_a.append(pwn.warp(twin.read(TN.ATROUS), late.h, late.out_width, late.out_height, fmt_a))
        want_s.append(pwn.warp(twin.read(TN.SIBSON), crop.h, crop.out_width, crop.out_height, fmt_s))
        if k:  # consecutive images differ in bytes, or a present of the wrong frame would pass
            assert want_a[k].shape != want_a[k - 1].shape or not np.array_equal(want_a[k], want_a[k - 1]), k
            assert not np.array_equal(want_s[k], want_s[k - 1]), k
        assert tick_a[k] == k + 1 and tick_s[k] == k + 1
        if k >= 2:
            take(a, tick_a[k - 2], want_a[k - 2], ("atrous", latency, iters, overlap, k - 2))
            take(s, tick_s[k - 2], want_s[k - 2], ("sibson", latency, iters, overlap, k - 2))
    for k in (N - 2, N - 1):
        take(a, tick_a[k], want_a[k], ("atrous", latency, iters, overlap, k))
        take(s, tick_s[k], want_s[k], ("sibson", latency, iters, overlap, k))
    assert_same_state(fovrt_mod, a, twin, "the context that presents ATROUS reprojected")
    assert_same_state(fovrt_mod, s, twin, "the context that presents a crop of SIBSON")
    for t in everyone:
        t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Mixed use: one ring for plain and warped presents, and presents around other calls
# ---------------------------------------------------------------------------------------------
def test_plain_and_warped_share_the_ring(fovrt_mod):
    """After each of four frames: SHADING plain, SHADING cropped, ATROUS at half size (eight slots, nothing taken
    before the last frame is enqueued, so the SHADING of frame k is read while the later frames rotate through the
    other slots). Tickets count across both kinds; times come back for both; a ticket released without being acquired
    frees its slot; a full ring refuses either kind and enqueues nothing."""
    TN = fovrt_mod.TextureName
    lib = fovrt_mod.load_library()
    STATE = fovrt_mod.FR_E_STATE
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    fmt = pnp.RGBA8
    t.present_enable(8, fmt)
    _cams, unis = camera_states(fovrt_mod, 4)
    crop = fovrt_mod.PresentWarp.crop(40, 30, 37, 25)
    half = fovrt_mod.PresentWarp.scale(W, H, W // 2, H // 2)
    tickets, want = [], []
    tk = C.c_uint64(99)
    for k in range(4):
        for x in (t, twin):
            x.set_camera_uniforms(unis[k])
            x.frame(timing=False)
        if k < 2:
            tickets += [t.present(TN.SHADING), t.present_warped(TN.SHADING, crop), t.present_warped(TN.ATROUS, half)]
            sh, at = twin.read(TN.SHADING), twin.read(TN.ATROUS)
            want += [pnp.pack(sh, fmt), pwn.warp(sh, crop.h, 37, 25, fmt), pwn.warp(at, half.h, W // 2, H // 2, fmt)]
        elif k == 2:
            tickets += [t.present_warped(TN.SHADING, crop), t.present(TN.ATROUS)]
            want += [pwn.warp(twin.read(TN.SHADING), crop.h, 37, 25, fmt), pnp.pack(twin.read(TN.ATROUS), fmt)]
            # eight are in flight: both kinds are refused, and the frame after the refusals is the twin's
            assert lib.fr_present_enqueue_warped(t._ctx, int(TN.ATROUS), C.byref(half.c_struct()), C.byref(tk)) == STATE
            assert lib.fr_present_enqueue(t._ctx, int(TN.ATROUS), C.byref(tk)) == STATE and tk.value == 99
    assert tickets == list(range(1, 9))
    for b in (TN.SHADING, TN.SIBSON, TN.ATROUS):
        assert equal_nan(t.read(b), twin.read(b)), b
    t.present_release(tickets[1])  # never acquired
    t9 = t.present_warped(TN.ATROUS, half)
    assert t9 == 9
    for i, (ticket, ref) in enumerate(zip(tickets, want)):
        if i == 1:
            continue
        got = t.present_acquire(ticket)
        assert got.shape == ref.shape and np.array_equal(got, ref), (i, mismatch_report(got, ref))
        times = t.present_times(ticket)
        assert isinstance(times["pack_ms"], float) and times["pack_ms"] >= 0 and times["copy_ms"] >= 0
        t.present_release(ticket)
    take(t, t9, pwn.warp(twin.read(TN.ATROUS), half.h, W // 2, H // 2, fmt), "the slot released without an acquire")
    assert_same_state(fovrt_mod, t, twin, "plain and warped presents in one ring")
    t.destroy(); twin.destroy()


def test_around_other_calls(fovrt_mod):
    """Warped presents between stage calls, before and after fr_write_buffer, across fr_snapshot / fr_restore and
    after a timed frame: each sees the image as it stands at its place in the stream order."""
    TN = fovrt_mod.TextureName
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    cams, unis = camera_states(fovrt_mod, 4)
    fmt = pnp.BGRA8 | pnp.TOP_DOWN
    t.present_enable(3, fmt)
    late = [fovrt_mod.PresentWarp.from_poses(cams[k], cams[k + 1], W, H, W, H) for k in range(3)]
    ref = lambda img, wp: pwn.warp(img, wp.h, wp.out_width, wp.out_height, fmt)
    for x in (t, twin):
        x.set_camera_uniforms(unis[0])
        x.frame(timing=False)
    # between stage calls: the present sees the Sibson pass's image, not the write that follows it
    for x in (t, twin):
        fovrt_mod.JumpFlooding(x).render(TN.SHADING)
        fovrt_mod.SibsonInterpolation(x).render()
    first = ref(twin.read(TN.SIBSON), late[0])
    tk = t.present_warped(TN.SIBSON, late[0])
    other = pnp.image(pnp.values(), W, H)
    for x in (t, twin):
        x.write(TN.SIBSON, other)
    assert not np.array_equal(first, ref(other, late[0]))
    take(t, tk, first, "a warped present between a stage call and a write")
    tk = t.present_warped(TN.SIBSON, late[0])
    take(t, tk, ref(other, late[0]), "a warped present after the write")
    # across snapshot / restore: the ticket enqueued before survives both, and the frame after equals the twin's
    for x in (t, twin):
        x.set_camera_uniforms(unis[1])
        x.frame(timing=False)
    want = ref(twin.read(TN.ATROUS), late[1])
    tk = t.present_warped(TN.ATROUS, late[1])
    snaps = [x.snapshot() for x in (t, twin)]
    assert snaps[0] == snaps[1]
    for x, sn in zip((t, twin), snaps):
        x.set_camera_uniforms(unis[2])
        x.frame(timing=False)
        x.restore(sn)
    take(t, tk, want, "a warped present across snapshot and restore")
    for x in (t, twin):
        x.set_camera_uniforms(unis[2])
        x.frame(timing=False)
    tk = t.present_warped(TN.ATROUS, late[2])
    take(t, tk, ref(twin.read(TN.ATROUS), late[2]), "the frame after the restore")
    # after a timed frame (every stage on the context stream, synchronised)
    for x in (t, twin):
        x.set_camera_uniforms(unis[0])
        x.frame(timing=True)
    crop = foveal_crop(fovrt_mod, (unis[0].gaze[0], unis[0].gaze[1]))
    tks = [t.present_warped(TN.ATROUS, late[0]), t.present_warped(TN.SHADING, crop), t.present(TN.SHADING)]
    take(t, tks[0], ref(twin.read(TN.ATROUS), late[0]), "after a timed frame, ATROUS")
    take(t, tks[1], ref(twin.read(TN.SHADING), crop), "after a timed frame, SHADING cropped")
    take(t, tks[2], pnp.pack(twin.read(TN.SHADING), fmt), "after a timed frame, SHADING plain")
    assert_same_state(fovrt_mod, t, twin, "warped presents around other calls")
    t.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(fovrt_mod):
    """Every refusal of the header's list for the two warped calls, each followed by a frame that equals the twin's;
    nothing is written to the destination and no ticket is taken; on a rank of a group both are FR_E_UNSUPPORTED."""
    import torch
    TN = fovrt_mod.TextureName
    lib = fovrt_mod.load_library()
    INV, STATE, UNS = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_STATE, fovrt_mod.FR_E_UNSUPPORTED
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    _cams, unis = camera_states(fovrt_mod, 3)
    dst = torch.full((H * W * 4 + 64,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dp = dst.data_ptr()
    AT = int(TN.ATROUS)
    tk = C.c_uint64(99)
    state = {"k": 0}
    keep = []

    def wp(h=pwn.IDENTITY, ow=0, oh=0):
        keep.append(PW(fovrt_mod, h, ow, oh).c_struct())
        return C.byref(keep[-1])

    def refused(code, what, fn, *args):
        assert fn(t._ctx, *args) == code, what
        assert tk.value == 99, what
        k = state["k"] = (state["k"] + 1) % 3
        for x in (t, twin):
            x.set_camera_uniforms(unis[k])
            x.frame(timing=False)
        for b in (TN.SHADING, TN.SIBSON, TN.ATROUS):
            assert equal_nan(t.read(b), twin.read(b)), (what, b)
        assert (dst.cpu().numpy() == 7).all(), what

    host, dev = lib.fr_present_enqueue_warped, lib.fr_present_enqueue_warped_device
    full = W * H * 4
    # before the feature is on
    refused(STATE, "enqueue, not enabled", host, AT, wp(), C.byref(tk))
    refused(STATE, "device enqueue, not enabled", dev, AT, wp(), C.c_void_p(dp), full)
    t.present_enable(2, pnp.RGBA8)
    refused(INV, "NULL ticket", host, AT, wp(), None)
    refused(INV, "NULL warp", host, AT, None, C.byref(tk))
    refused(INV, "NULL warp, device", dev, AT, None, C.c_void_p(dp), full)
    for k in (0, 8):
        for bad in (np.nan, -np.inf):
            h = np.array(pwn.IDENTITY, np.float32)
            h[k] = bad
            refused(INV, ("coefficient", k, bad), host, AT, wp(h), C.byref(tk))
            refused(INV, ("coefficient, device", k, bad), dev, AT, wp(h), C.c_void_p(dp), full)
    for ow, oh in ((W + 1, H), (W, H + 1), (0, H), (W, 0), (-1, H), (W, -4)):
        refused(INV, ("size", ow, oh), host, AT, wp(ow=ow, oh=oh), C.byref(tk))
        refused(INV, ("size, device", ow, oh), dev, AT, wp(ow=ow, oh=oh), C.c_void_p(dp), max(ow, 1) * max(oh, 1) * 4)
    for b in (TN.POSITION, TN.EXTRA, TN.MASK, 99, -1):
        refused(INV, ("buffer", b), host, int(b), wp(), C.byref(tk))
        refused(INV, ("device buffer", b), dev, int(b), wp(), C.c_void_p(dp), full)
    small = 40 * 30 * 4
    refused(INV, "bytes of the whole screen for a smaller output", dev, AT, wp(ow=40, oh=30), C.c_void_p(dp), full)
    refused(INV, "bytes short", dev, AT, wp(ow=40, oh=30), C.c_void_p(dp), small - 4)
    refused(INV, "bytes long", dev, AT, wp(ow=40, oh=30), C.c_void_p(dp), small + 4)
    refused(INV, "misaligned", dev, AT, wp(ow=40, oh=30), C.c_void_p(dp + 4), small)
    refused(INV, "NULL device_dst", dev, AT, wp(ow=40, oh=30), None, small)
    # the feature still works afterwards, and the tickets start at 1: no refusal took one
    crop = fovrt_mod.PresentWarp.crop(10, 20, 40, 30)
    ticket = t.present_warped(TN.ATROUS, crop)
    assert ticket == 1
    t.present_warped_to(TN.ATROUS, crop, dst[:small])
    want = pwn.warp(twin.read(TN.ATROUS), crop.h, 40, 30, pnp.RGBA8)
    take(t, ticket, want, "after the refusals")
    t.present_done(torch.cuda.current_stream())
    got = dst.cpu().numpy()
    assert np.array_equal(got[:small].reshape(30, 40, 4), want) and (got[small:] == 7).all()  # ow * oh * 4 bytes, no more
    dst.fill_(7)
    torch.cuda.synchronize()
    # a rank of a group
    other = mk(fovrt_mod)
    g = fovrt_mod.Group([t, other], views=1, tile=32)
    assert host(t._ctx, AT, wp(), C.byref(tk)) == UNS and tk.value == 99
    assert dev(t._ctx, AT, wp(), C.c_void_p(dp), full) == UNS
    g.synchronize()
    assert (dst.cpu().numpy() == 7).all()
    g.destroy()
    t.destroy(); twin.destroy(); other.destroy()
