"""GPU suite for the blended present (k_present_blend, k_present_blend_warp: a virtual image that is one buffer around
the gaze, another in the periphery and their smoothstep mix between two radii): the kernels in bytes against the numpy
restatement, blended presents between pipelined frames against a twin context that reads the float images after the
same frame, blended presents sharing the ring with the other kinds and standing around other calls, and the refusals.

Scene 1 (the bunny preset), procedural detail 1, 100 x 70 unless a size is given, 2 spp. No test here synchronises a
presenting context between an enqueue and its acquire: the acquire is the only wait."""
import ctypes as C

import numpy as np
import pytest

import present_blend_np as pbn
import present_np as pnp
import present_warp_np as pwn
from helpers import equal_nan
from test_gpu_bvh import mismatch_report
from test_gpu_present import H, W, assert_same_state, mk, take
from test_gpu_present_warp import camera_states, foveal_crop

pytestmark = pytest.mark.gpu

R_IN, R_OUT = 10.0, 25.0


def PB(fovrt, gaze, r_in, r_out, inner=None, outer=None):
    TN = fovrt.TextureName
    return fovrt.PresentBlend(gaze, r_in, r_out, TN.SIBSON if inner is None else inner, TN.ATROUS if outer is None else outer)


def ref_of(inner, outer, bl, wp, fmt):
    """The restatement's bytes of a blended present of two float images, plain (wp None) or through a PresentWarp."""
    if wp is None:
        return pbn.pack(inner, outer, bl.gaze, bl.inner_radius_px, bl.outer_radius_px, fmt)
    return pbn.warp(inner, outer, bl.gaze, bl.inner_radius_px, bl.outer_radius_px, wp.h, wp.out_width, wp.out_height, fmt)


# ---------------------------------------------------------------------------------------------
# 1. The kernels are the rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", pwn.SCREENS)
def test_kernel_is_the_rule(fovrt_mod, w, h):
    """Four different images over the present suite's value set in the four presentable buffers (ATROUS after one
    A-Trous pass, so that the image the view names is the pass's output). Every format and every blend case of the CPU
    suite, over buffer pairs that rotate (one with SHADING, one whose two ids are equal), plain and through the
    identity, an odd crop and a 2 degree turn, to the host ring and into a torch tensor: the bytes are the
    restatement's. At 100 x 70 also the two cases whose weight rounds to 0 and to 1 inside the ramp, with the source of
    weight zero filled with NaN."""
    import torch
    TN = fovrt_mod.TextureName
    t = mk(fovrt_mod, w, h)
    fovrt_mod.ATrous(t).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    bufs = (TN.SIBSON, TN.PULLPUSH, TN.SHADING, TN.ATROUS)
    a, b = pbn.sources(w, h, 0)
    c, d = pbn.sources(w, h, 1) if w * h * 3 < len(pnp.values()) else (a[::-1, ::-1].copy(), b[::-1, ::-1].copy())
    img = dict(zip(bufs, (a, b, c, d)))
    for buf in bufs:
        t.write(buf, img[buf])
    pairs = [(TN.SIBSON, TN.ATROUS), (TN.SHADING, TN.ATROUS), (TN.PULLPUSH, TN.PULLPUSH), (TN.ATROUS, TN.SIBSON),
             (TN.PULLPUSH, TN.SHADING)]
    named = {n: fovrt_mod.PresentWarp(hm, ow, oh) for n, hm, ow, oh in pwn.cases(fovrt_mod, w, h)}
    warps = [None, named["identity"], named["odd crop"], named["turn 2.0 about 1"]]
    dst = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()

    def both(bl, wp, ref, what):
        n = ref.size
        ticket = t.present_blended(bl, wp)
        t.present_blended_to(bl, dst[:n], wp)
        take(t, ticket, ref, what + ("host",))
        t.present_done(s)
        got = dst[:n].cpu().numpy().reshape(ref.shape)  # (on torch's current stream, behind the kernel)
        assert np.array_equal(got, ref), what + ("device", mismatch_report(got, ref))
        assert (got[..., 3] == 255).all()

    cases = pbn.cases(w, h)
    for i, fmt in enumerate(pnp.FORMATS):
        t.present_enable(3, fmt)
        for j, (name, gaze, r_in, r_out, _ramp) in enumerate(cases):
            inner, outer = pairs[(i + j) % len(pairs)]
            bl = PB(fovrt_mod, gaze, r_in, r_out, inner, outer)
            for k, wp in enumerate(warps):
                both(bl, wp, ref_of(img[inner], img[outer], bl, wp, fmt), (w, h, fmt, name, inner, outer, k))
    if (w, h) == (100, 70):
        good = pnp.image(pnp.values()[10:], w, h)
        for i, (name, gaze, r_in, r_out, value, texel) in enumerate(pbn.POISON):
            m = pbn.poison_texels(w, h, gaze, r_in, r_out, value)
            assert m.any() and m[texel[1], texel[0]], name
            bad = good.copy()
            bad[m] = np.nan
            inner, outer = (good, bad) if value == 0.0 else (bad, good)
            t.write(TN.SIBSON, inner)
            t.write(TN.ATROUS, outer)
            bl = PB(fovrt_mod, gaze, r_in, r_out)
            for fmt in pnp.FORMATS[2 * i:2 * i + 2]:
                t.present_enable(3, fmt)
                ref = ref_of(inner, outer, bl, None, fmt)
                mm = m[::-1] if fmt & pnp.TOP_DOWN else m
                assert np.array_equal(ref[mm], pnp.pack(good, fmt)[mm])
                for k, wp in enumerate(warps[:2]):
                    both(bl, wp, ref, (w, h, fmt, name, k))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Pipelined frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latency,iters,overlap", [(False, 1, False), (True, 1, False), (False, 2, False),
                                                   (True, 2, False), (False, 1, True)])
def test_pipelined_frames(fovrt_mod, latency, iters, overlap):
    """Eight untimed frames with the camera and the gaze moved before each and a blended present after every frame:
    SIBSON inside and ATROUS outside that frame's gaze (radii 10 and 25) on one context, SHADING inside and ATROUS
    outside through a foveal crop on another; three slots, ticket k - 2 taken after ticket k is enqueued, no
    synchronize. Every image is the restatement over what a twin reads after the same frame, and after the eighth frame
    both presenting contexts are the twin, bit for bit. overlap: overlapped geometry updates with a pose enqueued
    before each frame."""
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
    _cams, unis = camera_states(fovrt_mod, N)
    want_a, want_s, tick_a, tick_s = [], [], [], []
    for k in range(N):
        for t in everyone:
            t.set_camera_uniforms(unis[k])
            if overlap:
                t.set_model_transforms(pose("turning", pos0, models, k), enqueue=True)
        gaze = (unis[k].gaze[0], unis[k].gaze[1])
        assert gaze == (18 + 9 * k, 12 + 6 * k)
        zi, zr, zo = (int(z.sum()) for z in pbn.zones(W, H, gaze, R_IN, R_OUT))
        assert zi == 317 and zr >= 1109 and zo >= 5059, (k, zi, zr, zo)
        bl_a = PB(fovrt_mod, gaze, R_IN, R_OUT)
        bl_s = PB(fovrt_mod, gaze, R_IN, R_OUT, TN.SHADING, TN.ATROUS)
        dflt = a.present_blend_default()  # the gaze the next launch uses is this frame's
        assert tuple(dflt.gaze) == gaze and (dflt.inner_buffer, dflt.outer_buffer) == (TN.SIBSON, TN.ATROUS)
        crop = foveal_crop(fovrt_mod, gaze)
        a.frame(timing=False)
        tick_a.append(a.present_blended(bl_a))
        s.frame(timing=False)
        tick_s.append(s.present_blended(bl_s, crop))
        twin.frame(timing=False)
        sib, shd, atr = twin.read(TN.SIBSON), twin.read(TN.SHADING), twin.read(TN.ATROUS)
        want_a.append(ref_of(sib, atr, bl_a, None, fmt_a))
        want_s.append(ref_of(shd, atr, bl_s, crop, fmt_s))
        # the image is neither source's plain pack: a present of one buffer alone would not pass
        assert not np.array_equal(want_a[k], pnp.pack(sib, fmt_a)) and not np.array_equal(want_a[k], pnp.pack(atr, fmt_a)), k
        if k:  # consecutive images differ in bytes, or a present of the wrong frame would pass
            assert not np.array_equal(want_a[k], want_a[k - 1]), k
            assert not np.array_equal(want_s[k], want_s[k - 1]), k
        assert tick_a[k] == k + 1 and tick_s[k] == k + 1
        if k >= 2:
            take(a, tick_a[k - 2], want_a[k - 2], ("sibson / atrous", latency, iters, overlap, k - 2))
            take(s, tick_s[k - 2], want_s[k - 2], ("shading / atrous, cropped", latency, iters, overlap, k - 2))
    for k in (N - 2, N - 1):
        take(a, tick_a[k], want_a[k], ("sibson / atrous", latency, iters, overlap, k))
        take(s, tick_s[k], want_s[k], ("shading / atrous, cropped", latency, iters, overlap, k))
    assert_same_state(fovrt_mod, a, twin, "the context that presents SIBSON / ATROUS blended")
    assert_same_state(fovrt_mod, s, twin, "the context that presents SHADING / ATROUS blended through a crop")
    for t in everyone:
        t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Sharing the ring, and blended presents around other calls
# ---------------------------------------------------------------------------------------------
def test_all_kinds_share_the_ring(fovrt_mod):
    """After each of three frames: ATROUS plain, SIBSON cropped, SIBSON / ATROUS blended, SHADING / ATROUS blended at
    half size (eight slots; nothing is taken before the ring is full, so the SHADING of frame k is read while later
    frames run). Tickets count across the kinds; times come back for a blended ticket; a full ring refuses a blended
    present and enqueues nothing."""
    TN = fovrt_mod.TextureName
    lib = fovrt_mod.load_library()
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    fmt = pnp.RGBA8
    t.present_enable(8, fmt)
    _cams, unis = camera_states(fovrt_mod, 3)
    crop = fovrt_mod.PresentWarp.crop(40, 30, 37, 25)
    half = fovrt_mod.PresentWarp.scale(W, H, W // 2, H // 2)
    tickets, want = [], []
    tk = C.c_uint64(99)
    for k in range(3):
        for x in (t, twin):
            x.set_camera_uniforms(unis[k])
            x.frame(timing=False)
        gaze = (unis[k].gaze[0], unis[k].gaze[1])
        bl = PB(fovrt_mod, gaze, R_IN, R_OUT)
        bs = PB(fovrt_mod, gaze, R_IN, R_OUT, TN.SHADING, TN.ATROUS)
        sib, shd, atr = twin.read(TN.SIBSON), twin.read(TN.SHADING), twin.read(TN.ATROUS)
        if k < 2:
            tickets += [t.present(TN.ATROUS), t.present_warped(TN.SIBSON, crop), t.present_blended(bl), t.present_blended(bs, half)]
            want += [pnp.pack(atr, fmt), pwn.warp(sib, crop.h, 37, 25, fmt), ref_of(sib, atr, bl, None, fmt),
                     ref_of(shd, atr, bs, half, fmt)]
        else:  # eight are in flight
            assert lib.fr_present_enqueue_blended(t._ctx, C.byref(bl.c_struct()), None, C.byref(tk)) == fovrt_mod.FR_E_STATE
            assert lib.fr_present_enqueue_blended(t._ctx, C.byref(bs.c_struct()), C.byref(half.c_struct()),
                                                  C.byref(tk)) == fovrt_mod.FR_E_STATE and tk.value == 99
    assert tickets == list(range(1, 9))
    for b in (TN.SHADING, TN.SIBSON, TN.ATROUS):
        assert equal_nan(t.read(b), twin.read(b)), b
    for i, (ticket, ref) in enumerate(zip(tickets, want)):
        got = t.present_acquire(ticket)
        assert got.shape == ref.shape and np.array_equal(got, ref), (i, mismatch_report(got, ref))
        times = t.present_times(ticket)
        assert isinstance(times["pack_ms"], float) and times["pack_ms"] >= 0 and times["copy_ms"] >= 0
        t.present_release(ticket)
    assert_same_state(fovrt_mod, t, twin, "plain, warped and blended presents in one ring")
    t.destroy(); twin.destroy()


def test_around_other_calls(fovrt_mod):
    """Blended presents between stage calls and fr_write_buffer, across fr_snapshot / fr_restore and after a timed
    frame: each sees both images as they stand at its place in the stream order. fr_present_blend_default follows
    fr_set_gaze and fr_set_foveation."""
    TN = fovrt_mod.TextureName
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    _cams, unis = camera_states(fovrt_mod, 3)
    fmt = pnp.BGRA8 | pnp.TOP_DOWN
    t.present_enable(3, fmt)
    gz = lambda k: (unis[k].gaze[0], unis[k].gaze[1])
    for x in (t, twin):
        x.set_camera_uniforms(unis[1])
        x.frame(timing=False)
    # between stage calls: the present sees the Sibson pass's image, not the write that follows it
    for x in (t, twin):
        fovrt_mod.JumpFlooding(x).render(TN.SHADING)
        fovrt_mod.SibsonInterpolation(x).render()
    bl = PB(fovrt_mod, gz(1), R_IN, R_OUT)
    atr = twin.read(TN.ATROUS)
    first = ref_of(twin.read(TN.SIBSON), atr, bl, None, fmt)
    tk = t.present_blended(bl)
    other = pnp.image(pnp.values(), W, H)
    for x in (t, twin):
        x.write(TN.SIBSON, other)
    second = ref_of(other, atr, bl, None, fmt)
    assert not np.array_equal(first, second)
    take(t, tk, first, "a blended present between a stage call and a write")
    tk = t.present_blended(bl)
    take(t, tk, second, "a blended present after the write")
    # across snapshot / restore: the ticket enqueued before survives both, and the frame after equals the twin's
    for x in (t, twin):
        x.set_camera_uniforms(unis[2])
        x.frame(timing=False)
    bl = PB(fovrt_mod, gz(2), R_IN, R_OUT, TN.SHADING, TN.ATROUS)
    crop = foveal_crop(fovrt_mod, gz(2))
    want = ref_of(twin.read(TN.SHADING), twin.read(TN.ATROUS), bl, crop, fmt)
    tk = t.present_blended(bl, crop)
    snaps = [x.snapshot() for x in (t, twin)]
    assert snaps[0] == snaps[1]
    for x, sn in zip((t, twin), snaps):
        x.set_camera_uniforms(unis[0])
        x.frame(timing=False)
        x.restore(sn)
    take(t, tk, want, "a blended present across snapshot and restore")
    for x in (t, twin):
        x.set_camera_uniforms(unis[0])
        x.frame(timing=False)
    bl = PB(fovrt_mod, gz(0), R_IN, R_OUT)
    tk = t.present_blended(bl)
    take(t, tk, ref_of(twin.read(TN.SIBSON), twin.read(TN.ATROUS), bl, None, fmt), "the frame after the restore")
    # after a timed frame (every stage on the context stream, synchronised)
    for x in (t, twin):
        x.set_camera_uniforms(unis[1])
        x.frame(timing=True)
    bl, bs = PB(fovrt_mod, gz(1), R_IN, R_OUT), PB(fovrt_mod, gz(1), R_IN, R_OUT, TN.SHADING, TN.PULLPUSH)
    tks = [t.present_blended(bl), t.present_blended(bs, crop), t.present(TN.SHADING)]
    rd = {b: twin.read(b) for b in (TN.SIBSON, TN.ATROUS, TN.SHADING, TN.PULLPUSH)}
    take(t, tks[0], ref_of(rd[TN.SIBSON], rd[TN.ATROUS], bl, None, fmt), "after a timed frame, SIBSON / ATROUS")
    take(t, tks[1], ref_of(rd[TN.SHADING], rd[TN.PULLPUSH], bs, crop, fmt), "after a timed frame, SHADING / PULLPUSH cropped")
    take(t, tks[2], pnp.pack(rd[TN.SHADING], fmt), "after a timed frame, SHADING plain")
    # the default blend follows the gaze and the foveation radius, without a frame between
    for x in (t, twin):
        x.set_gaze(31.0, 20.0, fullscreen=True)
        x.set_foveation(radius_px=7.25)
    d = t.present_blend_default()
    assert tuple(d.gaze) == (31.0, float(H - 20)) and d.inner_radius_px == np.float32(7.25) and d.outer_radius_px == np.float32(14.5)
    assert (d.inner_buffer, d.outer_buffer) == (TN.SIBSON, TN.ATROUS)
    assert t.foveation()["radius_px"] == 7.25
    for x in (t, twin):
        x.frame(timing=False)
    tk = t.present_blended(d)
    take(t, tk, ref_of(twin.read(TN.SIBSON), twin.read(TN.ATROUS), d, None, fmt), "the default blend after set_gaze")
    assert_same_state(fovrt_mod, t, twin, "blended presents around other calls")
    t.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(fovrt_mod):
    """Every refusal of the header's list for the two blended calls, each followed by a frame that equals the twin's;
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
    tk = C.c_uint64(99)
    state = {"k": 0}
    keep = []

    def bl(gaze=(30.0, 20.0), r_in=R_IN, r_out=R_OUT, inner=TN.SIBSON, outer=TN.ATROUS):
        keep.append(fovrt_mod.PresentBlend(gaze, r_in, r_out, inner, outer).c_struct())
        return C.byref(keep[-1])

    def wp(h=pwn.IDENTITY, ow=0, oh=0):
        keep.append(fovrt_mod.PresentWarp(h, ow, oh).c_struct())
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

    host, dev = lib.fr_present_enqueue_blended, lib.fr_present_enqueue_blended_device
    full = W * H * 4
    D = C.c_void_p(dp)

    def pair(code, what, blend, warp=None, bytes_=full):
        refused(code, (what, "host"), host, blend, warp, C.byref(tk))
        refused(code, (what, "device"), dev, blend, warp, D, bytes_)

    pair(STATE, "not enabled", bl())
    t.present_enable(2, pnp.RGBA8)
    refused(INV, "NULL ticket", host, bl(), None, None)
    pair(INV, "NULL blend", None)
    for b in (TN.POSITION, TN.EXTRA, TN.MASK, 99, -1):
        pair(INV, ("inner buffer", b), bl(inner=int(b)))
        pair(INV, ("outer buffer", b), bl(outer=int(b)))
    for bad in (np.nan, np.inf, -np.inf):
        pair(INV, ("gaze x", bad), bl(gaze=(bad, 20.0)))
        pair(INV, ("gaze y", bad), bl(gaze=(30.0, bad)))
        pair(INV, ("inner radius", bad), bl(r_in=bad, r_out=np.inf))
        pair(INV, ("outer radius", bad), bl(r_out=bad))
    pair(INV, "inner > outer", bl(r_in=26.0))
    pair(INV, "a negative radius", bl(r_in=-1.0))
    pair(INV, "two negative radii", bl(r_in=-2.0, r_out=-1.0))
    pair(INV, "outer * outer not finite", bl(r_out=2e19))
    # the warp's refusals, when one is given
    h = np.array(pwn.IDENTITY, np.float32)
    h[8] = np.nan
    pair(INV, "a non-finite coefficient", bl(), wp(h))
    for ow, oh in ((W + 1, H), (0, H), (W, -4)):
        pair(INV, ("size", ow, oh), bl(), wp(ow=ow, oh=oh), max(ow, 1) * max(oh, 1) * 4)
    small = 40 * 30 * 4
    refused(INV, "bytes of the whole screen for a smaller output", dev, bl(), wp(ow=40, oh=30), D, full)
    refused(INV, "bytes short", dev, bl(), None, D, full - 4)
    refused(INV, "bytes long", dev, bl(), None, D, full + 4)
    refused(INV, "misaligned", dev, bl(), wp(ow=40, oh=30), C.c_void_p(dp + 4), small)
    refused(INV, "NULL device_dst", dev, bl(), None, None, full)
    # the feature still works afterwards, and the tickets start at 1: no refusal took one
    crop = fovrt_mod.PresentWarp.crop(10, 20, 40, 30)
    blend = fovrt_mod.PresentBlend((30.0, 20.0), R_IN, R_OUT)
    ticket = t.present_blended(blend, crop)
    assert ticket == 1
    t.present_blended_to(blend, dst[:small], crop)
    want = ref_of(twin.read(TN.SIBSON), twin.read(TN.ATROUS), blend, crop, pnp.RGBA8)
    take(t, ticket, want, "after the refusals")
    t.present_done(torch.cuda.current_stream())
    got = dst.cpu().numpy()
    assert np.array_equal(got[:small].reshape(30, 40, 4), want) and (got[small:] == 7).all()  # ow * oh * 4 bytes, no more
    dst.fill_(7)
    torch.cuda.synchronize()
    # a full ring
    t1, t2 = t.present_blended(blend), t.present_blended(blend)
    refused(STATE, "every slot is held", host, bl(), None, C.byref(tk))
    t.present_release(t1); t.present_release(t2)
    # a rank of a group
    other = mk(fovrt_mod)
    g = fovrt_mod.Group([t, other], views=1, tile=32)
    assert host(t._ctx, bl(), None, C.byref(tk)) == UNS and tk.value == 99
    assert dev(t._ctx, bl(), None, D, full) == UNS
    g.synchronize()
    assert (dst.cpu().numpy() == 7).all()
    g.destroy()
    t.destroy(); twin.destroy(); other.destroy()
