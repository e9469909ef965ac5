"""GPU suite for present (8-bit frames delivered in stream order): the pack kernel (k_present_pack) in bytes against the
numpy restatement, presents between pipelined frames against a twin context that reads the float image after the same
frame, the ring's semantics, presents around other calls, the refusals, and the order in which every enqueue refuses.

Scene 1 (the bunny preset), procedural detail 1, 100 x 70 unless a size is given, 2 spp. No test here synchronises a
presenting context between an enqueue and its acquire: the acquire is the only wait."""
import ctypes as C

import numpy as np
import pytest

import present_np as pnp
from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan
from test_gpu_bvh import mismatch_report

pytestmark = pytest.mark.gpu

W, H = 100, 70
SPP = 2
# W x H: a row shorter than a lane's span, the 4-texel tail, and (rows of more than 64 lanes) a second block along x
# with 16-byte rows and with a tail
SCREENS = [(1, 1), (3, 1), (65, 3), (67, 5), (100, 70), (260, 2), (261, 3)]


def mk(fovrt, w=W, h=H, latency=False, **kw):
    t = fovrt.PathTracer(fovrt.Config(width=w, height=h, scene=1, mask_mode=4, spp=SPP, diffuse_max_depth=1,
                                      texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, detail=1, **kw))
    assert t.initialize()
    if latency:
        t.set_pipeline_mode(fovrt.PIPELINE_LATENCY)
    return t


def cameras(fovrt, n, w=W, h=H):
    """n camera / gaze states, each moved against the one before (and reprojecting from it): consecutive frames differ."""
    out, prev = [], None
    for k in range(n):
        cam = fovrt.Camera.preset(1, w, h)
        tgt = cam.target.copy()
        cam.setPosition(cam.pos + np.array([0.05 * k, 0.02 * k, -0.04 * k], np.float32))
        cam.lookAt(tgt)
        cam.prev = prev
        prev = (cam.pos.copy(), cam.rot.copy(), cam.fovy, cam.znear, cam.zfar, cam.aspect)
        u = cam.uniforms(w, h)
        u.gaze[0], u.gaze[1] = float(18 + 9 * k), float(12 + 6 * k)
        out.append(u)
    return out


def all_buffers(fovrt):
    TN = fovrt.TextureName
    return (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.WEIGHT, TN.HISTORY, TN.SHADING, TN.EXTRA, TN.JFA_COORD,
            TN.JFA_COLOR, TN.SIBSON, TN.PULLPUSH, TN.ATROUS, TN.DEPTH_CACHE, TN.HISTORY_CACHE, TN.MASK, TN.GCLASS)


def assert_same_state(fovrt, a, b, what):
    """Every output buffer, the count, the active list, the stats, the JumpFlooding reuse count and the snapshot."""
    TN = fovrt.TextureName
    for tid in all_buffers(fovrt):
        x, y = a.read(tid), b.read(tid)
        assert equal_nan(x, y), (what, tid, mismatch_report(x, y))
    n = a.ray_count()
    assert n == b.ray_count(), (what, "count")
    assert np.array_equal(a.read(TN.THREAD)[:n], b.read(TN.THREAD)[:n]), (what, "active list")
    assert a.stats() == b.stats(), (what, "stats")
    assert a.jfa_reuse_count() == b.jfa_reuse_count(), (what, "jfa reuse")
    assert a.snapshot() == b.snapshot(), (what, "snapshot")


def take(t, ticket, ref, what, wait=True):
    """Acquires, compares with the expected bytes, releases."""
    got = t.present_acquire(ticket, wait=wait)
    assert got is not None, (what, "pending after a blocking acquire")
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert np.array_equal(got, ref), (what, ticket, mismatch_report(got, ref))
    t.present_release(ticket)


# ---------------------------------------------------------------------------------------------
# 3. The kernel is the rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SCREENS)
def test_kernel_is_the_rule(fovrt_mod, w, h):
    """The CPU suite's value set (edge values first; 100 x 70 holds all of it) written into each presentable buffer,
    presented to the host and into a torch tensor: the bytes are present_np's in both formats and both row orders.
    ATROUS is written after one A-Trous pass, so that the image the view names is the pass's output."""
    import torch
    TN = fovrt_mod.TextureName
    t = mk(fovrt_mod, w, h)
    vals = pnp.values()
    fovrt_mod.ATrous(t).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)
    dst = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for i, fmt in enumerate(pnp.FORMATS):
        t.present_enable(2, fmt)
        for j, buf in enumerate((TN.SIBSON, TN.PULLPUSH, TN.SHADING, TN.ATROUS)):
            img = pnp.image(vals, w, h, start=(0 if w * h >= 7000 else 257 * (4 * i + j)))
            ref = pnp.pack(img, fmt)
            t.write(buf, img)
            ticket = t.present(buf)
            t.present_to(buf, dst)
            take(t, ticket, ref, (w, h, fmt, buf, "host"))
            s = torch.cuda.current_stream()
            t.present_done(s)
            got = dst.cpu().numpy().reshape(h, w, 4)  # (on torch's current stream, behind the pack)
            assert np.array_equal(got, ref), (w, h, fmt, buf, "device", mismatch_report(got, ref))
            assert (got[..., 3] == 255).all()
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Pipelined frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latency,iters,overlap", [(False, 1, False), (True, 1, False), (False, 2, False),
                                                   (True, 2, False), (False, 1, True), (True, 2, True)])
def test_pipelined_frames(fovrt_mod, latency, iters, overlap):
    """Eight untimed frames with the camera and the gaze moved before each, a present after every frame (ATROUS on one
    context, SIBSON on another, three slots), ticket k - 2 taken after ticket k is enqueued, no synchronize: every
    image is present_np of what a twin reads after the same frame, and after the eighth frame both presenting
    contexts are the twin, bit for bit. overlap: overlapped geometry updates with a pose enqueued before each frame."""
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
    cams = cameras(fovrt_mod, N)
    want_a, want_s, tick_a, tick_s = [], [], [], []
    for k in range(N):
        for t in everyone:
            t.set_camera_uniforms(cams[k])
            if overlap:
                t.set_model_transforms(pose("turning", pos0, models, k), enqueue=True)
        a.frame(timing=False)
        tick_a.append(a.present(TN.ATROUS))
        s.frame(timing=False)
        tick_s.append(s.present(TN.SIBSON))
        twin.frame(timing=False)
        at, sib = twin.read(TN.ATROUS), twin.read(TN.SIBSON)
        want_a.append(pnp.pack(at, fmt_a))
        want_s.append(pnp.pack(sib, fmt_s))
        if k:  # consecutive frames differ in bytes, or a present of the wrong frame would pass
            assert not np.array_equal(want_a[k], want_a[k - 1]) and not np.array_equal(want_s[k], want_s[k - 1]), k
        assert tick_a[k] == k + 1 and tick_s[k] == k + 1
        if k >= 2:
            take(a, tick_a[k - 2], want_a[k - 2], ("atrous", latency, iters, overlap, k - 2))
            take(s, tick_s[k - 2], want_s[k - 2], ("sibson", latency, iters, overlap, k - 2))
    for k in (N - 2, N - 1):
        take(a, tick_a[k], want_a[k], ("atrous", latency, iters, overlap, k))
        take(s, tick_s[k], want_s[k], ("sibson", latency, iters, overlap, k))
    assert_same_state(fovrt_mod, a, twin, "the context that presents ATROUS")
    assert_same_state(fovrt_mod, s, twin, "the context that presents SIBSON")
    for t in everyone:
        t.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Both outputs of one frame, and SHADING through the slot rotation
# ---------------------------------------------------------------------------------------------
def test_both_outputs_and_shading_of_one_frame(fovrt_mod):
    """SIBSON, ATROUS and SHADING presented after each of four frames (eight slots, nothing taken before the last
    frame is enqueued, so the SHADING of frame k is read while frames k + 1 .. rotate through the other slots and
    frame k + 3 waits to overwrite it), all against the twin."""
    TN = fovrt_mod.TextureName
    bufs = (TN.SIBSON, TN.ATROUS, TN.SHADING)
    for n_frames, sets in ((2, (bufs,)), (4, ((TN.SHADING,), (TN.SIBSON, TN.ATROUS)))):
        for which in sets:
            t, twin = mk(fovrt_mod), mk(fovrt_mod)
            t.present_enable(8, pnp.RGBA8)
            cams = cameras(fovrt_mod, n_frames)
            tickets, want = [], []
            for k in range(n_frames):
                for x in (t, twin):
                    x.set_camera_uniforms(cams[k])
                    x.frame(timing=False)
                for b in which:
                    tickets.append(t.present(b))
                    want.append(pnp.pack(twin.read(b), pnp.RGBA8))
            for i, (tk, ref) in enumerate(zip(tickets, want)):
                take(t, tk, ref, ("frame", i // len(which), which[i % len(which)]))
            assert_same_state(fovrt_mod, t, twin, which)
            t.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 6. Ring semantics
# ---------------------------------------------------------------------------------------------
def test_ring_semantics(fovrt_mod):
    TN = fovrt_mod.TextureName
    lib = fovrt_mod.load_library()
    STATE, INV = fovrt_mod.FR_E_STATE, fovrt_mod.FR_E_INVALID
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    cams = cameras(fovrt_mod, 4)
    fmt = pnp.RGBA8

    def frame(k):
        for x in (t, twin):
            x.set_camera_uniforms(cams[k])
            x.frame(timing=False)
        return pnp.pack(twin.read(TN.ATROUS), fmt)

    t.present_enable(2, fmt)
    want = {}
    want[1] = frame(0); t1 = t.present(TN.ATROUS)
    want[2] = frame(1); t2 = t.present(TN.ATROUS)
    want[3] = frame(2)
    tk = C.c_uint64(99)
    assert lib.fr_present_enqueue(t._ctx, int(TN.ATROUS), C.byref(tk)) == STATE and tk.value == 99  # full
    want4 = frame(3)  # the frame after the refusal is the twin's
    assert equal_nan(t.read(TN.SHADING), twin.read(TN.SHADING))
    # re-enabling with a held ticket: refused, the ring stays
    assert lib.fr_present_enable(t._ctx, 3, fmt) == STATE
    assert lib.fr_present_enable(t._ctx, 0, fmt) == STATE
    # release without acquire, out of order (the second first), then the third enqueue succeeds
    t.present_release(t2)
    assert lib.fr_present_release(t._ctx, t2) == INV  # already released
    p = C.c_void_p(5)
    assert lib.fr_present_acquire(t._ctx, t2, 1, C.byref(p)) == INV and p.value == 5
    assert lib.fr_present_acquire(t._ctx, 12345, 1, C.byref(p)) == INV
    t3 = t.present(TN.ATROUS)
    assert (t1, t2, t3) == (1, 2, 3)
    # wait = 0: pending or there; after FR_OK the bytes are right
    got = None
    for _ in range(200000):
        got = t.present_acquire(t3, wait=False)
        if got is not None:
            break
    assert got is not None, "the third present never landed"
    assert np.array_equal(got, want4), mismatch_report(got, want4)
    again = t.present_acquire(t3)  # a second acquire of a held ticket gives the same image
    assert again.ctypes.data == got.ctypes.data
    assert isinstance(t.present_times(t3)["pack_ms"], float)
    take(t, t1, want[1], "the first ticket, acquired last")
    t.present_release(t3)
    # with every ticket released the ring may be remade; tickets keep counting
    t.present_enable(3, pnp.BGRA8)
    t4 = t.present(TN.ATROUS)
    assert t4 == 4
    take(t, t4, pnp.pack(twin.read(TN.ATROUS), pnp.BGRA8), "after the ring was remade")
    # off: the other calls answer FR_E_STATE
    t.present_enable(0)
    assert lib.fr_present_enqueue(t._ctx, int(TN.ATROUS), C.byref(tk)) == STATE and tk.value == 99
    assert lib.fr_present_acquire(t._ctx, t4, 1, C.byref(p)) == STATE
    assert lib.fr_present_release(t._ctx, t4) == STATE
    assert lib.fr_present_done(t._ctx, None) == STATE
    assert_same_state(fovrt_mod, t, twin, "ring semantics")
    t.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 7. Around other calls
# ---------------------------------------------------------------------------------------------
def test_around_other_calls(fovrt_mod):
    TN = fovrt_mod.TextureName
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    cams = cameras(fovrt_mod, 3)
    fmt = pnp.BGRA8 | pnp.TOP_DOWN
    t.present_enable(3, fmt)
    for x in (t, twin):
        x.set_camera_uniforms(cams[0])
        x.frame(timing=False)
    # between stage calls: the present sees the Sibson pass's image, not the write that follows it
    for x in (t, twin):
        fovrt_mod.JumpFlooding(x).render(TN.SHADING)
        fovrt_mod.SibsonInterpolation(x).render()
    first = pnp.pack(twin.read(TN.SIBSON), fmt)
    tk = t.present(TN.SIBSON)
    other = pnp.image(pnp.values(), W, H)
    for x in (t, twin):
        x.write(TN.SIBSON, other)
    assert not np.array_equal(first, pnp.pack(other, fmt))
    take(t, tk, first, "a present between a stage call and a write")
    tk = t.present(TN.SIBSON)
    take(t, tk, pnp.pack(other, fmt), "a present after the write")
    # across snapshot / restore: the ticket enqueued before survives both, and the frame after equals the twin's
    for x in (t, twin):
        x.set_camera_uniforms(cams[1])
        x.frame(timing=False)
    want = pnp.pack(twin.read(TN.ATROUS), fmt)
    tk = t.present(TN.ATROUS)
    snaps = [x.snapshot() for x in (t, twin)]
    assert snaps[0] == snaps[1]
    for x, sn in zip((t, twin), snaps):
        x.set_camera_uniforms(cams[2])
        x.frame(timing=False)
        x.restore(sn)
    take(t, tk, want, "a present across snapshot and restore")
    for x in (t, twin):
        x.set_camera_uniforms(cams[2])
        x.frame(timing=False)
    tk = t.present(TN.ATROUS)
    take(t, tk, pnp.pack(twin.read(TN.ATROUS), fmt), "the frame after the restore")
    # after a timed frame (every stage on the context stream, synchronised)
    for x in (t, twin):
        x.set_camera_uniforms(cams[0])
        x.frame(timing=True)
    tks = [t.present(b) for b in (TN.ATROUS, TN.SHADING)]
    for tk, b in zip(tks, (TN.ATROUS, TN.SHADING)):
        take(t, tk, pnp.pack(twin.read(b), fmt), ("after a timed frame", b))
    assert_same_state(fovrt_mod, t, twin, "around other calls")
    t.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 8. Refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(fovrt_mod):
    """Every refusal of the header's list, each followed by a frame that equals the twin's; the enqueued forms on a
    rank of a two-context group are FR_E_UNSUPPORTED."""
    import torch
    TN = fovrt_mod.TextureName
    lib = fovrt_mod.load_library()
    INV, STATE, UNS = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_STATE, fovrt_mod.FR_E_UNSUPPORTED
    t, twin = mk(fovrt_mod), mk(fovrt_mod)
    cams = cameras(fovrt_mod, 3)
    dst = torch.full((H * W * 4 + 64,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dp, nbytes = dst.data_ptr(), W * H * 4
    AT = int(TN.ATROUS)
    tk, p = C.c_uint64(99), C.c_void_p(5)
    state = {"k": 0}

    def refused(code, what, fn, *args):
        assert fn(t._ctx, *args) == code, what
        assert tk.value == 99 and p.value == 5, what
        k = state["k"] = (state["k"] + 1) % 3
        for x in (t, twin):
            x.set_camera_uniforms(cams[k])
            x.frame(timing=False)
        for b in (TN.SHADING, TN.SIBSON, TN.ATROUS):
            assert equal_nan(t.read(b), twin.read(b)), (what, b)
        assert (dst.cpu().numpy() == 7).all(), what

    # before the feature is on
    refused(STATE, "enqueue, not enabled", lib.fr_present_enqueue, AT, C.byref(tk))
    refused(STATE, "device enqueue, not enabled", lib.fr_present_enqueue_device, AT, C.c_void_p(dp), nbytes)
    refused(STATE, "acquire, not enabled", lib.fr_present_acquire, 1, 1, C.byref(p))
    for slots, fmt in ((-1, 0), (9, 0), (2, 2), (2, 0x200), (2, -1)):
        refused(INV, ("enable", slots, fmt), lib.fr_present_enable, slots, fmt)
    refused(STATE, "still not enabled", lib.fr_present_enqueue, AT, C.byref(tk))
    t.present_enable(2, pnp.RGBA8)
    refused(INV, "NULL ticket", lib.fr_present_enqueue, AT, None)
    refused(INV, "NULL host pointer", lib.fr_present_acquire, 1, 1, None)
    for b in (TN.POSITION, TN.EXTRA, TN.JFA_COLOR, TN.MASK, TN.HISTORY, 99, -1):
        refused(INV, ("buffer", b), lib.fr_present_enqueue, int(b), C.byref(tk))
        refused(INV, ("device buffer", b), lib.fr_present_enqueue_device, int(b), C.c_void_p(dp), nbytes)
    refused(INV, "bytes short", lib.fr_present_enqueue_device, AT, C.c_void_p(dp), nbytes - 4)
    refused(INV, "bytes long", lib.fr_present_enqueue_device, AT, C.c_void_p(dp), nbytes + 4)
    refused(INV, "misaligned", lib.fr_present_enqueue_device, AT, C.c_void_p(dp + 4), nbytes)
    refused(INV, "NULL device_dst", lib.fr_present_enqueue_device, AT, None, nbytes)
    # the feature still works afterwards, and the tickets start at 1: no refusal took one
    ticket = t.present(TN.ATROUS)
    assert ticket == 1
    take(t, ticket, pnp.pack(twin.read(TN.ATROUS), pnp.RGBA8), "after the refusals")
    # a rank of a group
    other = mk(fovrt_mod)
    g = fovrt_mod.Group([t, other], views=1, tile=32)
    assert lib.fr_present_enqueue(t._ctx, AT, C.byref(tk)) == UNS and tk.value == 99
    assert lib.fr_present_enqueue_device(t._ctx, AT, C.c_void_p(dp), nbytes) == UNS
    g.synchronize()
    assert (dst.cpu().numpy() == 7).all()
    g.destroy()
    t.destroy(); twin.destroy(); other.destroy()


# ---------------------------------------------------------------------------------------------
# 9. The order of the refusals
# ---------------------------------------------------------------------------------------------
def test_refusal_order(fovrt_mod):
    """Two faults at once through each of the eight enqueue entry points, on a 16 x 12 screen: the call answers with
    the code and the text of the fault that comes first in the order NULL context or ticket; reprojection or warp;
    (device forms) device_dst, then bytes; blend; buffer ids; group or sharded; ring off; reprojection not enabled;
    ring full. The ticket word stays untouched, nothing is written to the destination, and a plain present afterwards
    gives the right bytes with the next ticket."""
    import torch
    TN = fovrt_mod.TextureName
    lib = fovrt_mod.load_library()
    INV, STATE, UNS = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_STATE, fovrt_mod.FR_E_UNSUPPORTED
    w, h = 16, 12
    t = mk(fovrt_mod, w, h)
    full = w * h * 4
    dst = torch.full((full + 64,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dp = dst.data_ptr()
    SIB, POS = int(TN.SIBSON), int(TN.POSITION)
    tk = C.c_uint64(99)
    keep = []
    FORMS = {"plain": "", "warped": "_warped", "blended": "_blended", "reprojected": "_reprojected"}
    BAD_WARP = {"plain": None, "warped": "the warp is NULL", "blended": "the warp is NULL",
                "reprojected": "the reprojection is NULL"}
    BAD_DST, BAD_BYTES, BAD_BLEND = "device_dst is NULL or not", "bytes != the output's", "the blend is NULL"
    BAD_BUFFER, GROUP, RING_OFF = "the buffer is not", "a rank of a group or sharded", "presenting is not enabled"
    REPROJECT_OFF, RING_FULL = "reprojected presents are not enabled", "every slot of the ring is held"

    def ref_to(x):
        keep.append(x.c_struct())
        return C.byref(keep[-1])

    def warp(bad):
        hm = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
        if bad:
            hm[4] = np.nan
        return fovrt_mod.PresentWarp(hm)

    def args(form, device, faults):
        buf = POS if "buffer" in faults else SIB
        if form == "plain":
            a = [buf]
        elif form == "warped":
            a = [buf, ref_to(warp("warp" in faults))]
        elif form == "blended":
            a = [ref_to(fovrt_mod.PresentBlend((8.0, 6.0), 9.0 if "blend" in faults else 3.0, 6.0, buf, TN.ATROUS)),
                 ref_to(warp("warp" in faults))]
        else:
            vp = np.eye(4, dtype=np.float32).reshape(16)
            if "warp" in faults:
                vp[5] = np.inf
            a = [buf, ref_to(fovrt_mod.PresentReproject(vp, warp(False)))]
        if device:
            return a + [C.c_void_p(dp + (4 if "dst" in faults else 0)), full + (4 if "bytes" in faults else 0)]
        return a + [None if "ticket" in faults else C.byref(tk)]

    def refused(form, device, faults, code, text):
        """text: what the message holds behind the entry point's name; None: no message is left (NULL ticket)."""
        name = "fr_present_enqueue" + FORMS[form] + ("_device" if device else "")
        what = (name, faults)
        before = t.last_error()
        assert getattr(lib, name)(t._ctx, *args(form, device, faults.split())) == code, what
        assert tk.value == 99, what
        msg = t.last_error()
        if text is None:
            assert msg == before, (what, msg)
        else:
            assert msg.startswith(name + ":") and text in msg, (what, msg)
        if device:
            assert (dst.cpu().numpy() == 7).all(), what

    # the ring off, reprojected presents never enabled, no group
    for form in FORMS:  # (first: the context's message is none of the ones that a wrong order would leave here)
        refused(form, False, "ticket buffer" if form == "plain" else "ticket warp", INV, None)
    for form in FORMS:
        for device in (False, True):
            if BAD_WARP[form]:
                refused(form, device, "warp", INV, BAD_WARP[form])  # ... and the ring is off
                refused(form, device, "warp buffer", INV, BAD_WARP[form])
            refused(form, device, "buffer", INV, BAD_BUFFER)  # ... and the ring is off
            refused(form, device, "", STATE, RING_OFF)  # ... and (reprojected) the reprojection was never enabled
        if BAD_WARP[form]:
            refused(form, True, "warp dst", INV, BAD_WARP[form])
            refused(form, True, "warp bytes", INV, BAD_WARP[form])
        refused(form, True, "dst bytes", INV, BAD_DST)
        refused(form, True, "dst", INV, BAD_DST)  # ... and the ring is off
        refused(form, True, "bytes buffer", INV, BAD_BYTES)
    for device in (False, True):
        refused("blended", device, "warp blend", INV, BAD_WARP["blended"])
        refused("blended", device, "blend buffer", INV, BAD_BLEND)
        refused("blended", device, "blend", INV, BAD_BLEND)  # ... and the ring is off
    refused("blended", True, "dst blend", INV, BAD_DST)
    refused("blended", True, "bytes blend", INV, BAD_BYTES)
    # a rank of a group, the ring still off
    g = fovrt_mod.Group([t], views=1, tile=16)
    for form in FORMS:
        for device in (False, True):
            refused(form, device, "buffer", INV, BAD_BUFFER)
            refused(form, device, "", UNS, GROUP)
    g.destroy()
    # one slot, held: the ring is full; reprojected presents still not enabled
    img = pnp.image(pnp.values(), w, h)
    want = pnp.pack(img, pnp.BGRA8 | pnp.TOP_DOWN)
    t.write(TN.SIBSON, img)
    t.present_enable(1, pnp.BGRA8 | pnp.TOP_DOWN)
    held = t.present(TN.SIBSON)
    for form in FORMS:
        if BAD_WARP[form]:
            refused(form, False, "warp", INV, BAD_WARP[form])
        refused(form, False, "buffer", INV, BAD_BUFFER)
        refused(form, False, "", STATE, REPROJECT_OFF if form == "reprojected" else RING_FULL)
    refused("blended", False, "blend", INV, BAD_BLEND)
    refused("reprojected", True, "", STATE, REPROJECT_OFF)
    t.present_reproject_enable()
    refused("reprojected", False, "", STATE, RING_FULL)
    assert held == 1
    take(t, held, want, "the held ticket")
    ticket = t.present(TN.SIBSON)  # no refusal took a ticket
    assert ticket == 2
    take(t, ticket, want, "after the refusals")
    t.destroy()
