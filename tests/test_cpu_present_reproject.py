"""CPU suite for the reprojected present (a depth-aware splat of POSITION): the rule on the host
(fr_present_reproject_pack, the functions k_present_splat and k_present_resolve run) against the numpy restatement in
bytes on the shared case set, its consequences (equal poses, all misses, ties, cracks, disocclusions),
fr_present_reproject_from_poses, the refusals, and the share of a traced frame that keeps its place, without a
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import present_np as pnp
import present_reproject_cases as prc
import present_reproject_np as prn
import present_warp_np as pwn
import ray_cases as rc
from test_cpu_present import PKG, host_cxx

NAMES = ["fr_present_reproject_from_poses", "fr_present_reproject_pack", "fr_present_reproject_enable",
         "fr_present_enqueue_reprojected", "fr_present_enqueue_reprojected_device"]
W, H = 100, 70


def ref(img, pos, rp, fmt):
    return prn.reproject(img, pos, rp.vp, rp.fallback.h, rp.fallback.out_width, rp.fallback.out_height, fmt)


def named(fovrt, w, h, ow, oh, name):
    return dict(prc.reprojections(fovrt, w, h, ow, oh))[name]


def test_symbols_are_exported(fovrt_mod):
    lib = fovrt_mod.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
    assert C.sizeof(fovrt_mod.fr_present_reproject) == 16 * 4 + 9 * 4 + 2 * 4


def test_restatement_pins():
    """What the rule says of texels anyone can check by hand: a 2 x 1 image under vp = identity, so clip = the point
    itself with w = 1."""
    S = np.zeros((1, 2, 4), pnp.F)
    S[0, 0, :3], S[0, 1, :3] = (0.0, 1.0, 0.2), (1.0, 0.0, 0.2)
    ident = np.eye(4, dtype=pnp.F).reshape(16)
    vp = ident.copy()
    vp[12:] = (0, 0, 0, 1)  # w = 1 for every point
    border = [0, 0, 0, 255]
    out_of_range = (1, 0, -5, 0, 1, -5, 0, 0, 1)  # a fallback that is border everywhere
    at = lambda P: prn.reproject(S, P, vp, out_of_range, 0, 0, pnp.RGBA8)[0].tolist()
    P = np.ones((1, 2, 4), pnp.F)
    P[0, 0, :3], P[0, 1, :3] = (-0.5, 0.0, 3.0), (0.5, 0.0, 3.0)  # each on its own centre: sx = 0.5 and 1.5
    assert at(P) == [[0, 255, 51, 255], [255, 0, 51, 255]]
    P[0, 1, :3] = (-0.5, 0.0, 3.0)  # both on texel 0, equal depth: the smaller word, 0x..33FF00 < 0x..3300FF; nothing
    assert at(P) == [[255, 0, 51, 255], border]  # on texel 1, and no crack in a 2 x 1 image
    P[0, 0, :3] = (0, 0, 0)  # a miss takes no part
    assert at(P) == [[255, 0, 51, 255], border]
    P[0, 1, :3] = (1.0, 0.0, 3.0)  # sx = ow: outside
    assert at(P) == [border, border]
    P[0, 1, :3] = (-1.0, 0.0, 3.0)  # sx = 0: inside
    assert at(P) == [[255, 0, 51, 255], border]
    vp[12:] = (0, 0, 0, 0)  # w = 0: behind
    assert at(P) == [border, border]
    # the nearer texel wins whatever its word: w = z, texel 0 at depth 3 and texel 1 at depth 2 on one place
    vp[12:] = (0, 0, 1, 0)
    P[0, 0, :3], P[0, 1, :3] = (-1.5, 0.0, 3.0), (-1.0, 0.0, 2.0)
    assert at(P) == [[255, 0, 51, 255], border]
    P[0, 1, :3] = (-2.0, 0.0, 4.0)
    assert at(P) == [[0, 255, 51, 255], border]
    # a crack: three texels, the middle place empty, takes the nearer neighbour's word
    S3 = np.zeros((1, 3, 4), pnp.F)
    S3[0, :, 0] = (0.2, 0.4, 0.6)
    P3 = np.ones((1, 3, 4), pnp.F)
    P3[0, :, :3] = [(-2.0, 0, 3.0), (-2.0, 0, 3.0), (1.0, 0, 2.0)]  # ndc -2/3, -2/3, 1/2: places 0, 0, 2
    got = prn.reproject(S3, P3, vp, out_of_range, 0, 0, pnp.RGBA8)[0].tolist()
    assert got == [[51, 0, 0, 255], [153, 0, 0, 255], [153, 0, 0, 255]]


@pytest.mark.parametrize("w,h,ow,oh", prc.SCREENS)
def test_host_rule_equals_numpy(fovrt_mod, w, h, ow, oh):
    """fr_present_reproject_pack equals present_reproject_np byte for byte on every POSITION case, display pose and
    format; alpha is 255 everywhere. Over the set every zone of the rule occurs: covered, crack, fallback."""
    rps = prc.reprojections(fovrt_mod, w, h, ow, oh)
    imgs = prc.sources(w, h)
    seen = np.zeros(3, bool)
    for i, pname in enumerate(prc.POSITIONS):
        pos = prc.position(fovrt_mod, pname, w, h)
        for j, (dname, rp) in enumerate(rps):
            img = imgs[(i + j) % 4]
            for fmt in pnp.FORMATS:
                got = fovrt_mod.present_reproject_pack(img, pos, rp, fmt)
                want = ref(img, pos, rp, fmt)
                assert got.shape == want.shape == (oh, ow, 4) and got.dtype == np.uint8
                assert np.array_equal(got, want), (w, h, pname, dname, fmt, np.argwhere(got != want)[:4].tolist())
                assert (got[..., 3] == 255).all()
            covered, crack = prn.zones(prn.splat(img, pos, rp.vp, ow, oh, pnp.RGBA8))
            seen |= np.array([covered.any(), crack.any(), (~covered & ~crack).any()])
    assert seen[0] and seen[2] and (seen[1] or w * h < 7000)


@pytest.mark.parametrize("w,h,ow,oh", [s for s in prc.SCREENS if s[:2] == s[2:]])
def test_equal_poses_give_the_plain_present(fovrt_mod, w, h, ow, oh):
    """Case (a) at equal poses: every texel of the plane lands in its own place (fp32 puts it within 1e-3 texel of
    its centre, the margin is half a texel) and the misses take the identity fallback, so the bytes are
    fr_present_pack's."""
    rp = named(fovrt_mod, w, h, ow, oh, "equal")
    pos = prc.position(fovrt_mod, prc.POSITIONS[0], w, h)
    ok, ox, oy, _cw = prn.place(pos, rp.vp, ow, oh)
    jj, ii = np.mgrid[0:h, 0:w]
    assert (ox[ok] == ii[ok]).all() and (oy[ok] == jj[ok]).all()
    assert np.array_equal(~ok, (pos[..., :3] == 0).all(-1))
    for k, img in enumerate(prc.sources(w, h)):
        for fmt in pnp.FORMATS:
            got = fovrt_mod.present_reproject_pack(img, pos, rp, fmt)
            assert np.array_equal(got, fovrt_mod.present_pack(img, fmt)), (w, h, k, fmt)


@pytest.mark.parametrize("w,h,ow,oh", prc.SCREENS)
def test_all_misses_give_the_fallback(fovrt_mod, w, h, ow, oh):
    """Case (d): nothing lands, every texel is fr_present_warp_pack of the fallback."""
    pos = prc.position(fovrt_mod, prc.POSITIONS[3], w, h)
    img = prc.sources(w, h)[1]
    for dname, rp in prc.reprojections(fovrt_mod, w, h, ow, oh):
        for fmt in pnp.FORMATS:
            got = fovrt_mod.present_reproject_pack(img, pos, rp, fmt)
            assert np.array_equal(got, fovrt_mod.present_warp_pack(img, rp.fallback, fmt)), (w, h, dname, fmt)


def test_ties_go_to_the_smaller_word(fovrt_mod):
    """Case (c) at equal poses: texels 2 k and 2 k + 1 of every other row hold one position, so both land on place
    2 k with one depth, and the place shows the smaller of their two words."""
    rp = named(fovrt_mod, W, H, W, H, "equal")
    pos = prc.position(fovrt_mod, prc.POSITIONS[2], W, H)
    img = prc.sources(W, H)[0]
    n_tied = 0
    for fmt in (pnp.RGBA8, pnp.BGRA8):
        got = fovrt_mod.present_reproject_pack(img, pos, rp, fmt).view("<u4")[..., 0]
        words = prn.words(img, fmt)
        for j in range(0, H, prc.TIE_ROWS):
            for i in range(0, (W // 2) * 2, 2):
                if (pos[j, i, :3] == 0).all():
                    continue
                assert np.array_equal(pos[j, i], pos[j, i + 1])
                assert got[j, i] == min(words[j, i], words[j, i + 1]), (fmt, i, j)
                n_tied += words[j, i] != words[j, i + 1]
    assert n_tied > 1000  # the two colours differ almost everywhere: the tie is exercised


@pytest.mark.parametrize("pose", ["closer 0.3", "closer 1.0"])
def test_cracks_take_a_neighbours_word(fovrt_mod, pose):
    """Case (a) seen from closer: the plane's texels spread, and every place nothing landed on whose left and right,
    or lower and upper, neighbours are covered carries the word of one of its covered neighbours; there are such
    places."""
    rp = named(fovrt_mod, W, H, W, H, pose)
    pos = prc.position(fovrt_mod, prc.POSITIONS[0], W, H)
    img = prc.sources(W, H)[2]
    K = prn.splat(img, pos, rp.vp, W, H, pnp.RGBA8)
    covered = K != prn.EMPTY
    got = fovrt_mod.present_reproject_pack(img, pos, rp, pnp.RGBA8).view("<u4")[..., 0]
    n = 0
    for y in range(H):
        for x in range(W):
            if covered[y, x]:
                continue
            lr = 0 < x < W - 1 and covered[y, x - 1] and covered[y, x + 1]
            du = 0 < y < H - 1 and covered[y - 1, x] and covered[y + 1, x]
            if not (lr or du):
                continue
            around = [K[b, a] for a, b in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1))
                      if 0 <= a < W and 0 <= b < H and covered[b, a]]
            assert int(got[y, x]) in {int(k) & 0xFFFFFFFF for k in around}, (x, y)
            assert int(got[y, x]) == int(min(around)) & 0xFFFFFFFF, (x, y)
            n += 1
    assert n >= 1, "no crack in the case"


def test_disocclusions_take_the_fallback(fovrt_mod):
    """Case (b) under the lateral shift: the near plane moves farther across the image than the far one, and the band
    it uncovers (no texel landed, no covered pair around it) holds the fallback homography's bytes."""
    rp = named(fovrt_mod, W, H, W, H, "lateral")
    pos = prc.position(fovrt_mod, prc.POSITIONS[1], W, H)
    img = prc.sources(W, H)[3]
    covered, crack = prn.zones(prn.splat(img, pos, rp.vp, W, H, pnp.RGBA8))
    bare = ~covered & ~crack
    inner = bare[:, 5:W - 5]  # away from the band the shift leaves at the image's edge
    assert inner.all(0).sum() >= 2, "no disoccluded band of whole columns inside the image"
    for fmt in pnp.FORMATS:
        got = fovrt_mod.present_reproject_pack(img, pos, rp, fmt)
        fb = fovrt_mod.present_warp_pack(img, rp.fallback, fmt)
        m = bare[::-1] if fmt & pnp.TOP_DOWN else bare
        assert np.array_equal(got[m], fb[m]), fmt
        assert not np.array_equal(got, fb)


def pv32(cam):
    """proj * view of fr_camera_matrices' fp32 matrices, summed in f64 in index order, rounded once."""
    v, p = (m.astype(np.float64) for m in cam._matrices())
    out = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            s = 0.0
            for k in range(4):
                s += p[r, k] * v[k, c]
            out[r, c] = s
    return out.astype(np.float32).reshape(16)


def test_from_poses(fovrt_mod):
    """vp is the display camera's proj * view; the fallback is fr_present_warp_from_poses of the same arguments; equal
    poses give the rendered camera's vp and the exact scale; a refusal leaves *rp untouched."""
    lib = fovrt_mod.load_library()
    for w, h, ow, oh in prc.SCREENS:
        cam = prc.camera(fovrt_mod, w, h)
        for name, d in prc.displays(fovrt_mod, cam):
            rp = fovrt_mod.PresentReproject.from_poses(cam, d, w, h, ow, oh, 0.9)
            wp = fovrt_mod.PresentWarp.from_poses(cam, d, w, h, ow, oh, 0.9)
            assert np.array_equal(rp.vp, pv32(d)), (w, h, name)
            assert np.array_equal(rp.fallback.h, wp.h) and (rp.fallback.out_width, rp.fallback.out_height) == (ow, oh)
        same = fovrt_mod.PresentReproject.from_poses(cam, cam, w, h, ow, oh)
        assert np.array_equal(same.vp, pv32(cam))
        assert np.array_equal(same.fallback.h, fovrt_mod.PresentWarp.scale(w, h, ow, oh).h)
    cam = prc.camera(fovrt_mod, W, H)
    r, d = cam._pose(), cam._pose()
    rp = fovrt_mod.fr_present_reproject()
    C.memset(C.byref(rp), 0x5A, C.sizeof(rp))
    before = bytes(rp)
    f = lib.fr_present_reproject_from_poses
    INV = fovrt_mod.FR_E_INVALID
    one = C.c_float(1.0)
    assert f(None, C.byref(d), W, H, W, H, one, C.byref(rp)) == INV
    assert f(C.byref(r), None, W, H, W, H, one, C.byref(rp)) == INV
    assert f(C.byref(r), C.byref(d), W, H, W, H, one, None) == INV
    for size in ((0, H, W, H), (W, 0, W, H), (W, H, 0, H), (W, H, W, 32768), (-1, H, W, H)):
        assert f(C.byref(r), C.byref(d), *size, one, C.byref(rp)) == INV, size
    assert f(C.byref(r), C.byref(d), W, H, W, H, C.c_float(np.nan), C.byref(rp)) == INV
    bad = cam._pose()
    bad.pos[0] = float("nan")
    assert f(C.byref(r), C.byref(bad), W, H, W, H, one, C.byref(rp)) == INV
    behind = pwn.turned(fovrt_mod, cam, 1, 120.0)._pose()  # the output's corner lies behind the rendered camera
    assert f(C.byref(r), C.byref(behind), W, H, W, H, one, C.byref(rp)) == INV
    assert bytes(rp) == before
    assert f(C.byref(r), C.byref(d), W, H, W, H, one, C.byref(rp)) == fovrt_mod.FR_OK and bytes(rp) != before


def test_pack_refusals(fovrt_mod):
    """Every argument refusal of fr_present_reproject_pack: nothing is written."""
    lib = fovrt_mod.load_library()
    INV = fovrt_mod.FR_E_INVALID
    w, h = 8, 4
    img = np.ascontiguousarray(pwn.source(w, h))
    pos = np.ascontiguousarray(prc.position(fovrt_mod, prc.POSITIONS[0], w, h))
    out = np.full(w * h * 4 + 16, 7, np.uint8)
    good = named(fovrt_mod, w, h, w, h, "turn 2")
    keep = []

    def call(rgba=img, position=pos, width=w, height=h, fmt=pnp.RGBA8, rp=good):
        if rp is not None:
            keep.append(rp.c_struct())
        return lib.fr_present_reproject_pack(None if rgba is None else C.c_void_p(rgba.ctypes.data),
                                             None if position is None else C.c_void_p(position.ctypes.data), width,
                                             height, fmt, None if rp is None else C.byref(keep[-1]),
                                             C.c_void_p(out.ctypes.data))

    def with_(vp=None, hm=None, ow=w, oh=h):
        r = fovrt_mod.PresentReproject(good.vp if vp is None else vp,
                                       fovrt_mod.PresentWarp(good.fallback.h if hm is None else hm, ow, oh))
        return r

    assert call(rgba=None) == INV and call(position=None) == INV and call(rp=None) == INV
    assert lib.fr_present_reproject_pack(C.c_void_p(img.ctypes.data), C.c_void_p(pos.ctypes.data), w, h, 0,
                                         C.byref(good.c_struct()), None) == INV
    for width, height in ((0, h), (w, 0), (-3, h), (32768, h), (w, 32768)):
        assert call(width=width, height=height) == INV, (width, height)
    for fmt in (2, 0x200, 0x101 + 1, -1):
        assert call(fmt=fmt) == INV, fmt
    for k in (0, 7, 15):
        for bad in (np.nan, np.inf, -np.inf):
            vp = good.vp.copy()
            vp[k] = bad
            assert call(rp=with_(vp=vp)) == INV, (k, bad)
    for k in (0, 8):
        hm = good.fallback.h.copy()
        hm[k] = np.nan
        assert call(rp=with_(hm=hm)) == INV, k
    for ow, oh in ((w + 1, h), (w, h + 1), (0, h), (w, 0), (-1, h)):
        assert call(rp=with_(ow=ow, oh=oh)) == INV, (ow, oh)
    assert (out == 7).all()
    assert call() == fovrt_mod.FR_OK and (out[w * h * 4:] == 7).all() and not (out[:w * h * 4] == 7).all()
    assert call(rp=with_(ow=0, oh=0)) == fovrt_mod.FR_OK  # 0, 0: the source's size


@pytest.mark.parametrize("scene", [1, 2])
def test_traced_frames_keep_their_places(fovrt_mod, oracle, scene, capsys):
    """The oracle's G-buffer of the preset view at 100 x 70, reprojected to the pose it was traced with: the share of
    texels that equal the plain present, reported and not held to a threshold (the hit point is offset along the
    normal, so a texel at a grazing angle may land next door). What must hold: the bytes are the restatement's."""
    cam = fovrt_mod.Camera.preset(scene, W, H)
    g = oracle.gbuffer(oracle.OracleScene(rc.scene_arrays(fovrt_mod, scene)), cam.uniforms(W, H), W, H, 0)
    pos, img = g["position"], g["diffuse"]
    rp = fovrt_mod.PresentReproject.from_poses(cam, cam, W, H)
    got = fovrt_mod.present_reproject_pack(img, pos, rp, pnp.RGBA8)
    assert np.array_equal(got, ref(img, pos, rp, pnp.RGBA8))
    plain = fovrt_mod.present_pack(img, pnp.RGBA8)
    same = (got == plain).all(-1)
    ok, ox, oy, _cw = prn.place(pos, rp.vp, W, H)
    jj, ii = np.mgrid[0:H, 0:W]
    home = ok & (ox == ii) & (oy == jj)
    # The G-buffer's primary ray of texel (i, j) goes through the texel's lower left corner (NDC 2 i / W - 1), so its
    # hit point projects onto the boundary between two places and rounding picks the side. A caller who wants the
    # points in the middle of their places adds row 3 of vp, times 1 / ow and 1 / oh, to rows 0 and 1 (half a texel in
    # NDC): reported as "centred".
    centred = fovrt_mod.PresentReproject(rp.vp.copy(), rp.fallback)
    centred.vp[0:4] = (rp.vp[0:4].astype(np.float64) + rp.vp[12:16].astype(np.float64) / W).astype(np.float32)
    centred.vp[4:8] = (rp.vp[4:8].astype(np.float64) + rp.vp[12:16].astype(np.float64) / H).astype(np.float32)
    got_c = fovrt_mod.present_reproject_pack(img, pos, centred, pnp.RGBA8)
    assert np.array_equal(got_c, ref(img, pos, centred, pnp.RGBA8))
    okc, oxc, oyc, _ = prn.place(pos, centred.vp, W, H)
    home_c = okc & (oxc == ii) & (oyc == jj)
    with capsys.disabled():
        print(f"\n[reprojected present, scene {scene}, {W} x {H}, equal poses] texels equal to the plain present: "
              f"{same.mean():.4f}; hits: {ok.mean():.4f}; hits that land on their own place: "
              f"{home.sum() / max(ok.sum(), 1):.4f}; with vp centred by half a texel: equal "
              f"{(got_c == plain).all(-1).mean():.4f}, own place {home_c.sum() / max(okc.sum(), 1):.4f}")
    assert ok.any() and same.any()


def test_rule_under_the_host_sanitizers(tmp_path):
    """tools/present_reproject_check.cpp (its own main, no device, nothing of it loaded into this process) builds with
    AddressSanitizer and UndefinedBehaviorSanitizer and exits 0 after driving the rule's functions of fr_math.h over
    hostile positions and matrices with every array behind a checked index."""
    exe = tmp_path / "present_reproject_check"
    r = subprocess.run([host_cxx(), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o",
                        str(exe), os.path.join(PKG, "tools", "present_reproject_check.cpp")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "fallback texels: ok" in r.stdout
