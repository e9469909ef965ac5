"""CPU suite for the warped present (a homography between the image and the 8-bit texels: late reprojection, crop,
scale): the rule on the host (fr_present_warp_pack, the function k_present_warp runs) against the numpy restatement in
bytes on the shared case set, its consequences (identity, integer shifts), fr_present_warp_from_poses against a direct
f64 projection, the refusals, and the ABI surface without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import present_np as pnp
import present_warp_np as pwn
from helpers import ROOT

NAMES = ["fr_present_warp_pack", "fr_present_warp_from_poses", "fr_present_enqueue_warped",
         "fr_present_enqueue_warped_device"]


def W_(fovrt, h, ow=0, oh=0):
    return fovrt.PresentWarp(h, ow, oh)


# ---------------------------------------------------------------------------------------------
# 1. The host rule against numpy
# ---------------------------------------------------------------------------------------------
def test_restatement_pins():
    """What the rule says of texels anyone can check by hand: a 2 x 1 image sampled at its centres, half way between
    them, in the half texel outside it where the edge repeats, and beyond."""
    F = pnp.F
    S = np.zeros((1, 2, 4), F)
    S[0, 0, :3], S[0, 1, :3] = (0.0, 1.0, 0.2), (1.0, 0.0, 0.2)
    at = lambda c: pwn.warp(S, (0, 0, c, 0, 0, 0.5, 0, 0, 1), 1, 1, pnp.RGBA8)[0, 0].tolist()
    assert at(0.5) == [0, 255, 51, 255] and at(1.5) == [255, 0, 51, 255]
    assert at(1.0) == [128, 128, 51, 255]  # 0.5 * 255 + 0.5 = 128.0: round half up
    assert at(0.0) == [0, 255, 51, 255] and at(2.0) == [0, 0, 0, 255]  # fx = -0.5 is inside, fx = W - 0.5 is not
    assert at(-0.001) == [0, 0, 0, 255]
    assert pwn.warp(S, (1, 0, 0, 0, 1, 0, 0, 0, 0), 0, 0, pnp.RGBA8).tolist() == [[[0, 0, 0, 255]] * 2]  # w = 0
    assert pwn.warp(S, (1, 0, 0, 0, 1, 0, 0, 0, -1), 0, 0, pnp.RGBA8).tolist() == [[[0, 0, 0, 255]] * 2]  # w < 0
    S[0, 1, 0] = np.nan  # a tap of weight zero is not read; one of any weight is
    assert at(0.5)[0] == 0 and at(0.75) == [0, 191, 51, 255]  # NaN -> 0; 0.75 * 255 + 0.5 = 191.75


@pytest.mark.parametrize("w,h", pwn.SCREENS)
def test_host_rule_equals_numpy(fovrt_mod, w, h):
    """fr_present_warp_pack equals present_warp_np byte for byte on the whole case set, in every format, over the
    present suite's value set (a small screen walks three stretches of it); alpha is 255 everywhere."""
    cases = pwn.cases(fovrt_mod, w, h)
    seen_border = seen_image = False
    for k in range(1 if w * h >= 7000 else 3):
        img = pwn.source(w, h, k)
        for i, (name, hm, ow, oh) in enumerate(cases):
            for fmt in pnp.FORMATS:
                got = fovrt_mod.present_warp_pack(img, W_(fovrt_mod, hm, ow, oh), fmt)
                ref = pwn.warp(img, hm, ow, oh, fmt)
                assert got.shape == ref.shape == ((oh or h), (ow or w), 4) and got.dtype == np.uint8
                assert np.array_equal(got, ref), (w, h, name, fmt, k, np.argwhere(got != ref)[:4].tolist())
                assert (got[..., 3] == 255).all()
            inside = pwn.sample(img, hm, ow or w, oh or h)[1]
            seen_border |= bool((~inside).any())
            seen_image |= bool(inside.any())
    assert seen_border and seen_image


@pytest.mark.parametrize("w,h", pwn.SCREENS)
def test_identity_is_the_plain_present(fovrt_mod, w, h):
    """h = identity over the whole screen gives fr_present_pack's bytes for every source value, NaN and Inf next door
    included; so do the identity the scale constructor gives and fr_present_warp_from_poses of equal poses."""
    cam = pwn.case_camera(fovrt_mod, w, h)
    same = fovrt_mod.PresentWarp.from_poses(cam, cam, w, h)
    assert same.h.tolist() == list(pwn.IDENTITY) and (same.out_width, same.out_height) == (w, h)
    warps = (fovrt_mod.PresentWarp.identity(), fovrt_mod.PresentWarp.scale(w, h, w, h), same,
             fovrt_mod.PresentWarp.crop(0, 0, w, h))
    for k in range(3):
        img = pwn.source(w, h, k)
        for fmt in pnp.FORMATS:
            plain = fovrt_mod.present_pack(img, fmt)
            for wp in warps:
                assert np.array_equal(fovrt_mod.present_warp_pack(img, wp, fmt), plain), (w, h, fmt, k)


@pytest.mark.parametrize("w,h", pwn.SCREENS)
def test_integer_shifts_are_slices(fovrt_mod, w, h):
    """h = [1 0 dx; 0 1 dy; 0 0 1] with integers: numpy slicing of fr_present_pack's bytes, border texels where the
    map leaves the image; a crop is the same slice cut to the output's size."""
    img = pwn.source(w, h)
    border = np.array([0, 0, 0, 255], np.uint8)
    shifts = {(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (w // 3, -(h // 3)), (-(w // 2), h // 2), (w, 0), (0, -h)}
    for fmt in pnp.FORMATS:
        plain = fovrt_mod.present_pack(img, pnp.RGBA8 | (fmt & 0xFF))  # rows bottom-up
        for dx, dy in sorted(shifts):
            for ow, oh in ((w, h), (max(1, w - 1), max(1, (h + 1) // 2))):
                want = np.empty((oh, ow, 4), np.uint8)
                want[:] = border
                ys, xs = np.arange(oh) + dy, np.arange(ow) + dx
                oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
                want[np.ix_(oky, okx)] = plain[np.ix_(ys[oky], xs[okx])]
                if fmt & pnp.TOP_DOWN:
                    want = want[::-1]
                got = fovrt_mod.present_warp_pack(img, fovrt_mod.PresentWarp.crop(dx, dy, ow, oh), fmt)
                assert np.array_equal(got, want), (w, h, fmt, dx, dy, ow, oh)


# ---------------------------------------------------------------------------------------------
# 2. fr_present_warp_from_poses against a direct f64 projection
# ---------------------------------------------------------------------------------------------
def pv64(cam):
    v, p = cam._matrices()
    return p.astype(np.float64) @ v.astype(np.float64)


def direct(rendered, display, W, H, ow, oh, depth, xs, ys):
    """Where the rendered camera sees the world point on the display camera's ray through output texel centre
    (x + 0.5, y + 0.5) at NDC depth `depth`: source texel coordinates and the rendered camera's clip w, in f64."""
    x, y = np.meshgrid(xs.astype(np.float64) + 0.5, ys.astype(np.float64) + 0.5)
    ndc = np.stack([2 * x / ow - 1, 2 * y / oh - 1, np.full(x.shape, float(depth)), np.ones(x.shape)], -1)
    world = ndc @ np.linalg.inv(pv64(display)).T
    world = world / world[..., 3:4]
    clip = world @ pv64(rendered).T
    return (clip[..., 0] / clip[..., 3] + 1) * W / 2, (clip[..., 1] / clip[..., 3] + 1) * H / 2, clip[..., 3]


def by_h(h, xs, ys):
    h = np.asarray(h, np.float32).astype(np.float64)
    x, y = np.meshgrid(xs.astype(np.float64) + 0.5, ys.astype(np.float64) + 0.5)
    w = h[6] * x + h[7] * y + h[8]
    return (h[0] * x + h[1] * y + h[2]) / w, (h[3] * x + h[4] * y + h[5]) / w, w


BOUND = 1.0 / 64  # pixels: storage rounding moves a 4K coordinate by about 2e-4; a convention error is 0.5 or more


@pytest.mark.parametrize("W,H,ow,oh", [(100, 70, 100, 70), (100, 70, 64, 33), (3840, 2160, 3840, 2160),
                                       (3840, 2160, 1920, 1080)])
def test_from_poses_is_the_projection(fovrt_mod, W, H, ow, oh):
    """Rotations of 0.5, 2 and 10 degrees about each axis (both ways) and a small translation at depth 0.9: every 16th
    output pixel has w > 0 at fovy 45 and lands within 1 / 64 pixel of the direct projection; a pure rotation gives
    the same map for ndc_depth 0 and 1 within that bound, and its last coefficient is 1."""
    cam = fovrt_mod.Camera.preset(1, W, H)
    xs, ys = np.arange(0, ow, 16), np.arange(0, oh, 16)
    worst = 0.0
    for deg in (0.5, 2.0, 10.0, -0.5, -2.0, -10.0):
        for axis in range(3):
            disp = pwn.turned(fovrt_mod, cam, axis, deg)
            maps = [fovrt_mod.present_warp_from_poses(cam, disp, W, H, ow, oh, z) for z in (1.0, 0.0)]
            for wp, z in zip(maps, (1.0, 0.0)):
                assert wp.h[8] == 1.0 and (wp.out_width, wp.out_height) == (ow, oh)
                ex, ey, ew = direct(cam, disp, W, H, ow, oh, z, xs, ys)
                gx, gy, gw = by_h(wp.h, xs, ys)
                assert (ew > 0).all() and (gw > 0).all(), (deg, axis, z)
                err = max(np.abs(gx - ex).max(), np.abs(gy - ey).max())
                worst = max(worst, err)
                assert err <= BOUND, (deg, axis, z, err)
            a, b = by_h(maps[0].h, xs, ys), by_h(maps[1].h, xs, ys)
            assert max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()) <= BOUND, (deg, axis)
    disp = pwn.turned(fovrt_mod, cam, 1, 1.0, (0.02, -0.01, 0.015))
    near, far = (fovrt_mod.present_warp_from_poses(cam, disp, W, H, ow, oh, z) for z in (0.9, 1.0))
    ex, ey, ew = direct(cam, disp, W, H, ow, oh, 0.9, xs, ys)
    gx, gy, gw = by_h(near.h, xs, ys)
    err = max(np.abs(gx - ex).max(), np.abs(gy - ey).max())
    assert (gw > 0).all() and err <= BOUND, err
    assert not np.array_equal(near.h, far.h)  # with the eye moved the depth matters
    print("worst coordinate error, pixels:", worst, err)


def test_from_poses_exact_cases_and_refusals(fovrt_mod):
    lib = fovrt_mod.load_library()
    INV = fovrt_mod.FR_E_INVALID
    cam = fovrt_mod.Camera.preset(1, 100, 70)
    for (W, H, ow, oh) in ((100, 70, 100, 70), (3840, 2160, 3840, 2160), (49, 31, 49, 31), (1, 1, 1, 1)):
        for z in (0.0, 0.9, 1.0, -1.0):
            wp = fovrt_mod.present_warp_from_poses(cam, cam, W, H, ow, oh, z)
            assert wp.h.tolist() == list(pwn.IDENTITY), (W, H, z)
    wp = fovrt_mod.present_warp_from_poses(cam, cam, 100, 70, 49, 33, 1.0)  # equal poses, another size: the scale
    assert wp.h.tolist() == fovrt_mod.PresentWarp.scale(100, 70, 49, 33).h.tolist()
    r, d = cam._pose(), pwn.turned(fovrt_mod, cam, 1, 2.0)._pose()
    out = fovrt_mod.fr_present_warp()
    out.h[0], out.out_width = 7.0, 7
    call = lambda *a: lib.fr_present_warp_from_poses(*a)
    assert call(None, C.byref(d), 100, 70, 100, 70, 1.0, C.byref(out)) == INV
    assert call(C.byref(r), None, 100, 70, 100, 70, 1.0, C.byref(out)) == INV
    assert call(C.byref(r), C.byref(d), 100, 70, 100, 70, 1.0, None) == INV
    for sizes in ((0, 70, 100, 70), (100, 0, 100, 70), (100, 70, 0, 70), (100, 70, 100, 0), (32768, 70, 100, 70),
                  (100, 70, 100, 32768), (-1, 70, 100, 70)):
        assert call(C.byref(r), C.byref(d), *sizes, 1.0, C.byref(out)) == INV, sizes
    for z in (np.nan, np.inf, -np.inf):
        assert call(C.byref(r), C.byref(d), 100, 70, 100, 70, z, C.byref(out)) == INV
    flat = cam._pose()
    flat.zfar = flat.znear  # the projection is not finite
    assert call(C.byref(r), C.byref(flat), 100, 70, 100, 70, 1.0, C.byref(out)) == INV
    flat = cam._pose()
    flat.aspect = 0.0
    assert call(C.byref(r), C.byref(flat), 100, 70, 100, 70, 1.0, C.byref(out)) == INV
    # corner (0, 0) of the output on or behind the rendered camera's eye plane: h[8] cannot be scaled to 1
    back = pwn.turned(fovrt_mod, cam, 1, 120.0)._pose()
    assert call(C.byref(r), C.byref(back), 100, 70, 100, 70, 1.0, C.byref(out)) == INV
    strip = fovrt_mod.Camera.preset(1, 260, 2)  # aspect 130: the viewport's corners are 1.1 degrees from the eye plane
    rs = strip._pose()
    # (a turn to the left takes corner (0, 0), the lower left one, behind it; a turn to the right does the same to the
    # right-hand corners only, whose texels are border)
    assert call(C.byref(rs), C.byref(pwn.turned(fovrt_mod, strip, 1, 10.0)._pose()), 260, 2, 260, 2, 1.0, C.byref(out)) == INV
    assert out.h[0] == 7.0 and out.out_width == 7  # a refusal leaves *warp alone
    assert call(C.byref(rs), C.byref(pwn.turned(fovrt_mod, strip, 1, -10.0)._pose()), 260, 2, 260, 2, 1.0, C.byref(out)) == 0
    assert call(C.byref(r), C.byref(d), 100, 70, 100, 70, 1.0, C.byref(out)) == 0 and out.h[8] == 1.0


# ---------------------------------------------------------------------------------------------
# 3. Refusals of the host rule, and the surface
# ---------------------------------------------------------------------------------------------
def test_warp_pack_refusals(fovrt_mod):
    lib = fovrt_mod.load_library()
    INV = fovrt_mod.FR_E_INVALID
    img = np.zeros((2, 3, 4), np.float32)
    out = np.full((2, 3, 4), 7, np.uint8)
    p, o = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)

    def wp(h=pwn.IDENTITY, ow=0, oh=0):
        return C.byref(W_(fovrt_mod, h, ow, oh).c_struct())

    assert lib.fr_present_warp_pack(None, 3, 2, 0, wp(), o) == INV
    assert lib.fr_present_warp_pack(p, 3, 2, 0, wp(), None) == INV
    assert lib.fr_present_warp_pack(p, 3, 2, 0, None, o) == INV
    for w, h in ((0, 2), (3, 0), (-1, 2), (32768, 1), (1, 32768)):
        assert lib.fr_present_warp_pack(p, w, h, 0, wp(), o) == INV
    for fmt in (2, -1, 0x200, 0x102, 0x1000):
        assert lib.fr_present_warp_pack(p, 3, 2, fmt, wp(), o) == INV
    for ow, oh in ((4, 2), (3, 3), (0, 2), (3, 0), (-1, 2), (3, -1), (32768, 1)):
        assert lib.fr_present_warp_pack(p, 3, 2, 0, wp(ow=ow, oh=oh), o) == INV, (ow, oh)
    for k in range(9):
        for bad in (np.nan, np.inf, -np.inf):
            h = np.array(pwn.IDENTITY, np.float32)
            h[k] = bad
            assert lib.fr_present_warp_pack(p, 3, 2, 0, wp(h), o) == INV, (k, bad)
    assert (out == 7).all()  # a refusal writes nothing
    assert lib.fr_present_warp_pack(p, 3, 2, 0x101, wp(ow=2, oh=1), o) == 0
    assert (out.reshape(-1)[:8].reshape(2, 4) == [0, 0, 0, 255]).all() and (out.reshape(-1)[8:] == 7).all()  # tight


def test_abi_surface_without_a_device(fovrt_mod):
    """The names are in the header, the mirror and the library; the calls that take a context answer FR_E_INVALID for
    NULL and touch nothing; the version is the one the earlier additions kept."""
    from test_cpu_abi import header_symbols
    lib = fovrt_mod.load_library()
    syms = header_symbols()
    for n in NAMES:
        assert n in syms and n in fovrt_mod._SIGS and hasattr(lib, n), n
    assert lib.fr_abi_version() == 2
    INV = fovrt_mod.FR_E_INVALID
    t = C.c_uint64(99)
    wp = C.byref(fovrt_mod.PresentWarp.identity().c_struct())
    AT = int(fovrt_mod.TextureName.ATROUS)
    assert lib.fr_present_enqueue_warped(None, AT, wp, C.byref(t)) == INV and t.value == 99
    assert lib.fr_present_enqueue_warped_device(None, AT, wp, C.c_void_p(256), 64) == INV
    assert C.sizeof(fovrt_mod.fr_present_warp) == 44
    for m in ("present_warped", "present_warped_to"):
        assert callable(getattr(fovrt_mod.PathTracer, m)), m
    for m in ("identity", "crop", "scale", "from_poses"):
        assert callable(getattr(fovrt_mod.PresentWarp, m)), m
    assert callable(fovrt_mod.present_warp_pack) and callable(fovrt_mod.present_warp_from_poses)
    c = fovrt_mod.PresentWarp.crop(5, 7, 9, 11)
    assert c.h.tolist() == [1, 0, 5, 0, 1, 7, 0, 0, 1] and c.shape(100, 70) == (11, 9)
    assert fovrt_mod.PresentWarp.identity().shape(100, 70) == (70, 100)
    s = fovrt_mod.PresentWarp.scale(100, 70, 30, 20)
    assert s.h[0] == np.float32(100) / np.float32(30) and s.h[4] == np.float32(3.5)


FACADE_USER = r"""
#include "fovrt.hpp"
// the members exist with these signatures (never called: no device here)
using PT = fovrt::PathTracer;
uint64_t (PT::*warped)(int, const fr_present_warp&) = &PT::present_warped;
void (PT::*to)(int, const fr_present_warp&, void*, size_t) = &PT::present_warped_to;
static_assert(sizeof(fr_present_warp) == 44 && sizeof(fovrt::PresentWarp) == 44, "");
int main() {
  fovrt::PresentWarp id = fovrt::PresentWarp::identity(), c = fovrt::PresentWarp::crop(1, 2, 3, 4),
                     s = fovrt::PresentWarp::scale(8, 6, 4, 3);
  if (!(id.h[0] == 1 && id.h[4] == 1 && id.h[8] == 1 && id.out_width == 0 && c.h[2] == 1 && c.h[5] == 2 &&
        c.out_width == 3 && c.out_height == 4 && s.h[0] == 2 && s.h[4] == 2)) return 2;
  return warped && to && &fovrt::present_warp_pack && &fovrt::PresentWarp::from_poses ? 0 : 1;
}
"""


def test_cpp_facade_builds_with_a_plain_host_compiler(tmp_path):
    from test_cpu_present import host_cxx
    src = tmp_path / "user.cpp"
    src.write_text(FACADE_USER)
    r = subprocess.run([host_cxx(), "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
