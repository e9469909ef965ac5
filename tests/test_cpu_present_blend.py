"""CPU suite for the blended present (a virtual image that is one buffer around the gaze, another in the periphery and
their smoothstep mix between two radii): the rule on the host (fr_present_blend_pack, the functions k_present_blend
and k_present_blend_warp run) against the numpy restatement in bytes, its consequences (hard edge, all inner, all
outer, weights that round to 0 and 1 inside the ramp, the warp over the blend), the refusals, and the ABI surface
without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import present_blend_np as pbn
import present_np as pnp
import present_warp_np as pwn
from helpers import ROOT

F = np.float32
NAMES = ["fr_present_blend_default", "fr_present_blend_pack", "fr_present_enqueue_blended",
         "fr_present_enqueue_blended_device"]


def B_(fovrt, gaze, r_in, r_out):
    return fovrt.PresentBlend(gaze, r_in, r_out)


# ---------------------------------------------------------------------------------------------
# 1. The host rule against numpy
# ---------------------------------------------------------------------------------------------
def test_restatement_pins():
    """What the rule says of weights anyone can check by hand, and of a d2 that is not finite."""
    s = pbn.s_of(np.array([0.0, 1.0, 2.5, 4.0, 5.0, np.inf, np.nan, -np.inf], F), 1.0, 4.0)
    assert s.tolist() == [0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 1.0, 0.0]  # t = 0.5: 0.25 * (3 - 1)
    assert pbn.s_of(np.array([1.75], F), 1.0, 4.0)[0] == F(0.0625) * F(2.5)  # t = 0.25
    assert pbn.s_of(np.array([1.0, 2.0], F), 1.0, 1.0).tolist() == [0.0, 1.0]  # no ramp: nothing divides by zero
    # smoothstep in this arithmetic never exceeds 1 (every t that is a multiple of 2^-24, which holds all t >= 0.5)
    t = (np.arange(2 ** 24 + 1, dtype=np.float64) / 2 ** 24).astype(F)
    assert pbn.s_of(t, 0.0, 1.0).max() == 1.0
    a, b = np.zeros((1, 4, 4), F), np.ones((1, 4, 4), F)
    a[..., 1], b[..., 1] = 0.5, 0.5
    # gaze on texel 0, radii 1 and 3: d2 = 0, 1, 4, 9 -> s = 0, 0, t = 3 / 8, 1
    out = pbn.pack(a, b, (0.0, 0.0), 1.0, 3.0, pnp.RGBA8)[0]
    s2 = float(F(0.375) * F(0.375) * (F(3) - F(0.75)))
    assert out[:, 0].tolist() == [0, 0, int(s2 * 255 + 0.5), 255] and (out[:, 1] == 128).all() and (out[:, 3] == 255).all()


@pytest.mark.parametrize("w,h", pwn.SCREENS)
def test_host_rule_equals_numpy(fovrt_mod, w, h):
    """fr_present_blend_pack equals present_blend_np byte for byte on the case set, in every format, over the present
    suite's value set in both sources (two different images; a small screen walks three stretches of it). Where a case
    claims a ramp, all three zones are there and the bytes of the ramp are neither plain pack's. The hard edge is a
    select between the two plain packs, radii 0 give fr_present_pack(outer), radii beyond the diagonal
    fr_present_pack(inner)."""
    for k in range(1 if w * h >= 7000 else 3):
        inner, outer = pbn.sources(w, h, k)
        assert not np.array_equal(inner, outer, equal_nan=True)
        for name, gaze, r_in, r_out, ramp in pbn.cases(w, h):
            zi, zr, zo = pbn.zones(w, h, gaze, r_in, r_out)
            if ramp:
                assert zi.any() and zr.any() and zo.any(), (w, h, name)
            for fmt in pnp.FORMATS:
                got = fovrt_mod.present_blend_pack(inner, outer, B_(fovrt_mod, gaze, r_in, r_out), None, fmt)
                ref = pbn.pack(inner, outer, gaze, r_in, r_out, fmt)
                assert got.shape == ref.shape == (h, w, 4) and got.dtype == np.uint8
                assert np.array_equal(got, ref), (w, h, name, fmt, k, np.argwhere(got != ref)[:4].tolist())
                assert (got[..., 3] == 255).all()
                pi, po = fovrt_mod.present_pack(inner, fmt), fovrt_mod.present_pack(outer, fmt)
                flip = (lambda m: m[::-1]) if fmt & pnp.TOP_DOWN else (lambda m: m)
                if ramp:
                    m = flip(zr)
                    assert not np.array_equal(got[m], pi[m]) and not np.array_equal(got[m], po[m]), (w, h, name, fmt)
                if name == "hard edge":
                    assert not zr.any()
                    assert np.array_equal(got, np.where(flip(zi)[..., None], pi, po)), (w, h, fmt)
                if name == "all outer":
                    assert zo.all() and np.array_equal(got, po), (w, h, fmt)
                if name == "all inner":
                    assert zi.all() and np.array_equal(got, pi), (w, h, fmt)


@pytest.mark.parametrize("case", pbn.POISON, ids=[c[0] for c in pbn.POISON])
def test_weight_zero_source_is_not_read(fovrt_mod, case):
    """Inside the open ramp s rounds to exactly 0 (t * t underflows) and to exactly 1 (t within 2^-13 of 1). The select
    is on s: with the source of weight zero filled with NaN the bytes there are the other source's."""
    name, gaze, r_in, r_out, value, texel = case
    w, h = 100, 70
    m = pbn.poison_texels(w, h, gaze, r_in, r_out, value)
    assert m.any() and m[texel[1], texel[0]], name  # such texels exist in the restatement, the issue's among them
    if value == 1.0:
        assert m.sum() == 7 and pbn.dist2(w, h, gaze)[texel[1], texel[0]] == 16776250.0
    good = pnp.image(pnp.values()[10:], w, h)  # (past the specials: no NaN of its own)
    inner, outer = (good.copy(), good.copy())
    poisoned = outer if value == 0.0 else inner
    poisoned[m] = np.nan
    for fmt in pnp.FORMATS:
        got = fovrt_mod.present_blend_pack(inner, outer, B_(fovrt_mod, gaze, r_in, r_out), None, fmt)
        assert np.array_equal(got, pbn.pack(inner, outer, gaze, r_in, r_out, fmt)), (name, fmt)
        mm = m[::-1] if fmt & pnp.TOP_DOWN else m
        assert np.array_equal(got[mm], fovrt_mod.present_pack(good, fmt)[mm]), (name, fmt)
    # and the poison is seen where its weight is not zero: the comparison above is not vacuous
    poisoned[...] = np.nan
    got = fovrt_mod.present_blend_pack(inner, outer, B_(fovrt_mod, gaze, r_in, r_out), None, pnp.RGBA8)
    ramp = pbn.zones(w, h, gaze, r_in, r_out)[1] & ~m
    assert ramp.any() and (got[ramp][:, :3] == 0).all()


# ---------------------------------------------------------------------------------------------
# 2. Through the warp
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", pwn.SCREENS)
def test_warp_over_the_blend(fovrt_mod, w, h):
    """The identity gives the plain blended bytes; integer shifts are numpy slices of them with border texels where the
    map leaves the image; a 2 degree turn and an odd crop equal present_warp_np over the virtual image (the blend at
    each tap, before the filter)."""
    inner, outer = pbn.sources(w, h)
    border = np.array([0, 0, 0, 255], np.uint8)
    named = {n: (hm, ow, oh) for n, hm, ow, oh in pwn.cases(fovrt_mod, w, h)}
    for name, gaze, r_in, r_out, _ramp in pbn.cases(w, h)[:5]:
        bl = B_(fovrt_mod, gaze, r_in, r_out)
        for fmt in pnp.FORMATS:
            plain = fovrt_mod.present_blend_pack(inner, outer, bl, None, fmt)
            for wp in (fovrt_mod.PresentWarp.identity(), fovrt_mod.PresentWarp.crop(0, 0, w, h)):
                assert np.array_equal(fovrt_mod.present_blend_pack(inner, outer, bl, wp, fmt), plain), (w, h, name, fmt)
            up = fovrt_mod.present_blend_pack(inner, outer, bl, None, fmt & 0xFF)  # rows bottom-up
            for dx, dy in ((1, 0), (0, -1), (w // 3, -(h // 3)), (-(w // 2), h // 2), (w, 0)):
                ow, oh = max(1, w - 1), max(1, (h + 1) // 2)
                want = np.empty((oh, ow, 4), np.uint8)
                want[:] = border
                ys, xs = np.arange(oh) + dy, np.arange(ow) + dx
                oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
                want[np.ix_(oky, okx)] = up[np.ix_(ys[oky], xs[okx])]
                if fmt & pnp.TOP_DOWN:
                    want = want[::-1]
                got = fovrt_mod.present_blend_pack(inner, outer, bl, fovrt_mod.PresentWarp.crop(dx, dy, ow, oh), fmt)
                assert np.array_equal(got, want), (w, h, name, fmt, dx, dy)
            for cname in ("turn 2.0 about 1", "odd crop", "half both"):
                hm, ow, oh = named[cname]
                got = fovrt_mod.present_blend_pack(inner, outer, bl, fovrt_mod.PresentWarp(hm, ow, oh), fmt)
                ref = pbn.warp(inner, outer, gaze, r_in, r_out, hm, ow, oh, fmt)
                assert np.array_equal(got, ref), (w, h, name, cname, fmt, np.argwhere(got != ref)[:4].tolist())


# ---------------------------------------------------------------------------------------------
# 3. Refusals of the host rule, and the surface
# ---------------------------------------------------------------------------------------------
def test_blend_pack_refusals(fovrt_mod):
    lib = fovrt_mod.load_library()
    INV = fovrt_mod.FR_E_INVALID
    a, b = np.zeros((2, 3, 4), F), np.ones((2, 3, 4), F)
    out = np.full((2, 3, 4), 7, np.uint8)
    pa, pb_, o = C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(out.ctypes.data)
    keep = []

    def bl(gaze=(1.0, 1.0), r_in=1.0, r_out=2.0):
        keep.append(B_(fovrt_mod, gaze, r_in, r_out).c_struct())
        return C.byref(keep[-1])

    def wp(h=pwn.IDENTITY, ow=0, oh=0):
        keep.append(fovrt_mod.PresentWarp(h, ow, oh).c_struct())
        return C.byref(keep[-1])

    call = lib.fr_present_blend_pack
    assert call(None, pb_, 3, 2, 0, bl(), None, o) == INV
    assert call(pa, None, 3, 2, 0, bl(), None, o) == INV
    assert call(pa, pb_, 3, 2, 0, bl(), None, None) == INV
    assert call(pa, pb_, 3, 2, 0, None, None, o) == INV
    for w, h in ((0, 2), (3, 0), (-1, 2), (32768, 1), (1, 32768)):
        assert call(pa, pb_, w, h, 0, bl(), None, o) == INV
    for fmt in (2, -1, 0x200, 0x102, 0x1000):
        assert call(pa, pb_, 3, 2, fmt, bl(), None, o) == INV
    for bad in (np.nan, np.inf, -np.inf):
        assert call(pa, pb_, 3, 2, 0, bl(gaze=(bad, 1.0)), None, o) == INV
        assert call(pa, pb_, 3, 2, 0, bl(gaze=(1.0, bad)), None, o) == INV
        assert call(pa, pb_, 3, 2, 0, bl(r_in=bad, r_out=np.inf), None, o) == INV
        assert call(pa, pb_, 3, 2, 0, bl(r_out=bad), None, o) == INV
    assert call(pa, pb_, 3, 2, 0, bl(r_in=2.0, r_out=1.0), None, o) == INV  # inner > outer
    assert call(pa, pb_, 3, 2, 0, bl(r_in=-1.0, r_out=1.0), None, o) == INV  # a negative radius
    assert call(pa, pb_, 3, 2, 0, bl(r_in=-2.0, r_out=-1.0), None, o) == INV
    assert call(pa, pb_, 3, 2, 0, bl(r_out=2e19), None, o) == INV  # outer * outer is not finite in fp32
    for ow, oh in ((4, 2), (3, 3), (0, 2), (-1, 2)):
        assert call(pa, pb_, 3, 2, 0, bl(), wp(ow=ow, oh=oh), o) == INV
    h = np.array(pwn.IDENTITY, F)
    h[4] = np.nan
    assert call(pa, pb_, 3, 2, 0, bl(), wp(h), o) == INV
    assert (out == 7).all()  # a refusal writes nothing
    # accepted: radii at the limits of the rule, the ids are ignored, the output is tight
    big = fovrt_mod.PresentBlend((1e30, -1e30), 0.0, 1.8e19, 99, -5)
    assert call(pa, pb_, 3, 2, 0, C.byref(big.c_struct()), None, o) == 0 and (out[..., :3] == 255).all()  # d2 = Inf: outer
    out[:] = 7
    assert call(pa, pb_, 3, 2, 0x101, bl(gaze=(0.0, 0.0), r_in=0.0, r_out=0.0), wp(ow=2, oh=1), o) == 0
    assert (out.reshape(-1)[:8].reshape(2, 4) == [[0, 0, 0, 255], [255, 255, 255, 255]]).all()  # texel (0, 0) is inner
    assert (out.reshape(-1)[8:] == 7).all()


def test_abi_surface_without_a_device(fovrt_mod):
    """The names are in the header, the mirror and the library; the calls that take a context answer FR_E_INVALID for
    NULL and touch nothing; the version is the one the earlier additions kept."""
    from test_cpu_abi import header_symbols
    lib = fovrt_mod.load_library()
    syms = header_symbols()
    for n in NAMES:
        assert n in syms and n in fovrt_mod._SIGS and hasattr(lib, n), n
    assert lib.fr_abi_version() == 2
    # two ints and four floats, as the header declares the struct: 24 bytes, no padding
    assert C.sizeof(fovrt_mod.fr_present_blend) == 24
    assert [f[0] for f in fovrt_mod.fr_present_blend._fields_] == ["inner_buffer", "outer_buffer", "gaze", "inner_radius_px",
                                                                   "outer_radius_px"]
    INV = fovrt_mod.FR_E_INVALID
    t = C.c_uint64(99)
    b = fovrt_mod.PresentBlend((1, 2), 3, 4).c_struct()
    assert lib.fr_present_enqueue_blended(None, C.byref(b), None, C.byref(t)) == INV and t.value == 99
    assert lib.fr_present_enqueue_blended_device(None, C.byref(b), None, C.c_void_p(256), 64) == INV
    assert lib.fr_present_blend_default(None, C.byref(b)) == INV
    assert (b.inner_buffer, b.outer_buffer, b.gaze[0], b.gaze[1], b.inner_radius_px, b.outer_radius_px) == \
        (int(fovrt_mod.TextureName.SIBSON), int(fovrt_mod.TextureName.ATROUS), 1.0, 2.0, 3.0, 4.0)
    for m in ("present_blended", "present_blended_to", "present_blend_default"):
        assert callable(getattr(fovrt_mod.PathTracer, m)), m
    assert callable(fovrt_mod.present_blend_pack)
    header = open(os.path.join(ROOT, "include", "fovrt.h")).read()
    assert "a gaze-contingent blend" not in header


FACADE_USER = r"""
#include <cstdio>
#include <cmath>
#include "fovrt.hpp"
#include "fr_math.h"
using PT = fovrt::PathTracer;
uint64_t (PT::*blended)(const fr_present_blend&, const fr_present_warp*) = &PT::present_blended;
void (PT::*to)(const fr_present_blend&, void*, size_t, const fr_present_warp*) = &PT::present_blended_to;
fovrt::PresentBlend (PT::*dflt)() = &PT::present_blend_default;
static_assert(sizeof(fr_present_blend) == 24 && sizeof(fovrt::PresentBlend) == 24, "");
int main() {
  if (!(blended && to && dflt)) return 1;
  // the rule's function on a d2 that is not a number, and on +-Inf
  std::printf("%g %g %g\n", fr::present_blend_s(NAN, 1.0f, 4.0f), fr::present_blend_s(INFINITY, 1.0f, 4.0f),
              fr::present_blend_s(-INFINITY, 1.0f, 4.0f));
  const int W = 7, H = 5;
  std::vector<float> a((size_t)W * H * 4), b(a.size());
  for (size_t k = 0; k < a.size(); k++) { a[k] = (float)(k % 11) / 10.0f; b[k] = (float)(k % 7) / 6.0f; }
  const fovrt::PresentBlend bl(2.25f, 1.5f, 1.25f, 4.5f);
  const fovrt::PresentWarp crop = fovrt::PresentWarp::crop(1, 1, 5, 3);
  for (const fr_present_warp* w : {(const fr_present_warp*)nullptr, (const fr_present_warp*)&crop}) {
    for (uint8_t v : fovrt::present_blend_pack(a, b, W, H, bl, w, FR_PRESENT_BGRA8)) std::printf("%02x", v);
    std::printf("\n");
  }
  return 0;
}
"""


def test_cpp_facade_builds_and_gives_the_same_bytes(fovrt_mod, tmp_path):
    """include/fovrt.hpp with a plain host compiler: the members exist, and present_blend_pack gives the restatement's
    bytes plain and through a crop. The same program states what present_blend_s (csrc/fr_math.h, compiled here for the
    host alone, without contraction) gives a d2 that is NaN: the outer source."""
    from test_cpu_present import host_cxx
    src, exe = tmp_path / "user.cpp", tmp_path / "user"
    src.write_text(FACADE_USER)
    pkg = os.path.dirname(fovrt_mod.LIB_PATH)
    r = subprocess.run([host_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(pkg, "csrc"), "-o", str(exe), str(src), fovrt_mod.LIB_PATH,
                        "-Wl,-rpath," + pkg, "-Wl,--allow-shlib-undefined"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split()
    assert lines[:3] == ["1", "1", "0"]
    W, H = 7, 5
    k = np.arange(W * H * 4)
    a = ((k % 11).astype(F) / F(10)).astype(F).reshape(H, W, 4)
    b = ((k % 7).astype(F) / F(6)).astype(F).reshape(H, W, 4)
    plain = pbn.pack(a, b, (2.25, 1.5), 1.25, 4.5, pnp.BGRA8)
    crop = pbn.warp(a, b, (2.25, 1.5), 1.25, 4.5, (1, 0, 1, 0, 1, 1, 0, 0, 1), 5, 3, pnp.BGRA8)
    assert lines[3] == plain.tobytes().hex() and lines[4] == crop.tobytes().hex()
    assert pbn.zones(W, H, (2.25, 1.5), 1.25, 4.5)[1].any()
