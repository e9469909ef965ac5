"""The blended present rule (include/fovrt.h, "Present": a virtual image that mixes two sources around a gaze point)
restated in numpy float32, one rounded operation at a time, and the case set the CPU and GPU suites share.

  dx = i - gx, dy = j - gy, d2 = dx dx + dy dy            r0sq = r_in r_in, r1sq = r_out r_out (one product each)
  d2 <= r0sq: s = 0;  not d2 < r1sq: s = 1 (NaN too);  else t = (d2 - r0sq) / (r1sq - r0sq), s = (t t) (3 - 2 t)
  s == 0: inner;  s == 1: outer;  else inner (1 - s) + outer s per channel        a source of weight 0 is not read

numpy rounds every float32 operation on its own, divides correctly rounded and keeps subnormals, which is the rule's
arithmetic. The virtual image then goes through present_np.pack or stands as the source of present_warp_np.warp."""
import numpy as np

import present_np as pnp
import present_warp_np as pwn

F = np.float32


def s_of(d2, r0sq, r1sq):
    """The weight of the outer source for squared distances d2 (any shape)."""
    d2, r0sq, r1sq = np.asarray(d2, F), F(r0sq), F(r1sq)
    with np.errstate(all="ignore"):  # (the ramp's arithmetic is formed everywhere and selected where it applies)
        t = ((d2 - r0sq).astype(F) / (r1sq - r0sq)).astype(F)
        a = (F(2) * t).astype(F)
        b = (F(3) - a).astype(F)
        c = (t * t).astype(F)
        ramp = (c * b).astype(F)
        return np.where(d2 <= r0sq, F(0), np.where(~(d2 < r1sq), F(1), ramp)).astype(F)


def dist2(W, H, gaze):
    gx, gy = F(gaze[0]), F(gaze[1])
    with np.errstate(over="ignore"):
        dx = (np.arange(W, dtype=F) - gx).astype(F)[None, :]
        dy = (np.arange(H, dtype=F) - gy).astype(F)[:, None]
        return ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)


def squares(r_in, r_out):
    with np.errstate(over="ignore"):
        return (F(r_in) * F(r_in)).astype(F), (F(r_out) * F(r_out)).astype(F)


def weight(W, H, gaze, r_in, r_out):
    """(H, W) float32: s of every source texel, row 0 at the bottom."""
    return s_of(dist2(W, H, gaze), *squares(r_in, r_out))


def zones(W, H, gaze, r_in, r_out):
    """(inner, ramp, outer) texel masks by the zone tests (not by s)."""
    d2 = dist2(W, H, gaze)
    r0sq, r1sq = squares(r_in, r_out)
    inner, outer = d2 <= r0sq, ~(d2 <= r0sq) & ~(d2 < r1sq)
    return inner, ~inner & ~outer, outer


def blend(inner, outer, gaze, r_in, r_out):
    """The virtual image, (H, W, 4) float32 (alpha 0: it is never converted)."""
    inner, outer = np.asarray(inner, F), np.asarray(outer, F)
    H, W = inner.shape[:2]
    s = weight(W, H, gaze, r_in, r_out)[..., None]
    with np.errstate(all="ignore"):  # (the arm not taken may hold NaN or Inf * 0)
        u = (F(1) - s).astype(F)
        mix = ((inner[..., :3] * u).astype(F) + (outer[..., :3] * s).astype(F)).astype(F)
    rgb = np.where(s == 0, inner[..., :3], np.where(s == 1, outer[..., :3], mix)).astype(F)
    return np.concatenate([rgb, np.zeros((H, W, 1), F)], axis=2)


def pack(inner, outer, gaze, r_in, r_out, fmt):
    return pnp.pack(blend(inner, outer, gaze, r_in, r_out), fmt)


def warp(inner, outer, gaze, r_in, r_out, h, ow, oh, fmt):
    return pwn.warp(blend(inner, outer, gaze, r_in, r_out), h, ow, oh, fmt)


# ---------------------------------------------------------------------------------------------
# The case set
# ---------------------------------------------------------------------------------------------
def cases(W, H):
    """[(name, gaze, r_in, r_out, ramp)] for a W x H screen; ramp: the case claims all three zones (asserted on the
    restatement where the screen is large enough to hold them: 100 x 70)."""
    diag = float(np.hypot(W, H))
    big = W >= 100 and H >= 70
    return [
        ("centred", (W // 2, H - H // 2), 0.15 * min(W, H) + 1, 0.45 * min(W, H) + 2, big),
        ("corner", (0, 0), 0.2 * diag, 0.6 * diag, big),
        ("off screen", (-0.3 * W - 2, 1.2 * H + 1), 0.5 * diag, 1.1 * diag, big),
        ("fractional", (0.37 * W + 0.3125, 0.61 * H - 0.171875), 0.11 * diag + 0.37, 0.43 * diag + 0.73, big),
        ("hard edge", (0.5 * W, 0.5 * H), 0.3 * min(W, H) + 0.5, 0.3 * min(W, H) + 0.5, False),
        ("all outer", (0.5, 0.5), 0.0, 0.0, False),  # the gaze between texels: no d2 is 0
        ("all inner", (W // 2, H // 2), 2 * diag + 1, 3 * diag + 1, False),
    ]


# Weight exactly 0 and exactly 1 inside the open ramp, at 100 x 70: (name, gaze, r_in, r_out, the weight that occurs,
# a texel (i, j) that has it). The source of weight zero is poisoned there.
POISON = [
    ("s == 0 in the ramp", (0.0, 0.0), 0.0, 2.0 ** 40, 0.0, (1, 0)),
    ("s == 1 in the ramp", (-4095.0, -20.0), 0.0, 4096.0, 1.0, (0, 65)),
]


def poison_texels(W, H, gaze, r_in, r_out, value):
    """The texels of the open ramp whose s is exactly `value` (0 or 1)."""
    s = weight(W, H, gaze, r_in, r_out)
    return zones(W, H, gaze, r_in, r_out)[1] & (s == F(value))


def sources(W, H, k=0):
    """Two different images over the present suite's value set (NaN, +-Inf, -0, the half steps, out-of-range values)."""
    vals = pnp.values()
    n = len(vals)
    full = W * H * 3 >= n
    a = pnp.image(vals, W, H, start=0 if full else 257 * k)
    b = pnp.image(vals[::-1].copy(), W, H, start=(n // 3) if full else 257 * k + 101)
    return a, b
