"""The present rule (include/fovrt.h, "Present") restated in numpy float32, one rounded operation at a time, and the
value set the CPU and GPU suites share.

  v = (x != x) ? 0 : min(max(x, 0), 1)        NaN -> 0, -Inf -> 0, +Inf -> 1, -0 -> 0
  q = (uint8)(uint32)(v * 255 + 0.5)          one product, one sum, truncation
"""
import numpy as np

F = np.float32
RGBA8, BGRA8, TOP_DOWN = 0, 1, 0x100
FORMATS = (RGBA8, BGRA8, RGBA8 | TOP_DOWN, BGRA8 | TOP_DOWN)


def unorm8(x):
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(x), F(0), np.minimum(np.maximum(x, F(0)), F(1))).astype(F)
    p = (v * F(255)).astype(F)  # the product, rounded
    s = (p + F(0.5)).astype(F)  # the sum, rounded
    return s.astype(np.uint32).astype(np.uint8)  # in [0.5, 255.5]: the conversion truncates


def pack(rgba, fmt):
    """(H, W, 4) float32 -> (H, W, 4) uint8: r g b 255 or b g r 255 per texel; TOP_DOWN: output row r = image row H-1-r."""
    rgba = np.asarray(rgba, F)
    q = unorm8(rgba[..., :3])
    if fmt & 0xFF == BGRA8:
        q = q[..., ::-1]
    out = np.concatenate([q, np.full(q.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return np.ascontiguousarray(out[::-1] if fmt & TOP_DOWN else out)


def half_steps():
    """The 255 half steps (k + 0.5) / 255 in fp32 with the floats one ulp either side of each: where an fma, which
    rounds v * 255 + 0.5 once, and the rule, which rounds twice, part ways."""
    h = ((np.arange(255, dtype=F) + F(0.5)) / F(255)).astype(F)
    return np.stack([np.nextafter(h, F(0)), h, np.nextafter(h, F(2))], axis=1).reshape(-1)


def values(seed=7):
    """Edge values first (small screens hold a prefix of the set): the specials, the half steps, k / 255, then 10^4
    random floats in [-0.25, 1.25]."""
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 2.0, np.finfo(F).smallest_subnormal,
                        np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2))], F)
    exact = (np.arange(256, dtype=F) / F(255)).astype(F)
    rnd = np.random.default_rng(seed).uniform(-0.25, 1.25, 10000).astype(F)
    return np.concatenate([special, half_steps(), exact, rnd])


ALPHAS = np.array([np.nan, 0.0, 0.3, 1.0, -5.0, np.inf], F)  # alpha is stored but never converted


def image(vals, w, h, start=0):
    """An (h, w, 4) image whose r, g, b channels walk `vals` from `start` (wrapping) in texel order; alpha cycles
    through ALPHAS."""
    n = w * h
    idx = (start + np.arange(3 * n)) % len(vals)
    img = np.empty((h, w, 4), F)
    img[..., :3] = vals[idx].reshape(h, w, 3)
    img[..., 3] = ALPHAS[np.arange(n) % len(ALPHAS)].reshape(h, w)
    return img
