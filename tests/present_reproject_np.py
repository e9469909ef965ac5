"""The reprojected present rule (include/fovrt.h, "Present": a depth-aware splat of POSITION) restated in numpy float32,
one rounded operation at a time.

  clear    K[y][x] = all ones                                     K: oh x ow uint64, row 0 at the bottom
  splat    p = P[j][i]; skip p.xyz == 0
           cx = ((vp0 px + vp1 py) + vp2 pz) + vp3, cy (row 1), cw (row 3); skip !(cw > 0)
           sx = ((cx (1 / cw)) 0.5 + 0.5) ow, sy alike with oh; skip outside [0, ow) x [0, oh) (NaN, Inf: outside)
           K[(int)sy][(int)sx] = min(., bits(cw) << 32 | the texel's packed word)        np.minimum.at on uint64
  resolve  covered: the low word; else in a crack (left and right covered, or below and above covered): the low
           word of the smallest neighbouring key; else the fallback homography's texel (present_warp_np)

numpy rounds every float32 operation on its own, divides correctly rounded and keeps subnormals, which is the rule's
arithmetic."""
import numpy as np

import present_np as pnp
import present_warp_np as pwn

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LOW = np.uint64(0xFFFFFFFF)


def words(S, fmt):
    """(H, W) uint32: each texel's four output bytes as one word, byte 0 lowest, rows bottom-up."""
    return np.ascontiguousarray(pnp.pack(S, fmt & 0xFF)).view("<u4")[..., 0]


def place(P, vp, ow, oh):
    """Where each source texel lands: the (H, W) mask of the texels that take part, ox, oy (valid under the mask) and
    clip w."""
    P = np.asarray(P, F)
    vp = np.asarray(vp, F).reshape(16)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(all="ignore"):
        miss = (x == 0) & (y == 0) & (z == 0)
        row = lambda r: ((((vp[4 * r] * x).astype(F) + (vp[4 * r + 1] * y).astype(F)).astype(F)
                          + (vp[4 * r + 2] * z).astype(F)).astype(F) + vp[4 * r + 3]).astype(F)
        cx, cy, cw = row(0), row(1), row(3)
        front = cw > 0
        iw = (F(1) / cw).astype(F)
        sx = ((((cx * iw).astype(F) * F(0.5)).astype(F) + F(0.5)).astype(F) * F(ow)).astype(F)
        sy = ((((cy * iw).astype(F) * F(0.5)).astype(F) + F(0.5)).astype(F) * F(oh)).astype(F)
        ok = ~miss & front & (sx >= 0) & (sx < F(ow)) & (sy >= 0) & (sy < F(oh))
    ox = np.where(ok, sx, F(0)).astype(np.int64)
    oy = np.where(ok, sy, F(0)).astype(np.int64)
    return ok, ox, oy, cw


def splat(S, P, vp, ow, oh, fmt):
    """K as the splat leaves it: (oh, ow) uint64, row 0 at the bottom."""
    ok, ox, oy, cw = place(P, vp, ow, oh)
    key = (np.ascontiguousarray(cw).view(np.uint32).astype(np.uint64) << np.uint64(32)) | words(S, fmt).astype(np.uint64)
    K = np.full(oh * ow, EMPTY, np.uint64)
    np.minimum.at(K, (oy * ow + ox)[ok], key[ok])
    return K.reshape(oh, ow)


def neighbours(K):
    """left, right, below, above of every place; outside the image: EMPTY (not covered)."""
    Kp = np.full((K.shape[0] + 2, K.shape[1] + 2), EMPTY, np.uint64)
    Kp[1:-1, 1:-1] = K
    return Kp[1:-1, :-2], Kp[1:-1, 2:], Kp[:-2, 1:-1], Kp[2:, 1:-1]


def zones(K):
    """(covered, crack): where a texel landed, and where none did but the crack rule holds."""
    l, r, d, u = neighbours(K)
    covered = K != EMPTY
    crack = ~covered & (((l != EMPTY) & (r != EMPTY)) | ((d != EMPTY) & (u != EMPTY)))
    return covered, crack


def reproject(S, P, vp, h, ow, oh, fmt):
    """(H, W, 4) float32 source and POSITION -> (oh, ow, 4) uint8 by the rule; ow = oh = 0: the source's size."""
    H, W = np.asarray(S).shape[:2]
    if ow == 0 and oh == 0:
        ow, oh = W, H
    K = splat(S, P, vp, ow, oh, fmt)
    covered, crack = zones(K)
    l, r, d, u = neighbours(K)
    near = np.minimum(np.minimum(l, r), np.minimum(d, u))
    fallback = np.ascontiguousarray(pwn.warp(S, h, ow, oh, fmt & 0xFF)).view("<u4")[..., 0]
    word = np.where(covered, K & LOW, np.where(crack, near & LOW, fallback.astype(np.uint64))).astype("<u4")
    out = np.ascontiguousarray(word).view(np.uint8).reshape(oh, ow, 4)
    return np.ascontiguousarray(out[::-1] if fmt & pnp.TOP_DOWN else out)
