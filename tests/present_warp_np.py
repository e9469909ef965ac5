"""The warped present rule (include/fovrt.h, "Present": a homography between the image and the 8-bit texels) restated in
numpy float32, one rounded operation at a time, and the case set the CPU and GPU suites share.

  px = x + 0.5, py = y + 0.5                       y = r, or oh - 1 - r with TOP_DOWN
  u = (h0 px + h1 py) + h2,  v, w alike            w <= 0 (or NaN): border
  fx = u (1 / w) - 0.5, fy alike                   outside [-0.5, W - 0.5) x [-0.5, H - 0.5) (or NaN, Inf): border
  bilinear over (floor fx, floor fy), taps clamped to the image, a tap of weight 0 not read; present_np.unorm8;
  alpha 255; border = 0, 0, 0, 255

numpy rounds every float32 operation on its own, divides correctly rounded and keeps subnormals, which is the rule's
arithmetic."""
import numpy as np

import present_np as pnp

F = np.float32
IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)
# W x H, as the present suite: a row shorter than a lane's span, the 4-texel tail, a second block along x with and
# without 16-byte rows
SCREENS = [(1, 1), (3, 1), (67, 5), (100, 70), (260, 2), (261, 3)]


def sample(S, h, ow, oh):
    """The (oh, ow, 3) float32 values the rule forms before the 8-bit conversion, rows bottom-up, and the (oh, ow)
    mask of the texels that are not border (their values are 0 here)."""
    S = np.asarray(S, F)
    H, W = S.shape[:2]
    h = np.asarray(h, F).reshape(9)
    px = (np.arange(ow, dtype=F) + F(0.5))[None, :]
    py = (np.arange(oh, dtype=F) + F(0.5))[:, None]
    with np.errstate(all="ignore"):
        u = ((h[0] * px + h[1] * py) + h[2]).astype(F)
        v = ((h[3] * px + h[4] * py) + h[5]).astype(F)
        w = ((h[6] * px + h[7] * py) + h[8]).astype(F)
        front = w > 0
        iw = (F(1) / w).astype(F)
        fx = (u * iw - F(0.5)).astype(F)
        fy = (v * iw - F(0.5)).astype(F)
        inside = front & (fx >= F(-0.5)) & (fx < F(W) - F(0.5)) & (fy >= F(-0.5)) & (fy < F(H) - F(0.5))
    fx = np.where(inside, fx, F(0))
    fy = np.where(inside, fy, F(0))
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0).astype(F), (fy - y0).astype(F)
    xa, xb = np.maximum(x0.astype(np.int64), 0), np.minimum(x0.astype(np.int64) + 1, W - 1)
    ya, yb = np.maximum(y0.astype(np.int64), 0), np.minimum(y0.astype(np.int64) + 1, H - 1)
    sx, sy = (F(1) - tx).astype(F)[..., None], (F(1) - ty).astype(F)[..., None]
    tx3, ty3 = tx[..., None], ty[..., None]
    rgb = S[..., :3]

    def row(j):
        with np.errstate(all="ignore"):  # (the arm not taken may hold Inf * 0)
            mix = ((rgb[j, xa] * sx).astype(F) + (rgb[j, xb] * tx3).astype(F)).astype(F)
        return np.where(tx3 == 0, rgb[j, xa], mix)

    ra, rb = row(ya), row(yb)
    with np.errstate(all="ignore"):
        mix = ((ra * sy).astype(F) + (rb * ty3).astype(F)).astype(F)
    val = np.where(ty3 == 0, ra, mix)
    return np.where(inside[..., None], val, F(0)).astype(F), inside


def warp(S, h, ow, oh, fmt):
    """(H, W, 4) float32 -> (oh, ow, 4) uint8 by the rule; ow = oh = 0: the source's size."""
    H, W = np.asarray(S).shape[:2]
    if ow == 0 and oh == 0:
        ow, oh = W, H
    val, inside = sample(S, h, ow, oh)
    q = np.where(inside[..., None], pnp.unorm8(val), np.uint8(0))
    if fmt & 0xFF == pnp.BGRA8:
        q = q[..., ::-1]
    out = np.concatenate([q, np.full(q.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return np.ascontiguousarray(out[::-1] if fmt & pnp.TOP_DOWN else out)


# ---------------------------------------------------------------------------------------------
# Poses
# ---------------------------------------------------------------------------------------------
def quat_mul(a, b):
    """glm quaternions (w, x, y, z)."""
    aw, ax, ay, az = [float(t) for t in a]
    bw, bx, by, bz = [float(t) for t in b]
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], np.float64)


def turned(fovrt, cam, axis, deg, move=(0.0, 0.0, 0.0)):
    """A copy of the camera turned by `deg` about its own axis 0, 1 or 2 and moved by `move`."""
    out = fovrt.Camera()
    out.fovy, out.znear, out.zfar, out.aspect = cam.fovy, cam.znear, cam.zfar, cam.aspect
    half = np.deg2rad(deg) / 2
    q = np.zeros(4)
    q[0], q[1 + axis] = np.cos(half), np.sin(half)
    out.setRotation(quat_mul(cam.rot, q).astype(F))
    out.setPosition(np.asarray(cam.pos, F) + np.asarray(move, F))
    return out


def case_camera(fovrt, W, H):
    """Scene 1's preset camera. The aspect is W / H up to 4 and 4 beyond: the 260 x 2 and 261 x 3 strips would put the
    viewport's corners within two degrees of the eye plane, and a turn of 2 degrees takes corner (0, 0) behind it,
    which fr_present_warp_from_poses refuses (the CPU suite tests that refusal on its own)."""
    cam = fovrt.Camera.preset(1, W, H)
    cam.aspect = F(min(W / H, 4.0))
    return cam


# ---------------------------------------------------------------------------------------------
# The case set
# ---------------------------------------------------------------------------------------------
def out_sizes(W, H):
    """Output sizes no larger than the screen with ow % 4 of both kinds whatever W % 4 is."""
    a = max(1, (W // 4) * 4) if W >= 4 else W  # a multiple of four where the screen has room for one
    b = max(1, a - 1) if a > 1 else 1
    return [(a, H), (b, max(1, H - 1))]


def cases(fovrt, W, H):
    """[(name, h as nine float32, ow, oh)] for a W x H screen; (0, 0) stands for the screen's size."""
    up = lambda t, to: np.nextafter(F(t), F(to))
    out = [("identity", IDENTITY, 0, 0)]
    dx, dy = max(1, W // 3), max(1, H // 3)
    for name, sx, sy in (("shift left", dx, 0), ("shift right", -dx, 0), ("shift down", 0, dy), ("shift up", 0, -dy),
                         ("shift both", dx, -dy)):
        out.append((name, (1, 0, sx, 0, 1, sy, 0, 0, 1), 0, 0))
    for name, sx, sy in (("half x", 0.5, 0), ("half y", 0, 0.5), ("half both", -0.5, 0.5)):
        out.append((name, (1, 0, sx, 0, 1, sy, 0, 0, 1), 0, 0))
    out.append(("half size", (2, 0, 0, 0, 2, 0, 0, 0, 1), max(1, W // 2), max(1, H // 2)))
    ow, oh = max(1, (2 * W) // 3), max(1, (3 * H) // 4)
    out.append(("scale", (F(W) / F(ow), 0, 0, 0, F(H) / F(oh), 0, 0, 0, 1), ow, oh))
    ow, oh = max(1, (W // 2) | 1 if W > 1 else 1), max(1, (H // 2) | 1 if H > 1 else 1)
    ow, oh = min(ow, W), min(oh, H)
    out.append(("odd crop", (1, 0, (W - ow) // 2, 0, 1, (H - oh) // 2, 0, 0, 1), ow, oh))
    cam = case_camera(fovrt, W, H)
    sizes = out_sizes(W, H)
    n = 0
    for deg in (0.5, 2.0, 10.0):
        for axis in range(3):
            ow, oh = sizes[n % 2]
            n += 1
            wp = fovrt.present_warp_from_poses(cam, turned(fovrt, cam, axis, deg), W, H, ow, oh, 1.0)
            out.append((f"turn {deg} about {axis}", tuple(wp.h), ow, oh))
    wp = fovrt.present_warp_from_poses(cam, turned(fovrt, cam, 1, 1.0, (0.02, -0.01, 0.015)), W, H, W, H, 0.9)
    out.append(("moved, depth 0.9", tuple(wp.h), W, H))
    out.append(("w changes sign", (1, 0, 0, 0, 1, 0, F(-2) / F(W), 0, 1), 0, 0))
    out.append(("w changes sign along y", (1, 0, 0, 0, 1, 0, 0, F(2) / F(H), -1), 0, 0))
    out.append(("quotient overflows", (1e30, 0, 0, 0, 1e30, 0, 0, 0, 1e-30), 0, 0))
    out.append(("subnormal reciprocal", (1e38, 0, 0, 0, 1e38, 0, 0, 0, 1e38), 0, 0))
    # fx (then fy) the same for every output texel: exactly on -0.5 and on W - 0.5, and one float either side
    # (c - 0.5 is exact for c = 2^-25 and -2^-24: the floats next to -0.5)
    for name, c in (("on -0.5", F(0)), ("inside -0.5", F(2.0 ** -25)), ("outside -0.5", F(-2.0 ** -24)),
                    ("on W - 0.5", F(W)), ("inside W - 0.5", up(W, 0)), ("outside W - 0.5", up(W, 2 * W + 1))):
        out.append(("fx " + name, (0, 0, c, 0, 1, 0, 0, 0, 1), 0, 0))
    for name, c in (("on -0.5", F(0)), ("inside -0.5", F(2.0 ** -25)), ("outside -0.5", F(-2.0 ** -24)),
                    ("on H - 0.5", F(H)), ("inside H - 0.5", up(H, 0)), ("outside H - 0.5", up(H, 2 * H + 1))):
        out.append(("fy " + name, (1, 0, 0, 0, 0, c, 0, 0, 1), 0, 0))
    return [(name, np.asarray(h, F), int(ow), int(oh)) for name, h, ow, oh in out]


def source(W, H, k=0):
    """The present suite's value set under the taps: NaN, +-Inf, -0, the half steps and out-of-range values. 100 x 70
    holds all of it; a smaller screen holds the stretch that starts at 257 k."""
    return pnp.image(pnp.values(), W, H, start=0 if W * H * 3 >= len(pnp.values()) else 257 * k)
