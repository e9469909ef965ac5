"""numpy restatement of foveation control (include/fovrt.h, beside fr_set_foveation): the 8 x 8 ordered-dither rank
table, the eccentricity mask and the ray budget's controller. fp32 throughout, every operation rounded on its own
(numpy float32 arithmetic never fuses), written from the rule's text and not from the library's source."""
import numpy as np

f32 = np.float32

# the screens, gazes and parameters both suites hold the mask to (gaze None: the screen's centre)
SCREENS = [(100, 70), (65, 3), (16, 1), (7, 5), (1, 1)]
GAZES = [None, (3.5, 66.25), (-20.0, 200.0)]
FLOORS = [1, 16, 64]
# (W, H, gaze, budget T, start radius): the closed-loop inputs; all reach the deadband within 12 launches
LOOPS = [(100, 70, (50.0, 35.0), 1400, 2.0), (100, 70, (3.5, 66.25), 1400, 30.0), (65, 3, (10.0, 1.0), 60, 1.0),
         (200, 136, (199.0, 0.0), 5440, 5.0)]


def centre(W, H):
    return (W / 2.0, H / 2.0)


def r2_values(W, H):
    return [f32(1.0), f32(106.25), r2_max(W, H)]


def r2_max(W, H):
    return f32(f32(W) * f32(W)) + f32(f32(H) * f32(H))


def rank(x, y):
    """The rank of pixel (x, y): bit i of a = (x & 7) ^ (y & 7) and of y & 7, interleaved from the top."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    yb = y & 7
    a = (x & 7) ^ yb
    r = np.zeros(np.broadcast(x, y).shape, np.int64)
    for i in range(3):
        r += (2 * ((a >> i) & 1) + ((yb >> i) & 1)) << (2 * (2 - i))
    return r


def rank_table():
    return rank(np.arange(8)[None, :], np.arange(8)[:, None])


def mask(W, H, gaze, r2, floor_ranks=1):
    """The eccentricity mask, H x W uint8."""
    x = np.arange(W, dtype=np.int64)[None, :].repeat(H, 0)
    y = np.arange(H, dtype=np.int64)[:, None].repeat(W, 1)
    rk = rank(x, y)
    dx = x.astype(np.float32) - f32(gaze[0])
    dy = y.astype(np.float32) - f32(gaze[1])
    d2 = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
    lhs = rk.astype(np.float32) * d2
    rhs = f32(64.0) * f32(r2)
    assert d2.dtype == np.float32 and lhs.dtype == np.float32 and rhs.dtype == np.float32
    return ((rk < floor_ranks) | (lhs < rhs)).astype(np.uint8)


def control(r2, n, T, tolerance, W, H):
    """One controller step from the count n of the last compaction: (next r2, held)."""
    nf, tf = f32(max(int(n), 1)), f32(T)
    if abs(f32(nf - tf)) <= f32(f32(tolerance) * tf):
        return f32(r2), True
    ratio = min(max(f32(tf / nf), f32(0.5)), f32(2.0))
    return min(max(f32(f32(r2) * ratio), f32(1.0)), r2_max(W, H)), False


def radius_r2(radius_px):
    return f32(f32(radius_px) * f32(radius_px))


def closed_loop(W, H, gaze, T, radius_px, launches, tolerance=0.02, floor_ranks=1, counts=None):
    """`launches` sampling launches, a compaction after each: [(r2 used, count, held)] per launch. counts: the counts
    to feed the controller instead of the restatement's own (a device's)."""
    r2 = radius_r2(radius_px)
    out = []
    held = False
    for k in range(launches):
        if k:
            r2, held = control(r2, out[-1][1], T, tolerance, W, H)
        n = int(mask(W, H, gaze, r2, floor_ranks).sum()) if counts is None else int(counts[k])
        out.append((r2, n, held))
    return out


def in_band(n, T, tolerance=0.02):
    return abs(f32(f32(max(n, 1)) - f32(T))) <= f32(f32(tolerance) * f32(T))
