"""Inputs for the reconstruction tests (pure numpy, no GPU): a synthetic G-buffer shaped like a traced
one, the same with a few non-finite texels, and the shape lists the CPU and GPU tests share.

Shapes are (W, H); images are (H, W, 4) float32, row 0 first."""
import numpy as np

# A-Trous: deep passes (count 4 and 5: step width 8 and 16, the untiled kernel). At 40x24 twice the
# step width exceeds the image, so most taps are off screen. 9x70 (CPU only): narrower than one tap row.
ATROUS_DEEP_SHAPES = [(83, 45), (40, 24)]
ATROUS_DEEP_COUNTS = [4, 5]
ATROUS_CPU_SHAPES = ATROUS_DEEP_SHAPES + [(9, 70)]
ATROUS_CPU_COUNTS = [1, 3, 4, 5]
# Structured input at the tiled passes: 83x45 has an odd height (a ragged last row pair for the two-row
# kernel), 16x33 is one block wide and taller than wide, 203x77 has interior and edge blocks.
ATROUS_STRUCT_SHAPES = [(83, 45), (16, 33), (203, 77)]
ATROUS_STRUCT_COUNTS = [1, 2, 3]
# (at 40x24 the NaNs of count 4 cover the whole image; at 130x97 most texels stay finite)
ATROUS_NONFINITE_SHAPES = [(40, 24), (130, 97)]
ATROUS_NONFINITE_COUNTS = [1, 3, 4]
ATROUS_ARM_SHAPES = [(83, 45), (203, 77)]
ATROUS_ARM_COUNTS = [1, 3]

# The README's bars for A-Trous (max abs error): device against the oracle, and against atrous_np.
ATROUS_BAR_ORACLE = 2e-6
ATROUS_BAR_NP = 4e-6

# Pull-push below one 64-texel tile, and taller than wide. S = 2 (the last three) is degenerate in the
# reference's host loop (test_cpu_recon_cases.test_pullpush_s2_follows_the_host_loop).
PULLPUSH_SHAPES = [(1, 1), (3, 2), (7, 5), (33, 17), (17, 33), (70, 130), (63, 64), (65, 3), (2, 2), (2, 1), (1, 2)]
PULLPUSH_DENSITIES = (0.1, 0.01, 0.3, 0.0, 1.0)

JFA_THIN_SHAPES = [(65, 3), (3, 65)]

SKY = np.array([0.5, 0.7, 1.0, 1.0], np.float32)


def gbuffer_case(W, H, seed):
    """(pos, nrm, col): a ground plane receding from 18 to 60 units, a box 4 units away in front of it
    with two faces meeting in a crease (normals (-0.6, 0, 0.8) and (0.6, 0, 0.8)), a band of miss texels
    on top (pos = nrm = 0, one flat colour: every weight among them is exactly 1), elsewhere a 4x4 checker
    of 0.2 / 0.8 plus sigma 0.05 noise, alpha 1. Box and ground are at least 13 units apart, so every
    weight across that edge is exactly 0 in expf and in a flushing exp2 (e^-169)."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:H, 0:W]
    u = (c + 0.5) / W
    v = (r + 0.5) / H
    sky = v < 0.2
    box = (u >= 0.3) & (u < 0.7) & (v >= 0.45) & (v < 0.85)
    pos = np.zeros((H, W, 4), np.float64)
    nrm = np.zeros((H, W, 4), np.float64)
    z = 18.0 + 42.0 * (1.0 - (v - 0.2) / 0.8)
    pos[..., 0], pos[..., 2], pos[..., 3] = (u - 0.5) * 1.2 * z, -z, 1.0
    nrm[..., 1], nrm[..., 3] = 1.0, 1.0
    bz = 4.0 + np.abs(u - 0.5) * 3.0
    bpos = np.stack([(u - 0.5) * 4.0, (0.85 - v) * 4.0, -bz, np.ones_like(u)], -1)
    bnrm = np.stack([np.where(u < 0.5, -0.6, 0.6), np.zeros_like(u), np.full_like(u, 0.8), np.ones_like(u)], -1)
    pos[box], nrm[box] = bpos[box], bnrm[box]
    pos[sky], nrm[sky] = 0.0, 0.0
    col = np.where(((r // 4 + c // 4) % 2 == 0)[..., None], 0.2, 0.8) + rng.normal(0.0, 0.05, (H, W, 4)) * [1, 1, 1, 0]
    col[..., 3] = 1.0
    col[sky] = SKY
    return pos.astype(np.float32), nrm.astype(np.float32), col.astype(np.float32)


def _d2(a, b):
    t = a.astype(np.float64) - b.astype(np.float64)
    return t * t  # per channel


def _band_free(pos, nrm, col, x, y, step_widths, lo, hi):
    """True when, for every tap that has (x, y) as its centre or as its neighbour, the finite part of
    ec + en + ep (float64; non-finite squared differences left out) lies outside [lo, hi]."""
    H, W = col.shape[:2]
    with np.errstate(all="ignore"):
        for it, sw in enumerate(step_widths):
            for i in range(25):
                ox, oy = (i % 5 - 2) * sw, (2 - i // 5) * sw
                tx, ty = x + ox, y + oy
                if (ox == 0 and oy == 0) or tx < 0 or tx >= W or ty < 0 or ty >= H:
                    continue
                # the 5x5 offsets are symmetric, so this one pair covers both directions
                terms = np.concatenate([_d2(col[y, x], col[ty, tx]), _d2(nrm[y, x], nrm[ty, tx]) / 2.0 ** it,
                                        _d2(pos[y, x], pos[ty, tx])])
                e = terms[np.isfinite(terms)].sum()
                if lo <= e <= hi:
                    return False
    return True


NONFINITE_KINDS = ("nan_pos", "inf_pos", "inf_col", "nan_col_channel", "nan_nrm")


def nonfinite_case(W, H, seed, counts=(1, 3, 4)):
    """gbuffer_case with five isolated texels made non-finite: a NaN position, a +Inf position (xyz), a
    +Inf colour (rgb), a colour with one NaN channel, a NaN normal. Returns (pos, nrm, col, planted) with
    planted = {kind: (x, y)}.

    Every tap that touches a planted texel has the finite part of its exponent ec + en + ep outside
    [70, 120] at every step width the given counts use (checked in float64 on the input colours with a
    margin of 8 on either side, more than the colour term can move in later passes: four channels
    within [0, 1.2]): the weight is then a normal number or exactly 0 both in expf and in a flushing
    hardware exp2. In between, Inf * denormal against Inf * 0 would differ legitimately."""
    pos, nrm, col = gbuffer_case(W, H, seed)
    rng = np.random.default_rng(seed + 1000)
    sws = [1 << k for k in range(max(counts))]
    lo, hi = 70.0 - 8.0, 120.0 + 8.0
    order = rng.permutation(W * H)
    planted = {}
    for kind in NONFINITE_KINDS:
        for p in order:
            y, x = divmod(int(p), W)
            if pos[y, x, 3] == 0:  # plant on geometry, not in the miss band
                continue
            if any(max(abs(x - px), abs(y - py)) < 3 for px, py in planted.values()):
                continue
            if _band_free(pos, nrm, col, x, y, sws, lo, hi):
                planted[kind] = (x, y)
                break
        else:
            raise AssertionError(f"no placement for {kind} at {W}x{H}")
    for kind, (x, y) in planted.items():
        if kind == "nan_pos":
            pos[y, x, :3] = np.nan
        elif kind == "inf_pos":
            pos[y, x, :3] = np.inf
        elif kind == "inf_col":
            col[y, x, :3] = np.inf
        elif kind == "nan_col_channel":
            col[y, x, 1] = np.nan
        else:
            nrm[y, x, :3] = np.nan
    for x, y in planted.values():  # the condition, on the case as it is returned
        assert _band_free(pos, nrm, col, x, y, sws, lo, hi), (x, y)
    return pos, nrm, col, planted


def noise_case(W, H, seed):
    """The input of test_atrous_within_tolerance: uniform noise in [0, 1) for position, normal, colour."""
    rng = np.random.default_rng(seed)
    return tuple(rng.random((H, W, 4), dtype=np.float32) for _ in range(3))


def pullpush_frames(W, H):
    """Five sparse frames per shape: densities 0.1, 0.01, 0.3, empty and full."""
    from helpers import sparse_image
    rng = np.random.default_rng(W + 7 * H)
    return [sparse_image(W, H, (rng.random((H, W)) < p).astype(np.uint8), seed=k)
            for k, p in enumerate(PULLPUSH_DENSITIES)]
