"""Shared helpers for the fovrt test-suite (no GPU work at import time)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The suite's textures are stored with it (tests/golden/textures/README.md), so every checkout tests the same scenes.
ASSET_DIR = os.path.join(ROOT, "tests", "golden", "textures")
ASSETS_PRESENT = all(os.path.exists(os.path.join(ASSET_DIR, p))
                     for p in ("CedarCity.hdr", "grid.ppm", "bunny/bunny.PPM", "vokselia_spawn/vokselia_spawn.png"))
TEXTURE_MODE = 0 if ASSETS_PRESENT else 1
GOLDEN = os.path.join(ROOT, "tests", "golden")


def tea16_py(v0, v1):
    """random.h:31-46 in pure Python (uint32 wrap-around)."""
    M = 0xFFFFFFFF
    s0 = 0
    for _ in range(16):
        s0 = (s0 + 0x9e3779b9) & M
        v0 = (v0 + ((((v1 << 4) & M) + 0xa341316c) & M ^ ((v1 + s0) & M) ^ (((v1 >> 5) + 0xc8013ea4) & M))) & M
        v1 = (v1 + ((((v0 << 4) & M) + 0xad90777d) & M ^ ((v0 + s0) & M) ^ (((v0 >> 5) + 0x7e95761e) & M))) & M
    return v0


def rnd_py(seed, n):
    out = []
    for _ in range(n):
        seed = (1664525 * seed + 1013904223) & 0xFFFFFFFF
        out.append(np.float32(seed & 0xFFFFFF) / np.float32(16777216.0))
    return np.array(out, np.float32), seed


def logpolar_mask_np(W, H, gx, gy, signed=False):
    """Independent numpy restatement of the log-polar round trip (shared_helper_funcs.h:376-412,
    samplingStep.cu:180-182) with the pinned semantics: transcendentals correctly rounded to fp32
    (evaluated in f64), PTX saturating float->int conversion, uint32 wrap-around, 0xFFFFFFFF for
    make_uint2(-1.0f)."""
    f32 = np.float32
    x = np.arange(W, dtype=np.uint32)[None, :].repeat(H, 0)
    y = np.arange(H, dtype=np.uint32)[:, None].repeat(W, 1)
    cx, cy = f32(gx), f32(gy)
    bx, by = f32(W) * f32(0.25), f32(H) * f32(0.25)

    def cr(fn, *a):
        return fn(*[np.asarray(v, np.float64) for v in a]).astype(np.float32)

    def l2(a, b):
        a, b = f32(a), f32(b)
        return np.sqrt(f32(a * a) + f32(b * b), dtype=np.float32)

    def s32(v):
        v = np.asarray(v, np.float32)
        out = np.zeros(v.shape, np.int64)
        ok = ~np.isnan(v)
        out[ok] = np.clip(np.trunc(v[ok].astype(np.float64)), -2 ** 31, 2 ** 31 - 1)
        return (out & 0xFFFFFFFF).astype(np.uint32)

    xp = (x.astype(np.float32) - cx).astype(np.float32)
    yp = (y.astype(np.float32) - cy).astype(np.float32)
    L = cr(np.log, max(max(l2(cx, cy), l2(bx - cx, by - cy)), max(l2(cx, by - cy), l2(bx - cx, cy))))
    with np.errstate(all="ignore"):
        lg = cr(np.log, l2(xp, yp))
        ux = s32((cr(np.power, (lg / L).astype(np.float32), 4.0) * bx).astype(np.float32))
        two_pi = f32(2.0) * f32(np.pi)
        ang = (cr(np.arctan2, yp, xp) + (two_pi * np.where(yp < 0, f32(1), f32(0))).astype(np.float32)).astype(np.float32)
        uy = s32((ang * (by / two_pi)).astype(np.float32))
        inv_ok = ~((ux.astype(np.float32) >= bx) | (uy.astype(np.float32) >= by))
        B = two_pi / by
        K = cr(np.power, (ux.astype(np.float32) / bx).astype(np.float32), f32(1.0) / f32(4.0))
        e = cr(np.exp, (L * K).astype(np.float32))
        ox = s32((e * cr(np.cos, (B * uy.astype(np.float32)).astype(np.float32)) + cx).astype(np.float32))
        oy = s32((e * cr(np.sin, (B * uy.astype(np.float32)).astype(np.float32)) + cy).astype(np.float32))
    ox = np.where(inv_ok, ox, np.uint32(0xFFFFFFFF))
    oy = np.where(inv_ok, oy, np.uint32(0xFFFFFFFF))
    if signed:  # FR_MASK_LOGPOLAR_SIGNED: int32 differences instead of uint32 wrap-around
        dx = (x.astype(np.int64) - ox.astype(np.int32).astype(np.int64)).astype(np.int32).astype(np.float32)
        dy = (y.astype(np.int64) - oy.astype(np.int32).astype(np.int64)).astype(np.int32).astype(np.float32)
    else:
        dx = (x - ox).astype(np.float32)
        dy = (y - oy).astype(np.float32)
    thr = np.sqrt(l2(f32(1.5), f32(1.5)), dtype=np.float32)
    return (l2(dx, dy) < thr).astype(np.uint8)


def jfa_np(shading):
    """Independent vectorised numpy restatement of cpFS + jfFS ping-pong (FR/JumpFlooding.cpp:60-140)."""
    H, W = shading.shape[:2]
    f32 = np.float32
    gx = (np.arange(W, dtype=np.float32) + f32(0.5))[None, :].repeat(H, 0)
    gy = (np.arange(H, dtype=np.float32) + f32(0.5))[:, None].repeat(W, 1)
    fx, fy = gx / f32(W), gy / f32(H)
    coord = np.stack([fx, fy, np.zeros_like(fx), shading[..., 3]], -1).astype(np.float32)
    color = shading.astype(np.float32).copy()
    step = 1
    while step * 2 < W or step * 2 < H:
        step *= 2
    order = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
    while step >= 1:
        c, col = coord.copy(), color.copy()
        dx0 = (c[..., 0] - fx).astype(np.float32)
        dy0 = (c[..., 1] - fy).astype(np.float32)
        dist = np.where(c[..., 3] > 0, np.sqrt(dx0 * dx0 + dy0 * dy0, dtype=np.float32), f32(0))
        for ox, oy in order:
            qx = np.arange(W) + ox * step
            qy = np.arange(H) + oy * step
            valid = ((qx >= 0) & (qx < W))[None, :] & ((qy >= 0) & (qy < H))[:, None]
            qxc = np.broadcast_to(np.clip(qx, 0, W - 1)[None, :], (H, W))
            qyc = np.broadcast_to(np.clip(qy, 0, H - 1)[:, None], (H, W))
            nb = coord[qyc, qxc]
            ncol = color[qyc, qxc]
            ndx = (nb[..., 0] - fx).astype(np.float32)
            ndy = (nb[..., 1] - fy).astype(np.float32)
            nd = np.sqrt(ndx * ndx + ndy * ndy, dtype=np.float32)
            take = valid & (nb[..., 3] >= 1) & ((c[..., 3] < 1) | (nd < dist))
            c = np.where(take[..., None], nb, c)
            col = np.where(take[..., None], ncol, col)
            dist = np.where(take, nd, dist)
        coord, color = c, col
        step //= 2
    return coord, color


def sparse_image(W, H, mask, seed=7):
    """Synthetic shading image: colours rnd(tea16(idx, 7)) in [0,1), alpha = mask."""
    rng = np.random.default_rng(seed)
    img = rng.random((H, W, 4), dtype=np.float32)
    img[..., 3] = mask.astype(np.float32)
    img[..., :3] *= mask[..., None]
    return img


def equal_nan(a, b):
    return np.array_equal(a, b, equal_nan=True)


def rmse_per_channel(a, b):
    d = np.nan_to_num(a.astype(np.float64) - b.astype(np.float64), nan=1e9)
    return np.sqrt(np.mean(d * d, axis=tuple(range(d.ndim - 1))))


class PullPushNp:
    """Independent numpy restatement of PullPushInterpolation::render (FR/PullPushInterpolation.cpp:
    48-216) with pullFS.glsl:26-80, pushFS.glsl:39-102 and pullpushFinal.glsl:14-19 as the spec,
    written from the shader sources (not from oracle/oracle.cpp). Dispatches run over their write
    region only (texels outside it re-store their own value: pullFS.glsl:45-47, pushFS.glsl:52-54);
    reads of the atlas being written see it as it was when the dispatch began (the resolution of the
    reference's in-dispatch races that oracle and GPU share). Input zero-padded to
    S x S, S = 2^ceil(log2(max(W, H))) (the reference requires W = H = 2^e). Atlases 1.5S x S
    RGBA32F persist across calls (the push atlas carries texels across frames). At S <= 2 the host
    loop never writes the region render returns (zeros: tests/test_cpu_recon_cases.py)."""

    def __init__(self, W, H):
        S = 1
        while S < W or S < H:
            S *= 2
        self.W, self.H, self.S, self.e = W, H, S, S.bit_length() - 1
        self.AW = S + S // 2
        self.pull = np.zeros((S, self.AW, 4), np.float32)
        self.push = np.zeros((S, self.AW, 4), np.float32)

    def _load(self, img, x, y):
        """imageLoad with out-of-range reads returning 0 (x, y integer arrays)."""
        ok = (x >= 0) & (y >= 0) & (x < self.AW) & (y < self.S)
        v = img[np.clip(y, 0, self.S - 1), np.clip(x, 0, self.AW - 1)]
        return np.where(ok[..., None], v, np.float32(0))

    def render(self, sparse):
        f32 = np.float32
        W, H, S, e = self.W, self.H, self.S, self.e
        pad = np.zeros((S, S, 4), np.float32)
        pad[:H, :W] = sparse
        # pull, first dispatch (count -1): textureLod(inTex, gid / 2^e, 0) on [0,S)^2 = the input
        self.pull[:, :S] = pad
        # pull levels: step e-1 .. 0 written at (S, 2^step - 1), count 0, 1, ...
        for count, step in enumerate(range(e - 1, -1, -1)):
            n = 1 << step
            gy, gx = np.mgrid[n - 1:2 * n - 1, S:S + n]
            if count < 1:
                qx, qy = (gx - S) * 2, (gy - (S // 2 - 1)) * 2
            else:
                qx = (gx - S) * 2 + S
                qy = (gy - (n - 1)) * 2 + (n - 1 + n)
            snap = self.pull.copy()
            acc = np.zeros(gx.shape + (4,), np.float32)
            hits = np.zeros(gx.shape, np.int32)
            for ox, oy in ((0, 0), (1, 0), (1, 1), (0, 1)):  # pullFS.glsl:17-20
                rw = self._load(snap, qx + ox, qy + oy)
                take = rw[..., 3] > 0
                acc = np.where(take[..., None], (acc + rw).astype(np.float32), acc)
                hits += take
            a = acc[..., 3:4].copy()
            div = np.where(hits[..., None] > 0, (acc / np.where(a == 0, f32(1), a)).astype(np.float32), acc)
            self.pull[gy, gx] = np.concatenate([div[..., :3], (hits > 0).astype(np.float32)[..., None]], -1)
        # push: the 1x1 level at (S, 0) copies the pull texel (count -1)
        if S < self.AW:  # (S = 1: the atlas is 1 x 1 and the region lies outside it)
            self.push[0, S] = self.pull[0, S]
        offs = ((1, -1), (1, 0), (1, 1), (0, -1), (0, 0), (0, 1), (-1, -1), (-1, 0), (-1, 1))  # pushFS.glsl:27-31
        filt = [f32(1 / 16), f32(1 / 8), f32(1 / 16), f32(1 / 8), f32(1 / 4), f32(1 / 8), f32(1 / 16), f32(1 / 8),
                f32(1 / 16)]
        wox, woy = S, 1
        for count, step in zip(range(1, e + 1), range(e - 1, -1, -1)):
            n = 1 << count
            gy, gx = np.mgrid[woy:woy + n, wox:wox + n]
            inside = (gx < self.AW) & (gy < S)  # the dispatch runs over the atlas
            gy, gx = gy[inside], gx[inside]

            def tdiv2(v):  # GLSL ivec2 /= 2: truncation toward zero
                return np.sign(v) * (np.abs(v) // 2)
            if step > 0:
                qx = tdiv2(gx - S) + S
                qy = tdiv2(gy - (n - 1)) + (n - 1 - n // 2)
            else:
                qx = tdiv2(gx) + S
                qy = tdiv2(gy) + (S // 2 - 1)
            snap = self.push.copy()
            nxt = self.pull[gy, gx]
            find = np.zeros(gx.shape, np.int64)
            found = np.zeros(gx.shape, bool)
            for i, (ox, oy) in enumerate(offs):
                fc = self._load(self.pull, qx + ox, qy + oy)
                hit = (fc[..., 3] > 0) & ~found
                find = np.where(hit, i, find)
                found |= hit
            acc = np.zeros(gx.shape + (4,), np.float32)
            for i in range(9):
                k = (i + find) % 9
                ox = np.array([o[0] for o in offs])[k]
                oy = np.array([o[1] for o in offs])[k]
                acc = (acc + (filt[i] * self._load(snap, qx + ox, qy + oy)).astype(np.float32)).astype(np.float32)
            self.push[gy, gx] = np.where((nxt[..., 3] > 0)[..., None], nxt, acc)
            woy += 1 << count
            # PullPushInterpolation.cpp:191-197: the write offset moves to (0, 0) after step-- when the
            # NEXT dispatch is the last one (step == 0). At S = 2 the only dispatch already has step 0
            # and still writes at (S, 1): the full-resolution region is never written (render's output
            # stays what the atlas held, zeros).
            if step - 1 == 0:
                wox, woy = 0, 0
        return self.push[:H, :W].copy()  # pullpushFinal.glsl:14-19


def atrous_np(count, pos, nrm, col):
    """Independent numpy restatement of ATrous::render (FR/ATrous.cpp:47-132) with atFS.glsl:40-90 as
    the spec: 25 B3 taps at gl_FragCoord + offset * stepWidth (skipped off-screen), edge-stopping
    weights min(exp(-d2 / phi), 1) over colour (RGBA), normal (RGBA, / stepWidth^2) and position
    (RGBA); later iterations halve n_phi and double stepWidth. Taps sit on texel centres, so every
    texture2D read is the texel itself. exp is numpy's float32 exp (GLSL leaves its precision to
    the driver): compare with a tolerance."""
    f32 = np.float32
    H, W = col.shape[:2]
    k1 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float64)
    kern = np.outer(k1, k1).astype(np.float32)  # atFS.glsl:18-24 (rows y = +2 .. -2)
    c_phi = n_phi = p_phi = f32(1.0)
    sw = 1
    cur = col.astype(np.float32)
    for it in range(count):
        if it:
            n_phi = f32(n_phi * f32(0.5))
            sw *= 2
        s = np.zeros_like(cur)
        cw = np.zeros(cur.shape[:2], np.float32)
        for i in range(25):
            ox, oy = i % 5 - 2, 2 - i // 5
            ys = np.arange(H) + oy * sw
            xs = np.arange(W) + ox * sw
            okm = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
            yy = np.clip(ys, 0, H - 1)[:, None]
            xx = np.clip(xs, 0, W - 1)[None, :]
            ct, nt, pt = cur[yy, xx], nrm[yy, xx], pos[yy, xx]

            def d2(a, b):
                t = (a - b).astype(np.float32)
                return (((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]).astype(np.float32)
                         + t[..., 2] * t[..., 2]).astype(np.float32) + t[..., 3] * t[..., 3]).astype(np.float32)
            with np.errstate(over="ignore", invalid="ignore"):
                c_w = np.minimum(np.exp(-d2(cur, ct) / c_phi), f32(1))
                n_w = np.minimum(np.exp(-np.maximum(d2(nrm, nt) / f32(sw * sw), f32(0)) / n_phi), f32(1))
                p_w = np.minimum(np.exp(-d2(pos, pt) / p_phi), f32(1))
            w = (c_w * n_w * p_w).astype(np.float32)
            k = kern[i // 5, i % 5]
            wk = np.where(okm, (w * k).astype(np.float32), f32(0))  # cum_w += weight * kernel[i]
            # sum += ctmp * weight * kernel[i]: (ctmp * weight) * kernel[i]
            s = np.where(okm[..., None], (s + ((ct * w[..., None]).astype(np.float32) * k)).astype(np.float32), s)
            cw = (cw + wk).astype(np.float32)
        cur = (s / cw[..., None]).astype(np.float32)
    return cur


# ---------------------------------------------------------------------------------------------
# Second restatements of the stages the oracle alone pinned: numpy float32, written from the
# reference text, not from the oracle. Arithmetic pins shared with the product: fp32 with
# fma.rn exactly where the reference's compiled sampling_step contracts (tests/ptx_np.py), CUDA's atanf /
# sinf / cosf transcribed, expf (ex2.approx in the PTX) and the log-polar functions (no compiled text)
# correctly rounded (evaluated in float64, rounded once), PTX saturating float->uint conversion. The GLSL
# passes (JFA, Sibson, pull-push, A-Trous) stay unfused.
# ---------------------------------------------------------------------------------------------
_F = np.float32


def _cr(fn, *a):
    with np.errstate(all="ignore"):
        return fn(*[np.asarray(v, np.float64) for v in a]).astype(np.float32)


def _u32_sat(v):
    """make_uint2(float) = cvt.rzi.u32: truncate, saturate, NaN -> 0."""
    v = np.asarray(v, np.float32).astype(np.float64)
    out = np.where(np.isnan(v) | (v <= 0), 0.0, np.minimum(np.trunc(v), 4294967295.0))
    return out.astype(np.uint64).astype(np.uint32)


def _round_away(v):
    """CUDA roundf: half away from zero."""
    v = np.asarray(v, np.float32)
    return (np.sign(v) * np.floor(np.abs(v).astype(np.float64) + 0.5)).astype(np.float32)


def _len2(a, b):
    a, b = np.asarray(a, _F), np.asarray(b, _F)
    return np.sqrt((a * a + b * b).astype(_F), dtype=_F)


def _len2c(a, b):
    """sqrt(fma(a, a, b * b)): sampling_step's 2-D lengths as its PTX forms them (samplingStep.ptx:276-288)."""
    import ptx_np
    a, b = np.asarray(a, _F), np.asarray(b, _F)
    return ptx_np.sqrt(ptx_np.fma(a, a, (b * b).astype(_F)))


# uint2 offset[9] = {(-1, +1), (0, +1), (+1, +1), (-1, +0), (0, +0), (+1, +0), (-1, -1), (0, -1), (+1, -1)}
# (shared_helper_funcs.h:20-24): each "(a, b)" is C's comma operator, so the initialiser is the nine
# scalars b, and they fill the uint2 array flat; the rest of the array is zero.
_COMMA_PAIRS = [(-1, +1), (0, +1), (+1, +1), (-1, +0), (0, +0), (+1, +0), (-1, -1), (0, -1), (+1, -1)]
_OFFSET_FLAT = [b for (_a, b) in _COMMA_PAIRS] + [0] * 9
SOBEL_OFFSETS = np.array(_OFFSET_FLAT, np.int64).reshape(9, 2) & 0xFFFFFFFF  # uint wrap-around
SOBEL_GX = np.array([-1, -0.0, 1, -2, 0, 2, -1, -0.0, 1], np.float32)   # gx[9] (:109-113)
SOBEL_GY = np.array([-1, -2, -1, -0.0, 0, 0, 1, 2, 1], np.float32)      # gy[9] (:114-118)
_MASK_25 = np.array([[1, 1, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1], [1, 1, 1, 1]], bool)  # (:238-243)
_MASK_50 = np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]], bool)
_MASK_75 = np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], bool)


def _sobel(buf, ux, uy, g, W, H, scale=4):
    """gradient_x / gradient_y (shared_helper_funcs.h:129-151): nine taps at launch_uv + offset[i] * scale
    in uint arithmetic, skipped when the tap is outside the buffer ((float)uv >= size; uv < 0 is never
    true for a uint), summed in tap order as fma((x + y + z) / 3, g[i], sum) (samplingStep.ptx:355-359)."""
    import ptx_np
    res = np.zeros(ux.shape, _F)
    for i in range(9):
        kx = (ux.astype(np.int64) + int(SOBEL_OFFSETS[i, 0]) * scale) & 0xFFFFFFFF
        ky = (uy.astype(np.int64) + int(SOBEL_OFFSETS[i, 1]) * scale) & 0xFFFFFFFF
        ok = ~((kx.astype(np.float32) >= _F(W)) | (ky.astype(np.float32) >= _F(H)))
        kxc, kyc = np.where(ok, kx, 0).astype(np.int64), np.where(ok, ky, 0).astype(np.int64)
        d = buf[kyc, kxc]
        mean = (((d[..., 0] + d[..., 1]).astype(_F) + d[..., 2]).astype(_F) / _F(3.0)).astype(_F)
        res = np.where(ok, ptx_np.fma(mean, g[i], res), res)
    return res


def sampling_np(W, H, mask_mode, gaze, prev_eye, bbox, position, depth, depth_cache, weight, normal, diffuse,
                scene_epsilon=1e-3):
    """sampling_step (FR/cuda/samplingStep.cu:72-239) with its helpers (shared_helper_funcs.h: RGBY :66-76,
    depth_saliency :93-103, gradient_x/_y :129-151, orientation_by_sobel :152-154, gradient :155-160,
    velocity_map :206-212, heatmap :232-234, masked_sampling :257-300). Returns (mask u8, weight, extra).
    The gaze texel read of depth_saliency clamps to the screen (the pinned choice for off-window gazes)."""
    import ptx_np
    f = _F
    y, x = np.mgrid[0:H, 0:W]
    x = x.astype(np.uint32); y = y.astype(np.uint32)
    screen_x, screen_y = f(W), f(H)
    qu, qv = weight[..., 0].astype(f), weight[..., 1].astype(f)
    # reprojection validity (:96-142)
    valid = np.zeros((H, W), f)
    inside = (qu > f(-1)) & (qv > f(-1)) & (f(0) <= qu) & (qu < screen_x - f(0.5)) & (f(0) <= qv) & (qv < screen_y - f(0.5))
    qx = np.minimum(_u32_sat(_round_away(qu)), W - 1).astype(np.int64)
    qy = np.minimum(_u32_sat(_round_away(qv)), H - 1).astype(np.int64)
    prev = depth_cache[qy, qx, 0]
    dpx = (position[..., 0] - f(prev_eye[0])).astype(f)
    dpy = (position[..., 1] - f(prev_eye[1])).astype(f)
    dpz = (position[..., 2] - f(prev_eye[2])).astype(f)
    cur = ptx_np.length3(np.stack([dpx, dpy, dpz], -1))  # samplingStep.ptx:258-267
    hit = np.abs((prev - cur).astype(f)) < f(scene_epsilon)
    valid = np.where(inside & hit, f(1), f(0))
    # gaze distance (:145), normalised by the screen diagonal
    gx, gy = f(gaze[0]), f(gaze[1])
    gaze_dist = (_len2c(x.astype(f) - gx, y.astype(f) - gy) / _len2c(screen_x, screen_y)).astype(f)
    # features at the 4x4 cell origin (:186-211)
    sx, sy = (4 * (x // 4)).astype(np.uint32), (4 * (y // 4)).astype(np.uint32)
    rgba = diffuse[sy.astype(np.int64), sx.astype(np.int64)]
    r, g, b = rgba[..., 0], rgba[..., 1], rgba[..., 2]
    R = (r - ((g + b).astype(f) / f(2))).astype(f)
    G = (g - ((r + b).astype(f) / f(2))).astype(f)
    B = (b - ((r + g).astype(f) / f(2))).astype(f)
    Y = ((((r + g).astype(f) / f(2)).astype(f) - (np.abs((r - g).astype(f)) / f(2)).astype(f)).astype(f) - b).astype(f)
    Lm = (((r + g).astype(f) + b).astype(f) / f(3)).astype(f)
    rg, by = (R - G).astype(f), (B - Y).astype(f)
    dgx = _sobel(diffuse, sx, sy, SOBEL_GX, W, H)
    dgy = _sobel(diffuse, sx, sy, SOBEL_GY, W, H)
    with np.errstate(all="ignore"):
        s_orient = ptx_np.atanf((dgy / dgx).astype(f))  # CUDA's atanf (samplingStep.ptx:748-784)
    # depth_saliency(depth_buffer, sampling_uv, make_uint2(gaze), length(bbox_max - bbox_min) * 0.005)
    ex = (f(bbox[3]) - f(bbox[0])); ey = (f(bbox[4]) - f(bbox[1])); ez = (f(bbox[5]) - f(bbox[2]))
    theta = (ptx_np.length3(np.array([ex, ey, ez], f)) * f(0.005)).astype(f)
    gzx = min(int(_u32_sat(gx)), W - 1)
    gzy = min(int(_u32_sat(gy)), H - 1)
    focal = depth[gzy, gzx, 0]
    dep = (depth[sy.astype(np.int64), sx.astype(np.int64), 0] - focal).astype(f)
    dd = (f(0.4) * theta).astype(f)
    two_pi = (f(2.0) * f(np.pi)).astype(f)
    s_depth = ((f(1) / (dd * np.sqrt(two_pi, dtype=f)).astype(f)).astype(f) *
               _cr(np.exp, (-(dep * dep).astype(f) / (dd * dd).astype(f)).astype(f))).astype(f)
    s_depth = (s_depth * (f(1) * theta).astype(f)).astype(f)
    s_shadow = normal[sy.astype(np.int64), sx.astype(np.int64), 3]
    ngx = _sobel(normal, sx, sy, SOBEL_GX, W, H)
    ngy = _sobel(normal, sx, sy, SOBEL_GY, W, H)
    s_ngrad = _len2c(ngx, ngy)
    vel = (_len2c(x.astype(f) - qu, y.astype(f) - qv) * f(0.5)).astype(f)
    vel = np.where((qu < f(0)) & (qv < f(0)), f(0), vel)
    m = f(-0.4)
    va = ((vel / f(20)).astype(f) * (vel / f(20)).astype(f)).astype(f)
    s_vel = ptx_np.fma(_cr(np.exp, (-va / (m * m).astype(f)).astype(f)),
                       (f(1) / (m * np.sqrt(two_pi, dtype=f)).astype(f)).astype(f), f(1))  # :1147
    sal = (ptx_np.fma((rg + by).astype(f), f(0.5), Lm) + s_orient).astype(f) / f(3)
    sal = np.fmax(sal.astype(f), s_ngrad)
    sal = (sal * s_depth).astype(f)
    sal = (np.fmax(sal, s_vel) * s_shadow).astype(f)
    # masked_sampling (:257-300): rings around the gaze, OR a saliency-driven pattern; mask_XX[x % 4][y % 4]
    mx, my = (x % 4).astype(np.int64), (y % 4).astype(np.int64)
    r0 = f(0.07); r1 = (r0 * f(1.5)).astype(f); r2 = (r0 * f(2.0)).astype(f)
    ring = np.where((f(0) <= gaze_dist) & (gaze_dist < r0), True,
                    np.where((r0 < gaze_dist) & (gaze_dist <= r1), _MASK_25[mx, my],
                             np.where((r1 < gaze_dist) & (gaze_dist <= r2), _MASK_50[mx, my], False)))
    extra8 = ((x % 8) == 0) & ((y % 8) == 0)
    salm = np.where((f(0.01) < sal) & (sal < f(0.4)), _MASK_75[mx, my],
                    np.where((f(0.4) <= sal) & (sal < f(0.6)), _MASK_50[mx, my],
                             np.where(f(0.6) <= sal, _MASK_25[mx, my], extra8)))  # (g3 branch unreachable)
    if mask_mode == 0:
        mask = ring | salm
    elif mask_mode in (1, 4):
        mask = logpolar_mask_np(W, H, gx, gy, signed=mask_mode == 4).astype(bool)
    elif mask_mode == 2:
        mask = ((x % 2) == 0) & ((y % 2) == 0)
    else:
        mask = np.ones((H, W), bool)
    w_out = np.stack([qu, qv, valid, np.zeros_like(valid)], -1).astype(f)
    half_pi = f(np.pi / 2)
    pi = f(np.pi)
    extra = np.stack([ptx_np.cosf(((sal * half_pi).astype(f) - half_pi).astype(f)),
                      (ptx_np.sinf((sal * pi).astype(f)) * f(1.5)).astype(f),
                      ptx_np.cosf((sal * half_pi).astype(f)), np.ones_like(sal)], -1).astype(f)
    return mask.astype(np.uint8), w_out, extra


def _gl_linear_repeat(img, u, v):
    """texture2D with GL_LINEAR + GL_REPEAT at (u, v) (JumpFlooding's colour texture, FR/JumpFlooding.cpp:
    152-153), with the texture unit's 8-bit fixed-point fraction."""
    f = _F
    Ht, Wt = img.shape[:2]
    tx = (u * f(Wt) - f(0.5)).astype(f)
    ty = (v * f(Ht) - f(0.5)).astype(f)
    x0, y0 = np.floor(tx), np.floor(ty)
    a = (np.floor(((tx - x0).astype(f) * f(256)).astype(f) + f(0.5)) * f(1 / 256)).astype(f)
    b = (np.floor(((ty - y0).astype(f) * f(256)).astype(f) + f(0.5)) * f(1 / 256)).astype(f)
    ix = np.clip(np.nan_to_num(x0.astype(np.float64)), -2 ** 31, 2 ** 31 - 1).astype(np.int64)
    iy = np.clip(np.nan_to_num(y0.astype(np.float64)), -2 ** 31, 2 ** 31 - 1).astype(np.int64)
    X0, X1 = ix % Wt, (ix + 1) % Wt
    Y0, Y1 = iy % Ht, (iy + 1) % Ht
    w00 = ((f(1) - a) * (f(1) - b)).astype(f)
    w10 = (a * (f(1) - b)).astype(f)
    w01 = ((f(1) - a) * b).astype(f)
    w11 = (a * b).astype(f)
    out = (img[Y0, X0] * w00[..., None]).astype(f)
    out = (out + (img[Y0, X1] * w10[..., None]).astype(f)).astype(f)
    out = (out + (img[Y1, X0] * w01[..., None]).astype(f)).astype(f)
    return (out + (img[Y1, X1] * w11[..., None]).astype(f)).astype(f)


def sibson_np(coord, color):
    """sibsonFS.glsl:16-49 (the active "#if 1" branch), vectorised over pixels: the disc of radius
    distance(closest, frag) walked by the shader's f32 loops (h, w += 1/size), taps outside [0, 1) and
    beyond the radius skipped, GL_LINEAR colour at every tap; the average, or the closest seed's colour
    when no tap lands."""
    f = _F
    H, W = coord.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    fx = ((x.astype(f) + f(0.5)) / f(W)).astype(f)
    fy = ((y.astype(f) + f(0.5)) / f(H)).astype(f)
    cs, ct = coord[..., 0], coord[..., 1]
    closest_color = _gl_linear_repeat(color, cs, ct)
    d = _len2((cs - fx).astype(f), (ct - fy).astype(f))
    min_x, min_y = (fx - d).astype(f), (fy - d).astype(f)
    max_x, max_y = (fx + d).astype(f), (fy + d).astype(f)
    inc_x, inc_y = (f(1) / f(W)).astype(f), (f(1) / f(H)).astype(f)
    acc = np.zeros((H, W, 4), f)
    h = min_y.copy()
    while True:
        row_on = h < max_y
        if not row_on.any():
            break
        w = min_x.copy()
        while True:
            on = row_on & (w < max_x)
            if not on.any():
                break
            tap = on & ~((w < f(0)) | (w >= f(1)) | (h < f(0)) | (h >= f(1)))
            rad = _len2((fx - w).astype(f), (fy - h).astype(f))
            tap &= ~(rad > d)
            if tap.any():
                c = _gl_linear_repeat(color, w[tap], h[tap])
                add = np.concatenate([c[:, :3], np.ones((c.shape[0], 1), f)], 1)
                acc[tap] = (acc[tap] + add).astype(f)
            w = np.where(on, (w + inc_x).astype(f), w)
        h = np.where(row_on, (h + inc_y).astype(f), h)
    out = np.empty((H, W, 4), f)
    some = acc[..., 3] > f(0)
    out[some, :3] = (acc[some, :3] / acc[some, 3:4]).astype(f)
    out[some, 3] = f(1)
    out[~some] = closest_color[~some]
    return out


# The second restatement of entries 0 and 3 and the material programs (tests/trace_np.py).
from trace_np import SceneNp, gbuffer_np, shade_np  # noqa: E402,F401
