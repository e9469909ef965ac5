"""A numpy restatement of the motion-aware G-buffer (fr_set_motion_reprojection, include/fovrt.h), built on
trace_np.SceneNp: what the first G-buffer after a position update writes to WEIGHT, and the history validity the
sampling stage of that frame derives from it.

Test infrastructure only. For each pixel the camera ray is cast as trace_np.gbuffer_np casts it, the hit comes from
SceneNp.closest (brute force over every triangle, bit-exact, ties to the lowest primitive), and the rule is applied
in scalar fp32 with ptx_np.fma wherever the kernel writes an fma:

    w       = 1 - beta - gamma                                        (left to right)
    blend(P).c = fma(w, P[3k].c, fma(beta, P[3k+1].c, gamma * P[3k+2].c))
    delta   = blend(prev) - blend(cur)
    hp_prev = hp if delta == (0, 0, 0) else hp + delta                hp = front_hit_point, what POSITION stores
    WEIGHT  = (reprojection of hp_prev by prev_vp, length(hp_prev - prev_eye), 1); a miss is (-1, -1, 0, 1)

The sampling stage then tests |DEPTH_CACHE[round(qu, qv)].x - WEIGHT.z| < scene_epsilon where helpers.sampling_np
tests the distance of POSITION from the previous eye, and leaves (qu, qv, valid, 0)."""
import numpy as np

import trace_np as tn
from helpers import _round_away, _u32_sat

f = np.float32


def _blend(P, k, w, beta, gamma):
    p0, p1, p2 = P[k]
    return tuple(tn.fma(w, p0[c], tn.fma(beta, p1[c], f(gamma * p2[c]))) for c in range(3))


def motion_gbuffer_np(sc, prev_pos, cam, W, H, count_ties=False):
    """sc: SceneNp over the positions the launch traces; prev_pos: (ntris, 3, 3) float32, the positions the previous
    launch traced; cam: fr_camera uniforms. Returns {"weight": (H, W, 4) float32, "prim": (H, W) int32 hit triangle
    or -1, "ties": pixels whose closest distance two or more triangles share (count_ties only)}."""
    prev_pos = np.asarray(prev_pos, np.float32).reshape(-1, 3, 3)
    cur_pos = sc.pos
    assert prev_pos.shape == cur_pos.shape
    weight = np.zeros((H, W, 4), np.float32)
    prim = np.full((H, W), -1, np.int32)
    ties = np.zeros((H, W), bool)
    inv_vp, prev_vp = list(cam.inv_vp[:]), list(cam.prev_vp[:])
    eye, prev_eye = tn.v3(*cam.eye[:]), tn.v3(*cam.prev_eye[:])
    screen = (f(W), f(H))
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                ndc = (tn.fma(f(f(x) / screen[0]), f(2), f(-1)), tn.fma(f(f(y) / screen[1]), f(2), f(-1)))
                tmp = tn.mat_vec(inv_vp, (ndc[0], ndc[1], f(-1), f(1)))
                d = tn.normalize(tn.sub(tn.div_w(tmp), eye))
                h = sc.closest(eye, d, tn.EPS)
                if h is None:
                    weight[y, x] = (-1, -1, 0, 1)
                    continue
                k, t, beta, gamma = h
                if count_ties:
                    hit, ts, _, _ = sc._tests(eye, d, tn.EPS, np.inf)
                    ties[y, x] = int((hit & (ts == t)).sum()) > 1
                prim[y, x] = k
                hp = sc.attributes(k, t, beta, gamma, eye, d)["front"]
                w = f(f(f(1) - beta) - gamma)
                delta = tn.sub(_blend(prev_pos, k, w, beta, gamma), _blend(cur_pos, k, w, beta, gamma))
                hp_prev = hp if (delta[0] == 0 and delta[1] == 0 and delta[2] == 0) else tn.add(hp, delta)
                p = tn.mat_vec(prev_vp, (hp_prev[0], hp_prev[1], hp_prev[2], f(1)))
                iw = f(f(1) / p[3])  # compute_reprojection as g_diffuse.ptx:659-689 (trace_np.gbuffer_np)
                q = tuple(f(tn.fma(f(p[c] * iw), screen[c], screen[c]) * f(0.5)) for c in range(2))
                weight[y, x] = (q[0], q[1], tn.length(tn.sub(hp_prev, prev_eye)), 1)
    return {"weight": weight, "prim": prim, "ties": ties}


def motion_sampling_weight_np(weight, depth_cache, scene_epsilon=1e-3):
    """WEIGHT after the motion form of the sampling stage: helpers.sampling_np's validity (samplingStep.cu:96-142)
    with the G-buffer's WEIGHT.z in place of length(position - prev_eye)."""
    weight = np.asarray(weight, np.float32)
    H, W = weight.shape[:2]
    qu, qv, dist = weight[..., 0], weight[..., 1], weight[..., 2]
    with np.errstate(all="ignore"):
        inside = ((qu > f(-1)) & (qv > f(-1)) & (f(0) <= qu) & (qu < f(W) - f(0.5)) & (f(0) <= qv) &
                  (qv < f(H) - f(0.5)))
        qx = np.minimum(_u32_sat(_round_away(qu)), W - 1).astype(np.int64)
        qy = np.minimum(_u32_sat(_round_away(qv)), H - 1).astype(np.int64)
        prev = np.asarray(depth_cache, np.float32)[qy, qx, 0]
        hit = np.abs((prev - dist).astype(f)) < f(scene_epsilon)
    valid = np.where(inside & hit, f(1), f(0))
    return np.stack([qu, qv, valid, np.zeros_like(valid)], -1).astype(f)


# ---------------------------------------------------------------------------------------------
# The cases the CPU and GPU suites share: (previous positions, current positions) of a scene and the two cameras
# ---------------------------------------------------------------------------------------------
BOX = slice(2, 14)  # the refractive box of the box preset: triangles 2..13 (0, 1: the ground)


def _shift(base, sel, v):
    pos = base.copy()
    pos[sel] += np.asarray(v, np.float32)
    return pos


def box_case(base, name):
    """(prev, cur) positions of the box preset (base: (14, 3, 3)); only the refractive box moves.
    small   a few centimetres, on screen before and after
    far     the previous box stood 8 units to the right: every reprojection of a box pixel leaves the screen
    behind  the previous box stood behind the previous camera (z beyond the eye's 3.5): clip-space w < 0
    tie     the box's last face is laid over the face the preset camera sees (triangles 12, 13 = 10, 11), and the
            copies come from elsewhere: every ray through that face is a tie in t, as a ray through an edge that
            two triangles share is, and only the lowest primitive's motion is the right one"""
    base = np.asarray(base, np.float32).reshape(-1, 3, 3)
    cur = _shift(base, BOX, (0.05, 0.0, -0.03))
    if name == "small":
        return base.copy(), cur
    if name == "far":
        return _shift(base, BOX, (8.0, 0.0, 0.0)), cur
    if name == "behind":
        return _shift(base, BOX, (0.0, 0.0, 6.0)), cur
    if name == "tie":
        prev = base.copy()
        cur[12], cur[13] = cur[10], cur[11]
        prev[12], prev[13] = base[10] + np.float32(0.5), base[11] + np.float32(0.5)
        return prev, cur
    raise KeyError(name)


def sine(base, phase, amp=0.05):
    """test_gpu_bvh_refit.sine: every vertex rides a wave in y."""
    pos = np.asarray(base, np.float32).copy()
    pos[..., 1] += np.float32(amp) * np.sin(np.float32(3.0) * pos[..., 0] + np.float32(phase)).astype(np.float32)
    return pos


def cameras(fovrt, scene, W, H, panned, shift=None):
    """(uniforms of the frame before the update, uniforms of the frame after it). Still: one pose, prev == cur.
    Panned: the second frame's pose has moved and turned, its prev is the first frame's pose. shift: the second
    pose is the first translated by it (camera and target)."""
    cam = fovrt.Camera.preset(scene, W, H)
    first = cam.uniforms(W, H)
    if not panned and shift is None:
        return first, first
    cam.setPrevState()
    if shift is not None:
        cam.setPosition(np.asarray(cam.pos, np.float32) + np.asarray(shift, np.float32))
        cam.lookAt(np.asarray(cam.target, np.float32) + np.asarray(shift, np.float32))
    else:
        cam.setPosition(np.asarray(cam.pos, np.float32) + np.array([0.06, 0.02, -0.04], np.float32))
        cam.lookAt(np.asarray(cam.target, np.float32) + np.array([0.15, 0.05, 0.0], np.float32))
    return first, cam.uniforms(W, H)


# "It does what it is for": the whole box preset and the camera move by TRANSLATE between two frames. Every
# component is a power of two (the translated scene is exact up to the rounding of the sums); the vertical part
# moves the ground under a reprojection that ignores the motion by 0.125 / cos(view angle) > 1e-3 in depth.
TRANSLATE = (0.25, 0.125, -0.5)
TRANSLATE_SIZE = (45, 29)


def translate_case(base):
    """(positions before, positions after) of the translated box preset. The ground is cut down to a pad of
    2.5 x 2.5 under the box first: the identity reprojection of a pixel in column 0 or row 0 lands within 1e-4 of 0
    on either side, and the sampling stage rejects the negative ones (0 <= qu), still geometry or not; with the
    full ground that alone is 2 % of the hit pixels at this size, with the pad the left column sees the sky."""
    base = np.asarray(base, np.float32).reshape(-1, 3, 3)
    box = base[BOX].reshape(-1, 3)
    c = ((box.min(0) + box.max(0)) * np.float32(0.5)).astype(np.float32)
    before = base.copy()
    for axis in (0, 2):
        before[:2, :, axis] = c[axis] + np.sign(base[:2, :, axis]) * np.float32(1.25)
    return before, (before + np.asarray(TRANSLATE, np.float32)).astype(np.float32)
