"""Adversarial geometry for the BVH builders: pure functions (base_pos[n, 3, 3], seed) -> pos[n, 3, 3],
float32 and finite, every vertex inside the base scene's bounding box (the coordinate scale at which the
bit-exact tests pin the traversal arithmetic). Each case drives the device LBVH (k_bvh.hip) down a path the
preset scenes never take; its docstring says which. Where a case does not fix which triangle goes where, the
seed permutes the triangle order (the Morton sort then has work to do); the property a case claims holds for
every seed.

Also here: the three camera poses the BVH tests look from, and their primary rays in numpy.
"""
import numpy as np

F = np.float32


def _box(base):
    flat = np.asarray(base, F).reshape(-1, 3)
    return flat.min(0), flat.max(0)


def _finish(pos, base, seed, shuffle=True):
    lo, hi = _box(base)
    pos = np.clip(np.asarray(pos, F), lo, hi)
    if shuffle:
        pos = pos[np.random.default_rng(seed).permutation(pos.shape[0])]
    assert pos.shape == np.asarray(base).shape and pos.dtype == F and np.isfinite(pos).all()
    return np.ascontiguousarray(pos)


def _at(lo, hi, fx, fy, fz):
    """The point at fractions (fx, fy, fz) of the box, float32."""
    return (lo + (hi - lo) * np.array([fx, fy, fz], F)).astype(F)


def identical(base, seed):
    """Every triangle is the same tilted triangle in the middle of the box: all Morton codes are equal (the
    hierarchy comes from kdelta's index tie-break alone), every hit is an exact t tie, and the lowest
    primitive index has to win."""
    lo, hi = _box(base)
    tri = np.stack([_at(lo, hi, 0.40, 0.05, 0.62), _at(lo, hi, 0.62, 0.10, 0.45), _at(lo, hi, 0.45, 0.95, 0.42)])
    return _finish(np.broadcast_to(tri, np.asarray(base).shape).copy(), base, seed, shuffle=False)


def pairs(base, seed):
    """Triangle 2k+1 is an exact copy of triangle 2k of the base geometry: equal boxes, equal centroids and
    equal codes in pairs, and every surface (the glass faces too) is there twice."""
    pos = np.asarray(base, F).copy()
    m = pos.shape[0] // 2
    pos[1:2 * m:2] = pos[0:2 * m:2]
    return _finish(pos, base, seed, shuffle=False)


def _sheet(base, seed, axis):
    lo, hi = _box(base)
    n = np.asarray(base).shape[0]
    g = int(np.ceil(np.sqrt((n + 1) // 2)))  # g x g cells, two triangles each
    u, v = [a for a in range(3) if a != axis]
    gu = (lo[u] + (hi[u] - lo[u]) * (np.arange(g + 1) / g)).astype(F)
    gv = (lo[v] + (hi[v] - lo[v]) * (np.arange(g + 1) / g)).astype(F)
    k = np.arange(n)
    cell, upper = k // 2, k % 2 == 1
    iu, iv = cell % g, cell // g
    pos = np.empty((n, 3, 3), F)
    pos[..., axis] = F(0.5) * (lo[axis] + hi[axis])
    # lower triangle (u0 v0, u1 v0, u0 v1), upper triangle (u1 v1, u0 v1, u1 v0): they share the diagonal only
    pos[:, 0, u] = np.where(upper, gu[iu + 1], gu[iu]); pos[:, 0, v] = np.where(upper, gv[iv + 1], gv[iv])
    pos[:, 1, u] = np.where(upper, gu[iu], gu[iu + 1]); pos[:, 1, v] = np.where(upper, gv[iv + 1], gv[iv])
    pos[:, 2, u] = np.where(upper, gu[iu + 1], gu[iu]); pos[:, 2, v] = np.where(upper, gv[iv], gv[iv + 1])
    return _finish(pos, base, seed)


def sheet_z(base, seed):
    """A grid of non-overlapping triangles on the plane z = the box's middle: the centroid extent on z is
    exactly 0 (k_morton's 0.5 branch), and every box has zero thickness."""
    return _sheet(base, seed, 2)


def sheet_x(base, seed):
    """As sheet_z on a plane x = const (the most significant Morton axis is the dead one)."""
    return _sheet(base, seed, 0)


def line(base, seed):
    """A row of small triangles along x whose boxes share their y and z intervals exactly: two centroid
    extents are 0, the codes differ in every third bit only."""
    lo, hi = _box(base)
    n = np.asarray(base).shape[0]
    xs = (lo[0] + (hi[0] - lo[0]) * (np.arange(n + 1) / n)).astype(F)
    y0, y1 = _at(lo, hi, 0, 0.25, 0)[1], _at(lo, hi, 0, 0.75, 0)[1]
    z0, z1 = _at(lo, hi, 0, 0, 0.47)[2], _at(lo, hi, 0, 0, 0.53)[2]
    pos = np.empty((n, 3, 3), F)
    pos[:, 0] = np.stack([xs[:-1], np.full(n, y0, F), np.full(n, z0, F)], 1)
    pos[:, 1] = np.stack([xs[1:], np.full(n, y1, F), np.full(n, z0, F)], 1)
    pos[:, 2] = np.stack([xs[:-1], np.full(n, y0, F), np.full(n, z1, F)], 1)
    return _finish(pos, base, seed)


def degenerate_mix(base, seed):
    """The base geometry with every third triangle collapsed to a point and every fifth (of the rest) to a
    segment: zero-area triangles and zero-area boxes among the entries the collapse ranks by area."""
    pos = np.asarray(base, F).copy()
    k = np.arange(pos.shape[0])
    point, seg = k % 3 == 0, (k % 3 != 0) & (k % 5 == 0)
    pos[point, 1] = pos[point, 0]
    pos[point, 2] = pos[point, 0]
    pos[seg, 2] = pos[seg, 1]
    return _finish(pos, base, seed, shuffle=False)


def degenerate_counts(n):
    """(points, segments) degenerate_mix makes of n triangles."""
    k = np.arange(n)
    return int((k % 3 == 0).sum()), int(((k % 3 != 0) & (k % 5 == 0)).sum())


def two_scales(base, seed):
    """The first half is the base geometry; the second half is the base scaled by 2^-10 about the box's
    lower corner, so hundreds of triangles share one Morton cell; triangle 0 spans the whole box."""
    lo, hi = _box(base)
    pos = np.asarray(base, F).copy()
    h = pos.shape[0] // 2
    pos[h:] = lo + (pos[h:] - lo) * F(2.0 ** -10)
    # (a tilted plane that holds no camera of poses(): a ray inside a triangle's plane divides by n.d, the
    # rounding residue of a zero, and the t that comes out lies in no box: brute force and any tree differ there)
    pos[0] = np.stack([_at(lo, hi, 0.0, 0.0, 0.25), _at(lo, hi, 1.0, 1.0, 0.0), _at(lo, hi, 0.3, 0.5, 1.0)])
    pos[0, 0, :2], pos[0, 1, :], pos[0, 2, 2] = lo[:2], [hi[0], hi[1], lo[2]], hi[2]
    return _finish(pos, base, seed, shuffle=False)


def comb(base, seed):
    """Triangle k is a small triangle at x = x_min + extent * 2^-(k mod 24): each next tooth halves the
    distance to the box's face, which gives a deep, one-sided Morton hierarchy; the teeth past 2^-10 share
    the first cell."""
    lo, hi = _box(base)
    n = np.asarray(base).shape[0]
    ext = hi - lo
    k = np.arange(n)
    x = (lo[0] + ext[0] * np.exp2(-(k % 24).astype(np.float64))).astype(F)
    row = k // 24
    rows = max(1, (n + 23) // 24)
    side = int(np.ceil(np.sqrt(rows)))
    fy = (row % side + 0.1) / side
    fz = (row // side + 0.1) / side
    y0 = (lo[1] + ext[1] * fy).astype(F)
    z0 = (lo[2] + ext[2] * fz).astype(F)
    sy, sz, sx = F(ext[1] * 0.8 / side), F(ext[2] * 0.8 / side), F(ext[0] / 16)
    pos = np.empty((n, 3, 3), F)
    pos[:, 0] = np.stack([x, y0, z0], 1)
    pos[:, 1] = np.stack([x, y0 + sy, z0 + sz], 1)
    pos[:, 2] = np.stack([x - sx, y0, z0 + sz], 1)
    return _finish(pos, base, seed, shuffle=False)


CASES = {f.__name__: f for f in (identical, pairs, sheet_z, sheet_x, line, degenerate_mix, two_scales, comb)}


# ---------------------------------------------------------------------------------------------
# Camera poses and their primary rays
# ---------------------------------------------------------------------------------------------
def poses(fovrt, scene, bbox, W, H):
    """Three cameras: the scene's preset pose, a pose from the opposite side of the bounding box (the preset
    eye mirrored through the box's vertical axis, looking at the box's middle), and a pose from above,
    looking down at the middle."""
    bbox = np.asarray(bbox, F)
    mid = F(0.5) * (bbox[:3] + bbox[3:])
    a = fovrt.Camera.preset(scene, W, H)
    b = fovrt.Camera.preset(scene, W, H)
    b.setPosition(np.array([2 * mid[0] - a.pos[0], a.pos[1], 2 * mid[2] - a.pos[2]], F))
    b.lookAt(mid)
    c = fovrt.Camera.preset(scene, W, H)
    c.setPosition(np.array([mid[0] + F(0.25), bbox[4] + F(7.0), mid[2] + F(0.5)], F))
    c.lookAt(mid, up=(0.0, 0.0, -1.0))
    return {"preset": a, "opposite": b, "above": c}


def primary_rays(uni, W, H, tmin=1e-3):
    """The pixel-centre-less primary rays of entry 0 (direction through inv_vp * (ndc, -1, 1)), numpy float32:
    rows (origin, direction, tmin, tmax) as OracleScene.closest takes them."""
    m = np.array(uni.inv_vp[:], F).reshape(4, 4)
    eye = np.array(uni.eye[:], F)
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    ndc = np.stack([x / F(W) * F(2) - F(1), y / F(H) * F(2) - F(1), np.full_like(x, -1), np.ones_like(x)], -1)
    p = ndc.reshape(-1, 4) @ m.T
    d = p[:, :3] / p[:, 3:] - eye
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    n = d.shape[0]
    return np.concatenate([np.broadcast_to(eye, (n, 3)), d, np.full((n, 1), tmin, F), np.full((n, 1), np.inf, F)],
                          1).astype(F)
