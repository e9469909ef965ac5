"""The smooth-vertex weld and the normal rule of fr_update_geometry (include/fovrt.h), restated in numpy float32.

weld_np: corners 3 t + k of triangles with normals are one vertex when their rest positions and rest normals are
equal, all six floats by bits after adding +0.0f; ids in order of first corner; -1 without normals.
recompute_np: per vertex, the crosses of its corners' triangles summed sequentially in ascending corner order,
every operation rounded to float32 on its own (numpy never fuses); then the two fallbacks.
"""
import numpy as np

F = np.float32
HAS_NORMALS = 0x100
FLT_MIN = np.finfo(F).tiny


def mirrored_pairs(base, seed=0):
    """Triangle 2k+1 is triangle 2k of the base geometry with its last two vertices exchanged: its cross is the
    exact negative (x - y == -(y - x) in floating point). A vertex whose corners lie in such pairs sums to exactly
    zero over triangles that can be normalised: the rule's first fallback, which bvh_cases' geometry (same-way
    copies, collapsed triangles) never reaches."""
    pos = np.asarray(base, F).copy()
    m = pos.shape[0] // 2
    pos[1:2 * m:2] = pos[0:2 * m:2][:, [0, 2, 1]]
    return np.ascontiguousarray(pos)


def weld_np(pos, nrm, flags):
    """(corner_vertex int32[3 n], nverts) of a scene's rest pose."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    nrm = np.asarray(nrm, F).reshape(-1, 3)
    has = np.repeat((np.asarray(flags) & HAS_NORMALS) != 0, 3)
    key = np.ascontiguousarray(np.concatenate([pos, nrm], 1) + F(0.0)).view(np.uint32)
    cv = np.full(pos.shape[0], -1, np.int32)
    if has.any():
        _, first, inv = np.unique(key[has], axis=0, return_index=True, return_inverse=True)
        ids = np.empty(first.size, np.int32)
        ids[np.argsort(first, kind="stable")] = np.arange(first.size, dtype=np.int32)
        cv[has] = ids[np.asarray(inv).reshape(-1)]
        return cv, int(first.size)
    return cv, 0


def cross_np(a, b):
    """fr_math.h's cross, unfused."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


def dot_np(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def _normalised(v):
    """(v * (1 / sqrt(dot(v, v))), ok) with ok where FLT_MIN <= dot < inf."""
    d = dot_np(v, v)
    ok = (d >= FLT_MIN) & (d < np.inf)
    inv = F(1.0) / np.sqrt(np.where(ok, d, F(1.0)), dtype=F)
    return (v * inv[..., None]).astype(F), ok


def recompute_np(pos, corner_vertex, nverts, current):
    """The normals (n x 3 x 3 float32) the rule gives over pos, starting from `current` (kept on corners without
    a vertex and where both fallbacks fail), and the number of corners that took (vertex normal, own triangle's
    normal, kept theirs)."""
    pos = np.asarray(pos, F).reshape(-1, 3, 3)
    cv = np.asarray(corner_vertex, np.int32)
    out = np.array(current, F).reshape(-1, 3).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        face = cross_np(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0])
        corners = np.flatnonzero(cv >= 0)
        order = corners[np.argsort(cv[corners], kind="stable")]  # by vertex, ascending corner inside a vertex
        v_of = cv[order]
        start = np.searchsorted(v_of, np.arange(nverts))
        valence = np.diff(np.append(start, order.size))
        acc = np.zeros((nverts, 3), F)
        for j in range(int(valence.max()) if nverts else 0):
            live = np.flatnonzero(valence > j)
            acc[live] = acc[live] + face[order[start[live] + j] // 3]
        vn, vok = _normalised(acc)
        fn, fok = _normalised(face)
    own = fok[corners // 3]
    smooth = vok[cv[corners]]
    first = ~smooth & own
    out[corners[smooth]] = vn[cv[corners[smooth]]]
    out[corners[first]] = fn[corners[first] // 3]
    return out.reshape(-1, 3, 3), (int(smooth.sum()), int(first.sum()), int((~smooth & ~own).sum()))
