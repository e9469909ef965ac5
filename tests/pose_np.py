"""numpy restatement of the model-pose rule of include/fovrt.h (fr_set_model_transforms): float32, one rounded
operation at a time, no fma, with the identity bypass. Written from the header's text, not from the kernel.

    p'.c = ((M[c][0] p.x + M[c][1] p.y) + M[c][2] p.z) + M[c][3]
    K[r][c] = A[r1][c1] A[r2][c2] - A[r1][c2] A[r2][c1]      (r1, r2) = ((r + 1) % 3, (r + 2) % 3), (c1, c2) likewise
    n'.c = (K[c][0] n.x + K[c][1] n.y) + K[c][2] n.z
    det = (A[0][0] K[0][0] + A[0][1] K[0][1]) + A[0][2] K[0][2]
"""
import numpy as np

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
HAS_NORMALS = 0x100


def identities(n):
    return np.tile(IDENTITY, (n, 1)).reshape(n, 3, 4)


def matrices(m):
    m = np.ascontiguousarray(m, F)
    return m.reshape(m.shape[0], 3, 4)


def cofactors(M):
    """(K, det) of one 3 x 4 matrix: float32 scalars all the way (numpy rounds every scalar operation)."""
    A = np.asarray(M, F).reshape(3, 4)[:, :3]
    K = np.empty((3, 3), F)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
                K[r, c] = F(A[r1, c1] * A[r2, c2]) - F(A[r1, c2] * A[r2, c1])
        det = F(F(F(A[0, 0] * K[0, 0]) + F(A[0, 1] * K[0, 1])) + F(A[0, 2] * K[0, 2]))
    return K, det


def is_identity(M):
    return bool((np.asarray(M, F).reshape(12) == IDENTITY).all())  # ==: -0 counts as 0


def _rows(R, v, ncols):
    """out[..., c] = (R[c][0] v.x + R[c][1] v.y) + R[c][2] v.z (+ R[c][3]), every operation rounded to float32."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for c in range(3):
            s = ((R[c, 0] * x).astype(F) + (R[c, 1] * y).astype(F)).astype(F)
            s = (s + (R[c, 2] * z).astype(F)).astype(F)
            out[..., c] = (s + R[c, 3]).astype(F) if ncols == 4 else s
    return out


def pose_np(pos, nrm, models, m, flags=None):
    """(X, N): the rest arrays pos and nrm (ntris x 3 x 3 float32) posed by m (nmodels x 3 x 4). models: the model
    table, (name, first_tri, ntris) per model. flags (per triangle): triangles without normals keep theirs."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3, 3)
    nrm = np.ascontiguousarray(nrm, F).reshape(-1, 3, 3)
    m = matrices(m)
    assert len(models) == m.shape[0]
    X, N = pos.copy(), nrm.copy()
    for (_, first, nt), M in zip(models, m):
        if is_identity(M):
            continue  # rest bits: the arithmetic would turn a -0 into +0
        K, _ = cofactors(M)
        sl = slice(first, first + nt)
        X[sl] = _rows(M, pos[sl], 4)
        N[sl] = _rows(K, nrm[sl], 3)
    if flags is not None:
        keep = (np.asarray(flags) & HAS_NORMALS) == 0
        N[keep] = nrm[keep]
    return X, N


def rotation(axis, degrees):
    """A float32 rotation matrix (3 x 3) about a coordinate axis; 90 degrees gives exact zeros and ones."""
    q, r = divmod(degrees, 90)
    if r == 0:
        c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][int(q) % 4]
    else:
        c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R.astype(F)


def about(A, centre, t=(0, 0, 0)):
    """The 3 x 4 matrix of v -> A (v - centre) + centre + t, in float32 (any float32 matrix is a valid pose)."""
    A = np.asarray(A, np.float64)
    centre = np.asarray(centre, np.float64)
    M = np.empty((3, 4), F)
    M[:, :3] = A
    M[:, 3] = centre - A @ centre + np.asarray(t, np.float64)
    return M
