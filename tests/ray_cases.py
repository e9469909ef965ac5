"""Ray sets for the ray-query tests (pure numpy, no GPU), shared by tests/test_cpu_ray_queries.py, which asserts each
set's preconditions on the references alone, and tests/test_gpu_ray_queries.py.

A set is an (n, 8) float32 array of rows (o, d, tmin, tmax), the layout OracleScene.closest takes; fr_rays() turns it
into the ABI's fr_ray layout (origin, tmin, dir, tmax) and hit_records() turns the oracle's answers (t, prim, beta,
gamma) into fr_ray_hit records. Scenes are the procedural ones (texture_mode 1, mesh_mode 1, detail 1): 14 triangles
in the box scene, 9,106 in the bunny scene."""
import numpy as np

import trace_cases as tc
from helpers import ASSET_DIR

F = np.float32
SIZE = (33, 17)                          # the camera sets' screen
BATCH_SIZES = [1, 63, 64, 65, 64 * 7 + 5]
QUERY_VIEWS = [n for n in tc.VIEW_NAMES if tc.VIEWS[n][0] in (0, 1)]
HIT_DTYPE = np.dtype([("t", F), ("beta", F), ("gamma", F), ("prim", np.int32)])
MISS = np.array([(np.inf, 0.0, 0.0, -1)], HIT_DTYPE)[0]

_SCENES = {}


def config(fovrt, scene, W=SIZE[0], H=SIZE[1], builder=0, **kw):
    return fovrt.Config(width=W, height=H, scene=scene, texture_mode=1, mesh_mode=1, detail=1, bvh_builder=builder,
                        asset_dir=ASSET_DIR, **kw)


def scene_arrays(fovrt, scene):
    """The scene's arrays, loaded once per session (no device)."""
    if scene not in _SCENES:
        _SCENES[scene] = fovrt.Scene(config(fovrt, scene)).arrays()
    return _SCENES[scene]


def rows(o, d, tmin=1e-3, tmax=np.inf):
    o, d = np.atleast_2d(np.asarray(o, F)), np.atleast_2d(np.asarray(d, F))
    n = max(len(o), len(d))
    r = np.empty((n, 8), F)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, tmin, tmax
    return r


def fr_rays(r):
    """Rows (o, d, tmin, tmax) -> fr_ray rows (origin, tmin, dir, tmax)."""
    r = np.asarray(r, F).reshape(-1, 8)
    return np.ascontiguousarray(r[:, [0, 1, 2, 6, 3, 4, 5, 7]])


def hit_records(out):
    """OracleScene.closest's rows (t, prim, beta, gamma) -> fr_ray_hit records; the oracle's miss (prim < 0) becomes
    the ABI's (inf, 0, 0, -1)."""
    out = np.asarray(out, F).reshape(-1, 4)
    h = np.empty(len(out), HIT_DTYPE)
    h["t"], h["beta"], h["gamma"], h["prim"] = out[:, 0], out[:, 2], out[:, 3], out[:, 1].astype(np.int32)
    h[out[:, 1] < 0] = MISS
    return h


def closest_np(sc, r):
    """SceneNp.closest on every row, as fr_ray_hit records."""
    h = np.empty(len(r), HIT_DTYPE)
    for i, q in enumerate(np.asarray(r, F)):
        c = sc.closest(q[0:3], q[3:6], q[6], q[7])
        h[i] = MISS if c is None else (c[1], c[2], c[3], c[0])
    return h


def same_records(a, b):
    return a.tobytes() == b.tobytes()


def domain(bbox):
    """The guaranteed domain of origins: the scene box grown on each side by its longest edge."""
    b = np.asarray(bbox, np.float64)
    L = float((b[3:6] - b[0:3]).max())
    return b[0:3] - L, b[3:6] + L, L


def camera_rows(fovrt, name):
    W, H = SIZE
    uni = tc.camera(fovrt, name, W, H).uniforms(W, H)
    eye, d = tc.camera_rays_np(uni, W, H)
    return tc.closest_rays(eye, d)


def _points_on(a, tris, rng):
    """One random interior point of each listed triangle (float64)."""
    P = np.asarray(a["pos"], np.float64).reshape(-1, 3, 3)[tris]
    w = rng.dirichlet((2.0, 2.0, 2.0), len(tris))
    return np.einsum("nk,nkc->nc", w, P)


def random_rows(a, n=600, seed=11):
    """Random origins in the guaranteed domain with random unnormalised directions (lengths 1e-3 .. 1e3, log-uniform).
    Three in five are aimed at a random point of the scene box, so that both answers are well represented."""
    rng = np.random.default_rng(seed)
    lo, hi, _L = domain(a["bbox"])
    b = np.asarray(a["bbox"], np.float64)
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    aimed = rng.random(n) < 0.6
    d[aimed] = (rng.uniform(b[0:3], b[3:6], (n, 3)) - o)[aimed]
    d *= (10.0 ** rng.uniform(-3, 3, n) / np.linalg.norm(d, axis=1))[:, None]
    d = d.astype(F)
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    d[ln < 1e-3] *= F(1.01)
    d[ln > 1e3] *= F(0.99)
    return rows(o, d, 1e-3, np.inf)


def zero_rows(a, seed=5, per=16):
    """Rays with one and with two components of +-0 (both signs of zero), aimed at points of the scene's triangles
    from inside the guaranteed domain."""
    rng = np.random.default_rng(seed)
    nt = len(a["flags"])
    _lo, _hi, L = domain(a["bbox"])
    out = []
    for axis in range(3):
        for zero in (0.0, -0.0):
            tris = rng.integers(0, nt, per)
            p = _points_on(a, tris, rng)
            # one zero component: the ray runs in a plane of constant coordinate `axis`
            d = rng.normal(size=(per, 3)) * rng.uniform(0.05, 3.0, (per, 1))
            d[:, axis] = zero
            tau = 0.5 * L / np.linalg.norm(d, axis=1) * rng.uniform(0.2, 1.0, per)
            out.append(rows(p - d * tau[:, None], d))
            # two zero components: the ray runs along `axis`
            d2 = np.zeros((per, 3))
            d2[:, (axis + 1) % 3] = zero
            d2[:, (axis + 2) % 3] = -zero
            d2[:, axis] = rng.choice([-1.0, 1.0], per) * rng.uniform(0.05, 3.0, per)
            tau = 0.5 * L / np.abs(d2[:, axis]) * rng.uniform(0.2, 1.0, per)
            out.append(rows(p - d2 * tau[:, None], d2))
    return np.concatenate(out)


def edge_vertex_rows(a, seed=3):
    """Rays aimed at every vertex and every edge midpoint of the scene's triangles (the box scene: shared by two to
    six triangles), from four origins each."""
    rng = np.random.default_rng(seed)
    P = np.asarray(a["pos"], F).reshape(-1, 3, 3)
    targets = np.concatenate([P.reshape(-1, 3), ((P + np.roll(P, 1, axis=1)) * F(0.5)).reshape(-1, 3)])
    targets = np.unique(targets, axis=0)
    b = np.asarray(a["bbox"], np.float64)
    centre = 0.5 * (b[0:3] + b[3:6])
    out = []
    for k in range(4):
        o = (centre + rng.uniform(-1.0, 1.0, 3) * (b[3:6] - b[0:3]) * 0.6 + np.array([0.0, 2.0 + k, 0.0])).astype(F)
        out.append(rows(o, (targets - o).astype(F)))
    return np.concatenate(out)


TIE_PAIRS = [(11, 2), (12, 5), (13, 8)]  # (moved triangle, the triangle it is moved onto), box scene


def tie_positions(a):
    """The box scene's positions (ntris, 3, 3) with three triangles moved onto three others: a device update cannot
    change the triangle count, so the coincident pairs are made by moving existing triangles."""
    P = np.asarray(a["pos"], F).reshape(-1, 3, 3).copy()
    for dst, src in TIE_PAIRS:
        P[dst] = P[src]
    return P


def tie_arrays(a):
    b = dict(a)
    b["pos"] = tie_positions(a).reshape(np.asarray(a["pos"]).shape)
    return b


def tie_rows(a, seed=9, per=30):
    """Rays at interior points of the coincident pairs, from a third of a unit off the face on either side."""
    rng = np.random.default_rng(seed)
    P = tie_positions(a).astype(np.float64)
    out = []
    for _dst, src in TIE_PAIRS:
        p = _points_on({"pos": P}, np.full(per, src), rng)
        n = np.cross(P[src, 1] - P[src, 0], P[src, 2] - P[src, 0])
        n /= np.linalg.norm(n)
        o = p + n * (rng.choice([-0.3, 0.3], per))[:, None] + rng.normal(size=(per, 3)) * 0.05
        out.append(rows(o, (p - o) * rng.uniform(0.5, 4.0, (per, 1))))
    return np.concatenate(out)


def window_rows(r, hits):
    """For each hit ray of a base set, three copies: tmax = t (loses that hit), tmin = t (likewise) and
    tmax = nextafter(t, inf) (keeps it). Returns (rows, kind (0, 1, 2), the base hit of each row)."""
    sel = hits["prim"] >= 0
    base, t = np.asarray(r, F)[sel], hits["t"][sel]
    a, b, c = base.copy(), base.copy(), base.copy()
    a[:, 7] = t
    b[:, 6] = t
    c[:, 7] = np.nextafter(t, F(np.inf))
    n = len(base)
    return np.concatenate([a, b, c]), np.repeat([0, 1, 2], n), np.concatenate([hits[sel]] * 3)


def degenerate_rows(a):
    """A NaN in each of the eight floats, an infinite origin or direction component of either sign, the direction
    (0, 0, 0) with every sign pattern of a zero, and empty windows (tmin == tmax, tmin > tmax, both infinite)."""
    b = np.asarray(a["bbox"], np.float64)
    o = 0.5 * (b[0:3] + b[3:6]) + np.array([0.0, 1.0, 0.0])
    good = rows(o, np.array([0.1, -1.0, 0.2]), 1e-3, np.inf)[0]  # a ray that hits the ground
    out = []
    for k in range(8):
        q = good.copy(); q[k] = np.nan; out.append(q)
    for k in range(6):
        for s in (np.inf, -np.inf):
            q = good.copy(); q[k] = s; out.append(q)
    for z in [(0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, -0.0, -0.0), (-0.0, -0.0, -0.0)]:
        q = good.copy(); q[3:6] = z; out.append(q)
    for tmin, tmax in [(1.0, 1.0), (2.0, 1.0), (np.inf, np.inf), (-np.inf, -np.inf), (0.5, -np.inf)]:
        q = good.copy(); q[6], q[7] = tmin, tmax; out.append(q)
    return np.array(out, F), good


def refill_rows(a, n=BATCH_SIZES[-1], seed=21):
    """The bunny scene's 64 * 7 + 5 batch: even rays leave the scene upwards (a miss at the root), odd rays are aimed
    through the bunny's triangles from beside it (deep traversals), so that answered lanes refill beside busy ones."""
    rng = np.random.default_rng(seed)
    b = np.asarray(a["bbox"], np.float64)
    nt = len(a["flags"])
    p = _points_on(a, rng.integers(nt // 4, nt, n), rng)
    o = p + rng.normal(size=(n, 3)) * 0.8 + np.array([0.0, 0.6, 0.0])
    d = (p - o) * rng.uniform(0.5, 2.0, (n, 1))
    up = np.arange(n) % 2 == 0
    o[up] = rng.uniform(b[0:3], b[3:6], (n, 3))[up] + np.array([0.0, b[4] - b[1] + 0.5, 0.0])
    d[up] = np.abs(rng.normal(size=(n, 3)))[up] * np.array([0.3, 1.0, 0.3])
    return rows(o, d)


def light_centre(a):
    L = np.asarray(a["light"], np.float64)
    return L[0:3] + 0.5 * L[3:6] + 0.5 * L[6:9]


def shadow_rows(a, n=300, seed=17):
    """Shadow rays as the engine casts them (unit direction, tmax = the distance to the light, tmin = 1e-3): from
    points a little above the ground's triangles 0 and 1 towards the light, two in three of them under the scene's
    other models (through the glass, or into an opaque model's shadow), and one in six from below the ground (opaque:
    exactly 0)."""
    rng = np.random.default_rng(seed)
    P = np.asarray(a["pos"], np.float64).reshape(-1, 3, 3)
    c = light_centre(a)
    ground_y = P[0:2, :, 1].max()
    others = P[2:].reshape(-1, 3)
    lo, hi = others.min(0), others.max(0)
    g = np.empty((n, 3))
    g[:, 1] = ground_y + 0.01
    under = rng.random(n) < 0.67
    # the foot of a ray that passes through a point q of the other models' box: q projected from the light
    q = rng.uniform(lo, hi, (n, 3))
    s = (g[:, 1] - c[1]) / (q[:, 1] - c[1])
    g[:, 0] = c[0] + (q[:, 0] - c[0]) * s
    g[:, 2] = c[2] + (q[:, 2] - c[2]) * s
    wide = rng.uniform(P[0:2].reshape(-1, 3).min(0), P[0:2].reshape(-1, 3).max(0), (n, 3)) * 0.5
    g[~under, 0], g[~under, 2] = wide[~under, 0], wide[~under, 2]
    below = rng.random(n) < 1.0 / 6.0
    g[below, 1] = ground_y - 0.5
    v = c - g
    dist = np.linalg.norm(v, axis=1)
    return rows(g, v / dist[:, None], 1e-3, dist.astype(F))


def shadow_np(sc, r):
    """SceneNp.shadow on every row (float32, shape (n,))."""
    out = np.empty(len(r), F)
    for i, q in enumerate(np.asarray(r, F)):
        out[i] = sc.shadow(tuple(q[0:3]), tuple(q[3:6]), q[6], q[7])[0]
    return out


def far_rows(a, n=400, seed=23):
    """Outside the guaranteed domain: origins 1e4 units out, aimed at points of the scene's triangles."""
    rng = np.random.default_rng(seed)
    p = _points_on(a, rng.integers(0, len(a["flags"]), n), rng)
    u = rng.normal(size=(n, 3))
    o = p + u / np.linalg.norm(u, axis=1)[:, None] * 1e4
    return rows(o, (p - o) / 1e4 * rng.uniform(0.5, 2.0, (n, 1)), 1e-3, np.inf)


def closest_sets(fovrt, scene):
    """name -> rows of every closest-hit base set of a scene (window copies are derived from their answers)."""
    a = scene_arrays(fovrt, scene)
    s = {f"view_{n}": camera_rows(fovrt, n) for n in QUERY_VIEWS if tc.VIEWS[n][0] == scene}
    s["random"] = random_rows(a)
    s["zeros"] = zero_rows(a)
    if scene == 0:
        s["edges"] = edge_vertex_rows(a)
    if scene == 1:
        s["refill"] = refill_rows(a)
    return s
