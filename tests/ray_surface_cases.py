"""Cases and references for the second part of the ray queries (FR_RAYS_SURFACE and per-ray model masks), pure numpy,
shared by tests/test_cpu_ray_surface.py, which asserts their preconditions on the references alone, and
tests/test_gpu_ray_surface.py. Rows, scenes and hit records are tests/ray_cases.py's.

surface_np builds the 80-byte fr_ray_surface records from the numpy restatement of the closest-hit programs
(trace_np.SceneNp.attributes / kd, pinned to the oracle's G-buffer). The masked references answer a ray over the
scene with every triangle of an excluded model collapsed onto its first vertex: the triangle keeps its index and fails
intersect_triangle on every ray (its normal is 0, so 1 / n.d is infinite and no comparison of the test holds)."""
import numpy as np

import ray_cases as rc
import trace_np as tn

F = np.float32
SURFACE_DTYPE = np.dtype([("t", F), ("beta", F), ("gamma", F), ("prim", np.int32),
                          ("point", F, 3), ("model", np.int32), ("ng", F, 3), ("u", F),
                          ("ns", F, 3), ("v", F), ("kd", F, 3), ("surface", np.int32)])
OFFSETS = {"t": 0, "beta": 4, "gamma": 8, "prim": 12, "point": 16, "model": 28, "ng": 32, "u": 44, "ns": 48, "v": 60,
           "kd": 64, "surface": 76}

_MODELS = {}


def models(fovrt, scene):
    """[(name, first_tri, ntris)] of a procedural scene (no device)."""
    if scene not in _MODELS:
        _MODELS[scene] = fovrt.Scene(rc.config(fovrt, scene)).models()
    return _MODELS[scene]


def model_of(ms, prim):
    first = np.array([m[1] for m in ms], np.int64)
    p = np.asarray(prim).astype(np.int64)
    return np.where(p < 0, -1, np.searchsorted(first, p, side="right") - 1).astype(np.int32)


def miss_surface():
    r = np.zeros(1, SURFACE_DTYPE)[0]
    r["t"], r["prim"], r["model"] = np.inf, -1, -1
    return r


def surface_np(nsc, r, hits, ms):
    """The fr_ray_surface record of each row (o, d, tmin, tmax) whose closest hit is hits[i] (fr_ray_hit records)."""
    out = np.zeros(len(r), SURFACE_DTYPE)
    out[:] = miss_surface()
    model = model_of(ms, hits["prim"])
    for i, (q, h) in enumerate(zip(np.asarray(r, F), hits)):
        k = int(h["prim"])
        if k < 0:
            continue
        o, d = tuple(q[0:3]), tuple(q[3:6])
        a = nsc.attributes(k, h["t"], h["beta"], h["gamma"], o, d)
        ng = tn.normalize(a["geo"])             # the attribute, normalised a second time
        ns = tn.normalize(a["shading"])         # (without normals the attribute is geo: ns == ng)
        fl = int(nsc.flags[k])
        mtype, _tex = nsc.material(k)
        back = 1 if tn.dot(d, a["geo"]) > 0 else 0
        rec = out[i]
        rec["t"], rec["beta"], rec["gamma"], rec["prim"] = h["t"], h["beta"], h["gamma"], k
        rec["point"], rec["model"] = a["front"], model[i]
        rec["ng"], rec["u"] = ng, a["uv"][0]
        rec["ns"], rec["v"] = ns, a["uv"][1]
        rec["kd"] = nsc.kd(k, a["uv"])
        rec["surface"] = (fl & 0xFF) | mtype << 8 | (fl & 0x300) << 8 | back << 18
    return out


def surface_type(word):
    return (np.asarray(word) >> 8) & 0xFF


def class_of_type(rec):
    """GCLASS of each record: refraction 0, reflection 1, diffuse 2, miss 3."""
    cls = np.array([2, 1, 0], np.uint8)[np.clip(surface_type(rec["surface"]), 0, 2)]
    return np.where(rec["prim"] < 0, np.uint8(3), cls).astype(np.uint8)


def selected(ms, mask):
    """Per triangle: does `mask` select its model? Bits at or above the model count are ignored."""
    nt = ms[-1][1] + ms[-1][2]
    sel = np.zeros(nt, bool)
    for i, (_n, first, cnt) in enumerate(ms):
        if (int(mask) >> i) & 1:
            sel[first:first + cnt] = True
    return sel


def collapsed(arrays, ms, mask):
    """The scene arrays with every triangle of a model `mask` excludes collapsed onto its first vertex."""
    b = dict(arrays)
    P = np.asarray(arrays["pos"], F).reshape(-1, 3, 3).copy()
    out = ~selected(ms, mask)
    P[out, 1] = P[out, 0]
    P[out, 2] = P[out, 0]
    b["pos"] = P.reshape(np.asarray(arrays["pos"]).shape)
    return b


def _valid(ms, masks):
    return np.asarray(masks, np.uint32) & np.uint32((1 << len(ms)) - 1)


def masked_reference(oracle, arrays, ms, r, masks, brute=True):
    """fr_ray_hit records: each group of rays with one mask value answered by the oracle over collapsed(...)."""
    r = np.asarray(r, F)
    out = np.empty(len(r), rc.HIT_DTYPE)
    out[:] = rc.MISS
    valid = _valid(ms, masks)
    for m in np.unique(valid):
        if m == 0:
            continue
        sel = valid == m
        out[sel] = rc.hit_records(oracle.OracleScene(collapsed(arrays, ms, m)).closest(r[sel], brute=brute))
    return out


def masked_np(arrays, ms, r, masks, what="closest"):
    """The numpy restatement over the collapsed arrays: fr_ray_hit records, or transmittance (what="shadow")."""
    r = np.asarray(r, F)
    valid = _valid(ms, masks)
    out = np.empty(len(r), rc.HIT_DTYPE) if what == "closest" else np.ones(len(r), F)
    if what == "closest":
        out[:] = rc.MISS
    for m in np.unique(valid):
        if m == 0:
            continue
        sel = valid == m
        nsc = tn.SceneNp(collapsed(arrays, ms, m))
        out[sel] = rc.closest_np(nsc, r[sel]) if what == "closest" else rc.shadow_np(nsc, r[sel])
    return out


def aimed_rows(arrays, ms, seed=31, per=150):
    """(rows, masks): per model, `per` random triangles with one interior point each, origins uniform in the scene box
    lifted above the ground (y = |y| + 0.05), aimed at the point with direction lengths log-uniform in 0.1 .. 10, and
    a uniform random mask per ray over the scene's models."""
    rng = np.random.default_rng(seed)
    b = np.asarray(arrays["bbox"], np.float64)
    out = []
    for _name, first, cnt in ms:
        tris = rng.integers(first, first + cnt, per)
        p = rc._points_on(arrays, tris, rng)
        o = rng.uniform(b[0:3], b[3:6], (per, 3))
        o[:, 1] = np.abs(o[:, 1]) + 0.05
        d = p - o
        d *= (10.0 ** rng.uniform(-1, 1, per) / np.linalg.norm(d, axis=1))[:, None]
        out.append(rc.rows(o, d))
    r = np.concatenate(out)
    masks = rng.integers(0, 1 << len(ms), len(r)).astype(np.uint32)
    return r, masks


def aimed_counts(ms, plain, masked, masks):
    """(see-through answers, per model of the revealed hit, misses under a non-zero mask, zero masks): a see-through
    answer is a hit in a selected model where the unmasked hit lies in an excluded one."""
    valid = _valid(ms, masks)
    pm, mm = model_of(ms, plain["prim"]), model_of(ms, masked["prim"])
    through = (masked["prim"] >= 0) & (plain["prim"] >= 0) & (pm != mm)
    per_model = [int((through & (mm == i)).sum()) for i in range(len(ms))]
    lost = (valid != 0) & (masked["prim"] < 0) & (plain["prim"] >= 0)
    return int(through.sum()), per_model, int(lost.sum()), int((valid == 0).sum())


def crossings(nsc, row):
    """The material types of the triangles a row (o, d, tmin, tmax) crosses inside its window."""
    hit, _t, _b, _g = nsc._tests(row[0:3], row[3:6], row[6], row[7])
    return [nsc.material(int(k))[0] for k in np.nonzero(hit)[0]]


# Scenes whose triangles lack normals or uv. The procedural scenes give every triangle both (flags & 0x300 == 0x300);
# an OBJ box with vn lines and no vt gives 0x100, one without vn lines gives 0, beside an OBJ ground with both.
BOX_WITHOUT_NORMALS = "v 0 0 0\nv 100 0 0\nv 0 100 0\nv 0 0 100\nf 1 3 2\nf 1 2 4\nf 1 4 3\nf 2 3 4\n"
OBJ_SCENES = {"normals": 0x100, "bare": 0}   # name -> flags & 0x300 of the box's four triangles
OBJ_EYE, OBJ_TARGET = (-1.6, 1.4, 3.4), (-3.2, 0.45, 1.5)


def obj_scene_config(fovrt, directory, name, W=rc.SIZE[0], H=rc.SIZE[1]):
    """Writes the OBJ files of scene `name` under `directory` and returns the Config that loads them (scene 0: the
    ground and the box, mesh_mode 2: the files are required)."""
    import os
    from test_cpu_abi import GROUND_OBJ, TETRA_OBJ
    d = os.path.join(str(directory), name)
    os.makedirs(os.path.join(d, "box"), exist_ok=True)
    with open(os.path.join(d, "ground.obj"), "w") as fh:
        fh.write(GROUND_OBJ)
    with open(os.path.join(d, "box", "box.obj"), "w") as fh:
        fh.write(TETRA_OBJ if name == "normals" else BOX_WITHOUT_NORMALS)
    return fovrt.Config(width=W, height=H, scene=0, texture_mode=1, mesh_mode=2, asset_dir=d)


def obj_camera(fovrt, W=rc.SIZE[0], H=rc.SIZE[1]):
    """A camera on the OBJ box (trace_cases.camera's projection)."""
    cam = fovrt.Camera()
    cam.setRotation((1, 0, 0, 0))
    cam.setPosition(OBJ_EYE)
    cam.lookAt(OBJ_TARGET, (0.0, 1.0, 0.0))
    cam.setProjectMode(fovrt.Camera.PM_Perspective, 45, 0.1, 500.1)
    cam.setScreen((W, H))
    cam.setViewport((0, 0, W, H))
    return cam


def obj_rows(fovrt, arrays, seed=47, per=10):
    """Camera rays on the box, and rays at `per` interior points of every triangle from both of its sides, with
    directions of lengths 0.2 to 5."""
    import trace_cases as tc
    W, H = rc.SIZE
    eye, d = tc.camera_rays_np(obj_camera(fovrt).uniforms(W, H), W, H)
    rng = np.random.default_rng(seed)
    nt = len(arrays["flags"])
    tris = np.repeat(np.arange(nt), per)
    p = rc._points_on(arrays, tris, rng)
    P = np.asarray(arrays["pos"], np.float64).reshape(-1, 3, 3)[tris]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    n /= np.linalg.norm(n, axis=1)[:, None]
    o = p + n * rng.choice([-0.4, 0.4], len(p))[:, None] + rng.normal(size=p.shape) * 0.05
    dirs = (p - o) * rng.uniform(0.5, 12.0, (len(p), 1))
    return np.concatenate([tc.closest_rays(eye, d), rc.rows(o, dirs)])


def shadow_masks(ms, n):
    """Masks for ray_cases.shadow_rows: every model for the even rays, every model but the refractive box for the odd
    ones."""
    names = [m[0] for m in ms]
    every = (1 << len(ms)) - 1
    masks = np.full(n, every, np.uint32)
    masks[1::2] = every & ~(1 << names.index("box"))
    return masks
