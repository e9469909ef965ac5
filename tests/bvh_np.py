"""A validator of the four-wide BVH in plain numpy, written from fr_device.h's description of BvhNode and
TriGeo and from what the traversal (k_trace.hip) assumes of a tree; it calls neither builder.

check_tree raises BvhError naming the first offending node, slot and value. What it checks:
  shape     prim is a permutation; every node below the reported count is reached from node 0 exactly once;
            at most one node per triangle
  slots     empty (count < 0): box +inf / -inf, child 0; inner (count == 0): a valid node index;
            leaf (count > 0): a range inside [0, n) of at most leaf_max triangles
  layout    the inner children of a node are base, base + 1, ... in slot order (one traversal stack entry
            covers them); its leaf ranges are back to back in slot order (the union-span leaf test); the
            leaf ranges of all nodes partition [0, n)
  boxes     every slot's box is inflate(min) / inflate(max) over the vertices below it, bit for bit
  leaves    tri_geo[j] is (p0, e0 = p1 - p0, e1 = p0 - p2, cross(e1, e0)) of pos[prim[j]], bit for bit
  numbers   the reported stack need (at most FR_BVH_STACK) and depth are the tree's own
"""
import numpy as np

F = np.float32
FR_BVH_STACK = 24

# struct BvhNode (fr_device.h): six f4 slabs (component k = child slot k), then child[4], count[4]; 128 bytes
NODE_DTYPE = np.dtype([("lox", F, 4), ("hix", F, 4), ("loy", F, 4), ("hiy", F, 4), ("loz", F, 4), ("hiz", F, 4),
                       ("child", np.int32, 4), ("count", np.int32, 4)])
assert NODE_DTYPE.itemsize == 128
TRI_FLOATS = 12  # struct TriGeo: p0.xyz e0.x | e0.yz e1.xy | e1.z n.xyz


class BvhError(AssertionError):
    pass


def _fail(msg):
    raise BvhError(msg)


def _first(bad):
    """Index tuple of the first True of a boolean array."""
    return tuple(int(v) for v in np.argwhere(bad)[0])


def inflate_lo(v):
    """scene.cpp inflate_lo: v - (1e-5f + 4e-7f * |v|), every operation rounded to fp32."""
    v = np.asarray(v, F)
    return v - (F(1e-5) + F(4e-7) * np.abs(v))


def inflate_hi(v):
    v = np.asarray(v, F)
    return v + (F(1e-5) + F(4e-7) * np.abs(v))


def tri_geo_of(tri):
    """TriGeo rows (m x 12) of triangles tri (m x 3 x 3), with the unfused cross product of fr_math.h."""
    tri = np.asarray(tri, F)
    p0, p1, p2 = tri[:, 0], tri[:, 1], tri[:, 2]
    e0, e1 = p1 - p0, p0 - p2
    a, b = e1, e0
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                  a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    return np.concatenate([p0, e0, e1, n], 1).astype(F)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_tree(nodes, tri_geo, prim, pos, reported_nodes, reported_max_stack, reported_depth, leaf_max=2):
    """nodes: NODE_DTYPE array (at least reported_nodes entries); tri_geo: n x 12 float32 in leaf order;
    prim: n int32, leaf order -> primitive; pos: n x 3 x 3 float32 in primitive order."""
    nodes = np.asarray(nodes)
    if nodes.dtype != NODE_DTYPE:
        _fail(f"nodes have dtype {nodes.dtype}, not BvhNode")
    pos = np.asarray(pos, F).reshape(-1, 3, 3)
    prim = np.asarray(prim).reshape(-1)
    tri_geo = np.asarray(tri_geo, F).reshape(-1, TRI_FLOATS)
    n, N = pos.shape[0], int(reported_nodes)
    if prim.shape[0] != n or tri_geo.shape[0] != n:
        _fail(f"{prim.shape[0]} leaf-order indices and {tri_geo.shape[0]} TriGeo for {n} triangles")
    if not 1 <= N <= n:
        _fail(f"reported node count {N} outside [1, {n}] (the arrays hold one node per triangle)")
    if nodes.shape[0] < N:
        _fail(f"{nodes.shape[0]} nodes read, {N} reported")
    nodes = nodes[:N]

    # --- prim is a permutation of 0 .. n-1
    seen = np.bincount(np.clip(prim, 0, n - 1), minlength=n)
    if ((prim < 0) | (prim >= n)).any():
        j = _first((prim < 0) | (prim >= n))[0]
        _fail(f"prim[{j}] = {int(prim[j])} outside [0, {n})")
    if (seen != 1).any():
        p = _first(seen != 1)[0]
        _fail(f"primitive {p} appears {int(seen[p])} times in prim (at {np.flatnonzero(prim == p)[:4].tolist()})")

    child, count = nodes["child"].astype(np.int64), nodes["count"].astype(np.int64)
    lo = np.stack([nodes["lox"], nodes["loy"], nodes["loz"]], -1)  # N x 4 x 3
    hi = np.stack([nodes["hix"], nodes["hiy"], nodes["hiz"]], -1)
    empty, inner, leaf = count < 0, count == 0, count > 0

    # --- slot kinds
    bad = empty & ((child != 0) | ~np.all(np.isposinf(lo), -1) | ~np.all(np.isneginf(hi), -1))
    if bad.any():
        i, k = _first(bad)
        _fail(f"node {i} slot {k}: empty slot with child {child[i, k]}, lo {lo[i, k]}, hi {hi[i, k]}")
    bad = inner & ((child < 0) | (child >= N))
    if bad.any():
        i, k = _first(bad)
        _fail(f"node {i} slot {k}: inner child {child[i, k]} outside [0, {N})")
    bad = leaf & ((child < 0) | (child + count > n))
    if bad.any():
        i, k = _first(bad)
        _fail(f"node {i} slot {k}: leaf range [{child[i, k]}, {child[i, k] + count[i, k]}) outside [0, {n})")
    bad = leaf & (count > leaf_max)
    if bad.any():
        i, k = _first(bad)
        _fail(f"node {i} slot {k}: leaf of {count[i, k]} triangles, more than {leaf_max}")

    # --- child layout within a node: inner children base, base + 1, ...; leaf ranges back to back
    nxt_inner = np.full(N, -1, np.int64)
    nxt_leaf = np.full(N, -1, np.int64)
    for k in range(4):
        c = child[:, k]
        bad = inner[:, k] & (nxt_inner >= 0) & (c != nxt_inner)
        if bad.any():
            i = _first(bad)[0]
            _fail(f"node {i} slot {k}: inner child {c[i]}, expected {nxt_inner[i]} (inner children {child[i][inner[i]].tolist()}"
                  f" are not consecutive in slot order)")
        nxt_inner = np.where(inner[:, k], c + 1, nxt_inner)
        bad = leaf[:, k] & (nxt_leaf >= 0) & (c != nxt_leaf)
        if bad.any():
            i = _first(bad)[0]
            _fail(f"node {i} slot {k}: leaf range starts at {c[i]}, expected {nxt_leaf[i]} (leaf ranges of a node are"
                  f" not back to back)")
        nxt_leaf = np.where(leaf[:, k], c + count[:, k], nxt_leaf)

    # --- a tree: every node below N reached from node 0 exactly once
    refs = np.bincount(child[inner], minlength=N)
    if refs[0] != 0:
        i, k = _first(inner & (child == 0))
        _fail(f"node {i} slot {k}: the root is an inner child")
    if (refs[1:] > 1).any():
        c = int(np.flatnonzero(refs[1:] > 1)[0]) + 1
        i, k = _first(inner & (child == c))
        _fail(f"node {i} slot {k}: node {c} is the child of {int(refs[c])} slots")
    if (refs[1:] == 0).any():
        c = int(np.flatnonzero(refs[1:] == 0)[0]) + 1
        _fail(f"node {c}: orphan, no slot points to it")
    ninner = inner.sum(1)
    pushes = (ninner > 1).astype(np.int64)  # a traversal step pushes one stack entry when it has > 1 inner child
    stack = np.full(N, -1, np.int64)
    level = np.full(N, -1, np.int64)
    stack[0], level[0] = pushes[0], 0
    levels = [np.array([0], np.int64)]
    while True:
        cur = levels[-1]
        m = inner[cur]
        kids = child[cur][m]
        if kids.size == 0:
            break
        par = np.repeat(cur, m.sum(1))
        stack[kids] = stack[par] + pushes[kids]
        level[kids] = level[par] + 1
        levels.append(kids)
        if len(levels) > N:
            _fail("the nodes reached from node 0 form a cycle")
    if (level < 0).any():  # (every node has one parent, so the rest are cycles off the root)
        _fail(f"node {_first(level < 0)[0]}: not reached from node 0")

    # --- the leaf ranges of all nodes partition [0, n)
    li, lk = np.nonzero(leaf)
    order = np.argsort(child[li, lk], kind="stable")
    li, lk = li[order], lk[order]
    start, end = child[li, lk], child[li, lk] + count[li, lk]
    if start.size == 0:
        _fail("the tree has no leaf")
    expect = np.concatenate([[0], end[:-1]])
    if (start != expect).any():
        j = _first(start != expect)[0]
        what = "overlaps the range before it" if start[j] < expect[j] else "leaves a gap"
        _fail(f"node {li[j]} slot {lk[j]}: leaf range [{start[j]}, {end[j]}) {what} (expected start {expect[j]})")
    if end[-1] != n:
        _fail(f"node {li[-1]} slot {lk[-1]}: the last leaf range ends at {end[-1]}, not at {n}")

    # --- boxes: bottom-up min / max over the vertices below each slot, then the inflation, bit for bit
    tmin, tmax = pos[prim].min(1), pos[prim].max(1)  # leaf order, n x 3
    raw_lo = np.full((N, 4, 3), np.inf, F)
    raw_hi = np.full((N, 4, 3), -np.inf, F)
    for j in range(int(count.max())):
        sel = leaf & (count > j)
        idx = (child + j)[sel]
        raw_lo[sel] = np.minimum(raw_lo[sel], tmin[idx])
        raw_hi[sel] = np.maximum(raw_hi[sel], tmax[idx])
    for cur in reversed(levels):
        m = inner[cur]
        kids = child[cur][m]
        if kids.size == 0:
            continue
        sub_lo, sub_hi = raw_lo[cur], raw_hi[cur]
        sub_lo[m] = raw_lo[kids].min(1)
        sub_hi[m] = raw_hi[kids].max(1)
        raw_lo[cur], raw_hi[cur] = sub_lo, sub_hi
    full = ~empty
    with np.errstate(invalid="ignore"):  # (inf - inf in the empty slots, which are not compared)
        want_lo, want_hi = inflate_lo(raw_lo), inflate_hi(raw_hi)
    for name, got, want, raw in (("lo", lo, want_lo, raw_lo), ("hi", hi, want_hi, raw_hi)):
        bad = full[..., None] & (_bits(got) != _bits(want))
        if bad.any():
            i, k, ax = _first(bad)
            _fail(f"node {i} slot {k}: box {name}.{'xyz'[ax]} = {float(got[i, k, ax])!r}, expected "
                  f"{float(want[i, k, ax])!r} = inflate({float(raw[i, k, ax])!r})")

    # --- leaf geometry
    want = tri_geo_of(pos[prim])
    bad = _bits(tri_geo) != _bits(want)
    if bad.any():
        j, q = _first(bad)
        _fail(f"tri_geo[{j}] (primitive {int(prim[j])}) float {q}: {float(tri_geo[j, q])!r}, expected {float(want[j, q])!r}")

    # --- the reported numbers
    if int(stack.max()) != int(reported_max_stack):
        _fail(f"node {int(stack.argmax())}: its path needs {int(stack.max())} stack entries, {reported_max_stack} reported")
    if int(reported_max_stack) > FR_BVH_STACK:
        _fail(f"stack need {reported_max_stack} exceeds FR_BVH_STACK = {FR_BVH_STACK}")
    if int(level.max()) != int(reported_depth):
        _fail(f"node {int(level.argmax())}: at level {int(level.max())}, depth {reported_depth} reported")
    return {"nodes": N, "max_stack": int(stack.max()), "depth": int(level.max()), "leaves": int(start.size)}


# ---------------------------------------------------------------------------------------------
# Reading a tree through the library's test hooks (fr__bvh_read, fr__scene_bvh: not in include/fovrt.h)
# ---------------------------------------------------------------------------------------------
def read_tree(fovrt, tracer):
    """The tree a PathTracer traverses, copied from the device: (nodes, tri_geo, prim)."""
    import ctypes as C
    lib = fovrt.load_library()
    fn = lib.fr__bvh_read
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    a = fovrt.fr_scene_arrays()
    tracer._check(lib.fr_scene_export(tracer._ctx, C.byref(a)))
    nodes = np.zeros(a.bvh_nodes, NODE_DTYPE)
    tri = np.zeros((a.num_tris, TRI_FLOATS), F)
    prim = np.full(a.num_tris, -1, np.int32)
    # one byte short of any array is refused
    assert fn(tracer._ctx, nodes.ctypes.data, nodes.nbytes - 1, tri.ctypes.data, tri.nbytes, prim.ctypes.data,
              prim.nbytes) == fovrt.FR_E_INVALID
    assert fn(tracer._ctx, nodes.ctypes.data, nodes.nbytes, tri.ctypes.data, tri.nbytes, prim.ctypes.data,
              prim.nbytes - 1) == fovrt.FR_E_INVALID
    tracer._check(fn(tracer._ctx, nodes.ctypes.data, nodes.nbytes, tri.ctypes.data, tri.nbytes, prim.ctypes.data,
                     prim.nbytes))
    return nodes, tri, prim


def scene_tree(fovrt, scene):
    """The host-built tree of a fovrt.Scene (copies): (nodes, tri_geo, prim)."""
    import ctypes as C
    lib = fovrt.load_library()
    fn = lib.fr__scene_bvh
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                   C.POINTER(C.c_int)]
    pn, pt, pp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nn, nt = C.c_int(), C.c_int()
    assert fn(scene._h, C.byref(pn), C.byref(nn), C.byref(pt), C.byref(pp), C.byref(nt)) == 0
    nodes = np.frombuffer(C.string_at(pn.value, nn.value * NODE_DTYPE.itemsize), NODE_DTYPE).copy()
    tri = np.frombuffer(C.string_at(pt.value, nt.value * TRI_FLOATS * 4), F).reshape(-1, TRI_FLOATS).copy()
    prim = np.frombuffer(C.string_at(pp.value, nt.value * 4), np.int32).copy()
    return nodes, tri, prim


def check_tracer_tree(fovrt, tracer, leaf_max=2):
    """check_tree on the tree a PathTracer traverses, against its own exported positions and numbers."""
    a = tracer.scene_arrays()
    nodes, tri, prim = read_tree(fovrt, tracer)
    return check_tree(nodes, tri, prim, a["pos"].reshape(-1, 3, 3), a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"],
                      leaf_max)
