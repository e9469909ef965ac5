"""numpy references for the BVH refit and the tree's SAH cost, written from fr_device.h's BvhNode / TriGeo and
bvh_np's restatement of the inflation and the leaf geometry; they call no library code.

refit_np     the one right answer of a refit, in bytes: topology (child, count, prim, node order) kept, every
             slot box = inflate(raw min / max over the vertices below the slot), raw boxes carried bottom-up
             (an inflated box is never inflated again), tri_geo recomputed from pos[prim]
sah_cost_np  1 + (sum over non-empty slots of area(stored box) * w) / area(union of node 0's slot boxes),
             w = 1 for an inner slot, the triangle count for a leaf slot; float64
"""
import numpy as np

import bvh_np

F = np.float32


def _levels(child, inner):
    """Node indices level by level from node 0."""
    levels = [np.array([0], np.int64)]
    while True:
        cur = levels[-1]
        kids = child[cur][inner[cur]]
        if kids.size == 0:
            return levels
        levels.append(kids)
        assert len(levels) <= child.shape[0], "cycle"


def refit_np(nodes, prim, pos):
    """(nodes, tri_geo) of the tree `nodes` / `prim` refitted over pos (n x 3 x 3, primitive order)."""
    nodes = np.array(nodes, copy=True)
    assert nodes.dtype == bvh_np.NODE_DTYPE
    pos = np.asarray(pos, F).reshape(-1, 3, 3)
    prim = np.asarray(prim).reshape(-1)
    N = nodes.shape[0]
    child, count = nodes["child"].astype(np.int64), nodes["count"].astype(np.int64)
    empty, inner, leaf = count < 0, count == 0, count > 0
    tmin, tmax = pos[prim].min(1), pos[prim].max(1)  # leaf order
    raw_lo = np.full((N, 4, 3), np.inf, F)
    raw_hi = np.full((N, 4, 3), -np.inf, F)
    for j in range(int(count.max())):
        sel = leaf & (count > j)
        idx = (child + j)[sel]
        raw_lo[sel] = np.minimum(raw_lo[sel], tmin[idx])
        raw_hi[sel] = np.maximum(raw_hi[sel], tmax[idx])
    for cur in reversed(_levels(child, inner)):
        m = inner[cur]
        kids = child[cur][m]
        if kids.size == 0:
            continue
        sub_lo, sub_hi = raw_lo[cur], raw_hi[cur]
        sub_lo[m] = raw_lo[kids].min(1)  # a child node's raw box: the union of its slots' raw boxes
        sub_hi[m] = raw_hi[kids].max(1)
        raw_lo[cur], raw_hi[cur] = sub_lo, sub_hi
    with np.errstate(invalid="ignore"):  # (inf - inf in the empty slots, which keep +inf / -inf below)
        lo, hi = bvh_np.inflate_lo(raw_lo), bvh_np.inflate_hi(raw_hi)
    lo[empty], hi[empty] = np.inf, -np.inf
    for a, ax in enumerate("xyz"):
        nodes["lo" + ax] = lo[..., a]
        nodes["hi" + ax] = hi[..., a]
    return nodes, bvh_np.tri_geo_of(pos[prim])


def canonical_tree(nodes, tri_geo, prim):
    """The same tree with its nodes renumbered breadth first (slot order) and its leaf ranges laid out in that
    order: two device LBVH builds of the same triangles differ only in which index the nodes of a level took
    (an atomic counter hands them out), so their canonical forms are equal bytes."""
    nodes, tri_geo, prim = np.asarray(nodes), np.asarray(tri_geo), np.asarray(prim)
    N = nodes.shape[0]
    child, count = nodes["child"].astype(np.int64), nodes["count"]
    order = np.concatenate(_levels(child, count == 0))
    assert order.shape[0] == N and np.unique(order).shape[0] == N
    new_of = np.empty(N, np.int64)
    new_of[order] = np.arange(N)
    out = nodes[order].copy()
    c, cnt = out["child"].astype(np.int64), out["count"].astype(np.int64)
    inner, leaf = cnt == 0, cnt > 0
    c[inner] = new_of[c[inner]]
    starts, counts = c[leaf], cnt[leaf]  # canonical node order, then slot order
    new_start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    src = np.repeat(starts - new_start, counts) + np.arange(int(counts.sum()))
    c[leaf] = new_start
    out["child"] = c.astype(np.int32)
    return out, tri_geo[src], prim[src]


def sah_cost_np(nodes):
    nodes = np.asarray(nodes)
    lo = np.stack([nodes["lox"], nodes["loy"], nodes["loz"]], -1).astype(np.float64)  # N x 4 x 3
    hi = np.stack([nodes["hix"], nodes["hiy"], nodes["hiz"]], -1).astype(np.float64)
    count = nodes["count"].astype(np.int64)
    full = count >= 0

    def area(lo, hi):
        d = hi - lo
        return 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])

    w = np.where(count > 0, count, 1).astype(np.float64)
    total = float((area(lo[full], hi[full]) * w[full]).sum())
    root = area(lo[0][full[0]].min(0), hi[0][full[0]].max(0))
    return 1.0 + total / float(root)
