"""The canonical form of a four-wide BVH, for comparing the trees of two builders that follow the same rule (the
device SAH builder, k_bvh_sah.hip, and the host builder it restates): everything a tree stores except what the
rule leaves free, which is the index a node takes among the nodes of its level and the order of the triangles
inside one leaf. Also the ctypes wrapper of the host-only test hook fr__scene_rebuild_over.
"""
import ctypes as C

import numpy as np

import bvh_np

F = np.float32
BOXES = ("lox", "hix", "loy", "hiy", "loz", "hiz")


def canonical(nodes, prim):
    """The tree walked from node 0, depth first in slot order, flattened to an int64 array. Per slot: its count, the
    six stored box floats as bits, then for a leaf slot its primitives in ascending order and for an inner slot the
    child's own walk. Node indices and leaf offsets do not appear."""
    nodes, prim = np.asarray(nodes), np.asarray(prim)
    assert nodes.dtype == bvh_np.NODE_DTYPE
    bits = np.stack([np.ascontiguousarray(nodes[b]).view(np.uint32) for b in BOXES], -1).astype(np.int64)  # N x 4 x 6
    child, count = nodes["child"].tolist(), nodes["count"].tolist()
    bits = bits.tolist()
    prim = prim.tolist()
    out = []
    stack = [0]
    visited = 0
    while stack:
        i = stack.pop()
        visited += 1
        assert visited <= len(child), "the nodes reached from node 0 form a cycle"
        inner = []
        for k in range(4):
            c = count[i][k]
            out.append(c)
            out.extend(bits[i][k])
            if c > 0:
                out.extend(sorted(prim[child[i][k]:child[i][k] + c]))
            elif c == 0:
                # a marker in place of the child's walk, which follows this node's slots in slot order: the walks
                # are of self-delimiting form (four slots each), so the sequence determines the tree
                out.append(-2)
                inner.append(child[i][k])
        stack.extend(reversed(inner))
    return np.asarray(out, np.int64)


def geometric(base):
    """As many triangles as base has, on one line along x: small triangles at x = 8 * 2^-(k mod 125). Every split is
    on x, and of a node's sixteen bins the lowest holds every scale but the four largest, which is also the cheapest
    cut while more than twenty scales remain: the spine of the binary tree loses four scales (then three, two, one)
    per level and passes depth 30, where a node is a leaf whatever it holds. The triangles of one scale have equal
    centroids."""
    n = np.asarray(base).shape[0]
    x = (np.float32(8.0) * np.exp2(-(np.arange(n) % 125).astype(np.float32))).astype(np.float32)
    s = np.float32(1e-3)
    pos = np.zeros((n, 3, 3), np.float32)
    pos[:, :, 0] = x[:, None]
    pos[:, 1, 1] = s
    pos[:, 2, 2] = s
    return pos


def scene_rebuild_over(fovrt, scene, pos):
    """fr__scene_rebuild_over: replaces the positions of a fovrt.Scene with pos (n x 3 x 3) and builds the host
    builder's tree over them (read it with bvh_np.scene_tree, its numbers with scene.arrays()). Returns the
    number of splits that took the host's median fallback over centroids that differ (the device builder's
    documented failure)."""
    lib = fovrt.load_library()
    fn = lib.fr__scene_rebuild_over
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    a = np.ascontiguousarray(pos, F).reshape(-1, 9)
    rc = fn(scene._h, a.ctypes.data, a.shape[0])
    assert rc >= 0, f"fr__scene_rebuild_over: status {rc}"
    return rc
