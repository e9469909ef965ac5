"""Cases and references for per-model visibility (fr_set_model_visibility), pure numpy, shared by
tests/test_cpu_visibility.py, which asserts their preconditions on the references alone, and
tests/test_gpu_visibility.py.

The reference of a hidden model is ray_surface_cases.collapsed: every triangle of the model collapsed onto its first
vertex. The oracle, the numpy restatements and the tree validators run over those arrays as over any others; the
scene box stays the true positions' (collapsed() copies it)."""
import numpy as np

import bvh_np
import ray_cases as rc
import ray_surface_cases as rs

F = np.float32
W, H = 100, 70  # the frames' screen: partial 8x8 tiles, 16x16 blocks and 16-pixel groups
ALL = 0xFFFFFFFF

# (scene) -> the sets of hidden models the frame tests render
FRAME_CASES = {0: [("box",)],
               1: [("box",), ("bunny",), ("earth",), ("ground",), ("ground", "box", "bunny", "earth")]}

_HOST = {}
_GBUF = {}


def host(fovrt, scene):
    """(arrays, models, (nodes, tri_geo, prim) of the host builder's tree) of a procedural scene, once, read-only."""
    if scene not in _HOST:
        sc = fovrt.Scene(rc.config(fovrt, scene))
        tree = bvh_np.scene_tree(fovrt, sc)
        for v in tree:
            v.setflags(write=False)
        _HOST[scene] = (sc.arrays(), sc.models(), tree)
    return _HOST[scene]


def valid(ms):
    return (1 << len(ms)) - 1


def hiding(ms, names):
    """The mask that hides the named models and shows every other one (high bits set, as FR_VISIBLE_ALL has them)."""
    all_names = [m[0] for m in ms]
    mask = ALL
    for n in names:
        mask &= ~(1 << all_names.index(n))
    return mask & ALL


def tree_masks(ms):
    """Each single model hidden, each single model visible, nothing visible, everything visible."""
    v = valid(ms)
    out = [v & ~(1 << i) for i in range(len(ms))] + [1 << i for i in range(len(ms))] + [0, v]
    return list(dict.fromkeys(out))


def collapsed_pos(arrays, ms, vis):
    """C(P, visible) as n x 3 x 3."""
    return rs.collapsed(arrays, ms, vis)["pos"].reshape(-1, 3, 3)


def preset_uniforms(fovrt, scene):
    return fovrt.Camera.preset(scene, W, H).uniforms(W, H)


def oracle_gbuffer(fovrt, oracle, scene, vis):
    """The oracle's frame-0 G-buffer of a procedural scene under `vis` from the preset camera, once per mask."""
    a, ms, _tree = host(fovrt, scene)
    key = (scene, vis & valid(ms))
    if key not in _GBUF:
        _GBUF[key] = oracle.gbuffer(oracle.OracleScene(rs.collapsed(a, ms, vis)), preset_uniforms(fovrt, scene), W, H, 0)
    return _GBUF[key]


def differing_pixels(g, g0):
    """The fraction of pixels at which two G-buffers differ in any bit of any output."""
    diff = np.zeros(g0["position"].shape[:2], bool)
    for k in g0:
        diff |= (np.ascontiguousarray(g[k]).view(np.uint32) != np.ascontiguousarray(g0[k]).view(np.uint32)).any(-1)
    return float(diff.mean())
