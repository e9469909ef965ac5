"""CPU suite for what the device SAH builder's GPU tests stand on: the canonical form of a tree (bvh_canon_np) is not
vacuous, and the host builder run over any geometry (fr__scene_rebuild_over) gives valid trees, the preset's own
tree over the preset's positions, and never takes the one path the device builder is allowed to refuse.
"""
import numpy as np
import pytest

import bvh_cases
import bvh_np
from bvh_canon_np import canonical, geometric, scene_rebuild_over

NUMBERS = ("bvh_nodes", "bvh_depth", "bvh_max_stack")


def make_scene(fovrt, scene):
    return fovrt.Scene(fovrt.Config(scene=scene, texture_mode=1, detail=1))


@pytest.fixture(scope="module")
def rest(fovrt_mod):
    """{scene: (arrays, (nodes, tri, prim))} of the presets at rest."""
    out = {}
    for scene in (0, 1):
        sc = make_scene(fovrt_mod, scene)
        out[scene] = (sc.arrays(), bvh_np.scene_tree(fovrt_mod, sc))
    return out


def renumbered(nodes, prim, seed):
    """The same tree with its nodes under a random permutation (the root stays), child indices and leaf ranges
    rewritten to match, and the primitives of every leaf reversed."""
    rng = np.random.default_rng(seed)
    N = nodes.shape[0]
    perm = np.concatenate([[0], 1 + rng.permutation(N - 1)])
    out = np.empty_like(nodes)
    out[perm] = nodes
    inner = out["count"] == 0
    out["child"][inner] = perm[out["child"][inner]]
    new_prim = np.empty_like(prim)
    at = 0
    for i in range(N):
        for k in range(4):
            c = int(out["count"][i, k])
            if c > 0:
                first = int(out["child"][i, k])
                new_prim[at:at + c] = prim[first:first + c][::-1]
                out["child"][i, k] = at
                at += c
    assert at == prim.shape[0]
    return out, new_prim


@pytest.mark.parametrize("scene", [0, 1])
def test_canonical_form_ignores_numbering_and_leaf_order(rest, scene):
    nodes, _, prim = rest[scene][1]
    want = canonical(nodes, prim)
    for seed in (1, 2):
        n2, p2 = renumbered(nodes, prim, seed)
        assert p2.tobytes() != prim.tobytes()
        assert n2.tobytes() != nodes.tobytes() or nodes.shape[0] <= 2  # (scene 0: the root and one node)
        assert np.array_equal(canonical(n2, p2), want)


@pytest.mark.parametrize("scene", [0, 1])
def test_canonical_form_tells_trees_apart(fovrt_mod, rest, scene):
    arrays, (nodes, _, prim) = rest[scene]
    want = canonical(nodes, prim)
    # one bit of one stored box
    n2 = nodes.copy()
    n2["hiy"].view(np.uint32)[n2.shape[0] // 2, 0] ^= 1
    assert not np.array_equal(canonical(n2, prim), want)
    # two primitives of different leaves exchanged
    p2 = prim.copy()
    p2[0], p2[-1] = prim[-1], prim[0]
    assert not np.array_equal(canonical(nodes, p2), want)
    # the host tree over other geometry
    sc = make_scene(fovrt_mod, scene)
    scene_rebuild_over(fovrt_mod, sc, bvh_cases.CASES["comb"](arrays["pos"].reshape(-1, 3, 3), 0))
    n3, _, p3 = bvh_np.scene_tree(fovrt_mod, sc)
    assert not np.array_equal(canonical(n3, p3), want)


@pytest.mark.parametrize("scene", [0, 1])
def test_rebuild_over_rest_positions_reproduces_the_scene_tree(fovrt_mod, rest, scene):
    arrays, tree = rest[scene]
    sc = make_scene(fovrt_mod, scene)
    assert scene_rebuild_over(fovrt_mod, sc, arrays["pos"]) == 0
    for name, a, b in zip(("nodes", "tri_geo", "prim"), bvh_np.scene_tree(fovrt_mod, sc), tree):
        assert a.tobytes() == b.tobytes(), name
    after = sc.arrays()
    assert {k: after[k] for k in NUMBERS} == {k: arrays[k] for k in NUMBERS}
    assert np.array_equal(after["bbox"], arrays["bbox"])


@pytest.mark.parametrize("case", sorted(bvh_cases.CASES))
@pytest.mark.parametrize("scene", [0, 1])
def test_rebuild_over_every_case(fovrt_mod, rest, scene, case):
    arrays = rest[scene][0]
    pos = bvh_cases.CASES[case](arrays["pos"].reshape(-1, 3, 3), 0)
    sc = make_scene(fovrt_mod, scene)
    # the condition under which the device builder may answer FR_E_UNSUPPORTED: these inputs stay clear of it
    assert scene_rebuild_over(fovrt_mod, sc, pos) == 0
    a = sc.arrays()
    assert np.array_equal(a["pos"].reshape(-1, 3, 3), pos)
    nodes, tri, prim = bvh_np.scene_tree(fovrt_mod, sc)
    assert nodes.shape[0] == a["bvh_nodes"]
    # a node at depth 30 is a leaf whatever it holds
    leaf_max = max(2, int(nodes["count"].max()))
    out = bvh_np.check_tree(nodes, tri, prim, pos, a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"], leaf_max=leaf_max)
    print(f"scene {scene} {case}: {out} leaf_max {leaf_max}")
    if case != "comb":
        assert leaf_max == 2


def test_geometric_comb_reaches_depth_30(fovrt_mod, rest):
    """The geometry the GPU suite uses for the depth limit: leaves of more than two triangles on the host, a valid
    tree, and no median fallback."""
    pos = geometric(rest[1][0]["pos"].reshape(-1, 3, 3))
    sc = make_scene(fovrt_mod, 1)
    assert scene_rebuild_over(fovrt_mod, sc, pos) == 0
    a = sc.arrays()
    nodes, tri, prim = bvh_np.scene_tree(fovrt_mod, sc)
    leaf_max = int(nodes["count"].max())
    out = bvh_np.check_tree(nodes, tri, prim, pos, a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"], leaf_max=leaf_max)
    print(f"geometric: {out} leaf_max {leaf_max}")
    assert leaf_max > 2
    with pytest.raises(bvh_np.BvhError, match="more than 2"):
        bvh_np.check_tree(nodes, tri, prim, pos, a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"])


def test_rebuild_over_refuses_bad_arguments(fovrt_mod, rest):
    import ctypes as C
    lib = fovrt_mod.load_library()
    fn = lib.fr__scene_rebuild_over
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    sc = make_scene(fovrt_mod, 0)
    pos = np.ascontiguousarray(rest[0][0]["pos"], np.float32).reshape(-1, 9).copy()
    assert fn(sc._h, pos.ctypes.data, pos.shape[0] - 1) == fovrt_mod.FR_E_INVALID
    assert fn(sc._h, None, pos.shape[0]) == fovrt_mod.FR_E_INVALID
    pos[3, 4] = np.inf
    assert fn(sc._h, pos.ctypes.data, pos.shape[0]) == fovrt_mod.FR_E_INVALID
    for name, a, b in zip(("nodes", "tri_geo", "prim"), bvh_np.scene_tree(fovrt_mod, sc), rest[0][1]):
        assert a.tobytes() == b.tobytes(), name
