"""CPU suite for the BVH refit's references (bvh_refit_np): refit_np against the validator of the trees
(bvh_np.check_tree) on the host builder's topology, sah_cost_np against a value computed by hand, so that the
GPU tests of test_gpu_bvh_refit.py compare with something checked. Also the new calls' NULL-context answers."""
import ctypes as C

import numpy as np
import pytest

import bvh_cases
import bvh_np
from bvh_refit_np import refit_np, sah_cost_np

F = np.float32


@pytest.fixture(scope="module")
def host_trees(fovrt_mod):
    """scene -> (arrays, (nodes, tri_geo, prim)) of the host binned-SAH builder, read-only."""
    out = {}
    for scene in (0, 1):
        sc = fovrt_mod.Scene(fovrt_mod.Config(scene=scene, texture_mode=1, detail=1))
        a = sc.arrays()
        tree = bvh_np.scene_tree(fovrt_mod, sc)
        for v in tree:
            v.setflags(write=False)
        out[scene] = (a, tree)
    return out


@pytest.mark.parametrize("scene", [0, 1])
def test_refit_over_unchanged_positions_returns_the_same_bytes(host_trees, scene):
    a, (nodes, tri, prim) = host_trees[scene]
    got_nodes, got_tri = refit_np(nodes, prim, a["pos"].reshape(-1, 3, 3))
    assert got_nodes.tobytes() == nodes.tobytes()
    assert got_tri.tobytes() == tri.tobytes()


@pytest.mark.parametrize("case", sorted(bvh_cases.CASES))
@pytest.mark.parametrize("scene", [0, 1])
def test_refit_over_every_case_is_a_valid_tree_with_the_same_numbers(host_trees, scene, case):
    a, (nodes, tri, prim) = host_trees[scene]
    pos = bvh_cases.CASES[case](a["pos"].reshape(-1, 3, 3), 0)
    got_nodes, got_tri = refit_np(nodes, prim, pos)
    for name in ("child", "count"):
        assert np.array_equal(got_nodes[name], nodes[name])
    out = bvh_np.check_tree(got_nodes, got_tri, prim, pos, a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"])
    assert out["nodes"] == a["bvh_nodes"]


def _slot(nodes, i, k, lo, hi, child, count):
    for a, ax in enumerate("xyz"):
        nodes[i]["lo" + ax][k], nodes[i]["hi" + ax][k] = lo[a], hi[a]
    nodes[i]["child"][k], nodes[i]["count"][k] = child, count


def test_cost_of_a_hand_made_two_node_tree():
    """node 0: inner -> node 1, box (0,0,0)-(2,1,1): area 2 (2 + 1 + 2) = 10, weight 1
               leaf of 2,        box (2,0,0)-(4,2,1): area 2 (4 + 2 + 2) = 16, weight 2
       node 1: leaf of 1,        box (0,0,0)-(1,1,1): area 6, weight 1
               leaf of 2,        box (1,0,0)-(2,1,1): area 6, weight 2
       root = union of node 0's slots = (0,0,0)-(4,2,1): area 2 (8 + 2 + 4) = 28
       cost = 1 + (10 + 32 + 6 + 12) / 28"""
    nodes = np.zeros(2, bvh_np.NODE_DTYPE)
    for i in range(2):
        for k in range(4):
            _slot(nodes, i, k, [np.inf] * 3, [-np.inf] * 3, 0, -1)
    _slot(nodes, 0, 0, [0, 0, 0], [2, 1, 1], 1, 0)
    _slot(nodes, 0, 1, [2, 0, 0], [4, 2, 1], 3, 2)
    _slot(nodes, 1, 0, [0, 0, 0], [1, 1, 1], 0, 1)
    _slot(nodes, 1, 1, [1, 0, 0], [2, 1, 1], 1, 2)
    assert sah_cost_np(nodes) == 1.0 + 60.0 / 28.0
    # a leaf's weight is its triangle count; an empty slot adds nothing, whatever box it holds
    nodes[1]["count"][1] = 1
    assert sah_cost_np(nodes) == 1.0 + 54.0 / 28.0


@pytest.mark.parametrize("scene", [0, 1])
def test_comb_refit_costs_more_than_the_base_tree(host_trees, scene):
    """What test_gpu_bvh_refit.py asserts of the device's number, first on the references: a one-sided pile of
    teeth cannot fit the base topology better than the geometry it was built for."""
    a, (nodes, tri, prim) = host_trees[scene]
    pos = bvh_cases.CASES["comb"](a["pos"].reshape(-1, 3, 3), 0)
    before, after = sah_cost_np(nodes), sah_cost_np(refit_np(nodes, prim, pos)[0])
    print(f"scene {scene}: cost {before:.3f} -> {after:.3f} after the comb refit")
    assert after > before


@pytest.mark.parametrize("scene", [0, 1])
def test_canonical_form_undoes_a_renumbering(host_trees, scene):
    """canonical_tree (what the GPU tests compare two device-built trees by): a valid tree with the same numbers,
    a fixed point of itself, and the same bytes for a copy whose nodes below the root were shuffled and whose
    leaf ranges were laid out in the shuffled order."""
    from bvh_refit_np import canonical_tree
    a, (nodes, tri, prim) = host_trees[scene]
    pos = a["pos"].reshape(-1, 3, 3)
    canon = canonical_tree(nodes, tri, prim)
    bvh_np.check_tree(*canon, pos, a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"])
    again = canonical_tree(*canon)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(canon, again))
    # shuffle: sibling groups (the inner children of one node) stay consecutive, the groups move
    N = nodes.shape[0]
    child, count = nodes["child"].astype(np.int64), nodes["count"].astype(np.int64)
    groups = [child[i][count[i] == 0] for i in range(N) if (count[i] == 0).any()]
    rng = np.random.default_rng(3)
    order = np.concatenate([[0]] + [groups[g] for g in rng.permutation(len(groups))]).astype(np.int64)
    new_of = np.empty(N, np.int64)
    new_of[order] = np.arange(N)
    sh = nodes[order].copy()
    c, cnt = sh["child"].astype(np.int64), sh["count"].astype(np.int64)
    c[cnt == 0] = new_of[c[cnt == 0]]
    leaf = cnt > 0
    starts, counts = c[leaf], cnt[leaf]
    new_start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    src = np.repeat(starts - new_start, counts) + np.arange(int(counts.sum()))
    c[leaf] = new_start
    sh["child"] = c.astype(np.int32)
    sh_tri, sh_prim = tri[src], prim[src]
    bvh_np.check_tree(sh, sh_tri, sh_prim, pos, a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"])
    if N > 8:
        assert sh.tobytes() != nodes.tobytes()
    back = canonical_tree(sh, sh_tri, sh_prim)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(canon, back))


def test_null_context_is_invalid(fovrt_mod):
    lib = fovrt_mod.load_library()
    ms, cost = C.c_float(), C.c_float()
    xyz = (C.c_float * 9)()
    assert lib.fr_refit_bvh(None, C.byref(ms)) == fovrt_mod.FR_E_INVALID
    for where in (fovrt_mod.FR_MEM_HOST, fovrt_mod.FR_MEM_DEVICE):
        for how in (fovrt_mod.FR_BVH_REBUILD, fovrt_mod.FR_BVH_REFIT):
            assert lib.fr_update_positions(None, C.cast(xyz, C.c_void_p), 1, where, how) == fovrt_mod.FR_E_INVALID
    assert lib.fr_bvh_sah_cost(None, C.byref(cost)) == fovrt_mod.FR_E_INVALID
