"""Per-model visibility on the references alone (no device): what tests/test_gpu_visibility.py takes for granted.

The ABI's four calls exist and refuse a NULL context. For every mask of both procedural scenes the collapsed positions
refit the host tree into a valid tree with the scene's numbers, and the host builder builds over them. For every
(scene, hidden set) the GPU frame tests render, the oracle's G-buffer over the collapsed arrays is finite and differs
from the all-visible one in at least 0.5 % of the pixels at the preset camera, so a device that ignored the call cannot
pass. Measured at 100 x 70 (percent of pixels that differ): scene 0 box 28.5, ground 42.4; scene 1 box 0.8, bunny 4.7,
earth 3.1, ground 61.2, everything 69.7. Oracle shading with the ground hidden and with nothing visible is finite.
And k_hide's tile does not line up with scene 1's model boundaries."""
import ctypes as C

import numpy as np
import pytest

import bvh_np
import ray_surface_cases as rs
import visibility_cases as vc
from bvh_canon_np import scene_rebuild_over
from bvh_refit_np import refit_np, sah_cost_np

NAMES = ("fr_model_visibility_enable", "fr_set_model_visibility", "fr_set_model_visibility_enqueue",
         "fr_model_visibility")


def test_symbols_exist_and_refuse_a_null_context(fovrt_mod):
    lib = fovrt_mod.load_library()
    for s in NAMES:
        assert hasattr(lib, s) and s in fovrt_mod._SIGS, s
    E = fovrt_mod.FR_E_INVALID
    v = C.c_uint32(7)
    assert lib.fr_model_visibility_enable(None, 1) == E
    assert lib.fr_set_model_visibility(None, 1, fovrt_mod.FR_BVH_REFIT) == E
    assert lib.fr_set_model_visibility_enqueue(None, 1) == E
    assert lib.fr_model_visibility(None, C.byref(v)) == E and v.value == 7
    for m in ("enable_model_visibility", "set_model_visibility", "model_visibility"):
        assert callable(getattr(fovrt_mod.PathTracer, m)), m


@pytest.mark.parametrize("scene", [0, 1])
def test_every_mask_refits_into_a_valid_tree_and_rebuilds_on_the_host(fovrt_mod, scene):
    a, ms, (nodes, _tri, prim) = vc.host(fovrt_mod, scene)
    assert len(ms) == (2, 4)[scene]
    twin = fovrt_mod.Scene(vc.rc.config(fovrt_mod, scene))
    for vis in range(1 << len(ms)):
        P = vc.collapsed_pos(a, ms, vis)
        hidden = ~rs.selected(ms, vis)
        assert (P[hidden, 1] == P[hidden, 0]).all() and (P[hidden, 2] == P[hidden, 0]).all()
        assert P[~hidden].tobytes() == a["pos"].reshape(-1, 3, 3)[~hidden].tobytes()
        got_nodes, got_tri = refit_np(nodes, prim, P)
        out = bvh_np.check_tree(got_nodes, got_tri, prim, P, a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"])
        assert out["nodes"] == a["bvh_nodes"], (scene, vis)
        assert scene_rebuild_over(fovrt_mod, twin, P) >= 0, (scene, vis)
        hn, ht, hp = bvh_np.scene_tree(fovrt_mod, twin)
        b = twin.arrays()
        bvh_np.check_tree(hn, ht, hp, P, b["bvh_nodes"], b["bvh_max_stack"], b["bvh_depth"],
                          leaf_max=max(2, int(hn["count"].max())))
    # the costs the rebuild policy's note quotes (scene 1, refit of the host tree): showing a model looks like growth
    if scene == 1:
        cost = {vis: sah_cost_np(refit_np(nodes, prim, vc.collapsed_pos(a, ms, vis))[0]) for vis in (15, 2, 1)}
        print("refit cost: all", cost[15], "only the box", cost[2], "only the ground", cost[1])
        assert cost[2] < cost[1] < cost[15]


@pytest.mark.parametrize("scene,hide", [(s, h) for s in vc.FRAME_CASES for h in vc.FRAME_CASES[s]] + [(0, ("ground",))])
def test_hiding_changes_the_oracles_gbuffer(fovrt_mod, oracle, scene, hide):
    _a, ms, _tree = vc.host(fovrt_mod, scene)
    g0 = vc.oracle_gbuffer(fovrt_mod, oracle, scene, vc.ALL)
    g = vc.oracle_gbuffer(fovrt_mod, oracle, scene, vc.hiding(ms, hide))
    for k in g:
        assert np.isfinite(g[k]).all(), (scene, hide, k)
    frac = vc.differing_pixels(g, g0)
    print(f"scene {scene} hidden {hide}: {100 * frac:.1f} % of the pixels differ")
    assert frac >= 0.005, (scene, hide, frac)


@pytest.mark.parametrize("hide", [("ground",), ("ground", "box", "bunny", "earth")])
def test_oracle_shading_without_the_ground_and_without_anything_is_finite(fovrt_mod, oracle, hide):
    a, ms, _tree = vc.host(fovrt_mod, 1)
    W, H = vc.W, vc.H
    uni = vc.preset_uniforms(fovrt_mod, 1)
    osc = oracle.OracleScene(rs.collapsed(a, ms, vc.hiding(ms, hide)), diffuse_max_depth=3)
    g = oracle.gbuffer(osc, uni, W, H, 0)
    z = np.zeros((H, W, 4), np.float32)
    s = oracle.sampling(osc, uni, W, H, fovrt_mod.MASK_ALL, g["position"], g["depth"], z, g["weight"], g["normal"],
                        g["diffuse"])
    assert int(s["mask"].sum()) == W * H
    sh = oracle.shading(osc, uni, W, H, 0, 2, s["mask"], s["weight"], z)
    assert np.isfinite(sh["shading"]).all() and np.isfinite(sh["history"]).all()


def test_model_boundaries_fall_inside_k_hides_tiles(fovrt_mod):
    lib = fovrt_mod.load_library()
    tile = lib.fr__visibility_tile()
    _a, ms, _tree = vc.host(fovrt_mod, 1)
    firsts = [m[1] for m in ms[1:]]
    assert firsts == [2, 14, 5134]
    assert tile > 0 and tile % 64 == 0
    assert any(f % tile != 0 and f % 64 != 0 for f in firsts)
    # several blocks, a ragged last tile, and a last float4 that is only partly the array's
    nt = ms[-1][1] + ms[-1][2]
    assert nt > 2 * tile and nt % tile != 0 and (9 * nt) % 4 != 0
