"""CPU suite for the BVH: the numpy validator (bvh_np.check_tree) against a hand-made tree and one mutation
per invariant, the host binned-SAH builder's trees of the presets, the adversarial geometry of bvh_cases (each
case has the property it claims), and the oracle's own tree against its brute force on every case, which is
what the GPU comparisons of test_gpu_bvh.py rest on."""
import numpy as np
import pytest

import bvh_cases
import bvh_np
from bvh_np import BvhError, NODE_DTYPE, check_tree

F = np.float32
W, H = 64, 48


# ---------------------------------------------------------------------------------------------
# The validator: a hand-made four-node tree over ten triangles
#   node 0: inner 1 | inner 2 | leaf [0, 2) | empty        (two inner children: one stack entry)
#   node 1: leaf [2, 4) | inner 3 | leaf [4, 5) | empty
#   node 2: leaf [5, 6) | leaf [6, 8) | empty | empty
#   node 3: leaf [8, 9) | leaf [9, 10) | empty | empty     (level 2)
# Its boxes are computed here slot by slot with scalar float32 arithmetic over explicit vertex lists.
# ---------------------------------------------------------------------------------------------
TOPOLOGY = [[("inner", 1), ("inner", 2), ("leaf", 0, 2)],
            [("leaf", 2, 2), ("inner", 3), ("leaf", 4, 1)],
            [("leaf", 5, 1), ("leaf", 6, 2)],
            [("leaf", 8, 1), ("leaf", 9, 1)]]
PRIM = np.array([7, 2, 9, 0, 4, 1, 8, 3, 6, 5], np.int32)


def _below(slot):
    """Leaf-order triangle indices below a slot of TOPOLOGY."""
    if slot[0] == "leaf":
        return list(range(slot[1], slot[1] + slot[2]))
    return [j for s in TOPOLOGY[slot[1]] for j in _below(s)]


def _scalar_inflate(v, sign):
    pad = F(F(1e-5) + F(F(4e-7) * F(abs(v))))
    return F(v - pad) if sign < 0 else F(v + pad)


def hand_tree():
    rng = np.random.default_rng(11)
    pos = (rng.uniform(-2, 2, (10, 1, 3)) + rng.uniform(-0.3, 0.3, (10, 3, 3))).astype(F)
    pos[4, :, 1] = F(0.5)  # an axis-aligned triangle: a box of zero thickness
    nodes = np.zeros(4, NODE_DTYPE)
    for i, slots in enumerate(TOPOLOGY):
        for k in range(4):
            if k >= len(slots):
                for ax in "xyz":
                    nodes[i]["lo" + ax][k], nodes[i]["hi" + ax][k] = np.inf, -np.inf
                nodes[i]["child"][k], nodes[i]["count"][k] = 0, -1
                continue
            verts = [pos[PRIM[j], v] for j in _below(slots[k]) for v in range(3)]
            for a, ax in enumerate("xyz"):
                nodes[i]["lo" + ax][k] = _scalar_inflate(min(float(p[a]) for p in verts), -1)
                nodes[i]["hi" + ax][k] = _scalar_inflate(max(float(p[a]) for p in verts), +1)
            nodes[i]["child"][k] = slots[k][1]
            nodes[i]["count"][k] = slots[k][2] if slots[k][0] == "leaf" else 0
    tri = np.zeros((10, 12), F)
    for j in range(10):
        p0, p1, p2 = pos[PRIM[j]]
        e0, e1 = p1 - p0, p0 - p2
        nrm = [F(F(e1[1] * e0[2]) - F(e1[2] * e0[1])), F(F(e1[2] * e0[0]) - F(e1[0] * e0[2])),
               F(F(e1[0] * e0[1]) - F(e1[1] * e0[0]))]
        tri[j] = [*p0, *e0, *e1, *nrm]
    return nodes, tri, PRIM.copy(), pos


def _check(nodes, tri, prim, pos, n_nodes=4, stack=1, depth=2, **kw):
    return check_tree(nodes, tri, prim, pos, n_nodes, stack, depth, **kw)


def test_inflation_known_answers():
    """inflate(1) by hand: the pad is 1e-5f + 4e-7f = 1.04e-5, which is 87.2 ulps of [1, 2) and 174.5 ulps of
    [0.5, 1): hi = 1 + 87 * 2^-23, lo = 1 - 174 * 2^-24 (174.48 rounds down)."""
    assert bvh_np.inflate_hi(F(1.0)).view(np.uint32) == 0x3F800057
    assert bvh_np.inflate_lo(F(1.0)).view(np.uint32) == 0x3F800000 - 174
    assert bvh_np.inflate_lo(F(0.0)) == -F(1e-5) and bvh_np.inflate_hi(F(-0.0)) == F(1e-5)
    assert _scalar_inflate(F(1.0), +1).view(np.uint32) == 0x3F800057


def test_validator_accepts_the_hand_made_tree():
    out = _check(*hand_tree())
    assert out == {"nodes": 4, "max_stack": 1, "depth": 2, "leaves": 7}


def _swap_inner(nodes, tri, prim, pos):
    for name in ("lox", "hix", "loy", "hiy", "loz", "hiz", "child"):  # the boxes stay right: only the order is wrong
        nodes[0][name][[0, 1]] = nodes[0][name][[1, 0]]


def _duplicate_prim(nodes, tri, prim, pos):
    prim[3] = prim[4]


def _shrink_hi(nodes, tri, prim, pos):
    nodes[1]["hix"][1] = np.nextafter(nodes[1]["hix"][1], F(-np.inf))


def _shrink_lo(nodes, tri, prim, pos):
    nodes[0]["loz"][0] = np.nextafter(nodes[0]["loz"][0], F(np.inf))


def _grow_hi(nodes, tri, prim, pos):
    nodes[2]["hiy"][1] = np.nextafter(nodes[2]["hiy"][1], F(np.inf))


def _leaf_gap(nodes, tri, prim, pos):
    nodes[2]["child"][1], nodes[2]["count"][1] = 7, 1  # triangle 6 is in no leaf


def _leaf_overlap(nodes, tri, prim, pos):
    nodes[2]["count"][0] = 2  # triangle 6 is in two leaves


def _gap_between_nodes(nodes, tri, prim, pos):
    nodes[3]["child"][0], nodes[3]["count"][0] = 9, 1  # back to back inside every node, triangle 8 in no leaf
    nodes[3]["child"][1], nodes[3]["count"][1] = 0, -1
    for ax in "xyz":
        nodes[3]["lo" + ax][1], nodes[3]["hi" + ax][1] = np.inf, -np.inf


def _orphan(nodes, tri, prim, pos):
    nodes[1]["child"][1], nodes[1]["count"][1] = 0, -1  # nothing points to node 3 any more
    for ax in "xyz":
        nodes[1]["lo" + ax][1], nodes[1]["hi" + ax][1] = np.inf, -np.inf


def _shared_child(nodes, tri, prim, pos):
    nodes[1]["child"][1] = 2  # node 2 has two parents, node 3 none


def _empty_with_box(nodes, tri, prim, pos):
    nodes[2]["lox"][3] = F(0.0)


def _empty_with_child(nodes, tri, prim, pos):
    nodes[2]["child"][2] = 1


def _leaf_out_of_range(nodes, tri, prim, pos):
    nodes[3]["count"][1] = 2


def _inner_out_of_range(nodes, tri, prim, pos):
    nodes[1]["child"][1] = 4


def _tri_geo_ulp(nodes, tri, prim, pos):
    tri[5, 10] = np.nextafter(tri[5, 10], F(np.inf))


def _tri_geo_wrong_prim(nodes, tri, prim, pos):
    tri[[2, 3]] = tri[[3, 2]]


MUTATIONS = [(_swap_inner, "not consecutive"), (_duplicate_prim, "appears"), (_shrink_hi, r"node 1 slot 1: box hi\.x"),
             (_shrink_lo, r"node 0 slot 0: box lo\.z"), (_grow_hi, r"node 2 slot 1: box hi\.y"),
             (_leaf_gap, "node 2 slot 1: .*not back to back"), (_leaf_overlap, "node 2 slot 1: .*not back to back"),
             (_gap_between_nodes, "leaves a gap"), (_orphan, "node 3: orphan"), (_shared_child, "node 2 is the child of 2"),
             (_empty_with_box, "node 2 slot 3: empty slot"), (_empty_with_child, "node 2 slot 2: empty slot"),
             (_leaf_out_of_range, r"node 3 slot 1: leaf range \[9, 11\)"), (_inner_out_of_range, "node 1 slot 1: inner child 4"),
             (_tri_geo_ulp, r"tri_geo\[5\]"), (_tri_geo_wrong_prim, r"tri_geo\[2\]")]


@pytest.mark.parametrize("mutate,message", MUTATIONS, ids=[m[0].__name__.lstrip("_") for m in MUTATIONS])
def test_validator_rejects_one_mutation_per_invariant(mutate, message):
    tree = hand_tree()
    mutate(*tree)
    with pytest.raises(BvhError, match=message):
        _check(*tree)


@pytest.mark.parametrize("kw,message", [(dict(stack=0), "needs 1 stack entries, 0 reported"),
                                        (dict(stack=2), "needs 1 stack entries, 2 reported"),
                                        (dict(depth=1), "at level 2, depth 1 reported"),
                                        (dict(depth=3), "at level 2, depth 3 reported"),
                                        (dict(n_nodes=3), "inner child 3 outside"),
                                        (dict(n_nodes=11), "node count 11 outside"),
                                        (dict(leaf_max=1), "leaf of 2 triangles")])
def test_validator_rejects_wrong_reported_numbers(kw, message):
    with pytest.raises(BvhError, match=message):
        _check(*hand_tree(), **kw)


def test_validator_rejects_a_stack_deeper_than_the_traversal_has():
    """A chain of 26 nodes with two inner children each (the second a one-leaf node) needs 26 stack entries:
    consistent with what is reported, and more than FR_BVH_STACK."""
    depth = 26
    n = 2 * depth + 2
    pos = (np.arange(n, dtype=F)[:, None, None] + np.random.default_rng(5).uniform(0, 0.5, (n, 3, 3))).astype(F)
    nodes = np.zeros(2 * depth + 1, NODE_DTYPE)
    nodes["count"][:] = -1
    for name in ("lox", "loy", "loz"):
        nodes[name][:] = np.inf
    for name in ("hix", "hiy", "hiz"):
        nodes[name][:] = -np.inf
    tmin, tmax = pos.min(1), pos.max(1)

    def put(i, k, child, count, first, last):  # slot k of node i covers triangles [first, last)
        nodes[i]["child"][k], nodes[i]["count"][k] = child, count
        for a, ax in enumerate("xyz"):
            nodes[i]["lo" + ax][k] = bvh_np.inflate_lo(tmin[first:last, a].min())
            nodes[i]["hi" + ax][k] = bvh_np.inflate_hi(tmax[first:last, a].max())

    # chain node c (index 2c): inner 2c+1 (a one-leaf node over triangle 2c) | inner 2c+2 (the rest of the chain)
    # | leaf [2c+1, 2c+2); the last node holds the last two triangles
    for c in range(depth):
        put(2 * c, 0, 2 * c + 1, 0, 2 * c, 2 * c + 1)
        put(2 * c, 1, 2 * c + 2, 0, 2 * c + 2, n)
        put(2 * c, 2, 2 * c + 1, 1, 2 * c + 1, 2 * c + 2)
        put(2 * c + 1, 0, 2 * c, 1, 2 * c, 2 * c + 1)
    put(2 * depth, 0, 2 * depth, 2, 2 * depth, n)
    prim = np.arange(n, dtype=np.int32)
    tri = bvh_np.tri_geo_of(pos)
    with pytest.raises(BvhError, match="exceeds FR_BVH_STACK"):
        check_tree(nodes, tri, prim, pos, 2 * depth + 1, depth, depth)
    with pytest.raises(BvhError, match="needs 26 stack entries"):
        check_tree(nodes, tri, prim, pos, 2 * depth + 1, 24, depth)


# ---------------------------------------------------------------------------------------------
# The host builder's trees of the presets
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,detail", [(0, 1), (1, 1), (2, 1), (1, 0)])
def test_host_builder_trees_of_the_presets(fovrt_mod, scene, detail):
    sc = fovrt_mod.Scene(fovrt_mod.Config(scene=scene, texture_mode=1, detail=detail))
    a = sc.arrays()
    nodes, tri, prim = bvh_np.scene_tree(fovrt_mod, sc)
    assert nodes.shape[0] == a["bvh_nodes"] and prim.shape[0] == len(a["flags"])
    out = check_tree(nodes, tri, prim, a["pos"].reshape(-1, 3, 3), a["bvh_nodes"], a["bvh_max_stack"], a["bvh_depth"])
    assert out["leaves"] >= (len(a["flags"]) + 1) // 2


# ---------------------------------------------------------------------------------------------
# The adversarial cases: what they claim, and the oracle's tree against its brute force on each
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_scenes(fovrt_mod):
    out = {}
    for scene in (0, 1):
        out[scene] = fovrt_mod.Scene(fovrt_mod.Config(scene=scene, texture_mode=1, detail=1)).arrays()
    return out


def _centroid_extent(pos):
    """The extent k_morton divides by: max - min of the box centres (lo + hi) * 0.5, float32."""
    c = (pos.min(1) + pos.max(1)) * F(0.5)
    return c.max(0) - c.min(0)


def _zero_area(pos):
    return np.all(bvh_np.tri_geo_of(pos)[:, 9:12] == 0, axis=1)


@pytest.mark.parametrize("scene", [0, 1])
@pytest.mark.parametrize("seed", [0, 5])
def test_cases_are_what_they_claim(base_scenes, scene, seed):
    a = base_scenes[scene]
    base = a["pos"].reshape(-1, 3, 3)
    n = base.shape[0]
    lo, hi = a["bbox"][:3], a["bbox"][3:]
    assert not _zero_area(base).any()
    made = {name: fn(base, seed) for name, fn in bvh_cases.CASES.items()}
    assert set(made) == {"identical", "pairs", "sheet_z", "sheet_x", "line", "degenerate_mix", "two_scales", "comb"}
    for name, pos in made.items():
        assert pos.shape == base.shape and pos.dtype == F and np.isfinite(pos).all(), name
        assert (pos >= lo).all() and (pos <= hi).all(), name
        assert np.array_equal(pos, bvh_cases.CASES[name](base, seed)), name  # pure
    assert (made["identical"] == made["identical"][0]).all() and not _zero_area(made["identical"]).any()
    assert np.array_equal(_centroid_extent(made["identical"]), np.zeros(3, F))
    p = made["pairs"]
    assert np.array_equal(p[1::2], p[0:2 * (n // 2):2]) and np.array_equal(p[0::2], base[0::2])
    for name, dead in (("sheet_z", [2]), ("sheet_x", [0]), ("line", [1, 2])):
        ext = _centroid_extent(made[name])
        live = [ax for ax in range(3) if ax not in dead]
        assert (ext[dead] == 0).all() and (ext[live] > 0).all(), (name, ext)
        assert not _zero_area(made[name]).any(), name
    for name, ax in (("sheet_z", 2), ("sheet_x", 0)):  # non-overlapping: the areas add up to the rectangle's
        g = bvh_np.tri_geo_of(made[name]).astype(np.float64)
        area = 0.5 * np.abs(g[:, 9 + ax]).sum()
        u, v = [b for b in range(3) if b != ax]
        cells = int(np.ceil(np.sqrt((n + 1) // 2))) ** 2
        assert np.isclose(area, (hi[u] - lo[u]) * (hi[v] - lo[v]) * (n / 2) / cells, rtol=1e-5), name
    points, segs = bvh_cases.degenerate_counts(n)
    d = made["degenerate_mix"]
    is_point = np.all(d == d[:, :1], axis=(1, 2))
    assert is_point.sum() == points == (n + 2) // 3
    assert _zero_area(d).sum() == points + segs and (_zero_area(d) & ~is_point).sum() == segs > 0
    t = made["two_scales"]
    h = n // 2
    assert np.array_equal(t[1:h], base[1:h])
    assert np.array_equal(t[0].min(0), lo) and np.array_equal(t[0].max(0), hi)
    assert ((t[h:] - lo) <= (hi - lo) * F(2.0 ** -10)).all() and len(np.unique(t[h:].reshape(-1, 3), axis=0)) > 1
    c = made["comb"]
    want_x = (lo[0] + (hi[0] - lo[0]) * np.exp2(-(np.arange(n) % 24).astype(np.float64))).astype(F)
    assert np.array_equal(c[:, 0, 0], want_x) and len(np.unique(want_x)) == min(n, 24)
    assert not _zero_area(c).any()


@pytest.fixture(scope="module")
def pose_rays(fovrt_mod, base_scenes):
    out = {}
    for scene, a in base_scenes.items():
        cams = bvh_cases.poses(fovrt_mod, scene, a["bbox"], W, H)
        out[scene] = np.concatenate([bvh_cases.primary_rays(c.uniforms(W, H), W, H) for c in cams.values()])
        assert np.isfinite(out[scene][:, :7]).all()
    return out


@pytest.mark.parametrize("scene", [0, 1])
@pytest.mark.parametrize("case", sorted(bvh_cases.CASES))
def test_oracle_tree_equals_brute_force_on_every_case(oracle, base_scenes, pose_rays, scene, case):
    """The reference the GPU tests compare with: the oracle's closest hit through its own BVH equals its brute
    force over all triangles (t, primitive and barycentrics, bit for bit) for the rays of the three poses."""
    a = dict(base_scenes[scene])
    pos = bvh_cases.CASES[case](a["pos"].reshape(-1, 3, 3), 0)
    a["pos"] = pos.reshape(-1, 9)
    sc = oracle.OracleScene(a)
    rays = pose_rays[scene]
    assert rays.shape == (3 * W * H, 8)
    A, B = sc.closest(rays), sc.closest(rays, brute=True)
    hits = (B[:, 1] >= 0).mean()
    print(f"scene {scene} {case}: {hits:.3f} of the rays hit")
    assert hits >= 0.05, hits
    assert np.array_equal(A, B), np.argwhere(A != B)[:5]
