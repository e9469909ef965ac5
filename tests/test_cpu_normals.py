"""CPU suite for the smooth-vertex weld behind fr_update_geometry's normals (no device): fr_scene_normal_groups
against normals_np.weld_np, the creases of the box scene, and the rule at the rest pose against the normals the
scene was built with."""
import numpy as np
import pytest

import bvh_cases
from normals_np import HAS_NORMALS, mirrored_pairs, recompute_np, weld_np

# (triangles, smooth vertices) of the procedural presets at detail=1
COUNTS = {0: (14, 28), 1: (9106, 4671), 2: (34638, 23017)}


@pytest.fixture(scope="module")
def scenes(fovrt_mod):
    out = {}
    for scene in COUNTS:
        sc = fovrt_mod.Scene(fovrt_mod.Config(scene=scene, texture_mode=1, detail=1, mesh_mode=1))
        a = sc.arrays()
        cv, nv = sc.normal_groups()
        for v in (a["pos"], a["nrm"], a["flags"], cv):
            v.setflags(write=False)
        out[scene] = (a, cv, nv)
    return out


@pytest.mark.parametrize("scene", sorted(COUNTS))
def test_weld_equals_numpy(scenes, scene):
    a, cv, nv = scenes[scene]
    want_cv, want_nv = weld_np(a["pos"], a["nrm"], a["flags"])
    assert (a["flags"].size, nv) == COUNTS[scene]
    assert nv == want_nv
    assert cv.dtype == np.int32 and np.array_equal(cv, want_cv)
    # ids in order of first corner: the first appearances of 0, 1, 2, ... are ascending and complete
    seen = cv[cv >= 0]
    _, first = np.unique(seen, return_index=True)
    assert np.array_equal(np.sort(first), first) and first.size == nv
    valence = np.bincount(seen, minlength=nv)
    print(f"scene {scene}: {nv} vertices, valence mean {valence.mean():.2f} max {valence.max()}")
    assert valence.min() >= 1 and valence.max() <= 64


def test_creases_stay_apart_and_triangles_without_normals_have_no_vertex(scenes):
    a, cv, nv = scenes[0]
    pos, nrm = a["pos"].reshape(-1, 3), a["nrm"].reshape(-1, 3)
    has = np.repeat((a["flags"] & HAS_NORMALS) != 0, 3)
    assert has.all()  # every preset triangle carries normals
    # the cube's corners: one position, three face normals, three vertices
    _, inv, count = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    creased = 0
    for p in np.flatnonzero(count > 1):
        at = np.flatnonzero(inv == p)
        normals = np.unique(nrm[at], axis=0).shape[0]
        assert np.unique(cv[at]).size == normals
        creased += normals > 1
    assert creased >= 8
    # a corner is welded only to corners with its position and its normal
    for v in range(nv):
        at = np.flatnonzero(cv == v)
        assert (pos[at] == pos[at[0]]).all() and (nrm[at] == nrm[at[0]]).all()
    # without the flag: no vertex, and -0 welds with +0
    flags = a["flags"].copy()
    flags[::2] &= ~HAS_NORMALS
    cv2, nv2 = weld_np(a["pos"], a["nrm"], flags)
    assert (cv2.reshape(-1, 3)[::2] == -1).all() and (cv2.reshape(-1, 3)[1::2] >= 0).all()
    p0 = np.zeros((2, 9), np.float32)
    p1 = p0.copy()
    p1[1, 0] = -0.0
    n = np.tile(np.float32([0, 1, 0]), (2, 3))
    f = np.full(2, HAS_NORMALS, np.int32)
    assert weld_np(p1, n, f)[1] == weld_np(p0, n, f)[1] == 1


@pytest.mark.parametrize("scene", sorted(COUNTS))
def test_rest_pose_recompute_agrees_with_the_stored_normals(scenes, scene):
    """Cosine >= 0.998 on every corner: the stored normals are area-weighted sums in double, the rule sums up to
    64 crosses in fp32; the measured worst is 0.998663, at the UV sphere's pole. No vertex is degenerate."""
    a, cv, nv = scenes[scene]
    got, (smooth, first, kept) = recompute_np(a["pos"], cv, nv, a["nrm"])
    assert (first, kept) == (0, 0) and smooth == cv.size
    stored = a["nrm"].reshape(-1, 3).astype(np.float64)
    cos = (got.reshape(-1, 3).astype(np.float64) * stored).sum(1) / np.linalg.norm(stored, axis=1)
    print(f"scene {scene}: worst cosine {cos.min():.6f}, 1st percentile {np.percentile(cos, 1):.6f}")
    assert cos.min() >= 0.998
    assert np.abs(np.linalg.norm(got.reshape(-1, 3).astype(np.float64), axis=1) - 1).max() <= 1e-6


def test_adversarial_cases_reach_both_fallbacks(scenes):
    """The GPU suite compares the device with recompute_np on this geometry; here, that it takes every branch
    of the rule: a vertex whose sum cannot be normalised over a triangle that can, and a corner whose triangle
    cannot either. bvh_cases' geometry reaches only the second of the two (degenerate_mix, two_scales: a
    collapsed triangle alone at its vertices); mirrored_pairs is there for the first."""
    reached = np.zeros(3, np.int64)
    cases = dict(bvh_cases.CASES, mirrored_pairs=mirrored_pairs)
    for scene in (0, 1):
        a, cv, nv = scenes[scene]
        base = a["pos"].reshape(-1, 3, 3)
        for case in sorted(cases):
            _, counts = recompute_np(cases[case](base, 0), cv, nv, a["nrm"])
            print(f"scene {scene} {case}: (vertex, own triangle, kept) = {counts}")
            reached += counts
    assert (reached > 0).all(), reached
