"""CPU suite for model poses: the model table of the preset scenes (fr_scene_model_count / fr_scene_model_info) and
the sanity of pose_np, the numpy restatement the GPU suite holds fr_set_model_transforms to."""
import ctypes as C

import numpy as np
import pytest

import pose_np as pn

F = np.float32
NAMES = {0: ["ground", "box"], 1: ["ground", "box", "bunny", "earth"],
         2: ["ground", "vokselia_spawn", "box", "bunny", "earth"]}


def scene(fovrt, preset):
    return fovrt.Scene(fovrt.Config(scene=preset, texture_mode=1, detail=1))


# ---------------------------------------------------------------------------------------------
# The model table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", [0, 1, 2])
def test_models_partition_the_triangles_in_order(fovrt_mod, preset):
    sc = scene(fovrt_mod, preset)
    models, ntris = sc.models(), sc.arrays()["flags"].shape[0]
    assert len(models) == {0: 2, 1: 4, 2: 5}[preset]
    assert [name for name, _, _ in models] == NAMES[preset]  # the names add_mesh records
    assert len(models) <= 16  # FR_MAX_MODELS
    at = 0
    for name, first, n in models:
        assert first == at and n > 0, (name, first, n)
        at += n
    assert at == ntris


def test_box_scene_is_fourteen_triangles(fovrt_mod):
    """The GPU suite relies on it: two models inside one wave."""
    assert scene(fovrt_mod, 0).models() == [("ground", 0, 2), ("box", 2, 12)]


def test_bad_model_index_is_refused(fovrt_mod):
    lib = fovrt_mod.load_library()
    sc = scene(fovrt_mod, 1)
    name, first, n, count = C.c_char_p(), C.c_int(-7), C.c_int(-7), C.c_int()
    assert lib.fr_scene_model_count(sc._h, C.byref(count)) == 0 and count.value == 4
    for i in (-1, 4, 1 << 20):
        assert lib.fr_scene_model_info(sc._h, i, C.byref(name), C.byref(first), C.byref(n)) == fovrt_mod.FR_E_INVALID
        assert (first.value, n.value) == (-7, -7)
    assert lib.fr_scene_model_info(None, 0, C.byref(name), C.byref(first), C.byref(n)) == fovrt_mod.FR_E_INVALID
    assert lib.fr_scene_model_count(None, C.byref(count)) == fovrt_mod.FR_E_INVALID
    assert lib.fr_model_count(None, C.byref(count)) == fovrt_mod.FR_E_INVALID
    assert lib.fr_model_info(None, 0, C.byref(name), C.byref(first), C.byref(n)) == fovrt_mod.FR_E_INVALID
    # any output may be NULL
    assert lib.fr_scene_model_info(sc._h, 3, None, None, C.byref(n)) == 0 and n.value > 0
    assert lib.fr_scene_model_info(sc._h, 3, C.byref(name), None, None) == 0 and name.value == b"earth"


def test_pose_calls_refuse_a_null_context(fovrt_mod):
    lib = fovrt_mod.load_library()
    m = (C.c_float * 12)(*pn.IDENTITY)
    assert lib.fr_model_pose_enable(None, 1) == fovrt_mod.FR_E_INVALID
    assert lib.fr_set_model_transforms(None, m, 1, fovrt_mod.FR_BVH_REFIT) == fovrt_mod.FR_E_INVALID
    assert lib.fr_set_model_transforms_enqueue(None, m, 1) == fovrt_mod.FR_E_INVALID
    assert lib.fr_model_transforms(None, m, 1) == fovrt_mod.FR_E_INVALID


# ---------------------------------------------------------------------------------------------
# pose_np
# ---------------------------------------------------------------------------------------------
def soup(n=257, seed=3):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-4, 4, (n, 3, 3)).astype(F)
    nrm = rng.normal(size=(n, 3, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True).astype(F)
    models = [("a", 0, 100), ("b", 100, 57), ("c", 157, n - 157)]
    return pos, nrm, models


def wild_matrix():
    """A rotation about two axes with a non-uniform scale and a translation."""
    A = pn.rotation(1, 33.0).astype(np.float64) @ pn.rotation(0, -71.0).astype(np.float64) @ np.diag([0.5, 3.0, 1.25])
    return pn.about(A, (0.3, -1.0, 2.0), (1.5, -0.25, 7.0))


def test_identity_pose_returns_the_rest_bits():
    pos, nrm, models = soup()
    pos[5, 1, 2] = F(-0.0)
    nrm[150, 0, 0] = F(-0.0)
    ident = pn.identities(3)
    ident[1, 0, 1] = F(-0.0)  # compares equal to the identity
    X, N = pn.pose_np(pos, nrm, models, ident)
    assert X.tobytes() == pos.tobytes() and N.tobytes() == nrm.tobytes()
    assert np.signbit(X[5, 1, 2]) and np.signbit(N[150, 0, 0])
    # and the arithmetic, were it run, would lose the sign: that is why the bypass exists
    nearly = ident.copy()
    nearly[0, 0, 3] = np.finfo(F).tiny  # not the identity; the z row still ends in "+ 0"
    X2, _ = pn.pose_np(pos, nrm, models, nearly)
    assert X2[5, 1, 2] == 0 and not np.signbit(X2[5, 1, 2])


def test_models_are_posed_each_by_its_own_matrix():
    pos, nrm, models = soup()
    m = pn.identities(3)
    m[1] = wild_matrix()
    X, N = pn.pose_np(pos, nrm, models, m)
    for sl in (slice(0, 100), slice(157, None)):
        assert X[sl].tobytes() == pos[sl].tobytes() and N[sl].tobytes() == nrm[sl].tobytes()
    assert not np.array_equal(X[100:157], pos[100:157])
    # triangles without normals keep theirs
    flags = np.full(pos.shape[0], 0x100, np.int32)
    flags[120] = 0
    _, N2 = pn.pose_np(pos, nrm, models, m, flags)
    assert N2[120].tobytes() == nrm[120].tobytes() and N2[121].tobytes() == N[121].tobytes()


def row_sums64(R, v):
    """The rule's sum of every row of R over v in float64, and the largest magnitude that enters or leaves one of
    its operations (the products, the translation when R has one, the running sums)."""
    R, v = np.asarray(R, np.float64), np.asarray(v, np.float64)
    prod = v[..., None, :] * R[:, :3]
    s1 = prod[..., 0] + prod[..., 1]
    s2 = s1 + prod[..., 2]
    parts = [np.abs(prod).max(-1), np.abs(s1), np.abs(s2)]
    out = s2
    if R.shape[1] == 4:
        out = s2 + R[:, 3]
        parts += [np.broadcast_to(np.abs(R[:, 3]), out.shape), np.abs(out)]
    return out, np.maximum.reduce(parts)


def test_rule_agrees_with_float64_within_four_ulp_of_the_largest_term():
    """The unit is the float32 spacing at the largest magnitude among the terms of a sum and its running sums: a
    position takes six rounded operations and a normal five, each off by at most half a spacing of its own result,
    so 3 and 2.5 of these units bound the error and 4 holds with room. (Measured against the spacing at the largest
    product or translation alone, the position's last additions, whose results can be up to four times that term,
    take the worst corner of this sample to 4.004; no bound of 4 holds for the rule in that unit.) The normal's
    float64 evaluation uses the rule's float32 cofactors, which the next test holds to det A^-T."""
    pos, nrm, _ = soup(n=2000)
    M = wild_matrix()
    X, N = pn.pose_np(pos, nrm, [("all", 0, pos.shape[0])], M[None])
    K, _ = pn.cofactors(M)
    worst = {}
    for name, got, R, v in (("positions", X, M, pos), ("normals", N, K, nrm)):
        want, largest = row_sums64(R, v)
        ulps = np.abs(got.astype(np.float64) - want) / np.spacing(largest.astype(F)).astype(np.float64)
        worst[name] = float(ulps.max())
    print("worst error in ulp of the largest term:", worst)
    assert worst["positions"] <= 4.0 and worst["normals"] <= 4.0
    assert worst["positions"] > 0.0  # float32 did round


def test_cofactors_are_det_times_the_inverse_transpose():
    M = wild_matrix()
    K, det = pn.cofactors(M)
    A = M[:, :3].astype(np.float64)
    assert det > 0 and np.isclose(det, np.linalg.det(A), rtol=1e-5)
    assert np.allclose(K.astype(np.float64) @ A.T, float(det) * np.eye(3), atol=1e-5 * abs(float(det)))
    assert np.allclose(K, np.linalg.det(A) * np.linalg.inv(A).T, rtol=1e-4, atol=1e-5)
    # a mirror has a negative determinant, a flattened model none
    assert pn.cofactors(np.diag([1.0, -1.0, 1.0, 0.0])[:3])[1] < 0
    assert pn.cofactors(np.diag([1.0, 0.0, 1.0, 0.0])[:3])[1] == 0
    # 90 degrees: exact zeros and ones
    R = pn.rotation(2, 90.0)
    assert set(np.abs(R).ravel().tolist()) == {0.0, 1.0}
    assert pn.cofactors(np.concatenate([R, np.zeros((3, 1), F)], 1))[1] == 1.0
