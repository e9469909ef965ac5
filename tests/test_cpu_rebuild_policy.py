"""CPU suite for the device-triggered rebuild (fr_rebuild_bvh_enqueue_if, fr_set_rebuild_policy,
fr_bvh_rebuild_policy_status): what can be said without a device, and the condition on the inputs of the GPU suite
(test_gpu_rebuild_policy.py).

The device decides by `cost > ratio * baseline`, and its cost is held to the synchronous call's to 1e-4 relative,
so a GPU test may only pose decisions far from the threshold. This file fixes the two deformations those tests use
and checks, on the host builder's trees of scenes 0 and 1 with refit_np and sah_cost_np, that a mild step keeps a
refitted tree within 5 % of its cost when built, and that the grown geometry refits to at least 1.5 times it. The
GPU tests use ratio 1.25: a skip sits below 1.05 / 0.95 = 1.11 of any adopted baseline and a build above 1.5 / 1.05 =
1.43 of it, thousands of times the cost tolerance away from 1.25 on either side."""
import ctypes as C

import numpy as np
import pytest

import bvh_np
from bvh_canon_np import scene_rebuild_over
from bvh_refit_np import refit_np, sah_cost_np
from helpers import ASSET_DIR, TEXTURE_MODE

F = np.float32
NAMES = ("fr_rebuild_bvh_enqueue_if", "fr_set_rebuild_policy", "fr_bvh_rebuild_policy_status")
RATIO = 1.25          # the GPU tests' threshold
MILD_BAND = (0.95, 1.05)  # refitted cost / cost when built, after a mild step
GROWN_MIN = 1.5       # the same quotient over the grown geometry
MILD_STEPS = 9        # the phases f the GPU tests use: 0 .. 8


def mild(base, f, amp=0.05):
    """A small wave along y (test_gpu_bvh_sah.sine): a refitted tree stays as good as it was."""
    pos = np.array(base, F, copy=True).reshape(-1, 3, 3)
    pos[..., 1] += F(amp) * np.sin(F(3.0) * pos[..., 0] + F(f)).astype(F)
    return pos


def grown(base, seed=7, scale=0.3):
    """Every triangle translated rigidly by its own seeded random offset, each component 0.5 to 1.5 times `scale` of
    the scene box's diagonal: the triangles stay what they were, the boxes of a refitted tree grow to the size of
    the scene. Even triangles go one way and odd ones the other, so the two halves of a quad, which a builder puts
    into one leaf, part: with offsets of either sign the 14 triangles of scene 0 refit to 1.3 times the built
    cost only (its floor's leaf, which is the root's box whatever moves, is two thirds of the cost)."""
    pos = np.array(base, F, copy=True).reshape(-1, 3, 3)
    flat = pos.reshape(-1, 3)
    diag = float(np.linalg.norm(flat.max(0).astype(np.float64) - flat.min(0).astype(np.float64)))
    off = np.random.default_rng(seed).uniform(0.5, 1.5, (pos.shape[0], 1, 3)) * (scale * diag)
    off *= np.where(np.arange(pos.shape[0]) % 2 == 0, -1.0, 1.0)[:, None, None]
    return (pos + off.astype(F)).astype(F)


def mild_pose(base, models, f, grow=1.0):
    """Poses for set_model_transforms: every model but the first translated by a few centimetres that grow with f
    (mild: a refitted tree keeps its cost), each scaled by `grow` about its own middle first (grow = 4: the models
    swell inside a scene box that hardly changes, and so does the cost of any tree over them)."""
    import pose_np as pn
    out = []
    for i, (_, first, n) in enumerate(models):
        if i == 0:
            out.append(pn.identities(1)[0])
            continue
        p = np.asarray(base, F).reshape(-1, 3, 3)[first:first + n].reshape(-1, 3).astype(np.float64)
        out.append(pn.about(np.eye(3) * grow, 0.5 * (p.min(0) + p.max(0)), (0.01 * f * (i % 2), 0.0, 0.005 * f)))
    return np.stack(out).astype(F)


def cost_f32(nodes):
    """(sum of the cost terms, root area) in float32, as the device forms them (the order of the sum apart): what
    overflows there overflows here."""
    lo = np.stack([nodes["lox"], nodes["loy"], nodes["loz"]], -1)
    hi = np.stack([nodes["hix"], nodes["hiy"], nodes["hiz"]], -1)
    count = nodes["count"]
    full = count >= 0
    with np.errstate(all="ignore"):
        d = (hi - lo).astype(F)
        area = F(2) * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])
        terms = np.where(full, area * np.where(count > 0, count, 1).astype(F), F(0))
        rd = hi[0][full[0]].max(0) - lo[0][full[0]].min(0)
        return terms.sum(dtype=F), F(2) * (rd[0] * rd[1] + rd[1] * rd[2] + rd[2] * rd[0])


def failing_positions(fovrt, host, nodes0, prim0, base):
    """Positions over which a conditional build is attempted and fails on the device (builder 2): the grown
    geometry, little of it (scale 0.003), times 2^e for the first e at which the host builder reports a median
    fallback (the device builder's documented failure) while the refitted tree's cost is still finite in float32
    with a factor 16 to spare, and at least GROWN_MIN times the built tree's. The hook is the condition."""
    built = sah_cost_np(nodes0)
    g = grown(base, scale=0.003)
    for e in range(50, 60):
        pos = (g * F(2.0 ** e)).astype(F)
        if not np.isfinite(pos).all():
            break
        with np.errstate(all="ignore"):
            total, root = cost_f32(refit_np(nodes0, prim0, pos)[0])
        if not (np.isfinite(total) and float(total) * 16.0 < float(np.finfo(F).max) and root > 0):
            break
        if scene_rebuild_over(fovrt, host, pos) >= 1:
            assert (1.0 + float(total) / float(root)) / built >= GROWN_MIN
            return pos
    raise AssertionError("no power of two makes the host builder fall back to a median under a finite cost")


def test_library_exports_the_three_calls(fovrt_mod):
    lib = fovrt_mod.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in fovrt_mod._SIGS, name  # (test_cpu_abi then demands them of the header)


def test_null_context_is_invalid_without_a_device(fovrt_mod):
    lib = fovrt_mod.load_library()
    assert lib.fr_rebuild_bvh_enqueue_if(None, 1.25) == fovrt_mod.FR_E_INVALID
    assert lib.fr_set_rebuild_policy(None, 1.25, 8) == fovrt_mod.FR_E_INVALID
    e, s = C.c_uint64(7), C.c_uint64(7)
    l, b = C.c_float(7.0), C.c_float(7.0)
    assert lib.fr_bvh_rebuild_policy_status(None, C.byref(e), C.byref(s), C.byref(l), C.byref(b)) == fovrt_mod.FR_E_INVALID
    assert lib.fr_bvh_rebuild_policy_status(None, None, None, None, None) == fovrt_mod.FR_E_INVALID
    assert (e.value, s.value, l.value, b.value) == (7, 7, 7.0, 7.0)


def test_python_facade_has_the_three_methods(fovrt_mod):
    for name in ("rebuild_bvh_enqueue_if", "set_rebuild_policy", "bvh_rebuild_policy_status"):
        assert callable(getattr(fovrt_mod.PathTracer, name, None)), name


@pytest.mark.parametrize("scene", [0, 1])
def test_deformations_decide_far_from_the_threshold(fovrt_mod, scene):
    host = fovrt_mod.Scene(fovrt_mod.Config(scene=scene, texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, detail=1))
    base = host.arrays()["pos"].reshape(-1, 3, 3).copy()
    nodes0, _, prim0 = bvh_np.scene_tree(fovrt_mod, host)
    built = sah_cost_np(nodes0)

    def quotient(nodes, prim, pos, own):
        return sah_cost_np(refit_np(nodes, prim, pos)[0]) / own

    q_mild = [quotient(nodes0, prim0, mild(base, f), built) for f in range(MILD_STEPS)]
    g = grown(base)
    q_grown = quotient(nodes0, prim0, g, built)
    assert scene_rebuild_over(fovrt_mod, host, g) == 0, "the grown geometry must take no median fallback on the host"
    nodes1, _, prim1 = bvh_np.scene_tree(fovrt_mod, host)
    rebuilt = sah_cost_np(nodes1)
    q_after = [quotient(nodes1, prim1, mild(g, f), rebuilt) for f in range(MILD_STEPS)]
    print(f"scene {scene}: cost built {built:.4f}; mild / built {min(q_mild):.4f} .. {max(q_mild):.4f}; "
          f"grown / built {q_grown:.4f}; cost rebuilt over grown {rebuilt:.4f}; "
          f"mild / rebuilt {min(q_after):.4f} .. {max(q_after):.4f}")
    lo, hi = MILD_BAND
    assert lo <= min(q_mild) and max(q_mild) <= hi, q_mild
    assert q_grown >= GROWN_MIN, q_grown
    assert lo <= min(q_after) and max(q_after) <= hi, q_after
    # what the band buys: any mild cost over any mild baseline skips, the grown cost over any mild baseline builds
    assert hi / lo < RATIO * (1.0 - 0.01) and GROWN_MIN / hi > RATIO * (1.0 + 0.01)


def test_pose_and_failing_inputs_of_the_gpu_suite(fovrt_mod):
    """Scene 1: the poses of the policy test decide far from the threshold as well (a swollen scene costs twice the
    rest pose's tree; a few centimetres cost nothing), and a geometry exists over which the device attempts a build
    that fails."""
    import pose_np as pn
    host = fovrt_mod.Scene(fovrt_mod.Config(scene=1, texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, detail=1))
    a = host.arrays()
    base, nrm = a["pos"].reshape(-1, 3, 3).copy(), a["nrm"].reshape(-1, 3, 3).copy()
    models = host.models()
    nodes0, _, prim0 = bvh_np.scene_tree(fovrt_mod, host)
    built = sah_cost_np(nodes0)

    def posed(f, grow=1.0):
        return pn.pose_np(base, nrm, models, mild_pose(base, models, f, grow))[0]

    q_mild = [sah_cost_np(refit_np(nodes0, prim0, posed(f))[0]) / built for f in range(MILD_STEPS)]
    q_grown = sah_cost_np(refit_np(nodes0, prim0, posed(5, 4.0))[0]) / built
    assert scene_rebuild_over(fovrt_mod, host, posed(5, 4.0)) == 0
    nodes1, _, prim1 = bvh_np.scene_tree(fovrt_mod, host)
    rebuilt = sah_cost_np(nodes1)
    q_after = [sah_cost_np(refit_np(nodes1, prim1, posed(f, 4.0))[0]) / rebuilt for f in range(MILD_STEPS)]
    print(f"poses: mild / built {min(q_mild):.4f} .. {max(q_mild):.4f}; grown / built {q_grown:.4f}; "
          f"mild / rebuilt {min(q_after):.4f} .. {max(q_after):.4f}")
    lo, hi = MILD_BAND
    assert lo <= min(q_mild) and max(q_mild) <= hi, q_mild
    assert q_grown >= GROWN_MIN, q_grown
    assert lo <= min(q_after) and max(q_after) <= hi, q_after
    scene_rebuild_over(fovrt_mod, host, base)
    failing_positions(fovrt_mod, host, nodes0, prim0, base)
