"""CPU suite for motion reprojection (fr_set_motion_reprojection): the numpy restatement the GPU suite compares the
kernels with (tests/motion_np.py) against the restatements it extends, and the ABI entry without a device.

With prev == cur the rule must vanish: delta is exactly zero on every hit, so WEIGHT.xy are trace_np.gbuffer_np's
reprojection bits and WEIGHT.z is the distance helpers.sampling_np computes for itself (length(position - prev_eye),
ptx_np.length3). The translated box preset is the condition of the GPU suite's "does what it is for" test: the
restatement alone, with the oracle's depth of the frame before, must find the history valid on at least 99 % of the
hit pixels."""
import ctypes as C

import numpy as np
import pytest

import motion_np as mn
import ptx_np
import trace_np as tn
from helpers import ASSET_DIR, TEXTURE_MODE, sampling_np


def scene_arrays(fovrt, scene):
    return fovrt.Scene(fovrt.Config(scene=scene, texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, detail=1)).arrays()


@pytest.mark.parametrize("scene,W,H", [(0, 45, 29), (1, 21, 13)])
def test_unmoved_geometry_gives_the_plain_gbuffer_weight(fovrt_mod, scene, W, H):
    a = scene_arrays(fovrt_mod, scene)
    sc = tn.SceneNp(a)
    _, uni = mn.cameras(fovrt_mod, scene, W, H, panned=True)  # prev_vp / prev_eye differ from the current pose
    g = tn.gbuffer_np(sc, uni, W, H, 0)
    m = mn.motion_gbuffer_np(sc, sc.pos.copy(), uni, W, H)
    hit = m["prim"] >= 0
    assert 0.3 < hit.mean() < 1.0  # hits and misses both
    assert np.array_equal(hit, (g["position"][..., :3] != 0).any(-1))
    for ch in (0, 1, 3):
        assert m["weight"][..., ch].tobytes() == g["weight"][..., ch].tobytes(), ch
    assert (m["weight"][~hit] == np.array([-1, -1, 0, 1], np.float32)).all()
    prev_eye = np.array(uni.prev_eye[:], np.float32)
    dist = ptx_np.length3((g["position"][..., :3] - prev_eye).astype(np.float32))
    assert m["weight"][..., 2][hit].tobytes() == np.asarray(dist, np.float32)[hit].tobytes()
    # ... so the motion form of the sampling stage finds the validity the plain one finds
    depth_cache = np.random.default_rng(3).uniform(0, 8, (H, W, 4)).astype(np.float32)
    depth_cache[hit, 0] = dist[hit]  # valid wherever the reprojection lands on a pixel that stores this distance
    _, want, _ = sampling_np(W, H, fovrt_mod.MASK_ALL, (uni.gaze[0], uni.gaze[1]), prev_eye, a["bbox"], g["position"],
                             g["depth"], depth_cache, g["weight"], g["normal"], g["diffuse"])
    got = mn.motion_sampling_weight_np(m["weight"], depth_cache)
    assert got.tobytes() == want.tobytes()


def test_translated_scene_and_camera_keep_their_history(fovrt_mod, oracle):
    """The condition of test_gpu_motion's third test, on the restatement alone."""
    W, H = mn.TRANSLATE_SIZE
    a = scene_arrays(fovrt_mod, 0)
    base, moved = mn.translate_case(a["pos"])
    uni1, uni2 = mn.cameras(fovrt_mod, 0, W, H, panned=False, shift=mn.TRANSLATE)
    depth_cache = oracle.gbuffer(oracle.OracleScene(dict(a, pos=base.reshape(-1, 9))), uni1, W, H, 0)["depth"]
    a2 = dict(a, pos=moved.reshape(-1, 9))
    m = mn.motion_gbuffer_np(tn.SceneNp(a2), base, uni2, W, H)
    w = mn.motion_sampling_weight_np(m["weight"], depth_cache)
    hit = m["prim"] >= 0
    frac = float((w[..., 2][hit] > 0).mean())
    print(f"hit pixels {int(hit.sum())}, valid {frac:.4f}")
    assert hit.sum() > 0.4 * W * H and frac >= 0.99
    # the same frame reprojected as over still geometry (prev == cur) loses it
    still = mn.motion_gbuffer_np(tn.SceneNp(a2), moved, uni2, W, H)
    lost = float((mn.motion_sampling_weight_np(still["weight"], depth_cache)[..., 2][hit] == 0).mean())
    print(f"without the motion: invalid on {lost:.4f}")
    assert lost > 0.5


def test_library_exports_the_entry_and_rejects_a_null_context(fovrt_mod):
    lib = fovrt_mod.load_library()
    assert "fr_set_motion_reprojection" in fovrt_mod._SIGS
    fn = lib.fr_set_motion_reprojection
    assert fn(None, 1) == fovrt_mod.FR_E_INVALID
    assert fn(C.c_void_p(0), 0) == fovrt_mod.FR_E_INVALID
    assert hasattr(fovrt_mod.PathTracer, "set_motion_reprojection")
