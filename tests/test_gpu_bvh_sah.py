"""GPU suite for the device binned-SAH builder (fr_config.bvh_builder = 2, k_bvh_sah.hip): its tree is the host
builder's tree over the same positions, up to the numbering of the nodes of a level and the order inside a leaf
(bvh_canon_np.canonical removes both), on the presets and on bvh_cases' adversarial geometry; frames over it are
builder 0's; and what follows a build (refit, enqueued and overlapped updates, updates from device memory, a
rejected update) works over this tree as over the others.
"""
import numpy as np
import pytest

import bvh_cases
import bvh_np
from bvh_canon_np import canonical, geometric, scene_rebuild_over
from bvh_refit_np import canonical_tree, refit_np
from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan
from test_gpu_bvh import GBUFFER, case_reference, make_tracer, mismatch_report, tree_bytes

pytestmark = pytest.mark.gpu

NUMBERS = ("bvh_nodes", "bvh_depth", "bvh_max_stack")
W, H = 64, 48
SAH = 2

_host = {}


def host_scene(fovrt, scene):
    """The host-only twin of a preset (one per scene; scene_rebuild_over moves it)."""
    if scene not in _host:
        _host[scene] = fovrt.Scene(fovrt.Config(scene=scene, texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, detail=1))
    return _host[scene]


def numbers(arrays):
    return {k: arrays[k] for k in NUMBERS}


def assert_tree_is_hosts(fovrt, t, host, what):
    """The tracer's tree against the host scene's: canonical form and the three exported numbers."""
    nodes, _, prim = bvh_np.read_tree(fovrt, t)
    hn, _, hp = bvh_np.scene_tree(fovrt, host)
    got, want = canonical(nodes, prim), canonical(hn, hp)
    assert got.shape == want.shape and np.array_equal(got, want), (
        what, got.shape, want.shape, int(np.argmax(got[:min(got.size, want.size)] != want[:min(got.size, want.size)])))
    assert numbers(t.scene_arrays()) == numbers(host.arrays()), what


def sine(base, f, amp=0.05):
    pos = base.copy()
    pos[..., 1] += np.float32(amp) * np.sin(np.float32(3.0) * base[..., 0] + np.float32(f)).astype(np.float32)
    return pos


# ---------------------------------------------------------------------------------------------
# 1. The builder exists (fr_create answered "bad bvh_builder" before it did)
# ---------------------------------------------------------------------------------------------
def test_builder_2_initialises(fovrt_mod):
    t = fovrt_mod.PathTracer(fovrt_mod.Config(width=W, height=H, scene=1, texture_mode=TEXTURE_MODE,
                                              asset_dir=ASSET_DIR, detail=1, bvh_builder=SAH))
    assert t.initialize(), t.last_error()
    assert t.scene_arrays()["bvh_nodes"] > 1
    t.destroy()
    bad = fovrt_mod.PathTracer(fovrt_mod.Config(width=W, height=H, scene=1, texture_mode=TEXTURE_MODE,
                                                asset_dir=ASSET_DIR, detail=1, bvh_builder=3))
    with pytest.raises(fovrt_mod.FovrtError) as e:
        bad.initialize()
    assert e.value.code == fovrt_mod.FR_E_INVALID


# ---------------------------------------------------------------------------------------------
# 2. The presets: fr_create's tree and fr_rebuild_bvh's (the spare arrays') are the host's
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [0, 1, 2])
def test_preset_tree_is_the_host_builders(fovrt_mod, scene):
    t = make_tracer(fovrt_mod, W, H, scene, SAH)
    host = host_scene(fovrt_mod, scene)
    pos = t.scene_arrays()["pos"]
    assert scene_rebuild_over(fovrt_mod, host, pos) == 0  # (the twin may have been moved by another test)
    out = bvh_np.check_tracer_tree(fovrt_mod, t)
    print(f"scene {scene}: {out}")
    assert_tree_is_hosts(fovrt_mod, t, host, "fr_create")
    assert t.rebuild_bvh() > 0.0
    assert bvh_np.check_tracer_tree(fovrt_mod, t) == out
    assert_tree_is_hosts(fovrt_mod, t, host, "fr_rebuild_bvh")
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Adversarial geometry through fr_set_positions: the host's tree, and the oracle's G-buffer over it
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(bvh_cases.CASES))
@pytest.mark.parametrize("scene", [0, 1])
def test_adversarial_tree_is_the_host_builders(fovrt_mod, oracle, scene, case):
    TN = fovrt_mod.TextureName
    w, h = (32, 24) if case == "identical" else (W, H)  # identical: every ray tests every triangle
    t = make_tracer(fovrt_mod, w, h, scene, SAH)
    pos, ref = case_reference(fovrt_mod, oracle, t, scene, case, w, h)
    host = host_scene(fovrt_mod, scene)
    assert scene_rebuild_over(fovrt_mod, host, pos) == 0
    t.set_positions(pos)
    assert np.array_equal(t.scene_arrays()["pos"].reshape(-1, 3, 3), pos)
    leaf_max = max(2, int(bvh_np.scene_tree(fovrt_mod, host)[0]["count"].max()))
    out = bvh_np.check_tracer_tree(fovrt_mod, t, leaf_max=leaf_max)
    print(f"scene {scene} {case}: {out}")
    assert_tree_is_hosts(fovrt_mod, t, host, case)
    for pose, (uni, g) in ref.items():
        t.reset_accumulation()
        assert t.m_accumFrame == 0
        t.set_camera_uniforms(uni)
        t.geometry_launch()
        for name, tid in zip(GBUFFER, (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE)):
            got = t.read(tid)
            assert equal_nan(got, g[name]), (pose, name, mismatch_report(got, g[name]))
    assert t.stats()["overflow"] == 0
    t.destroy()


def test_depth_30_leaves_are_the_host_builders(fovrt_mod):
    """A collinear geometric comb 125 scales deep: the binary tree reaches depth 30, whose nodes are leaves of more than two
    triangles (bvh_cases' comb does not get there under binned SAH)."""
    t = make_tracer(fovrt_mod, W, H, 1, SAH)
    pos = geometric(t.scene_arrays()["pos"].reshape(-1, 3, 3))
    host = host_scene(fovrt_mod, 1)
    assert scene_rebuild_over(fovrt_mod, host, pos) == 0
    leaf_max = int(bvh_np.scene_tree(fovrt_mod, host)[0]["count"].max())
    assert leaf_max > 2, "the geometry does not reach depth 30 on the host"
    t.set_positions(pos)
    out = bvh_np.check_tracer_tree(fovrt_mod, t, leaf_max=leaf_max)
    print(f"geometric: {out} leaf_max {leaf_max}")
    assert_tree_is_hosts(fovrt_mod, t, host, "geometric")
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Frames over this tree are builder 0's, in both pipeline modes; the SAH cost agrees
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_frames_equal_host_built(fovrt_mod, mode):
    TN = fovrt_mod.TextureName
    host = make_tracer(fovrt_mod, 160, 96, 1, 0, mask=4, spp=2, dmd=2)
    dev = make_tracer(fovrt_mod, 160, 96, 1, SAH, mask=4, spp=2, dmd=2)
    for t in (host, dev):
        t.set_pipeline_mode(mode)
    for _ in range(3):
        host.frame(timing=False)
        dev.frame(timing=False)
    for tid in (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.SHADING, TN.HISTORY_CACHE, TN.ATROUS):
        assert equal_nan(dev.read(tid), host.read(tid)), tid
    assert dev.stats()["segments"] == host.stats()["segments"]
    ch, cd = host.bvh_sah_cost(), dev.bvh_sah_cost()
    print(f"SAH cost host {ch} device {cd}")
    assert abs(cd - ch) <= 1e-4 * ch
    host.destroy(); dev.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Downstream over this tree
# ---------------------------------------------------------------------------------------------
def test_refit_over_the_device_tree(fovrt_mod):
    t = make_tracer(fovrt_mod, W, H, 1, SAH)
    base = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    nodes0, _, prim0 = bvh_np.read_tree(fovrt_mod, t)
    before = numbers(t.scene_arrays())
    pos = sine(base, 1.0, amp=0.1)
    t.set_positions(pos, update="refit")
    nodes, tri, prim = bvh_np.read_tree(fovrt_mod, t)
    want_nodes, want_tri = refit_np(nodes0, prim0, pos)
    assert prim.tobytes() == prim0.tobytes()
    assert nodes.tobytes() == want_nodes.tobytes() and tri.tobytes() == want_tri.tobytes()
    assert numbers(t.scene_arrays()) == before
    bvh_np.check_tracer_tree(fovrt_mod, t)
    t.destroy()


def test_enqueued_overlapped_update_equals_the_synchronous_one(fovrt_mod):
    import torch
    TN = fovrt_mod.TextureName
    a = make_tracer(fovrt_mod, W, H, 1, SAH, mask=4, spp=2)
    b = make_tracer(fovrt_mod, W, H, 1, SAH, mask=4, spp=2)
    a.set_geometry_overlap(True)
    nodes0, _, prim0 = bvh_np.read_tree(fovrt_mod, a)
    base = a.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    pos = sine(base, 2.0, amp=0.1)
    dev = torch.from_numpy(pos.reshape(-1, 9)).to("cuda:0")
    torch.cuda.synchronize()
    a.frame(timing=False); b.frame(timing=False)
    a.update_geometry_enqueue(dev)
    b.set_positions_device(dev.data_ptr(), pos.shape[0], update="refit")
    a.frame(timing=False); b.frame(timing=False)
    a.synchronize(); b.synchronize()
    assert a.geometry_update_status() == (1, 0)
    # two contexts' builds number the nodes of a level differently: the same bytes once both are renumbered, and
    # over this context's own numbering the refit's one right answer
    ta, tb = bvh_np.read_tree(fovrt_mod, a), bvh_np.read_tree(fovrt_mod, b)
    for name, x, y in zip(("nodes", "tri_geo", "prim"), canonical_tree(*ta), canonical_tree(*tb)):
        assert x.tobytes() == y.tobytes(), name
    want_nodes, want_tri = refit_np(nodes0, prim0, pos)
    assert ta[0].tobytes() == want_nodes.tobytes() and ta[1].tobytes() == want_tri.tobytes()
    assert ta[2].tobytes() == prim0.tobytes()
    for tid in (TN.POSITION, TN.NORMAL, TN.SHADING, TN.ATROUS):
        assert equal_nan(a.read(tid), b.read(tid)), tid
    bvh_np.check_tracer_tree(fovrt_mod, a)
    a.destroy(); b.destroy()


def test_rebuild_from_device_memory_is_the_host_builders(fovrt_mod):
    import torch
    t = make_tracer(fovrt_mod, W, H, 1, SAH)
    pos = sine(t.scene_arrays()["pos"].reshape(-1, 3, 3).copy(), 1.0, amp=0.2)
    host = host_scene(fovrt_mod, 1)
    assert scene_rebuild_over(fovrt_mod, host, pos) == 0
    dev = torch.from_numpy(pos.reshape(-1, 9)).to("cuda:0")
    torch.cuda.synchronize()
    t.set_positions_device(dev.data_ptr(), pos.shape[0], update="rebuild", normals="recompute")  # fr_update_geometry
    assert np.array_equal(t.scene_arrays()["pos"].reshape(-1, 3, 3), pos)
    bvh_np.check_tracer_tree(fovrt_mod, t)
    assert_tree_is_hosts(fovrt_mod, t, host, "fr_update_geometry, device memory, FR_BVH_REBUILD")
    t.destroy()


def test_rejected_update_leaves_the_tree_alone(fovrt_mod):
    t = make_tracer(fovrt_mod, W, H, 1, SAH)
    before, nums = tree_bytes(fovrt_mod, t), numbers(t.scene_arrays())
    bad = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    bad[bad.shape[0] // 2, 1, 2] = np.nan
    with pytest.raises(fovrt_mod.FovrtError) as e:
        t.set_positions(bad)
    assert e.value.code == fovrt_mod.FR_E_INVALID
    assert tree_bytes(fovrt_mod, t) == before
    assert numbers(t.scene_arrays()) == nums
    bvh_np.check_tracer_tree(fovrt_mod, t)
    t.destroy()


def test_rebuilds_allocate_nothing(fovrt_mod):
    import torch
    t = make_tracer(fovrt_mod, W, H, 1, SAH)
    t.rebuild_bvh()
    t.synchronize()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()
    for _ in range(10):
        assert t.rebuild_bvh() > 0.0
    t.synchronize()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info() == before
    bvh_np.check_tracer_tree(fovrt_mod, t)
    t.destroy()
