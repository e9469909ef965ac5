"""GPU suite for the stream-ordered rebuild (fr_rebuild_bvh_enqueue, fr_bvh_rebuild_status): the context's builder
on a fixed launch schedule, behind enqueued updates and beside pipelined frames, against the synchronous
fr_rebuild_bvh at the same point of the stream order.

Context A enqueues (update or pose, then the rebuild) and renders untimed fr_frame with no synchronising call in
between; its twin takes the same arrays through the synchronous calls. Compared: the tree (the host builder's on a
builder-2 context; canonical_tree form between two device builds), the three exported numbers, the SAH cost and
the frames' buffers by bytes. Sizes and helpers are the neighbouring suites'."""
import numpy as np
import pytest

import bvh_cases
import bvh_np
import motion_np as mn
import test_gpu_pose as tp
from bvh_canon_np import geometric, scene_rebuild_over
from bvh_refit_np import canonical_tree, refit_np
from helpers import equal_nan
from test_gpu_bvh import make_tracer, mismatch_report, tree_bytes
from test_gpu_bvh_sah import SAH, assert_tree_is_hosts, host_scene, numbers, sine
from test_gpu_geometry_overlap import addresses
from test_gpu_update_enqueue import dev, mk, settle, sync_update

pytestmark = pytest.mark.gpu

W, H = 64, 48


def frame_ids(fovrt):
    TN = fovrt.TextureName
    return (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.WEIGHT, TN.SHADING, TN.HISTORY_CACHE, TN.ATROUS)


def assert_same_frames(fovrt, a, b, what):
    for tid in frame_ids(fovrt):
        x, y = a.read(tid), b.read(tid)
        assert equal_nan(x, y), (what, tid, mismatch_report(x, y))
    sa, sb = a.stats(), b.stats()
    assert sa["segments"] == sb["segments"], what
    assert sa["overflow"] == 0 and sb["overflow"] == 0, what


def assert_same_canonical_tree(fovrt, a, b, what):
    ta, tb = bvh_np.read_tree(fovrt, a), bvh_np.read_tree(fovrt, b)
    for name, x, y in zip(("nodes", "tri_geo", "prim"), canonical_tree(*ta), canonical_tree(*tb)):
        assert x.tobytes() == y.tobytes(), (what, name)
    assert numbers(a.scene_arrays()) == numbers(b.scene_arrays()), what


def base_of(t):
    return t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()


# ---------------------------------------------------------------------------------------------
# 1. The tree is the host builder's (builder 2)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
def test_enqueued_rebuild_is_the_host_builders_tree(fovrt_mod, overlap):
    t = make_tracer(fovrt_mod, W, H, 1, SAH, mask=4, spp=2)
    t.set_geometry_overlap(overlap)
    pos = sine(base_of(t), 1.0, amp=0.1)
    host = host_scene(fovrt_mod, 1)
    assert scene_rebuild_over(fovrt_mod, host, pos) == 0
    xyz = dev(pos)
    settle()
    t.frame(timing=False)
    t.update_geometry_enqueue(xyz)
    t.rebuild_bvh_enqueue()
    t.frame(timing=False)
    assert_tree_is_hosts(fovrt_mod, t, host, f"enqueued rebuild, overlap={overlap}")
    print(bvh_np.check_tracer_tree(fovrt_mod, t))
    assert t.bvh_rebuild_status() == (1, 0)
    assert t.geometry_update_status() == (1, 0)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Adversarial geometry (builder 2), fed by an enqueued update and an enqueued rebuild
# ---------------------------------------------------------------------------------------------
def adversarial(fovrt, scene, make_pos, what):
    t = make_tracer(fovrt, W, H, scene, SAH)
    pos = make_pos(base_of(t))
    host = host_scene(fovrt, scene)
    assert scene_rebuild_over(fovrt, host, pos) == 0, "the input must take no median fallback on the host"
    xyz = dev(pos)
    settle()
    t.update_geometry_enqueue(xyz)
    t.rebuild_bvh_enqueue()
    leaf_max = max(2, int(bvh_np.scene_tree(fovrt, host)[0]["count"].max()))
    assert_tree_is_hosts(fovrt, t, host, what)
    out = bvh_np.check_tracer_tree(fovrt, t, leaf_max=leaf_max)
    print(f"{what}: {out} leaf_max {leaf_max}")
    assert t.bvh_rebuild_status() == (1, 0)
    t.destroy()
    return leaf_max


@pytest.mark.parametrize("case", sorted(bvh_cases.CASES))
def test_adversarial_enqueued_rebuild_is_the_host_builders(fovrt_mod, case):
    adversarial(fovrt_mod, 0, lambda base: bvh_cases.CASES[case](base, 0), case)


def test_depth_30_enqueued_rebuild_is_the_host_builders(fovrt_mod):
    """bvh_canon_np.geometric reaches depth 30: the fixed schedule's last level."""
    assert adversarial(fovrt_mod, 1, geometric, "geometric") > 2, "the geometry does not reach depth 30"


# ---------------------------------------------------------------------------------------------
# 3. Builders 0 and 1: the LBVH in stream order
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_enqueued_lbvh_rebuild_equals_the_synchronous_one(fovrt_mod, builder):
    a, b = make_tracer(fovrt_mod, W, H, 1, builder), make_tracer(fovrt_mod, W, H, 1, builder)
    if builder == 0:
        a.rebuild_bvh()  # the first device build makes the arrays an enqueued one needs
    xyz = dev(sine(base_of(a), 2.0, amp=0.1))
    settle()
    a.update_geometry_enqueue(xyz)
    a.rebuild_bvh_enqueue()
    sync_update(b, xyz, "keep")
    b.rebuild_bvh()
    assert_same_canonical_tree(fovrt_mod, a, b, f"builder {builder}")
    ca, cb = a.bvh_sah_cost(), b.bvh_sah_cost()
    print(f"builder {builder}: SAH cost enqueued {ca} synchronous {cb}")
    assert abs(ca - cb) <= 1e-4 * cb
    bvh_np.check_tracer_tree(fovrt_mod, a)
    assert a.bvh_rebuild_status() == (1, 0)
    a.destroy(); b.destroy()


def test_builder_0_before_its_first_device_build_is_refused(fovrt_mod):
    t = make_tracer(fovrt_mod, W, H, 1, 0)
    before, nums = tree_bytes(fovrt_mod, t), numbers(t.scene_arrays())
    with pytest.raises(fovrt_mod.FovrtError) as e:
        t.rebuild_bvh_enqueue()
    assert e.value.code == fovrt_mod.FR_E_STATE
    assert "fr_rebuild_bvh" in t.last_error(), t.last_error()
    assert tree_bytes(fovrt_mod, t) == before and numbers(t.scene_arrays()) == nums
    assert t.bvh_rebuild_status() == (0, 0)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. A refit over a tree the host has not seen
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("builder", [1, SAH])
def test_refit_behind_an_enqueued_rebuild_takes_the_node_count_from_the_device(fovrt_mod, builder, overlap):
    a, twin = make_tracer(fovrt_mod, W, H, 1, builder), make_tracer(fovrt_mod, W, H, 1, builder)
    a.set_geometry_overlap(overlap)
    base = base_of(a)
    n0 = a.scene_arrays()["bvh_nodes"]
    chosen = None
    for amp in (0.1, 0.2, 0.3, 0.4):  # the first deformation whose rebuilt tree has another node count (the twin says)
        xyz1 = dev(sine(base, 1.0, amp=amp))
        settle()
        sync_update(twin, xyz1, "keep")
        twin.rebuild_bvh()
        if twin.scene_arrays()["bvh_nodes"] != n0:
            chosen = xyz1
            break
    assert chosen is not None, "no deformation changed the node count: a stale host count could pass"
    xyz2 = dev(sine(base, 2.0, amp=0.05))
    settle()
    a.update_geometry_enqueue(chosen)
    a.rebuild_bvh_enqueue()
    a.update_geometry_enqueue(xyz2)
    a.synchronize()
    sync_update(twin, xyz2, "keep")
    assert a.scene_arrays()["bvh_nodes"] != n0
    assert_same_canonical_tree(fovrt_mod, a, twin, f"builder {builder} overlap={overlap}")
    bvh_np.check_tracer_tree(fovrt_mod, a)
    assert a.geometry_update_status() == (2, 0) and a.bvh_rebuild_status() == (1, 0)
    a.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("latency", [False, True])
def test_update_and_rebuild_before_every_pipelined_frame(fovrt_mod, latency, overlap, motion):
    a, b = mk(fovrt_mod, motion, SAH, latency=latency), mk(fovrt_mod, motion, SAH, latency=latency)
    a.set_geometry_overlap(overlap)
    base = base_of(a)
    xyz = [dev(mn.sine(base, f)) for f in range(4)]
    settle()
    for f in range(4):
        a.update_geometry_enqueue(xyz[f], normals="recompute")
        a.rebuild_bvh_enqueue()
        a.frame(timing=False)
        sync_update(b, xyz[f], "recompute")
        b.rebuild_bvh()
        b.frame(timing=False)
        if f >= 2:
            assert_same_frames(fovrt_mod, a, b, f"frame {f} latency={latency} overlap={overlap} motion={motion}")
    assert a.bvh_rebuild_status() == (4, 0) and a.geometry_update_status() == (4, 0)
    for k in ("pos", "nrm", "bbox"):
        assert a.scene_arrays()[k].tobytes() == b.scene_arrays()[k].tobytes(), k
    assert numbers(a.scene_arrays()) == numbers(b.scene_arrays())
    a.destroy(); b.destroy()


@pytest.mark.parametrize("overlap", [False, True])
def test_pose_and_rebuild_before_every_pipelined_frame(fovrt_mod, overlap):
    a, b = tp.mk(fovrt_mod, 1, builder=1, motion=True), tp.mk(fovrt_mod, 1, builder=1, motion=True)
    a.set_geometry_overlap(overlap)
    pos0, _, _ = tp.rest(a)
    models = a.models()
    ms = [tp.pose("turning", pos0, models, f) for f in range(4)]
    for f in range(4):
        a.set_model_transforms(ms[f], enqueue=True)
        a.rebuild_bvh_enqueue()
        a.frame(timing=False)
        b.set_model_transforms(ms[f], update="refit")
        b.rebuild_bvh()
        b.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, f"pose {f} overlap={overlap}")
    assert a.bvh_rebuild_status() == (4, 0) and a.geometry_update_status() == (4, 0)
    assert_same_canonical_tree(fovrt_mod, a, b, "poses")
    a.destroy(); b.destroy()


@pytest.mark.parametrize("overlap", [False, True])
def test_two_rebuilds_and_an_update_before_one_gbuffer(fovrt_mod, overlap):
    a, b = mk(fovrt_mod, True, SAH), mk(fovrt_mod, True, SAH)
    a.set_geometry_overlap(overlap)
    base = base_of(a)
    xyz = [dev(mn.sine(base, f)) for f in range(2)]
    settle()
    for f in range(2):
        a.rebuild_bvh_enqueue()
        a.update_geometry_enqueue(xyz[f], normals="recompute")
        a.rebuild_bvh_enqueue()
        a.frame(timing=False)
        b.rebuild_bvh()
        sync_update(b, xyz[f], "recompute")
        b.rebuild_bvh()
        b.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, f"round {f} overlap={overlap}")
    assert a.bvh_rebuild_status() == (4, 0)
    assert numbers(a.scene_arrays()) == numbers(b.scene_arrays())
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 6. A build that fails on the device (builder 2): finite positions whose every SAH area overflows
# ---------------------------------------------------------------------------------------------
def overflowing_positions(fovrt, host, base):
    """base * 2^e for the first e >= 65 at which the host builder reports a median fallback (the device builder's
    documented failure): the hook is the condition, not the constant."""
    for e in range(65, 100):
        pos = (base * np.float32(2.0 ** e)).astype(np.float32)
        if np.isfinite(pos).all() and scene_rebuild_over(fovrt, host, pos) >= 1:
            return pos
    raise AssertionError("no power of two makes the host builder fall back to a median")


@pytest.mark.parametrize("overlap", [False, True])
def test_build_that_fails_on_the_device_keeps_the_tree(fovrt_mod, overlap):
    a, ref = mk(fovrt_mod, False, SAH), mk(fovrt_mod, False, SAH)
    a.set_geometry_overlap(overlap)
    base = base_of(a)
    host = host_scene(fovrt_mod, 1)
    bad = overflowing_positions(fovrt_mod, host, base)
    good = mn.sine(base, 1.0)
    assert scene_rebuild_over(fovrt_mod, host, good) == 0
    nodes0, _, prim0 = bvh_np.read_tree(fovrt_mod, a)
    nums = numbers(a.scene_arrays())
    d_bad, d_good = dev(bad), dev(good)
    settle()
    a.update_geometry_enqueue(d_bad)
    a.rebuild_bvh_enqueue()
    assert a.geometry_update_status() == (1, 0)
    assert a.bvh_rebuild_status() == (0, 1)
    assert "SAH" in a.last_error() and "finite" in a.last_error(), a.last_error()
    nodes, tri, prim = bvh_np.read_tree(fovrt_mod, a)
    want_nodes, want_tri = refit_np(nodes0, prim0, bad)
    assert prim.tobytes() == prim0.tobytes()
    assert nodes.tobytes() == want_nodes.tobytes() and tri.tobytes() == want_tri.tobytes()
    assert numbers(a.scene_arrays()) == nums
    a.update_geometry_enqueue(d_good, normals="recompute")
    a.rebuild_bvh_enqueue()
    sync_update(ref, d_good, "recompute")
    ref.rebuild_bvh()
    for f in range(2):
        a.frame(timing=False)
        ref.frame(timing=False)
        assert_same_frames(fovrt_mod, a, ref, f"frame {f} after the failed build, overlap={overlap}")
    assert a.bvh_rebuild_status() == (1, 1) and a.geometry_update_status() == (2, 0)
    assert_tree_is_hosts(fovrt_mod, a, host, "good rebuild after the failed one")
    a.destroy(); ref.destroy()


# ---------------------------------------------------------------------------------------------
# 7. Refusals
# ---------------------------------------------------------------------------------------------
def test_group_ranks_and_sharded_contexts_are_refused(fovrt_mod):
    a, other = mk(fovrt_mod, False, 1), mk(fovrt_mod, False, 1)
    before = {t: (tree_bytes(fovrt_mod, t), addresses(fovrt_mod, t)) for t in (a, other)}
    g = fovrt_mod.Group([a, other], views=1, tile=64)
    for t in (a, other):
        with pytest.raises(fovrt_mod.FovrtError) as e:
            t.rebuild_bvh_enqueue()
        assert e.value.code == fovrt_mod.FR_E_UNSUPPORTED and "group" in t.last_error()
    g.destroy()
    other.set_shard_plan(0, 2, 32, fovrt_mod.shard_plan(160, 96, 32, 2))
    with pytest.raises(fovrt_mod.FovrtError) as e:
        other.rebuild_bvh_enqueue()
    assert e.value.code == fovrt_mod.FR_E_UNSUPPORTED and "sharded" in other.last_error()
    for t in (a, other):
        assert t.bvh_rebuild_status() == (0, 0)
        assert (tree_bytes(fovrt_mod, t), addresses(fovrt_mod, t)) == before[t]
    a.rebuild_bvh_enqueue()  # free again
    assert a.bvh_rebuild_status() == (1, 0)
    a.destroy(); other.destroy()


# ---------------------------------------------------------------------------------------------
# 8. The call does not wait
# ---------------------------------------------------------------------------------------------
def test_enqueued_rebuild_returns_before_its_input_exists(fovrt_mod):
    """The positions are produced on a side stream behind test_gpu_update_enqueue's ballast chain, made longer (64
    passes over 512 MiB: 64 GiB of traffic, 15 ms and more on this GPU, against the one to three milliseconds of
    host time the rebuild's few hundred launches take; the parent's update enqueue alone is a dozen launches) and
    the update waits for them on the device (ready_event); the rebuild is enqueued behind it. When the rebuild call
    returns the producer's event must still be incomplete: a call that waited for its own work would have waited for
    the producer. An event already complete then says nothing (the ballast was too short for this machine): the
    test skips with that reason rather than passing."""
    import torch
    a, twin = mk(fovrt_mod, False, SAH), mk(fovrt_mod, False, SAH)
    pos = mn.sine(base_of(a), 1.0)
    src = dev(pos)
    buf = torch.empty_like(src)
    ballast = torch.ones(128 << 20, device="cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    settle()
    with torch.cuda.stream(side):
        for _ in range(64):
            ballast.mul_(1.0001)
        buf.copy_(src)
        ev = torch.cuda.Event()
        ev.record(side)
    a.update_geometry_enqueue(buf, ready_event=ev)
    a.rebuild_bvh_enqueue()
    still_running = not ev.query()
    a.synchronize()
    settle()
    if not still_running:
        a.destroy(); twin.destroy()
        pytest.skip("the producer's event was complete when the call returned: the ballast did not outlast the enqueue")
    sync_update(twin, src, "keep")
    twin.rebuild_bvh()
    host = host_scene(fovrt_mod, 1)
    assert scene_rebuild_over(fovrt_mod, host, pos) == 0
    assert_tree_is_hosts(fovrt_mod, a, host, "behind the producer")
    assert_same_canonical_tree(fovrt_mod, a, twin, "behind the producer")
    assert a.scene_arrays()["pos"].tobytes() == twin.scene_arrays()["pos"].tobytes()
    assert a.bvh_rebuild_status() == (1, 0)
    a.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 9. No allocation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("builder", [1, SAH])
def test_enqueued_rebuilds_allocate_nothing(fovrt_mod, builder, overlap):
    import torch
    a = mk(fovrt_mod, False, builder)
    a.set_geometry_overlap(overlap)
    base = base_of(a)
    xyz = [dev(mn.sine(base, f)) for f in range(3)]
    a.update_geometry_enqueue(xyz[0])  # (as the neighbouring suites: the runtime's own first-use allocations)
    a.rebuild_bvh_enqueue()
    a.frame(timing=False)
    a.synchronize()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()
    for f in range(10):
        a.update_geometry_enqueue(xyz[f % 3])
        a.rebuild_bvh_enqueue()
    a.synchronize()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info() == before
    assert a.bvh_rebuild_status() == (11, 0)
    bvh_np.check_tracer_tree(fovrt_mod, a)
    a.destroy()


# ---------------------------------------------------------------------------------------------
# 10. Mixed with what exists
# ---------------------------------------------------------------------------------------------
def test_enqueued_rebuilds_mixed_with_the_synchronous_calls(fovrt_mod):
    a, b = mk(fovrt_mod, True, SAH), mk(fovrt_mod, True, SAH)
    base = base_of(a)
    xyz = [dev(mn.sine(base, f)) for f in range(5)]
    settle()

    def frames(what):
        a.frame(timing=False)
        b.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, what)

    def update(f):
        a.update_geometry_enqueue(xyz[f], normals="recompute")
        sync_update(b, xyz[f], "recompute")

    update(0)
    a.rebuild_bvh_enqueue(); b.rebuild_bvh()
    frames("enqueued rebuild")
    update(1)
    a.rebuild_bvh_enqueue(); b.rebuild_bvh()
    snap = a.snapshot()  # right behind the enqueue
    a.restore(snap); b.restore(snap)
    frames("snapshot / restore")
    update(2)
    a.refit_bvh(); b.refit_bvh()  # over a tree whose numbers the host has to fetch first
    frames("synchronous refit")
    a.rebuild_bvh(); b.rebuild_bvh()
    frames("synchronous rebuild")
    update(3)
    a.rebuild_bvh_enqueue(); b.rebuild_bvh()
    frames("enqueued rebuild again")
    for on in (True, False):
        a.set_geometry_overlap(on)
        update(4 if on else 0)
        a.rebuild_bvh_enqueue(); b.rebuild_bvh()
        frames(f"overlap={on}")
    host = host_scene(fovrt_mod, 1)
    assert scene_rebuild_over(fovrt_mod, host, a.scene_arrays()["pos"].reshape(-1, 3, 3)) == 0
    assert_tree_is_hosts(fovrt_mod, a, host, "mixed")
    assert_tree_is_hosts(fovrt_mod, b, host, "mixed, twin")
    ca, cb = a.bvh_sah_cost(), b.bvh_sah_cost()
    assert abs(ca - cb) <= 1e-4 * cb, (ca, cb)
    assert a.bvh_rebuild_status() == (5, 0) and b.bvh_rebuild_status() == (0, 0)
    a.destroy(); b.destroy()
