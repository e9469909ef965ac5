"""GPU suite for overlapped geometry updates (fr_set_geometry_overlap): enqueued updates that refit into a second
tree and write second normals on the front stages' stream, against the synchronous fr_update_geometry (device
memory, refit), bit for bit.

Context A has overlap on, takes its updates through the enqueued calls and renders untimed fr_frame; context B takes
the same arrays through the synchronous call and renders stage by stage. Everything they leave is compared by bytes:
the frame's buffers, positions, normals, scene box and the tree. The destination of an overlapped update is two
updates old, so the traps are the states in which "write nothing" would have been right in place: FR_NORMALS_KEEP,
a rejected update, a tree another call replaced in between. Sizes and helpers are test_gpu_update_enqueue's."""
import ctypes as C

import numpy as np
import pytest

import bvh_np
import motion_np as mn
import test_gpu_pose as tp
from test_gpu_bvh import tree_bytes
from test_gpu_update_enqueue import (W, H, assert_same_frames, assert_same_state, dev, given_normals, mk, rest,
                                     settle, state, sync_frame, sync_update)

pytestmark = pytest.mark.gpu


def mk_on(fovrt, *args, **kw):
    t = mk(fovrt, *args, **kw)
    t.set_geometry_overlap(True)
    return t


def addresses(fovrt, t):
    """(tree, normals): the device addresses in use (the library's test hook, not in include/fovrt.h)."""
    fn = fovrt.load_library().fr__scene_addresses
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    fn.restype = C.c_int
    nodes, shade = C.c_void_p(), C.c_void_p()
    assert fn(t._ctx, C.byref(nodes), C.byref(shade)) == 0
    return nodes.value, shade.value


def arrays(a, frames, normals="given"):
    """Device positions (and normals) of `frames` updates, prepared before the loop."""
    base, nrm0, _ = rest(a)
    xyz = [dev(mn.sine(base, f)) for f in range(frames)]
    nrm = [dev(given_normals(nrm0, f)) for f in range(frames)] if normals == "given" else [normals] * frames
    settle()
    return xyz, nrm


# ---------------------------------------------------------------------------------------------
# 1. Six frames, an update before each: both sets are the destination three times, every frame slot is reused
# ---------------------------------------------------------------------------------------------
def run_equal(fovrt, latency, motion, normals, builder=0, frames=6):
    a, b = mk_on(fovrt, motion, builder, latency=latency), mk(fovrt, motion, builder)
    xyz, nrm = arrays(a, frames, normals)
    for f in range(frames):
        a.update_geometry_enqueue(xyz[f], normals=nrm[f])
        a.frame(timing=False)
        sync_update(b, xyz[f], nrm[f])
        sync_frame(fovrt, b)
        if f >= frames - 2:  # one frame read each set
            assert_same_frames(fovrt, a, b, f"frame {f}")
    what = f"latency={latency} motion={motion} normals={normals} builder={builder}"
    assert_same_frames(fovrt, a, b, what)
    assert_same_state(fovrt, a, b, what, tree=builder == 0)
    if builder == 1:  # as test_gpu_update_enqueue.run_equal: the structure, and a's bytes against its own refit
        assert bvh_np.check_tracer_tree(fovrt, a) == bvh_np.check_tracer_tree(fovrt, b)
        mine = tree_bytes(fovrt, a)
        a.refit_bvh()
        assert tree_bytes(fovrt, a) == mine, "the out-of-place refit's bytes are not the synchronous refit's"
    assert a.geometry_update_status() == (frames, 0)
    assert b.geometry_update_status() == (0, 0)
    a.destroy(); b.destroy()


@pytest.mark.parametrize("normals", ["keep", "recompute", "given"])
@pytest.mark.parametrize("motion", [True, False])
@pytest.mark.parametrize("latency", [False, True])
def test_overlapped_updates_equal_synchronous_updates(fovrt_mod, latency, motion, normals):
    run_equal(fovrt_mod, latency, motion, normals)


def test_overlapped_updates_equal_synchronous_updates_on_a_device_built_tree(fovrt_mod):
    run_equal(fovrt_mod, False, True, "recompute", builder=1)


def test_overlapped_poses_equal_synchronous_poses(fovrt_mod):
    a, b = tp.mk(fovrt_mod, 1, motion=True), tp.mk(fovrt_mod, 1, motion=True)
    a.set_geometry_overlap(True)
    pos0, _, _ = tp.rest(a)
    models = a.models()
    ms = [tp.pose("turning", pos0, models, f) for f in range(6)]
    for f in range(6):
        a.set_model_transforms(ms[f], enqueue=True)
        a.frame(timing=False)
        b.set_model_transforms(ms[f], update="refit")
        sync_frame(fovrt_mod, b)
        tp.assert_same_frames(fovrt_mod, a, b, f"pose {f}")
    assert a.geometry_update_status() == (6, 0)
    assert_same_state(fovrt_mod, a, b, "poses")
    assert a.model_transforms().tobytes() == ms[5].tobytes()
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 2. The other set is stale: FR_NORMALS_KEEP and rejected updates must bring nothing back
# ---------------------------------------------------------------------------------------------
def test_keep_after_given_normals_keeps_the_given_normals(fovrt_mod):
    a, b = mk_on(fovrt_mod), mk(fovrt_mod)
    xyz, nrm = arrays(a, 3)
    n1 = nrm[1]
    for f, n in enumerate((n1, "keep", "keep")):
        a.update_geometry_enqueue(xyz[f], normals=n)
        a.frame(timing=False)
        sync_update(b, xyz[f], n)
        sync_frame(fovrt_mod, b)
        assert_same_frames(fovrt_mod, a, b, f"update {f}")
        assert a.scene_arrays()["nrm"].tobytes() == n1.cpu().numpy().tobytes(), f"update {f}: not the given normals"
    assert_same_state(fovrt_mod, a, b, "given, keep, keep")
    a.destroy(); b.destroy()


@pytest.mark.parametrize("at", [1, 2])  # the rejected update's index: odd and even, so either set is its destination
@pytest.mark.parametrize("bad", ["position", "normal"])
def test_rejected_overlapped_update_changes_nothing(fovrt_mod, bad, at):
    """a: accepted given updates 0 .. at - 1, then a bad one, then two frames; twin never sees the bad one."""
    a, twin = mk_on(fovrt_mod), mk(fovrt_mod)
    base, nrm0, _ = rest(a)
    n = base.shape[0]
    xyz, nrm = arrays(a, at + 1)
    poisoned = mn.sine(base, at).copy().reshape(-1, 9)
    bad_nrm = given_normals(nrm0, at).copy().reshape(-1, 9)
    if bad == "position":
        poisoned[n // 3, 7] = np.nan
    else:
        bad_nrm[n // 2, 4] = np.nan
    bad_xyz, bad_n = dev(poisoned), dev(bad_nrm)
    settle()
    for f in range(at):
        a.update_geometry_enqueue(xyz[f], normals=nrm[f])
        a.frame(timing=False)
        sync_update(twin, xyz[f], nrm[f])
        sync_frame(fovrt_mod, twin)
    a.update_geometry_enqueue(bad_xyz, normals=bad_n)  # the host learns nothing: no error here
    for f in range(2):
        a.frame(timing=False)
        sync_frame(fovrt_mod, twin)
        assert_same_frames(fovrt_mod, a, twin, f"frame {f} after the rejected update")
    assert a.geometry_update_status() == (at, 1)
    assert bad in a.last_error() and "not finite" in a.last_error(), a.last_error()
    assert_same_state(fovrt_mod, a, twin, "after the rejected update")
    a.update_geometry_enqueue(xyz[at], normals="keep")  # and the set the rejected update wrote is a good source
    a.frame(timing=False)
    sync_update(twin, xyz[at], "keep")
    sync_frame(fovrt_mod, twin)
    assert_same_frames(fovrt_mod, a, twin, "good update after the rejected one")
    assert_same_state(fovrt_mod, a, twin, "good update after the rejected one")
    assert a.geometry_update_status() == (at + 1, 1)
    a.destroy(); twin.destroy()


# ---------------------------------------------------------------------------------------------
# 3. One, two and three updates before one G-buffer (the set parity flips each time)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_several_overlapped_updates_before_one_gbuffer(fovrt_mod, k):
    a, b = mk_on(fovrt_mod), mk(fovrt_mod)
    xyz, nrm = arrays(a, 2 * k)
    for r in range(2):  # the second round reprojects from what the first round's G-buffer traced
        for f in range(k * r, k * r + k):
            n = nrm[f] if f % 2 else "recompute"
            a.update_geometry_enqueue(xyz[f], normals=n)
            sync_update(b, xyz[f], n)
        a.frame(timing=False)
        sync_frame(fovrt_mod, b)
        assert_same_frames(fovrt_mod, a, b, f"{k} updates, round {r}")
    assert_same_state(fovrt_mod, a, b, f"{k} updates, one frame")
    assert a.geometry_update_status() == (2 * k, 0)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Other calls between overlapped updates
# ---------------------------------------------------------------------------------------------
def between_sync_update(fovrt, a, b, xyz, nrm):
    sync_update(a, xyz[6], nrm[6])
    sync_update(b, xyz[6], nrm[6])


def between_refit(fovrt, a, b, xyz, nrm):
    a.refit_bvh(); b.refit_bvh()


def between_rebuild(fovrt, a, b, xyz, nrm):
    a.rebuild_bvh(); b.rebuild_bvh()


def between_set_normals(fovrt, a, b, xyz, nrm):
    a.set_normals_device(nrm[6].data_ptr(), nrm[6].shape[0])
    b.set_normals_device(nrm[6].data_ptr(), nrm[6].shape[0])


def between_recompute(fovrt, a, b, xyz, nrm):
    a.recompute_normals(); b.recompute_normals()


def between_timed_frame(fovrt, a, b, xyz, nrm):
    a.frame(timing=True)
    sync_frame(fovrt, b)
    assert_same_frames(fovrt, a, b, "the timed frame")


def between_stage_calls(fovrt, a, b, xyz, nrm):
    sync_frame(fovrt, a)
    sync_frame(fovrt, b)
    assert_same_frames(fovrt, a, b, "the stage calls")


def between_queries(fovrt, a, b, xyz, nrm):
    """Right after an enqueue, no synchronise in between: the calls order themselves behind the update."""
    a.update_geometry_enqueue(xyz[6], normals=nrm[6])
    cost, got = a.bvh_sah_cost(), a.scene_arrays()
    sync_update(b, xyz[6], nrm[6])
    assert cost == b.bvh_sah_cost()
    want = b.scene_arrays()
    for key in ("pos", "nrm", "bbox"):
        assert got[key].tobytes() == want[key].tobytes(), key
    a.update_geometry_enqueue(xyz[6], normals=nrm[6])  # (a's count of applied updates stays even)
    assert a.geometry_update_status()[1] == 0


BETWEEN = {"sync_update": between_sync_update, "refit": between_refit, "rebuild": between_rebuild,
           "set_normals": between_set_normals, "recompute_normals": between_recompute,
           "timed_frame": between_timed_frame, "stage_calls": between_stage_calls, "queries": between_queries}


@pytest.mark.parametrize("what", sorted(BETWEEN))
def test_other_calls_between_overlapped_updates(fovrt_mod, what):
    """Overlapped updates and frames, the call (on both contexts), then overlapped updates and frames again: with one
    and with two updates before it, so that either set is the scene's when the call comes."""
    builder = 1 if what == "rebuild" else 0
    for before in (1, 2):
        a, b = mk_on(fovrt_mod, True, builder), mk(fovrt_mod, True, builder)
        xyz, nrm = arrays(a, 7)
        kinds = [nrm[0], "keep", "recompute", "keep", nrm[4], "keep"]
        def step(f):
            a.update_geometry_enqueue(xyz[f], normals=kinds[f])
            a.frame(timing=False)
            sync_update(b, xyz[f], kinds[f])
            sync_frame(fovrt_mod, b)
            assert_same_frames(fovrt_mod, a, b, f"{what} before={before} update {f}")
        for f in range(before):
            step(f)
        BETWEEN[what](fovrt_mod, a, b, xyz, nrm)
        for f in range(before, before + 3):
            step(f)
        if builder == 0:
            assert_same_state(fovrt_mod, a, b, what)
        else:
            assert_same_state(fovrt_mod, a, b, what, tree=False)
            assert bvh_np.check_tracer_tree(fovrt_mod, a) == bvh_np.check_tracer_tree(fovrt_mod, b)
            mine = tree_bytes(fovrt_mod, a)
            a.refit_bvh()
            assert tree_bytes(fovrt_mod, a) == mine
        a.destroy(); b.destroy()


def test_snapshot_after_overlapped_updates_restores_into_a_synchronous_context(fovrt_mod):
    a = mk_on(fovrt_mod)
    xyz, nrm = arrays(a, 3)
    b = mk(fovrt_mod)
    for f in range(2):
        a.update_geometry_enqueue(xyz[f], normals=nrm[f])
        a.frame(timing=False)
    a.update_geometry_enqueue(xyz[2], normals="keep")
    snap = a.snapshot()  # right behind the enqueue
    sync_update(b, xyz[1], nrm[1])
    sync_update(b, xyz[2], "keep")
    b.restore(snap)
    a.restore(snap)
    for f in range(2):
        a.frame(timing=False)
        b.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, f"frame {f} after restore")
    assert_same_state(fovrt_mod, a, b, "after restore")
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 5. The switch
# ---------------------------------------------------------------------------------------------
def test_overlap_toggled_between_updates(fovrt_mod):
    a, b = mk(fovrt_mod), mk(fovrt_mod)
    xyz, nrm = arrays(a, 6)
    kinds = [nrm[0], "keep", "keep", nrm[3], "keep", "recompute"]
    for f, on in enumerate((True, True, False, False, True, True)):
        a.set_geometry_overlap(on)
        a.update_geometry_enqueue(xyz[f], normals=kinds[f])
        a.frame(timing=False)
        sync_update(b, xyz[f], kinds[f])
        sync_frame(fovrt_mod, b)
        assert_same_frames(fovrt_mod, a, b, f"update {f} overlap={on}")
    assert_same_state(fovrt_mod, a, b, "toggled")
    assert a.geometry_update_status() == (6, 0)
    a.destroy(); b.destroy()


def test_overlap_switched_off_equals_never_switched_on(fovrt_mod):
    a, b = mk(fovrt_mod), mk(fovrt_mod)
    a.set_geometry_overlap(True)
    a.set_geometry_overlap(False)
    xyz, nrm = arrays(a, 3)
    where = addresses(fovrt_mod, a)
    for f in range(3):
        for t in (a, b):
            t.update_geometry_enqueue(xyz[f], normals=nrm[f])
            t.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, f"frame {f}")
        assert addresses(fovrt_mod, a) == where
    assert_same_state(fovrt_mod, a, b, "off after on")
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 6. Producer and consumer ordering, on the front stages' stream
# ---------------------------------------------------------------------------------------------
def test_producer_event_and_consumed_wait_order_the_callers_stream_with_overlap(fovrt_mod):
    """test_gpu_update_enqueue's race with overlap on: ready_event orders the update's first read, now on the front
    stages' stream, behind a slow producer, and geometry_consumed orders the caller's overwrite behind the update's
    reads there. Probabilistic, as that test's docstring says; a missing wait shows nowhere else."""
    import torch
    a, b = mk_on(fovrt_mod), mk(fovrt_mod)
    base, _, _ = rest(a)
    frames = 6
    src = [dev(mn.sine(base, f)) for f in range(frames)]
    work = [torch.empty_like(src[0]), torch.empty_like(src[0])]
    ballast = torch.ones(32 << 20, device="cuda:0")  # 128 MiB a pass
    side = torch.cuda.Stream(device="cuda:0")
    settle()
    for f in range(frames):
        buf = work[f & 1]
        with torch.cuda.stream(side):
            for _ in range(8):
                ballast.mul_(1.0001)
            buf.copy_(src[f])
            ev = torch.cuda.Event()
            ev.record(side)
        a.update_geometry_enqueue(buf, normals="recompute", ready_event=ev)
        a.frame(timing=False)
        a.geometry_consumed(side)
        with torch.cuda.stream(side):
            buf.fill_(float("nan"))
        sync_update(b, src[f], "recompute")
        sync_frame(fovrt_mod, b)
    assert_same_frames(fovrt_mod, a, b, "producer / consumer")
    assert_same_state(fovrt_mod, a, b, "producer / consumer")
    assert a.geometry_update_status() == (frames, 0)
    settle()
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 7. Refusals
# ---------------------------------------------------------------------------------------------
def test_refusals(fovrt_mod):
    lib = fovrt_mod.load_library()
    a, other = mk(fovrt_mod), mk(fovrt_mod)
    for on in (2, -1):
        assert lib.fr_set_geometry_overlap(a._ctx, on) == fovrt_mod.FR_E_INVALID
        assert "0 or 1" in a.last_error()
    a.set_geometry_overlap(True)
    other.set_geometry_overlap(True)
    xyz, _ = arrays(a, 1, "keep")
    before = state(fovrt_mod, a)
    g = fovrt_mod.Group([a, other], views=1, tile=64)
    for t in (a, other):
        with pytest.raises(fovrt_mod.FovrtError) as e:
            t.update_geometry_enqueue(xyz[0])
        assert e.value.code == fovrt_mod.FR_E_UNSUPPORTED and "group" in t.last_error()
    g.destroy()
    other.set_shard_plan(0, 2, 32, fovrt_mod.shard_plan(W, H, 32, 2))
    with pytest.raises(fovrt_mod.FovrtError) as e:
        other.update_geometry_enqueue(xyz[0])
    assert e.value.code == fovrt_mod.FR_E_UNSUPPORTED and "sharded" in other.last_error()
    assert a.geometry_update_status() == (0, 0) and other.geometry_update_status() == (0, 0)
    assert state(fovrt_mod, a) == before
    a.update_geometry_enqueue(xyz[0])  # free again
    assert a.geometry_update_status() == (1, 0)
    a.destroy(); other.destroy()


# ---------------------------------------------------------------------------------------------
# 8. No allocation after the first enable
# ---------------------------------------------------------------------------------------------
def test_overlapped_updates_allocate_nothing(fovrt_mod):
    import torch
    a = mk_on(fovrt_mod)
    xyz, nrm = arrays(a, 6)
    a.update_geometry_enqueue(xyz[0], normals=nrm[0])
    a.frame(timing=False)
    a.synchronize()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()
    for f in range(6):
        a.update_geometry_enqueue(xyz[f], normals=(nrm[f], "keep", "recompute")[f % 3])
        a.frame(timing=False)
    a.set_geometry_overlap(False)
    a.set_geometry_overlap(True)  # the second set exists: nothing is made again
    a.update_geometry_enqueue(xyz[0])
    a.synchronize()
    assert a.geometry_update_status() == (8, 0)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info() == before
    a.destroy()


# ---------------------------------------------------------------------------------------------
# 9. Two sets, alternating
# ---------------------------------------------------------------------------------------------
def test_tree_in_use_alternates_between_two_addresses(fovrt_mod):
    a = mk(fovrt_mod)
    xyz, nrm = arrays(a, 6)
    a.update_geometry_enqueue(xyz[0])
    a.frame(timing=False)
    first = addresses(fovrt_mod, a)
    a.update_geometry_enqueue(xyz[1])
    assert addresses(fovrt_mod, a) == first, "in place: one address"
    a.set_geometry_overlap(True)
    seen = [addresses(fovrt_mod, a)]
    for f in range(6):
        a.update_geometry_enqueue(xyz[f], normals=nrm[f])
        a.frame(timing=False)
        seen.append(addresses(fovrt_mod, a))
    assert seen[0] == first
    assert all(s == seen[i % 2] for i, s in enumerate(seen)), seen
    assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]
    a.set_geometry_overlap(False)
    now = addresses(fovrt_mod, a)
    a.update_geometry_enqueue(xyz[0])
    a.frame(timing=False)
    assert addresses(fovrt_mod, a) == now
    assert a.geometry_update_status() == (9, 0)
    a.destroy()
