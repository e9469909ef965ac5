"""GPU suite for stream-ordered geometry updates: fr_update_geometry_enqueue against the synchronous
fr_update_geometry (device memory, refit), bit for bit.

Context A takes its positions through the enqueued call and renders pipelined frames with no synchronising call in
between; context B takes the same positions through the synchronous call and renders stage by stage. Everything
they leave is compared by bytes: the frame's buffers, the scene arrays (positions, normals, box) and the tree.
Positions live in torch device tensors, prepared before the loop (a synchronise there, none inside it)."""
import ctypes as C

import numpy as np
import pytest

import bvh_np
import motion_np as mn
from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan
from test_gpu_bvh import make_tracer, mismatch_report, tree_bytes

pytestmark = pytest.mark.gpu

W, H = 160, 96  # test_update_before_every_pipelined_frame's size: 10 x 6 sampling blocks, several G-buffer tiles
F = np.float32


def bufs(fovrt):
    TN = fovrt.TextureName
    return (TN.SHADING, TN.HISTORY_CACHE, TN.WEIGHT, TN.SIBSON, TN.ATROUS)


def mk(fovrt, motion=True, builder=0, mask=4, latency=False):
    t = make_tracer(fovrt, W, H, 1, builder, mask=mask, spp=2)
    if motion:
        t.set_motion_reprojection(True)
    if latency:
        t.set_pipeline_mode(fovrt.PIPELINE_LATENCY)
    return t


def sync_frame(fovrt, t):
    """One frame stage by stage, as test_update_before_every_pipelined_frame renders its reference."""
    TN = fovrt.TextureName
    t.geometry_launch(); t.sampling_launch(); t.optimize_launch(); t.shading_launch()
    fovrt.JumpFlooding(t).render(TN.SHADING)
    fovrt.SibsonInterpolation(t).render()
    fovrt.PullPushInterpolation(t).render(TN.SHADING)
    fovrt.ATrous(t).render(1, TN.POSITION, TN.NORMAL, TN.PULLPUSH)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1, 9)).to("cuda:0")


def settle():
    import torch
    torch.cuda.synchronize()


def rest(t):
    a = t.scene_arrays()
    return a["pos"].reshape(-1, 3, 3).copy(), a["nrm"].reshape(-1, 3, 3).copy(), a


def given_normals(nrm0, f):
    """Some other finite unit normals for frame f: every triangle's corner normals rotated by f corners."""
    return np.roll(nrm0, f % 3, axis=1)


def state(fovrt, t, tree=True):
    a = t.scene_arrays()
    s = {k: a[k].tobytes() for k in ("pos", "nrm", "bbox")}
    if tree:
        s.update(zip(("nodes", "tri_geo", "prim"), tree_bytes(fovrt, t)))
    return s


def assert_same_state(fovrt, a, b, what="", tree=True):
    sa, sb = state(fovrt, a, tree), state(fovrt, b, tree)
    for k in sa:
        assert sa[k] == sb[k], f"{what}: {k} differs"


def assert_same_frames(fovrt, a, b, what="", ids=None):
    for tid in ids or bufs(fovrt):
        x, y = a.read(tid), b.read(tid)
        assert equal_nan(x, y), (what, tid, mismatch_report(x, y))


def sync_update(t, xyz, normals):
    """fr_update_geometry / fr_update_positions from device memory with a refit. normals: "keep", "recompute" or a tensor."""
    t.set_positions_device(xyz.data_ptr(), xyz.shape[0], update="refit",
                           normals=normals if isinstance(normals, str) else normals.data_ptr())


# ---------------------------------------------------------------------------------------------
# 1. Equal to the synchronous path
# ---------------------------------------------------------------------------------------------
def run_equal(fovrt, latency, motion, normals, builder=0, frames=6):
    a, b = mk(fovrt, motion, builder, latency=latency), mk(fovrt, motion, builder)
    base, nrm0, _ = rest(a)
    xyz = [dev(mn.sine(base, f)) for f in range(frames)]
    nrm = [dev(given_normals(nrm0, f)) for f in range(frames)] if normals == "given" else [normals] * frames
    settle()
    for f in range(frames):
        a.update_geometry_enqueue(xyz[f], normals=nrm[f])
        a.frame(timing=False)
        sync_update(b, xyz[f], nrm[f])
        sync_frame(fovrt, b)
    what = f"latency={latency} motion={motion} normals={normals} builder={builder}"
    assert_same_frames(fovrt, a, b, what)
    assert_same_state(fovrt, a, b, what, tree=builder == 0)
    if builder == 1:
        # Two device-built trees of the same triangles are the same hierarchy, but the order in which the nodes of
        # a level take their indices is free (test_gpu_bvh.test_preset_tree_structure), so their bytes are not
        # comparable across contexts. Compared instead: the structure, and the bytes of a's own tree against the
        # synchronous refit of it over the positions in place (which changes no byte of a refitted tree).
        assert bvh_np.check_tracer_tree(fovrt, a) == bvh_np.check_tracer_tree(fovrt, b)
        mine = tree_bytes(fovrt, a)
        a.refit_bvh()
        assert tree_bytes(fovrt, a) == mine, "the enqueued refit's bytes are not the synchronous refit's"
    assert a.geometry_update_status() == (frames, 0)
    assert b.geometry_update_status() == (0, 0)
    a.destroy(); b.destroy()


@pytest.mark.parametrize("normals", ["keep", "recompute", "given"])
@pytest.mark.parametrize("motion", [True, False])
@pytest.mark.parametrize("latency", [False, True])
def test_enqueued_updates_equal_synchronous_updates(fovrt_mod, latency, motion, normals):
    run_equal(fovrt_mod, latency, motion, normals)


def test_enqueued_updates_equal_synchronous_updates_on_a_device_built_tree(fovrt_mod):
    run_equal(fovrt_mod, False, True, "recompute", builder=1)


# ---------------------------------------------------------------------------------------------
# 2. The saliency mask reads the scene box, which only the device knows after an enqueued update
# ---------------------------------------------------------------------------------------------
def test_saliency_mask_follows_the_box_of_enqueued_updates(fovrt_mod):
    TN = fovrt_mod.TextureName
    a, b = mk(fovrt_mod, mask=0), mk(fovrt_mod, mask=0)
    base, _, arrays0 = rest(a)
    xyz = [dev(mn.sine(base, f)) for f in range(3)]
    settle()
    for f in range(3):
        a.update_geometry_enqueue(xyz[f], normals="recompute")
        a.frame(timing=False)
        sync_update(b, xyz[f], "recompute")
        sync_frame(fovrt_mod, b)
    box = a.scene_arrays()["bbox"]
    assert box.tobytes() != arrays0["bbox"].tobytes(), "the deformation must change the scene box"
    assert box.tobytes() == b.scene_arrays()["bbox"].tobytes()
    assert a.ray_count() == b.ray_count()
    assert a.ray_count() > 0
    assert np.array_equal(a.read(TN.MASK), b.read(TN.MASK))
    assert_same_frames(fovrt_mod, a, b, "saliency", ids=(TN.SHADING,))
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Rejected on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [True, False])
@pytest.mark.parametrize("bad", ["position", "normal"])
def test_update_rejected_on_the_device_changes_nothing(fovrt_mod, bad, motion):
    """a: gets a bad update; twin: never sees it (and takes every good one through the synchronous call)."""
    a, twin = mk(fovrt_mod, motion), mk(fovrt_mod, motion)
    base, nrm0, _ = rest(a)
    n = base.shape[0]
    pos = [mn.sine(base, f) for f in range(3)]
    xyz = [dev(p) for p in pos]
    nrm = [dev(given_normals(nrm0, f)) for f in range(3)]
    poisoned = pos[1].copy().reshape(-1, 9)
    bad_nrm = given_normals(nrm0, 1).copy().reshape(-1, 9)
    if bad == "position":
        poisoned[n // 3, 7] = np.nan
    else:
        bad_nrm[n // 2, 4] = np.inf  # every triangle of this scene has normals
    bad_xyz, bad_n = dev(poisoned), dev(bad_nrm)
    settle()
    a.update_geometry_enqueue(xyz[0], normals=nrm[0])
    a.frame(timing=False)
    sync_update(twin, xyz[0], nrm[0])
    sync_frame(fovrt_mod, twin)
    assert a.geometry_update_status() == (1, 0)
    a.update_geometry_enqueue(bad_xyz, normals=bad_n)  # the host learns nothing: no error here
    assert a.geometry_update_status() == (1, 1)
    assert bad in a.last_error() and "not finite" in a.last_error(), a.last_error()
    assert_same_state(fovrt_mod, a, twin, "after the rejected update")
    for f in range(2):
        a.frame(timing=False)
        sync_frame(fovrt_mod, twin)
        assert_same_frames(fovrt_mod, a, twin, f"frame {f} after the rejected update")
    a.update_geometry_enqueue(xyz[2], normals=nrm[2])
    a.frame(timing=False)
    sync_update(twin, xyz[2], nrm[2])
    sync_frame(fovrt_mod, twin)
    assert a.geometry_update_status() == (2, 1)
    assert_same_frames(fovrt_mod, a, twin, "good update after the rejected one")
    assert_same_state(fovrt_mod, a, twin, "good update after the rejected one")
    a.destroy(); twin.destroy()


def test_bad_normal_on_a_triangle_without_normals_is_ignored(fovrt_mod, tmp_path):
    """The preset scenes give every triangle normals; an OBJ box without vn lines gives four triangles that have
    none (flags & 0x100 clear). An Inf in their given normals is neither checked nor written: the update applies."""
    from test_cpu_abi import GROUND_OBJ
    (tmp_path / "box").mkdir()
    (tmp_path / "ground.obj").write_text(GROUND_OBJ)
    (tmp_path / "box" / "box.obj").write_text("v 0 0 0\nv 100 0 0\nv 0 100 0\nv 0 0 100\n"
                                              "f 1 3 2\nf 1 2 4\nf 1 4 3\nf 2 3 4\n")
    def make():
        t = fovrt_mod.PathTracer(fovrt_mod.Config(width=W, height=H, scene=0, mask_mode=4, spp=2, texture_mode=1,
                                                  mesh_mode=2, asset_dir=str(tmp_path)))
        assert t.initialize()
        return t
    a, b = make(), make()
    base, nrm0, arrays = rest(a)
    without = np.nonzero((arrays["flags"] & 0x100) == 0)[0]
    assert len(without) == 4 and len(arrays["flags"]) == 6
    pos = mn.sine(base, 1.0)
    nrm = nrm0.copy().reshape(-1, 9)
    nrm[without[1], 4] = np.inf
    xyz, d_nrm = dev(pos), dev(nrm)
    settle()
    a.update_geometry_enqueue(xyz, normals=d_nrm)
    a.frame(timing=False)
    sync_update(b, xyz, d_nrm)
    sync_frame(fovrt_mod, b)
    assert a.geometry_update_status() == (1, 0)
    assert_same_frames(fovrt_mod, a, b, "ignored normal")
    assert_same_state(fovrt_mod, a, b, "ignored normal")
    assert a.scene_arrays()["pos"].tobytes() == pos.tobytes()
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Rejected on the host
# ---------------------------------------------------------------------------------------------
def test_update_rejected_on_the_host_enqueues_nothing(fovrt_mod):
    lib = fovrt_mod.load_library()
    a = mk(fovrt_mod)
    base, nrm0, _ = rest(a)
    n = base.shape[0]
    xyz = dev(mn.sine(base, 1.0))
    settle()
    a.frame(timing=False)
    before, shading = state(fovrt_mod, a), a.read(fovrt_mod.TextureName.SHADING)
    p = C.c_void_p(xyz.data_ptr())
    GIVEN = fovrt_mod.FR_NORMALS_GIVEN
    cases = [("triangle count", (p, None, n - 1, 0, None)), ("positions are NULL", (None, None, n, 0, None)),
             ("bad normals kind", (p, None, n, 7, None)), ("without normals", (p, None, n, GIVEN, None))]
    for msg, args in cases:
        assert lib.fr_update_geometry_enqueue(a._ctx, *args) == fovrt_mod.FR_E_INVALID, msg
        assert msg in a.last_error(), (msg, a.last_error())
        assert a.geometry_update_status() == (0, 0), msg
    with pytest.raises(fovrt_mod.FovrtError) as e:
        a.update_geometry_enqueue(xyz, ntris=n - 1)
    assert e.value.code == fovrt_mod.FR_E_INVALID
    assert state(fovrt_mod, a) == before
    assert equal_nan(a.read(fovrt_mod.TextureName.SHADING), shading)
    # a rank of a group is updated by its caller through the synchronous calls
    other = mk(fovrt_mod)
    g = fovrt_mod.Group([a, other], views=1, tile=64)
    for t in (a, other):
        with pytest.raises(fovrt_mod.FovrtError) as e:
            t.update_geometry_enqueue(xyz)
        assert e.value.code == fovrt_mod.FR_E_UNSUPPORTED
        assert "group" in t.last_error()
        assert t.geometry_update_status() == (0, 0)
    g.destroy()
    assert state(fovrt_mod, a) == before
    a.update_geometry_enqueue(xyz)  # free again
    assert a.geometry_update_status() == (1, 0)
    a.destroy(); other.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Producer and consumer ordering
# ---------------------------------------------------------------------------------------------
def test_producer_event_and_consumed_wait_order_the_callers_stream(fovrt_mod):
    """The positions are produced on a side stream behind a chain of large elementwise kernels, so they are not
    ready when the update is enqueued (ready_event orders its first read), and the tensor is overwritten with NaN
    on that stream right after geometry_consumed (which orders the overwrite behind the update's reads). A missing
    wait on either side shows here only with some probability (it is a race on the device); the test exists because
    a missing wait can show nowhere else."""
    import torch
    a, b = mk(fovrt_mod), mk(fovrt_mod)
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
# 6. Several updates before one G-buffer; synchronous and enqueued updates mixed
# ---------------------------------------------------------------------------------------------
def test_several_enqueued_updates_before_one_gbuffer(fovrt_mod):
    a, b = mk(fovrt_mod), mk(fovrt_mod)
    base, _, _ = rest(a)
    xyz = [dev(mn.sine(base, f)) for f in range(6)]
    settle()
    for r in range(2):  # the second round reprojects from what the first round's G-buffer traced
        for f in range(3 * r, 3 * r + 3):
            a.update_geometry_enqueue(xyz[f], normals="recompute")
            sync_update(b, xyz[f], "recompute")
        a.frame(timing=False)
        sync_frame(fovrt_mod, b)
    assert_same_frames(fovrt_mod, a, b, "three updates, one frame")
    assert_same_state(fovrt_mod, a, b, "three updates, one frame")
    a.destroy(); b.destroy()


def test_synchronous_and_enqueued_updates_alternate(fovrt_mod):
    a, b = mk(fovrt_mod), mk(fovrt_mod)
    base, _, _ = rest(a)
    xyz = [dev(mn.sine(base, f)) for f in range(4)]
    settle()
    for f in range(4):
        if f % 2 == 0:
            a.update_geometry_enqueue(xyz[f], normals="recompute")
        else:
            sync_update(a, xyz[f], "recompute")
        sync_update(b, xyz[f], "recompute")
        a.frame(timing=False)
        sync_frame(fovrt_mod, b)
    assert_same_frames(fovrt_mod, a, b, "alternating")
    assert_same_state(fovrt_mod, a, b, "alternating")
    assert a.geometry_update_status() == (2, 0)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 7. Snapshot
# ---------------------------------------------------------------------------------------------
def test_snapshot_after_an_enqueued_update_restores_into_a_synchronous_context(fovrt_mod):
    a = mk(fovrt_mod)
    base, _, _ = rest(a)
    xyz = dev(mn.sine(base, 1.0))
    settle()
    a.update_geometry_enqueue(xyz, normals="recompute")
    a.frame(timing=False)
    snap = a.snapshot()
    b = mk(fovrt_mod)
    sync_update(b, xyz, "recompute")
    b.restore(snap)
    a.frame(timing=False)
    b.frame(timing=False)
    assert_same_frames(fovrt_mod, a, b, "after restore")
    assert_same_state(fovrt_mod, a, b, "after restore")
    a.destroy(); b.destroy()
