"""GPU suite for the device-triggered rebuild: fr_rebuild_bvh_enqueue_if, fr_set_rebuild_policy and
fr_bvh_rebuild_policy_status.

Context A enqueues (update or pose, then the conditional rebuild, then an untimed fr_frame). Its twin B takes the same
arrays through the synchronous calls and decides on the host by the same rule: c = fr_bvh_sah_cost; a stale baseline
adopts c; else c > 1.25 * baseline calls fr_rebuild_bvh and takes the new tree's cost as the baseline. The device's
cost is held to the synchronous one to 1e-4 relative only, so every decision here is posed far from the threshold:
test_cpu_rebuild_policy.py fixes the deformations and checks their margins on the host builder's trees, and the twin
asserts at every decision that its own quotient is 1 % and more away from 1.25 (a hundred times the cost tolerance)."""
import numpy as np
import pytest

import bvh_np
from bvh_canon_np import scene_rebuild_over
from bvh_refit_np import refit_np
from test_cpu_rebuild_policy import RATIO, failing_positions, grown, mild, mild_pose
from test_gpu_bvh import make_tracer, tree_bytes
from test_gpu_bvh_sah import SAH, assert_tree_is_hosts, host_scene, numbers
from test_gpu_geometry_overlap import addresses
from test_gpu_rebuild_enqueue import assert_same_canonical_tree, assert_same_frames, base_of
from test_gpu_update_enqueue import dev, settle, sync_update

pytestmark = pytest.mark.gpu

W, H = 64, 48
F = np.float32
COST_TOL = 1e-4  # the device's cost against fr_bvh_sah_cost (the bar that call is held to against numpy)


def mk(fovrt, scene=1, builder=SAH, overlap=False, motion=False, latency=False, pose=False):
    t = make_tracer(fovrt, W, H, scene, builder, mask=4, spp=2)
    if builder == 0:
        t.rebuild_bvh()  # the first device build makes the arrays an enqueued one needs
    if motion:
        t.set_motion_reprojection(True)
    if latency:
        t.set_pipeline_mode(fovrt.PIPELINE_LATENCY)
    if pose:
        t.enable_model_pose()
    t.set_geometry_overlap(overlap)
    return t


class Twin:
    """The caller who asks the synchronous calls."""

    def __init__(self, t):
        self.t, self.stale, self.base, self.last = t, True, None, None
        self.evaluated = self.skipped = self.built = 0

    def decide(self):
        c = self.t.bvh_sah_cost()
        self.last = c
        self.evaluated += 1
        if self.stale:
            self.base, self.stale = c, False
            self.skipped += 1
            return "adopt"
        q = c / (RATIO * self.base)
        assert abs(q - 1.0) > 0.01, f"a decision at {q} of the threshold says nothing about the device's"
        if F(c) > F(RATIO) * F(self.base):
            self.t.rebuild_bvh()
            self.base = self.last = self.t.bvh_sah_cost()
            self.built += 1
            return "build"
        self.skipped += 1
        return "skip"


def assert_policy_status(a, twin, what, failed=0):
    ev, sk, last, base = a.bvh_rebuild_policy_status()
    assert (ev, sk) == (twin.evaluated + failed, twin.skipped), (what, ev, sk)
    assert a.bvh_rebuild_status() == (twin.built, failed), what
    print(f"{what}: last {last} base {base}; twin last {twin.last} base {twin.base}")
    assert abs(last - twin.last) <= COST_TOL * twin.last, (what, last, twin.last)
    assert abs(base - twin.base) <= COST_TOL * twin.base, (what, base, twin.base)


def sequence(base):
    """adopt, mild, mild, grown, mild (over the grown geometry)."""
    g = grown(base)
    return [mild(base, 0), mild(base, 1), mild(base, 2), g, mild(g, 4)], ["adopt", "skip", "skip", "build", "skip"]


# ---------------------------------------------------------------------------------------------
# 1. Decisions and trees (builder 2)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("scene", [0, 1])
def test_decisions_trees_and_frames_are_the_twins(fovrt_mod, scene, overlap):
    a, b = mk(fovrt_mod, scene, overlap=overlap), mk(fovrt_mod, scene)
    twin = Twin(b)
    base = base_of(a)
    nodes0, _, prim0 = bvh_np.read_tree(fovrt_mod, a)
    host = host_scene(fovrt_mod, scene)
    pos, want = sequence(base)
    xyz = [dev(p) for p in pos]
    settle()
    for f, (p, x, w) in enumerate(zip(pos, xyz, want)):
        what = f"scene {scene} overlap={overlap} step {f} ({w})"
        a.update_geometry_enqueue(x, normals="recompute")
        a.rebuild_bvh_enqueue_if(RATIO)
        a.frame(timing=False)
        sync_update(b, x, "recompute")
        assert twin.decide() == w, what
        b.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, what)
        assert_same_canonical_tree(fovrt_mod, a, b, what)
        if f < 3:  # before the build: the original tree, refitted
            nodes, tri, prim = bvh_np.read_tree(fovrt_mod, a)
            want_nodes, want_tri = refit_np(nodes0, prim0, p)
            assert prim.tobytes() == prim0.tobytes(), what
            assert nodes.tobytes() == want_nodes.tobytes() and tri.tobytes() == want_tri.tobytes(), what
        if f == 3:  # the build: the host builder's tree over the current positions
            assert scene_rebuild_over(fovrt_mod, host, p) == 0
            assert_tree_is_hosts(fovrt_mod, a, host, what)
    assert a.bvh_rebuild_status() == (1, 0)
    assert a.bvh_rebuild_policy_status()[:2] == (5, 4)
    assert_policy_status(a, twin, f"scene {scene} overlap={overlap}")
    assert a.geometry_update_status() == (5, 0)
    bvh_np.check_tracer_tree(fovrt_mod, a)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Builders 0 and 1: the LBVH
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_lbvh_decisions_and_trees_are_the_twins(fovrt_mod, builder):
    a, b = mk(fovrt_mod, 1, builder), mk(fovrt_mod, 1, builder)
    twin = Twin(b)
    pos, want = sequence(base_of(a))
    xyz = [dev(p) for p in pos]
    settle()
    for f, (x, w) in enumerate(zip(xyz, want)):  # (no host reader of A inside the loop)
        a.update_geometry_enqueue(x)
        a.rebuild_bvh_enqueue_if(RATIO)
        sync_update(b, x, "keep")
        assert twin.decide() == w, (builder, f)
    assert_same_canonical_tree(fovrt_mod, a, b, f"builder {builder}")
    assert_policy_status(a, twin, f"builder {builder}")
    bvh_np.check_tracer_tree(fovrt_mod, a)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 3. A skipped build leaves bytes alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("builder", [1, SAH])
def test_skipped_build_leaves_the_tree_alone(fovrt_mod, builder, overlap):
    a = mk(fovrt_mod, 1, builder, overlap=overlap)
    base = base_of(a)
    xyz, big = dev(mild(base, 1)), dev(grown(base))
    settle()
    a.update_geometry_enqueue(xyz)
    a.rebuild_bvh_enqueue_if(RATIO)  # adopts
    before, nums = tree_bytes(fovrt_mod, a), numbers(a.scene_arrays())
    for _ in range(3):  # both sets of arrays are the destination
        a.rebuild_bvh_enqueue_if(RATIO)
        assert tree_bytes(fovrt_mod, a) == before and numbers(a.scene_arrays()) == nums
    assert a.bvh_rebuild_status() == (0, 0) and a.bvh_rebuild_policy_status()[:2] == (4, 4)
    # the node count known to the device alone: a skipped call right behind a built one, no host reader between;
    # the tree it leaves is the one an unconditional rebuild over the same positions builds
    ref = mk(fovrt_mod, 1, builder)
    a.update_geometry_enqueue(big)
    a.rebuild_bvh_enqueue_if(RATIO)
    a.rebuild_bvh_enqueue_if(RATIO)
    sync_update(ref, big, "keep")
    ref.rebuild_bvh()
    assert_same_canonical_tree(fovrt_mod, a, ref, f"builder {builder} overlap={overlap}")
    ev, sk, last, cost_base = a.bvh_rebuild_policy_status()
    assert (ev, sk) == (6, 5) and a.bvh_rebuild_status() == (1, 0)
    c = ref.bvh_sah_cost()
    assert abs(last - c) <= COST_TOL * c and abs(cost_base - c) <= COST_TOL * c, (last, cost_base, c)
    built = tree_bytes(fovrt_mod, a)
    a.rebuild_bvh_enqueue_if(RATIO)
    assert tree_bytes(fovrt_mod, a) == built
    bvh_np.check_tracer_tree(fovrt_mod, a)
    a.destroy(); ref.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Baseline rules
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["enqueue", "synchronous"])
def test_a_tree_installed_by_another_route_is_adopted(fovrt_mod, how):
    a = mk(fovrt_mod)
    base = base_of(a)
    big = dev(grown(base))
    settle()
    a.rebuild_bvh_enqueue_if(RATIO)  # adopts the preset's tree
    a.rebuild_bvh_enqueue() if how == "enqueue" else a.rebuild_bvh()
    a.update_geometry_enqueue(big)
    a.rebuild_bvh_enqueue_if(RATIO)  # far above the old baseline, but the tree is new: adopt and skip
    ev, sk, last, cost_base = a.bvh_rebuild_policy_status()
    assert (ev, sk) == (2, 2) and last == cost_base
    assert a.bvh_rebuild_status() == ((1, 0) if how == "enqueue" else (0, 0))
    c = a.bvh_sah_cost()
    assert abs(last - c) <= COST_TOL * c
    a.rebuild_bvh_enqueue_if(RATIO)  # and now it is the baseline
    assert a.bvh_rebuild_policy_status()[:2] == (3, 3)
    a.destroy()


def test_rejected_update_then_the_conditional_call_changes_nothing(fovrt_mod):
    a = mk(fovrt_mod)
    base = base_of(a)
    bad = grown(base)
    bad[3, 1, 2] = np.nan
    x0, xbad = dev(mild(base, 0)), dev(bad)
    settle()
    a.update_geometry_enqueue(x0)
    a.rebuild_bvh_enqueue_if(RATIO)
    before, status = tree_bytes(fovrt_mod, a), a.bvh_rebuild_policy_status()
    a.update_geometry_enqueue(xbad)
    a.rebuild_bvh_enqueue_if(RATIO)
    assert a.geometry_update_status() == (1, 1)
    assert tree_bytes(fovrt_mod, a) == before
    ev, sk, last, cost_base = a.bvh_rebuild_policy_status()
    assert (ev, sk, cost_base) == (status[0] + 1, status[1] + 1, status[3])
    assert abs(last - status[2]) <= COST_TOL * status[2]
    assert a.bvh_rebuild_status() == (0, 0)
    a.destroy()


@pytest.mark.parametrize("overlap", [False, True])
def test_two_conditional_calls_before_one_gbuffer(fovrt_mod, overlap):
    a, b = mk(fovrt_mod, overlap=overlap), mk(fovrt_mod)
    twin = Twin(b)
    base = base_of(a)
    x0, big = dev(mild(base, 0)), dev(grown(base))
    settle()
    a.update_geometry_enqueue(x0, normals="recompute")
    a.rebuild_bvh_enqueue_if(RATIO)
    a.frame(timing=False)
    a.update_geometry_enqueue(big, normals="recompute")
    a.rebuild_bvh_enqueue_if(RATIO)
    a.rebuild_bvh_enqueue_if(RATIO)
    a.frame(timing=False)
    sync_update(b, x0, "recompute")
    assert twin.decide() == "adopt"
    b.frame(timing=False)
    sync_update(b, big, "recompute")
    assert twin.decide() == "build" and twin.decide() == "skip"
    b.frame(timing=False)
    assert_same_frames(fovrt_mod, a, b, f"overlap={overlap}")
    assert_same_canonical_tree(fovrt_mod, a, b, f"overlap={overlap}")
    assert_policy_status(a, twin, f"two calls, overlap={overlap}")
    a.destroy(); b.destroy()


@pytest.mark.parametrize("overlap", [False, True])
def test_conditional_build_that_fails_on_the_device_keeps_tree_and_baseline(fovrt_mod, overlap):
    a, b = mk(fovrt_mod, overlap=overlap), mk(fovrt_mod)
    twin = Twin(b)
    base = base_of(a)
    host = host_scene(fovrt_mod, 1)
    nodes0, _, prim0 = bvh_np.read_tree(fovrt_mod, a)
    bad = failing_positions(fovrt_mod, host, nodes0, prim0, base)
    good = mild(base, 1)
    d_bad, d_good = dev(bad), dev(good)
    settle()
    a.rebuild_bvh_enqueue_if(RATIO)
    assert twin.decide() == "adopt"
    a.update_geometry_enqueue(d_bad)
    a.rebuild_bvh_enqueue_if(RATIO)  # the cost is finite and far above the baseline; the builder fails
    assert a.bvh_rebuild_status() == (0, 1)
    assert "SAH" in a.last_error() and "finite" in a.last_error(), a.last_error()
    ev, sk, last, cost_base = a.bvh_rebuild_policy_status()
    assert (ev, sk) == (2, 1) and abs(cost_base - twin.base) <= COST_TOL * twin.base
    assert last > RATIO * 1.01 * cost_base
    nodes, tri, prim = bvh_np.read_tree(fovrt_mod, a)
    want_nodes, want_tri = refit_np(nodes0, prim0, bad)
    assert prim.tobytes() == prim0.tobytes()
    assert nodes.tobytes() == want_nodes.tobytes() and tri.tobytes() == want_tri.tobytes()
    # sane geometry next: as if the failed call had not been made
    a.update_geometry_enqueue(d_good, normals="recompute")
    a.rebuild_bvh_enqueue_if(RATIO)
    sync_update(b, d_good, "recompute")
    assert twin.decide() == "skip"
    a.frame(timing=False); b.frame(timing=False)
    assert_same_frames(fovrt_mod, a, b, f"after the failed build, overlap={overlap}")
    assert_same_canonical_tree(fovrt_mod, a, b, f"after the failed build, overlap={overlap}")
    assert_policy_status(a, twin, f"after the failed build, overlap={overlap}", failed=1)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 5. The policy
# ---------------------------------------------------------------------------------------------
def policy_pattern(base):
    """Nine updates whose third, sixth and ninth are followed by an evaluation: adopt, build, skip."""
    g = grown(base)
    return [mild(base, f) for f in range(5)] + [g] + [mild(g, f) for f in (6, 7, 8)]


@pytest.mark.parametrize("overlap", [False, True])
def test_policy_equals_the_explicit_calls(fovrt_mod, overlap):
    a, b = mk(fovrt_mod, overlap=overlap), mk(fovrt_mod, overlap=overlap)
    xyz = [dev(p) for p in policy_pattern(base_of(a))]
    settle()
    a.set_rebuild_policy(RATIO, 3)
    for f, x in enumerate(xyz):
        a.update_geometry_enqueue(x, normals="recompute")
        a.frame(timing=False)
        b.update_geometry_enqueue(x, normals="recompute")
        if f % 3 == 2:
            b.rebuild_bvh_enqueue_if(RATIO)
        b.frame(timing=False)
    assert_same_frames(fovrt_mod, a, b, f"policy, overlap={overlap}")
    assert_same_canonical_tree(fovrt_mod, a, b, f"policy, overlap={overlap}")
    sa, sb = a.bvh_rebuild_policy_status(), b.bvh_rebuild_policy_status()
    assert sa[:2] == sb[:2] == (3, 2), (sa, sb)
    assert abs(sa[2] - sb[2]) <= COST_TOL * sb[2] and abs(sa[3] - sb[3]) <= COST_TOL * sb[3], (sa, sb)
    assert a.bvh_rebuild_status() == b.bvh_rebuild_status() == (1, 0)
    # period 0 stops it
    a.set_rebuild_policy(0.0, 0)
    for x in xyz[:3]:
        a.update_geometry_enqueue(x)
    assert a.bvh_rebuild_policy_status()[:2] == (3, 2) and a.geometry_update_status() == (12, 0)
    a.destroy(); b.destroy()


def test_policy_counts_enqueued_poses(fovrt_mod):
    a, b = mk(fovrt_mod, pose=True), mk(fovrt_mod, pose=True)
    base, models = base_of(a), a.models()
    ms = [mild_pose(base, models, f, 4.0 if f >= 5 else 1.0) for f in range(9)]
    a.set_rebuild_policy(RATIO, 3)
    for f, m in enumerate(ms):
        a.set_model_transforms(m, enqueue=True)
        a.frame(timing=False)
        b.set_model_transforms(m, enqueue=True)
        if f % 3 == 2:
            b.rebuild_bvh_enqueue_if(RATIO)
        b.frame(timing=False)
    assert_same_frames(fovrt_mod, a, b, "policy over poses")
    assert_same_canonical_tree(fovrt_mod, a, b, "policy over poses")
    sa, sb = a.bvh_rebuild_policy_status(), b.bvh_rebuild_policy_status()
    assert sa[:2] == sb[:2] == (3, 2), (sa, sb)
    assert a.bvh_rebuild_status() == b.bvh_rebuild_status() == (1, 0)
    # the decisions are the ones a host caller takes, far from the threshold: rest pose, swollen, swollen
    c = mk(fovrt_mod, pose=True)
    twin = Twin(c)
    want = {2: "adopt", 5: "build", 8: "skip"}
    for f, m in enumerate(ms):
        c.set_model_transforms(m, update="refit")
        assert f not in want or twin.decide() == want[f], f
    assert_policy_status(a, twin, "policy over poses")
    a.destroy(); b.destroy(); c.destroy()


# ---------------------------------------------------------------------------------------------
# 6. Mixed with what exists; refusals; no allocation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latency", [False, True])
def test_conditional_rebuild_with_motion_latency_and_snapshot(fovrt_mod, latency):
    a, b = mk(fovrt_mod, motion=True, latency=latency), mk(fovrt_mod, motion=True, latency=latency)
    twin = Twin(b)
    pos, want = sequence(base_of(a))
    xyz = [dev(p) for p in pos]
    settle()
    for f, (x, w) in enumerate(zip(xyz, want)):
        a.update_geometry_enqueue(x, normals="recompute")
        a.rebuild_bvh_enqueue_if(RATIO)
        sync_update(b, x, "recompute")
        assert twin.decide() == w, f
        if f == 3:
            snap = a.snapshot()  # right behind the build
            a.restore(snap); b.restore(snap)
        a.frame(timing=False); b.frame(timing=False)
        assert_same_frames(fovrt_mod, a, b, f"latency={latency} step {f}")
    assert_policy_status(a, twin, f"latency={latency}")
    a.destroy(); b.destroy()


def test_refusals_change_nothing(fovrt_mod):
    import torch
    E = fovrt_mod.FovrtError
    a, raw, other = mk(fovrt_mod), make_tracer(fovrt_mod, W, H, 1, 0), mk(fovrt_mod)
    a.rebuild_bvh_enqueue_if(RATIO)
    other.set_shard_plan(0, 2, 32, fovrt_mod.shard_plan(W, H, 32, 2))

    def state(t):
        t.synchronize()
        torch.cuda.synchronize()
        return (t.bvh_rebuild_status(), t.bvh_rebuild_policy_status(), tree_bytes(fovrt_mod, t), addresses(fovrt_mod, t),
                torch.cuda.mem_get_info())

    def refused(t, code, call, *args):
        before = state(t)
        with pytest.raises(E) as e:
            getattr(t, call)(*args)
        assert e.value.code == code, (call, args, t.last_error())
        assert state(t) == before, (call, args)

    for ratio in (float("nan"), float("inf"), 0.5):
        refused(a, fovrt_mod.FR_E_INVALID, "rebuild_bvh_enqueue_if", ratio)
        refused(a, fovrt_mod.FR_E_INVALID, "set_rebuild_policy", ratio, 3)
    refused(a, fovrt_mod.FR_E_INVALID, "set_rebuild_policy", RATIO, -1)
    refused(raw, fovrt_mod.FR_E_STATE, "rebuild_bvh_enqueue_if", RATIO)
    refused(raw, fovrt_mod.FR_E_STATE, "set_rebuild_policy", RATIO, 3)
    refused(other, fovrt_mod.FR_E_UNSUPPORTED, "rebuild_bvh_enqueue_if", RATIO)
    refused(other, fovrt_mod.FR_E_UNSUPPORTED, "set_rebuild_policy", RATIO, 3)
    # a refused policy is no policy: updates evaluate nothing
    x = dev(mild(base_of(a), 1))
    settle()
    a.update_geometry_enqueue(x)
    assert a.bvh_rebuild_policy_status()[:2] == (1, 1)
    a.destroy(); raw.destroy(); other.destroy()


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("builder", [1, SAH])
def test_conditional_rebuilds_allocate_nothing(fovrt_mod, builder, overlap):
    import torch
    a = mk(fovrt_mod, 1, builder, overlap=overlap)
    base = base_of(a)
    g = grown(base)
    xyz = [dev(p) for p in (mild(base, 0), g, mild(g, 1))]
    a.update_geometry_enqueue(xyz[0])  # (as the neighbouring suites: the runtime's own first-use allocations)
    a.rebuild_bvh_enqueue_if(RATIO)
    a.frame(timing=False)
    a.synchronize()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()
    a.set_rebuild_policy(RATIO, 2)
    for f in range(6):  # skips, builds (every return to the base geometry or to the grown one) and the policy's calls
        a.update_geometry_enqueue(xyz[f % 3])
        a.rebuild_bvh_enqueue_if(RATIO)
    a.synchronize()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info() == before
    ev, sk, _, _ = a.bvh_rebuild_policy_status()
    built, failed = a.bvh_rebuild_status()
    assert ev == 1 + 6 + 3 and failed == 0 and built >= 1 and built + sk == ev, (ev, sk, built)
    bvh_np.check_tracer_tree(fovrt_mod, a)
    a.destroy()
