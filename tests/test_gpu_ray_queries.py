"""GPU suite for ray queries (fr_trace_rays, fr_trace_rays_enqueue, fr_rays_consumed): the closest hit against the
oracle's brute force over every triangle, bit for bit in all four fields; the transmittance against the numpy
restatement; the link to the frame's G-buffer; the scene a query sees while it moves, in place and overlapped; the
stream order of the caller's arrays; frames untouched by queries; refusals; and what holds outside the guaranteed
domain. The ray sets are tests/ray_cases.py's, whose preconditions tests/test_cpu_ray_queries.py asserts."""
import numpy as np
import pytest

import ray_cases as rc
import trace_cases as tc
import trace_np as tn
from helpers import equal_nan
from test_cpu_ray_queries import refs
from test_cpu_rebuild_policy import RATIO, grown, mild

pytestmark = pytest.mark.gpu

F = np.float32
_TRACERS = {}


def mk(fovrt, scene, builder=0, W=rc.SIZE[0], H=rc.SIZE[1], **kw):
    t = fovrt.PathTracer(rc.config(fovrt, scene, W, H, builder, **kw))
    assert t.initialize(), t.last_error()
    return t


@pytest.fixture(scope="module")
def still(fovrt_mod):
    """Contexts whose scene no test moves, one per (scene, builder), shared by the read-only tests."""
    def get(scene, builder=0):
        if (scene, builder) not in _TRACERS:
            _TRACERS[scene, builder] = mk(fovrt_mod, scene, builder)
        return _TRACERS[scene, builder]
    yield get
    for t in _TRACERS.values():
        t.destroy()
    _TRACERS.clear()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def settle():
    import torch
    torch.cuda.synchronize()


def hits_of(x):
    """A device tensor of n x 4 words -> fr_ray_hit records."""
    return x.cpu().numpy().view(rc.HIT_DTYPE).reshape(-1)


def out_hits(n, fill=np.nan):
    import torch
    return torch.full((n, 4), fill, dtype=torch.float32, device="cuda:0")


def query(t, r, where, kind="closest"):
    """The synchronous form over rows (o, d, tmin, tmax), from host or from device memory."""
    fr = rc.fr_rays(r)
    if where == "host":
        return t.trace_rays(fr, kind)
    import torch
    x = dev(fr)
    n = len(fr)
    out = out_hits(n) if kind == "closest" else torch.full((n,), np.nan, dtype=torch.float32, device="cuda:0")
    settle()
    t.trace_rays(x, kind, out=out, n=n)
    return hits_of(out) if kind == "closest" else out.cpu().numpy()


def report(got, want, r):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return "equal"
    i = bad[0]
    return f"{len(bad)} of {len(got)} differ; first {i}: gpu {got[i]} reference {want[i]} ray {r[i].tolist()}"


def brute(oracle, arrays, r):
    return rc.hit_records(oracle.OracleScene(arrays).closest(r, brute=True))


# ---------------------------------------------------------------------------------------------
# 1. Closest hit: bit equality with the oracle's brute force
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("scene", [0, 1])
def test_closest_equals_brute_force_on_every_set(fovrt_mod, oracle, still, scene, where):
    a, osc, _nsc, sets = refs(fovrt_mod, oracle, scene)
    t = still(scene)
    for name, (r, want) in sets.items():
        got = query(t, r, where)
        assert got.dtype == rc.HIT_DTYPE
        assert rc.same_records(got, want), (name, report(got, want, r))
        w, _kind, _base = rc.window_rows(r, want)
        if len(w):
            got, ref = query(t, w, where), rc.hit_records(osc.closest(w, brute=True))
            assert rc.same_records(got, ref), (name, "windows", report(got, ref, w))
    d, _good = rc.degenerate_rows(a)
    got = query(t, d, where)
    assert (got == rc.MISS).all(), np.nonzero(got != rc.MISS)[0]


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_zero_and_tie_sets_on_every_builder(fovrt_mod, oracle, builder):
    a, _osc, _nsc, sets = refs(fovrt_mod, oracle, 0)
    t = mk(fovrt_mod, 0, builder)
    r, want = sets["zeros"]
    got = query(t, r, "host")
    assert rc.same_records(got, want), report(got, want, r)
    for update in ("refit", "rebuild"):
        t.set_positions(rc.tie_positions(a), update=update)
        moved = t.scene_arrays()
        assert moved["pos"].tobytes() == rc.tie_positions(a).tobytes()
        r = rc.tie_rows(a)
        want = brute(oracle, moved, r)
        assert np.isin(want["prim"], [s for _d, s in rc.TIE_PAIRS]).sum() >= 50
        for where in ("host", "device"):
            got = query(t, r, where)
            assert rc.same_records(got, want), (update, where, report(got, want, r))
    t.destroy()


@pytest.mark.parametrize("n", rc.BATCH_SIZES)
def test_every_batch_size(fovrt_mod, oracle, still, n):
    _a, _osc, _nsc, sets = refs(fovrt_mod, oracle, 1)
    r, want = sets["refill"]
    assert len(r) == rc.BATCH_SIZES[-1]
    r, want = r[len(r) - n:], want[len(r) - n:]
    for where in ("host", "device"):
        got = query(still(1), r, where)
        assert len(got) == n and rc.same_records(got, want), (where, report(got, want, r))


def test_one_block_refills_its_lanes(fovrt_mod, oracle, monkeypatch):
    """FOVRT_RAYQ_BLOCKS=1: two waves answer eight chunks, whose rays alternate misses and deep hits."""
    _a, _osc, nsc, sets = refs(fovrt_mod, oracle, 1)
    r, want = sets["refill"]
    hit = want["prim"] >= 0
    assert (hit[1::2].mean() > 0.9) and not hit[0::2].any()
    monkeypatch.setenv("FOVRT_RAYQ_BLOCKS", "1")
    t = mk(fovrt_mod, 1)
    monkeypatch.delenv("FOVRT_RAYQ_BLOCKS")
    for where in ("host", "device"):
        got = query(t, r, where)
        assert rc.same_records(got, want), (where, report(got, want, r))
    s = rc.shadow_rows(rc.scene_arrays(fovrt_mod, 1))
    check_transmittance(query(t, s, "device", "transmittance"), rc.shadow_np(nsc, s))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 2. Transmittance against the numpy restatement
# ---------------------------------------------------------------------------------------------
def check_transmittance(got, want):
    """Exactly 0 where it is 0, exactly 1 where it is 1, otherwise within one fp32 ulp: the f64 product of the fp32
    factors is exact to 2^-53 per factor whatever the order, so the two orders round to the same float or to
    neighbours."""
    assert got.dtype == np.float32 and got.shape == want.shape
    zero, one = want == 0, want == 1
    assert (got[zero] == 0).all() and (got[one] == 1).all()
    mid = ~zero & ~one
    assert ((got[mid] > 0) & (got[mid] < 1)).all()
    ulp = np.spacing(want[mid])
    err = np.abs(got[mid].astype(np.float64) - want[mid].astype(np.float64))
    print("transmittance: zero", int(zero.sum()), "one", int(one.sum()), "between", int(mid.sum()),
          "worst error in ulps", float((err / ulp).max()) if mid.any() else 0.0)
    assert (err <= ulp).all(), float((err / ulp).max())


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("scene", [0, 1])
def test_transmittance_equals_the_restatement(fovrt_mod, oracle, still, scene, where):
    a, _osc, nsc, _sets = refs(fovrt_mod, oracle, scene)
    s = rc.shadow_rows(a)
    d, _good = rc.degenerate_rows(a)
    check_transmittance(query(still(scene), s, where, "transmittance"), rc.shadow_np(nsc, s))
    assert (query(still(scene), d, where, "transmittance") == 1).all()


# ---------------------------------------------------------------------------------------------
# 3. The link to the frame: a camera ray's triangle has the class the G-buffer wrote
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.QUERY_VIEWS)
def test_camera_rays_hit_the_class_the_gbuffer_wrote(fovrt_mod, still, name):
    W, H = rc.SIZE
    scene = tc.VIEWS[name][0]
    t = still(scene)
    t.update_optix_variables(tc.camera(fovrt_mod, name, W, H))
    t.geometry_launch()
    gclass = t.read(fovrt_mod.TextureName.GCLASS).reshape(H, W)
    got = query(t, rc.camera_rows(fovrt_mod, name), "host")
    cls = tc.classes_np(t.scene_arrays(), got["prim"]).reshape(H, W)
    assert np.array_equal(cls, gclass), (name, int((cls != gclass).sum()))
    model = t.model_of(got)
    ms = t.models()
    assert ((model >= 0) == (got["prim"] >= 0)).all()
    for i, (_n, first, cnt) in enumerate(ms):
        sel = model == i
        assert ((got["prim"][sel] >= first) & (got["prim"][sel] < first + cnt)).all()


# ---------------------------------------------------------------------------------------------
# 4. The moving scene
# ---------------------------------------------------------------------------------------------
def with_pos(arrays, pos):
    b = dict(arrays)
    b["pos"] = np.asarray(pos, F).reshape(np.asarray(arrays["pos"]).shape)
    return b


@pytest.mark.parametrize("overlap", [False, True])
def test_queries_see_the_scene_at_their_place_in_the_stream(fovrt_mod, oracle, overlap):
    _a, _osc, _nsc, sets = refs(fovrt_mod, oracle, 1)
    r = np.concatenate([sets["random"][0], sets["view_bunny_close"][0], sets["view_along_z"][0]])
    n = len(r)
    t = mk(fovrt_mod, 1, builder=2)
    t.set_geometry_overlap(overlap)
    base = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    nt = base.shape[0]
    rays = dev(rc.fr_rays(r))
    xs = [mild(base, f) for f in range(8)] + [grown(base)]
    xd = [dev(x.reshape(-1, 9)) for x in xs]
    poisoned = xs[0].copy().reshape(-1, 9)
    poisoned[nt // 3, 7] = np.nan
    bad = dev(poisoned)
    settle()

    def enqueued():
        out = out_hits(n)
        settle()
        t.trace_rays_enqueue(rays, out, n=n)
        return out

    def check(out, what, pos=None):
        t.synchronize()
        arrays = t.scene_arrays()
        if pos is not None:
            assert arrays["pos"].tobytes() == np.asarray(pos, F).tobytes(), what
        want = brute(oracle, arrays, r)
        got = hits_of(out) if out is not None else query(t, r, "host")
        assert rc.same_records(got, want), (what, report(got, want, r))
        return want

    first = check(None, "the scene as created")
    t.set_positions(xs[0], update="refit")
    moved = check(None, "fr_update_geometry, refit", xs[0])
    assert not rc.same_records(first, moved), "the deformation must change the answers"
    t.set_positions(xs[1], update="rebuild")
    check(None, "fr_update_geometry, rebuild", xs[1])
    t.update_geometry_enqueue(xd[2])
    check(enqueued(), "fr_update_geometry_enqueue", xs[2])
    t.rebuild_bvh_enqueue()
    check(enqueued(), "fr_rebuild_bvh_enqueue", xs[2])
    assert t.bvh_rebuild_status() == (1, 0)
    t.rebuild_bvh_enqueue_if(RATIO)  # adopts the new tree's cost: a skip
    check(enqueued(), "fr_rebuild_bvh_enqueue_if, adopted", xs[2])
    t.update_geometry_enqueue(xd[3])
    t.rebuild_bvh_enqueue_if(RATIO)  # a mild step: a skip
    check(enqueued(), "fr_rebuild_bvh_enqueue_if, skipped", xs[3])
    assert t.bvh_rebuild_status() == (1, 0) and t.bvh_rebuild_policy_status()[:2] == (2, 2)
    t.update_geometry_enqueue(xd[8])
    t.rebuild_bvh_enqueue_if(RATIO)  # the grown geometry: a build
    check(enqueued(), "fr_rebuild_bvh_enqueue_if, built", xs[8])
    assert t.bvh_rebuild_status() == (2, 0) and t.bvh_rebuild_policy_status()[:2] == (3, 2)

    # three update-then-query pairs back to back, no host wait between them: query k sees update k (with overlap on,
    # the third update overwrites the set the first query read: the set_read fence)
    outs = [out_hits(n) for _ in range(3)]
    settle()  # (the three fills; nothing of the context's is waited for between the pairs below)
    for k, out in zip((4, 5, 6), outs):
        t.update_geometry_enqueue(xd[k])
        t.trace_rays_enqueue(rays, out, n=n)
    t.synchronize()
    arrays = t.scene_arrays()
    wants = []
    for k, out in zip((4, 5, 6), outs):
        want = brute(oracle, with_pos(arrays, xs[k]), r)
        wants.append(want)
        got = hits_of(out)
        assert rc.same_records(got, want), (f"pair {k}", report(got, want, r))
    assert not rc.same_records(wants[0], wants[1]) and not rc.same_records(wants[1], wants[2])

    # a rejected update leaves the answers as they were
    applied, rejected = t.geometry_update_status()
    t.update_geometry_enqueue(bad)
    out = enqueued()
    t.synchronize()
    assert t.geometry_update_status() == (applied, rejected + 1)
    assert rc.same_records(hits_of(out), wants[2]), "after a rejected update"

    # poses in stream order
    t.enable_model_pose()
    names = [m[0] for m in t.models()]
    m = np.tile(np.eye(3, 4, dtype=F), (len(names), 1, 1))
    m[names.index("bunny"), :, 3] = (0.25, 0.125, -0.5)
    t.set_model_transforms(m, enqueue=True)
    posed = check(enqueued(), "fr_set_model_transforms_enqueue")
    assert not rc.same_records(posed, wants[2])
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 5. Stream order of the caller's arrays
# ---------------------------------------------------------------------------------------------
def test_enqueued_form_orders_the_callers_streams(fovrt_mod, oracle, still):
    import torch
    _a, _osc, _nsc, sets = refs(fovrt_mod, oracle, 1)
    r, want = sets["random"]
    n = len(r)
    t = still(1)
    src = dev(rc.fr_rays(r))
    rays = torch.zeros_like(src)
    out, copy = out_hits(n), out_hits(n, 0.0)
    ballast = torch.ones(32 << 20, device="cuda:0")
    producer, consumer = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    settle()
    with torch.cuda.stream(producer):
        for _ in range(8):
            ballast.mul_(1.0001)
        rays.copy_(src)  # the rays are still being written when the call below is made
        ev = torch.cuda.Event()
        ev.record(producer)
    t.trace_rays_enqueue(rays, out, n=n, ready_event=ev)
    t.rays_consumed(consumer)
    with torch.cuda.stream(consumer):
        copy.copy_(out)
    t.rays_consumed(producer)
    with torch.cuda.stream(producer):
        rays.fill_(float("nan"))  # garbage, right after the query has read them
    t.synchronize()
    settle()
    got = hits_of(copy)
    assert rc.same_records(got, want), report(got, want, r)
    assert rc.same_records(hits_of(out), want)
    sync = query(t, r, "device")
    assert rc.same_records(sync, got)


# ---------------------------------------------------------------------------------------------
# 6. Frames untouched
# ---------------------------------------------------------------------------------------------
def frame_buffers(fovrt):
    TN = fovrt.TextureName
    return (TN.POSITION, TN.NORMAL, TN.DEPTH, TN.DIFFUSE, TN.WEIGHT, TN.HISTORY, TN.SHADING, TN.EXTRA, TN.JFA_COORD,
            TN.JFA_COLOR, TN.SIBSON, TN.PULLPUSH, TN.ATROUS, TN.DEPTH_CACHE, TN.HISTORY_CACHE, TN.MASK, TN.GCLASS)


@pytest.mark.parametrize("every_frame", [True, False])
@pytest.mark.parametrize("latency", [False, True])
def test_queries_leave_frames_untouched(fovrt_mod, oracle, latency, every_frame):
    """every_frame: the buffers are compared after every frame (which drains the pipeline each time); otherwise only
    after the sixth, so that the six frames and the queries between them are in flight together."""
    W, H = 160, 96
    _a, _osc, _nsc, sets = refs(fovrt_mod, oracle, 1)
    r, want = sets["random"]
    n = len(r)
    a, b = (mk(fovrt_mod, 1, W=W, H=H, mask_mode=4, spp=2) for _ in range(2))
    for t in (a, b):
        if latency:
            t.set_pipeline_mode(fovrt_mod.PIPELINE_LATENCY)
    rays = dev(rc.fr_rays(r))
    outs = [out_hits(n) for _ in range(6)]
    settle()
    cam = tc.camera(fovrt_mod, "along_z", W, H)

    def compare(what):
        for tid in frame_buffers(fovrt_mod):
            assert equal_nan(a.read(tid), b.read(tid)), (what, tid)

    for f in range(6):
        cam.setPrevState()
        cam.lookAt(np.asarray(cam.target) + np.array(tc.PAN_STEP, F))
        for t in (a, b):
            t.update_optix_variables(cam)
        a.trace_rays_enqueue(rays, outs[f], n=n)
        a.frame(timing=False)
        b.frame(timing=False)
        if f == 3:
            got = query(a, r, "host")
            assert rc.same_records(got, want)
        if every_frame:
            compare(f"frame {f}")
    compare("the last frame")
    assert a.stats() == b.stats()
    assert a.jfa_reuse_count() == b.jfa_reuse_count()
    assert a.snapshot() == b.snapshot()
    a.synchronize()
    for out in outs:
        assert rc.same_records(hits_of(out), want)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 7. Refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_write_nothing(fovrt_mod, oracle):
    import ctypes as C
    import torch
    lib = fovrt_mod.load_library()
    _a, _osc, _nsc, sets = refs(fovrt_mod, oracle, 0)
    r, want = sets["random"]
    r, want = r[:100], want[:100]
    n = len(r)
    t = mk(fovrt_mod, 0)
    ctx = t._ctx
    fr = rc.fr_rays(r)
    rays = dev(fr)
    big = torch.full((2 * n + 1, 4), 7.0, dtype=torch.float32, device="cuda:0")  # out, prefilled
    host_out = np.full((n, 4), 7.0, F)
    settle()
    INV, UNS, DEV, HOST = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_UNSUPPORTED, fovrt_mod.FR_MEM_DEVICE, fovrt_mod.FR_MEM_HOST
    rp, op, hp, hop = rays.data_ptr(), big.data_ptr(), fr.ctypes.data, host_out.ctypes.data
    p = C.c_void_p

    def refused(code, what, sync=None, enq=None):
        if sync is not None:
            assert lib.fr_trace_rays(ctx, *sync) == code, what
        if enq is not None:
            assert lib.fr_trace_rays_enqueue(ctx, *enq) == code, what
        t.synchronize()
        settle()
        assert (big.cpu().numpy() == 7.0).all() and (host_out == 7.0).all(), what
        got = query(t, r, "device")  # the next query is right
        assert rc.same_records(got, want), what

    refused(INV, "NULL rays", (None, n, DEV, 0, p(op)), (None, n, 0, p(op), None))
    refused(INV, "NULL out", (p(rp), n, DEV, 0, None), (p(rp), n, 0, None, None))
    refused(INV, "NULL host rays", (None, n, HOST, 0, p(hop)))
    refused(INV, "bad kind", (p(rp), n, DEV, 2, p(op)), (p(rp), n, -1, p(op), None))
    refused(INV, "bad where", (p(rp), n, 2, 0, p(op)))
    refused(INV, "n > 2^30", (p(rp), (1 << 30) + 1, DEV, 0, p(op)), (p(rp), (1 << 30) + 1, 0, p(op), None))
    refused(INV, "rays not aligned", (p(rp + 4), n - 1, DEV, 0, p(op)), (p(rp + 8), n - 1, 0, p(op), None))
    refused(INV, "hits not aligned", (p(rp), n, DEV, 0, p(op + 4)), (p(rp), n, 0, p(op + 8), None))
    refused(INV, "transmittance not aligned", (p(rp), n, DEV, 1, p(op + 2)), (p(rp), n, 1, p(op + 1), None))
    both = torch.full((3 * n, 4), 7.0, dtype=torch.float32, device="cuda:0")
    settle()
    bp = both.data_ptr()
    refused(INV, "overlap", (p(bp), n, DEV, 0, p(bp + 16 * n)), (p(bp + 16), n, 0, p(bp), None))
    assert (both.cpu().numpy() == 7.0).all()
    assert "overlap" in t.last_error()
    # n == 0 is accepted and writes nothing
    assert lib.fr_trace_rays(ctx, p(rp), 0, DEV, 0, p(op)) == 0
    assert lib.fr_trace_rays(ctx, None, 0, HOST, 0, None) == 0
    assert lib.fr_trace_rays_enqueue(ctx, p(rp), 0, 0, p(op), None) == 0
    refused(0, "n == 0")
    # transmittance answers into a 4-byte aligned array
    s = rc.shadow_rows(rc.scene_arrays(fovrt_mod, 0))[:64]
    sd = dev(rc.fr_rays(s))
    tout = torch.full((65,), 7.0, dtype=torch.float32, device="cuda:0")
    settle()
    assert lib.fr_trace_rays(ctx, p(sd.data_ptr()), 64, DEV, 1, p(tout.data_ptr() + 4)) == 0
    check_transmittance(tout.cpu().numpy()[1:], rc.shadow_np(tn.SceneNp(rc.scene_arrays(fovrt_mod, 0)), s))
    assert tout.cpu().numpy()[0] == 7.0
    # a host batch above the reservation
    assert lib.fr_trace_rays(ctx, p(hp), n, HOST, 0, p(hop)) == INV
    assert "reservation of 0" in t.last_error(), t.last_error()
    assert lib.fr_ray_query_reserve(ctx, n - 1) == 0
    assert lib.fr_trace_rays(ctx, p(hp), n, HOST, 0, p(hop)) == INV
    assert f"reservation of {n - 1}" in t.last_error(), t.last_error()
    assert (host_out == 7.0).all()
    assert lib.fr_ray_query_reserve(ctx, n) == 0
    assert lib.fr_ray_query_reserve(ctx, 1) == 0  # (never shrinks)
    assert lib.fr_trace_rays(ctx, p(hp), n, HOST, 0, p(hop)) == 0
    assert rc.same_records(host_out.view(rc.HIT_DTYPE).reshape(-1), want)
    assert lib.fr_ray_query_reserve(ctx, (1 << 30) + 1) == INV
    # the enqueued form on a sharded context; the synchronous form answers there
    t.destroy()
    W, H = 160, 96  # (the shard plan of test_gpu_rebuild_enqueue's refusal test)
    t = mk(fovrt_mod, 0, W=W, H=H)
    t.set_shard_plan(0, 2, 32, fovrt_mod.shard_plan(W, H, 32, 2))
    assert lib.fr_trace_rays_enqueue(t._ctx, p(rp), n, 0, p(op), None) == UNS
    assert "sharded" in t.last_error()
    t.synchronize()
    assert (big.cpu().numpy() == 7.0).all()
    got = query(t, r, "device")
    assert rc.same_records(got, want)
    assert rc.same_records(query(t, r, "host"), want)
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 8. Outside the guaranteed domain
# ---------------------------------------------------------------------------------------------
def test_far_origins_return_only_true_hits(fovrt_mod, oracle, still):
    """Origins 1e4 units out: every hit returned is the bits of that triangle's own test, inside the window.
    Closestness is not asserted."""
    a, _osc, nsc, _sets = refs(fovrt_mod, oracle, 1)
    r = rc.far_rows(a)
    got = query(still(1), r, "device")
    hit = got["prim"] >= 0
    print("far origins: hits", int(hit.sum()), "of", len(r))
    assert (got[~hit] == rc.MISS).all()
    for q, h in zip(r[hit], got[hit]):
        ok, tt, b, g = nsc._tests(q[0:3], q[3:6], q[6], q[7])
        k = int(h["prim"])
        assert ok[k] and (tt[k], b[k], g[k]) == (h["t"], h["beta"], h["gamma"]), (k, h)
        assert q[6] < h["t"] < q[7]
