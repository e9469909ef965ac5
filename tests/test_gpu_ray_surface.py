"""GPU suite for the second part of the ray queries (fr_trace_rays_masked, fr_trace_rays_masked_enqueue,
fr_ray_query_reserve_kind): FR_RAYS_SURFACE against the numpy restatement of the closest-hit programs, against
FR_RAYS_CLOSEST and against the context's own G-buffer, bit for bit; per-ray model masks against the oracle's brute
force over the scene with the excluded models collapsed; the scene such queries see while it moves, in place and
overlapped; frames untouched; refusals. The cases are tests/ray_surface_cases.py's, whose preconditions
tests/test_cpu_ray_surface.py asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_cases as rc
import ray_surface_cases as rs
import trace_cases as tc
import trace_np as tn
from helpers import equal_nan
from test_cpu_ray_queries import refs
from test_cpu_ray_surface import aimed
from test_cpu_rebuild_policy import mild
from test_gpu_ray_queries import check_transmittance, frame_buffers

pytestmark = pytest.mark.gpu

F = np.float32
CAMERA_VIEWS = {0: ["box_close", "inside_box"], 1: ["bunny_close", "along_z"]}
_TRACERS = {}
_SURF = {}


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
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def settle():
    import torch
    torch.cuda.synchronize()


WORDS = {"closest": 4, "transmittance": 1, "surface": 20}
DTYPES = {"closest": rc.HIT_DTYPE, "transmittance": np.dtype(F), "surface": rs.SURFACE_DTYPE}


def out_buf(n, kind, fill=np.nan):
    import torch
    return torch.full((n, WORDS[kind]), fill, dtype=torch.float32, device="cuda:0")


def records(x, kind):
    return x.cpu().numpy().view(DTYPES[kind]).reshape(-1)


def query(t, r, where, kind="closest", masks=None):
    """The synchronous form over rows (o, d, tmin, tmax), from host or from device memory."""
    fr = rc.fr_rays(r)
    if where == "host":
        return t.trace_rays(fr, kind, masks=masks)
    x, m = dev(fr), (dev(masks) if masks is not None else None)
    out = out_buf(len(fr), kind)
    settle()
    t.trace_rays(x, kind, out=out, n=len(fr), masks=m)
    return records(out, kind)


def report(got, want, r):
    if got.dtype.names is None:
        bad = np.nonzero(got != want)[0]
        return f"{len(bad)} differ" if len(bad) else "equal"
    bad = np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[0]
    if not len(bad):
        return "equal"
    i = bad[0]
    fields = [n for n in got.dtype.names if got[i][n].tobytes() != want[i][n].tobytes()]
    return (f"{len(bad)} of {len(got)} differ; first {i} in {fields}: gpu {got[i]} reference {want[i]} "
            f"ray {np.asarray(r)[i].tolist()}")


def surface_ref(fovrt, oracle, scene, name):
    """(rows, unmasked brute-force hits, surface_np records) of a base set of a still scene, computed once."""
    if (scene, name) not in _SURF:
        a, _osc, nsc, sets = refs(fovrt, oracle, scene)
        r, hits = sets[name]
        _SURF[scene, name] = (r, hits, rs.surface_np(nsc, r, hits, rs.models(fovrt, scene)))
    return _SURF[scene, name]


# ---------------------------------------------------------------------------------------------
# 1. Surface on camera rays: FR_RAYS_CLOSEST, the G-buffer, the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1, 2])
@pytest.mark.parametrize("scene", [0, 1])
def test_surface_on_camera_rays_equals_the_gbuffer_and_the_restatement(fovrt_mod, oracle, still, scene, builder):
    W, H = rc.SIZE
    TN = fovrt_mod.TextureName
    t = still(scene, builder)
    for name in CAMERA_VIEWS[scene]:
        r, hits, want = surface_ref(fovrt_mod, oracle, scene, f"view_{name}")
        got = query(t, r, "device", "surface")
        assert got.dtype == rs.SURFACE_DTYPE and len(got) == W * H
        closest = query(t, r, "device")
        for f in ("t", "beta", "gamma", "prim"):
            assert got[f].tobytes() == closest[f].tobytes(), (name, f)
        assert rc.same_records(closest, hits), name
        t.update_optix_variables(tc.camera(fovrt_mod, name, W, H))
        t.geometry_launch()
        pos, nrm, dif = (t.read(b).reshape(-1, 4) for b in (TN.POSITION, TN.NORMAL, TN.DIFFUSE))
        gclass = t.read(TN.GCLASS).reshape(-1)
        hit = got["prim"] >= 0
        assert np.array_equal(got["point"][hit], pos[hit, :3]), name
        half = (got["ng"][hit].astype(np.float64) * 0.5 + 0.5).astype(F)  # (one rounding, as fma(ng, 0.5, 0.5))
        assert np.array_equal(half, nrm[hit, :3]), name
        assert np.array_equal(got["kd"][hit], dif[hit, :3]), name
        assert np.array_equal(rs.class_of_type(got), gclass), name
        assert rc.same_records(got, want), (name, report(got, want, r))
        assert rc.same_records(query(t, r, "host", "surface"), want), name


# ---------------------------------------------------------------------------------------------
# 2. Surface on the other sets
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [0, 1])
def test_surface_on_random_zero_and_edge_sets(fovrt_mod, oracle, still, scene):
    a, _osc, _nsc, sets = refs(fovrt_mod, oracle, scene)
    t = still(scene)
    seen = np.zeros(0, np.int32)
    for name in ("random", "zeros") + (("edges",) if scene == 0 else ()):
        r, hits, want = surface_ref(fovrt_mod, oracle, scene, name)
        for where in ("host", "device"):
            got = query(t, r, where, "surface")
            assert rc.same_records(got, want), (name, where, report(got, want, r))
        assert (want[hits["prim"] < 0] == rs.miss_surface()).all() and ((hits["prim"] < 0).any() or name != "random")
        seen = np.concatenate([seen, want["surface"][hits["prim"] >= 0]])
        if name == "random":
            ln = np.linalg.norm(r[:, 3:6].astype(np.float64), axis=1)[hits["prim"] >= 0]
            assert (ln < 0.5).any() and (ln > 2.0).any()  # unnormalised directions among the hits
    # back and front faces, and what the scenes' triangles carry: the procedural scenes give every triangle normals
    # and uv (triangles without them: test_surface_on_triangles_without_normals_and_uv)
    assert ((seen >> 18) & 1).any() and not ((seen >> 18) & 1).all()
    flags = np.asarray(a["flags"])
    assert set(((seen >> 16) & 3).tolist()) == set(((flags >> 8) & 3).tolist())
    d, _good = rc.degenerate_rows(a)
    for where in ("host", "device"):
        got = query(t, d, where, "surface")
        assert (got == rs.miss_surface()).all(), where


def test_surface_on_triangles_without_normals_and_uv(fovrt_mod, oracle, tmp_path):
    """The OBJ scenes of ray_surface_cases: a box with vertex normals and no uv (flags & 0x300 == 0x100) and one with
    neither (0), beside a ground with both. The whole record equals surface_np on camera rays and on rays at every
    triangle from both sides; every flag combination occurs among the hits; the context's own G-buffer agrees."""
    from test_cpu_ray_surface import check_obj_records, obj_refs
    W, H = rc.SIZE
    TN = fovrt_mod.TextureName
    seen = set()
    for name in rs.OBJ_SCENES:
        a, ms, r, hits, want = obj_refs(fovrt_mod, oracle, tmp_path, name)
        t = fovrt_mod.PathTracer(rs.obj_scene_config(fovrt_mod, tmp_path, name))
        assert t.initialize(), t.last_error()
        assert t.models() == ms and t.scene_arrays()["flags"].tobytes() == np.asarray(a["flags"]).tobytes()
        for where in ("host", "device"):
            got = query(t, r, where, "surface")
            assert rc.same_records(got, want), (name, where, report(got, want, r))
        seen |= check_obj_records(a, name, hits, got)
        t.update_optix_variables(rs.obj_camera(fovrt_mod))
        t.geometry_launch()
        cam = got[:W * H]
        hit = cam["prim"] >= 0
        pos, nrm, dif = (t.read(b).reshape(-1, 4) for b in (TN.POSITION, TN.NORMAL, TN.DIFFUSE))
        assert np.array_equal(cam["point"][hit], pos[hit, :3]), name
        half = (cam["ng"][hit].astype(np.float64) * 0.5 + 0.5).astype(F)
        assert np.array_equal(half, nrm[hit, :3]) and np.array_equal(cam["kd"][hit], dif[hit, :3]), name
        assert np.array_equal(rs.class_of_type(cam), t.read(TN.GCLASS).reshape(-1)), name
        # masks on such a scene: the box alone, the ground alone
        masks = np.tile(np.array([1, 2], np.uint32), (len(r) + 1) // 2)[:len(r)]
        mh = rs.masked_reference(oracle, a, ms, r, masks)
        mw = rs.surface_np(tn.SceneNp(a), r, mh, ms)
        got = query(t, r, "device", "surface", masks)
        assert rc.same_records(got, mw), (name, "masked", report(got, mw, r))
        t.destroy()
    assert seen == {0x300, 0x100, 0}


def test_null_masks_through_the_masked_calls_are_the_unmasked_calls(fovrt_mod, oracle, still):
    """fr_trace_rays_masked and fr_trace_rays_masked_enqueue with masks = NULL, kinds 0 and 1, against fr_trace_rays
    and fr_trace_rays_enqueue: the same bits (the facade never takes this route: it sends such a query to the old
    calls)."""
    import torch
    lib = fovrt_mod.load_library()
    t = still(1)
    ctx = t._ctx
    p = C.c_void_p
    DEV, HOST = fovrt_mod.FR_MEM_DEVICE, fovrt_mod.FR_MEM_HOST
    _a, _ms, r, _masks, plain, _brute = aimed(fovrt_mod, oracle, 1)
    s = rc.shadow_rows(rc.scene_arrays(fovrt_mod, 1))
    for kind, rows_ in ((0, r), (1, s)):
        fr = rc.fr_rays(rows_)
        n = len(fr)
        name = "closest" if kind == 0 else "transmittance"
        x = dev(fr)
        outs = [out_buf(n, name) for _ in range(4)]
        settle()
        assert lib.fr_trace_rays(ctx, p(x.data_ptr()), n, DEV, kind, p(outs[0].data_ptr())) == 0
        assert lib.fr_trace_rays_masked(ctx, p(x.data_ptr()), None, n, DEV, kind, p(outs[1].data_ptr())) == 0, t.last_error()
        assert lib.fr_trace_rays_enqueue(ctx, p(x.data_ptr()), n, kind, p(outs[2].data_ptr()), None) == 0
        assert lib.fr_trace_rays_masked_enqueue(ctx, p(x.data_ptr()), None, n, kind, p(outs[3].data_ptr()), None) == 0
        t.synchronize()
        settle()
        ref = outs[0].cpu().numpy().tobytes()
        assert not np.isnan(outs[0].cpu().numpy()).any()
        for k in (1, 2, 3):
            assert outs[k].cpu().numpy().tobytes() == ref, (name, k)
        if kind == 0:
            assert rc.same_records(records(outs[0], name), plain)
        # the host form: the plain reservation serves the masked call with NULL masks, as it serves fr_trace_rays
        h0, h1 = np.full((n, WORDS[name]), 7.0, F), np.full((n, WORDS[name]), 7.0, F)
        assert lib.fr_ray_query_reserve(ctx, n) == 0
        assert lib.fr_trace_rays(ctx, p(fr.ctypes.data), n, HOST, kind, p(h0.ctypes.data)) == 0
        assert lib.fr_trace_rays_masked(ctx, p(fr.ctypes.data), None, n, HOST, kind, p(h1.ctypes.data)) == 0, t.last_error()
        assert h0.tobytes() == h1.tobytes() == ref, name


def test_tie_pairs_report_the_lower_triangles_surface(fovrt_mod, oracle):
    a = rc.scene_arrays(fovrt_mod, 0)
    ms = rs.models(fovrt_mod, 0)
    t = mk(fovrt_mod, 0)
    t.set_positions(rc.tie_positions(a), update="rebuild")
    moved = t.scene_arrays()
    r = rc.tie_rows(a)
    hits = rc.hit_records(oracle.OracleScene(moved).closest(r, brute=True))
    assert np.isin(hits["prim"], [s for _d, s in rc.TIE_PAIRS]).sum() >= 50
    want = rs.surface_np(tn.SceneNp(moved), r, hits, ms)
    for where in ("host", "device"):
        got = query(t, r, where, "surface")
        assert rc.same_records(got, want), (where, report(got, want, r))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 3. Batch sizes, refills and the staging area
# ---------------------------------------------------------------------------------------------
def test_every_batch_size_with_one_block(fovrt_mod, oracle):
    """FOVRT_RAYQ_BLOCKS=1: two waves answer up to eight chunks of rays that alternate misses and deep hits."""
    lib = fovrt_mod.load_library()
    r, hits, want = surface_ref(fovrt_mod, oracle, 1, "refill")
    ms = rs.models(fovrt_mod, 1)
    rng = np.random.default_rng(41)
    masks = rng.integers(0, 1 << len(ms), len(r)).astype(np.uint32) | np.uint32(1 << 2)  # (the bunny stays in)
    a = rc.scene_arrays(fovrt_mod, 1)
    mwant = rs.surface_np(tn.SceneNp(a), r, rs.masked_reference(oracle, a, ms, r, masks), ms)
    os.environ["FOVRT_RAYQ_BLOCKS"] = "1"
    try:
        t = mk(fovrt_mod, 1)
    finally:
        del os.environ["FOVRT_RAYQ_BLOCKS"]
    p = C.c_void_p
    for n in rc.BATCH_SIZES:
        rn, wn, mn, mwn = r[len(r) - n:], want[len(r) - n:], masks[len(r) - n:], mwant[len(r) - n:]
        got = query(t, rn, "device", "surface")
        assert len(got) == n and rc.same_records(got, wn), (n, report(got, wn, rn))
        got = query(t, rn, "device", "surface", mn)
        assert rc.same_records(got, mwn), (n, "masked", report(got, mwn, rn))
        # the host form: a plain reservation of n rays (48 B each) does not hold n surface records
        fr, mc = rc.fr_rays(rn), np.ascontiguousarray(mn)
        out = np.full((n, 20), 7.0, F)
        assert lib.fr_ray_query_reserve(t._ctx, n) == 0
        assert lib.fr_trace_rays_masked(t._ctx, p(fr.ctypes.data), p(mc.ctypes.data), n, fovrt_mod.FR_MEM_HOST, 2,
                                        p(out.ctypes.data)) == fovrt_mod.FR_E_INVALID, n
        assert "fr_ray_query_reserve_kind" in t.last_error() and (out == 7.0).all()
        assert lib.fr_ray_query_reserve_kind(t._ctx, n, 2, 1) == 0
        assert lib.fr_trace_rays_masked(t._ctx, p(fr.ctypes.data), p(mc.ctypes.data), n, fovrt_mod.FR_MEM_HOST, 2,
                                        p(out.ctypes.data)) == 0, t.last_error()
        assert rc.same_records(out.view(rs.SURFACE_DTYPE).reshape(-1), mwn), (n, "host")
        assert rc.same_records(query(t, rn, "host", "surface"), wn), (n, "host, unmasked")
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 4. Masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("scene", [0, 1])
def test_masked_queries_equal_the_masked_references(fovrt_mod, oracle, still, scene, where):
    a, ms, r, masks, plain, brute = aimed(fovrt_mod, oracle, scene)
    t = still(scene)
    got = query(t, r, where, "closest", masks)
    assert rc.same_records(got, brute), report(got, brute, r)
    if ("aimed", scene) not in _SURF:
        _SURF["aimed", scene] = rs.surface_np(tn.SceneNp(a), r, brute, ms)
    want = _SURF["aimed", scene]
    got = query(t, r, where, "surface", masks)
    assert rc.same_records(got, want), report(got, want, r)
    # bits above the model count are ignored; masks = NULL is the unmasked call; mask 0 is a miss or 1.0
    high = masks | np.uint32(0xFFFFFF00)
    assert rc.same_records(query(t, r, where, "closest", high), brute)
    every = np.full(len(r), (1 << len(ms)) - 1, np.uint32)
    assert rc.same_records(query(t, r, where, "closest", every), plain)
    assert rc.same_records(query(t, r, where, "closest"), plain)
    none = np.full(len(r), 0xFFFFFFFF & ~((1 << len(ms)) - 1), np.uint32)
    assert (query(t, r, where, "closest", none) == rc.MISS).all()
    assert (query(t, r, where, "surface", none) == rs.miss_surface()).all()
    assert (query(t, r, where, "transmittance", none) == 1).all()


@pytest.mark.parametrize("scene", [0, 1])
def test_masked_transmittance_on_the_aimed_set(fovrt_mod, oracle, still, scene):
    """Exactly 0 and 1 where the restatement says so, within one ulp between. These rays' directions are not unit
    vectors (0.1 to 10), which spreads |ns.d| over the whole range of the Schlick term's power. With the platform's
    powf, which the frame's shadow rays and the unmasked queries use, the device missed this bound here (measured:
    up to 5 ulp in scene 0 and 94 in scene 1, masked or not; each such answer is reached from the restatement's by
    one last bit of one power, which 1 - schlick magnifies where the power is near 1). The masked queries round the
    power once, x^5 in f64 (schlick5_rounded_once, k_trace.hip), which is glibc's powf on every factor of these
    sets."""
    a, ms, r, masks, _plain, _brute = aimed(fovrt_mod, oracle, scene)
    want = rs.masked_np(a, ms, r, masks, "shadow")
    for where in ("host", "device"):
        check_transmittance(query(still(scene), r, where, "transmittance", masks), want)


def test_masked_transmittance_on_the_shadow_set(fovrt_mod, still):
    for scene in (0, 1):
        a, ms = rc.scene_arrays(fovrt_mod, scene), rs.models(fovrt_mod, scene)
        s = rc.shadow_rows(a)
        masks = rs.shadow_masks(ms, len(s))
        want = rs.masked_np(a, ms, s, masks, "shadow")
        for where in ("host", "device"):
            check_transmittance(query(still(scene), s, where, "transmittance", masks), want)


def test_the_model_edge_inside_one_chunk(fovrt_mod, oracle, still):
    """Scene 0's triangles 1 (the ground's last) and 2 (the box's first): rays at both, masks 01 and 10 by turns."""
    a, ms = rc.scene_arrays(fovrt_mod, 0), rs.models(fovrt_mod, 0)
    assert ms[0][1:] == (0, 2) and ms[1][1] == 2
    rng = np.random.default_rng(43)
    tris = np.tile([1, 2], 32)
    p = rc._points_on(a, tris, rng)
    o = p + np.array([0.3, 2.0, 0.4]) + rng.normal(size=p.shape) * 0.1
    r = rc.rows(o, p - o)
    masks = np.tile(np.array([1, 1, 2, 2], np.uint32), 16)
    want = rs.masked_reference(oracle, a, ms, r, masks)
    plain = rc.hit_records(oracle.OracleScene(a).closest(r, brute=True))
    assert (plain["prim"][0::2] == 1).sum() >= 16 and (plain["prim"][1::2] == 2).sum() >= 16
    assert not rc.same_records(want, plain)
    assert (rs.model_of(ms, want["prim"])[want["prim"] >= 0] == np.log2(masks[want["prim"] >= 0])).all()
    for where in ("host", "device"):
        got = query(still(0), r, where, "closest", masks)
        assert rc.same_records(got, want), (where, report(got, want, r))


# ---------------------------------------------------------------------------------------------
# 5. The moving scene
# ---------------------------------------------------------------------------------------------
def moving_refs(oracle, arrays, ms, r, masks):
    hits = rs.masked_reference(oracle, arrays, ms, r, masks)
    return hits, rs.surface_np(tn.SceneNp(arrays), r, hits, ms)


@pytest.mark.parametrize("overlap", [False, True])
def test_surface_and_masks_see_the_scene_at_their_place_in_the_stream(fovrt_mod, oracle, overlap):
    _a, ms, r, masks, _plain, _brute = aimed(fovrt_mod, oracle, 1)
    r, masks = r[::3], masks[::3]
    n = len(r)
    t = mk(fovrt_mod, 1, builder=2)
    t.set_geometry_overlap(overlap)
    base = t.scene_arrays()["pos"].reshape(-1, 3, 3).copy()
    rays, dmasks = dev(rc.fr_rays(r)), dev(masks)
    xd = dev(mild(base, 2).reshape(-1, 9))
    settle()

    def enqueued(kind):
        out = out_buf(n, kind)
        settle()
        t.trace_rays_enqueue(rays, out, n=n, kind=kind, masks=dmasks)
        return out

    # an enqueued update with recomputed normals, then the two queries
    t.update_geometry_enqueue(xd, normals="recompute")
    oc, osf = enqueued("closest"), enqueued("surface")
    t.synchronize()
    moved = t.scene_arrays()
    assert moved["pos"].tobytes() == mild(base, 2).tobytes()
    hits, want = moving_refs(oracle, moved, ms, r, masks)
    first = hits
    assert rc.same_records(records(oc, "closest"), hits), report(records(oc, "closest"), hits, r)
    assert rc.same_records(records(osf, "surface"), want), report(records(osf, "surface"), want, r)

    # poses in stream order: each pose's arrays are taken from a synchronous pose first (a pose is a function of
    # the rest geometry alone), then three pose-then-query pairs go back to back with no host wait between them
    t.enable_model_pose()
    names = [m[0] for m in ms]
    poses, wants = [], []
    for k in range(3):
        m = np.tile(np.eye(3, 4, dtype=F), (len(names), 1, 1))
        m[names.index("bunny"), :, 3] = (0.25 * (k + 1), 0.125, -0.5 + 0.2 * k)
        m[names.index("earth"), :, 3] = (0.0, 0.1 * k, 0.3)
        poses.append(m)
        t.set_model_transforms(m)
        wants.append(moving_refs(oracle, t.scene_arrays(), ms, r, masks))
    assert not rc.same_records(wants[0][0], first) and not rc.same_records(wants[0][0], wants[1][0])
    assert not rc.same_records(wants[1][0], wants[2][0])
    t.set_model_transforms(poses[2], enqueue=True)
    osf = enqueued("surface")
    t.synchronize()
    assert rc.same_records(records(osf, "surface"), wants[2][1]), "fr_set_model_transforms_enqueue"
    outs = [(out_buf(n, "closest"), out_buf(n, "surface")) for _ in range(3)]
    settle()
    for m, (oc, osf) in zip(poses, outs):
        t.set_model_transforms(m, enqueue=True)
        t.trace_rays_enqueue(rays, oc, n=n, kind="closest", masks=dmasks)
        t.trace_rays_enqueue(rays, osf, n=n, kind="surface", masks=dmasks)
    t.synchronize()
    for k, ((oc, osf), (hits, want)) in enumerate(zip(outs, wants)):
        assert rc.same_records(records(oc, "closest"), hits), (f"pair {k}", report(records(oc, "closest"), hits, r))
        assert rc.same_records(records(osf, "surface"), want), (f"pair {k}", report(records(osf, "surface"), want, r))
    t.destroy()


# ---------------------------------------------------------------------------------------------
# 6. Frames untouched
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latency", [False, True])
def test_masked_surface_queries_leave_frames_untouched(fovrt_mod, oracle, latency):
    W, H = 160, 96
    _a, _ms, r, masks, _plain, _brute = aimed(fovrt_mod, oracle, 1)
    n = len(r)
    a, b = (mk(fovrt_mod, 1, W=W, H=H, mask_mode=4, spp=2) for _ in range(2))
    for t in (a, b):
        if latency:
            t.set_pipeline_mode(fovrt_mod.PIPELINE_LATENCY)
    rays, dmasks = dev(rc.fr_rays(r)), dev(masks)
    outs = [out_buf(n, "surface") for _ in range(6)]
    settle()
    cam = tc.camera(fovrt_mod, "along_z", W, H)
    for f in range(6):
        cam.setPrevState()
        cam.lookAt(np.asarray(cam.target) + np.array(tc.PAN_STEP, F))
        for t in (a, b):
            t.update_optix_variables(cam)
        a.trace_rays_enqueue(rays, outs[f], n=n, kind="surface", masks=dmasks)
        a.frame(timing=False)
        b.frame(timing=False)
    for tid in frame_buffers(fovrt_mod):
        assert equal_nan(a.read(tid), b.read(tid)), tid
    assert a.stats() == b.stats()
    assert a.jfa_reuse_count() == b.jfa_reuse_count()
    assert a.snapshot() == b.snapshot()
    a.synchronize()
    if ("aimed", 1) not in _SURF:
        _SURF["aimed", 1] = rs.surface_np(tn.SceneNp(_a), r, _brute, _ms)
    want = _SURF["aimed", 1]
    for out in outs:
        assert rc.same_records(records(out, "surface"), want)
    a.destroy(); b.destroy()


# ---------------------------------------------------------------------------------------------
# 7. Refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_write_nothing(fovrt_mod, oracle):
    import torch
    lib = fovrt_mod.load_library()
    a, ms, r, masks, _plain, brute = aimed(fovrt_mod, oracle, 0)
    r, masks, brute = r[:100], masks[:100], brute[:100]
    n = len(r)
    t = mk(fovrt_mod, 0)
    ctx = t._ctx
    fr = rc.fr_rays(r)
    # one allocation: a gap | rays | masks | out, so that every overlap below is between known addresses inside it
    gap = 16 * n + 16
    arena = torch.full(((gap + 32 * n + 4 * n + 16 + 80 * (n + 2)) // 4,), 7.0, dtype=torch.float32, device="cuda:0")
    base = arena.data_ptr()
    assert base % 16 == 0
    rp = base + gap
    mp = rp + 32 * n
    op = (mp + 4 * n + 15) // 16 * 16
    assert op + 80 * (n + 1) <= base + 4 * arena.numel()
    rw, mw, ow = (rp - base) // 4, (mp - base) // 4, (op - base) // 4
    arena[rw:rw + 8 * n] = torch.from_numpy(fr.reshape(-1)).to("cuda:0")
    arena[mw:mw + n] = torch.from_numpy(masks.view(F)).to("cuda:0")
    host_out = np.full((n, 20), 7.0, F)
    settle()
    INV, UNS, DEV, HOST = fovrt_mod.FR_E_INVALID, fovrt_mod.FR_E_UNSUPPORTED, fovrt_mod.FR_MEM_DEVICE, fovrt_mod.FR_MEM_HOST
    p = C.c_void_p
    out_words = slice(ow, None)

    def refused(code, what, sync=None, enq=None):
        if sync is not None:
            assert lib.fr_trace_rays_masked(ctx, *sync) == code, (what, t.last_error())
        if enq is not None:
            assert lib.fr_trace_rays_masked_enqueue(ctx, *enq) == code, (what, t.last_error())
        t.synchronize()
        settle()
        host = arena.cpu().numpy()
        assert (host[out_words] == 7.0).all() and (host[:rw] == 7.0).all() and (host_out == 7.0).all(), what
        assert host[rw:rw + 8 * n].tobytes() == fr.tobytes() and host[mw:mw + n].tobytes() == masks.tobytes(), what

    refused(INV, "masks not aligned", (p(rp), p(mp + 2), n - 1, DEV, 0, p(op)), (p(rp), p(mp + 1), n - 1, 0, p(op), None))
    refused(INV, "surface out not aligned", (p(rp), p(mp), n, DEV, 2, p(op + 8)), (p(rp), None, n, 2, p(op + 4), None))
    refused(INV, "bad kind", (p(rp), p(mp), n, DEV, 3, p(op)), (p(rp), p(mp), n, -1, p(op), None))
    refused(INV, "bad where", (p(rp), p(mp), n, 2, 2, p(op)))
    refused(INV, "NULL out", (p(rp), p(mp), n, DEV, 2, None), (p(rp), p(mp), n, 2, None, None))
    # overlaps: out below the rays so that only an 80-byte stride reaches them; out below the masks likewise
    lo = rp - 16 * n - 16  # (16 n + 16 bytes below the rays: clear of them at 16 B per ray, into them at 80)
    assert lib.fr_trace_rays_masked(ctx, p(rp), None, n, DEV, 2, p(lo)) == INV and "rays and out overlap" in t.last_error()
    refused(INV, "rays and surface out", None, (p(rp), None, n, 2, p(lo), None))
    refused(INV, "masks and out", (p(rp), p(op + 16), n, DEV, 0, p(op)), (p(rp), p(op + 80 * n - 4), n, 2, p(op), None))
    assert "masks and out overlap" in t.last_error()
    # the unmasked calls keep their two kinds
    assert lib.fr_trace_rays(ctx, p(rp), n, DEV, 2, p(op)) == INV
    assert lib.fr_trace_rays_enqueue(ctx, p(rp), n, 2, p(op), None) == INV
    refused(INV, "kind 2 through fr_trace_rays")
    # a host batch above the area
    hm = np.ascontiguousarray(masks)
    assert lib.fr_trace_rays_masked(ctx, p(fr.ctypes.data), p(hm.ctypes.data), n, HOST, 2, p(host_out.ctypes.data)) == INV
    assert lib.fr_ray_query_reserve_kind(ctx, n, 2, 0) == 0  # (room for the records, none for the masks)
    assert lib.fr_trace_rays_masked(ctx, p(fr.ctypes.data), p(hm.ctypes.data), n, HOST, 2, p(host_out.ctypes.data)) == INV
    assert lib.fr_ray_query_reserve_kind(ctx, n, 3, 0) == INV and lib.fr_ray_query_reserve_kind(ctx, n, 0, 2) == INV
    refused(INV, "a host batch above the area")
    # ... and everything accepted answers
    assert lib.fr_trace_rays_masked(ctx, p(rp), p(mp), n, DEV, 0, p(op)) == 0
    settle()
    got = arena.cpu().numpy()[out_words][:4 * n].view(rc.HIT_DTYPE).reshape(-1)
    assert rc.same_records(got, brute)
    assert lib.fr_trace_rays_masked(ctx, p(rp), p(mp), 0, DEV, 2, p(op)) == 0
    # the enqueued form on a sharded context; the synchronous form answers there
    t.destroy()
    W, H = 160, 96
    t = mk(fovrt_mod, 0, W=W, H=H)
    t.set_shard_plan(0, 2, 32, fovrt_mod.shard_plan(W, H, 32, 2))
    arena[out_words] = 7.0
    settle()
    assert lib.fr_trace_rays_masked_enqueue(t._ctx, p(rp), p(mp), n, 2, p(op), None) == UNS
    assert "sharded" in t.last_error()
    t.synchronize()
    assert (arena.cpu().numpy()[out_words] == 7.0).all()
    assert rc.same_records(query(t, r, "device", "closest", masks), brute)
    t.destroy()
