"""The ray-query cases (tests/ray_cases.py) are what they claim, on the references alone, before the GPU suite trusts
them: the oracle's tree path, its brute-force path and the numpy restatement agree bit for bit on every set; the
random set mixes hits and misses; the tie set resolves to the lower triangle of each coincident pair; the window
copies lose and keep the hit they are made from; every degenerate ray is a miss; the transmittance set holds all
three kinds of answer. And the host-side pieces of the ABI: the record sizes, the symbols, the refusals that need no
context."""
import ctypes as C

import numpy as np
import pytest

import ray_cases as rc
import trace_np as tn

_REFS = {}


def refs(fovrt, oracle, scene):
    """(arrays, OracleScene, SceneNp, {set: (rows, brute-force records)}) of a scene, computed once."""
    if scene not in _REFS:
        a = rc.scene_arrays(fovrt, scene)
        osc = oracle.OracleScene(a)
        sets = {k: (r, rc.hit_records(osc.closest(r, brute=True))) for k, r in rc.closest_sets(fovrt, scene).items()}
        _REFS[scene] = (a, osc, tn.SceneNp(a), sets)
    return _REFS[scene]


@pytest.mark.parametrize("scene", [0, 1])
def test_references_agree_on_every_set(fovrt_mod, oracle, scene):
    a, osc, nsc, sets = refs(fovrt_mod, oracle, scene)
    assert len(a["flags"]) == (14, 9106)[scene]
    for name, (r, brute) in sets.items():
        assert rc.same_records(rc.hit_records(osc.closest(r)), brute), name
        assert rc.same_records(rc.closest_np(nsc, r), brute), name
        if name.startswith("view_"):
            assert len(r) == rc.SIZE[0] * rc.SIZE[1]


@pytest.mark.parametrize("scene", [0, 1])
def test_random_set_lies_in_the_domain_and_mixes_hits_and_misses(fovrt_mod, oracle, scene):
    a, _osc, _nsc, sets = refs(fovrt_mod, oracle, scene)
    r, brute = sets["random"]
    lo, hi, _L = rc.domain(a["bbox"])
    assert ((r[:, 0:3] >= lo) & (r[:, 0:3] <= hi)).all()
    ln = np.linalg.norm(r[:, 3:6].astype(np.float64), axis=1)
    assert (ln >= 1e-3).all() and (ln <= 1e3).all()
    assert ln.min() < 1e-2 and ln.max() > 1e2
    share = float((brute["prim"] >= 0).mean())
    print("random set, scene", scene, "hit share", share)
    assert 0.3 <= share <= 0.7


@pytest.mark.parametrize("scene", [0, 1])
def test_zero_set_has_one_and_two_zero_components_of_both_signs(fovrt_mod, oracle, scene):
    a, _osc, _nsc, sets = refs(fovrt_mod, oracle, scene)
    r, brute = sets["zeros"]
    d = r[:, 3:6]
    z = d == 0
    assert (z.sum(1) == 1).sum() >= 40 and (z.sum(1) == 2).sum() >= 40
    assert (z & np.signbit(d)).any() and (z & ~np.signbit(d)).any()
    assert (brute["prim"] >= 0).mean() > 0.5
    lo, hi, _L = rc.domain(a["bbox"])
    assert ((r[:, 0:3] >= lo) & (r[:, 0:3] <= hi)).all()


def test_edge_set_hits_shared_edges_and_vertices(fovrt_mod, oracle):
    """At a shared edge or vertex several triangles answer with the same t, or nearly: the set is only worth its
    name if a good share of its rays has a second triangle within 1e-5 of the closest t."""
    _a, _osc, nsc, sets = refs(fovrt_mod, oracle, 0)
    r, brute = sets["edges"]
    close = 0
    for q, h in zip(r, brute):
        hit, t, _b, _g = nsc._tests(q[0:3], q[3:6], q[6], q[7])
        if h["prim"] >= 0:
            close += int((hit & (np.abs(t - h["t"]) <= 1e-5 * max(1.0, abs(h["t"])))).sum() >= 2)
    print("edge set: rays with two triangles at the closest t:", close, "of", len(r))
    assert close >= 20


def test_tie_set_returns_the_lower_triangle_of_each_pair(fovrt_mod, oracle):
    a = rc.scene_arrays(fovrt_mod, 0)
    ta = rc.tie_arrays(a)
    P = ta["pos"].reshape(-1, 3, 3)
    for dst, src in rc.TIE_PAIRS:
        assert dst > src and np.array_equal(P[dst], P[src])
    osc, nsc = oracle.OracleScene(ta), tn.SceneNp(ta)
    r = rc.tie_rows(a)
    brute = rc.hit_records(osc.closest(r, brute=True))
    assert rc.same_records(rc.hit_records(osc.closest(r)), brute)
    assert rc.same_records(rc.closest_np(nsc, r), brute)
    lower = np.isin(brute["prim"], [s for _d, s in rc.TIE_PAIRS])
    assert lower.sum() >= 50, lower.sum()
    assert not np.isin(brute["prim"], [d for d, _s in rc.TIE_PAIRS]).any()
    twin = dict((s, d) for d, s in rc.TIE_PAIRS)
    for q, h in zip(r[lower], brute[lower]):  # the twin answers with the same bits
        hit, t, b, g = nsc._tests(q[0:3], q[3:6], q[6], q[7])
        k = twin[int(h["prim"])]
        assert hit[k] and (t[k], b[k], g[k]) == (h["t"], h["beta"], h["gamma"])


@pytest.mark.parametrize("scene", [0, 1])
def test_window_copies_lose_and_keep_their_hit(fovrt_mod, oracle, scene):
    _a, osc, nsc, sets = refs(fovrt_mod, oracle, scene)
    for name, (r, brute) in sets.items():
        w, kind, base = rc.window_rows(r, brute)
        if not len(w):
            continue
        got = rc.hit_records(osc.closest(w, brute=True))
        assert rc.same_records(rc.hit_records(osc.closest(w)), got), name
        same = (got["prim"] == base["prim"]) & (got["t"] == base["t"])
        assert not same[kind == 0].any(), name      # tmax = t: the end is strict
        assert not same[kind == 1].any(), name      # tmin = t: likewise
        assert rc.same_records(got[kind == 2], base[kind == 2]), name  # tmax = nextafter(t): kept
        assert (got["t"][kind == 1] > base["t"][kind == 1]).all()
        sub = slice(0, None, max(1, len(w) // 120))  # the restatement on a sample (it costs a millisecond per ray)
        assert rc.same_records(rc.closest_np(nsc, w[sub]), got[sub]), name


@pytest.mark.parametrize("scene", [0, 1])
def test_degenerate_rays_miss_on_both_oracle_paths(fovrt_mod, oracle, scene):
    a, osc, _nsc, _sets = refs(fovrt_mod, oracle, scene)
    d, good = rc.degenerate_rows(a)
    assert len(d) == 8 + 12 + 4 + 5
    assert rc.hit_records(osc.closest(good[None], brute=True))["prim"][0] >= 0  # the ray they are made from hits
    for brute in (True, False):
        got = rc.hit_records(osc.closest(d, brute=brute))
        assert (got == rc.MISS).all(), (brute, np.nonzero(got != rc.MISS)[0])


@pytest.mark.parametrize("scene", [0, 1])
def test_transmittance_set_holds_all_three_answers(fovrt_mod, oracle, scene):
    a, _osc, nsc, _sets = refs(fovrt_mod, oracle, scene)
    s = rc.shadow_rows(a)
    assert len(s) == 300
    v = rc.shadow_np(nsc, s)
    counts = (int((v == 0).sum()), int((v == 1).sum()), int(((v > 0) & (v < 1)).sum()))
    print("transmittance set, scene", scene, "(zero, one, between):", counts)
    assert min(counts) >= 20 and sum(counts) == len(s)


def test_far_set_is_outside_the_domain(fovrt_mod):
    a = rc.scene_arrays(fovrt_mod, 1)
    lo, hi, _L = rc.domain(a["bbox"])
    r = rc.far_rows(a)
    assert (((r[:, 0:3] < lo) | (r[:, 0:3] > hi)).any(1)).all()
    assert np.allclose(np.linalg.norm(r[:, 0:3], axis=1), 1e4, rtol=1e-2)


def test_batch_sizes_straddle_a_chunk():
    assert rc.BATCH_SIZES == [1, 63, 64, 65, 64 * 7 + 5]


# ---------------------------------------------------------------------------------------------
# The host side of the ABI
# ---------------------------------------------------------------------------------------------
def test_record_sizes(fovrt_mod):
    assert C.sizeof(fovrt_mod.fr_ray) == 32 and C.sizeof(fovrt_mod.fr_ray_hit) == 16
    assert fovrt_mod.RAY_DTYPE.itemsize == 32 and fovrt_mod.RAY_HIT_DTYPE.itemsize == 16
    assert fovrt_mod.fr_ray.tmin.offset == 12 and fovrt_mod.fr_ray.dir.offset == 16 and fovrt_mod.fr_ray.tmax.offset == 28
    assert fovrt_mod.fr_ray_hit.prim.offset == 12
    assert rc.HIT_DTYPE == fovrt_mod.RAY_HIT_DTYPE
    r = rc.rows([[1, 2, 3]], [[4, 5, 6]], 7, 8)
    q = rc.fr_rays(r).view(fovrt_mod.RAY_DTYPE)[0, 0]
    assert (q["origin"].tolist(), float(q["tmin"]), q["dir"].tolist(), float(q["tmax"])) == ([1, 2, 3], 7, [4, 5, 6], 8)
    assert (fovrt_mod.FR_RAYS_CLOSEST, fovrt_mod.FR_RAYS_TRANSMITTANCE) == (0, 1)


def test_symbols_exist(fovrt_mod):
    lib = fovrt_mod.load_library()
    for s in ("fr_ray_query_reserve", "fr_trace_rays", "fr_trace_rays_enqueue", "fr_rays_consumed"):
        assert hasattr(lib, s) and s in fovrt_mod._SIGS, s
    for m in ("ray_query_reserve", "trace_rays", "trace_rays_enqueue", "rays_consumed", "model_of"):
        assert callable(getattr(fovrt_mod.PathTracer, m)), m


def test_null_context_is_refused(fovrt_mod):
    """The only refusal that needs no context: every other one is reported through the context's error text."""
    lib = fovrt_mod.load_library()
    rays = rc.fr_rays(rc.rows([[0, 1, 0]], [[0, -1, 0]]))
    out = np.full(4, 7.0, np.float32)
    E = fovrt_mod.FR_E_INVALID
    assert lib.fr_ray_query_reserve(None, 16) == E
    assert lib.fr_trace_rays(None, C.c_void_p(rays.ctypes.data), 1, 0, 0, C.c_void_p(out.ctypes.data)) == E
    assert lib.fr_trace_rays_enqueue(None, C.c_void_p(rays.ctypes.data), 1, 0, C.c_void_p(out.ctypes.data), None) == E
    assert lib.fr_rays_consumed(None, None) == E
    assert (out == 7.0).all()
