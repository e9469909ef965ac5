"""Deferred and retained frame state against an eager twin, across call sequences.

The frame path skips work behind host flags (an image owed and written on demand, retained state that still
describes a buffer; state_sequence_cases.py names them). Every case of MATRIX and every walk of WALKS makes the same
calls, prefix, disturber, observer, on

  default  a context created with no knob set, and
  plain    one created with FOVRT_JFA_LAZY_OUTPUTS=0, FOVRT_EXTRA_LAZY=0, FOVRT_JFA_REUSE=0 and FOVRT_EARLY_SETUP=0
           (every shortcut off; the knobs are read in fr_create),

and, for the walks, on a third context whose knob subset comes from the walk's seed. Then:

1. every buffer the observer read is bit-equal between the arms (NaNs in the same places), the bar each shortcut's own
   test holds it to; no tolerance;
2. the plain context is anchored to the oracle, so both cannot be wrong alike: after an observer that ran
   JumpFlooding, JFA_COORD and JFA_COLOR are oracle.jfa of the SHADING it read, bit for bit; after one that ran
   Sibson, SIBSON is held to oracle.sibson of the JFA outputs with the run form's bars (alpha equal, SIB_RUN_MAX,
   SIB_RUN_RMSE, imported from test_gpu_parity.py); after a restore followed by Sibson alone, SIBSON is also, bit for
   bit, the SIBSON read before the restore (a restore touches neither JFA output);
3. the ray-query disturber answers what the same batch answered before the prefix, and what follows it still holds.

A case the API refuses (FovrtError) must be refused at the same step with the same code on every arm and be listed
in state_sequence_cases.REFUSED. Counters and timings (jfa_reuse_count, stats) are not compared: they differ by
design.

Sizes 96x64 (whole 16x16 blocks) and 100x70 (ragged on both axes, a partial last word of the JFA seed bitmap): the
sizes at which the shortcuts' own tests exercise every kernel involved; the subject here is the host's flags. The
contexts of a size are made once per module; a case that took a view of EXTRA (which makes a context eager for good)
has them made anew."""
import zlib

import numpy as np
import pytest

import state_sequence_cases as sc
from helpers import ASSET_DIR, TEXTURE_MODE, rmse_per_channel
from test_gpu_parity import SIB_RUN_MAX, SIB_RUN_RMSE

pytestmark = pytest.mark.gpu

GROUPS = sc.matrix_groups()
REFUSALS_MET = {}  # case -> (step, code), as met on the device
CASES_RUN = [0]


def make_tracer(fovrt, W, H):
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=sc.SCENE, mask_mode=sc.MASK_MODE, spp=sc.SPP,
                                      diffuse_max_depth=sc.DIFFUSE_MAX_DEPTH, sibson_mode=sc.SIBSON_MODE,
                                      texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR))
    assert t.initialize()
    return t


class Pool:
    """The contexts of one size, by arm name, with the snapshot each gave right after fr_create."""
    ARMS = {"default": (), "plain": sc.KNOBS}

    def __init__(self, fovrt, W, H):
        self.fovrt, self.W, self.H = fovrt, W, H
        self.cameras, self.gazes = sc.camera_list(fovrt, W, H), sc.gaze_list(W, H)
        self.arms, self.base = {}, {}
        for name, knobs in self.ARMS.items():
            self.make(name, knobs)
        t = self.arms["default"]
        self.rest, self.models = t.scene_arrays()["pos"], t.models()

    def make(self, name, knobs_off):
        self.drop(name)
        with pytest.MonkeyPatch.context() as mp:
            for k in sc.KNOBS:
                mp.delenv(k, raising=False)
            for k in knobs_off:
                mp.setenv(k, "0")
            t = make_tracer(self.fovrt, self.W, self.H)
        self.arms[name], self.base[name] = t, t.snapshot()

    def drop(self, name):
        if name in self.arms:
            self.arms.pop(name).destroy()

    def renew_if_spoiled(self):
        if any(getattr(t, "_seq_spoiled", False) for t in self.arms.values()):
            for name, knobs in self.ARMS.items():
                self.make(name, knobs)

    def destroy(self):
        for name in list(self.arms):
            self.drop(name)


@pytest.fixture(scope="module")
def pools(fovrt_mod):
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = Pool(fovrt_mod, W, H)
        return made[(W, H)]

    yield get
    for p in made.values():
        p.destroy()


def run(pool, arm, seed, prefix, steps):
    """prefix, then steps, on one arm: the Env it leaves (env.refused: the step and code of a FovrtError)."""
    fovrt, t = pool.fovrt, pool.arms[arm]
    env = sc.Env(pool.cameras, pool.gazes, seed, pool.base[arm], pool.rest, pool.models)
    env.refused, at = None, "reset"
    try:
        hooks = [s.before_prefix for s in steps if s.before_prefix]
        if hooks:  # (from the state every prefix starts from, which it then makes again)
            sc.reset(fovrt, t, env)
            hooks[0](fovrt, t, env)
        at = prefix.name
        prefix.fn(fovrt, t, env)
        for i, s in enumerate(steps):
            at = f"{i}:{s.name}"
            s.fn(fovrt, t, env)
    except fovrt.FovrtError as e:
        if e.code == fovrt.FR_E_HIP:  # a device failure is never a refusal
            raise
        env.refused = (at, e.code)
    return env


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def report(a, b):
    bad = bits(a) != bits(b)
    i = tuple(np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} differ; first {i}: {a[i]} against {b[i]}"


def assert_same(what, got, want):
    """Two arms' observations: the same reads in the same order, bit for bit."""
    assert got.refused == want.refused, (what, "refused", got.refused, want.refused)
    assert [n for n, _ in got.obs] == [n for n, _ in want.obs], what
    for k, ((step, a), (_, b)) in enumerate(zip(got.obs, want.obs)):
        assert list(a) == list(b), (what, step)
        for name in a:
            assert np.array_equal(bits(a[name]), bits(b[name])), (what, f"observation {k}: {step}", name,
                                                                 report(a[name], b[name]))


def assert_anchored(oracle, what, env):
    """The plain arm against the oracle, for every observation of an observer that ran JumpFlooding or Sibson."""
    for k, (step, got) in enumerate(env.obs):
        o = sc.BY_NAME.get(step)
        if not isinstance(o, sc.Observer):
            continue
        where = (what, f"observation {k}: {step}")
        if o.ran_jfa:
            coord, color = oracle.jfa(got["SHADING"])
            assert np.array_equal(bits(got["JFA_COORD"]), bits(coord)), where + ("JFA_COORD", report(got["JFA_COORD"], coord))
            assert np.array_equal(bits(got["JFA_COLOR"]), bits(color)), where + ("JFA_COLOR", report(got["JFA_COLOR"], color))
        if o.ran_sibson:
            sf, ref = got["SIBSON"], oracle.sibson(got["JFA_COORD"], got["JFA_COLOR"])
            assert np.array_equal(sf[..., 3], ref[..., 3]), where + ("SIBSON alpha",)
            assert np.abs(sf - ref).max() <= SIB_RUN_MAX, where + (np.abs(sf - ref).max(),)
            assert (rmse_per_channel(sf, ref) <= SIB_RUN_RMSE).all(), where + (rmse_per_channel(sf, ref),)


def assert_rays_undisturbed(what, env):
    for step, got in env.obs:
        if step == "trace_rays" and env.ray_ref is not None and got["at_rest"][0]:
            ref = env.ray_ref.view(np.float32).reshape(-1, 4)
            assert np.array_equal(bits(got["hits"]), bits(ref)), (what, "the ray batch", report(got["hits"], ref))
            assert (env.ray_ref["prim"] >= 0).any() and (env.ray_ref["prim"] < 0).any(), "hits and misses"


def case_seed(*names):
    return zlib.crc32("/".join(names).encode())


@pytest.mark.parametrize("W,H", sc.SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("prefix,disturber", list(GROUPS), ids=lambda v: str(v))
def test_matrix(fovrt_mod, oracle, pools, prefix, disturber, W, H):
    pool = pools(W, H)
    P, D = sc.BY_NAME[prefix], sc.BY_NAME[disturber]
    for oname in GROUPS[(prefix, disturber)]:
        case = (prefix, disturber, oname)
        what = case + ((W, H),)
        envs = {arm: run(pool, arm, case_seed(*case), P, [D, sc.BY_NAME[oname]]) for arm in Pool.ARMS}
        pool.renew_if_spoiled()
        CASES_RUN[0] += 1
        plain = envs["plain"]
        assert_same(what, envs["default"], plain)
        if plain.refused:
            REFUSALS_MET[what] = plain.refused
            assert case in sc.REFUSED and sc.REFUSED[case] == plain.refused[1], (what, "refused", plain.refused)
            continue
        assert case not in sc.REFUSED, (what, "listed as refused, and was not")
        assert plain.obs and plain.obs[-1][0] == oname, what
        assert_anchored(oracle, what, plain)
        assert_rays_undisturbed(what, plain)
        if disturber in sc.RESTORES and oname == "sibson_alone":
            for arm, env in envs.items():
                assert np.array_equal(bits(env.obs[-1][1]["SIBSON"]), bits(env.sibson_before)), (
                    what, arm, "SIBSON after the restore against SIBSON before it",
                    report(env.obs[-1][1]["SIBSON"], env.sibson_before))


@pytest.mark.parametrize("W,H", sc.SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("seed", sc.WALK_SEEDS)
def test_walk(fovrt_mod, oracle, pools, seed, W, H):
    pool = pools(W, H)
    prefix, names, knobs = sc.walk(seed)
    steps = [sc.BY_NAME[n] for n in names]
    what = (f"walk {seed}", (W, H), f"third context without {'+'.join(knobs)}", prefix, names)
    pool.make("mixed", knobs)
    try:
        envs = {arm: run(pool, arm, seed, sc.BY_NAME[prefix], steps) for arm in ("default", "plain", "mixed")}
    finally:
        pool.drop("mixed")
        pool.renew_if_spoiled()
    plain = envs["plain"]
    assert plain.refused is None, (what, "refused", plain.refused)
    assert_same(what + ("default",), envs["default"], plain)
    assert_same(what + ("mixed",), envs["mixed"], plain)
    assert sum(isinstance(sc.BY_NAME[s], sc.Observer) for s, _ in plain.obs) == sum(
        isinstance(s, sc.Observer) for s in steps), what
    assert_anchored(oracle, what, plain)
    assert_rays_undisturbed(what, plain)


def test_refusals_met_are_the_listed_ones():
    """After the matrix (file order): what the device refused is what the cases module lists, and it is little."""
    print(f"state sequences: {CASES_RUN[0]} matrix cases run, {len(REFUSALS_MET)} refused: {sorted(REFUSALS_MET)}")
    assert {w[:3] for w in REFUSALS_MET} <= set(sc.REFUSED)
    assert len({w[:3] for w in REFUSALS_MET}) <= sc.MAX_REFUSED_FRACTION * len(sc.MATRIX)
