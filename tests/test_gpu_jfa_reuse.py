"""JumpFlooding skips its passes when the seed set {alpha >= 1} of its input equals the previous launch's
(k_jfa.hip): the retained final state is the one the passes would compute. Every case runs a default context
beside one created with FOVRT_JFA_REUSE=0, whose every launch runs its passes, and holds the two to each other
bit for bit; fr_jfa_reuse_count tells reuse from recomputation.

Sizes: 80x60 (max step 64, 7 passes: the last pass reads G), 130x70 (max step 128, 8 passes: it reads H) and
203x77 (15,631 pixels: the last bitmap word is partial)."""
import numpy as np
import pytest

from helpers import ASSET_DIR, TEXTURE_MODE, equal_nan, rmse_per_channel, sparse_image

pytestmark = pytest.mark.gpu

SIB_RUN_MAX, SIB_RUN_RMSE = 4e-3, 5e-5  # the run form's bars (README, tests/test_gpu_parity.py)
SIZES = [(80, 60), (130, 70), (203, 77)]
FW, FH = 96, 64  # the fr_frame cases: the bunny, signed log-polar mask, 1 spp

TN = None


@pytest.fixture(scope="module", autouse=True)
def _tn(fovrt_mod):
    global TN
    TN = fovrt_mod.TextureName


def make_tracer(fovrt, W, H, scene=0, mask=3, spp=1, dmd=1, **kw):
    t = fovrt.PathTracer(fovrt.Config(width=W, height=H, scene=scene, mask_mode=mask, spp=spp, diffuse_max_depth=dmd,
                                      texture_mode=TEXTURE_MODE, asset_dir=ASSET_DIR, **kw))
    assert t.initialize()
    return t


@pytest.fixture
def pair(fovrt_mod, monkeypatch):
    """make(W, H, **config) -> (default context, context whose every JumpFlooding runs its passes)."""
    made = []

    def make(W, H, **kw):
        reuse = make_tracer(fovrt_mod, W, H, **kw)
        monkeypatch.setenv("FOVRT_JFA_REUSE", "0")
        forced = make_tracer(fovrt_mod, W, H, **kw)
        monkeypatch.delenv("FOVRT_JFA_REUSE")
        made.extend([reuse, forced])
        return reuse, forced

    yield make
    for t in made:
        t.destroy()


def report(a, b):
    bad = ~np.isclose(a, b, rtol=0, atol=0, equal_nan=True)
    if not bad.any():
        return "equal"
    i = tuple(np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} differ; first {i}: {a[i]} against {b[i]}"


def seed_mask(W, H, seed, density=0.03):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


def stages(fovrt_mod, t, img):
    """write SHADING, JumpFlooding, Sibson; then the three outputs (JFA_COORD is written when it is read)."""
    t.write(TN.SHADING, img)
    fovrt_mod.JumpFlooding(t).render(TN.SHADING)
    fovrt_mod.SibsonInterpolation(t).render()
    return {tid: t.read(tid) for tid in (TN.JFA_COLOR, TN.JFA_COORD, TN.SIBSON)}


_oracle_refs = {}


def oracle_stages(oracle, key, img):
    """(coord, color, sibson) of the oracle for an input, computed once per module."""
    if key not in _oracle_refs:
        coord, color = oracle.jfa(img)
        _oracle_refs[key] = (coord, color, oracle.sibson(coord, color))
    return _oracle_refs[key]


def launch(fovrt_mod, oracle, reuse, forced, img, what, key=None):
    """One launch on both contexts: equal outputs, and (key given) the oracle's as the parity tests hold them:
    JumpFlooding bit for bit, the run form of Sibson inside its bars."""
    a, b = stages(fovrt_mod, reuse, img), stages(fovrt_mod, forced, img)
    for tid in a:
        assert equal_nan(a[tid], b[tid]), (what, tid, report(a[tid], b[tid]))
    if key is not None:
        coord, color, sib = oracle_stages(oracle, key, img)
        assert equal_nan(a[TN.JFA_COORD], coord), (what, report(a[TN.JFA_COORD], coord))
        assert equal_nan(a[TN.JFA_COLOR], color), (what, report(a[TN.JFA_COLOR], color))
        sf = a[TN.SIBSON]
        assert np.isfinite(sf).all() and np.array_equal(sf[..., 3], sib[..., 3]), what
        assert np.abs(sf - sib).max() <= SIB_RUN_MAX, (what, np.abs(sf - sib).max())
        assert (rmse_per_channel(sf, sib) <= SIB_RUN_RMSE).all(), (what, rmse_per_channel(sf, sib))
    return a


def counts(reuse, forced):
    assert forced.jfa_reuse_count() == 0
    return reuse.jfa_reuse_count()


# ---------------------------------------------------------------------------------------------
# Stage calls
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sibson_mode", [0, 1])
@pytest.mark.parametrize("W,H", SIZES)
def test_same_seeds_new_colours(fovrt_mod, oracle, pair, W, H, sibson_mode):
    """The second launch's passes are skipped; its colours are the second input's. (sibson_mode 1: k_jfa_final and
    the per-tap Sibson; the oracle comparison is the run form's.)"""
    reuse, forced = pair(W, H, sibson_mode=sibson_mode)
    m = seed_mask(W, H, W)
    one, two = sparse_image(W, H, m, seed=1), sparse_image(W, H, m, seed=2)
    key = (W, H, "colours") if sibson_mode == 0 else None
    launch(fovrt_mod, oracle, reuse, forced, one, "first")
    assert counts(reuse, forced) == 0
    out = launch(fovrt_mod, oracle, reuse, forced, two, "second", key)
    assert counts(reuse, forced) == 1
    assert not equal_nan(out[TN.JFA_COLOR], stages(fovrt_mod, forced, one)[TN.JFA_COLOR])  # (the colours did change)


@pytest.mark.parametrize("W,H", SIZES)
def test_same_seed_set_other_alphas(fovrt_mod, oracle, pair, W, H):
    """Alpha 1.0 against 3.0 on the seeds, 0.0 against 0.5 elsewhere: the same set, the passes are skipped."""
    reuse, forced = pair(W, H)
    m = seed_mask(W, H, W + 1)
    one = sparse_image(W, H, m, seed=3)
    two = sparse_image(W, H, m, seed=4)
    two[..., 3] = np.where(m != 0, np.float32(3.0), np.float32(0.5))
    launch(fovrt_mod, oracle, reuse, forced, one, "first")
    launch(fovrt_mod, oracle, reuse, forced, two, "second", (W, H, "alphas"))
    assert counts(reuse, forced) == 1


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("W,H", SIZES)
def test_one_pixel_toggled_across_one(fovrt_mod, oracle, pair, W, H, which):
    """Pixel 0, or the last pixel (203x77: in the partial word), seeded in B and not in A. A, B, A: no launch is
    skipped, and the third equals a fresh context's A."""
    reuse, forced = pair(W, H)
    m = seed_mask(W, H, W + 2)
    y, x = (0, 0) if which == "first" else (H - 1, W - 1)
    m[y, x] = 0
    A = sparse_image(W, H, m, seed=5)
    B = A.copy()
    B[y, x] = (0.25, 0.5, 0.75, 1.0)
    launch(fovrt_mod, oracle, reuse, forced, A, "A")
    launch(fovrt_mod, oracle, reuse, forced, B, "B", (W, H, "toggle-B", which))
    third = launch(fovrt_mod, oracle, reuse, forced, A, "A again", (W, H, "toggle-A", which))
    assert counts(reuse, forced) == 0
    fresh = make_tracer(fovrt_mod, W, H)
    want = stages(fovrt_mod, fresh, A)
    fresh.destroy()
    for tid in want:
        assert equal_nan(third[tid], want[tid]), (tid, report(third[tid], want[tid]))


@pytest.mark.parametrize("W,H", SIZES)
def test_no_seed_then_seeds_then_the_same_seeds(fovrt_mod, oracle, pair, W, H):
    reuse, forced = pair(W, H)
    none = sparse_image(W, H, np.zeros((H, W), np.uint8), seed=6)
    m = seed_mask(W, H, W + 3)
    launch(fovrt_mod, oracle, reuse, forced, none, "no seed", (W, H, "none"))
    assert counts(reuse, forced) == 0
    launch(fovrt_mod, oracle, reuse, forced, sparse_image(W, H, m, seed=7), "seeds")
    assert counts(reuse, forced) == 0
    launch(fovrt_mod, oracle, reuse, forced, sparse_image(W, H, m, seed=8), "the same seeds", (W, H, "appeared"))
    assert counts(reuse, forced) == 1
    # ... and an empty set again is a change, the one after it none
    launch(fovrt_mod, oracle, reuse, forced, none, "no seed again")
    assert counts(reuse, forced) == 1
    launch(fovrt_mod, oracle, reuse, forced, none, "no seed, repeated")
    assert counts(reuse, forced) == 2


@pytest.mark.parametrize("W,H", SIZES)
def test_nan_alpha_counts_as_unseeded(fovrt_mod, oracle, pair, W, H):
    """A former seed whose alpha becomes NaN leaves the set (k_jfa_init's alpha >= 1 is false for it): the launch
    is not skipped; a repeat of it is. (No oracle here: it takes a NaN alpha for a seed.)"""
    reuse, forced = pair(W, H)
    m = seed_mask(W, H, W + 4)
    ys, xs = np.nonzero(m)
    one = sparse_image(W, H, m, seed=9)
    two = one.copy()
    two[ys[0], xs[0], 3] = np.nan
    two[ys[-1], xs[-1], 3] = np.nan
    launch(fovrt_mod, oracle, reuse, forced, one, "seeds")
    out = launch(fovrt_mod, oracle, reuse, forced, two, "two of them NaN")
    assert counts(reuse, forced) == 0
    # neither is anybody's seed any more
    sx = np.floor(out[TN.JFA_COORD][..., 0] * W).astype(int)
    sy = np.floor(out[TN.JFA_COORD][..., 1] * H).astype(int)
    for k in (0, -1):
        assert not ((sx == xs[k]) & (sy == ys[k])).any()
    launch(fovrt_mod, oracle, reuse, forced, two, "the same again")
    assert counts(reuse, forced) == 1


@pytest.mark.parametrize("W,H", SIZES)
def test_jfa_coord_read_after_a_skipped_launch(fovrt_mod, oracle, pair, W, H):
    """fr_read_buffer(JFA_COORD) right after a JumpFlooding whose passes were skipped, with no Sibson between:
    k_jfa_coord reads the retained state."""
    reuse, forced = pair(W, H)
    m = seed_mask(W, H, W + 5)
    one, two = sparse_image(W, H, m, seed=10), sparse_image(W, H, m, seed=11)
    launch(fovrt_mod, oracle, reuse, forced, one, "first")
    got = []
    for t in (reuse, forced):
        t.write(TN.SHADING, two)
        fovrt_mod.JumpFlooding(t).render(TN.SHADING)
        got.append(t.read(TN.JFA_COORD))
    assert counts(reuse, forced) == 1
    assert equal_nan(got[0], got[1]), report(got[0], got[1])
    assert equal_nan(got[0], oracle.jfa(two)[0])


@pytest.mark.parametrize("W,H", SIZES)
def test_jfa_color_written_between_launches(fovrt_mod, oracle, pair, W, H):
    """fr_write_buffer(JFA_COLOR) after a launch: Sibson reads the written colours, and the next launch (skipped)
    gives the outputs of its own input again."""
    reuse, forced = pair(W, H)
    m = seed_mask(W, H, W + 6)
    one = sparse_image(W, H, m, seed=12)
    first = launch(fovrt_mod, oracle, reuse, forced, one, "first")
    other = np.random.default_rng(13).random((H, W, 4), dtype=np.float32)
    other[..., 3] = first[TN.JFA_COLOR][..., 3]
    sib = []
    for t in (reuse, forced):
        t.write(TN.JFA_COLOR, other)
        fovrt_mod.SibsonInterpolation(t).render()
        sib.append(t.read(TN.SIBSON))
    assert equal_nan(sib[0], sib[1]), report(sib[0], sib[1])
    assert not equal_nan(sib[0], first[TN.SIBSON])
    again = launch(fovrt_mod, oracle, reuse, forced, one, "after the write", (W, H, "written"))
    assert counts(reuse, forced) == 1
    for tid in again:
        assert equal_nan(again[tid], first[tid]), (tid, report(again[tid], first[tid]))


def test_two_contexts_share_nothing(fovrt_mod, oracle, pair):
    """Two default contexts of one size in one process, launched in turns on different seed sets: each skips on
    its own bitmap, word and generation."""
    W, H = 130, 70
    a, forced = pair(W, H)
    b = make_tracer(fovrt_mod, W, H)
    ma, mb = seed_mask(W, H, 21), seed_mask(W, H, 22)
    ia, ib = sparse_image(W, H, ma, seed=14), sparse_image(W, H, mb, seed=15)
    stages(fovrt_mod, a, ia)
    stages(fovrt_mod, b, ia)  # b's first launch, on a's set: its own first, not skipped
    assert (a.jfa_reuse_count(), b.jfa_reuse_count()) == (0, 0)
    stages(fovrt_mod, b, ib)  # b moves on
    outa = stages(fovrt_mod, a, ia)  # a's set is still a's
    assert (a.jfa_reuse_count(), b.jfa_reuse_count()) == (1, 0)
    outb = stages(fovrt_mod, b, ib)
    assert (a.jfa_reuse_count(), b.jfa_reuse_count()) == (1, 1)
    wa, wb = stages(fovrt_mod, forced, ia), stages(fovrt_mod, forced, ib)
    for tid in wa:
        assert equal_nan(outa[tid], wa[tid]) and equal_nan(outb[tid], wb[tid]), tid
    assert forced.jfa_reuse_count() == 0
    b.destroy()


# ---------------------------------------------------------------------------------------------
# fr_frame: the bunny at 96x64, signed log-polar mask, 1 spp
# ---------------------------------------------------------------------------------------------
FRAME_OUTS = ("SHADING", "SIBSON", "PULLPUSH", "ATROUS")


def frame_pair(pair, fovrt_mod, latency=False):
    reuse, forced = pair(FW, FH, scene=fovrt_mod.SCENE_BUNNY, mask=fovrt_mod.MASK_LOGPOLAR_SIGNED)
    if latency:
        for t in (reuse, forced):
            t.set_pipeline_mode(fovrt_mod.PIPELINE_LATENCY)
    return reuse, forced


def frame_both(reuse, forced, what, before=None):
    """One fr_frame on both contexts (before(t) first): equal outputs; the frame's seed set, as the device's
    SHADING has it."""
    for t in (reuse, forced):
        if before:
            before(t)
        t.frame(timing=False)
    for name in FRAME_OUTS:
        a, b = reuse.read(getattr(TN, name)), forced.read(getattr(TN, name))
        assert equal_nan(a, b), (what, name, report(a, b))
    return reuse.read(TN.SHADING)[..., 3] >= 1.0


def run_frames(reuse, forced, n, before=None):
    """n frames; per frame its seed set and whether its JumpFlooding skipped its passes."""
    seeds, skipped = [], []
    for f in range(n):
        c0 = reuse.jfa_reuse_count()
        seeds.append(frame_both(reuse, forced, f, (lambda t, f=f: before(t, f)) if before else None))
        skipped.append(reuse.jfa_reuse_count() - c0)
    assert forced.jfa_reuse_count() == 0
    return seeds, skipped


def same_as_before(seeds):
    return [0] + [int(np.array_equal(seeds[f], seeds[f - 1])) for f in range(1, len(seeds))]


@pytest.fixture(scope="module")
def oracle_still_seed_sets(fovrt_mod, oracle):
    """The seed sets (SHADING.w >= 1) of six still frames on the CPU oracle, at the frame cases' configuration."""
    t = make_tracer(fovrt_mod, FW, FH, scene=fovrt_mod.SCENE_BUNNY, mask=fovrt_mod.MASK_LOGPOLAR_SIGNED)
    arrays = t.scene_arrays()
    t.destroy()
    uni = fovrt_mod.Camera.preset(fovrt_mod.SCENE_BUNNY, FW, FH).uniforms(FW, FH)
    osc = oracle.OracleScene(arrays, diffuse_max_depth=1)
    hist = np.zeros((FH, FW, 4), np.float32)
    depth_cache = np.zeros((FH, FW, 4), np.float32)
    sets = []
    for frame in range(6):
        g = oracle.gbuffer(osc, uni, FW, FH, frame)
        s = oracle.sampling(osc, uni, FW, FH, fovrt_mod.MASK_LOGPOLAR_SIGNED, g["position"], g["depth"], depth_cache,
                            g["weight"], g["normal"], g["diffuse"])
        sh = oracle.shading(osc, uni, FW, FH, frame, 1, s["mask"], s["weight"], hist)
        sets.append(sh["shading"][..., 3] >= 1.0)
        hist, depth_cache = sh["history"], g["depth"]
    return sets


@pytest.mark.parametrize("latency", [False, True])
def test_still_frames(fovrt_mod, pair, oracle_still_seed_sets, latency):
    """Six still frames, pipelined and in latency mode. On the oracle the seed set is steady from the second frame
    on, so at least the last four frames skip their passes; on the device every frame whose set is the previous
    frame's skips them, and no other."""
    steady = same_as_before(oracle_still_seed_sets)
    assert oracle_still_seed_sets[1].any() and steady[2:] == [1, 1, 1, 1], steady
    reuse, forced = frame_pair(pair, fovrt_mod, latency)
    seeds, skipped = run_frames(reuse, forced, 6)
    print("still frames: seeds", [int(s.sum()) for s in seeds], "skipped", skipped, "oracle steady", steady)
    assert skipped == same_as_before(seeds)
    assert sum(skipped) >= 4
    assert reuse.jfa_reuse_count() == sum(skipped)


def test_gaze_moved_once(fovrt_mod, pair):
    """Frames 0-2 at the centre, 3-7 at another gaze: the frame after the move runs its passes, the later ones
    skip them again."""
    reuse, forced = frame_pair(pair, fovrt_mod)

    def before(t, f):
        if f == 3:
            t.set_gaze(FW / 2 + 17, (FH / 2 - 9) / 1.25)

    seeds, skipped = run_frames(reuse, forced, 8, before)
    print("gaze moved at 3: seeds", [int(s.sum()) for s in seeds], "skipped", skipped)
    assert skipped == same_as_before(seeds)
    assert not np.array_equal(seeds[3], seeds[2]) and skipped[3] == 0
    assert skipped[2] == 1 and skipped[5:] == [1, 1, 1]


def test_panning_frames(fovrt_mod, pair):
    reuse, forced = frame_pair(pair, fovrt_mod)
    cam = fovrt_mod.Camera.preset(fovrt_mod.SCENE_BUNNY, FW, FH)

    def before(t, f):
        if t is reuse:
            cam.setPrevState()
            cam.lookAt(np.asarray(cam.target) + np.array([0.01, 0.005, 0.0], np.float32))
        t.update_optix_variables(cam)

    seeds, skipped = run_frames(reuse, forced, 3, before)
    print("panning: seeds", [int(s.sum()) for s in seeds], "skipped", skipped)
    assert skipped == same_as_before(seeds)


def test_snapshot_restore(fovrt_mod, pair):
    """Still frames, so the frame after the restore has the seed set of the frame before it: it runs its passes all
    the same (a snapshot carries no JFA state), and replays the frame that followed the snapshot bit for bit."""
    reuse, forced = frame_pair(pair, fovrt_mod)
    run_frames(reuse, forced, 3)
    snaps = [t.snapshot() for t in (reuse, forced)]
    seeds, skipped = run_frames(reuse, forced, 3)
    assert skipped == [1, 1, 1], skipped
    outs = FRAME_OUTS + ("JFA_COLOR", "HISTORY_CACHE")
    for t, snap in zip((reuse, forced), snaps):
        t.restore(snap)
    c0 = reuse.jfa_reuse_count()
    replay = frame_both(reuse, forced, "replay")
    assert np.array_equal(replay, seeds[0])
    assert reuse.jfa_reuse_count() == c0  # not skipped
    fresh = make_tracer(fovrt_mod, FW, FH, scene=fovrt_mod.SCENE_BUNNY, mask=fovrt_mod.MASK_LOGPOLAR_SIGNED)
    fresh.restore(snaps[0])
    fresh.frame(timing=False)
    for name in outs:
        a, b = reuse.read(getattr(TN, name)), fresh.read(getattr(TN, name))
        assert equal_nan(a, b), (name, report(a, b))
    assert fresh.jfa_reuse_count() == 0
    fresh.destroy()
    frame_both(reuse, forced, "after the replay")
    assert reuse.jfa_reuse_count() == c0 + 1
