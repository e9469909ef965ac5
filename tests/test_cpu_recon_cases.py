"""The reconstruction references agree with each other on the inputs the device is then held to
(tests/test_gpu_recon_edges.py): A-Trous on a G-buffer-shaped input at deep passes and with non-finite
texels, pull-push below one tile, taller than wide, and at the smallest atlases."""
import numpy as np
import pytest

import recon_cases as rc
from helpers import PullPushNp, atrous_np, equal_nan


@pytest.fixture(scope="module")
def gbuffers():
    return {s: rc.gbuffer_case(*s, seed=s[0] + s[1]) for s in rc.ATROUS_CPU_SHAPES}


def test_gbuffer_case_spans_the_weight_range():
    """Weights of exactly 1 (identical miss texels) and exactly 0 (box against ground, > 13 units), a
    crease, and positions of scene magnitude."""
    pos, nrm, col = rc.gbuffer_case(83, 45, 1)
    miss = (pos == 0).all(-1) & (nrm == 0).all(-1)
    assert miss.any() and (col[miss] == rc.SKY).all()
    assert np.abs(pos[..., :3]).max() > 30
    d = np.sum((pos[:, 1:].astype(np.float64) - pos[:, :-1]) ** 2, -1)
    assert (d > 169).any()  # a depth edge between horizontal neighbours: e^-169 = 0 in f32
    assert np.exp(np.float32(-169.0)) == 0
    n = np.sum((nrm[:, 1:] - nrm[:, :-1]) ** 2, -1)
    assert np.isclose(n, 1.44).any()  # the crease
    assert (col[..., 3] == 1).all()


@pytest.mark.parametrize("count", rc.ATROUS_CPU_COUNTS)
@pytest.mark.parametrize("W,H", rc.ATROUS_CPU_SHAPES)
def test_atrous_oracle_equals_numpy_on_gbuffer(oracle, gbuffers, W, H, count):
    pos, nrm, col = gbuffers[(W, H)]
    a, b = oracle.atrous(count, pos, nrm, col), atrous_np(count, pos, nrm, col)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    err = np.abs(a - b).max()
    print(f"{W}x{H} count {count}: oracle - numpy max {err:.3g}")
    assert err <= rc.ATROUS_BAR_NP


@pytest.mark.parametrize("count", rc.ATROUS_NONFINITE_COUNTS)
@pytest.mark.parametrize("W,H", rc.ATROUS_NONFINITE_SHAPES)
def test_atrous_nonfinite_texels_oracle_rule(oracle, W, H, count):
    """What atFS does with non-finite texels, as the oracle (C fminf / fmaxf) pins it, and where the numpy
    restatement differs.

    A weight term is min(exp(-d2 / phi), 1). The oracle's fminf returns the other operand for a NaN, so
    a NaN squared distance (a NaN texel, or Inf - Inf) gives that term the weight 1; numpy's np.minimum
    propagates the NaN, so the whole tap, and the output texel, become NaN. GLSL leaves min() with a
    NaN operand undefined, so neither is "the" reference; the device follows the oracle
    (observable differences). Consequences pinned here, on the first pass:
      - NaN position or NaN normal: the texel filters as if that term matched everywhere; it and its
        neighbours stay finite;
      - Inf position: weight 0 to and from every neighbour, the texel keeps its own colour;
      - Inf colour: the texel stays +Inf in the planted channels, every texel within two taps becomes
        NaN there (Inf * 0);
      - a NaN colour channel: NaN in that channel for every texel within two taps, the other channels
        finite.
    atrous_np may only make more texels NaN, never fewer, and agrees wherever it is not NaN."""
    pos, nrm, col, planted = rc.nonfinite_case(W, H, seed=5)
    ref = oracle.atrous(count, pos, nrm, col)
    with np.errstate(invalid="ignore"):
        mine = atrous_np(count, pos, nrm, col)
    nan_o, nan_n = np.isnan(ref), np.isnan(mine)
    print(f"{W}x{H} count {count}: oracle {int(nan_o.any(-1).sum())} NaN texels, numpy {int(nan_n.any(-1).sum())}; "
          f"oracle Inf texels {int(np.isinf(ref).any(-1).sum())}")
    assert (nan_n | ~nan_o).all(), "numpy has fewer NaNs than the oracle"
    assert nan_n.sum() > nan_o.sum()
    ok = ~nan_n
    assert np.array_equal(np.isinf(ref) & ok, np.isinf(mine) & ok)
    fin = ok & np.isfinite(ref)
    assert fin.any() or (W, H, count) == (40, 24, 4)  # (there the NaNs cover the whole image)
    if fin.any():
        assert np.abs(ref[fin] - mine[fin]).max() <= rc.ATROUS_BAR_NP
    if count == 1:
        reach = lambda k: (np.abs(np.mgrid[0:H, 0:W][1] - planted[k][0]) <= 2) & \
                          (np.abs(np.mgrid[0:H, 0:W][0] - planted[k][1]) <= 2)
        x, y = planted["inf_col"]
        want_inf = np.zeros((H, W, 4), bool)
        want_inf[y, x, :3] = True
        assert np.array_equal(np.isposinf(ref), want_inf) and not np.isneginf(ref).any()
        want_nan = np.zeros((H, W, 4), bool)
        want_nan[..., :3] |= reach("inf_col")[..., None]
        want_nan[y, x, :3] = False
        want_nan[..., 1] |= reach("nan_col_channel")
        assert np.array_equal(nan_o, want_nan)
        x, y = planted["inf_pos"]
        assert np.allclose(ref[y, x], col[y, x], rtol=3e-7, atol=0)  # (c * 9/64) / (9/64): two roundings
    else:
        # later passes: the sets only grow, along the taps (2 * (2^count - 1) texels in all)
        r = 2 * ((1 << count) - 1)
        near = np.zeros((H, W), bool)
        for k in ("inf_col", "nan_col_channel"):
            px, py = planted[k]
            near[max(0, py - r):py + r + 1, max(0, px - r):px + r + 1] = True
        assert not (~np.isfinite(ref)).any(-1)[~near].any()
        assert np.isfinite(ref[..., 3]).all()  # alpha is never planted


@pytest.fixture(scope="module")
def pp_oracle_runs(oracle):
    out = {}
    for W, H in rc.PULLPUSH_SHAPES:
        st = oracle.PullPushState(W, H)
        out[(W, H)] = [st.render(img) for img in rc.pullpush_frames(W, H)]
    return out


@pytest.mark.parametrize("W,H", rc.PULLPUSH_SHAPES)
def test_pullpush_oracle_equals_numpy_tiny_and_tall(pp_oracle_runs, W, H):
    mine = PullPushNp(W, H)
    for k, img in enumerate(rc.pullpush_frames(W, H)):
        assert equal_nan(pp_oracle_runs[(W, H)][k], mine.render(img)), k


@pytest.mark.parametrize("W,H", [(2, 2), (2, 1), (1, 2)])
def test_pullpush_s2_follows_the_host_loop(pp_oracle_runs, W, H):
    """S = 2 (e = 1) is degenerate in the reference's own host loop, and both restatements keep that.

    PullPushInterpolation::render's push loop starts at writeOffset (S, 1) and moves it to (0, 0) at
    the END of an iteration, after step--, when the next dispatch is the last (step == 0). With e = 1
    the first and only iteration already has step = 0, so the full-resolution level is written at
    (S, 1) - mostly outside the 3 x 2 atlas - and the region [0, S)^2 that pullpushFinal copies out is
    never written: the output is all zeros, for a fully covered input too. The oracle followed the
    loop; PullPushNp tested step == 0 at the start of the iteration, passed the input through, and was
    fixed. (1x1, e = 0, is degenerate the same way: no push dispatch touches texel (0, 0).)"""
    for k, out in enumerate(pp_oracle_runs[(W, H)]):
        assert not out.any(), k
    mine = PullPushNp(W, H)
    full = rc.pullpush_frames(W, H)[4]
    assert (full[..., 3] == 1).all()
    assert not mine.render(full).any()
