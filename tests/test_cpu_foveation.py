"""CPU suite for foveation control: the rank table, the host statement of the eccentricity mask
(fr_foveation_mask, the function k_ecc_mask runs) against the numpy restatement bit for bit, the mask's properties,
the closed loop of the ray budget's controller, fr_foveation_default and every refusal that needs no device."""
import ctypes as C

import numpy as np
import pytest

import foveation_np as fnp


def test_rank_table_is_the_ordered_dither_permutation():
    t = fnp.rank_table()
    assert sorted(t.reshape(-1).tolist()) == list(range(64))
    assert t[0, 0] == 0
    assert t[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42]
    assert t[1].tolist() == [48, 16, 56, 24, 50, 18, 58, 26]
    # periodic in 8, and the 8 x 8 grid of rank 0 is the reference's peripheral grid
    assert fnp.rank(8 + 3, 16 + 5) == t[5, 3]
    assert (fnp.mask(40, 24, (-1e4, -1e4), 0.0)[::8, ::8] == 1).all()


@pytest.mark.parametrize("W,H", fnp.SCREENS)
def test_host_mask_equals_numpy_bit_for_bit(fovrt_mod, W, H):
    for gaze in fnp.GAZES:
        g = gaze or fnp.centre(W, H)
        for r2 in fnp.r2_values(W, H):
            for fl in fnp.FLOORS:
                got, n = fovrt_mod.foveation_mask(W, H, g, r2, fl)
                ref = fnp.mask(W, H, g, r2, fl)
                assert got.shape == (H, W) and np.array_equal(got, ref), (W, H, g, float(r2), fl)
                assert n == int(ref.sum()) == fovrt_mod.foveation_mask(W, H, g, r2, fl, count_only=True)


@pytest.mark.parametrize("W,H", fnp.SCREENS)
def test_mask_grows_with_r2_and_fills_the_screen(W, H):
    for gaze in fnp.GAZES:
        g = gaze or fnp.centre(W, H)
        prev = None
        for r2 in [np.float32(0.0), np.float32(0.5)] + fnp.r2_values(W, H):
            m = fnp.mask(W, H, g, r2)
            if prev is not None:
                assert (m >= prev).all(), (W, H, g, float(r2))
            prev = m
        # inside the radius every pixel is sampled, whatever its rank
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        d2 = (x - g[0]) ** 2 + (y - g[1]) ** 2
        assert (fnp.mask(W, H, g, np.float32(106.25))[d2 < 106.0] == 1).all()
        # the floor alone: floor_ranks / 64 of every 8 x 8 cell
        far = fnp.mask(64, 64, (-1e4, -1e4), 0.0, 16)
        assert int(far.sum()) == 64 * 64 * 16 // 64
    on = fnp.centre(W, H)
    assert fnp.mask(W, H, on, fnp.r2_max(W, H)).all()
    assert fnp.mask(W, H, (3.5, min(66.25, H - 0.75)), fnp.r2_max(W, H)).all()
    assert fnp.mask(W, H, on, 0.0, 64).all()


@pytest.mark.parametrize("W,H,gaze,T,radius", fnp.LOOPS)
def test_closed_loop_reaches_the_deadband_and_holds(W, H, gaze, T, radius):
    steps = fnp.closed_loop(W, H, gaze, T, radius, 16)
    first = next(k for k, (_, n, _) in enumerate(steps) if fnp.in_band(n, T))
    assert first < 12, (first, [n for _, n, _ in steps])
    r2 = steps[first][0]
    for k in range(first + 1, len(steps)):  # held: r2 and the count stay
        assert steps[k][2] and steps[k][0] == r2 and steps[k][1] == steps[first][1], k
    # monotone from one side until then
    ns = [n for _, n, _ in steps[:first + 1]]
    assert ns == sorted(ns) or ns == sorted(ns, reverse=True), ns
    print(W, H, gaze, T, "deadband at launch", first, "count", steps[first][1])


def test_controller_clamps_and_guards():
    W, H = 100, 70
    assert fnp.control(4.0, 0, 1000, 0.02, W, H) == (np.float32(8.0), False)       # n = 0 counts as 1, ratio <= 2
    assert fnp.control(4.0, 100000, 10, 0.02, W, H) == (np.float32(2.0), False)    # ratio >= 0.5
    assert fnp.control(1.5, 100000, 10, 0.02, W, H) == (np.float32(1.0), False)    # r2 >= 1
    assert fnp.control(14000.0, 10, 7000, 0.0, W, H) == (fnp.r2_max(W, H), False)  # r2 <= W^2 + H^2
    assert fnp.control(9.0, 1020, 1000, 0.02, W, H) == (np.float32(9.0), True)     # |n - T| = tolerance * T: held
    assert not fnp.control(9.0, 1021, 1000, 0.02, W, H)[1]


def test_foveation_default(fovrt_mod):
    for W, H in fnp.SCREENS + [(3840, 2160)]:
        d = fovrt_mod.foveation_default(W, H)
        r = np.float32(0.07) * np.sqrt(fnp.r2_max(W, H), dtype=np.float32)
        assert np.float32(d["radius_px"]) == r and d["radius_px"] > 0
        assert d["floor_ranks"] == 1 and d["ray_budget"] == 0 and np.float32(d["tolerance"]) == np.float32(0.02)


def test_refusals_that_need_no_device(fovrt_mod):
    lib = fovrt_mod.load_library()
    INV = fovrt_mod.FR_E_INVALID
    f = fovrt_mod.fr_foveation()
    assert lib.fr_foveation_default(0, 10, C.byref(f)) == INV
    assert lib.fr_foveation_default(10, 40000, C.byref(f)) == INV
    assert lib.fr_foveation_default(10, 10, None) == INV
    g = (C.c_float * 2)(1.0, 1.0)
    n = C.c_uint32(77)
    bad = [(0, 4, g, 1.0, 1), (4, -1, g, 1.0, 1), (4, 4, None, 1.0, 1), (4, 4, g, -1.0, 1), (4, 4, g, float("nan"), 1),
           (4, 4, g, float("inf"), 1), (4, 4, g, 1.0, 0), (4, 4, g, 1.0, 65),
           (4, 4, (C.c_float * 2)(float("nan"), 0.0), 1.0, 1), (4, 4, (C.c_float * 2)(0.0, float("inf")), 1.0, 1)]
    for W, H, gz, r2, fl in bad:
        buf = np.full(16, 9, np.uint8)
        assert lib.fr_foveation_mask(W, H, gz, r2, fl, C.c_void_p(buf.ctypes.data), C.byref(n)) == INV, (W, H, r2, fl)
        assert (buf == 9).all() and n.value == 77
    # both outputs are optional
    assert lib.fr_foveation_mask(4, 4, g, 1.0, 1, None, None) == 0
    # every context call refuses a NULL context
    for name, args in [("fr_set_foveation", (C.byref(f),)), ("fr_get_foveation", (C.byref(f),)),
                       ("fr_foveation_status", (None, None, None, None)), ("fr_set_mask_mode", (5,)),
                       ("fr_get_mask_mode", (C.byref(C.c_int()),)), ("fr_sampling_mask_enable", (1,)),
                       ("fr_set_sampling_mask", (C.c_void_p(16), 1, 0)),
                       ("fr_set_sampling_mask_enqueue", (C.c_void_p(16), 1, None)),
                       ("fr_sampling_mask_consumed", (None,))]:
        assert getattr(lib, name)(None, *args) == INV, name
    assert fovrt_mod.MASK_ECCENTRIC == 5 and fovrt_mod.MASK_CALLER == 6
    assert fovrt_mod.STEERED_MASKS == {"eccentric": 5, "caller": 6} and not set(fovrt_mod.STEERED_MASKS) & set(fovrt_mod.MASKS)
