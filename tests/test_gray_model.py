"""tests/gray_model.py, the definition of psm_gray_compute, checked on the CPU: against a float64 evaluation of the same formulas
(transcription errors), for what the aggregation buys on Cones / Teddy (quality), and for its selection (oracle.wta)."""
import numpy as np
import pytest

import gray_model as M

# (W, H, D): the shapes tests/test_gpu_gray.py holds the device to
SHAPES = [(8, 8, 2), (9, 40, 2), (33, 21, 33), (67, 45, 16), (131, 70, 33), (150, 37, 130)]


def noise_pair(W, H, seed=None):
    rng = np.random.default_rng(1000 * W + H if seed is None else seed)
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


def green(golden, name):
    z = golden(name + "_pair.npz")
    return np.ascontiguousarray(z["l_bgr"][:, :, 1]), np.ascontiguousarray(z["r_bgr"][:, :, 1]), z


def max_dq(slice32, l, r, D):
    """max |q32 - q64| over both sides and every slice; slice32(side_object, d) is the fp32 evaluation under test."""
    worst = 0.0
    for side in (0, 1):
        s32, s64 = M.Side(l, r, side, M.F32), M.Side(l, r, side, M.F64)
        for d in range(D):
            worst = max(worst, float(np.max(np.abs(slice32(s32, d).astype(np.float64) - s64.slice(d)))))
    return worst


# Measured here (fp32 model against the float64 evaluation, 8-bit noise): 4.6e-8, 5.4e-8, 1.5e-7, 1.4e-7, 1.4e-7, 1.4e-7 for the six
# shapes in order; the bound is four times the largest.
SMALL_MEASURED = 1.46e-7
SMALL_BOUND = 4 * SMALL_MEASURED
# Cones green planes at D = 64, both sides: 2.39e-5 (flat regions: inv up to 1e4 amplifies the rounding of cov)
CONES_MEASURED = 2.39e-5
CONES_BOUND = 4 * CONES_MEASURED


@pytest.mark.parametrize("W,H,D", SHAPES)
def test_transcription_small(oracle, W, H, D):
    l, r = noise_pair(W, H)
    got = max_dq(lambda s, d: s.slice(d), l, r, D)
    print(f"{W}x{H}x{D}: max|dq| = {got:.3e} (bound {SMALL_BOUND:.3e})")
    assert got <= SMALL_BOUND


def test_transcription_cones(oracle, golden):
    l, r, _ = green(golden, "cones")
    got = max_dq(lambda s, d: s.slice(d), l, r, 64)
    print(f"cones: max|dq| = {got:.3e} (bound {CONES_BOUND:.3e})")
    assert got <= CONES_BOUND


def test_bound_catches_a_wrong_tap_border_or_operand(oracle):
    """The bound means something: the same comparison of a model with one deliberate slip - a gradient tap, the border predicate,
    an operand of b - lies far outside it."""
    W, H, D = 67, 45, 16
    l, r = noise_pair(W, H)

    def wrong_tap(s, d):        # G = I(x+1) - I(x) instead of I(x+1) - I(x-1)
        t = M.Side(l, r, int(s.right))
        x = np.arange(W)
        t.G = t.I[:, M.r101(x + 1, W)] - t.I
        return t.slice(d)

    def wrong_border(s, d):     # the border one column too wide: x <= d / x >= W - d - 1
        c = s.cost(d)
        bc = M.border_cost(s.I, s.G)
        col = W - d - 1 if s.right else d
        if 0 <= col < W:
            c[:, col] = bc[:, col]
        return M.filter_slice(s.I, s.mI, s.inv, c)[0]

    def wrong_operand(s, d):    # b = mp - a mp instead of mp - a mI
        p = s.cost(d)
        mp = M.F32.box(p)
        a = s.inv * (M.F32.box(s.I * p) - s.mI * mp)
        return M.F32.box(mp - a * mp) + M.F32.box(a) * s.I

    for slip in (wrong_tap, wrong_border, wrong_operand):
        got = max_dq(slip, l, r, D)
        print(f"{slip.__name__}: max|dq| = {got:.3e}")
        assert got > 100 * SMALL_BOUND, slip.__name__


# left-map bad pixels under oracle.eval_bad_pixels(map, gt_l, occl, 64, 4) of the committed model
PINNED = {"cones": 27009, "teddy": 34156}


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_quality(oracle, golden, name):
    l, r, z = green(golden, name)
    lmap, _ = M.maps(l, r, 64)
    raw, _ = M.maps_unaggregated(l, r, 64)
    bad, _ = oracle.eval_bad_pixels(lmap, z["gt_l"], z["occl"], 64, 4)
    bad_raw, _ = oracle.eval_bad_pixels(raw, z["gt_l"], z["occl"], 64, 4)
    print(f"{name}: {bad} bad pixels ({100.0 * bad / lmap.size:.2f} %), unaggregated {bad_raw} ({100.0 * bad_raw / lmap.size:.2f} %)")
    assert 2 * bad < bad_raw          # the aggregation helps: 16 % / 20 % against 59 % / 61 %
    assert bad == PINNED[name]


@pytest.mark.parametrize("W,H,D", SHAPES)
def test_selection_is_oracle_wta(oracle, W, H, D):
    l, r = noise_pair(W, H)
    lmap, rmap = M.maps(l, r, D)
    for side, got in ((0, lmap), (1, rmap)):
        assert np.array_equal(got, oracle.wta(M.volume(l, r, side, 0, D)))


def test_constant_pair_selects_the_lowest_candidate(oracle):
    """Exact ties go to the lowest candidate.  On a constant pair every interior cost is 0, so d = 1 ties with every other slice
    wherever the windows see no border column - and wins; nothing selects d = 0."""
    W, H, D = 40, 16, 8
    l = np.full((H, W), 77, np.uint8)
    lmap, rmap = M.maps(l, l.copy(), D)
    assert np.all(lmap == 1) and np.all(rmap == 1)
