"""-m gpu: the SGM stage under a disparity range (psm_sgm_set_range, DispEst.SGBM_GPU(min_disparity=..., num_disparities=...)) against
the definition, tests/sgm_range_model.py.  Everything is integer: C, S and the int16 map equal the model with 0 differing elements -
np.array_equal, there is no tolerance anywhere in this file.

The contexts are built with max_disp 4: the range is independent of it (and of the width).  Above 256 disparities the cost kernels
walk a tile once per 256 of them (the WIDE forms), a lane of k_sgm_path / k_sgm_select holds 8 (Dp <= 512) or 16 disparities, Dp is
D rounded up to 8 or 16, and the packed minima carry a 10-bit index: the shapes below are the smallest that reach each form."""
import functools

import numpy as np
import pytest

import fuzz_inputs as F
import sgm_bt_model as B
import sgm_model as M
import sgm_range_model as R
import speckle_model as K

pytestmark = pytest.mark.gpu

MODES = ("sgbm", "hh", "3way", "hh4")
MAXDIS = 4


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def shifted_pair(W, H, s, seed, spoil=True):
    """Noise, and the right image such that L[x] = R[clamp(x - s)] - except, with spoil, in a block of the right image that is noise
    of its own: pixels there match nothing (not unique, or rejected by the consistency test)."""
    rng = np.random.default_rng([seed, W, H])
    l = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = np.ascontiguousarray(l[:, np.clip(np.arange(W) + s, 0, W - 1)])
    if spoil:
        y0, x0 = H // 4, W // 3
        r[y0:y0 + H // 2, x0:x0 + W // 4] = rng.integers(0, 256, (H // 2, W // 4, 3), dtype=np.uint8)
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


@functools.lru_cache(maxsize=None)
def noise_pair(W, H, seed):
    l, r = np.random.default_rng([seed, W, H]).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


@functools.lru_cache(maxsize=None)
def noise_model(W, H, seed, dmin, D, mode="hh", cap=0, bs=0):
    """sgm_range_model.sgm of noise_pair(W, H, seed): computed once, shared, left unchanged"""
    return frozen(R.sgm(*noise_pair(W, H, seed), dmin, D, mode, pre_filter_cap=cap, block_size=bs))


def frozen(ref):
    for k in ("C", "S", "disp"):
        ref[k].setflags(write=False)
    return ref


def expected_map(ref, speckle=(0, 0)):
    if speckle[0] <= 0:
        return ref["disp"]
    return K.filter_speckles(ref["disp"], ref["invalid"], speckle[0], 16 * speckle[1])[0]


def check(name, de, ref, disp, speckle=(0, 0)):
    """C, S and the map of the last compute of `de` against a model result: 0 differing elements"""
    Cd, Sd = de.sgm_costs()
    assert disp.dtype == np.int16 and Cd.dtype == np.uint16 and Sd.dtype == np.uint32
    assert Cd.shape == ref["C"].shape and Sd.shape == ref["S"].shape
    want = expected_map(ref, speckle)
    n = [int(np.count_nonzero(a != b)) for a, b in ((Cd, ref["C"]), (Sd, ref["S"]), (disp, want))]
    print(f"[sgm-range] {name}: differing elements C {n[0]}  S {n[1]}  map {n[2]}  (max S {int(ref['S'].max())})")
    assert np.array_equal(Cd, ref["C"]), (name, n, np.argwhere(Cd != ref["C"])[:8].tolist())
    assert np.array_equal(Sd, ref["S"]), (name, n, np.argwhere(Sd != ref["S"])[:8].tolist())
    assert np.array_equal(disp, want), (name, n, np.argwhere(disp != want)[:8].tolist())


def run(de, dmin, D, **kw):
    return de.SGBM_GPU(min_disparity=dmin, num_disparities=D, **kw)


# ---------------------------------------------------------------------------------------------------- lane counts and padding

# 257: the smallest NV 8 (Dp 264, no multiple of 64); 300; 509, 511: NV 8 ALL with padding; 512: ALL; 513: the smallest NV 16 (Dp 528);
# 1021, 1023: NV 16 ALL with padding; 1024: ALL
LANE_D = (257, 300, 509, 511, 512, 513, 1021, 1023, 1024)


@pytest.mark.parametrize("D", LANE_D)
def test_lane_counts_and_padding(psm, D):
    W, H = 40, 12
    l, r = noise_pair(W, H, D)
    with psm.DispEst(l, r, MAXDIS) as de:
        check(f"{W}x{H}x{D} SAD", de, noise_model(W, H, D, 0, D), run(de, 0, D))
        check(f"{W}x{H}x{D} cap 63 bs 5", de, noise_model(W, H, D, 0, D, "hh", 63, 5), run(de, 0, D, pre_filter_cap=63, block_size=5))
        # the range around 0: both clamps act and the winners sit in the middle lanes, not in the first
        check(f"{W}x{H}x{D} SAD min {-(D // 2)}", de, noise_model(W, H, D, -(D // 2), D), run(de, -(D // 2), D))


@pytest.mark.parametrize("D", (300, 512, 1024))
def test_every_mode_at_wide_ranges(psm, D):
    W, H = 40, 12
    l, r = noise_pair(W, H, D)
    with psm.DispEst(l, r, MAXDIS) as de:
        for mode in MODES:
            check(f"{W}x{H}x{D} {mode}", de, noise_model(W, H, D, -(D // 2), D, mode), run(de, -(D // 2), D, mode=mode))
            check(f"{W}x{H}x{D} {mode} min 0", de, noise_model(W, H, D, 0, D, mode), run(de, 0, D, mode=mode))


@pytest.mark.parametrize("W,H,D", [(600, 9, 512), (1100, 8, 1024)])
def test_rows_wider_than_the_range(psm, W, H, D):
    """the staged span and the interior x - delta >= 0 of the cost kernels, not only the clamp"""
    l, r = shifted_pair(W, H, D - 40, D)
    ref = R.sgm(l, r, 0, D)
    assert np.count_nonzero(ref["best"] >= 256) > W                          # winners above the 8-bit index
    with psm.DispEst(l, r, MAXDIS) as de:
        check(f"{W}x{H}x{D} SAD", de, ref, run(de, 0, D))
        if D <= 512:
            check(f"{W}x{H}x{D} cap 63", de, R.sgm(l, r, 0, D, pre_filter_cap=63), run(de, 0, D, pre_filter_cap=63))
        else:                                          # (the model's paths and selection once per case: they do not depend on the cost's kind)
            run(de, 0, D, pre_filter_cap=63)
            planes = B.prefilter(l, 63), B.prefilter(r, 63)
            assert np.array_equal(de.sgm_costs()[0], M.block_cost(R.pixel_cost_planes(*planes, 0, D), 5))


@pytest.mark.parametrize("W", (33, 129, 161))
def test_tile_seams_at_every_chunk(psm, W):
    """SGM_TX = 32 and SGM_BT_TX = 128 are crossed at both chunks of 256 disparities, with the widest block"""
    H, D = 9, 300
    l, r = noise_pair(W, H, 7)
    with psm.DispEst(l, r, MAXDIS) as de:
        check(f"{W}x{H}x{D} bs 7 SAD", de, noise_model(W, H, 7, -150, D, "hh", 0, 7), run(de, -150, D, block_size=7))
        check(f"{W}x{H}x{D} bs 7 cap 63", de, noise_model(W, H, 7, -150, D, "hh", 63, 7), run(de, -150, D, block_size=7, pre_filter_cap=63))
        check(f"{W}x{H}x{D} bs 7 SAD min 0", de, noise_model(W, H, 7, 0, D, "hh", 0, 7), run(de, 0, D, block_size=7))


# ---------------------------------------------------------------------------------------------------- min_disparity

MINS = (-40, -7, -1, 1, 5, 16, 45)


def _true_shift(dmin, D):
    """-1 where the range holds it (valid pixels are then -16, the invalid value of range (0, .)), else a third into the range"""
    return -1 if dmin <= -1 < dmin + D else dmin + D // 3


@pytest.mark.parametrize("W,H,D", [(37, 11, 64), (40, 12, 300)])
@pytest.mark.parametrize("dmin", MINS)
def test_min_disparity(psm, W, H, D, dmin):
    """Every minimum with disp12_max_diff 0, 1 and off, without and with the speckle filter.  The filter runs with two windows: 100,
    and W H, under which every component is a speckle.  A filter that still took -16 for the background would make the invalid
    pixels of small components -16 instead of leaving them, and would leave the valid pixels at -16 (true shift -1) alone: the
    model's own map must tell the two apart under at least one of the windows."""
    s = _true_shift(dmin, D)
    l, r = shifted_pair(W, H, s, 1000 + dmin)
    told_apart = False
    with psm.DispEst(l, r, MAXDIS) as de:
        for m in (0, 1, -1):
            ref = R.sgm(l, r, dmin, D, disp12_max_diff=m)
            inv = ref["invalid"]
            assert inv == (dmin - 1) * 16 != -16
            if s == -1 and W > 8 - dmin:
                assert np.count_nonzero(ref["valid"] & (ref["disp"] == -16)) > W
            check(f"{W}x{H}x{D} min {dmin} m {m}", de, ref, run(de, dmin, D, disp12_max_diff=m))
            for speckle in ((100, 32), (W * H, 32)):
                right = K.filter_speckles(ref["disp"], inv, speckle[0], 16 * speckle[1])
                wrong = K.filter_speckles(ref["disp"], -16, speckle[0], 16 * speckle[1])
                told_apart |= not np.array_equal(right[0], wrong[0])
                disp = run(de, dmin, D, disp12_max_diff=m, speckle_window_size=speckle[0], speckle_range=speckle[1])
                check(f"{W}x{H}x{D} min {dmin} m {m} speckle {speckle}", de, ref, disp, speckle)
                assert np.array_equal(de.sgm_speckle_sizes(), right[1])
    assert told_apart


def test_valid_values_can_be_negative(psm):
    """A pair whose true shift is negative: the valid d16 are negative, and some unique pixels with a negative d16 are rejected by
    the consistency test - a validity test `v >= 0` would let them through."""
    W, H, dmin, D, s = 48, 12, -20, 24, -9
    l, r = shifted_pair(W, H, s, 5)
    ref = R.sgm(l, r, dmin, D, disp12_max_diff=0)
    assert np.count_nonzero(ref["valid"] & (ref["disp"] < 0)) > W * H // 3
    assert np.any(ref["unique"] & ~ref["valid"] & (ref["d16"] < 0))
    assert np.all(ref["disp"] < 0)
    with psm.DispEst(l, r, MAXDIS) as de:
        check("negative shift", de, ref, run(de, dmin, D, disp12_max_diff=0))
        gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
        check("negative shift, gray", de, R.sgm(gl, gr, dmin, D, disp12_max_diff=0), run(de, dmin, D, disp12_max_diff=0, gray=(gl, gr)))


# ---------------------------------------------------------------------------------------------------- the key's width

def test_winners_above_2_to_the_18_with_an_index_above_255(psm):
    """fuzz_inputs.high_floor_pair (its generator takes no D: the size is the argument) at 1024 disparities around 0: the winner's own
    S needs the 19th bit, its index the 9th and 10th - the packed minimum uses all 29 bits"""
    W, H, dmin, D = 560, 8, -500, 1024
    l, r = F.high_floor_pair(W, H, np.random.default_rng(D))
    ref = R.sgm(l, r, dmin, D, **F.HIGH_FLOOR_PARAMS)
    minS = ref["S"].min(axis=2)
    assert np.count_nonzero((ref["best"] >= 256) & (minS >= 1 << 18)) > W * H // 4
    assert np.count_nonzero(ref["best"] >= 512) > W * H // 8
    with psm.DispEst(l, r, MAXDIS) as de:
        check("high floor", de, ref, run(de, dmin, D, **F.HIGH_FLOOR_PARAMS))


def half_period_pair(W, H, delta, phase):
    """The saturating construction of fuzz_inputs.saturating_pair restated for a range of 1024: the right image is 0 / 255 by column
    with a half period of 512 (its alternation by column ties every second disparity, so the lowest index would win).  Against the
    left image, R moved by delta, the disparity delta costs 0 at every pixel and delta +- 512 costs 255 ch at every pixel; no other
    disparity within 1023 of delta costs 0 everywhere."""
    b = lambda x: ((((x + phase) >> 9) & 1) * 255).astype(np.uint8)
    x = np.arange(W)
    r = np.broadcast_to(b(x)[None, :, None], (H, W, 3))
    l = np.broadcast_to(b(x - delta)[None, :, None], (H, W, 3))         # (beyond the row's ends too: what R would show there)
    return np.ascontiguousarray(l), np.ascontiguousarray(r)


def test_a_saturating_pair_at_1024(psm):
    """S at 8 * 65535 in the volume, winners with an index above 255"""
    W, H, dmin, D = 560, 22, -600, 1024
    k_star = 300
    l, r = half_period_pair(W, H, dmin + k_star, 40)
    kw = F.saturating_params(3)
    ref = R.sgm(l, r, dmin, D, **kw)
    assert ref["max_l"] == 65535 and int(ref["S"].max()) == 8 * 65535
    assert np.count_nonzero(ref["unique"] & (ref["best"] == k_star)) > W
    with psm.DispEst(l, r, MAXDIS) as de:
        check("saturating", de, ref, run(de, dmin, D, **kw))


def test_exact_ties_whose_lowest_index_is_above_255(psm):
    """A constant left image; a right image that is the same constant except its last column.  The low indices (far negative
    disparities) all read the last column; from some index above 255 on every disparity reads the constant: S ties exactly at 0
    there, and the lowest of them must win."""
    W, H, D = 40, 12, 1024
    dmin = -(W + 300)
    l = np.full((H, W, 3), 90, np.uint8)
    r = l.copy()
    r[:, -1] = 200
    for extra in (dict(), dict(uniqueness_ratio=0, disp12_max_diff=-1)):
        ref = R.sgm(l, r, dmin, D, **extra)
        best = ref["best"].astype(int)
        assert best.min() > 255
        ties = np.take_along_axis(ref["S"], (best + 7)[:, :, None], 2)[:, :, 0] == ref["S"].min(axis=2)
        assert np.all(ties)
        with psm.DispEst(l, r, MAXDIS) as de:
            check(f"ties {extra}", de, ref, run(de, dmin, D, **extra))
    l, r = F.tie_pair("stripes", W, H, 300, 3)
    with psm.DispEst(l, r, MAXDIS) as de:
        check("stripes", de, R.sgm(l, r, -150, 300), run(de, -150, 300))


# ---------------------------------------------------------------------------------------------------- state

def test_no_volume_size_or_pointer_of_an_earlier_range_survives(psm):
    """(0, 0) -> (-5, 300) -> (0, 0) -> (3, 64) -> (0, 1024) on one context, another pair at every step: each result is the model's"""
    W, H, maxdis = 40, 12, 16
    with psm.DispEst(*noise_pair(W, H, 0), maxdis) as de:
        for i, (dmin, nd) in enumerate(((0, 0), (-5, 300), (0, 0), (3, 64), (0, 1024), (0, 0))):
            l, r = shifted_pair(W, H, dmin + 2, 50 + i)
            de.setInputImages(l, r)
            D = nd or maxdis
            ref = R.sgm(l, r, dmin, D)
            check(f"step {i}: range ({dmin}, {nd})", de, ref, run(de, dmin, nd))
            assert de.sgm_costs()[0].shape == (H, W, D)


def test_cones_is_reproduced_after_a_wide_range(psm, golden):
    """The golden map of Cones at (0, 0); a range of 300 and one of 1024 on the same context in between (6 * W * H * Dp bytes of
    volumes, allocated again at every change; the models of those sizes take minutes, the small chain above holds every step to
    its model)."""
    p, g = golden("cones_pair.npz"), golden("cones_sgm.npz")
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        assert np.array_equal(de.SGBM_GPU(), g["disp"])
        for dmin, D in ((-5, 300), (0, 1024)):
            wide = run(de, dmin, D)
            ok = wide != (dmin - 1) * 16
            assert ok.any() and wide[ok].min() >= 16 * dmin - 8 and wide[ok].max() <= 16 * (dmin + D - 1) + 8
            assert np.array_equal(de.SGBM_GPU(), g["disp"])
        assert de.sgm_costs()[1].shape == g["disp"].shape + (64,)


def test_values_outside_the_ranges_are_refused_on_a_context(psm):
    with psm.DispEst(*noise_pair(40, 12, 0), MAXDIS) as de:
        before = run(de, -3, 40)
        for bad in ((-1025, 0), (1025, 0), (0, 1), (0, 1025), (0, -2)):
            assert de._lib.psm_sgm_set_range(de._h, *bad) != 0
            assert "psm_sgm_set_range" in psm.capi.last_error(de._h)
        assert np.array_equal(de.sgm_disparity(), before)                                 # the setting and the result are untouched
        de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
        assert np.array_equal(de.sgm_disparity(), before)


# ---------------------------------------------------------------------------------------------------- batches

def test_a_batch_equals_the_single_calls(psm):
    from primestereomatch_amd import dispest
    W, H, dmin, D = 40, 12, -5, 300
    pairs = [shifted_pair(W, H, s, 70 + s) for s in (-3, 20, 250)]
    des = [psm.DispEst(l, r, MAXDIS) for l, r in pairs]
    try:
        first = dispest.sgbm_batch(des)                                                   # (0, 0): the table names these volumes ...
        maps = dispest.sgbm_batch(des, min_disparity=dmin, num_disparities=D, speckle_window_size=20, speckle_range=2)   # ... not these
        for i, (de, disp) in enumerate(zip(des, maps)):
            l, r = pairs[i]
            check(f"batch pair {i}", de, R.sgm(l, r, dmin, D), disp, (20, 2))
            with psm.DispEst(l, r, MAXDIS) as one:
                single = run(one, dmin, D, speckle_window_size=20, speckle_range=2)
                assert np.array_equal(single, disp)
                assert all(np.array_equal(a, b) for a, b in zip(one.sgm_costs(), de.sgm_costs()))
        again = dispest.sgbm_batch(des)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    finally:
        for d in des:
            d.close()


def test_batches_refuse_mixed_ranges(psm):
    from primestereomatch_amd import dispest
    W, H = 40, 12
    des = [psm.DispEst(*noise_pair(W, H, s), MAXDIS) for s in range(3)]
    try:
        before = dispest.sgbm_batch(des, min_disparity=-5, num_disparities=300)
        des[2]._ck(des[2]._lib.psm_sgm_set_range(des[2]._h, -5, 301), "set_range")
        with pytest.raises(psm.capi.PsmError, match=r"context 2 has another disparity range \(min -5, 301 disparities\) than context 0 \(min -5, 300\)"):
            dispest.sgm_compute_batch(des)
        des[2]._ck(des[2]._lib.psm_sgm_set_range(des[2]._h, -5, 300), "set_range")
        des[1]._ck(des[1]._lib.psm_sgm_set_range(des[1]._h, -4, 300), "set_range")
        with pytest.raises(psm.capi.PsmError, match=r"context 1 has another disparity range \(min -4, 300 disparities\)"):
            dispest.sgm_compute_batch(des)
        for de, disp in zip(des, before):                                                 # nothing was enqueued: the results are still there
            assert np.array_equal(de.sgm_disparity(), disp)
            assert de.sgm_costs()[1].shape == (H, W, 300)
    finally:
        for d in des:
            d.close()


# ---------------------------------------------------------------------------------------------------- a seeded sweep

def sweep_cases(n, seed):
    """-> (W, H, D, min_disparity, mode, cap, kw, seed): D over [2, 1024] with every lane count drawn, min over [-64, 64]"""
    rng = np.random.default_rng(seed)
    bands = ((2, 64), (65, 128), (129, 256), (257, 512), (513, 1024))
    out = []
    for i in range(n):
        lo, hi = bands[i % len(bands)]
        D = int(rng.integers(lo, hi + 1))
        W, H = int(rng.integers(8, 97)), int(rng.integers(8, 25))
        dmin = int(rng.integers(-64, 65))
        mode = MODES[int(rng.integers(0, 4))]
        cap = int(rng.choice([1, 15, 31, 63])) if i % 2 else 0
        bs = int(rng.choice([1, 3, 5, 7]))
        kw = dict(block_size=bs, uniqueness_ratio=int(rng.choice([0, 10, 50])), disp12_max_diff=int(rng.choice([-1, 0, 1, 5])))
        out.append((W, H, D, dmin, mode, cap, kw, int(rng.integers(0, 1 << 30))))
    return out


SWEEP = sweep_cases(20, 20261019)


@pytest.mark.parametrize("W,H,D,dmin,mode,cap,kw,seed", SWEEP)
def test_seeded_sweep(psm, W, H, D, dmin, mode, cap, kw, seed):
    rng = np.random.default_rng(seed)
    kind = str(rng.choice(("noise", "shift", "binary", "synth")))
    if kind == "shift":
        l, r = shifted_pair(W, H, dmin + int(rng.integers(0, D)), seed)
    else:
        l, r = F.sgm_content(kind, W, H, min(D, W), rng)
    speckle = (int(rng.integers(1, 200)), int(rng.integers(0, 40))) if rng.random() < 0.3 else (0, 0)
    ref = R.sgm(l, r, dmin, D, mode, pre_filter_cap=cap, **kw)
    with psm.DispEst(l, r, MAXDIS) as de:
        disp = run(de, dmin, D, mode=mode, pre_filter_cap=cap, speckle_window_size=speckle[0], speckle_range=speckle[1], **kw)
        check(f"seed {seed}: {W}x{H}x{D} min {dmin} {kind} {mode} cap {cap} {kw} speckle {speckle}", de, ref, disp, speckle)


def test_the_sweep_draws_every_form():
    assert len(SWEEP) >= 20
    assert {c[4] for c in SWEEP} == set(MODES) and {c[5] > 0 for c in SWEEP} == {True, False}
    assert any(c[2] > 512 for c in SWEEP) and any(256 < c[2] <= 512 for c in SWEEP) and any(c[2] <= 64 for c in SWEEP)
    assert any(c[3] < 0 for c in SWEEP) and any(c[3] > 0 for c in SWEEP)
