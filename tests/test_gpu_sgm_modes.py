"""-m gpu: StereoSGBM's modes on the device (psm_sgm_set_mode, DispEst.SGBM_GPU(mode=...)) against the definition,
tests/sgm_mode_model.py.  Everything is integer: C, S and the map equal the model with 0 differing elements - there is no tolerance anywhere in this file.

A context is at least 8 x 8 (psm_create refuses less: test_images_under_8_rows_or_columns_exist_in_the_models_only), so the
device shapes start there: heights 8 .. 11 are the four remainders of H by the four rows of a workgroup (0 to 3 waves leave at
the wave-uniform exit past H), widths 8 and 9 the shortest paths.  Rows of 1, 2 and 3 columns and images of 1 to 5 rows are held
to the same sums by the CPU tests (tests/test_sgm_mode_model.py)."""
import functools

import numpy as np
import pytest

import fuzz_inputs as F
import sgm_mode_model as MM
import speckle_model as K

pytestmark = pytest.mark.gpu

REDUCED = ("sgbm", "3way", "hh4")
NDIR = {"sgbm": 5, "hh": 8, "3way": 3, "hh4": 4}


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@functools.lru_cache(maxsize=None)
def pair(W, H, D, seed):
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=seed)
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


@functools.lru_cache(maxsize=None)
def model(W, H, D, seed, mode):
    """sgm_mode_model.sgm of pair (W, H, D, seed) at the default parameters: computed once, shared, left unchanged"""
    ref = MM.sgm(*pair(W, H, D, seed), D, mode)
    for k in ("C", "S", "disp"):
        ref[k].setflags(write=False)
    return ref


def differing(name, de, ref, disp, speckle=(0, 0)):
    """C, S and the map (through the speckle model where the filter ran) of the last compute of `de` against a model result ->
    the counts of differing elements, printed"""
    want, _ = K.sgbm_speckle(ref["disp"], *speckle)
    Cd, Sd = de.sgm_costs()
    assert disp.dtype == np.int16 and Cd.dtype == np.uint16 and Sd.dtype == np.uint32
    n = [int(np.count_nonzero(a != b)) for a, b in ((Cd, ref["C"]), (Sd, ref["S"]), (disp, want))]
    print(f"[sgm-modes] {name}: differing elements C {n[0]}  S {n[1]}  map {n[2]}  (max S {int(ref['S'].max())})")
    return n


def check(name, de, ref, disp, speckle=(0, 0)):
    n = differing(name, de, ref, disp, speckle)
    assert n == [0, 0, 0], (name, n, np.argwhere(de.sgm_costs()[1] != ref["S"])[:8].tolist())


def test_images_under_8_rows_or_columns_exist_in_the_models_only(psm):
    for W, H, D in ((2, 8, 2), (3, 8, 2), (256, 3, 256), (255, 5, 253), (16, 1, 4)):
        with pytest.raises(psm.capi.PsmError):
            psm.DispEst(np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8), D)
        assert "8x8" in psm.capi.last_error(None)


# tests/test_gpu_sgm.py's shapes, and the padding lanes of four disparities per lane (Dp = 256: the ALL form)
@pytest.mark.parametrize("W,H,D", [(67, 45, 16), (131, 70, 33), (33, 21, 33), (9, 40, 2), (150, 37, 130), (140, 33, 129), (256, 8, 256),
                                   (255, 9, 253)])
def test_every_mode_on_small_pairs(psm, W, H, D):
    l, r = pair(W, H, D, W)
    with psm.DispEst(l, r, D) as de:
        for mode in REDUCED:
            check(f"{W}x{H}x{D} {mode}", de, model(W, H, D, W, mode), de.SGBM_GPU(mode=mode))
            by_value = de.SGBM_GPU(mode=MM.VALUES[mode])                                  # OpenCV's integer
            check(f"{W}x{H}x{D} mode {MM.VALUES[mode]}", de, model(W, H, D, W, mode), by_value)


# Short rows and few rows, where a reduced mode's first (storing) launch is a row direction: a row path of W columns takes SGM_U = 8
# steps per batch of loads, W = 15 .. 17 stand on both sides of two batches (where the branch-free main loop first runs), 31 .. 34
# of four, 63 .. 65 of eight.  D + 1 = W with D at and below 64, 128 and 256: the ALL forms and their padding lanes, and the
# narrowest image a context of that D accepts.
ROWS_SHAPES = ([(8, 8, 2), (8, 9, 8), (9, 10, 2), (9, 11, 9)] +
               [(W, 8 + i % 4, 2 + (5 * i) % 14) for i, W in enumerate((15, 16, 17, 31, 32, 33, 34, 63, 64, 65))] +
               [(D + 1, 9, D) for D in (61, 63, 64, 125, 127, 253, 255)])


@pytest.mark.parametrize("W,H,D", ROWS_SHAPES)
def test_short_rows_and_few_rows(psm, W, H, D):
    assert D <= 15 or W == D + 1
    rng = np.random.default_rng(W * 1000 + H)
    l, r = F.sgm_content("noise", W, H, D, rng)
    with psm.DispEst(l, r, D) as de:
        for mode in ("3way", "sgbm"):
            check(f"rows {W}x{H}x{D} {mode}", de, MM.sgm(l, r, D, mode), de.SGBM_GPU(mode=mode))


def test_the_first_direction_stores(psm):
    """hh -> 3way -> sgbm -> hh4 -> hh on one context, twice, another pair in between: no sum of an earlier mode or frame survives
    in S."""
    W, H, D = 120, 50, 40
    other = pair(W, H, D, 1)
    with psm.DispEst(*pair(W, H, D, 0), D) as de:
        first = de.SGBM_GPU(mode="hh")
        check("hh", de, model(W, H, D, 0, "hh"), first)
        S_first = de.sgm_costs()[1]
        for turn in (0, 1):
            check(f"3way, turn {turn}", de, model(W, H, D, 0, "3way"), de.SGBM_GPU(mode="3way"))
            check(f"sgbm, turn {turn}", de, model(W, H, D, 0, "sgbm"), de.SGBM_GPU(mode="sgbm"))
            de.setInputImages(*other)
            check(f"hh4, turn {turn}, the other pair", de, model(W, H, D, 1, "hh4"), de.SGBM_GPU(mode="hh4"))
            check(f"hh, turn {turn}, the other pair", de, model(W, H, D, 1, "hh"), de.SGBM_GPU(mode="hh"))
            de.setInputImages(*pair(W, H, D, 0))
            check(f"hh4, turn {turn}", de, model(W, H, D, 0, "hh4"), de.SGBM_GPU(mode="hh4"))
        last = de.SGBM_GPU()                                                               # the default is hh
        check("hh again", de, model(W, H, D, 0, "hh"), last)
        assert np.array_equal(first, last) and np.array_equal(S_first, de.sgm_costs()[1])


# Cones / Teddy at D 64, defaults, SAD: (max S, map elements != the hh map) - the figures tests/test_sgm_mode_model.py pins
FIGURES = {"sgbm": ((75600, 89990), (85795, 100654)), "3way": ((45360, 89033), (51477, 100181)), "hh4": ((60480, 71262), (68636, 84360))}


@pytest.mark.parametrize("i,name", [(0, "cones"), (1, "teddy")])
def test_the_modes_are_different_algorithms(psm, golden, i, name):
    p, g = golden(f"{name}_pair.npz"), golden(f"{name}_sgm.npz")
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        assert np.array_equal(de.SGBM_GPU(mode="hh"), g["disp"])
        for mode, figures in FIGURES.items():
            disp = de.SGBM_GPU(mode=mode)
            got = (int(de.sgm_costs()[1].max()), int(np.count_nonzero(disp != g["disp"])))
            print(f"[sgm-modes] {name} {mode}: max S {got[0]}  map elements != hh {got[1]}")
            assert got == figures[i]


@pytest.mark.parametrize("mode", REDUCED)
def test_everything_downstream_composes(psm, mode):
    W, H, D = 131, 38, 33
    l, r = pair(W, H, D, 21)
    kw = dict(mode=mode)
    with psm.DispEst(l, r, D) as de:
        ref = MM.sgm(l, r, D, mode, pre_filter_cap=63)
        check(f"{mode} cap 63", de, ref, de.SGBM_GPU(pre_filter_cap=63, **kw))
        for side in (0, 1):
            assert np.array_equal(de.sgm_prefiltered(side), ref["planes"][side])
        disp = de.SGBM_GPU(speckle_window_size=100, speckle_range=32, **kw)
        check(f"{mode} speckle", de, model(W, H, D, 21, mode), disp, (100, 32))
        assert np.array_equal(de.sgm_speckle_sizes(), K.sgbm_speckle(model(W, H, D, 21, mode)["disp"], 100, 32)[1])
        gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
        check(f"{mode} gray", de, MM.sgm(gl, gr, D, mode), de.SGBM_GPU(gray=(gl, gr), **kw))
        de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        check(f"{mode} timed", de, model(W, H, D, 21, mode), de.SGBM_GPU(**kw))
        assert len(de.sgm_times()) == 3 and all(t > 0 for t in de.sgm_times())
    rng = np.random.default_rng(7)
    lf, rf = F.float_pair(l, r, rng)
    with psm.DispEst(lf, rf, D) as df:
        check(f"{mode} float pair", df, MM.sgm(lf, rf, D, mode), df.SGBM_GPU(**kw))


# (W, H, D, d_star, block size): a path cost climbs by 255 ch bs^2 a step, so the columns need 86 rows at block size 1, 10 at 3
@pytest.mark.parametrize("W,H,D,d_star,bs", [(200, 190, 7, 3, 1), (200, 40, 6, 2, 3), (260, 30, 130, 5, 3)])
def test_saturating_pairs(psm, W, H, D, d_star, bs):
    """L_r at 65535 on every path of the mode, S at directions x 65535"""
    l, r = F.saturating_pair(W, H, D, d_star)
    kw = F.saturating_params(bs)
    with psm.DispEst(l, r, D) as de:
        for mode in REDUCED:
            ref = MM.sgm(l, r, D, mode, **kw)
            assert ref["max_l"] == 65535 and int(ref["S"].max()) == NDIR[mode] * 65535
            check(f"saturating {W}x{H}x{D} bs {bs} {mode}", de, ref, de.SGBM_GPU(mode=mode, **kw))


@pytest.mark.parametrize("kind,W,H,D,seed", F.TIE_CASES)
def test_exact_ties(psm, kind, W, H, D, seed):
    l, r = F.tie_pair(kind, W, H, D, seed)
    with psm.DispEst(l, r, D) as de:
        for mode in REDUCED:
            for extra in (dict(), dict(uniqueness_ratio=0, disp12_max_diff=-1)):
                check(f"{kind} {W}x{H}x{D} {mode} {extra}", de, MM.sgm(l, r, D, mode, **extra), de.SGBM_GPU(mode=mode, **extra))


@pytest.mark.parametrize("mode", REDUCED)
def test_batches_equal_the_single_calls(psm, mode):
    from primestereomatch_amd import dispest
    W, H, D = 93, 41, 24
    pairs = [F.sgm_content(kind, W, H, D, np.random.default_rng(i)) for i, kind in enumerate(("synth", "noise", "half_flat"))]
    des = [psm.DispEst(l, r, D) for l, r in pairs]
    try:
        maps = dispest.sgbm_batch(des, mode=mode)
        for i, (de, disp) in enumerate(zip(des, maps)):
            l, r = pairs[i]
            check(f"batch {mode} pair {i}", de, MM.sgm(l, r, D, mode), disp)
            with psm.DispEst(l, r, D) as one:
                single = one.SGBM_GPU(mode=mode)
                assert np.array_equal(single, disp)
                assert all(np.array_equal(a, b) for a, b in zip(one.sgm_costs(), de.sgm_costs()))
    finally:
        for d in des:
            d.close()


def test_batches_refuse_mixed_modes(psm):
    from primestereomatch_amd import dispest
    W, H, D = 64, 32, 16
    des = [psm.DispEst(*pair(W, H, D, s), D) for s in range(3)]
    try:
        before = dispest.sgbm_batch(des, mode="3way")
        des[2]._ck(des[2]._lib.psm_sgm_set_mode(des[2]._h, MM.VALUES["sgbm"]), "set_mode")
        with pytest.raises(psm.capi.PsmError, match=r"context 2 has another mode \(0\) than context 0 \(2\)"):
            dispest.sgm_compute_batch(des)
        des[2]._ck(des[2]._lib.psm_sgm_set_mode(des[2]._h, MM.VALUES["3way"]), "set_mode")
        des[1]._ck(des[1]._lib.psm_sgm_set_mode(des[1]._h, MM.VALUES["hh"]), "set_mode")
        with pytest.raises(psm.capi.PsmError, match=r"context 1 has another mode \(1\) than context 0 \(2\)"):
            dispest.sgm_compute_batch(des)
        for de, disp in zip(des, before):                                                 # nothing was enqueued: the results are still there
            assert np.array_equal(de.sgm_disparity(), disp)
        for bad in (-1, 4):
            assert des[0]._lib.psm_sgm_set_mode(des[0]._h, bad) != 0
            assert all(w in psm.capi.last_error(des[0]._h) for w in ("MODE_SGBM", "MODE_HH", "MODE_SGBM_3WAY", "MODE_HH4"))
        with pytest.raises(ValueError):
            des[0].SGBM_GPU(mode="hh8")
    finally:
        for d in des:
            d.close()


SWEEP = F.sgm_geometries(24, 20261018)


@pytest.mark.parametrize("W,H,D,seed", SWEEP)
def test_seeded_sweep(psm, W, H, D, seed):
    rng = np.random.default_rng([seed, 1])                                                # the draws of this file, apart from sgm_case's
    mode, bt = str(rng.choice(REDUCED)), bool(rng.random() < 0.4)
    kind, l, r, kw, gray, speckle = F.sgm_case(W, H, D, seed, bt)
    g = (np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])) if gray else None
    ref = MM.sgm(*(g or (l, r)), D, mode, **kw)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(gray=g, speckle_window_size=speckle[0], speckle_range=speckle[1], mode=mode, **kw)
        check(f"{W}x{H}x{D} {kind} {mode} {kw} gray {gray} speckle {speckle}", de, ref, disp, speckle)


def test_the_sweep_draws_every_mode():
    drawn = {str(np.random.default_rng([seed, 1]).choice(REDUCED)) for W, H, D, seed in SWEEP}
    assert len(SWEEP) >= 24 and drawn == set(REDUCED)
