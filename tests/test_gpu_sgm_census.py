"""-m gpu: the SGM stage's census cost on the device (psm_sgm_set_census, DispEst.SGBM_GPU(census=(w, h))) against its definition,
the numpy model tests/sgm_census_model.py.  Everything is integer: the code planes of both images, the block costs C, the summed
path costs S and the final int16 map must equal the model with 0 differing elements - there is no tolerance anywhere in this
file."""
import functools
import hashlib

import numpy as np
import pytest

import sgm_bt_model as B
import sgm_census_model as Z
import sgm_range_model as R
import speckle_model as K

pytestmark = pytest.mark.gpu

COST_TILE_W = 32    # SGM_TX: the pixels of a row a workgroup of k_sgm_census_cost owns
CENSUS_TILE_W = 32  # SGM_CEN_TX, SGM_CEN_TY: the tile of pixels a workgroup of k_sgm_census owns
CENSUS_TILE_H = 8
PASS_D = 256        # the disparities of one pass of k_sgm_census_cost: the right span is staged again for every pass


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def compare(name, de, ref, disp):
    """Both code planes, C, S and the map of the last SGBM_GPU of `de` against a model result; prints the counts, asserts 0."""
    Cd, Sd = de.sgm_costs()
    tl, tr = de.sgm_census(0), de.sgm_census(1)
    assert tl.shape == ref["codes"][0].shape and tl.dtype == np.uint64
    n = [int(np.count_nonzero(a != b)) for a, b in ((tl, ref["codes"][0]), (tr, ref["codes"][1]), (Cd, ref["C"]), (Sd, ref["S"]),
                                                    (disp, ref["disp"]))]
    print(f"[sgm-census] {name}: differing elements codes {n[0]} + {n[1]}  C {n[2]}  S {n[3]}  map {n[4]}  (valid {ref['valid'].mean():.3f})")
    assert disp.dtype == np.int16 and Cd.dtype == np.uint16 and Sd.dtype == np.uint32
    assert n == [0, 0, 0, 0, 0]


def compare_other(name, de, ref, disp):
    Cd, Sd = de.sgm_costs()
    n = [int(np.count_nonzero(a != b)) for a, b in ((Cd, ref["C"]), (Sd, ref["S"]), (disp, ref["disp"]))]
    print(f"[sgm-census] {name}: differing elements C {n[0]}  S {n[1]}  map {n[2]}")
    assert n == [0, 0, 0]


@functools.lru_cache(maxsize=None)
def pair(W, H, D, seed=0):
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=seed)
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


@functools.lru_cache(maxsize=None)
def model(W, H, D, seed, census=(9, 7), dmin=0):
    """The model on pair(W, H, D, seed) at the default parameters: computed once, shared by the tests that need it, read-only."""
    ref = Z.sgm(*pair(W, H, D, seed), dmin, D, census=census)
    for k in ("C", "S", "disp"):
        ref[k].setflags(write=False)
    return ref


def run(psm, name, l, r, D, census=(9, 7), dmin=0, **kw):
    """D disparities from dmin on through the range (a context's own max_disp is at most 256 and at most the width)"""
    with psm.DispEst(l, r, min(D, 256, l.shape[1])) as de:
        disp = de.SGBM_GPU(census=census, min_disparity=dmin, num_disparities=D, **kw)
        compare(name, de, Z.sgm(l, r, dmin, D, census=census, **kw), disp)


# the seams of the cost kernel's 32-pixel tile, 1, 2 and 4 disparities per lane downstream, W = D; then the seams of the census
# kernel's own tile in both axes (its columns coincide with the cost kernel's), two and three tiles with a remainder.  9 x 7 on the
# 8 x 8 image: the taps clamp past both edges at once
@pytest.mark.parametrize("W,H,D", [
    (8, 8, 8), (9, 40, 2), (33, 21, 33), (67, 45, 16), (131, 70, 33), (140, 33, 129), (150, 37, 130),
    (COST_TILE_W - 1, 9, 8), (COST_TILE_W, 9, 8), (COST_TILE_W + 1, 9, 8), (2 * COST_TILE_W + 1, 8, 12),
    (CENSUS_TILE_W - 1, CENSUS_TILE_H, 6), (CENSUS_TILE_W, CENSUS_TILE_H + 1, 6), (CENSUS_TILE_W + 1, 2 * CENSUS_TILE_H - 1, 6),
    (16, 2 * CENSUS_TILE_H, 6), (12, 2 * CENSUS_TILE_H + 1, 5), (3 * CENSUS_TILE_W + 2, 3 * CENSUS_TILE_H + 2, 9)])
def test_small_pairs_equal_the_model(psm, W, H, D):
    l, r = pair(W, H, D, W)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(census=(9, 7))
        compare(f"{W}x{H}x{D}", de, model(W, H, D, W), disp)


@pytest.mark.parametrize("win", [(3, 3), (5, 5), (7, 5), (7, 7), (9, 3), (9, 7)])
def test_each_window(psm, win):
    W, H, D = 67, 45, 16
    l, r = pair(W, H, D, W)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(census=win)
        compare(f"window {win[0]}x{win[1]}", de, model(W, H, D, W, win), disp)
        assert int(max(de.sgm_census(0).max(), de.sgm_census(1).max())) < 1 << (win[0] * win[1] - 1)      # the bits above are 0


@pytest.mark.parametrize("bs", [1, 3, 5, 7])
def test_each_block_size(psm, bs):
    W, H, D = 93, 41, 24
    l, r = pair(W, H, D, bs)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(block_size=bs, census=(9, 7))
        compare(f"bs {bs}", de, Z.sgm(l, r, 0, D, census=(9, 7), block_size=bs), disp)
        if bs == 1:                                        # the pixel cost itself
            assert np.array_equal(de.sgm_costs()[0], Z.pixel_cost(l, r, 0, D, 9, 7))


def test_block_and_window_past_both_edges_at_once(psm):
    l, r = pair(8, 8, 8, 9)
    run(psm, "8x8x8 bs 7", l, r, 8, block_size=7)


# the lanes at or beyond D, up to Dp, store 0; 64 and 256 are the ALL form downstream
@pytest.mark.parametrize("D", [61, 62, 63, 64, 253, 254, 255, 256])
def test_padding_lanes(psm, D):
    W, H = 40, 9
    l, r = pair(W, H, 16, D)
    run(psm, f"D {D}", l, r, D)


# above 256 disparities: two passes with one real lane in the second, two passes, four; a negative minimum reaches past the right
# edge, -300 puts whole passes there
@pytest.mark.parametrize("dmin", [0, -7, -300])
@pytest.mark.parametrize("D", [PASS_D + 1, 300, 4 * PASS_D])
def test_wide_ranges(psm, D, dmin):
    W, H = 48, 9
    l, r = pair(W, H, 16, 3)
    run(psm, f"D {D} min {dmin}", l, r, D, dmin=dmin)


@pytest.mark.parametrize("D,dmin", [(4 * PASS_D, -7), (2 * PASS_D + 3, 0)])
def test_wide_range_with_the_largest_block(psm, D, dmin):
    """block_size 7 over several passes: the kernel's largest LDS use."""
    W, H = 48, 9
    l, r = pair(W, H, 16, 5)
    run(psm, f"D {D} min {dmin} bs 7", l, r, D, dmin=dmin, block_size=7)


def adversarial(kind, W, H):
    rng = np.random.default_rng(len(kind))
    if kind == "two levels":
        l, r = (rng.integers(0, 2, (H, W, 3)) * 3 + 100).astype(np.uint8), (rng.integers(0, 2, (H, W, 3)) * 3 + 100).astype(np.uint8)
    elif kind == "checkerboard":
        y, x = np.mgrid[:H, :W]
        l = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
        r = np.roll(l, -3, axis=1)
    elif kind == "constant":
        l, r = np.full((H, W, 3), 77, np.uint8), np.full((H, W, 3), 200, np.uint8)
    elif kind == "impulse":
        l, r = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
        l[H // 2, W // 2] = 255
    else:
        l, r = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8), (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return np.ascontiguousarray(l), np.ascontiguousarray(r)


@pytest.mark.parametrize("kind", ["two levels", "checkerboard", "constant", "impulse", "0/255 noise"])
def test_adversarial_inputs(psm, kind):
    W, H, D = 70, 30, 20
    l, r = adversarial(kind, W, H)
    kw = dict(block_size=7, P1=100, P2=65535 - 49 * 3 * 255) if kind == "0/255 noise" else {}
    ref = Z.sgm(l, r, 0, D, census=(9, 7), **kw)
    if kind == "constant":                                 # every C is 0, every winner index 0
        assert not ref["C"].any() and not ref["best"].any()
    if kind == "impulse":                                  # the pixel cost reaches win_w win_h - 1
        assert int(Z.pixel_cost(l, r, 0, D, 9, 7).max()) == 62
    print(f"[sgm-census] {kind}: max C {int(ref['C'].max())}  max L_r {ref['max_l']}")
    with psm.DispEst(l, r, D) as de:
        compare(kind, de, ref, de.SGBM_GPU(census=(9, 7), **kw))
    if kind == "impulse":
        with psm.DispEst(l, r, D) as de:
            disp = de.SGBM_GPU(census=(9, 7), block_size=1)
            compare("impulse bs 1", de, Z.sgm(l, r, 0, D, census=(9, 7), block_size=1), disp)
            assert int(de.sgm_costs()[0].max()) == 62


@pytest.mark.parametrize("W,H,D", [(67, 45, 16), (131, 70, 33)])
def test_one_channel_pair(psm, W, H, D):
    l, r = pair(W, H, D, 5)
    gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(gray=(gl, gr), census=(9, 7))
        compare(f"gray {W}x{H}x{D}", de, Z.sgm(gl, gr, 0, D, census=(9, 7)), disp)
        # the staged colour pair is still there, and still the one the next call uses
        compare("colour after gray", de, model(W, H, D, 5), de.SGBM_GPU(census=(9, 7)))


def test_float_upload_gives_the_8_bit_result(psm):
    W, H, D = 131, 70, 33
    l, r = pair(W, H, D, 5)
    lf, rf = (a.astype(np.float32) * np.float32(1 / 255.0) for a in (l, r))
    with psm.DispEst(l, r, D) as de:
        d8 = de.SGBM_GPU(census=(9, 7))
        de.setInputImages(lf, rf)
        df = de.SGBM_GPU(census=(9, 7))
        compare("float upload", de, model(W, H, D, 5), df)
    assert np.array_equal(d8, df)


def test_async_matches_sync(psm):
    W, H, D = 120, 50, 40
    l, r = pair(W, H, D, 4)
    with psm.DispEst(l, r, D) as de:
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        de._ck(de._lib.psm_sgm_set_census(de._h, 9, 7), "psm_sgm_set_census")
        for _ in range(3):                                 # queued behind each other, no host synchronisation in between
            de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
        compare("async", de, model(W, H, D, 4), de.sgm_disparity())
        t = de.sgm_times()
        print(f"[sgm-census] times ms: cost {t[0]:.3f} paths {t[1]:.3f} select {t[2]:.3f}")
        assert len(t) == 3 and all(v > 0 for v in t)


@pytest.mark.parametrize("mode", ["sgbm", "hh", "3way", "hh4"])
def test_every_mode_with_the_speckle_filter_and_without_the_consistency_test(psm, mode):
    W, H, D = 160, 90, 32
    l, r = pair(W, H, D, 12)
    ref = Z.sgm(l, r, 0, D, census=(9, 7), mode=mode)
    off = Z.sgm(l, r, 0, D, census=(9, 7), mode=mode, disp12_max_diff=-1)
    with psm.DispEst(l, r, D) as de:
        compare(f"mode {mode}", de, ref, de.SGBM_GPU(census=(9, 7), mode=mode))
        compare(f"mode {mode}, no consistency test", de, off, de.SGBM_GPU(census=(9, 7), mode=mode, disp12_max_diff=-1))
        disp = de.SGBM_GPU(census=(9, 7), mode=mode, speckle_window_size=100, speckle_range=32)
        want, _ = K.sgbm_speckle(ref["disp"], 100, 32)
        print(f"[sgm-census] mode {mode}, speckle on top: {int(np.count_nonzero(want != ref['disp']))} pixels removed, "
              f"{int(np.count_nonzero(disp != want))} differing")
        assert np.array_equal(disp, want)
        Cd, Sd = de.sgm_costs()
        assert np.array_equal(Cd, ref["C"]) and np.array_equal(Sd, ref["S"])
    if mode == "hh":
        assert not np.array_equal(want, ref["disp"]) and not np.array_equal(off["disp"], ref["disp"])


def test_the_setting_persists_and_0_0_is_the_sad_stage(psm):
    capi = psm.capi
    W, H, D = 90, 44, 20
    l, r = pair(W, H, D, 8)
    kw = dict(block_size=3, uniqueness_ratio=5, disp12_max_diff=2)
    with psm.DispEst(l, r, D) as de:
        lib, h = de._lib, de._h
        with pytest.raises(capi.PsmError):                 # no compute at all
            de.sgm_census(1)
        assert "psm_sgm_download_census" in capi.last_error(h)
        assert lib.psm_sgm_set_census(h, 7, 5) == 0
        for setter in ((lib.psm_sgm_set_params, (3, 0, 0, 5, 2)), (lib.psm_sgm_set_speckle, (0, 0)), (lib.psm_sgm_set_mode, (1,)),
                       (lib.psm_sgm_set_range, (0, 0)), (lib.psm_sgm_set_prefilter, (0,))):
            assert setter[0](h, *setter[1]) == 0
        for i in range(2):                                 # ... across computes too
            assert lib.psm_sgm_compute(h) == 0
            compare(f"after the other setters, compute {i}", de, Z.sgm(l, r, 0, D, census=(7, 5), **kw), de.sgm_disparity())
        for bad in ((4, 5), (9, 9), (0, 3)):
            assert lib.psm_sgm_set_census(h, *bad) != 0 and "psm_sgm_set_census" in capi.last_error(h)
        assert lib.psm_sgm_compute(h) == 0                 # a refused window changes nothing
        compare("after the refusals", de, Z.sgm(l, r, 0, D, census=(7, 5), **kw), de.sgm_disparity())
        assert lib.psm_sgm_set_census(h, 0, 0) == 0
        assert lib.psm_sgm_compute(h) == 0
        compare_other("(0, 0) afterwards", de, R.sgm(l, r, 0, D, **kw), de.sgm_disparity())
        with pytest.raises(capi.PsmError):                 # the last compute ran another cost
            de.sgm_census(0)
        assert "psm_sgm_download_census" in capi.last_error(h)


def test_a_window_together_with_a_cap_is_refused(psm):
    capi = psm.capi
    W, H, D = 90, 44, 20
    l, r = pair(W, H, D, 8)
    gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
    with psm.DispEst(l, r, D) as de:
        before = de.SGBM_GPU(census=(9, 7))
        for kw in ({}, dict(gray=(gl, gr))):
            with pytest.raises(capi.PsmError):
                de.SGBM_GPU(census=(9, 7), pre_filter_cap=63, **kw)
            msg = capi.last_error(de._h)
            assert "psm_sgm_set_census" in msg and "psm_sgm_set_prefilter" in msg and "9 x 7" in msg and "63" in msg
            compare("the previous result after the refusal", de, model(W, H, D, 8), de.sgm_disparity())
        assert np.array_equal(before, de.sgm_disparity())
        # the setters did not care about the order: (0, 0) with the cap still 63 is the Birchfield-Tomasi stage
        assert de._lib.psm_sgm_set_census(de._h, 0, 0) == 0
        assert de._lib.psm_sgm_compute(de._h) == 0
        compare_other("cap 63 after set_census(0, 0)", de, B.sgm(l, r, D, pre_filter_cap=63), de.sgm_disparity())


def test_release_scratch_then_recompute(psm):
    W, H, D = 90, 44, 20
    l, r = pair(W, H, D, 8)
    with psm.DispEst(l, r, D) as de:
        compare("before", de, model(W, H, D, 8), de.SGBM_GPU(census=(9, 7)))
        de.release_scratch()
        with pytest.raises(psm.capi.PsmError):
            de.sgm_census(0)                               # the codes went with the buffers
        compare("after release", de, model(W, H, D, 8), de.SGBM_GPU(census=(9, 7)))


def test_a_batch_equals_the_single_calls_and_the_model(psm):
    from primestereomatch_amd import dispest
    W, H, D = 67, 45, 16
    des = [psm.DispEst(*pair(W, H, D, s), D) for s in (67, 1, 2)]
    try:
        maps = dispest.sgbm_batch(des, census=(9, 7))
        for s, de, disp in zip((67, 1, 2), des, maps):
            compare(f"batch of 3, seed {s}", de, model(W, H, D, s), disp)
        kept = [(de.sgm_costs(), de.sgm_census(0), de.sgm_census(1)) for de in des]
        for s, de, disp, k in zip((67, 1, 2), des, maps, kept):      # a single compute on a context of the batch: the same bits
            single = de.SGBM_GPU(census=(9, 7))
            compare(f"single after the batch, seed {s}", de, model(W, H, D, s), single)
            assert np.array_equal(single, disp) and np.array_equal(de.sgm_costs()[1], k[0][1])
            assert np.array_equal(de.sgm_census(0), k[1]) and np.array_equal(de.sgm_census(1), k[2])
        maps = dispest.sgbm_batch(des, census=(5, 5), block_size=3)      # ... and a batch after the singles, another window
        for s, de, disp in zip((67, 1, 2), des, maps):
            compare(f"second batch, seed {s}", de, Z.sgm(*pair(W, H, D, s), 0, D, census=(5, 5), block_size=3), disp)
    finally:
        for d in des:
            d.close()


def test_batches_refuse_differing_windows_and_a_cap_beside_a_window(psm):
    from primestereomatch_amd import dispest
    capi = psm.capi
    W, H, D = 67, 45, 16
    des = [psm.DispEst(*pair(W, H, D, s), D) for s in (67, 1, 2)]
    try:
        maps = dispest.sgbm_batch(des, census=(9, 7))
        assert des[2]._lib.psm_sgm_set_census(des[2]._h, 7, 7) == 0
        with pytest.raises(capi.PsmError):
            dispest.sgm_compute_batch(des)
        msg = capi.last_error(des[0]._h)
        assert "context 2" in msg and "census" in msg and "7 x 7" in msg and "9 x 7" in msg
        assert des[2]._lib.psm_sgm_set_census(des[2]._h, 9, 7) == 0
        assert des[1]._lib.psm_sgm_set_prefilter(des[1]._h, 63) == 0
        with pytest.raises(capi.PsmError):
            dispest.sgm_compute_batch(des)
        msg = capi.last_error(des[0]._h)
        assert "context 1" in msg and "psm_sgm_set_census" in msg and "psm_sgm_set_prefilter" in msg
        for s, de, disp in zip((67, 1, 2), des, maps):     # nothing was enqueued: every previous result is still readable
            compare(f"after the refusals, seed {s}", de, model(W, H, D, s), de.sgm_disparity())
            assert np.array_equal(de.sgm_disparity(), disp)
    finally:
        for d in des:
            d.close()


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_goldens(psm, golden, name):
    p, g = golden(f"{name}_pair.npz"), golden(f"{name}_sgm_census.npz")
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        disp = de.SGBM_GPU(census=(9, 7))
        Cd, Sd = de.sgm_costs()
        tl, tr = de.sgm_census(0), de.sgm_census(1)
    print(f"[sgm-census] {name}: differing map elements {int(np.count_nonzero(disp != g['disp']))}")
    assert sha(tl) == str(g["sha_codes_l"]) and sha(tr) == str(g["sha_codes_r"])
    assert sha(Cd) == str(g["sha_C"]) and sha(Sd) == str(g["sha_S"])
    assert np.array_equal(disp, g["disp"])
    assert np.array_equal(disp >= 0, g["valid"].astype(bool))


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_harness_forwards_the_window(psm, golden, name):
    from primestereomatch_amd import harness
    p, g = golden(f"{name}_pair.npz"), golden(f"{name}_sgm_census.npz")
    out = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], p["occl"], 4, census=(9, 7))
    assert np.array_equal(out["disp16"], g["disp"])
    best = harness.error_vs_ground_truth(g["best"], p["gt_l"], p["occl"], 64, 4)[0]
    print(f"[sgm-census] {name}: bp_percent_int {out['bp_percent_int']:.2f}, %BP of best {best:.2f}, cost {out['cost_ms']:.3f} ms")
    assert out["bp_percent_int"] == harness.error_vs_ground_truth(np.maximum(g["disp"], 0) >> 4, p["gt_l"], p["occl"], 64, 4)[0]
    if name == "cones":
        both = harness.compute_sgbm_batch([(p["l_bgr"], p["r_bgr"])] * 2, 64, census=(9, 7))
        assert all(np.array_equal(o["disp16"], g["disp"]) for o in both)


def test_cpp_demo_sgbm_census(psm, golden, tmp_path):
    """psm_demo's sgbm_census word: the C++ mirror with setSGBMCensus(9, 7) on Cones dumps the map the Python side gives."""
    import os
    import subprocess
    from conftest import ROOT
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    if not os.path.exists(demo):
        subprocess.run(["make", "-C", os.path.join(ROOT, "primestereomatch_amd", "host")], check=True)
    p, g = golden("cones_pair.npz"), golden("cones_sgm_census.npz")
    H, W, _ = p["l_bgr"].shape
    p["l_bgr"].tofile(tmp_path / "l.raw")
    p["r_bgr"].tofile(tmp_path / "r.raw")
    env = dict(os.environ, PRIMESM_HIP_LIB=psm.capi.LIB_PATH)
    q = subprocess.run([demo, str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(W), str(H), "64", str(tmp_path / "o"),
                        "1", "f32", "0", "0", "0", "0", "2", "0", "sgbm_census"], env=env, capture_output=True, text=True, timeout=300)
    assert q.returncode == 0, q.stderr
    assert "STEREO SGBM Times" in q.stdout and "Speckle Time" not in q.stdout and "equal the single run's" in q.stdout
    d = np.fromfile(tmp_path / "o_sgbm16.raw", np.int16).reshape(H, W)
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        assert np.array_equal(d, de.SGBM_GPU(census=(9, 7)))
    assert np.array_equal(d, g["disp"])
