"""-m gpu: the 8-bit maps of both views from the SGM stage (psm_sgm_select_maps, DispEst.SGBMSelect_GPU, dispest.sgbm_select_batch)
against the definition, tests/sgm_maps_model.py, applied to THE DEVICE'S OWN S (sgm_costs(), which the other SGM tests pin to the
SGM models): that isolates the new kernel and keeps the numpy SGM out of this file.  Everything is integer: np.array_equal, there
is no tolerance anywhere.  Behind the maps the post-processing chain and the score stage run as behind DispSelect_GPU; the chain's
reference is the oracle's on the same maps."""
import ctypes as C
import functools

import numpy as np
import pytest

import score_model as SC
import sgm_maps_chain as K
import sgm_maps_model as MM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@functools.lru_cache(maxsize=None)
def noise_pair(W, H, seed, ch=3, dtype="u8"):
    shape = (2, H, W, 3) if ch == 3 else (2, H, W)
    l, r = np.random.default_rng([seed, W, H]).integers(0, 256, shape, dtype=np.uint8)
    if dtype == "f32":
        l, r = l.astype(np.float32) * np.float32(1 / 255.0), r.astype(np.float32) * np.float32(1 / 255.0)
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


def constant_pair(W, H):
    img = np.full((H, W, 3), 93, np.uint8)
    return img, img.copy()


def want_maps(de, dmin=0):
    """the model on the device's own S of the last compute"""
    return MM.maps(de.sgm_costs()[1], dmin, de.maxDis)


def check(name, de, dmin=0):
    wl, wr = want_maps(de, dmin)
    gl, gr = (m.copy() for m in de.SGBMSelect_GPU())
    n = [int(np.count_nonzero(a != b)) for a, b in ((gl, wl), (gr, wr))]
    print(f"[sgm-maps] {name}: differing elements left {n[0]}  right {n[1]}")
    assert gl.dtype == gr.dtype == np.uint8
    assert np.array_equal(gl, wl), (name, n, np.argwhere(gl != wl)[:8].tolist())
    assert np.array_equal(gr, wr), (name, n, np.argwhere(gr != wr)[:8].tolist())
    dl, dr = de.download_maps()                                    # ... and they are the context's current maps
    assert np.array_equal(dl, wl) and np.array_equal(dr, wr)
    return gl, gr


# ------------------------------------------------------------------------------------------------------------------ shapes

# W = D; a range with columns that have no candidate; padding elements of Dp (61, 62, 63 -> 64); every NV with a row one past
# four waves' worth of pixels; NV 2.
# What the library admits bounds the shapes: a context has 8 rows at least and max_disp <= width (psm_create), and the call needs
# dmin + D <= max_disp - so the heights are 8 where fewer rows would do (a row is a workgroup of its own), and W < D, which the
# definition covers (tests/test_sgm_maps_model.py), cannot reach the device: the narrowest image for 64 disparities has 64
# columns, where every right pixel but the first has fewer than D candidates; test_w_below_d_cannot_be_asked shows the refusal.
SHAPES = [(64, 8, 64, 0, 0), (33, 9, 7, 3, 4), (70, 8, 61, 0, 0), (70, 8, 62, 0, 0), (70, 8, 63, 0, 0), (257, 8, 256, 0, 0),
          (130, 8, 128, 0, 0)]


@pytest.mark.parametrize("W,H,maxdis,dmin,nd", SHAPES)
def test_shapes(psm, W, H, maxdis, dmin, nd):
    l, r = noise_pair(W, H, maxdis)
    with psm.DispEst(l, r, maxdis) as de:
        de.SGBM_GPU(min_disparity=dmin, num_disparities=nd)
        _, gr = check(f"{W}x{H}x{nd or maxdis} min {dmin}", de, dmin)
        if dmin:
            assert np.all(gr[:, W - dmin:] == 0)


def test_w_below_d_cannot_be_asked(psm):
    W, H = 20, 8
    l, r = noise_pair(W, H, 64)
    with pytest.raises(psm.capi.PsmError, match="max_disp 64 > width 20"):
        psm.DispEst(l, r, 64)
    with psm.DispEst(l, r, 16) as de:
        de.SGBM_GPU(num_disparities=64)                                          # the stage itself takes D > W
        with pytest.raises(psm.capi.PsmError, match="psm_sgm_select_maps: the result's range"):
            de.SGBMSelect_GPU()


@pytest.fixture(scope="module")
def middlebury(psm, golden, oracle):
    """Cones and Teddy through the stage once: the pair, the device's S, the model's maps of it and the oracle's chain on them -
    computed once, shared, left unchanged"""
    out = {}
    for name in ("cones", "teddy"):
        p = golden(f"{name}_pair.npz")
        with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
            de.SGBM_GPU()
            lm, rm = want_maps(de)
        ref = {"pair": p, "lmap": lm, "rmap": rm, "chain": K.chain(oracle, p["l_bgr"], lm, rm, 64)}
        for a in (lm, rm, *(v for v in ref["chain"].values())):
            a.setflags(write=False)
        out[name] = ref
    return out


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_middlebury(psm, golden, oracle, middlebury, name):
    ref = middlebury[name]
    p = ref["pair"]
    assert np.array_equal(ref["lmap"], golden(f"{name}_sgm.npz")["best"])        # the model's S, too
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        de.SGBM_GPU()
        gl, gr = de.SGBMSelect_GPU()
        assert np.array_equal(gl, ref["lmap"]) and np.array_equal(gr, ref["rmap"])
    got = tuple(K.bad_pixels(oracle, m, p["gt_l"], p["occl"], 64) for m in (ref["lmap"], ref["chain"]["lfill"], ref["chain"]["lmed"]))
    print(f"[sgm-maps] {name}: bad pixels WTA / + lrCheck + fillInv / + wgtMedian {got}")
    assert got == K.SAD_COUNTS[name]


def test_channels_and_depths(psm):
    W, H, D = 70, 8, 62
    l, r = noise_pair(W, H, 1)
    lf, rf = noise_pair(W, H, 1, dtype="f32")
    gl, gr = noise_pair(W, H, 2, ch=1)
    with psm.DispEst(l, r, D) as de:
        de.SGBM_GPU()
        a = check("3 channels u8", de)
        de.SGBM_GPU(gray=(gl, gr))
        g = check("1 channel u8", de)
        assert not np.array_equal(a[0], g[0])
    with psm.DispEst(lf, rf, D) as de:
        de.SGBM_GPU()
        f = check("3 channels f32", de)
        assert np.array_equal(f[0], a[0]) and np.array_equal(f[1], a[1])         # (quantised on the device to the same bytes)


COSTS = ({}, {"pre_filter_cap": 63}, {"census": (9, 7)})


def test_every_cost_and_mode(psm):
    W, H, D = 70, 8, 62
    l, r = noise_pair(W, H, 3)
    with psm.DispEst(l, r, D) as de:
        for cost in COSTS:
            for mode in ("sgbm", "hh", "3way", "hh4"):
                de.SGBM_GPU(mode=mode, **cost)
                check(f"{cost or 'SAD'} {mode}", de)


# ------------------------------------------------------------------------------------------------------------ exact ties of S

def test_constant_pair_gives_zero_maps(psm):
    W, H, D = 45, 8, 16
    with psm.DispEst(*constant_pair(W, H), D) as de:
        de.SGBM_GPU()
        assert not de.sgm_costs()[1].any()
        gl, gr = check("constant", de)
        assert not gl.any() and not gr.any()


def test_ties_along_a_diagonal_take_the_lowest_disparity(psm):
    """A black left image and a right image of black and white columns, block size 1: a pixel cost depends on x - k alone, the column
    of the right image - S repeats along the diagonals the right view searches.  The lowest k must win there while a higher k of the
    same tie wins in the left view."""
    W, H, D = 40, 8, 16
    l = np.zeros((H, W, 3), np.uint8)
    cols = (np.random.default_rng(1).integers(0, 2, (1, W, 1)) * 255).astype(np.uint8)
    r = np.ascontiguousarray(np.repeat(np.tile(cols, (H, 1, 1)), 3, axis=2))
    with psm.DispEst(l, r, D) as de:
        de.SGBM_GPU(block_size=1)
        S = de.sgm_costs()[1].astype(np.int64)
        gl, gr = check("diagonal ties", de)
    tied = split = 0
    for y in range(H):
        for xr in range(W):
            cand = [(S[y, xr + k, k], k) for k in range(D) if xr + k < W]
            ks = [k for s, k in cand if s == min(cand)[0]]
            tied += len(ks) > 1
            assert gr[y, xr] == ks[0]
            split += any(gl[y, xr + k] == k for k in ks[1:])
    print(f"[sgm-maps] right pixels with a tied minimum {tied}, of them with a higher k of the tie winning on the left {split}")
    assert tied >= 50 and split >= 5


# ------------------------------------------------------------------------------------------------------------------- ranges

def test_the_range_is_the_results_not_the_settings(psm):
    W, H, D = 90, 8, 64
    l, r = noise_pair(W, H, 5)
    with psm.DispEst(l, r, D) as de:
        de.SGBM_GPU(min_disparity=5, num_disparities=40)
        gl, gr = check("range (5, 40)", de, 5)
        assert np.all(gr[:, -5:] == 0) and gl.min() >= 5 and gl.max() < 45
        de._ck(de._lib.psm_sgm_set_range(de._h, 0, 0), "set_range")             # no compute follows
        again = de.SGBMSelect_GPU()
        assert np.array_equal(again[0], gl) and np.array_equal(again[1], gr)


@pytest.mark.parametrize("dmin,nd", [(-1, 16), (40, 40)])
def test_ranges_outside_the_maps_are_refused(psm, dmin, nd):
    W, H, D = 70, 8, 64
    l, r = noise_pair(W, H, 6)
    with psm.DispEst(l, r, D) as de:
        de.SGBM_GPU()
        before = [m.copy() for m in de.SGBMSelect_GPU()]
        de.SGBM_GPU(min_disparity=dmin, num_disparities=nd)
        with pytest.raises(psm.capi.PsmError) as e:
            de.SGBMSelect_GPU()
        msg = str(e.value)
        assert "psm_sgm_select_maps" in msg and str(dmin) in msg and str(nd) in msg and "64" in msg
        dl, dr = de.download_maps()                                              # the previous maps are still current
        assert np.array_equal(dl, before[0]) and np.array_equal(dr, before[1])
        de.LRCheck_GPU()


# -------------------------------------------------------------------------------------------------------------------- state

def test_refused_without_a_result(psm):
    W, H, D = 40, 8, 16
    l, r = noise_pair(W, H, 7)
    with psm.DispEst(l, r, D) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_sgm_select_maps: no SGM result"):
            de.SGBMSelect_GPU()
        de.SGBM_GPU()
        check("before the release", de)
        de.release_scratch()
        with pytest.raises(psm.capi.PsmError, match="psm_sgm_select_maps: no SGM result"):
            de.SGBMSelect_GPU()
        de.SGBM_GPU()
        check("after the release", de)
        # a stride shorter than a row
        assert de._lib.psm_sgm_select_maps(de._h, de.lDisMap.ctypes.data_as(C.c_void_p), None, W - 1) != 0
        assert "stride" in psm.capi.last_error(de._h) and str(W - 1) in psm.capi.last_error(de._h)


def test_shards_and_stripes_are_refused(psm):
    W, H, D = 40, 12, 16
    l, r = noise_pair(W, H, 8)
    with psm.DispEst(l, r, D, d_range=(0, 8)) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_sgm_select_maps: a disparity shard"):
            de.SGBMSelect_GPU()
    with psm.DispEst(l, r, D) as de:
        de.SGBM_GPU()
        de.set_rows(4, 8)
        with pytest.raises(psm.capi.PsmError, match="psm_sgm_select_maps: a row stripe"):
            de.SGBMSelect_GPU()
        de.set_rows(0, 0)
        check("stripe lifted", de)


def test_the_stage_keeps_its_results(psm):
    W, H, D = 64, 24, 32
    l, r = noise_pair(W, H, 9)
    with psm.DispEst(l, r, D) as de:
        d16 = de.SGBM_GPU(speckle_window_size=20, speckle_range=2)
        Cv, Sv = de.sgm_costs()
        sizes = de.sgm_speckle_sizes()
        check("with the speckle filter", de)
        assert np.array_equal(de.sgm_disparity(), d16)
        C2, S2 = de.sgm_costs()
        assert np.array_equal(C2, Cv) and np.array_equal(S2, Sv) and np.array_equal(de.sgm_speckle_sizes(), sizes)


def test_the_chain_runs_behind_the_maps(psm, oracle, middlebury):
    ref = middlebury["cones"]
    p, c = ref["pair"], ref["chain"]
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        de.SGBM_GPU()
        de.SGBMSelect_GPU()
        with pytest.raises(psm.capi.PsmError, match="psm_fill_invalid"):        # no mask of these maps yet
            de.FillInv_GPU()
        de.LRCheck_GPU()
        assert np.array_equal(de.lValid, c["lvalid"]) and np.array_equal(de.rValid, c["rvalid"])
        de.FillInv_GPU()
        assert np.array_equal(de.lDisMap, c["lfill"]) and np.array_equal(de.rDisMap, c["rfill"])
        de.WgtMedian_GPU()
        assert np.array_equal(de.lDisMap, c["lmed"])
        rmed = oracle.wgt_median(oracle.u8_to_f32(np.ascontiguousarray(p["r_bgr"])), c["rfill"], c["rvalid"], 64, right=True)
        assert np.array_equal(de.rDisMap, rmed)


def test_score_reads_the_maps(psm, middlebury):
    ref = middlebury["cones"]
    p = ref["pair"]
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        de.SGBM_GPU()
        de.SGBMSelect_GPU(download=False)
        de.set_truth(p["gt_l"], p["occl"])
        rec = de.Score_GPU(SC.GIF)
        m = SC.score(SC.GIF, (ref["lmap"], ref["rmap"]), p["gt_l"], p["occl"], 64)
        for k in SC.RECORD_KEYS:
            assert rec[k] == m[k], (k, rec[k], m[k])
        assert rec["bad"] == K.SAD_COUNTS["cones"][0]
        ld, rd, em = de.score_maps(right=True)
        assert np.array_equal(ld, m["ldisp"]) and np.array_equal(rd, m["rdisp"]) and np.array_equal(em, m["emap"])


def test_the_guided_filter_path_is_untouched(psm, golden, middlebury):
    ref = middlebury["cones"]
    p, gold = ref["pair"], golden("cones_oracle_d64.npz")
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        de.SGBM_GPU()
        # in the middle of the guided-filter sequence: the filtered result is pending, the maps are the SGM stage's
        de.CostConst_GPU(); de.CostFilter_GPU()
        gl, gr = de.SGBMSelect_GPU()
        assert np.array_equal(gl, ref["lmap"]) and np.array_equal(gr, ref["rmap"])
        de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, gold["ldisp"]) and np.array_equal(de.rDisMap, gold["rdisp"])
        # ... and behind a guided-filter select the call replaces the maps
        gl, gr = de.SGBMSelect_GPU()
        assert np.array_equal(gl, ref["lmap"]) and np.array_equal(gr, ref["rmap"])
        dl, dr = de.download_maps()
        assert np.array_equal(dl, ref["lmap"]) and np.array_equal(dr, ref["rmap"])
        # the whole sequence afterwards: the golden maps again
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, gold["ldisp"]) and np.array_equal(de.rDisMap, gold["rdisp"])


def test_the_launch_is_timed_under_profile(psm):
    W, H, D = 70, 8, 62
    l, r = noise_pair(W, H, 3)
    with psm.DispEst(l, r, D) as de:
        de.SGBM_GPU()
        de.SGBMSelect_GPU()
        with pytest.raises(psm.capi.PsmError, match="psm_sgm_maps_time"):
            de.sgm_maps_time()
        de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        de.SGBM_GPU()
        de.SGBMSelect_GPU()
        assert de.sgm_maps_time() > 0.0


# -------------------------------------------------------------------------------------------------------------------- batch

def test_batch_equals_the_single_calls(psm):
    from primestereomatch_amd import dispest
    W, H, D = 70, 9, 62
    pairs = [noise_pair(W, H, 11), constant_pair(W, H), noise_pair(W, H, 12)]
    singles = []
    for l, r in pairs:
        with psm.DispEst(l, r, D) as de:
            de.SGBM_GPU()
            singles.append([m.copy() for m in check("single", de)])
    des = [psm.DispEst(l, r, D) for l, r in pairs]
    try:
        dispest.sgbm_batch(des)
        dispest.sgbm_select_batch(des)
        for de, (wl, wr) in zip(des, singles):
            gl, gr = de.download_maps()
            assert np.array_equal(gl, wl) and np.array_equal(gr, wr)
        assert not singles[1][0].any() and not singles[1][1].any()
        de = des[2]
        de.LRCheck_GPU()                                                          # as behind the single call: maps, no mask before
        gl, gr = de.SGBMSelect_GPU()
        assert np.array_equal(gl, singles[2][0]) and np.array_equal(gr, singles[2][1])
        # mismatched ranges: the message names the index
        des[1].SGBM_GPU(min_disparity=2, num_disparities=40)
        with pytest.raises(psm.capi.PsmError) as e:
            dispest.sgbm_select_batch(des)
        assert "psm_sgm_select_maps_batch" in str(e.value) and "context 1" in str(e.value) and "40" in str(e.value)
        gl, gr = des[0].download_maps()                                           # nothing was enqueued
        assert np.array_equal(gl, singles[0][0]) and np.array_equal(gr, singles[0][1])
    finally:
        for de in des:
            de.close()


# ------------------------------------------------------------------------------------------------------------------ harness

def test_harness_post_process(psm, middlebury):
    from primestereomatch_amd import harness
    ref = middlebury["cones"]
    p = ref["pair"]
    plain = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], p["occl"])
    assert not any(k.endswith("_pp") for k in plain)
    want = 100.0 * K.SAD_COUNTS["cones"][2] / K.PIXELS
    for tail in (False, True):
        out = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], p["occl"], post_process=True, device_tail=tail)
        assert np.array_equal(out["lDisMap_pp"], ref["chain"]["lmed"])
        print(f"[sgm-maps] harness device_tail {tail}: bp_percent_pp {out['bp_percent_pp']:.4f} (int {out['bp_percent_int']:.4f})")
        assert out["bp_percent_pp"] == want
        assert out["bp_percent_int"] == plain["bp_percent_int"] and np.array_equal(out["disp16"], plain["disp16"])
    outs = harness.compute_sgbm_batch([(p["l_bgr"], p["r_bgr"])] * 2, 64, [p["gt_l"]] * 2, [p["occl"]] * 2, post_process=True)
    for out in outs:
        assert np.array_equal(out["lDisMap_pp"], ref["chain"]["lmed"]) and out["bp_percent_pp"] == want


# --------------------------------------------------------------------------------------------------------------- C++ mirror

def test_cpp_demo_sgbm_pp(psm, middlebury, tmp_path):
    """psm_demo's sgbm word with pp: DispEst::SGBMSelect, the chain and the score stage in the C++ mirror - the filtered left map it
    dumps is the oracle chain's, the figure it prints comes from the pinned count."""
    import os
    import subprocess
    from conftest import ROOT
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    ref = middlebury["cones"]
    p = ref["pair"]
    H, W, _ = p["l_bgr"].shape
    for key in ("l_bgr", "r_bgr", "gt_l", "occl"):
        p[key].tofile(tmp_path / f"{key}.raw")
    env = dict(os.environ, PRIMESM_HIP_LIB=psm.capi.LIB_PATH)
    q = subprocess.run([demo, str(tmp_path / "l_bgr.raw"), str(tmp_path / "r_bgr.raw"), str(W), str(H), "64", str(tmp_path / "o"),
                        "1", "f32", "0", "0", "0", "0", "0", "0", "sgbm", str(tmp_path / "gt_l.raw"), str(tmp_path / "occl.raw"), "pp"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert q.returncode == 0, q.stdout + q.stderr
    got = np.fromfile(tmp_path / "o_sgbm_pp_ldisp.raw", np.uint8).reshape(H, W)
    assert np.array_equal(got, ref["chain"]["lmed"])
    assert "SGBM post-processed (lrCheck, fillInv, wgtMedian): %%BP = %.2f%%" % (100.0 * K.SAD_COUNTS["cones"][2] / K.PIXELS) in q.stdout
