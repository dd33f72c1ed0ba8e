"""-m gpu: the SGM stage's prefiltered Birchfield-Tomasi cost on the device (psm_sgm_set_prefilter, DispEst.SGBM_GPU(pre_filter_cap=...))
against its definition, the numpy model tests/sgm_bt_model.py.  Everything is integer: the prefiltered planes, the block costs C,
the summed path costs S and the final int16 map must equal the model with 0 differing elements - there is no tolerance anywhere
in this file."""
import hashlib

import numpy as np
import pytest

import sgm_bt_model as B
import sgm_model as M
import speckle_model as K

pytestmark = pytest.mark.gpu

TILE_W = 128        # SGM_BT_TX: the columns a workgroup of k_sgm_bt_rows owns
SEGMENT_H = 32      # SGM_BT_YS: the rows a thread of k_sgm_bt_cols marches down


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
    """The planes, C, S and the map of the last SGBM_GPU of `de` against a model result; prints the counts, asserts 0."""
    Cd, Sd = de.sgm_costs()
    pl, pr = de.sgm_prefiltered(0), de.sgm_prefiltered(1)
    assert pl.shape == ref["planes"][0].shape and pl.dtype == np.uint8
    n = [int(np.count_nonzero(a != b)) for a, b in ((pl, ref["planes"][0]), (pr, ref["planes"][1]), (Cd, ref["C"]), (Sd, ref["S"]),
                                                    (disp, ref["disp"]))]
    print(f"[sgm-bt] {name}: differing elements planes {n[0]} + {n[1]}  C {n[2]}  S {n[3]}  map {n[4]}  (valid {ref['valid'].mean():.3f})")
    assert disp.dtype == np.int16 and Cd.dtype == np.uint16 and Sd.dtype == np.uint32
    assert n == [0, 0, 0, 0, 0]


def compare_sad(name, de, ref, disp):
    Cd, Sd = de.sgm_costs()
    n = [int(np.count_nonzero(a != b)) for a, b in ((Cd, ref["C"]), (Sd, ref["S"]), (disp, ref["disp"]))]
    print(f"[sgm-bt] {name}: differing elements C {n[0]}  S {n[1]}  map {n[2]}")
    assert n == [0, 0, 0]


def pair(W, H, D, seed=0):
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=seed)
    return l, r


# the smallest context with W = D; 1, 2 and 4 disparities per lane downstream, D not a multiple of 4 / 64; widths at the seams of
# the column tiles, heights at the seams of the row segments, three tiles and three segments
@pytest.mark.parametrize("W,H,D", [
    (8, 8, 8), (9, 40, 2), (33, 21, 33), (67, 45, 16), (131, 70, 33), (140, 33, 129), (150, 37, 130),
    (TILE_W - 1, 9, 8), (TILE_W, 9, 8), (TILE_W + 1, 9, 8), (2 * TILE_W + 1, 8, 12),
    (16, SEGMENT_H - 1, 6), (16, SEGMENT_H, 6), (16, SEGMENT_H + 1, 6), (12, 2 * SEGMENT_H + 1, 5)])
def test_small_pairs_equal_the_model(psm, W, H, D):
    l, r = pair(W, H, D, seed=W)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(pre_filter_cap=63)
        compare(f"{W}x{H}x{D}", de, B.sgm(l, r, D, pre_filter_cap=63), disp)


@pytest.mark.parametrize("bs", [1, 3, 5, 7])
def test_each_block_size(psm, bs):
    W, H, D = 93, 41, 24
    l, r = pair(W, H, D, seed=bs)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(block_size=bs, pre_filter_cap=63)
        ref = B.sgm(l, r, D, pre_filter_cap=63, block_size=bs)
        compare(f"bs {bs}", de, ref, disp)
        if bs == 1:                                        # the pixel cost itself
            assert np.array_equal(de.sgm_costs()[0], B.pixel_cost_bt(l, r, D, 63))


def test_block_past_both_edges_at_once(psm):
    l, r = pair(8, 8, 8, seed=9)
    with psm.DispEst(l, r, 8) as de:
        disp = de.SGBM_GPU(block_size=7, pre_filter_cap=63)
        compare("8x8x8 bs 7", de, B.sgm(l, r, 8, pre_filter_cap=63, block_size=7), disp)


@pytest.mark.parametrize("cap", [1, 15, 16, 31, 63])
def test_each_cap(psm, cap):
    W, H, D = 77, 35, 20
    l, r = pair(W, H, D, seed=21)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(pre_filter_cap=cap)
        compare(f"cap {cap}", de, B.sgm(l, r, D, pre_filter_cap=cap), disp)


def test_caps_outside_the_range_are_refused(psm):
    capi = psm.capi
    l, r = pair(32, 16, 8)
    with psm.DispEst(l, r, 8) as de:
        for cap in (-1, 64):
            with pytest.raises(capi.PsmError):
                de.SGBM_GPU(pre_filter_cap=cap)
            assert "psm_sgm_set_prefilter" in capi.last_error(de._h)
        with pytest.raises(capi.PsmError, match="no result"):
            de.sgm_disparity()                             # nothing above launched anything
        compare_sad("after the refusals", de, M.sgm(l, r, 8), de.SGBM_GPU())       # ... and the setting is still 0


def test_binary_noise_with_the_largest_costs(psm):
    """0 / 255 noise: every Sobel value is clipped or near it, every intensity bound is 0, 127 or 255 - the largest pixel costs -
    with the largest block and the largest P2 the 16-bit condition admits."""
    W, H, D = 70, 30, 20
    rng = np.random.default_rng(17)
    l = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    r = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    kw = dict(block_size=7, P1=100, P2=65535 - 49 * 3 * 255)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(pre_filter_cap=63, **kw)
        ref = B.sgm(l, r, D, pre_filter_cap=63, **kw)
        print(f"[sgm-bt] noise: max C {int(ref['C'].max())}  max L_r {ref['max_l']}")
        compare("binary noise", de, ref, disp)


@pytest.mark.parametrize("W,H,D", [(67, 45, 16), (131, 70, 33)])
def test_one_channel_pair(psm, W, H, D):
    l, r = pair(W, H, D, seed=5)
    gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(gray=(gl, gr), pre_filter_cap=63)
        compare(f"gray {W}x{H}x{D}", de, B.sgm(gl, gr, D, pre_filter_cap=63), disp)
        # the staged colour pair is still there, and still the one the next call uses
        compare("colour after gray", de, B.sgm(l, r, D, pre_filter_cap=63), de.SGBM_GPU(pre_filter_cap=63))


def test_float_upload_gives_the_8_bit_result(psm):
    W, H, D = 131, 70, 33
    l, r = pair(W, H, D, seed=3)
    lf, rf = (a.astype(np.float32) * np.float32(1 / 255.0) for a in (l, r))      # src/StereoMatch.cpp:195-196
    with psm.DispEst(l, r, D) as de:
        d8 = de.SGBM_GPU(pre_filter_cap=63)
        de.setInputImages(lf, rf)
        df = de.SGBM_GPU(pre_filter_cap=63)
        compare("float upload", de, B.sgm(l, r, D, pre_filter_cap=63), df)
    assert np.array_equal(d8, df)


def test_the_setting_persists_and_cap_0_is_the_sad_stage(psm):
    capi = psm.capi
    W, H, D = 90, 44, 20
    l, r = pair(W, H, D, seed=8)
    with psm.DispEst(l, r, D) as de:
        lib, h = de._lib, de._h
        assert lib.psm_sgm_set_prefilter(h, 63) == 0
        assert lib.psm_sgm_set_params(h, 3, 0, 0, 5, 2) == 0
        assert lib.psm_sgm_set_speckle(h, 0, 0) == 0
        assert lib.psm_sgm_compute(h) == 0
        compare("after set_params and set_speckle", de, B.sgm(l, r, D, pre_filter_cap=63, block_size=3, uniqueness_ratio=5, disp12_max_diff=2),
                de.sgm_disparity())
        assert lib.psm_sgm_set_prefilter(h, 0) == 0
        assert lib.psm_sgm_compute(h) == 0
        compare_sad("cap 0 afterwards", de, M.sgm(l, r, D, block_size=3, uniqueness_ratio=5, disp12_max_diff=2), de.sgm_disparity())
        with pytest.raises(capi.PsmError):
            de.sgm_prefiltered(0)
        assert "psm_sgm_download_prefiltered" in capi.last_error(h)
    with psm.DispEst(l, r, D) as de:                       # no compute at all
        with pytest.raises(capi.PsmError):
            de.sgm_prefiltered(1)
        assert "psm_sgm_download_prefiltered" in capi.last_error(de._h)


def test_speckle_filter_on_top(psm):
    W, H, D = 160, 90, 32
    l, r = pair(W, H, D, seed=12)
    ref = B.sgm(l, r, D, pre_filter_cap=63)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(pre_filter_cap=63, speckle_window_size=100, speckle_range=32)
        want, _ = K.sgbm_speckle(ref["disp"], 100, 32)
        print(f"[sgm-bt] speckle on top: {int(np.count_nonzero(want != ref['disp']))} pixels removed, "
              f"{int(np.count_nonzero(disp != want))} differing")
        assert np.array_equal(disp, want) and not np.array_equal(want, ref["disp"])
        Cd, Sd = de.sgm_costs()
        assert np.array_equal(Cd, ref["C"]) and np.array_equal(Sd, ref["S"])


def test_async_matches_sync(psm):
    W, H, D = 120, 50, 40
    l, r = pair(W, H, D, seed=4)
    ref = B.sgm(l, r, D, pre_filter_cap=63)
    with psm.DispEst(l, r, D) as de:
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        de._ck(de._lib.psm_sgm_set_prefilter(de._h, 63), "psm_sgm_set_prefilter")
        for _ in range(3):                                 # queued behind each other, no host synchronisation in between
            de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
        compare("async", de, ref, de.sgm_disparity())
        t = de.sgm_times()
        print(f"[sgm-bt] times ms: cost {t[0]:.3f} paths {t[1]:.3f} select {t[2]:.3f}")
        assert len(t) == 3 and all(v > 0 for v in t)


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_goldens(psm, golden, name):
    p, g = golden(f"{name}_pair.npz"), golden(f"{name}_sgm_bt.npz")
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        disp = de.SGBM_GPU(pre_filter_cap=63)
        Cd, Sd = de.sgm_costs()
        pl, pr = de.sgm_prefiltered(0), de.sgm_prefiltered(1)
    print(f"[sgm-bt] {name}: differing map elements {int(np.count_nonzero(disp != g['disp']))}")
    assert sha(pl) == str(g["sha_planes_l"]) and sha(pr) == str(g["sha_planes_r"])
    assert sha(Cd) == str(g["sha_C"]) and sha(Sd) == str(g["sha_S"])
    assert np.array_equal(disp, g["disp"])
    assert np.array_equal(disp >= 0, g["valid"].astype(bool))


def test_release_scratch_then_recompute(psm):
    W, H, D = 90, 44, 20
    l, r = pair(W, H, D, seed=6)
    ref = B.sgm(l, r, D, pre_filter_cap=63)
    with psm.DispEst(l, r, D) as de:
        compare("before", de, ref, de.SGBM_GPU(pre_filter_cap=63))
        de.release_scratch()
        with pytest.raises(psm.capi.PsmError):
            de.sgm_prefiltered(0)                          # the planes went with the buffers
        compare("after release", de, ref, de.SGBM_GPU(pre_filter_cap=63))


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_harness_forwards_the_cap(psm, golden, name):
    from primestereomatch_amd import harness
    p, g = golden(f"{name}_pair.npz"), golden(f"{name}_sgm_bt.npz")
    out = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], p["occl"], 4, pre_filter_cap=63)
    assert np.array_equal(out["disp16"], g["disp"])
    best = harness.error_vs_ground_truth(g["best"], p["gt_l"], p["occl"], 64, 4)[0]
    print(f"[sgm-bt] {name}: bp_percent_int {out['bp_percent_int']:.2f}, %BP of best {best:.2f}, cost {out['cost_ms']:.3f} ms")
    assert out["bp_percent_int"] == harness.error_vs_ground_truth(np.maximum(g["disp"], 0) >> 4, p["gt_l"], p["occl"], 64, 4)[0]


def test_cpp_demo_sgbm_ref(psm, golden, tmp_path):
    """psm_demo's sgbm_ref word: the C++ mirror with the reference's whole configuration (setSGBMPreFilterCap(63),
    setSGBMSpeckle(100, 32)) on Cones gives the golden map through the speckle model."""
    import os
    import subprocess
    from conftest import ROOT
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    if not os.path.exists(demo):
        subprocess.run(["make", "-C", os.path.join(ROOT, "primestereomatch_amd", "host")], check=True)
    p, g = golden("cones_pair.npz"), golden("cones_sgm_bt.npz")
    H, W, _ = p["l_bgr"].shape
    p["l_bgr"].tofile(tmp_path / "l.raw")
    p["r_bgr"].tofile(tmp_path / "r.raw")
    env = dict(os.environ, PRIMESM_HIP_LIB=psm.capi.LIB_PATH)
    q = subprocess.run([demo, str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(W), str(H), "64", str(tmp_path / "o"),
                        "1", "f32", "0", "0", "0", "0", "0", "0", "sgbm_ref"], env=env, capture_output=True, text=True, timeout=300)
    assert q.returncode == 0, q.stderr
    assert "STEREO SGBM Times" in q.stdout and "Speckle Time" in q.stdout
    d = np.fromfile(tmp_path / "o_sgbm16.raw", np.int16).reshape(H, W)
    want, _ = K.sgbm_speckle(g["disp"], 100, 32)
    assert np.array_equal(d, want) and not np.array_equal(want, g["disp"])
