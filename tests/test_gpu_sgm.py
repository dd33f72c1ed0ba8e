"""-m gpu: semi-global matching on the device (psm_sgm_compute, DispEst.SGBM_GPU) against its definition, the numpy model
tests/sgm_model.py.  Everything is integer: block costs C, summed path costs S and the final int16 map must equal the model with
0 differing elements - there is no tolerance anywhere in this file."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import sgm_model as M

pytestmark = pytest.mark.gpu


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
    """C, S and the map of the last SGBM_GPU of `de` against a model result; prints the counts, asserts 0."""
    Cd, Sd = de.sgm_costs()
    nc, ns, nd = (int(np.count_nonzero(a != b)) for a, b in ((Cd, ref["C"]), (Sd, ref["S"]), (disp, ref["disp"])))
    print(f"[sgm] {name}: differing elements C {nc}  S {ns}  map {nd}  (valid {ref['valid'].mean():.3f})")
    assert disp.dtype == np.int16 and Cd.dtype == np.uint16 and Sd.dtype == np.uint32
    assert (nc, ns, nd) == (0, 0, 0)


def pair(psm, W, H, D, seed=0):
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=seed)
    return l, r


# odd sizes, D not a multiple of 16 / 64, W == D (the narrowest image a context accepts: psm_create refuses max_disp > width, so
# W < D exists in the model tests only), 1, 2 and 4 disparities per lane
@pytest.mark.parametrize("W,H,D", [(67, 45, 16), (131, 70, 33), (33, 21, 33), (70, 9, 70), (9, 40, 2), (150, 37, 130), (140, 33, 129)])
def test_small_pairs_equal_the_model(psm, W, H, D):
    l, r = pair(psm, W, H, D, seed=W)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU()
        compare(f"{W}x{H}x{D}", de, M.sgm(l, r, D), disp)


def test_w_below_d_is_refused_at_creation(psm):
    l, r = pair(psm, 24, 16, 8)
    with pytest.raises(psm.capi.PsmError):
        psm.DispEst(l, r, 32)
    assert "width" in psm.capi.last_error(None)


@pytest.mark.parametrize("W,H,D", [(67, 45, 16), (131, 70, 33), (40, 23, 40)])
def test_one_channel_pair(psm, W, H, D):
    l, r = pair(psm, W, H, D, seed=5)
    gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(gray=(gl, gr))
        compare(f"gray {W}x{H}x{D}", de, M.sgm(gl, gr, D), disp)
        # the staged colour pair is still there, and still the one the next call uses
        compare("colour after gray", de, M.sgm(l, r, D), de.SGBM_GPU())


@pytest.mark.parametrize("bs", [1, 3, 5, 7])
def test_each_block_size(psm, bs):
    W, H, D = 93, 41, 24
    l, r = pair(psm, W, H, D, seed=bs)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(block_size=bs)
        compare(f"bs {bs}", de, M.sgm(l, r, D, block_size=bs), disp)


@pytest.mark.parametrize("kw", [
    dict(P1=1, P2=1), dict(P1=7, P2=7000), dict(P1=600, P2=600, block_size=3), dict(uniqueness_ratio=0), dict(uniqueness_ratio=99),
    dict(disp12_max_diff=-1), dict(disp12_max_diff=0), dict(disp12_max_diff=5, uniqueness_ratio=30),
    dict(uniqueness_ratio=0, disp12_max_diff=-1), dict(block_size=7, P1=100, P2=65535 - 49 * 3 * 255)])
def test_non_default_parameters(psm, kw):
    W, H, D = 101, 39, 48
    l, r = pair(psm, W, H, D, seed=11)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(**kw)
        ref = M.sgm(l, r, D, **kw)
        compare(str(kw), de, ref, disp)
        if kw.get("uniqueness_ratio") == 0 and kw.get("disp12_max_diff", 1) < 0:
            assert disp.min() >= 0                     # no invalid pixel is left


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_goldens(psm, golden, name):
    p, g = golden(f"{name}_pair.npz"), golden(f"{name}_sgm.npz")
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        disp = de.SGBM_GPU()
        Cd, Sd = de.sgm_costs()
    print(f"[sgm] {name}: differing map elements {int(np.count_nonzero(disp != g['disp']))}")
    assert np.array_equal(disp, g["disp"])
    assert sha(Cd) == str(g["sha_C"]) and sha(Sd) == str(g["sha_S"])
    assert np.array_equal(disp >= 0, g["valid"].astype(bool))


@pytest.mark.parametrize("W,H,D", [(320, 180, 128), (640, 360, 256)])
def test_large_disparity_ranges_against_the_live_model(psm, W, H, D):
    l, r = pair(psm, W, H, D, seed=2)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU()
        compare(f"{W}x{H}x{D}", de, M.sgm(l, r, D), disp)


def test_float_upload_gives_the_8_bit_map(psm):
    W, H, D = 131, 70, 33
    l, r = pair(psm, W, H, D, seed=3)
    lf, rf = (a.astype(np.float32) * np.float32(1 / 255.0) for a in (l, r))      # src/StereoMatch.cpp:195-196
    with psm.DispEst(l, r, D) as de:
        d8 = de.SGBM_GPU()
        de.setInputImages(lf, rf)
        df = de.SGBM_GPU()
        compare("float upload", de, M.sgm(l, r, D), df)
    assert np.array_equal(d8, df)
    assert np.array_equal(M.quantise(lf), l)


def test_fresh_results_per_call_and_per_pair(psm):
    W, H, D = 120, 50, 40
    l0, r0 = pair(psm, W, H, D, seed=0)
    l1, r1 = pair(psm, W, H, D, seed=1)
    ref0, ref1 = M.sgm(l0, r0, D), M.sgm(l1, r1, D)
    assert not np.array_equal(ref0["disp"], ref1["disp"])
    with psm.DispEst(l0, r0, D) as de:
        compare("first", de, ref0, de.SGBM_GPU())
        compare("again", de, ref0, de.SGBM_GPU())
        de.setInputImages(l1, r1)
        compare("new pair", de, ref1, de.SGBM_GPU())
        compare("other parameters", de, M.sgm(l1, r1, D, block_size=3, uniqueness_ratio=0), de.SGBM_GPU(block_size=3, uniqueness_ratio=0))
        de.setInputImages(l0, r0)
        compare("first pair again", de, ref0, de.SGBM_GPU())


def test_async_matches_sync_and_times_need_profile(psm):
    W, H, D = 120, 50, 40
    l, r = pair(psm, W, H, D, seed=4)
    ref = M.sgm(l, r, D)
    with psm.DispEst(l, r, D) as de:
        with pytest.raises(psm.capi.PsmError):
            de.SGBM_GPU()
            de.sgm_times()                                 # not timed
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        for _ in range(3):                                 # queued behind each other, no host synchronisation in between
            de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
        compare("async", de, ref, de.sgm_disparity())
        t = de.sgm_times()
        print(f"[sgm] times ms: cost {t[0]:.3f} paths {t[1]:.3f} select {t[2]:.3f}")
        assert len(t) == 3 and all(v > 0 for v in t)


def test_release_scratch_then_recompute(psm):
    W, H, D = 90, 44, 20
    l, r = pair(psm, W, H, D, seed=6)
    ref = M.sgm(l, r, D)
    with psm.DispEst(l, r, D) as de:
        compare("before", de, ref, de.SGBM_GPU())
        de.release_scratch()
        with pytest.raises(psm.capi.PsmError):
            de.sgm_disparity()                             # the result went with the buffers
        compare("after release", de, ref, de.SGBM_GPU())


def test_isolation_from_the_gif_path(psm):
    W, H, D = 128, 48, 32
    l, r = pair(psm, W, H, D, seed=7)
    ref = M.sgm(l, r, D)
    with psm.DispEst(l, r, D) as plain:
        plain.CostConst_GPU(); plain.CostFilter_GPU(); plain.DispSelect_GPU(); plain.LRCheck_GPU()
        want = [a.copy() for a in (plain.lDisMap, plain.rDisMap, plain.lValid, plain.rValid)]
    with psm.DispEst(l, r, D) as de:
        maps = [de.SGBM_GPU()]
        de.CostConst_GPU()
        maps.append(de.SGBM_GPU())
        de.CostFilter_GPU()
        maps.append(de.SGBM_GPU())
        de.DispSelect_GPU()
        maps.append(de.SGBM_GPU())
        de.LRCheck_GPU()
        maps.append(de.SGBM_GPU())
        got = [de.lDisMap, de.rDisMap, de.lValid, de.rValid]
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        for m in maps:
            assert np.array_equal(m, ref["disp"])
        # and with the volumes materialised in between
        lv = de.download_volume(0)
        de.SGBM_GPU()
        assert np.array_equal(de.download_volume(0), lv)
        assert np.array_equal(de.download_maps()[0], want[0])


def test_refusals(psm):
    capi = psm.capi
    W, H, D = 64, 32, 16
    l, r = pair(psm, W, H, D)
    with psm.DispEst(l, r, D, d_range=(0, 8)) as sh:
        with pytest.raises(capi.PsmError, match="shard"):
            sh.SGBM_GPU()
    with psm.DispEst(l, r, D, d_stride=(1, 2)) as sh:
        with pytest.raises(capi.PsmError, match="shard"):
            sh.SGBM_GPU()
    with psm.DispEst(l, r, D) as de:
        de.set_rows(8, 24)
        with pytest.raises(capi.PsmError, match="stripe"):
            de.SGBM_GPU()
        de.set_rows(0, 0)
        for kw, word in ((dict(block_size=4), "block_size"), (dict(block_size=9), "block_size"), (dict(P1=10, P2=5), "P1"),
                         (dict(P1=-1), "P1"), (dict(block_size=7, P2=65535 - 49 * 3 * 255 + 1), "65535"),
                         (dict(uniqueness_ratio=100), "uniqueness_ratio"), (dict(uniqueness_ratio=-1), "uniqueness_ratio")):
            with pytest.raises(capi.PsmError, match=word):
                de.SGBM_GPU(**kw)
        with pytest.raises(capi.PsmError, match="no result"):
            de.sgm_disparity()                             # nothing above launched anything
        de.SGBM_GPU()                                      # a refused parameter set leaves the accepted one in force
    # a context nothing was uploaded to
    import ctypes as C
    lib, h = capi.load(), C.c_void_p()
    assert lib.psm_create(C.byref(h), W, H, D, capi.PSM_F32, 0) == 0
    try:
        assert lib.psm_sgm_compute(h) != 0
        assert "no image pair" in capi.last_error(h)
        out = np.zeros((H, W), np.int16)
        assert lib.psm_sgm_download_disparity(h, out.ctypes.data_as(C.c_void_p), 0) != 0
    finally:
        lib.psm_destroy(h)


def test_cpp_demo_sgbm(psm, golden, tmp_path):
    """psm_demo's sgbm argument: DispEst::SGBM_GPU of the C++ mirror on Cones gives the golden map."""
    from conftest import ROOT
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    if not os.path.exists(demo):
        subprocess.run(["make", "-C", os.path.join(ROOT, "primestereomatch_amd", "host")], check=True)
    p, g = golden("cones_pair.npz"), golden("cones_sgm.npz")
    H, W, _ = p["l_bgr"].shape
    p["l_bgr"].tofile(tmp_path / "l.raw")
    p["r_bgr"].tofile(tmp_path / "r.raw")
    env = dict(os.environ, PRIMESM_HIP_LIB=psm.capi.LIB_PATH)
    for float_input in ("0", "1"):
        q = subprocess.run([demo, str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(W), str(H), "64", str(tmp_path / "o"),
                            "1", "f32", float_input, "0", "0", "0", "0", "0", "sgbm"], env=env, capture_output=True, text=True, timeout=300)
        assert q.returncode == 0, q.stderr
        assert "STEREO SGBM Times" in q.stdout and "Paths Time" in q.stdout
        d = np.fromfile(tmp_path / "o_sgbm16.raw", np.int16).reshape(H, W)
        assert sha(d) == sha(g["disp"])


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_harness_compute_sgbm(psm, golden, name):
    from primestereomatch_amd import harness
    p, g = golden(f"{name}_pair.npz"), golden(f"{name}_sgm.npz")
    out = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], p["occl"], 4)
    assert np.array_equal(out["disp16"], g["disp"])
    shown = M.display_map(g["disp"], 4)                    # the model through the same host-side conversion
    assert np.array_equal(out["lDispMap"], shown)
    bp, avg, bad, _ = harness.error_vs_ground_truth(shown, p["gt_l"], p["occl"], 64, 1)
    assert (out["bp_percent"], out["avg_err"], out["bad_pixels"]) == (bp, avg, bad)
    bpi = harness.error_vs_ground_truth(np.maximum(g["disp"], 0) >> 4, p["gt_l"], p["occl"], 64, 4)[0]
    assert out["bp_percent_int"] == bpi
    print(f"[sgm] {name}: %BP as displayed {out['bp_percent']:.2f}, bp_percent_int {bpi:.2f}")
