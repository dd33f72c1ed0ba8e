"""-m gpu: the Fast Guided Filter over a one-channel pair (psm_gray_compute_fgf, DispEst.Gray_GPU(subsample_rate=s),
harness.compute_gray(subsample_rate=s)) against its definition, tests/gray_fgf_model.py.  There is no tolerance anywhere:
np.array_equal on maps, planes and volumes compared as bit patterns.

The edges of the kernels (psm_gray_fgf.hip, gray_fgf_plan) and the shapes that sit on either side of them, per rate s (R = 8 / s,
k = 2 R + 1, ws = W / s, hs = H / s):
  accepted sizes  ws, hs > R: 10 x 10 (s = 2), 12 x 12 (s = 4), 16 x 16 (s = 8) are the smallest
  column strips   blur4_march owns 64 - 2 R subsampled columns per wave: ws = 56 | 57 (s = 2), 60 | 61 (s = 4), 62 | 63 (s = 8),
                  that is W = 112 | 114, 240 | 244, 496 | 504; W = 115, 247, 511 are one below the next multiple of s, so the
                  nearest-neighbour map drops columns
  row segments    of the model and smooth launches: seg = 4 k subsampled rows for images as small as these (gray_fgf_plan aims at
                  4096 waves and never goes below 4 k rows): 36 (s = 2), 20 (s = 4), 12 (s = 8); hs = seg | seg + 1 - the second a
                  last segment of one row - is H = 72 | 74, 80 | 84, 96 | 104
  row blocks      the full-resolution kernel takes 4 columns x 4 rows per thread at s = 4 and 8 and 4 x 2 at s = 2, its blocks
                  starting two rows above the image at s = 4 and one at s = 2: H = 40 .. 43 (H % 4 = 0 .. 3, H % s != 0 among them);
                  256 threads x 4 columns: W = 1028 is a second x-block
  slice pairs     a wave of the model and smooth launches carries two slices, from d = 1 on: D = 2 (one live slot, the other
                  dead), 3 (both), 4 (a second wave)
  slice chunks    32 slices per chunk: D = 33 (one full chunk) | 34 (a second chunk of one slice), 65 | 66
  border slices   psm_create refuses max_disp > width, so no call has a slice whose every column is border cost; D = W = 16 is the
                  nearest: slice 15 has one column that is not (test_no_context_has_more_slices_than_columns holds the refusal)
The hook walks its chunks from d0 on, so its ranges begin, end and straddle a chunk edge by choice of (d0, d1).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gray_fgf_model as F
import gray_model as M
import score_model as SC
from test_gpu_gray import check_maps, pair, same_bits, want_maps as want_gray_maps

pytestmark = pytest.mark.gpu

RATES = (2, 4, 8)
SEG = {2: 36, 4: 20, 8: 12}      # subsampled rows per segment at the sizes of this file (gray_fgf_plan)


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def fpair(kind, W, H, seed=0):
    """test_gpu_gray.py's generator, and the kinds it does not have"""
    if kind == "constant float":
        return _ro(np.full((H, W), 1000.3, np.float32), np.full((H, W), 1000.3, np.float32))
    if kind == "periodic":       # 0 / 1, period 32 along x, the right plane the left one moved by 3: slices d and d + 32 tie exactly
        base = np.random.default_rng([seed, W, H, 32]).integers(0, 2, (H, 32)).astype(np.float32)
        wide = np.tile(base, (1, W // 32 + 2))
        return _ro(np.ascontiguousarray(wide[:, :W]), np.ascontiguousarray(wide[:, 3:W + 3]))
    return pair(kind, W, H, seed)


@functools.lru_cache(maxsize=None)
def want_maps(kind, W, H, D, s, seed=0):
    """the model's maps: computed once per case, shared, left unchanged"""
    return _ro(*F.maps(*fpair(kind, W, H, seed), D, s))


def run(de, l, r, s, **kw):
    return de.Gray_GPU(l, r, subsample_rate=s, **kw)


# ------------------------------------------------------------------------------------------------------------------ shapes

def _shapes():
    out = [(10, 10, 2, 2), (12, 12, 2, 2), (12, 12, 2, 4), (16, 16, 2, 2), (16, 16, 2, 4), (16, 16, 2, 8)]      # (W, H, D, s): the smallest
    strips = {2: (112, 114, 115), 4: (240, 244, 247), 8: (496, 504, 511)}
    for s in RATES:
        out += [(W, 24, 3, s) for W in strips[s]]                                    # one strip | two strips | dropped columns
        out += [(40, s * SEG[s], 3, s), (40, s * (SEG[s] + 1), 3, s)]                # one segment | a last segment of one row
        out += [(40, H, 3, s) for H in (40, 41, 42, 43)]                             # row blocks, H % s != 0
        out += [(40, 24, D, s) for D in (2, 3, 4)]                                   # slice pairs
        out += [(70, 24, D, s) for D in (33, 34, 65, 66)]                            # slice chunks
        out += [(16, 16, 16, s)]                                                     # D = W
    out += [(1028, 24, 3, 4)]                                                        # a second x-block
    return out


@pytest.mark.parametrize("W,H,D,s", _shapes())
def test_shapes(psm, W, H, D, s):
    l, r = fpair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        got = [m.copy() for m in run(de, l, r, s)]
        check_maps(f"{W}x{H}x{D} s={s}", got, want_maps("noise", W, H, D, s))
        check_maps("download_maps", de.download_maps(), want_maps("noise", W, H, D, s))      # they are the context's current maps


def test_no_context_has_more_slices_than_columns(psm):
    with pytest.raises(psm.capi.PsmError, match="psm_create: max_disp 20 > width 16"):
        psm.DispEst.blank(16, 16, 20)


# ---------------------------------------------------------------------------------------------------------------- contents

KINDS = ["shifted", "binary", "constant", "float", "constant float"]      # tests/test_gray_fgf_model.py: all planes finite


@pytest.mark.parametrize("s", RATES)
@pytest.mark.parametrize("kind", KINDS)
def test_contents(psm, kind, s):
    W, H, D = 131, 70, 16
    l, r = fpair(kind, W, H)
    with psm.DispEst.blank(H, W, D) as de:
        check_maps(f"{kind} s={s}", run(de, l, r, s), want_maps(kind, W, H, D, s))
        side = 1
        wq, wm = F.volume(l, r, side, s, 0, D, want_model=True)
        q, m = de.gray_fgf_volume(side, 0, D, want_model=True)
        assert same_bits(de.gray_fgf_guidance(side), F.Side(l, r, side, s).planes()), (kind, "guidance")
        assert same_bits(m, wm), (kind, "model", int(np.count_nonzero(m != wm)))
        assert same_bits(q, wq), (kind, "q", int(np.count_nonzero(q != wq)))


@pytest.mark.parametrize("s", RATES)
def test_u8_equals_f32_of_the_same_bytes(psm, oracle, s):
    W, H, D = 131, 70, 16
    l, r = fpair("noise", W, H)
    lf, rf = oracle.u8_to_f32(l), oracle.u8_to_f32(r)
    with psm.DispEst.blank(H, W, D) as de:
        a = [m.copy() for m in run(de, l, r, s)]
        pa = [de.gray_fgf_guidance(k) for k in (0, 1)]
        b = [m.copy() for m in run(de, lf, rf, s)]
        pb = [de.gray_fgf_guidance(k) for k in (0, 1)]
    check_maps("u8", a, want_maps("noise", W, H, D, s))
    check_maps("f32 of the same bytes", b, a)
    assert all(same_bits(x, y) for x, y in zip(pa, pb))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_padded_strides(psm, oracle, dtype):
    W, H, D, s = 131, 70, 16, 4
    l, r = fpair("noise", W, H)
    src = (l, r) if dtype == np.uint8 else (oracle.u8_to_f32(l), oracle.u8_to_f32(r))
    pad = [np.full((H, W + 7), 200, dtype) for _ in src]              # junk behind every row
    for p, v in zip(pad, src):
        p[:, :W] = v
    views = [p[:, :W] for p in pad]
    assert views[0].strides[0] == (W + 7) * np.dtype(dtype).itemsize
    with psm.DispEst.blank(H, W, D) as de:
        check_maps(f"padded {np.dtype(dtype).name}", run(de, *views, s), want_maps("noise", W, H, D, s))
        # ... and padded map rows
        lm, rm = np.full((H, W + 5), 255, np.uint8), np.full((H, W + 5), 255, np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        de._ck(de._lib.psm_gray_compute_fgf(de._h, vp(views[0]), vp(views[1]), views[0].strides[0], int(dtype == np.float32), s, vp(lm), vp(rm), W + 5),
               "padded maps")
        check_maps("padded map rows", (lm[:, :W], rm[:, :W]), want_maps("noise", W, H, D, s))
        assert np.all(lm[:, W:] == 255) and np.all(rm[:, W:] == 255)


# ------------------------------------------------------------------------------------------------------------------- hooks

@pytest.mark.parametrize("kind,W,H,D,s", [("noise", 67, 45, 16, 2), ("float", 131, 33, 8, 4), ("noise", 115, 43, 3, 8), ("noise", 16, 16, 2, 8)])
def test_guidance_planes(psm, kind, W, H, D, s):
    l, r = fpair(kind, W, H)
    with psm.DispEst.blank(H, W, D) as de:
        run(de, l, r, s, download=False)
        for side in (0, 1):
            got, want = de.gray_fgf_guidance(side), F.Side(l, r, side, s).planes()
            assert got.shape == (3, H // s, W // s)
            for k, nm in enumerate(("Is", "mI", "den")):
                assert same_bits(got[k], want[k]), (kind, side, nm, int(np.count_nonzero(got[k] != want[k])))


# (d0, d1) against the chunk of 32 slices the walk starts at d0: inside one, exactly one, one more than one, across two edges,
# slice 0 (which the selection never computes), the last slices
RANGES = {4: [(0, 5), (1, 33), (1, 34), (30, 36), (3, 70), (60, 70), (69, 70)], 2: [(0, 34), (30, 36)], 8: [(0, 2), (1, 34), (5, 70)]}


@pytest.mark.parametrize("s", RATES)
def test_volume_slices(psm, s):
    W, H, D = 70, 24, 70
    l, r = fpair("noise", W, H, 3)
    with psm.DispEst.blank(H, W, D) as de:
        before = [m.copy() for m in run(de, l, r, s)]
        for side in (0, 1):
            wq, wm = F.volume(l, r, side, s, 0, D, want_model=True)
            for d0, d1 in RANGES[s]:
                q, m = de.gray_fgf_volume(side, d0, d1, want_model=True)
                assert same_bits(q, wq[d0:d1]), ("q", side, d0, d1, int(np.count_nonzero(q != wq[d0:d1])))
                for k, nm in enumerate(("a", "b", "blur(a)", "blur(b)")):
                    assert same_bits(m[:, k], wm[d0:d1, k]), (nm, side, d0, d1)
            assert same_bits(de.gray_fgf_volume(side, 7, 9), wq[7:9])                      # model NULL
        check_maps("maps untouched by the hooks", de.download_maps(), before)


def test_an_exact_tie_across_a_chunk_seam_goes_to_the_lower_d(psm):
    """The periodic 0 / 1 pair: the slices 3 and 35 are exactly 0 away from the borders, in different chunks (1 .. 32 | 33 .. 39).
    Their keys meet in the key plane, whichever chunk's atomic comes first: 3 wins."""
    W, H, D, s = 131, 40, 40, 4
    l, r = fpair("periodic", W, H)
    vol = F.volume(l, r, 0, s, 0, D)
    best = vol[1:].min(axis=0)
    tie = (vol[3] == best) & (vol[35] == best)
    assert int(np.count_nonzero(tie)) > W * H // 4                                        # the model has the tie in plenty of pixels
    want = want_maps("periodic", W, H, D, s)
    assert np.all(want[0][tie] <= 3)
    with psm.DispEst.blank(H, W, D) as de:
        check_maps("periodic", run(de, l, r, s), want)


# ----------------------------------------------------------------------------------------------------------- committed pairs

@functools.lru_cache(maxsize=None)
def _green(name):
    from conftest import GOLDEN
    import os
    p = np.load(os.path.join(GOLDEN, f"{name}_pair.npz"))
    gl, gr = np.ascontiguousarray(p["l_bgr"][:, :, 1]), np.ascontiguousarray(p["r_bgr"][:, :, 1])
    return _ro(gl, gr) + (p["gt_l"], p["occl"])


@functools.lru_cache(maxsize=None)
def _green_maps(name, s):
    gl, gr, _, _ = _green(name)
    return _ro(*F.maps(gl, gr, 64, s))


PINNED = {("cones", 2): 24295, ("cones", 4): 30464, ("cones", 8): 47346,          # tests/test_gray_fgf_model.py
          ("teddy", 2): 34332, ("teddy", 4): 40940, ("teddy", 8): 55379}


@pytest.mark.parametrize("s", RATES)
@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_middlebury(psm, oracle, name, s):
    gl, gr, gt, occl = _green(name)
    H, W = gl.shape
    want = _green_maps(name, s)
    with psm.DispEst.blank(H, W, 64) as de:
        check_maps(f"{name} s={s}", run(de, gl, gr, s), want)
    bad, _ = oracle.eval_bad_pixels(want[0], gt, occl, 64, 4)
    assert bad == PINNED[name, s]


def test_the_chain_and_the_score_run_behind_it(psm, oracle):
    gl, gr, gt, occl = _green("cones")
    H, W = gl.shape
    lm, rm = _green_maps("cones", 4)
    lv, rv = oracle.lr_check(lm, rm)
    with psm.DispEst.blank(H, W, 64) as de:
        run(de, gl, gr, 4, download=False)
        with pytest.raises(psm.capi.PsmError, match="psm_fill_invalid"):      # no mask of these maps yet
            de.FillInv_GPU()
        de.set_truth(gt, occl)
        rec = de.Score_GPU(SC.GIF)
        m = SC.score(SC.GIF, (lm, rm), gt, occl, 64)
        for k in SC.RECORD_KEYS:
            assert rec[k] == m[k], (k, rec[k], m[k])
        assert rec["bad"] == PINNED["cones", 4]
        de.LRCheck_GPU()
        assert np.array_equal(de.lValid, lv) and np.array_equal(de.rValid, rv)
        de.FillInv_GPU()
        assert np.array_equal(de.lDisMap, oracle.fill_inv(lm, lv)) and np.array_equal(de.rDisMap, oracle.fill_inv(rm, rv))


def test_harness_compute_gray(psm, oracle):
    from primestereomatch_amd import harness
    gl, gr, gt, occl = _green("teddy")
    lm, rm = _green_maps("teddy", 4)
    lv, _ = oracle.lr_check(lm, rm)
    out = harness.compute_gray(gl, gr, 64, gt, occl, lr_check=True, fill=True, subsample_rate=4)
    assert np.array_equal(out["lDisMap_raw"], lm) and np.array_equal(out["rDisMap_raw"], rm)
    assert np.array_equal(out["lValid"], lv) and np.array_equal(out["lDisMap"], oracle.fill_inv(lm, lv))
    assert out["gray_ms"] > 0.0
    plain = harness.compute_gray(gl, gr, 64, gt, occl, lr_check=False, subsample_rate=4)
    assert plain["bad_pixels"] == PINNED["teddy", 4]


# ------------------------------------------------------------------------------------------------------------------- state

def test_both_forms_on_one_context(psm):
    """each call gives its own model's maps whatever ran before it, and the hooks follow the last call"""
    W, H, D = 67, 45, 16
    l, r = fpair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        check_maps("fgf first", run(de, l, r, 4), want_maps("noise", W, H, D, 4))
        check_maps("gray behind fgf", de.Gray_GPU(l, r), want_gray_maps("noise", W, H, D))
        assert same_bits(de.gray_guidance(0), M.Side(l, r, 0).planes())
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_guidance: the planes belong to psm_gray_compute "):
            de.gray_fgf_guidance(0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_volume: the planes belong to psm_gray_compute "):
            de.gray_fgf_volume(0, 0, 1)
        for s in (2, 8, 4):      # a lower rate needs larger planes, a higher one fits
            check_maps(f"fgf {s} behind gray", run(de, l, r, s), want_maps("noise", W, H, D, s))
            assert same_bits(de.gray_fgf_guidance(1), F.Side(l, r, 1, s).planes())
            assert same_bits(de.gray_fgf_volume(1, 0, D), F.volume(l, r, 1, s, 0, D))
        with pytest.raises(psm.capi.PsmError, match="psm_gray_guidance: the planes belong to psm_gray_compute_fgf"):
            de.gray_guidance(0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_volume: the planes belong to psm_gray_compute_fgf"):
            de.gray_volume(0, 0, 1)
    with psm.DispEst.blank(H, W, D) as de:
        check_maps("gray first", de.Gray_GPU(l, r), want_gray_maps("noise", W, H, D))
        check_maps("fgf behind gray", run(de, l, r, 2), want_maps("noise", W, H, D, 2))
        check_maps("gray again", de.Gray_GPU(l, r), want_gray_maps("noise", W, H, D))


def test_the_colour_paths_pending_result_survives(psm, oracle):
    from primestereomatch_amd import synth
    W, H, D, s = 128, 48, 40, 4
    l, r, _ = synth.make_pair(W, H, D, seed=1)
    gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
    want = F.maps(gl, gr, D, s)
    ref = oracle.pipeline_f32(l, r, D, threads=4)
    with psm.DispEst(l, r, D) as de:
        de.CostConst_GPU(); de.CostFilter_GPU()                       # the filtered result is pending as packed minima
        check_maps("fgf in the middle of the colour sequence", run(de, gl, gr, s), want)
        de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])
        check_maps("fgf behind a colour select", run(de, gl, gr, s), want)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()  # the whole colour sequence afterwards
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])


def test_async_and_synchronize(psm):
    W, H, D, s = 131, 70, 33, 4
    l, r = fpair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        assert run(de, l, r, s, download=False) is None
        de.synchronize()
        check_maps("async", de.download_maps(), want_maps("noise", W, H, D, s))


def test_release_and_recompute(psm):
    W, H, D, s = 67, 45, 16, 4
    l, r = fpair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_guidance: no pair"):
            de.gray_fgf_guidance(0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_volume: no pair"):
            de.gray_fgf_volume(0, 0, 1)
        check_maps("before the release", run(de, l, r, s), want_maps("noise", W, H, D, s))
        de.release_scratch()
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_guidance: no pair"):
            de.gray_fgf_guidance(0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_volume: no pair"):
            de.gray_fgf_volume(0, 0, 1)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_time"):
            de.gray_time()
        check_maps("after the release", run(de, l, r, s), want_maps("noise", W, H, D, s))
        assert same_bits(de.gray_fgf_guidance(1), F.Side(l, r, 1, s).planes())


def test_profile_times_the_call(psm):
    W, H, D, s = 67, 45, 16, 4
    l, r = fpair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        run(de, l, r, s)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_time"):
            de.gray_time()
        de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        run(de, l, r, s)
        assert de.gray_time() > 0.0


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refusals(psm):
    W, H, D = 40, 12, 16
    l, r = fpair("noise", W, H)
    lib = psm.capi.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lm, rm = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    assert lib.psm_gray_compute_fgf(None, vp(l), vp(r), 0, 0, 2, None, None, 0) != 0
    assert "psm_gray_compute_fgf" in psm.capi.last_error(None)
    with psm.DispEst.blank(H, W, D) as de:
        before = [m.copy() for m in run(de, *fpair("shifted", W, H), 2)]

        def refused(words, *args):
            assert lib.psm_gray_compute_fgf(de._h, *args) != 0
            msg = psm.capi.last_error(de._h)
            assert "psm_gray_compute_fgf" in msg and all(w in msg for w in words), msg
            check_maps("the previous maps stay current", de.download_maps(), before)

        refused(["NULL"], None, vp(r), 0, 0, 2, vp(lm), vp(rm), 0)
        refused(["NULL"], vp(l), None, 0, 0, 2, vp(lm), vp(rm), 0)
        refused(["depth", "7"], vp(l), vp(r), 0, 7, 2, vp(lm), vp(rm), 0)
        refused(["stride", str(W - 1)], vp(l), vp(r), W - 1, 0, 2, vp(lm), vp(rm), 0)
        refused(["stride", str(4 * W - 4)], vp(l), vp(r), 4 * W - 4, 1, 2, vp(lm), vp(rm), 0)
        refused(["map stride", str(W - 1)], vp(l), vp(r), 0, 0, 2, vp(lm), vp(rm), W - 1)
        for rate in (0, 1, 3, 16, -2):
            refused(["subsample_rate", str(rate), "{2,4,8}"], vp(l), vp(r), 0, 0, rate, vp(lm), vp(rm), 0)
        refused(["too small", "40x12", "subsample_rate 8"], vp(l), vp(r), 0, 0, 8, vp(lm), vp(rm), 0)      # hs = 12 / 8 = 1 is not above 8 / 8
        de.set_rows(4, 8)
        refused(["row stripe"], vp(l), vp(r), 0, 0, 2, vp(lm), vp(rm), 0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_guidance: a row stripe"):
            de.gray_fgf_guidance(0)
        de.set_rows(0, 0)
        assert not lm.any() and not rm.any()                          # nothing was written to the caller's maps either
        check_maps("and the call works again", run(de, l, r, 2), want_maps("noise", W, H, D, 2))
        hooks = de.gray_fgf_guidance(0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_guidance: bad side 2"):
            de.gray_fgf_guidance(2)
        with pytest.raises(psm.capi.PsmError, match=r"psm_gray_fgf_volume: slices \[3,3\)"):
            de.gray_fgf_volume(0, 3, 3)
        with pytest.raises(psm.capi.PsmError, match=r"psm_gray_fgf_volume: slices \[0,17\)"):
            de.gray_fgf_volume(0, 0, 17)
        assert same_bits(de.gray_fgf_guidance(0), hooks)
    # W / s or H / s not above 8 / s: one below the smallest accepted size on either axis, per rate
    for s, small in ((2, 10), (4, 12), (8, 16)):
        for w, h in ((small - 1, small), (small, small - 1)):
            a, b = fpair("noise", w, h)
            with psm.DispEst.blank(h, w, 2) as de:
                with pytest.raises(psm.capi.PsmError, match=f"psm_gray_compute_fgf: {w}x{h} too small for subsample_rate {s}"):
                    run(de, a, b, s)
                check_maps("the full-resolution filter takes it", de.Gray_GPU(a, b), want_gray_maps("noise", w, h, 2))
    with psm.DispEst.blank(H, W, D, dtype="u8") as de:
        with pytest.raises(psm.capi.PsmError, match="psm_gray_compute_fgf: an 8-bit context"):
            run(de, l, r, 2)
    with psm.DispEst.blank(H, W, D, d_range=(0, 8)) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_gray_compute_fgf: a disparity shard"):
            run(de, l, r, 2)
    with psm.DispEst.blank(H, W, D, d_stride=(1, 2)) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_gray_compute_fgf: a disparity shard"):
            run(de, l, r, 2)
