"""-m gpu: the guided-filter path over a one-channel pair (psm_gray_compute, DispEst.Gray_GPU, harness.compute_gray) against its
definition, tests/gray_model.py.  There is no tolerance anywhere: np.array_equal on maps and planes, volumes compared as bit patterns.

The edges of the kernels (psm_gray.hip, gray_plan) and the shapes that sit on either side of them:
  column strips   56 output columns per wave                        W = 56 | 57, 112 | 113 (and the issue's 63, 64, 65, 129)
  row segments    16 rows in the guidance launch and, for images as small as these, in the chunk launches: H = 16 | 17, 32 | 33;
                  a chunk launch of more waves than the device holds at once takes longer segments (gray_plan): on the 256 CUs of
                  an MI355X 672 x 400 x 17 runs segments of 24 rows and the Middlebury pairs at D = 64 segments of 32, the last
                  one short in both
  slice chunks    32 slices per chunk for images this small, from d = 1 on: D = 33 (one full chunk) | 34 (a second chunk of one
                  slice), 65 | 66; D = 130 is four chunks and one slice
  slice groups    a wave carries four slices: D = 2, 3, 4 (one to three live slots, the others dead), 5 (a full group) | 6
The hook walks its chunks from d0 on, so its ranges begin, end and straddle a chunk edge by choice of (d0, d1).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gray_model as M
import score_model as SC

pytestmark = pytest.mark.gpu

DC = 32           # slices per chunk at the sizes of this file (gray_plan: GRAY_DC_MAX)


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
def pair(kind, W, H, seed=0):
    rng = np.random.default_rng([seed, W, H])
    if kind == "noise":
        l, r = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    elif kind == "shifted":      # a textured scene with a real disparity of 3: structure for the filter to aggregate
        base = rng.integers(0, 256, (H, W + 3), dtype=np.uint8)
        l, r = np.ascontiguousarray(base[:, :W]), np.ascontiguousarray(base[:, 3:])
    elif kind == "binary":       # 0 / 1: exact ties everywhere
        l, r = (rng.integers(0, 2, (2, H, W)).astype(np.float32))
    elif kind == "constant":
        l = np.full((H, W), 93, np.uint8)
        r = l.copy()
    elif kind == "float":        # negatives, magnitudes up to 2^10
        l, r = (rng.uniform(-1024.0, 1024.0, (2, H, W)).astype(np.float32))
        l[0, 0], r[-1, -1] = np.float32(1024.0), np.float32(-1024.0)
    else:
        raise KeyError(kind)
    return _ro(np.ascontiguousarray(l), np.ascontiguousarray(r))


@functools.lru_cache(maxsize=None)
def want_maps(kind, W, H, D, seed=0):
    """the model's maps: computed once per case, shared, left unchanged"""
    return _ro(*M.maps(*pair(kind, W, H, seed), D))


def check_maps(name, got, want):
    n = [int(np.count_nonzero(g != w)) for g, w in zip(got, want)]
    print(f"[gray] {name}: differing map elements left {n[0]}  right {n[1]}")
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and np.array_equal(g, w), (name, n, np.argwhere(g != w)[:8].tolist())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ shapes

SHAPES = [(8, 8, 2), (9, 40, 2), (33, 21, 33), (67, 45, 16), (131, 70, 33), (150, 37, 130),
          (63, 9, 5), (64, 9, 5), (65, 9, 6), (129, 9, 5),                       # the issue's widths; slice groups
          (56, 8, 3), (57, 8, 3), (112, 8, 3), (113, 8, 3),                      # column strips
          (40, 16, 3), (40, 17, 3), (40, 32, 4), (40, 33, 4),                    # row segments
          (70, 9, 34), (70, 9, 65), (70, 9, 66)]                                 # slice chunks (33: above)


@pytest.mark.parametrize("W,H,D", SHAPES)
def test_shapes(psm, W, H, D):
    l, r = pair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        got = [m.copy() for m in de.Gray_GPU(l, r)]
        check_maps(f"{W}x{H}x{D}", got, want_maps("noise", W, H, D))
        check_maps("download_maps", de.download_maps(), want_maps("noise", W, H, D))      # they are the context's current maps


def test_longer_row_segments(psm):
    """672 x 400 x 17: the chunk launches run segments of 24 rows (16 full ones and a short one), twelve strips wide."""
    W, H, D = 672, 400, 17
    l, r = pair("shifted", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        check_maps(f"{W}x{H}x{D}", de.Gray_GPU(l, r), want_maps("shifted", W, H, D))


# ------------------------------------------------------------------------------------------------------------------- hooks

@pytest.mark.parametrize("kind,W,H,D", [("noise", 67, 45, 16), ("float", 131, 33, 8), ("noise", 57, 17, 3)])
def test_guidance_planes(psm, kind, W, H, D):
    l, r = pair(kind, W, H)
    with psm.DispEst.blank(H, W, D) as de:
        de.Gray_GPU(l, r, download=False)
        for side in (0, 1):
            got, want = de.gray_guidance(side), M.Side(l, r, side).planes()
            for k, nm in enumerate(("I", "G", "mI", "inv")):
                assert same_bits(got[k], want[k]), (kind, side, nm, int(np.count_nonzero(got[k] != want[k])))


# (d0, d1) against the chunk of 32 slices the walk starts at d0: inside one, exactly one, one more than one, across two edges,
# slice 0 (which the selection never computes), the last slices
RANGES = [(0, 5), (1, 33), (1, 34), (30, 36), (3, 70), (60, 70), (69, 70)]


def test_volume_slices(psm):
    W, H, D = 70, 19, 70
    l, r = pair("noise", W, H, 3)
    with psm.DispEst.blank(H, W, D) as de:
        before = [m.copy() for m in de.Gray_GPU(l, r)]
        for side in (0, 1):
            wq, wab = M.volume(l, r, side, 0, D, want_ab=True)
            for d0, d1 in RANGES:
                q, ab = de.gray_volume(side, d0, d1, want_ab=True)
                assert same_bits(q, wq[d0:d1]), ("q", side, d0, d1, int(np.count_nonzero(q != wq[d0:d1])))
                assert same_bits(ab, wab[d0:d1]), ("ab", side, d0, d1)
            assert same_bits(de.gray_volume(side, 7, 9), wq[7:9])                      # ab NULL
        check_maps("maps untouched by the hooks", de.download_maps(), before)


def test_volume_of_a_float_pair(psm):
    W, H, D = 65, 17, 6
    l, r = pair("float", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        de.Gray_GPU(l, r, download=False)
        for side in (0, 1):
            wq, wab = M.volume(l, r, side, 0, D, want_ab=True)
            q, ab = de.gray_volume(side, 0, D, want_ab=True)
            assert same_bits(q, wq) and same_bits(ab, wab), side


# ---------------------------------------------------------------------------------------------------------------- contents

@pytest.mark.parametrize("kind,W,H,D", [("binary", 67, 21, 16), ("constant", 40, 16, 8), ("float", 131, 33, 33), ("shifted", 129, 40, 16)])
def test_contents(psm, kind, W, H, D):
    l, r = pair(kind, W, H)
    with psm.DispEst.blank(H, W, D) as de:
        got = de.Gray_GPU(l, r)
        check_maps(kind, got, want_maps(kind, W, H, D))
        if kind == "constant":
            assert np.all(got[0] == 1) and np.all(got[1] == 1)          # exact ties go to the lowest candidate


def test_u8_equals_f32_of_the_same_bytes(psm, oracle):
    W, H, D = 67, 21, 16
    l, r = pair("noise", W, H)
    lf, rf = oracle.u8_to_f32(l), oracle.u8_to_f32(r)
    with psm.DispEst.blank(H, W, D) as de:
        a = [m.copy() for m in de.Gray_GPU(l, r)]
        pa = [de.gray_guidance(s) for s in (0, 1)]
        b = [m.copy() for m in de.Gray_GPU(lf, rf)]
        pb = [de.gray_guidance(s) for s in (0, 1)]
    check_maps("u8", a, want_maps("noise", W, H, D))
    check_maps("f32 of the same bytes", b, a)
    assert all(same_bits(x, y) for x, y in zip(pa, pb))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_padded_strides(psm, oracle, dtype):
    W, H, D = 65, 21, 9
    l, r = pair("noise", W, H)
    src = (l, r) if dtype == np.uint8 else (oracle.u8_to_f32(l), oracle.u8_to_f32(r))
    pad = [np.full((H, W + 7), 200, dtype) for _ in src]              # junk behind every row
    for p, s in zip(pad, src):
        p[:, :W] = s
    views = [p[:, :W] for p in pad]
    assert views[0].strides[0] == (W + 7) * np.dtype(dtype).itemsize
    with psm.DispEst.blank(H, W, D) as de:
        check_maps(f"padded {np.dtype(dtype).name}", de.Gray_GPU(*views), want_maps("noise", W, H, D))
        # ... and padded map rows
        lm, rm = np.full((H, W + 5), 255, np.uint8), np.full((H, W + 5), 255, np.uint8)
        de._ck(de._lib.psm_gray_compute(de._h, views[0].ctypes.data_as(C.c_void_p), views[1].ctypes.data_as(C.c_void_p), views[0].strides[0],
                                        int(dtype == np.float32), lm.ctypes.data_as(C.c_void_p), rm.ctypes.data_as(C.c_void_p), W + 5), "padded maps")
        check_maps("padded map rows", (lm[:, :W], rm[:, :W]), want_maps("noise", W, H, D))
        assert np.all(lm[:, W:] == 255) and np.all(rm[:, W:] == 255)


@pytest.fixture(scope="module")
def middlebury(golden, oracle):
    """The green planes of Cones and Teddy at D = 64 through the model once: planes, maps, the oracle's chain on them."""
    out = {}
    for name in ("cones", "teddy"):
        p = golden(f"{name}_pair.npz")
        gl, gr = np.ascontiguousarray(p["l_bgr"][:, :, 1]), np.ascontiguousarray(p["r_bgr"][:, :, 1])
        lm, rm = M.maps(gl, gr, 64)
        lv, rv = oracle.lr_check(lm, rm)
        ref = {"pair": p, "gl": gl, "gr": gr, "lmap": lm, "rmap": rm, "lvalid": lv, "rvalid": rv,
               "lfill": oracle.fill_inv(lm, lv), "rfill": oracle.fill_inv(rm, rv)}
        _ro(*(v for k, v in ref.items() if k != "pair"))
        out[name] = ref
    return out


PINNED = {"cones": 27009, "teddy": 34156}         # tests/test_gray_model.py


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_middlebury(psm, oracle, middlebury, name):
    ref = middlebury[name]
    H, W = ref["gl"].shape
    with psm.DispEst.blank(H, W, 64) as de:
        check_maps(name, de.Gray_GPU(ref["gl"], ref["gr"]), (ref["lmap"], ref["rmap"]))
    bad, _ = oracle.eval_bad_pixels(ref["lmap"], ref["pair"]["gt_l"], ref["pair"]["occl"], 64, 4)
    assert bad == PINNED[name]


# ------------------------------------------------------------------------------------------------------------------- state

def test_the_colour_paths_pending_result_survives(psm, oracle):
    from primestereomatch_amd import synth
    W, H, D = 128, 48, 40
    l, r, _ = synth.make_pair(W, H, D, seed=1)
    gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
    want = M.maps(gl, gr, D)
    ref = oracle.pipeline_f32(l, r, D, threads=4)
    with psm.DispEst(l, r, D) as de:
        de.CostConst_GPU(); de.CostFilter_GPU()                       # the filtered result is pending as packed minima
        check_maps("gray in the middle of the colour sequence", de.Gray_GPU(gl, gr), want)
        de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])
        check_maps("gray behind a colour select", de.Gray_GPU(gl, gr), want)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()  # the whole colour sequence afterwards
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])


def test_the_chain_and_the_score_run_behind_it(psm, middlebury):
    ref = middlebury["cones"]
    p = ref["pair"]
    H, W = ref["gl"].shape
    with psm.DispEst.blank(H, W, 64) as de:
        de.Gray_GPU(ref["gl"], ref["gr"], download=False)
        with pytest.raises(psm.capi.PsmError, match="psm_fill_invalid"):      # no mask of these maps yet
            de.FillInv_GPU()
        de.set_truth(p["gt_l"], p["occl"])
        rec = de.Score_GPU(SC.GIF)
        m = SC.score(SC.GIF, (ref["lmap"], ref["rmap"]), p["gt_l"], p["occl"], 64)
        for k in SC.RECORD_KEYS:
            assert rec[k] == m[k], (k, rec[k], m[k])
        assert rec["bad"] == PINNED["cones"]
        de.LRCheck_GPU()
        assert np.array_equal(de.lValid, ref["lvalid"]) and np.array_equal(de.rValid, ref["rvalid"])
        de.FillInv_GPU()
        assert np.array_equal(de.lDisMap, ref["lfill"]) and np.array_equal(de.rDisMap, ref["rfill"])


def test_async_and_synchronize(psm):
    W, H, D = 131, 70, 33
    l, r = pair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        assert de.Gray_GPU(l, r, download=False) is None
        de.synchronize()
        check_maps("async", de.download_maps(), want_maps("noise", W, H, D))


def test_release_and_recompute(psm):
    W, H, D = 67, 45, 16
    l, r = pair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_gray_guidance: no pair"):
            de.gray_guidance(0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_volume: no pair"):
            de.gray_volume(0, 0, 1)
        check_maps("before the release", de.Gray_GPU(l, r), want_maps("noise", W, H, D))
        de.release_scratch()
        with pytest.raises(psm.capi.PsmError, match="psm_gray_guidance: no pair"):
            de.gray_guidance(0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_time"):
            de.gray_time()
        check_maps("after the release", de.Gray_GPU(l, r), want_maps("noise", W, H, D))
        assert same_bits(de.gray_guidance(1), M.Side(l, r, 1).planes())


def test_two_calls_with_different_pairs(psm):
    W, H, D = 67, 45, 16
    with psm.DispEst.blank(H, W, D) as de:
        for kind, seed in (("noise", 0), ("shifted", 0), ("noise", 1), ("noise", 0)):
            check_maps(f"{kind} {seed}", de.Gray_GPU(*pair(kind, W, H, seed)), want_maps(kind, W, H, D, seed))


def test_profile_times_the_call(psm):
    W, H, D = 67, 45, 16
    l, r = pair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        de.Gray_GPU(l, r)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_time"):
            de.gray_time()
        de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        de.Gray_GPU(l, r)
        assert de.gray_time() > 0.0


def test_flags_of_the_float_path_are_ignored(psm):
    W, H, D = 67, 45, 16
    l, r = pair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        for flags in (psm.capi.PSM_FLAG_F32_TOL, psm.capi.PSM_FLAG_FMA_SOLVE, psm.capi.PSM_FLAG_STORE_FILTERED):
            de.set_option(psm.capi.PSM_OPT_FLAGS, flags)
            check_maps(f"flags {flags}", de.Gray_GPU(l, r), want_maps("noise", W, H, D))


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refusals(psm):
    W, H, D = 40, 12, 16
    l, r = pair("noise", W, H)
    lib = psm.capi.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lm, rm = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    assert lib.psm_gray_compute(None, vp(l), vp(r), 0, 0, None, None, 0) != 0
    assert "psm_gray_compute" in psm.capi.last_error(None)
    with psm.DispEst.blank(H, W, D) as de:
        before = [m.copy() for m in de.Gray_GPU(*pair("shifted", W, H))]

        def refused(words, *args):
            assert lib.psm_gray_compute(de._h, *args) != 0
            msg = psm.capi.last_error(de._h)
            assert "psm_gray_compute" in msg and all(w in msg for w in words), msg
            check_maps("the previous maps stay current", de.download_maps(), before)

        refused(["NULL"], None, vp(r), 0, 0, vp(lm), vp(rm), 0)
        refused(["NULL"], vp(l), None, 0, 0, vp(lm), vp(rm), 0)
        refused(["depth", "7"], vp(l), vp(r), 0, 7, vp(lm), vp(rm), 0)
        refused(["stride", str(W - 1)], vp(l), vp(r), W - 1, 0, vp(lm), vp(rm), 0)
        refused(["stride", str(4 * W - 4)], vp(l), vp(r), 4 * W - 4, 1, vp(lm), vp(rm), 0)
        refused(["map stride", str(W - 1)], vp(l), vp(r), 0, 0, vp(lm), vp(rm), W - 1)
        de.set_rows(4, 8)
        refused(["row stripe"], vp(l), vp(r), 0, 0, vp(lm), vp(rm), 0)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_guidance: a row stripe"):
            de.gray_guidance(0)
        de.set_rows(0, 0)
        assert not lm.any() and not rm.any()                          # nothing was written to the caller's maps either
        check_maps("and the call works again", de.Gray_GPU(l, r), want_maps("noise", W, H, D))
    with psm.DispEst.blank(H, W, D, dtype="u8") as de:
        with pytest.raises(psm.capi.PsmError, match="psm_gray_compute: an 8-bit context"):
            de.Gray_GPU(l, r)
    with psm.DispEst.blank(H, W, D, d_range=(0, 8)) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_gray_compute: a disparity shard"):
            de.Gray_GPU(l, r)
    with psm.DispEst.blank(H, W, D, d_stride=(1, 2)) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_gray_compute: a disparity shard"):
            de.Gray_GPU(l, r)


def test_a_blank_object_has_no_colour_pair(psm):
    """DispEst.blank: the gray call needs no staged pair and stages none - the colour path is refused before and after it."""
    W, H, D = 40, 12, 16
    l, r = pair("noise", W, H)
    with psm.DispEst.blank(H, W, D) as de:
        with pytest.raises(psm.capi.PsmError, match="psm_cost_construct: no image pair"):
            de.CostConst_GPU()
        check_maps("blank", de.Gray_GPU(l, r), want_maps("noise", W, H, D))
        with pytest.raises(psm.capi.PsmError, match="psm_cost_construct: no image pair"):
            de.CostConst_GPU()


# ----------------------------------------------------------------------------------------------------------------- harness

def test_harness_compute_gray(psm, middlebury):
    from primestereomatch_amd import harness
    ref = middlebury["teddy"]
    p = ref["pair"]
    for tail in (False, True):
        out = harness.compute_gray(ref["gl"], ref["gr"], 64, p["gt_l"], p["occl"], lr_check=True, fill=True, device_tail=tail)
        assert np.array_equal(out["lDisMap_raw"], ref["lmap"]) and np.array_equal(out["rDisMap_raw"], ref["rmap"])
        assert np.array_equal(out["lValid"], ref["lvalid"]) and np.array_equal(out["lDisMap"], ref["lfill"])
        assert out["gray_ms"] > 0.0 and "bp_percent" in out
    plain = harness.compute_gray(ref["gl"], ref["gr"], 64, p["gt_l"], p["occl"], lr_check=False)
    assert np.array_equal(plain["lDisMap"], ref["lmap"]) and plain["bad_pixels"] == PINNED["teddy"] and "lValid" not in plain
