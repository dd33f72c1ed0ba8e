"""The numpy model of the SGM stage's census cost (tests/sgm_census_model.py) against an independent scalar restatement of its
definition, against known answers, against the figures a first scratch writing of the definition gave, and against the committed
fixtures; then the surface of psm_sgm_set_census / psm_sgm_download_census without a device.  All integer, no tolerance."""
import ctypes as C
import hashlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sgm_census_model as Z
import sgm_model as M
import sgm_range_model as R

from conftest import ROOT

WINDOWS = [(3, 3), (5, 5), (7, 5), (7, 7), (9, 3), (9, 7)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the definition once more, with plain loops and no helper of the model ------------------------------------------------------
def scalar_gray(img):
    H, W = img.shape[:2]
    if img.ndim == 2 or img.shape[2] == 1:
        return [[int(img.reshape(H, W)[y][x]) for x in range(W)] for y in range(H)]
    return [[(1868 * int(img[y][x][0]) + 9617 * int(img[y][x][1]) + 4899 * int(img[y][x][2]) + 8192) >> 14 for x in range(W)]
            for y in range(H)]


def scalar_codes(img, w, h):
    g = scalar_gray(img)
    H, W = len(g), len(g[0])
    T = np.zeros((H, W), np.uint64)
    for y in range(H):
        for x in range(W):
            code, i = 0, 0
            for dy in range(-(h // 2), h // 2 + 1):
                for dx in range(-(w // 2), w // 2 + 1):
                    if dy == 0 and dx == 0:
                        continue
                    if g[min(max(y + dy, 0), H - 1)][min(max(x + dx, 0), W - 1)] < g[y][x]:
                        code |= 1 << i
                    i += 1
            assert i == w * h - 1 and code < 1 << (w * h - 1)
            T[y, x] = code
    return T


def scalar_cost(TL, TR, dmin, D):
    H, W = TL.shape
    c = np.zeros((H, W, D), np.int32)
    for y in range(H):
        for x in range(W):
            for k in range(D):
                xr = min(max(x - (dmin + k), 0), W - 1)
                c[y, x, k] = bin(int(TL[y, x]) ^ int(TR[y, xr])).count("1")
    return c


# 9x5; 3x2 and 2x1: every window reaches past both edges at once; 13x4 D 13: W = D; a negative minimum reaches past the right edge
@pytest.mark.parametrize("W,H,D,dmin", [(9, 5, 4, 0), (3, 2, 3, 0), (2, 1, 2, -1), (13, 4, 13, 0), (11, 6, 7, -4), (10, 5, 5, 3)])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("win", WINDOWS)
def test_model_equals_the_scalar_restatement(W, H, D, dmin, ch, win):
    rng = np.random.default_rng(W * 1000 + H * 10 + ch + win[0] * 7 + win[1])
    L = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    Rt = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    TL, TR = scalar_codes(L, *win), scalar_codes(Rt, *win)
    assert np.array_equal(Z.codes(L, *win), TL) and np.array_equal(Z.codes(Rt, *win), TR)
    c = scalar_cost(TL, TR, dmin, D)
    assert np.array_equal(Z.pixel_cost(L, Rt, dmin, D, *win), c)
    if ch == 1:                                           # a 2-d image is the 1-channel image
        assert np.array_equal(Z.pixel_cost(L[:, :, 0], Rt[:, :, 0], dmin, D, *win), c)


# ---- known answers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", WINDOWS)
def test_codes_of_a_constant_image_are_0(win):
    for ch in (1, 3):
        img = np.full((8, 12, ch), 200, np.uint8)
        assert Z.codes(img, *win).dtype == np.uint64 and not Z.codes(img, *win).any()
        assert not Z.pixel_cost(img, img, -2, 6, *win).any()


def test_bit_i_is_tap_i_by_hand():
    """3 x 3 on a 5 x 5 image: the taps are NW N NE W E SW S SE = bits 0 .. 7.  The centre pixel (2, 2) = 50 sees
    40 50 60 / 10 . 90 / 50 49 51: darker are NW (bit 0), W (bit 3) and S (bit 6); N and SW TIE with the centre and give 0."""
    g = np.full((5, 5), 100, np.uint8)
    g[1, 1:4] = (40, 50, 60)
    g[2, 1:4] = (10, 50, 90)
    g[3, 1:4] = (50, 49, 51)
    T = Z.codes(g, 3, 3)
    assert int(T[2, 2]) == (1 << 0) | (1 << 3) | (1 << 6) == 73
    assert Z.taps(3, 3) == [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    # the corner (0, 0) = 100 is replicated: its taps N, W, NW, NE, SW are 100 (ties); E = g[0][1] = 100, S = g[1][0] = 100,
    # SE = g[1][1] = 40 < 100: bit 7 only
    assert int(T[0, 0]) == 1 << 7
    # (1, 0) = 100: W is itself replicated; E = 40 (bit 4), SE = g[2][1] = 10 (bit 7), NE = g[0][1] = 100
    assert int(T[1, 0]) == (1 << 4) | (1 << 7)
    # the taps of a 9 x 7 window: 62 of them, tap 31 is the one left of the centre, tap 32 the one right of it
    t = Z.taps(9, 7)
    assert len(t) == 62 and t[0] == (-3, -4) and t[30] == (0, -1) and t[31] == (0, 1) and t[61] == (3, 4)


@pytest.mark.parametrize("win", WINDOWS)
def test_cost_bound_is_reached_on_an_impulse_pair(win):
    """Left: a bright impulse (every tap darker: all win_w win_h - 1 bits); right: constant (code 0)."""
    w, h = win
    L = np.zeros((9, 13), np.uint8)
    L[4, 6] = 255
    Rt = np.zeros((9, 13), np.uint8)
    assert int(Z.codes(L, w, h)[4, 6]) == (1 << (w * h - 1)) - 1
    c = Z.pixel_cost(L, Rt, 0, 4, w, h)
    print(f"[sgm-census-model] {w}x{h}: max c {int(c.max())}, bound {w * h - 1}")
    assert c.max() == w * h - 1 == c[4, 6, 0] and c.max() <= 62
    rng = np.random.default_rng(w + h)
    A = (rng.integers(0, 2, (24, 40, 3)) * 255).astype(np.uint8)
    B = (rng.integers(0, 2, (24, 40, 3)) * 255).astype(np.uint8)
    o = Z.sgm(A, B, 0, 16, census=win, block_size=7, P1=100, P2=65535 - 49 * 3 * 255)
    assert o["C"].dtype == np.uint16 and int(o["C"].max()) <= 49 * (w * h - 1) <= 3038 and o["max_l"] <= 65535


def test_block_size_1_is_the_pixel_cost_and_reaches_62_on_cones(golden):
    p = golden("cones_pair.npz")
    l, r = p["l_bgr"][100:160], p["r_bgr"][100:160]
    o = Z.sgm(l, r, 0, 64, census=(9, 7), block_size=1)
    assert np.array_equal(o["C"], Z.pixel_cost(l, r, 0, 64, 9, 7))
    assert int(Z.pixel_cost(p["l_bgr"], p["r_bgr"], 0, 64, 9, 7).max()) == 62


@pytest.mark.parametrize("win", [(5, 5), (9, 7)])
def test_codes_survive_gain_and_offset(win):
    """g -> a g + b, a > 0, nothing saturating: the order of any two values is kept, so is every code - what the cost exists for."""
    rng = np.random.default_rng(11)
    g = rng.integers(0, 100, (20, 30), dtype=np.uint8)
    T = Z.codes(g, *win)
    for a, b in ((1, 37), (2, 0), (2, 55)):
        assert np.array_equal(Z.codes((a * g.astype(np.int32) + b).astype(np.uint8), *win), T)
    assert not np.array_equal(Z.codes(255 - g, *win), T)


def test_a_darker_right_camera_changes_the_sad_map_not_the_census_map():
    """Right image 0.6 R + 20 (exact on multiples of 5: no rounding, no saturation, the order and the ties kept)."""
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(64, 32, 12, seed=4)
    gl = (l[:, :, 1] // 5 * 5).astype(np.uint8)
    gr = (r[:, :, 1] // 5 * 5).astype(np.uint8)
    dark = (gr.astype(np.int32) * 3 // 5 + 20).astype(np.uint8)
    assert np.array_equal(dark.astype(np.int32), (gr.astype(np.int32) * 6 + 200) // 10) and dark.max() < 255
    a, b = Z.sgm(gl, gr, 0, 12, census=(9, 7)), Z.sgm(gl, dark, 0, 12, census=(9, 7))
    assert np.array_equal(a["codes"][1], b["codes"][1]) and np.array_equal(a["C"], b["C"]) and np.array_equal(a["disp"], b["disp"])
    sa, sb = M.sgm(gl, gr, 12), M.sgm(gl, dark, 12)
    n = int(np.count_nonzero(sa["disp"] != sb["disp"]))
    print(f"[sgm-census-model] darker right camera: SAD map differs in {n} of {sa['disp'].size} pixels, census map in 0")
    assert n > 0


def test_gray_is_as_defined():
    rng = np.random.default_rng(2)
    bgr = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    g = Z.gray(bgr)
    assert g.dtype == np.uint8 and g.tolist() == scalar_gray(bgr)
    assert Z.GRAY_B + Z.GRAY_G + Z.GRAY_R == 16384
    assert int(Z.gray(np.full((1, 1, 3), 255, np.uint8))[0, 0]) == 255 and int(Z.gray(np.zeros((1, 1, 3), np.uint8))[0, 0]) == 0
    one = np.zeros((1, 3, 3), np.uint8)
    one[0, 0, 0] = one[0, 1, 1] = one[0, 2, 2] = 255                       # pure B, G, R in the staged order
    assert Z.gray(one)[0].tolist() == [(1868 * 255 + 8192) >> 14, (9617 * 255 + 8192) >> 14, (4899 * 255 + 8192) >> 14] == [29, 150, 76]
    mono = rng.integers(0, 256, (6, 9), dtype=np.uint8)
    assert np.array_equal(Z.gray(mono), mono) and np.array_equal(Z.gray(mono[:, :, None]), mono)


def test_a_float_pair_is_quantised_first():
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(40, 20, 8, seed=6)
    lf, rf = (a.astype(np.float32) * np.float32(1 / 255.0) for a in (l, r))
    assert np.array_equal(M.quantise(lf), l)
    a, b = Z.sgm(l, r, 0, 8, census=(7, 5)), Z.sgm(lf, rf, 0, 8, census=(7, 5))
    for k in ("C", "S", "disp"):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(a["codes"][0], b["codes"][0]) and np.array_equal(a["codes"][1], b["codes"][1])
    half = np.full((4, 6), 0.5, np.float32)                                # 127.5 -> 128 (ties to even)
    assert np.array_equal(Z.gray(half), np.full((4, 6), 128, np.uint8))


def test_the_range_models_right_column_is_used():
    rng = np.random.default_rng(8)
    W, H, D, dmin = 14, 5, 9, -5
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    Rt = rng.integers(0, 256, (H, W), dtype=np.uint8)
    TL, TR = Z.codes(L, 5, 5), Z.codes(Rt, 5, 5)
    c = Z.pixel_cost(L, Rt, dmin, D, 5, 5)
    for k in range(D):
        xr = R.right_columns(W, dmin, k)
        assert xr.max() == W - 1 if dmin + k < 0 else xr.min() == 0                   # clamped on the side it reaches past
        assert np.array_equal(c[:, :, k], Z.popcount(TL ^ TR[:, xr]))
    o = Z.sgm(L, Rt, dmin, D, census=(5, 5), block_size=3)
    assert o["range"] == (dmin, D) and o["invalid"] == (dmin - 1) * 16
    assert np.array_equal(o["C"], M.block_cost(c, 3))


def test_census_off_is_the_range_model_and_bad_windows_are_refused():
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(40, 20, 12, seed=2)
    for off in (None, (0, 0)):
        a, b = Z.sgm(l, r, 0, 12, census=off, block_size=3), R.sgm(l, r, 0, 12, block_size=3)
        assert a.keys() == b.keys()
        for k in b:
            assert np.array_equal(a[k], b[k]), k
    o = Z.sgm(l, r, 0, 12, census=(9, 7), block_size=3)
    assert o["params"][:3] == (3, 8 * 3 * 9, 32 * 3 * 9)                   # P1, P2 from the pair's channels, whatever the cost
    assert not np.array_equal(o["C"], b["C"])
    for bad in ((1, 1), (4, 5), (5, 4), (11, 7), (9, 9), (3, 1), (0, 3), (-3, 3)):
        with pytest.raises(ValueError):
            Z.check_window(*bad)


# ---- the figures of the first scratch writing, and the fixtures ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def middlebury(golden):
    out = {}
    for name in ("cones", "teddy"):
        p = golden(f"{name}_pair.npz")
        out[name] = (p, Z.sgm(p["l_bgr"], p["r_bgr"], 0, 64, census=(9, 7)))
    return out


def bp_of(p, o):
    from primestereomatch_amd import harness
    return harness.error_vs_ground_truth(o["best"], p["gt_l"], p["occl"], 64, 4)[0]


def test_cones_9x7_gives_the_scratch_figures(middlebury):
    p, o = middlebury["cones"]
    got = (round(bp_of(p, o), 2), int(o["C"].max()), int(o["S"].max()), o["max_l"])
    print(f"[sgm-census-model] cones 9x7, defaults: %BP {got[0]:.2f}  max C {got[1]}  max S {got[2]}  max L_r {got[3]}")
    assert got == (3.95, 1393, 30344, 3793)


def test_cones_5x5_and_7x7_give_the_scratch_figures(golden):
    p = golden("cones_pair.npz")
    a = bp_of(p, Z.sgm(p["l_bgr"], p["r_bgr"], 0, 64, census=(5, 5)))
    b = bp_of(p, Z.sgm(p["l_bgr"], p["r_bgr"], 0, 64, census=(7, 7), block_size=3, P1=60, P2=300))
    print(f"[sgm-census-model] cones: %BP 5x5 defaults {a:.2f}, 7x7 bs 3 P1 60 P2 300 {b:.2f}")
    assert (round(a, 2), round(b, 2)) == (4.83, 3.36)


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_model_is_pinned_to_the_fixtures(middlebury, golden, name):
    _, o = middlebury[name]
    g = golden(f"{name}_sgm_census.npz")
    assert sorted(g.files) == ["best", "disp", "sha_C", "sha_S", "sha_codes_l", "sha_codes_r", "valid"]
    assert g["disp"].dtype == np.int16 and np.array_equal(o["disp"], g["disp"])
    assert np.array_equal(o["best"], g["best"]) and np.array_equal(o["valid"], g["valid"].astype(bool))
    assert sha(o["C"]) == str(g["sha_C"]) and sha(o["S"]) == str(g["sha_S"])
    assert sha(o["codes"][0]) == str(g["sha_codes_l"]) and sha(o["codes"][1]) == str(g["sha_codes_r"])
    assert o["codes"][0].shape == o["disp"].shape and o["codes"][0].dtype == np.uint64
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"{name}_sgm_census.npz")) < 1000000


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_quality_against_the_other_two_costs(middlebury, golden, name):
    """%BP of `best` under the occlusion mask: census 9 x 7 3.95 / 6.82 against SAD 4.97 / 10.46 and Birchfield-Tomasi 4.76 / 10.14."""
    from primestereomatch_amd import harness
    p, o = middlebury[name]
    bp = bp_of(p, o)
    sad = harness.error_vs_ground_truth(golden(f"{name}_sgm.npz")["best"], p["gt_l"], p["occl"], 64, 4)[0]
    bt = harness.error_vs_ground_truth(golden(f"{name}_sgm_bt.npz")["best"], p["gt_l"], p["occl"], 64, 4)[0]
    print(f"[sgm-census-model] {name}: %BP of best {bp:.2f} (SAD {sad:.2f}, Birchfield-Tomasi {bt:.2f})")
    assert round(bp, 2) == {"cones": 3.95, "teddy": 6.82}[name] and bp < bt < sad


# ---- the ABI without a device ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_capi_binds_both_symbols(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    assert decl["psm_sgm_set_census"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int])
    assert decl["psm_sgm_download_census"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p])
    lib = built.load()
    assert hasattr(lib, "psm_sgm_set_census") and hasattr(lib, "psm_sgm_download_census")
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT psm_sgm_set_census\b", out) and re.search(r"\bT psm_sgm_download_census\b", out)


def test_null_and_bad_windows_are_refused_without_a_device(built):
    lib = built.load()
    for ok in ((9, 7), (0, 0), (3, 3), (5, 7), (9, 3)):                    # in range: only the context is missing
        assert lib.psm_sgm_set_census(None, *ok) != 0
        assert "psm_sgm_set_census" in built.last_error(None) and "NULL" in built.last_error(None)
    for bad in ((4, 5), (5, 4), (8, 6), (1, 1), (1, 3), (3, 1), (11, 7), (9, 9), (0, 3), (3, 0), (-3, 3), (-9, -7), (1 << 20, 3)):
        assert lib.psm_sgm_set_census(None, *bad) != 0
        msg = built.last_error(None)
        assert "psm_sgm_set_census" in msg and f"{bad[0]} x {bad[1]}" in msg and "odd" in msg and "NULL" not in msg
        with pytest.raises(ValueError):                                     # the model's bounds are the library's
            Z.check_window(*bad)
    assert lib.psm_sgm_download_census(None, 0, None) != 0


class _Recorder:
    """stands where the loaded library stands in a DispEst: every psm_* call is recorded and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args[1:]))
            return 0
        return call


def _fake(dispest, maxDis=64, W=12, H=8):
    de = object.__new__(dispest.DispEst)
    de._lib, de._h, de.wid, de.hei, de.maxDis = _Recorder(), 1, W, H, maxDis
    return de


def test_the_python_keyword_reaches_the_call(built, monkeypatch):
    from primestereomatch_amd import dispest, harness
    for f in (dispest.DispEst.SGBM_GPU, dispest.sgbm_batch):
        assert inspect.signature(f).parameters["census"].default is None
    de = _fake(dispest)
    de.SGBM_GPU(census=(9, 7))
    names = [n for n, _ in de._lib.calls]
    assert ("psm_sgm_set_census", (9, 7)) in de._lib.calls and names.index("psm_sgm_set_census") < names.index("psm_sgm_compute")
    assert de.sgm_census(1).shape == (8, 12) and de.sgm_census(1).dtype == np.uint64
    for off in (None, (0, 0)):                                              # the setting is the call's: the default again
        del de._lib.calls[:]
        de.SGBM_GPU(census=off) if off else de.SGBM_GPU()
        assert ("psm_sgm_set_census", (0, 0)) in de._lib.calls
    des = [_fake(dispest) for _ in range(3)]
    monkeypatch.setattr(dispest, "sgm_compute_batch", lambda ds: None)
    assert len(dispest.sgbm_batch(des, census=(5, 5))) == 3
    for d in des:
        assert ("psm_sgm_set_census", (5, 5)) in d._lib.calls
    assert "census" in harness.compute_sgbm.__doc__


def test_header_and_host_carry_the_census():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"int psm_sgm_set_census\(psm_ctx \*ctx, int win_w, int win_h\);", text)
    assert re.search(r"int psm_sgm_download_census\(psm_ctx \*ctx, int side, uint64_t \*codes\);", text)
    block = text[text.index("A third pixel cost"):text.index("int psm_sgm_set_census(")]
    for phrase in ("1868 B + 9617 G + 4899 R + 8192) >> 14", "strictly", "replicated", "popcount", "3 <= win_w <= 9", "3 <= win_h <= 7",
                   "pre_filter_cap > 0", "16 * W * H", "No library's convention"):
        assert phrase in block, phrase
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    assert "setSGBMCensus(int winW, int winH)" in open(os.path.join(host, "DispEst.h")).read()
    assert '"sgbm_census"' in open(os.path.join(host, "psm_demo.cpp")).read()
