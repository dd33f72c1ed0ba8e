"""The model of the SGM stage's modes (tests/sgm_mode_model.py) - the definition tests/test_gpu_sgm_modes.py holds the device to -
against an independent scalar restatement with the direction lists written out here, a known answer, sgm_model itself for "hh",
and the figures of the Middlebury fixtures.  CPU only; everything is integer."""
import numpy as np
import pytest

import sgm_bt_model as B
import sgm_mode_model as MM
import sgm_model as M
from test_sgm_model import scalar_sgm

# the direction lists, written out a second time (dy, dx): the step from the predecessor to the pixel
WRITTEN_OUT = {
    "sgbm": [(0, 1), (0, -1), (1, 0), (1, 1), (1, -1)],
    "hh": [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)],
    "3way": [(0, 1), (0, -1), (1, 0)],
    "hh4": [(0, 1), (0, -1), (1, 0), (-1, 0)],
}
OPENCV_ENUM = {"sgbm": 0, "hh": 1, "3way": 2, "hh4": 3}

# Cones / Teddy at D 64, default parameters, SAD cost: (max S, valid pixels, map elements != HH's, bp_percent_int)
FIGURES = {
    "hh": ((120960, 153174, 0, 9.20), (137272, 151721, 0, 13.90)),
    "sgbm": ((75600, 153413, 89990, 10.61), (85795, 154056, 100654, 13.64)),
    "3way": ((45360, 154423, 89033, 9.45), (51477, 155897, 100181, 12.12)),
    "hh4": ((60480, 153574, 71262, 8.77), (68636, 153492, 84360, 13.04)),
}
MAX_L = (15120, 17159)          # the largest single-path cost of the two pairs


def test_the_table_of_modes():
    assert set(MM.MODES) == set(WRITTEN_OUT) | set(OPENCV_ENUM.values())
    for name, dirs in WRITTEN_OUT.items():
        assert list(MM.MODES[name]) == dirs and MM.MODES[OPENCV_ENUM[name]] is MM.MODES[name]
        assert MM.VALUES[name] == OPENCV_ENUM[name]
    with pytest.raises(KeyError):
        MM.sgm(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8), 2, "hh8")


@pytest.mark.parametrize("mode", ["sgbm", "3way", "hh4", "hh"])
@pytest.mark.parametrize("W,H,D,ch,kw", [
    (9, 7, 6, 3, {}), (5, 6, 8, 3, dict(block_size=3)),            # the second: W < D
    (11, 5, 4, 1, dict(block_size=1, P1=3, P2=40)), (10, 6, 5, 3, dict(block_size=3, P1=20, P2=20, uniqueness_ratio=0, disp12_max_diff=-1)),
    (12, 1, 5, 3, dict(block_size=3)), (1, 9, 2, 1, {}), (2, 3, 2, 1, dict(block_size=1))])
def test_model_equals_the_scalar_restatement(W, H, D, ch, kw, mode):
    rng = np.random.default_rng(W * 100 + H)
    L = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    R = np.roll(L, -2, axis=1) if W > 4 else rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    R = (R.astype(np.int32) + rng.integers(-6, 7, R.shape)).clip(0, 255).astype(np.uint8)
    if ch == 1:
        L, R = L[:, :, 0], R[:, :, 0]
    o = MM.sgm(L, R, D, mode, **kw)
    bs, P1, P2, u, m = o["params"]
    C, S, best, disp = scalar_sgm(L, R, D, bs, P1, P2, u, m, directions=WRITTEN_OUT[mode])
    assert np.array_equal(o["C"], C) and np.array_equal(o["S"], S)
    assert np.array_equal(o["best"], best) and np.array_equal(o["disp"], disp)
    by_value = MM.sgm(L, R, D, OPENCV_ENUM[mode], **kw)
    assert np.array_equal(by_value["S"], o["S"]) and np.array_equal(by_value["disp"], o["disp"])


@pytest.mark.parametrize("mode", ["sgbm", "hh", "3way", "hh4"])
def test_constant_pair_gives_zero_everywhere(mode):
    for ch in (1, 3):
        img = np.full((20, 30, ch), 93, np.uint8)
        o = MM.sgm(img, img, 16, mode)
        assert not o["C"].any() and not o["S"].any()
        assert not o["disp"].any() and o["valid"].all()


def test_hh_is_sgm_model_itself():
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(70, 31, 20, seed=3)
    for kw in ({}, dict(block_size=3, uniqueness_ratio=0), dict(P1=7, P2=700, disp12_max_diff=-1)):
        a, b = MM.sgm(l, r, 20, "hh", **kw), M.sgm(l, r, 20, **kw)
        assert a.keys() == b.keys()
        for k in ("C", "S", "best", "unique", "valid", "d16", "disp2", "disp"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        assert a["max_l"] == b["max_l"] and a["params"] == b["params"]
    # ... and with the prefiltered cost, sgm_bt_model's
    a, b = MM.sgm(l, r, 20, "hh", pre_filter_cap=63), B.sgm(l, r, 20, pre_filter_cap=63)
    assert np.array_equal(a["C"], b["C"]) and np.array_equal(a["S"], b["S"]) and np.array_equal(a["disp"], b["disp"])
    assert all(np.array_equal(p, q) for p, q in zip(a["planes"], b["planes"]))


def test_a_reduced_mode_sums_the_paths_of_its_directions():
    rng = np.random.default_rng(5)
    C = rng.integers(0, 900, (7, 9, 6)).astype(np.uint16)
    for name, dirs in WRITTEN_OUT.items():
        want = sum(M.path_cost(C, r, 11, 70).astype(np.int64) for r in dirs)
        assert np.array_equal(M.aggregate(C, 11, 70, directions=MM.MODES[name]), want)


@pytest.fixture(scope="module")
def middlebury(golden):
    """Both pairs in every mode - computed once for the tests below."""
    out = {}
    for i, name in enumerate(("cones", "teddy")):
        p = golden(f"{name}_pair.npz")
        out[name] = (i, p, {mode: MM.sgm(p["l_bgr"], p["r_bgr"], 64, mode) for mode in FIGURES})
    return out


@pytest.mark.parametrize("mode", ["hh", "sgbm", "3way", "hh4"])
@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_figures_of_the_middlebury_pairs(middlebury, golden, name, mode):
    from primestereomatch_amd import harness
    i, p, runs = middlebury[name]
    o = runs[mode]
    max_s, valid, differing, bp = FIGURES[mode][i]
    got_bp = harness.error_vs_ground_truth(np.maximum(o["disp"], 0) >> 4, p["gt_l"], p["occl"], 64, 4)[0]
    got = (int(o["S"].max()), int(o["valid"].sum()), int(np.count_nonzero(o["disp"] != runs["hh"]["disp"])), round(float(got_bp), 2))
    print(f"[sgm-modes] {name} {mode}: max S {got[0]}  valid {got[1]}  != hh {got[2]}  bp_percent_int {got_bp:.2f}  max L_r {o['max_l']}")
    assert got == (max_s, valid, differing, bp)
    # the analytic check: every direction reaches the largest single-path cost at the same voxel of these pairs
    assert o["max_l"] == MAX_L[i] and max_s == len(MM.MODES[mode]) * MAX_L[i]
    if mode == "hh":
        assert np.array_equal(o["disp"], golden(f"{name}_sgm.npz")["disp"])
