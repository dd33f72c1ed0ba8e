"""tests/score_model.py, the definition of the score stage, against what the package computes on the host today
(harness.error_vs_ground_truth, harness._finish_sgbm): every returned value, on the committed Cones / Teddy results and on seeded
random maps; the mask step over its whole table; the flat-map case, which is the model's own statement.  No GPU."""
import numpy as np
import pytest

import score_model as S

from primestereomatch_amd import harness

PAIRS = ("cones", "teddy")
GIF_RAW_WTA_BP = {"cones": 14.50, "teddy": 19.83}      # README.md; tests/test_gpu_parity.py pins the same figures


def _harness_gif(lmap, gt, mask, D, scale, thr):
    bp, avg, bad, emap = harness.error_vs_ground_truth(lmap, gt, mask, D, scale, thr)
    disp = harness._finish({"lDisMap": lmap}, D, None, None, scale, thr, False)["lDispMap"]
    return disp, emap, bp, avg, bad


def _same_gif(lmap, gt, mask, D, scale, thr):
    disp, emap, bp, avg, bad = _harness_gif(lmap, gt, mask, D, scale, thr)
    m = S.score(S.GIF, lmap, gt, mask, D, scale, thr)
    assert np.array_equal(m["ldisp"], disp) and np.array_equal(m["emap"], emap)
    assert (m["bad"], m["bp_percent"], m["avg_err"]) == (bad, bp, avg)
    assert m["err_sum"] == int(emap.astype(np.int64).sum()) and m["pixels"] == emap.size and m["unit"] == 127 // D
    return m


def _same_sgm(d16, gt, mask, D, scale, thr):
    h = harness._finish_sgbm({"disp16": d16}, D, gt, mask, scale, thr, False)
    m = S.score(S.SGM, d16, gt, mask, D, scale, thr)
    assert np.array_equal(m["ldisp"], h["lDispMap"])
    assert (m["min_val"], m["max_val"], m["flags"]) == (int(d16.min()), int(d16.max()), 0)
    if gt is not None:
        assert (m["bad"], m["bp_percent"], m["avg_err"]) == (h["bad_pixels"], h["bp_percent"], h["avg_err"])
        # the metric ran on the display map as it is, scale 1
        assert np.array_equal(m["emap"], harness.error_vs_ground_truth(h["lDispMap"], gt, mask, D, 1, thr)[3])
        assert S.score(S.SGM_INT, d16, gt, mask, D, scale, thr)["bp_percent"] == h["bp_percent_int"]
    return m


@pytest.mark.parametrize("name", PAIRS)
@pytest.mark.parametrize("masked", (True, False))
def test_gif_goldens(golden, name, masked):
    pair, lmap = golden(f"{name}_pair.npz"), golden(f"{name}_oracle_d64.npz")["ldisp"]
    m = _same_gif(lmap, pair["gt_l"], pair["occl"] if masked else None, 64, 4, 4)
    if masked:
        assert round(m["bp_percent"], 2) == GIF_RAW_WTA_BP[name]


@pytest.mark.parametrize("name", PAIRS)
@pytest.mark.parametrize("masked", (True, False))
def test_sgm_goldens(golden, name, masked):
    pair, d16 = golden(f"{name}_pair.npz"), golden(f"{name}_sgm.npz")["disp"]
    _same_sgm(d16, pair["gt_l"], pair["occl"] if masked else None, 64, 4, 4)
    _same_sgm(d16, None, None, 64, 4, 4)


def test_seeded_random_maps():
    rng = np.random.default_rng(20240611)
    for i in range(24):
        H, W = int(rng.integers(3, 40)), int(rng.integers(9, 150))
        D = int(rng.choice([2, 8, 16, 64, 127, 128, 200, 256]))
        scale, thr = int(rng.choice([1, 3, 4, 16, 255])), int(rng.choice([0, 1, 4, 30, 255]))
        gt = rng.integers(0, 256, (H, W)).astype(np.uint8)
        mask = None if i % 3 == 0 else rng.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (H, W))
        _same_gif(rng.integers(0, 256, (H, W)).astype(np.uint8), gt, mask, D, scale, thr)
        lo = int(rng.integers(-17000, 1000))
        d16 = rng.integers(lo, int(rng.integers(lo + 2, 17000)), (H, W)).astype(np.int16)
        _same_sgm(d16, gt, mask, D, scale, thr)


def test_mask_step_whole_table():
    """Every (e, k): the model's integers against the harness's expression, and against exact rational rounding where the float
    factor cannot matter (e * k a multiple of 255)."""
    e, k = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = S.mask_step(e, k)
    ref = np.clip(np.rint(e.astype(np.int32) * k.astype(np.float64) * float(np.float32(1 / 255.0))), 0, 255).astype(np.int64)
    assert np.array_equal(got, ref)
    exact = (e * k) % 255 == 0
    assert np.array_equal(got[exact], (e * k)[exact] // 255)
    assert got[255, 255] == 255 and got[0].max() == 0 and got[:, 0].max() == 0
    assert np.array_equal(got[:, 255], np.arange(256))                                   # a full mask value keeps the error
    assert np.all(np.abs(got - e * k / 255.0) <= 0.5 + 1e-6)
    # the metric applies it, and PSM_MASK_DISC first drops every value up to 254
    p, g = e.astype(np.uint8), np.zeros((256, 256), np.uint8)
    emap, bad, err_sum, unit = S.metric(p, g, k.astype(np.uint8), 128, 0, S.MASK_NONOCC)
    assert unit == 0 and np.array_equal(emap[:, 129:], got[:, 129:]) and emap[:, :129].max() == 0
    disc = S.metric(p, g, k.astype(np.uint8), 128, 0, S.MASK_DISC)[0]
    assert disc[:, :255].max() == 0 and np.array_equal(disc[:, 255], np.arange(256))
    assert np.array_equal(S.metric(p, g, k.astype(np.uint8), 128, 0, S.MASK_NONE)[0][:, 129:], p[:, 129:])


def test_flat_map_is_the_models_own_statement():
    for v in (-16, 0, 800, (-1024 - 1) * 16):
        d16 = np.full((4, 64), v, np.int16)
        gt = np.full((4, 64), 9, np.uint8)
        m = S.score(S.SGM, d16, gt, None, 16, 4, 0)
        assert m["flags"] == S.FLAT and (m["min_val"], m["max_val"]) == (v, v)
        assert not m["ldisp"].any()
        assert m["bad"] == 4 * (64 - 17) and m["err_sum"] == 9 * m["bad"] and m["unit"] == 7
    assert S.score(S.SGM, np.array([[0, 1] * 32] * 4, np.int16), None, None, 16)["flags"] == 0


def test_display_roundings():
    """cvRound is ties-to-even in both steps; negative products saturate to 0; there is no offset."""
    d16 = np.array([[-16, 0, 510, 1020, 10, 14, 40, 56] * 8] * 4, np.int16)             # max - min = 1036
    assert S.display_sgm(np.array([[0, 10, 14, 255]], np.int16), 1)[0].tolist() == [[0, 2, 4, 64]]   # alpha 1: 10 / 4 -> 2, 14 / 4 -> 4
    disp, mn, mx, flags = S.display_sgm(d16, 4)
    assert (mn, mx, flags) == (-16, 1020, 0) and disp[0, 0] == 0
    assert S.display_u8(np.array([0, 63, 64, 255], np.uint8), 4).tolist() == [0, 252, 255, 255]
    assert S.display_sgm_int(np.array([-16, 15, 16, 1023 * 16 + 8], np.int16), 3).tolist() == [0, 0, 3, 255]


def test_unit_and_columns():
    p = np.full((3, 300), 200, np.uint8)
    g = np.zeros((3, 300), np.uint8)
    for D, unit in ((2, 63), (64, 1), (127, 1), (128, 0), (256, 0)):
        emap, bad, err_sum, u = S.metric(p, g, None, D, 1)
        assert u == unit and bad == 3 * (300 - D - 1) and emap[:, :D + 1].max() == 0
        rec = {"bad": bad, "err_sum": err_sum, "pixels": 900, "unit": u}
        assert S.figures(rec)[1] == ((err_sum / 900) / u if u else 0.0)
    assert S.metric(p[:, :65], g[:, :65], None, 64, 0)[1] == 0 and S.metric(p[:, :66], g[:, :66], None, 64, 0)[1] == 3
