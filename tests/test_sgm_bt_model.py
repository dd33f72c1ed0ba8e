"""The numpy model of the SGM stage's prefiltered Birchfield-Tomasi cost (tests/sgm_bt_model.py) against an independent scalar
restatement of its definition, against known answers, and against the committed fixtures.  No GPU; all integer, no tolerance."""
import hashlib
import os

import numpy as np
import pytest

import sgm_bt_model as B
import sgm_model as M

from conftest import ROOT


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the definition once more, with plain loops and no helper of the model --------------------------------------------------
def scalar_planes(img, cap):
    H, W, ch = img.shape
    ft = max(cap, 15) | 1
    out = [[[0] * (2 * ch) for _ in range(W)] for _ in range(H)]
    for y in range(H):
        yn, ys = max(y - 1, 0), min(y + 1, H - 1)
        for x in range(W):
            for k in range(ch):
                if x == 0 or x == W - 1:
                    out[y][x][k] = ft
                    out[y][x][ch + k] = ft
                else:
                    g = (2 * (int(img[y][x + 1][k]) - int(img[y][x - 1][k])) + (int(img[yn][x + 1][k]) - int(img[yn][x - 1][k]))
                         + (int(img[ys][x + 1][k]) - int(img[ys][x - 1][k])))
                    out[y][x][k] = min(max(g, -ft), ft) + ft
                    out[y][x][ch + k] = int(img[y][x][k])
    return out


def scalar_lo_hi(row, x, n, W):
    a = row[x][n]
    al = (a + row[x - 1][n]) // 2 if x > 0 else a
    ar = (a + row[x + 1][n]) // 2 if x < W - 1 else a
    return min(a, al, ar), max(a, al, ar)


def scalar_cost(L, R, D, cap):
    H, W, ch = L.shape
    U, V = scalar_planes(L, cap), scalar_planes(R, cap)
    c = np.zeros((H, W, D), np.int32)
    for y in range(H):
        for x in range(W):
            for d in range(D):
                xr = max(x - d, 0)
                t = 0
                for n in range(2 * ch):
                    shift = 0 if n < ch else 2
                    u, v = U[y][x][n], V[y][xr][n]
                    lov, hiv = scalar_lo_hi(V[y], xr, n, W)
                    lou, hiu = scalar_lo_hi(U[y], x, n, W)
                    c0 = max(0, u - hiv, lov - u)
                    c1 = max(0, v - hiu, lou - v)
                    t += min(c0, c1) >> shift
                c[y, x, d] = t
    return np.array(U, np.uint8), np.array(V, np.uint8), c


# 9x5 D 4; 2x3 D 2: every column is a border column; 3x1 D 3: H = 1, both row neighbours are the row itself; 13x4 D 13: W = D
@pytest.mark.parametrize("W,H,D", [(9, 5, 4), (2, 3, 2), (3, 1, 3), (13, 4, 13)])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("cap", [1, 31, 63])
def test_model_equals_the_scalar_restatement(W, H, D, ch, cap):
    rng = np.random.default_rng(W * 1000 + H * 10 + ch + cap)
    L = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    U, V, c = scalar_cost(L, R, D, cap)
    assert np.array_equal(B.prefilter(L, cap), U) and np.array_equal(B.prefilter(R, cap), V)
    assert np.array_equal(B.pixel_cost_bt(L, R, D, cap), c)
    if ch == 1:                                           # a 2-d image is the 1-channel image
        assert np.array_equal(B.pixel_cost_bt(L[:, :, 0], R[:, :, 0], D, cap), c)


# ---- known answers -------------------------------------------------------------------------------------------------------------
def test_constant_63_costs_nothing():
    for ch in (1, 3):
        img = np.full((8, 12, ch), 63, np.uint8)
        assert not B.pixel_cost_bt(img, img, 6, 63).any()


def test_identical_images_cost_nothing_at_disparity_0():
    rng = np.random.default_rng(3)
    for ch in (1, 3):
        img = rng.integers(0, 256, (7, 15, ch), dtype=np.uint8)
        for cap in (1, 31, 63):
            assert not B.pixel_cost_bt(img, img, 5, cap)[:, :, 0].any()


def test_constant_200_meets_the_border_column():
    """The right border column holds 63, not 200: wherever x - d <= 0 < x the intensity plane costs (200 - (200 + 63) // 2) >> 2."""
    img = np.full((8, 12), 200, np.uint8)
    c = B.pixel_cost_bt(img, img, 6, 63)
    assert (200 - 263 // 2) >> 2 == 17
    x = np.arange(12)[None, :, None]
    d = np.arange(6)[None, None, :]
    hit = np.broadcast_to((x - d <= 0) & (x > 0), c.shape)
    assert np.all(c[hit] == 17)
    assert c[0, 3, 3] == 17 and c[0, 1, 1] == 17 and c[0, 5, 3] == 0


def test_ramp_planes():
    img = np.tile((4 * np.arange(40)).astype(np.uint8), (5, 1))
    p = B.prefilter(img, 63)
    assert p.shape == (5, 40, 2)
    assert np.all(p[:, :, 0] == np.array([63] + [95] * 38 + [63]))             # g = 4 * 8 = 32 -> 32 + 63
    assert np.all(p[:, :, 1] == np.array([63] + list(range(4, 156, 4)) + [63]))
    assert np.all(B.prefilter(img, 1)[:, :, 0] == np.array([15] + [30] * 38 + [15]))       # ft 15: g clipped to 15


def test_caps_that_share_a_threshold():
    assert [B.filter_threshold(c) for c in (1, 14, 15, 16, 17, 18, 62, 63)] == [15, 15, 15, 17, 17, 19, 63, 63]
    rng = np.random.default_rng(5)
    L = rng.integers(0, 256, (9, 20, 3), dtype=np.uint8)
    R = rng.integers(0, 256, (9, 20, 3), dtype=np.uint8)
    c = {cap: B.pixel_cost_bt(L, R, 8, cap) for cap in (1, 14, 15, 16, 17)}
    assert np.array_equal(c[1], c[15]) and np.array_equal(c[16], c[17])
    assert not np.array_equal(c[14], c[16])
    for cap in (0, 64, -1):
        with pytest.raises(ValueError):
            B.filter_threshold(cap)


def test_cap_0_is_the_sad_stage():
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(40, 20, 12, seed=2)
    a, b = B.sgm(l, r, 12, pre_filter_cap=0, block_size=3), M.sgm(l, r, 12, block_size=3)
    assert a.keys() == b.keys()
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(B.sgm(l, r, 12, pre_filter_cap=63, block_size=3)["C"], b["C"])


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("cap", [1, 31, 63])
def test_cost_bound_on_binary_noise(ch, cap):
    """c <= ch (2 ft + 63): a P plane contributes at most 2 ft, a Q plane at most 255 >> 2 = 63 - so the condition
    bs^2 ch 255 + P2 <= 65535 still keeps a path cost in 16 bits."""
    rng = np.random.default_rng(ch + cap)
    L = (rng.integers(0, 2, (24, 40, ch)) * 255).astype(np.uint8)
    R = (rng.integers(0, 2, (24, 40, ch)) * 255).astype(np.uint8)
    ft = B.filter_threshold(cap)
    c = B.pixel_cost_bt(L, R, 16, cap)
    print(f"[sgm-bt-model] ch {ch} cap {cap}: max c {int(c.max())}, bound {ch * (2 * ft + 63)}")
    assert c.max() <= ch * (2 * ft + 63) < ch * 255
    P2 = 65535 - 49 * ch * 255
    o = B.sgm(L, R, 16, pre_filter_cap=cap, block_size=7, P1=100, P2=P2)
    assert o["C"].dtype == np.uint16 and int(o["C"].max()) <= 49 * ch * (2 * ft + 63)
    assert o["max_l"] <= 65535


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def middlebury(golden):
    out = {}
    for name in ("cones", "teddy"):
        p = golden(f"{name}_pair.npz")
        out[name] = (p, B.sgm(p["l_bgr"], p["r_bgr"], 64, pre_filter_cap=63))
    return out


# what a second writing of the definition gave: max C, max S, valid pixels, the first 16 hex digits of SHA-256 of C, S and the map
SECOND_WRITING = {"cones": (7708, 80864, 153439, "628aa0cd52e3e2d7", "c148addf58a9cd27", "32dc9259e7d1f23c"),
                  "teddy": (8059, 83672, 152643, "23c80bf9df61cc95", "8368f3b2112a533f", "66bb477551539c27")}


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_model_is_pinned_to_the_fixtures_and_the_second_writing(middlebury, golden, name):
    _, o = middlebury[name]
    g = golden(f"{name}_sgm_bt.npz")
    assert g["disp"].dtype == np.int16 and np.array_equal(o["disp"], g["disp"])
    assert np.array_equal(o["best"], g["best"]) and np.array_equal(o["valid"], g["valid"].astype(bool))
    assert sha(o["C"]) == str(g["sha_C"]) and sha(o["S"]) == str(g["sha_S"])
    assert sha(o["planes"][0]) == str(g["sha_planes_l"]) and sha(o["planes"][1]) == str(g["sha_planes_r"])
    assert o["planes"][0].shape == o["disp"].shape + (6,) and o["planes"][0].dtype == np.uint8
    max_c, max_s, valid, hc, hs, hm = SECOND_WRITING[name]
    got = (int(o["C"].max()), int(o["S"].max()), int(o["valid"].sum()), sha(o["C"])[:16], sha(o["S"])[:16], sha(o["disp"])[:16])
    print(f"[sgm-bt-model] {name}: {got}")
    assert got == (max_c, max_s, valid, hc, hs, hm)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"{name}_sgm_bt.npz")) < 1 << 20


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_quality_against_the_sad_cost(middlebury, golden, name):
    """%BP of `best` under the occlusion mask (harness.error_vs_ground_truth(best, gt_l, occl, 64, 4)): 4.76 / 10.14 against the
    SAD cost's 4.97 / 10.46."""
    from primestereomatch_amd import harness
    p, o = middlebury[name]
    bp = harness.error_vs_ground_truth(o["best"], p["gt_l"], p["occl"], 64, 4)[0]
    sad = harness.error_vs_ground_truth(golden(f"{name}_sgm.npz")["best"], p["gt_l"], p["occl"], 64, 4)[0]
    print(f"[sgm-bt-model] {name}: %BP of best {bp:.2f} (SAD cost {sad:.2f})")
    assert round(bp, 2) == {"cones": 4.76, "teddy": 10.14}[name] and bp < sad
