"""The numpy model of the semi-global matching stage (tests/sgm_model.py) - the definition the device is compared with in
tests/test_gpu_sgm.py - against known answers, an independent scalar restatement, its own bounds, the quality relation to the
GIF path and the committed fixtures.  CPU only."""
import hashlib
import os
import sys

import numpy as np
import pytest

import sgm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# %BP of the GIF path's raw WTA left map under the non-occluded mask, D = 64: the figures tests/test_gpu_parity.py::
# test_harness_reproduces_reference_metric pins (and README.md quotes)
GIF_RAW_WTA_BP = {"cones": 14.50, "teddy": 19.83}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- an independent restatement: scalar loops straight from the text of the definition ----
def scalar_sgm(L, R, D, bs, P1, P2, u, m, directions=M.DIRECTIONS):
    L = L[:, :, None] if L.ndim == 2 else L
    R = R[:, :, None] if R.ndim == 2 else R
    H, W, ch = L.shape
    h = bs // 2
    cl = lambda v, n: min(max(v, 0), n - 1)
    c = [[[sum(abs(int(L[y][x][k]) - int(R[y][max(x - d, 0)][k])) for k in range(ch)) for d in range(D)] for x in range(W)] for y in range(H)]
    C = [[[sum(c[cl(y + j, H)][cl(x + i, W)][d] for j in range(-h, h + 1) for i in range(-h, h + 1)) for d in range(D)]
          for x in range(W)] for y in range(H)]
    S = [[[0] * D for _ in range(W)] for _ in range(H)]
    for dy, dx in directions:
        Lr = [[None] * W for _ in range(H)]
        for y in (range(H) if dy >= 0 else range(H - 1, -1, -1)):
            for x in (range(W) if dx >= 0 else range(W - 1, -1, -1)):
                py, px = y - dy, x - dx
                if not (0 <= py < H and 0 <= px < W):
                    Lr[y][x] = list(C[y][x])
                    continue
                p = Lr[py][px]
                mr = min(p)
                out = []
                for d in range(D):
                    t = [p[d], mr + P2]
                    if d > 0:
                        t.append(p[d - 1] + P1)
                    if d < D - 1:
                        t.append(p[d + 1] + P1)
                    out.append(C[y][x][d] + min(t) - mr)
                Lr[y][x] = out
        for y in range(H):
            for x in range(W):
                for d in range(D):
                    S[y][x][d] += Lr[y][x][d]
    best = [[min(range(D), key=lambda d: (S[y][x][d], d)) for x in range(W)] for y in range(H)]
    d16 = [[0] * W for _ in range(H)]
    uniq = [[True] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            b, s = best[y][x], S[y][x]
            uniq[y][x] = not any(abs(d - b) > 1 and s[d] * (100 - u) < s[b] * 100 for d in range(D))
            d16[y][x] = b * 16
            if 0 < b < D - 1:
                den = max(s[b - 1] + s[b + 1] - 2 * s[b], 1)
                d16[y][x] += ((s[b - 1] - s[b + 1]) * 16 + den) // (2 * den)
    disp = [[-16] * W for _ in range(H)]
    for y in range(H):
        land = {}
        for x in range(W):
            b = best[y][x]
            if uniq[y][x] and x - b >= 0:
                land[x - b] = min(land.get(x - b, (1 << 60, 0)), (S[y][x][b], b))
        disp2 = [land[x][1] if x in land else -1 for x in range(W)]
        for x in range(W):
            if not uniq[y][x]:
                continue
            ok = True
            if m >= 0:
                bad = lambda xq, dq: 0 <= xq < W and disp2[xq] >= 0 and abs(disp2[xq] - dq) > m
                da, db = d16[y][x] >> 4, (d16[y][x] + 15) >> 4
                ok = not (bad(x - da, da) and bad(x - db, db))
            if ok:
                disp[y][x] = d16[y][x]
    return np.array(C), np.array(S), np.array(best), np.array(disp)


@pytest.mark.parametrize("W,H,D,ch,kw", [
    (9, 7, 6, 3, {}), (5, 6, 8, 3, dict(block_size=3)),            # the second: W < D
    (11, 5, 4, 1, dict(block_size=1, P1=3, P2=40)), (8, 8, 7, 1, dict(block_size=7, uniqueness_ratio=40, disp12_max_diff=0)),
    (10, 6, 5, 3, dict(block_size=3, P1=20, P2=20, uniqueness_ratio=0, disp12_max_diff=-1)), (12, 1, 5, 3, dict(block_size=3)),
    (1, 9, 2, 1, {})])
def test_model_equals_the_scalar_restatement(W, H, D, ch, kw):
    rng = np.random.default_rng(W * 100 + H)
    L = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    R = np.roll(L, -2, axis=1) if W > 4 else rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    R = (R.astype(np.int32) + rng.integers(-6, 7, R.shape)).clip(0, 255).astype(np.uint8)
    if ch == 1:
        L, R = L[:, :, 0], R[:, :, 0]
    o = M.sgm(L, R, D, **kw)
    bs, P1, P2, u, m = o["params"]
    C, S, best, disp = scalar_sgm(L, R, D, bs, P1, P2, u, m)
    assert np.array_equal(o["C"], C) and np.array_equal(o["S"], S)
    assert np.array_equal(o["best"], best) and np.array_equal(o["disp"], disp)
    assert np.array_equal(o["disp"] >= 0, o["valid"])


def test_constant_pair_gives_zero_everywhere():
    for ch in (1, 3):
        img = np.full((20, 30, ch), 93, np.uint8)
        o = M.sgm(img, img, 16)
        assert not o["C"].any() and not o["S"].any()
        assert not o["disp"].any() and o["valid"].all()


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("k,D,bs", [(5, 16, 5), (0, 8, 3), (11, 24, 7), (3, 16, 1), (14, 16, 3)])
def test_right_image_as_the_exact_shift_of_the_left(k, D, bs, ch):
    """The right image is the left one shifted by k: R[y][x - k] = L[y][x].  On every pixel at least D + bs columns from the left
    edge and bs pixels from the other edges:
      - a ramp texture (costs symmetric about k: C(k + e) = C(k - e)) gives exactly 16 k;
      - a noise texture gives best = k, valid, and a sub-pixel term inside its range |d16 - 16 k| <= 8 - NOT 16 k on every pixel:
        the term is floor(((S(k-1) - S(k+1)) 16 + den) / (2 den)), zero only where the two neighbours' costs differ by less than
        den / 16, which independent noise does not give (measured on this model: 10 % to 100 % of such pixels sit at exactly 16 k,
        depending on block size and channel count)."""
    H, W = 40, 96
    rng = np.random.default_rng(k)
    inner = (slice(bs, H - bs), slice(D + bs, W - bs))
    # ramp: 2 per column, 1 per row, a different offset per channel; no wrap (2 * 110 + 40 + 30 < 256)
    x, y = np.arange(W + k)[None, :, None], np.arange(H)[:, None, None]
    full = (2 * x + y + 10 * np.arange(ch)[None, None, :]).astype(np.uint8)
    o = M.sgm(full[:, :W], full[:, k:], D, block_size=bs)
    assert (o["disp"][inner] == 16 * k).all()
    full = rng.integers(0, 256, (H, W + k, ch), dtype=np.uint8)
    o = M.sgm(full[:, :W], full[:, k:], D, block_size=bs)
    assert (o["best"][inner] == k).all() and o["valid"][inner].all()
    assert (np.abs(o["disp"][inner].astype(int) - 16 * k) <= 8).all()


def test_equal_penalties_reduce_to_a_two_term_minimum():
    rng = np.random.default_rng(7)
    H, W, D, P = 6, 9, 5, 37
    C = rng.integers(0, 500, (H, W, D)).astype(np.uint16)
    for dy, dx in M.DIRECTIONS:
        got = M.path_cost(C, (dy, dx), P, P)
        want = np.zeros((H, W, D), np.int64)
        for y in (range(H) if dy >= 0 else range(H - 1, -1, -1)):
            for x in (range(W) if dx >= 0 else range(W - 1, -1, -1)):
                py, px = y - dy, x - dx
                if 0 <= py < H and 0 <= px < W:
                    mr = want[py, px].min()
                    want[y, x] = C[y, x] + np.minimum(want[py, px], mr + P) - mr
                else:
                    want[y, x] = C[y, x]
        assert np.array_equal(got, want)


def test_one_direction_on_a_one_row_image():
    rng = np.random.default_rng(8)
    W, D, P1, P2 = 17, 6, 9, 50
    C = rng.integers(0, 300, (1, W, D)).astype(np.uint16)
    for dx in (1, -1):
        got = M.path_cost(C, (0, dx), P1, P2)[0]
        xs = list(range(W)) if dx > 0 else list(range(W - 1, -1, -1))
        prev = [int(v) for v in C[0, xs[0]]]
        assert list(got[xs[0]]) == prev
        for x in xs[1:]:
            mr = min(prev)
            cur = []
            for d in range(D):
                best = min(prev[d], mr + P2)
                if d > 0:
                    best = min(best, prev[d - 1] + P1)
                if d + 1 < D:
                    best = min(best, prev[d + 1] + P1)
                cur.append(int(C[0, x, d]) + best - mr)
            assert list(got[x]) == cur
            prev = cur
    # the vertical directions of a one-row image have no predecessor anywhere
    assert np.array_equal(M.path_cost(C, (1, 0), P1, P2), C) and np.array_equal(M.path_cost(C, (-1, 1), P1, P2), C)


def test_no_invalid_pixel_without_uniqueness_and_consistency():
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(80, 40, 24, seed=1)
    o = M.sgm(l, r, 24, uniqueness_ratio=0, disp12_max_diff=-1)
    assert o["valid"].all() and o["disp"].min() >= 0
    assert not M.sgm(l, r, 24)["valid"].all()              # (the defaults do reject pixels of this pair)


def test_parameter_conditions_are_rejected():
    img = np.zeros((8, 8, 3), np.uint8)
    for kw in (dict(block_size=2), dict(block_size=9), dict(P1=10, P2=9), dict(P1=-3), dict(block_size=7, P2=65535 - 49 * 3 * 255 + 1),
               dict(uniqueness_ratio=100), dict(uniqueness_ratio=-1)):
        with pytest.raises(ValueError):
            M.sgm(img, img, 4, **kw)
    M.sgm(img, img, 4, block_size=7, P2=65535 - 49 * 3 * 255)          # the boundary itself is inside
    for D in (1, 257):
        with pytest.raises(ValueError):
            M.sgm(img, img, D)
    with pytest.raises(ValueError):
        M.sgm(np.zeros((8, 8, 2), np.uint8), np.zeros((8, 8, 2), np.uint8), 4)
    assert M.resolve_params(3) == (5, 600, 2400, 10, 1) and M.resolve_params(1, 3) == (3, 72, 288, 10, 1)   # setupOpenCVSGBM's values


def test_quantise_is_convert_to_8u_255():
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(M.quantise(u.astype(np.float32) * np.float32(1 / 255.0)), u)     # the round trip of src/StereoMatch.cpp:195, 175
    f = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, -1.0, 2.0], np.float32)
    want = np.clip(np.rint(f * np.float32(255.0)), 0, 255).astype(np.uint8)
    assert np.array_equal(M.quantise(f), want) and want[-2] == 0 and want[-1] == 255


def test_quantise_sends_nan_to_0_and_infinities_to_the_ends():
    """The device's fminf(fmaxf(rintf(f * 255.0f), 0.0f), 255.0f): fmaxf(NaN, 0) is 0.  The model says so itself instead of leaving
    NaN to a float -> uint8 cast, as jwmf_model.feature_u8 does for its feature image."""
    f = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 1.0, np.nan], np.float32)
    with np.errstate(all="raise"):                           # no invalid cast on the way
        got = M.quantise(f)
    assert got.dtype == np.uint8 and got.tolist() == [0, 0, 255, 0, 0, 255, 0]
    img = np.full((3, 4, 3), np.nan, np.float32)
    assert not M.quantise(img).any() and not M._as3(img[:, :, 0]).any()


def test_display_map_rounds_as_opencv_does():
    d16 = np.array([[-16, 0, 160, 1008]], np.int16)          # alpha = 255 / 1024
    out = M.display_map(d16, 4)
    a = np.float32(255.0 / 1024.0)
    step1 = [0, 0, int(np.rint(np.float32(160) * a)), int(np.rint(np.float32(1008) * a))]
    assert list(out[0]) == [min(255, int(np.rint(v * 0.25)) * 4) for v in step1]
    assert np.rint(np.float32(10) * np.float32(0.25)) == 2 and np.rint(np.float32(14) * np.float32(0.25)) == 4   # ties to even


@pytest.fixture(scope="module")
def middlebury(golden):
    out = {}
    for name in ("cones", "teddy"):
        p = golden(f"{name}_pair.npz")
        out[name] = (p, M.sgm(p["l_bgr"], p["r_bgr"], 64))
    return out


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_bounds_hold_on_the_middlebury_pairs(middlebury, name):
    _, o = middlebury[name]
    bs, P1, P2, _, _ = o["params"]
    print(f"[sgm-model] {name}: max C {int(o['C'].max())}  max L_r {o['max_l']}  max S {int(o['S'].max())}")
    assert int(o["C"].max()) <= bs * bs * 3 * 255
    assert o["max_l"] <= int(o["C"].max()) + P2 <= 65535
    assert int(o["S"].max()) < 1 << 19


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_quality_beats_the_gif_paths_raw_wta(middlebury, name):
    from primestereomatch_amd import harness
    p, o = middlebury[name]
    bp = harness.error_vs_ground_truth(o["best"], p["gt_l"], p["occl"], 64, 4)[0]
    print(f"[sgm-model] {name}: %BP of the integer WTA {bp:.2f} (GIF raw WTA {GIF_RAW_WTA_BP[name]:.2f}), valid {o['valid'].mean():.3f}")
    assert bp < GIF_RAW_WTA_BP[name]


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_model_is_pinned_to_the_fixtures(middlebury, golden, name):
    _, o = middlebury[name]
    g = golden(f"{name}_sgm.npz")
    assert g["disp"].dtype == np.int16 and np.array_equal(o["disp"], g["disp"])
    assert np.array_equal(o["best"], g["best"]) and np.array_equal(o["valid"], g["valid"].astype(bool))
    assert sha(o["C"]) == str(g["sha_C"]) and sha(o["S"]) == str(g["sha_S"])
    for f in (f"{name}_sgm.npz",):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) < 1 << 20
