"""CPU: tests/sgm_range_model.py, the definition of the SGM stage under a disparity range (psm_sgm_set_range), held to
 - an independent scalar restatement (plain Python integers, one voxel at a time) on tiny pairs, W < D, min_disparity > W and
   min_disparity <= -W among them;
 - the three existing models at range (0, D): the result dictionaries are identical;
 - the slice identity: range (m >= 0, D) on C equals the slice [m, m + D) of the existing model's C at D' = m + D <= 256, and S
   likewise once the paths run over that slice;
 - a known answer: a right image that is the exact shift of a ramp texture by s, s negative and s > 256."""
import numpy as np
import pytest

import sgm_bt_model as B
import sgm_mode_model as MM
import sgm_model as M
import sgm_range_model as R

INF = 1 << 28


# ------------------------------------------------------------------------------------------------- the scalar restatement

def _clamp(v, n):
    return 0 if v < 0 else (n - 1 if v > n - 1 else v)


def _scalar_pixel_cost(L, Rt, dmin, D, cap):
    H, W, ch = L.shape
    c = [[[0] * D for _ in range(W)] for _ in range(H)]
    if cap == 0:
        for y in range(H):
            for x in range(W):
                for k in range(D):
                    xr = _clamp(x - (dmin + k), W)
                    c[y][x][k] = sum(abs(int(L[y, x, q]) - int(Rt[y, xr, q])) for q in range(ch))
        return c
    U, V = B.prefilter(L, cap).astype(int), B.prefilter(Rt, cap).astype(int)       # (the prefilter is sgm_bt_model's, untouched)
    n = 2 * ch

    def lo_hi(a, y, x, q):
        v = int(a[y, x, q])
        vl = (v + int(a[y, x - 1, q])) // 2 if x > 0 else v
        vr = (v + int(a[y, x + 1, q])) // 2 if x < W - 1 else v
        return min(v, vl, vr), max(v, vl, vr)
    for y in range(H):
        for x in range(W):
            for k in range(D):
                xr = _clamp(x - (dmin + k), W)
                t = 0
                for q in range(n):
                    u, v = int(U[y, x, q]), int(V[y, xr, q])
                    lu, hu = lo_hi(U, y, x, q)
                    lv, hv = lo_hi(V, y, xr, q)
                    c0 = max(0, u - hv, lv - u)
                    c1 = max(0, v - hu, lu - v)
                    t += min(c0, c1) >> (0 if q < ch else 2)
                c[y][x][k] = t
    return c


def scalar_sgm(L, Rt, dmin, D, directions, cap=0, bs=5, P1=0, P2=0, u=10, m=1):
    L, Rt = M._as3(L), M._as3(Rt)
    H, W, ch = L.shape
    P1 = P1 or 8 * ch * bs * bs
    P2 = P2 or 32 * ch * bs * bs
    c = _scalar_pixel_cost(L, Rt, dmin, D, cap)
    h = bs // 2
    C = [[[sum(c[_clamp(y + j, H)][_clamp(x + i, W)][k] for j in range(-h, h + 1) for i in range(-h, h + 1)) for k in range(D)]
          for x in range(W)] for y in range(H)]
    S = [[[0] * D for _ in range(W)] for _ in range(H)]
    for dy, dx in directions:
        Lr = [[None] * W for _ in range(H)]
        for y in (range(H) if dy >= 0 else range(H - 1, -1, -1)):
            for x in (range(W) if dx >= 0 else range(W - 1, -1, -1)):
                py, px = y - dy, x - dx
                if not (0 <= py < H and 0 <= px < W):
                    Lr[y][x] = list(C[y][x])
                else:
                    p = Lr[py][px]
                    mn = min(p)
                    Lr[y][x] = [C[y][x][k] + min(p[k], p[k - 1] + P1 if k > 0 else INF, p[k + 1] + P1 if k < D - 1 else INF, mn + P2) - mn
                                for k in range(D)]
                for k in range(D):
                    S[y][x][k] += Lr[y][x][k]
    inv = (dmin - 1) * 16
    best = [[0] * W for _ in range(H)]
    d16 = [[0] * W for _ in range(H)]
    unique = [[False] * W for _ in range(H)]
    land = [[None] * W for _ in range(H)]                      # (minS, best_k) of the winner, None: nothing landed
    for y in range(H):
        for x in range(W):
            s = S[y][x]
            b = min(range(D), key=lambda k: (s[k], k))
            best[y][x] = b
            unique[y][x] = not any(abs(k - b) > 1 and s[k] * (100 - u) < s[b] * 100 for k in range(D))
            v = 16 * (dmin + b)
            if 0 < b < D - 1:
                den = max(s[b - 1] + s[b + 1] - 2 * s[b], 1)
                v += ((s[b - 1] - s[b + 1]) * 16 + den) // (2 * den)
            d16[y][x] = v
            xl = x - (dmin + b)
            if unique[y][x] and 0 <= xl < W and (land[y][xl] is None or (s[b], b) < land[y][xl]):
                land[y][xl] = (s[b], b)
    disp = np.empty((H, W), np.int16)
    for y in range(H):
        for x in range(W):
            ok = unique[y][x]
            if ok and m >= 0:
                def bad(dq):
                    xq = x - dq
                    return 0 <= xq < W and land[y][xq] is not None and abs(dmin + land[y][xq][1] - dq) > m
                v = d16[y][x]
                ok = not (bad(v >> 4) and bad((v + 15) >> 4))          # (Python's >> floors)
            disp[y, x] = d16[y][x] if ok else inv
    return {"C": np.array(C), "S": np.array(S), "best": np.array(best), "d16": np.array(d16), "unique": np.array(unique), "disp": disp,
            "landed": np.array([[e is not None for e in row] for row in land])}


# (W, H, ch, min_disparity, D, mode, cap, extra): W < D | min > W | min <= -W (both: every column clamps) | straddling 0 | m off
TINY = [
    (5, 3, 3, -2, 7, "hh", 0, {}),
    (6, 4, 1, 9, 4, "hh", 0, {}),
    (5, 3, 3, -5, 3, "sgbm", 0, {}),
    (5, 4, 1, -9, 4, "3way", 63, {}),
    (7, 3, 3, 2, 9, "hh4", 31, dict(block_size=3)),
    (9, 3, 1, -3, 8, "hh", 15, dict(block_size=1, disp12_max_diff=0, uniqueness_ratio=0)),
    (8, 2, 3, -1, 3, "hh", 0, dict(block_size=3, disp12_max_diff=-1)),
    (4, 2, 1, 1024, 2, "hh", 0, {}),
    (4, 2, 1, -1024, 5, "hh", 1, {}),
]


@pytest.mark.parametrize("W,H,ch,dmin,D,mode,cap,extra", TINY)
def test_the_model_equals_a_scalar_restatement(W, H, ch, dmin, D, mode, cap, extra):
    rng = np.random.default_rng(W * 100 + D)
    shape = (H, W, ch) if ch == 3 else (H, W)
    l, r = rng.integers(0, 256, (2,) + shape, dtype=np.uint8)
    r = np.where(rng.random(shape) < 0.5, np.roll(l, -(dmin + D // 2), axis=1), r).astype(np.uint8)     # some columns do match
    ref = R.sgm(l, r, dmin, D, mode, pre_filter_cap=cap, **extra)
    kw = dict(bs=extra.get("block_size", 5), u=extra.get("uniqueness_ratio", 10), m=extra.get("disp12_max_diff", 1))
    got = scalar_sgm(l, r, dmin, D, MM.MODES[mode], cap, **kw)
    for k in ("C", "S", "best", "d16", "unique", "disp", "landed"):
        assert np.array_equal(ref[k], got[k]), k
    assert ref["invalid"] == (dmin - 1) * 16 and ref["disp"].dtype == np.int16
    assert not np.any(ref["valid"] & (ref["disp"] == ref["invalid"]))
    assert np.all(ref["disp2"][ref["landed"]] >= dmin) and np.all(ref["disp2"][~ref["landed"]] == dmin - 1)


def test_the_range_is_checked():
    l = np.zeros((4, 6), np.uint8)
    for dmin, D in ((-1025, 4), (1025, 4), (0, 1), (0, 1025)):
        with pytest.raises(ValueError):
            R.sgm(l, l, dmin, D)
    assert 16 * (R.MAX_MIN + R.MAX_D - 1) + 8 <= 32767 and R.invalid_value(-R.MAX_MIN) >= -32768


# ------------------------------------------------------------------------------------------------- the existing models at (0, D)

def _pair(W, H, D, seed, ch=3):
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=seed)
    if ch == 1:
        return np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
    return l, r


def _same(old, new):
    for k, v in old.items():
        if k == "planes":
            assert all(np.array_equal(a, b) for a, b in zip(v, new[k]))
        elif isinstance(v, np.ndarray):
            assert v.dtype == new[k].dtype and np.array_equal(v, new[k]), k
        else:
            assert v == new[k], k
    assert set(new) - set(old) == {"landed", "invalid", "range"}
    assert np.array_equal(new["landed"], old["disp2"] >= 0) and new["invalid"] == M.INVALID


@pytest.mark.parametrize("W,H,D,ch", [(40, 12, 16, 3), (23, 9, 33, 1), (12, 8, 30, 3)])
def test_range_0_D_is_the_existing_models(W, H, D, ch):
    l, r = _pair(W, H, min(D, W), W, ch)
    _same(M.sgm(l, r, D), R.sgm(l, r, 0, D))
    _same(M.sgm(l, r, D, block_size=3, uniqueness_ratio=0, disp12_max_diff=0), R.sgm(l, r, 0, D, block_size=3, uniqueness_ratio=0,
                                                                                      disp12_max_diff=0))
    _same(B.sgm(l, r, D, pre_filter_cap=63), R.sgm(l, r, 0, D, pre_filter_cap=63))
    for mode in ("sgbm", "3way", "hh4", 1):
        _same(MM.sgm(l, r, D, mode), R.sgm(l, r, 0, D, mode))
    _same(MM.sgm(l, r, D, "3way", pre_filter_cap=15), R.sgm(l, r, 0, D, "3way", pre_filter_cap=15))


# ------------------------------------------------------------------------------------------------- slices of the existing model

@pytest.mark.parametrize("W,H,m,D,cap", [(40, 10, 5, 20, 0), (30, 9, 45, 16, 0), (37, 8, 16, 64, 63), (24, 8, 200, 56, 0)])
def test_a_non_negative_minimum_is_a_slice_of_the_existing_model(W, H, m, D, cap):
    """x - (m + k) >= -(m + k): for delta >= 0 the right clamp never acts, so C is the old C's slice; S is the old aggregate of
    that slice (the paths see only the range's disparities)."""
    assert m + D <= 256
    rng = np.random.default_rng(m)
    l, r = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    old = B.sgm(l, r, m + D, pre_filter_cap=cap)
    new = R.sgm(l, r, m, D, pre_filter_cap=cap)
    assert np.array_equal(new["C"], old["C"][:, :, m:m + D])
    bs, P1, P2, u, mm = old["params"]
    assert np.array_equal(new["S"], M.aggregate(np.ascontiguousarray(old["C"][:, :, m:m + D]), P1, P2))
    best, minS, unique, d16 = M.select(new["S"], u)
    assert np.array_equal(new["d16"], d16 + 16 * m) and np.array_equal(new["unique"], unique)


# ------------------------------------------------------------------------------------------------- a known answer

def ramp_pair(W, H, s):
    """A ramp texture (37 x + 11 y + 50 ch mod 256: no two columns within 255 of each other agree) and its exact shift: the left
    pixel x shows what the right image shows at x - s, wherever x - s is a column."""
    y, x, q = np.mgrid[0:H, 0:W + abs(s), 0:3]
    wide = ((37 * x + 11 * y + 50 * q) % 256).astype(np.uint8)
    if s >= 0:                                                   # L[x] = wide[x] = R[x - s]
        return np.ascontiguousarray(wide[:, :W]), np.ascontiguousarray(wide[:, s:s + W])
    return np.ascontiguousarray(wide[:, -s:-s + W]), np.ascontiguousarray(wide[:, :W])   # L[x] = wide[x + |s|] = R[x + |s|]


@pytest.mark.parametrize("W,H,s,dmin,D,cap", [(60, 8, -5, -12, 20, 0), (60, 8, -5, -12, 20, 63), (340, 6, 260, 250, 32, 0), (48, 8, 3, -4, 12, 0)])
def test_an_exact_shift_is_found(W, H, s, dmin, D, cap):
    l, r = ramp_pair(W, H, s)
    x = np.arange(W)
    inside = (x - s >= 0) & (x - s < W)
    assert np.array_equal(l[:, inside], r[:, (x - s)[inside]])                                  # the pair is what it claims to be
    ref = R.sgm(l, r, dmin, D, pre_filter_cap=cap)
    # the columns whose whole 5 x 5 block, at every disparity of the range, reads right columns without a clamp
    core = (x - 2 - (dmin + D - 1) >= 0) & (x + 2 - dmin <= W - 1)
    assert core.sum() >= 8
    assert np.all(ref["C"][:, core, s - dmin] == 0)
    assert np.all(ref["best"][:, core] == s - dmin)
    assert np.all(ref["valid"][:, core])
    assert np.all(np.abs(ref["disp"][:, core].astype(int) - 16 * s) <= 8)
    if s < 0:
        assert np.all(ref["disp"][:, core] < 0)                  # valid and negative: validity is "!= invalid", never ">= 0"
