"""tests/gray_fgf_model.py, the definition of psm_gray_compute_fgf, checked on the CPU: its three OpenCV primitives against the
committed oracle (bit for bit), the model against a float64 evaluation of the same formulas (transcription errors), what the
aggregation buys on Cones / Teddy at every rate (quality), its selection (oracle.wta), and that every kind of content the GPU tests
compare as bit patterns gives finite planes."""
import numpy as np
import pytest

import gray_fgf_model as F
import gray_model as M

RATES = (2, 4, 8)
# (W, H): the sizes the primitives are pinned at; the squares are the smallest each rate accepts (10: s = 2, 12: s = 4, 16: s = 8)
PRIM_SIZES = [(67, 45), (131, 70), (450, 375), (10, 10), (12, 12), (16, 16)]
# (W, H, D): noise shapes of the float64 comparison
SHAPES = [(16, 16, 2), (67, 45, 16), (131, 70, 33), (150, 37, 130)]


def noise_pair(W, H, seed=None):
    rng = np.random.default_rng(1000 * W + H if seed is None else seed)
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


def green(golden, name):
    z = golden(name + "_pair.npz")
    return np.ascontiguousarray(z["l_bgr"][:, :, 1]), np.ascontiguousarray(z["r_bgr"][:, :, 1]), z


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------- primitives against the oracle

@pytest.mark.parametrize("s", RATES)
@pytest.mark.parametrize("W,H", PRIM_SIZES)
def test_primitives_are_the_oracles(oracle, W, H, s):
    if not F.accepted(W, H, s):
        assert W in (10, 12) and s > (2 if W == 10 else 4)      # only the small squares fall below a rate's bound
        return
    k = 2 * (8 // s) + 1
    p = np.random.default_rng([W, H, s]).random((H, W), dtype=np.float32)
    # zero guidance: the covariances are 0, so a = 0 and b = mean_p - the filter is up(blur(blur(nn(p))))
    zero = np.zeros((H, W, 3), np.float32)
    want = oracle.fgf_filter(zero, oracle.fgf_setup(zero, s), p, s)
    got = F.up(F.blur(F.blur(F.nn(p, s), k), k), H, W)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    # the plane tripled into three channels: [0] is the subsampled channel, [3] its mean
    setup = oracle.fgf_setup(np.ascontiguousarray(np.repeat(p[:, :, None], 3, axis=2)), s)
    assert np.array_equal(bits(setup[0]), bits(F.nn(p, s)))
    assert np.array_equal(bits(setup[3]), bits(F.blur(F.nn(p, s), k)))


# -------------------------------------------------------------------------------------- the model against its float64 evaluation

def max_dq(slice32, l, r, D, s):
    """max |q32 - q64| over both sides and every slice; slice32(side_object, d) is the fp32 evaluation under test."""
    worst = 0.0
    for side in (0, 1):
        s32, s64 = F.Side(l, r, side, s, F.F32), F.Side(l, r, side, s, F.F64)
        for d in range(D):
            worst = max(worst, float(np.max(np.abs(slice32(s32, d).astype(np.float64) - s64.slice(d)))))
    return worst


# Measured here (fp32 model against the float64 evaluation), per rate.  8-bit noise, the four SHAPES in order:
#   s = 2: 7.6e-8, 1.6e-7, 2.5e-7, 2.4e-7     s = 4: 1.4e-7, 1.7e-7, 2.7e-7, 2.6e-7     s = 8: 1.8e-7, 1.3e-6, 8.3e-7, 3.8e-6
# (at s = 8 the 3 x 3 window sees nine pixels: den comes close to its 1e-4 floor far more often, and 1 / den amplifies the rounding
# of the covariance); the green planes of Cones and Teddy at D = 64, both sides, for the same reason in their flat regions.
# The bound is four times the largest measured value, tests/test_gray_model.py's convention.
NOISE_MEASURED = {2: 2.52e-7, 4: 2.68e-7, 8: 3.80e-6}
PAIR_MEASURED = {("cones", 2): 3.54e-6, ("cones", 4): 2.08e-5, ("cones", 8): 5.10e-5,
                 ("teddy", 2): 1.00e-5, ("teddy", 4): 1.83e-5, ("teddy", 8): 1.09e-4}


@pytest.mark.parametrize("s", RATES)
@pytest.mark.parametrize("W,H,D", SHAPES)
def test_transcription_noise(oracle, W, H, D, s):
    l, r = noise_pair(W, H)
    got = max_dq(lambda sd, d: sd.slice(d), l, r, D, s)
    print(f"{W}x{H}x{D} s={s}: max|dq| = {got:.3e} (bound {4 * NOISE_MEASURED[s]:.3e})")
    assert got <= 4 * NOISE_MEASURED[s]


@pytest.mark.parametrize("s", RATES)
@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_transcription_pairs(oracle, golden, name, s):
    l, r, _ = green(golden, name)
    got = max_dq(lambda sd, d: sd.slice(d), l, r, 64, s)
    print(f"{name} s={s}: max|dq| = {got:.3e} (bound {4 * PAIR_MEASURED[name, s]:.3e})")
    assert got <= 4 * PAIR_MEASURED[name, s]


@pytest.mark.parametrize("s", RATES)
def test_bound_catches_a_wrong_index_clamp_or_operand(oracle, s):
    """The bound means something: the same comparison of a model with one deliberate slip - a NN index off by one, `up` without
    the clamp at the far end, an operand of b - lies orders of magnitude outside it."""
    W, H, D = 67, 45, 16
    l, r = noise_pair(W, H)
    k = 2 * (8 // s) + 1

    def model(sd, ps, up=F.up, b_operand=None):
        mp, mIp = F.blur(ps, k), F.blur(sd.Is * ps, k)
        a = (mIp - sd.mI * mp) / sd.den
        b = mp - a * (sd.mI if b_operand is None else b_operand(mp))
        return up(F.blur(a, k), H, W) * sd.I + up(F.blur(b, k), H, W)

    def wrong_nn(sd, d):          # the cost sampled one column to the right of the NN map's
        p = sd.cost(d)
        xi = np.minimum(F.nn_index(W, s) + 1, W - 1)
        return model(sd, np.ascontiguousarray(p[np.ix_(F.nn_index(H, s), xi)]))

    def wrong_up(sd, d):          # no clamp at the far end: the last half cell extrapolates past the last sample
        def up(m, H_, W_):
            def axis(ssize, dsize):
                f = ((np.arange(dsize) + 0.5) * (float(ssize) / dsize) - 0.5).astype(np.float32)
                sx = np.floor(f).astype(np.int64)
                f = f - sx.astype(np.float32)
                f[sx < 0] = 0
                sx = np.maximum(sx, 0)
                return np.minimum(sx, ssize - 2), np.where(sx >= ssize - 1, f + np.float32(1.0), f).astype(np.float32)
            (sx, fx), (sy, fy) = axis(m.shape[1], W_), axis(m.shape[0], H_)
            rows = m[:, sx] * (np.float32(1) - fx)[None, :] + m[:, sx + 1] * fx[None, :]
            return rows[sy, :] * (np.float32(1) - fy)[:, None] + rows[sy + 1, :] * fy[:, None]
        return model(sd, F.nn(sd.cost(d), s), up=up)

    def wrong_operand(sd, d):     # b = mp - a mp instead of mp - a mI
        return model(sd, F.nn(sd.cost(d), s), b_operand=lambda mp: mp)

    bound = 4 * NOISE_MEASURED[s]
    right = max_dq(lambda sd, d: model(sd, F.nn(sd.cost(d), s)), l, r, D, s)
    assert right <= bound                                      # the harness of the slips is the model itself
    for slip in (wrong_nn, wrong_up, wrong_operand):
        got = max_dq(slip, l, r, D, s)
        print(f"s={s} {slip.__name__}: max|dq| = {got:.3e}")
        assert got > 100 * bound, slip.__name__


# ----------------------------------------------------------------------------------------------------------------------- quality

# left-map bad pixels under oracle.eval_bad_pixels(map, gt_l, occl, 64, 4) of the committed model: 14.40 / 18.05 / 28.06 % of Cones,
# 20.34 / 24.26 / 32.82 % of Teddy (the full gray filter: 16.01 / 20.24 %; the unaggregated cost: 59.05 / 61.05 %)
PINNED = {("cones", 2): 24295, ("cones", 4): 30464, ("cones", 8): 47346,
          ("teddy", 2): 34332, ("teddy", 4): 40940, ("teddy", 8): 55379}


_RAW_BAD = {}      # name -> bad pixels of the unaggregated cost: computed once, shared by the rates


@pytest.mark.parametrize("s", RATES)
@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_quality(oracle, golden, name, s):
    l, r, z = green(golden, name)
    lmap, _ = F.maps(l, r, 64, s)
    bad, _ = oracle.eval_bad_pixels(lmap, z["gt_l"], z["occl"], 64, 4)
    if name not in _RAW_BAD:
        raw, _ = M.maps_unaggregated(l, r, 64)
        _RAW_BAD[name] = oracle.eval_bad_pixels(raw, z["gt_l"], z["occl"], 64, 4)[0]
    bad_raw = _RAW_BAD[name]
    print(f"{name} s={s}: {bad} bad pixels ({100.0 * bad / lmap.size:.2f} %), unaggregated {bad_raw} ({100.0 * bad_raw / lmap.size:.2f} %)")
    assert 1.8 * bad <= bad_raw           # every rate beats the unaggregated cost by a factor of at least 1.8
    assert bad == PINNED[name, s]


# --------------------------------------------------------------------------------------------------------------------- selection

@pytest.mark.parametrize("s", RATES)
@pytest.mark.parametrize("W,H,D", SHAPES)
def test_selection_is_oracle_wta(oracle, W, H, D, s):
    l, r = noise_pair(W, H)
    lmap, rmap = F.maps(l, r, D, s)
    for side, got in ((0, lmap), (1, rmap)):
        assert np.array_equal(got, oracle.wta(F.volume(l, r, side, s, 0, D)))


@pytest.mark.parametrize("s", RATES)
def test_constant_pair_never_selects_slice_0(oracle, s):
    """On a constant pair every interior cost is 0 and every slice ties with every other wherever its windows see no border column.
    d = 0 is never a candidate, so nothing selects it although its slice is 0 everywhere; where slice 1 is exactly 0 - it ties with
    every slice whose windows see no border column either - the lowest candidate, 1, wins."""
    W, H, D = 40, 16, 8
    l = np.full((H, W), 77, np.uint8)
    lmap, rmap = F.maps(l, l.copy(), D, s)
    assert np.all(lmap >= 1) and np.all(rmap >= 1)
    for side, got in ((0, lmap), (1, rmap)):
        vol = F.volume(l, l.copy(), side, s, 0, D)
        assert np.all(vol[0] == 0)
        tie = (vol[1] == 0) & np.all(vol[1:] >= 0, axis=0)
        assert tie.any() and np.all(got[tie] == 1)


# ---------------------------------------------------------------------------------------------------------- finite model planes

def content_pairs(W, H):
    """every content kind tests/test_gpu_gray_fgf.py compares as bit patterns"""
    rng = np.random.default_rng([W, H, 5])
    fl = rng.uniform(-1024.0, 1024.0, (2, H, W)).astype(np.float32)
    return {"noise": tuple(rng.integers(0, 256, (2, H, W), dtype=np.uint8)),
            "binary": tuple(rng.integers(0, 2, (2, H, W)).astype(np.float32)),
            "constant": (np.full((H, W), 93, np.uint8), np.full((H, W), 93, np.uint8)),
            "float": (fl[0], fl[1]),
            "constant float": (np.full((H, W), 1000.3, np.float32), np.full((H, W), 1000.3, np.float32))}


@pytest.mark.parametrize("s", RATES)
def test_model_planes_are_finite(oracle, s):
    """0 / 0 gives NaNs of different sign on the host and on the device, so volumes are compared as bit patterns only on content
    for which this holds; the smallest den is 1e-4f (a variance that rounds to 0 or below it is possible, a den of 0 is not on
    these pairs)."""
    W, H, D = 131, 70, 16
    for kind, (l, r) in content_pairs(W, H).items():
        for side in (0, 1):
            sd = F.Side(l, r, side, s)
            assert np.all(np.isfinite(sd.planes())), (kind, side)
            assert np.all(sd.den != 0), (kind, side)
            q, model = F.volume(l, r, side, s, 0, D, want_model=True)
            assert np.all(np.isfinite(q)) and np.all(np.isfinite(model)), (kind, side)
        if kind == "constant":
            assert float(F.Side(l, r, 0, s).den.min()) <= float(np.float32(1e-4)) * 1.01
