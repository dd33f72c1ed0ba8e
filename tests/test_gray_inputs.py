"""tests/gray_inputs.py held to its own conditions, on the model alone (no GPU): what keeps tests/test_gpu_gray_adversarial.py from
passing vacuously.  Every condition is asserted for the full-resolution form (s = 0) and for the Fast Guided Filter at s = 2, 4, 8,
each at its own size, and for both sides.

Counted here (mixed | every slice NaN, of the image's pixels; left side, right side), seed 0:
                 s = 0 (70 x 19)         s = 2 (102 x 27)          s = 4 (118 x 38)          s = 8 (150 x 52)
  nan_pos        838 | 463, 650 | 522    1100 | 1654, 968 | 1765   2222 | 2262, 1645 | 2707  4017 | 3731, 2629 | 4618
  nan_neg, pinf, ninf: the same counts (a special value of any kind makes the same planes NaN)
  overflow       225 | 195, 225 | 248    712 | 806, 972 | 753      1142 | 1120, 1520 | 1187  2249 | 1482, 2600 | 2018
  all            946 | 359, 974 | 332    1293 | 1461, 1289 | 1439  2938 | 1546, 2374 | 1891  5146 | 2456, 4264 | 2986
  of             1330                    2754                      4484                      7800
Seam ties (left, right, of): periodic 884, 935 of 1632 (s = 0); 731, 765 of 1632 (2); 986, 986 of 1904 (4); 1156, 1292 of 2176 (8);
periodic70 1445, 1462 of 2720 (0); 1275, 1275 of 2720 (2); 1530, 1598 of 2992 (4); 1700, 1762 of 3264 (8).
Negative minima (left, right, of 1330): 1330, 1330 (0); 1330, 1330 (2); 1307, 1329 (4); 1250, 1330 (8).
"""
import numpy as np
import pytest

import gray_inputs as GI
import gray_model as M

FORMS = GI.FORMS
SIDES = (0, 1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _oracle_built(oracle):
    """the model's box is the oracle's"""


# ------------------------------------------------------------------------------------------------------------ the pairs themselves

@pytest.mark.parametrize("s", FORMS)
@pytest.mark.parametrize("kind", GI.PLANTED)
def test_planted_values_are_in_both_planes_on_and_off_the_border(kind, s):
    W, H, D = GI.size(kind, s)
    l, r = GI.pair(kind, s)
    cl, cr = GI.pair("clean", s, like=kind)
    want = sorted(int(v) for v in bits(np.array(GI.VALUES[kind])))
    for plane, clean, where in zip((l, r), (cl, cr), GI.sites(W, H, s)):
        changed = np.argwhere(bits(plane) != bits(clean))
        where = where[:GI.NSITES[kind]]
        assert sorted(map(tuple, changed.tolist())) == sorted(where), (kind, s)
        assert sorted(set(int(bits(plane)[y, x]) for y, x in where)) == want, (kind, s)          # every value of the kind, bit for bit
        edge = [y in (0, H - 1) or x in (0, W - 1) for y, x in where]
        assert any(edge) and not all(edge), (kind, s, where)
        assert all(y in GI.sampled(H, s) and x in GI.sampled(W, s) for y, x in where if (y, x) != (H - 1, W - 1))      # the subsampling reads them
    (yl, xl), (yr, xr) = GI.sites(W, H, s)[0][0], GI.sites(W, H, s)[1][0]
    assert yl == yr and 1 <= xl - xr < D and bits(l)[yl, xl] == bits(r)[yr, xr]                  # the aligned pair
    assert not l.flags.writeable and not r.flags.writeable
    assert GI.pair(kind, s)[0] is l                                                              # cached


def test_the_two_nan_patterns():
    assert int(bits(GI.pair("nan_pos")[0]).max()) == 0x7FC00000 and int(bits(GI.pair("nan_neg")[0]).max()) == 0xFFC00000
    l, r = GI.pair("all_slices")
    assert np.all(bits(l) == 0xFFC00000) and np.all(bits(r) == 0x7FC00000)
    l, r = GI.pair("left_nan")
    assert np.all(bits(l) == 0xFFC00000) and np.all(np.isfinite(r))
    with np.errstate(all="ignore"):
        assert 3e19 < np.finfo(np.float32).max and np.isinf(np.float32(3e19) * np.float32(3e19))


# --------------------------------------------------------------------------------------------------------------------- mixed pixels

@pytest.mark.parametrize("s", FORMS)
@pytest.mark.parametrize("kind", GI.PLANTED)
def test_a_tenth_of_the_pixels_have_nan_and_finite_slices(kind, s):
    for side in SIDES:
        c = GI.census(kind, s, side)
        print(f"{kind} s={s} side {side}: mixed {c['mixed']}  every slice NaN {c['dead']}  of {c['total']}")
        assert 10 * c["mixed"] >= c["total"], (kind, s, side, c)
        assert c["dead"] > 0, (kind, s, side, c)                    # and some pixels have no candidate at all


@pytest.mark.parametrize("s", FORMS)
def test_the_overflow_pair_is_finite_and_its_guidance_is_not(s):
    l, r = GI.pair("overflow", s)
    assert np.isfinite(l).all() and np.isfinite(r).all()
    for side in SIDES:
        q = GI.volume("overflow", s, side)[0]
        d = GI.align_d(*GI.size("overflow", s)[:2], s)
        y, x = GI.sites(*GI.size("overflow", s)[:2], s)[side][0]
        assert np.isfinite(q[d, y, x]) and np.isnan(np.delete(q[1:, y, x], d - 1)).all(), (s, side)      # the aligned slice alone


# --------------------------------------------------------------------------------------------------------------------- map-0 pixels

@pytest.mark.parametrize("s", FORMS)
def test_map_zero_pixels(s):
    for m in GI.maps("all_slices", s):
        assert not m.any()
    for side in SIDES:
        assert GI.census("all_slices", s, side)["dead"] == m.size
        m, c = GI.maps("all", s)[side], GI.census("all", s, side)
        none = np.isnan(GI.volume("all", s, side)[0][1:]).all(axis=0)
        assert none.any() and not none.all() and not m[none].any() and m[~none].all(), (s, side)      # 0 exactly where no slice is a candidate
        assert c["dead"] == int(none.sum())
    lm, rm = GI.maps("left_nan", s)
    W = lm.shape[1]
    assert not lm.any() and not rm[:, :W // 4].any() and rm[:, -1].all()


@pytest.mark.parametrize("s", FORMS)
@pytest.mark.parametrize("kind", ["nan_neg", "all"])
def test_a_selection_that_lets_a_nan_win_gives_other_maps(kind, s):
    """the failure the GPU tests are after, played through on the model: the 64-bit key order with 0xFFC00000 below every cost"""
    for side in SIDES:
        q = GI.volume(kind, s, side)[0]
        b = np.ascontiguousarray(q + np.float32(0)).view(np.int32)
        hi = b ^ ((b >> 31) & 0x7FFFFFFF)                            # negative floats: magnitude bits flipped, the sign bit kept
        key = hi.astype(np.int64) * 256 + np.arange(q.shape[0])[:, None, None]
        key[0] = np.iinfo(np.int64).max                             # slice 0 is no candidate
        wrong = (np.minimum(key.min(axis=0), np.int64(0x7F800000) * 256) % 256).astype(np.uint8)      # the start: (+inf, 0)
        sign_set = np.isnan(q[1:]) & (bits(q[1:]) >> 31 == 1)
        finite_keys = GI.maps(kind, s)[side]
        if kind == "nan_neg" and s == 0:
            assert sign_set.any()                                    # the planted NaN's sign reaches q (the form that keys every slice)
        if sign_set.any():
            assert not np.array_equal(wrong, finite_keys), (kind, s, side)
        else:
            assert np.array_equal(wrong, finite_keys), (kind, s, side)      # without one, the key order is the model's


# ----------------------------------------------------------------------------------------------------------------------- seam ties

@pytest.mark.parametrize("s", FORMS)
@pytest.mark.parametrize("kind", list(GI.TIE))
def test_seam_ties(kind, s):
    W, H, D = GI.size(kind, s)
    assert all(d < D for d in GI.TIE[kind]) and len({(d - 1) // 32 for d in GI.TIE[kind]}) == len(GI.TIE[kind])      # one per chunk
    for side in SIDES:
        tie = GI.ties(kind, s, side)
        n = int(np.count_nonzero(tie))
        print(f"{kind} s={s} side {side}: slices {GI.TIE[kind]} tie at the minimum in {n} of {tie.size} pixels")
        assert 4 * n >= tie.size, (kind, s, side, n)
        assert np.all(GI.maps(kind, s)[side][tie] <= 3), (kind, s, side)


def test_periodic_bytes_are_the_float_planes(oracle):
    for kind in GI.TIE:
        for u8, f32 in zip(GI.as_bytes(kind), GI.pair(kind)):
            assert u8.dtype == np.uint8 and set(np.unique(u8)) == {0, 255}
            assert np.array_equal(bits(M.to_f32(u8)), bits(f32))
        l = GI.pair(kind)[0]
        assert np.array_equal(l[:, :32], l[:, 32:64]) and all(np.array_equal(row, l[0]) or np.array_equal(row, 1 - l[0]) for row in l)
        assert len({tuple(row) for row in l}) == 2                                               # rows of both polarities


# ----------------------------------------------------------------------------------------------------------------- negative minima

@pytest.mark.parametrize("s", FORMS)
def test_negative_minima(s):
    l, r = GI.pair("negative", s)
    assert np.isfinite(l).all() and np.isfinite(r).all()
    for side in SIDES:
        q = GI.volume("negative", s, side)[0]
        assert np.isfinite(q).all()
        mn = GI.minimum("negative", s, side)
        n = int(np.count_nonzero(mn < 0))
        print(f"negative s={s} side {side}: the minimum is below zero in {n} of {mn.size} pixels, {len(np.unique(mn[mn < 0]))} distinct values")
        assert 4 * n >= mn.size, (s, side, n)
        assert 2 * len(np.unique(mn[mn < 0])) >= n                                               # not one value over and over


def test_results_are_cached_and_read_only():
    a = GI.maps("all", 4)
    assert GI.maps("all", 4)[0] is a[0] and not a[0].flags.writeable
    v = GI.volume("all", 4, 1)
    assert GI.volume("all", 4, 1)[0] is v[0] and not v[0].flags.writeable and not v[1].flags.writeable
    with pytest.raises(ValueError):
        a[0][0, 0] = 1
