"""CPU checks of tests/sgm_maps_model.py, the definition of psm_sgm_select_maps: the vectorised form against a per-pixel brute force
on dense ties, constant and shifted pairs, and - on the Cones / Teddy goldens - the bad-pixel counts of the model's maps through
the oracle's post-processing chain, pinned as integers."""
import numpy as np
import pytest

import sgm_maps_chain as K
import sgm_maps_model as MM
import sgm_model as M


# (H, W, D, dmin): W < D, columns without a candidate, D no multiple of anything
@pytest.mark.parametrize("H,W,D,dmin", [(3, 20, 64, 0), (4, 33, 7, 3), (2, 9, 2, 8), (2, 5, 40, 6)])
def test_model_equals_the_brute_force_on_dense_ties(H, W, D, dmin):
    S = np.random.default_rng([H, W, D, dmin]).integers(0, 6, (H, W, D)).astype(np.uint32)
    lm, rm = MM.maps(S, dmin)
    lb, rb = MM.maps_brute(S, dmin)
    assert lm.dtype == rm.dtype == np.uint8
    assert np.array_equal(lm, lb) and np.array_equal(rm, rb)
    if dmin:
        assert np.all(rm[:, max(W - dmin, 0):] == 0)               # the columns without a candidate
        assert np.all(rm[:, :max(W - dmin, 0)] >= dmin)


@pytest.mark.parametrize("dmin,D,max_disp", [(-1, 16, 64), (40, 40, 64), (0, 257, 257), (1, 256, 257)])
def test_ranges_outside_the_definition_are_refused(dmin, D, max_disp):
    with pytest.raises(ValueError):
        MM.maps(np.zeros((2, 4, D), np.uint32), dmin, max_disp)


@pytest.mark.parametrize("dmin", [0, 3])
def test_constant_images_give_the_minimum_disparity(dmin):
    img = np.full((6, 20, 3), 77, np.uint8)
    S = M.sgm(img, img, 8)["S"]
    assert not S.any()
    lm, rm = MM.maps(S, dmin)
    assert np.all(lm == dmin)
    assert np.all(rm[:, :20 - dmin] == dmin) and np.all(rm[:, 20 - dmin:] == 0)


def test_a_shifted_pair_recovers_the_shift_in_both_views():
    W, H, D, k = 48, 12, 16, 5
    l = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = np.ascontiguousarray(l[:, np.clip(np.arange(W) + k, 0, W - 1)])          # L[x] = R[x - k]
    lm, rm = MM.maps(M.sgm(l, r, D)["S"])
    assert np.all(lm[:, D:] == k)                                   # left pixels whose match is inside the image
    assert np.all(rm[:, :W - D] == k)                               # right pixels whose every candidate is


@pytest.fixture(scope="module")
def middlebury(golden):
    out = {}
    for name in ("cones", "teddy"):
        p = golden(f"{name}_pair.npz")
        out[name] = (p, M.aggregate(M.block_cost(M.pixel_cost(p["l_bgr"], p["r_bgr"], 64), 5), 8 * 75, 32 * 75))
    return out


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_the_chain_on_the_goldens_gives_the_pinned_counts(middlebury, golden, oracle, name):
    p, S = middlebury[name]
    lm, rm = MM.maps(S)
    assert np.array_equal(lm, golden(f"{name}_sgm.npz")["best"])   # the stage's own winner-takes-all
    c = K.chain(oracle, p["l_bgr"], lm, rm, 64)
    got = tuple(K.bad_pixels(oracle, m, p["gt_l"], p["occl"], 64) for m in (lm, c["lfill"], c["lmed"]))
    print(f"[sgm-maps-model] {name}: bad pixels WTA / + lrCheck + fillInv / + wgtMedian {got} of {K.PIXELS}")
    assert got == K.SAD_COUNTS[name]
