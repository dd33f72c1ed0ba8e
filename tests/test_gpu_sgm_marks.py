"""-m gpu: what a compute of the SGM stage leaves behind - the map and the marks that decide which of the stage's downloads answer
(psm_sgm_download_prefiltered, _census, _speckle_sizes, psm_sgm_times, psm_sgm_speckle_time) - through a walk that alternates
single pairs and batches, the three pixel costs, the gray path, the speckle filter and PSM_OPT_PROFILE on two contexts.  Single
pairs and batches go through one launch sequence in psm_api_sgm.cpp; this file pins that both leave a context in the same state.
40 x 24 with 16 disparities: two 32-column cost tiles with a remainder, 2 x 3 census tiles of 32 x 8, one disparity per lane
downstream.  Everything is integer: 0 differing elements, no tolerance anywhere in this file."""
import functools

import numpy as np
import pytest

import sgm_bt_model as B
import sgm_census_model as Z
import sgm_model as M
import speckle_model as K

pytestmark = pytest.mark.gpu

W, H, D = 40, 24, 16
SEEDS = (0, 1)
SPECKLE = dict(speckle_window_size=20, speckle_range=2)       # small enough to remove pixels of both maps at this size
PAD = 6             # the strided downloads: bytes between two rows


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@functools.lru_cache(maxsize=None)
def pair(seed):
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=seed)
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


@functools.lru_cache(maxsize=None)
def model(kind, seed):
    """The model's result for pair(seed) under one of the walk's settings: computed once, shared, read-only."""
    l, r = pair(seed)
    if kind == "sad":
        ref = M.sgm(l, r, D)
    elif kind == "census":
        ref = Z.sgm(l, r, 0, D, census=(5, 5))
    elif kind == "bt_gray":
        ref = B.sgm(np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1]), D, pre_filter_cap=63)
    else:
        ref = B.sgm(l, r, D, pre_filter_cap=63)
        ref["filtered"], ref["sizes"] = K.sgbm_speckle(ref["disp"], SPECKLE["speckle_window_size"], SPECKLE["speckle_range"])
        assert not np.array_equal(ref["filtered"], ref["disp"])
    ref["disp"].setflags(write=False)
    return ref


def answers(psm, call):
    """True: the download succeeded; False: it was refused with a message of its own."""
    try:
        call()
        return True
    except psm.capi.PsmError:
        return False


def check(psm, step, de, disp, planes=None, census=None, sizes=None, times=False, speckle_time=False):
    """The state of one context: its map equals `disp`; planes / census / sizes: the model's arrays where that download has to
    answer, None where it has to be refused; times / speckle_time: whether those two answer."""
    got = de.sgm_disparity()
    n = int(np.count_nonzero(got != disp))
    print(f"[sgm-marks] {step}: differing map elements {n}")
    assert got.dtype == np.int16 and n == 0
    for side in (0, 1):
        if planes is None:
            assert not answers(psm, lambda: de.sgm_prefiltered(side)), step
            assert "psm_sgm_download_prefiltered" in psm.capi.last_error(de._h)
        else:
            p = de.sgm_prefiltered(side)
            assert p.shape == planes[side].shape and np.array_equal(p, planes[side]), step
        if census is None:
            assert not answers(psm, lambda: de.sgm_census(side)), step
            assert "psm_sgm_download_census" in psm.capi.last_error(de._h)
        else:
            assert np.array_equal(de.sgm_census(side), census[side]), step
    if sizes is None:
        assert not answers(psm, de.sgm_speckle_sizes), step
        assert "psm_sgm_download_speckle_sizes" in psm.capi.last_error(de._h)
    else:
        assert np.array_equal(de.sgm_speckle_sizes(), sizes), step
    assert answers(psm, de.sgm_times) == times, step
    assert answers(psm, de.sgm_speckle_time) == speckle_time, step
    if times:
        assert all(t > 0 for t in de.sgm_times()), step
    if speckle_time:
        assert de.sgm_speckle_time() > 0, step


def test_the_marks_a_compute_leaves(psm):
    from primestereomatch_amd import dispest
    des = [psm.DispEst(*pair(s), D) for s in SEEDS]
    a, b = des
    sad, cen, gray, bt = ([model(k, s) for s in SEEDS] for k in ("sad", "census", "bt_gray", "bt"))
    try:
        # 1: colour SAD, single - context 1 has no result at all
        a.SGBM_GPU()
        check(psm, "1 single SAD, context 0", a, sad[0]["disp"])
        assert not answers(psm, b.sgm_disparity) and "psm_sgm_download_disparity" in psm.capi.last_error(b._h)

        # 2: colour census 5 x 5, batch of 2 - the codes are there on both contexts
        maps = dispest.sgbm_batch(des, census=(5, 5))
        for i, de in enumerate(des):
            assert np.array_equal(maps[i], cen[i]["disp"])
            check(psm, f"2 batch census, context {i}", de, cen[i]["disp"], census=cen[i]["codes"])

        # 3: gray Birchfield-Tomasi, single - 2 x 1 planes; context 1 stays where the batch left it
        l, r = pair(SEEDS[0])
        a.SGBM_GPU(gray=(np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])), pre_filter_cap=63)
        assert gray[0]["planes"][0].shape == (H, W, 2)
        check(psm, "3 single gray BT, context 0", a, gray[0]["disp"], planes=gray[0]["planes"])
        check(psm, "3 single gray BT, context 1", b, cen[1]["disp"], census=cen[1]["codes"])

        # 4: colour Birchfield-Tomasi with the speckle filter, batch of 2 - 2 x 3 planes and the component sizes
        maps = dispest.sgbm_batch(des, pre_filter_cap=63, **SPECKLE)
        for i, de in enumerate(des):
            assert bt[i]["planes"][0].shape == (H, W, 6) and np.array_equal(maps[i], bt[i]["filtered"])
            check(psm, f"4 batch BT + speckle, context {i}", de, bt[i]["filtered"], planes=bt[i]["planes"], sizes=bt[i]["sizes"])

        # 5: colour SAD, single, timed - the filter is off again: no filter time, but the sizes of step 4 are still the last run's
        a.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        a.SGBM_GPU()
        check(psm, "5 single SAD timed, context 0", a, sad[0]["disp"], sizes=bt[0]["sizes"], times=True)
        check(psm, "5 single SAD timed, context 1", b, bt[1]["filtered"], planes=bt[1]["planes"], sizes=bt[1]["sizes"])

        # a timed batch counts as timed on context 0 only - also where context 1's own last compute was timed
        b.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        b.SGBM_GPU()
        check(psm, "single SAD timed, context 1", b, sad[1]["disp"], sizes=bt[1]["sizes"], times=True)
        maps = dispest.sgbm_batch(des, pre_filter_cap=63, **SPECKLE)
        check(psm, "batch timed, context 0", a, bt[0]["filtered"], planes=bt[0]["planes"], sizes=bt[0]["sizes"], times=True, speckle_time=True)
        check(psm, "batch timed, context 1", b, bt[1]["filtered"], planes=bt[1]["planes"], sizes=bt[1]["sizes"])
    finally:
        for d in des:
            d.close()


def test_a_refused_batch_leaves_both_previous_maps(psm):
    from primestereomatch_amd import dispest
    des = [psm.DispEst(*pair(s), D) for s in SEEDS]
    try:
        a, b = des
        a.SGBM_GPU(census=(5, 5))
        b.SGBM_GPU(pre_filter_cap=63)
        before = [a.sgm_disparity(), b.sgm_disparity()]
        for de in des:                                     # one setting for both, then context 1 alone leaves it
            for setter, args in ((de._lib.psm_sgm_set_census, (0, 0)), (de._lib.psm_sgm_set_prefilter, (0,))):
                assert setter(de._h, *args) == 0
        assert b._lib.psm_sgm_set_mode(b._h, 0) == 0
        with pytest.raises(psm.capi.PsmError, match=r"context 1 has another mode \(0\) than context 0 \(1\)"):
            dispest.sgm_compute_batch(des)
        # nothing was enqueued and nothing forgotten: both contexts are where their own computes left them
        check(psm, "refused batch, context 0", a, model("census", 0)["disp"], census=model("census", 0)["codes"])
        check(psm, "refused batch, context 1", b, model("bt", 1)["disp"], planes=model("bt", 1)["planes"])
        assert np.array_equal(a.sgm_disparity(), before[0]) and np.array_equal(b.sgm_disparity(), before[1])
    finally:
        for d in des:
            d.close()


def test_strided_downloads_leave_the_padding_alone(psm):
    from primestereomatch_amd.dispest import _ptr
    ref = model("bt", 0)
    with psm.DispEst(*pair(0), D) as de:
        de.SGBM_GPU(pre_filter_cap=63, **SPECKLE)
        for name, fn, want in (("disparity", de._lib.psm_sgm_download_disparity, ref["filtered"]),
                               ("speckle sizes", de._lib.psm_sgm_download_speckle_sizes, ref["sizes"].astype(np.int32))):
            row = W * want.dtype.itemsize
            buf = np.full((H, row + PAD), 0xa5, np.uint8)
            de._ck(fn(de._h, _ptr(buf), row + PAD), name)
            got = np.ascontiguousarray(buf[:, :row]).view(want.dtype)
            print(f"[sgm-marks] strided {name}: differing elements {int(np.count_nonzero(got != want))}")
            assert np.array_equal(got, want) and np.all(buf[:, row:] == 0xa5)
            packed = np.empty((H, W), want.dtype)          # stride 0: the row size, the direct copy
            de._ck(fn(de._h, _ptr(packed), 0), name)
            assert np.array_equal(packed, want)
            assert fn(de._h, _ptr(buf), row - 1) != 0 and "stride" in psm.capi.last_error(de._h)
