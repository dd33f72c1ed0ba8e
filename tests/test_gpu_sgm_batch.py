"""-m gpu: semi-global matching of several pairs in one set of launches (psm_sgm_compute_batch, dispest.sgbm_batch) against the
numpy models (tests/sgm_model.py, sgm_bt_model.py, speckle_model.py) and against SGBM_GPU on single objects.  Everything is
integer: C, S, the prefiltered planes, the speckle sizes and the int16 maps must be equal with 0 differing elements - there is
no tolerance anywhere in this file.  Every pair of a batch has a seed of its own, so a pair that read another's buffers cannot
pass."""
import functools
import hashlib

import numpy as np
import pytest

import sgm_bt_model as B
import sgm_model as M
import speckle_model as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def pair(W, H, D, seed):
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=seed)
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


@functools.lru_cache(maxsize=None)
def model(W, H, D, seed):
    """sgm_model.sgm of pair (W, H, D, seed) at the default parameters: computed once, shared by every test that needs it."""
    ref = M.sgm(*pair(W, H, D, seed), D)
    for k in ("C", "S", "disp"):
        ref[k].setflags(write=False)
    return ref


def differing(de, ref, disp):
    Cd, Sd = de.sgm_costs()
    return [int(np.count_nonzero(a != b)) for a, b in ((Cd, ref["C"]), (Sd, ref["S"]), (disp, ref["disp"]))]


def open_all(psm, pairs, D):
    return [psm.DispEst(l, r, D) for l, r in pairs]


def close_all(des):
    for d in des:
        d.close()


# one disparity per lane, partial | Dp = 64, the unpredicated ALL form | two per lane, ALL | four per lane, partial | W = D
SHAPES = [(67, 45, 16), (70, 9, 64), (136, 20, 128), (150, 37, 130), (33, 21, 33)]
CASES = [(W, H, D, n) for W, H, D in SHAPES for n in (1, 2, 3, 5)] + [(33, 21, 33, 9)]


@pytest.mark.parametrize("W,H,D,n", CASES)
def test_batches_equal_the_model(psm, W, H, D, n):
    from primestereomatch_amd import dispest
    des = open_all(psm, [pair(W, H, D, s) for s in range(n)], D)
    try:
        maps = dispest.sgbm_batch(des)
        assert len(maps) == n
        for s, (de, disp) in enumerate(zip(des, maps)):
            d = differing(de, model(W, H, D, s), disp)
            print(f"[sgm-batch] {W}x{H}x{D} n {n} pair {s}: differing elements C {d[0]}  S {d[1]}  map {d[2]}")
            assert disp.dtype == np.int16 and d == [0, 0, 0]
    finally:
        close_all(des)


SETTINGS = [dict(block_size=1), dict(block_size=3), dict(block_size=5), dict(block_size=7),
            dict(pre_filter_cap=63), dict(pre_filter_cap=17), dict(block_size=1, pre_filter_cap=63), dict(block_size=7, pre_filter_cap=63),
            dict(speckle_window_size=100, speckle_range=32), dict(speckle_window_size=5, speckle_range=1),
            dict(pre_filter_cap=63, speckle_window_size=100, speckle_range=32),
            dict(disp12_max_diff=-1), dict(uniqueness_ratio=0)]


@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_batch_equals_singles_under_every_setting(psm, kw):
    from primestereomatch_amd import dispest
    W, H, D, n = 93, 41, 24, 3
    pairs = [pair(W, H, D, 10 + s) for s in range(n)]
    cap = kw.get("pre_filter_cap", 0)
    win, rng = kw.get("speckle_window_size", 0), kw.get("speckle_range", 0)
    mkw = {k: v for k, v in kw.items() if k in ("block_size", "uniqueness_ratio", "disp12_max_diff")}
    des = open_all(psm, pairs, D)
    try:
        maps = dispest.sgbm_batch(des, **kw)
        for s, (de, disp) in enumerate(zip(des, maps)):
            l, r = pairs[s]
            ref = B.sgm(l, r, D, pre_filter_cap=cap, **mkw) if cap else M.sgm(l, r, D, **mkw)
            want, sizes = K.sgbm_speckle(ref["disp"], win, rng)
            with psm.DispEst(l, r, D) as one:
                single = one.SGBM_GPU(**kw)
                Cb, Sb = de.sgm_costs()
                C1, S1 = one.sgm_costs()
                assert np.array_equal(Cb, C1) and np.array_equal(Sb, S1) and np.array_equal(disp, single)
                assert np.array_equal(Cb, ref["C"]) and np.array_equal(Sb, ref["S"]) and np.array_equal(disp, want)
                if cap:
                    for side in (0, 1):
                        pb = de.sgm_prefiltered(side)
                        assert np.array_equal(pb, one.sgm_prefiltered(side)) and np.array_equal(pb, ref["planes"][side])
                else:
                    with pytest.raises(psm.capi.PsmError):
                        de.sgm_prefiltered(0)
                if win:
                    zb = de.sgm_speckle_sizes()
                    assert np.array_equal(zb, one.sgm_speckle_sizes()) and np.array_equal(zb, sizes)
                else:
                    with pytest.raises(psm.capi.PsmError):
                        de.sgm_speckle_sizes()
    finally:
        close_all(des)


def test_float_pairs_equal_the_8_bit_batch(psm):
    from primestereomatch_amd import dispest
    W, H, D, n = 93, 41, 24, 2
    pairs = [pair(W, H, D, 10 + s) for s in range(n)]
    fpairs = [tuple(a.astype(np.float32) * np.float32(1 / 255.0) for a in p) for p in pairs]      # src/StereoMatch.cpp:195-196
    d8, df = open_all(psm, pairs, D), open_all(psm, fpairs, D)
    try:
        m8 = dispest.sgbm_batch(d8, pre_filter_cap=63)
        mf = dispest.sgbm_batch(df, pre_filter_cap=63)
        for a, b, ma, mb in zip(d8, df, m8, mf):
            assert np.array_equal(ma, mb)
            for x, y in zip(a.sgm_costs() + (a.sgm_prefiltered(0), a.sgm_prefiltered(1)), b.sgm_costs() + (b.sgm_prefiltered(0), b.sgm_prefiltered(1))):
                assert np.array_equal(x, y)
        # a float pair beside an 8-bit one: another depth
        with pytest.raises(psm.capi.PsmError, match="context 1"):
            dispest.sgbm_batch([d8[0], df[1]], pre_filter_cap=63)
    finally:
        close_all(d8 + df)


@pytest.mark.parametrize("cap", [0, 63])
def test_cones_and_teddy_in_one_batch(psm, golden, cap):
    from primestereomatch_amd import dispest
    names = ["cones", "teddy"]
    ps = [golden(f"{n}_pair.npz") for n in names]
    gs = [golden(f"{n}_sgm_bt.npz" if cap else f"{n}_sgm.npz") for n in names]
    des = open_all(psm, [(p["l_bgr"], p["r_bgr"]) for p in ps], 64)
    try:
        maps = dispest.sgbm_batch(des, pre_filter_cap=cap)
        for name, de, disp, g in zip(names, des, maps, gs):
            Cd, Sd = de.sgm_costs()
            print(f"[sgm-batch] {name} cap {cap}: differing map elements {int(np.count_nonzero(disp != g['disp']))}")
            assert np.array_equal(disp, g["disp"])
            assert sha(Cd) == str(g["sha_C"]) and sha(Sd) == str(g["sha_S"])
    finally:
        close_all(des)


def test_frame_loop(psm):
    """Three frames through the same four contexts: new pairs, the batch, the downloads.  In the second round the pairs arrive
    with setInputImages_async and are adopted on each context's own stream (CostConst_GPU): the image slots swap, so a table that
    was not refreshed reads the previous frame's pairs, and a batch that did not wait for the members' streams reads slots the
    copies have not filled."""
    from primestereomatch_amd import dispest
    W, H, D, n = 67, 45, 16, 4
    des = open_all(psm, [pair(W, H, D, 0)] * n, D)
    try:
        for frame in range(3):
            seeds = [(frame + s) % 5 for s in range(n)]
            for de, s in zip(des, seeds):
                if frame == 1:
                    de.setInputImages_async(*pair(W, H, D, s))
                    de.CostConst_GPU()
                else:
                    de.setInputImages(*pair(W, H, D, s))
            maps = dispest.sgbm_batch(des)
            for de, s, disp in zip(des, seeds, maps):
                d = differing(de, model(W, H, D, s), disp)
                print(f"[sgm-batch] frame {frame} seed {s}: differing elements C {d[0]}  S {d[1]}  map {d[2]}")
                assert d == [0, 0, 0]
    finally:
        close_all(des)


def test_independence(psm):
    from primestereomatch_amd import dispest
    W, H, D, n = 67, 45, 16, 3
    des = open_all(psm, [pair(W, H, D, s) for s in range(n)], D)
    try:
        dispest.compute_batch(des)
        before = [tuple(m.copy() for m in de.download_maps()) for de in des]
        maps = dispest.sgbm_batch(des, speckle_window_size=100, speckle_range=32)
        for de, (lm, rm) in zip(des, before):
            lm2, rm2 = de.download_maps()
            assert np.array_equal(lm, lm2) and np.array_equal(rm, rm2)
        # a single compute with another pair on one member; the others keep their batch results
        des[1].setInputImages(*pair(W, H, D, 4))
        single = des[1].SGBM_GPU()
        assert differing(des[1], model(W, H, D, 4), single) == [0, 0, 0]
        for s in (0, 2):
            want, sizes = K.sgbm_speckle(model(W, H, D, s)["disp"], 100, 32)
            assert np.array_equal(des[s].sgm_disparity(), want) and np.array_equal(maps[s], want)
            assert differing(des[s], model(W, H, D, s), model(W, H, D, s)["disp"])[:2] == [0, 0]
            assert np.array_equal(des[s].sgm_speckle_sizes(), sizes)
        # the filter on a caller's map leaves a member's results alone
        f = des[0].filter_speckles(model(W, H, D, 2)["disp"], -16, 100, 512)
        assert np.array_equal(f, K.filter_speckles(model(W, H, D, 2)["disp"], -16, 100, 512)[0])
        assert np.array_equal(des[0].sgm_disparity(), maps[0])
        # the times of a batch are context 0's
        des[0].set_option(psm.capi.PSM_OPT_PROFILE, 1)
        dispest.sgbm_batch(des, speckle_window_size=100, speckle_range=32)
        assert all(t > 0 for t in des[0].sgm_times()) and des[0].sgm_speckle_time() > 0
        with pytest.raises(psm.capi.PsmError):
            des[1].sgm_times()
        with pytest.raises(psm.capi.PsmError):
            des[1].sgm_speckle_time()
    finally:
        close_all(des)


def test_shared_streams_and_async(psm):
    from primestereomatch_amd import dispest
    W, H, D, n = 67, 45, 16, 3
    des = open_all(psm, [pair(W, H, D, s) for s in range(n)], D)
    try:
        dispest.share_streams(des)
        des[0].set_option(psm.capi.PSM_OPT_ASYNC, 1)
        for _ in range(2):                                  # queued behind each other, no host synchronisation in between
            dispest.sgm_compute_batch(des)
        for s, de in enumerate(des):
            assert differing(de, model(W, H, D, s), de.sgm_disparity()) == [0, 0, 0]
    finally:
        close_all(des)


def refusal_cases(psm):
    W, H, D = 67, 45, 16
    l, r = pair(W, H, D, 1)

    def plain():
        return psm.DispEst(l, r, D)

    def other_width():
        return psm.DispEst(*pair(70, H, D, 1), D)

    def other_max_disp():
        return psm.DispEst(l, r, D + 4)

    def other_block_size():
        de = plain()
        de._ck(de._lib.psm_sgm_set_params(de._h, 3, 0, 0, 10, 1), "psm_sgm_set_params")
        return de

    def other_cap():
        de = plain()
        de._ck(de._lib.psm_sgm_set_prefilter(de._h, 63), "psm_sgm_set_prefilter")
        return de

    def other_speckle_window():
        de = plain()
        de._ck(de._lib.psm_sgm_set_speckle(de._h, 100, 32), "psm_sgm_set_speckle")
        return de

    def shard():
        return psm.DispEst(l, r, D, d_range=(0, D // 2))

    def stripe():
        de = plain()
        de.set_rows(8, 24)
        return de

    return [other_width, other_max_disp, other_block_size, other_cap, other_speckle_window, shard, stripe]


@pytest.mark.parametrize("case", range(7), ids=["width", "max_disp", "block_size", "pre_filter_cap", "speckle_window", "shard", "row_stripe"])
def test_refusals(psm, case):
    from primestereomatch_amd import dispest
    W, H, D = 67, 45, 16
    des = open_all(psm, [pair(W, H, D, s) for s in range(2)], D)
    odd = refusal_cases(psm)[case]()
    try:
        earlier = dispest.sgbm_batch(des)
        with pytest.raises(psm.capi.PsmError, match=r"context 2\b"):
            dispest.sgm_compute_batch(des + [odd])
        for s, de in enumerate(des):                        # nothing was enqueued, the earlier results are still there
            assert np.array_equal(de.sgm_disparity(), earlier[s])
            assert differing(de, model(W, H, D, s), earlier[s]) == [0, 0, 0]
    finally:
        close_all(des + [odd])


def test_refusals_repeated_and_without_a_pair(psm):
    import ctypes as C
    from primestereomatch_amd import dispest
    capi = psm.capi
    W, H, D = 67, 45, 16
    des = open_all(psm, [pair(W, H, D, s) for s in range(2)], D)
    h = C.c_void_p()
    try:
        earlier = dispest.sgbm_batch(des)
        with pytest.raises(capi.PsmError, match=r"context 2 appears twice"):
            dispest.sgm_compute_batch(des + [des[0]])
        lib = des[0]._lib
        assert lib.psm_create(C.byref(h), W, H, D, capi.PSM_F32, 0) == 0       # a context nothing was uploaded to
        arr = (C.c_void_p * 3)(des[0]._h, des[1]._h, h)
        assert lib.psm_sgm_compute_batch(arr, 3) != 0
        assert "context 2 has no image pair" in capi.last_error(des[0]._h)
        assert lib.psm_sgm_compute_batch(arr, 0) != 0 and lib.psm_sgm_compute_batch(arr, 4097) != 0
        arr[1] = None
        assert lib.psm_sgm_compute_batch(arr, 3) != 0
        assert "context 1 is NULL" in capi.last_error(des[0]._h)
        for s, de in enumerate(des):
            assert np.array_equal(de.sgm_disparity(), earlier[s])
    finally:
        if h.value:
            des[0]._lib.psm_destroy(h)
        close_all(des)


def test_sgm_only_async_frame_loop(psm):
    """construct(i) (adopts pair i); setInputImages_async(pair i + 1); SGBM(i) - no guided filter in between, PSM_OPT_ASYNC on, the
    host synchronises only in each frame's read-back.  The SGM stage reads the image slots and records that it has (images_read),
    so the copy into the slot of two frames ago is ordered behind it.  Every frame's map must be the model's for THAT frame's pair.
    This guards the mark; it cannot prove an ordering, and passes without the mark too unless the copy happens to overtake the
    stage - the proof is the code: one function, called by every reader."""
    W, H, D, frames = 67, 45, 16, 5
    with psm.DispEst(*pair(W, H, D, 0), D) as de:
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        de.setInputImages_async(*pair(W, H, D, 0))
        for i in range(frames):
            de.CostConst_GPU()
            if i + 1 < frames:
                de.setInputImages_async(*pair(W, H, D, i + 1))
            disp = de.SGBM_GPU()
            n = int(np.count_nonzero(disp != model(W, H, D, i)["disp"]))
            print(f"[sgm-loop] frame {i}: differing map elements {n}")
            assert n == 0, i


def test_sgm_only_async_frame_loop_of_a_batch(psm):
    """The same loop through psm_sgm_compute_batch with three contexts on shared streams, each with a pair sequence of its own: the
    mark is recorded for every member on the shared stream.  A guard like the one above, not a proof."""
    from primestereomatch_amd import dispest
    W, H, D, frames, n = 67, 45, 16, 5, 3

    def seed(i, k):                                      # frame i of context k
        return (i + 2 * k) % 7

    des = open_all(psm, [pair(W, H, D, seed(0, k)) for k in range(n)], D)
    try:
        dispest.share_streams(des)
        for k, de in enumerate(des):
            de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
            de.setInputImages_async(*pair(W, H, D, seed(0, k)))
        for i in range(frames):
            for de in des:
                de.CostConst_GPU()
            for k, de in enumerate(des):
                if i + 1 < frames:
                    de.setInputImages_async(*pair(W, H, D, seed(i + 1, k)))
            maps = dispest.sgbm_batch(des)
            for k, disp in enumerate(maps):
                assert np.array_equal(disp, model(W, H, D, seed(i, k))["disp"]), (i, k)
    finally:
        close_all(des)


def test_harness_batch(psm, golden):
    from primestereomatch_amd import harness
    ps = [golden(f"{n}_pair.npz") for n in ("cones", "teddy")]
    gs = [golden(f"{n}_sgm_bt.npz") for n in ("cones", "teddy")]
    outs = harness.compute_sgbm_batch([(p["l_bgr"], p["r_bgr"]) for p in ps], 64, [p["gt_l"] for p in ps], [p["occl"] for p in ps], 4,
                                      pre_filter_cap=63)
    for p, g, out in zip(ps, gs, outs):
        one = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], p["occl"], 4, pre_filter_cap=63)
        assert np.array_equal(out["disp16"], g["disp"]) and np.array_equal(out["lDispMap"], one["lDispMap"])
        assert out["bp_percent"] == one["bp_percent"] and out["bp_percent_int"] == one["bp_percent_int"]
        assert out["paths_ms"] > 0


def test_cpp_demo_sgbm_batch(psm, golden, tmp_path):
    """psm_demo's batch and sgbm_ref arguments together: DispEst::SGBMBatch on three copies of Cones, checked by the demo against
    its own single run."""
    import os
    import subprocess
    from conftest import ROOT
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    p = golden("cones_pair.npz")
    H, W, _ = p["l_bgr"].shape
    p["l_bgr"].tofile(tmp_path / "l.raw")
    p["r_bgr"].tofile(tmp_path / "r.raw")
    env = dict(os.environ, PRIMESM_HIP_LIB=psm.capi.LIB_PATH)
    q = subprocess.run([demo, str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(W), str(H), "64", str(tmp_path / "o"),
                        "1", "f32", "0", "0", "0", "0", "3", "0", "sgbm_ref"], env=env, capture_output=True, text=True, timeout=300)
    assert q.returncode == 0, q.stdout + q.stderr
    assert "SGBM batch:\t 3 pairs" in q.stdout and "maps equal the single run's" in q.stdout
