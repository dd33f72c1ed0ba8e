"""-m gpu tests added in round 2:

* weighted-median post-filter (psm_wgt_median, src/PP.cpp:145-247) against the oracle's sequential in-place restatement -
  integer maps, bit-exact; the mismatch count (device exp vs host libm exp, narrowed to float) is reported and must be 0;
* the HIP filtered volumes against the oracle evaluated in OPENCV'S OWN summation order (PSMO_BOX_OCV: RowSum/ColumnSum
  running sums) - the order the reference binary executes at src/CVF.cpp:50,63,82,88,158,160 - within the north-star
  tolerance, WTA maps identical (expected and asserted: 0 differing voxels on the Middlebury pairs).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def _wm_inputs(H, W, D, seed, frac_invalid, smooth=True):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if smooth:   # piecewise-constant colours + small noise: colour weights that are not all ~0
        base = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3))
        img = np.clip(np.kron(base, np.ones((8, 8, 1)))[:H, :W] + rng.integers(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8)
    lm = rng.integers(0, D, (H, W)).astype(np.uint8)
    rm = rng.integers(0, D, (H, W)).astype(np.uint8)
    lv = (rng.random((H, W)) > frac_invalid).astype(np.uint8)
    rv = (rng.random((H, W)) > frac_invalid).astype(np.uint8)
    return img, lm, rm, lv, rv


WM_FORMS = {"sweeps": 0, "dataflow": 4194304, "fallback": 8388608}   # PSM_OPT_FLAGS: parallel form (default) / row-dataflow
#                                                                     form only / 2 sweeps, then the dataflow form from the input


@pytest.mark.parametrize("form", sorted(WM_FORMS))
@pytest.mark.parametrize("H,W,D,frac", [(21, 26, 16, 0.3), (40, 70, 64, 0.6), (33, 210, 200, 1.0), (12, 9, 8, 0.5),
                                        (48, 256, 256, 0.15)])
def test_wgt_median_random_maps(psm, oracle, H, W, D, frac, form):
    from primestereomatch_amd import capi
    l, lm, rm, lv, rv = _wm_inputs(H, W, D, seed=H * W + D, frac_invalid=frac)
    r = np.roll(l, 3, axis=1)
    with psm.DispEst(l, r, D) as de:
        de.set_option(capi.PSM_OPT_FLAGS, WM_FORMS[form])
        de.upload_maps(lm, rm, lv, rv)
        de.WgtMedian_GPU()
        gl, gr = de.lDisMap.copy(), de.rDisMap.copy()
        sweeps, evals = de.wgt_median_stats()
    print(f"[wmf] {form}: sweeps {sweeps}, evaluations {evals}")
    if form == "dataflow":
        assert sweeps == [-1, -1]
    elif form == "sweeps":
        assert min(sweeps) >= 1          # the parallel form reached its fixed point (no fall-back on these maps)
    el = oracle.wgt_median(oracle.u8_to_f32(l), lm, lv, D, right=False)
    er = oracle.wgt_median(oracle.u8_to_f32(r), rm, rv, D, right=True)
    print(f"[wmf] {W}x{H} D={D}: left mismatches {(gl != el).sum()}, right {(gr != er).sum()} "
          f"of {(lv == 0).sum()} / {(rv == 0).sum()} filtered pixels")
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    assert np.array_equal(gl[lv != 0], lm[lv != 0])


@pytest.mark.parametrize("flags", [0, 16777216, 4194304])
def test_wgt_median_long_lists_with_and_without_the_weight_cache(psm, oracle, flags):
    """From 8192 invalid pixels per map a sweep evaluates one pixel per LANE, reads the window weights formed once by
    k_wm_weights and finds the next sweep's pixels by marking + gathering; PSM_FLAG_WMF_NO_CACHE (or a cache that does not fit)
    makes the same kernel form its weights in place; 4194304 is the dataflow form.  All against the oracle, on a map whose first
    sweeps are long and whose last ones are short (every evaluation / dependents path runs).

    This input is the one that exposed __fsqrt_rn (round 3): all three forms put 46 where the oracle has 48 at (59, 58) of the
    right map - a running sum one ulp below half the total, and 51 of that window's 361 weights one ulp off because the HIP
    intrinsic is not correctly rounded (sqrt(162.0f) among them).  The weights are bit-identical to the host's now by
    construction: correctly rounded roots through double, exp as glibc forms it (psm_exp.h, pinned by
    tests/test_oracle.py::test_wm_exp_is_the_host_libm_exp)."""
    from primestereomatch_amd import capi
    H, W, D = 110, 230, 96
    l, lm, rm, lv, rv = _wm_inputs(H, W, D, seed=77, frac_invalid=0.55)
    assert (lv == 0).sum() >= 8192 and (rv == 0).sum() >= 8192
    r = np.roll(l, 5, axis=1)
    with psm.DispEst(l, r, D) as de:
        de.set_option(capi.PSM_OPT_FLAGS, flags)
        de.upload_maps(lm, rm, lv, rv)
        de.WgtMedian_GPU()
        gl, gr = de.lDisMap.copy(), de.rDisMap.copy()
        sweeps, evals = de.wgt_median_stats()
    assert flags == 4194304 or min(sweeps) >= 2
    el = oracle.wgt_median(oracle.u8_to_f32(l), lm, lv, D, right=False)
    er = oracle.wgt_median(oracle.u8_to_f32(r), rm, rv, D, right=True)
    print(f"[wmf] {W}x{H} D={D} flags {flags}: sweeps {sweeps}, evaluations {evals}, mismatches {(gl != el).sum()} + {(gr != er).sum()}")
    assert np.array_equal(gl, el) and np.array_equal(gr, er)


def test_wgt_median_forms_in_turn_on_one_context(psm, oracle):
    """One context through every form of the driver in turn - sweeps with the cache, without it, the dataflow form, two sweeps and
    the fall-back, then the first two again - on the inputs of the long-list test, uploaded anew for every run, with
    psm_release_scratch between each run and the next: every run allocates its scratch again (wm_free gave it back), lays the
    sweep block out again and meets the page-locked snapshots, the events and the statistics another form left behind.  Both maps
    are the oracle's every time."""
    from primestereomatch_amd import capi
    H, W, D = 110, 230, 96
    l, lm, rm, lv, rv = _wm_inputs(H, W, D, seed=77, frac_invalid=0.55)
    assert (lv == 0).sum() >= 8192 and (rv == 0).sum() >= 8192
    r = np.roll(l, 5, axis=1)
    el = oracle.wgt_median(oracle.u8_to_f32(l), lm, lv, D, right=False)
    er = oracle.wgt_median(oracle.u8_to_f32(r), rm, rv, D, right=True)
    NO_CACHE, DATAFLOW, TWO_SWEEPS = 16777216, 4194304, 8388608
    with psm.DispEst(l, r, D) as de:
        for run, flags in enumerate((0, NO_CACHE, DATAFLOW, TWO_SWEEPS, 0, NO_CACHE)):
            if run:
                de.release_scratch()
            de.set_option(capi.PSM_OPT_FLAGS, flags)
            de.upload_maps(lm, rm, lv, rv)
            de.WgtMedian_GPU()
            sweeps, evals = de.wgt_median_stats()
            print(f"[wmf] run {run} flags {flags}: sweeps {sweeps}, evaluations {evals}")
            assert np.array_equal(de.lDisMap, el) and np.array_equal(de.rDisMap, er), run
            if flags == DATAFLOW:
                assert sweeps == [-1, -1]
            elif flags in (0, NO_CACHE):
                assert min(sweeps) >= 2, run


def test_wgt_median_repeats_give_one_map(psm, oracle):
    """Round 6: a changed pixel is written the moment it is found, so which evaluations of a sweep see it depends on timing - the
    number of evaluations may differ between runs, the maps may not (the fixed point is unique).  The same dense input twelve times,
    from the fifth on with a second context filtering another map on its own stream and host thread to stir the timing: one map, the oracle's."""
    H, W, D = 110, 230, 96
    l, lm, rm, lv, rv = _wm_inputs(H, W, D, seed=123, frac_invalid=0.6)
    r = np.roll(l, 5, axis=1)
    el = oracle.wgt_median(oracle.u8_to_f32(l), lm, lv, D, right=False)
    er = oracle.wgt_median(oracle.u8_to_f32(r), rm, rv, D, right=True)
    import threading
    seen = set()
    with psm.DispEst(l, r, D) as de, psm.DispEst(r, l, D) as other:
        stop = threading.Event()

        def stir():                        # (its own context and stream; the C calls release the interpreter lock)
            while not stop.is_set():
                other.upload_maps(rm, lm, rv, lv)
                other.WgtMedian_GPU()

        th = threading.Thread(target=stir)
        try:
            for rep in range(12):
                if rep == 4:
                    th.start()
                de.upload_maps(lm, rm, lv, rv)
                de.WgtMedian_GPU()
                assert np.array_equal(de.lDisMap, el) and np.array_equal(de.rDisMap, er), rep
                seen.add(tuple(de.wgt_median_stats()[1]))
        finally:
            stop.set()
            if th.is_alive():
                th.join()
    print(f"[wmf] 12 repeats: {len(seen)} different evaluation counts {sorted(seen)[:3]} ...")


@pytest.mark.parametrize("fl,fr", [(0.0, 0.5), (0.5, 0.0), (0.55, 0.02), (0.01, 0.6), (0.0, 0.0)])
@pytest.mark.parametrize("flags", [0, 16777216])
def test_wgt_median_unequal_maps_share_their_launches(psm, oracle, fl, fr, flags):
    """Round 6: both maps go through every sweep launch side by side (WmPair) and one decision - weight cache or not, wave
    form only or all four launches - holds for the pair.  Maps that differ in everything the decision looks at: one without a
    single invalid pixel beside one with a long list, a short list (below WM_LANE_MIN: wave form, weights formed in place when
    alone) beside a long one, nothing to do at all; 111 x 233 pixels is no multiple of the 16 pixels a thread of the seed launch
    takes, so its tail path and the odd offset of the right map's planes run as well."""
    from primestereomatch_amd import capi
    H, W, D = 111, 233, 80
    l, lm, rm, _, _ = _wm_inputs(H, W, D, seed=int(1000 * fl + 10 * fr) + 5, frac_invalid=0.5)
    rng = np.random.default_rng(9)
    lv = (rng.random((H, W)) >= fl).astype(np.uint8)
    rv = (rng.random((H, W)) >= fr).astype(np.uint8)
    r = np.roll(l, 4, axis=1)
    with psm.DispEst(l, r, D) as de:
        de.set_option(capi.PSM_OPT_FLAGS, flags)
        for rep in range(2):              # (the second call reuses the sweep state, the cache and the counters of the first)
            de.upload_maps(lm, rm, lv, rv)
            de.WgtMedian_GPU()
        gl, gr = de.lDisMap.copy(), de.rDisMap.copy()
        sweeps, evals = de.wgt_median_stats()
    el = oracle.wgt_median(oracle.u8_to_f32(l), lm, lv, D, right=False)
    er = oracle.wgt_median(oracle.u8_to_f32(r), rm, rv, D, right=True)
    print(f"[wmf] invalid {int((lv == 0).sum())} / {int((rv == 0).sum())}, flags {flags}: sweeps {sweeps}, evaluations {evals}")
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    assert min(sweeps) >= 1 and (fl > 0 or evals[0] == 0) and (fr > 0 or evals[1] == 0)


@pytest.mark.parametrize("form", ["sweeps", "dataflow"])
@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_wgt_median_after_lr_check_middlebury(psm, oracle, golden, name, form):
    """PP::processDM's sequence (src/PP.cpp:405-410): lrCheck -> fillInv -> wgtMedian on the real pair."""
    from primestereomatch_amd import capi
    pair = golden(f"{name}_pair.npz")
    l, r = pair["l_bgr"], pair["r_bgr"]
    with psm.DispEst(l, r, 64) as de:
        de.set_option(capi.PSM_OPT_FLAGS, WM_FORMS[form])
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        de.LRCheck_GPU()
        lv, rv = de.lValid.copy(), de.rValid.copy()
        de.FillInv_GPU()
        lf, rf = de.lDisMap.copy(), de.rDisMap.copy()
        de.WgtMedian_GPU()
        gl, gr = de.lDisMap.copy(), de.rDisMap.copy()
        us = de.stage_time_us(3)
        sweeps, evals = de.wgt_median_stats()
    print(f"[wmf] {name} ({form}): sweeps {sweeps}, evaluations {evals}")
    el = oracle.wgt_median(oracle.u8_to_f32(l), lf, lv, 64, right=False)
    er = oracle.wgt_median(oracle.u8_to_f32(r), rf, rv, 64, right=True)
    nl, nr = int((gl != el).sum()), int((gr != er).sum())
    print(f"[wmf] {name}: {int((lv == 0).sum())} + {int((rv == 0).sum())} pixels filtered, mismatches vs oracle: {nl} + {nr}; "
          f"PP stage {us / 1e3:.2f} ms")
    assert nl == 0 and nr == 0
    assert not np.array_equal(gl, lf)          # the filter did something


def test_wgt_median_needs_lr_check(psm):
    from primestereomatch_amd import capi
    rng = np.random.default_rng(0)
    l = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    with psm.DispEst(l, l, 8) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        with pytest.raises(capi.PsmError):
            de.WgtMedian_GPU()                 # no validity mask yet
        de.LRCheck_GPU()
        de.WgtMedian_GPU()
        # a new WTA invalidates the mask (stale validity after new maps)
        de.DispSelect_GPU()
        with pytest.raises(capi.PsmError):
            de.FillInv_GPU()


def test_create_rejects_what_the_kernels_cannot_address(psm):
    from primestereomatch_amd import capi
    rng = np.random.default_rng(1)
    l = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    with pytest.raises(capi.PsmError):
        psm.DispEst(l, l, 32)                  # max_disp > width: lrCheck's modulo goes negative (undefined in the reference)
    lib = capi.load()
    import ctypes as C
    h = C.c_void_p()
    assert lib.psm_create(C.byref(h), 16384, 8192, 64, 0, 0) != 0       # W*H >= 2^27: 32-bit plane offsets
    assert b"too large" in lib.psm_last_error(None) or b"8192" in lib.psm_last_error(None)


def test_merge_ctx_checks_the_shards(psm):
    """psm_disp_merge_ctx must refuse shards that have not run their partial WTA for this frame or that do not
    tile [0, D)."""
    from primestereomatch_amd import capi
    rng = np.random.default_rng(2)
    l = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    r = np.roll(l, 2, axis=1)
    D = 12
    shards = [psm.DispEst(l, r, D, d_range=(0, 5)), psm.DispEst(l, r, D, d_range=(5, 12))]
    try:
        for s in shards:
            s.CostConst_GPU(); s.CostFilter_GPU()
        shards[0].DispSelect_partial()
        with pytest.raises(capi.PsmError):
            shards[0].DispSelect_merge_ctx(shards)            # shard 1 has no minima yet
        shards[1].DispSelect_partial()
        with pytest.raises(capi.PsmError):
            shards[0].DispSelect_merge_ctx(shards[:1])        # slices 5..11 missing
        with pytest.raises(capi.PsmError):
            shards[0].DispSelect_merge_ctx([shards[0], shards[1], shards[1]])   # slices held twice
        shards[0].DispSelect_merge_ctx(shards)
        with psm.DispEst(l, r, D) as whole:
            whole.CostConst_GPU(); whole.CostFilter_GPU(); whole.DispSelect_GPU()
            assert np.array_equal(whole.lDisMap, shards[0].lDisMap) and np.array_equal(whole.rDisMap, shards[0].rDisMap)
        # a new frame invalidates the minima again
        shards[1].CostConst_GPU()
        with pytest.raises(capi.PsmError):
            shards[0].DispSelect_merge_ctx(shards)
    finally:
        for s in shards:
            s.close()


# ------------------------------------------------------------------------------------------
# HIP path vs the oracle in OpenCV's own summation order
# ------------------------------------------------------------------------------------------
def _gpu_pipeline(psm, l, r, D):
    with psm.DispEst(l, r, D) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        return de.lDisMap.copy(), de.rDisMap.copy(), de.download_volume(0), de.download_volume(1)


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_hip_vs_opencv_order_oracle_middlebury(psm, oracle, golden, name):
    pair = golden(f"{name}_pair.npz")
    l, r = pair["l_bgr"], pair["r_bgr"]
    ld, rd, lv, rv = _gpu_pipeline(psm, l, r, 64)
    with oracle.box_order(oracle.BOX_OCV):
        ref = oracle.pipeline_f32(l, r, 64, threads=8, want_volumes=True)
    for nm, g, e in (("lvol", lv, ref["lvol"]), ("rvol", rv, ref["rvol"])):
        d = np.abs(g.astype(np.float64) - e)
        print(f"[ocv-order] {name} {nm}: max|dq|={d.max():.3e}  voxels>1e-4: {int((d > TOL).sum())}  bit-different: {int((g != e).sum())}")
        assert d.max() <= TOL
    nmap = int((ld != ref["ldisp"]).sum() + (rd != ref["rdisp"]).sum())
    print(f"[ocv-order] {name}: WTA pixels different from the OpenCV-order evaluation: {nmap}")
    assert nmap == 0


@pytest.mark.parametrize("W,H,D,band", [(1280, 720, 128, (300, 380)), (1920, 1080, 256, (500, 564))])
def test_hip_vs_opencv_order_oracle_full_size_band(psm, oracle, W, H, D, band):
    """C3 / C4 geometry: a few slices of the full-size run against the OpenCV-order oracle.  The running column sums of
    the OpenCV order depend on every row above, so the oracle filters the whole plane (two slices only)."""
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=0)
    d_lo, d_hi = D // 2, D // 2 + 2
    with psm.DispEst(l, r, D, d_range=(d_lo, d_hi)) as de:
        de.CostConst_GPU(); de.CostFilter_GPU()
        q = de.download_volume(0)
    lf, rf = oracle.u8_to_f32(l), oracle.u8_to_f32(r)
    lG, rG = oracle.cvc_preprocess(lf), oracle.cvc_preprocess(rf)
    with oracle.box_order(oracle.BOX_OCV):
        rgb, mean, var = oracle.cvf_preprocess(lf)
        for d in range(d_lo, d_hi):
            qq = oracle.guided_filter(rgb, mean, var, oracle.cvc_build(lf, rf, lG, rG, d))
            dd = np.abs(q[d - d_lo].astype(np.float64) - qq)
            print(f"[ocv-order] {W}x{H} d={d}: max|dq|={dd.max():.3e}  voxels>1e-4: {int((dd > TOL).sum())}  "
                  f"bit-different: {int((q[d - d_lo] != qq).sum())} of {qq.size}")
            assert dd.max() <= TOL


def test_device_wm_weights_equal_the_host(psm, oracle):
    """Round-3 advisor finding: the weighted median's parity rests on the device forming every weight as the host does - roots
    (the right map's two sqrtf; __fsqrt_rn is NOT correctly rounded on this ROCm, so they go through the double root) and
    glibc's exp.  Operand by operand, both forms, including sqrt(162.0f) (wx = wy = 9) and colour distances from u8 images."""
    import ctypes as C
    lib = psm.capi.load()
    rng = np.random.default_rng(11)
    n = 200000
    p3 = (rng.integers(0, 256, size=(n, 3)).astype(np.float32) * np.float32(1 / 255.0)).astype(np.float32)
    q3 = (rng.integers(0, 256, size=(n, 3)).astype(np.float32) * np.float32(1 / 255.0)).astype(np.float32)
    q3[: n // 4] = p3[: n // 4] + rng.integers(-3, 4, size=(n // 4, 3)).astype(np.float32) * np.float32(1 / 255.0)   # near colours: weights far from 0
    wxy = rng.integers(-9, 10, size=(n, 2)).astype(np.int32)
    wxy[0] = (9, 9); wxy[1] = (-9, 9)                      # disWgt = 162
    pq = np.zeros((n, 8), np.float32)
    pq[:, 0:3], pq[:, 4:7] = p3, q3
    fn = lib.psm_debug_wm_weights
    fn.restype = C.c_int
    for right in (0, 1):
        dev = np.empty(n, np.float32)
        assert fn(pq.ctypes.data_as(C.c_void_p), wxy.ctypes.data_as(C.c_void_p), n, right, dev.ctypes.data_as(C.c_void_p)) == 0
        host = oracle.wm_weights(p3[:20000], q3[:20000], wxy[:20000, 0], wxy[:20000, 1], right)
        bad = np.flatnonzero(dev[:20000].view(np.uint32) != host.view(np.uint32))
        assert bad.size == 0, (right, bad[:5], dev[bad[:5]], host[bad[:5]])
        assert np.isfinite(dev).all() and (dev[: n // 4] > 0).any()


def test_device_wm_weights_with_overflowing_colour_distances(psm, oracle):
    """Round-4 advisor finding: float images are accepted at any scale; channel differences around 1.8e19 make the squared colour
    distance overflow to +inf.  The reference then forms exp(-inf) = 0 (src/PP.cpp:175,224); the FMA refinements that replace the
    double division and the root are proven for FINITE operands only and would give NaN - they must fall back.  Also NaN colours:
    the host's NaN weight, bit for bit."""
    import ctypes as C
    lib = psm.capi.load()
    big = np.float32(3e19)
    p3 = np.array([[big, 0, 0], [big, big, 0], [1e10, 0, 0], [np.float32(1.8e19), 0, 0], [np.nan, 0, 0], [0.5, 0.25, 0.125]], np.float32)
    q3 = np.array([[-big, 0, 0], [0, 0, big], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0.5, 0.25, 0.125]], np.float32)
    wxy = np.array([[0, 0], [3, -2], [9, 9], [1, 1], [0, 0], [0, 0]], np.int32)
    n = len(p3)
    pq = np.zeros((n, 8), np.float32)
    pq[:, 0:3], pq[:, 4:7] = p3, q3
    fn = lib.psm_debug_wm_weights
    fn.restype = C.c_int
    for right in (0, 1):
        dev = np.empty(n, np.float32)
        assert fn(pq.ctypes.data_as(C.c_void_p), wxy.ctypes.data_as(C.c_void_p), n, right, dev.ctypes.data_as(C.c_void_p)) == 0
        with np.errstate(all="ignore"):
            host = oracle.wm_weights(p3, q3, wxy[:, 0], wxy[:, 1], right)
        fin = ~np.isnan(host)                 # (a NaN colour gives a NaN weight on both sides; its sign / payload bits carry no meaning)
        assert np.array_equal(np.isnan(dev), ~fin) and not fin[4], (right, dev, host)
        assert np.array_equal(dev[fin].view(np.uint32), host[fin].view(np.uint32)), (right, dev, host)
        assert dev[0] == 0 and dev[1] == 0 and dev[5] == 1.0

