"""-m gpu: state-machine and entry-point regressions of the C ABI that are not about arithmetic - the round-2 advisor
findings (partial volume upload after a striped CostConst, stripe bookkeeping across psm_set_rows / FGF / merge), the frame
loop entries (psm_upload_pair_async, psm_download_maps_async / _wait), the in-kernel launch time stamps, and the domain of
the scaled window sums of the select forms."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def test_partial_volume_upload_after_striped_cost_construct(psm, oracle):
    """psm_set_rows + lazy CostConst leaves only a stripe of g1 prepared (the g1 record is that stripe): a partial psm_upload_volume must
    still materialise every other slice from the WHOLE image first (round-2 advisor finding: it skipped that and left
    uninitialised slices marked as real costs)."""
    from primestereomatch_amd import synth
    W, H, D = 140, 60, 9
    l, r, _ = synth.make_pair(W, H, D, seed=4)
    ref = oracle.pipeline_f32(l, r, D, threads=4, want_raw=True)
    patch = np.full((2, H, W), 0.25, np.float32)
    with psm.DispEst(l, r, D) as de:
        de.set_rows(20, 40)
        de.CostConst_GPU()
        de.upload_volume(0, patch, d0=3)
        got = de.download_volume(0)
        exp = ref["raw_l"].copy()
        exp[3:5] = patch
        assert np.array_equal(got, exp)
        assert np.array_equal(de.download_volume(1), ref["raw_r"])


def test_stripe_bookkeeping_follows_the_filter_not_set_rows(psm, oracle):
    from primestereomatch_amd import capi, synth
    W, H, D = 150, 64, 10
    l, r, _ = synth.make_pair(W, H, D, seed=6)
    ref = oracle.pipeline_f32(l, r, D, threads=4)
    a, b = psm.DispEst(l, r, D), psm.DispEst(l, r, D)
    try:
        a.set_rows(0, 30); b.set_rows(30, H)
        for c in (a, b):
            c.CostConst_GPU(); c.CostFilter_GPU(); c.DispSelect_GPU()
        # psm_set_rows after the filter only concerns the NEXT filter: the gather still takes the rows the maps were made for
        a.set_rows(5, 9); b.set_rows(0, 0)
        a.gather_rows_ctx([a, b])
        assert np.array_equal(a.lDisMap, ref["ldisp"]) and np.array_equal(a.rDisMap, ref["rdisp"])
        a.LRCheck_GPU()                                   # gathered maps are whole
        assert np.array_equal(a.lValid, oracle.lr_check(ref["ldisp"], ref["rdisp"])[0])
        # stripe-only maps are refused by the post-processing ...
        b.set_rows(30, H)
        b.CostConst_GPU(); b.CostFilter_GPU(); b.DispSelect_GPU()
        with pytest.raises(capi.PsmError):
            b.LRCheck_GPU()
        # ... the FGF path refuses a stripe, and whole-image FGF results clear the stripe state
        with pytest.raises(capi.PsmError):
            b.CostFilter_FGF_GPU()
        b.set_rows(0, 0)
        b.CostConst_GPU(); b.CostFilter_FGF_GPU(); b.DispSelect_GPU()
        fg = oracle.pipeline_fgf(l, r, D, s=4)
        assert np.array_equal(b.lDisMap, fg["ldisp"])
        b.LRCheck_GPU()
        # ... as do uploaded maps and a WTA over a materialised (whole) volume
        a.set_rows(0, 30)
        a.CostConst_GPU(); a.CostFilter_GPU(); a.DispSelect_GPU()
        a.upload_maps(ref["ldisp"], ref["rdisp"])
        a.LRCheck_GPU()
        a.CostConst_GPU(); a.CostFilter_GPU()
        a.download_volume(0); a.download_volume(1)        # materialises both sides (whole image)
        a.DispSelect_GPU()
        assert np.array_equal(a.lDisMap, ref["ldisp"])
        a.LRCheck_GPU()
    finally:
        a.close(); b.close()


def test_frame_loop_async_upload_and_download(psm, oracle):
    """psm_upload_pair_async / psm_download_maps_async: frame i+1's pair travels and frame i-1's maps return while frame
    i computes; every frame's maps equal the oracle's (three different pairs, two rounds)."""
    from primestereomatch_amd import synth
    W, H, D = 200, 90, 24
    pairs = [synth.make_pair(W, H, D, seed=s)[:2] for s in (1, 2, 3)]
    refs = [oracle.pipeline_f32(l, r, D, threads=4) for l, r in pairs]
    seq = [0, 1, 2, 0, 2, 1]
    with psm.DispEst(*pairs[seq[0]], D) as de:
        got = []
        for i, k in enumerate(seq):
            de.CostConst_GPU()                              # adopts the pair staged during the previous frame
            if i + 1 < len(seq):
                de.setInputImages_async(*pairs[seq[i + 1]])  # travels while this frame is filtered
            de.CostFilter_GPU(); de.DispSelect_device()
            if i > 0:
                got.append(tuple(m.copy() for m in de.download_maps_wait()))   # maps of frame i-1
            de.download_maps_async()
        got.append(tuple(m.copy() for m in de.download_maps_wait()))
        assert len(got) == len(seq)
        for k, (lm, rm) in zip(seq, got):
            assert np.array_equal(lm, refs[k]["ldisp"]) and np.array_equal(rm, refs[k]["rdisp"]), k
        # a blocking upload supersedes a staged pair
        de.setInputImages_async(*pairs[1])
        de.setInputImages(*pairs[2])
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, refs[2]["ldisp"])


def test_single_phase_filter_writes_the_maps_once(psm, oracle):
    """Below 112 slices the filter's plane reduction writes the maps itself (psm_disp_select launches nothing): a second select
    after post-processing rewrote the maps in place must extract the raw WTA maps from the keys again, and a one-side filter or
    a new pair in between must not leave a stale early map behind."""
    from primestereomatch_amd import synth
    W, H, D = 180, 70, 20
    pa, pb = (synth.make_pair(W, H, D, seed=s)[:2] for s in (11, 12))
    ra, rb = (oracle.pipeline_f32(l, r, D, threads=4) for l, r in (pa, pb))
    with psm.DispEst(*pa, D) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, ra["ldisp"]) and np.array_equal(de.rDisMap, ra["rdisp"])
        de.LRCheck_GPU(); de.FillInv_GPU()                                  # rewrites the maps in place
        lv, rv = oracle.lr_check(ra["ldisp"], ra["rdisp"])
        assert np.array_equal(de.lDisMap, oracle.fill_inv(ra["ldisp"], lv))
        de.DispSelect_GPU()                                                # the raw maps again, from the keys
        assert np.array_equal(de.lDisMap, ra["ldisp"]) and np.array_equal(de.rDisMap, ra["rdisp"])
        # filter, then a new pair, then the full sequence: nothing of pair a survives
        de.CostConst_GPU(); de.CostFilter_GPU()
        de.setInputImages(*pb)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, rb["ldisp"]) and np.array_equal(de.rDisMap, rb["rdisp"])
        # both sides filtered together (early maps), then fresh costs filtered side by side (keys rewritten): the select must not skip
        de.CostConst_GPU(); de.CostFilter_GPU()
        de.CostConst_GPU(); de.CostFilter_side(0); de.CostFilter_side(1)
        de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, rb["ldisp"]) and np.array_equal(de.rDisMap, rb["rdisp"])


def test_upload_of_rows_that_are_not_a_multiple_of_four_bytes(psm, oracle):
    """A 450-pixel (Middlebury) or 451-pixel row is 1350 / 1353 bytes: hipMemcpy2D copied such images row by row (6.5 ms for
    the 1 MB pair; 18.9 ms at 1919 x 1080).  Contiguous images travel as one linear copy, pitched ones with odd rows are packed
    first - same maps either way, and the blocking upload stays far below the old time."""
    import ctypes as C
    import time
    from primestereomatch_amd import capi, synth
    W, H, D = 451, 120, 12
    l, r, _ = synth.make_pair(W, H, D, seed=21)
    ref = oracle.pipeline_f32(l, r, D, threads=4)
    with psm.DispEst(l, r, D) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])
        de.synchronize()
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter(); de.setInputImages(l, r); best = min(best, time.perf_counter() - t0)
        assert best < 2e-3, f"blocking upload of a {W}x{H} pair took {1e3 * best:.2f} ms"
        # pitched images (a region of a wider buffer): stride 1353 + 7 bytes
        pitch = W * 3 + 7
        bl, br = (np.zeros((H, pitch), np.uint8) for _ in range(2))
        bl[:, :W * 3] = l.reshape(H, W * 3); br[:, :W * 3] = r.reshape(H, W * 3)
        rc = de._lib.psm_upload_pair(de._h, bl.ctypes.data_as(C.c_void_p), br.ctypes.data_as(C.c_void_p), 3, pitch, capi.PSM_IMG_U8)
        assert rc == 0
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])


def test_filter_launch_time_stamps(psm):
    """PSM_OPT_PROFILE 2: the fused filter kernel stamps its own start / end; two launches per frame at 120 slices (planes
    phase, key phase), durations positive and below the frame's wall time; results unchanged."""
    import time
    from primestereomatch_amd import capi, synth
    W, H, D = 320, 120, 120
    l, r, _ = synth.make_pair(W, H, D, seed=9)
    with psm.DispEst(l, r, D) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        base = de.lDisMap.copy()
        de.set_option(capi.PSM_OPT_PROFILE, 2)
        de.filter_launch_times()
        t0 = time.perf_counter()
        for _ in range(3):
            de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        lt = de.filter_launch_times()
        assert [f for _, f in lt] == [1, 2, 1, 2, 1, 2], lt
        assert all(0.0 < ms < wall_ms for ms, _ in lt), (lt, wall_ms)
        assert sum(ms for ms, _ in lt) < wall_ms
        assert de.filter_launch_times() == []
        assert np.array_equal(de.lDisMap, base)


@pytest.mark.parametrize("k", [-60, -20, 0, 20, 60])
def test_scaled_sums_domain(psm, oracle, k):
    """The select forms carry the 1/64 of the box filters as one exact 2^-12 at the end (psm_pc.hip): bit-identical to the
    oracle while no intermediate leaves the normal fp32 range.  Uploaded cost volumes scaled by 2^k, k = -60 .. 60 (costs
    from 1e-18 to 1e18): the select path's maps equal the WTA of the oracle's filtered volume, and the storing form's
    volume is bit-identical to it."""
    from primestereomatch_amd import capi
    rng = np.random.default_rng(12)
    H, W, D = 40, 130, 7
    l = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    r = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    l[10:20, 30:60] = 77                                   # ill-conditioned patch
    vol = ((rng.random((D, H, W), dtype=np.float32) * 2.7 - 0.3) * np.float32(2.0 ** k)).astype(np.float32)
    q = []
    for img in (l, r):
        rgb, mean, var = oracle.cvf_preprocess(oracle.u8_to_f32(img))
        q.append(np.stack([oracle.guided_filter(rgb, mean, var, vol[d]) for d in range(D)]))
    with psm.DispEst(l, r, D) as de:
        de.upload_volume(0, vol); de.upload_volume(1, vol)
        de.CostFilter_GPU()                                # select form (costs read from the uploaded volumes)
        de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, oracle.wta(q[0])) and np.array_equal(de.rDisMap, oracle.wta(q[1]))
        assert np.array_equal(de.download_volume(0), q[0]) and np.array_equal(de.download_volume(1), q[1])


def test_async_download_is_not_raced_by_later_map_writers(psm, oracle):
    """Round-3 advisor finding: psm_download_maps_async promises the maps as they were when it was called; every later entry
    that rewrites the device maps in place (fillInv, wgtMedian, psm_upload_maps, a gather / merge into them) must wait for that
    copy on the device.  A large pair makes the D2H long enough for the race to show without the wait."""
    from primestereomatch_amd import synth
    W, H, D = 1920, 1080, 16
    l, r, _ = synth.make_pair(W, H, D, seed=3)
    with psm.DispEst(l, r, D) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        raw = [de.lDisMap.copy(), de.rDisMap.copy()]
        de.LRCheck_GPU()
        for writer in ("fill", "median", "upload"):
            de.upload_maps(raw[0], raw[1], de.lValid, de.rValid)
            de.download_maps_async()
            if writer == "fill":
                de._ck(de._lib.psm_fill_invalid(de._h, None, None, 0), "fill")
            elif writer == "median":
                de._ck(de._lib.psm_wgt_median(de._h, None, None, 0), "wmf")
            else:
                de.upload_maps(np.zeros_like(raw[0]), np.zeros_like(raw[1]))
            lm, rm = de.download_maps_wait()
            assert np.array_equal(lm, raw[0]) and np.array_equal(rm, raw[1]), writer
            after = [m.copy() for m in de.download_maps()]
            assert not (np.array_equal(after[0], raw[0]) and np.array_equal(after[1], raw[1])), writer   # the writer did run


def _forms(de):
    return sorted({f for _, f in de.filter_launch_times()})


@pytest.mark.parametrize("k,stored", [(-120, True), (100, True), (58, False), (-55, False)])
def test_scaled_sums_guard_on_uploaded_volumes(psm, oracle, k, stored):
    """Round-3 verdict: the select forms' scaled window sums have a domain; a volume outside it (2^-120, 2^100) must run the
    storing form - the oracle's arithmetic at any scale - instead of silently disagreeing with it."""
    from primestereomatch_amd import capi
    rng = np.random.default_rng(3)
    H, W, D = 40, 130, 6
    l = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    r = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    vol = ((rng.random((D, H, W), dtype=np.float32) * 2.7 + 0.1) * np.float32(2.0 ** k)).astype(np.float32)
    q = []
    for img in (l, r):
        rgb, mean, var = oracle.cvf_preprocess(oracle.u8_to_f32(img))
        q.append(np.stack([oracle.guided_filter(rgb, mean, var, vol[d]) for d in range(D)]))
    with psm.DispEst(l, r, D) as de:
        de.set_option(capi.PSM_OPT_PROFILE, 2)
        de.upload_volume(0, vol); de.upload_volume(1, vol)
        de.filter_launch_times()
        de.CostFilter_GPU(); de.DispSelect_GPU()
        forms = _forms(de)
        assert (forms == [0]) == stored, forms                         # 0 = storing form, 1 / 2 = select forms
        assert np.array_equal(de.download_volume(0), q[0]) and np.array_equal(de.download_volume(1), q[1])
        assert np.array_equal(de.lDisMap, oracle.wta(q[0])) and np.array_equal(de.rDisMap, oracle.wta(q[1]))
        de.CostConst_GPU(); de.filter_launch_times()                   # new costs from the images: the guard is lifted
        de.CostFilter_GPU(); de.DispSelect_GPU()
        assert 0 not in _forms(de)


def test_scaled_sums_guard_on_float_images(psm, oracle):
    """Float images as the reference hands them over (x 1/255, src/StereoMatch.cpp:195-198) stay on the select path and give
    the u8 upload's maps; images far outside [2^-10, 2^10] go through the storing form - blocking and asynchronous upload."""
    from primestereomatch_amd import capi, synth
    W, H, D = 150, 70, 12
    l, r, _ = synth.make_pair(W, H, D, seed=8)
    ref = oracle.pipeline_f32(l, r, D, threads=4)
    lf, rf = oracle.u8_to_f32(l), oracle.u8_to_f32(r)
    big = np.float32(2.0 ** 14)
    with psm.DispEst(lf, rf, D) as de:
        de.set_option(capi.PSM_OPT_PROFILE, 2)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert 0 not in _forms(de)
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])
        de.setInputImages(lf * big, rf * big)                          # outside: storing form
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert _forms(de) == [0]
        scaled_maps = [de.lDisMap.copy(), de.rDisMap.copy()]
        de.setInputImages_async(lf, rf)                                # next frame inside again, staged asynchronously
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert 0 not in _forms(de)
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])
        de.setInputImages_async(lf * big, rf * big)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert _forms(de) == [0]
        assert np.array_equal(de.lDisMap, scaled_maps[0]) and np.array_equal(de.rDisMap, scaled_maps[1])
    with psm.DispEst(lf * big, rf * big, D) as de:                     # (the explicit storing flag gives the same maps)
        de.set_option(capi.PSM_OPT_FLAGS, capi.PSM_FLAG_STORE_FILTERED)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        assert np.array_equal(de.lDisMap, scaled_maps[0]) and np.array_equal(de.rDisMap, scaled_maps[1])


def test_release_scratch_gives_memory_back_and_changes_nothing(psm, oracle):
    """psm_release_scratch: the on-first-use scratch (weighted-median sweep state and weight cache, minima planes, exchange buffers)
    goes back to the device; maps / minima survive and the next calls allocate again and give the same results."""
    import ctypes as C
    from primestereomatch_amd import synth
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        a, b = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(a), C.byref(b)) == 0
        return a.value

    W, H, D = 640, 360, 48
    l, r, _ = synth.make_pair(W, H, D, seed=12)
    ref = oracle.pipeline_f32(l, r, D, threads=8)
    with psm.DispEst(l, r, D) as de:
        def frame():
            de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
            assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])
            de.LRCheck_GPU(); de.FillInv_GPU(); de.WgtMedian_GPU()
            return de.lDisMap.copy(), de.rDisMap.copy()
        a = frame()
        held = free_bytes()
        de.release_scratch()
        assert free_bytes() > held + (8 << 20)             # (minima planes + sweep scratch + weight cache of a 640 x 360 pair: tens of MB)
        lm, rm = de.download_maps()                        # the maps are state, not scratch
        assert np.array_equal(lm, a[0]) and np.array_equal(rm, a[1])
        b = frame()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("frames,dtype", [(1, "f32"), (2, "f32"), (3, "u8")])
def test_frame_ring_returns_every_frames_maps_in_order(psm, oracle, frames, dtype):
    """FrameRing: `frames` contexts take the frames of a stream in turn (two frames in the device's queues); every frame's maps
    come back, in order, and equal the oracle's for THAT frame's pair."""
    from primestereomatch_amd import synth
    W, H, D = 200, 120, 24
    pairs = [synth.make_pair(W, H, D, seed=40 + k)[:2] for k in range(7)]
    want = [(oracle.pipeline_u8 if dtype == "u8" else oracle.pipeline_f32)(l, r, D, threads=8) for l, r in pairs]
    got = []
    with psm.FrameRing(*pairs[0], D, frames=frames, dtype=dtype) as ring:
        for l, r in pairs:
            out = ring.push(l, r)
            if out is not None:
                got.append(out)
        assert len(got) == len(pairs) - frames
        got += ring.flush()
        assert ring.flush() == []
    assert len(got) == len(pairs)
    for k, ((lm, rm), e) in enumerate(zip(got, want)):
        assert np.array_equal(lm, e["ldisp"]) and np.array_equal(rm, e["rdisp"]), k

