"""-m gpu: the score stage (psm_score: display maps and the reference's error record on the device) against its definition,
tests/score_model.py.  Everything is integer or a single IEEE operation with a defined rounding: the planes must be equal with 0
differing elements (np.array_equal) and every integer of the record equal - there is no tolerance anywhere in this file.
A context is at least 8 rows high (psm_create), so the small cases run at H = 8."""
import ctypes as C
import functools

import numpy as np
import pytest

import score_model as S

pytestmark = pytest.mark.gpu

H8 = 8
MASK_VALUES = np.array([0, 1, 127, 128, 254, 255], np.uint8)


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def blank(psm, W, H, D):
    z = np.zeros((H, W, 3), np.uint8)
    return psm.DispEst(z, z, D)


def rnd(seed):
    return np.random.default_rng(seed)


def device(de, source, data, gt=None, mask=None, scale=4, thr=4, mode=S.MASK_NONOCC):
    """parameters, truth and result to the context, one psm_score -> (record, planes)"""
    de.set_score_params(scale, thr, mode)
    if gt is None:
        de.clear_truth()
    else:
        de.set_truth(gt, mask)
    if source == S.GIF:
        de.upload_maps(data[0], data[1])
    else:
        de.upload_sgm_map(data)
    rec = de.Score_GPU(source)
    return rec, de.score_maps(right=source == S.GIF)


def equal(rec, planes, m):
    for k in S.RECORD_KEYS:
        assert rec[k] == m[k], (k, rec[k], m[k])
    assert rec["bp_percent"] == m["bp_percent"] and rec["avg_err"] == m["avg_err"]
    assert np.array_equal(planes[0], m["ldisp"])
    assert np.array_equal(planes[-1], m["emap"])
    if len(planes) == 3:
        assert np.array_equal(planes[1], m["rdisp"])


def same(de, source, data, D, gt=None, mask=None, scale=4, thr=4, mode=S.MASK_NONOCC):
    rec, planes = device(de, source, data, gt, mask, scale, thr, mode)
    m = S.score(source, data, gt, mask, D, scale, thr, mode)
    equal(rec, planes, m)
    return rec, planes, m


# ---- Cones and Teddy, all three sources, mask on / off / DISC ----
@pytest.mark.parametrize("name", ("cones", "teddy"))
def test_goldens_all_sources_and_masks(psm, golden, name):
    pair, orc, d16 = golden(f"{name}_pair.npz"), golden(f"{name}_oracle_d64.npz"), golden(f"{name}_sgm.npz")["disp"]
    gt, occl = pair["gt_l"], pair["occl"]
    synth = rnd(7).choice(MASK_VALUES, gt.shape)
    with blank(psm, gt.shape[1], gt.shape[0], 64) as de:
        for source, data in ((S.GIF, (orc["ldisp"], orc["rdisp"])), (S.SGM, d16), (S.SGM_INT, d16)):
            rec = same(de, source, data, 64, gt, occl)[0]
            assert rec["bad"] > 0 and rec["unit"] == 1
            same(de, source, data, 64, gt, None)
            same(de, source, data, 64, gt, occl, mode=S.MASK_NONE)
            same(de, source, data, 64, gt, synth, mode=S.MASK_DISC)
            same(de, source, data, 64, gt, synth, mode=S.MASK_NONOCC)
            rec, planes, _ = same(de, source, data, 64)                      # no truth: display and min / max all the same
            assert rec["bad"] == rec["err_sum"] == 0 and not planes[-1].any()
    assert round(S.score(S.GIF, orc["ldisp"], gt, occl, 64)["bp_percent"], 2) == {"cones": 14.50, "teddy": 19.83}[name]


# ---- row ends, padded strides ----
@pytest.mark.parametrize("W", (65, 67, 130, 258))
def test_row_ends_and_padded_strides(psm, W):
    from primestereomatch_amd import capi
    g = rnd(W)
    D = 16
    maps = (g.integers(0, 256, (H8, W)).astype(np.uint8), g.integers(0, 256, (H8, W)).astype(np.uint8))
    d16 = g.integers(-16, 16 * D, (H8, W)).astype(np.int16)
    pad = g.integers(0, 256, (2, H8, W + 7)).astype(np.uint8)                 # truth and mask as views of padded rows
    gt, mask = pad[0][:, :W], pad[1][:, :W]
    assert gt.strides[0] == W + 7
    with blank(psm, W, H8, D) as de:
        for source, data in ((S.GIF, maps), (S.SGM, d16), (S.SGM_INT, d16)):
            rec, planes, m = same(de, source, data, D, gt, mask, scale=3, thr=2)
            assert rec["bad"] > 0
        # ... and the planes into padded rows: the padding stays as it was
        out = np.full((3, H8, W + 5), 0xA5, np.uint8)
        de.upload_maps(*maps)
        de.Score_GPU(S.GIF)
        lib = capi.load()
        p = [out[i].ctypes.data_as(C.c_void_p) for i in range(3)]
        capi.check(lib.psm_score_download(de._h, p[0], p[1], p[2], W + 5), de._h)
        m = S.score(S.GIF, maps, gt, mask, D, 3, 2)
        for i, k in enumerate(("ldisp", "rdisp", "emap")):
            assert np.array_equal(out[i][:, :W], m[k]) and (out[i][:, W:] == 0xA5).all()
        assert lib.psm_score_download(de._h, p[0], None, None, W - 1) != 0 and "stride" in capi.last_error(de._h)
        assert lib.psm_score_set_truth(de._h, p[0], None, W - 1) != 0 and "stride" in capi.last_error(de._h)


# ---- the left columns ----
def test_column_zeroing(psm):
    D = 16
    for W, live in ((D + 1, 0), (D + 2, 1)):
        maps = (np.full((H8, W), 50, np.uint8), np.zeros((H8, W), np.uint8))
        gt = np.zeros((H8, W), np.uint8)
        with blank(psm, W, H8, D) as de:
            rec, planes, _ = same(de, S.GIF, maps, D, gt, None)
            assert rec["bad"] == live * H8 and rec["err_sum"] == live * H8 * 200
            assert not planes[-1][:, :D + 1].any()


# ---- unit = 127 / max_disp ----
@pytest.mark.parametrize("D,W,unit", ((127, 130, 1), (128, 130, 0), (256, 258, 0), (2, 65, 63)))
def test_unit(psm, D, W, unit):
    g = rnd(D)
    maps = (g.integers(0, 256, (H8, W)).astype(np.uint8), g.integers(0, 256, (H8, W)).astype(np.uint8))
    gt = g.integers(0, 256, (H8, W)).astype(np.uint8)
    with blank(psm, W, H8, D) as de:
        for thr in (0, 1, 4):
            rec = same(de, S.GIF, maps, D, gt, None, scale=1, thr=thr)[0]
            assert rec["unit"] == unit
            if unit == 0:                                  # the threshold is 0 whatever error_threshold says; Avg Err is 0.0
                assert rec["avg_err"] == 0.0
                assert rec["bad"] == int(np.count_nonzero((maps[0] != gt)[:, D + 1:]))


# ---- threshold edges: every e against every mask value ----
@pytest.mark.parametrize("thr", (0, 4, 255))
def test_threshold_edges(psm, thr):
    """256 x 256 live pixels (behind the max_disp + 1 columns the metric zeroes): row e, column k -> p = e, g = 0, mask = k."""
    D = 31
    unit = 127 // D
    W = 256 + D + 1
    e, k = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    p = np.zeros((256, W), np.uint8)
    mask = np.zeros((256, W), np.uint8)
    p[:, D + 1:], mask[:, D + 1:] = e, k
    p[:, :D + 1] = 255                                     # (errors there would count if the columns were live)
    gt = np.zeros((256, W), np.uint8)
    with blank(psm, W, 256, D) as de:
        rec, planes, m = same(de, S.GIF, (p, p), D, gt, mask, scale=1, thr=thr)
        emap = planes[-1][:, D + 1:]
        edge = thr * unit
        assert not emap[:min(edge, 255) + 1].any()                          # e <= t * unit stays zero, under every mask value
        if edge + 1 <= 255:
            assert emap[edge + 1, 255] == edge + 1                          # e == t * unit + 1 counts (mask 255 keeps it)
            assert rec["bad"] == int(np.count_nonzero(S.mask_step(e, k)[edge + 1:]))
        else:
            assert rec["bad"] == 0
        same(de, S.GIF, (p, p), D, gt, mask, scale=1, thr=thr, mode=S.MASK_DISC)
        rec = same(de, S.GIF, (p, p), D, gt, None, scale=1, thr=thr)[0]
        assert rec["bad"] == 256 * max(255 - edge, 0)


# ---- saturation of v * scale_factor ----
@pytest.mark.parametrize("scale", (1, 3, 4, 255))
def test_scale_saturation(psm, scale):
    v = np.arange(64 * H8, dtype=np.int64).reshape(H8, 64)
    maps = ((v % 256).astype(np.uint8), (255 - v % 256).astype(np.uint8))
    d16 = ((v * 37) % (256 * 16) - 16).astype(np.int16)
    gt = np.full((H8, 64), 128, np.uint8)
    with blank(psm, 64, H8, 16) as de:
        planes = same(de, S.GIF, maps, 16, gt, None, scale=scale)[1]
        assert planes[0].max() == 255 and planes[0][0, 1] == min(scale, 255)
        same(de, S.SGM_INT, d16, 16, gt, None, scale=scale)
        same(de, S.SGM, d16, 16, gt, None, scale=scale)


# ---- the SGBM display conversion ----
def _tile(values):
    return np.resize(np.asarray(values, np.int16), (H8, 64))


SGM_MAPS = {
    "extremes": _tile([-16, 16 * 1023 + 8]),
    "range_extreme_invalid": _tile([(-1024 - 1) * 16, 0, 16 * 1023 + 8, -16400 + 1, 5000, -3]),
    "fp32_product_on_half": _tile([0, 510] + list(range(1, 125, 2))),                    # alpha = 0.5 exactly: odd v -> x.5
    "quarter_ties": _tile(list(range(256))),                                             # alpha = 1: m = v; 10 -> 2, 14 -> 4
    "flat": _tile([800]),
    "flat_invalid": _tile([-16]),
    "min_is_max_minus_1": _tile([100, 101]),
    "min_is_max_minus_1_negative": _tile([-16, -15]),
}


@pytest.mark.parametrize("case", sorted(SGM_MAPS))
def test_sgbm_display(psm, case):
    d16 = SGM_MAPS[case]
    gt = np.full((H8, 64), 40, np.uint8)
    with blank(psm, 64, H8, 16) as de:
        for scale in (1, 4):
            rec, planes, m = same(de, S.SGM, d16, 16, gt, None, scale=scale, thr=0)
            assert (rec["min_val"], rec["max_val"]) == (int(d16.min()), int(d16.max()))
            assert (rec["flags"] == S.FLAT) == case.startswith("flat")
            disp = planes[0]
            if case.startswith("flat"):
                assert not disp.any()
            if case == "quarter_ties" and scale == 1:
                assert disp[0, 10] == 2 and disp[0, 14] == 4 and disp[0, 2] == 0 and disp[0, 6] == 2 and disp.reshape(-1)[255] == 64
            if case == "fp32_product_on_half" and scale == 1:
                # v = 1, 3, 5, 7 -> 0.5, 1.5, 2.5, 3.5 -> 0, 2, 2, 4 (ties to even), then / 4
                assert disp[0, 2:6].tolist() == [0, 0, 0, 1] and disp[0, 1] == 64
            if case == "min_is_max_minus_1" and scale == 1:
                assert (disp == 64).all()                                                 # 255 * 100 saturates; 255 / 4 -> 64
            if case == "min_is_max_minus_1_negative":
                assert not disp.any()                                                     # negative products saturate to 0
            if case == "extremes":
                assert disp[0, 0] == 0 and disp[0, 1] == 64 * scale - (scale > 3)
        same(de, S.SGM_INT, d16, 16, gt, None)


# ---- the scored map is the current one, after every post-processing call ----
def test_scores_follow_post_processing(psm, golden):
    pair = golden("cones_pair.npz")
    gt, occl = pair["gt_l"], pair["occl"]
    with psm.DispEst(pair["l_bgr"], pair["r_bgr"], 64) as de:
        de.set_truth(gt, occl)
        de.CostConst_GPU()
        de.CostFilter_GPU()
        de.DispSelect_GPU()
        seen = []
        for step in (None, de.LRCheck_GPU, de.FillInv_GPU, de.WgtMedian_GPU, de.JointWMF_GPU):
            if step:
                step()
            rec = de.Score_GPU(S.GIF)
            l, r = (m.copy() for m in de.download_maps())
            equal(rec, de.score_maps(right=True), S.score(S.GIF, (l, r), gt, occl, 64))
            seen.append(rec["bad"])
        assert seen[0] == seen[1] and len(set(seen)) >= 3                       # the check changes no map; fill and medians do
        assert round(100.0 * seen[0] / gt.size, 2) == 14.50


# ---- refusals ----
def test_refusals(psm):
    from primestereomatch_amd import capi, synth
    l, r, _ = synth.make_pair(64, 16, 16, seed=3)
    with psm.DispEst(l, r, 16) as de:
        for source, word in ((S.GIF, "no disparity maps"), (S.SGM, "no SGM result"), (S.SGM_INT, "no SGM result"), (3, "source 3")):
            with pytest.raises(capi.PsmError, match=word):
                de.Score_GPU(source)
        with pytest.raises(capi.PsmError, match="no psm_score ran"):
            de.score_maps()
        for bad, word in (((0, 4, 1), "scale_factor 0"), ((4, 256, 1), "error_threshold 256"), ((4, 4, 3), "mask_mode 3")):
            with pytest.raises(capi.PsmError, match=word):
                de.set_score_params(*bad)
        de.set_rows(0, 8)                                   # maps that cover a row stripe only
        de.CostConst_GPU()
        de.CostFilter_GPU()
        de.DispSelect_GPU()
        with pytest.raises(capi.PsmError, match="row stripe"):
            de.Score_GPU(S.GIF)
        de.upload_sgm_map(np.zeros((16, 64), np.int16))
        de.Score_GPU(S.SGM)
        with pytest.raises(capi.PsmError, match="PSM_SCORE_GIF only"):
            de.score_maps(right=True)
        de.upload_sgm_map(None)
        with pytest.raises(capi.PsmError, match="no SGM result"):
            de.Score_GPU(S.SGM)


def test_truth_survives_release_scratch(psm):
    g = rnd(11)
    W, D = 67, 16
    maps = (g.integers(0, 64, (H8, W)).astype(np.uint8), g.integers(0, 64, (H8, W)).astype(np.uint8))
    gt, mask = g.integers(0, 256, (H8, W)).astype(np.uint8), g.choice(MASK_VALUES, (H8, W))
    from primestereomatch_amd import capi
    with blank(psm, W, H8, D) as de:
        rec = same(de, S.GIF, maps, D, gt, mask)[0]
        de.release_scratch()
        with pytest.raises(capi.PsmError, match="no psm_score ran"):
            de.score_maps()
        again = de.Score_GPU(S.GIF)                          # the truth, the mask and the maps are still there
        assert again == rec
        equal(again, de.score_maps(right=True), S.score(S.GIF, maps, gt, mask, D))


# ---- batches ----
@functools.lru_cache(maxsize=None)
def batch_inputs(n):
    g = rnd(100 + n)
    W, H = 130, 9
    out = []
    for _ in range(n):
        out.append({"maps": (g.integers(0, 256, (H, W)).astype(np.uint8), g.integers(0, 256, (H, W)).astype(np.uint8)),
                    "d16": g.integers(-16, 16 * 64, (H, W)).astype(np.int16),
                    "gt": g.integers(0, 256, (H, W)).astype(np.uint8), "mask": g.choice(MASK_VALUES, (H, W))})
    return out


@pytest.mark.parametrize("n", (1, 3, 8))
def test_batch_equals_single_calls(psm, n):
    from primestereomatch_amd import dispest
    D = 16
    ins = batch_inputs(n)
    des = [blank(psm, 130, 9, D) for _ in range(n)]
    try:
        for source in (S.GIF, S.SGM, S.SGM_INT):
            single = []
            for de, x in zip(des, ins):
                data = x["maps"] if source == S.GIF else x["d16"]
                rec, planes, _ = same(de, source, data, D, x["gt"], x["mask"], scale=3, thr=1)
                single.append((rec, planes))
            recs = dispest.score_batch(des, source)
            for de, rec, (srec, splanes) in zip(des, recs, single):
                assert rec == srec
                planes = de.score_maps(right=source == S.GIF)
                assert all(np.array_equal(a, b) for a, b in zip(planes, splanes))
            assert len({r["err_sum"] for r in recs}) == n                         # (every context scored its own result)
            for de, (srec, splanes) in zip(des, single):                         # ... and is where its own psm_score leaves it
                assert de.Score_GPU(source) == srec
                assert all(np.array_equal(a, b) for a, b in zip(de.score_maps(right=source == S.GIF), splanes))
    finally:
        for de in des:
            de.close()


def test_batch_refusals_name_the_context(psm):
    from primestereomatch_amd import capi, dispest
    ins = batch_inputs(3)
    des = [blank(psm, 130, 9, 16) for _ in range(3)]
    try:
        for de, x in zip(des, ins):
            de.upload_maps(*x["maps"])
            de.set_truth(x["gt"], x["mask"])
        des[2].clear_truth()
        with pytest.raises(capi.PsmError, match="context 2 has no ground truth"):
            dispest.score_batch(des, S.GIF)
        des[2].set_truth(ins[2]["gt"], ins[2]["mask"])
        des[1].set_score_params(4, 5, S.MASK_NONOCC)
        with pytest.raises(capi.PsmError, match="context 1 has other score parameters"):
            dispest.score_batch(des, S.GIF)
        des[1].set_score_params(4, 4, S.MASK_NONOCC)
        with pytest.raises(capi.PsmError, match="context 0: no SGM result"):
            dispest.score_batch(des, S.SGM)
        with blank(psm, 131, 9, 16) as other:
            other.upload_maps(np.zeros((9, 131), np.uint8), np.zeros((9, 131), np.uint8))
            with pytest.raises(capi.PsmError, match="context 3 has another width"):
                dispest.score_batch(des + [other], S.GIF)
        assert len(dispest.score_batch(des, S.GIF)) == 3
    finally:
        for de in des:
            de.close()


# ---- frames in flight ----
def test_frame_ring_with_a_truth(psm):
    from primestereomatch_amd import synth
    W, H, D = 130, 9, 16
    frames = [synth.make_pair(W, H, D, seed=20 + i)[:2] for i in range(5)]
    g = rnd(5)
    gt, mask = g.integers(0, 4 * D, (H, W)).astype(np.uint8), g.choice(MASK_VALUES, (H, W))

    def run(**kw):
        out = []
        with psm.FrameRing(frames[0][0], frames[0][1], D, frames=2, **kw) as ring:
            for l, r in frames:
                done = ring.push(l, r)
                if done is not None:
                    out.append(done)
            out.extend(ring.flush())
        return out

    plain, scored = run(), run(truth=(gt, mask), scale_factor=4, error_threshold=1)
    assert len(plain) == len(scored) == 5 and all(len(p) == 2 for p in plain) and all(len(s) == 3 for s in scored)
    with blank(psm, W, H, D) as de:
        for (pl, pr), (sl, sr, rec) in zip(plain, scored):
            assert np.array_equal(pl, sl) and np.array_equal(pr, sr)
            sync = same(de, S.GIF, (sl, sr), D, gt, mask, scale=4, thr=1)[0]       # the synchronous call, and the model
            assert rec == sync
    assert len({s[2]["bad"] for s in scored}) > 1


# ---- the harness: the device tail equals the numpy tail, key for key ----
def _same_records(a, b):
    assert set(a) == set(b)
    for k in a:
        if k.endswith("_ms"):
            continue
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
        else:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k


@pytest.mark.parametrize("algo", ("gif", "sgbm"))
def test_harness_device_tail_single(psm, golden, algo):
    from primestereomatch_amd import harness
    p = golden("cones_pair.npz")
    f = harness.compute if algo == "gif" else harness.compute_sgbm
    for mask in (p["occl"], None):
        host = f(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], mask)
        dev = f(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], mask, device_tail=True)
        _same_records(host, dev)
        assert "bp_percent" in dev and ("bp_percent_int" in dev) == (algo == "sgbm")
    _same_records(f(p["l_bgr"], p["r_bgr"], 64), f(p["l_bgr"], p["r_bgr"], 64, device_tail=True))      # no truth: the display map alone


@pytest.mark.parametrize("algo", ("gif", "sgbm"))
def test_harness_device_tail_batch(psm, golden, algo):
    from primestereomatch_amd import harness
    ps = [golden("cones_pair.npz"), golden("teddy_pair.npz")]
    pairs, gts, masks = [(p["l_bgr"], p["r_bgr"]) for p in ps], [p["gt_l"] for p in ps], [p["occl"] for p in ps]
    f = harness.compute_batch if algo == "gif" else harness.compute_sgbm_batch
    host, dev = f(pairs, 64, gts, masks), f(pairs, 64, gts, masks, device_tail=True)
    assert len(host) == len(dev) == 2
    for a, b in zip(host, dev):
        _same_records(a, b)
    assert host[0]["bad_pixels"] != host[1]["bad_pixels"]
