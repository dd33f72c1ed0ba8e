"""-m gpu: the batch entry of the WLS smoothing stage (psm_wls_filter_batch: psm_wls_filter of several contexts in one set of
1 + 2 T launches, the context on a grid axis of its own) against the stage's definition, tests/wls_model.py, and against the
member's own single call on a second context.  Every comparison is of bit patterns - the int16 maps, and the float planes and the
table as uint32 - with 0 differing: there is no tolerance anywhere in this file.  The maps are injected (psm_score_upload_sgm_map,
psm_upload_maps), so no matcher runs except where a test is about one.

The shapes are those of tests/test_gpu_wls.py, whose docstring explains them: the smallest ones on the edges of the kernels' tiles,
waves and chunks.  What a batch adds is the member axis: every member has its own map, holes, guide, lambda and sigma, so a member
that read another's record, table or planes would differ from its model."""
import ctypes as C

import numpy as np
import pytest

import depth_model as DM
import score_model as SM
import wls_model as M
from test_gpu_wls import equal, fetch, hip_runtime, holes, noise, refused, rnd, smooth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def case(guide, v, dmin=0, **params):
    """a member: its guide, its int16 map (through the hook plane), the minDisparity of its range and its setWLS parameters"""
    return {"guide": guide, "v": v, "dmin": dmin, "params": params}


def member(W, H, i, seed=0, **params):
    """member i of a batch: guides alternate between noise and smooth, every member has holes of its own"""
    guide = noise(W, H, seed + i) if i % 2 == 0 else smooth(W, H, seed + i)
    return case(guide, holes(W, H, seed + 7 * i + 1), **params)


def model_of(c):
    return M.wls(c["v"], (c["dmin"] - 1) * 16, DM.quantise(c["guide"]), **c["params"])


def context(psm, c, D=8):
    de = psm.DispEst(c["guide"], c["guide"], D)
    prepare(de, c)
    return de


def prepare(de, c):
    de.setWLS(**c["params"])
    if c["dmin"]:
        de._ck(de._lib.psm_sgm_set_range(de._h, c["dmin"], 0), "set_range")
    de.upload_sgm_map(c["v"])


def single(psm, c, D=8):
    """the member's own psm_wls_filter on a second context"""
    with context(psm, c, D) as de:
        de.WLS_GPU(psm.capi.PSM_WLS_SGM)
        return fetch(de)


class Members:
    def __init__(self, psm, cases, D=8):
        self.des = []
        try:
            for c in cases:
                self.des.append(context(psm, c, D))
        except Exception:
            self.close()
            raise

    def close(self):
        for de in self.des:
            de.close()

    def __enter__(self):
        return self.des

    def __exit__(self, *exc):
        self.close()


def check(psm, des, cases, singles=True, **kw):
    """one batch over `des`; every member against its model and its own single call -> what the members hold, and the models"""
    maps = psm.wls_batch(des, **kw)
    got, models = [fetch(de) for de in des], [model_of(c) for c in cases]
    for g, m, c, w16 in zip(got, models, cases, maps):
        equal(g, m)
        assert np.array_equal(w16, m["disp"])
        if singles:
            equal(g, single(psm, c))
    return got, models


# ---- the member axis ----
@pytest.mark.parametrize("n", (1, 2, 3, 8))
@pytest.mark.parametrize("W,H", ((65, 9), (9, 65), (70, 130)))
def test_batch_sizes(psm, W, H, n):
    cases = [member(W, H, i, seed=W + n) for i in range(n)]
    with Members(psm, cases) as des:
        got, _ = check(psm, des, cases)
        assert len({g["disp"].tobytes() for g in got}) == n                            # n different members, n different results


def test_members_are_isolated_from_each_other(psm):
    W, H = 70, 130
    tiny = np.float32(np.finfo(np.float32).tiny)
    flat = np.full((H, W, 3), 90, np.uint8)
    void = np.full((H, W), -16, np.int16)
    one = void.copy()
    one[7, 33] = 555
    ext = rnd(5).choice(np.array([-32768, 32767, -16], np.int16), (H, W))
    cases = [case(noise(W, H, 70), holes(W, H, 70)),                                  # subnormal and zero den (asserted below)
             case(flat, void),                                                        # all invalid
             case(flat, one),                                                         # a single valid pixel
             case(smooth(W, H, 2), ext),                                              # the int16 extremes
             case(smooth(W, H, 3), holes(W, H, 3), lam=4.0e6, sigma=250.0),
             case(noise(W, H, 4), holes(W, H, 4), lam=1.0e-3, sigma=1.0e-3)]
    with Members(psm, cases) as des:
        got, models = check(psm, des, cases)
    den = models[0]["den"]
    assert ((den > 0) & (den < tiny)).sum() > 20 and (den == 0).sum() > 20             # what pins that subnormals are kept
    assert (models[0]["disp"] == -16).any() and (models[0]["disp"] != -16).any()
    assert (got[1]["disp"] == -16).all() and (got[1]["q"].view(np.uint32) == M.VOID_BITS).all() and (got[1]["den"] == 0).all()
    assert (got[2]["disp"] == 555).all()
    assert (ext == 32767).any() and (ext == -32768).any() and got[3]["disp"].min() >= -16   # the extremes went in, the result stays in range
    assert not np.array_equal(got[4]["tab"], got[5]["tab"])                            # every member read its own table


@pytest.mark.parametrize("W,H", ((64, 9), (129, 10), (10, 129), (8, 8), (8, 1500)))
def test_seams(psm, W, H):
    cases = [member(W, H, i, seed=H) for i in range(3)]
    with Members(psm, cases) as des:
        check(psm, des, cases)


@pytest.mark.parametrize("T", (1, 4))
def test_iterations(psm, T):
    W, H = 65, 70
    cases = [member(W, H, i, seed=T, lam=50.0 * (i + 1), sigma=1.0 + i, iterations=T) for i in range(3)]
    with Members(psm, cases) as des:
        got, _ = check(psm, des, cases)
        des[2].setWLS(lam=150.0, sigma=3.0, iterations=T % 4 + 1)                      # another T on one member: the launch count is the batch's
        with pytest.raises(psm.capi.PsmError):
            psm.wls_batch(des)
        msg = psm.capi.last_error(des[0]._h)
        assert msg.startswith("psm_wls_filter_batch:") and "context 2" in msg and "iterations" in msg, msg
        for de, g in zip(des, got):
            equal(fetch(de), g)


def test_gif_source_with_and_without_the_mask(psm):
    capi = psm.capi
    W, H, D = 65, 12, 8
    r = rnd(17)
    guides = [smooth(W, H, 3), noise(W, H, 3)]
    lmaps = [r.integers(0, D, (H, W), dtype=np.uint8) for _ in range(2)]
    lvs = [(r.random((H, W)) < 0.7).astype(np.uint8) * 255 for _ in range(2)]
    lvs[0][0, :4] = [0, 1, 255, 128]                                                  # any non-zero byte is valid
    des = [psm.DispEst(g, g, D) for g in guides]
    try:
        for de, lmap, lv in zip(des, lmaps, lvs):
            de.upload_maps(lmap, lmap, lv, lv)
        for mask in (False, True):
            psm.wls_batch(des, capi.PSM_WLS_GIF, use_mask=mask)
            for de, g, lmap, lv in zip(des, guides, lmaps, lvs):
                got = fetch(de)
                equal(got, M.wls(*M.gif_source(lmap, lv if mask else None), g))
                with psm.DispEst(g, g, D) as alone:                                   # the member's own single call
                    alone.upload_maps(lmap, lmap, lv, lv)
                    alone.WLS_GPU(capi.PSM_WLS_GIF, use_mask=mask)
                    equal(got, fetch(alone))
        keep = [fetch(de) for de in des]
        des[1].upload_maps(lmaps[1], lmaps[1])                                        # member 1 loses its mask
        with pytest.raises(psm.capi.PsmError):
            psm.wls_batch(des, capi.PSM_WLS_GIF, use_mask=True)
        msg = capi.last_error(des[0]._h)
        assert msg.startswith("psm_wls_filter_batch: context 1:") and "PSM_WLS_USE_MASK" in msg and "mask" in msg, msg
        for de, k in zip(des, keep):
            equal(fetch(de), k)
    finally:
        for de in des:
            de.close()


def test_one_channel_float_and_uint8_guides_in_one_batch(psm):
    capi = psm.capi
    W, H, D = 65, 12, 8
    left8 = noise(W, H, 8) // 16
    leftf = rnd(21).random((H, W, 3)).astype(np.float32) * np.float32(1.2) - np.float32(0.1)       # some outside [0, 1]: saturation
    gl, gr = rnd(23).integers(0, 32, (H, W), dtype=np.uint8), rnd(24).integers(0, 32, (H, W), dtype=np.uint8)
    v8, vf = holes(W, H, 7), holes(W, H, 8)
    with psm.DispEst(left8, left8, D) as a, psm.DispEst(leftf, leftf, D) as b, psm.DispEst(left8, left8, D) as c:
        a.upload_sgm_map(v8)
        b.upload_sgm_map(vf)
        m16 = c.SGBM_GPU(gray=(gl, gr))                                               # its left plane guides, as one channel
        psm.wls_batch([a, b, c])
        want = [M.wls(v8, -16, left8), M.wls(vf, -16, DM.quantise(leftf)), M.wls(m16, -16, gl)]
        got = [fetch(de) for de in (a, b, c)]
        for g, w in zip(got, want):
            equal(g, w)
        for de, g in zip((a, b, c), got):                                             # ... and each member's own single call on itself
            de.WLS_GPU(capi.PSM_WLS_SGM)
            equal(fetch(de), g)


# ---- behind a real matcher ----
def test_golden_pairs_through_sgbm_batch_then_wls_batch(psm, golden):
    from primestereomatch_amd import dispest
    capi = psm.capi
    pairs = [golden(f"{name}_pair.npz") for name in ("cones", "teddy")]
    wants = [golden(f"{name}_wls.npz") for name in ("cones", "teddy")]
    des = [psm.DispEst(p["l_bgr"], p["r_bgr"], 64) for p in pairs]
    try:
        d16s = dispest.sgbm_batch(des)
        maps = psm.wls_batch(des)
        for de, p, want, d16, w16 in zip(des, pairs, wants, d16s, maps):
            got = fetch(de)
            assert np.array_equal(got["disp"], want["disp"]) and np.array_equal(w16, want["disp"])      # the committed map ...
            equal(got, M.wls(d16, -16, p["l_bgr"]))                                    # ... every plane of the model on the device's own SGM map
            with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as alone:                     # ... and the single sequence
                assert np.array_equal(alone.SGBM_GPU(), d16)
                alone.WLS_GPU(capi.PSM_WLS_SGM)
                equal(got, fetch(alone))
    finally:
        for de in des:
            de.close()


def test_another_min_disparity_behind_sgbm_batch(psm, golden):
    from primestereomatch_amd import dispest
    crops = []
    for name in ("cones", "teddy"):
        p = golden(f"{name}_pair.npz")
        crops.append((np.ascontiguousarray(p["l_bgr"][100:196, 200:360]), np.ascontiguousarray(p["r_bgr"][100:196, 200:360])))
    des = [psm.DispEst(l, r, 32) for l, r in crops]
    try:
        d16s = dispest.sgbm_batch(des, min_disparity=3, num_disparities=24)
        psm.wls_batch(des)
        for de, (l, r), d16 in zip(des, crops, d16s):
            got = fetch(de)
            assert (d16 == 32).any() and got["disp"].min() >= 32                       # invalid = (3 - 1) * 16, clamped to inv + 1 from below
            equal(got, M.wls(d16, 32, l))
            with psm.DispEst(l, r, 32) as alone:
                assert np.array_equal(alone.SGBM_GPU(min_disparity=3, num_disparities=24), d16)
                alone.WLS_GPU(psm.capi.PSM_WLS_SGM)
                equal(got, fetch(alone))
    finally:
        for de in des:
            de.close()


# ---- refusals ----
def test_refusals_on_live_contexts_leave_every_previous_result(psm, golden):
    capi = psm.capi
    lib = capi.load()
    W, H, D = 64, 16, 16
    cases = [member(W, H, i, seed=11, lam=10.0 + i, sigma=2.0 + i, iterations=2) for i in range(3)]
    lmap = np.ones((H, W), np.uint8)

    def call(des, source=capi.PSM_WLS_SGM, flags=0, n=None):
        arr = (C.c_void_p * len(des))(*[d._h if d is not None else None for d in des])
        return lib.psm_wls_filter_batch(arr, len(des) if n is None else n, source, flags)

    with Members(psm, cases, D) as des:
        a, b, c = des
        for de in des:
            de.upload_maps(lmap, lmap)                                                # (GIF maps without a mask)
        keep, _ = check(psm, des, cases, singles=False)

        def refuse(rc, *words):
            """non-zero, the message on context 0 names the member, every member still downloads its previous result"""
            refused(psm, a, rc, "psm_wls_filter_batch:", *words)
            for de, k in zip(des, keep):
                equal(fetch(de), k)

        refuse(call([a, None, c]), "context 1 is NULL")
        refuse(call([a, b, a]), "context 2 appears twice")
        refuse(call([a] * 4097), "4097 contexts", "4096")
        refuse(call(des, source=2), "source 2")
        refuse(call(des, source=-1), "source -1")
        refuse(call(des, flags=2), "flag bits 0x2")
        refuse(call(des, flags=capi.PSM_WLS_USE_MASK), "PSM_WLS_USE_MASK", "SGM source")
        refuse(call(des, capi.PSM_WLS_GIF, capi.PSM_WLS_USE_MASK), "context 0:", "PSM_WLS_USE_MASK", "mask")
        # calls no context can receive the message of: it is psm_last_error(NULL)'s
        for args, word in (((None, 3, capi.PSM_WLS_SGM, 0), "NULL"), (((C.c_void_p * 1)(a._h), 0, capi.PSM_WLS_SGM, 0), "n 0"),
                           (((C.c_void_p * 2)(None, a._h), 2, capi.PSM_WLS_SGM, 0), "context 0 is NULL")):
            assert lib.psm_wls_filter_batch(*args) != 0
            assert capi.last_error(None).startswith("psm_wls_filter_batch:") and word in capi.last_error(None)
        # another geometry, another number of iterations
        for (w, h), word in (((W + 8, H), "width"), ((W, H + 8), "height")):
            g = smooth(w, h, 1)
            with psm.DispEst(g, g, D) as other:
                other.setWLS(iterations=2)
                other.upload_sgm_map(holes(w, h, 1))
                refuse(call([a, b, other]), "context 2", word)
        b.setWLS(lam=11.0, sigma=3.0, iterations=3)
        refuse(call(des), "context 1", "iterations 3")
        b.setWLS(lam=11.0, sigma=3.0, iterations=2)
        # what psm_wls_filter refuses about a context, by member
        c.upload_sgm_map(None)                                                        # member 2 loses its SGM source
        refuse(call(des), "context 2:", "no SGM result")
        c.upload_sgm_map(cases[2]["v"])
        h = C.c_void_p()
        assert lib.psm_create(C.byref(h), W, H, D, capi.PSM_F32, 0) == 0              # a bare context: no pair, no maps
        try:
            arr = (C.c_void_p * 3)(a._h, b._h, h)
            assert lib.psm_wls_set_params(h, 8000.0, 1.5, 2) == 0
            assert lib.psm_score_upload_sgm_map(h, cases[0]["v"].ctypes.data_as(C.c_void_p), 0) == 0
            refuse(lib.psm_wls_filter_batch(arr, 3, capi.PSM_WLS_SGM, 0), "context 2:", "no current image pair")
            refuse(lib.psm_wls_filter_batch(arr, 3, capi.PSM_WLS_GIF, 0), "context 2:", "no disparity maps")
        finally:
            lib.psm_destroy(h)
        p = golden("cones_pair.npz")
        l, r = np.ascontiguousarray(p["l_bgr"][:H, :W]), np.ascontiguousarray(p["r_bgr"][:H, :W])
        with psm.DispEst(l, r, D) as stripe:                                          # maps that cover a row stripe only
            stripe.setWLS(iterations=2)
            stripe.set_rows(0, 8)
            stripe.CostConst_GPU(); stripe.CostFilter_GPU(); stripe.DispSelect_GPU()
            refuse(call([a, stripe, c], capi.PSM_WLS_GIF), "context 1:", "row stripe")
        check(psm, des, cases, singles=False)                                          # ... and the batch still runs


# ---- the table of the members' records ----
def test_table_reuse(psm):
    W, H = 65, 20
    cases = [member(W, H, i, seed=31) for i in range(4)]
    with Members(psm, cases) as des:
        check(psm, des, cases, singles=False)
        for i, (de, c) in enumerate(zip(des, cases)):                                 # the same list, other parameters (and another map)
            c["params"] = {"lam": 30.0 * (i + 1), "sigma": 0.5 + i, "iterations": 2}
            c["v"] = holes(W, H, 40 + i)
            prepare(de, c)
        check(psm, des, cases, singles=False)
        check(psm, des[::-1], cases[::-1], singles=False)                              # the reversed list: another first context, another table
        check(psm, des[1:3], cases[1:3], singles=False)                                # a subset with another first context
        des[0].release_scratch()                                                      # the old first context gives its planes and its table back
        prepare(des[0], cases[0])
        check(psm, des, cases)


def test_a_single_call_between_two_batches(psm):
    W, H = 65, 20
    cases = [member(W, H, i, seed=51) for i in range(3)]
    with Members(psm, cases) as des:
        before, _ = check(psm, des, cases, singles=False)
        cases[1]["params"] = {"lam": 3.0, "sigma": 9.0, "iterations": 3}
        prepare(des[1], cases[1])
        des[1].WLS_GPU(psm.capi.PSM_WLS_SGM)
        equal(fetch(des[1]), model_of(cases[1]))
        for i in (0, 2):                                                              # nothing of the other members changed
            equal(fetch(des[i]), before[i])
        check(psm, des, cases, singles=False)


# ---- the options of context 0 ----
def test_async_on_a_callers_stream(psm):
    capi = psm.capi
    W, H = 129, 70
    cases = [member(W, H, i, seed=15) for i in range(3)]
    hip = hip_runtime()
    stream = C.c_void_p()
    with Members(psm, cases) as des:
        assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0                   # hipStreamNonBlocking
        des[0].set_stream(stream.value)
        des[0].set_option(capi.PSM_OPT_ASYNC, 1)
        assert psm.wls_batch(des) is None                                             # the call returns behind the launches
        for de in des:
            de.wls_wait()                                                             # ... and every member collects
            refused(psm, de, de._lib.psm_wls_wait(de._h), "psm_wls_wait:", "no asynchronous")
        for de, c in zip(des, cases):
            equal(fetch(de), model_of(c))
        assert psm.wls_batch(des) is None                                             # the downloads wait for an asynchronous run too
        for de, c in zip(des[::-1], cases[::-1]):
            equal(fetch(de), model_of(c))
        des[0].set_option(capi.PSM_OPT_ASYNC, 0)
        des[0].set_stream(None)
        des[0].synchronize()
        assert hip.hipStreamDestroy(stream) == 0


def test_profile_time_is_context_0s(psm):
    W, H = 65, 12
    cases = [member(W, H, i, seed=16) for i in range(2)]
    with Members(psm, cases) as des:
        des[0].set_option(psm.capi.PSM_OPT_PROFILE, 1)
        check(psm, des, cases, singles=False)
        assert 0.0 < des[0].wls_time() < 1000.0
        refused(psm, des[1], des[1]._lib.psm_wls_time(des[1]._h, C.byref(C.c_double())), "psm_wls_time:", "not timed")


# ---- publishing ----
def test_publishing_feeds_the_batched_readers(psm):
    from primestereomatch_amd import dispest
    capi = psm.capi
    W, H, D = 70, 40, 8
    Q = DM.q_from_projections([[700.0, 0, 30.0, 0], [0, 700.0, 20.0, 0], [0, 0, 1, 0]], [[700.0, 0, 30.0, -84000.0], [0, 700.0, 20.0, 0], [0, 0, 1, 0]])
    guides = [noise(W, H, 17 + i) for i in range(3)]
    gts = [rnd(18 + i).integers(0, 4 * D, (H, W), dtype=np.uint8) for i in range(3)]
    des = [psm.DispEst(g, np.roll(g, -3, axis=1), D) for g in guides]                 # disparity 3, holes along the left border
    try:
        for i, (de, gt) in enumerate(zip(des, gts)):
            de.setReprojection(Q)
            de.set_score_params(4, 1, capi.PSM_MASK_NONE)
            de.set_truth(gt)
            de.setWLS(lam=40.0 + i, sigma=60.0, iterations=2)
        m16s = dispest.sgbm_batch(des)                                                # a compute's maps under the filter
        w16s = psm.wls_batch(des)
        for i, (m16, w16, g) in enumerate(zip(m16s, w16s, guides)):
            assert np.array_equal(w16, M.wls(m16, -16, g, 40.0 + i, 60.0, 2)["disp"]) and not np.array_equal(w16, m16)
        for de in des[:2]:
            de.wls_publish(True)
        read = [w16s[0], w16s[1], m16s[2]]                                            # member 2, left unpublished, gives its unfiltered map
        outputs = capi.PSM_DEPTH_XYZ | capi.PSM_DEPTH_Z | capi.PSM_DEPTH_CLOUD
        counts = dispest.reproject_batch(des, capi.PSM_DEPTH_SGM, outputs)
        for de, d, g, count in zip(des, read, guides, counts):
            model = DM.reproject(d.astype(np.float64) * 0.0625, d == -16, Q, (0, 0), (0.0, DM.FLT_MAX), g)
            xyz, z = de.reprojected()
            cloud = de.cloud()
            assert count == len(model[2]) == len(cloud) and cloud.tobytes() == model[2].tobytes()
            assert np.array_equal(xyz.view(np.uint32), model[0].view(np.uint32)) and np.array_equal(z.view(np.uint32), model[1].view(np.uint32))
        for source, name in ((capi.PSM_SCORE_SGM, SM.SGM), (capi.PSM_SCORE_SGM_INT, SM.SGM_INT)):
            recs = dispest.score_batch(des, source)
            for de, d, gt, rec in zip(des, read, gts, recs):
                want = SM.score(name, d, gt, None, D, 4, 1, SM.MASK_NONE)
                ldisp, emap = de.score_maps()
                assert np.array_equal(ldisp, want["ldisp"]) and np.array_equal(emap, want["emap"])
                for k in ("min_val", "max_val", "pixels", "bad", "err_sum", "unit", "flags"):
                    assert rec[k] == want[k], k
    finally:
        for de in des:
            de.close()


# ---- the upper layers ----
@pytest.mark.parametrize("lr_check", (False, True))
def test_frame_ring_delivers_each_frame_its_filtered_map(psm, lr_check):
    from primestereomatch_amd import synth
    capi = psm.capi
    W, H, D = 65, 12, 8
    frames = [synth.make_pair(W, H, D, seed=s)[:2] for s in range(4)]
    with psm.FrameRing(frames[0][0], frames[0][1], D, frames=2, lr_check=lr_check, wls={}) as ring:
        got = []
        for l, r in frames:
            out = ring.push(l, r)
            if out is not None:
                got.append(out)
        got += ring.flush()
    assert len(got) == 4
    for (l, r), out in zip(frames, got):
        assert len(out) == 3 and out[2].dtype == np.int16 and out[2].shape == (H, W)
        with psm.DispEst(l, r, D) as de:                                              # a plain DispEst through the same stages
            de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
            if lr_check:
                de.LRCheck_GPU()
            de.WLS_GPU(capi.PSM_WLS_GIF, use_mask=lr_check)
            assert np.array_equal(out[0], de.lDisMap) and np.array_equal(out[2], de.wls_map())
            lv = de.lValid if lr_check else None
        assert np.array_equal(out[2], M.wls(*M.gif_source(out[0], lv), DM.quantise(l))["disp"])
    if not lr_check:
        with psm.FrameRing(frames[0][0], frames[0][1], D, frames=2) as ring:          # without the argument the tuples are as before
            ring.push(*frames[0])
            assert all(len(out) == 2 for out in ring.flush())


def test_harness_batch_gives_the_single_records(psm, golden):
    from primestereomatch_amd import harness
    Q = DM.q_from_projections([[700.0, 0, 200.0, 0], [0, 700.0, 180.0, 0], [0, 0, 1, 0]], [[700.0, 0, 200.0, -84000.0], [0, 700.0, 180.0, 0], [0, 0, 1, 0]])
    ps = [golden(f"{name}_pair.npz") for name in ("cones", "teddy")]
    pairs = [(p["l_bgr"], p["r_bgr"]) for p in ps]
    gts, masks = [p["gt_l"] for p in ps], [p["occl"] for p in ps]
    outs = harness.compute_sgbm_batch(pairs, 64, gts=gts, masks=masks, wls={}, depth=Q)
    times = {"cost_ms", "paths_ms", "select_ms"}
    for (l, r), gt, mask, out, name in zip(pairs, gts, masks, outs, ("cones", "teddy")):
        want = harness.compute_sgbm(l, r, 64, gt=gt, mask=mask, wls={}, depth=Q)
        assert set(out) == set(want) and {"wls16", "bp_percent_wls", "xyz", "z", "cloud"} <= set(out)
        for k in set(want) - times:
            if isinstance(want[k], np.ndarray):
                assert out[k].dtype == want[k].dtype and out[k].tobytes() == want[k].tobytes(), k
            else:
                assert out[k] == want[k], k
        assert np.array_equal(out["wls16"], golden(f"{name}_wls.npz")["disp"])
    plain = harness.compute_sgbm_batch(pairs, 64, gts=gts, masks=masks)                # the defaults add nothing
    assert all(not ({"wls16", "bp_percent_wls", "xyz", "z", "cloud"} & set(o)) for o in plain)
