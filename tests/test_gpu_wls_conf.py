"""-m gpu: psm_wls_filter with PSM_WLS_CONFIDENCE - k_sgm_right16, k_wls_conf and the weighted start of k_wls_init - against its
definition, tests/wls_conf_model.py.  Every comparison is of integers or of bit patterns (right16, conf, disp; num, den and q as
uint32) with 0 differing: there is no tolerance anywhere in this file.  S and the int16 map are the SGM stage's own (downloaded:
its agreement with its model is test_gpu_sgm*.py's subject), on seeded noise pairs, with the SAD and the census cost.

Shapes (W, H, D, dmin).  A context is at least 8 x 8, so rows are 8 where the kernel's row count plays no part (k_sgm_right16: one
workgroup per row, whatever H is):
    (70, 8, 8, 0)                        a wave edge in the row of k_sgm_right16 (threads 64 .. 69 of the gather loop)
    (64, 8, 64, 0), (65, 8, 65, 0)       the per-lane count's edge: 1 disparity per lane, full; 2 per lane with one live in the second
    (33, 8, 16, 20)                      trailing columns without a candidate
    (40, 8, 300, -7)                     the wide form (8 per lane, 10 key bits in use) and landing columns right of x
    (200, 8, 130, 0)                     4 per lane, more disparities than most columns have candidates
    (8, 8, 2, 0)                         the smallest image and range the SGM stage accepts
    (63 | 64 | 65) x (11 | 12 | 13)      one below, at and one above the 64 x 4 tile of k_wls_conf
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import depth_model as DM
import fuzz_inputs as F
import wls_conf_model as CM
import wls_model as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = ((70, 8, 8, 0), (64, 8, 64, 0), (65, 8, 65, 0), (33, 8, 16, 20), (40, 8, 300, -7), (200, 8, 130, 0), (8, 8, 2, 0))
TILE_EDGES = tuple((W, H, 16, 0) for W in (63, 64, 65) for H in (11, 12, 13))


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def rnd(seed):
    return np.random.default_rng(seed)


def noise_pair(W, H, shift, seed):
    """a left image of smoothed noise and the right one it becomes `shift` columns further left, plus a little noise of its own"""
    r = rnd(seed)
    base = r.integers(0, 256, (H, W + abs(shift), 3)).astype(np.int64)
    base = (base + np.roll(base, 1, 1) + np.roll(base, 1, 0)) // 3
    a = max(-shift, 0)                                              # L[x] = base[a + x], R[x] = L[x + shift]
    l = base[:, a:a + W]
    rr = np.clip(base[:, a + shift:a + shift + W] + r.integers(-3, 4, l.shape), 0, 255)
    return np.ascontiguousarray(l.astype(np.uint8)), np.ascontiguousarray(rr.astype(np.uint8))


def fetch(de, right=True):
    q, num, den = de.wls_planes()
    conf, r16 = de.download_wls_confidence(right)
    return {"disp": de.wls_map(), "q": q, "num": num, "den": den, "conf": conf, "right16": r16}


def equal(got, model):
    for k in ("right16", "conf", "disp"):
        if model[k] is None:
            assert got[k] is None, k
        else:
            assert got[k].dtype == model[k].dtype and np.array_equal(got[k], model[k]), (k, int((got[k] != model[k]).sum()))
    for k in ("num", "den", "q"):
        assert np.array_equal(got[k].view(np.uint32), model[k].view(np.uint32)), (k, int((got[k].view(np.uint32) != model[k].view(np.uint32)).sum()))


def flagged(psm, de, guide, dmin, conf, wls=None, S=None, m16=None):
    """one flagged psm_wls_filter of the context's SGM result against the model -> (got, model)"""
    if m16 is None:
        m16 = de.sgm_disparity()
    if S is None and conf.get("terms", 3) & CM.LR:
        S = de.sgm_costs()[1]
    de.setWLS(**(wls or {}))
    de.WLS_GPU(psm.capi.PSM_WLS_SGM, confidence=conf)
    right = bool(conf.get("terms", 3) & CM.LR)
    got = fetch(de, right)
    model = CM.wls(m16, (dmin - 1) * 16, DM.quantise(guide), S=S, dmin=dmin, **(wls or {}), **conf)
    equal(got, model)
    return got, model


# (the tile edges of k_wls_conf do not depend on the cost: one of them runs with the census cost too)
@pytest.mark.parametrize("W,H,D,dmin,cost", tuple(s + ("sad",) for s in SHAPES + TILE_EDGES) + tuple(s + ("census",) for s in SHAPES + TILE_EDGES[:1]))
def test_shapes(psm, W, H, D, dmin, cost):
    l, r = noise_pair(W, H, min(max(dmin + D // 3, -W // 2), W // 2), W + H + D)
    with psm.DispEst(l, r, 8) as de:
        m16 = de.SGBM_GPU(min_disparity=dmin, num_disparities=D, uniqueness_ratio=5, census=(5, 5) if cost == "census" else None)
        got, model = flagged(psm, de, l, dmin, {}, m16=m16)
        rinv = CM.rinv_of(dmin)
        none = got["right16"] == rinv
        if (W, H, D, dmin) == (33, 8, 16, 20):
            assert none[:, -20:].all() and not none[:, :-20].any()
        if (D, dmin) == (16, 0):
            assert len(np.unique(got["conf"])) > 2                  # graded, not binary (the pair's true disparity lies in the range)


@pytest.mark.parametrize("W,H,D,d_star,bs", (F.SATURATING_CASES[1], F.SATURATING_CASES[3]))
def test_saturating_pairs(psm, W, H, D, d_star, bs):
    """S = 524 280 = 8 * 65535 in the volume: keys that use all 29 bits, sub-pixel sums of the largest costs"""
    l, r = F.saturating_pair(W, H, D, d_star)
    with psm.DispEst(l, r, D) as de:
        m16 = de.SGBM_GPU(**F.saturating_params(bs))
        S = de.sgm_costs()[1]
        assert int(S.max()) == 524280
        flagged(psm, de, l, 0, {}, S=S, m16=m16, wls={"iterations": 1})


@pytest.mark.parametrize("conf", ({"radius": 1}, {"radius": 3}, {"radius": 4}, {"var_shift": 0}, {"var_shift": 16}, {"lr_thresh": 1},
                                  {"lr_thresh": 32767}, {"terms": CM.LR}, {"terms": CM.VAR}, {"terms": CM.VAR, "radius": 4, "var_shift": 3}))
def test_parameters_and_each_term_alone(psm, conf):
    W, H, D = 70, 13, 16
    l, r = noise_pair(W, H, 5, 77)
    with psm.DispEst(l, r, D) as de:
        de.SGBM_GPU(uniqueness_ratio=5)
        got, model = flagged(psm, de, l, 0, conf)
        valid = de.sgm_disparity() != -16
        if conf.get("terms") == CM.VAR:
            assert np.array_equal(got["conf"], CM.var_term(de.sgm_disparity(), -16, conf.get("radius", 2), conf.get("var_shift", 8)))
        if conf.get("var_shift") == 16 and valid.any():
            assert (got["conf"][valid] > 0).any()


def test_a_radius_wider_than_the_image_and_injected_maps(psm):
    """the variance term alone needs only the map: through the hook plane, on the smallest context (a 9 x 9 window over 8 x 8)"""
    W, H = 8, 8
    guide = rnd(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    var4 = {"terms": CM.VAR, "radius": 4, "var_shift": 0}
    with psm.DispEst(guide, guide, 8) as de:
        for v in (np.full((H, W), -16, np.int16), None, rnd(4).integers(0, 100, (H, W)).astype(np.int16)):
            if v is None:
                v = np.full((H, W), -16, np.int16)
                v[5, 2] = 777                                                         # one valid pixel: n = 1
            de.upload_sgm_map(v)
            got, model = flagged(psm, de, guide, 0, var4, m16=v)
            if (v == -16).all():
                assert not got["conf"].any() and (got["disp"] == -16).all() and (got["den"] == 0).all()
            elif (v != -16).sum() == 1:
                assert got["conf"][5, 2] == 255 and got["conf"].sum() == 255
        # ... and the extremes of int16 alternating: the largest window sums
        v = np.where((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0, -32768, 32767).astype(np.int16)
        de.upload_sgm_map(v)
        flagged(psm, de, guide, 0, {"terms": CM.VAR, "radius": 4, "var_shift": 16}, m16=v)
        de.upload_sgm_map(None)


def test_guides_and_iterations(psm):
    W, H, D = 65, 12, 8
    l, r = noise_pair(W, H, 2, 5)
    lf, rf = l.astype(np.float32) / np.float32(255.0) * np.float32(1.1), r.astype(np.float32) / np.float32(255.0) * np.float32(1.1)
    with psm.DispEst(lf, rf, D) as de:                                                # a float pair
        de.SGBM_GPU()
        for T in (1, 4):
            flagged(psm, de, lf, 0, {}, wls={"iterations": T})
    gl, gr = np.ascontiguousarray(l[:, :, 0]), np.ascontiguousarray(r[:, :, 0])
    with psm.DispEst(l, r, D) as de:                                                  # uint8; then the one-channel compute, whose left plane guides
        de.SGBM_GPU()
        flagged(psm, de, l, 0, {}, wls={"iterations": 1})
        m16 = de.SGBM_GPU(gray=(gl, gr))
        S = de.sgm_costs()[1]
        de.setWLS()
        de.WLS_GPU(psm.capi.PSM_WLS_SGM, confidence={})
        equal(fetch(de), CM.wls(m16, -16, gl, S=S, dmin=0))


def test_refusals(psm):
    capi = psm.capi
    lib = capi.load()
    W, H, D = 16, 8, 8
    l, r = noise_pair(W, H, 2, 9)
    CONF = capi.PSM_WLS_CONFIDENCE
    with psm.DispEst(l, r, D) as de, psm.DispEst(l, r, D) as other:
        h = de._h
        refused = lambda flags, source=capi.PSM_WLS_SGM: (lib.psm_wls_filter(h, source, flags) != 0, capi.last_error(h))
        bad, msg = refused(CONF)
        assert bad and "no SGM result" in msg                                         # nothing at all yet
        de.upload_sgm_map(np.zeros((H, W), np.int16))
        bad, msg = refused(CONF)
        assert bad and "psm_score_upload_sgm_map" in msg and "L-R term" in msg        # the hook plane: S does not belong to it
        de.setWLSConfidence(terms=CM.VAR)
        assert lib.psm_wls_filter(h, capi.PSM_WLS_SGM, CONF) == 0                     # ... the variance term alone needs only the map
        before = fetch(de, right=False)
        de.setWLSConfidence()
        de.upload_sgm_map(None)
        bad, msg = refused(CONF)
        assert bad and "no SGM result" in msg                                         # hook off, no compute
        de.upload_maps(np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8))
        bad, msg = refused(CONF, capi.PSM_WLS_GIF)
        assert bad and "PSM_WLS_CONFIDENCE" in msg and "GIF" in msg
        bad, msg = refused(4)
        assert bad and "unknown flag bits 0x4" in msg
        bad, msg = refused(CONF | 8)
        assert bad and "unknown flag bits 0x8" in msg
        for args, word in (((0, 24, 2, 8), "terms 0"), ((4, 24, 2, 8), "terms 4"), ((3, 0, 2, 8), "lr_thresh 0"), ((3, 32768, 2, 8), "lr_thresh 32768"),
                           ((3, 24, 0, 8), "radius 0"), ((3, 24, 5, 8), "radius 5"), ((3, 24, 2, -1), "var_shift -1"), ((3, 24, 2, 17), "var_shift 17")):
            assert lib.psm_wls_set_confidence(h, *args) != 0 and word in capi.last_error(h)
        equal(fetch(de, right=False), before)                                         # every refusal left the previous result downloadable
        assert lib.psm_wls_download_confidence(h, None, 0, np.empty((H, W), np.int16).ctypes.data_as(C.c_void_p), 0) != 0
        assert "without the L-R term" in capi.last_error(h)
        de.SGBM_GPU()
        de.release_scratch()
        bad, msg = refused(CONF)
        assert bad and "no SGM result" in msg                                         # released: S went with the stage's result
        # a batch names the member
        other.SGBM_GPU()
        de.upload_sgm_map(np.zeros((H, W), np.int16))
        arr = (C.c_void_p * 2)(other._h, de._h)
        assert lib.psm_wls_filter_batch(arr, 2, capi.PSM_WLS_SGM, CONF) != 0
        msg = capi.last_error(other._h)
        assert msg.startswith("psm_wls_filter_batch: context 1:") and "psm_score_upload_sgm_map" in msg
        de.upload_sgm_map(None)
        # no flag: no confidence to download
        de.SGBM_GPU()
        de.WLS_GPU(capi.PSM_WLS_SGM)
        assert lib.psm_wls_download_confidence(h, np.empty((H, W), np.uint8).ctypes.data_as(C.c_void_p), 0, None, 0) != 0
        assert "without PSM_WLS_CONFIDENCE" in capi.last_error(h)


def test_flag_off_after_flag_on_async_and_release(psm):
    capi = psm.capi
    W, H, D = 70, 20, 16
    l, r = noise_pair(W, H, 4, 31)
    guide = DM.quantise(l)
    with psm.DispEst(l, r, D) as de:
        m16 = de.SGBM_GPU(uniqueness_ratio=5)
        S = de.sgm_costs()[1]
        plain = M.wls(m16, -16, guide)

        def unflagged():
            de.WLS_GPU(capi.PSM_WLS_SGM)
            q, num, den = de.wls_planes()
            assert np.array_equal(de.wls_map(), plain["disp"])
            for k, a in (("q", q), ("num", num), ("den", den)):
                assert np.array_equal(a.view(np.uint32), plain[k].view(np.uint32)), k

        unflagged()
        got, model = flagged(psm, de, l, 0, {}, S=S, m16=m16)
        assert not np.array_equal(got["disp"], plain["disp"])                         # (the flag does change the result on this pair)
        unflagged()                                                                   # nothing leaks through the state
        de.set_option(capi.PSM_OPT_ASYNC, 1)
        de.WLS_GPU(capi.PSM_WLS_SGM, confidence={"lr_thresh": 40})
        de.wls_wait()
        equal(fetch(de), CM.wls(m16, -16, guide, S=S, lr_thresh=40))
        de.set_option(capi.PSM_OPT_ASYNC, 0)
        de.release_scratch()                                                          # the planes and S are gone, the parameters stay
        m16b = de.SGBM_GPU(uniqueness_ratio=5)
        assert np.array_equal(m16b, m16)
        de._ck(de._lib.psm_wls_filter(de._h, capi.PSM_WLS_SGM, capi.PSM_WLS_CONFIDENCE), "filter")
        equal(fetch(de), CM.wls(m16, -16, guide, S=S, lr_thresh=40))
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        de.WLS_GPU(capi.PSM_WLS_SGM, confidence={})
        assert 0.0 < de.wls_conf_time() < de.wls_time()


@pytest.mark.parametrize("n", (1, 3))
def test_batches(psm, n):
    """every member with its own pair, range-independent parameters and terms: against the model and against its own single call"""
    W, H, D = 66, 13, 16
    confs = ({"lr_thresh": 30, "radius": 3}, {"terms": CM.VAR, "var_shift": 6}, {"terms": CM.LR, "lr_thresh": 9})[:n]
    wls = ({"lam": 500.0}, {"sigma": 3.0}, {})[:n]
    pairs = [noise_pair(W, H, 3 + i, 50 + i) for i in range(n)]
    des = [psm.DispEst(l, r, D) for l, r in pairs]
    singles = [psm.DispEst(l, r, D) for l, r in pairs]
    try:
        for de, k in zip(des, wls):
            de.SGBM_GPU(uniqueness_ratio=5)
            de.setWLS(**k)
        maps = psm.wls_batch(des, psm.capi.PSM_WLS_SGM, confidence=list(confs))
        for i, (de, one) in enumerate(zip(des, singles)):
            right = bool(confs[i].get("terms", 3) & CM.LR)
            got = fetch(de, right)
            assert np.array_equal(maps[i], got["disp"])
            S = de.sgm_costs()[1] if right else None
            equal(got, CM.wls(de.sgm_disparity(), -16, DM.quantise(pairs[i][0]), S=S, dmin=0, **wls[i], **confs[i]))
            one.SGBM_GPU(uniqueness_ratio=5)
            one.setWLS(**wls[i])
            one.WLS_GPU(psm.capi.PSM_WLS_SGM, confidence=confs[i])
            equal(got, fetch(one, right))
    finally:
        for de in des + singles:
            de.close()


@pytest.mark.parametrize("name", ("cones", "teddy"))
def test_cones_and_teddy_against_the_goldens(psm, golden, name):
    p, want = golden(f"{name}_pair.npz"), golden(f"{name}_wls_conf.npz")
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        m16 = de.SGBM_GPU()
        assert np.array_equal(m16, golden(f"{name}_sgm.npz")["disp"])
        de.WLS_GPU(psm.capi.PSM_WLS_SGM, confidence={})
        got = fetch(de)
    man = json.load(open(os.path.join(GOLDEN, "manifest_wls_conf.json")))[name.capitalize()]["wls_conf"]
    for k in ("right16", "conf", "disp"):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
        assert man["sha256"][k] == hashlib.sha256(got[k].tobytes()).hexdigest()
    assert int((got["disp"] == -16).sum()) == man["void"]
