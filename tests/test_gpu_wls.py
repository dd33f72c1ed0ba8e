"""-m gpu: the WLS smoothing stage (psm_wls_filter: the Fast Global Smoother over an int16 disparity map in 16ths, guided by the left
image) against its definition, tests/wls_model.py.  Every comparison is of bit patterns - the int16 map, and the float planes and
the table as uint32 - with 0 differing: there is no tolerance anywhere in this file.  The maps are injected (psm_score_upload_sgm_map,
psm_upload_maps), so no matcher runs except where a test is about one.

Shapes.  One lane owns one line (a row in the row pass, a column in the column pass) and a wave holds 64 lines (WLS_LINES); the row
pass moves tiles of 64 steps (WLS_STEPS) through LDS, the column pass keeps the loads of 8 steps (WLS_CHUNK) in flight.  A context
is at least 8 x 8, so the shapes (W x H) are the smallest legal ones on those edges:
    8 x 8                   the smallest context: one wave with 8 live lines in both passes, one chunk, a tile an eighth full
    63 x 9, 64 x 9, 65 x 9  row pass: a tile one step short, exactly one tile, a second tile of one step (the carry between tiles);
                            column pass: one lane short of a wave, a whole wave, a second workgroup with one live lane;
                            9 rows: a second chunk of one step
    9 x 63, 9 x 64, 9 x 65  the transposes: the same edges for the lines of the row pass and the steps of the column pass
    129 x 10, 10 x 129      a third tile / wave of one, a 17th chunk of one
    70 x 130                the case whose model has subnormal and zero elements in den (asserted on the model)
    8 x 1500                lines far shorter than a tile, 24 workgroups in the row pass, 188 chunks
    450 x 375               several workgroups in both passes (6 and 8), 8 tiles with the last 2 steps wide
"""
import ctypes as C

import numpy as np
import pytest

import depth_model as DM
import score_model as SM
import wls_model as M

pytestmark = pytest.mark.gpu

SHAPES = ((8, 8), (63, 9), (64, 9), (65, 9), (9, 63), (9, 64), (9, 65), (129, 10), (10, 129), (70, 130), (8, 1500), (450, 375))


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def rnd(seed):
    return np.random.default_rng(seed)


def noise(W, H, seed=0):
    """a guide of independent bytes: most links are weak, many weights subnormal or zero"""
    return rnd(2000 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def smooth(W, H, seed=0):
    """a guide of small steps with a few edges: strong links, the smoothing reaches far"""
    r = rnd(3000 + seed)
    g = r.integers(100, 104, (H, W, 3)).astype(np.int64)
    g[:, W // 2:] += 9
    g[H // 3:, :] += 5
    return g.astype(np.uint8)


def holes(W, H, seed=0, lo=0, hi=16 * 64, inv=-16, frac=0.3):
    r = rnd(4000 + seed)
    v = r.integers(lo, hi, (H, W)).astype(np.int16)
    v[v == inv] = inv + 1
    v[r.random((H, W)) < frac] = inv
    return v


def fetch(de):
    q, num, den = de.wls_planes()
    return {"disp": de.wls_map(), "q": q, "num": num, "den": den, "tab": de.wls_table()}


def equal(got, model):
    assert got["disp"].dtype == np.int16 and np.array_equal(got["disp"], model["disp"])
    for k in ("q", "num", "den", "tab"):
        assert np.array_equal(got[k].view(np.uint32), model[k].view(np.uint32)), k


def sgm_case(psm, de, v, guide, inv=-16, **params):
    """the int16 map through the hook plane, one psm_wls_filter, against the model"""
    de.setWLS(**params)
    de.upload_sgm_map(v)
    de.WLS_GPU(psm.capi.PSM_WLS_SGM)
    got, model = fetch(de), M.wls(v, inv, DM.quantise(guide), **params)
    assert not np.isnan(model["num"]).any() and not np.isnan(model["den"]).any()      # (the working planes hold defined bits)
    equal(got, model)
    return got, model


@pytest.mark.parametrize("W,H", SHAPES)
def test_shapes(psm, W, H):
    tiny = np.float32(np.finfo(np.float32).tiny)
    for k, guide in enumerate((noise(W, H, W), smooth(W, H, H))):
        with psm.DispEst(guide, guide, 8) as de:
            got, model = sgm_case(psm, de, holes(W, H, W + k), guide)
            if (W, H) == (70, 130) and k == 0:
                den = model["den"]
                assert ((den > 0) & (den < tiny)).sum() > 20 and (den == 0).sum() > 20      # what pins that subnormals are kept
                assert (model["disp"] == -16).any() and (model["disp"] != -16).any()
            if k == 1:
                assert (model["disp"] != -16).all()                                          # every hole is filled


@pytest.mark.parametrize("params", ({"iterations": 1}, {"iterations": 2}, {"iterations": 4}, {"lam": 4.0e6, "sigma": 250.0},
                                    {"lam": 1.0e-3, "sigma": 1.0e-3}, {"lam": 0.75, "sigma": 1.0e6, "iterations": 4}, {"lam": 4.0e6, "sigma": 1.0e-3, "iterations": 2}))
def test_parameters(psm, params):
    W, H = 65, 70
    for k, guide in enumerate((noise(W, H, 5), smooth(W, H, 5))):
        with psm.DispEst(guide, guide, 8) as de:
            sgm_case(psm, de, holes(W, H, 50 + k), guide, **params)


def test_one_channel_and_float_guides_and_the_gray_compute(psm):
    capi = psm.capi
    W, H, D = 65, 12, 8
    v = holes(W, H, 7)
    leftf = rnd(21).random((H, W, 3)).astype(np.float32) * np.float32(1.2) - np.float32(0.1)       # some outside [0, 1]: saturation
    leftf[0, 0] = [0.5, 127.5 / 255.0, 0.0]
    with psm.DispEst(leftf, leftf, D) as de:
        sgm_case(psm, de, v, leftf)
    left8 = noise(W, H, 8) // 16
    gl, gr = rnd(23).integers(0, 32, (H, W), dtype=np.uint8), rnd(24).integers(0, 32, (H, W), dtype=np.uint8)
    with psm.DispEst(left8, left8, D) as de:
        m16 = de.SGBM_GPU(gray=(gl, gr))                                             # its left plane guides, as one channel
        de.WLS_GPU(capi.PSM_WLS_SGM)
        equal(fetch(de), M.wls(m16, -16, gl))
        lmap = rnd(25).integers(0, D, (H, W), dtype=np.uint8)
        de.upload_maps(lmap, lmap)
        de.WLS_GPU(capi.PSM_WLS_GIF)                                                 # the GIF source keeps the staged pair
        equal(fetch(de), M.wls(*M.gif_source(lmap), left8))
        m16 = de.SGBM_GPU()                                                          # ... and a 3-channel compute brings the SGM source back to it
        de.WLS_GPU(capi.PSM_WLS_SGM)
        equal(fetch(de), M.wls(m16, -16, left8))
    # the gray compute is the exception to "no current pair": a bare context, never given a pair
    lib = capi.load()
    h = C.c_void_p()
    assert lib.psm_create(C.byref(h), W, H, D, capi.PSM_F32, 0) == 0
    try:
        assert lib.psm_score_upload_sgm_map(h, v.ctypes.data_as(C.c_void_p), 0) == 0
        assert lib.psm_wls_filter(h, capi.PSM_WLS_SGM, 0) != 0
        assert capi.last_error(h).startswith("psm_wls_filter: no current image pair")
        assert lib.psm_sgm_compute_gray(h, gl.ctypes.data_as(C.c_void_p), gr.ctypes.data_as(C.c_void_p), W) == 0
        assert lib.psm_wls_filter(h, capi.PSM_WLS_SGM, 0) == 0                        # (the hook plane is the map, the gray plane the guide)
        disp = np.empty((H, W), np.int16)
        assert lib.psm_wls_download(h, disp.ctypes.data_as(C.c_void_p), None, None, None, 0) == 0
        assert np.array_equal(disp, M.wls(v, -16, gl)["disp"])
    finally:
        lib.psm_destroy(h)


@pytest.mark.parametrize("W,H,D", ((65, 12, 8), (450, 375, 64)))
def test_gif_source_with_and_without_the_mask(psm, W, H, D):
    capi = psm.capi
    r = rnd(17)
    lmap, rmap = r.integers(0, D, (H, W), dtype=np.uint8), r.integers(0, D, (H, W), dtype=np.uint8)
    lv, rv = (r.random((H, W)) < 0.7).astype(np.uint8) * 255, (r.random((H, W)) < 0.5).astype(np.uint8) * 255
    lv[0, :4] = [0, 1, 255, 128]                                                      # any non-zero byte is valid
    guide = smooth(W, H, 3)
    with psm.DispEst(guide, guide, D) as de:
        de.upload_maps(lmap, rmap, lv, rv)
        de.WLS_GPU(capi.PSM_WLS_GIF)
        plain = fetch(de)
        equal(plain, M.wls(*M.gif_source(lmap), guide))
        assert (plain["den"] > 0.5).all()                                             # nothing was missing
        de.WLS_GPU(capi.PSM_WLS_GIF, use_mask=True)
        masked = fetch(de)
        equal(masked, M.wls(*M.gif_source(lmap, lv), guide))
        assert not np.array_equal(masked["disp"], plain["disp"])


def test_another_min_disparity(psm):
    W, H = 65, 12
    guide = smooth(W, H, 9)
    with psm.DispEst(guide, guide, 8) as de:
        de._ck(de._lib.psm_sgm_set_range(de._h, 5, 0), "set_range")                    # invalid = (5 - 1) * 16 = 64; -16 is a disparity now
        v = holes(W, H, 9, lo=-40, hi=16 * 64, inv=64)
        v[0, :3] = [-16, 64, 65]
        got, model = sgm_case(psm, de, v, guide, inv=64, lam=2.0, sigma=0.25)
        assert (model["disp"] >= 65).sum() > 100 and got["disp"].min() >= 64           # clamped to inv + 1 from below: never mistaken for a hole
        de._ck(de._lib.psm_sgm_set_range(de._h, -3, 0), "set_range")                   # invalid = -64
        sgm_case(psm, de, holes(W, H, 10, lo=-63, hi=900, inv=-64), guide, inv=-64)


def test_wall_single_pixel_all_invalid_and_extremes(psm):
    W, H = 70, 20
    flat = np.full((H, W, 3), 90, np.uint8)
    with psm.DispEst(flat, flat, 8) as de:
        v = np.full((H, W), -16, np.int16)
        got, _ = sgm_case(psm, de, v, flat)                                           # all invalid: all inv, all void
        assert (got["disp"] == -16).all() and (got["q"].view(np.uint32) == M.VOID_BITS).all() and (got["den"] == 0).all()
        v[7, 33] = 555
        got, _ = sgm_case(psm, de, v, flat)                                           # one valid pixel on a flat guide: its value everywhere
        assert (got["disp"] == 555).all()
        for ext in (32767, -32768):
            e = holes(W, H, 3)
            e[e != -16] = ext
            got, _ = sgm_case(psm, de, e, flat)
            assert got["disp"].min() >= -16 and (got["disp"] == max(ext, -15)).any()    # the extremes stay in range
        mixed = rnd(5).choice(np.array([-32768, 32767, -16], np.int16), (H, W))
        sgm_case(psm, de, mixed, flat)
    wall = flat.copy()
    wall[:, 40:, 1] = 255
    wall[:, :40, 1] = 0                                                                # a 0 / 255 step in one channel
    with psm.DispEst(wall, wall, 8) as de:
        v = np.full((H, W), -16, np.int16)
        v[:, :40] = holes(40, H, 6)
        got, _ = sgm_case(psm, de, v, wall)
        assert (got["disp"][:, 40:] == -16).all() and (got["disp"][:, :40] != -16).all()   # inv beyond the wall


def refused(psm, de, rc, *words):
    assert rc != 0
    msg = psm.capi.last_error(de._h)
    assert msg.startswith(words[0]), msg
    for w in words:
        assert w in msg, (w, msg)


def test_refusals_on_a_live_context_leave_the_previous_result(psm, golden):
    capi = psm.capi
    lib = capi.load()
    W, H = 16, 16
    guide = smooth(W, H, 11)
    with psm.DispEst(guide, guide, 8) as de:
        h = de._h
        buf = np.empty((H, W), np.float32)
        refused(psm, de, lib.psm_wls_download(h, None, buf.ctypes.data_as(C.c_void_p), None, None, 0), "psm_wls_download:", "no psm_wls_filter ran")
        refused(psm, de, lib.psm_wls_download_table(h, buf.ctypes.data_as(C.c_void_p)), "psm_wls_download_table:", "no psm_wls_filter ran")
        refused(psm, de, lib.psm_wls_wait(h), "psm_wls_wait:", "no asynchronous")
        refused(psm, de, lib.psm_wls_publish(h, 1), "psm_wls_publish:", "no psm_wls_filter ran")
        refused(psm, de, lib.psm_wls_time(h, C.byref(C.c_double())), "psm_wls_time:", "not timed")
        refused(psm, de, lib.psm_wls_filter(h, capi.PSM_WLS_SGM, 0), "psm_wls_filter:", "no SGM result")
        refused(psm, de, lib.psm_wls_filter(h, capi.PSM_WLS_GIF, 0), "psm_wls_filter:", "no disparity maps")
        for bad in ((0.0, 1.5, 3), (-1.0, 1.5, 3), (np.nan, 1.5, 3), (np.inf, 1.5, 3)):
            refused(psm, de, lib.psm_wls_set_params(h, *bad), "psm_wls_set_params:", "lambda")
        for bad in ((8000.0, 0.0, 3), (8000.0, -2.0, 3), (8000.0, np.nan, 3), (8000.0, np.inf, 3)):
            refused(psm, de, lib.psm_wls_set_params(h, *bad), "psm_wls_set_params:", "sigma")
        for bad in (0, 5, -1):
            refused(psm, de, lib.psm_wls_set_params(h, 8000.0, 1.5, bad), "psm_wls_set_params:", "iterations", "[1, 4]")
        got, model = sgm_case(psm, de, holes(W, H, 11), guide)                        # a good result to keep (a refused setting set nothing)
        refused(psm, de, lib.psm_wls_filter(h, 2, 0), "psm_wls_filter:", "source 2")
        refused(psm, de, lib.psm_wls_filter(h, -1, 0), "psm_wls_filter:", "source -1")
        refused(psm, de, lib.psm_wls_filter(h, capi.PSM_WLS_SGM, 2), "psm_wls_filter:", "flag bits 0x2")
        refused(psm, de, lib.psm_wls_filter(h, capi.PSM_WLS_SGM, 1), "psm_wls_filter:", "PSM_WLS_USE_MASK", "SGM source")
        refused(psm, de, lib.psm_wls_filter(h, capi.PSM_WLS_GIF, 0), "psm_wls_filter:", "no disparity maps")
        lmap = np.ones((H, W), np.uint8)
        de.upload_maps(lmap, lmap)
        refused(psm, de, lib.psm_wls_filter(h, capi.PSM_WLS_GIF, 1), "psm_wls_filter:", "PSM_WLS_USE_MASK", "mask")      # no current mask
        for bad in (4 * W - 4, 4 * W + 2):
            refused(psm, de, lib.psm_wls_download(h, None, buf.ctypes.data_as(C.c_void_p), None, None, bad), "psm_wls_download: stride")
        equal(fetch(de), model)                                                       # the previous result is still there, bit for bit
    # maps that cover a row stripe only
    p = golden("cones_pair.npz")
    l, r = np.ascontiguousarray(p["l_bgr"][:16, :64]), np.ascontiguousarray(p["r_bgr"][:16, :64])
    with psm.DispEst(l, r, 16) as de:
        de.set_rows(0, 8)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        refused(psm, de, lib.psm_wls_filter(de._h, capi.PSM_WLS_GIF, 0), "psm_wls_filter:", "row stripe")
    # no current pair
    h = C.c_void_p()
    assert lib.psm_create(C.byref(h), W, H, 8, capi.PSM_F32, 0) == 0
    try:
        v = holes(W, H, 12)
        assert lib.psm_score_upload_sgm_map(h, v.ctypes.data_as(C.c_void_p), 0) == 0
        assert lib.psm_wls_filter(h, capi.PSM_WLS_SGM, 0) != 0 and capi.last_error(h).startswith("psm_wls_filter: no current image pair")
    finally:
        lib.psm_destroy(h)


def test_strided_download(psm):
    W, H = 35, 11
    guide = smooth(W, H, 13)
    with psm.DispEst(guide, guide, 8) as de:
        got, model = sgm_case(psm, de, holes(W, H, 13), guide)
        pitch = W + 5                                                                 # floats per row; the int16 rows are half as far apart
        q, num, den = (np.full((H, pitch), 7.0, np.float32) for _ in range(3))
        disp = np.full((H, 2 * pitch), 7, np.int16)
        de._ck(de._lib.psm_wls_download(de._h, *(a.ctypes.data_as(C.c_void_p) for a in (disp, q, num, den)), 4 * pitch), "download")
        for a, k in ((q, "q"), (num, "num"), (den, "den")):
            assert np.array_equal(a[:, :W].view(np.uint32), model[k].view(np.uint32)) and (a[:, W:] == 7.0).all()
        rows = disp.reshape(-1)[:H * pitch].reshape(H, pitch)                        # rows 2 pitch bytes apart
        assert np.array_equal(rows[:, :W], model["disp"]) and (rows[:, W:] == 7).all()


# ---- independence and publishing ----
def test_the_stage_writes_nothing_another_stage_reads_and_repeats_itself(psm, golden):
    capi = psm.capi
    p = golden("cones_pair.npz")
    l, r = np.ascontiguousarray(p["l_bgr"][:96, :160]), np.ascontiguousarray(p["r_bgr"][:96, :160])
    with psm.DispEst(l, r, 32) as de:
        d16 = de.SGBM_GPU()
        de.SGBMSelect_GPU()
        de.LRCheck_GPU()

        def state():
            de.download_maps()
            return [a.copy() for a in (de.sgm_disparity(), de.lDisMap, de.rDisMap, *de.download_valid())]
        before = state()
        de.WLS_GPU(capi.PSM_WLS_SGM)
        first = fetch(de)
        equal(first, M.wls(d16, -16, l))
        de.WLS_GPU(capi.PSM_WLS_GIF, use_mask=True)
        equal(fetch(de), M.wls(*M.gif_source(before[1], before[3]), l))
        de.WLS_GPU(capi.PSM_WLS_SGM)
        equal(fetch(de), first)                                                      # a second call gives equal bits
        for a, b in zip(before, state()):
            assert a.tobytes() == b.tobytes()


def hip_runtime():
    """the HIP runtime the library is bound to, as this process has it loaded"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def test_async_on_a_callers_stream(psm):
    capi = psm.capi
    W, H = 129, 70
    guide = smooth(W, H, 15)
    v = holes(W, H, 15)
    hip = hip_runtime()
    stream = C.c_void_p()
    with psm.DispEst(guide, guide, 8) as de:
        de.upload_sgm_map(v)
        assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0                   # hipStreamNonBlocking
        de.set_stream(stream.value)
        de.set_option(capi.PSM_OPT_ASYNC, 1)
        de.WLS_GPU(capi.PSM_WLS_SGM)
        de.wls_wait()
        refused(psm, de, de._lib.psm_wls_wait(de._h), "psm_wls_wait:", "no asynchronous")
        equal(fetch(de), M.wls(v, -16, guide))
        de.WLS_GPU(capi.PSM_WLS_SGM)                                                  # the downloads wait for an asynchronous run too
        equal(fetch(de), M.wls(v, -16, guide))
        de.set_option(capi.PSM_OPT_ASYNC, 0)
        de.set_stream(None)
        de.synchronize()
        assert hip.hipStreamDestroy(stream) == 0


def test_profile_time(psm):
    W, H = 65, 12
    guide = smooth(W, H, 16)
    with psm.DispEst(guide, guide, 8) as de:
        de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        sgm_case(psm, de, holes(W, H, 16), guide)
        assert 0.0 < de.wls_time() < 1000.0


def depth_equal(de, capi, d16, inv, Q, left):
    outputs = capi.PSM_DEPTH_XYZ | capi.PSM_DEPTH_Z | capi.PSM_DEPTH_CLOUD
    count = de.Reproject_GPU(capi.PSM_DEPTH_SGM, outputs)
    xyz, z = de.reprojected()
    cloud = de.cloud()
    d = np.asarray(d16, np.int16)
    model = DM.reproject(d.astype(np.float64) * 0.0625, d == inv, Q, (0, 0), (0.0, DM.FLT_MAX), left)
    assert count == len(model[2]) == len(cloud)
    assert np.array_equal(xyz.view(np.uint32), model[0].view(np.uint32)) and np.array_equal(z.view(np.uint32), model[1].view(np.uint32))
    assert cloud.tobytes() == model[2].tobytes()
    return count


def score_equal(de, capi, d16, gt, D):
    for source, name in ((capi.PSM_SCORE_SGM, SM.SGM), (capi.PSM_SCORE_SGM_INT, SM.SGM_INT)):
        rec = de.Score_GPU(source)
        want = SM.score(name, d16, gt, None, D, 4, 1, SM.MASK_NONE)              # (the parameters test_publishing sets)
        ldisp, emap = de.score_maps()
        assert np.array_equal(ldisp, want["ldisp"]) and np.array_equal(emap, want["emap"])
        for k in ("min_val", "max_val", "pixels", "bad", "err_sum", "unit", "flags"):
            assert rec[k] == want[k], k


def test_publishing(psm):
    capi = psm.capi
    W, H, D = 70, 40, 8
    Q = DM.q_from_projections([[700.0, 0, 30.0, 0], [0, 700.0, 20.0, 0], [0, 0, 1, 0]], [[700.0, 0, 30.0, -84000.0], [0, 700.0, 20.0, 0], [0, 0, 1, 0]])
    guide = noise(W, H, 17)
    right = np.roll(guide, -3, axis=1)                                                # disparity 3, holes along the left border
    v = holes(W, H, 17, hi=16 * D)
    gt = rnd(18).integers(0, 4 * D, (H, W), dtype=np.uint8)
    with psm.DispEst(guide, right, D) as de:
        de.setReprojection(Q)
        de.set_score_params(4, 1, capi.PSM_MASK_NONE)
        de.set_truth(gt)
        m16 = de.SGBM_GPU()                                                           # a compute's map under the filter
        de.setWLS(lam=40.0, sigma=60.0, iterations=2)
        de.WLS_GPU(capi.PSM_WLS_SGM)
        w16 = fetch(de)["disp"]
        assert np.array_equal(w16, M.wls(m16, -16, guide, 40.0, 60.0, 2)["disp"]) and not np.array_equal(w16, m16)
        today = depth_equal(de, capi, m16, -16, Q, guide)                             # off: the SGM stage's map
        score_equal(de, capi, m16, gt, D)
        de.wls_publish(True)
        dense = depth_equal(de, capi, w16, -16, Q, guide)                             # on: the filtered map, every output
        score_equal(de, capi, w16, gt, D)
        assert dense >= today
        de.upload_sgm_map(v)                                                          # the hook plane wins while it is on ...
        depth_equal(de, capi, v, -16, Q, guide)
        score_equal(de, capi, v, gt, D)
        de.WLS_GPU(capi.PSM_WLS_SGM)                                                  # ... and is what the filter reads
        h16 = fetch(de)["disp"]
        assert np.array_equal(h16, M.wls(v, -16, guide, 40.0, 60.0, 2)["disp"])
        depth_equal(de, capi, v, -16, Q, guide)
        de.upload_sgm_map(None)                                                       # the hook dropped: the published result, now the hook map's
        depth_equal(de, capi, h16, -16, Q, guide)
        de.WLS_GPU(capi.PSM_WLS_SGM)                                                  # published, the filter still reads the SGM stage's map
        assert np.array_equal(fetch(de)["disp"], w16)
        # a result with another invalid value travels with its own
        n16 = de.SGBM_GPU(min_disparity=2, num_disparities=6)
        de.WLS_GPU(capi.PSM_WLS_SGM)
        x16 = fetch(de)["disp"]
        assert np.array_equal(x16, M.wls(n16, 16, guide, 40.0, 60.0, 2)["disp"])
        depth_equal(de, capi, x16, 16, Q, guide)
        de.wls_publish(False)                                                         # off again: today's results
        depth_equal(de, capi, n16, 16, Q, guide)
        score_equal(de, capi, n16, gt, D)


def test_release_scratch_then_rerun(psm):
    capi = psm.capi
    W, H = 65, 12
    guide = smooth(W, H, 19)
    v = holes(W, H, 19)
    with psm.DispEst(guide, guide, 8) as de:
        first, model = sgm_case(psm, de, v, guide, lam=100.0, sigma=2.0, iterations=2)
        de.wls_publish(True)
        de.release_scratch()
        refused(psm, de, de._lib.psm_wls_download(de._h, None, None, None, None, 0), "psm_wls_download:", "no psm_wls_filter ran")   # the planes went with the scratch ...
        refused(psm, de, de._lib.psm_wls_publish(de._h, 1), "psm_wls_publish:", "no psm_wls_filter ran")                             # ... and publishing is off
        de.upload_sgm_map(v)
        de.WLS_GPU(capi.PSM_WLS_SGM)                                                  # ... the parameters did not
        equal(fetch(de), model)


@pytest.mark.parametrize("name", ("cones", "teddy"))
def test_golden_pairs_from_a_real_compute_and_through_the_harness(psm, golden, name):
    from primestereomatch_amd import harness
    capi = psm.capi
    p, want = golden(f"{name}_pair.npz"), golden(f"{name}_wls.npz")
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        d16 = de.SGBM_GPU()
        de.WLS_GPU(capi.PSM_WLS_SGM)
        got = fetch(de)
        assert np.array_equal(got["disp"], want["disp"])                               # the committed map ...
        equal(got, M.wls(d16, -16, p["l_bgr"]))                                        # ... and every plane of the model on the device's own SGM map
    out = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, gt=p["gt_l"], mask=p["occl"], wls={})
    assert np.array_equal(out["wls16"], want["disp"])
    assert out["bp_percent_wls"] == float(want["bp_percent_wls"]) < out["bp_percent_int"]
    plain = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, gt=p["gt_l"], mask=p["occl"])
    assert "wls16" not in plain and "bp_percent_wls" not in plain
