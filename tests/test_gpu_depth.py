"""-m gpu: the reprojection stage (psm_reproject: cv::reprojectImageTo3D of the current result and the compacted, coloured point
cloud on the device) against its definition, tests/depth_model.py.  Every comparison is of bit patterns - the planes as uint32,
the records as bytes - with 0 differing: there is no tolerance anywhere in this file.  The maps are injected (psm_upload_maps,
psm_score_upload_sgm_map), so no matcher runs except where a test is about one.

Shapes.  The kernels see an image as W H pixels in raster order: 256 per workgroup (a tile, DP_TILE), 64 per wave, and the scan's
single workgroup has 256 threads (DP_SCAN), each of which takes ceil(tiles / 256) consecutive tiles.  A context is at least 8 x 8
(psm_create refuses anything smaller), so 1 x 1, 63 x 2, 64 x 1, 65 x 3, 257 x 3 and 3 x 1500 cannot exist; the shapes below are
the smallest legal ones that hit the same edges:
    8 x 8       64 pixels: the smallest context - exactly one wave, three quarters of its tile idle
    15 x 17     255: the last wave one lane short (63 of 64), the tile one pixel short
    16 x 16     256: exactly one tile
    35 x 11     385: one lane past a wave edge (256 + 128 + 1)
    27 x 19     513: one pixel past a tile edge - a third tile with a single live lane
    8 x 1500    12 000: rows far shorter than a wave (a wave spans 8 rows), 47 tiles
    450 x 375   168 750: 660 tiles - more tiles than the scan workgroup has threads (256), three tiles per scan thread
"""
import ctypes as C
import os

import numpy as np
import pytest

import depth_model as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = ((8, 8), (15, 17), (16, 16), (35, 11), (27, 19), (8, 1500), (450, 375))
TILE = 256


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@pytest.fixture(scope="module")
def cal():
    from primestereomatch_amd import rectify
    return rectify.read_opencv_yaml(os.path.join(GOLDEN, "zed_extrinsics.yml"))


def rnd(seed):
    return np.random.default_rng(seed)


def image(W, H, seed=0):
    return rnd(1000 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def context(psm, W, H, D=8, left=None):
    left = image(W, H) if left is None else left
    return psm.DispEst(left, left, D), left


def all_outputs(capi):
    return capi.PSM_DEPTH_XYZ | capi.PSM_DEPTH_Z | capi.PSM_DEPTH_CLOUD


def fetch(de, count):
    xyz, z = de.reprojected()
    cloud = de.cloud() if de._depth_outputs & 4 else None
    assert cloud is None or len(cloud) == count
    return count, xyz, z, cloud


def equal(got, model):
    """(count, xyz, z, cloud) of the device against (xyz, z, cloud) of the model, whatever of it the outputs named"""
    count, xyz, z, cloud = got
    assert count == len(model[2]), (count, len(model[2]))
    if xyz is not None:
        assert np.array_equal(xyz.view(np.uint32), model[0].view(np.uint32))
    if z is not None:
        assert np.array_equal(z.view(np.uint32), model[1].view(np.uint32))
    if cloud is not None:
        assert cloud.dtype == M.POINT and cloud.tobytes() == model[2].tobytes()


def sgm_case(psm, de, d16, Q, left, crop=(0, 0), zr=(0.0, M.FLT_MAX), outputs=None, dmin=0):
    """the int16 map through the hook plane, one psm_reproject, against the model"""
    outputs = all_outputs(psm.capi) if outputs is None else outputs
    de.setReprojection(Q, crop, zr)
    de.upload_sgm_map(d16)
    got = fetch(de, de.Reproject_GPU(psm.capi.PSM_DEPTH_SGM, outputs))
    model = M.reproject(*M.sgm_disparity(d16, dmin), Q, crop, zr, left)
    equal(got, model)
    return got, model


KEPT, FAR, MISSING = 160, 16, -16        # with the fixture Q and the range (0, 1000]: z = 255.6 kept, z = 2556 dropped, invalid


def pattern_map(keep, seed):
    """an int16 map whose kept pixels are exactly `keep` (flat, raster order): the others are missing or out of range"""
    d16 = np.where(rnd(seed).random(keep.size) < 0.5, FAR, MISSING).astype(np.int16)
    d16[keep] = KEPT
    return d16


@pytest.mark.parametrize("W,H", SHAPES)
def test_shapes_and_keep_patterns(psm, cal, W, H):
    N = W * H
    tiles = (N + TILE - 1) // TILE
    assert (W, H) != (450, 375) or tiles == 660 > 256
    idx = np.arange(N)
    patterns = {
        "all": np.ones(N, bool),
        "none": np.zeros(N, bool),
        "alternating": idx % 2 == 1,
        "last pixel alone": idx == N - 1,                                  # the last live lane of the last tile
        "first pixel alone": idx == 0,
        "random": rnd(W).random(N) < 0.37,
    }
    if N >= TILE:
        patterns["last lane of the last whole tile alone"] = idx == (N // TILE) * TILE - 1
        patterns["a whole wave empty in the middle of a tile"] = ~((idx >= 64) & (idx < 128))
    if tiles >= 8:
        patterns["a run of whole empty tiles"] = ~((idx >= 2 * TILE) & (idx < (tiles - 3) * TILE))
        patterns["one pixel per tile"] = idx % TILE == (idx // TILE) % TILE
    de, left = context(psm, W, H)
    with de:
        for k, (name, keep) in enumerate(patterns.items()):
            got, model = sgm_case(psm, de, pattern_map(keep, k).reshape(H, W), cal["Q"], left, zr=(0.0, 1000.0))
            assert got[0] == int(keep.sum()), name
            if name == "none":
                assert got[0] == 0 and got[3].shape == (0,)                # count 0 and a zero-length download


# ---- arithmetic ----
def q_variants(cal):
    Q = cal["Q"]
    out = {"fixture": (Q, (0, 0), (0.0, M.FLT_MAX))}
    q = Q.copy(); q[3, 3] = 0.25
    out["Q33 != 0: disparity 0 is finite"] = (q, (0, 0), (0.0, M.FLT_MAX))
    q = Q.copy(); q[3, 2] = -q[3, 2]
    out["negative baseline sign"] = (q, (0, 0), (0.0, M.FLT_MAX))
    out["crop"] = (Q, (217, 101), (0.0, 400.0))
    out["negative crop"] = (Q, (-32768, 32767), (0.0, M.FLT_MAX))
    q = Q.copy(); q[2, 3] = 1e60
    out["float overflow"] = (q, (3, 4), (0.0, M.FLT_MAX))
    q = Q.copy(); q[2, 3] = -1e60; q[0, 3] = 1e55
    out["float overflow, both signs"] = (q, (3, 4), (-np.inf, np.inf))
    q = Q.copy(); q[2, 3] = 3e-42; q[0, 0] = 1e-44; q[1, 1] = 1e-44; q[0, 3] = -1e-43; q[1, 3] = 0.0
    out["subnormal floats"] = (q, (0, 0), (0.0, M.FLT_MAX))
    q = rnd(5).normal(size=(4, 4))
    out["a full random Q"] = (q, (-7, 9), (-0.75, 0.5))
    return out


@pytest.mark.parametrize("case", ("fixture", "Q33 != 0: disparity 0 is finite", "negative baseline sign", "crop", "negative crop",
                                  "float overflow", "float overflow, both signs", "subnormal floats", "a full random Q"))
def test_arithmetic(psm, cal, case):
    W, H = 35, 11
    Q, crop, zr = q_variants(cal)[case]
    d16 = rnd(7).integers(0, 16 * 64, (H, W)).astype(np.int16)                  # (no negative disparities: z has Q's sign)
    d16[0, :6] = [0, 0, -16, 1, 16, 17]
    de, left = context(psm, W, H)
    with de:
        got, model = sgm_case(psm, de, d16, Q, left, crop, zr)
    xyz, bits = model[0], model[0].view(np.uint32)
    void = bits[..., 2] == M.VOID_BITS
    nan = np.isnan(got[1])
    assert (got[1].view(np.uint32)[nan] == M.VOID_BITS).all()                   # no NaN but the stored pattern reaches memory
    if case == "fixture":
        assert void[0, 0] and void[0, 2] and 0 < got[0] < W * H
    if case.startswith("Q33"):
        assert not void[0, 0] and np.isfinite(xyz[0, 0]).all()
    if case == "negative baseline sign":
        assert got[0] == 0 and (xyz[..., 2][~void] < 0).all() and (~void).sum() > 300      # negative z, all dropped by the range
    if case == "float overflow":
        assert np.isposinf(xyz[..., 2][~void]).all() and got[0] == 0 and (~void).any()      # +inf in the planes, none in the cloud
    if case == "float overflow, both signs":
        assert np.isneginf(xyz[..., 2][~void]).all() and np.isinf(xyz[..., 0][~void]).any() and got[0] == 0
    if case == "subnormal floats":
        tiny = np.float32(np.finfo(np.float32).tiny)
        z = xyz[..., 2][~void]
        assert ((z > 0) & (z < tiny)).sum() > 300 and got[0] == int((~void).sum())            # kept: subnormal, yet above z_min = 0
        assert (np.abs(xyz[..., 0][~void]) < tiny).all()


def test_the_range_is_open_below_and_closed_above(psm, cal):
    W, H = 35, 11
    d16 = rnd(11).integers(16, 16 * 40, (H, W)).astype(np.int16)
    z = M.reproject(*M.sgm_disparity(d16), cal["Q"])[1]
    vals = np.unique(z)
    lo, hi = float(vals[len(vals) // 3]), float(vals[2 * len(vals) // 3])       # two stored values
    de, left = context(psm, W, H)
    with de:
        got, model = sgm_case(psm, de, d16, cal["Q"], left, zr=(lo, hi))
    assert (z == np.float32(lo)).any() and (z == np.float32(hi)).any()
    assert got[0] == int(((z > np.float32(lo)) & (z <= np.float32(hi))).sum())
    assert np.float32(hi) in got[3]["z"] and np.float32(lo) not in got[3]["z"]


def test_int16_extremes_and_the_invalid_value_of_another_range(psm, cal):
    W, H = 35, 11
    d16 = rnd(13).integers(-32768, 32768, (H, W)).astype(np.int16)
    d16[0, :8] = [-32768, 32767, -16, 64, 0, -1, 1, 80]
    Q = cal["Q"].copy()
    Q[3, 3] = 0.01
    de, left = context(psm, W, H)
    with de:
        sgm_case(psm, de, d16, Q, left, zr=(-np.inf, np.inf))
        de._ck(de._lib.psm_sgm_set_range(de._h, 5, 0), "set_range")                # invalid = (5 - 1) * 16 = 64; -16 is a disparity now
        got, model = sgm_case(psm, de, d16, Q, left, zr=(-np.inf, np.inf), dmin=5)
        assert got[1].view(np.uint32)[0, 3, 2] == M.VOID_BITS and got[1].view(np.uint32)[0, 2, 2] != M.VOID_BITS
        de._ck(de._lib.psm_sgm_set_range(de._h, -3, 0), "set_range")               # invalid = -64
        sgm_case(psm, de, np.where(d16 == 64, -64, d16).astype(np.int16), Q, left, zr=(-np.inf, np.inf), dmin=-3)


# ---- sources and flags ----
@pytest.mark.parametrize("W,H,D", ((35, 11, 8), (450, 375, 64)))
def test_gif_source_with_and_without_the_mask(psm, cal, W, H, D):
    capi = psm.capi
    r = rnd(17)
    lmap, rmap = r.integers(0, D, (H, W), dtype=np.uint8), r.integers(0, D, (H, W), dtype=np.uint8)
    lv, rv = (r.random((H, W)) < 0.7).astype(np.uint8) * 255, (r.random((H, W)) < 0.5).astype(np.uint8) * 255
    lv[0, :4] = [0, 1, 255, 128]                                                  # any non-zero byte is valid
    de, left = context(psm, W, H, D)
    zr = (0.0, 2556.0 / (D / 4.0))                                               # z = 2556 / d: the disparities from D / 4 up are kept
    with de:
        de.setReprojection(cal["Q"], (2, 3), zr)
        de.upload_maps(lmap, rmap, lv, rv)
        got = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_GIF, all_outputs(capi)))
        equal(got, M.reproject(*M.gif_disparity(lmap), cal["Q"], (2, 3), zr, left))
        masked = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_GIF, all_outputs(capi), use_mask=True))
        equal(masked, M.reproject(*M.gif_disparity(lmap, lv), cal["Q"], (2, 3), zr, left))
        assert 0 < masked[0] < got[0] < W * H


def test_sgm_source_on_cones_from_a_compute_and_from_the_hook(psm, cal, golden):
    capi = psm.capi
    p, g = golden("cones_pair.npz"), golden("cones_sgm.npz")
    zr = (0.0, 100.0)
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        de.setReprojection(cal["Q"], (0, 0), zr)
        d16 = de.SGBM_GPU()
        got = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_SGM, all_outputs(capi)))
        equal(got, M.reproject(*M.sgm_disparity(d16), cal["Q"], (0, 0), zr, p["l_bgr"]))       # the model on the device's own map
        de.upload_sgm_map(g["disp"])
        got = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_SGM, all_outputs(capi)))
        equal(got, M.reproject(*M.sgm_disparity(g["disp"]), cal["Q"], (0, 0), zr, p["l_bgr"]))
        assert got[0] == 96678
        de.upload_sgm_map(None)                                                   # the compute's map again
        assert de.Reproject_GPU(capi.PSM_DEPTH_SGM, capi.PSM_DEPTH_CLOUD) == len(M.reproject(*M.sgm_disparity(d16), cal["Q"], (0, 0), zr)[2])


def test_colours_of_uint8_float_and_one_channel_pairs(psm, cal):
    capi = psm.capi
    W, H, D = 35, 11, 8
    d16 = rnd(19).integers(16, 16 * D, (H, W)).astype(np.int16)
    lmap = rnd(19).integers(1, D, (H, W), dtype=np.uint8)
    left8 = image(W, H, 3)
    leftf = rnd(21).random((H, W, 3)).astype(np.float32) * np.float32(1.2) - np.float32(0.1)       # some outside [0, 1]: saturation
    leftf[0, 0] = [0.5, 127.5 / 255.0, 0.0]
    for left in (left8, leftf):
        with psm.DispEst(left, left, D) as de:
            de.setReprojection(cal["Q"])
            de.upload_sgm_map(d16)
            de.upload_maps(lmap, lmap)
            for source, dm in ((capi.PSM_DEPTH_SGM, M.sgm_disparity(d16)), (capi.PSM_DEPTH_GIF, M.gif_disparity(lmap))):
                got = fetch(de, de.Reproject_GPU(source, capi.PSM_DEPTH_CLOUD))
                equal(got, M.reproject(*dm, cal["Q"], left=left))
                assert got[0] == W * H and (got[3]["a"] == 255).all()
    # a one-channel pair: the result of psm_sgm_compute_gray brings its own left plane, the byte three times
    gl, gr = rnd(23).integers(0, 256, (H, W), dtype=np.uint8), rnd(24).integers(0, 256, (H, W), dtype=np.uint8)
    with psm.DispEst(left8, left8, D) as de:
        de.setReprojection(cal["Q"], z_range=(-np.inf, np.inf))
        m16 = de.SGBM_GPU(gray=(gl, gr))
        got = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_SGM, capi.PSM_DEPTH_CLOUD))
        equal(got, M.reproject(*M.sgm_disparity(m16), cal["Q"], z_range=(-np.inf, np.inf), left=gl))
        # the GIF source of the same context keeps the staged pair's colours
        de.upload_maps(lmap, lmap)
        got = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_GIF, capi.PSM_DEPTH_CLOUD))
        equal(got, M.reproject(*M.gif_disparity(lmap), cal["Q"], z_range=(-np.inf, np.inf), left=left8))
        # ... and a 3-channel compute brings the SGM source back to them
        m16 = de.SGBM_GPU()
        got = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_SGM, capi.PSM_DEPTH_CLOUD))
        equal(got, M.reproject(*M.sgm_disparity(m16), cal["Q"], z_range=(-np.inf, np.inf), left=left8))


# ---- output sets ----
@pytest.mark.parametrize("W,H", ((27, 19), (450, 375)))
def test_every_output_subset_gives_the_bits_of_the_full_set(psm, cal, W, H):
    d16 = rnd(29).integers(-16, 16 * 64, (H, W)).astype(np.int16)
    zr = (0.0, 60.0)
    model = M.reproject(*M.sgm_disparity(d16), cal["Q"], (0, 0), zr, image(W, H))
    for outputs in range(1, 8):
        de, left = context(psm, W, H)                                             # a fresh context: only what was asked for exists
        with de:
            got, _ = sgm_case(psm, de, d16, cal["Q"], left, zr=zr, outputs=outputs)
            assert (got[1] is not None) == bool(outputs & 1) and (got[2] is not None) == bool(outputs & 2) and (got[3] is not None) == bool(outputs & 4)
            assert got[0] == len(model[2])
            # what was not among the outputs is refused by name
            lib, h = de._lib, de._h
            buf = np.empty((H, W, 3), np.float32)
            if not outputs & 1:
                assert lib.psm_reproject_download(h, buf.ctypes.data_as(C.c_void_p), None, 0) != 0 and "PSM_DEPTH_XYZ" in psm.capi.last_error(h)
            if not outputs & 2:
                assert lib.psm_reproject_download(h, None, buf.ctypes.data_as(C.c_void_p), 0) != 0 and "PSM_DEPTH_Z" in psm.capi.last_error(h)
            if not outputs & 4:
                assert lib.psm_reproject_download_cloud(h, None, 0, None) != 0 and "PSM_DEPTH_CLOUD" in psm.capi.last_error(h)


def test_strided_download(psm, cal):
    W, H = 35, 11
    d16 = rnd(31).integers(-16, 16 * 64, (H, W)).astype(np.int16)
    de, left = context(psm, W, H)
    with de:
        got, model = sgm_case(psm, de, d16, cal["Q"], left)
        pitch = W + 5                                                             # floats per row of z
        z = np.full((H, pitch), 7.0, np.float32)
        xyz = np.full((H, 3 * pitch), 7.0, np.float32)
        de._ck(de._lib.psm_reproject_download(de._h, xyz.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 4 * pitch), "download")
        assert np.array_equal(z[:, :W].view(np.uint32), model[1].view(np.uint32)) and (z[:, W:] == 7.0).all()
        assert np.array_equal(xyz[:, :3 * W].view(np.uint32), model[0].reshape(H, 3 * W).view(np.uint32)) and (xyz[:, 3 * W:] == 7.0).all()
        for bad in (4 * W - 4, 4 * W + 2):
            assert de._lib.psm_reproject_download(de._h, None, z.ctypes.data_as(C.c_void_p), bad) != 0
            assert psm.capi.last_error(de._h).startswith("psm_reproject_download: stride")


# ---- state ----
def test_the_stage_writes_nothing_another_stage_reads(psm, cal, golden):
    capi = psm.capi
    p = golden("cones_pair.npz")
    l, r = p["l_bgr"][:64, :96], p["r_bgr"][:64, :96]
    with psm.DispEst(np.ascontiguousarray(l), np.ascontiguousarray(r), 16) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU(); de.LRCheck_GPU()
        de.SGBM_GPU()
        de.set_truth(np.ascontiguousarray(p["gt_l"][:64, :96]))
        de.Score_GPU(capi.PSM_SCORE_GIF)

        def snapshot():
            maps = [m.copy() for m in de.download_maps()]
            valid = [m.copy() for m in de.download_valid()]
            return maps + valid + [de.sgm_disparity()] + list(de.sgm_costs()) + list(de.score_maps(right=True)) + list(de.download_images())

        before = snapshot()
        de.setReprojection(cal["Q"], (5, 6), (0.0, 500.0))
        for source, mask in ((capi.PSM_DEPTH_GIF, True), (capi.PSM_DEPTH_GIF, False), (capi.PSM_DEPTH_SGM, False)):
            n = de.Reproject_GPU(source, all_outputs(capi), use_mask=mask)
            assert 0 < n < 64 * 96
        after = snapshot()
        assert len(before) == len(after) == 12
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
        # ... and the mask the GIF source used is the one the L-R check made
        got = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_GIF, all_outputs(capi), use_mask=True))
        equal(got, M.reproject(*M.gif_disparity(before[0], before[2]), cal["Q"], (5, 6), (0.0, 500.0), np.ascontiguousarray(l)))


def test_release_scratch_then_rerun(psm, cal):
    capi = psm.capi
    W, H = 27, 19
    d16 = rnd(37).integers(-16, 16 * 64, (H, W)).astype(np.int16)
    de, left = context(psm, W, H)
    with de:
        first, model = sgm_case(psm, de, d16, cal["Q"], left, (1, 2), (0.0, 80.0))
        de.release_scratch()
        assert de._lib.psm_reproject_download_cloud(de._h, None, 0, None) != 0
        assert "no psm_reproject ran" in capi.last_error(de._h)                    # the planes went with the scratch ...
        de.upload_sgm_map(d16)                                                    # (the hook plane stays; the parameters too)
        again = fetch(de, de.Reproject_GPU(capi.PSM_DEPTH_SGM, all_outputs(capi)))
        equal(again, model)                                                       # ... Q, crop and range did not
        assert again[3].tobytes() == first[3].tobytes()


def refused(psm, de, rc, *words):
    assert rc != 0
    msg = psm.capi.last_error(de._h)
    for w in words:
        assert w in msg, (w, msg)


def test_refusals_on_a_live_context_leave_the_previous_result(psm, cal):
    capi = psm.capi
    W, H = 16, 16
    lib = capi.load()
    n = C.c_uint32()
    ALL = all_outputs(capi)
    de, left = context(psm, W, H)
    with de:
        h = de._h
        refused(psm, de, lib.psm_reproject_download(h, None, None, 0), "psm_reproject_download:", "no psm_reproject ran")      # a download before any run
        refused(psm, de, lib.psm_reproject_download_cloud(h, None, 0, None), "psm_reproject_download_cloud:", "no psm_reproject ran")
        refused(psm, de, lib.psm_reproject_wait(h, C.byref(n)), "psm_reproject_wait:", "no asynchronous")
        de.upload_sgm_map(np.full((H, W), KEPT, np.int16))
        refused(psm, de, lib.psm_reproject(h, 1, ALL, 0, C.byref(n)), "psm_reproject:", "no Q set")
        q = cal["Q"].reshape(-1).copy()
        q[5] = np.nan
        refused(psm, de, lib.psm_reproject_set_q(h, (C.c_double * 16)(*q), 0, 0), "psm_reproject_set_q:", "Q[1][1]", "finite")
        refused(psm, de, lib.psm_reproject_set_q(h, (C.c_double * 16)(*cal["Q"].reshape(-1)), 40000, 0), "psm_reproject_set_q:", "[-32768, 32767]")
        refused(psm, de, lib.psm_reproject(h, 1, ALL, 0, C.byref(n)), "no Q set")                  # a refused Q sets nothing
        # a good result to keep
        got, model = sgm_case(psm, de, rnd(41).integers(-16, 16 * 64, (H, W)).astype(np.int16), cal["Q"], left, (1, 1), (0.0, 90.0))
        for zr in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (1.0, np.nan)):
            refused(psm, de, lib.psm_reproject_set_range(h, *zr), "psm_reproject_set_range:", "z_min")
        refused(psm, de, lib.psm_reproject(h, 2, ALL, 0, C.byref(n)), "psm_reproject:", "source 2")
        refused(psm, de, lib.psm_reproject(h, 1, 0, 0, C.byref(n)), "psm_reproject:", "outputs == 0")
        refused(psm, de, lib.psm_reproject(h, 1, 8 | 1, 0, C.byref(n)), "psm_reproject:", "output bits 0x8")
        refused(psm, de, lib.psm_reproject(h, 1, ALL, 4, C.byref(n)), "psm_reproject:", "flag bits 0x4")
        refused(psm, de, lib.psm_reproject(h, 1, ALL, 1, C.byref(n)), "psm_reproject:", "PSM_DEPTH_USE_MASK", "SGM source")
        refused(psm, de, lib.psm_reproject(h, 0, ALL, 0, C.byref(n)), "psm_reproject:", "no disparity maps")       # a GIF source without current maps
        refused(psm, de, lib.psm_reproject(h, 1, ALL, 0, None), "psm_reproject:", "NULL count")
        lmap = np.ones((H, W), np.uint8)
        de.upload_maps(lmap, lmap)
        refused(psm, de, lib.psm_reproject(h, 0, ALL, 1, C.byref(n)), "psm_reproject:", "PSM_DEPTH_USE_MASK", "mask")      # no current mask
        rec = np.empty(W * H, capi.point_dtype())
        refused(psm, de, lib.psm_reproject_download_cloud(h, rec.ctypes.data_as(C.c_void_p), got[0] - 1, C.byref(n)),
                "psm_reproject_download_cloud:", "max_records", str(got[0]))
        # the previous result is still there, bit for bit
        equal(fetch(de, got[0]), model)
    # an SGM source with neither a compute nor the hook plane; maps that cover a row stripe only
    p = np.load(os.path.join(GOLDEN, "cones_pair.npz"))
    l, r = np.ascontiguousarray(p["l_bgr"][:16, :64]), np.ascontiguousarray(p["r_bgr"][:16, :64])
    with psm.DispEst(l, r, 16) as de:
        de.setReprojection(cal["Q"])
        refused(psm, de, lib.psm_reproject(de._h, 1, ALL, 0, C.byref(n)), "psm_reproject:", "no SGM result")
        de.set_rows(0, 8)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        refused(psm, de, lib.psm_reproject(de._h, 0, ALL, 0, C.byref(n)), "psm_reproject:", "row stripe")


def test_the_cloud_needs_a_pair_only_when_asked_for(psm, cal):
    """A context made through the C ABI alone has no pair until one is uploaded: the dense planes need none."""
    capi = psm.capi
    lib = capi.load()
    W, H = 16, 16
    h = C.c_void_p()
    assert lib.psm_create(C.byref(h), W, H, 8, capi.PSM_F32, 0) == 0
    try:
        n = C.c_uint32()
        d16 = np.full((H, W), KEPT, np.int16)
        assert lib.psm_score_upload_sgm_map(h, d16.ctypes.data_as(C.c_void_p), 0) == 0
        assert lib.psm_reproject_set_q(h, (C.c_double * 16)(*cal["Q"].reshape(-1)), 0, 0) == 0
        assert lib.psm_reproject(h, 1, capi.PSM_DEPTH_CLOUD, 0, C.byref(n)) != 0
        msg = capi.last_error(h)
        assert msg.startswith("psm_reproject:") and "PSM_DEPTH_CLOUD" in msg and "pair" in msg
        assert lib.psm_reproject(h, 1, capi.PSM_DEPTH_XYZ | capi.PSM_DEPTH_Z, 0, C.byref(n)) == 0 and n.value == W * H
        z = np.empty((H, W), np.float32)
        assert lib.psm_reproject_download(h, None, z.ctypes.data_as(C.c_void_p), 0) == 0
        assert np.array_equal(z.view(np.uint32), M.reproject(*M.sgm_disparity(d16), cal["Q"])[1].view(np.uint32))
    finally:
        lib.psm_destroy(h)


# ---- async and the ring ----
def test_async_with_wait(psm, cal):
    capi = psm.capi
    W, H = 35, 11
    d16 = rnd(43).integers(-16, 16 * 64, (H, W)).astype(np.int16)
    de, left = context(psm, W, H)
    with de:
        de.set_option(capi.PSM_OPT_ASYNC, 1)
        de.setReprojection(cal["Q"], (0, 0), (0.0, 70.0))
        de.upload_sgm_map(d16)
        assert de.Reproject_GPU(capi.PSM_DEPTH_SGM, all_outputs(capi)) is None
        count = de.reproject_wait()
        model = M.reproject(*M.sgm_disparity(d16), cal["Q"], (0, 0), (0.0, 70.0), left)
        equal(fetch(de, count), model)
        assert de._lib.psm_reproject_wait(de._h, C.byref(C.c_uint32())) != 0 and "no asynchronous" in capi.last_error(de._h)      # one count in flight
        # a download without the wait synchronises with the count's copy itself
        assert de.Reproject_GPU(capi.PSM_DEPTH_SGM, capi.PSM_DEPTH_CLOUD) is None
        assert de.cloud().tobytes() == model[2].tobytes()


def test_frame_ring_returns_each_frame_its_own_cloud(psm, cal):
    capi = psm.capi
    from primestereomatch_amd import synth
    W, H, D = 96, 64, 16
    frames = [synth.make_pair(W, H, D, seed=s)[:2] for s in range(4)]
    zr = (0.0, 2000.0)
    for outputs in (capi.PSM_DEPTH_CLOUD, all_outputs(capi)):
        with psm.FrameRing(frames[0][0], frames[0][1], D, frames=2, reproject=outputs) as ring:
            ring.setReprojection(cal["Q"], (4, 2), zr)
            got = []
            for l, r in frames:
                out = ring.push_async(l, r)                                       # the pair travels on the copy stream
                if out is not None:
                    got.append(out)
            got += ring.flush()
            assert len(got) == 4
            clouds = []
            for (l, r), out in zip(frames, got):
                assert len(out) == 3
                lmap, extra = out[0], out[2]
                model = M.reproject(*M.gif_disparity(lmap), cal["Q"], (4, 2), zr, l)
                if outputs == capi.PSM_DEPTH_CLOUD:
                    assert extra.tobytes() == model[2].tobytes()
                    clouds.append(extra.tobytes())
                else:
                    equal((len(extra["cloud"]), extra["xyz"], extra["z"], extra["cloud"]), model)
            assert outputs != capi.PSM_DEPTH_CLOUD or len(set(clouds)) == 4           # four distinct frames, four distinct clouds
    with psm.FrameRing(frames[0][0], frames[0][1], D, frames=2) as ring:          # without the argument everything is as before
        ring.push(*frames[0])
        assert all(len(out) == 2 for out in ring.flush())


# ---- batch ----
@pytest.mark.parametrize("n", (1, 2, 5))
def test_batch_gives_the_single_calls_bits(psm, cal, n):
    capi = psm.capi
    from primestereomatch_amd import dispest
    W, H, D = 27, 19, 8
    des, want = [], []
    try:
        for i in range(n):
            r = rnd(50 + i)
            left = image(W, H, i) if i % 2 == 0 else r.random((H, W, 3)).astype(np.float32)
            de = psm.DispEst(left, left, D)
            des.append(de)
            Q = cal["Q"].copy()
            Q[3, 3] = 0.01 * i
            Q[2, 3] *= 1.0 + 0.25 * i
            crop, zr = (3 * i, 7 - i), (0.0, 150.0 + 40.0 * i)
            d16 = r.integers(-16, 16 * 64, (H, W)).astype(np.int16)
            lmap = r.integers(0, D, (H, W), dtype=np.uint8)
            lv = (r.random((H, W)) < 0.6).astype(np.uint8) * 255
            de.setReprojection(Q, crop, zr)
            de.upload_sgm_map(d16)
            de.upload_maps(lmap, lmap, lv, lv)
            want.append({(capi.PSM_DEPTH_SGM, False): M.reproject(*M.sgm_disparity(d16), Q, crop, zr, left),
                         (capi.PSM_DEPTH_GIF, False): M.reproject(*M.gif_disparity(lmap), Q, crop, zr, left),
                         (capi.PSM_DEPTH_GIF, True): M.reproject(*M.gif_disparity(lmap, lv), Q, crop, zr, left)})
        for (source, mask) in want[0]:
            for outputs in (all_outputs(capi), capi.PSM_DEPTH_CLOUD, capi.PSM_DEPTH_Z):
                counts = dispest.reproject_batch(des, source, outputs, use_mask=mask)
                singles = []
                for de, w, count in zip(des, want, counts):
                    got = fetch(de, count)
                    equal(got, w[(source, mask)])
                    singles.append(got)
                # ... and the single calls give the same bits (every context is where its own call would have left it)
                for de, got in zip(des, singles):
                    again = fetch(de, de.Reproject_GPU(source, outputs, use_mask=mask))
                    for a, b in zip(got[1:], again[1:]):
                        assert (a is None and b is None) or a.tobytes() == b.tobytes()
                    assert got[0] == again[0]
        assert len({len(w[(capi.PSM_DEPTH_SGM, False)][2]) for w in want}) == n      # different maps, different counts
    finally:
        for de in des:
            de.close()


def test_batch_refuses_a_mismatched_member_by_name(psm, cal):
    capi = psm.capi
    lib = capi.load()
    a, _ = context(psm, 27, 19)
    b, _ = context(psm, 27, 19)
    c, _ = context(psm, 19, 27)
    with a, b, c:
        d16 = np.full((19, 27), KEPT, np.int16)
        for de in (a, b):
            de.setReprojection(cal["Q"])
            de.upload_sgm_map(d16)
        c.setReprojection(cal["Q"])
        c.upload_sgm_map(d16.reshape(27, 19))
        counts = (C.c_uint32 * 3)()

        def call(des, source=1, outputs=4, flags=0):
            arr = (C.c_void_p * len(des))(*[d._h for d in des])
            return lib.psm_reproject_batch(arr, len(des), source, outputs, flags, counts)

        assert call([a, b]) == 0 and list(counts)[:2] == [27 * 19] * 2
        keep = a.cloud().tobytes()
        assert call([a, b, c]) != 0
        msg = capi.last_error(a._h)
        assert msg.startswith("psm_reproject_batch:") and "context 2" in msg and "width" in msg
        assert call([a, a]) != 0 and "context 1 appears twice" in capi.last_error(a._h)
        b.upload_sgm_map(None)                                                    # member 1 loses its SGM source
        assert call([a, b]) != 0
        msg = capi.last_error(a._h)
        assert msg.startswith("psm_reproject_batch: context 1:") and "no SGM result" in msg
        assert call([a, b], outputs=0) != 0 and "outputs == 0" in capi.last_error(a._h)
        assert a.cloud().tobytes() == keep                                        # nothing was enqueued: the previous result stands


# ---- the upper layers ----
def test_harness_returns_planes_and_cloud(psm, cal, golden):
    from primestereomatch_amd import harness
    p, g = golden("cones_pair.npz"), golden("cones_sgm.npz")
    l, r = np.ascontiguousarray(p["l_bgr"][:96, :128]), np.ascontiguousarray(p["r_bgr"][:96, :128])
    opt = {"Q": cal["Q"], "crop": (10, 20), "z_range": (0.0, 400.0), "use_mask": True}
    out = harness.compute(l, r, 32, depth=opt)
    lf = l.astype(np.float32) * np.float32(1 / 255.0)                              # what compute() hands the device in float mode
    model = M.reproject(*M.gif_disparity(out["lDisMap"], out["lValid"]), cal["Q"], (10, 20), (0.0, 400.0), lf)
    equal((len(out["cloud"]), out["xyz"], out["z"], out["cloud"]), model)
    assert 0 < len(out["cloud"]) < l.shape[0] * l.shape[1]
    assert "cloud" not in harness.compute(l, r, 32)                               # the default is unchanged
    out = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, depth={"Q": cal["Q"], "z_range": (0.0, 100.0)})
    assert np.array_equal(out["disp16"], g["disp"]) and len(out["cloud"]) == 96678
    equal((96678, out["xyz"], out["z"], out["cloud"]), M.reproject(*M.sgm_disparity(g["disp"]), cal["Q"], (0, 0), (0.0, 100.0), p["l_bgr"]))


def test_cpp_demo_writes_the_cloud_as_ply(psm, cal, golden, tmp_path):
    """psm_demo's --ply option: DispEst::Reproject of the C++ mirror on a crop of Cones, against the model on the demo's own map
    and mask"""
    import subprocess
    from conftest import ROOT
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    if not os.path.exists(demo):
        subprocess.run(["make", "-C", os.path.join(ROOT, "primestereomatch_amd", "host")], check=True)
    p = golden("cones_pair.npz")
    l, r = np.ascontiguousarray(p["l_bgr"][:96, :128]), np.ascontiguousarray(p["r_bgr"][:96, :128])
    H, W, _ = l.shape
    l.tofile(tmp_path / "l.raw")
    r.tofile(tmp_path / "r.raw")
    env = dict(os.environ, PRIMESM_HIP_LIB=psm.capi.LIB_PATH)
    qtext = ",".join(repr(float(v)) for v in cal["Q"].reshape(-1))
    q = subprocess.run([demo, str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(W), str(H), "32", str(tmp_path / "o"), "--ply",
                        str(tmp_path / "c.ply"), "--q", qtext], env=env, capture_output=True, text=True, timeout=120)
    assert q.returncode == 0, q.stderr
    lmap = np.fromfile(tmp_path / "o_ldisp.raw", np.uint8).reshape(H, W)
    lvalid = np.fromfile(tmp_path / "o_lvalid.raw", np.uint8).reshape(H, W)
    model = M.reproject(*M.gif_disparity(lmap, lvalid), cal["Q"], left=l)[2]
    assert f"Point cloud:\t {len(model)} of {W * H} pixels kept" in q.stdout and 0 < len(model) < W * H
    head, body = (tmp_path / "c.ply").read_bytes().split(b"end_header\n")
    assert b"format binary_little_endian 1.0" in head and f"element vertex {len(model)}\n".encode() in head
    v = np.frombuffer(body, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    assert np.array_equal(v["p"].view(np.uint32), np.stack([model["x"], model["y"], model["z"]], -1).view(np.uint32))
    assert np.array_equal(v["c"], np.stack([model["r"], model["g"], model["b"]], -1))
