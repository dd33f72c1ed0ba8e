"""-m gpu: video mode - the camera frame is rectified (cv::remap, INTER_LINEAR, CV_16SC2 maps, constant border 0) and cropped on
the device (k_rectify) straight into the staged image slot.  The staged pair must equal the independent numpy statement
(rectify_model.remap_u8) with 0 differing bytes; everything downstream must see an ordinary 8-bit pair: the maps of a rectified
frame are those of a second context given the model's pair through psm_upload_pair, and the oracle's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rectify_model as RM
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

MAP_W, MAP_H = 1280, 720
CLEAN_CROP = (160, 104, 960, 512)


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@pytest.fixture(scope="module")
def zed():
    """The maps of the reference's ZED calibration at 1280 x 720, from the MODEL (the library's builder is pinned to it bit for
    bit by tests/test_rectify_model.py)."""
    cal = RM.parse_opencv_yaml(os.path.join(GOLDEN, "zed_intrinsics.yml"))
    cal.update(RM.parse_opencv_yaml(os.path.join(GOLDEN, "zed_extrinsics.yml")))
    l = RM.build_maps(cal["M1"], cal["D1"], cal["R1"], cal["P1"], MAP_W, MAP_H)
    r = RM.build_maps(cal["M2"], cal["D2"], cal["R2"], cal["P2"], MAP_W, MAP_H)
    return (l[0], r[0]), (l[1], r[1])


_frames = {}


def eyes(seed, w=MAP_W, h=MAP_H):
    """An unrectified pair of eye images from a seed (synth.make_pair: textured, with flat rectangles)."""
    from primestereomatch_amd import synth
    if (seed, w, h) not in _frames:
        _frames[(seed, w, h)] = synth.make_pair(w, h, 64, seed=seed)[:2]
    return _frames[(seed, w, h)]


def rect_of(zed, crop, src_w=MAP_W, src_h=MAP_H):
    from primestereomatch_amd.rectify import Rectification
    return Rectification(zed[0], zed[1], src_w, src_h, crop)


def model_pair(l, r, rect):
    return (RM.remap_u8(l, rect.map_xy[0], rect.map_frac[0], rect.crop), RM.remap_u8(r, rect.map_xy[1], rect.map_frac[1], rect.crop))


def blank_de(psm, rect, D=16, **kw):
    z = np.zeros((rect.crop[3], rect.crop[2], 3), np.uint8)
    return psm.DispEst(z, z, D, **kw)


def upload_eyes(de, l, r, stride=None, asynchronous=False):
    fn = de._lib.psm_upload_pair_rectified_async if asynchronous else de._lib.psm_upload_pair_rectified
    return fn(de._h, l.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), 3, l.strides[0] if stride is None else stride)


def assert_same_bytes(got, exp, what):
    n = int(np.count_nonzero(got != exp))
    print(f"{what}: {n} differing bytes of {exp.size}")
    assert got.shape == exp.shape and n == 0, what


# ---- 5. the staged pair == the model, 0 differing bytes ----
@pytest.mark.parametrize("name,crop", [("clean", CLEAN_CROP), ("full", (0, 0, MAP_W, MAP_H)), ("odd", (333, 171, 450, 375)),
                                       ("corner", (1280 - 131, 720 - 77, 131, 77))])
def test_rectified_pair_equals_model(psm, zed, name, crop):
    """clean: every tap inside; full: the border and the left camera's saturated zones; odd: 450 x 375 at odd offsets (rows of
    1350 bytes: the output's dword stores cross row ends); corner: a small window in the saturated corner."""
    rect = rect_of(zed, crop)
    l, r = eyes(1)
    with blank_de(psm, rect) as de:
        de.setRectification(rect)
        assert upload_eyes(de, l, r) == 0, psm.capi.last_error(de._h)
        gl, gr = de.download_images()
    el, er = model_pair(l, r, rect)
    assert_same_bytes(gl, el, f"{name} left")
    assert_same_bytes(gr, er, f"{name} right")
    if name == "full":
        mx, my = zed[0][0][..., 0].astype(np.int64), zed[0][0][..., 1].astype(np.int64)
        gone = (mx + 1 < 0) | (mx >= MAP_W) | (my + 1 < 0) | (my >= MAP_H)      # no tap inside the source: black
        assert gone.any() and not el[gone].any() and el[360, 640].any()


def test_side_by_side_frame_two_pointers_one_pitch(psm, zed):
    """A 2560 x 720 camera frame: l = frame, r = frame + 3 * src_w, the frame's pitch - no copy of the halves."""
    rect = rect_of(zed, CLEAN_CROP)
    l, r = eyes(2)
    frame = np.ascontiguousarray(np.concatenate([l, r], axis=1))
    assert frame.shape == (720, 2560, 3)
    with blank_de(psm, rect) as de:
        de.setRectification(rect)
        de.setInputFrame(frame)
        gl, gr = de.download_images()
        # ... and rows with padding behind them (a pitch that is no multiple of 4)
        padded = np.zeros((720, 2560 * 3 + 7), np.uint8)
        padded[:, :2560 * 3] = frame.reshape(720, -1)
        lp = padded[:, :1280 * 3]
        rp = padded[:, 1280 * 3:2560 * 3]
        rc = de._lib.psm_upload_pair_rectified(de._h, C.c_void_p(lp.ctypes.data), C.c_void_p(rp.ctypes.data), 3, padded.strides[0])
        assert rc == 0, psm.capi.last_error(de._h)
        pl, pr = de.download_images()
    el, er = model_pair(l, r, rect)
    assert_same_bytes(gl, el, "side-by-side left")
    assert_same_bytes(gr, er, "side-by-side right")
    assert_same_bytes(pl, el, "padded pitch left")
    assert_same_bytes(pr, er, "padded pitch right")


def test_source_smaller_than_maps(psm, zed):
    """Eye images of 1000 x 600 under the 1280 x 720 maps: every tap beyond the source reads 0."""
    rect = rect_of(zed, (0, 0, MAP_W, MAP_H), src_w=1000, src_h=600)
    l, r = eyes(3, 1000, 600)
    with blank_de(psm, rect) as de:
        de.setRectification(rect)
        assert upload_eyes(de, l, r) == 0, psm.capi.last_error(de._h)
        gl, gr = de.download_images()
    el, er = model_pair(l, r, rect)
    assert_same_bytes(gl, el, "small source left")
    assert_same_bytes(gr, er, "small source right")
    assert el[50:550, 1100:].max() == 0 and el.any()


@pytest.mark.parametrize("seed,sw,sh,mw,mh,crop", [(0, 37, 29, 61, 47, (3, 2, 53, 41)), (1, 2, 1, 40, 40, (0, 0, 40, 40)),
                                                   (2, 64, 64, 257, 19, (0, 0, 257, 19))])
def test_random_maps(psm, seed, sw, sh, mw, mh, crop):
    """Arbitrary (non-smooth) maps: coordinates in [-3, src + 2], every fraction - correctness does not depend on locality."""
    from primestereomatch_amd.rectify import Rectification
    rng = np.random.default_rng(100 + seed)
    mxy = [np.stack([rng.integers(-3, sw + 3, size=(mh, mw)), rng.integers(-3, sh + 3, size=(mh, mw))], -1).astype(np.int16) for _ in range(2)]
    mfr = [rng.integers(0, 1024, size=(mh, mw)).astype(np.uint16) for _ in range(2)]
    l = rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8)
    r = rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8)
    rect = Rectification(tuple(mxy), tuple(mfr), sw, sh, crop)
    with blank_de(psm, rect, D=8) as de:
        de.setRectification(rect)
        assert upload_eyes(de, l, r) == 0, psm.capi.last_error(de._h)
        gl, gr = de.download_images()
    el, er = model_pair(l, r, rect)
    assert_same_bytes(gl, el, "random left")
    assert_same_bytes(gr, er, "random right")


# ---- 6. downstream: an ordinary 8-bit pair ----
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_maps_of_rectified_frame_equal_uploaded_pair_and_oracle(psm, oracle, zed, dtype):
    rect = rect_of(zed, CLEAN_CROP)
    l, r = eyes(4)
    frame = np.concatenate([l, r], axis=1)
    el, er = model_pair(l, r, rect)
    with blank_de(psm, rect, D=64, dtype=dtype) as de, psm.DispEst(el, er, 64, dtype=dtype) as plain:
        de.setRectification(rect)
        de.setInputFrame(frame)
        for d in (de, plain):
            d.CostConst_GPU()
            d.CostFilter_GPU()
            d.DispSelect_GPU()
            d.LRCheck_GPU()
        for a, b in ((de.lDisMap, plain.lDisMap), (de.rDisMap, plain.rDisMap), (de.lValid, plain.lValid), (de.rValid, plain.rValid)):
            assert np.array_equal(a, b)
        ref = (oracle.pipeline_u8 if dtype == "u8" else oracle.pipeline_f32)(el, er, 64, threads=8)
        assert np.array_equal(de.lDisMap, ref["ldisp"]) and np.array_equal(de.rDisMap, ref["rdisp"])
        lv, rv = oracle.lr_check(ref["ldisp"], ref["rdisp"])
        assert np.array_equal(de.lValid, lv) and np.array_equal(de.rValid, rv)


def test_harness_compute_video(psm, zed):
    from primestereomatch_amd import harness
    rect = rect_of(zed, (400, 200, 320, 200))
    l, r = eyes(4)
    el, er = model_pair(l, r, rect)
    out = harness.compute_video(np.concatenate([l, r], axis=1), rect, maxDis=32, dtype="u8")
    assert np.array_equal(out["lFrame"], el) and np.array_equal(out["rFrame"], er)
    ref = harness.compute(el, er, maxDis=32, dtype="u8")
    for k in ("lDisMap", "rDisMap", "lValid", "rValid", "lDispMap"):
        assert np.array_equal(out[k], ref[k]), k


# ---- 7. frame loop, ring, batch ----
LOOP_CROP = (400, 200, 320, 200)


def blocking_maps(psm, rect, frames, D, dtype):
    out = []
    with blank_de(psm, rect, D=D, dtype=dtype) as de:
        de.setRectification(rect)
        for f in frames:
            de.setInputFrame(f)
            de.CostConst_GPU()
            de.CostFilter_GPU()
            de.DispSelect_GPU()
            out.append((de.lDisMap.copy(), de.rDisMap.copy()))
    return out


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_frame_loop_async_equals_blocking(psm, zed, dtype):
    """construct(i); upload(i + 1); filter(i); select(i) with 5 distinct frames; every frame's maps and staged images equal
    its blocking run's."""
    rect = rect_of(zed, LOOP_CROP)
    frames = [np.concatenate(eyes(s), axis=1) for s in (1, 2, 3, 4, 1)]
    frames[4] = frames[4][::-1].copy()                       # a fifth, different frame
    want = blocking_maps(psm, rect, frames, 32, dtype)
    assert not np.array_equal(want[0][0], want[1][0])
    with blank_de(psm, rect, D=32, dtype=dtype) as de:
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        de.setRectification(rect)
        de.setInputFrame_async(frames[0])
        for i in range(len(frames)):
            de.CostConst_GPU()
            if i + 1 < len(frames):
                de.setInputFrame_async(frames[i + 1])
            de.CostFilter_GPU()
            de.DispSelect_device()
            lm, rm = de.download_maps()
            assert np.array_equal(lm, want[i][0]) and np.array_equal(rm, want[i][1]), i
            gl, gr = de.download_images()
            el, er = model_pair(frames[i][:, :MAP_W], frames[i][:, MAP_W:], rect)
            assert np.array_equal(gl, el) and np.array_equal(gr, er), i


@pytest.mark.parametrize("pad", [0, 5], ids=["contiguous", "padded"])
def test_mixed_async_frame_loop(psm, pad):
    """One context, frames staged in turn by setInputImages_async and setInputFrame_async (the two forms share the staging slots and
    their events), at the random-map geometry: 53 x 41 pairs, 37 x 29 eyes - rows of 159 and 111 bytes, no multiple of 4, so with
    `pad` bytes behind every row both forms pack row by row.  Strict alternation gives each form one slot of its page-locked
    buffer only; the pair staged and then superseded by a blocking setInputImages in the middle shifts the parity, so both slots of
    both buffers are filled twice.  Every frame's staged bytes equal the CPU model's and its maps those of the same pair uploaded the
    blocking way."""
    from primestereomatch_amd.rectify import Rectification
    sw, sh, mw, mh, crop, D = 37, 29, 61, 47, (3, 2, 53, 41), 8
    W, H = crop[2], crop[3]
    rng = np.random.default_rng(77)
    mxy = [np.stack([rng.integers(-3, sw + 3, size=(mh, mw)), rng.integers(-3, sh + 3, size=(mh, mw))], -1).astype(np.int16) for _ in range(2)]
    mfr = [rng.integers(0, 1024, size=(mh, mw)).astype(np.uint16) for _ in range(2)]
    rect = Rectification(tuple(mxy), tuple(mfr), sw, sh, crop)
    vp = C.c_void_p

    def padded(a):                                   # the same rows, `pad` bytes apart from the next
        buf = np.zeros((a.shape[0], a.shape[1] * 3 + pad), np.uint8)
        buf[:, :a.shape[1] * 3] = a.reshape(a.shape[0], -1)
        return buf

    def stage(de, kind, l, r):
        lp, rp = padded(l), padded(r)
        if kind == "pair":
            rc = de._lib.psm_upload_pair_async(de._h, vp(lp.ctypes.data), vp(rp.ctypes.data), 3, lp.strides[0], psm.capi.PSM_IMG_U8)
        else:
            rc = de._lib.psm_upload_pair_rectified_async(de._h, vp(lp.ctypes.data), vp(rp.ctypes.data), 3, lp.strides[0])
        assert rc == 0, psm.capi.last_error(de._h)

    kinds = ["pair", "eyes", "pair", "eyes", "blocking", "pair", "eyes", "pair", "eyes"]
    src = [tuple(rng.integers(0, 256, size=(sh, sw, 3) if k == "eyes" else (H, W, 3), dtype=np.uint8) for _ in range(2)) for k in kinds]
    want = [model_pair(*s, rect) if k == "eyes" else s for k, s in zip(kinds, src)]
    ghost = tuple(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(2))
    with blank_de(psm, rect, D=D) as de, blank_de(psm, rect, D=D) as plain:
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        de.setRectification(rect)
        stage(de, kinds[0], *src[0])
        for i, (el, er) in enumerate(want):
            de.CostConst_GPU()
            if i + 1 < len(kinds):                   # the next frame travels; ahead of the blocking one, a pair nobody will see
                stage(de, *((kinds[i + 1],) + src[i + 1] if kinds[i + 1] != "blocking" else ("pair",) + ghost))
            de.CostFilter_GPU()
            de.DispSelect_device()
            lm, rm = (m.copy() for m in de.download_maps())
            gl, gr = de.download_images()
            assert_same_bytes(gl, el, f"frame {i} ({kinds[i]}) left")
            assert_same_bytes(gr, er, f"frame {i} ({kinds[i]}) right")
            plain.setInputImages(el, er)
            plain.CostConst_GPU()
            plain.CostFilter_GPU()
            plain.DispSelect_GPU()
            assert np.array_equal(lm, plain.lDisMap) and np.array_equal(rm, plain.rDisMap), i
            if i + 1 < len(kinds) and kinds[i + 1] == "blocking":
                de.setInputImages(*src[i + 1])       # supersedes the staged pair: the next CostConst_GPU adopts nothing
    assert not np.array_equal(want[4][0], ghost[0])


def test_frame_ring_push_frame(psm, zed):
    from primestereomatch_amd.dispest import FrameRing
    rect = rect_of(zed, LOOP_CROP)
    frames = [np.concatenate(eyes(s), axis=1) for s in (1, 2, 3, 4)] + [np.concatenate(eyes(2)[::-1], axis=1)]
    want = blocking_maps(psm, rect, frames, 32, "f32")
    z = np.zeros((LOOP_CROP[3], LOOP_CROP[2], 3), np.uint8)
    got = []
    with FrameRing(z, z, 32, frames=2) as ring:
        ring.setRectification(rect)
        for f in frames:
            done = ring.push_frame(f)
            if done is not None:
                got.append(done)
        got += ring.flush()
    assert len(got) == len(frames)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), i


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_batch_of_rectified_contexts_equals_singles(psm, zed, dtype):
    from primestereomatch_amd.dispest import compute_batch
    rect = rect_of(zed, LOOP_CROP)
    frames = [np.concatenate(eyes(s), axis=1) for s in (1, 2, 3)]
    want = blocking_maps(psm, rect, frames, 32, dtype)
    des = [blank_de(psm, rect, D=32, dtype=dtype) for _ in frames]
    try:
        for k, (de, f) in enumerate(zip(des, frames)):
            de.setRectification(rect)
            if k == 1:
                de.setInputFrame_async(f)                    # one of them staged: the batch adopts it
            else:
                de.setInputFrame(f)
        compute_batch(des)
        for i, de in enumerate(des):
            lm, rm = de.download_maps()
            assert np.array_equal(lm, want[i][0]) and np.array_equal(rm, want[i][1]), i
    finally:
        for de in des:
            de.close()


# ---- 8. refusals, profile, life cycle ----
def test_refusals_name_the_cause(psm, zed):
    capi = psm.capi
    rect = rect_of(zed, CLEAN_CROP)
    l, r = eyes(1)
    vp = C.c_void_p

    def set_maps(de, side, xy, fr, src_w=MAP_W, src_h=MAP_H, cx=160, cy=104):
        xy = np.ascontiguousarray(xy)
        fr = np.ascontiguousarray(fr)
        return de._lib.psm_rectify_set_maps(de._h, side, xy.ctypes.data_as(vp), fr.ctypes.data_as(vp), xy.shape[1], xy.shape[0], src_w, src_h, cx, cy)

    with blank_de(psm, rect) as de:
        # maps missing: none, then only the left side's
        for fn in (False, True):
            assert upload_eyes(de, l, r, asynchronous=fn) != 0
            assert "no rectification maps for the left side" in capi.last_error(de._h)
        assert set_maps(de, 0, zed[0][0], zed[1][0]) == 0
        assert upload_eyes(de, l, r) != 0 and "no rectification maps for the right side" in capi.last_error(de._h)
        # crop outside the maps
        assert set_maps(de, 1, zed[0][1], zed[1][1], cx=400) != 0 and "outside the 1280 x 720 maps" in capi.last_error(de._h)
        assert set_maps(de, 1, zed[0][1], zed[1][1], cy=-1) != 0 and "outside" in capi.last_error(de._h)
        # map_frac >= 1024
        bad = zed[1][1].copy()
        bad[300, 700] = 1024
        assert set_maps(de, 1, zed[0][1], bad) != 0 and ">= 1024" in capi.last_error(de._h)
        # bad side, source size beyond the int16 coordinates
        assert set_maps(de, 2, zed[0][1], zed[1][1]) != 0 and "bad side" in capi.last_error(de._h)
        assert set_maps(de, 1, zed[0][1], zed[1][1], src_w=40000) != 0 and "32767" in capi.last_error(de._h)
        # source sizes differing between the two sides
        assert set_maps(de, 1, zed[0][1], zed[1][1], src_w=1000) == 0
        assert upload_eyes(de, l, r) != 0 and "source sizes of the two sides differ" in capi.last_error(de._h)
        assert set_maps(de, 1, zed[0][1], zed[1][1]) == 0
        # channels != 3, stride below the row size
        assert de._lib.psm_upload_pair_rectified(de._h, l.ctypes.data_as(vp), r.ctypes.data_as(vp), 1, 0) != 0
        assert "channels" in capi.last_error(de._h)
        assert de._lib.psm_upload_pair_rectified_async(de._h, l.ctypes.data_as(vp), r.ctypes.data_as(vp), 4, 0) != 0
        assert "channels" in capi.last_error(de._h)
        assert upload_eyes(de, l, r, stride=100) != 0 and "stride" in capi.last_error(de._h)
        # nothing refused above left a pair behind: the blank pair of the constructor is still the current one
        gl, _ = de.download_images()
        assert not gl.any()
        # float depth: frames are 8-bit (the Python mirror refuses before the library is asked), and a float pair is not handed out
        de.setRectification(rect)
        with pytest.raises(ValueError, match="uint8"):
            de.setInputFrame(np.zeros((720, 2560, 3), np.float32))
        f = np.zeros((512, 960, 3), np.float32)
        de.setInputImages(f, f)
        with pytest.raises(capi.PsmError, match="float pair"):
            de.download_images()
        # ... and now everything is in place
        assert upload_eyes(de, l, r) == 0, capi.last_error(de._h)
        assert np.array_equal(de.download_images()[0], model_pair(l, r, rect)[0])


@pytest.mark.parametrize("asynchronous", [False, True])
def test_one_rectified_upload_is_one_prep_launch(psm, zed, asynchronous):
    capi = psm.capi
    rect = rect_of(zed, LOOP_CROP)
    l, r = eyes(1)
    with blank_de(psm, rect) as de:
        de.setRectification(rect)
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        de.reset_kernel_times()
        before = [de.kernel_time_ms(k)[1] for k in range(13)]
        assert upload_eyes(de, l, r, asynchronous=asynchronous) == 0, capi.last_error(de._h)
        ms, n = de.kernel_time_ms(capi.PSM_K_PREP)
        after = [de.kernel_time_ms(k)[1] for k in range(13)]
        print(f"k_rectify ({'copy' if asynchronous else 'context'} stream): {ms:.4f} ms")
        assert n == before[capi.PSM_K_PREP] + 1 and ms > 0
        assert [a - b for a, b in zip(after, before)] == [1] + [0] * 12


def test_release_scratch_and_clear(psm, zed):
    capi = psm.capi
    rect = rect_of(zed, LOOP_CROP)
    l, r = eyes(2)
    el, er = model_pair(l, r, rect)
    with blank_de(psm, rect) as de:
        de.setRectification(rect)
        de.setInputFrame_async(np.concatenate([l, r], axis=1))
        de.release_scratch()                                       # the source slots go, the maps and the staged pair stay
        de.CostConst_GPU()
        assert np.array_equal(de.download_images()[1], er)
        assert upload_eyes(de, r, l) == 0                          # slots come back on demand
        assert np.array_equal(de.download_images()[0], RM.remap_u8(r, rect.map_xy[0], rect.map_frac[0], rect.crop))
        de.clearRectification()
        assert upload_eyes(de, l, r) != 0 and "no rectification maps" in capi.last_error(de._h)
        # maps for a source of another size after a first use: the slots are re-made
        small = rect_of(zed, LOOP_CROP, src_w=1100, src_h=650)
        de.setRectification(small)
        ls, rs = eyes(5, 1100, 650)
        assert upload_eyes(de, ls, rs) == 0, capi.last_error(de._h)
        assert np.array_equal(de.download_images()[0], model_pair(ls, rs, small)[0])


# ---- 9. the C++ mirror ----
@pytest.mark.parametrize("mode", ["f32", "u8"])
def test_cpp_rectify_demo(psm, zed, tmp_path, mode):
    """host/psm_rectify_demo: setRectification + setInputFrame + downloadImages, the stage calls, DispEst::computeVideoFrame's loop
    and FrameRing::push_frame - images == the model's, maps == the Python run's."""
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_rectify_demo")
    if not os.path.exists(demo):
        subprocess.run(["make", "-C", os.path.join(ROOT, "primestereomatch_amd", "host")], check=True)
    crop = LOOP_CROP
    rect = rect_of(zed, crop)
    l, r = eyes(3)
    frame = np.ascontiguousarray(np.concatenate([l, r], axis=1))
    frame.tofile(tmp_path / "frame.raw")
    for s, name in enumerate("lr"):
        zed[0][s].tofile(tmp_path / f"m_{name}_xy.raw")
        zed[1][s].tofile(tmp_path / f"m_{name}_frac.raw")
    env = dict(os.environ, PRIMESM_HIP_LIB=psm.capi.LIB_PATH)
    W, H = crop[2], crop[3]
    p = subprocess.run([demo, str(tmp_path / "frame.raw"), str(MAP_W), str(MAP_H), str(tmp_path / "m"), str(MAP_W), str(MAP_H), str(crop[0]),
                        str(crop[1]), str(W), str(H), "32", str(tmp_path / "o"), mode, "4", "4"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    assert "Rectified" in p.stdout and "Frame loop" in p.stdout and "Frame ring" in p.stdout and "DIFFER" not in p.stdout
    el, er = model_pair(l, r, rect)
    assert np.array_equal(np.fromfile(tmp_path / "o_limg.raw", np.uint8).reshape(H, W, 3), el)
    assert np.array_equal(np.fromfile(tmp_path / "o_rimg.raw", np.uint8).reshape(H, W, 3), er)
    want = blocking_maps(psm, rect, [frame], 32, mode)[0]
    for tag in ("", "_loop", "_ring"):
        assert np.array_equal(np.fromfile(tmp_path / f"o_ldisp{tag}.raw", np.uint8).reshape(H, W), want[0]), tag
        assert np.array_equal(np.fromfile(tmp_path / f"o_rdisp{tag}.raw", np.uint8).reshape(H, W), want[1]), tag
