"""-m gpu: the speckle filter of the semi-global matching stage on the device (psm_sgm_set_speckle, psm_sgm_filter_speckles;
DispEst.SGBM_GPU(speckle_window_size=, speckle_range=), DispEst.filter_speckles) against its definition, the numpy model
tests/speckle_model.py.  Everything is integer: the filtered map and the plane of component sizes must equal the model with
0 differing elements - there is no tolerance anywhere in this file."""
import ctypes as C
import time

import numpy as np
import pytest

import speckle_model as M

pytestmark = pytest.mark.gpu

NEW = -16
REF = dict(speckle_window_size=100, speckle_range=32)      # setupOpenCVSGBM, src/StereoMatch.cpp:639-660


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def blank_ctx(psm, W, H, **kw):
    """A context of the map's size; the filter reads nothing of its pair."""
    img = np.zeros((H, W, 3), np.uint8)
    return psm.DispEst(img, img, kw.pop("D", 2), **kw)


def check(name, de, got, want):
    """The map `got` and the size plane of de's last filter run against a model result; prints the counts, asserts 0."""
    sizes = de.sgm_speckle_sizes()
    nm, ns = int(np.count_nonzero(got != want[0])), int(np.count_nonzero(sizes != want[1]))
    print(f"[speckle] {name}: differing elements map {nm}  sizes {ns}  (components' largest {int(want[1].max())})")
    assert got.dtype == np.int16 and sizes.dtype == np.int32 and got.shape == want[0].shape
    assert (nm, ns) == (0, 0)


def run(psm, name, img, new_val, max_size, max_diff, de=None):
    img = np.ascontiguousarray(img, dtype=np.int16)
    want = M.filter_speckles(img, new_val, max_size, max_diff)
    if de is not None:
        check(name, de, de.filter_speckles(img, new_val, max_size, max_diff), want)
        return
    with blank_ctx(psm, img.shape[1], img.shape[0]) as d:
        check(name, d, d.filter_speckles(img, new_val, max_size, max_diff), want)


# ---- adversarial maps ------------------------------------------------------------------------------------------------------
def serpentine(W, H, val=160, far=2000):
    """One path through the whole image: full rows of `val` on the even lines, joined alternately at the right and the left end by
    one pixel of the odd lines, which are `far` elsewhere."""
    img = np.full((H, W), far, np.int16)
    img[0::2] = val
    img[1::4, W - 1] = val
    img[3::4, 0] = val
    return img


def spiral(W, H, val=160, far=-3000):
    """A rectangular spiral of `val`, one pixel wide, walls of `far` one pixel wide between its turns."""
    img = np.full((H, W), far, np.int16)
    x0, y0, x1, y1 = 0, 0, W - 1, H - 1
    x, y = 0, 0
    img[0, 0] = val
    while True:
        moved = False
        for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            if dx == 1: tx, ty = x1, y
            elif dy == 1: tx, ty = x, y1
            elif dx == -1: tx, ty = x0, y
            else: tx, ty = x, y0
            if (tx, ty) == (x, y):
                return img
            img[min(y, ty):max(y, ty) + 1, min(x, tx):max(x, tx) + 1] = val
            x, y = tx, ty
            moved = True
            if dx == 1: y0 += 2
            elif dy == 1: x1 -= 2
            elif dx == -1: y1 -= 2
            else: x0 += 2
            if x0 > x1 or y0 > y1:
                return img
        if not moved:
            return img


def checkerboard(W, H, a=0, b=1000):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) & 1, b, a).astype(np.int16)


def comb(W, H, val=320, far=-16):
    """Vertical teeth one pixel wide on every second column, joined by one full row at the bottom: runs of length 1."""
    img = np.full((H, W), far, np.int16)
    img[:, 0::2] = val
    img[H - 1, :] = val
    return img


def ramp(W, H, step):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((xx + yy) * step - 20000).astype(np.int16)


SIZES = [(8, 8), (8, 37), (70, 8), (67, 45), (129, 33), (200, 64), (450, 375)]      # W not a multiple of 64; W = 8; H = 8


@pytest.mark.parametrize("W,H", SIZES)
def test_adversarial_maps(psm, W, H):
    with blank_ctx(psm, W, H) as de:
        s = serpentine(W, H)
        run(psm, "serpentine", s, NEW, 100, 512, de)
        assert int(M.filter_speckles(s, NEW, 0, 512)[1].max()) == int(np.count_nonzero(s == 160))      # one path, whole image
        run(psm, "serpentine removed", s, NEW, W * H, 0, de)
        run(psm, "spiral", spiral(W, H), NEW, 100, 512, de)
        run(psm, "spiral removed", spiral(W, H), NEW, W * H, 512, de)
        cb = checkerboard(W, H)
        run(psm, "checkerboard removed", cb, NEW, 1, 512, de)
        assert (de.filter_speckles(cb, NEW, 1, 512) == NEW).all()
        run(psm, "checkerboard kept", cb, NEW, 0, 512, de)
        assert np.array_equal(de.filter_speckles(cb, NEW, 0, 512), cb)
        const = np.full((H, W), 777, np.int16)
        run(psm, "constant kept", const, NEW, W * H - 1, 0, de)
        assert int(de.sgm_speckle_sizes().min()) == W * H
        run(psm, "constant removed", const, NEW, W * H, 0, de)
        run(psm, "comb", comb(W, H), NEW, 100, 512, de)
        run(psm, "comb, far value a vertex", comb(W, H, far=-1000), NEW, 100, 512, de)
        run(psm, "ramp at max_diff", ramp(W, H, 16), NEW, W * H - 1, 16, de)
        assert int(de.sgm_speckle_sizes().min()) == W * H
        run(psm, "ramp at max_diff + 1", ramp(W, H, 17), NEW, 1, 16, de)
        assert int(de.sgm_speckle_sizes().max()) == 1


@pytest.mark.parametrize("W,H", [(8, 8), (67, 45), (131, 70), (450, 375)])
def test_random_maps(psm, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    with blank_ctx(psm, W, H) as de:
        for nlev in (2, 3, 4, 5):
            levels = np.array([NEW, 0, 16, 48, 600], np.int16)[:nlev]
            for p_first in (0.2, 0.5):                     # sparse and dense holes
                p = np.full(nlev, (1 - p_first) / (nlev - 1)); p[0] = p_first
                img = levels[rng.choice(nlev, (H, W), p=p)]
                for max_size, max_diff in ((1, 0), (5, 0), (100, 16), (20, 32), (W * H, 600), (0, 16)):
                    run(psm, f"random {nlev} levels ({max_size}, {max_diff})", img, NEW, max_size, max_diff, de)


def test_other_new_values(psm):
    W, H = 93, 41
    rng = np.random.default_rng(3)
    levels = np.array([-16, 0, 16, 32, 48], np.int16)
    img = levels[rng.integers(0, 5, (H, W))]
    with blank_ctx(psm, W, H) as de:
        # 16 and 0 also occur as legitimate values next to the components: they are holes then, -16 an ordinary value
        for new_val in (16, 0, 32767, -32768, 5):
            for max_size, max_diff in ((3, 16), (50, 16), (4, 0)):
                run(psm, f"new_val {new_val} ({max_size}, {max_diff})", img, new_val, max_size, max_diff, de)


def test_int16_extremes(psm):
    W, H = 70, 19
    img = np.where(checkerboard(W, H) > 0, 32767, -32768).astype(np.int16)
    with blank_ctx(psm, W, H) as de:
        for md in (0, 32767, 65534):
            run(psm, f"extremes max_diff {md}", img, 0, 1, md, de)
            assert int(de.sgm_speckle_sizes().max()) == 1          # 32767 - (-32768) did not wrap
        run(psm, "extremes max_diff 65535", img, 0, 1, 65535, de)
        assert int(de.sgm_speckle_sizes().min()) == W * H
        run(psm, "extremes max_diff 2^31 - 1", img, 0, 1, 2 ** 31 - 1, de)
        img[:, : W // 2] = 32767
        img[:, W // 2:] = -32768
        run(psm, "two halves", img, 0, W * H // 2, 65534, de)


def test_1080p(psm):
    W, H = 1920, 1080
    with blank_ctx(psm, W, H) as de:
        run(psm, "1080p serpentine", serpentine(W, H), NEW, 100, 512, de)
        assert int(de.sgm_speckle_sizes().max()) == (H // 2) * W + (H // 2)
        run(psm, "1080p constant", np.full((H, W), 100, np.int16), NEW, 100, 512, de)
        rng = np.random.default_rng(0)
        img = np.array([NEW, 0, 16, 600], np.int16)[rng.choice(4, (H, W), p=(0.3, 0.3, 0.3, 0.1))]
        run(psm, "1080p random", img, NEW, 100, 16, de)


# ---- through the stage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_goldens_through_sgbm(psm, golden, name):
    p, g = golden(f"{name}_pair.npz"), golden(f"{name}_sgm.npz")
    want = M.filter_speckles(g["disp"], NEW, 100, 512)
    with psm.DispEst(p["l_bgr"], p["r_bgr"], 64) as de:
        plain = de.SGBM_GPU()
        C0, S0 = de.sgm_costs()
        assert np.array_equal(plain, g["disp"])
        check(f"{name} (100, 32)", de, de.SGBM_GPU(**REF), want)
        print(f"[speckle] {name}: pixels removed {int(np.count_nonzero(want[0] != g['disp']))}")
        C1, S1 = de.sgm_costs()
        assert np.array_equal(C0, C1) and np.array_equal(S0, S1)               # the filter touches the map only
        assert np.array_equal(de.sgm_disparity(), want[0])
        assert np.array_equal(de.SGBM_GPU(), g["disp"])                        # off again: the setting was that call's
        check(f"{name} (100, 32) again", de, de.SGBM_GPU(**REF), want)
        check(f"{name} (30, 1)", de, de.SGBM_GPU(speckle_window_size=30, speckle_range=1), M.filter_speckles(g["disp"], NEW, 30, 16))
        # set_params does not reset the setting, set_speckle(0, ...) turns it off
        de._ck(de._lib.psm_sgm_set_speckle(de._h, 100, 32), "psm_sgm_set_speckle")
        de._ck(de._lib.psm_sgm_set_params(de._h, 0, 0, 0, 10, 1), "psm_sgm_set_params")
        de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
        check(f"{name} after set_params", de, de.sgm_disparity(), want)
        de._ck(de._lib.psm_sgm_set_speckle(de._h, 0, 32), "psm_sgm_set_speckle")
        de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
        assert np.array_equal(de.sgm_disparity(), g["disp"])


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_gray_pairs_and_no_consistency_test(psm, golden, name):
    p = golden(f"{name}_pair.npz")
    l, r = p["l_bgr"], p["r_bgr"]
    gl, gr = np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])
    with psm.DispEst(l, r, 64) as de:
        for what, kw in (("gray", dict(gray=(gl, gr))), ("disp12_max_diff -1", dict(disp12_max_diff=-1)),
                         ("gray, disp12_max_diff -1", dict(gray=(gl, gr), disp12_max_diff=-1))):
            plain = de.SGBM_GPU(**kw)                      # the stage itself is held to its model in test_gpu_sgm.py
            check(f"{name} {what}", de, de.SGBM_GPU(**kw, **REF), M.filter_speckles(plain, NEW, 100, 512))


# ---- contract --------------------------------------------------------------------------------------------------------------
def test_refusals(psm):
    capi = psm.capi
    W, H = 64, 32
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, 16, seed=0)
    img = np.zeros((H, W), np.int16)
    with psm.DispEst(l, r, 16) as de:
        with pytest.raises(capi.PsmError, match="no filter run"):
            de.sgm_speckle_sizes()
        for kw in (dict(speckle_window_size=-1), dict(speckle_range=-1), dict(speckle_window_size=100, speckle_range=-5)):
            with pytest.raises(capi.PsmError, match="negative"):
                de.SGBM_GPU(**kw)
        for args, word in (((NEW, -1, 0), "max_speckle_size"), ((NEW, 0, -1), "max_diff"), ((40000, 1, 1), "new_val"), ((-40000, 1, 1), "new_val")):
            with pytest.raises(capi.PsmError, match=word):
                de.filter_speckles(img, *args)
        with pytest.raises(ValueError):
            de.filter_speckles(img.astype(np.int32), NEW, 1, 1)
        with pytest.raises(ValueError):
            de.filter_speckles(img[:, :-1], NEW, 1, 1)
        assert de._lib.psm_sgm_filter_speckles(de._h, None, 0, NEW, 1, 1) != 0 and "NULL" in capi.last_error(de._h)
        assert de._lib.psm_sgm_filter_speckles(de._h, img.ctypes.data_as(C.c_void_p), 2 * W - 2, NEW, 1, 1) != 0
        assert "stride" in capi.last_error(de._h)
        # the time: refused without a timed compute, without the filter, and after an untimed compute
        with pytest.raises(capi.PsmError, match="speckle"):
            de.SGBM_GPU(**REF)
            de.sgm_speckle_time()
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        de.SGBM_GPU()
        with pytest.raises(capi.PsmError, match="speckle"):
            de.sgm_speckle_time()
        de.SGBM_GPU(**REF)
        t, t3 = de.sgm_speckle_time(), de.sgm_times()
        print(f"[speckle] times ms: cost {t3[0]:.3f} paths {t3[1]:.3f} select {t3[2]:.3f} speckle {t:.3f}")
        assert t > 0 and len(t3) == 3 and all(v > 0 for v in t3)
        de.set_option(capi.PSM_OPT_PROFILE, 0)
        de.SGBM_GPU(**REF)
        with pytest.raises(capi.PsmError, match="speckle"):
            de.sgm_speckle_time()


def test_filter_leaves_the_last_compute_alone(psm):
    from primestereomatch_amd import synth
    W, H, D = 120, 50, 40
    l, r, _ = synth.make_pair(W, H, D, seed=4)
    rng = np.random.default_rng(0)
    other = np.array([NEW, 0, 16], np.int16)[rng.integers(0, 3, (H, W))]
    with psm.DispEst(l, r, D) as de:
        plain = de.SGBM_GPU()
        filt = de.SGBM_GPU(speckle_window_size=20, speckle_range=2)
        want = M.filter_speckles(plain, NEW, 20, 32)
        check("stage", de, filt, want)
        C0, S0 = de.sgm_costs()
        run(psm, "caller's map", other, NEW, 7, 0, de)
        assert np.array_equal(de.sgm_disparity(), want[0])                     # not the caller's map, not refiltered
        C1, S1 = de.sgm_costs()
        assert np.array_equal(C0, C1) and np.array_equal(S0, S1)
        # idempotent on its own output at the same parameters: what is left are components above the size
        again = de.filter_speckles(filt, NEW, 20, 32)
        assert np.array_equal(again, filt)


def test_on_shards_and_under_a_stripe(psm):
    W, H, D = 64, 32, 16
    img3 = np.zeros((H, W, 3), np.uint8)
    rng = np.random.default_rng(5)
    m = np.array([NEW, 0, 16, 64], np.int16)[rng.integers(0, 4, (H, W))]
    with psm.DispEst(img3, img3, D, d_range=(0, 8)) as sh:
        run(psm, "shard", m, NEW, 6, 16, sh)
    with psm.DispEst(img3, img3, D, d_stride=(1, 2)) as sh:
        run(psm, "strided shard", m, NEW, 6, 16, sh)
    with psm.DispEst(img3, img3, D) as de:
        de.set_rows(8, 24)
        run(psm, "row stripe", m, NEW, 6, 16, de)
    # a context nothing was uploaded to
    capi = psm.capi
    lib, h = capi.load(), C.c_void_p()
    assert lib.psm_create(C.byref(h), W, H, D, capi.PSM_F32, 0) == 0
    try:
        out = m.copy()
        assert lib.psm_sgm_filter_speckles(h, out.ctypes.data_as(C.c_void_p), 0, NEW, 6, 16) == 0
        assert np.array_equal(out, M.filter_speckles(m, NEW, 6, 16)[0])
    finally:
        lib.psm_destroy(h)


def test_pitched_buffers(psm):
    W, H = 77, 29
    rng = np.random.default_rng(6)
    m = np.array([NEW, 0, 16, 64], np.int16)[rng.integers(0, 4, (H, W))]
    want = M.filter_speckles(m, NEW, 9, 16)
    with blank_ctx(psm, W, H) as de:
        for pad in (1, 2, 51):                             # pitches that are and are not multiples of 4 bytes
            buf = np.full((H, W + pad), 12345, np.int16)
            buf[:, :W] = m
            de._ck(de._lib.psm_sgm_filter_speckles(de._h, buf.ctypes.data_as(C.c_void_p), buf.strides[0], NEW, 9, 16), "psm_sgm_filter_speckles")
            assert np.array_equal(buf[:, :W], want[0]) and (buf[:, W:] == 12345).all()
            sz = np.full((H, W + pad), -7, np.int32)
            de._ck(de._lib.psm_sgm_download_speckle_sizes(de._h, sz.ctypes.data_as(C.c_void_p), sz.strides[0]), "psm_sgm_download_speckle_sizes")
            assert np.array_equal(sz[:, :W], want[1]) and (sz[:, W:] == -7).all()


def test_async_compute_with_the_filter(psm):
    from primestereomatch_amd import synth
    capi = psm.capi
    W, H, D = 1280, 720, 128
    l, r, _ = synth.make_pair(W, H, D, seed=0)
    with psm.DispEst(l, r, D) as de:
        plain = de.SGBM_GPU()
        want = M.filter_speckles(plain, NEW, 100, 512)
        de.set_option(capi.PSM_OPT_ASYNC, 1)
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        de._ck(de._lib.psm_sgm_set_speckle(de._h, 100, 32), "psm_sgm_set_speckle")
        de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")              # (allocates the filter's planes)
        de.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):                                 # queued behind each other, no host synchronisation in between
            de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
        wall = (time.perf_counter() - t0) * 1e3
        de.synchronize()
        dev = sum(de.sgm_times()) + de.sgm_speckle_time()
        print(f"[speckle] async: 3 computes enqueued in {wall:.3f} ms, device time of one {dev:.3f} ms")
        assert wall < 3 * dev                              # the calls returned before the device had done their work
        check("async", de, de.sgm_disparity(), want)


def test_release_scratch_then_recompute(psm):
    from primestereomatch_amd import synth
    W, H, D = 90, 44, 20
    l, r, _ = synth.make_pair(W, H, D, seed=6)
    with psm.DispEst(l, r, D) as de:
        want = M.filter_speckles(de.SGBM_GPU(), NEW, 25, 16)
        check("before", de, de.SGBM_GPU(speckle_window_size=25, speckle_range=1), want)
        de.release_scratch()
        with pytest.raises(psm.capi.PsmError):
            de.sgm_speckle_sizes()                         # the plane went with the buffers
        check("after release", de, de.SGBM_GPU(speckle_window_size=25, speckle_range=1), want)
        de.release_scratch()
        run(psm, "filter_speckles after release", want[0], NEW, 40, 16, de)


def test_harness_reports_speckle_ms(psm, golden):
    from primestereomatch_amd import harness
    p, g = golden("cones_pair.npz"), golden("cones_sgm.npz")
    out = harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], p["occl"], 4, **REF)
    assert np.array_equal(out["disp16"], M.filter_speckles(g["disp"], NEW, 100, 512)[0])
    assert out["speckle_ms"] > 0
    assert "speckle_ms" not in harness.compute_sgbm(p["l_bgr"], p["r_bgr"], 64)
