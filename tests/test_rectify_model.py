"""CPU checks of the video-mode rectification: the calibration reader, the library's host-side map builder
(psm_rectify_build_maps) against the independent numpy statement in rectify_model.py - bit for bit -, the model's known
answers, and the "clean" crop the GPU tests use.  The counts printed / asserted as plain equalities below are records of the
reference's ZED calibration (tests/golden/zed_*.yml = the reference's data/intrinsics.yml, data/extrinsics.yml) at 1280 x 720,
the size whose principal point the calibration has."""
import os
import subprocess

import numpy as np
import pytest

import rectify_model as RM
from conftest import GOLDEN, ROOT

INTR = os.path.join(GOLDEN, "zed_intrinsics.yml")
EXTR = os.path.join(GOLDEN, "zed_extrinsics.yml")
MAP_W, MAP_H = 1280, 720
CLEAN_CROP = (160, 104, 960, 512)
CAMS = {"left": ("M1", "D1", "R1", "P1"), "right": ("M2", "D2", "R2", "P2")}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import rectify
    return rectify


@pytest.fixture(scope="module")
def cal(built):
    return built.load_calibration(INTR, EXTR)


def test_load_calibration(cal):
    assert cal["M1"].shape == (3, 3) and cal["M2"].shape == (3, 3)
    assert cal["D1"].shape == (1, 14) and cal["D2"].shape == (1, 14)
    assert cal["R1"].shape == (3, 3) and cal["R2"].shape == (3, 3)
    assert cal["P1"].shape == (3, 4) and cal["P2"].shape == (3, 4)
    assert cal["M1"][0, 0] == 7.0339557117042818e+02 and cal["M1"][0, 2] == 6.7290005245458997e+02
    assert cal["M2"][1, 2] == 3.7698450000005494e+02 and cal["M1"][2, 2] == 1.0
    assert cal["D1"][0, 0] == -1.6931452836351965e-01 and cal["D1"][0, 7] == -1.0513073240526044e-01
    assert cal["D2"][0, 7] == 1.4236858615791169e-03 and cal["D2"][0, 2] == 0.0
    assert cal["R1"][0, 1] == -3.7783696178740607e-03 and cal["R2"][2, 2] == 9.9987475240563262e-01
    assert cal["P2"][0, 3] == -2.5561950492603728e+03 and cal["P1"][0, 3] == 0.0
    # the product's reader and the model's agree on every matrix
    mine = RM.parse_opencv_yaml(INTR)
    mine.update(RM.parse_opencv_yaml(EXTR))
    assert set(mine) == set(cal)
    for k in mine:
        assert np.array_equal(mine[k], cal[k])


def test_load_calibration_refuses_other_files(built, tmp_path):
    p = tmp_path / "x.yml"
    p.write_text("M1: [1, 2]\n")
    with pytest.raises(ValueError):
        built.read_opencv_yaml(str(p))


@pytest.mark.parametrize("cam", ["left", "right"])
def test_build_maps_bit_for_bit(built, cal, cam):
    M, D, R, P = [cal[k] for k in CAMS[cam]]
    xy, fr = built.build_maps(M, D, R, P, MAP_W, MAP_H)
    mxy, mfr, stats = RM.build_maps(M, D, R, P, MAP_W, MAP_H, want_stats=True)
    assert xy.dtype == np.int16 and fr.dtype == np.uint16 and xy.shape == (MAP_H, MAP_W, 2) and fr.shape == (MAP_H, MAP_W)
    assert np.array_equal(xy, mxy)
    assert np.array_equal(fr, mfr)
    assert int(fr.max()) < 1024
    outside = RM.fully_outside(mxy, MAP_W, MAP_H)
    print(f"{cam}: |coordinate| > 32767 before saturation: {stats['coord_beyond_int16']}, non-finite: {stats['non_finite']}, "
          f"fully outside the source: {outside} of {MAP_W * MAP_H}")
    # plain counts of this calibration (k6 = -0.105 of the left camera makes the rational model's denominator cross zero in the
    # frame corners): 0.057 % of the left camera's entries saturate, 36 % / 25 % of the left / right frame is fully outside
    assert stats["non_finite"] == 0
    assert stats["coord_beyond_int16"] == {"left": 525, "right": 0}[cam]
    assert round(100.0 * outside / (MAP_W * MAP_H)) == {"left": 36, "right": 25}[cam]
    if cam == "left":       # the saturated entries are there, and they are the library's too
        sat = (np.abs(mxy.astype(np.int32)) >= 32767).any(axis=-1)
        assert sat.sum() >= 525 and np.array_equal(xy[sat], mxy[sat])


def test_build_maps_identity(built, cal):
    P = cal["P1"]
    xy, fr = built.build_maps(P[:, :3], None, np.eye(3), P, 320, 200)
    u, v = np.meshgrid(np.arange(320), np.arange(200))
    assert np.array_equal(xy[..., 0], u) and np.array_equal(xy[..., 1], v)
    assert not fr.any()
    mxy, mfr = RM.build_maps(P[:, :3], np.zeros(5), np.eye(3), P, 320, 200)
    assert np.array_equal(xy, mxy) and np.array_equal(fr, mfr)


@pytest.mark.parametrize("n_dist", [4, 5, 8, 12, 14])
def test_build_maps_coefficient_counts(built, cal, n_dist):
    """4, 5, 8, 12 or 14 coefficients, tangential and thin-prism terms non-zero: library == model."""
    D = np.array([-0.17, 0.03, 1.1e-3, -7e-4, 0.011, 0.02, -0.013, 0.004, 2e-4, -3e-4, 1e-4, 5e-5, 0.0, 0.0])[:n_dist]
    xy, fr = built.build_maps(cal["M2"], D, cal["R2"], cal["P2"], 333, 201)
    mxy, mfr = RM.build_maps(cal["M2"], D, cal["R2"], cal["P2"], 333, 201)
    assert np.array_equal(xy, mxy) and np.array_equal(fr, mfr)


def test_build_maps_refusals(built, cal):
    from primestereomatch_amd import capi
    with pytest.raises(capi.PsmError, match="tilt"):
        built.build_maps(cal["M1"], np.r_[np.zeros(12), 0.01, 0.0], cal["R1"], cal["P1"], 16, 16)
    with pytest.raises(capi.PsmError, match="coefficients"):
        built.build_maps(cal["M1"], np.zeros(6), cal["R1"], cal["P1"], 16, 16)
    with pytest.raises(capi.PsmError, match="singular"):
        built.build_maps(cal["M1"], None, np.zeros((3, 3)), cal["P1"], 16, 16)


def test_build_maps_non_finite(built, cal):
    """A denominator that is exactly zero at a pixel: map_xy = (-32768, -32768), frac = 0 - in the library and in the model."""
    P = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    D = np.array([0.0, 0, 0, 0, 0, -1.0, 0, 0])                      # 1 + k4 r2 = 0 where r2 = 1: (u, v) = (1, 0), (0, 1)
    xy, fr = built.build_maps(np.eye(3), D, np.eye(3), P, 4, 4)
    mxy, mfr, stats = RM.build_maps(np.eye(3), D, np.eye(3), P, 4, 4, want_stats=True)
    assert stats["non_finite"] >= 2
    assert np.array_equal(xy, mxy) and np.array_equal(fr, mfr)
    assert tuple(xy[0, 1]) == (-32768, -32768) and fr[0, 1] == 0 and tuple(xy[1, 0]) == (-32768, -32768)


def test_model_known_answers():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=(9, 11, 3), dtype=np.uint8)
    u, v = np.meshgrid(np.arange(11), np.arange(9))
    ident = np.stack([u, v], -1).astype(np.int16)
    zero = np.zeros((9, 11), np.uint16)
    assert np.array_equal(RM.remap_u8(src, ident, zero), src)
    # half a pixel to the right: fx = 16 -> (a + b + 1) >> 1; the last column's right tap is outside and reads 0
    half = RM.remap_u8(src, ident, np.full((9, 11), 16, np.uint16))
    a = src.astype(np.int32)
    b = np.concatenate([a[:, 1:], np.zeros((9, 1, 3), np.int32)], axis=1)
    assert np.array_equal(half, (a + b + 1) >> 1)
    # half a pixel down
    down = RM.remap_u8(src, ident, np.full((9, 11), 16 * 32, np.uint16))
    c = np.concatenate([a[1:], np.zeros((1, 11, 3), np.int32)], axis=0)
    assert np.array_equal(down, (a + c + 1) >> 1)
    # taps at -1 and at src_w / src_h read 0, each on its own
    m = np.array([[[-1, 0], [10, 0], [0, -1], [0, 8], [-2, 0], [11, 3], [-32768, -32768]]], np.int16)
    f = np.full((1, 7), 16 * 32 + 16, np.uint16)                        # all four weights 8192
    got = RM.remap_u8(src, m, f)[0].astype(np.int32)
    assert np.array_equal(got[0], (a[0, 0] + a[1, 0] + 2) >> 2)         # column -1 outside
    assert np.array_equal(got[1], (a[0, 10] + a[1, 10] + 2) >> 2)       # column 11 outside
    assert np.array_equal(got[2], (a[0, 0] + a[0, 1] + 2) >> 2)         # row -1 outside
    assert np.array_equal(got[3], (a[8, 0] + a[8, 1] + 2) >> 2)         # row 9 outside
    assert not got[4].any() and not got[5].any() and not got[6].any()
    # the weights of all 1024 fractions sum to INTER_REMAP_COEF_SCALE and are those of OpenCV's bilinear table
    w = np.stack(RM.weights(np.arange(1024)))
    assert np.all(w.sum(axis=0) == 32768) and w.min() == 0 and w.max() == 32768
    fx, fy = (np.arange(1024) & 31) / 32.0, (np.arange(1024) >> 5) / 32.0
    assert np.array_equal(w[3], np.rint(fx * fy * 32768).astype(np.int64))
    assert np.array_equal(w[0], np.rint((1 - fx) * (1 - fy) * 32768).astype(np.int64))


def test_clean_crop_has_every_tap_inside(cal):
    for cam in CAMS:
        M, D, R, P = [cal[k] for k in CAMS[cam]]
        xy, _ = RM.build_maps(M, D, R, P, MAP_W, MAP_H)
        assert RM.taps_inside(xy, MAP_W, MAP_H, CLEAN_CROP), cam
        assert not RM.taps_inside(xy, MAP_W, MAP_H, None), cam


def test_rectification_record(built, cal):
    rect = built.Rectification.from_calibration(cal, MAP_W, MAP_H, CLEAN_CROP)
    assert rect.crop == CLEAN_CROP and (rect.src_w, rect.src_h) == (MAP_W, MAP_H)
    assert rect.map_xy[0].shape == (MAP_H, MAP_W, 2) and rect.map_frac[1].shape == (MAP_H, MAP_W)
    s = built.scale_calibration(cal, 1.5)
    assert s["M1"][0, 0] == cal["M1"][0, 0] * 1.5 and s["P2"][1, 2] == cal["P2"][1, 2] * 1.5 and s["M1"][2, 2] == 1.0
    assert np.array_equal(s["D1"], cal["D1"]) and np.array_equal(s["R1"], cal["R1"])


def test_rectify_demo_builds_and_reports_no_device(built, tmp_path):
    from primestereomatch_amd import capi
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_rectify_demo")
    assert os.path.exists(demo)
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    np.zeros((16, 32, 3), np.uint8).tofile(tmp_path / "f.raw")
    for s in "lr":
        np.zeros((16, 16, 2), np.int16).tofile(tmp_path / f"m_{s}_xy.raw")
        np.zeros((16, 16), np.uint16).tofile(tmp_path / f"m_{s}_frac.raw")
    env = dict(os.environ, PRIMESM_HIP_LIB=capi.LIB_PATH)
    p = subprocess.run([demo, str(tmp_path / "f.raw"), "16", "16", str(tmp_path / "m"), "16", "16", "0", "0", "16", "16", "8", str(tmp_path / "o")],
                       env=env, capture_output=True, text=True)
    assert p.returncode == 3 and "no HIP device" in p.stderr
