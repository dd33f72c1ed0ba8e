"""CPU-only checks of the definition of the reprojection stage, tests/depth_model.py (psm_reproject): the numpy model
against a scalar statement of the same arithmetic, q_from_projections against a Q a real OpenCV wrote, the figures of the Cones
map, and the one NaN the planes may hold.  All comparisons are exact."""
import os

import numpy as np
import pytest

import depth_model as M
from conftest import GOLDEN


def fixture_cal():
    from primestereomatch_amd import rectify
    return rectify.read_opencv_yaml(os.path.join(GOLDEN, "zed_extrinsics.yml"))


def same_as_scalar(d, missing, Q, crop, zr):
    xyz, z, cloud = M.reproject(d, missing, Q, crop, zr)
    bits, keep = M.reproject_scalar(d, missing, Q, crop, zr)
    assert np.array_equal(xyz.view(np.uint32), bits)
    assert np.array_equal(z.view(np.uint32), bits[..., 2])
    assert len(cloud) == int(keep.sum())
    assert np.array_equal(np.stack([cloud["x"], cloud["y"], cloud["z"]], -1).view(np.uint32), bits[keep])
    return xyz, keep


@pytest.mark.parametrize("seed", range(6))
def test_the_model_equals_the_scalar_statement(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 7)), int(rng.integers(1, 9))
    Q = rng.normal(size=(4, 4)) * 10.0 ** rng.integers(-3, 4, size=(4, 4))
    crop = (int(rng.integers(-40, 40)), int(rng.integers(-40, 40)))
    zr = (-0.5, 3.0)
    d16 = rng.integers(-64, 1024, (H, W)).astype(np.int16)
    d16[rng.random((H, W)) < 0.2] = -16
    same_as_scalar(*M.sgm_disparity(d16), Q, crop, zr)
    lmap = rng.integers(0, 256, (H, W)).astype(np.uint8)
    same_as_scalar(*M.gif_disparity(lmap, rng.integers(0, 2, (H, W)).astype(np.uint8) * 255), Q, crop, zr)
    same_as_scalar(*M.gif_disparity(lmap), Q, crop, zr)


def test_the_model_equals_the_scalar_statement_at_the_edges_of_the_formats():
    cal = fixture_cal()
    d16 = np.array([[0, 1, -16, 32767, -32768, 16, 160, 1600]], np.int16)
    d, miss = M.sgm_disparity(d16)
    for scale in (1.0, 1e60, -1e60, 1e-42, 1e300, 1e-320):      # float overflow to +-inf, subnormal floats, double overflow, a subnormal double
        Q = cal["Q"].copy()
        Q[2, 3] *= scale
        xyz, keep = same_as_scalar(d, miss, Q, (0, 0), (0.0, M.FLT_MAX))
        assert not keep[0, 0] and xyz.view(np.uint32)[0, 0, 2] == M.VOID_BITS       # d = 0 with a CALIB_ZERO_DISPARITY Q: s_3 = 0
    Q = cal["Q"].copy()
    Q[3, 3] = 0.5                                                                  # disparity 0 is finite
    xyz, keep = same_as_scalar(d, miss, Q, (3, 5), (0.0, M.FLT_MAX))
    assert keep[0, 0] and np.isfinite(xyz[0, 0]).all()


def test_q_from_projections_reproduces_the_q_opencv_wrote():
    from primestereomatch_amd import rectify
    cal = fixture_cal()
    assert np.array_equal(M.q_from_projections(cal["P1"], cal["P2"]), cal["Q"])
    assert np.array_equal(rectify.q_from_projections(cal["P1"], cal["P2"]), cal["Q"])
    # half the resolution (an exact scaling): the scaled Q is the Q of the scaled projections
    half = rectify.scale_calibration({k: cal[k] for k in ("P1", "P2")} | {"M1": np.eye(3), "M2": np.eye(3)}, 0.5)
    assert np.array_equal(rectify.scale_q(cal["Q"], 0.5), M.q_from_projections(half["P1"], half["P2"]))
    assert np.array_equal(M.scale_q(cal["Q"], 0.5), rectify.scale_q(cal["Q"], 0.5))


def test_the_cones_map_gives_a_cloud_neither_empty_nor_full(golden):
    d16 = golden("cones_sgm.npz")["disp"]
    d, miss = M.sgm_disparity(d16)
    xyz, z, cloud = M.reproject(d, miss, fixture_cal()["Q"], (0, 0), (0.0, 100.0))
    void = xyz.view(np.uint32)[..., 2] == M.VOID_BITS
    assert d16.size == 168750
    assert int(miss.sum()) == 15576
    assert int(void.sum()) - int(miss.sum()) == 61 and int(((d16 == 0) & ~miss).sum()) == 61
    assert len(cloud) == 96678
    assert 40.57 <= float(cloud["z"].min()) < 40.58 and float(cloud["z"].max()) < 100.0
    assert np.array_equal(z, xyz[..., 2], equal_nan=True) and (cloud["a"] == 255).all()


def test_the_only_nan_is_the_void_pattern(golden):
    cal = fixture_cal()
    d, miss = M.sgm_disparity(golden("cones_sgm.npz")["disp"])
    for Q in (cal["Q"], cal["Q"] * -1.0, np.where(cal["Q"] == 0, 0.0, 1e200)):
        xyz, z, _ = M.reproject(d, miss, Q)
        bits = xyz.view(np.uint32)
        nan = np.isnan(xyz)
        assert M.VOID_BITS == 0x7FC00000 and (bits[nan] == M.VOID_BITS).all()
        assert nan.all(axis=-1)[nan.any(axis=-1)].all()                  # a void pixel is void in every component
        assert nan.any(axis=-1)[miss].all()


def test_the_record_is_16_bytes_and_colours_follow_the_pair():
    assert M.POINT.itemsize == 16 and [M.POINT.fields[k][1] for k in ("x", "y", "z", "b", "g", "r", "a")] == [0, 4, 8, 12, 13, 14, 15]
    lmap = np.full((2, 3), 4, np.uint8)
    Q = fixture_cal()["Q"]
    bgr = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)
    c = M.reproject(*M.gif_disparity(lmap), Q, left=bgr)[2]
    assert len(c) == 6 and list(c["b"]) == [0, 3, 6, 9, 12, 15] and list(c["r"]) == [2, 5, 8, 11, 14, 17]
    gray = np.arange(6, dtype=np.uint8).reshape(2, 3)
    c = M.reproject(*M.gif_disparity(lmap), Q, left=gray)[2]
    assert list(c["b"]) == list(c["g"]) == list(c["r"]) == [0, 1, 2, 3, 4, 5]
    f = np.array([[[0.5, 2.0, -1.0], [0.498, 0.002, 1.0 / 255.0], [0.0, 1.0, 0.3]]] * 2, np.float32)      # 127.5 -> 128 (even), saturation
    c = M.reproject(*M.gif_disparity(lmap), Q, left=f)[2]
    assert (c["b"][0], c["g"][0], c["r"][0]) == (128, 255, 0) and (c["b"][1], c["g"][1], c["r"][1]) == (127, 1, 1)
