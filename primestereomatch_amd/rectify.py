"""Video mode (StereoMatch's DE_VIDEO branch, src/StereoMatch.cpp:43-79,138-153,455-481): calibration files, the CV_16SC2
rectification maps and the record DispEst.setRectification takes.  The maps are built by the library's host-side
psm_rectify_build_maps (no device, no OpenCV needed); the remap itself runs on the device (psm_upload_pair_rectified).
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass

import numpy as np

from . import capi


def read_opencv_yaml(path: str) -> dict:
    """The subset of OpenCV's FileStorage YAML the reference's data/intrinsics.yml and data/extrinsics.yml use: `%YAML:1.0`,
    top-level `name: !!opencv-matrix` nodes with rows / cols / dt: d / data: [...].  -> {name: float64 array [rows, cols]}"""
    txt = open(path).read()
    if not txt.lstrip().startswith("%YAML:1.0"):
        raise ValueError(f"{path}: not an OpenCV %YAML:1.0 file")
    out = {}
    node = re.compile(r"^(\w+):\s*!!opencv-matrix\s*$(.*?)(?=^\w+:\s*!!opencv-matrix\s*$|\Z)", re.S | re.M)
    for m in node.finditer(txt):
        body = m.group(2)
        f = {k: re.search(rf"^\s*{k}:\s*(\S+)\s*$", body, re.M) for k in ("rows", "cols", "dt")}
        data = re.search(r"^\s*data:\s*\[(.*?)\]", body, re.S | re.M)
        if not all(f.values()) or not data:
            raise ValueError(f"{path}: malformed matrix node {m.group(1)}")
        if f["dt"].group(1) not in ("d", "f"):
            raise ValueError(f"{path}: {m.group(1)}: element type {f['dt'].group(1)} (d or f expected)")
        rows, cols = int(f["rows"].group(1)), int(f["cols"].group(1))
        vals = [float(v) for v in data.group(1).split(",")]
        if len(vals) != rows * cols:
            raise ValueError(f"{path}: {m.group(1)}: {len(vals)} values for {rows} x {cols}")
        out[m.group(1)] = np.array(vals, np.float64).reshape(rows, cols)
    return out


def load_calibration(intrinsics_yml: str, extrinsics_yml: str) -> dict:
    """-> {"M1", "D1", "M2", "D2", "R1", "R2", "P1", "P2", ...}: the matrices StereoMatch reads for its two
    initUndistortRectifyMap calls (src/StereoMatch.cpp:440-466)."""
    cal = read_opencv_yaml(intrinsics_yml)
    cal.update(read_opencv_yaml(extrinsics_yml))
    for k in ("M1", "D1", "M2", "D2", "R1", "R2", "P1", "P2"):
        if k not in cal:
            raise ValueError(f"calibration: matrix {k} missing")
    return cal


def scale_calibration(cal: dict, s: float) -> dict:
    """The same cameras at s times the resolution: focal lengths and principal points of M1, M2, P1, P2 scale, nothing else."""
    out = {k: v.copy() for k, v in cal.items()}
    for k in ("M1", "M2", "P1", "P2"):
        out[k][:2, :] *= s
    return out


def scale_q(Q, s: float):
    """The Q of the same cameras at s times the resolution (next to scale_calibration): -cx, -cy, f and (cx - cx2) / Tx - the last
    column - scale; 1 / Tx, the baseline's reciprocal, does not."""
    out = np.array(Q, np.float64).reshape(4, 4).copy()
    out[0, 3] *= s
    out[1, 3] *= s
    out[2, 3] *= s
    out[3, 3] *= s
    return out


def q_from_projections(P1, P2):
    """The Q of cv::stereoRectify (horizontal stereo) from its two projection matrices, for calibration files that do not carry
    it.  Reproduces the Q of tests/golden/zed_extrinsics.yml - a value a real OpenCV wrote - from that file's P1 and P2 bit for
    bit (tests/test_depth_model.py)."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    f, cx, cy, cx2 = P1[0, 0], P1[0, 2], P1[1, 2], P2[0, 2]
    tx = P2[0, 3] / f
    return np.array([[1.0, 0.0, 0.0, -cx], [0.0, 1.0, 0.0, -cy], [0.0, 0.0, 0.0, f], [0.0, 0.0, -1.0 / tx, (cx - cx2) / tx]], np.float64)


def build_maps(M, D, R, P, map_w: int, map_h: int):
    """initUndistortRectifyMap(M, D, R, P, Size(map_w, map_h), CV_16SC2) through psm_rectify_build_maps.
    -> (map_xy [map_h, map_w, 2] int16, map_frac [map_h, map_w] uint16)"""
    lib = capi.load()
    M = np.ascontiguousarray(M, np.float64).reshape(9)
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    P = np.ascontiguousarray(P, np.float64).reshape(12)
    D = np.ascontiguousarray(D if D is not None else [], np.float64).reshape(-1)
    xy = np.empty((map_h, map_w, 2), np.int16)
    fr = np.empty((map_h, map_w), np.uint16)
    pd = C.POINTER(C.c_double)
    capi.check(lib.psm_rectify_build_maps(M.ctypes.data_as(pd), D.ctypes.data_as(pd) if D.size else None, int(D.size), R.ctypes.data_as(pd),
                                          P.ctypes.data_as(pd), int(map_w), int(map_h), xy.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p)),
               None, "build_maps")
    return xy, fr


@dataclass
class Rectification:
    """What DispEst.setRectification takes: the maps of both sides (dense, map_h x map_w), the size of the eye images they index
    and the crop (x, y, w, h) of the rectified image that becomes the DispEst input - lFrame_rec(cropBox)."""
    map_xy: tuple          # (left, right) int16 [map_h, map_w, 2]
    map_frac: tuple        # (left, right) uint16 [map_h, map_w]
    src_w: int
    src_h: int
    crop: tuple = None     # (x, y, w, h); None: the whole src_w x src_h image
    Q: object = None       # the 4 x 4 Q of cv::stereoRectify (None: unknown) - DispEst.setRectification then sets the reprojection too

    def __post_init__(self):
        if self.crop is None:
            self.crop = (0, 0, int(self.src_w), int(self.src_h))

    @classmethod
    def from_calibration(cls, cal: dict, width: int, height: int, crop=None):
        """Both cameras' maps at width x height (the calibration's imgSize: maps and eye images have that size)."""
        l = build_maps(cal["M1"], cal["D1"], cal["R1"], cal["P1"], width, height)
        r = build_maps(cal["M2"], cal["D2"], cal["R2"], cal["P2"], width, height)
        Q = np.array(cal["Q"], np.float64).reshape(4, 4) if "Q" in cal else q_from_projections(cal["P1"], cal["P2"])
        return cls((l[0], r[0]), (l[1], r[1]), int(width), int(height), tuple(crop) if crop else (0, 0, int(width), int(height)), Q)
