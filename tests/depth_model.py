"""The definition of the reprojection stage (psm_reproject): cv::reprojectImageTo3D of a disparity map with the Q of
cv::stereoRectify (the reference computes it at src/StereoMatch.cpp:456-458 and drops it), and the ordered, compacted, coloured
point cloud.  numpy; the device equals it in every bit.

For pixel (x, y) of the W x H map, with Q (16 doubles, row-major), crop_x, crop_y, z_min, z_max:
    xf = (double)(x + crop_x), yf = (double)(y + crop_y)       the maps are the cropped image's, Q speaks of the uncropped one
    d  = the disparity as a double                             gif_disparity / sgm_disparity below
    s_i = ((Q[i][0]*xf + Q[i][1]*yf) + Q[i][2]*d) + Q[i][3]    i = 0..3; fp64, every product and sum rounded on its own
    r = 1.0 / s_3;  p_i = s_i * r                              i = 0..2: the reciprocal-then-multiply reading of Vec3d /= double
A point is void if its pixel is missing or any p_i is not finite; void pixels hold the stored pattern VOID_BITS in every
component of the dense planes.  Every other pixel holds (float)p_i, round to nearest even, +-inf and subnormals kept.  A pixel is
kept for the cloud if it is not void and z_min < zf <= z_max on the stored float zf.  The cloud: the records (POINT) of the kept
pixels in raster order, without gaps.  Agreement with a live OpenCV is unpinned.
"""
import numpy as np

VOID_BITS = 0x7FC00000
FLT_MAX = float(np.finfo(np.float32).max)
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])
DEPTH_GIF, DEPTH_SGM = 0, 1


def q_from_projections(P1, P2):
    """The Q of cv::stereoRectify (horizontal stereo) from its two projection matrices."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    f, cx, cy, cx2 = P1[0, 0], P1[0, 2], P1[1, 2], P2[0, 2]
    tx = P2[0, 3] / f
    return np.array([[1.0, 0.0, 0.0, -cx], [0.0, 1.0, 0.0, -cy], [0.0, 0.0, 0.0, f], [0.0, 0.0, -1.0 / tx, (cx - cx2) / tx]], np.float64)


def scale_q(Q, s):
    """The Q of the same cameras at s times the resolution (rectify.scale_calibration): the last column scales, 1 / Tx does not."""
    out = np.array(Q, np.float64).reshape(4, 4).copy()
    out[:, 3] *= s
    return out


def gif_disparity(lmap, lvalid=None):
    """PSM_DEPTH_GIF: d = the byte of the left 8-bit map; missing only under PSM_DEPTH_USE_MASK (lvalid given): validity byte 0.
    -> (d float64 [H, W], missing bool [H, W])"""
    lmap = np.asarray(lmap, np.uint8)
    missing = np.zeros(lmap.shape, bool) if lvalid is None else np.asarray(lvalid) == 0
    return lmap.astype(np.float64), missing


def sgm_disparity(d16, min_disparity=0):
    """PSM_DEPTH_SGM: d = v / 16 (exact) of the int16 map; missing: v == (min_disparity - 1) * 16."""
    d16 = np.asarray(d16, np.int16)
    return d16.astype(np.float64) * 0.0625, d16 == (min_disparity - 1) * 16


def quantise(img):
    """A left image [H, W] or [H, W, ch] as bytes: uint8 as it is, float as sgm_px (psm_sgm.hip) quantises it - the fp32 product
    with 255, rounded to nearest even, saturated."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    v = np.rint(img.astype(np.float32) * np.float32(255.0))
    return np.minimum(np.maximum(v, np.float32(0.0)), np.float32(255.0)).astype(np.uint8)


def reproject(d, missing, Q, crop=(0, 0), z_range=(0.0, FLT_MAX), left=None):
    """-> (xyz [H, W, 3] float32, z [H, W] float32, cloud [count] POINT).  d, missing: gif_disparity / sgm_disparity; left: the
    left image for the colours (None: zeros)."""
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    H, W = d.shape
    xf = (np.arange(W, dtype=np.int64) + int(crop[0])).astype(np.float64)[None, :]
    yf = (np.arange(H, dtype=np.int64) + int(crop[1])).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        s = [((Q[i, 0] * xf + Q[i, 1] * yf) + Q[i, 2] * d) + Q[i, 3] for i in range(4)]
        r = 1.0 / s[3]
        p = np.stack([s[i] * r for i in range(3)], axis=-1)
        void = missing | ~np.isfinite(p).all(axis=-1)
        xyz = p.astype(np.float32)
    bits = xyz.view(np.uint32)
    bits[void] = VOID_BITS
    zf = xyz[..., 2]
    with np.errstate(invalid="ignore"):
        keep = ~void & (zf > np.float32(z_range[0])) & (zf <= np.float32(z_range[1]))
    cloud = np.zeros(int(keep.sum()), POINT)
    cloud["x"], cloud["y"], cloud["z"] = xyz[keep, 0], xyz[keep, 1], xyz[keep, 2]
    cloud["a"] = 255
    if left is not None:
        q = quantise(left)
        q = q[..., None] if q.ndim == 2 else q
        for k, name in enumerate("bgr"):
            cloud[name] = q[..., min(k, q.shape[2] - 1)][keep]
    return xyz, np.ascontiguousarray(zf), cloud


def reproject_scalar(d, missing, Q, crop=(0, 0), z_range=(0.0, FLT_MAX)):
    """The same arithmetic, pixel by pixel in Python floats (IEEE doubles): -> (xyz bit patterns [H, W, 3] uint32, keep [H, W])."""
    import math
    import struct
    Q = [float(v) for v in np.asarray(Q, np.float64).reshape(16)]
    H, W = d.shape
    bits = np.empty((H, W, 3), np.uint32)
    keep = np.zeros((H, W), bool)
    zmin = float(np.float32(z_range[0]))
    zmax = float(np.float32(z_range[1]))

    def to_f32(v):
        try:
            return struct.unpack("<I", struct.pack("<f", v))[0]
        except OverflowError:                                # beyond the largest float: rounds to the infinity of its sign
            return 0x7F800000 if v > 0 else 0xFF800000

    for y in range(H):
        for x in range(W):
            xf, yf, dd = float(x + crop[0]), float(y + crop[1]), float(d[y, x])
            s = [((Q[4 * i] * xf + Q[4 * i + 1] * yf) + Q[4 * i + 2] * dd) + Q[4 * i + 3] for i in range(4)]
            r = 1.0 / s[3] if s[3] != 0.0 else math.copysign(math.inf, s[3])      # (Python raises where IEEE gives the infinity)
            p = [s[i] * r for i in range(3)]
            if bool(missing[y, x]) or not all(math.isfinite(v) for v in p):
                bits[y, x] = VOID_BITS
                continue
            bits[y, x] = [to_f32(v) for v in p]
            zf = struct.unpack("<f", struct.pack("<I", int(bits[y, x, 2])))[0]
            keep[y, x] = zmin < zf <= zmax
    return bits, keep
