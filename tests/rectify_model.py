"""Independent numpy statement of the rectification arithmetic (include/primesm_hip.h "video mode"): test
infrastructure, nothing of the product is imported here.

build_maps: initUndistortRectifyMap(M, D, R, P, size, CV_16SC2) in double, every pixel from its own (u, v).
remap_u8:   cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) with such maps on 8-bit images, followed by the crop.
build_maps_incremental: the reading of OpenCV's own loop, which advances X, Y, Z by additions along a row (a record of how many
            map entries the free choice changes; not a test threshold).
"""
import numpy as np

INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS
INTER_REMAP_COEF_SCALE = 1 << 15


def parse_opencv_yaml(path):
    """The %YAML:1.0 / !!opencv-matrix subset of the calibration files -> {name: float64 array}."""
    import re
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*!!opencv-matrix\s*\n\s*rows:\s*(\d+)\s*\n\s*cols:\s*(\d+)\s*\n\s*dt:\s*(\w+)\s*\n\s*data:\s*\[(.*?)\]",
                         txt, flags=re.S | re.M):
        vals = [float(v) for v in m.group(5).replace("\n", " ").split(",")]
        out[m.group(1)] = np.array(vals, np.float64).reshape(int(m.group(2)), int(m.group(3)))
    return out


def _inverse_rectification(R, P):
    """inv(P[:, :3] * R) by cofactors over the determinant, every sum left to right."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    P = np.asarray(P, np.float64).reshape(3, 4)
    A = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            A[i, j] = (P[i, 0] * R[0, j] + P[i, 1] * R[1, j]) + P[i, 2] * R[2, j]
    C = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[(i + 1) % 3, (j + 1) % 3] * A[(i + 2) % 3, (j + 2) % 3]
                       - A[(i + 1) % 3, (j + 2) % 3] * A[(i + 2) % 3, (j + 1) % 3])
    det = (A[0, 0] * C[0, 0] + A[0, 1] * C[0, 1]) + A[0, 2] * C[0, 2]
    iR = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            iR[i, j] = C[j, i] / det
    return iR


def _distort_and_quantise(X, Y, Z, M, D):
    M = np.asarray(M, np.float64).reshape(3, 3)
    k = np.zeros(14)
    D = np.asarray(D, np.float64).reshape(-1)
    assert D.size in (0, 4, 5, 8, 12, 14)
    k[:D.size] = D
    assert k[12] == 0 and k[13] == 0, "tilted sensor model not supported"
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = [np.float64(v) for v in k[:12]]
    fx, fy, u0, v0 = M[0, 0], M[1, 1], M[0, 2], M[1, 2]
    with np.errstate(all="ignore"):
        x = X / Z
        y = Y / Z
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = (2 * x) * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (((x * kr + p1 * _2xy) + p2 * (r2 + 2 * x2)) + s1 * r2) + (s2 * r2) * r2
        yd = (((y * kr + p1 * (r2 + 2 * y2)) + p2 * _2xy) + s3 * r2) + (s4 * r2) * r2
        mu = fx * xd + u0
        mv = fy * yd + v0
        finite = np.isfinite(mu) & np.isfinite(mv)
        su = np.where(finite, mu * 32.0, 0.0)
        sv = np.where(finite, mv * 32.0, 0.0)
    lo, hi = -2147483648.0, 2147483647.0
    iu = np.where(su <= lo, -2 ** 31, np.where(su >= hi, 2 ** 31 - 1, np.rint(np.clip(su, lo, hi)))).astype(np.int64)
    iv = np.where(sv <= lo, -2 ** 31, np.where(sv >= hi, 2 ** 31 - 1, np.rint(np.clip(sv, lo, hi)))).astype(np.int64)
    cx = np.clip(iu >> INTER_BITS, -32768, 32767)
    cy = np.clip(iv >> INTER_BITS, -32768, 32767)
    frac = (iv & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (iu & (INTER_TAB_SIZE - 1))
    cx = np.where(finite, cx, -32768)
    cy = np.where(finite, cy, -32768)
    frac = np.where(finite, frac, 0)
    map_xy = np.stack([cx, cy], axis=-1).astype(np.int16)
    stats = {"coord_beyond_int16": int(np.count_nonzero(finite & ((np.abs(iu >> INTER_BITS) > 32767) | (np.abs(iv >> INTER_BITS) > 32767)))),
             "non_finite": int(np.count_nonzero(~finite))}
    return map_xy, frac.astype(np.uint16), stats


def build_maps(M, D, R, P, map_w, map_h, want_stats=False):
    """-> (map_xy [map_h, map_w, 2] int16, map_frac [map_h, map_w] uint16)"""
    iR = _inverse_rectification(R, P)
    u = np.arange(map_w, dtype=np.float64)[None, :]
    v = np.arange(map_h, dtype=np.float64)[:, None]
    X = (iR[0, 0] * u + iR[0, 1] * v) + iR[0, 2]
    Y = (iR[1, 0] * u + iR[1, 1] * v) + iR[1, 2]
    Z = (iR[2, 0] * u + iR[2, 1] * v) + iR[2, 2]
    xy, fr, stats = _distort_and_quantise(X, Y, Z, M, D)
    return (xy, fr, stats) if want_stats else (xy, fr)


def build_maps_incremental(M, D, R, P, map_w, map_h):
    """OpenCV's loop: per row X = ir[1]*i + ir[2] ..., then X += ir[0] per column."""
    iR = _inverse_rectification(R, P)
    X = np.empty((map_h, map_w))
    Y = np.empty((map_h, map_w))
    Z = np.empty((map_h, map_w))
    i = np.arange(map_h, dtype=np.float64)
    x = iR[0, 1] * i + iR[0, 2]
    y = iR[1, 1] * i + iR[1, 2]
    z = iR[2, 1] * i + iR[2, 2]
    for j in range(map_w):
        X[:, j], Y[:, j], Z[:, j] = x, y, z
        x = x + iR[0, 0]
        y = y + iR[1, 0]
        z = z + iR[2, 0]
    xy, fr, _ = _distort_and_quantise(X, Y, Z, M, D)
    return xy, fr


def weights(frac):
    """-> (w00, w01, w10, w11) int64 of fy * 32 + fx"""
    frac = np.asarray(frac).astype(np.int64)
    fx = frac & 31
    fy = frac >> 5
    return (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32


def _tap(src, yy, xx):
    h, w = src.shape[:2]
    inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64)
    return v * inside[..., None]


def remap_u8(src, map_xy, map_frac, crop=None):
    """src: [src_h, src_w, 3] uint8; maps of one side; crop = (x, y, w, h) of the maps (None: all) -> [h, w, 3] uint8"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3
    if crop is not None:
        cx, cy, cw, ch = crop
        map_xy = map_xy[cy:cy + ch, cx:cx + cw]
        map_frac = map_frac[cy:cy + ch, cx:cx + cw]
    assert np.all(map_frac < 1024)
    mx = map_xy[..., 0].astype(np.int64)
    my = map_xy[..., 1].astype(np.int64)
    w00, w01, w10, w11 = [w[..., None] for w in weights(map_frac)]
    acc = (w00 * _tap(src, my, mx) + w01 * _tap(src, my, mx + 1) + w10 * _tap(src, my + 1, mx) + w11 * _tap(src, my + 1, mx + 1))
    out = (acc + (1 << 14)) >> 15
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def taps_inside(map_xy, src_w, src_h, crop=None):
    """every one of the four taps of every pixel of the window lies inside the source"""
    if crop is not None:
        cx, cy, cw, ch = crop
        map_xy = map_xy[cy:cy + ch, cx:cx + cw]
    mx = map_xy[..., 0].astype(np.int64)
    my = map_xy[..., 1].astype(np.int64)
    return bool(np.all((mx >= 0) & (mx + 1 < src_w) & (my >= 0) & (my + 1 < src_h)))


def fully_outside(map_xy, src_w, src_h):
    """number of pixels none of whose four taps lies inside the source"""
    mx = map_xy[..., 0].astype(np.int64)
    my = map_xy[..., 1].astype(np.int64)
    return int(np.count_nonzero((mx + 1 < 0) | (mx >= src_w) | (my + 1 < 0) | (my >= src_h)))
