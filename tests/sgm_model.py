"""numpy model of the semi-global matching stage (psm_sgm_compute) - the DEFINITION the device is held to, 0 differing elements.

Hirschmueller's recurrence with OpenCV's parameter names and the reference's parameter values (setupOpenCVSGBM,
src/StereoMatch.cpp:639-660: blockSize 5, P1 = 8 ch bs^2, P2 = 32 ch bs^2, disp12MaxDiff 1, uniquenessRatio 10, eight paths as
MODE_HH).  Everything is integer.  Not part of it, and open: the speckle filter (speckleWindowSize 100, speckleRange 32) and
OpenCV's Sobel-prefiltered Birchfield-Tomasi pixel cost (preFilterCap 63) - the pixel cost here is plain SAD.  Agreement with a
live cv::StereoSGBM is unpinned.

Inputs: an 8-bit pair [H][W] or [H][W][ch], ch in {1, 3}; disparities d in [0, D), 2 <= D <= 256, minDisparity 0.  A float pair
is quantised first as lFrame.convertTo(lFrame, CV_8U, 255) does (src/StereoMatch.cpp:174-177).

 1. pixel cost   c(x,y,d) = sum_ch |L[y][x][ch] - R[y][max(x-d, 0)][ch]|
 2. block cost   C(x,y,d) = sum_{j,i in [-bs/2, bs/2]} c(clampx(x+i), clampy(y+j), d)        (the plane c(.,.,d) replicated at the edge)
 3. paths        r = (dy,dx) in DIRECTIONS; with p-r inside the image and m_r = min_k L_r(p-r,k):
                 L_r(p,d) = C(p,d) + min(L_r(p-r,d), L_r(p-r,d-1)+P1, L_r(p-r,d+1)+P1, m_r+P2) - m_r   (d+-1 absent outside [0, D))
                 L_r(p,d) = C(p,d) where p-r is outside
 4. sum          S = sum_r L_r, exact
 5. select       best = argmin_d S (lowest d on ties), minS = S(best);
                 not unique if any d with |d-best| > 1 has S(d) (100-u) < minS 100;
                 0 < best < D-1: den = max(S(best-1)+S(best+1)-2 minS, 1), d16 = 16 best + ((S(best-1)-S(best+1)) 16 + den) // (2 den)
                 else d16 = 16 best
 6. consistency  disp2[y][x-best] = best of the lexicographically smallest (minS, best) over the unique pixels with x-best >= 0
                 (-1: none); m >= 0: da = d16 >> 4, db = (d16+15) >> 4; a probe (xq, dq) is bad if 0 <= xq < W, disp2[y][xq] >= 0 and
                 |disp2[y][xq] - dq| > m; the pixel is rejected if (x-da, da) and (x-db, db) are both bad
 7. output       int16: d16 where unique and not rejected, else -16 = (minDisparity - 1) * 16
"""
from __future__ import annotations

import numpy as np

DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))   # (dy, dx)
INVALID = -16
_INF = 1 << 28


def quantise(img):
    """convertTo(CV_8U, 255) of a float image: saturate_cast<uchar>(cvRound(f * 255.0f)), the product in fp32, ties to even.
    NaN -> 0: the device's fminf(fmaxf(rintf(f * 255.0f), 0.0f), 255.0f), where fmaxf(NaN, 0) is 0 (jwmf_model.feature_u8 alike)."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    with np.errstate(invalid="ignore"):                      # inf * 255, comparisons with NaN
        v = np.rint(img.astype(np.float32) * np.float32(255.0))
        return np.where(v > 0, np.minimum(v, np.float32(255)), np.float32(0)).astype(np.uint8)


def resolve_params(ch, block_size=0, P1=0, P2=0, uniqueness_ratio=10, disp12_max_diff=1):
    """0 for the first three: the default.  Raises ValueError naming the violated condition."""
    bs = block_size or 5
    if bs not in (1, 3, 5, 7):
        raise ValueError("block_size in {1, 3, 5, 7}")
    if ch not in (1, 3):
        raise ValueError("channels in {1, 3}")
    P1 = P1 or 8 * ch * bs * bs
    P2 = P2 or 32 * ch * bs * bs
    if not 0 < P1 <= P2:
        raise ValueError("0 < P1 <= P2")
    if bs * bs * ch * 255 + P2 > 65535:
        raise ValueError("bs^2 * ch * 255 + P2 <= 65535")
    if not 0 <= uniqueness_ratio < 100:
        raise ValueError("0 <= uniqueness_ratio < 100")
    return bs, int(P1), int(P2), int(uniqueness_ratio), int(disp12_max_diff)


def _as3(img):
    img = quantise(img)
    return img[:, :, None] if img.ndim == 2 else img


def pixel_cost(L, R, D):
    """-> c [H][W][D] int32"""
    L = _as3(L).astype(np.int32)
    R = _as3(R).astype(np.int32)
    H, W, _ = L.shape
    x = np.arange(W)
    c = np.empty((H, W, D), np.int32)
    for d in range(D):
        c[:, :, d] = np.abs(L - R[:, np.maximum(x - d, 0), :]).sum(axis=2)
    return c


def block_cost(c, bs):
    """-> C [H][W][D] uint16"""
    h = bs // 2
    H, W, _ = c.shape
    p = np.pad(c, ((h, h), (h, h), (0, 0)), mode="edge")
    C = np.zeros(c.shape, np.int32)
    for j in range(bs):
        for i in range(bs):
            C += p[j:j + H, i:i + W, :]
    assert C.max() <= 65535
    return C.astype(np.uint16)


def _step(Cp, Lp, has_pred, P1, P2):
    """One step of the recurrence for N pixels at once.  Cp, Lp: [N][D] int32; has_pred [N] bool."""
    m = Lp.min(axis=1, keepdims=True)
    lo = np.full_like(Lp, _INF)
    hi = np.full_like(Lp, _INF)
    lo[:, 1:] = Lp[:, :-1] + P1
    hi[:, :-1] = Lp[:, 1:] + P1
    L = Cp + np.minimum(np.minimum(Lp, lo), np.minimum(hi, m + P2)) - m
    return np.where(has_pred[:, None], L, Cp)


def path_cost(C, direction, P1, P2):
    """L_r of one direction (dy, dx) -> [H][W][D] int32"""
    dy, dx = direction
    C = C.astype(np.int32)
    H, W, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        prev = None
        for x in xs:
            L[:, x] = C[:, x] if prev is None else _step(C[:, x], L[:, prev], np.ones(H, bool), P1, P2)
            prev = x
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    prev = None
    xq = np.arange(W) - dx                       # the predecessor's column
    inside = (xq >= 0) & (xq < W)
    for y in ys:
        L[y] = C[y] if prev is None else _step(C[y], L[prev][np.clip(xq, 0, W - 1)], inside, P1, P2)
        prev = y
    return L


def aggregate(C, P1, P2, directions=DIRECTIONS, want_max_l=False):
    """-> S [H][W][D] uint32 (and the largest single-path cost)"""
    S = np.zeros(C.shape, np.int64)
    max_l = 0
    for r in directions:
        L = path_cost(C, r, P1, P2)
        max_l = max(max_l, int(L.max()))
        S += L
    S = S.astype(np.uint32)
    return (S, max_l) if want_max_l else S


def select(S, u):
    """-> best [H][W] int32, minS [H][W] int64, unique [H][W] bool, d16 [H][W] int32"""
    S = S.astype(np.int64)
    H, W, D = S.shape
    best = S.argmin(axis=2).astype(np.int32)            # (numpy: the first minimum = the lowest d)
    minS = S.min(axis=2)
    d = np.arange(D)[None, None, :]
    far = np.abs(d - best[:, :, None]) > 1
    unique = ~np.any(far & (S * (100 - u) < minS[:, :, None] * 100), axis=2)
    inner = (best > 0) & (best < D - 1)
    bm = np.clip(best - 1, 0, D - 1)[:, :, None]
    bp = np.clip(best + 1, 0, D - 1)[:, :, None]
    Sm = np.take_along_axis(S, bm, 2)[:, :, 0]
    Sp = np.take_along_axis(S, bp, 2)[:, :, 0]
    den = np.maximum(Sm + Sp - 2 * minS, 1)
    sub = ((Sm - Sp) * 16 + den) // (2 * den)           # floor division
    d16 = best * 16 + np.where(inner, sub, 0).astype(np.int32)
    return best, minS, unique, d16.astype(np.int32)


def consistency(best, minS, unique, d16, m):
    """-> (disp2 [H][W] int32, valid [H][W] bool)"""
    H, W = best.shape
    key = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    yy, xx = np.nonzero(unique & (np.arange(W)[None, :] - best >= 0))
    np.minimum.at(key, (yy, xx - best[yy, xx]), (minS[yy, xx] << 8) | best[yy, xx])
    disp2 = np.where(key == np.iinfo(np.int64).max, -1, key & 255).astype(np.int32)
    valid = unique.copy()
    if m >= 0:
        x = np.arange(W)[None, :]
        rows = np.arange(H)[:, None]

        def bad(dq):
            xq = x - dq
            ok = (xq >= 0) & (xq < W)
            t = disp2[rows, np.clip(xq, 0, W - 1)]
            return ok & (t >= 0) & (np.abs(t - dq) > m)
        valid &= ~(bad(d16 >> 4) & bad((d16 + 15) >> 4))
    return disp2, valid


def sgm(L, R, D, block_size=0, P1=0, P2=0, uniqueness_ratio=10, disp12_max_diff=1):
    """The whole stage.  -> dict: C u16, S u32 [H][W][D]; best u8, unique, valid bool, d16 int32, disp int16 [H][W]; max_l; params."""
    L, R = _as3(L), _as3(R)
    if L.shape != R.shape:
        raise ValueError("the two images differ in shape")
    if not 2 <= D <= 256:
        raise ValueError("2 <= D <= 256")
    bs, P1, P2, u, m = resolve_params(L.shape[2], block_size, P1, P2, uniqueness_ratio, disp12_max_diff)
    C = block_cost(pixel_cost(L, R, D), bs)
    S, max_l = aggregate(C, P1, P2, want_max_l=True)
    best, minS, unique, d16 = select(S, u)
    disp2, valid = consistency(best, minS, unique, d16, m)
    disp = np.where(valid, d16, INVALID).astype(np.int16)
    return {"C": C, "S": S, "best": best.astype(np.uint8), "unique": unique, "valid": valid, "d16": d16, "disp2": disp2,
            "disp": disp, "max_l": max_l, "params": (bs, P1, P2, u, m)}


def display_map(disp16, scale_factor):
    """The reference's display conversion of imgDisparity16S (src/StereoMatch.cpp:181-185), OpenCV's roundings written out:
    convertTo(CV_8U, a), a = 255 / (maxVal - minVal) formed in double: for a 16-bit source convertScale works in fp32 -
    saturate_cast<uchar>(cvRound((float)v * (float)a)), ties to even; lDispMap / 4 on a CV_8U Mat is convertTo with 0.25 -
    saturate_cast<uchar>(cvRound(v * 0.25f)), ties to even again; * scale_factor saturates."""
    v = np.asarray(disp16).astype(np.float32)
    a = np.float32(255.0 / (float(v.max()) - float(v.min())))
    m = np.clip(np.rint(v * a), 0, 255).astype(np.float32)
    m = np.clip(np.rint(m * np.float32(0.25)), 0, 255)
    return np.clip(m * scale_factor, 0, 255).astype(np.uint8)
