"""numpy model of the SGM stage's second pixel cost (psm_sgm_set_prefilter, DispEst.SGBM_GPU(pre_filter_cap=...)): StereoSGBM's
Sobel-prefiltered Birchfield-Tomasi cost - the DEFINITION the device is held to, 0 differing elements.  Steps 2-7 are sgm_model's,
imported and untouched; only step 1, the pixel cost, is replaced.  Agreement with a live cv::StereoSGBM is unpinned: the text
below is what is built.

pre_filter_cap = cap.  cap 0: step 1 of sgm_model (SAD).  1 <= cap <= 63: ft = max(cap, 15) | 1, and

 1a. prefiltered planes of an image I [H][W][ch] (ch in {1, 3}, W >= 2), over the whole image, yn = max(y-1, 0), ys = min(y+1, H-1):
       1 <= x <= W-2:  g = 2 (I[y][x+1] - I[y][x-1]) + (I[yn][x+1] - I[yn][x-1]) + (I[ys][x+1] - I[ys][x-1])   per channel k
                       P_k[y][x] = min(max(g, -ft), ft) + ft,   Q_k[y][x] = I[y][x][k]
       x = 0, x = W-1: P_k = Q_k = ft   (OpenCV presets the border columns of all its row buffers, the intensity rows included)
     plane order P_0 .. P_{ch-1}, Q_0 .. Q_{ch-1}; P planes have shift 0, Q planes shift 2
 1b. half-sample bounds of a plane row a:  al = x > 0 ? (a[x] + a[x-1]) // 2 : a[x],  ar = x < W-1 ? (a[x] + a[x+1]) // 2 : a[x],
       lo(a, x) = min(a[x], al, ar),  hi(a, x) = max(a[x], al, ar)
 1c. pixel cost, xr = max(x - d, 0), per plane with U of the left image and V of the right: u = U[y][x], v = V[y][xr],
       c0 = max(0, u - hi(V, xr), lo(V, xr) - u),  c1 = max(0, v - hi(U, x), lo(U, x) - v)
       c(x, y, d) = sum over the planes of min(c0, c1) >> shift
"""
from __future__ import annotations

import numpy as np

import sgm_model as M


def filter_threshold(cap):
    if not 1 <= cap <= 63:
        raise ValueError("1 <= pre_filter_cap <= 63")
    return max(int(cap), 15) | 1


def prefilter(img, cap):
    """-> planes [H][W][2 ch] uint8 in the order P_0 .. P_{ch-1}, Q_0 .. Q_{ch-1}"""
    ft = filter_threshold(cap)
    I = M._as3(img).astype(np.int32)
    H, W, ch = I.shape
    if W < 2:
        raise ValueError("W >= 2")
    yn = np.maximum(np.arange(H) - 1, 0)
    ys = np.minimum(np.arange(H) + 1, H - 1)
    out = np.full((H, W, 2 * ch), ft, np.int32)
    dx = I[:, 2:, :] - I[:, :-2, :]                     # I[.][x+1] - I[.][x-1] for x in 1 .. W-2
    g = 2 * dx + dx[yn] + dx[ys]
    out[:, 1:W - 1, :ch] = np.clip(g, -ft, ft) + ft
    out[:, 1:W - 1, ch:] = I[:, 1:W - 1, :]
    return out.astype(np.uint8)


def _bounds(a):
    """lo, hi of every plane row of a [H][W][n] int32"""
    al = a.copy()
    ar = a.copy()
    al[:, 1:] = (a[:, 1:] + a[:, :-1]) // 2
    ar[:, :-1] = (a[:, :-1] + a[:, 1:]) // 2
    return np.minimum(a, np.minimum(al, ar)), np.maximum(a, np.maximum(al, ar))


def pixel_cost_planes(U, V, D):
    """Step 1b, 1c on the two images' planes [H][W][2 ch] -> c [H][W][D] int32"""
    U = U.astype(np.int32)
    V = V.astype(np.int32)
    H, W, n = U.shape
    shift = np.repeat([0, 2], n // 2)
    loU, hiU = _bounds(U)
    loV, hiV = _bounds(V)
    x = np.arange(W)
    c = np.empty((H, W, D), np.int32)
    for d in range(D):
        xr = np.maximum(x - d, 0)
        v = V[:, xr]
        c0 = np.maximum(0, np.maximum(U - hiV[:, xr], loV[:, xr] - U))
        c1 = np.maximum(0, np.maximum(v - hiU, loU - v))
        c[:, :, d] = (np.minimum(c0, c1) >> shift).sum(axis=2)
    return c


def pixel_cost_bt(L, R, D, cap):
    """-> c [H][W][D] int32"""
    return pixel_cost_planes(prefilter(L, cap), prefilter(R, cap), D)


def sgm(L, R, D, pre_filter_cap=63, **params):
    """The whole stage with the prefiltered Birchfield-Tomasi cost.  -> the dict of sgm_model.sgm plus "planes": (left, right).
    pre_filter_cap 0: sgm_model.sgm itself (no planes)."""
    if pre_filter_cap == 0:
        return M.sgm(L, R, D, **params)
    L, R = M._as3(L), M._as3(R)
    if L.shape != R.shape:
        raise ValueError("the two images differ in shape")
    if not 2 <= D <= 256:
        raise ValueError("2 <= D <= 256")
    bs, P1, P2, u, m = M.resolve_params(L.shape[2], **params)
    planes = prefilter(L, pre_filter_cap), prefilter(R, pre_filter_cap)
    C = M.block_cost(pixel_cost_planes(planes[0], planes[1], D), bs)
    S, max_l = M.aggregate(C, P1, P2, want_max_l=True)
    best, minS, unique, d16 = M.select(S, u)
    disp2, valid = M.consistency(best, minS, unique, d16, m)
    disp = np.where(valid, d16, M.INVALID).astype(np.int16)
    return {"C": C, "S": S, "best": best.astype(np.uint8), "unique": unique, "valid": valid, "d16": d16, "disp2": disp2,
            "disp": disp, "max_l": max_l, "params": (bs, P1, P2, u, m), "planes": planes}
