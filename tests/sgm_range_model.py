"""numpy model of the SGM stage under a disparity range (psm_sgm_set_range, DispEst.SGBM_GPU(min_disparity=..., num_disparities=...)):
StereoSGBM::create's minDisparity and numDisparities - the DEFINITION the device is held to, 0 differing elements.  Block cost,
paths, sum and selection are sgm_model's, the prefilter and the half-sample bounds sgm_bt_model's, the direction lists
sgm_mode_model's, all imported and untouched; restated here is only what the range touches.

The D = num_disparities indices k in [0, D), 2 <= D <= 1024, stand for the disparities delta = min_disparity + k,
-1024 <= min_disparity <= 1024.  D is independent of the width: the clamp defines every case.

 1. pixel cost   xr = clamp(x - delta, 0, W - 1), clamped on BOTH sides (a negative delta reaches past the right edge);
                 SAD: c(x,y,k) = sum_ch |L[y][x][ch] - R[y][xr][ch]|;  Birchfield-Tomasi: step 1c of sgm_bt_model with this xr
                 (planes, bounds and border columns as they are)
 2-5.            block cost, paths, sum and selection over k, as sgm_model; d16 = 16 (min_disparity + best_k) + sub, sub only for
                 0 < best_k < D - 1
 6. consistency  a unique pixel lands at column x - (min_disparity + best_k) if that lies in [0, W); the lexicographically smallest
                 (minS, best_k) wins there and disp2 holds its delta; "nothing landed" is a state of its own ("landed" false: -1 can
                 be a disparity).  m >= 0: da = d16 >> 4, db = (d16 + 15) >> 4 (floors, also of a negative d16); a probe (x - dq, dq)
                 is bad if its column is inside the row, something landed there and |disp2 - dq| > m; both bad: rejected
 7. output       int16: d16 where unique and not rejected, else invalid = (min_disparity - 1) * 16.  The speckle filter, when on,
                 runs with newVal = invalid (speckle_model.filter_speckles).  |sub| <= 8: a valid value never equals invalid.
                 16 (min_disparity + D - 1) + 8 <= 32767 and invalid >= -32768 inside the ranges above; S <= 8 * 65535 as before.

Not OpenCV's convention: OpenCV leaves the columns outside [max(maxD, 0), W + min(minD, 0)) invalid; the stage keeps all columns,
as sgm_model does.  Agreement with a live cv::StereoSGBM is unpinned."""
from __future__ import annotations

import numpy as np

import sgm_bt_model as B
import sgm_mode_model as MM
import sgm_model as M

MAX_D = 1024
MAX_MIN = 1024


def check_range(min_disparity, D):
    if not -MAX_MIN <= min_disparity <= MAX_MIN:
        raise ValueError("-1024 <= min_disparity <= 1024")
    if not 2 <= D <= MAX_D:
        raise ValueError("2 <= num_disparities <= 1024")


def invalid_value(min_disparity):
    return (min_disparity - 1) * 16


def right_columns(W, min_disparity, k):
    return np.clip(np.arange(W) - (min_disparity + k), 0, W - 1)


def pixel_cost(L, R, min_disparity, D):
    """SAD -> c [H][W][D] int32"""
    L = M._as3(L).astype(np.int32)
    R = M._as3(R).astype(np.int32)
    H, W, _ = L.shape
    c = np.empty((H, W, D), np.int32)
    for k in range(D):
        c[:, :, k] = np.abs(L - R[:, right_columns(W, min_disparity, k), :]).sum(axis=2)
    return c


def pixel_cost_planes(U, V, min_disparity, D):
    """Step 1c of sgm_bt_model on the two images' planes [H][W][2 ch], with the range's xr -> c [H][W][D] int32"""
    U = U.astype(np.int32)
    V = V.astype(np.int32)
    H, W, n = U.shape
    shift = np.repeat([0, 2], n // 2)
    loU, hiU = B._bounds(U)
    loV, hiV = B._bounds(V)
    c = np.empty((H, W, D), np.int32)
    for k in range(D):
        xr = right_columns(W, min_disparity, k)
        v = V[:, xr]
        c0 = np.maximum(0, np.maximum(U - hiV[:, xr], loV[:, xr] - U))
        c1 = np.maximum(0, np.maximum(v - hiU, loU - v))
        c[:, :, k] = (np.minimum(c0, c1) >> shift).sum(axis=2)
    return c


def consistency(best, minS, unique, d16, m, min_disparity):
    """-> (disp2 [H][W] int32: delta where landed, min_disparity - 1 elsewhere; landed [H][W] bool; valid [H][W] bool)"""
    H, W = best.shape
    none = np.iinfo(np.int64).max
    key = np.full((H, W), none, np.int64)
    xl = np.arange(W)[None, :] - (min_disparity + best)
    yy, xx = np.nonzero(unique & (xl >= 0) & (xl < W))
    np.minimum.at(key, (yy, xl[yy, xx]), (minS[yy, xx] << 10) | best[yy, xx])
    landed = key != none
    disp2 = np.where(landed, min_disparity + (key & 1023), min_disparity - 1).astype(np.int32)
    valid = unique.copy()
    if m >= 0:
        x = np.arange(W)[None, :]
        rows = np.arange(H)[:, None]

        def bad(dq):
            xq = x - dq
            xc = np.clip(xq, 0, W - 1)
            return (xq >= 0) & (xq < W) & landed[rows, xc] & (np.abs(disp2[rows, xc] - dq) > m)
        valid &= ~(bad(d16 >> 4) & bad((d16 + 15) >> 4))
    return disp2, landed, valid


def sgm(L, R, min_disparity, D, mode="hh", pre_filter_cap=0, **params):
    """The whole stage over the disparities min_disparity .. min_disparity + D - 1.  -> the dict of sgm_model.sgm ("best": the index
    k, uint8 up to 256 disparities, uint16 above; "d16", "disp2", "disp" carry min_disparity) plus "landed", "invalid", "range",
    and "planes" when pre_filter_cap > 0."""
    check_range(min_disparity, D)
    directions = MM.MODES[mode]
    L, R = M._as3(L), M._as3(R)
    if L.shape != R.shape:
        raise ValueError("the two images differ in shape")
    bs, P1, P2, u, m = M.resolve_params(L.shape[2], **params)
    if pre_filter_cap:
        planes = B.prefilter(L, pre_filter_cap), B.prefilter(R, pre_filter_cap)
        c = pixel_cost_planes(planes[0], planes[1], min_disparity, D)
    else:
        c = pixel_cost(L, R, min_disparity, D)
    C = M.block_cost(c, bs)
    S, max_l = M.aggregate(C, P1, P2, directions=directions, want_max_l=True)
    best, minS, unique, d16 = M.select(S, u)
    d16 = d16 + 16 * min_disparity
    disp2, landed, valid = consistency(best, minS, unique, d16, m, min_disparity)
    invalid = invalid_value(min_disparity)
    disp = np.where(valid, d16, invalid).astype(np.int16)
    out = {"C": C, "S": S, "best": best.astype(np.uint8 if D <= 256 else np.uint16), "unique": unique, "valid": valid, "d16": d16,
           "disp2": disp2, "disp": disp, "max_l": max_l, "params": (bs, P1, P2, u, m), "landed": landed, "invalid": invalid,
           "range": (min_disparity, D)}
    if pre_filter_cap:
        out["planes"] = planes
    return out
