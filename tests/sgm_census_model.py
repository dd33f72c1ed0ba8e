"""numpy model of the SGM stage's third pixel cost (psm_sgm_set_census, DispEst.SGBM_GPU(census=(w, h))): the Hamming distance of
census transforms - the DEFINITION the device is held to, 0 differing elements.  Block cost, paths, sum and selection are
sgm_model's, the direction lists sgm_mode_model's, the right column, the consistency test and the output sgm_range_model's, all
imported and untouched; restated here is only step 1, the pixel cost.  Like the other two costs this is no library's convention:
the text below is what is built.

census = (win_w, win_h), both odd, 3 <= win_w <= 9, 3 <= win_h <= 7: win_w win_h - 1 <= 62 bits, one uint64 per pixel.

 1a. gray plane g [H][W] of the 8-bit image (a float image is quantised first, sgm_model.quantise):
       ch == 1: the byte;  ch == 3, staged order B, G, R: g = (1868 B + 9617 G + 4899 R + 8192) >> 14
     (the stage's own definition; the coefficients sum to 16384, so g <= 255)
 1b. code T [H][W] uint64: the taps (dy, dx) in raster order, dy from -(win_h // 2) up, dx from -(win_w // 2) up, the centre
     skipped, tap i = 0, 1, ...: bit i (bit 0 the least significant) is 1 iff
       g[clamp(y + dy, 0, H - 1)][clamp(x + dx, 0, W - 1)] < g[y][x]
     strictly (a tap equal to the centre gives 0); the plane is replicated at the image edge; the bits above win_w win_h - 2 are 0
 1c. pixel cost  c(x, y, k) = popcount(T_L[y][x] ^ T_R[y][xr]),  xr = clamp(x - (min_disparity + k), 0, W - 1)
     (sgm_range_model.right_columns; with the default range max(x - d, 0), as for the other two costs)

c <= win_w win_h - 1 <= 62, so C <= 49 * 62 = 3038: the condition bs^2 ch 255 + P2 <= 65535 holds as it is, and P1, P2 default to
8 ch bs^2 and 32 ch bs^2 with ch the pair's channels - the parameters do not depend on the cost.
"""
from __future__ import annotations

import numpy as np

import sgm_mode_model as MM
import sgm_model as M
import sgm_range_model as R

GRAY_B, GRAY_G, GRAY_R = 1868, 9617, 4899


def check_window(win_w, win_h):
    if not (3 <= win_w <= 9 and 3 <= win_h <= 7 and win_w % 2 == 1 and win_h % 2 == 1):
        raise ValueError("census window: odd, 3 <= win_w <= 9, 3 <= win_h <= 7")


def gray(img):
    """-> g [H][W] uint8"""
    I = M._as3(img).astype(np.int32)
    if I.shape[2] == 1:
        return I[:, :, 0].astype(np.uint8)
    if I.shape[2] != 3:
        raise ValueError("channels in {1, 3}")
    return ((GRAY_B * I[:, :, 0] + GRAY_G * I[:, :, 1] + GRAY_R * I[:, :, 2] + 8192) >> 14).astype(np.uint8)


def taps(win_w, win_h):
    """The (dy, dx) of tap 0, 1, ... in raster order, the centre skipped"""
    return [(dy, dx) for dy in range(-(win_h // 2), win_h // 2 + 1) for dx in range(-(win_w // 2), win_w // 2 + 1) if (dy, dx) != (0, 0)]


def codes(img, win_w, win_h):
    """-> T [H][W] uint64"""
    check_window(win_w, win_h)
    g = gray(img)
    H, W = g.shape
    hy, hx = win_h // 2, win_w // 2
    p = np.pad(g, ((hy, hy), (hx, hx)), mode="edge")
    T = np.zeros((H, W), np.uint64)
    for i, (dy, dx) in enumerate(taps(win_w, win_h)):
        T |= (p[hy + dy:hy + dy + H, hx + dx:hx + dx + W] < g).astype(np.uint64) << np.uint64(i)
    return T


def popcount(v):
    """of a uint64 array -> int32"""
    b = np.ascontiguousarray(v, np.uint64)
    return np.unpackbits(b.view(np.uint8).reshape(b.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int32)


def pixel_cost_codes(TL, TR, min_disparity, D):
    """Step 1c on the two code planes -> c [H][W][D] int32"""
    H, W = TL.shape
    c = np.empty((H, W, D), np.int32)
    for k in range(D):
        c[:, :, k] = popcount(TL ^ TR[:, R.right_columns(W, min_disparity, k)])
    return c


def pixel_cost(L, Rimg, min_disparity, D, win_w, win_h):
    """-> c [H][W][D] int32"""
    return pixel_cost_codes(codes(L, win_w, win_h), codes(Rimg, win_w, win_h), min_disparity, D)


def sgm(L, Rimg, min_disparity, D, census=(9, 7), mode="hh", **params):
    """The whole stage with the census cost over the disparities min_disparity .. min_disparity + D - 1.  -> the dict of
    sgm_range_model.sgm plus "codes": (T_L, T_R).  census None or (0, 0): sgm_range_model.sgm itself (the SAD cost, no codes)."""
    if census is None or tuple(census) == (0, 0):
        return R.sgm(L, Rimg, min_disparity, D, mode=mode, **params)
    win_w, win_h = census
    check_window(win_w, win_h)
    R.check_range(min_disparity, D)
    directions = MM.MODES[mode]
    L, Rimg = M._as3(L), M._as3(Rimg)
    if L.shape != Rimg.shape:
        raise ValueError("the two images differ in shape")
    bs, P1, P2, u, m = M.resolve_params(L.shape[2], **params)
    T = codes(L, win_w, win_h), codes(Rimg, win_w, win_h)
    C = M.block_cost(pixel_cost_codes(T[0], T[1], min_disparity, D), bs)
    S, max_l = M.aggregate(C, P1, P2, directions=directions, want_max_l=True)
    best, minS, unique, d16 = M.select(S, u)
    d16 = d16 + 16 * min_disparity
    disp2, landed, valid = R.consistency(best, minS, unique, d16, m, min_disparity)
    invalid = R.invalid_value(min_disparity)
    disp = np.where(valid, d16, invalid).astype(np.int16)
    return {"C": C, "S": S, "best": best.astype(np.uint8 if D <= 256 else np.uint16), "unique": unique, "valid": valid, "d16": d16,
            "disp2": disp2, "disp": disp, "max_l": max_l, "params": (bs, P1, P2, u, m), "landed": landed, "invalid": invalid,
            "range": (min_disparity, D), "codes": T}
