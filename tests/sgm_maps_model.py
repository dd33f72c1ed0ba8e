"""numpy model of psm_sgm_select_maps - the DEFINITION the device is held to, 0 differing elements.  All integer.

The 8-bit disparity maps of both views from the summed path costs S [H][W][D] of the SGM stage (tests/sgm_model.py and its
siblings), computed with the range (dmin, D): index k stands for the disparity dmin + k.

  left   lmap[y][x]  = dmin + argmin_k S[y][x][k], the lowest k on ties - select()'s `best`.  Uniqueness, the sub-pixel step and
                       the disp12MaxDiff test play no part: the post-processing chain's own lrCheck validates the maps.
  right  rmap[y][xr] = dmin + k of the smallest (S[y][xr + dmin + k][k], k) over the k in [0, D) with xr + dmin + k < W, the lowest
                       k on ties: Hirschmueller's D_m(q) = argmin_d S(q.x + d, q.y, d), the search along the epipolar line in the
                       same S.  A column without a candidate (the last dmin columns) gets 0.

Both maps are uint8; the call is defined for dmin >= 0 and dmin + D <= max_disp <= 256 only (the maps index the weighted median's
max_disp bins and fit 8 bits) - every other range raises ValueError.
"""
from __future__ import annotations

import numpy as np

KB = 8                                     # bits of k below S in a packed key: D <= 256
_NONE = np.iinfo(np.int64).max


def check_range(dmin, D, max_disp):
    if not (dmin >= 0 and D >= 1 and dmin + D <= max_disp <= 256):
        raise ValueError(f"range (min {dmin}, {D} disparities) is not inside [0, max_disp {max_disp}), max_disp <= 256")


def maps(S, dmin=0, max_disp=None):
    """S [H][W][D] -> (lmap, rmap) uint8 [H][W]; max_disp: D + dmin unless given."""
    S = np.asarray(S)
    H, W, D = S.shape
    check_range(dmin, D, dmin + D if max_disp is None else max_disp)
    S = S.astype(np.int64)
    lmap = (dmin + S.argmin(axis=2)).astype(np.uint8)              # (numpy: the first minimum = the lowest k)
    key = np.full((H, W), _NONE, np.int64)
    for k in range(D):
        s = dmin + k                                               # left column x = xr + s
        if s >= W:
            break
        key[:, :W - s] = np.minimum(key[:, :W - s], (S[:, s:, k] << KB) | k)
    rmap = np.where(key == _NONE, 0, dmin + (key & ((1 << KB) - 1))).astype(np.uint8)
    return lmap, rmap


def maps_brute(S, dmin=0):
    """The same by a loop over pixels and candidates, in the definition's words."""
    S = np.asarray(S)
    H, W, D = S.shape
    lmap = np.zeros((H, W), np.uint8)
    rmap = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            best = min(range(D), key=lambda k: (int(S[y, x, k]), k))
            lmap[y, x] = dmin + best
            cand = [(int(S[y, x + dmin + k, k]), k) for k in range(D) if x + dmin + k < W]
            rmap[y, x] = dmin + min(cand)[1] if cand else 0
    return lmap, rmap
