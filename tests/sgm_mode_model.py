"""numpy model of the SGM stage under StereoSGBM's modes (psm_sgm_set_mode, DispEst.SGBM_GPU(mode=...)) - the DEFINITION the device
is held to, 0 differing elements.  Steps 1-3 and 5-7 are sgm_model's (and sgm_bt_model's pixel cost), imported and untouched; only
the set of directions step 4 sums depends on the mode.  (dy, dx) is the step from the predecessor p-r to p.

    "sgbm" = 0   (0,1), (0,-1), (1,0), (1,1), (1,-1): OpenCV's single top-down pass plus the right-to-left row path of its selection
    "hh"   = 1   all eight: sgm_model.sgm itself
    "3way" = 2   (0,1), (0,-1), (1,0)
    "hh4"  = 3   (0,1), (0,-1), (1,0), (-1,0)

The values are OpenCV's enum.  Every path crosses the whole image (OpenCV's 3-way code restarts its paths in stripes cut by thread
count: not modelled).  Agreement with a live cv::StereoSGBM is unpinned in every mode."""
from __future__ import annotations

import numpy as np

import sgm_bt_model as B
import sgm_model as M

_D = M.DIRECTIONS
_BY_NAME = {"sgbm": (_D[0], _D[1], _D[2], _D[4], _D[5]), "hh": _D, "3way": _D[:3], "hh4": _D[:4]}
VALUES = {"sgbm": 0, "hh": 1, "3way": 2, "hh4": 3}
MODES = {**_BY_NAME, **{VALUES[k]: v for k, v in _BY_NAME.items()}}              # name or value -> direction tuple


def sgm(L, R, D, mode, pre_filter_cap=0, **params):
    """The whole stage in one mode.  -> the dict of sgm_model.sgm (plus "planes" when pre_filter_cap > 0)."""
    directions = MODES[mode]
    L, R = M._as3(L), M._as3(R)
    if L.shape != R.shape:
        raise ValueError("the two images differ in shape")
    if not 2 <= D <= 256:
        raise ValueError("2 <= D <= 256")
    bs, P1, P2, u, m = M.resolve_params(L.shape[2], **params)
    c = M.pixel_cost(L, R, D) if pre_filter_cap == 0 else B.pixel_cost_bt(L, R, D, pre_filter_cap)
    C = M.block_cost(c, bs)
    S, max_l = M.aggregate(C, P1, P2, directions=directions, want_max_l=True)
    best, minS, unique, d16 = M.select(S, u)
    disp2, valid = M.consistency(best, minS, unique, d16, m)
    disp = np.where(valid, d16, M.INVALID).astype(np.int16)
    out = {"C": C, "S": S, "best": best.astype(np.uint8), "unique": unique, "valid": valid, "d16": d16, "disp2": disp2,
           "disp": disp, "max_l": max_l, "params": (bs, P1, P2, u, m)}
    if pre_filter_cap:
        out["planes"] = (B.prefilter(L, pre_filter_cap), B.prefilter(R, pre_filter_cap))
    return out
