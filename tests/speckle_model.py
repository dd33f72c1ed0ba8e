"""numpy model of the speckle filter of the semi-global matching stage (psm_sgm_set_speckle, psm_sgm_filter_speckles) - the
DEFINITION the device is held to, 0 differing elements.

cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on a CV_16SC1 map, as StereoSGBM runs it on its final map when
speckleWindowSize > 0: filterSpeckles(disp, (minDisparity - 1) * 16, speckleWindowSize, 16 * speckleRange); the reference's
setupOpenCVSGBM (src/StereoMatch.cpp:639-660) gives (-16, 100, 512).  In graph terms:

  vertices   the pixels with img != newVal
  edges      4-neighbours p, q, both vertices, |img[p] - img[q]| <= maxDiff (the difference in 64 bits here: nothing wraps)
  result     every pixel of a connected component of AT MOST maxSpeckleSize pixels becomes newVal, every other pixel is unchanged

OpenCV does it by an in-place flood fill in raster order; the edge relation is symmetric and a pixel rewritten to newVal already
carries a label, so its regions are these components whatever the order (tests/test_speckle_model.py holds this model to a scalar
restatement of that walk).
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

SGBM_NEW_VAL = -16


def components(disp, new_val, max_diff):
    """-> (labels int64 [H][W], -1 for new_val pixels, else 0 .. n-1; n)."""
    disp = np.asarray(disp)
    assert disp.ndim == 2 and disp.dtype == np.int16
    H, W = disp.shape
    v = disp.astype(np.int64)
    vert = v != int(new_val)
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    eh = vert[:, 1:] & vert[:, :-1] & (np.abs(v[:, 1:] - v[:, :-1]) <= int(max_diff))
    ev = vert[1:, :] & vert[:-1, :] & (np.abs(v[1:, :] - v[:-1, :]) <= int(max_diff))
    src = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    dst = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(H * W, H * W))
    _, lab = connected_components(g, directed=False)           # every pixel, isolated ones and new_val pixels included
    lab = lab.reshape(H, W).astype(np.int64)
    lab[~vert] = -1
    used = np.unique(lab[vert])
    lab[vert] = np.searchsorted(used, lab[vert])
    return lab, int(used.size)


def filter_speckles(disp, new_val, max_size, max_diff):
    """-> (filtered int16 [H][W], sizes int32 [H][W]: the size of every pixel's component, 0 for new_val pixels)."""
    assert -32768 <= int(new_val) <= 32767 and int(max_size) >= 0 and int(max_diff) >= 0
    lab, n = components(disp, new_val, max_diff)
    vert = lab >= 0
    sizes = np.zeros(lab.shape, np.int32)
    sizes[vert] = np.bincount(lab[vert], minlength=n)[lab[vert]]
    out = np.array(disp, dtype=np.int16, copy=True)
    out[vert & (sizes <= int(max_size))] = new_val
    return out, sizes


def sgbm_speckle(disp, speckle_window_size, speckle_range):
    """What StereoSGBM does to its map: nothing for a window of 0, else filterSpeckles(disp, -16, window, 16 * range)."""
    if speckle_window_size <= 0:
        return np.array(disp, copy=True), None
    return filter_speckles(disp, SGBM_NEW_VAL, speckle_window_size, 16 * speckle_range)
