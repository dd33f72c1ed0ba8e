"""The definition of the score stage (psm_score): the display conversion of both algorithms and the error metric of
StereoMatch::compute (src/StereoMatch.cpp:181-185, 248-249, 275-309), stated pixel by pixel in integers and in single IEEE
operations - independently of primestereomatch_amd.harness, whose numpy tail it must reproduce (tests/test_score_model.py) and
which the device must equal in every element and counter (tests/test_gpu_score.py)."""
import numpy as np

GIF, SGM, SGM_INT = 0, 1, 2                      # PSM_SCORE_*
MASK_NONE, MASK_NONOCC, MASK_DISC = 0, 1, 2      # PSM_MASK_*
FLAT = 1                                         # PSM_SCORE_FLAT

INV255 = float(np.float32(1.0) / np.float32(255.0))      # eDispMap.mul(errMask, 1 / 255.f): a float factor, used in double


def _sat_u8(a):
    return np.minimum(np.maximum(a, 0), 255)


def display_u8(v, scale_factor):
    """convertTo(CV_8U, scale_factor) of an 8-bit map: min(v * scale_factor, 255)."""
    return np.minimum(np.asarray(v).astype(np.int64) * int(scale_factor), 255).astype(np.uint8)


def display_sgm(d16, scale_factor):
    """minMaxLoc; convertTo(CV_8U, 255 / (maxVal - minVal)); / 4; * scale_factor -> (display, min_val, max_val, flags).
    The factor is formed in double and used as a float; a 16-bit source is multiplied in fp32, rounded to nearest even and
    saturated (negative products: 0); Mat / 4 is convertTo(CV_8U, 0.25) - the same rounding.  No offset: minVal is not subtracted.
    A flat map (the reference divides by zero) is this model's own statement: alpha = 0, an all-zero display, FLAT."""
    d16 = np.asarray(d16)
    assert d16.dtype == np.int16
    mn, mx = int(d16.min()), int(d16.max())
    flat = mn == mx
    alpha = np.float32(0.0) if flat else np.float32(255.0 / (float(mx) - float(mn)))
    prod = d16.astype(np.float32) * alpha                                    # one fp32 multiply per pixel
    assert prod.dtype == np.float32
    m = _sat_u8(np.rint(prod)).astype(np.float32)
    q = _sat_u8(np.rint(m * np.float32(0.25))).astype(np.int64)
    return np.minimum(q * int(scale_factor), 255).astype(np.uint8), mn, mx, (FLAT if flat else 0)


def display_sgm_int(d16, scale_factor):
    """The integer disparity min(max(d16, 0) >> 4, 255), then as an 8-bit map."""
    v = np.minimum(np.maximum(np.asarray(d16).astype(np.int64), 0) >> 4, 255)
    return display_u8(v, scale_factor)


def mask_step(e, k):
    """e, k integer arrays in [0, 255] -> sat_u8(rne((double)(e * k) * (double)(1 / 255.f)))."""
    prod = (np.asarray(e).astype(np.int64) * np.asarray(k).astype(np.int64)).astype(np.float64) * INV255
    return _sat_u8(np.rint(prod)).astype(np.int64)


def metric(p, gt, mask, max_disp, error_threshold, mask_mode=MASK_NONOCC):
    """The error plane and counters of the 8-bit display map p -> (emap uint8, bad, err_sum, unit)."""
    p, gt = np.asarray(p), np.asarray(gt)
    assert p.dtype == np.uint8 and gt.dtype == np.uint8 and p.shape == gt.shape
    unit = 127 // int(max_disp)
    e = np.abs(p.astype(np.int64) - gt.astype(np.int64))
    x = np.arange(p.shape[1])[None, :]
    e = np.where(x <= max_disp, 0, e)
    e = np.where(e <= int(error_threshold) * unit, 0, e)
    if mask is not None and mask_mode != MASK_NONE:
        k = np.asarray(mask).astype(np.int64)
        if mask_mode == MASK_DISC:
            k = np.where(k > 254, k, 0)
        e = mask_step(e, k)
    return e.astype(np.uint8), int(np.count_nonzero(e)), int(e.sum()), unit


def figures(rec):
    """%BP and Avg Err from the record's integers, in double."""
    bp = 100.0 * rec["bad"] / rec["pixels"]
    avg = (rec["err_sum"] / rec["pixels"]) / rec["unit"] if rec["unit"] else 0.0
    return bp, avg


def score(source, data, gt, mask, max_disp, scale_factor=4, error_threshold=4, mask_mode=MASK_NONOCC):
    """psm_score.  data: the left 8-bit map, or (left, right) maps (GIF); the int16 map (SGM, SGM_INT); gt None: nothing is scored.
    -> dict: ldisp, rdisp (GIF with a right map, else None), emap, and the record's integers."""
    mn = mx = flags = 0
    rdisp = None
    if source == GIF:
        left, right = data if isinstance(data, tuple) else (data, None)
        ldisp = display_u8(left, scale_factor)
        rdisp = None if right is None else display_u8(right, scale_factor)
    elif source == SGM:
        ldisp, mn, mx, flags = display_sgm(data, scale_factor)
    else:
        ldisp = display_sgm_int(data, scale_factor)
    unit = 127 // int(max_disp)
    if gt is None:
        emap, bad, err_sum = np.zeros(ldisp.shape, np.uint8), 0, 0
    else:
        emap, bad, err_sum, unit = metric(ldisp, gt, mask, max_disp, error_threshold, mask_mode)
    rec = {"min_val": mn, "max_val": mx, "pixels": int(ldisp.size), "bad": bad, "err_sum": err_sum, "unit": unit, "flags": flags}
    rec["bp_percent"], rec["avg_err"] = figures(rec)
    return dict(rec, ldisp=ldisp, rdisp=rdisp, emap=emap)


RECORD_KEYS = ("min_val", "max_val", "pixels", "bad", "err_sum", "unit", "flags")
