"""numpy model of ONE evaluation of the weighted median (src/PP.cpp:145-247 wgtMedian, oracle/psm_oracle.c psmo_wgt_median) on a
frozen map, with the two things a device form may get wrong made switchable: the ORDER of the 361 fp32 additions into disHist /
sumWgt, and what happens to DENORMAL weights and sums.  Vectorised over pixels, sequential over the taps in float32.  It serves
tests/wmf_inputs.py (which keeps only inputs the switches change the result of) and tests/test_wmf_inputs.py; no GPU, numpy only.

Also the fully synchronous (Jacobi) iteration of the in-place recursion: how many sweeps a device that sees NO change of the
current sweep would need - the chain length of an input."""
from __future__ import annotations

import math

import numpy as np

R = 9                                   # MED_SZ / 2
TAPS = (2 * R + 1) ** 2                 # 361
ORDERS = ("raster", "rows_reversed", "cols_reversed", "pairwise")
F32_MIN = np.float32(np.finfo(np.float32).tiny)          # the smallest normal float

_WY, _WX = (a.reshape(-1) for a in np.mgrid[-R:R + 1, -R:R + 1])          # tap t = (wy + 9) * 19 + (wx + 9): raster order


def tap_order(order):
    """-> the 361 tap indices in the order their weights are added"""
    t = np.arange(TAPS).reshape(2 * R + 1, 2 * R + 1)
    if order in ("raster", "pairwise"):
        return t.reshape(-1)
    if order == "rows_reversed":
        return t[::-1].reshape(-1)
    if order == "cols_reversed":
        return t[:, ::-1].reshape(-1)
    raise ValueError(order)


def _libm_exp(arg):
    """(float)exp(double) through the host libm (math.exp), as psmo_wm_weight forms it; numpy's own exp is another function."""
    u, inv = np.unique(arg, return_inverse=True)
    e = np.array([math.exp(v) for v in u.tolist()], np.float64)
    return e[inv.reshape(arg.shape)].astype(np.float32)


def colour_weights(p3, q3, wy, wx, right):
    """psmo_wm_weight for arrays: p3, q3 [..., 3] float32 colours, wy, wx ints (broadcast against p3[..., 0])."""
    p3, q3 = np.asarray(p3, np.float32), np.asarray(q3, np.float32)
    dis = (np.asarray(wx) * np.asarray(wx) + np.asarray(wy) * np.asarray(wy)).astype(np.float32)
    d = p3 - q3
    clr = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if right:
        dis, clr = np.sqrt(dis), np.sqrt(clr)
    a = (-dis / np.float32(81)).astype(np.float32)
    arg = np.broadcast_arrays(a.astype(np.float64) - clr.astype(np.float64) / (0.1 * 0.1))[0]
    return _libm_exp(np.ascontiguousarray(arg))


def window(img_f32, pixels, right):
    """-> (flat indices of the taps [361, n], their weights [361, n] float32) of the listed pixels [n, 2] = (y, x)"""
    img = np.asarray(img_f32, np.float32)
    H, W, _ = img.shape
    pix = np.asarray(pixels, np.int64).reshape(-1, 2)
    qy = (pix[None, :, 0] + _WY[:, None] + H) % H
    qx = (pix[None, :, 1] + _WX[:, None] + W) % W
    wts = colour_weights(img[pix[:, 0], pix[:, 1]][None], img[qy, qx], _WY[:, None], _WX[:, None], right)
    return qy * W + qx, wts


def _ftz(a):
    return np.where(np.abs(a) < F32_MIN, np.float32(0), a).astype(np.float32)


def _pairwise(c):
    """sum over axis 0 as a balanced tree of fp32 additions (neighbours first)"""
    n = 1 << (len(c) - 1).bit_length()
    if n != len(c):
        c = np.concatenate([c, np.zeros((n - len(c),) + c.shape[1:], np.float32)])
    while len(c) > 1:
        c = c[0::2] + c[1::2]
    return c[0]


def median_of(wts, deps, order="raster", flush=False):
    """The histogram, the total, half of it and the ascending scan with >= of n windows: wts [361, n] float32 and deps [361, n]
    (the map values at the taps, 0 = no vote) in raster tap order.  Only the bins that occur are kept (and bin 0, which decides
    a window without a vote): an empty bin adds +0 and cannot be the first to reach half.  -> [n] uint8"""
    wts = np.asarray(wts, np.float32)
    deps = np.asarray(deps)
    n = wts.shape[1]
    vals = np.unique(np.concatenate([[0], deps.reshape(-1)]))
    rank = np.searchsorted(vals, deps)
    w = np.where(deps != 0, wts, np.float32(0)).astype(np.float32)
    if flush:
        w = _ftz(w)
    ar = np.arange(n)
    if order == "pairwise":
        hist = np.empty((n, len(vals)), np.float32)
        step = max(1, (32 << 20) // (512 * len(vals)))
        for lo in range(0, n, step):
            m = min(step, n - lo)
            c = np.zeros((TAPS, m, len(vals)), np.float32)
            c[np.arange(TAPS)[:, None], np.arange(m)[None], rank[:, lo:lo + m]] = w[:, lo:lo + m]
            hist[lo:lo + m] = _pairwise(c)
        tot = _pairwise(w)
        if flush:
            hist, tot = _ftz(hist), _ftz(tot)
    else:
        hist = np.zeros((n, len(vals)), np.float32)
        tot = np.zeros(n, np.float32)
        for t in tap_order(order):
            hist[ar, rank[t]] += w[t]
            tot += w[t]
            if flush:
                hist[ar, rank[t]] = _ftz(hist[ar, rank[t]])
                tot = _ftz(tot)
    half = tot / np.float32(2)
    if flush:
        half = _ftz(half)
        acc = np.zeros_like(hist)
        run = np.zeros(n, np.float32)
        for k in range(len(vals)):
            run = _ftz(run + hist[:, k])
            acc[:, k] = run
    else:
        acc = np.cumsum(hist, axis=1, dtype=np.float32)
    hit = acc >= half[:, None]
    return np.where(hit.any(axis=1), vals[np.argmax(hit, axis=1)], 0).astype(np.uint8)


def evaluate(img_f32, dis, pixels, D, right, order="raster", flush=False):
    """The weighted median of the listed pixels [n, 2] = (y, x) on the FROZEN map dis (no pixel sees another's result).
    order: one of ORDERS; flush: denormal weights and sums become 0.  For "raster" without flush this is oracle.wgt_median
    wherever no other invalid pixel lies in a listed pixel's window."""
    dis = np.asarray(dis)
    assert int(dis.max()) < D
    q, wts = window(img_f32, pixels, right)
    return median_of(wts, dis.reshape(-1)[q], order, flush)


def jacobi_sweeps(img_f32, dis, valid, D, right, cap):
    """Fully synchronous sweeps of the in-place recursion: every invalid pixel is evaluated from the PREVIOUS iterate at the earlier
    pixels of its window and from the input at the later ones (and at itself).  -> (sweeps, map): the number of sweeps up to and
    including the first that changes nothing (the count psm_wgt_median_stats reports), and that fixed point - the in-place map.
    (-1, last iterate) if `cap` sweeps do not get there.  Only pixels with a change among their earlier taps are evaluated
    again, which is the same iteration."""
    dis = np.ascontiguousarray(dis, np.uint8)
    assert int(dis.max()) < D
    H, W = dis.shape
    pix = np.argwhere(np.asarray(valid) == 0)
    cur = dis.copy()
    if len(pix) == 0:
        return 1, cur
    q, wts = window(img_f32, pix, right)
    flat = pix[:, 0] * W + pix[:, 1]
    earlier = q < flat[None]
    inp = dis.reshape(-1)
    active = np.arange(len(pix))
    for sweep in range(1, cap + 1):
        deps = np.where(earlier[:, active], cur.reshape(-1)[q[:, active]], inp[q[:, active]])
        new = median_of(wts[:, active], deps)
        chg = new != cur.reshape(-1)[flat[active]]
        if not chg.any():
            return sweep, cur
        changed = np.zeros(H * W, bool)
        changed[flat[active][chg]] = True
        cur.reshape(-1)[flat[active][chg]] = new[chg]
        active = np.flatnonzero((changed[q] & earlier).any(axis=0))
        if len(active) == 0:
            return sweep + 1, cur                  # (nobody is left to look: the next sweep is empty and changes nothing)
    return -1, cur
