"""numpy model of psm_gray_compute - the DEFINITION the device is held to, 0 differing bits in planes, volumes and maps.

The guided-filter path over a one-channel pair: the one-channel reading of GuidedFilter_cv (src/CVF.cpp:72-165, the primary oracle)
in the structure of FastGuidedFilterMono (src/fastguidedfilter.cpp:89-119), over costs that are myCostGrd (src/CVC.cpp:18-39) with
the colour sum over one channel.  fp32 throughout, every operation rounded on its own (numpy float32 arrays: no FMA), IEEE
division, subnormals kept.  `box` is cv::boxFilter(Size(8,8)) as this project fixes it - oracle.box8 (psmo_box8, tree order); the
oracle is imported as a checker's primitive only, the gradient and the costs are formed here (psmo_cvc_preprocess is 3-channel).

Per side, I the side's own plane and O the other one:

  input     a uint8 plane is converted as psm_upload_pair converts PSM_IMG_U8 (oracle.u8_to_f32: (float)u8 * (1/255.0f)); a
            float32 plane is used as it is
  gradient  G[y][x] = I[y][r101(x+1)] - I[y][r101(x-1)]                                  (0 at both row ends)
  cost      interior  c = 0.9f |I - O'| + (1.0f - 0.9f) |G - G_O'|
            border    c = 0.9f (float)fabs((double)I - 1.0) + (1.0f - 0.9f) (float)fabs((double)G - 1.0)
            left volume:  O' at x - d, border x < d;  right volume: O' at x + d of the LEFT image, border x >= W - d
  guidance  mI = box(I); var = box(I I) - mI mI; inv = 1.0f / (var + 1e-4f)              (independent of d; a reciprocal once per
            pixel, then a multiply - the 1 x 1 case of DET = 1 / DET, src/CVF.cpp:120-132)
  slice p   mp = box(p); mIp = box(I p); cov = mIp - mI mp; a = inv cov; b = mp - a mI; q = box(b) + box(a) I
  select    d = 1 .. D - 1 ascending, strict <, default 0 (oracle.wta): slice 0 is never a candidate
  maps      left from the left volume, right from the right volume, uint8

Every function takes `ar`, the arithmetic: F32 (the definition) or F64 (the same formulas in float64 with a float64 box over the
same taps - what tests/test_gray_model.py measures the definition's rounding against).
"""
from __future__ import annotations

import numpy as np

from oracle import psm_oracle_py as O


def r101(k, n):
    k = np.abs(k)
    return np.where(k >= n, 2 * (n - 1) - k, k)


def box64(p):
    """The 64 taps of psmo_box8 - rows r101(y-4+j), columns r101(x-4+i), i, j = 0..7 - summed in float64, times 1/64."""
    p = np.asarray(p, np.float64)
    H, W = p.shape
    hs = sum(p[:, r101(np.arange(W) - 4 + i, W)] for i in range(8))
    return sum(hs[r101(np.arange(H) - 4 + j, H), :] for j in range(8)) * (1.0 / 64)


class Arith:
    def __init__(self, dtype, box):
        self.t, self.box = dtype, box
        # the constants are the float32 values in either arithmetic
        self.alpha = dtype(np.float32(0.9))
        self.beta = dtype(np.float32(1.0) - np.float32(0.9))
        self.eps = dtype(np.float32(1e-4))
        self.one = dtype(1.0)


F32 = Arith(np.float32, O.box8)
F64 = Arith(np.float64, box64)


def to_f32(plane):
    plane = np.asarray(plane)
    if plane.dtype == np.uint8:
        return O.u8_to_f32(plane)
    if plane.dtype != np.float32:
        raise TypeError("a plane is uint8 or float32")
    return np.ascontiguousarray(plane)


def gradient(I):
    W = I.shape[1]
    x = np.arange(W)
    return I[:, r101(x + 1, W)] - I[:, r101(x - 1, W)]


def border_cost(I, G, ar=F32):
    """myCostGrd(lC, lG): BC_32F is the double 1.0 - differences in double, narrowed, then the fp32 weighting."""
    cI = np.abs(I.astype(np.float64) - 1.0).astype(ar.t)
    cG = np.abs(G.astype(np.float64) - 1.0).astype(ar.t)
    return ar.alpha * cI + ar.beta * cG


def cost_slice(I, G, Oth, GO, d, right, ar=F32):
    """Slice d of the side whose own plane is I: left volume (right False; Oth the right plane) or right volume (Oth the left)."""
    H, W = I.shape
    c = border_cost(I, G, ar)
    if d >= W:
        return c
    if not right:
        own, oth = slice(d, W), slice(0, W - d)
    else:
        own, oth = slice(0, W - d), slice(d, W)
    c[:, own] = ar.alpha * np.abs(I[:, own] - Oth[:, oth]) + ar.beta * np.abs(G[:, own] - GO[:, oth])
    return c


def guidance(I, ar=F32):
    mI = ar.box(I)
    var = ar.box(I * I) - mI * mI
    inv = ar.one / (var + ar.eps)
    return mI, inv


def filter_slice(I, mI, inv, p, ar=F32):
    mp = ar.box(p)
    mIp = ar.box(I * p)
    cov = mIp - mI * mp
    a = inv * cov
    b = mp - a * mI
    q = ar.box(b) + ar.box(a) * I
    return q, a, b


class Side:
    """One side of a pair: its planes and guidance; slice(d) is the filtered slice d."""

    def __init__(self, l, r, side, ar=F32):
        self.ar = ar
        pl = [to_f32(l).astype(ar.t), to_f32(r).astype(ar.t)]
        self.right = bool(side)
        self.I, self.O = pl[side], pl[side ^ 1]
        self.G, self.GO = gradient(self.I), gradient(self.O)
        self.mI, self.inv = guidance(self.I, ar)

    def planes(self):
        """What psm_gray_guidance returns: I, G, mI, inv."""
        return np.stack([self.I, self.G, self.mI, self.inv])

    def cost(self, d):
        return cost_slice(self.I, self.G, self.O, self.GO, d, self.right, self.ar)

    def slice(self, d, want_ab=False):
        q, a, b = filter_slice(self.I, self.mI, self.inv, self.cost(d), self.ar)
        return (q, a, b) if want_ab else q


def volume(l, r, side, d0, d1, ar=F32, want_ab=False):
    """The slices [d0, d1) of `side` as psm_gray_volume returns them: q [d1-d0][H][W] (and ab [d1-d0][2][H][W])."""
    s = Side(l, r, side, ar)
    out = [s.slice(d, True) for d in range(d0, d1)]
    q = np.stack([o[0] for o in out])
    if not want_ab:
        return q
    return q, np.stack([np.stack([o[1], o[2]]) for o in out])


def wta_running(slices, shape):
    """oracle.wta over slices d = 1, 2, ... given one by one: strict <, default 0 - no volume is held."""
    best = np.full(shape, np.inf, np.float32)
    disp = np.zeros(shape, np.uint8)
    for d, q in slices:
        m = q < best
        best[m] = q[m]
        disp[m] = d
    return disp


def maps(l, r, D):
    """(lmap, rmap) of psm_gray_compute."""
    out = []
    for side in (0, 1):
        s = Side(l, r, side)
        out.append(wta_running(((d, s.slice(d)) for d in range(1, D)), s.I.shape))
    return out[0], out[1]


def maps_unaggregated(l, r, D):
    """The same selection over the unfiltered costs (what the aggregation has to beat)."""
    out = []
    for side in (0, 1):
        s = Side(l, r, side)
        out.append(wta_running(((d, s.cost(d)) for d in range(1, D)), s.I.shape))
    return out[0], out[1]
