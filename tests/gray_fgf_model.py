"""numpy model of psm_gray_compute_fgf - the DEFINITION the device is held to, 0 differing bits in planes, volumes and maps.

FastGuidedFilterMono (src/fastguidedfilter.cpp:89-119), the one-channel half of FastGuidedFilter(I, 8, 1e-4, s), over the costs
of tests/gray_model.py: the guided filter runs on planes subsampled by s, its box shrinks to k = 2 (8 / s) + 1 taps, and the two
smoothed model planes are upsampled bilinearly before the linear model is applied at full resolution.  fp32 throughout, every
operation rounded on its own, IEEE division, subnormals kept.  The three OpenCV primitives are restated here as
oracle/psm_oracle.c states them (nn_maps, blur_k, lin_maps and the loop behind them); tests/test_gray_fgf_model.py pins them to it.

Per side, with I, G, the costs and the selection exactly as tests/gray_model.py has them; s in {2, 4, 8}, R = 8 / s, k = 2 R + 1,
hs = H / s, ws = W / s:

  nn(p)     cv::resize(INTER_NN) to hs x ws: source index min(floor(x * (1 / ((double)ws / W))), W - 1), rows alike
  blur(p)   cv::blur(Size(k, k)): taps -R .. R with REFLECT_101, fp64 sums - x taps left to right, then y taps top to bottom -,
            (float)(sum * (1.0 / (k k)))
  up(m)     cv::resize(INTER_LINEAR) to H x W: f = (float)((d + 0.5) * ((double)ssize / dsize) - 0.5), sx = floor(f), f -= sx, both
            clamped (sx < 0: 0, f = 0; sx >= ssize - 1: ssize - 1, f = 0); a row pass m[sx] (1.f - fx) + m[sx1] fx, then a column pass
  guidance  Is = nn(I); mI = blur(Is); den = (blur(Is Is) - mI mI) + 1e-4f
  slice d   ps = nn(cost_d); mp = blur(ps); mIp = blur(Is ps); a = (mIp - mI mp) / den (the reference's own per-voxel quotient,
            src/fastguidedfilter.cpp:111); b = mp - a mI; q = up(blur(a)) I + up(blur(b))
  select    d = 1 .. D - 1 ascending, strict <, default 0

Every function takes `ar`, the arithmetic: F32 (the definition) or F64 (the same formulas in float64, the blur without its final
narrowing - what tests/test_gray_fgf_model.py measures the definition's rounding against).
"""
from __future__ import annotations

import numpy as np

import gray_model as M

RATES = (2, 4, 8)


class Arith:
    def __init__(self, dtype, base):
        self.t, self.base = dtype, base
        self.eps = dtype(np.float32(1e-4))
        self.one = dtype(1.0)


F32 = Arith(np.float32, M.F32)
F64 = Arith(np.float64, M.F64)


def accepted(W, H, s):
    """The sizes psm_gray_compute_fgf takes: both subsampled axes longer than the blur radius (one REFLECT_101 fold is exact)."""
    return s in RATES and W // s > 8 // s and H // s > 8 // s


def nn_index(ssize, s):
    """nn_maps of one axis: the source index of every one of the ssize // s samples."""
    dsize = ssize // s
    inv = 1.0 / (float(dsize) / ssize)
    return np.minimum(np.floor(np.arange(dsize) * inv).astype(np.int64), ssize - 1)


def nn(p, s):
    H, W = p.shape
    return np.ascontiguousarray(p[np.ix_(nn_index(H, s), nn_index(W, s))])


def blur(p, k, ar=F32):
    """blur_k: fp64 sums in tap order; F32 narrows the scaled sum to float."""
    h, w = p.shape
    R = k // 2
    p64 = np.asarray(p, np.float64)
    x, y = np.arange(w), np.arange(h)
    hsum = np.zeros((h, w), np.float64)
    for i in range(-R, R + 1):
        hsum = hsum + p64[:, M.r101(x + i, w)]
    acc = np.zeros((h, w), np.float64)
    for j in range(-R, R + 1):
        acc = acc + hsum[M.r101(y + j, h), :]
    return (acc * (1.0 / (k * k))).astype(ar.t)


def lin_index(ssize, dsize):
    """lin_maps of one axis: (sx, sx1, the float32 weight of the second tap)."""
    scale = float(ssize) / dsize
    f = ((np.arange(dsize) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(f).astype(np.int64)
    f = f - sx.astype(np.float32)
    lo, hi = sx < 0, sx >= ssize - 1
    f[lo | hi] = np.float32(0.0)
    sx[lo] = 0
    sx[hi] = ssize - 1
    return sx, np.minimum(sx + 1, ssize - 1), f


def up(m, H, W, ar=F32):
    hs, ws = m.shape
    sx, sx1, fx = lin_index(ws, W)
    sy, sy1, fy = lin_index(hs, H)
    fx, fy = fx.astype(ar.t)[None, :], fy.astype(ar.t)[:, None]
    rows = m[:, sx] * (ar.one - fx) + m[:, sx1] * fx
    return rows[sy, :] * (ar.one - fy) + rows[sy1, :] * fy


class Side:
    """One side of a pair at rate s: its planes and subsampled guidance; slice(d) is the filtered slice d."""

    def __init__(self, l, r, side, s, ar=F32):
        if s not in RATES:
            raise ValueError("the rate is 2, 4 or 8")
        self.ar, self.s, self.k = ar, s, 2 * (8 // s) + 1
        pl = [M.to_f32(l).astype(ar.t), M.to_f32(r).astype(ar.t)]
        self.right = bool(side)
        self.I, self.O = pl[side], pl[side ^ 1]
        self.G, self.GO = M.gradient(self.I), M.gradient(self.O)
        self.Is = nn(self.I, s)
        self.mI = blur(self.Is, self.k, ar)
        self.den = (blur(self.Is * self.Is, self.k, ar) - self.mI * self.mI) + ar.eps

    def planes(self):
        """What psm_gray_fgf_guidance returns: Is, mI, den."""
        return np.stack([self.Is, self.mI, self.den])

    def cost(self, d):
        return M.cost_slice(self.I, self.G, self.O, self.GO, d, self.right, self.ar.base)

    def filter(self, p, want_model=False):
        """A full-resolution plane p through the filter: q, and - want_model - the four subsampled planes a, b, blur(a), blur(b)."""
        ar, k = self.ar, self.k
        ps = nn(p, self.s)
        mp = blur(ps, k, ar)
        mIp = blur(self.Is * ps, k, ar)
        a = (mIp - self.mI * mp) / self.den
        b = mp - a * self.mI
        ma, mb = blur(a, k, ar), blur(b, k, ar)
        H, W = self.I.shape
        q = up(ma, H, W, ar) * self.I + up(mb, H, W, ar)
        return (q, np.stack([a, b, ma, mb])) if want_model else q

    def slice(self, d, want_model=False):
        return self.filter(self.cost(d), want_model)


def volume(l, r, side, s, d0, d1, ar=F32, want_model=False):
    """The slices [d0, d1) of `side` as psm_gray_fgf_volume returns them: q [d1-d0][H][W] (and model [d1-d0][4][hs][ws])."""
    sd = Side(l, r, side, s, ar)
    out = [sd.slice(d, True) for d in range(d0, d1)]
    q = np.stack([o[0] for o in out])
    return (q, np.stack([o[1] for o in out])) if want_model else q


def maps(l, r, D, s):
    """(lmap, rmap) of psm_gray_compute_fgf."""
    out = []
    for side in (0, 1):
        sd = Side(l, r, side, s)
        out.append(M.wta_running(((d, sd.slice(d)) for d in range(1, D)), sd.I.shape))
    return out[0], out[1]
