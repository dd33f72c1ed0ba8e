"""The definition of the WLS smoothing stage (psm_wls_filter): the confidence-weighted, edge-aware global smoothing
of an int16 disparity map in 16ths by Min et al.'s Fast Global Smoother - separable tridiagonal solves along rows and columns,
guided by the left image - as users of cv::ximgproc::DisparityWLSFilter know it.  It follows no library's convention; this numpy
model is the definition and the device equals it in every bit.

Inputs: the map v [H, W] int16 with its invalid value inv; the guide g [H, W, ch] of bytes (depth_model.quantise of the left
image); lambda > 0, sigma > 0 (floats: the model rounds them to fp32 first, as the C ABI receives them), iterations T in 1..4.
    kh[y][x] = max over channels |g[y][x] - g[y][x+1]|  (x < W-1),   kv[y][x] the same between rows y and y+1;  both in 0..255
    tab[k]   = (float)exp(-(double)k / (double)sigma),  k = 0..255   (the C library's exp: math.exp is the same function)
    lam_t    = (float)((1.5 * (double)lambda * (double)4^(T-1-t)) / (double)(4^T - 1)),  t = 0..T-1
    den = valid ? 1.0f : 0.0f,   num = valid ? (float)v : 0.0f
For t = 0..T-1, first every row, then every column, as one line of N pixels with link indices k[0..N-2].  All fp32, every
operation rounded on its own (no FMA), 1.0f / m a correctly rounded division, subnormals kept; N = 1 is the identity:
    lw[n] = lam_t * tab[k[n]]                 a[n] = n > 0   ? -lw[n-1] : 0
                                              c[n] = n < N-1 ? -lw[n]   : 0
    b[n] = (1 - a[n]) - c[n]
    m = n ? b[n] - cp[n-1]*a[n] : b[0];       r = 1.0f / m;      cp[n] = c[n] * r
    np[n] = (num[n] - np[n-1]*a[n]) * r       (n = 0: num[0] * r)        dp likewise from den
    back:  u[N-1] = np[N-1];  u[n] = np[n] - cp[n]*u[n+1]                 likewise for den
num and den are replaced by their u.  End: q = num / den (one correctly rounded division); a pixel is good if den >= 2^-64 and
q is finite; a good pixel gets min(max(rintf(q), inv + 1), 32767), every other pixel inv; the float plane holds q for good pixels
and the stored pattern VOID_BITS elsewhere.
"""
import math

import numpy as np

VOID_BITS = 0x7FC00000
DEN_MIN = np.float32(2.0 ** -64)
DEFAULTS = {"lam": 8000.0, "sigma": 1.5, "iterations": 3}
WLS_SGM, WLS_GIF = 0, 1
F = np.float32


def table(sigma):
    """tab[0..255] float32"""
    s = float(F(sigma))
    return np.array([math.exp(-float(k) / s) for k in range(256)], np.float64).astype(F)


def lambdas(lam, T):
    """lam_t, t = 0..T-1, float32"""
    lam = float(F(lam))
    return [F((1.5 * lam * float(4 ** (T - 1 - t))) / float(4 ** T - 1)) for t in range(T)]


def links(guide):
    """-> (kh [H, W], kv [H, W]) uint8; the last column of kh and the last row of kv are 0 and never read"""
    g = np.asarray(guide, np.uint8)
    g = (g[..., None] if g.ndim == 2 else g).astype(np.int16)
    kh = np.zeros(g.shape[:2], np.uint8)
    kv = np.zeros(g.shape[:2], np.uint8)
    kh[:, :-1] = np.abs(g[:, :-1] - g[:, 1:]).max(axis=-1)
    kv[:-1, :] = np.abs(g[:-1, :] - g[1:, :]).max(axis=-1)
    return kh, kv


def solve_lines(x, lw, dtype=F):
    """One pass over the lines x [L, N] (several planes: [P, L, N]) with link weights lw [L, N-1] = lam_t * tab[k], already of
    `dtype`: the Thomas recurrence above, vectorised over the lines, serial along them.  dtype float64: the same recurrence in
    doubles (tests compare it with a dense solve)."""
    x = np.asarray(x, dtype)
    planes = x if x.ndim == 3 else x[None]
    P, L, N = planes.shape
    one, zero = dtype(1.0), dtype(0.0)
    cp = np.zeros((L, N), dtype)
    fw = np.zeros((P, L, N), dtype)
    with np.errstate(under="ignore"):
        for n in range(N):
            a = -lw[:, n - 1] if n > 0 else np.full(L, zero, dtype)
            c = -lw[:, n] if n < N - 1 else np.full(L, zero, dtype)
            b = (one - a) - c
            m = b - cp[:, n - 1] * a if n > 0 else b
            r = one / m
            cp[:, n] = c * r
            fw[:, :, n] = (planes[:, :, n] - fw[:, :, n - 1] * a) * r if n > 0 else planes[:, :, 0] * r
        u = np.empty_like(fw)
        u[:, :, N - 1] = fw[:, :, N - 1]
        for n in range(N - 2, -1, -1):
            u[:, :, n] = fw[:, :, n] - cp[:, n] * u[:, :, n + 1]
    return u if x.ndim == 3 else u[0]


def start(v, inv):
    """-> planes [2, H, W] float32: num, den"""
    v = np.asarray(v, np.int16)
    valid = v != inv
    return np.stack([np.where(valid, v.astype(F), F(0.0)), valid.astype(F)])


def smooth(v, inv, guide, lam=DEFAULTS["lam"], sigma=DEFAULTS["sigma"], iterations=DEFAULTS["iterations"], dtype=F):
    """The iterations: -> planes [2, H, W] (num, den) of `dtype`."""
    kh, kv = links(guide)
    tab = table(sigma).astype(dtype)
    pl = start(v, inv).astype(dtype)
    for lam_t in lambdas(lam, iterations):
        lam_t = dtype(lam_t)
        pl = solve_lines(pl, lam_t * tab[kh[:, :-1]], dtype)                                      # every row
        pl = solve_lines(pl.transpose(0, 2, 1), lam_t * tab[kv[:-1, :].T], dtype).transpose(0, 2, 1)   # every column
    return np.ascontiguousarray(pl)


def finish(num, den, inv):
    """-> (disp int16 [H, W], q float32 [H, W] with VOID_BITS in the void pixels)"""
    num, den = np.asarray(num, F), np.asarray(den, F)
    with np.errstate(all="ignore"):
        q = num / den
        good = (den >= DEN_MIN) & np.isfinite(q)
        r = np.minimum(np.maximum(np.rint(q), F(inv + 1)), F(32767.0))
    disp = np.where(good, np.where(good, r, F(0.0)).astype(np.int32), inv).astype(np.int16)
    bits = q.view(np.uint32).copy()
    bits[~good] = VOID_BITS
    return disp, bits.view(F)


def wls(v, inv, guide, lam=DEFAULTS["lam"], sigma=DEFAULTS["sigma"], iterations=DEFAULTS["iterations"]):
    """-> dict(disp int16, q float32, num float32, den float32, tab float32 [256])"""
    num, den = smooth(v, inv, guide, lam, sigma, iterations)
    disp, q = finish(num, den, inv)
    return {"disp": disp, "q": q, "num": num, "den": den, "tab": table(sigma)}


def gif_source(lmap, lvalid=None):
    """PSM_WLS_GIF: v = byte * 16, inv = -16; missing only under PSM_WLS_USE_MASK (lvalid given): validity byte 0.  -> (v, inv)"""
    v = np.asarray(lmap, np.uint8).astype(np.int16) * 16
    if lvalid is not None:
        v[np.asarray(lvalid) == 0] = -16
    return v, -16


def rounded_u8(d16):
    """the rounded 8-bit reading of a filtered map: min((max(v, 0) + 8) >> 4, 255)"""
    return np.minimum((np.maximum(np.asarray(d16, np.int32), 0) + 8) >> 4, 255).astype(np.uint8)
