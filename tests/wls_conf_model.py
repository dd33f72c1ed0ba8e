"""The definition of the graded confidence of the WLS smoothing stage (psm_wls_filter with PSM_WLS_CONFIDENCE): the
weight a pixel of the int16 map starts the solve with, from the left-right consistency of the SGM stage's summed costs S and from
the variance of the map around the pixel.  It follows no library's convention (cv::ximgproc::DisparityWLSFilter's confidence is its
model, not its definition); this numpy model is the definition and the device equals it in every bit.  All integer (int64
throughout) up to the start of the solve.

  right16(S, dmin)   the right view's sub-pixel map in 16ths from the same S [H][W][D]: for the right pixel (y, xr) the smallest
                     (S[y][xr + dmin + k][k], k) over the k in [0, D) with 0 <= xr + dmin + k < W, the lowest k on ties -
                     sgm_maps_model.maps' right search for every range the SGM stage takes (dmin in [-1024, 1024], D <= 1024).
                     With xl = xr + dmin + k and S0 that minimum: inner = 0 < k < D - 1 and xl - 1 >= 0 and xl + 1 < W;
                     Sm = S[y][xl - 1][k - 1], Sp = S[y][xl + 1][k + 1] (the neighbours on the same diagonal: the candidates
                     k - 1 and k + 1 of the same right pixel); den = max(Sm + Sp - 2 S0, 1), sub = ((Sm - Sp) 16 + den) // (2 den),
                     floor division (sgm_model.select's expressions).  Value (dmin + k) 16 + (inner ? sub : 0); a column without
                     a candidate gets rinv = (dmin - 1) 16.
  lr_term(v, inv, r16, rinv, thresh)   per left pixel: 0 where v == inv; else xq = x - ((v + 8) >> 4) (arithmetic shift); 0 if xq
                     is outside [0, W) or r16[y][xq] == rinv; else diff = |v - r16[y][xq]| and 255 - min((diff 255) // thresh, 255).
  var_term(v, inv, radius, shift)      over the (2 radius + 1)^2 window, pixels outside the image and invalid ones contributing
                     nothing: n the count, s the sum of v, ss the sum of v^2; t = (255 (n ss - s^2)) // (n^2 << shift); the term is
                     255 - min(t, 255) where the centre is valid, 0 elsewhere.  shift 8: one step of the term per square pixel of
                     disparity variance.  The largest intermediate is below 2^51 (81 taps, |v| <= 2^15).
  confidence         conf = (c_var c_lr + 127) // 255, a term that is switched off counting as 255, an invalid pixel 0: bytes.
  start              den = (float)conf, num = (float)conf * (float)v: one fp32 multiply, exact (8 bits times 16).  Everything
                     behind the start is wls_model unchanged.

Every function has a second statement (*_brute): loops over pixels in the words above.
"""
import numpy as np

import wls_model as W

LR, VAR = 1, 2
DEFAULTS = {"terms": LR | VAR, "lr_thresh": 24, "radius": 2, "var_shift": 8}
I = np.int64
F = np.float32
_NONE = np.iinfo(np.int64).max


def check_params(terms, lr_thresh, radius, var_shift):
    if terms not in (1, 2, 3) or not 1 <= lr_thresh <= 32767 or not 1 <= radius <= 4 or not 0 <= var_shift <= 16:
        raise ValueError(f"terms {terms} in {{1, 2, 3}}, lr_thresh {lr_thresh} in [1, 32767], radius {radius} in [1, 4], var_shift {var_shift} in [0, 16]")


def rinv_of(dmin):
    return (dmin - 1) * 16


def right16(S, dmin=0):
    """S [H][W][D] -> r16 int16 [H][W]"""
    S = np.asarray(S).astype(I)
    H, Wd, D = S.shape
    if not (-1024 <= dmin <= 1024 and 1 <= D <= 1024):
        raise ValueError(f"range (min {dmin}, {D} disparities)")
    key = np.full((H, Wd), _NONE, I)
    for k in range(D):
        lo, hi = max(0, -(dmin + k)), min(Wd, Wd - (dmin + k))       # the xr with 0 <= xr + dmin + k < W
        if lo < hi:
            key[:, lo:hi] = np.minimum(key[:, lo:hi], (S[:, lo + dmin + k:hi + dmin + k, k] << 10) | k)
    none = key == _NONE
    k = np.where(none, 0, key & 1023)
    S0 = np.where(none, 0, key >> 10)
    xl = np.arange(Wd)[None, :] + dmin + k
    inner = ~none & (k > 0) & (k < D - 1) & (xl - 1 >= 0) & (xl + 1 < Wd)
    rows = np.arange(H)[:, None]
    Sm = S[rows, np.clip(xl - 1, 0, Wd - 1), np.clip(k - 1, 0, D - 1)]
    Sp = S[rows, np.clip(xl + 1, 0, Wd - 1), np.clip(k + 1, 0, D - 1)]
    den = np.maximum(Sm + Sp - 2 * S0, 1)
    sub = ((Sm - Sp) * 16 + den) // (2 * den)
    out = (dmin + k) * 16 + np.where(inner, sub, 0)
    return np.where(none, rinv_of(dmin), out).astype(np.int16)


def right16_brute(S, dmin=0):
    S = np.asarray(S)
    H, Wd, D = S.shape
    out = np.zeros((H, Wd), np.int16)
    for y in range(H):
        for xr in range(Wd):
            cand = [(int(S[y, xr + dmin + k, k]), k) for k in range(D) if 0 <= xr + dmin + k < Wd]
            if not cand:
                out[y, xr] = rinv_of(dmin)
                continue
            S0, k = min(cand)
            xl = xr + dmin + k
            val = (dmin + k) * 16
            if 0 < k < D - 1 and xl - 1 >= 0 and xl + 1 < Wd:
                Sm, Sp = int(S[y, xl - 1, k - 1]), int(S[y, xl + 1, k + 1])
                den = max(Sm + Sp - 2 * S0, 1)
                val += ((Sm - Sp) * 16 + den) // (2 * den)
            out[y, xr] = val
    return out


def lr_term(v, inv, r16, rinv, thresh):
    """-> uint8 [H][W]"""
    v, r16 = np.asarray(v).astype(I), np.asarray(r16).astype(I)
    H, Wd = v.shape
    xq = np.arange(Wd)[None, :] - ((v + 8) >> 4)
    r = r16[np.arange(H)[:, None], np.clip(xq, 0, Wd - 1)]
    ok = (v != inv) & (xq >= 0) & (xq < Wd) & (r != rinv)
    term = 255 - np.minimum((np.abs(v - r) * 255) // thresh, 255)
    return np.where(ok, term, 0).astype(np.uint8)


def lr_term_brute(v, inv, r16, rinv, thresh):
    H, Wd = np.asarray(v).shape
    out = np.zeros((H, Wd), np.uint8)
    for y in range(H):
        for x in range(Wd):
            p = int(v[y][x])
            if p == inv:
                continue
            xq = x - ((p + 8) >> 4)
            if not 0 <= xq < Wd or int(r16[y][xq]) == rinv:
                continue
            out[y, x] = 255 - min((abs(p - int(r16[y][xq])) * 255) // thresh, 255)
    return out


def var_term(v, inv, radius, shift):
    """-> uint8 [H][W]"""
    v = np.asarray(v).astype(I)
    H, Wd = v.shape
    valid = v != inv
    r = radius
    pad = lambda a: np.pad(a, r)
    pn, ps, pss = pad(valid.astype(I)), pad(np.where(valid, v, 0)), pad(np.where(valid, v * v, 0))
    n, s, ss = np.zeros((H, Wd), I), np.zeros((H, Wd), I), np.zeros((H, Wd), I)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            n += pn[dy:dy + H, dx:dx + Wd]
            s += ps[dy:dy + H, dx:dx + Wd]
            ss += pss[dy:dy + H, dx:dx + Wd]
    t = (255 * (n * ss - s * s)) // (np.maximum(n, 1) ** 2 << shift)
    return np.where(valid, 255 - np.minimum(t, 255), 0).astype(np.uint8)


def var_term_brute(v, inv, radius, shift):
    H, Wd = np.asarray(v).shape
    out = np.zeros((H, Wd), np.uint8)
    for y in range(H):
        for x in range(Wd):
            if int(v[y][x]) == inv:
                continue
            win = [int(v[yy][xx]) for yy in range(y - radius, y + radius + 1) for xx in range(x - radius, x + radius + 1)
                   if 0 <= yy < H and 0 <= xx < Wd and int(v[yy][xx]) != inv]
            n, s, ss = len(win), sum(win), sum(p * p for p in win)
            out[y, x] = 255 - min((255 * (n * ss - s * s)) // (n * n << shift), 255)
    return out


def combine(v, inv, c_var=None, c_lr=None):
    """conf = (c_var c_lr + 127) // 255; a term that is None counts as 255; invalid pixels 0.  -> uint8 [H][W]"""
    v = np.asarray(v)
    a = np.full(v.shape, 255, I) if c_var is None else np.asarray(c_var).astype(I)
    b = np.full(v.shape, 255, I) if c_lr is None else np.asarray(c_lr).astype(I)
    return np.where(v != inv, (a * b + 127) // 255, 0).astype(np.uint8)


def combine_brute(v, inv, c_var=None, c_lr=None):
    H, Wd = np.asarray(v).shape
    out = np.zeros((H, Wd), np.uint8)
    for y in range(H):
        for x in range(Wd):
            if int(v[y][x]) != inv:
                a = 255 if c_var is None else int(c_var[y][x])
                b = 255 if c_lr is None else int(c_lr[y][x])
                out[y, x] = (a * b + 127) // 255
    return out


def confidence(v, inv, S=None, dmin=0, terms=DEFAULTS["terms"], lr_thresh=DEFAULTS["lr_thresh"], radius=DEFAULTS["radius"],
               var_shift=DEFAULTS["var_shift"]):
    """-> (conf uint8 [H][W], r16 int16 [H][W] or None without the L-R term).  S, dmin: the SGM stage's, of the range v belongs to."""
    check_params(terms, lr_thresh, radius, var_shift)
    r16 = right16(S, dmin) if terms & LR else None
    c_lr = lr_term(v, inv, r16, rinv_of(dmin), lr_thresh) if terms & LR else None
    c_var = var_term(v, inv, radius, var_shift) if terms & VAR else None
    return combine(v, inv, c_var, c_lr), r16


def start(v, conf):
    """-> planes [2, H, W] float32: num = (float)conf * (float)v, den = (float)conf"""
    c = np.asarray(conf, np.uint8).astype(F)
    return np.stack([c * np.asarray(v, np.int16).astype(F), c])


def wls(v, inv, guide, S=None, dmin=0, lam=W.DEFAULTS["lam"], sigma=W.DEFAULTS["sigma"], iterations=W.DEFAULTS["iterations"], **conf):
    """The flagged filter.  -> wls_model.wls's dict plus conf uint8, right16 int16 (None without the L-R term), and num0, den0: the start."""
    c, r16 = confidence(v, inv, S, dmin, **conf)
    pl = start(v, c)
    kh, kv = W.links(guide)
    tab = W.table(sigma)
    num0, den0 = pl[0].copy(), pl[1].copy()
    for lam_t in W.lambdas(lam, iterations):
        pl = W.solve_lines(pl, lam_t * tab[kh[:, :-1]])
        pl = W.solve_lines(pl.transpose(0, 2, 1), lam_t * tab[kv[:-1, :].T]).transpose(0, 2, 1)
    num, den = np.ascontiguousarray(pl)
    disp, q = W.finish(num, den, inv)
    return {"disp": disp, "q": q, "num": num, "den": den, "tab": tab, "conf": c, "right16": r16, "num0": num0, "den0": den0}
