"""Adversarial pairs and their expected values for the one-channel guided-filter path (psm_gray_compute and psm_gray_compute_fgf,
single and batch; tests/test_gpu_gray_adversarial.py runs them on the device, tests/test_gray_inputs.py holds them to their own
conditions on the CPU).  Pure numpy on tests/gray_model.py and tests/gray_fgf_model.py, no GPU; every function is a deterministic
function of its arguments, every result is cached and read-only.

A case is (kind, s): s = 0 is the full-resolution form, s = 2, 4, 8 the Fast Guided Filter at that rate.  Its size is SIZES[kind][s].

Non-finite kinds - a seeded uniform [0, 1) float32 pair with special values planted in BOTH planes, on and away from the border:
  nan_pos     0x7FC00000, the quiet NaN with the sign bit clear
  nan_neg     0xFFC00000, the one x86 forms for inf - inf and 0 / 0: as a WTA key it sorts below every finite cost
  pinf, ninf  +inf, -inf
  overflow    +-3e19: finite, I I overflows.  The guidance of the own side is inf wherever a window holds such a pixel, so there
              a = 0 cov is NaN in every slice whose I c overflows too - all of them, but for the slice that moves an equal value of
              the other plane onto it (the `aligned` sites below: c is small there, a = 0, q finite)
  all         every value above together, one per site
  all_slices  both planes wholly NaN (the left 0xFFC00000, the right 0x7FC00000): no pixel of either side has a candidate, both
              maps are 0
  left_nan    the left plane alone wholly 0xFFC00000: the left map is 0; the right side keeps the candidates of its border columns
              (x >= W - d: the border cost is formed from the own plane alone), so its map is 0 on the left and not on the right
A special value in a side's own plane makes every slice NaN around it (two boxes wide); one in the other plane makes slice d NaN
around x +- d: pixels where some slices are NaN and others finite - the ones where a NaN key could win a selection it must lose.
The left plane's sites sit in the right part of the image and the right plane's in the left part, so that the slices carry the
other plane's values into the columns the own plane left alive.

  periodic    0 / 1, period 32 along x, rows inverted at random, the right plane the left one moved by 3: the slices 3, 35 (and 67
              at D = 70) are the same bits away from their borders, in different 32-slice chunks
  negative    test_gpu_gray.py's "float" (uniform +-1024) moved up by 2^22.  "float" itself does not qualify: its costs are some
              hundreds and a q below zero needs the linear model to overshoot by as much - the model shows none at s = 0, 2, 4 and
              63 of 1330 pixels at s = 8.  Moved by 2^22 the planes' mean is 7000 standard deviations: var = box(I I) - mI mI
              cancels to a few ulps of 1.8e13 of either sign, and the winning q is below zero in nearly every pixel, with about as
              many distinct values as pixels (the key flips the magnitude bits of a negative float).  Every plane stays finite.
  (A pair of -0.0f against +0.0f planes was tried and is not kept: the model's minima are +0 in every pixel it has one, on both
  sides and at every rate - the costs are |.| of a difference or the border cost 1 - so it would not put both zeros before the key.)
  clean       the uniform pair with nothing planted (the neighbours of a batch, the pair behind all_slices)
"""
from __future__ import annotations

import functools

import numpy as np

import gray_fgf_model as F
import gray_model as M

FORMS = (0, 2, 4, 8)
NAN_POS, NAN_NEG = 0x7FC00000, 0xFFC00000
PLANTED = ("nan_pos", "nan_neg", "pinf", "ninf", "overflow", "all")
NONFINITE = PLANTED + ("all_slices", "left_nan")
KINDS = NONFINITE + ("periodic", "periodic70", "negative")

# (W, H, D) per kind and form.  D = 40 is two chunks of slices (1 .. 32 | 33 .. 39), D = 70 three.  The Fast Guided Filter spreads
# a special value over two blurs of radius 8 / s subsampled pixels and the bilinear taps - about 2 * 8 + s full-resolution pixels
# each way against the full form's 8: its images are as much wider as leaves a tenth of them mixed (test_gray_inputs.py), and as
# high as leaves rows no site reaches.
_NF = {0: (70, 19, 40), 2: (102, 27, 40), 4: (118, 38, 40), 8: (150, 52, 40)}
SIZES = {k: _NF for k in NONFINITE}
SIZES["periodic"] = {0: (96, 17, 40), 2: (96, 17, 40), 4: (112, 17, 40), 8: (128, 17, 40)}
SIZES["periodic70"] = {0: (160, 17, 70), 2: (160, 17, 70), 4: (176, 17, 70), 8: (192, 17, 70)}
SIZES["negative"] = {0: (70, 19, 40), 2: (70, 19, 40), 4: (70, 19, 40), 8: (70, 19, 40)}
NEGATIVE_SHIFT = np.float32(2.0 ** 22)
TIE = {"periodic": (3, 35), "periodic70": (3, 35, 67)}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


VALUES = {
    "nan_pos": (_f(NAN_POS),), "nan_neg": (_f(NAN_NEG),), "pinf": (np.float32(np.inf),), "ninf": (np.float32(-np.inf),),
    "overflow": (np.float32(3e19), np.float32(-3e19)),
    "all": (np.float32(3e19), _f(NAN_NEG), np.float32(np.inf), _f(NAN_POS), np.float32(-np.inf), np.float32(-3e19)),
}
NSITES = {k: 3 for k in PLANTED}
NSITES["all"] = 6


def size(kind, s=0):
    return SIZES[kind][s]


def sampled(n, s):
    """the pixels of an axis of n that the filter at form s reads from a plane: all of them (s = 0) or nn's"""
    return np.arange(n) if s == 0 else F.nn_index(n, s)


def sites(W, H, s):
    """-> (left sites, right sites): six (y, x) each, on pixels the form samples - but for the left plane's site 3, the last pixel
    of the image, which the subsampling reads only where W - 1 and H - 1 are sampled.  Site 0 of either plane is the `aligned`
    pair: the same row, the right plane's align_d columns to the left - slice align_d of the left side and of the right side move
    one onto the other.  Site 1 is on the border (row 0), site 2 inside."""
    ys, xs = sampled(H, s), sampled(W, s)

    def at(fy, fx, dj=0):
        j = int(np.argmin(np.abs(xs - fx * (W - 1)))) + dj
        return int(ys[np.argmin(np.abs(ys - fy * (H - 1)))]), int(xs[j])

    step = 1 if s == 0 else s
    dj = -max(1, 8 // step)
    left = [at(0.5, 0.62), at(0.0, 0.93), at(0.2, 0.88), (H - 1, W - 1), at(0.55, 1.0), at(0.8, 0.8)]
    right = [at(0.5, 0.62, dj), at(0.0, 0.0), at(0.8, 0.1), at(1.0, 0.2), at(0.45, 0.0), at(0.2, 0.05)]
    return left, right


def align_d(W, H, s):
    l, r = sites(W, H, s)
    return l[0][1] - r[0][1]


def uniform(W, H, seed):
    l, r = np.random.default_rng([seed, W, H, 7]).random((2, H, W), dtype=np.float32)
    return np.ascontiguousarray(l), np.ascontiguousarray(r)


@functools.lru_cache(maxsize=None)
def pair(kind, s=0, seed=0, like=None):
    """-> (l, r) of the case (kind, s); kind "clean": the uniform pair of the size of the case (like, s)"""
    if kind == "clean":
        W, H, _ = size(like, s)
        return _ro(*uniform(W, H, seed))
    W, H, D = size(kind, s)
    if kind in PLANTED:
        l, r = uniform(W, H, seed)
        vals, n = VALUES[kind], NSITES[kind]
        for plane, where in zip((l, r), sites(W, H, s)):
            for i, (y, x) in enumerate(where[:n]):
                plane[y, x] = vals[i % len(vals)]
    elif kind in ("all_slices", "left_nan"):
        l, r = uniform(W, H, seed)
        l.view(np.uint32)[:] = NAN_NEG
        if kind == "all_slices":
            r.view(np.uint32)[:] = NAN_POS
    elif kind in TIE:
        rng = np.random.default_rng([seed, W, H, 32])
        base = rng.integers(0, 2, 32)
        flip = rng.integers(0, 2, (H, 1))
        wide = np.tile(base[None, :] ^ flip, (1, W // 32 + 2)).astype(np.float32)
        l, r = np.ascontiguousarray(wide[:, :W]), np.ascontiguousarray(wide[:, 3:W + 3])
    elif kind == "negative":
        rng = np.random.default_rng([seed, W, H])                    # test_gpu_gray.py's "float"
        l, r = (rng.uniform(-1024.0, 1024.0, (2, H, W)).astype(np.float32))
        l[0, 0], r[-1, -1] = np.float32(1024.0), np.float32(-1024.0)
        l, r = np.ascontiguousarray(l + NEGATIVE_SHIFT), np.ascontiguousarray(r + NEGATIVE_SHIFT)
    else:
        raise KeyError(kind)
    return _ro(l, r)


def as_bytes(kind, s=0, seed=0):
    """a periodic pair as uint8 planes 0 / 255: psm_upload_pair's conversion gives back the float planes bit for bit"""
    return _ro(*((p * np.float32(255)).astype(np.uint8) for p in pair(kind, s, seed)))


@functools.lru_cache(maxsize=None)
def volume(kind, s, side, seed=0, like=None):
    """-> (q [D][H][W], model) of one side, slice 0 included: model is ab [D][2][H][W] (s = 0; a, b) or [D][4][hs][ws] (a, b,
    blur(a), blur(b))"""
    l, r = pair(kind, s, seed, like)
    D = size(like or kind, s)[2]
    with np.errstate(all="ignore"):
        if s == 0:
            return _ro(*M.volume(l, r, side, 0, D, want_ab=True))
        return _ro(*F.volume(l, r, side, s, 0, D, want_model=True))


@functools.lru_cache(maxsize=None)
def maps(kind, s=0, seed=0, like=None):
    """-> (lmap, rmap): the model's selection over its own volumes (strict <: a NaN is never a candidate; no candidate: 0)"""
    out = []
    for side in (0, 1):
        q = volume(kind, s, side, seed, like)[0]
        out.append(M.wta_running(((d, q[d]) for d in range(1, q.shape[0])), q.shape[1:]))
    return _ro(*out)


def census(kind, s, side, seed=0):
    """-> dict of pixel counts of one side over the candidates d >= 1: mixed (some slices NaN, others not), dead (every slice NaN),
    total"""
    q = volume(kind, s, side, seed)[0][1:]
    nan = np.isnan(q)
    return dict(mixed=int(np.count_nonzero(nan.any(axis=0) & ~nan.all(axis=0))), dead=int(np.count_nonzero(nan.all(axis=0))),
                total=int(nan[0].size))


def ties(kind, s, side, seed=0):
    """-> bool [H][W]: every slice of TIE[kind] equals the minimum over d >= 1"""
    q = volume(kind, s, side, seed)[0]
    best = q[1:].min(axis=0)
    return np.logical_and.reduce([q[d] == best for d in TIE[kind]])


def minimum(kind, s, side, seed=0):
    """-> float32 [H][W]: the winning q (NaNs skipped; +inf where no slice is a candidate)"""
    q = volume(kind, s, side, seed)[0][1:]
    with np.errstate(all="ignore"):
        return np.fmin.reduce(np.where(np.isnan(q), np.float32(np.inf), q), axis=0)
