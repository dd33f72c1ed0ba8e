"""The 8-bit char mode's own arithmetic, stated in numpy independently of oracle/psm_oracle.c (cost_u8, quant_u8, psmo_wta_u8)
and of the kernels (k_cvf_pc<.., U8>, k_cvc_u8, k_f32_to_u8, k_wta_u8) - DESIGN.md 2 and 4.6.  Every fp32 rounding is one numpy
float32 operation, so nothing here can contract into a fused multiply-add.  The guided filter itself is NOT restated: it is the
oracle's guided_filter on cost * (1/255.0f), pinned by the float suites.

Three mutant switches state plausible wrong readings (the CPU test proves that the cases of tests/u8_inputs.py see each of them):
    cost="fma"     0.9f * c + (1 - 0.9f) * g with the first product fused into the addition (one rounding instead of two)
    quant="floor"  q8 = clip(floor(q * 255 + 0.5))             (round half up instead of half to even)
    quant="wrap"   q8 = (uchar)(int)rint(q * 255)              (a wrapping cast, no clamp)
"""
import numpy as np

from shard_model import unpack_disp as unpack       # (the disparity of a packed key)
from test_gpu_border_skip import keys_of            # (packed minima of a volume: strict '<' in ascending d, d = 0 never a candidate)

F = np.float32
ALPHA = F(0.9)
BETA = F(1) - F(0.9)                                # fl(1 - 0.9f)
INV255 = F(1) / F(255)                              # 1 / 255.0f as the C compiler folds it


def gray(img):
    """cv::cvtColor's 8-bit fixed point with 14 fractional bits, the coefficients in memory order."""
    c = img.astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def grad(g):
    """Sobel(gray, CV_8U, 1, 0, ksize 1): sat_u8(g[x+1] - g[x-1]), REFLECT_101."""
    p = np.pad(g.astype(np.int64), ((0, 0), (1, 1)), mode="reflect")
    return np.clip(p[:, 2:] - p[:, :-2], 0, 255).astype(np.uint8)


def planes(img):
    """[H][W][4] int64: c0, c1, c2, gradient."""
    return np.concatenate([img.astype(np.int64), grad(gray(img)).astype(np.int64)[..., None]], axis=2)


def cost_terms(base, other, d, right):
    """(clr // 3, grd) of slice d: `base` is the volume's own image, `other` the one it is matched against - read at x - d (left
    volume) or x + d (right volume), and as 255 in all four planes where that column does not exist."""
    H, W, _ = base.shape
    o = np.full_like(other, 255)
    if d < W:
        if right:
            o[:, :W - d] = other[:, d:]
        else:
            o[:, d:] = other[:, :W - d]
    diff = np.abs(base - o)
    return diff[..., :3].sum(axis=2) // 3, diff[..., 3]


def cost(c, g, mode="canon"):
    """(uchar)(0.9f * c + (1 - 0.9f) * g): two products and one sum, each rounded to fp32, then truncated."""
    c, g = c.astype(F), g.astype(F)
    bg = BETA * g                                   # fl(fl(1 - 0.9f) * grd)
    if mode == "fma":                               # fl(0.9f * c + bg): the product is exact in fp64 (24 x 8 bits), so is the sum
        f = (ALPHA.astype(np.float64) * c.astype(np.float64) + bg.astype(np.float64)).astype(F)
    else:
        f = ALPHA * c + bg
    return np.trunc(f).astype(np.uint8)             # (0 <= f < 256: nothing to saturate)


def raw_volumes(l, r, D, cost_mode="canon"):
    """-> (left, right) [D][H][W] uint8; the right volume with the images swapped."""
    pl, pr = planes(l), planes(r)
    lv = np.stack([cost(*cost_terms(pl, pr, d, False), cost_mode) for d in range(D)])
    rv = np.stack([cost(*cost_terms(pr, pl, d, True), cost_mode) for d in range(D)])
    return lv, rv


def filter_q(oracle, img, vol):
    """The guided filter of every slice of an 8-bit volume under the 8-bit image `img` -> q [D][H][W] float32, not yet quantised."""
    rgb, mean, var = oracle.cvf_preprocess(img.astype(F) * INV255)
    return np.stack([oracle.guided_filter(rgb, mean, var, s.astype(F) * INV255) for s in vol])


def scaled(q):
    """fl(q * 255.0f): the number the quantisation rounds."""
    return q.astype(F) * F(255)


def quant(q, mode="canon"):
    x = scaled(q)
    nan = np.isnan(x)
    x = np.where(nan, F(0), x)
    if mode == "floor":
        v = np.clip(np.floor(x + F(0.5)), 0, 255)
    elif mode == "wrap":
        v = np.rint(x).astype(np.int64) & 255
    else:
        v = np.clip(np.rint(x), 0, 255)             # numpy's rint rounds halves to even, as rintf does
    return np.where(nan, 0, v).astype(np.uint8)


def wta(vol):
    """assets/dispsel.cl with the start value 256: d = 1 .. D-1 in ascending order, strict '<'; so a volume of 255 gives d = 1."""
    D = vol.shape[0]
    best = np.full(vol.shape[1:], 256, np.int64)
    disp = np.zeros(vol.shape[1:], np.uint8)
    for d in range(1, D):
        c = vol[d].astype(np.int64)
        win = c < best
        best = np.where(win, c, best)
        disp = np.where(win, d, disp).astype(np.uint8)
    return disp


def edges(x):
    """What a scaled value fl(q * 255) can do to a quantiser -> dict of boolean masks."""
    fl = np.floor(x)
    half = (x - fl == F(0.5)) & (x > 0) & (x < 255)
    return {"over": x > F(255.5), "under": x < F(-0.5), "half_even": half & (fl % 2 == 0), "half_odd": half & (fl % 2 == 1)}


def tie_masks(vol, S):
    """Pixels whose winning value is held by two or more candidate slices (d >= 1), and among them those where one holder has a
    local index = 0 mod S (a minima-plane slice of the two-phase selection) and another has not (a key-phase slice)."""
    v = vol[1:].astype(np.int64)
    hold = v == v.min(axis=0)
    d = np.arange(1, vol.shape[0])[:, None, None]
    seed = (hold & (d % S == 0)).any(axis=0)
    rest = (hold & (d % S != 0)).any(axis=0)
    return hold.sum(axis=0) >= 2, seed & rest


def from_raw(oracle, l, r, raw_l, raw_r, quant_mode="canon"):
    """Raw (or uploaded) 8-bit volumes -> everything the device is compared on."""
    ql, qr = filter_q(oracle, l, raw_l), filter_q(oracle, r, raw_r)
    lv, rv = quant(ql, quant_mode), quant(qr, quant_mode)
    return {"raw_l": raw_l, "raw_r": raw_r, "ql": ql, "qr": qr, "lvol": lv, "rvol": rv, "ldisp": wta(lv), "rdisp": wta(rv),
            "lkeys": keys_of(lv), "rkeys": keys_of(rv)}


def pipeline(oracle, l, r, D, cost_mode="canon", quant_mode="canon"):
    raw_l, raw_r = raw_volumes(l, r, D, cost_mode)
    return from_raw(oracle, l, r, raw_l, raw_r, quant_mode)
