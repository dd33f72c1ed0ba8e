"""Adversarial inputs for the 8-bit char mode (tests/test_u8_inputs.py proves on the CPU that each reaches its edge;
tests/test_gpu_u8_adversarial.py runs them through every form the mode has).  A case is a pair of 8-bit images and, for the
uploaded form, the two 8-bit cost volumes that psm_upload_volume puts in place of the built ones.  Seeds are fixed here.

Geometries: SMALL 100 x 24 x 12 (two column groups of the narrow layout, forced two-phase takes S = 5), TALL 96 x 208 x 12
(>= 200 rows: pc_seed_stride gives S = 8; seed_stride_rule below reads the bound from psm_pc.hip), TABLE 768 x 256 x 3.

Measured on the CPU model (tests/u8_model.py; test_u8_inputs.py asserts the bars, the figures are what the model gave when the
cases were written; python -m pytest -s tests/test_u8_inputs.py -k case_table prints it again).  a/b: left / right volume.
over / under: voxels of both sides with fl(q * 255) > 255.5 / < -0.5; halves: exact x.5 with even / odd
floor; ties: share of pixels (both maps) whose winning q8 is held by >= 2 slices, and of those the pixels where a holder with
d = 0 mod S meets one with d != 0 mod S, for S = 5 / 8; the mutant columns: elements of (raw volumes, filtered volumes, keys)
that the mutant changes.

table_black            over 0/0 under 2328/0 half_even 0/109 half_odd 0/76 ties 58% cross5 0 cross8 0 fma 2826/3246/1236 floor 0/109/37 wrap 0/2328/776 raw255 0%
table_white            over 0/0 under 0/131 half_even 0/6 half_odd 1/0 ties 58% cross5 0 cross8 0 fma 2826/3227/1242 floor 0/6/2 wrap 0/131/38 raw255 0%
extrap_0.5pc           over 9/0 under 10/503 half_even 0/0 half_odd 0/0 ties 18% cross5 459 cross8 244 fma 658/766/52 floor 0/0/0 wrap 0/522/63 raw255 0%
extrap_0.5pc_negative  over 8/0 under 10/525 half_even 0/0 half_odd 0/0 ties 19% cross5 478 cross8 272 fma 594/623/51 floor 0/0/0 wrap 0/543/64 raw255 0%
extrap_2pc             over 15/0 under 25/328 half_even 0/0 half_odd 1/0 ties 15% cross5 380 cross8 151 fma 634/667/49 floor 0/0/0 wrap 0/368/65 raw255 0%
extrap_2pc_negative    over 17/0 under 26/334 half_even 0/0 half_odd 0/2 ties 16% cross5 431 cross8 203 fma 592/608/37 floor 0/0/0 wrap 0/377/64 raw255 0%
extrap_checker         over 0/8 under 0/0 half_even 0/0 half_odd 0/0 ties 23% cross5 408 cross8 80 fma 0/0/0 floor 0/0/0 wrap 0/8/4 raw255 20%
half_100x24            over 0/0 under 0/0 half_even 6276/0 half_odd 4184/0 ties 90% cross5 4204 cross8 4065 fma 0/0/0 floor 0/6276/546 wrap 0/0/0 raw255 3%
half_96x208            over 0/1 under 0/0 half_even 27944/0 half_odd 12008/0 ties 90% cross5 34889 cross8 33721 fma 0/0/0 floor 0/27944/2436 wrap 0/1/1 raw255 3%
tie_const_100x24       over 0/0 under 0/0 half_even 0/0 half_odd 0/0 ties 91% cross5 4224 cross8 4080 fma 0/0/0 floor 0/0/0 wrap 0/0/0 raw255 0%
tie_step_100x24        over 0/0 under 79/228 half_even 112/162 half_odd 2/6 ties 74% cross5 3090 cross8 2715 fma 0/0/0 floor 0/274/0 wrap 0/307/13 raw255 0%
tie_columns_100x24     over 0/0 under 0/24 half_even 0/0 half_odd 0/0 ties 88% cross5 4224 cross8 4080 fma 0/0/0 floor 0/0/0 wrap 0/24/24 raw255 23%
tie_const_96x208       over 0/0 under 0/0 half_even 0/0 half_odd 0/0 ties 91% cross5 34944 cross8 33696 fma 0/0/0 floor 0/0/0 wrap 0/0/0 raw255 0%
tie_step_96x208        over 0/0 under 79/228 half_even 1124/1726 half_odd 2/6 ties 74% cross5 25162 cross8 22027 fma 0/0/0 floor 0/2850/0 wrap 0/307/13 raw255 0%
tie_columns_96x208     over 0/0 under 0/0 half_even 0/0 half_odd 0/0 ties 87% cross5 34736 cross8 33488 fma 0/0/0 floor 0/0/0 wrap 0/0/0 raw255 23%
sat_channel_noise      over 0/0 under 0/0 half_even 0/0 half_odd 0/2 ties 7% cross5 140 cross8 74 fma 0/0/0 floor 0/0/0 wrap 0/0/0 raw255 1%
sat_binary_inverse     over 53/19 under 0/0 half_even 0/0 half_odd 0/0 ties 7% cross5 154 cross8 85 fma 0/0/0 floor 0/0/0 wrap 0/72/28 raw255 21%
up_all255              over 0/0 under 0/0 half_even 0/0 half_odd 0/0 ties 100% cross5 4800 cross8 4800 fma 0/0/0 floor 0/0/0 wrap 0/0/0 raw255 100%
up_all0                over 0/0 under 0/0 half_even 0/0 half_odd 0/0 ties 100% cross5 4800 cross8 4800 fma 0/0/0 floor 0/0/0 wrap 0/0/0 raw255 0%
up_binary              over 1/0 under 0/1 half_even 1/0 half_odd 0/0 ties 4% cross5 64 cross8 38 fma 0/0/0 floor 0/1/1 wrap 0/2/2 raw255 50%
up_repeated_min        over 0/0 under 0/0 half_even 0/0 half_odd 0/0 ties 100% cross5 4800 cross8 4800 fma 0/0/0 floor 0/0/0 wrap 0/0/0 raw255 1%
up_stripes_100x24      over 0/0 under 0/0 half_even 3400/3400 half_odd 2000/2000 ties 0% cross5 0 cross8 0 fma 0/0/0 floor 0/6800/1200 wrap 0/0/0 raw255 2%
up_stripes_96x208      over 0/0 under 0/0 half_even 6720/6720 half_odd 11520/11520 ties 0% cross5 0 cross8 0 fma 0/0/0 floor 0/13440/3264 wrap 0/0/0 raw255 0%
"""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = namedtuple("Case", "name family l r vols W H D")     # vols: None, or (left, right) uint8 [D][H][W] to upload

SMALL, TALL, TABLE = (100, 24, 12), (96, 208, 12), (768, 256, 3)


def gray3(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g, np.uint8)[..., None], 3, axis=2))


def case(name, family, l, r, D, vols=None):
    H, W, _ = l.shape
    assert r.shape == l.shape and l.dtype == r.dtype == np.uint8
    if vols is not None:
        vols = tuple(np.ascontiguousarray(v, np.uint8) for v in vols)
        assert all(v.shape == (D, H, W) for v in vols)
    return Case(name, family, l, r, vols, W, H, D)


def seed_stride_rule():
    """(row bound, S below it, S from it up) as pc_seed_stride states them for 8-bit images below its pixel bound."""
    src = open(os.path.join(ROOT, "primestereomatch_amd", "csrc", "psm_pc.hip")).read()
    body = src[src.index("int pc_seed_stride(int W, int rows, bool u8)"):]
    body = body[:body.index("\n}")]
    m = re.search(r"if \(rows < (\d+) \|\| \(u8 && \(size_t\)W \* rows >= (\d+)\)\) return (\d+);.*\n\s*return (\d+);", body)
    assert m, body
    rows, pixels, below, above = map(int, m.groups())
    return rows, pixels, below, above


def seed_stride(H):
    """S of a forced two-phase selection over all H rows of an 8-bit case."""
    rows, _, below, above = seed_stride_rule()
    return below if H < rows else above


# ---- cost table: every pair (clr / 3, grd) -----------------------------------------------------------------------------------
def table_image():
    """Row c holds the triples (0, c, g), g = 0 .. 255: against a black image the centre pixel of a triple has a colour difference
    of c in every channel and a gradient sat(g - 0) = g against the black image's 0."""
    W, H, _ = TABLE
    t = np.zeros((H, W), np.uint8)
    t[:, 1::3] = np.arange(256, dtype=np.uint8)[:, None]
    t[:, 2::3] = np.arange(256, dtype=np.uint8)[None, :]
    return gray3(t)


def table_cases():
    W, H, D = TABLE
    t = table_image()
    return [case("table_black", "table", t, np.zeros_like(t), D),                     # the table is the left volume's own image
            case("table_white", "table", np.full_like(t, 255), t, D)]               # ... the right volume's own image, against white


# ---- extrapolation: the linear model a.I + b leaves [0, 1] ------------------------------------------------------------------
def extrapolation_pair(W, H, seed, share):
    rng = np.random.default_rng(seed)
    l = rng.integers(0, 32, (H, W)).astype(np.int64)
    l[rng.random((H, W)) < share] = 255
    r = np.empty_like(l)
    r[:, :W - 3] = l[:, 3:]
    r[:, W - 3:] = l[:, W - 4:W - 3]
    return l.astype(np.uint8), np.clip(r * 8, 0, 255).astype(np.uint8)


def checker_pair(W, H, seed):
    y, x = np.mgrid[0:H, 0:W]
    l = (((x // 4) + (y // 4)) % 2 * 255).astype(np.uint8)
    r = (np.random.default_rng(seed).integers(0, 2, (H, W)) * 255).astype(np.uint8)
    return l, r


def extrapolation_cases():
    W, H, D = SMALL
    out = []
    for share in (0.005, 0.02):
        l, r = extrapolation_pair(W, H, 41, share)
        tag = "%g" % (100 * share)
        out.append(case(f"extrap_{tag}pc", "extrap", gray3(l), gray3(r), D))
        out.append(case(f"extrap_{tag}pc_negative", "extrap", gray3(255 - l), gray3(255 - r), D))
    l, r = checker_pair(W, H, 43)
    out.append(case("extrap_checker", "extrap", gray3(l), gray3(r), D))
    return out


# ---- exact rounding halves ----------------------------------------------------------------------------------------------------
def colour_for_cost(k):
    """The smallest colour difference c with trunc(0.9f * c) = k (gradient 0); k <= 229."""
    c = np.arange(256)
    hit = np.nonzero(np.trunc(np.float32(0.9) * c.astype(np.float32)) == k)[0]
    assert hit.size, k
    return int(hit[0])


# one k per band, both parities, out of those whose k + 1/2 survives the fp32 roundings of cost / 255, the double box mean and
# x 255 (a scan of k = 0 .. 228 on the model: 0, 4, 8, 10, 16 .. 22, 32 .. 46, 64 .. 95, the odd k of 127 .. 189)
HALF_KS = {12: [42, 135], 16: [0, 17, 36, 65, 84, 127, 18, 143, 90, 167, 44, 189, 72]}


def stripes(W, H, band, ks, value=lambda k: k):
    """Period-2 vertical stripes value(k), value(k + 1) in horizontal bands of `band` rows."""
    out = np.zeros((H, W), np.uint8)
    for i, k in enumerate(ks):
        out[i * band:(i + 1) * band, 0::2] = value(k)
        out[i * band:(i + 1) * band, 1::2] = value(k + 1)
    return out


def half_cases():
    """A black left image is constant guidance with I.p = 0 exactly: a = 0 and q is the double box mean of the costs.  The right
    image's stripes have zero gradient (period 2), so the left volume's costs are k, k + 1 in stripes and their mean is k + 1/2."""
    out = []
    for (W, H, D), band in ((SMALL, 12), (TALL, 16)):
        assert len(HALF_KS[band]) * band == H
        r = stripes(W, H, band, HALF_KS[band], colour_for_cost)
        out.append(case(f"half_{W}x{H}", "half", gray3(np.zeros((H, W))), gray3(r), D))
    return out


# ---- ties on the winning value ------------------------------------------------------------------------------------------------
def tie_cases():
    out = []
    for W, H, D in (SMALL, TALL):
        tag = f"{W}x{H}"
        c = gray3(np.full((H, W), 90))
        out.append(case(f"tie_const_{tag}", "tie", c, c.copy(), D))
        s = np.full((H, W), 40)
        s[:, W // 2:] = 200
        s[H // 2:, W // 4:] += 30
        out.append(case(f"tie_step_{tag}", "tie", gray3(s), gray3(s), D))
        # 0/255 columns of period 3 against their shift by 2: the slices d = 2, 5, 8, 11 repeat the match, so the winning value meets
        # a seed slice of S = 5 (d = 5) and of S = 8 (d = 8) next to key-phase slices
        col = np.broadcast_to((np.arange(W + 2) % 3 == 0) * 255, (H, W + 2))
        out.append(case(f"tie_columns_{tag}", "tie", gray3(col[:, :W]), gray3(col[:, 2:]), D))
    return out


# ---- saturated costs ----------------------------------------------------------------------------------------------------------
def saturated_cases():
    W, H, D = SMALL
    rng = np.random.default_rng(47)
    l = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    r = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    b = (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8)
    return [case("sat_channel_noise", "sat", l, r, D), case("sat_binary_inverse", "sat", gray3(b), gray3(255 - b), D)]


# ---- uploaded 8-bit volumes: the storing path and the 8-bit WTA ---------------------------------------------------------------
def upload_cases():
    out = []
    W, H, D = SMALL
    rng = np.random.default_rng(53)
    l = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    shape = (D, H, W)
    out.append(case("up_all255", "upload", l, r, D, (np.full(shape, 255), np.full(shape, 255))))
    out.append(case("up_all0", "upload", l, r, D, (np.zeros(shape), np.zeros(shape))))
    out.append(case("up_binary", "upload", l, r, D, (rng.integers(0, 2, shape) * 255, rng.integers(0, 2, shape) * 255)))
    # the minimum repeats: slices 1, 5, 8 and D - 1 hold the same low plane, so their filtered slices are equal bit for bit
    vols = []
    for _ in range(2):
        v = rng.integers(128, 256, shape)
        v[[1, 5, 8, D - 1]] = rng.integers(0, 64, (H, W))[None]
        vols.append(v)
    out.append(case("up_repeated_min", "upload", l, r, D, tuple(vols)))
    # k / k + 1 stripes under a constant (black) image, one k per (slice, band), spread evenly over 0 .. 254
    for (W, H, D), band in ((SMALL, 12), (TALL, 16)):
        nb = (H + band - 1) // band
        ks = (np.arange(D * nb) * 254 // (D * nb - 1)).reshape(D, nb)
        v = np.stack([stripes(W, H, band, [int(k) for k in ks[d]]) for d in range(D)])
        black = gray3(np.zeros((H, W)))
        out.append(case(f"up_stripes_{W}x{H}", "upload", black, black.copy(), D, (v, v[::-1].copy())))
    return out


def all_cases():
    return table_cases() + extrapolation_cases() + half_cases() + tie_cases() + saturated_cases() + upload_cases()


CASES = all_cases()
IMAGE_CASES = [c for c in CASES if c.vols is None]
UPLOAD_CASES = [c for c in CASES if c.vols is not None]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# row stripes and disparity shards: the table, an extrapolation, the half and a tie case (the tall ones: their stripes cut a band)
SUBSET = ["table_black", "extrap_2pc_negative", "half_96x208", "tie_columns_96x208", "half_100x24"]
