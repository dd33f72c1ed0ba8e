"""Cases, contents and references for the seam, small-image and adversarial tests of the Fast Guided Filter path
(psm_cost_filter_fgf, psm_fgf.hip; tests/test_gpu_fgf_seams.py runs them on the device, tests/test_fgf_inputs.py holds them to
their own conditions on the CPU).  Pure numpy plus the CPU oracle, no GPU; every function is a deterministic function of its
arguments.

The references are composed from the oracle's stage functions (u8_to_f32, cvc_preprocess, cvc_build, fgf_setup, fgf_filter, wta)
so that they also take float pairs and uploaded volumes; on byte pairs they are psmo_pipeline_fgf bit for bit.  Nothing here has
a tolerance: the kernels evaluate the oracle's arithmetic operation for operation."""
from __future__ import annotations

import numpy as np

import fuzz_inputs as F
from primestereomatch_amd import synth

RATES = (2, 4, 8)
CONTENTS = ("synth", "noise", "binary", "constant", "half_flat")      # kinds of fuzz_inputs.sgm_content


def _oracle():
    from oracle import psm_oracle_py as O
    O.build()
    return O


def radius(s):
    return 8 // s                      # the blur radius of the subsampled image: k = 2 * (8 / s) + 1 taps


def strip_width(s):
    return 64 - 2 * radius(s)          # blur4_march: OUTW = 64 - 2 * R output columns of one wave


def nn_idx(size, s):
    """cv::resize INTER_NN source indices of an axis of `size` pixels subsampled by s (nn_src in psm_fgf.hip, nn_maps in the oracle):
    the pixels of the full-resolution axis that the filter reads from a cost slice - the others never reach it."""
    d = size // s
    return np.minimum(np.floor(np.arange(d) * (1.0 / (d / size))).astype(np.int64), size - 1)


# ------------------------------------------------------------------------------------------------------------------------ references

def _f32_image(img):
    img = np.asarray(img)
    return _oracle().u8_to_f32(img) if img.dtype == np.uint8 else np.ascontiguousarray(img, np.float32)


def reference(l, r, D, s, d_range=None):
    """CostConst -> CostFilter_FGF -> DispSelect of a uint8 or float32 pair from the oracle's stage functions
    -> {"lvol", "rvol", "ldisp", "rdisp"}; d_range = (d0, d1): the volumes hold those slices only, no maps."""
    O = _oracle()
    lf, rf = _f32_image(l), _f32_image(r)
    lg, rg = O.cvc_preprocess(lf), O.cvc_preprocess(rf)
    d0, d1 = d_range or (0, D)
    lset, rset = O.fgf_setup(lf, s), O.fgf_setup(rf, s)
    # buildCV_right takes the images swapped (src/DispEst.cpp:217,260)
    lvol = np.stack([O.fgf_filter(lf, lset, O.cvc_build(lf, rf, lg, rg, d), s) for d in range(d0, d1)])
    rvol = np.stack([O.fgf_filter(rf, rset, O.cvc_build(rf, lf, rg, lg, d, right=True), s) for d in range(d0, d1)])
    out = {"lvol": lvol, "rvol": rvol}
    if d_range is None:
        out["ldisp"], out["rdisp"] = O.wta(lvol), O.wta(rvol)
    return out


def reference_uploaded(img, vol, s):
    """psm_upload_volume -> psm_cost_filter_fgf -> psm_disp_select of one side: fgf_filter per slice with `img` as the guidance, then
    the winner-takes-all -> (filtered volume, map)"""
    O = _oracle()
    f = _f32_image(img)
    setup = O.fgf_setup(f, s)
    q = np.stack([O.fgf_filter(f, setup, vol[d], s) for d in range(vol.shape[0])])
    return q, O.wta(q)


# ---------------------------------------------------------------------------------------------------------------- launch arithmetic

def grid(W, H, D, s):
    """The grids psm_fgf.hip launches for a W x H image with D local slices at rate s, restated.

    launch_fgf_model:
        const int ws = W / sub, hs = H / sub, k = 2 * (8 / sub) + 1;
        const int nstrips = (ws + (64 - 2 * (k / 2)) - 1) / (64 - 2 * (k / 2));
        int nsegs = (8192 + nstrips * Dloc - 1) / (nstrips * Dloc);
        int seg = (hs + nsegs - 1) / nsegs;
        if (seg < 4 * k) seg = 4 * k;
        if (seg > hs) seg = hs;
        nsegs = (hs + seg - 1) / seg;
    launch_fgf_apply (launch_fgf_apply_wta: the same x and z, rb = 2 always):
        if (W % 4 == 0) {
            const int dchunk = Dloc < 32 ? Dloc : 32;
            const int rb = sub == 2 ? 2 : 4, yshift = (sub / 2) % rb;
            dim3 gf((W / 4 + 255) / 256, (H + yshift + rb - 1) / rb, (Dloc + dchunk - 1) / dchunk);
        } else {
            dim3 gf((W + 255) / 256, H, Dloc);                                        // k_fgf_apply: one slice per z

    -> dict: ws, hs, strips, last_strip (columns of the last strip), segs, seg, last_seg (rows of the last segment), fused (the
    4-pixel kernels k_fgf_apply4 / k_fgf_apply_wta run: W % 4 == 0), xblocks (of the apply kernel that runs), chunks (of 32 slices;
    what a thread of the 4-pixel kernels loops over), and for each of the two 4-pixel kernels (rb, rows of the first row block
    above the image, rows of the last one below it)."""
    ws, hs, k = W // s, H // s, 2 * (8 // s) + 1
    outw = 64 - 2 * (k // 2)
    strips = (ws + outw - 1) // outw
    nsegs = (8192 + strips * D - 1) // (strips * D)
    seg = (hs + nsegs - 1) // nsegs
    seg = max(seg, 4 * k)
    seg = min(seg, hs)
    nsegs = (hs + seg - 1) // seg
    fused = W % 4 == 0
    dchunk = min(D, 32)

    def rows(rb):
        yshift = (s // 2) % rb
        blocks = (H + yshift + rb - 1) // rb
        return rb, yshift, blocks * rb - yshift - H

    return dict(ws=ws, hs=hs, strips=strips, last_strip=ws - (strips - 1) * outw, segs=nsegs, seg=seg, last_seg=hs - (nsegs - 1) * seg,
                fused=fused, xblocks=(W // 4 + 255) // 256 if fused else (W + 255) // 256, chunks=(D + dchunk - 1) // dchunk,
                apply4=rows(2 if s == 2 else 4), apply_wta=rows(2))


def refused(W, H, s):
    """psm_cost_filter_fgf: if (ws <= rad || hs <= rad) return fail(c, "... too small for subsample_rate ...")"""
    return W // s <= radius(s) or H // s <= radius(s)


# -------------------------------------------------------------------------------------------------------------------------- the cases

def _case(tag, W, H, D, s, i):
    return (tag, W, H, D, s, CONTENTS[i % len(CONTENTS)], 7919 * i + 13 * W + H)


def seam_cases():
    """-> list of (tag, W, H, D, s, content kind, seed): the strips of blur4_march, the row segments of launch_fgf_model, the x-blocks
    and row blocks of the apply kernels and the 32-slice chunks, per rate.  The kinds go round CONTENTS."""
    geo = []
    # strips: exactly 64 - 2 R subsampled columns | one more: a strip of one column (W % s = 0 and != 0) | more | three strips
    geo += [("strips", W, 24, 3, 8) for W in (496, 504, 505, 512, 1000)]
    geo += [("strips", W, 24, 2, 4) for W in (240, 244, 247, 484)]
    geo += [("strips", W, 24, 3, 2) for W in (112, 114, 115, 117, 226, 228)]
    # segments: one of exactly 4 k rows | two, the last one row | three; H % s != 0 in the last
    geo += [("segments", 40, H, 2, 2) for H in (72, 74, 147)]
    geo += [("segments", 40, H, 3, 4) for H in (80, 84, 167)]
    geo += [("segments", 40, H, 2, 8) for H in (96, 104)] + [("segments", 44, 207, 3, 8)]          # 44: W % 4 = 0, W % 8 != 0
    # two strips and two segments in one launch (the shard test cuts these)
    geo += [("strips x segments", W, H, 3, s) for W, H, s in STRIPS_AND_SEGMENTS]
    # H % 4 = 0 .. 3 with 16-byte rows: the first and last row blocks of the 4-pixel kernels hang over the image
    geo += [("row blocks", 44, H, 2, s) for s in RATES for H in (40, 41, 42, 43)]
    # a second x-block of the 4-pixel kernels with one live thread | five blocks of k_fgf_apply, the last with 6 live threads
    geo += [("x-blocks", 1028, 10, 2, 2), ("x-blocks", 1028, 12, 3, 4), ("x-blocks", 1028, 16, 2, 8), ("x-blocks", 1030, 11, 2, 2)]
    # chunks of 32 slices: one full | one slice more | two full | ... (W % 4 = 0: the key merge of k_fgf_apply_wta)
    geo += [("chunks", 72, 12, D, 4) for D in (32, 33, 64, 65, 70)] + [("chunks", 72, 12, 33, 2), ("chunks", 72, 16, 65, 8)]
    return [_case(*g, i) for i, g in enumerate(geo)]


STRIPS_AND_SEGMENTS = ((116, 74, 2), (244, 84, 4), (504, 104, 8))          # (W, H, s): two strips, two segments, 16-byte rows


def small_sizes(s):
    """The full-resolution sizes whose subsampled size lies in [R + 1, 2 R]: a blur window reflects at both ends of the axis"""
    return list(range(s * (radius(s) + 1), s * (2 * radius(s) + 1)))


def small_cases():
    """-> the same tuples: every size of small_sizes as the width alone (height 40: subsampled 20, 10, 5), as the height alone, and
    both together (each width once, with the heights in falling order)."""
    geo = []
    for s in RATES:
        sizes = small_sizes(s)
        geo += [("small W", n, 40, 3, s) for n in sizes]
        geo += [("small H", 40, n, 2, s) for n in sizes]
        geo += [("small W H", n, m, 3, s) for n, m in zip(sizes, sizes[::-1])]
        geo += [("small W H", sizes[0], sizes[0], 2, s), ("small W H", sizes[-1], sizes[-1], 2, s)]
    return [_case(*g, 1000 + i) for i, g in enumerate(geo)]


def refusal_cases():
    """-> list of (W, H, s, refused): both sides of the library's bound per rate and axis - subsampled size R is refused ("too
    small"), R + 1 runs.  W = 8 or H = 8, the context's minimum, is on the refused side at every rate."""
    out = []
    for s in RATES:
        R = radius(s)
        at, above = [R * s, R * s + s - 1], [(R + 1) * s]                 # subsampled R (both ends of its range) | R + 1
        out += [(n, 40, s, True) for n in at] + [(40, n, s, True) for n in at] + [(8, 8, s, True)]
        out += [(n, 40, s, False) for n in above] + [(40, n, s, False) for n in above]
    return out


def cases():
    return seam_cases() + small_cases()


def content(case):
    """-> (l, r) uint8 [H][W][3] of a case tuple"""
    _, W, H, D, s, kind, seed = case
    return F.sgm_content(kind, W, H, D, np.random.default_rng(seed))


def _g(c):
    return grid(*c[1:5])


# (name, predicate on a case tuple): every entry holds for at least one case of cases(), for every rate where `per rate`
REQUIRED = (
    ("one strip of exactly 64 - 2 R columns", lambda c: _g(c)["strips"] == 1 and _g(c)["ws"] == strip_width(c[4])),
    ("a last strip of one column", lambda c: _g(c)["strips"] == 2 and _g(c)["last_strip"] == 1),
    ("a last strip of one column, W % s != 0", lambda c: _g(c)["strips"] == 2 and _g(c)["last_strip"] == 1 and c[1] % c[4]),
    ("three strips", lambda c: _g(c)["strips"] == 3),
    ("one segment of exactly 4 k rows", lambda c: _g(c)["segs"] == 1 and _g(c)["hs"] == 4 * (2 * radius(c[4]) + 1)),
    ("two segments, the last of one row", lambda c: _g(c)["segs"] == 2 and _g(c)["last_seg"] == 1),
    ("a last segment shorter than the radius", lambda c: _g(c)["segs"] >= 2 and _g(c)["last_seg"] <= radius(c[4])),
    ("three segments", lambda c: _g(c)["segs"] == 3),
    ("two strips and two segments, 16-byte rows", lambda c: _g(c)["strips"] >= 2 and _g(c)["segs"] >= 2 and _g(c)["fused"]),
    ("H % s != 0", lambda c: c[2] % c[4] != 0),
    ("W % s != 0", lambda c: c[1] % c[4] != 0),
    ("H % 4 = 0, 16-byte rows", lambda c: _g(c)["fused"] and c[2] % 4 == 0),
    ("H % 4 = 1, 16-byte rows", lambda c: _g(c)["fused"] and c[2] % 4 == 1),
    ("H % 4 = 2, 16-byte rows", lambda c: _g(c)["fused"] and c[2] % 4 == 2),
    ("H % 4 = 3, 16-byte rows", lambda c: _g(c)["fused"] and c[2] % 4 == 3),
    ("two x-blocks of the 4-pixel kernels, one live thread in the second", lambda c: _g(c)["fused"] and c[1] == 1028),
    ("k_fgf_apply (W % 4 != 0)", lambda c: not _g(c)["fused"]),
    ("every content kind", None),                                                                        # (checked as a set)
)
REQUIRED_ONCE = (
    ("several x-blocks of k_fgf_apply", lambda c: not _g(c)["fused"] and _g(c)["xblocks"] >= 2),
    ("W % s != 0 with 16-byte rows (s = 8 alone: 2 and 4 divide 4)", lambda c: c[4] == 8 and c[1] % 8 != 0 and _g(c)["fused"]),
) + tuple((f"D = {D}, 16-byte rows ({(D + 31) // 32} chunks, the last of {D - 32 * ((D - 1) // 32)})",
           lambda c, D=D: c[3] == D and _g(c)["fused"]) for D in (32, 33, 64, 65, 70))


def missing(case_list):
    """-> the names of the REQUIRED / REQUIRED_ONCE entries (with the rate) that no case of case_list meets, and the small sizes no
    case covers.  Empty for cases()."""
    out = []
    for name, has in REQUIRED:
        for s in RATES:
            mine = [c for c in case_list if c[4] == s]
            if has is None:
                if {c[5] for c in mine} != set(CONTENTS):
                    out.append((name, s))
            elif not any(has(c) for c in mine):
                out.append((name, s))
    out += [(name, None) for name, has in REQUIRED_ONCE if not any(has(c) for c in case_list)]
    for s in RATES:
        big = lambda n: n // s > 2 * radius(s)
        mine = [c for c in case_list if c[4] == s]
        for n in small_sizes(s):
            if not any(c[1] == n and big(c[2]) for c in mine):
                out.append((f"small width {n} alone", s))
            if not any(c[2] == n and big(c[1]) for c in mine):
                out.append((f"small height {n} alone", s))
            if not any(c[1] == n and c[2] in small_sizes(s) for c in mine):
                out.append((f"small width {n} with a small height", s))
            if not any(c[2] == n and c[1] in small_sizes(s) for c in mine):
                out.append((f"small height {n} with a small width", s))
    return out


# --------------------------------------------------------------------------------------------------------------------- float pairs

FLOAT_CASES = ((44, 26, 5, 2, 61), (52, 41, 4, 4, 62), (72, 43, 6, 8, 63))            # (W, H, D, s, seed)


def float_pair(W, H, D, seed):
    """fuzz_inputs.float_pair of a synth pair with the NaN and +-inf elements put back to byte / 255: one of them makes the guidance
    NaN within two blur radii, on these sizes everywhere.  Values below 0 and above 1, -0.0 and the exact .5 products stay."""
    rng = np.random.default_rng(seed)
    l, r, _ = synth.make_pair(W, H, D, seed=seed)
    out = []
    for f, u in zip(F.float_pair(l, r, rng), (l, r)):
        bad = ~np.isfinite(f)
        f[bad] = (u.astype(np.float32) * np.float32(1 / 255.0))[bad]
        out.append(f)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------- adversarial uploaded volumes

# three chunks of slices (32, 32, 6), 16-byte rows: the fused upsample + WTA; 72 wide: a context takes no max_disp above its width
ADV_W, ADV_H, ADV_D = 72, 24, 70
REPEATS = ((31, 32), (32, 63), (63, 64), (64, 69), (1, 69))          # pairs of equal slices either side of a chunk seam
NEGATIVE_D, NEGATIVE_OTHERS = 40, ((5, 3.0), (66, 4.0))             # the winner X - 5 | (slice, c): X - c in the other two chunks
SUBNORMAL_D, SUBNORMAL_OTHER = 50, 10
NAN_WINNER, NAN_SECOND, NAN_SLICE, NAN_HUGE = 20, 45, 33, 60
ADVERSARIAL = tuple(f"repeats-{a}-{b}" for a, b in REPEATS) + ("negative", "subnormal", "nan")


def adversarial_guidance():
    l, r, _ = synth.make_pair(ADV_W, ADV_H, 8, seed=4)
    return l, r


def _base(seed):
    X = np.random.default_rng(seed).random((ADV_H, ADV_W), dtype=np.float32)
    vol = np.empty((ADV_D, ADV_H, ADV_W), np.float32)
    vol[:] = X + np.float32(1)
    return X, vol


def nan_pixels(s):
    """-> (corner, patch): index arrays (ys, xs) of full-resolution pixels the subsampling at rate s reads - the first sampled pixel
    of the image, and the last two sampled rows x the last sampled column"""
    yi, xi = nn_idx(ADV_H, s), nn_idx(ADV_W, s)
    return (yi[:1], xi[:1]), (yi[-2:], xi[-1:])


def adversarial_volume(name, s):
    """-> float32 [70][24][72]; the properties test_fgf_inputs.py asserts of its reference:
    repeats-a-b  every slice X + 1, the slices a and b X itself: their filtered slices are the same bits and below every other
                 slice, so every pixel's winner is the lower of the two - the lowest-d rule across the merge of the chunks' keys
    negative     slice 40 is X - 5: it wins everywhere with a negative cost; the slices 5 and 66, in the other two chunks, are X - 3
                 and X - 4, negative everywhere too - the merge of the chunks' keys orders negative floats among themselves (keys
                 that kept the raw bits of a negative float would order them backwards and slice 5 would win)
    subnormal    slice 50 is 1e-41, slice 10 is 2e-41: the filtered slice 50 is subnormal and not zero, and wins; flushed to
                 zero both would be 0 and slice 10 would win
    nan          (rate-dependent: the special values sit on pixels the subsampling reads) slice 33 all NaN; slice 20 = X - 5, the
                 winner, with a NaN patch in one corner; slice 45 = X - 2 wins under the patch; the opposite corner pixel NaN in
                 every slice: the map is 0 around it; slice 60 = 3e38 X, whose products overflow"""
    if name.startswith("repeats"):
        a, b = (int(t) for t in name.split("-")[1:])
        X, vol = _base(100 + a)
        vol[a] = vol[b] = X
    elif name == "negative":
        X, vol = _base(200)
        vol[NEGATIVE_D] = X - np.float32(5)
        for d, c in NEGATIVE_OTHERS:
            vol[d] = X - np.float32(c)
    elif name == "subnormal":
        X, vol = _base(300)
        vol[SUBNORMAL_D] = np.float32(1e-41)
        vol[SUBNORMAL_OTHER] = np.float32(2e-41)
    elif name == "nan":
        X, vol = _base(400)
        corner, patch = nan_pixels(s)
        vol[NAN_WINNER] = X - np.float32(5)
        vol[NAN_SECOND] = X - np.float32(2)
        vol[NAN_HUGE] = np.float32(3e38) * X
        vol[NAN_SLICE] = np.nan
        vol[NAN_WINNER][np.ix_(*patch)] = np.nan
        vol[(slice(None),) + np.ix_(*corner)] = np.nan
    else:
        raise ValueError(name)
    return vol
