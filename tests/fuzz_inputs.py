"""Seeded generators of geometries, image pairs and settings for the sweeps of the SGM and JointWMF stages
(tests/test_gpu_sgm_fuzz.py, tests/test_gpu_jwmf_fuzz.py; held to their own conditions by tests/test_fuzz_inputs.py).  Pure numpy,
no GPU; every function is a deterministic function of its arguments (an rng argument is consumed, nothing else is drawn from).

The content kinds aim at what smooth textured pairs never produce: exact ties of S (constant, shift, stripes), the largest path
costs the 16-bit condition admits (saturating), floats that are no byte / 255 (float_pair), JointWMF images on either side of the
identity / k-means switch and maps that leave whole radix digits empty."""
from __future__ import annotations

import numpy as np

from primestereomatch_amd import synth

# ------------------------------------------------------------------------------------------------------------------ SGM: geometries

EDGE_W = (8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 255, 256, 257)      # around SGM_TX = 32, SGM_BT_TX = 128
EDGE_H = (8, 9, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65)                                     # SGM_U = 8, 2 SGM_U, SGM_BT_YS = 32
EDGE_D = (2, 3, 4, 5, 60, 61, 62, 63, 64, 65, 66, 124, 125, 126, 127, 128, 129, 253, 254, 255, 256)
VOXELS = 600_000           # cap on W H D: sgm_model.sgm takes about 0.1 s there; 256 x 8 x 256 = 524288 must fit

# what a list must contain whatever the draw: (name, predicate on (W, H, D), the geometry appended when the draw has none)
REQUIRED = (
    ("D in 61..63 (ALL form, one disparity per lane, padding lanes)", lambda W, H, D: 61 <= D <= 63, (65, 17, 62)),
    ("D in 125..127 (ALL form, two per lane)", lambda W, H, D: 125 <= D <= 127, (129, 16, 126)),
    ("D in 253..255 (ALL form, four per lane)", lambda W, H, D: 253 <= D <= 255, (255, 9, 253)),
    ("H = 8", lambda W, H, D: H == 8, (33, 8, 5)),
    ("W = 8", lambda W, H, D: W == 8, (8, 17, 4)),
    ("W in 31..33", lambda W, H, D: 31 <= W <= 33, (32, 15, 3)),
    ("W in 127..129", lambda W, H, D: 127 <= W <= 129, (128, 9, 60)),
    ("H in 31..33", lambda W, H, D: 31 <= H <= 33, (17, 32, 2)),
    ("W in 16..17 (2 SGM_U: the main loop of a path runs once or not at all)", lambda W, H, D: 16 <= W <= 17, (16, 9, 4)),
    ("H in 16..17", lambda W, H, D: 16 <= H <= 17, (9, 16, 3)),
)


def sgm_geometries(n, seed, voxels=VOXELS):
    """-> list of (W, H, D, seed): n drawn geometries, D <= W always (W is raised to a larger D, so W = D occurs), W H D <= voxels,
    followed by one explicit geometry for every entry of REQUIRED the draw missed."""
    assert voxels >= 256 * 256 * 8                   # the smallest image with D = 256
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        W = int(rng.choice(EDGE_W)) if rng.random() < 0.6 else int(rng.integers(8, 300))
        H = int(rng.choice(EDGE_H)) if rng.random() < 0.6 else int(rng.integers(8, 80))
        D = int(rng.choice(EDGE_D)) if rng.random() < 0.5 else int(rng.integers(2, 97))
        W = max(W, D)
        if W * H * D > voxels:                       # rows go first: the widths and D carry more seams than the heights
            H = max(8, voxels // (W * D))
        if W * H * D > voxels:
            W = max(D, 8, voxels // (H * D))
        assert W * H * D <= voxels and 2 <= D <= min(W, 256)
        out.append((W, H, D, int(rng.integers(0, 1 << 30))))
    for _, has, (W, H, D) in REQUIRED:
        if not any(has(*g[:3]) for g in out):
            out.append((W, H, D, int(rng.integers(0, 1 << 30))))
    return out


# --------------------------------------------------------------------------------------------------------------------- SGM: content

SGM_KINDS = ("synth", "noise", "binary", "constant", "shift", "stripes", "half_flat", "saturating")


def saturating_pair(W, H, D, d_star, ch=3):
    """The right image alternates 0 and 255 by column, the left one is R[:, max(x - d_star, 0)]: the pixel cost is 0 for every d of
    d_star's parity and 255 ch for the other, at every pixel.  With block size 1 or 3 and P1 = P2 = 65535 - bs^2 ch 255 the losing
    parity's path costs climb by 255 ch bs^2 a step until P2 caps them at 65535: the model's S reaches 8 * 65535 = 524280, the
    largest value psm_sgm_set_params admits (test_fuzz_inputs.py asserts it for SATURATING_CASES)."""
    assert 0 <= d_star < D
    x = np.arange(W)
    row = ((x & 1) * 255).astype(np.uint8)
    r = np.broadcast_to(row[None, :, None], (H, W, ch))
    l = r[:, np.maximum(x - d_star, 0), :]
    if ch == 1:
        return np.ascontiguousarray(l[:, :, 0]), np.ascontiguousarray(r[:, :, 0])
    return np.ascontiguousarray(l), np.ascontiguousarray(r)


def saturating_params(bs, ch=3):
    return dict(block_size=bs, P1=65535 - bs * bs * ch * 255, P2=65535 - bs * bs * ch * 255)


# (W, H, D, d_star, block size): 1 disparity per lane three times, 4 per lane (NV = 4, partial form) once
SATURATING_CASES = ((200, 190, 2, 1, 1), (200, 190, 7, 3, 1), (200, 190, 6, 2, 3), (260, 190, 130, 5, 1))


def high_floor_pair(W, H, rng, span=32):
    """A dark left image (bytes below span) and a bright right one (bytes from 256 - span): every pixel cost is near 255 ch at every
    d.  With block size 7 the block costs lie around 147 * (255 - span) = 32781 and S = sum of 8 path costs >= 8 C around 2^18 -
    the MINIMUM of S over d is above 2^18 at most pixels and S straddles 2^18 at the others.  The saturating pairs reach the
    largest S but their winner's S is small; here the winner's own S needs the 19th bit of the packed key of k_sgm_select."""
    l = rng.integers(0, span, (H, W, 3), dtype=np.uint8)
    r = rng.integers(256 - span, 256, (H, W, 3), dtype=np.uint8)
    return l, r


HIGH_FLOOR_PARAMS = dict(block_size=7, P1=64, P2=65535 - 49 * 3 * 255)
HIGH_FLOOR_CASES = ((70, 24, 62), (40, 20, 9), (136, 12, 130))          # (W, H, D): ALL with padding lanes | partial | four per lane


def high_floor_case(W, H, D):
    return high_floor_pair(W, H, np.random.default_rng(D))


def _shifted(img, k):
    """img moved left by k columns, the last column replicated: L[x] = R[x - k] where both are inside"""
    W = img.shape[1]
    return np.ascontiguousarray(img[:, np.minimum(np.arange(W) + k, W - 1)])


def stripes_pair(W, H, D, p, k, rng):
    """Vertical stripes of period p (p distinct colours, every row the same), the right image the left one moved by k: away from
    the left edge the pixel costs at d and d + p are the same numbers."""
    levels = rng.permutation(np.arange(0, 256, 256 // (3 * p)))[:3 * p].reshape(p, 3).astype(np.uint8)
    l = np.ascontiguousarray(np.broadcast_to(levels[np.arange(W) % p][None], (H, W, 3)))
    return l, _shifted(l, k)


def sgm_content(kind, W, H, D, rng):
    """-> (l, r) uint8 [H][W][3] of one of SGM_KINDS"""
    if kind == "synth":
        l, r, _ = synth.make_pair(W, H, D, seed=int(rng.integers(0, 1 << 16)))
    elif kind == "noise":
        l, r = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    elif kind == "binary":
        l, r = (rng.integers(0, 2, (2, H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)
    elif kind == "constant":
        l = np.empty((H, W, 3), np.uint8)
        l[:] = rng.integers(0, 256, 3, dtype=np.uint8)
        r = l.copy()
    elif kind == "shift":
        l = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        r = _shifted(l, int(rng.integers(0, D)))
    elif kind == "stripes":
        # the shift k with k - p and k + p both inside [0, D) where D has room: S then ties at the two, neither of them the winner
        # by the missing neighbour of d = 0 or d = D - 1
        p = int(rng.choice([p for p in (2, 3, 4, 8) if 2 * p < D] or [2]))
        k = int(rng.integers(p, D - p)) if 2 * p < D else int(rng.integers(0, D))
        l, r = stripes_pair(W, H, D, p, k, rng)
    elif kind == "half_flat":
        l, r, _ = synth.make_pair(W, H, D, seed=int(rng.integers(0, 1 << 16)))
        ys = slice(0, H // 2) if rng.random() < 0.5 else slice(H // 2, H)
        xs = slice(0, W // 2) if rng.random() < 0.5 else slice(W // 2, W)
        l[ys, xs] = r[ys, xs] = rng.integers(0, 256, 3, dtype=np.uint8)
    elif kind == "saturating":
        l, r = saturating_pair(W, H, D, int(rng.integers(0, D)), 3)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(l), np.ascontiguousarray(r)


# (kind, W, H, D, seed) of test_ties_on_the_device: one D of each ALL-with-padding range the time cap allows there, and a small one
TIE_CASES = tuple((kind, W, H, D, 100 * i + D) for i, kind in enumerate(("constant", "shift", "stripes"))
                  for W, H, D in ((70, 24, 62), (140, 17, 126), (40, 33, 9)))


def tie_pair(kind, W, H, D, seed):
    return sgm_content(kind, W, H, D, np.random.default_rng(seed))


def sgm_settings(rng, bt=False):
    """-> (kw of the models, gray, (speckle window, speckle range)): the drawn parameters of one case.  kw holds pre_filter_cap
    when bt.  The bound on P2 is the 3-channel one for a gray pair too: psm_sgm_set_params checks it for the staged colour pair."""
    bs = int(rng.choice([1, 3, 5, 7]))
    gray = bool(rng.random() < 0.3)
    bound = 65535 - bs * bs * 3 * 255
    kw = dict(block_size=bs, uniqueness_ratio=int(rng.choice([0, 10, 50, 99])), disp12_max_diff=int(rng.choice([-1, 0, 1, 5])))
    mode = int(rng.integers(0, 3))
    if mode == 1:                                   # equal
        kw["P1"] = kw["P2"] = int(rng.integers(1, bound + 1))
    elif mode == 2:                                 # P2 at its bound
        kw["P1"], kw["P2"] = int(rng.integers(1, bound + 1)), bound
    if bt:
        kw["pre_filter_cap"] = int(rng.choice([1, 15, 16, 31, 63]))
    speckle = (int(rng.integers(1, 200)), int(rng.integers(0, 40))) if rng.random() < 0.3 else (0, 0)
    return kw, gray, speckle


# --------------------------------------------------------------------------------------------------------------------- float pairs

def half_products():
    """float32 values f with fl(f * 255.0f) = k + 0.5 exactly, one or more for each k in 0 .. 254 that has any: the neighbours of
    (k + 0.5) / 255 are searched.  rint sends them to the even neighbour, floor(x + 0.5) would send all of them up."""
    out = []
    for k in range(255):
        f = np.float32((k + 0.5) / 255.0)
        cand = [f]
        for direction in (np.float32(-np.inf), np.float32(np.inf)):
            g = f
            for _ in range(4):
                g = np.nextafter(g, direction)
                cand.append(g)
        out += [c for c in cand if np.float32(c) * np.float32(255.0) == np.float32(k + 0.5)]
    return np.array(sorted(set(out)), np.float32)


def float_image(img, rng, share=0.25):
    """u8 * (1 / 255.0f) with `share` of the elements replaced by values in [-0.3, 1.3], +-inf, -0.0, exact .5 products and NaN -
    at least one of each."""
    f = (img.astype(np.float32) * np.float32(1 / 255.0)).reshape(-1)
    halves = half_products()
    n = max(int(f.size * share), 12)
    idx = rng.permutation(f.size)[:n]
    what = rng.integers(0, 6, n)
    what[:12] = np.repeat(np.arange(6), 2)           # every class is there, whatever the draw
    vals = np.empty(n, np.float32)
    vals[:] = rng.uniform(-0.3, 1.3, n).astype(np.float32)
    vals[:2] = (-0.25, 1.25)                         # class 0 holds one below 0 and one above 1
    vals[what == 1] = np.float32(np.inf)
    vals[what == 2] = np.float32(-np.inf)
    vals[what == 3] = np.float32(-0.0)
    vals[what == 4] = halves[rng.integers(0, len(halves), int(np.count_nonzero(what == 4)))]
    vals[what == 5] = np.float32(np.nan)
    f[idx] = vals
    return f.reshape(img.shape)


def float_pair(l, r, rng):
    return float_image(l, rng), float_image(r, rng)


# ------------------------------------------------------------------------------------------------------------------------ JointWMF

JW_EDGE = (8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49)               # around JW_TILE = 16
JW_IMAGES = ("random", "palette_n", "palette_n1", "two", "synth")
JW_MAPS = ("random", "constant", "extremes", "nibble", "ramp")
JW_SIGMAS = (0.0, 0.05, 1e6)                                         # the default | cross-cluster weights 0 | weights near 2^48


def jwmf_cases(n, seed):
    """-> list of (W, H, radius, n_clusters, depth, (left, right) image kinds, (left, right) map kinds, sigma, seed).  The two
    sides get different kinds.  n_clusters is lowered where an image of n_clusters + 1 distinct keys would not fit the pixels.
    A float pair (depth "f32") is the byte pair * (1 / 255.0f); float_image's outliers go into the kinds whose key count does
    not matter (random, synth)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        W = int(rng.choice(JW_EDGE)) if rng.random() < 0.6 else int(rng.integers(8, 60))
        H = int(rng.choice(JW_EDGE)) if rng.random() < 0.6 else int(rng.integers(8, 60))
        radius = int(rng.integers(1, 17))
        nc = int(rng.choice([1, 2, 3, 16, 255, 256])) if rng.random() < 0.6 else int(rng.integers(1, 257))
        nc = min(nc, W * H - 1)
        depth = "f32" if rng.random() < 0.3 else "u8"
        ik = tuple(str(k) for k in rng.choice(JW_IMAGES, 2, replace=False))
        mk = tuple(str(k) for k in rng.choice(JW_MAPS, 2, replace=False))
        sigma = float(rng.choice(JW_SIGMAS))
        out.append((W, H, radius, nc, depth, ik, mk, sigma, int(rng.integers(0, 1 << 30))))
    return out


def _palette(n, W, H, rng):
    """An image with exactly n distinct 6-bit keys (n <= W H), the low two bits of every byte free."""
    keys = rng.choice(64 ** 3, n, replace=False)
    which = np.concatenate([np.arange(n), rng.integers(0, n, W * H - n)])
    k = keys[rng.permutation(which)].reshape(H, W)
    img = np.stack([k >> 12, (k >> 6) & 63, k & 63], axis=-1) * 4 + rng.integers(0, 4, (H, W, 3))
    return img.astype(np.uint8)


def jwmf_image(kind, W, H, n_clusters, rng):
    """-> uint8 [H][W][3] of one of JW_IMAGES"""
    if kind == "random":                              # from 40 x 40 on: more than 1024 keys (chunk = 2 in jw_seed)
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "palette_n":                           # the last image the identity takes
        return _palette(n_clusters, W, H, rng)
    if kind == "palette_n1":                          # the first image k-means takes
        return _palette(n_clusters + 1, W, H, rng)
    if kind == "two":
        return _palette(2, W, H, rng)
    if kind == "synth":
        return synth.make_pair(W, H, 8, seed=int(rng.integers(0, 1 << 16)))[0]
    raise ValueError(kind)


def jwmf_map(kind, W, H, rng):
    """-> uint8 [H][W] of one of JW_MAPS: the kinds other than random leave digits of the median's two radix passes empty."""
    if kind == "random":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W), int(rng.integers(0, 256)), np.uint8)
    if kind == "extremes":
        return (rng.integers(0, 2, (H, W), dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "nibble":                              # one high nibble: the first pass has one bin
        return (16 * int(rng.integers(0, 16)) + rng.integers(0, 16, (H, W))).astype(np.uint8)
    if kind == "ramp":
        yy, xx = np.mgrid[0:H, 0:W]
        return ((3 * xx + 5 * yy + int(rng.integers(0, 256))) % 256).astype(np.uint8)
    raise ValueError(kind)


def jwmf_build(case):
    """-> ((l, r) images in the case's depth, (lmap, rmap)) of one jwmf_cases tuple"""
    W, H, radius, nc, depth, ik, mk, sigma, seed = case
    rng = np.random.default_rng(seed)
    imgs = [jwmf_image(k, W, H, nc, rng) for k in ik]
    maps = [jwmf_map(k, W, H, rng) for k in mk]
    if depth == "f32":
        imgs = [float_image(im, rng, 0.05) if k in ("random", "synth") else im.astype(np.float32) * np.float32(1 / 255.0)
                for im, k in zip(imgs, ik)]
    return tuple(imgs), tuple(maps)


# -------------------------------------------------------------------------------------------- the case lists the sweeps run

FLOAT_CASES = ((67, 21, 16, 31), (131, 17, 62, 32), (33, 9, 33, 33))             # (W, H, D, seed)


def sad_cases():
    return sgm_geometries(40, 20261017)


def bt_cases():
    return sgm_geometries(30, 777001)


def sgm_case(W, H, D, seed, bt=False):
    """-> (kind, l, r, kw, gray, speckle) of one geometry: content and settings drawn from the geometry's own seed"""
    rng = np.random.default_rng(seed)
    kind = str(rng.choice(SGM_KINDS))
    l, r = sgm_content(kind, W, H, D, rng)
    kw, gray, speckle = sgm_settings(rng, bt)
    return kind, l, r, kw, gray, speckle


def sgm_batches(n, seed):
    """-> list of (W, H, D, kinds, seed): the contexts of a batch share a geometry and hold different content kinds; the first
    batch puts a saturating, a constant and a noise pair into one launch."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (W, H, D, s) in enumerate(sgm_geometries(n, seed, voxels=600_000)[:n]):
        m = int(rng.choice([1, 2, 3, 5]))
        kinds = tuple(str(k) for k in rng.choice(SGM_KINDS, m, replace=False))
        out.append((W, H, D, ("saturating", "constant", "noise") if i == 0 else kinds, s))
    return out


def sgm_batch_case(W, H, D, kinds, seed):
    """-> (pairs, kw, speckle): one pair per kind, the settings shared (a batch takes no gray pair)"""
    rng = np.random.default_rng(seed)
    pairs = [sgm_content(k, W, H, D, rng) for k in kinds]
    bt = bool(rng.random() < 0.5)
    while True:
        kw, gray, speckle = sgm_settings(rng, bt)
        if not gray:
            return pairs, kw, speckle


JW_MANY_KEYS = (50, 40, 4, 256, "u8", ("random", "synth"), ("random", "ramp"), 0.0, 1998)    # left: 1024 < keys < 2048


def jw_cases():
    """40 drawn cases; then, for every width and height of JW_EDGE, every radius 1 .. 16 and n_clusters 2, 3, 255 the draw missed, one
    more drawn case with that field set; then JW_MANY_KEYS."""
    cases = jwmf_cases(40, 4711)
    donors = iter(jwmf_cases(3 * len(JW_EDGE) + 16, 4712))
    wanted = [(0, v) for v in JW_EDGE] + [(1, v) for v in JW_EDGE] + [(2, v) for v in range(1, 17)] + [(3, v) for v in (2, 3, 255)]
    for field, v in wanted:
        if not any(c[field] == v for c in cases):
            d = list(next(donors))
            d[field] = v
            d[3] = min(d[3], d[0] * d[1] - 1)
            cases.append(tuple(d))
    return cases + [JW_MANY_KEYS]


def host_clusters(seed):
    """A clustering as a host would bring it: 1 .. 256 centres anywhere in the key cube, every key labelled at random."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 257))
    return (rng.random((n, 3)) * 63).astype(np.float32), rng.integers(0, n, 64 ** 3).astype(np.uint8)


def jwmf_batches(n, seed):
    """-> list of batches, each a list of (case, (host clusters on the left, on the right)): 2 to 4 contexts of one geometry,
    radius, n_clusters, depth and sigma, with image and map kinds of their own.  The first batch: an identity pair beside a pair
    that needs k-means beside a pair with host clusters on both sides."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        W, H, radius, nc, depth, _, _, sigma, _ = jwmf_cases(1, int(rng.integers(0, 1 << 30)))[0]
        if i == 0:
            W, H, nc = 33, 17, 16
            kinds = [(("palette_n", "two"), (False, False)), (("random", "palette_n1"), (False, False)), (("random", "synth"), (True, True))]
        else:
            kinds = [(tuple(str(k) for k in rng.choice(JW_IMAGES, 2, replace=False)), (bool(rng.random() < 0.25), bool(rng.random() < 0.25)))
                     for _ in range(int(rng.integers(2, 5)))]
        batch = []
        for ik, host in kinds:
            mk = tuple(str(k) for k in rng.choice(JW_MAPS, 2, replace=False))
            batch.append(((W, H, radius, nc, depth, ik, mk, sigma, int(rng.integers(0, 1 << 30))), host))
        out.append(batch)
    return out
