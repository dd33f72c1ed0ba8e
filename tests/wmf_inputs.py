"""Seeded generators of adversarial inputs for the weighted median post-filter (tests/test_gpu_wmf_adversarial.py; held to their
own conditions by tests/test_wmf_inputs.py).  Pure numpy + tests/wmf_model.py, no GPU; every generator is a deterministic function of
its arguments and returns a WmInput: (img, lmap, rmap, lvalid, rvalid, pixels).  img is uint8 [2][H][W][3]: img[0] the left image,
img[1] the right one - the right map is weighted with the right image's colours, so a generator that places colours places them
in both.  pixels = (left, right), int [n, 2] arrays of (y, x): the pixels a generator has proven to have its property (empty
where it claims none).  Map values are < D everywhere (anything else is out of bounds in the reference).  The arrays of a cached
result are read-only.

What the inputs are for:
* knife_edge       - windows whose two voting bins have equal real-number sums: the result depends on the ORDER of the fp32 additions;
* denormal_windows - windows whose every voting weight is a denormal (or 0): the result depends on denormals being kept;
* domino           - chains of pixels each of which flips only after its left neighbours: many sweeps to the fixed point;
* zero_windows     - windows without a vote (sumWgt = 0, halfWgt = 0, result 0);
* counted_invalid  - an exact number of invalid pixels per side (the seams of the launch decisions);
* wm_geometries    - small images whose window wraps onto itself, D around the word seams of the histogram."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import wmf_model as M

CELL = 20                    # one invalid pixel per CELL x CELL pixels: the 19 x 19 windows of two cells share no pixel
GAP = 10                     # valid rows after the bulk rows: bulk pixels stay more than 9 rows from every cell, through the wrap too
L_MAX = 120                  # levels searched for the corner tap of a knife-edge window
FLAT = (0, 0, 100)           # the flat colour of the knife-edge images (a channel at 0: a colour at distance >= 1 exists)
FAR = (255, 255, 100)        # squared distance 2 from FLAT: weight exp(-200 - ...) = 0
TAP_FIRST, TAP_LAST = 0, M.TAPS - 1          # taps (-9, -9) and (9, 9)
NO_PIXELS = np.zeros((0, 2), np.int64)


class WmInput(NamedTuple):
    img: np.ndarray
    lmap: np.ndarray
    rmap: np.ndarray
    lvalid: np.ndarray
    rvalid: np.ndarray
    pixels: tuple


def to_f32(img_u8):
    """convertTo(CV_32F, 1 / 255.0f), as oracle.u8_to_f32"""
    return img_u8.astype(np.float32) * np.float32(1 / 255.0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _finish(img, lmap, rmap, lvalid, rvalid, D, pixels=(NO_PIXELS, NO_PIXELS)):
    assert img.dtype == np.uint8 and img.shape == (2,) + lmap.shape + (3,)
    for m, v in ((lmap, lvalid), (rmap, rvalid)):
        assert m.dtype == np.uint8 and v.dtype == np.uint8 and m.shape == v.shape == lmap.shape
        assert int(m.max()) < D, "map value out of the histogram"
    _frozen(img, lmap, rmap, lvalid, rvalid, *pixels)
    return WmInput(img, lmap, rmap, lvalid, rvalid, tuple(pixels))


def smooth_image(H, W, rng):
    """piecewise-constant colours + small noise: colour weights that are not all ~0"""
    base = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3))
    return np.clip(np.kron(base, np.ones((8, 8, 1)))[:H, :W] + rng.integers(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8)


def cell_centres(H, W):
    """-> [n, 2] (y, x): the centres of the cells, every window inside the image (no wrap)"""
    return np.array([(y, x) for y in range(CELL // 2, H - M.R, CELL) for x in range(CELL // 2, W - M.R, CELL)], np.int64)


def _with_bulk(H, W, D, bulk_rows, rng, img, maps, valids):
    """Appends bulk_rows rows of random invalid pixels (about 85 %) on smooth colours with random values, then GAP valid rows."""
    if not bulk_rows:
        return img, maps, valids
    HH = H + bulk_rows + GAP
    big = np.empty((2, HH, W, 3), np.uint8)
    big[:, :H] = img
    big[0, H:] = smooth_image(HH - H, W, rng)
    big[1, H:] = np.roll(big[0, H:], 3, axis=1)
    out_m, out_v = [], []
    for m, v in zip(maps, valids):
        mm = np.concatenate([m, rng.integers(0, D, (HH - H, W)).astype(np.uint8)])
        vv = np.ones((HH, W), np.uint8)
        vv[:H] = v
        vv[H:H + bulk_rows] = rng.random((bulk_rows, W)) > 0.85
        assert int((vv[H:] == 0).sum()) >= 8192, "the bulk rows must carry the lane form"
        out_m.append(mm)
        out_v.append(vv)
    return big, out_m, out_v


@functools.lru_cache(maxsize=None)
def knife_edge(H, W, D, seed, bulk_rows=0):
    """One isolated invalid pixel (own value 0: no vote) per cell on a flat image.  Its window holds two values a < b, tap (wy, wx)
    one of them and tap (-wy, -wx) the other: the weights are point-symmetric, so both bins have the same sum in real numbers and
    the result (a if fl(S_a) >= fl(total) / 2, else b) is decided by rounding - by the order of the additions.  Where that alone
    does not make the raster result differ from another order's (the left formula: the total has twice the magnitude and S_a
    stays a few ulp below half) the corner pair (+-9, +-9) is taken out of the balance: tap (9, 9) gets a colour at distance
    >= 1 (weight 0), tap (-9, -9) a third, smallest value c and a colour L levels from the centre's, so it adds a small e to the
    total and e to the running sum ahead of S_a, moving the margin by e / 2; L is searched per window with the model.
    pixels: the centres whose result differs between raster order and at least one other order of wmf_model.ORDERS."""
    assert D >= 4 and H >= CELL and W >= CELL
    rng = np.random.default_rng(seed)
    cen = cell_centres(H, W)
    n = len(cen)
    img = np.empty((2, H, W, 3), np.uint8)
    img[:] = FLAT
    maps, valids, listed = [], [], []
    flat3 = to_f32(np.array(FLAT, np.uint8))
    cand = np.arange(L_MAX + 1)                                         # candidate 0: the plain antisymmetric window
    near = to_f32(np.stack([cand, np.zeros_like(cand), np.full_like(cand, FLAT[2])], axis=1).astype(np.uint8))
    for side in (0, 1):
        # c < a < b of every cell: its own three values (the bins lie in one 64-bin word or in several)
        c, a, b = np.sort(np.stack([rng.choice(np.arange(1, D), 3, replace=False) for _ in range(n)]), axis=1).T
        dmap = rng.integers(1, D, (H, W)).astype(np.uint8)
        valid = np.ones((H, W), np.uint8)
        # the windows: taps t and 360 - t hold a and b in a random orientation, the centre 0
        deps = np.zeros((M.TAPS, n), np.int64)
        coin = rng.random((M.TAPS // 2, n)) < 0.5
        deps[:M.TAPS // 2] = np.where(coin, a[None], b[None])
        deps[M.TAPS // 2 + 1:] = np.where(coin, b[None], a[None])[::-1]
        # all candidates of all cells in one evaluation per order
        w0 = M.colour_weights(flat3, flat3, M._WY, M._WX, side)                         # [361]
        wts = np.repeat(w0[:, None], n * len(cand), axis=1).reshape(M.TAPS, n, len(cand)).copy()
        dd = np.repeat(deps[:, :, None], len(cand), axis=2)
        wts[TAP_FIRST, :, 1:] = M.colour_weights(flat3, near[1:], -M.R, -M.R, side)[None]
        wts[TAP_LAST, :, 1:] = M.colour_weights(flat3, to_f32(np.array(FAR, np.uint8)), M.R, M.R, side)
        dd[TAP_FIRST, :, 1:] = c[:, None]
        res = {o: M.median_of(wts.reshape(M.TAPS, -1), dd.reshape(M.TAPS, -1), o).reshape(n, len(cand)) for o in M.ORDERS}
        # the candidate that tells most orders from raster order (the first of them), else plain; a balanced tree differs from any
        # sequential order in most windows as they are, a reversed walk only near the margin
        sens = sum((res[o] != res["raster"]).astype(np.int64) for o in M.ORDERS[1:])
        level = np.argmax(sens, axis=1)
        for k, (y, x) in enumerate(cen):
            win = deps[:, k].reshape(2 * M.R + 1, 2 * M.R + 1).astype(np.uint8)
            if level[k]:
                win[0, 0] = c[k]
                img[side, y - M.R, x - M.R] = (level[k], FLAT[1], FLAT[2])
                img[side, y + M.R, x + M.R] = FAR
            dmap[y - M.R:y + M.R + 1, x - M.R:x + M.R + 1] = win
            valid[y, x] = 0
        maps.append(dmap)
        valids.append(valid)
    img, maps, valids = _with_bulk(H, W, D, bulk_rows, rng, img, maps, valids)
    for side in (0, 1):                                                 # the proof, on the finished image and map
        f = to_f32(img[side])
        res = {o: M.evaluate(f, maps[side], cen, D, side, o) for o in M.ORDERS}
        keep = np.zeros(n, bool)
        for o in M.ORDERS[1:]:
            keep |= res[o] != res["raster"]
        listed.append(cen[keep].copy())
    return _finish(img, maps[0], maps[1], valids[0], valids[1], D, listed)


@functools.lru_cache(maxsize=None)
def denormal_windows(H, W, D, seed, bulk_rows=0):
    """The grid of knife_edge; every image value is 0 .. 5 levels except the centres, whose colour is drawn from (244 .. 255,
    0 .. 39, 0 .. 39) until the model says that every voting weight of the window is a denormal or 0 (for the right formula:
    after its two roots) and that the result changes when denormals are flushed.  The windows hold random values 1 .. D - 1.
    pixels: all centres (the generator fails if a centre cannot be made to qualify)."""
    assert D >= 2
    rng = np.random.default_rng(seed)
    cen = cell_centres(H, W)
    n = len(cen)
    img = rng.integers(0, 6, (2, H, W, 3)).astype(np.uint8)
    maps, valids = [], []
    for side in (0, 1):
        dmap = rng.integers(1, D, (H, W)).astype(np.uint8)
        valid = np.ones((H, W), np.uint8)
        dmap[cen[:, 0], cen[:, 1]] = 0
        valid[cen[:, 0], cen[:, 1]] = 0
        todo = np.arange(n)
        for _ in range(50):
            col = np.stack([rng.integers(244, 256, len(todo)), rng.integers(0, 40, len(todo)), rng.integers(0, 40, len(todo))], axis=1)
            img[side, cen[todo, 0], cen[todo, 1]] = col
            q, wts = M.window(to_f32(img[side]), cen[todo], side)
            deps = dmap.reshape(-1)[q]
            small = (np.where(deps != 0, wts, 0) < M.F32_MIN).all(axis=0)
            differs = M.median_of(wts, deps) != M.median_of(wts, deps, flush=True)
            todo = todo[~(small & differs)]
            if len(todo) == 0:
                break
        assert len(todo) == 0, "no qualifying centre colour found"
        maps.append(dmap)
        valids.append(valid)
    img, maps, valids = _with_bulk(H, W, D, bulk_rows, rng, img, maps, valids)
    return _finish(img, maps[0], maps[1], valids[0], valids[1], D, (cen.copy(), cen.copy()))


def _row_colours(H):
    """H colours (H <= 27) from {0, 128, 255}^3: squared distance >= 0.248 between any two - weights below e^-24 across rows"""
    assert H <= 27
    lv = np.array([0, 128, 255])
    order = np.random.default_rng(H).permutation(27)[:H]
    return np.stack([lv[order // 9], lv[(order // 3) % 3], lv[order % 3]], axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def domino(H, W, period, seed_len, a, b, D=16):
    """Every row has a colour of its own, far from the others': the rows do not see each other.  Value b at every period-th column and
    in the first seed_len columns, valid; value a < b everywhere else, invalid.  An invalid pixel turns b once enough of its
    left neighbours have - in raster order all of them, in one pass; a sweep that sees only the previous sweep's map moves the
    front a few columns.  Both sides get the same image and map (the two formulas move the front at different speeds)."""
    assert 0 < a < b < D and seed_len >= M.R and H >= M.R and W >= 2 * M.R + 1
    img = np.empty((2, H, W, 3), np.uint8)
    img[:] = _row_colours(H)[None, :, None, :]
    x = np.arange(W)
    is_b = (x % period == 0) | (x < seed_len)
    dmap = np.broadcast_to(np.where(is_b, b, a).astype(np.uint8), (H, W)).copy()
    valid = np.broadcast_to(is_b.astype(np.uint8), (H, W)).copy()
    return _finish(img, dmap, dmap.copy(), valid, valid.copy(), D)


BLOCK = 32                   # zero regions are whole blocks, larger than a window


def _votes(dmap):
    """-> per pixel, the number of non-zero values in its (wrapped) window"""
    nz = (dmap != 0).astype(np.int64)
    return sum(np.roll(np.roll(nz, wy, axis=0), wx, axis=1) for wy in range(-M.R, M.R + 1) for wx in range(-M.R, M.R + 1))


@functools.lru_cache(maxsize=None)
def zero_windows(H, W, D, seed):
    """Blocks of BLOCK x BLOCK pixels of three kinds: non-zero (random values 1 .. D - 1), zero, and guarded zero - zero with its outer 9
    pixels valid.  Valid and invalid pixels are mixed half and half everywhere else, on smooth colours.  In a plain zero block the
    in-place recursion carries non-zero values inwards from its border (a filtered pixel is the only voter of the next one);
    in the core of a guarded block an invalid pixel never sees a voter: sumWgt = 0, halfWgt = 0, result 0.  Block (0, 0) is
    guarded, block (0, 1) non-zero and block (1, 0) plain zero, whatever the draw.
    pixels: the invalid pixels whose window holds no vote in the input and none at the fixed point of the recursion (the model's)."""
    assert D >= 2 and H >= 2 * BLOCK and W >= 2 * BLOCK
    rng = np.random.default_rng(seed)
    img = np.stack([smooth_image(H, W, rng), smooth_image(H, W, rng)])
    out_m, out_v, listed = [], [], []
    yy, xx = np.mgrid[0:H, 0:W]
    rim = (np.minimum(yy % BLOCK, BLOCK - 1 - yy % BLOCK) < M.R) | (np.minimum(xx % BLOCK, BLOCK - 1 - xx % BLOCK) < M.R)
    for side in (0, 1):
        kind = rng.integers(0, 3, (H // BLOCK + 1, W // BLOCK + 1))             # 0 non-zero | 1 zero | 2 guarded zero
        kind[0, 0], kind[0, 1], kind[1, 0] = 2, 0, 1
        kmap = np.kron(kind, np.ones((BLOCK, BLOCK), np.int64))[:H, :W]
        dmap = np.where(kmap != 0, 0, rng.integers(1, D, (H, W))).astype(np.uint8)
        valid = ((rng.random((H, W)) < 0.5) | ((kmap == 2) & rim)).astype(np.uint8)
        n, fixed = M.jacobi_sweeps(to_f32(img[side]), dmap, valid, D, side, cap=1000)
        assert n > 0
        listed.append(np.argwhere((_votes(dmap) == 0) & (_votes(fixed) == 0) & (valid == 0)))
        out_m.append(dmap)
        out_v.append(valid)
    return _finish(img, out_m[0], out_m[1], out_v[0], out_v[1], D, listed)


@functools.lru_cache(maxsize=None)
def counted_invalid(H, W, D, seed, n_left, n_right, map_seed=None):
    """Random values on smooth colours with exactly n_left / n_right invalid pixels at random places.  The images are drawn from
    seed; the maps and the places from map_seed where one is given (several inputs for one image pair)."""
    rng = np.random.default_rng(seed)
    left = smooth_image(H, W, rng)
    img = np.stack([left, np.roll(left, 4, axis=1)])
    if map_seed is not None:
        rng = np.random.default_rng(map_seed)
    maps = [rng.integers(0, D, (H, W)).astype(np.uint8) for _ in (0, 1)]
    valids = []
    for n in (n_left, n_right):
        assert 0 <= n <= H * W
        v = np.ones(H * W, np.uint8)
        v[rng.permutation(H * W)[:n]] = 0
        valids.append(v.reshape(H, W))
    return _finish(img, maps[0], maps[1], valids[0], valids[1], D)


# ------------------------------------------------------------------------------------------------------------------- geometries

EDGE_WH = (9, 10, 18, 19, 20, 21, 64, 65)          # the window wraps onto itself below 19; pixels with no wrap in x from W = 20
EDGE_D = (2, 3, 63, 64, 65, 128, 129, 191, 192, 193, 255, 256)          # around the 64-bin words of the wave form's histogram
FRACS = (0.02, 0.5, 1.0)
FORMS = {"sweeps": 0, "no_cache": 16777216, "dataflow": 4194304, "fallback": 8388608}          # PSM_OPT_FLAGS of the four forms

# what a list must contain whatever the draw: (name, predicate on (W, H, D), the geometry appended when the draw has none)
REQUIRED = (
    ("W = 9 and H = 9 (the smallest image the filter takes)", lambda W, H, D: W == 9 and H == 9, (9, 9, 5)),
    ("W = 19 (no pixel whose window stays inside its row)", lambda W, H, D: W == 19, (19, 12, 19)),
    ("W = 20 (exactly one such column)", lambda W, H, D: W == 20, (20, 21, 3)),
    ("D in 65..128 (two words)", lambda W, H, D: 65 <= D <= 128, (70, 10, 65)),
    ("D in 129..192 (three words)", lambda W, H, D: 129 <= D <= 192, (192, 9, 129)),
    ("D in 193..256 (four words)", lambda W, H, D: 193 <= D <= 256, (200, 10, 193)),
    ("D = 2", lambda W, H, D: D == 2, (21, 18, 2)),
)


def wm_geometries(n, seed):
    """-> list of (W, H, D, invalid fraction, form, seed): n drawn cases, W and H >= 9, 2 <= D <= min(W, 256) (a D above the drawn W
    raises W to it or is drawn again among 2, 3 and W), followed by one case for every entry of REQUIRED the draw missed."""
    rng = np.random.default_rng(seed)
    out = []

    def case(W, H, D):
        return (W, H, D, float(rng.choice(FRACS)), str(rng.choice(sorted(FORMS))), int(rng.integers(0, 1 << 30)))

    for _ in range(n):
        W = int(rng.choice(EDGE_WH)) if rng.random() < 0.7 else int(rng.integers(9, 70))
        H = int(rng.choice(EDGE_WH)) if rng.random() < 0.7 else int(rng.integers(9, 70))
        D = int(rng.choice(EDGE_D)) if rng.random() < 0.7 else int(rng.integers(2, 257))
        if D > W:
            if rng.random() < 0.5:
                W = D
            else:
                D = int(rng.choice([2, 3, W]))
        assert 2 <= D <= min(W, 256) and W >= 9 and H >= 9
        out.append(case(W, H, D))
    for _, has, (W, H, D) in REQUIRED:
        if not any(has(*g[:3]) for g in out):
            out.append(case(W, H, D))
    return out


@functools.lru_cache(maxsize=None)
def random_case(W, H, D, frac, seed):
    """All-random content of one wm_geometries case: unrelated colours at every pixel on the left, smooth ones on the right."""
    rng = np.random.default_rng(seed)
    img = np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), smooth_image(H, W, rng)])
    maps = [rng.integers(0, D, (H, W)).astype(np.uint8) for _ in (0, 1)]
    valids = [(rng.random((H, W)) >= frac).astype(np.uint8) for _ in (0, 1)]
    return _finish(img, maps[0], maps[1], valids[0], valids[1], D)


# ------------------------------------------------------------------------------------------- the cases the device tests run

# (H, W, D): 4 x 10 cells at one and three words of bins; four words need W >= D = 256 (psm_create refuses D > W): 4 x 13 cells
KNIFE_CASES = ((90, 210, 64), (90, 210, 129), (90, 270, 256))
BULK_ROWS = 48                                            # 48 x 210 x 0.85 = 8568 invalid pixels expected
DOMINO_CASES = {                                          # name -> (H, W, period, seed_len, a, b)
    "wave_9x800": (9, 800, 4, 12, 3, 7),                  # fewer than 8192 invalid pixels: the wave form
    "lane_12x1200": (12, 1200, 3, 12, 3, 7),              # more: the lane form
}
DOMINO_CONTROL = (9, 400, 2, 12, 3, 7)                    # period 2: b holds the majority at once, no chain
COUNTS = ((8191, 8191), (8192, 8192), (8193, 8193), (8256, 8256), (8257, 8257), (8191, 8193), (0, 8192))
COUNTED_GEO = (111, 233, 80)
ZERO_GEO = (80, 110)                                      # 2.5 x 3.4 blocks: cropped blocks at both far edges


def geometry_cases():
    return wm_geometries(24, 20261017)
