"""A shadow of the context (include/primesm_hip.h: what a psm_ctx holds between two calls) and a seeded generator of call
sequences over three contexts of one geometry - plain Python and numpy, no device, nothing of the library but its constants.

The shadow is the statement of the header's state promises ("may be called anywhere between them", "afterwards the context is
exactly where psm_upload_maps leaves it", "a later psm_disp_select yields the guided-filter maps again", "every context ends
where its own single call would have left it", "the previous result stays readable"): every op is a function of the shadow that
says what the call does to it or that the call is refused and nothing changes, and every reader says which bytes the context
must hand out afterwards.  tests/test_seq_model.py holds the generator to its conditions on the CPU; tests/test_gpu_sequences.py
replays the same walks on real contexts.

Two levels.  The shadow is SYMBOLIC: maps, masks, SGM results, clusterings and score records are expressions (hashable tuples
such as ("fill", ("gf", 1, "f32"), ("lr", ("gf", 1, "f32")))), so a walk is generated and replayed in microseconds.  Refs turns an
expression into bytes with the CPU definitions - the oracle (oracle/psm_oracle_py.py) for the guided-filter path, the L-R check,
the fill and the weighted median, tests/sgm_*_model.py, speckle_model.py, sgm_maps_model.py, jwmf_model.py, score_model.py and
rectify_model.py for the rest - and keeps every value for the session, keyed by its expression.  Nothing comes from the device.

Narrower than the calls allow: after psm_upload_volume of a few slices the shadow only knows that maps, mask and the filtered
result are gone and lets nothing but new costs follow (a filter of the patched volume has no one-call CPU definition here);
psm_download_volume is not read (both shapes have more than 16 slices; tests/test_gpu_parity.py and test_gpu_fuzz.py read
volumes); a second filter of a filtered volume and a select of unfiltered costs are defined by the library but not generated.

Two vocabularies.  generate(seed) deals the walks of SEEDS from OP_KINDS, as ever.  generate(seed, vocabulary="tail") deals the
walks of TAIL_SEEDS from TAIL_KINDS: the WLS stage, the reprojection stage, psm_post_process_batch, the hook plane of
psm_score_upload_sgm_map and psm_sgm_compute_gray, with the older calls their state depends on (pairs of every kind, the SGM
stage, the guided-filter frame, the post-processing stages, psm_release_scratch, the score stage).  What decides which int16 map,
which invalid value and which left image those stages read (psm_ctx.h: sgm_stage_map, sgm_source_map, colour_of) is stated once,
in World._stage_map, _source_map and _guide.  Not in the tail vocabulary: row stripes and disparity shards (the new stages refuse
stripe-only maps; test_gpu_wls.py and test_gpu_depth.py hold that refusal), psm_share_streams, the caller's map buffer,
JointWMF, and asynchronous batches."""
from __future__ import annotations

import numpy as np

# enum psm_flag / psm_score sources (include/primesm_hip.h; primestereomatch_amd/capi.py holds the same constants)
MATERIALISE, STORE = 128, 8192
TWO_PHASE_ON, TWO_PHASE_OFF = 1048576, 2097152
GIF, SGM, SGM_INT = 0, 1, 2

SHAPES = ((72, 40, 24), (130, 24, 20))      # W, H, D: one column group; two column groups in the narrow layout, H below a segment
NCTX = 3
NPAIRS = 4                                  # pairs 0 .. 2 are uploaded as they are, pair RECT is a rectified camera frame
RECT = 3
SRC = (90, 50)                              # the eye images of the camera frame (src_w, src_h)
FLAGS_SAFE = (0, TWO_PHASE_ON, TWO_PHASE_OFF)                       # compatible with row stripes
FLAGS_ANY = FLAGS_SAFE + (MATERIALISE, STORE, STORE | MATERIALISE)
MODES = ("sgbm", "hh", "3way", "hh4")
STEPS = 40

WLS_DEFAULT = (8000.0, 1.5, 3)                  # lambda, sigma, iterations of a new context
# the parameters a wls_params op draws from: the defaults; a large lambda with a large sigma; a tiny sigma (most links are cut: void
# pixels exist wherever a hole is walled in); then every other iteration count
WLS_PARAMS = (WLS_DEFAULT, (4.0e6, 250.0, 3), (30.0, 0.02, 3), (8000.0, 1.5, 1), (500.0, 4.0, 2), (60.0, 0.02, 4), (4.0e6, 250.0, 2), (500.0, 4.0, 4))
XYZ, Z, CLOUD = 1, 2, 4                          # PSM_DEPTH_*
LR, FILL, WM = 1, 2, 4                           # PSM_PP_*
PP_STAGES = (LR, LR | FILL, LR | FILL | WM, FILL)
# what a reproject_q op draws from.  Q 0: the Q of cv::stereoRectify for two cameras whose principal points differ, with a crop; Q 1:
# equal principal points (CALIB_ZERO_DISPARITY), so s_3 == 0 at disparity 0 and those pixels are void.  z-range 1 drops near and far.
Q_CROPS = ((3, 2), (0, 0))
Z_RANGES = ((0.0, float(np.finfo(np.float32).max)), (3600.0, 9000.0))


def q_matrix(qi):
    import depth_model as DM
    P1 = [[700.0, 0, 30.0, 0], [0, 700.0, 20.0, 0], [0, 0, 1, 0]]
    P2 = [[700.0, 0, 33.0 if qi == 0 else 30.0, -84000.0], [0, 700.0, 20.0, 0], [0, 0, 1, 0]]
    return DM.q_from_projections(P1, P2)


MAP_WRITERS = ("sgbm_select", "sgbm_select_batch", "upload_maps", "mapbuf", "gather", "merge")      # ... other than the filter
JWMF_OPS = ("jwmf", "jwmf_batch")


# ------------------------------------------------------------------------------------------------------------------- inputs

class Data:
    """The inputs of one walk, a function of (shape, seed) alone: image pairs, the camera frame behind pair RECT with its random
    rectification maps, two ground truths."""

    def __init__(self, shape, seed):
        import rectify_model as RM
        self.W, self.H, self.D = W, H, D = shape
        rng = np.random.default_rng([seed, W, H, D])
        self.pairs = [self._pair(rng) for _ in range(NPAIRS - 1)]
        sw, sh = SRC
        self.crop = (3, 2, W, H)
        mw, mh = W + 5, H + 4
        self.map_xy = tuple(np.stack([rng.integers(-3, sw + 3, size=(mh, mw)), rng.integers(-3, sh + 3, size=(mh, mw))], -1).astype(np.int16)
                            for _ in range(2))
        self.map_frac = tuple(rng.integers(0, 1024, size=(mh, mw)).astype(np.uint16) for _ in range(2))
        eyes = [rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8) for _ in range(2)]
        self.frame = np.ascontiguousarray(np.concatenate(eyes, axis=1))
        self.pairs.append(tuple(np.ascontiguousarray(RM.remap_u8(e, xy, fr, self.crop)) for e, xy, fr in zip(eyes, self.map_xy, self.map_frac)))
        self.truths = []
        for t in range(2):
            gt = rng.integers(0, 4 * D, size=(H, W)).astype(np.uint8)
            mask = np.where(rng.random((H, W)) < 0.8, 255, rng.integers(0, 255, size=(H, W))).astype(np.uint8) if t == 0 else None
            self.truths.append((gt, mask))
        for p in self.pairs:
            for a in p:
                a.setflags(write=False)

    def _pair(self, rng):
        """A textured left image and the right one as its shift by a disparity that differs between two bands, plus noise."""
        W, H, D = self.W, self.H, self.D
        coarse = rng.integers(0, 256, size=(H // 4 + 2, W // 4 + 2, 3))
        l = np.kron(coarse, np.ones((4, 4, 1), np.int64))[:H, :W] + rng.integers(-12, 13, size=(H, W, 3))
        l = np.clip(l, 0, 255).astype(np.uint8)
        r = np.empty_like(l)
        d0, d1 = int(rng.integers(1, D // 2)), int(rng.integers(D // 2, D - 1))
        for y in range(H):
            d = d0 if y < H // 2 else d1
            r[y] = np.roll(l[y], -d, axis=0)
        r = np.clip(r.astype(np.int64) + rng.integers(-3, 4, size=r.shape), 0, 255).astype(np.uint8)
        return np.ascontiguousarray(l), np.ascontiguousarray(r)

    def float_pair(self, k):
        """Pair k as the float images StereoMatch::compute hands over: byte * (1 / 255.0f)."""
        return tuple(a.astype(np.float32) * np.float32(1 / 255.0) for a in self.pairs[k])

    def gray(self, k):
        """The one-channel pair of an sgbm_gray op: the green planes of pair k."""
        return tuple(np.ascontiguousarray(a[..., 1]) for a in self.pairs[k])


def rand_maps(W, H, D, mseed):
    """The bytes of an upload_maps op: (lmap, rmap, lvalid, rvalid)."""
    rng = np.random.default_rng([mseed, 77])
    l, r = rng.integers(0, D, size=(2, H, W)).astype(np.uint8)
    lv, rv = (rng.random((2, H, W)) < 0.8).astype(np.uint8)
    return l, r, lv, rv


def rand_d16(W, H, D, mseed):
    """The caller's int16 map of a filter_speckles op: blocks of equal values with holes of the invalid value."""
    rng = np.random.default_rng([mseed, 78])
    m = np.kron(rng.integers(0, 16 * D, size=(H // 3 + 1, W // 3 + 1)), np.ones((3, 3), np.int64))[:H, :W]
    m = np.where(rng.random((H, W)) < 0.15, -16, m)
    return np.ascontiguousarray(m.astype(np.int16))


# ------------------------------------------------------------------------------------------------------- expected values

class Refs:
    """Expression -> bytes, by the CPU definitions; every value is computed once per session (the cache is keyed by the
    expression, which names its inputs completely)."""
    _cache: dict = {}

    def __init__(self, data: Data, oracle, key):
        self.d, self.O, self.key = data, oracle, key

    def __call__(self, e):
        k = (self.key, e)
        if k not in Refs._cache:
            v = getattr(self, "_" + e[0])(*e[1:])
            for a in (v if isinstance(v, tuple) else v.values() if isinstance(v, dict) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            Refs._cache[k] = v
        return Refs._cache[k]

    # maps: (left, right)
    def _gf(self, k, dtype):
        ref = (self.O.pipeline_u8 if dtype == "u8" else self.O.pipeline_f32)(*self.d.pairs[k], self.d.D, threads=4)
        return ref["ldisp"], ref["rdisp"]

    def _fgf(self, k, s):
        ref = self.O.pipeline_fgf(*self.d.pairs[k], self.d.D, s=s, threads=4)
        return ref["ldisp"], ref["rdisp"]

    def _up(self, mseed):
        return rand_maps(self.d.W, self.d.H, self.d.D, mseed)[:2]

    def _sgmaps(self, sgm):
        import sgm_maps_model as MM
        dmin, nd = sgm_range(sgm, self.d.D)
        return MM.maps(self(sgm)["S"], dmin, self.d.D)

    def _fill(self, maps, mask):
        return tuple(self.O.fill_inv(m, v) for m, v in zip(self(maps), self(mask)))

    def _wm(self, maps, mask, k):
        return tuple(self.O.wgt_median(self.O.u8_to_f32(np.ascontiguousarray(img)), m, v, self.d.D, right=bool(s))
                     for s, (img, m, v) in enumerate(zip(self.d.pairs[k], self(maps), self(mask))))

    def _jw(self, maps, k, radius):
        import jwmf_model as J
        out = []
        for s, (img, m) in enumerate(zip(self.d.pairs[k], self(maps))):
            cen, lok, _ = self(("cl", k, s))
            out.append(J.joint_wmf(m, img, radius, clusters=(cen, lok)))
        return tuple(out)

    # masks: (left, right)
    def _lr(self, maps):
        return tuple(self.O.lr_check(*self(maps)))

    def _upmask(self, mseed):
        return rand_maps(self.d.W, self.d.H, self.d.D, mseed)[2:]

    # the SGM stage
    def _sgm(self, k, cost, mode, dmin, nd, spk):
        import sgm_census_model as CM
        import speckle_model as K
        kw = {"census": cost[1:]} if cost[0] == "census" else {"census": None, "pre_filter_cap": cost[1] if cost[0] == "bt" else 0}
        pair = self.d.gray(k[1]) if isinstance(k, tuple) else self.d.pairs[k]          # ("g", k): psm_sgm_compute_gray
        ref = CM.sgm(*pair, dmin, nd or self.d.D, mode=mode, **kw)
        disp, sizes = ref["disp"], None
        if spk[0] > 0:
            disp, sizes = K.filter_speckles(ref["disp"], ref["invalid"], spk[0], 16 * spk[1])
        return {"d16": disp, "C": ref["C"], "S": ref["S"], "sizes": sizes}

    def _spk(self, sgm):
        return self(sgm)["sizes"]

    def _fspk(self, mseed, new_val, size, diff):
        import speckle_model as K
        out, sizes = K.filter_speckles(rand_d16(self.d.W, self.d.H, self.d.D, mseed), new_val, size, diff)
        return {"out": out, "sizes": sizes}

    # JointWMF's clustering of one image: (centres, label_of_key, iterations)
    def _cl(self, k, side):
        import jwmf_model as J
        m = J.clustering_of(self.d.pairs[k][side])
        return m["centres"], m["lok"], m["iterations"]

    # the score stage: score_model.score's dict
    def _score(self, source, data, truth):
        import score_model as SC
        gt, mask = self.d.truths[truth] if truth is not None else (None, None)
        return SC.score(source, tuple(self(data)) if source == GIF else self(data)["d16"], gt, mask, self.d.D)

    def _img(self, k):
        return self.d.pairs[k]

    # the hook plane of psm_score_upload_sgm_map: rand_d16 with its invalid value re-mapped to the setting's at the upload
    def _hook(self, mseed, inv):
        m = rand_d16(self.d.W, self.d.H, self.d.D, mseed).copy()
        m[m == -16] = inv
        return {"d16": m}

    # the left image as bytes: pair k, pair k as the quantised float pair, the left plane of a gray compute
    def _guide(self, kind, k):
        import depth_model as DM
        if kind == "gray":
            return self.d.gray(k)[0]
        return DM.quantise(self.d.float_pair(k)[0]) if kind == "fpair" else self.d.pairs[k][0]

    # the WLS stage: wls_model.wls's dict (plus "d16", the filtered map under the name the SGM sources read it by)
    def _wls(self, src, inv, guide, par):
        import wls_model as WM
        if src[0] == "gif":
            v, gif_inv = WM.gif_source(self(src[1])[0], self(src[2])[0] if src[2] is not None else None)
            assert gif_inv == inv
        else:
            v = self(src[1])["d16"]
        out = WM.wls(v, inv, self(guide), *par)
        out["d16"] = out["disp"]
        return out

    # the reprojection stage: {"xyz", "z", "cloud"} of depth_model.reproject
    def _depth(self, src, missing, qi, zi, colour):
        import depth_model as DM
        if src[0] == "gif":
            d, miss = DM.gif_disparity(self(src[1])[0], self(missing)[0] if missing is not None else None)
        else:
            d16 = self(src[1])["d16"]
            d, miss = d16.astype(np.float64) * 0.0625, d16 == missing
        xyz, z, cloud = DM.reproject(d, miss, q_matrix(qi), Q_CROPS[qi], Z_RANGES[zi], self(colour))
        return {"xyz": xyz, "z": z, "cloud": cloud}


def sgm_range(sgm, D):
    """(dmin, number of disparities) an SGM result expression was computed with"""
    return sgm[4], sgm[5] or D


# --------------------------------------------------------------------------------------------------------------- the shadow

class Ctx:
    """What the header says a context holds.  A new context is as DispEst's constructor leaves it: pair 0 uploaded."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.pair, self.staged = (0, False), None       # (index, uploaded as float); the pair of an asynchronous upload
        self.rows = None                                # the stripe in force (None: whole image)
        self.flags = 0
        self.cost, self.lazy = None, False              # None | "fresh" | "filt" | "patched" (slices uploaded); the costs are a recipe
        self.filt, self.filt_rows = None, None          # what a select yields: a maps expression, and the stripe it was filtered with
        self.window = False                             # between a single-phase CostFilter and the next DispSelect
        self.maps, self.maps_rows = None, None          # the current maps (rows None: whole image)
        self.mask, self.mask_fresh = None, False        # fresh: psm_lr_check on the current maps gives this mask again
        self.buf = "own"
        self.sgm, self.range_set, self.sizes = None, (0, 0), None
        self.jw = [None, None]
        self.truth, self.score, self.pending = None, None, None
        # the WLS stage: parameters, the result (("wls", source map, invalid value, guide, parameters)), the publish switch, an
        # asynchronous run not yet waited for
        self.wls_par, self.wls, self.wls_pub, self.wls_pending = WLS_DEFAULT, None, False, False
        # the reprojection stage: Q with its crop and the z-range (indices; no Q in a new context), the result ((("depth", map,
        # missing rule, Q, range, colour image), outputs)), an asynchronous count not yet collected
        self.q, self.zr, self.depth, self.depth_pending = None, 0, None, False
        self.hook = None                                # the hook plane: ("hook", mseed, the invalid value its holes were written with)

    def new_pair(self, k, fl):
        """adopt_new_pair: nothing derived from the previous pair survives; the SGM, score, WLS and reprojection stages keep their
        results (the new left image guides and colours their later runs)"""
        self.pair = (k, fl)
        self.cost, self.filt, self.window = None, None, False
        self.maps, self.mask = None, None
        self.jw = [None, None]

    def write_maps(self, expr, rows=None):
        self.maps, self.maps_rows, self.mask, self.mask_fresh = expr, rows, None, False

    def maps_gone(self):
        self.maps, self.mask = None, None

    @property
    def striped(self):
        return self.rows is not None

    @property
    def whole_maps(self):
        return self.maps is not None and self.maps_rows is None

    def depth_next(self):
        return (self.staged or self.pair)[1]


class Step:
    def __init__(self, kind, ctx, args=None, refused=None, window=False):
        self.kind, self.ctx, self.args, self.refused, self.window = kind, ctx, args or {}, refused, window

    def __repr__(self):
        a = " ".join(f"{k}={v}" for k, v in self.args.items())
        return f"{self.kind}[{self.ctx}] {a}".rstrip() + (f"  -> refused /{self.refused}/" if self.refused else "")

    def key(self):
        return (self.kind, self.ctx, tuple(sorted((k, repr(v)) for k, v in self.args.items())), self.refused, self.window)


class World:
    def __init__(self, shape, dtype):
        self.W, self.H, self.D = shape
        self.dtype = dtype
        self.ctxs = [Ctx(dtype) for _ in range(NCTX)]

    # ---- ops: each returns None, or the regex of the refusal (then nothing has changed) ----
    def apply(self, st: Step):
        return getattr(self, "op_" + st.kind)(st.ctx, **st.args)

    def _c(self, ci):
        return self.ctxs[ci]

    # pairs
    def op_images(self, ci, k):
        c = self._c(ci)
        c.staged = None
        c.new_pair(k, False)

    def op_images_async(self, ci, k):
        self._c(ci).staged = (k, False)

    def op_float(self, ci, k):
        c = self._c(ci)
        c.staged = None
        c.new_pair(k, True)

    def op_frame(self, ci):
        return self.op_images(ci, RECT)

    def op_frame_async(self, ci):
        return self.op_images_async(ci, RECT)

    # the guided-filter path
    def op_cost_const(self, ci):
        c = self._c(ci)
        if c.staged is not None:
            c.new_pair(*c.staged)
            c.staged = None
        c.lazy = not (c.flags & MATERIALISE) and (c.dtype == "f32" or not (c.flags & STORE))
        c.cost, c.filt, c.window = "fresh", None, False
        c.maps_gone()

    def _can_filter_both(self, c):
        return c.cost == "fresh" and c.lazy and not (c.flags & STORE)

    def op_cost_filter(self, ci):
        c = self._c(ci)
        if c.cost is None or (c.striped and not self._can_filter_both(c)):
            return r"psm_cost_filter\b"
        assert c.cost == "fresh", "a second filter of a filtered volume is outside the model"
        two_phase = not (c.flags & TWO_PHASE_OFF) and bool(c.flags & TWO_PHASE_ON)      # (both shapes have fewer than 112 slices)
        c.window = self._can_filter_both(c) and not two_phase
        c.filt, c.filt_rows = ("gf", c.pair[0], c.dtype), c.rows if self._can_filter_both(c) else None
        c.cost = "filt"
        c.maps_gone()

    def op_cost_filter_sides(self, ci):
        c = self._c(ci)
        if c.cost is None or c.striped:
            return r"psm_cost_filter_side"
        assert c.cost == "fresh"
        c.window = False
        c.filt, c.filt_rows, c.cost = ("gf", c.pair[0], c.dtype), None, "filt"
        c.maps_gone()

    def op_cost_filter_fgf(self, ci, s):
        c = self._c(ci)
        if c.dtype != "f32" or c.cost is None or c.striped:
            return r"psm_cost_filter_fgf"
        assert c.cost == "fresh"
        c.window = False
        c.filt, c.filt_rows, c.cost = ("fgf", c.pair[0], s), None, "filt"
        c.maps_gone()

    def op_disp_select(self, ci):
        c = self._c(ci)
        if c.cost is None:
            return r"psm_disp_select"
        assert c.cost == "filt", "a select of unfiltered costs is outside the model"
        c.window = False
        c.write_maps(c.filt, c.filt_rows)

    op_select_async = op_disp_select            # DispSelect_device + download_maps_async + download_maps_wait

    def op_upload_volume(self, ci, side, d0, n):
        c = self._c(ci)
        c.cost, c.lazy, c.filt, c.window = "patched", False, None, False
        c.maps_gone()

    def op_set_rows(self, ci, y0, y1, flags):
        c = self._c(ci)
        c.rows = None if (y0, y1) in ((0, 0), (0, self.H)) else (y0, y1)
        if flags is not None:
            c.flags = flags

    def op_flags(self, ci, flags):
        self._c(ci).flags = flags

    def op_mapbuf(self, ci, to):
        c = self._c(ci)
        if to != c.buf:
            c.maps_gone()
        c.buf = to

    def op_release_scratch(self, ci):
        """The SGM result, the score planes, the WLS planes with publishing and the reprojection planes go; parameters, Q, the
        z-range, the truth and the hook plane (psm_api_core.cpp: score_free(c, false) keeps what psm_score_set_truth and
        psm_score_upload_sgm_map uploaded) stay."""
        c = self._c(ci)
        c.sgm, c.sizes, c.score = None, None, None
        c.wls, c.wls_pub, c.wls_pending = None, False, False
        c.depth, c.depth_pending = None, False

    # post-processing
    def op_lr_check(self, ci):
        c = self._c(ci)
        if not c.whole_maps:
            return r"psm_lr_check"
        c.mask, c.mask_fresh = ("lr", c.maps), True

    def op_fill_inv(self, ci):
        c = self._c(ci)
        if c.mask is None:
            return r"psm_fill_invalid"
        c.maps, c.mask_fresh = ("fill", c.maps, c.mask), False

    def op_wgt_median(self, ci):
        c = self._c(ci)
        if c.mask is None:
            return r"psm_wgt_median"
        c.maps, c.mask_fresh = ("wm", c.maps, c.mask, c.pair[0]), False

    def op_jwmf(self, ci, radius):
        c = self._c(ci)
        if not c.whole_maps:
            return r"psm_joint_wmf"
        self._jwmf(c, radius)

    def _jwmf(self, c, radius):
        c.maps, c.mask_fresh = ("jw", c.maps, c.pair[0], radius), False          # (the valid masks stay as they are)
        c.jw = [("cl", c.pair[0], 0), ("cl", c.pair[0], 1)]

    def op_upload_maps(self, ci, mseed, masks):
        c = self._c(ci)
        c.write_maps(("up", mseed))
        if masks:
            c.mask = ("upmask", mseed)

    # the SGM stage
    def _sgm_expr(self, c, cost, mode, dmin, nd, spk):
        return ("sgm", c.pair[0], tuple(cost), mode, dmin, nd, tuple(spk))

    def op_sgbm(self, ci, cost, mode, dmin, nd, spk):
        c = self._c(ci)
        c.range_set = (dmin, nd)                    # (the settings are made before the compute is refused)
        if c.striped:
            return r"psm_sgm_compute"
        self._sgbm(c, cost, mode, dmin, nd, spk)

    def _sgbm(self, c, cost, mode, dmin, nd, spk):
        c.sgm = self._sgm_expr(c, cost, mode, dmin, nd, spk)
        if spk[0] > 0:
            c.sizes = ("spk", c.sgm)

    def _select_ok(self, c):
        if c.striped or c.sgm is None:
            return False
        dmin, nd = sgm_range(c.sgm, self.D)
        return dmin >= 0 and dmin + nd <= self.D

    def op_sgbm_select(self, ci):
        c = self._c(ci)
        if not self._select_ok(c):
            return r"psm_sgm_select_maps"
        c.write_maps(("sgmaps", c.sgm))

    def op_filter_speckles(self, ci, mseed, new_val, size, diff):
        self._c(ci).sizes = ("fspk", mseed, new_val, size, diff)

    def op_set_range(self, ci, dmin, nd):
        self._c(ci).range_set = (dmin, nd)

    # the score stage
    def op_set_truth(self, ci, t):
        self._c(ci).truth = t

    def op_clear_truth(self, ci):
        self._c(ci).truth = None

    def _score_data(self, c, source):
        if source == GIF:
            return c.maps if c.whole_maps else None
        src = self._source_map(c)
        return src[0] if src is not None else None

    def op_score(self, ci, source):
        c = self._c(ci)
        data = self._score_data(c, source)
        if data is None:
            return r"psm_score\b"
        c.score = ("score", source, data, c.truth)

    def op_score_async(self, ci, source):
        c = self._c(ci)
        r = self.op_score(ci, source)
        if r is None:
            c.pending = c.score
        return r

    def op_score_wait(self, ci):
        c = self._c(ci)
        if c.pending is None:
            return r"psm_score_wait"
        c.pending = None

    # several contexts
    def op_compute_batch(self, cis):
        cs = [self._c(i) for i in cis]
        if any(c.flags & (STORE | MATERIALISE) or c.flags != cs[0].flags or c.striped or c.depth_next() != cs[0].depth_next() for c in cs):
            return r"psm_compute_batch"
        for c in cs:
            if c.staged is not None:
                c.new_pair(*c.staged)
                c.staged = None
            c.lazy, c.cost, c.window = True, "filt", False
            c.filt, c.filt_rows = ("gf", c.pair[0], c.dtype), None
            c.write_maps(c.filt)

    def op_sgbm_batch(self, cis, cost, mode, dmin, nd, spk):
        cs = [self._c(i) for i in cis]
        for c in cs:
            c.range_set = (dmin, nd)
        if any(c.striped or c.pair[1] != cs[0].pair[1] for c in cs):
            return r"psm_sgm_compute_batch"
        for c in cs:
            self._sgbm(c, cost, mode, dmin, nd, spk)

    def op_sgbm_select_batch(self, cis):
        cs = [self._c(i) for i in cis]
        if any(not self._select_ok(c) or sgm_range(c.sgm, self.D) != sgm_range(cs[0].sgm, self.D) for c in cs):
            return r"psm_sgm_select_maps_batch"
        for c in cs:
            c.write_maps(("sgmaps", c.sgm))

    def op_jwmf_batch(self, cis, radius):
        cs = [self._c(i) for i in cis]
        if any(not c.whole_maps or c.pair[1] != cs[0].pair[1] for c in cs):
            return r"psm_joint_wmf_batch"
        for c in cs:
            self._jwmf(c, radius)

    def op_score_batch(self, cis, source):
        cs = [self._c(i) for i in cis]
        masked = [c.truth == 0 for c in cs]
        if any(self._score_data(c, source) is None or (c.truth is None) != (cs[0].truth is None) for c in cs) or len(set(masked)) > 1:
            return r"psm_score_batch"
        for c in cs:
            c.score = ("score", source, self._score_data(c, source), c.truth)

    def op_gather(self, ci, k, cut):
        """psm_gather_rows_ctx into context ci.  k None: the root is a member - it holds a stripe of its own maps and the other rows
        come from contexts made for the op; else the stripes [0, cut) and [cut, H) of pair k from two contexts made for the op."""
        c = self._c(ci)
        assert k is not None or (c.maps is not None and c.maps_rows is not None and c.maps[0] == "gf")
        c.write_maps(c.maps if k is None else ("gf", k, c.dtype))

    def op_merge(self, ci, k, cut):
        """psm_disp_merge_ctx of the disparity shards [0, cut) and [cut, D) of pair k, made for the op, into context ci"""
        c = self._c(ci)
        c.write_maps(("gf", k, c.dtype))

    # ---- which map, which invalid value, which left image (psm_ctx.h: sgm_stage_*, sgm_source_*, colour_of) ----
    def _stage_map(self, c):
        """What the SGM source of psm_wls_filter reads -> (expression, invalid value) or None.  The hook plane while it is on, with
        the invalid value of the CURRENT psm_sgm_set_range setting; else the last compute's map with the invalid value of the range it
        was computed with.  Never the WLS stage's own published result."""
        if c.hook is not None:
            return c.hook, (c.range_set[0] - 1) * 16
        if c.sgm is not None:
            return c.sgm, (sgm_range(c.sgm, self.D)[0] - 1) * 16
        return None

    def _source_map(self, c):
        """What the SGM sources of psm_score and psm_reproject read: the same, or - publishing on, a WLS result there, no hook plane -
        that result with the invalid value it was made with."""
        if c.wls_pub and c.wls is not None and c.hook is None:
            return c.wls, c.wls[2]
        return self._stage_map(c)

    def _guide(self, c, sgm_source):
        """The left image that guides psm_wls_filter and colours the cloud: under an SGM source with a result of psm_sgm_compute_gray
        that call's left plane (whichever map is read: the hook plane does not change it); else the current pair's, a float pair
        quantised."""
        if sgm_source and c.sgm is not None and isinstance(c.sgm[1], tuple):
            return ("guide", "gray", c.sgm[1][1])
        return ("guide", "fpair" if c.pair[1] else "pair", c.pair[0])

    # the hook plane and the one-channel compute
    def op_hook_map(self, ci, mseed):
        c = self._c(ci)
        c.hook = None if mseed is None else ("hook", mseed, (c.range_set[0] - 1) * 16)

    def op_sgbm_gray(self, ci, k, cost, mode, dmin, nd, spk):
        """psm_sgm_compute_gray on the green planes of pair k (the caller's memory: any pair, the staged colour pair is untouched)"""
        c = self._c(ci)
        c.range_set = (dmin, nd)
        if c.striped:
            return r"psm_sgm_compute_gray"
        c.sgm = ("sgm", ("g", k), tuple(cost), mode, dmin, nd, tuple(spk))
        if spk[0] > 0:
            c.sizes = ("spk", c.sgm)

    # the WLS stage.  source: "gif", "gifm" (PSM_WLS_USE_MASK), "sgm"
    def _wls_expr(self, c, source):
        if source == "sgm":
            src = self._stage_map(c)
            if src is None:
                return None
            return ("wls", ("d16", src[0]), src[1], self._guide(c, True), c.wls_par)
        if not c.whole_maps or (source == "gifm" and c.mask is None):
            return None
        return ("wls", ("gif", c.maps, c.mask if source == "gifm" else None), -16, self._guide(c, False), c.wls_par)

    def op_wls(self, ci, source, pending=False):
        c = self._c(ci)
        e = self._wls_expr(c, source)
        if e is None:
            return r"psm_wls_filter\b"
        c.wls, c.wls_pending = e, pending

    def op_wls_async(self, ci, source):
        return self.op_wls(ci, source, pending=True)

    def op_wls_wait(self, ci):
        c = self._c(ci)
        if not c.wls_pending:
            return r"psm_wls_wait"
        c.wls_pending = False

    def op_wls_batch(self, cis, source):
        cs = [self._c(i) for i in cis]
        es = [self._wls_expr(c, source) for c in cs]
        if any(e is None for e in es) or any(c.wls_par[2] != cs[0].wls_par[2] for c in cs):
            return r"psm_wls_filter_batch"
        for c, e in zip(cs, es):
            c.wls, c.wls_pending = e, False

    def op_wls_params(self, ci, lam, sigma, iterations):
        self._c(ci).wls_par = (lam, sigma, iterations)

    def op_wls_publish(self, ci, on):
        c = self._c(ci)
        if on and c.wls is None:
            return r"psm_wls_publish"
        c.wls_pub = bool(on)

    # the reprojection stage.  source as above; outs: a non-empty subset of XYZ | Z | CLOUD
    def _depth_expr(self, c, source):
        if c.q is None:
            return None
        if source == "sgm":
            src = self._source_map(c)
            if src is None:
                return None
            return ("depth", ("d16", src[0]), src[1], c.q, c.zr, self._guide(c, True))
        if not c.whole_maps or (source == "gifm" and c.mask is None):
            return None
        return ("depth", ("gif", c.maps), c.mask if source == "gifm" else None, c.q, c.zr, self._guide(c, False))

    def op_reproject(self, ci, source, outs, pending=False):
        c = self._c(ci)
        e = self._depth_expr(c, source)
        if e is None:
            return r"psm_reproject\b"
        c.depth, c.depth_pending = (e, outs), pending

    def op_reproject_async(self, ci, source, outs):
        return self.op_reproject(ci, source, outs, pending=True)

    def op_reproject_wait(self, ci):
        c = self._c(ci)
        if not c.depth_pending:
            return r"psm_reproject_wait"
        c.depth_pending = False

    def op_reproject_batch(self, cis, source, outs):
        cs = [self._c(i) for i in cis]
        es = [self._depth_expr(c, source) for c in cs]
        if any(e is None for e in es):
            return r"psm_reproject_batch"
        for c, e in zip(cs, es):
            c.depth, c.depth_pending = (e, outs), False

    def op_reproject_q(self, ci, q, zr):
        c = self._c(ci)
        c.q, c.zr = q, zr

    # psm_post_process_batch: the named stages in PP::processDM's order; every member ends where its own single calls leave it
    def op_pp_batch(self, cis, stages):
        cs = [self._c(i) for i in cis]
        if any(not c.whole_maps or (not stages & LR and c.mask is None) or c.pair[1] != cs[0].pair[1] for c in cs):
            return r"psm_post_process_batch"
        for i in cis:
            for bit, op in ((LR, self.op_lr_check), (FILL, self.op_fill_inv), (WM, self.op_wgt_median)):
                if stages & bit:
                    r = op(i)
                    assert r is None, r

    # ---- readers: name -> the expression(s) the shadow says the context holds, or None when undefined ----
    def readers(self, ci):
        c = self._c(ci)
        out = {}
        if c.wls is not None:
            out["wls_planes"] = ("wls", c.wls)
        if c.depth is not None:
            out["reprojected"] = ("depth",) + c.depth
            if c.depth[1] & CLOUD:
                out["cloud"] = ("depth",) + c.depth
        if c.maps is not None:
            out["download_maps"] = ("gf_path", c.maps, c.maps_rows)
        if c.mask is not None and c.mask_fresh:
            out["download_valid"] = ("pp", c.mask)
        if c.sgm is not None:
            out["sgm_disparity"] = ("sgm", c.sgm)
            out["sgm_costs"] = ("sgm", c.sgm)
        if c.sizes is not None:
            out["sgm_speckle_sizes"] = ("sgm", c.sizes)
        if c.score is not None:
            out["score_maps"] = ("score", c.score)
        if not c.pair[1]:
            out["download_images"] = ("pairs", ("img", c.pair[0]))
        if c.jw[0] is not None:
            out["jwmf_clusters"] = ("jwmf", tuple(c.jw))
        return out


STAGE_OF = {"images": "pairs", "images_async": "pairs", "float": "pairs", "frame": "pairs", "frame_async": "pairs",
            "cost_const": "gf_path", "cost_filter": "gf_path", "cost_filter_sides": "gf_path", "cost_filter_fgf": "gf_path",
            "disp_select": "gf_path", "select_async": "gf_path", "upload_volume": "gf_path", "set_rows": "gf_path", "flags": "gf_path", "mapbuf": "gf_path",
            "release_scratch": "scratch", "lr_check": "pp", "fill_inv": "pp", "wgt_median": "pp", "jwmf": "jwmf", "upload_maps": "pp",
            "sgbm": "sgm", "sgbm_select": "sgm", "filter_speckles": "sgm", "set_range": "sgm",
            "set_truth": "score", "clear_truth": "score", "score": "score", "score_async": "score", "score_wait": "score",
            "compute_batch": "gf_path", "sgbm_batch": "sgm", "sgbm_select_batch": "sgm", "jwmf_batch": "jwmf", "score_batch": "score",
            "gather": "exchange", "merge": "exchange"}
OP_KINDS = tuple(STAGE_OF)
# how often the generator proposes a kind when the state does not suggest one (the guided-filter frames open the windows)
_W = {"cost_const": 3.5, "flags": 0.6, "set_rows": 0.6, "images": 0.7, "images_async": 0.7, "clear_truth": 1.0, "set_truth": 1.3,
      "float": 2.5, "score_batch": 1.6, "sgbm_batch": 1.4, "cost_filter_sides": 1.3, "compute_batch": 1.3,
      "jwmf": 1.5, "jwmf_batch": 1.3, "score": 1.5, "score_async": 1.5, "sgbm_select": 1.3, "sgbm_select_batch": 1.3, "lr_check": 1.5,
      "fill_inv": 1.5, "wgt_median": 2.0, "gather": 0.6, "merge": 0.6, "mapbuf": 0.6, "upload_maps": 0.8}
_WEIGHTS = np.array([_W.get(k, 1.0) for k in OP_KINDS])
_WEIGHTS = _WEIGHTS / _WEIGHTS.sum()


# ------------------------------------------------------------------------------------------------------------ the generator

class Walk:
    def __init__(self, seed, shape, dtype, steps, vocabulary="default"):
        self.seed, self.shape, self.dtype, self.steps, self.vocabulary = seed, shape, dtype, steps, vocabulary

    def log(self, upto=None):
        W, H, D = self.shape
        head = f"walk {self.seed}: {W}x{H} D={D} {self.dtype}" + ("" if self.vocabulary == "default" else f" ({self.vocabulary} vocabulary)")
        return "\n".join([head] + [f"  {i:3d} {s!r}" for i, s in enumerate(self.steps[:upto])])


def _sgm_args(rng, D):
    cost = [("sad",), ("bt", int(rng.integers(1, 64))), ("census", int(rng.choice([3, 5, 9])), int(rng.choice([3, 5, 7])))][int(rng.integers(0, 3))]
    dmin, nd = [(0, 0), (0, 0), (0, D), (2, D - 4), (-3, 16), (0, D + 16)][int(rng.integers(0, 6))]
    spk = (int(rng.integers(1, 60)), int(rng.integers(0, 4))) if rng.random() < 0.4 else (0, 0)
    return {"cost": cost, "mode": MODES[int(rng.integers(0, 4))], "dmin": dmin, "nd": nd, "spk": spk}


def _subset(rng):
    n = int(rng.integers(1, NCTX + 1))
    return tuple(int(i) for i in rng.permutation(NCTX)[:n])


def _propose(rng, w: World, ci):
    """One op for context ci, biased towards what the shadow's state makes interesting.  -> (kind, ctx or contexts, args)"""
    c = w.ctxs[ci]
    H, D = w.H, w.D
    u = rng.random()
    if c.window and u < 0.8:                          # a single-phase filter has run and has not been selected: foreign writers
        pick = int(rng.integers(0, 9))
        if pick == 0:
            return ("upload_maps", ci, {"mseed": int(rng.integers(0, 1 << 16)), "masks": bool(rng.integers(0, 2))})
        if pick == 1:
            return ("mapbuf", ci, {"to": "caller" if c.buf == "own" else "own"})
        if pick == 2 and not c.striped:
            return ("gather", ci, {"k": int(rng.integers(0, NPAIRS)), "cut": int(rng.integers(1, H))})
        if pick == 3 and not c.striped:
            return ("merge", ci, {"k": int(rng.integers(0, NPAIRS)), "cut": int(rng.integers(1, D))})
        if pick in (4, 5) and not c.striped:
            if not w._select_ok(c):
                return ("sgbm", ci, dict(_sgm_args(rng, D), dmin=0, nd=0))
            if pick == 4:
                return ("sgbm_select", ci, {})
            others = [i for i in range(NCTX) if i != ci and w._select_ok(w.ctxs[i]) and sgm_range(w.ctxs[i].sgm, D) == sgm_range(c.sgm, D)]
            return ("sgbm_select_batch", tuple([ci] + others[:int(rng.integers(0, 3))]), {})
        return ("disp_select", ci, {})
    if c.cost == "fresh" and u < 0.8:                 # costs wait for their filter
        v = rng.random()
        if v < 0.66 or (c.striped and v < 0.9):
            return ("cost_filter", ci, {})
        if v < 0.78:
            return ("cost_filter_sides", ci, {})
        if v < 0.94:
            return ("cost_filter_fgf", ci, {"s": int(rng.choice([2, 4, 8]))}) if c.dtype == "f32" or v > 0.91 else ("cost_filter", ci, {})
        return ("images_async", ci, {"k": int(rng.integers(0, NPAIRS - 1))})
    if c.cost == "patched" and u < 0.7:               # slices were uploaded: the model follows again from new costs on
        return ("cost_const", ci, {})
    if c.cost == "filt" and c.maps is None and u < 0.8:
        return ("select_async" if rng.random() < 0.2 else "disp_select", ci, {})
    if c.pending is not None and u < 0.5:
        return ("score_wait", ci, {})
    if c.mask is not None and u < 0.45:               # a mask waits for the stages that need one
        return (("fill_inv", "wgt_median", "lr_check")[int(rng.integers(0, 3))], ci, {})
    if c.whole_maps and c.mask is None and u < 0.3:
        return ("lr_check", ci, {}) if rng.random() < 0.6 or c.pending is not None else ("score", ci, {"source": GIF})
    kind = OP_KINDS[int(rng.choice(len(OP_KINDS), p=_WEIGHTS))]
    if kind in ("images", "images_async", "float"):
        if kind == "float" and c.dtype != "f32":
            kind = "images"
        return (kind, ci, {"k": int(rng.integers(0, NPAIRS - 1))})
    if kind in ("frame", "frame_async", "cost_const", "cost_filter", "cost_filter_sides", "lr_check", "fill_inv", "wgt_median",
                "sgbm_select", "clear_truth", "score_wait"):
        if kind in ("cost_filter", "cost_filter_sides") and c.cost in ("filt", "patched"):
            kind = "cost_const"                       # (a second filter of a filtered volume is defined, but not by one oracle call)
        return (kind, ci, {})
    if kind == "disp_select" or kind == "select_async":
        return (kind if c.cost not in ("fresh", "patched") else "cost_filter" if c.cost == "fresh" else "cost_const", ci, {})
    if kind == "cost_filter_fgf":
        return (kind, ci, {"s": int(rng.choice([2, 4, 8]))}) if c.cost not in ("filt", "patched") else ("cost_const", ci, {})
    if kind == "upload_volume":
        d0 = int(rng.integers(0, D))
        return (kind, ci, {"side": int(rng.integers(0, 2)), "d0": d0, "n": int(rng.integers(1, min(4, D - d0) + 1))})
    if kind == "set_rows":
        if rng.random() < 0.4:
            return (kind, ci, {"y0": 0, "y1": int(rng.choice([0, H])), "flags": None})
        y0 = int(rng.integers(0, H - 1))
        return (kind, ci, {"y0": y0, "y1": int(rng.integers(y0 + 1, H + 1)), "flags": int(rng.choice(FLAGS_SAFE))})
    if kind == "flags":
        fl = int(rng.choice(FLAGS_SAFE if c.striped else FLAGS_ANY))
        return (kind, ci, {"flags": 0 if (c.dtype == "u8" and fl == STORE) else fl})
    if kind == "mapbuf":
        return (kind, ci, {"to": str(rng.choice(["caller", "own"]))})
    if kind == "release_scratch":
        return (kind, ci, {}) if c.pending is None and c.staged is None else ("score_wait" if c.pending is not None else "cost_const", ci, {})
    if kind == "jwmf":
        return (kind, ci, {"radius": int(rng.integers(2, 5))}) if not c.pair[1] and not c.window else ("lr_check", ci, {})
    if kind == "upload_maps":
        return (kind, ci, {"mseed": int(rng.integers(0, 1 << 16)), "masks": bool(rng.integers(0, 2))})
    if kind == "sgbm":
        return (kind, ci, _sgm_args(rng, D))
    if kind == "filter_speckles":
        return (kind, ci, {"mseed": int(rng.integers(0, 1 << 16)), "new_val": int(rng.choice([-16, 0])), "size": int(rng.integers(0, 40)),
                           "diff": int(rng.integers(0, 48))})
    if kind == "set_range":
        return (kind, ci, {"dmin": int(rng.integers(-4, 5)), "nd": int(rng.choice([0, 16, D + 8]))})
    if kind == "set_truth":
        return (kind, ci, {"t": int(rng.integers(0, 2))})
    if kind in ("score", "score_async"):
        if c.pending is not None:
            return ("score_wait", ci, {})
        return (kind, ci, {"source": int(rng.integers(0, 3))})
    cis = _subset(rng)
    if kind in _ELIGIBLE and rng.random() < 0.8:      # mostly a subset the call accepts
        ok = [i for i in range(NCTX) if _ELIGIBLE[kind](w, w.ctxs[i], c)]
        if ok:
            cis = tuple(int(i) for i in rng.permutation(ok)[:int(rng.integers(1, len(ok) + 1))])
    if kind == "compute_batch":
        return (kind, cis, {})
    if kind == "sgbm_batch":
        return (kind, cis, _sgm_args(rng, D))
    if kind == "sgbm_select_batch":
        return (kind, cis, {})
    if kind == "jwmf_batch":
        if any(w.ctxs[i].pair[1] or w.ctxs[i].window for i in cis):
            return ("lr_check", ci, {})
        return (kind, cis, {"radius": int(rng.integers(2, 5))})
    if kind == "score_batch":
        if any(w.ctxs[i].pending is not None for i in cis):
            return ("score_wait", ci, {})
        return (kind, cis, {"source": int(rng.integers(0, 3))})
    if kind == "gather":
        if c.maps is not None and c.maps_rows is not None and c.maps[0] == "gf":
            return (kind, ci, {"k": None, "cut": 0})
        return (kind, ci, {"k": int(rng.integers(0, NPAIRS)), "cut": int(rng.integers(1, H))})
    assert kind == "merge", kind
    return (kind, ci, {"k": int(rng.integers(0, NPAIRS)), "cut": int(rng.integers(1, D))})


_ELIGIBLE = {
    "compute_batch": lambda w, x, c: not x.striped and x.flags == c.flags and not x.flags & (STORE | MATERIALISE) and x.depth_next() == c.depth_next(),
    "sgbm_batch": lambda w, x, c: not x.striped and x.pair[1] == c.pair[1],
    "sgbm_select_batch": lambda w, x, c: w._select_ok(x) and (c.sgm is None or sgm_range(x.sgm, w.D) == sgm_range(c.sgm, w.D)),
    "jwmf_batch": lambda w, x, c: x.whole_maps and not x.pair[1] and not x.window,
    "score_batch": lambda w, x, c: x.pending is None and x.whole_maps and x.truth == c.truth,
}


def generate(seed, steps=STEPS, vocabulary="default") -> Walk:
    """The walk of a seed: ops, each followed by one or two readers of another stage than the one just driven, and by one reader
    on every context a batch op did not name.  The refusals are the shadow's; at most a quarter of the ops are refused.
    vocabulary "default": the ops of OP_KINDS, the walks of SEEDS; "tail": the ops of TAIL_KINDS, the walks of TAIL_SEEDS."""
    if vocabulary == "tail":
        return _generate_tail(seed, steps)
    assert vocabulary == "default", vocabulary
    rng = np.random.default_rng([seed, 20240])
    shape = SHAPES[seed % 2]
    dtype = "u8" if (shape == SHAPES[0] and seed % 8 in (2, 6)) else "f32"
    w = World(shape, dtype)
    out, refused = [], 0
    mode = seed % 5                                  # a fifth of the walks each: forced two-phase, forced single-phase, stripes
    if mode in (0, 1):
        for ci in range(NCTX):
            out.append(Step("flags", ci, {"flags": TWO_PHASE_ON if mode == 0 else TWO_PHASE_OFF}))
    elif mode == 2:
        y0 = int(rng.integers(0, shape[1] // 2))
        out.append(Step("set_rows", 0, {"y0": y0, "y1": int(rng.integers(y0 + 4, shape[1] + 1)), "flags": 0}))
    out += [Step("cost_const", 0), Step("cost_filter", 0), Step("sgbm", 1, dict(_sgm_args(rng, shape[2]), dmin=0, nd=0))]
    for st in out:
        st.window = w.ctxs[st.ctx].window
        assert w.apply(st) is None
    out.append(Step("read", 1, {"what": "sgm_disparity"}))
    n_ops = len(out) - 1
    steps += n_ops
    while n_ops < steps + 3 * NCTX:
        if n_ops >= steps:                           # the walk ends with a whole frame on every context
            ci = (n_ops - steps) // 3
            st = Step(("cost_const", "cost_filter", "disp_select")[(n_ops - steps) % 3], ci, window=w.ctxs[ci].window)
            assert w.apply(st) is None, st
            out.append(st)
            n_ops += 1
            if st.kind == "disp_select":
                out.append(Step("read", ci, {"what": "download_maps"}))
            continue
        ci = int(rng.integers(0, NCTX))
        kind, ctx, args = _propose(rng, w, ci)
        first = ctx if isinstance(ctx, int) else ctx[0]
        st = Step(kind, ctx, args, window=w.ctxs[first].window if kind != "sgbm_select_batch" else any(w.ctxs[i].window for i in ctx))
        trial = _copy(w)
        st.refused = trial.apply(st)
        if st.refused is not None:
            if 4 * (refused + 1) > n_ops + 1:        # (keeps the share of refusals below a quarter at every prefix)
                continue
            refused += 1
        else:
            w = trial
        out.append(st)
        n_ops += 1
        named = (ctx,) if isinstance(ctx, int) else ctx
        # readers: of the driven context(s) from other stages; of every other context when a batch ran
        for i in range(NCTX):
            rd = w.readers(i)
            if i in named:
                rd = {n: v for n, v in rd.items() if v[0] != STAGE_OF[kind]} or rd
                take = min(len(rd), int(rng.integers(1, 3))) if i == named[0] else min(len(rd), 1)
            else:
                take = min(len(rd), 1) if not isinstance(ctx, int) else 0
            names = sorted(rd)
            if take:                                 # (the staged images change rarely: read them rarely)
                p = np.array([0.1 if n == "download_images" else 3.0 if n in ("download_valid", "jwmf_clusters") else 1.0 for n in names])
                for j in rng.choice(len(names), size=take, replace=False, p=p / p.sum()):
                    out.append(Step("read", i, {"what": names[int(j)]}))
    return Walk(seed, shape, dtype, out)


def _copy(w: World) -> World:
    import copy
    return copy.deepcopy(w)


def replay(walk: Walk):
    """The walk on the shadow alone.  Yields (index, step, world after the step, what a read step must see); raises when the
    shadow's refusal differs from the recorded one."""
    w = World(walk.shape, walk.dtype)
    for i, st in enumerate(walk.steps):
        if st.kind == "read":
            rd = w.readers(st.ctx)
            if st.args["what"] not in rd:
                raise AssertionError(f"step {i}: {st!r} reads what the shadow says is undefined")
            yield i, st, w, rd[st.args["what"]][1:]
            continue
        trial = _copy(w)
        got = trial.apply(st)
        if got != st.refused:
            raise AssertionError(f"step {i}: {st!r}: the shadow says {got!r}")
        if got is None:
            w = trial
        yield i, st, w, None


SEEDS = tuple(range(40))


# ---------------------------------------------------------------------------------------------------- the tail vocabulary

NEW_KINDS = ("wls", "wls_async", "wls_wait", "wls_batch", "wls_params", "wls_publish", "hook_map", "reproject", "reproject_async",
             "reproject_wait", "reproject_batch", "reproject_q", "pp_batch", "sgbm_gray")
NEW_READERS = ("wls_planes", "reprojected", "cloud")
_OLDER = ("images", "images_async", "float", "frame", "frame_async", "cost_const", "cost_filter", "disp_select", "release_scratch",
          "lr_check", "fill_inv", "wgt_median", "upload_maps", "sgbm", "sgbm_batch", "sgbm_select", "set_range", "set_truth", "score",
          "score_async", "score_wait", "score_batch")
TAIL_STAGE_OF = dict({k: STAGE_OF[k] for k in _OLDER}, wls="wls", wls_async="wls", wls_wait="wls", wls_batch="wls", wls_params="wls",
                     wls_publish="wls", hook_map="score", reproject="depth", reproject_async="depth", reproject_wait="depth",
                     reproject_batch="depth", reproject_q="depth", pp_batch="pp", sgbm_gray="sgm")
TAIL_KINDS = tuple(TAIL_STAGE_OF)
_TW = {"wls": 2.0, "reproject": 2.0, "wls_batch": 1.6, "reproject_batch": 1.6, "pp_batch": 1.8, "wls_publish": 1.6, "hook_map": 1.4,
       "wls_params": 1.9, "wls_async": 1.2, "reproject_async": 1.2, "wls_wait": 0.9, "reproject_wait": 0.9, "sgbm_gray": 1.0,
       "images": 0.6, "images_async": 0.5, "float": 0.6, "frame": 0.4, "frame_async": 0.4, "cost_const": 0.8, "cost_filter": 0.3,
       "disp_select": 0.3, "release_scratch": 0.8, "lr_check": 0.9, "fill_inv": 0.5, "wgt_median": 0.5, "upload_maps": 0.9,
       "sgbm": 1.0, "sgbm_batch": 0.6, "sgbm_select": 0.7, "set_range": 0.8, "set_truth": 0.5, "score": 1.2, "score_async": 0.5,
       "score_wait": 0.3, "score_batch": 0.7, "reproject_q": 0.9}
_TAIL_WEIGHTS = np.array([_TW[k] for k in TAIL_KINDS])
_TAIL_WEIGHTS = _TAIL_WEIGHTS / _TAIL_WEIGHTS.sum()
_SOURCES = ("gif", "gifm", "sgm")
# the reader that sees what a carried-out op of the tail vocabulary wrote (read first, ahead of the readers of other stages)
_OWN_READER = {"wls": ("wls_planes",), "wls_wait": ("wls_planes",), "wls_batch": ("wls_planes",), "reproject": ("reprojected", "cloud"),
               "reproject_wait": ("reprojected", "cloud"), "reproject_batch": ("reprojected", "cloud"), "score": ("score_maps",),
               "score_batch": ("score_maps",), "pp_batch": ("download_maps", "download_valid"), "sgbm_gray": ("sgm_disparity",)}


def _a_source(rng, w, c, depth):
    """mostly a source the call accepts in this state"""
    ok = [s for s in _SOURCES if (w._depth_expr(c, s) if depth else w._wls_expr(c, s)) is not None]
    if ok and rng.random() < 0.85:
        return ok[int(rng.integers(0, len(ok)))]
    return _SOURCES[int(rng.integers(0, 3))]


def _wls_par(j):
    lam, sigma, it = WLS_PARAMS[j]
    return {"lam": lam, "sigma": sigma, "iterations": it}


def _members(rng, w, free, ok):
    """a batch's contexts: mostly a subset, in any order, of those among `free` that the call accepts"""
    el = [i for i in free if ok(w.ctxs[i])]
    pool = el if el and rng.random() < 0.85 else list(free)
    return tuple(int(i) for i in rng.permutation(pool)[:int(rng.integers(1, len(pool) + 1))])


def _propose_tail(rng, w: World, ci, free):
    """One op of the tail vocabulary for context ci (a batch: among the contexts `free`).  -> (kind, ctx or contexts, args)"""
    c = w.ctxs[ci]
    D = w.D
    u = rng.random()
    if c.cost == "fresh":                             # a guided-filter frame runs on to its select
        return ("cost_filter", ci, {})
    if c.cost == "filt" and c.maps is None and u < 0.85:
        return ("disp_select", ci, {})
    if c.wls_pending and u < 0.5:
        return ("wls_wait", ci, {})
    if c.depth_pending and u < 0.5:
        return ("reproject_wait", ci, {})
    if c.pending is not None and u < 0.5:
        return ("score_wait", ci, {})
    kind = TAIL_KINDS[int(rng.choice(len(TAIL_KINDS), p=_TAIL_WEIGHTS))]
    if kind in ("images", "images_async", "float"):
        if kind == "float" and c.dtype != "f32":
            kind = "images"
        return (kind, ci, {"k": int(rng.integers(0, NPAIRS - 1))})
    if kind in ("frame", "frame_async", "cost_const", "lr_check", "fill_inv", "wgt_median", "sgbm_select", "score_wait", "wls_wait",
                "reproject_wait"):
        return (kind, ci, {})
    if kind == "cost_filter":
        return (kind if c.cost is None else "cost_const", ci, {})
    if kind == "disp_select":
        return (kind, ci, {})
    if kind == "release_scratch":
        return (kind, ci, {}) if c.pending is None and c.staged is None else ("score_wait" if c.pending is not None else "cost_const", ci, {})
    if kind == "upload_maps":
        return (kind, ci, {"mseed": int(rng.integers(0, 1 << 16)), "masks": bool(rng.integers(0, 2))})
    if kind == "sgbm":
        return (kind, ci, _sgm_args(rng, D))
    if kind == "sgbm_gray":
        return (kind, ci, dict(_sgm_args(rng, D), k=int(rng.integers(0, NPAIRS))))
    if kind == "set_range":
        return (kind, ci, {"dmin": int(rng.integers(-4, 5)), "nd": int(rng.choice([0, 16, D + 8]))})
    if kind == "set_truth":
        return (kind, ci, {"t": int(rng.integers(0, 2))})
    if kind in ("score", "score_async"):
        if c.pending is not None:
            return ("score_wait", ci, {})
        return (kind, ci, {"source": int(rng.integers(0, 3))})
    if kind in ("wls", "wls_async"):
        return (kind, ci, {"source": _a_source(rng, w, c, False)})
    if kind in ("reproject", "reproject_async"):
        return (kind, ci, {"source": _a_source(rng, w, c, True), "outs": int(rng.integers(1, 8))})
    if kind == "wls_params":
        return (kind, ci, _wls_par(int(rng.integers(0, len(WLS_PARAMS)))))
    if kind == "wls_publish":
        return (kind, ci, {"on": bool(rng.random() < 0.7)})
    if kind == "hook_map":
        return (kind, ci, {"mseed": None if c.hook is not None and rng.random() < 0.4 else int(rng.integers(0, 1 << 16))})
    if kind == "reproject_q":
        return (kind, ci, {"q": int(rng.integers(0, 2)), "zr": int(rng.integers(0, 2))})
    if kind == "sgbm_batch":
        return (kind, _members(rng, w, free, lambda x: x.pair[1] == c.pair[1]), _sgm_args(rng, D))
    if kind == "score_batch":
        source = int(rng.integers(0, 3))
        cis = _members(rng, w, free, lambda x: x.pending is None and w._score_data(x, source) is not None and x.truth == c.truth)
        if any(w.ctxs[i].pending is not None for i in cis):
            return ("score_wait", ci, {})
        return (kind, cis, {"source": source})
    if kind == "wls_batch":
        source = _a_source(rng, w, c, False)
        return (kind, _members(rng, w, free, lambda x: w._wls_expr(x, source) is not None and x.wls_par[2] == c.wls_par[2]), {"source": source})
    if kind == "reproject_batch":
        source = _a_source(rng, w, c, True)
        return (kind, _members(rng, w, free, lambda x: w._depth_expr(x, source) is not None), {"source": source, "outs": int(rng.integers(1, 8))})
    assert kind == "pp_batch", kind
    stages = PP_STAGES[int(rng.integers(0, len(PP_STAGES)))]
    return (kind, _members(rng, w, free, lambda x: x.whole_maps and (stages & LR or x.mask is not None) and x.pair[1] == c.pair[1]), {"stages": stages})


# The interleavings tests/test_seq_model.py asks of the tail walks, as scripts: each yields the ops of one context (the batch
# scripts: of all three) in order, reading the shadow as it stands when the op is due (H.w).  Ops of other contexts fall between.
class _Holder:
    w: World = None


def _plain_sgm(dmin=0, nd=0):
    return {"cost": ("sad",), "mode": "hh", "dmin": dmin, "nd": nd, "spk": (0, 0)}


def _mseed(rng):
    return int(rng.integers(0, 1 << 16))


def _quiet(H, ci):
    """ahead of a release_scratch: nothing staged, no record in flight (the shadow does not follow those through the release)"""
    c = H.w.ctxs[ci]
    if c.pending is not None:
        yield ("score_wait", ci, {})
    if c.staged is not None:
        yield ("cost_const", ci, {})
        yield ("cost_filter", ci, {})
        yield ("disp_select", ci, {})


def _score_sgm(H, ci, source):
    if H.w.ctxs[ci].pending is not None:
        yield ("score_wait", ci, {})
    yield ("score", ci, {"source": source})


def _m_hook_over_published(rng, H, ci):
    if H.w.ctxs[ci].hook is not None:
        yield ("hook_map", ci, {"mseed": None})
    yield ("sgbm", ci, _sgm_args(rng, H.w.D))
    yield ("wls", ci, {"source": "sgm"})
    yield ("wls_publish", ci, {"on": True})
    yield ("hook_map", ci, {"mseed": _mseed(rng)})
    yield from _score_sgm(H, ci, SGM)
    yield ("reproject", ci, {"source": "sgm", "outs": int(rng.integers(1, 8))})
    yield ("hook_map", ci, {"mseed": None})
    yield from _score_sgm(H, ci, SGM_INT)
    yield ("reproject", ci, {"source": "sgm", "outs": int(rng.integers(1, 8)) | CLOUD})


def _m_stale_invalid(rng, H, ci):
    if H.w.ctxs[ci].hook is not None:
        yield ("hook_map", ci, {"mseed": None})
    yield ("sgbm", ci, _plain_sgm())
    yield ("wls", ci, {"source": "sgm"})
    yield ("wls_publish", ci, {"on": True})
    yield ("sgbm", ci, dict(_sgm_args(rng, H.w.D), **dict(zip(("dmin", "nd"), ((2, H.w.D - 4), (-3, 16))[int(rng.integers(0, 2))]))))
    yield ("reproject", ci, {"source": "sgm", "outs": XYZ | CLOUD})
    yield from _score_sgm(H, ci, SGM)


def _m_hook_invalid(rng, H, ci):
    yield ("hook_map", ci, {"mseed": _mseed(rng)})
    yield ("set_range", ci, {"dmin": 3, "nd": 0})
    yield ("reproject", ci, {"source": "sgm", "outs": int(rng.integers(1, 8))})
    yield ("wls", ci, {"source": "sgm"})
    yield ("set_range", ci, {"dmin": -2, "nd": 0})
    yield ("reproject", ci, {"source": "sgm", "outs": Z | CLOUD})


def _m_rerun_after_release(rng, H, ci):
    yield ("hook_map", ci, {"mseed": _mseed(rng)})
    yield ("wls", ci, {"source": "sgm"})
    yield ("wls_publish", ci, {"on": True})
    yield ("reproject", ci, {"source": "sgm", "outs": int(rng.integers(1, 8))})
    yield from _quiet(H, ci)
    yield ("release_scratch", ci, {})
    yield ("reproject", ci, {"source": "sgm", "outs": int(rng.integers(1, 8))})
    yield ("wls", ci, {"source": "sgm"})


def _m_table_reload(rng, H, ci):
    a, b = ((0, 2), (1, 5), (4, 0), (2, 1), (3, 5), (6, 2), (7, 5))[int(rng.integers(0, 7))]          # two entries of WLS_PARAMS of different sigma
    if H.w._stage_map(H.w.ctxs[ci]) is None:
        yield ("hook_map", ci, {"mseed": _mseed(rng)})
    yield ("wls_params", ci, _wls_par(a))
    yield ("wls", ci, {"source": "sgm"})
    yield ("wls_params", ci, _wls_par(b))
    if rng.random() < 0.5:
        yield ("wls", ci, {"source": "sgm"})
        yield ("wls_params", ci, _wls_par(a))
        yield ("wls", ci, {"source": "sgm"})
        return
    yield ("wls", ci, {"source": "sgm"})
    yield ("hook_map", ci, {"mseed": _mseed(rng)})   # (the SGM source must outlive the release)
    yield from _quiet(H, ci)
    yield ("release_scratch", ci, {})
    yield ("wls_params", ci, _wls_par(a))
    yield ("wls", ci, {"source": "sgm"})


def _a_new_pair(rng, H, ci):
    c = H.w.ctxs[ci]
    kinds = ["images", "frame"] + (["float"] if c.dtype == "f32" else [])
    kind = kinds[int(rng.integers(0, len(kinds)))]
    if kind == "frame":
        return (kind, ci, {}) if c.pair != (RECT, False) else ("images", ci, {"k": 1})
    k = int(rng.integers(0, NPAIRS - 1))
    if (k, kind == "float") == c.pair:
        k = (k + 1) % (NPAIRS - 1)
    return (kind, ci, {"k": k})


def _m_guide_follows_pair(rng, H, ci):
    yield ("hook_map", ci, {"mseed": _mseed(rng)})
    yield ("wls", ci, {"source": "sgm"})
    yield ("reproject", ci, {"source": "sgm", "outs": CLOUD})
    yield _a_new_pair(rng, H, ci)
    yield ("wls", ci, {"source": "sgm"})
    yield ("reproject", ci, {"source": "sgm", "outs": CLOUD | Z})


def _m_staged_not_adopted(rng, H, ci):
    yield ("hook_map", ci, {"mseed": _mseed(rng)})
    yield ("wls_async", ci, {"source": "sgm"})
    yield ("images_async", ci, {"k": (H.w.ctxs[ci].pair[0] + 1) % (NPAIRS - 1)})
    yield ("wls_wait", ci, {})
    yield ("reproject_async", ci, {"source": "sgm", "outs": CLOUD | int(rng.integers(0, 4))})
    yield ("frame_async", ci, {}) if rng.random() < 0.5 else ("images_async", ci, {"k": (H.w.ctxs[ci].pair[0] + 2) % (NPAIRS - 1)})
    yield ("reproject_wait", ci, {})


def _m_gray_guide(rng, H, ci):
    if H.w.ctxs[ci].hook is not None and rng.random() < 0.6:      # (with the hook plane on the gray plane guides all the same)
        yield ("hook_map", ci, {"mseed": None})
    yield ("sgbm_gray", ci, dict(_sgm_args(rng, H.w.D), k=int(rng.integers(0, NPAIRS))))
    yield ("wls", ci, {"source": "sgm"})
    yield ("reproject", ci, {"source": "sgm", "outs": CLOUD | int(rng.integers(0, 4))})
    yield ("sgbm", ci, _sgm_args(rng, H.w.D))
    yield ("wls", ci, {"source": "sgm"})
    yield ("reproject", ci, {"source": "sgm", "outs": CLOUD})


def _m_own_wls(rng, H, ci):
    order = [int(i) for i in rng.permutation(NCTX)]
    for i, j in zip(order, rng.permutation(3)):       # (entries 0 .. 2 of WLS_PARAMS: one iteration count, three lambdas and sigmas)
        if H.w._stage_map(H.w.ctxs[i]) is None:
            yield ("hook_map", i, {"mseed": _mseed(rng)})
        yield ("wls_params", i, _wls_par(int(j)))
    yield ("wls_batch", tuple(order), {"source": "sgm"})
    yield ("wls_batch", (order[1], order[0]), {"source": "sgm"})
    yield ("wls_params", order[0], _wls_par((int(rng.integers(0, 3)))))
    yield ("wls_batch", (order[2], order[0], order[1]), {"source": "sgm"})


def _m_own_depth_pp(rng, H, ci):
    order = [int(i) for i in rng.permutation(NCTX)]
    for i in order:
        if H.w.ctxs[i].pair[1]:                       # (the members of a psm_post_process_batch hold pairs of one depth)
            yield ("images", i, {"k": H.w.ctxs[i].pair[0]})
        if not H.w.ctxs[i].whole_maps:
            yield ("upload_maps", i, {"mseed": _mseed(rng), "masks": bool(rng.integers(0, 2))})
    yield ("pp_batch", tuple(order), {"stages": LR | FILL})
    yield ("reproject_batch", tuple(order), {"source": "gifm", "outs": int(rng.integers(1, 8))})
    yield ("pp_batch", (order[2], order[0]), {"stages": PP_STAGES[int(rng.integers(0, 4))]})
    yield ("reproject_batch", (order[1], order[2], order[0]), {"source": "gif", "outs": int(rng.integers(1, 8)) | CLOUD})


def _m_batch_against_single(rng, H, ci):
    if rng.random() < 0.5:
        yield ("upload_maps", ci, {"mseed": _mseed(rng), "masks": bool(rng.integers(0, 2))})
    else:
        yield ("sgbm", ci, _plain_sgm())
        yield ("sgbm_select", ci, {})
    stages = PP_STAGES[int(rng.integers(0, 3))]
    c = H.w.ctxs[ci]
    others = [i for i in range(NCTX) if i != ci and H.w.ctxs[i].whole_maps and H.w.ctxs[i].pair[1] == c.pair[1]]
    cis = [ci] + others[:int(rng.integers(0, 3))]
    yield ("pp_batch", tuple(int(i) for i in rng.permutation(cis)), {"stages": stages})
    yield ("pp_batch", (ci,), {"stages": LR})


_MOTIFS = (_m_hook_over_published, _m_stale_invalid, _m_hook_invalid, _m_rerun_after_release, _m_table_reload, _m_guide_follows_pair,
           _m_staged_not_adopted, _m_gray_guide, _m_own_wls, _m_own_depth_pp, _m_batch_against_single)
_ALL_CTX = (_m_own_wls, _m_own_depth_pp, _m_batch_against_single)          # scripts whose batches name every context


def _generate_tail(seed, steps) -> Walk:
    """A walk of the tail vocabulary: four of the scripts above, one after the other, each on a context of its own choice, with
    seeded ops of the other contexts between their steps and of any context between the scripts.  After every op that wrote a result
    its own reader, then readers of other stages as in generate."""
    rng = np.random.default_rng([seed, 20241])
    shape = SHAPES[seed % 2]
    dtype = "u8" if (shape == SHAPES[0] and seed % 6 == 4) else "f32"
    H = _Holder()
    H.w = World(shape, dtype)
    out, count = [], {"ops": 0, "refused": 0}

    def push(kind, ctx, args, forced=False):
        w = H.w
        named = (ctx,) if isinstance(ctx, int) else tuple(ctx)
        st = Step(kind, ctx, args, window=any(w.ctxs[i].window for i in named))
        trial = _copy(w)
        st.refused = trial.apply(st)
        if st.refused is not None:
            if 4 * (count["refused"] + 1) > count["ops"] + 1:        # (keeps the share of refusals below a quarter at every prefix)
                return
            count["refused"] += 1
        else:
            H.w = w = trial
        out.append(st)
        count["ops"] += 1
        if forced:
            return
        own = _OWN_READER.get(kind, ()) if st.refused is None else ()
        for i in range(NCTX):
            rd = w.readers(i)
            first = [n for n in own if n in rd] if i in named else []
            for n in first:
                out.append(Step("read", i, {"what": n}))
            rd = {n: v for n, v in rd.items() if n not in first}
            if i in named:
                rd = {n: v for n, v in rd.items() if v[0] != TAIL_STAGE_OF[kind]} or rd
                take = min(len(rd), 1)
            else:
                take = min(len(rd), 1) if not isinstance(ctx, int) and rng.random() < 0.5 else 0
            names = sorted(rd)
            if take:
                p = np.array([0.1 if n == "download_images" else 3.0 if n in NEW_READERS + ("score_maps", "download_valid") else 1.0 for n in names])
                for j in rng.choice(len(names), size=take, replace=False, p=p / p.sum()):
                    out.append(Step("read", i, {"what": names[int(j)]}))

    for ci in range(NCTX):                            # every context starts with a Q; one with maps, one with a compute, one with a hook plane
        push("reproject_q", ci, {"q": int(rng.integers(0, 2)), "zr": int(rng.integers(0, 2))}, forced=True)
    for kind in ("cost_const", "cost_filter", "disp_select"):
        push(kind, 0, {}, forced=True)
    push("sgbm", 1, dict(_sgm_args(rng, shape[2]), dmin=0, nd=0))
    push("hook_map", 2, {"mseed": _mseed(rng)})
    steps += count["ops"]
    scripts = [_MOTIFS[(4 * seed + 5 * j) % len(_MOTIFS)] for j in range(4)]
    script, busy = None, ()
    while count["ops"] < steps:
        if script is None and scripts and rng.random() < 0.6:
            m = scripts.pop(0)
            ci = int(rng.integers(0, NCTX))
            script, busy = m(rng, H, ci), (tuple(range(NCTX)) if m in _ALL_CTX else (ci,))
        free = [i for i in range(NCTX) if i not in busy]
        if script is not None and (not free or rng.random() < 0.7):
            try:
                push(*next(script))
            except StopIteration:
                script, busy = None, ()
            continue
        ci = int(free[int(rng.integers(0, len(free)))])
        kind, ctx, args = _propose_tail(rng, H.w, ci, free)
        push(kind, ctx, args)
    return Walk(seed, shape, dtype, out, vocabulary="tail")


TAIL_SEEDS = tuple(range(100, 124))
