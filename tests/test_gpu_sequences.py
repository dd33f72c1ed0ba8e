"""-m gpu: one context through every stage, against the models.  tests/seq_model.py is the shadow of what include/primesm_hip.h
says a context holds between two calls; here its walks and a set of named interleavings run on real contexts, and after every
call the bytes the context hands out - maps, masks, the SGM stage's planes, score planes and records, the staged pair, the
JointWMF clustering - must equal what the CPU definitions give for the shadow's state.  Everything is bit for bit: there is no
tolerance in this file.  A call the header says is refused must raise capi.PsmError naming the call, and the readers behind it
must still see the state from before.  The walks of the tail vocabulary (test_tail_walk) do the same for the WLS stage, the
reprojection stage, psm_post_process_batch, the hook plane and the gray compute: the int16 map and the float planes of
psm_wls_download and the weight table as bit patterns, the dense planes of psm_reproject_download as bit patterns, the cloud's
count and record bytes.

One process, at most six contexts alive: three of the walk, one whose key plane serves as the caller's map buffer
(psm_set_map_buffer wants device memory; the plane is never written, that context does not filter), two made and closed inside
a gather or merge op.  No step is chosen to make the device fault: every refused step is refused before anything is enqueued."""
import numpy as np
import pytest

import seq_model as S

pytestmark = pytest.mark.gpu

ON, OFF = S.TWO_PHASE_ON, S.TWO_PHASE_OFF


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


class Rig:
    """The contexts of a walk or a scenario, the inputs (seq_model.Data) and the expected values (seq_model.Refs)."""

    def __init__(self, psm, oracle, shape, dtype, seed, nctx=S.NCTX):
        from primestereomatch_amd.rectify import Rectification
        self.psm, self.capi, self.shape, self.dtype = psm, psm.capi, shape, dtype
        self.W, self.H, self.D = shape
        self.data = S.Data(shape, seed)
        self.R = S.Refs(self.data, oracle, (shape, seed))
        self.des, self.spare = [], None
        self.rect = Rectification(self.data.map_xy, self.data.map_frac, S.SRC[0], S.SRC[1], self.data.crop)
        try:
            for _ in range(nctx):
                self.des.append(self.new())
                self.des[-1].setRectification(self.rect)
            self.spare = self.new()
        except Exception:
            self.close()
            raise
        ptr, nbytes = self.spare.partial_keys()
        self.slot = (2 * self.W * self.H + 4 + 255) // 256 * 256
        assert nctx * self.slot <= nbytes
        self.caller_buf = [ptr + i * self.slot for i in range(nctx)]

    def new(self, pair=0, **kw):
        return self.psm.DispEst(*self.data.pairs[pair], self.D, dtype=self.dtype, **kw)

    def close(self):
        for de in self.des + ([self.spare] if self.spare is not None else []):
            de.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- the pieces the scenarios and the walks share ----
    def frame(self, de, select=True):
        de.CostConst_GPU(); de.CostFilter_GPU()
        if select:
            de.DispSelect_GPU()

    def gather_into(self, root, k, cut, member_rows=None):
        """psm_gather_rows_ctx into root: the stripes of pair k from contexts made here; member_rows: root holds these rows itself."""
        H = self.H
        spans = [(0, cut), (cut, H)] if member_rows is None else [(0, member_rows[0]), (member_rows[1], H)]
        temps = []
        try:
            for y0, y1 in spans:
                if y1 > y0:
                    t = self.new(k)
                    temps.append(t)
                    t.set_rows(y0, y1)
                    self.frame(t)
            root.gather_rows_ctx(([root] if member_rows is not None else []) + temps)
        finally:
            for t in temps:
                t.close()

    def merge_into(self, root, k, cut):
        """psm_disp_merge_ctx into root: the disparity shards [0, cut) and [cut, D) of pair k from contexts made here"""
        shards = []
        try:
            for d0, d1 in ((0, cut), (cut, self.D)):
                s = self.new(k, d_range=(d0, d1))
                shards.append(s)
                s.CostConst_GPU(); s.CostFilter_GPU(); s.DispSelect_partial()
            root.DispSelect_merge_ctx(shards)
        finally:
            for s in shards:
                s.close()

    def mapbuf(self, i, to):
        self.des[i].set_map_buffer(self.caller_buf[i] if to == "caller" else None)

    def sgbm_kw(self, cost, mode, dmin, nd, spk):
        return dict(mode=mode, min_disparity=dmin, num_disparities=nd, speckle_window_size=spk[0], speckle_range=spk[1],
                    pre_filter_cap=cost[1] if cost[0] == "bt" else 0, census=tuple(cost[1:]) if cost[0] == "census" else None)

    def check_record(self, rec, expr, what):
        m = self.R(expr)
        import score_model as SC
        for key in SC.RECORD_KEYS:
            assert rec[key] == m[key], (what, key, rec[key], m[key])

    def maps_are(self, de, expr, rows=None, what=""):
        y0, y1 = rows or (0, self.H)
        wl, wr = self.R(expr)
        gl, gr = de.download_maps()
        n = [int(np.count_nonzero(a[y0:y1] != b[y0:y1])) for a, b in ((gl, wl), (gr, wr))]
        assert n == [0, 0], (what, expr, rows, n)

    # ---- a walk's step on the device ----
    def run(self, st, before, after):
        """The op of a step; before / after: the shadow around it.  Results the call itself hands back are compared here."""
        from primestereomatch_amd import dispest
        a = st.args
        if not isinstance(st.ctx, int):
            des = [self.des[i] for i in st.ctx]
            if st.kind == "compute_batch":
                dispest.compute_batch(des)
            elif st.kind == "sgbm_batch":
                maps = dispest.sgbm_batch(des, **self.sgbm_kw(**a))
                for i, m in zip(st.ctx, maps):
                    assert same(m, self.R(after.ctxs[i].sgm)["d16"]), ("sgbm_batch", i)
            elif st.kind == "sgbm_select_batch":
                dispest.sgbm_select_batch(des)
            elif st.kind == "jwmf_batch":
                dispest.joint_wmf_batch(des, a["radius"])
            elif st.kind == "score_batch":
                for i, rec in zip(st.ctx, dispest.score_batch(des, a["source"])):
                    self.check_record(rec, after.ctxs[i].score, ("score_batch", i))
            elif st.kind == "wls_batch":
                src, mask = self.wls_source(a["source"])
                for i, m in zip(st.ctx, dispest.wls_batch(des, src, use_mask=mask)):
                    assert same(m, self.R(after.ctxs[i].wls)["disp"]), ("wls_batch", i)
            elif st.kind == "reproject_batch":
                src, mask = self.depth_source(a["source"])
                for i, n in zip(st.ctx, dispest.reproject_batch(des, src, a["outs"], use_mask=mask)):
                    assert n == len(self.R(after.ctxs[i].depth[0])["cloud"]), ("reproject_batch", i, n)
            elif st.kind == "pp_batch":
                dispest.post_process_batch(des, bool(a["stages"] & S.LR), bool(a["stages"] & S.FILL), bool(a["stages"] & S.WM))
                for i, d in zip(st.ctx, des):            # (the call's own downloads: psm_download_maps and psm_download_valid of every member)
                    c = after.ctxs[i]
                    assert same(d.lDisMap, self.R(c.maps)[0]) and same(d.rDisMap, self.R(c.maps)[1]), ("post_process_batch: maps", i)
                    assert same(d.lValid, self.R(c.mask)[0]) and same(d.rValid, self.R(c.mask)[1]), ("post_process_batch: masks", i)
            else:
                raise KeyError(st.kind)
            return
        i, de, c = st.ctx, self.des[st.ctx], after.ctxs[st.ctx]
        k = st.kind
        if k == "images":
            de.setInputImages(*self.data.pairs[a["k"]])
        elif k == "images_async":
            de.setInputImages_async(*self.data.pairs[a["k"]])
        elif k == "float":
            de.setInputImages(*self.data.float_pair(a["k"]))
        elif k == "frame":
            de.setInputFrame(self.data.frame)
        elif k == "frame_async":
            de.setInputFrame_async(self.data.frame)
        elif k == "cost_const":
            de.CostConst_GPU()
        elif k == "cost_filter":
            de.CostFilter_GPU()
        elif k == "cost_filter_sides":
            de.CostFilter_side(0); de.CostFilter_side(1)
        elif k == "cost_filter_fgf":
            de.setSubsampleRate(a["s"]); de.CostFilter_FGF_GPU()
        elif k == "disp_select":
            de.DispSelect_GPU()
        elif k == "select_async":
            de.DispSelect_device(); de.download_maps_async()
            y0, y1 = c.maps_rows or (0, self.H)
            for got, want in zip(de.download_maps_wait(), self.R(c.maps)):
                assert np.array_equal(got[y0:y1], want[y0:y1]), "download_maps_wait"
        elif k == "upload_volume":
            fill = np.uint8(64) if self.dtype == "u8" else np.float32(0.25)
            de.upload_volume(a["side"], np.full((a["n"], self.H, self.W), fill), d0=a["d0"])
        elif k == "set_rows":
            de.set_rows(a["y0"], a["y1"])
            if a["flags"] is not None:
                de.set_option(self.capi.PSM_OPT_FLAGS, a["flags"])
        elif k == "flags":
            de.set_option(self.capi.PSM_OPT_FLAGS, a["flags"])
        elif k == "mapbuf":
            self.mapbuf(i, a["to"])
        elif k == "release_scratch":
            de.release_scratch()
        elif k == "lr_check":
            de.LRCheck_GPU()
            if st.refused is not None:
                return
            lv, rv = self.R(c.mask)
            assert same(de.lValid, lv) and same(de.rValid, rv), "LRCheck_GPU"
        elif k == "fill_inv":
            de.FillInv_GPU()
        elif k == "wgt_median":
            de.WgtMedian_GPU()
        elif k == "jwmf":
            de.JointWMF_GPU(a["radius"])
        elif k == "upload_maps":
            l, r, lv, rv = S.rand_maps(self.W, self.H, self.D, a["mseed"])
            de.upload_maps(l, r, *((lv, rv) if a["masks"] else ()))
        elif k == "sgbm":
            assert same(de.SGBM_GPU(**self.sgbm_kw(**a)), self.R(c.sgm)["d16"]), "SGBM_GPU"
        elif k == "sgbm_select":
            de.SGBMSelect_GPU()
        elif k == "filter_speckles":
            got = de.filter_speckles(S.rand_d16(self.W, self.H, self.D, a["mseed"]), a["new_val"], a["size"], a["diff"])
            assert same(got, self.R(c.sizes)["out"]), "filter_speckles"
        elif k == "set_range":
            de._ck(de._lib.psm_sgm_set_range(de._h, a["dmin"], a["nd"]), "set_range")
        elif k == "set_truth":
            de.set_truth(*self.data.truths[a["t"]])
        elif k == "clear_truth":
            de.clear_truth()
        elif k == "score":
            self.check_record(de.Score_GPU(a["source"]), c.score, "Score_GPU")
        elif k == "score_async":
            de.set_option(self.capi.PSM_OPT_ASYNC, 1)
            try:
                assert de.Score_GPU(a["source"]) is None
            finally:
                de.set_option(self.capi.PSM_OPT_ASYNC, 0)
        elif k == "score_wait":
            rec = de.score_wait()
            self.check_record(rec, before.ctxs[i].pending, "score_wait")
        elif k == "gather":
            b = before.ctxs[i]
            if a["k"] is None:
                self.gather_into(de, b.maps[1], 0, member_rows=b.maps_rows)
            else:
                self.gather_into(de, a["k"], a["cut"])
        elif k == "merge":
            self.merge_into(de, a["k"], a["cut"])
        elif k == "wls":
            src, mask = self.wls_source(a["source"])
            de.WLS_GPU(src, use_mask=mask)
        elif k == "wls_async":
            src, mask = self.wls_source(a["source"])
            self.asynchronous(de, lambda: de.WLS_GPU(src, use_mask=mask))
        elif k == "wls_wait":
            de.wls_wait()
        elif k == "wls_params":
            de.setWLS(a["lam"], a["sigma"], a["iterations"])
        elif k == "wls_publish":
            de.wls_publish(a["on"])
        elif k == "hook_map":
            de.upload_sgm_map(None if a["mseed"] is None else self.R(c.hook)["d16"])
        elif k == "reproject":
            src, mask = self.depth_source(a["source"])
            n = de.Reproject_GPU(src, a["outs"], use_mask=mask)
            assert n == len(self.R(c.depth[0])["cloud"]), ("Reproject_GPU", n)
        elif k == "reproject_async":
            src, mask = self.depth_source(a["source"])
            assert self.asynchronous(de, lambda: de.Reproject_GPU(src, a["outs"], use_mask=mask)) is None
        elif k == "reproject_wait":
            n = de.reproject_wait()
            assert n == len(self.R(c.depth[0])["cloud"]), ("reproject_wait", n)
        elif k == "reproject_q":
            de.setReprojection(S.q_matrix(a["q"]), S.Q_CROPS[a["q"]], S.Z_RANGES[a["zr"]])
        elif k == "sgbm_gray":
            kw = self.sgbm_kw(a["cost"], a["mode"], a["dmin"], a["nd"], a["spk"])
            assert same(de.SGBM_GPU(gray=self.data.gray(a["k"]), **kw), self.R(c.sgm)["d16"]), "SGBM_GPU(gray=...)"
        else:
            raise KeyError(k)

    def wls_source(self, source):
        return (self.capi.PSM_WLS_SGM if source == "sgm" else self.capi.PSM_WLS_GIF), source == "gifm"

    def depth_source(self, source):
        return (self.capi.PSM_DEPTH_SGM if source == "sgm" else self.capi.PSM_DEPTH_GIF), source == "gifm"

    def asynchronous(self, de, call):
        de.set_option(self.capi.PSM_OPT_ASYNC, 1)
        try:
            return call()
        finally:
            de.set_option(self.capi.PSM_OPT_ASYNC, 0)

    def wls_is(self, de, expr, what=""):
        """every plane of the WLS stage against the model: the int16 map; q, num, den and the table as bit patterns"""
        m = self.R(expr)
        q, num, den = de.wls_planes()
        got = {"disp": de.wls_map(), "q": q, "num": num, "den": den, "tab": de.wls_table()}
        assert got["disp"].dtype == np.int16
        bad = [k for k in ("disp", "q", "num", "den", "tab")
               if not np.array_equal(got[k] if k == "disp" else got[k].view(np.uint32), m[k] if k == "disp" else m[k].view(np.uint32))]
        assert not bad, (what, bad, expr)

    def depth_is(self, de, expr, outs, what=""):
        """the planes of the reprojection stage that were among the outputs, and the cloud, against the model; the planes that were
        not are refused, naming psm_reproject_download"""
        import ctypes as C
        capi = self.capi
        m = self.R(expr)
        de._depth_outputs = outs                          # (the wrapper sizes its arrays by the last Reproject_GPU it was asked for)
        xyz, z = de.reprojected()
        assert (xyz is not None) == bool(outs & S.XYZ) and (z is not None) == bool(outs & S.Z)
        if xyz is not None:
            assert np.array_equal(xyz.view(np.uint32), m["xyz"].view(np.uint32)), (what, "xyz", expr)
        if z is not None:
            assert np.array_equal(z.view(np.uint32), m["z"].view(np.uint32)), (what, "z", expr)
        buf = np.empty((self.H, self.W, 3), np.float32)
        for bit, args in ((S.XYZ, (buf.ctypes.data_as(C.c_void_p), None)), (S.Z, (None, buf.ctypes.data_as(C.c_void_p)))):
            if not outs & bit:
                assert de._lib.psm_reproject_download(de._h, *args, 0) != 0 and capi.last_error(de._h).startswith("psm_reproject_download"), (what, bit)
        if outs & S.CLOUD:
            self.cloud_is(de, expr, what)
        else:
            with pytest.raises(capi.PsmError, match="psm_reproject_download_cloud"):
                de.cloud()

    def cloud_is(self, de, expr, what=""):
        m = self.R(expr)["cloud"]
        got = de.cloud()
        assert len(got) == len(m) and got.tobytes() == m.tobytes(), (what, "cloud", len(got), len(m), expr)

    def read(self, st, want):
        """A reader against the shadow.  -> None, or what differs."""
        de, what = self.des[st.ctx], st.args["what"]
        R = self.R
        if what == "download_maps":
            y0, y1 = want[1] or (0, self.H)
            pairs = [(g[y0:y1], w[y0:y1]) for g, w in zip(de.download_maps(), R(want[0]))]
        elif what == "download_valid":
            pairs = list(zip(de.download_valid(), R(want[0])))
        elif what == "sgm_disparity":
            pairs = [(de.sgm_disparity(), R(want[0])["d16"])]
        elif what == "sgm_costs":
            de._sgm_d = S.sgm_range(want[0], self.D)[1]             # (the wrapper sizes its arrays by the last SGBM_GPU it was asked for)
            pairs = [(de.sgm_costs()[1], R(want[0])["S"])]
        elif what == "sgm_speckle_sizes":
            v = R(want[0])
            pairs = [(de.sgm_speckle_sizes(), v["sizes"] if isinstance(v, dict) else v)]
        elif what == "score_maps":
            m = R(want[0])
            if want[0][1] == S.GIF:
                pairs = list(zip(de.score_maps(right=True), (m["ldisp"], m["rdisp"], m["emap"])))
            else:
                pairs = list(zip(de.score_maps(), (m["ldisp"], m["emap"])))
        elif what == "download_images":
            pairs = list(zip(de.download_images(), R(want[0])))
        elif what == "wls_planes":
            self.wls_is(de, want[0], what)
            return None
        elif what == "reprojected":
            self.depth_is(de, want[0], want[1], what)
            return None
        elif what == "cloud":
            self.cloud_is(de, want[0], what)
            return None
        elif what == "jwmf_clusters":
            pairs = []
            for side, e in enumerate(want[0]):
                cen, lok, it = de.jwmf_clusters(side)
                wc, wl, wi = R(e)
                pairs += [(cen, wc), (lok, wl), (np.int64(it), np.int64(wi))]
        else:
            raise KeyError(what)
        bad = [j for j, (g, w) in enumerate(pairs) if not np.array_equal(g, w)]
        return f"{what}: element(s) {bad} differ, {[int(np.count_nonzero(np.asarray(pairs[j][0]) != np.asarray(pairs[j][1]))) for j in bad]} values" if bad else None


# ------------------------------------------------------------------------------------------------------------- seeded walks

@pytest.mark.parametrize("seed", S.SEEDS)
def test_walk(psm, oracle, seed):
    """One walk of tests/seq_model.py on real contexts, op by op.  On a mismatch the walk's log up to that step is the failure's
    message: a reproducible script."""
    replay_on_the_device(psm, oracle, S.generate(seed), seed)


def replay_on_the_device(psm, oracle, walk, seed):
    import copy
    with Rig(psm, oracle, walk.shape, walk.dtype, seed) as rig:
        before = S.World(walk.shape, walk.dtype)
        for i, st, after, want in S.replay(walk):
            try:
                if st.kind == "read":
                    diff = rig.read(st, want)
                    assert diff is None, diff
                elif st.refused is not None:
                    with pytest.raises(psm.capi.PsmError, match=st.refused):
                        rig.run(st, before, after)
                else:
                    rig.run(st, before, after)
            except BaseException as e:
                raise AssertionError(f"step {i} ({st!r}): {type(e).__name__}: {str(e)[:600]}\n{walk.log(i + 1)}") from e
            before = copy.deepcopy(after)


@pytest.mark.parametrize("seed", S.TAIL_SEEDS)
def test_tail_walk(psm, oracle, seed):
    """One walk of the tail vocabulary (the WLS stage, the reprojection stage, psm_post_process_batch, the hook plane, the gray
    compute, between the older calls) on real contexts, op by op, as test_walk."""
    replay_on_the_device(psm, oracle, S.generate(seed, vocabulary="tail"), seed)


# ---------------------------------------------------------------------------------------------------------- named scenarios

SHAPE_A, SHAPE_B = S.SHAPES
WRITERS = ("sgbm_select", "sgbm_select_batch", "upload_maps", "gather", "merge", "mapbuf")


@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("shape,dtype,flags", [(SHAPE_A, "f32", 0), (SHAPE_B, "f32", OFF), (SHAPE_A, "f32", ON), (SHAPE_A, "u8", 0)])
def test_early_map_against_every_foreign_writer(psm, oracle, writer, shape, dtype, flags):
    """CostConst; CostFilter on pair A - single-phase: the filter's own reduction has filled the map buffer, a select has nothing
    left to launch - then something else writes the map buffer, then DispSelect: pair A's oracle maps every time.  With
    TWO_PHASE_ON there is no early map and the same must hold."""
    from primestereomatch_amd import dispest
    A, B = 1, 2
    with Rig(psm, oracle, shape, dtype, 101, nctx=2) as rig:
        de, other = rig.des
        de.set_option(psm.capi.PSM_OPT_FLAGS, flags)
        de.setInputImages(*rig.data.pairs[A])
        if writer.startswith("sgbm"):
            for d in rig.des:
                d.SGBM_GPU()
        rig.frame(de, select=False)
        if writer == "sgbm_select":
            de.SGBMSelect_GPU()
        elif writer == "sgbm_select_batch":
            dispest.sgbm_select_batch([other, de])
        elif writer == "upload_maps":
            de.upload_maps(*S.rand_maps(rig.W, rig.H, rig.D, 5)[:2])
        elif writer == "gather":
            rig.gather_into(de, B, rig.H // 2 + 1)
        elif writer == "merge":
            rig.merge_into(de, B, rig.D // 3)
        else:
            rig.mapbuf(0, "caller"); rig.mapbuf(0, "own")
        if writer == "mapbuf":
            with pytest.raises(psm.capi.PsmError, match="psm_download_maps"):
                de.download_maps()
        else:                                           # the writer's maps are current until the select
            want = {"sgbm_select": ("sgmaps", ("sgm", A, ("sad",), "hh", 0, 0, (0, 0))), "upload_maps": ("up", 5)}.get(writer, ("gf", B, dtype))
            if writer == "sgbm_select_batch":
                want = ("sgmaps", ("sgm", A, ("sad",), "hh", 0, 0, (0, 0)))
            rig.maps_are(de, want, what=f"after {writer}")
        de.DispSelect_GPU()
        wl, wr = rig.R(("gf", A, dtype))
        n = [int(np.count_nonzero(g != w)) for g, w in ((de.lDisMap, wl), (de.rDisMap, wr))]
        assert n == [0, 0], f"DispSelect after {writer}: {n} bytes differ from the oracle maps of the filtered pair"
        rig.maps_are(de, ("gf", A, dtype), what="download_maps after the select")


@pytest.mark.parametrize("writer", ["upload_maps", "sgbm_select", "gather"])
@pytest.mark.parametrize("flags", [0, ON])
def test_stripe_maps_after_foreign_whole_maps(psm, oracle, writer, flags):
    """A striped filter, then whole-image maps from elsewhere, then DispSelect of the minima still pending: the maps are the
    stripe's again - equal to the oracle's on its rows, and refused by the stages that want whole maps."""
    A, B = 1, 2
    with Rig(psm, oracle, SHAPE_A, "f32", 108, nctx=1) as rig:
        de = rig.des[0]
        rows = (9, 27)
        de.setInputImages(*rig.data.pairs[A])
        de.SGBM_GPU()
        de.set_option(psm.capi.PSM_OPT_FLAGS, flags)
        de.set_rows(*rows)
        rig.frame(de, select=False)
        if writer == "upload_maps":
            de.upload_maps(*S.rand_maps(rig.W, rig.H, rig.D, 6)[:2])
            whole = ("up", 6)
        elif writer == "sgbm_select":
            de.set_rows(0, 0)                        # (the SGM stage refuses a stripe in force; the filtered stripe stays what it is)
            de.SGBMSelect_GPU()
            whole = ("sgmaps", ("sgm", A, ("sad",), "hh", 0, 0, (0, 0)))
        else:
            rig.gather_into(de, B, 11)
            whole = ("gf", B, "f32")
        rig.maps_are(de, whole, what=f"whole maps from {writer}")
        de.LRCheck_GPU()                                                     # whole maps: accepted
        lv, rv = rig.R(("lr", whole))
        assert same(de.lValid, lv) and same(de.rValid, rv)
        de.DispSelect_GPU()
        rig.maps_are(de, ("gf", A, "f32"), rows=rows, what="the stripe's maps again")
        for call, fn in (("psm_lr_check", de.LRCheck_GPU), ("psm_joint_wmf", de.JointWMF_GPU), ("psm_score", de.Score_GPU)):
            with pytest.raises(psm.capi.PsmError, match=call):
                fn()
        rig.gather_into(de, A, 0, member_rows=rows)                          # ... until the other rows arrive
        rig.maps_are(de, ("gf", A, "f32"), what="gathered")
        de.LRCheck_GPU()
        lv, rv = rig.R(("lr", ("gf", A, "f32")))
        assert same(de.lValid, lv) and same(de.rValid, rv)


def test_sgm_result_across_the_guided_filter_path_and_back(psm, oracle):
    with Rig(psm, oracle, SHAPE_A, "f32", 102, nctx=1) as rig:
        de, R, D = rig.des[0], rig.R, rig.D
        args = dict(cost=("census", 5, 3), mode="3way", dmin=2, nd=D - 4, spk=(25, 2))
        sgm = ("sgm", 0, args["cost"], args["mode"], 2, D - 4, args["spk"])
        first = de.SGBM_GPU(**rig.sgbm_kw(**args)).copy()
        assert same(first, R(sgm)["d16"])

        def unchanged(where):
            de._sgm_d = D - 4
            Cv, Sv = de.sgm_costs()
            assert same(de.sgm_disparity(), R(sgm)["d16"]) and same(Cv, R(sgm)["C"]) and same(Sv, R(sgm)["S"]), where
            assert same(de.sgm_speckle_sizes(), R(sgm)["sizes"]), where

        unchanged("after the compute")
        rig.frame(de)
        de.LRCheck_GPU(); de.FillInv_GPU(); de.WgtMedian_GPU(); de.JointWMF_GPU(3)
        gf = ("gf", 0, "f32")
        pp = ("jw", ("wm", ("fill", gf, ("lr", gf)), ("lr", gf), 0), 0, 3)
        rig.maps_are(de, pp, what="the guided-filter frame with post-processing")
        de._ck(de._lib.psm_sgm_set_range(de._h, 0, 16), "set_range")
        unchanged("after a guided-filter frame, post-processing, JointWMF and psm_sgm_set_range")
        de.SGBMSelect_GPU()                                                  # the result's range, not the setting's
        rig.maps_are(de, ("sgmaps", sgm), what="SGBMSelect after set_range")
        de.release_scratch()
        with pytest.raises(psm.capi.PsmError, match="psm_sgm_select_maps"):
            de.SGBMSelect_GPU()
        rig.maps_are(de, ("sgmaps", sgm), what="the maps behind the refused select")
        with pytest.raises(psm.capi.PsmError, match="psm_sgm_download_disparity"):
            de.sgm_disparity()
        assert same(de.SGBM_GPU(**rig.sgbm_kw(**args)), first)
        unchanged("the second compute")


def test_jwmf_clustering_cache(psm, oracle):
    from primestereomatch_amd import dispest
    A, B = 0, 1
    with Rig(psm, oracle, SHAPE_A, "f32", 103, nctx=2) as rig:
        de, other = rig.des
        R = rig.R
        up = S.rand_maps(rig.W, rig.H, rig.D, 9)[:2]

        def clusters_are(d, k, where):
            for side in (0, 1):
                cen, lok, it = d.jwmf_clusters(side)
                wc, wl, wi = R(("cl", k, side))
                assert same(cen, wc) and same(lok, wl) and it == wi, (where, side)

        de.upload_maps(*up); de.JointWMF_GPU(2)
        clusters_are(de, A, "pair A")
        rig.maps_are(de, ("jw", ("up", 9), A, 2))
        de.setInputImages(*rig.data.pairs[B])                                # a new pair: the clustering goes with the old one
        with pytest.raises(psm.capi.PsmError, match="psm_joint_wmf_clusters"):
            de.jwmf_clusters(0)
        de.upload_maps(*up); de.JointWMF_GPU(2)
        clusters_are(de, B, "pair B")
        rig.maps_are(de, ("jw", ("up", 9), B, 2))
        de.setInputImages_async(*rig.data.pairs[A])                          # staged, not adopted: still pair B's
        de.upload_maps(*up); de.JointWMF_GPU(3)
        clusters_are(de, B, "pair B with pair A staged")
        rig.maps_are(de, ("jw", ("up", 9), B, 3))
        # clusters set for one side only, then a batch with this context: that side keeps them, the other is clustered
        cen, lok, _ = R(("cl", A, 0))                                        # (any valid clustering that is not pair B's own)
        de.setInputImages(*rig.data.pairs[B])
        de.set_jwmf_clusters(1, cen, lok)
        de.upload_maps(*up); other.upload_maps(*up)
        dispest.joint_wmf_batch([other, de], 2)
        got = de.jwmf_clusters(1)
        assert same(got[0], cen) and same(got[1], lok) and got[2] == 0, "the side whose clusters the host set was clustered again"
        wc, wl, wi = R(("cl", B, 0))
        got = de.jwmf_clusters(0)
        assert same(got[0], wc) and same(got[1], wl) and got[2] == wi
        import jwmf_model as J
        assert same(de.download_maps()[1].copy(), J.joint_wmf(up[1], rig.data.pairs[B][1], 2, clusters=(cen, lok)))
        clusters_are(other, 0, "the other member")
        rig.maps_are(other, ("jw", ("up", 9), 0, 2))


def test_batch_tables_sgm_and_score(psm, oracle):
    """The device tables of the batches are uploaded only when an entry changed: a member whose buffers were given back and
    allocated again, members in another order and a subset must all be seen."""
    from primestereomatch_amd import dispest
    with Rig(psm, oracle, SHAPE_B, "f32", 104) as rig:
        a, b, c = rig.des
        R = rig.R
        for k, de in enumerate(rig.des):
            de.setInputImages(*rig.data.pairs[k])
            de.set_truth(*rig.data.truths[0])
        sgm = [("sgm", k, ("sad",), "hh", 0, 0, (0, 0)) for k in range(3)]
        for de, m, e in zip(rig.des, dispest.sgbm_batch([a, b, c]), sgm):
            assert same(m, R(e)["d16"])
        b.release_scratch()
        for de, m, e in zip((c, b), dispest.sgbm_batch([c, b]), (sgm[2], sgm[1])):
            assert same(m, R(e)["d16"])
        dispest.sgbm_select_batch([b, c])
        rig.maps_are(b, ("sgmaps", sgm[1])); rig.maps_are(c, ("sgmaps", sgm[2]))
        for de, e in zip(rig.des, sgm):                                      # a keeps its result, b and c have theirs
            assert same(de.sgm_disparity(), R(e)["d16"]) and same(de.sgm_costs()[1], R(e)["S"])
        with pytest.raises(psm.capi.PsmError, match="psm_download_maps"):
            a.download_maps()
        for de, rec, e in zip((c, b), dispest.score_batch([c, b]), (sgm[2], sgm[1])):
            rig.check_record(rec, ("score", S.GIF, ("sgmaps", e), 0), "score_batch")
        b.release_scratch()
        # (b's SGM result went with its scratch: the batch over an SGM source must refuse it, naming the call)
        with pytest.raises(psm.capi.PsmError, match="psm_score_batch"):
            dispest.score_batch([c, b], S.SGM)
        for de, rec, e in zip((c, a), dispest.score_batch([c, a], S.SGM), (sgm[2], sgm[0])):
            rig.check_record(rec, ("score", S.SGM, e, 0), "score_batch SGM")
            m = R(("score", S.SGM, e, 0))
            ld, em = de.score_maps()
            assert same(ld, m["ldisp"]) and same(em, m["emap"])


def test_batch_tables_compute_and_jwmf(psm, oracle):
    from primestereomatch_amd import dispest
    with Rig(psm, oracle, SHAPE_B, "f32", 105) as rig:
        a, b, c = rig.des
        for k, de in enumerate(rig.des):
            de.setInputImages(*rig.data.pairs[k])
        gf = [("gf", k, "f32") for k in range(3)]
        dispest.compute_batch([a, b, c])
        for de, e in zip(rig.des, gf):
            rig.maps_are(de, e, what="compute_batch of three")
        b.release_scratch()
        b.setInputImages_async(*rig.data.pairs[0])                           # b's next frame is pair 0
        dispest.compute_batch([c, b])
        rig.maps_are(a, gf[0], what="a, not in the batch"); rig.maps_are(c, gf[2]); rig.maps_are(b, gf[0], what="b after its staged pair")
        dispest.joint_wmf_batch([a, b, c], 2)
        rig.maps_are(a, ("jw", gf[0], 0, 2)); rig.maps_are(b, ("jw", gf[0], 0, 2)); rig.maps_are(c, ("jw", gf[2], 2, 2))
        b.release_scratch()
        b.setInputImages(*rig.data.pairs[1])
        rig.frame(b)
        dispest.joint_wmf_batch([c, b], 3)
        rig.maps_are(b, ("jw", gf[1], 1, 3)); rig.maps_are(c, ("jw", ("jw", gf[2], 2, 2), 2, 3))
        rig.maps_are(a, ("jw", gf[0], 0, 2), what="a, not in the batch")
        dispest.joint_wmf_batch([b], 2)
        rig.maps_are(b, ("jw", ("jw", gf[1], 1, 3), 1, 2))


def test_score_follows_the_maps(psm, oracle):
    with Rig(psm, oracle, SHAPE_A, "f32", 106, nctx=1) as rig:
        de = rig.des[0]
        de.set_truth(*rig.data.truths[0])
        de.SGBM_GPU()
        sgm = ("sgm", 0, ("sad",), "hh", 0, 0, (0, 0))
        gf = ("gf", 0, "f32")
        lr = ("lr", gf)

        def scored(maps, where):
            rig.check_record(de.Score_GPU(S.GIF), ("score", S.GIF, maps, 0), where)
            m = rig.R(("score", S.GIF, maps, 0))
            for g, w in zip(de.score_maps(right=True), (m["ldisp"], m["rdisp"], m["emap"])):
                assert same(g, w), where

        rig.frame(de)
        scored(gf, "select")
        de.LRCheck_GPU(); de.FillInv_GPU()
        scored(("fill", gf, lr), "L-R check + fill")
        de.WgtMedian_GPU()
        wm = ("wm", ("fill", gf, lr), lr, 0)
        scored(wm, "weighted median")
        de.JointWMF_GPU(2)
        scored(("jw", wm, 0, 2), "JointWMF")
        de.SGBMSelect_GPU()
        scored(("sgmaps", sgm), "SGM select")
        de.upload_maps(*S.rand_maps(rig.W, rig.H, rig.D, 3)[:2])
        scored(("up", 3), "upload_maps")
        # an asynchronous record collected after two further stages: the record of the maps as they were
        de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        assert de.Score_GPU(S.GIF) is None
        de.set_option(psm.capi.PSM_OPT_ASYNC, 0)
        de.SGBMSelect_GPU(); de.LRCheck_GPU()
        rig.check_record(de.score_wait(), ("score", S.GIF, ("up", 3), 0), "score_wait")
        with pytest.raises(psm.capi.PsmError, match="psm_score_wait"):
            de.score_wait()
        scored(("sgmaps", sgm), "after the wait")


def test_mask_lifetime(psm, oracle):
    """Every writer of new maps drops the mask: FillInv and WgtMedian are refused until the next LRCheck, which then checks the maps
    that are there."""
    from primestereomatch_amd import dispest
    with Rig(psm, oracle, SHAPE_A, "f32", 107, nctx=2) as rig:
        de, other = rig.des
        R = rig.R
        sgm = ("sgm", 0, ("sad",), "hh", 0, 0, (0, 0))
        for d in rig.des:
            d.SGBM_GPU()
        gf = ("gf", 0, "f32")
        writers = {
            "DispSelect": (lambda: de.DispSelect_GPU(), gf),
            "SGBMSelect": (lambda: de.SGBMSelect_GPU(), ("sgmaps", sgm)),
            "sgbm_select_batch": (lambda: dispest.sgbm_select_batch([other, de]), ("sgmaps", sgm)),
            "upload_maps": (lambda: de.upload_maps(*S.rand_maps(rig.W, rig.H, rig.D, 4)[:2]), ("up", 4)),
            "gather": (lambda: rig.gather_into(de, 2, 7), ("gf", 2, "f32")),
            "merge": (lambda: rig.merge_into(de, 1, 5), ("gf", 1, "f32")),
            "compute_batch": (lambda: dispest.compute_batch([de]), gf),
        }
        rig.frame(de)
        for name, (write, maps) in writers.items():
            de.LRCheck_GPU()
            de.FillInv_GPU()                                                 # (with a mask: accepted)
            write()
            for call, fn in (("psm_fill_invalid", de.FillInv_GPU), ("psm_wgt_median", de.WgtMedian_GPU)):
                with pytest.raises(psm.capi.PsmError, match=call):
                    fn()
            rig.maps_are(de, maps, what=f"{name}: the maps behind the refusals")
            de.LRCheck_GPU()
            lv, rv = R(("lr", maps))
            assert same(de.lValid, lv) and same(de.rValid, rv), name
            de.FillInv_GPU()
            rig.maps_are(de, ("fill", maps, ("lr", maps)), what=f"{name}: fill")
        # JointWMF filters in place and keeps the mask it found
        de.DispSelect_GPU(); de.LRCheck_GPU(); de.JointWMF_GPU(2); de.FillInv_GPU()
        rig.maps_are(de, ("fill", ("jw", gf, 0, 2), ("lr", gf)), what="fill behind JointWMF")


def test_batch_tables_wls_reproject_and_pp(psm, oracle):
    """The device tables of psm_wls_filter_batch, psm_reproject_batch and psm_post_process_batch, as test_batch_tables_sgm_and_score
    for the older ones: three members; one gives back its scratch and gets new buffers; two in another order; a member that changed
    lambda and sigma only; a member alone; the first context of one batch as the last of the next; and a member without an SGM result,
    which makes the SGM-source batches refuse with every other member's planes still what they were."""
    from primestereomatch_amd import dispest
    capi = psm.capi
    with Rig(psm, oracle, SHAPE_B, "f32", 109) as rig:
        a, b, c = rig.des
        R = rig.R
        pars = [S.WLS_PARAMS[0], S.WLS_PARAMS[1], S.WLS_PARAMS[2]]          # one iteration count, three lambdas and sigmas
        up = [("up", 20 + k) for k in range(3)]
        sgm = [("sgm", k, ("sad",), "hh", 0, 0, (0, 0)) for k in range(3)]
        maps = list(up)
        for k, de in enumerate(rig.des):
            de.setInputImages(*rig.data.pairs[k])
            de.setReprojection(S.q_matrix(k % 2), S.Q_CROPS[k % 2], S.Z_RANGES[k % 2])
            de.setWLS(*pars[k])
            de.upload_maps(*S.rand_maps(rig.W, rig.H, rig.D, 20 + k)[:2])

        def wls_e(k):
            return ("wls", ("d16", sgm[k]), -16, ("guide", "pair", k), pars[k])

        def depth_e(k, gif=False):
            return ("depth", ("gif", maps[k]) if gif else ("d16", sgm[k]), None if gif else -16, k % 2, k % 2, ("guide", "pair", k))

        def wls_run(ks):
            for k, m in zip(ks, dispest.wls_batch([rig.des[k] for k in ks], capi.PSM_WLS_SGM)):
                assert same(m, R(wls_e(k))["disp"]), ("wls_batch", ks, k)
                rig.wls_is(rig.des[k], wls_e(k), ("wls_batch", ks, k))

        def depth_run(ks, outs, gif=False):
            counts = dispest.reproject_batch([rig.des[k] for k in ks], capi.PSM_DEPTH_GIF if gif else capi.PSM_DEPTH_SGM, outs)
            for k, n in zip(ks, counts):
                assert n == len(R(depth_e(k, gif))["cloud"]), ("reproject_batch", ks, k)
                rig.depth_is(rig.des[k], depth_e(k, gif), outs, ("reproject_batch", ks, k))

        def pp_run(ks, stages):
            dispest.post_process_batch([rig.des[k] for k in ks], bool(stages & S.LR), bool(stages & S.FILL), bool(stages & S.WM))
            for k in ks:
                lr = ("lr", maps[k])
                if stages & S.FILL:
                    maps[k] = ("fill", maps[k], lr)
                if stages & S.WM:
                    maps[k] = ("wm", maps[k], lr, k)
                rig.maps_are(rig.des[k], maps[k], what=("post_process_batch", ks, k))
                if stages == S.LR:
                    assert all(same(g, w) for g, w in zip(rig.des[k].download_valid(), R(lr))), ("post_process_batch", ks, k)

        for de, m, e in zip(rig.des, dispest.sgbm_batch([a, b, c]), sgm):
            assert same(m, R(e)["d16"])
        wls_run((0, 1, 2)); depth_run((0, 1, 2), 7); pp_run((0, 1, 2), S.LR | S.FILL)
        b.release_scratch()                                                  # b's planes of all three stages go; its maps stay
        assert same(b.SGBM_GPU(), R(sgm[1])["d16"])
        wls_run((2, 1)); depth_run((2, 1), S.CLOUD | S.Z); pp_run((2, 1), S.LR | S.FILL | S.WM)
        rig.wls_is(a, wls_e(0), "a, not in the batch"); rig.depth_is(a, depth_e(0), 7, "a, not in the batch"); rig.maps_are(a, maps[0])
        pars[1] = (123.0, 7.0, 3)                                            # lambda and sigma only: the entry's lambdas, b's weight table
        b.setWLS(*pars[1])
        wls_run((2, 1))
        wls_run((1,)); depth_run((1,), S.XYZ, gif=True); pp_run((1,), S.LR)
        wls_run((1, 2, 0)); depth_run((1, 2, 0), S.CLOUD, gif=True); pp_run((1, 2, 0), S.LR)      # a: first of the first batches, last here
        b.release_scratch()
        # (b's SGM result went with its scratch: the SGM-source batches must refuse it, naming the call)
        with pytest.raises(capi.PsmError, match="psm_wls_filter_batch"):
            dispest.wls_batch([c, b, a], capi.PSM_WLS_SGM)
        with pytest.raises(capi.PsmError, match="psm_reproject_batch"):
            dispest.reproject_batch([c, b, a], capi.PSM_DEPTH_SGM, 7)
        for k in (0, 2):
            rig.wls_is(rig.des[k], wls_e(k), "behind the refusals"); rig.depth_is(rig.des[k], depth_e(k, gif=True), S.CLOUD, "behind the refusals")
        for call, fn in (("psm_wls_download", b.wls_map), ("psm_reproject_download_cloud", b.cloud)):
            with pytest.raises(capi.PsmError, match=call):
                fn()
        wls_run((2, 0)); depth_run((0, 2), 7)


def test_published_map_lifetime(psm, oracle):
    """Which int16 map and which invalid value the SGM sources of psm_score and psm_reproject read (psm_ctx.h: sgm_stage_map,
    wls_published, sgm_source_map, sgm_source_invalid), stepped through: hook plane on or off, publishing on or off, a compute or
    none, psm_release_scratch.  At every stop the score record and planes of both SGM sources, the dense planes and the cloud."""
    capi = psm.capi
    with Rig(psm, oracle, SHAPE_A, "f32", 110, nctx=1) as rig:
        de, R, D = rig.des[0], rig.R, rig.D
        de.setReprojection(S.q_matrix(0), S.Q_CROPS[0], S.Z_RANGES[0])
        de.set_truth(*rig.data.truths[0])
        guide = ("guide", "pair", 0)
        sgm0, sgm2 = ("sgm", 0, ("sad",), "hh", 0, 0, (0, 0)), ("sgm", 0, ("sad",), "hh", 2, D - 4, (0, 0))
        hook = ("hook", 7, -16)

        def stop(src, inv, where):
            for source in (S.SGM, S.SGM_INT):
                e = ("score", source, src, 0)
                rig.check_record(de.Score_GPU(source), e, where)
                ld, em = de.score_maps()
                assert same(ld, R(e)["ldisp"]) and same(em, R(e)["emap"]), where
            e = ("depth", ("d16", src), inv, 0, 0, guide)
            assert de.Reproject_GPU(capi.PSM_DEPTH_SGM, 7) == len(R(e)["cloud"]), where
            rig.depth_is(de, e, 7, where)

        def wls(src, inv, where):
            e = ("wls", ("d16", src), inv, guide, S.WLS_DEFAULT)
            de.WLS_GPU(capi.PSM_WLS_SGM)
            rig.wls_is(de, e, where)
            return e

        assert same(de.SGBM_GPU(), R(sgm0)["d16"])
        stop(sgm0, -16, "a compute")
        w0 = wls(sgm0, -16, "the filter of the compute's map")
        stop(sgm0, -16, "a WLS result that is not published")
        de.wls_publish(True)
        stop(w0, -16, "published")
        de.upload_sgm_map(R(hook)["d16"])
        stop(hook, -16, "the hook plane wins over a published result")
        w1 = wls(hook, -16, "the filter reads the hook plane")
        stop(hook, -16, "... which still wins")
        de._ck(de._lib.psm_sgm_set_range(de._h, 3, 0), "set_range")
        stop(hook, 32, "the hook plane's invalid value is the current setting's")
        de.upload_sgm_map(None)
        stop(w1, -16, "the hook dropped: the published result with the invalid value it was made with")
        assert same(de.SGBM_GPU(min_disparity=2, num_disparities=D - 4), R(sgm2)["d16"])
        stop(w1, -16, "a compute with another min_disparity: the published map keeps its own invalid value")
        w2 = wls(sgm2, 16, "published, the filter still reads the SGM stage's map, never its own")
        stop(w2, 16, "the new result is the published one")
        de.wls_publish(False)
        stop(sgm2, 16, "publishing off: the compute's map with its range's invalid value")
        de.wls_publish(True)
        de.release_scratch()                                                 # the compute, the WLS planes and publishing go
        for call, fn in (("psm_score", lambda: de.Score_GPU(S.SGM)), ("psm_reproject", lambda: de.Reproject_GPU(capi.PSM_DEPTH_SGM, 7)),
                         ("psm_wls_filter", lambda: de.WLS_GPU(capi.PSM_WLS_SGM)), ("psm_wls_publish", lambda: de.wls_publish(True))):
            with pytest.raises(capi.PsmError, match=call):
                fn()
        de.upload_sgm_map(R(hook)["d16"])
        stop(hook, 16, "after the release: the hook plane alone, the setting is still (2, D - 4)")
        de.upload_sgm_map(None)
        assert same(de.SGBM_GPU(), R(sgm0)["d16"])
        stop(sgm0, -16, "the release switched publishing off: the compute's map again")


def test_guide_and_colours_follow_the_pair(psm, oracle):
    """The left image that guides psm_wls_filter and colours the cloud (psm_ctx.h: colour_of) is the current pair's at the time of the
    call - a u8 pair, a float pair quantised, a rectified frame; a staged pair counts from its adoption on - and under an SGM source
    the left plane of a gray compute, whichever map is read."""
    capi = psm.capi
    with Rig(psm, oracle, SHAPE_A, "f32", 111, nctx=1) as rig:
        de, R = rig.des[0], rig.R
        de.setReprojection(S.q_matrix(0), S.Q_CROPS[0], S.Z_RANGES[0])
        hook = ("hook", 9, -16)
        de.upload_sgm_map(R(hook)["d16"])

        def both(guide, where, src=hook):
            we = ("wls", ("d16", src), -16, guide, S.WLS_DEFAULT)
            de.WLS_GPU(capi.PSM_WLS_SGM)
            rig.wls_is(de, we, where)
            e = ("depth", ("d16", src), -16, 0, 0, guide)
            assert de.Reproject_GPU(capi.PSM_DEPTH_SGM, S.CLOUD | S.Z) == len(R(e)["cloud"]), where
            rig.depth_is(de, e, S.CLOUD | S.Z, where)
            return we

        both(("guide", "pair", 0), "the constructor's pair")
        de.setInputImages(*rig.data.pairs[1])
        both(("guide", "pair", 1), "a u8 pair")
        de.setInputImages(*rig.data.float_pair(2))
        both(("guide", "fpair", 2), "a float pair")
        de.setInputFrame(rig.data.frame)
        rect = both(("guide", "pair", S.RECT), "a rectified frame")
        de.setInputImages_async(*rig.data.pairs[0])
        both(("guide", "pair", S.RECT), "a staged pair is not the current one")
        rig.asynchronous(de, lambda: de.WLS_GPU(capi.PSM_WLS_SGM))            # an asynchronous run, then a staged upload next to it
        de.setInputImages_async(*rig.data.pairs[1])
        de.wls_wait()
        rig.wls_is(de, rect, "the asynchronous run read the frame, not the pair staged behind it")
        assert rig.asynchronous(de, lambda: de.Reproject_GPU(capi.PSM_DEPTH_SGM, S.CLOUD)) is None
        de.setInputImages_async(*rig.data.pairs[1])
        e = ("depth", ("d16", hook), -16, 0, 0, ("guide", "pair", S.RECT))
        assert de.reproject_wait() == len(R(e)["cloud"])
        rig.cloud_is(de, e, "the asynchronous cloud took the frame's colours")
        rig.frame(de)                                                        # CostConst adopts the staged pair
        both(("guide", "pair", 1), "adopted")
        gray = ("sgm", ("g", 2), ("sad",), "hh", 0, 0, (0, 0))
        assert same(de.SGBM_GPU(gray=rig.data.gray(2)), R(gray)["d16"])
        both(("guide", "gray", 2), "a gray compute: its left plane, though the hook plane is the map")
        de.upload_sgm_map(None)
        both(("guide", "gray", 2), "... and with its own map", src=gray)
        de.WLS_GPU(capi.PSM_WLS_GIF)                                          # the GIF source keeps the pair
        rig.wls_is(de, ("wls", ("gif", ("gf", 1, "f32"), None), -16, ("guide", "pair", 1), S.WLS_DEFAULT), "the GIF source")
        colour = ("sgm", 1, ("sad",), "hh", 0, 0, (0, 0))
        assert same(de.SGBM_GPU(), R(colour)["d16"])
        both(("guide", "pair", 1), "a 3-channel compute brings the SGM source back to the pair", src=colour)
