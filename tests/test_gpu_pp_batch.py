"""-m gpu: PP::processDM's own sequence - lrCheck, fillInv, wgtMedian - of several contexts in shared launches
(psm_post_process_batch, dispest.post_process_batch) against oracle.lr_check / fill_inv / wgt_median AND against the single calls on
fresh contexts.  Every comparison is np.array_equal on all pixels of all members - maps and masks - without a tolerance.  Sweep and
evaluation counts may differ from run to run: only their sanity is asserted (-1 or 1 .. 96; the dataflow form reports -1) - but for
a batch of one, which is the single calls' launch sequence and schedule and must report their sweeps.
Inputs: tests/wmf_inputs.py.

One case cannot be built as written: histogram word seams "D in {2, 64, 65, 129, 256} at 21 x 20" - a context takes no max_disp
above its width (psm_create), so those members are 20 rows of max(21, D) columns."""
import ctypes as C
import os

import numpy as np
import pytest

import wmf_inputs as G
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LR, FILL, MED = 1, 2, 4                 # PSM_PP_LR_CHECK, PSM_PP_FILL, PSM_PP_WGT_MEDIAN
ALL = LR | FILL | MED
NO_CACHE, DATAFLOW, TWO_SWEEPS = G.FORMS["no_cache"], G.FORMS["dataflow"], G.FORMS["fallback"]
CAP = 96


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def _oracle_stages(oracle, inp, D, stages):
    maps, valid = [inp.lmap, inp.rmap], [inp.lvalid, inp.rvalid]
    if stages & LR:
        valid = list(oracle.lr_check(maps[0], maps[1]))
    if stages & FILL:
        maps = [oracle.fill_inv(maps[s], valid[s]) for s in (0, 1)]
    if stages & MED:
        maps = [oracle.wgt_median(oracle.u8_to_f32(inp.img[s]), maps[s], valid[s], D, right=bool(s)) for s in (0, 1)]
    out = tuple(np.array(a, copy=True) for a in (maps[0], maps[1], valid[0], valid[1]))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def expected(oracle):
    """(lmap, rmap, lvalid, rvalid) of the oracle's stages on an input, computed once per (input, stages); never written to."""
    cache = {}

    def get(inp, D, stages):
        key = (id(inp), D, stages)
        if key not in cache:
            cache[key] = (inp, _oracle_stages(oracle, inp, D, stages))      # (the input is kept: its id stays its own)
        return cache[key][1]
    return get


def _context(psm, inp, D, flags=0, masks=True):
    from primestereomatch_amd import capi
    de = psm.DispEst(inp.img[0], inp.img[1], D)
    try:
        if flags:
            de.set_option(capi.PSM_OPT_FLAGS, flags)
        if masks:
            de.upload_maps(inp.lmap, inp.rmap, inp.lvalid, inp.rvalid)
        else:
            de.upload_maps(inp.lmap, inp.rmap)
    except Exception:
        de.close()
        raise
    return de


def _close(des):
    for d in des:
        d.close()


def _results(d):
    """The device's maps and masks of a context, as fresh downloads."""
    lm, rm = d.download_maps()
    d._ck(d._lib.psm_download_valid(d._h, d.lValid.ctypes.data_as(C.c_void_p), d.rValid.ctypes.data_as(C.c_void_p), d.wid), "download_valid")
    return lm.copy(), rm.copy(), d.lValid.copy(), d.rValid.copy()


def _singles(psm, inp, D, stages, flags=0):
    """-> (maps and masks, sweeps) of the single calls of `stages` on a fresh context."""
    de = _context(psm, inp, D, flags, masks=not stages & LR)
    try:
        if stages & LR:
            de.LRCheck_device()
        if stages & FILL:
            de.FillInv_GPU()
        if stages & MED:
            de.WgtMedian_GPU()
        return _results(de), de.wgt_median_stats()[0]
    finally:
        de.close()


def _sane(sweeps, dataflow=False):
    assert all(s == -1 or 1 <= s <= CAP for s in sweeps), sweeps
    if dataflow:
        assert sweeps == [-1, -1]


def _same(got, want, what):
    for g, w, name in zip(got, want, ("left map", "right map", "left mask", "right mask")):
        assert np.array_equal(g, w), f"{what}: {name}: {int((g != w).sum())} pixels differ"


def _batch(psm, expected, inps, D, stages, flags=0, label="", des=None, dataflow=False, equal_sweeps=False):
    """One psm_post_process_batch of `stages` on fresh contexts of the inputs (or on `des`): every member's maps and masks equal the
    oracle's and the single calls'.  equal_sweeps: the sweeps the single calls report are the member's.  -> the sweeps per member."""
    from primestereomatch_amd import dispest
    own = des is None
    if own:
        des = [_context(psm, inp, D, flags, masks=not stages & LR) for inp in inps]
    try:
        dispest.post_process_batch(des, lr_check=bool(stages & LR), fill=bool(stages & FILL), median=bool(stages & MED))
        sweeps = []
        for i, (d, inp) in enumerate(zip(des, inps)):
            got = (d.lDisMap, d.rDisMap, d.lValid, d.rValid)
            _same(got, _results(d), f"{label} member {i} (download=True against fresh downloads)")
            _same(got, expected(inp, D, stages), f"{label} member {i} against the oracle")
            single, single_sweeps = _singles(psm, inp, D, stages, flags)
            _same(got, single, f"{label} member {i} against the single calls")
            sw = d.wgt_median_stats()[0]
            if stages & MED:
                _sane(sw, dataflow)
                _sane(single_sweeps, dataflow)
                if equal_sweeps:
                    print(f"[pp-batch] {label} member {i}: sweeps {sw}, the single calls' {single_sweeps}")
                    assert sw == single_sweeps, (label, i, sw, single_sweeps)
            sweeps.append(sw)
        print(f"[pp-batch] {label}: n = {len(des)}, stages {stages}, sweeps {sweeps}")
        return sweeps
    finally:
        if own:
            _close(des)


# ------------------------------------------------------------------------------------------ batch sizes

@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_batch_sizes(psm, expected, n):
    inps = [G.random_case(64, 65, 64, G.FRACS[i % 3], 700 + i) for i in range(n)]
    _batch(psm, expected, inps, 64, ALL, label=f"sizes n={n}")
    _batch(psm, expected, inps, 64, MED, label=f"sizes n={n} (the masks of the inputs)")


# ------------------------------------------------------------------------------------------ a batch of one (the record by value)

@pytest.mark.parametrize("form", ["sweeps", "no_cache", "fallback", "dataflow"])
def test_a_batch_of_one_in_every_form(psm, expected, form):
    """n = 1 takes the single calls' path through the batch's entry - the record in the kernarg, no device table - in each form of
    the median; its sweeps are the single calls', which follow the same schedule."""
    inp = G.random_case(64, 65, 64, 1.0, 1300)
    for stages in (ALL, MED):
        sweeps = _batch(psm, expected, [inp], 64, stages, G.FORMS[form], label=f"one, {form}, stages {stages}", dataflow=form == "dataflow",
                        equal_sweeps=True)
        if form == "fallback":
            assert sweeps == [[-1, -1]]                        # (all pixels invalid: no fixed point in two sweeps, both maps fall back)


@pytest.mark.parametrize("counts", [(8192, 0), (0, 8192)])
def test_a_batch_of_one_at_the_cache_threshold_beside_an_empty_side(psm, expected, counts):
    """8192 invalid pixels on one side - the cache's threshold and the first list of the lane form - and none on the other, which
    the one weights launch over both sides must skip."""
    H, W, D = G.COUNTED_GEO
    inp = G.counted_invalid(H, W, D, 11, counts[0], counts[1], map_seed=140)
    for form in ("sweeps", "no_cache"):
        sweeps = _batch(psm, expected, [inp], D, MED, G.FORMS[form], label=f"one, {counts}, {form}", equal_sweeps=True)
        assert sweeps[0][counts.index(0)] == 1                 # (an empty list: its first sweep changes nothing)
    _batch(psm, expected, [inp], D, FILL | MED, label=f"one, {counts}, fill + median", equal_sweeps=True)


@pytest.mark.parametrize("W,H,D", [(9, 9, 9), (64, 9, 64), (65, 9, 65)])
def test_a_batch_of_one_at_the_smallest_geometry_and_the_word_seam(psm, expected, W, H, D):
    """The smallest image the median accepts, 9 x 9, and the 64-bin word seam of the wave form's histogram, D = 64 and 65.  9 x 9
    with D = 64 cannot be built as written - a context takes no max_disp above its width (psm_create) - so 9 x 9 runs with D = 9 and
    the seam on 9 rows of D columns."""
    inp = G.random_case(W, H, D, 0.5, 1400 + D)
    _batch(psm, expected, [inp], D, ALL, label=f"one, {W}x{H} D={D}", equal_sweeps=True)
    _batch(psm, expected, [inp], D, MED, label=f"one, {W}x{H} D={D} (the masks of the input)", equal_sweeps=True)


def test_the_counters_home_through_changing_roles(psm, expected):
    """The counters, their snapshots and the events of every call lie with the call's first context.  One context runs the single
    calls, heads a batch of three (which grows the block), runs the single calls again on fresh maps, gives its scratch back and runs
    them once more, and is then a member of a batch another context heads - every step against the oracle.  (A batch of three takes
    three contexts: the one followed here and two beside it.)"""
    W, H, D = 64, 65, 64
    inps = [G.random_case(W, H, D, G.FRACS[(i + 1) % 3], 1500 + i) for i in range(3)]
    fresh = [G.random_case(W, H, D, G.FRACS[i % 3], 1600 + i) for i in range(3)]
    des = [_context(psm, inp, D, masks=False) for inp in inps]
    a = des[0]

    def singles(inp, what):
        a.upload_maps(inp.lmap, inp.rmap)
        a.LRCheck_device()
        a.FillInv_GPU()
        a.WgtMedian_GPU()
        _same(_results(a), expected(G.WmInput(inps[0].img, inp.lmap, inp.rmap, inp.lvalid, inp.rvalid, inp.pixels), D, ALL), what)
        _sane(a.wgt_median_stats()[0])

    def batch(order, maps, what):
        members = []
        for k in order:
            des[k].upload_maps(maps[k].lmap, maps[k].rmap)
            members.append(G.WmInput(inps[k].img, maps[k].lmap, maps[k].rmap, maps[k].lvalid, maps[k].rvalid, maps[k].pixels))
        _batch(psm, expected, members, D, ALL, label=what, des=[des[k] for k in order])

    try:
        singles(inps[0], "the single calls on a new context")
        batch([0, 1, 2], inps, "heading a batch of three")
        singles(fresh[0], "the single calls after heading a batch")
        a.release_scratch()
        singles(fresh[1], "the single calls after psm_release_scratch")
        batch([1, 0], fresh, "a member of another context's batch")
        batch([0], inps, "a batch of one after all of them")
    finally:
        _close(des)


# ------------------------------------------------------------------------------------------ mixed forms in one launch

@pytest.mark.parametrize("form", ["sweeps", "no_cache"])
def test_mixed_forms_in_one_launch(psm, expected, form):
    """Empty, wave-form and lane-form lists side by side (8192 invalid pixels: the first list of the lane form and the cache's
    threshold; 8257: one pixel into another block of 64)."""
    H, W, D = G.COUNTED_GEO
    counts = [(0, 0), (0, 8192), (8191, 8193), (8257, 8257)]
    inps = [G.counted_invalid(H, W, D, 11, a, b, map_seed=100 + i) for i, (a, b) in enumerate(counts)]
    sweeps = _batch(psm, expected, inps, D, MED, G.FORMS[form], label=f"mixed {form}")
    assert sweeps[0] == [1, 1] and sweeps[1][0] == 1          # (an empty list: its first sweep changes nothing)


# ------------------------------------------------------------------------------------------ histogram word seams, wrapping windows

@pytest.mark.parametrize("D", [2, 64, 65, 129, 256])
def test_histogram_word_seams(psm, expected, D):
    W, H = max(21, D), 20
    inps = [G.random_case(W, H, D, G.FRACS[i], 900 + 7 * D + i) for i in range(3)]
    _batch(psm, expected, inps, D, MED, label=f"D={D}")
    _batch(psm, expected, inps, D, ALL, label=f"D={D} all stages")


@pytest.mark.parametrize("W,H", [(9, 9), (9, 10), (19, 21)])
def test_windows_that_wrap_onto_themselves(psm, expected, W, H):
    D = min(W, 8)
    inps = [G.random_case(W, H, D, G.FRACS[i], 40 + W * H + i) for i in range(3)]
    _batch(psm, expected, inps, D, MED, label=f"{W}x{H}")
    _batch(psm, expected, inps, D, ALL, label=f"{W}x{H} all stages")


# ------------------------------------------------------------------------------------------ order and denormals

def test_order_and_denormal_sensitive_members(psm, expected):
    H, W, D = G.KNIFE_CASES[0]
    knife, den = G.knife_edge(H, W, D, 5, G.BULK_ROWS), G.denormal_windows(H, W, D, 6, G.BULK_ROWS)
    rnd = G.random_case(W, knife.lmap.shape[0], D, 0.5, 77)
    assert knife.lmap.shape == den.lmap.shape == rnd.lmap.shape
    from primestereomatch_amd import dispest
    des = [_context(psm, inp, D) for inp in (knife, den, rnd)]
    try:
        dispest.post_process_batch(des, lr_check=False, median=True)
        for name, d, inp in zip(("knife_edge", "denormal_windows", "random"), des, (knife, den, rnd)):
            want = expected(inp, D, MED)
            for s, (g, e) in enumerate(((d.lDisMap, want[0]), (d.rDisMap, want[1]))):
                p = inp.pixels[s]
                bad = int((g[p[:, 0], p[:, 1]] != e[p[:, 0], p[:, 1]]).sum()) if len(p) else 0
                print(f"[pp-batch] {name} side {s}: {len(p)} sensitive pixels, {bad} wrong; whole map {int((g != e).sum())} wrong")
                assert bad == 0
            _same((d.lDisMap, d.rDisMap, d.lValid, d.rValid), want, name)
            _sane(d.wgt_median_stats()[0])
        assert min(len(p) for p in knife.pixels) >= 8 and min(len(p) for p in den.pixels) >= 8
        single, _ = _singles(psm, knife, D, MED)
        _same((des[0].lDisMap, des[0].rDisMap, des[0].lValid, des[0].rValid), single, "knife_edge against the single call")
    finally:
        _close(des)


# ------------------------------------------------------------------------------------------ leaving the sweeps at the cap

def test_every_member_falls_back_after_two_sweeps(psm, expected):
    inps = [G.random_case(64, 65, 64, G.FRACS[1 + i % 2], 300 + i) for i in range(3)]
    sweeps = _batch(psm, expected, inps, 64, MED, TWO_SWEEPS, label="two sweeps")
    print(f"[pp-batch] two sweeps: {sweeps}")
    assert all(s in (-1, 1, 2) for sw in sweeps for s in sw)
    assert any(s == -1 for sw in sweeps for s in sw)           # (half and all pixels invalid: no fixed point in two sweeps)
    _batch(psm, expected, inps, 64, MED, DATAFLOW, label="dataflow only", dataflow=True)


def test_one_domino_beside_quick_members(psm, expected):
    """The smallest domino (9 x 800, the wave form) needs 196 synchronous sweeps: it leaves the sweeps at the cap, is restored and
    takes the dataflow form, while the control-like members (period 2) of the same geometry finish in their first sweeps."""
    name = min(G.DOMINO_CASES, key=lambda k: G.DOMINO_CASES[k][0] * G.DOMINO_CASES[k][1])
    H, W, period, seed_len, a, b = G.DOMINO_CASES[name]
    chain = G.domino(H, W, period, seed_len, a, b)
    quick = [G.domino(H, W, 2, seed_len, a, b), G.domino(H, W, 2, seed_len + 3, a, b)]
    sweeps = _batch(psm, expected, [quick[0], chain, quick[1]], 16, MED, label=f"domino {name}")
    print(f"[pp-batch] domino {name}: sweeps {sweeps}")
    assert not np.array_equal(expected(chain, 16, MED)[0], chain.lmap)
    assert all(1 <= s <= 3 for s in sweeps[0] + sweeps[2]), sweeps
    assert sweeps[1] == [-1, -1], sweeps


# ------------------------------------------------------------------------------------------ lrCheck / fillInv seams

def _rows_input(W, H, D, seed):
    """Maps for the L-R check with rows it finds wholly valid (equal constant maps), wholly invalid (values below 2) and mixed;
    masks for the fill with rows wholly invalid, wholly valid, and valid at the row's ends only."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    lmap = rng.integers(0, D, (H, W)).astype(np.uint8)
    rmap = rng.integers(0, D, (H, W)).astype(np.uint8)
    lmap[0], rmap[0] = 5, 5                    # every pixel passes
    lmap[1], rmap[1] = 1, 1                    # none does
    lmap[2] = rmap[2] = rng.integers(2, 4, W).astype(np.uint8)      # mixed: equal maps, the match is shifted
    lv = (rng.random((H, W)) < 0.5).astype(np.uint8)
    rv = (rng.random((H, W)) < 0.5).astype(np.uint8)
    for v in (lv, rv):
        v[3], v[4] = 0, 1
        v[5] = 0; v[5, 0] = v[5, -1] = 1
        v[6] = 0; v[6, 0] = 1
        v[7] = 0; v[7, -1] = 1
    return G.WmInput(img, lmap, rmap, lv, rv, (G.NO_PIXELS, G.NO_PIXELS))


@pytest.mark.parametrize("W", [63, 64, 65, 129, 257])
def test_lr_check_and_fill_seams(psm, expected, W):
    H, D = 9, 16
    inps = [_rows_input(W, H, D, 3 * W + i) for i in range(3)]
    _batch(psm, expected, inps, D, LR, label=f"W={W} lr")
    _batch(psm, expected, inps, D, LR | FILL, label=f"W={W} lr + fill")
    _batch(psm, expected, inps, D, FILL, label=f"W={W} fill on uploaded masks")
    _batch(psm, expected, inps, D, ALL, label=f"W={W} all")
    want = expected(inps[0], D, LR)
    assert want[2][0].all() and not want[2][1].any()          # (the rows are what they were built to be)


# ------------------------------------------------------------------------------------------ stage subsets

@pytest.mark.parametrize("stages", [LR, LR | FILL])
def test_subsets_without_the_median_stay_asynchronous(psm, expected, stages):
    from primestereomatch_amd import capi, dispest
    inps = [G.random_case(64, 65, 64, 0.5, 500 + i) for i in range(3)]
    des = [_context(psm, inp, 64, masks=False) for inp in inps]
    try:
        for d in des:
            d.set_option(capi.PSM_OPT_ASYNC, 1)
        dispest.post_process_batch(des, lr_check=True, fill=bool(stages & FILL), download=False)
        for d in des:
            d.synchronize()
        for i, (d, inp) in enumerate(zip(des, inps)):
            _same(_results(d), expected(inp, 64, stages), f"async member {i}")
            _same(_results(d), _singles(psm, inp, 64, stages)[0], f"async member {i} against the single calls")
    finally:
        _close(des)


@pytest.mark.parametrize("stages", [FILL | MED, MED])
def test_subsets_on_uploaded_masks(psm, expected, stages):
    inps = [G.random_case(64, 65, 64, G.FRACS[i], 600 + i) for i in range(3)]
    _batch(psm, expected, inps, 64, stages, label=f"subset {stages}")


# ------------------------------------------------------------------------------------------ refusals

def _state(d):
    return _results(d) + (d.wgt_median_stats(),)


def test_refusals_name_the_member_and_leave_everything(psm):
    from primestereomatch_amd import capi, dispest
    W, H, D = 64, 65, 64
    inps = [G.random_case(W, H, D, 0.5, 800 + i) for i in range(2)]
    des = [_context(psm, inp, D) for inp in inps]
    bad = {}
    try:
        dispest.post_process_batch(des, lr_check=False, fill=True, median=True)
        before = [_state(d) for d in des]
        bad["no mask"] = _context(psm, inps[0], D, masks=False)
        bad["no maps"] = psm.DispEst(inps[0].img[0], inps[0].img[1], D)
        bad["stripe"] = psm.DispEst(inps[0].img[0], inps[0].img[1], D)
        bad["stripe"].set_rows(0, H // 2)
        bad["stripe"].CostConst_GPU(); bad["stripe"].CostFilter_GPU(); bad["stripe"].DispSelect_GPU()
        bad["max_disp"] = psm.DispEst(inps[0].img[0], inps[0].img[1], 32)
        bad["max_disp"].upload_maps(inps[0].lmap // 2, inps[0].rmap // 2, inps[0].lvalid, inps[0].rvalid)
        bad["flags"] = _context(psm, inps[0], D, NO_CACHE)
        kept = {k: _state(bad[k]) for k in ("max_disp", "flags")}
        kept["no mask"] = tuple(a.copy() for a in bad["no mask"].download_maps())
        cases = [("no mask", des + [bad["no mask"]], dict(lr_check=False, fill=True), 2),
                 ("no maps", [des[0], bad["no maps"], des[1]], dict(lr_check=True), 1),
                 ("stripe", des + [bad["stripe"]], dict(lr_check=True), 2),
                 ("twice", des + [des[0]], dict(lr_check=True, fill=True, median=True), 2),
                 ("max_disp", [des[0], bad["max_disp"]], dict(lr_check=False, median=True), 1),
                 ("flags", des + [bad["flags"]], dict(lr_check=False, median=True), 2)]
        for name, members, kw, index in cases:
            with pytest.raises(capi.PsmError, match=rf"post_process_batch.*context {index}\b"):
                dispest.post_process_batch(members, **kw)
            for d, e in zip(des, before):
                now = _state(d)
                _same(now[:4], e[:4], f"after the refusal '{name}'")
                assert now[4] == e[4], name
            for k in ("max_disp", "flags"):
                now = _state(bad[k])
                _same(now[:4], kept[k][:4], f"the refused member after '{name}'")
                assert now[4] == kept[k][4]
            _same(bad["no mask"].download_maps(), kept["no mask"], f"the member without a mask after '{name}'")
            with pytest.raises(capi.PsmError):
                bad["no mask"].FillInv_GPU()                   # (it still has no mask)
        lib = capi.load()
        arr = (C.c_void_p * 2)(des[0]._h, des[1]._h)
        assert lib.psm_post_process_batch(arr, 0, ALL) != 0    # n = 0
        assert lib.psm_post_process_batch(arr, 4097, ALL) != 0 and lib.psm_post_process_batch(arr, 2, 0) != 0 and lib.psm_post_process_batch(arr, 2, 8) != 0
        arr = (C.c_void_p * 2)(des[0]._h, None)
        assert lib.psm_post_process_batch(arr, 2, LR) != 0
        for d, e in zip(des, before):
            now = _state(d)
            _same(now[:4], e[:4], "after n = 0 and the bad arguments")
            assert now[4] == e[4]
    finally:
        _close(des + list(bad.values()))


# ------------------------------------------------------------------------------------------ state

def test_two_calls_new_maps_another_order_singles_between(psm, expected):
    from primestereomatch_amd import dispest
    W, H, D = 64, 65, 64
    first = [G.random_case(W, H, D, G.FRACS[i % 3], 1000 + i) for i in range(3)]
    second = [G.random_case(W, H, D, G.FRACS[(i + 1) % 3], 1100 + i) for i in range(3)]
    des = [_context(psm, inp, D, masks=False) for inp in first]
    try:
        _batch(psm, expected, first, D, ALL, label="first call", des=des)
        # new maps (on the same images: the pair stays each context's own) and the members in another order, another first context
        mixed = []
        for d, inp, new in zip(des, first, second):
            d.upload_maps(new.lmap, new.rmap)
            mixed.append(G.WmInput(inp.img, new.lmap, new.rmap, new.lvalid, new.rvalid, new.pixels))
        order = [2, 0, 1]
        _batch(psm, expected, [mixed[i] for i in order], D, ALL, label="second call, another order", des=[des[i] for i in order])
        # a single psm_wgt_median on a member after a batch ...
        des[1].upload_maps(first[1].lmap, first[1].rmap, first[1].lvalid, first[1].rvalid)
        des[1].WgtMedian_GPU()
        want = expected(first[1], D, MED)
        _same(_results(des[1]), want, "a single call after a batch")
        _same(_results(des[1]), _singles(psm, first[1], D, MED)[0], "a single call after a batch against a fresh context's")
        _sane(des[1].wgt_median_stats()[0])
        # ... and a batch after singles
        for d, inp in zip(des, first):
            d.upload_maps(inp.lmap, inp.rmap, inp.lvalid, inp.rvalid)
        des[0].FillInv_GPU()
        des[0].WgtMedian_GPU()
        after_single = _results(des[0])
        _same(after_single, expected(first[0], D, FILL | MED), "singles before the batch")
        des[0].upload_maps(first[0].lmap, first[0].rmap, first[0].lvalid, first[0].rvalid)
        _batch(psm, expected, first, D, FILL | MED, label="a batch after singles", des=des)
        _same(_results(des[0]), after_single, "the batch against the same member's singles")
    finally:
        _close(des)


def test_a_pending_download_on_a_member_stream_and_shared_streams(psm, expected):
    from primestereomatch_amd import dispest
    W, H, D = 64, 65, 64
    inps = [G.random_case(W, H, D, 0.5, 1200 + i) for i in range(3)]
    des = [_context(psm, inp, D, masks=False) for inp in inps]
    try:
        des[1].download_maps_async()                           # (reads the maps as uploaded; the batch's fill must wait for it)
        dispest.post_process_batch(des, lr_check=True, fill=True, median=True, download=False)
        lm, rm = des[1].download_maps_wait()
        assert np.array_equal(lm, inps[1].lmap) and np.array_equal(rm, inps[1].rmap)
        for i, (d, inp) in enumerate(zip(des, inps)):
            _same(_results(d), expected(inp, D, ALL), f"member {i} behind a pending download")
        # the same batch under psm_share_streams
        dispest.share_streams(des)
        for d, inp in zip(des, inps):
            d.upload_maps(inp.lmap, inp.rmap)
        _batch(psm, expected, inps, D, ALL, label="shared streams", des=des)
    finally:
        _close(des)


# ------------------------------------------------------------------------------------------ harness

def test_middlebury_through_the_harness(psm):
    from primestereomatch_amd import harness
    pair = [dict(np.load(os.path.join(GOLDEN, f"{n}_pair.npz"))) for n in ("cones", "teddy")]
    outs = harness.compute_batch([(p["l_bgr"], p["r_bgr"]) for p in pair], 64, [p["gt_l"] for p in pair], [p["occl"] for p in pair],
                                 process_dm=True)
    assert len(outs) == 2
    for n, p, out in zip(("cones", "teddy"), pair, outs):
        one = harness.compute(p["l_bgr"], p["r_bgr"], 64, p["gt_l"], p["occl"], process_dm=True)
        for k in ("lDisMap", "rDisMap", "lDisMap_raw", "rDisMap_raw", "lValid", "rValid"):
            assert np.array_equal(out[k], one[k]), (n, k)
        assert out["bp_percent"] == one["bp_percent"], n
        assert not np.array_equal(out["lDisMap"], out["lDisMap_raw"])
        print(f"[pp-batch] {n}: %BP after processDM {out['bp_percent']:.2f}")
    plain = harness.compute_batch([(p["l_bgr"], p["r_bgr"]) for p in pair], 64)
    for out, ref in zip(plain, outs):                          # the default is unchanged: no raw maps, the L-R check's masks
        assert "lDisMap_raw" not in out
        assert np.array_equal(out["lValid"], ref["lValid"]) and np.array_equal(out["lDisMap"], ref["lDisMap_raw"])
