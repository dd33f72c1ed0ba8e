"""-m gpu: a batch of ONE against the single call, stage by stage - the default path (prep, guidance, fused select filter,
reduction), SGM with the speckle filter on, its map select, score, depth, WLS.  The two reach their pair's record through different
sources (psm_kernels.h, Recs: the single call passes it by value in the kernarg, the batch - of one too - reads the device table),
launch by launch the same kernels: every output must be equal in every bit, and equal to the stage's numpy model (the default
path: the CPU oracle).  No tolerance anywhere in this file.

Shapes: the smallest image a context takes, 8 x 8, and 65 x 9 - one row past the 64-line group of the WLS passes, and inside one
256-pixel tile of the depth, WLS and score kernels at 8 x 8 but across three of them at 65 x 9.  SGM runs them with 2 and 9
disparities: a context takes no max_disp above its width (psm_create), and the stage needs two.  The default path has shapes of
its own (DEFAULT_SHAPES)."""
import os

import numpy as np
import pytest

import depth_model as DM
import score_model as SM
import sgm_bt_model as B
import sgm_maps_model as MM
import sgm_model as M
import speckle_model as K
import wls_model as WM
from conftest import GOLDEN
import test_gpu_depth as TD
import test_gpu_score as TS
import test_gpu_wls as TW

pytestmark = pytest.mark.gpu

SHAPES = ((8, 8, 2), (65, 9, 9))


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@pytest.fixture(scope="module")
def cal():
    from primestereomatch_amd import rectify
    return rectify.read_opencv_yaml(os.path.join(GOLDEN, "zed_extrinsics.yml"))


def rnd(seed):
    return np.random.default_rng(seed)


# ---- the default path: psm_cost_construct + psm_cost_filter + psm_disp_select against psm_compute_batch ----
# 8 x 8 x 8: the smallest context - one guidance strip, one column group, one partial 4-row record of the reduction; 57 x 9: two
# 56-column guidance strips, H no multiple of 4; 108 x 9 x 12: the narrow layout's three 50-column groups.  (With 2 disparities an
# 8 x 8 map would be constant, and a constant map cannot tell a wrong pointer.)
DEFAULT_SHAPES = ((8, 8, 8), (57, 9, 8), (108, 9, 12))
SEEDS = (1, 2, 3)
TWO_PHASE_ON, MATERIALISE_COSTS = 1048576, 128           # PSM_FLAG_* (include/primesm_hip.h)
_default_refs = {}


def default_refs(oracle, W, H, D, dtype):
    """the pairs of SEEDS and the oracle's maps of each: computed once per shape and mode, shared by the tests below, never written to"""
    key = (W, H, D, dtype)
    if key not in _default_refs:
        from primestereomatch_amd import synth
        pairs = [synth.make_pair(W, H, D, seed)[:2] for seed in SEEDS]
        pipe = oracle.pipeline_u8 if dtype == "u8" else oracle.pipeline_f32
        maps = []
        for l, r in pairs:
            ref = pipe(l, r, D, threads=2)
            maps.append((ref["ldisp"], ref["rdisp"]))
            for m in maps[-1]:
                m.setflags(write=False)
                assert len(np.unique(m)) >= 2, "a constant map cannot tell a wrong pointer"
        _default_refs[key] = (pairs, maps)
    return _default_refs[key]


def guidance(de):
    """all 14 planes of both images, as bit patterns (an 8-bit context keeps a pixel's bytes in GrdX's slot: not a number)"""
    return [de.download_guidance(side).view(np.uint32).copy() for side in (0, 1)]


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("flags", (0, TWO_PHASE_ON))
@pytest.mark.parametrize("dtype", ("f32", "u8"))
@pytest.mark.parametrize("W,H,D", DEFAULT_SHAPES)
def test_default_path(psm, oracle, W, H, D, dtype, flags):
    from primestereomatch_amd.dispest import compute_batch
    capi = psm.capi
    pairs, want = default_refs(oracle, W, H, D, dtype)
    single = []                                                                  # per pair: (maps, guidance) of the three single calls
    # the batches run on contexts of their own that never saw a single call: outputs they did not write could not come out equal
    with psm.DispEst(*pairs[0], D, dtype=dtype) as one:
        one.set_option(capi.PSM_OPT_FLAGS, flags)
        for (l, r), w in zip(pairs, want):
            one.setInputImages(l, r)
            one.CostConst_GPU(); one.CostFilter_GPU(); one.DispSelect_GPU()
            single.append(((one.lDisMap.copy(), one.rDisMap.copy()), guidance(one)))
            assert same(single[-1][0], w)
    members = [psm.DispEst(l, r, D, dtype=dtype) for l, r in pairs]
    try:
        for de in members:
            de.set_option(capi.PSM_OPT_FLAGS, flags)
        compute_batch(members[:1])                                               # a batch of one reads the device table
        assert same(members[0].download_maps(), single[0][0]) and same(members[0].download_maps(), want[0])
        assert same(guidance(members[0]), single[0][1])
        compute_batch(members)                                                   # the three pairs in one set of launches
        for de, (maps, planes), w in zip(members, single, want):
            assert same(de.download_maps(), maps) and same(de.download_maps(), w)
            assert same(guidance(de), planes)
    finally:
        for de in members:
            de.close()


def test_one_volume_reduction(psm, oracle):
    """psm_cost_filter_side over a materialised volume: the one-volume plane form and the reduction of ONE side (grid y = 1), whose
    record carries the context's scratch and the side's half of the key planes"""
    W, H, D = 57, 9, 8
    pairs, want = default_refs(oracle, W, H, D, "f32")
    with psm.DispEst(*pairs[0], D) as de:
        de.set_option(psm.capi.PSM_OPT_FLAGS, MATERIALISE_COSTS)
        de.CostConst_GPU()
        de.CostFilter_side(0); de.CostFilter_side(1)
        de.DispSelect_GPU()
        assert same((de.lDisMap, de.rDisMap), want[0])


def test_prep_of_a_row_stripe(psm, oracle):
    """an 8-bit context prepares the rows of its stripe only (k_prep, k_prep_u8: the first row is an argument), then the whole image"""
    W, H, D = 57, 40, 8
    pairs, want = default_refs(oracle, W, H, D, "u8")
    with psm.DispEst(*pairs[0], D, dtype="u8") as de:
        de.set_rows(11, 23)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_device()
        assert same([m[11:23] for m in de.download_maps()], [m[11:23] for m in want[0]])
        de.set_rows(0, 0)
        for k in (0, 1):                                                         # whole-image frames, of this pair and of a new one
            de.setInputImages(*pairs[k])
            de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
            assert same((de.lDisMap, de.rDisMap), want[k])


@pytest.mark.parametrize("cap", (0, 63))
@pytest.mark.parametrize("W,H,D", SHAPES)
def test_sgm_with_the_speckle_filter(psm, W, H, D, cap):
    from primestereomatch_amd import dispest
    g = rnd(W + cap)
    l = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = np.roll(l, -1, axis=1)                                                   # a shifted copy: most pixels match, so components form
    r[::3] = g.integers(0, 256, r[::3].shape, dtype=np.uint8)                    # ... and every third row does not: speckles
    kw = dict(speckle_window_size=6, speckle_range=0)                            # range 0: only equal d16 values connect
    if cap:
        kw["pre_filter_cap"] = cap
    ref = B.sgm(l, r, D, pre_filter_cap=cap) if cap else M.sgm(l, r, D)
    want, sizes = K.sgbm_speckle(ref["disp"], 6, 0)
    with psm.DispEst(l, r, D) as one, psm.DispEst(l, r, D) as member:
        single = one.SGBM_GPU(**kw)
        batch = dispest.sgbm_batch([member], **kw)[0]
        assert single.dtype == np.int16 and np.array_equal(batch, single) and np.array_equal(batch, want)
        for a, b, m in zip(member.sgm_costs(), one.sgm_costs(), (ref["C"], ref["S"])):
            assert np.array_equal(a, b) and np.array_equal(a, m)
        zb = member.sgm_speckle_sizes()
        assert np.array_equal(zb, one.sgm_speckle_sizes()) and np.array_equal(zb, sizes)
        if cap:
            for side in (0, 1):
                pb = member.sgm_prefiltered(side)
                assert np.array_equal(pb, one.sgm_prefiltered(side)) and np.array_equal(pb, ref["planes"][side])
    assert W == 8 or (want != ref["disp"]).sum() > 50                            # at 65 x 9 the filter removes speckles (8 x 8 x 2 is one component)


@pytest.mark.parametrize("W,H,D", SHAPES)
def test_sgm_map_select(psm, W, H, D):
    from primestereomatch_amd import dispest
    l, r = rnd(30 + W).integers(0, 256, (2, H, W, 3), dtype=np.uint8)            # unrelated images: the winners vary from pixel to pixel
    want = MM.maps(M.sgm(l, r, D)["S"], 0, D)                                    # the model's maps of the model's S
    # the batch runs on a context of its own that never saw a single call: maps it did not write could not come out equal
    with psm.DispEst(l, r, D) as one, psm.DispEst(l, r, D) as member:
        one.SGBM_GPU()
        dispest.sgbm_batch([member])
        single = [m.copy() for m in one.SGBMSelect_GPU()]
        dispest.sgbm_select_batch([member])
        batch = member.download_maps()
        for b, s, w in zip(batch, single, want):
            assert b.dtype == np.uint8 and np.array_equal(b, s) and np.array_equal(b, w)
    assert all(len(np.unique(w)) == D for w in want)                             # every disparity of the range wins somewhere


@pytest.mark.parametrize("W,H,D", SHAPES)
def test_score(psm, W, H, D):
    from primestereomatch_amd import dispest
    g = rnd(10 + W)
    maps = (g.integers(0, 256, (H, W)).astype(np.uint8), g.integers(0, 256, (H, W)).astype(np.uint8))
    d16 = g.integers(-16, 16 * 64, (H, W)).astype(np.int16)
    gt, mask = g.integers(0, 256, (H, W)).astype(np.uint8), g.choice(TS.MASK_VALUES, (H, W))
    # the batch runs on a context of its own that never saw a single call: planes it did not write could not come out equal
    with TS.blank(psm, W, H, D) as de, TS.blank(psm, W, H, D) as member:
        member.set_score_params(3, 1, SM.MASK_NONOCC)
        member.set_truth(gt, mask)
        member.upload_maps(*maps)
        member.upload_sgm_map(d16)
        for source in (SM.GIF, SM.SGM, SM.SGM_INT):
            rec, planes, _ = TS.same(de, source, maps if source == SM.GIF else d16, D, gt, mask, scale=3, thr=1)      # the single call, against the model
            brec = dispest.score_batch([member], source)[0]
            assert brec == rec
            bplanes = member.score_maps(right=source == SM.GIF)
            assert len(bplanes) == len(planes) and all(np.array_equal(a, b) for a, b in zip(bplanes, planes))


@pytest.mark.parametrize("W,H,D", SHAPES)
def test_depth(psm, cal, W, H, D):
    capi = psm.capi
    from primestereomatch_amd import dispest
    g = rnd(20 + W)
    left = TD.image(W, H, W)
    d16 = g.integers(-16, 16 * 64, (H, W)).astype(np.int16)
    lmap = g.integers(0, D, (H, W), dtype=np.uint8)
    lv = (g.random((H, W)) < 0.6).astype(np.uint8) * 255
    crop, zr = (3, 5), (0.0, 150.0)
    want = {(capi.PSM_DEPTH_SGM, False): DM.reproject(*DM.sgm_disparity(d16), cal["Q"], crop, zr, left),
            (capi.PSM_DEPTH_GIF, False): DM.reproject(*DM.gif_disparity(lmap), cal["Q"], crop, zr, left),
            (capi.PSM_DEPTH_GIF, True): DM.reproject(*DM.gif_disparity(lmap, lv), cal["Q"], crop, zr, left)}
    # the batch runs on a context of its own that never saw a single call: planes it did not write could not come out equal
    with psm.DispEst(left, left, D) as de, psm.DispEst(left, left, D) as member:
        for c in (de, member):
            c.setReprojection(cal["Q"], crop, zr)
            c.upload_sgm_map(d16)
            c.upload_maps(lmap, lmap, lv, lv)
        for (source, use_mask), model in want.items():
            for outputs in (TD.all_outputs(capi), capi.PSM_DEPTH_CLOUD):
                single = TD.fetch(de, de.Reproject_GPU(source, outputs, use_mask=use_mask))
                TD.equal(single, model)
                batch = TD.fetch(member, dispest.reproject_batch([member], source, outputs, use_mask=use_mask)[0])
                assert batch[0] == single[0]
                for a, b in zip(batch[1:], single[1:]):
                    assert (a is None and b is None) or a.tobytes() == b.tobytes()


@pytest.mark.parametrize("T", (1, 3))
@pytest.mark.parametrize("W,H,D", SHAPES)
def test_wls(psm, W, H, D, T):
    guide, v = TW.noise(W, H, W), TW.holes(W, H, W + 1)
    params = dict(lam=900.0, sigma=2.5, iterations=T)
    model = WM.wls(v, -16, DM.quantise(guide), **params)
    got = []
    for batch in (False, True):
        with psm.DispEst(guide, guide, 8) as de:                                 # (8: the context's max_disp, no part of the filter)
            de.setWLS(**params)
            de.upload_sgm_map(v)
            if batch:
                assert np.array_equal(psm.wls_batch([de])[0], model["disp"])
            else:
                de.WLS_GPU(psm.capi.PSM_WLS_SGM)
            got.append(TW.fetch(de))
            TW.equal(got[-1], model)
    TW.equal(got[1], got[0])
