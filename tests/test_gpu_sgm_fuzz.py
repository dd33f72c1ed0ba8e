"""-m gpu seeded sweep of the semi-global matching stage (psm_sgm_compute, psm_sgm_compute_gray, psm_sgm_compute_batch) against
its definitions, the numpy models tests/sgm_model.py, sgm_bt_model.py and speckle_model.py: random geometries around the tile,
segment and lane seams with adversarial content (tests/fuzz_inputs.py; its conditions are held by tests/test_fuzz_inputs.py on
the CPU), random settings, both pixel costs, the speckle filter, single calls and batches.  Everything is integer: the prefiltered
planes, C, S, the component sizes and the int16 map must equal the model with 0 differing elements - there is no tolerance anywhere
in this file.

What the hand-picked shapes of test_gpu_sgm*.py do not reach and this file does:
  * the unpredicated ALL form of k_sgm_path / k_sgm_select with padding lanes, D in 61..63, 125..127, 253..255
  * S = 8 * 65535 = 524280, the largest sum psm_sgm_set_params admits, in the packed key (S << 8 | d) of k_sgm_select, and
    pairs whose smallest S over d is itself above 2^18 (the winner's key needs the 19th bit)
  * exact ties of S (constant pairs, stripes), minS = 0 in the uniqueness test, den clamped to 1
  * float pairs that are no byte / 255: exact .5 products, values below 0 and above 1, infinities, -0.0, NaN
  * SGM_TX = 32, SGM_BT_TX = 128, SGM_BT_YS = 32 and SGM_U = 8 seams under every block size and both costs"""
import numpy as np
import pytest

import fuzz_inputs as F
import sgm_bt_model as B
import sgm_model as M
import speckle_model as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def model(l, r, D, kw):
    """sgm_bt_model.sgm when kw holds a cap, else sgm_model.sgm"""
    return B.sgm(l, r, D, **kw) if kw.get("pre_filter_cap") else M.sgm(l, r, D, **{k: v for k, v in kw.items() if k != "pre_filter_cap"})


def differing(name, de, ref, disp, speckle=(0, 0)):
    """The planes (where the cost has them), C, S, the component sizes (where the filter ran) and the map of the last compute of
    `de` against a model result -> the counts of differing elements, printed."""
    want, sizes = K.sgbm_speckle(ref["disp"], *speckle)
    Cd, Sd = de.sgm_costs()
    assert disp.dtype == np.int16 and Cd.dtype == np.uint16 and Sd.dtype == np.uint32
    pairs = [("C", Cd, ref["C"]), ("S", Sd, ref["S"]), ("map", disp, want)]
    if "planes" in ref:
        pairs = [("planes l", de.sgm_prefiltered(0), ref["planes"][0]), ("planes r", de.sgm_prefiltered(1), ref["planes"][1])] + pairs
    if sizes is not None:
        pairs.append(("sizes", de.sgm_speckle_sizes(), sizes))
    n = {}
    for what, a, b in pairs:
        assert a.shape == b.shape, (what, a.shape, b.shape)
        n[what] = int(np.count_nonzero(a != b))
    print(f"[sgm-fuzz] {name}: differing elements {n}  (valid {ref['valid'].mean():.3f}, max L_r {ref['max_l']}, max S {int(ref['S'].max())})")
    return n


def where(de, ref):
    """For a failing case: the first differing voxels of S as (y, x, d)"""
    Sd = de.sgm_costs()[1]
    return np.argwhere(Sd != ref["S"])[:8].tolist()


def run_single(psm, W, H, D, seed, bt):
    kind, l, r, kw, gray, speckle = F.sgm_case(W, H, D, seed, bt)
    g = (np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])) if gray else None
    ref = model(*(g or (l, r)), D, kw)
    with psm.DispEst(l, r, D) as de:
        disp = de.SGBM_GPU(gray=g, speckle_window_size=speckle[0], speckle_range=speckle[1], **kw)
        n = differing(f"{W}x{H}x{D} {kind} {kw} gray {gray} speckle {speckle}", de, ref, disp, speckle)
        assert not any(n.values()), (n, where(de, ref))


@pytest.mark.parametrize("W,H,D,seed", F.sad_cases())
def test_random_geometry_sad(psm, W, H, D, seed):
    run_single(psm, W, H, D, seed, bt=False)


@pytest.mark.parametrize("W,H,D,seed", F.bt_cases())
def test_random_geometry_bt(psm, W, H, D, seed):
    run_single(psm, W, H, D, seed, bt=True)


@pytest.mark.parametrize("bs", [1, 3, 5, 7])
@pytest.mark.parametrize("cap", [0, 63])
def test_tile_and_path_seams_under_every_block_size(psm, bs, cap):
    """Widths at SGM_TX = 32 with every block size, on noise (a block that reads across the tile's edge reads unrelated bytes);
    H = 8 is a straight path of exactly SGM_U steps, 16 and 17 stand at the entry condition of the path's main loop."""
    rng = np.random.default_rng(1000 * cap + bs)
    kw = dict(block_size=bs, pre_filter_cap=cap)
    for W, H, D in ((31, 8, 5), (32, 16, 31), (33, 17, 33), (16, 33, 4), (17, 9, 17), (65, 8, 7)):
        l, r = F.sgm_content("noise", W, H, D, rng)
        ref = model(l, r, D, kw)
        with psm.DispEst(l, r, D) as de:
            n = differing(f"{W}x{H}x{D} bs {bs} cap {cap}", de, ref, de.SGBM_GPU(**kw))
            assert not any(n.values()), (n, where(de, ref))


@pytest.mark.parametrize("W,H,D,d_star,bs", F.SATURATING_CASES)
def test_saturating_pairs_reach_the_packing_bound(psm, W, H, D, d_star, bs):
    """L_r = 65535 on every path and S = 524280 = 8 * 65535 on the device: a path cost kept in 16 bits with an off-by-one, or a
    sum or rival product that loses its top bit, fails here.  (The winner's S is small on these pairs, so the d they select does
    not need the key's 19th bit: test_minimum_of_s_above_2_pow_18 is the test of that.)  D = 2, 7, 6: one disparity per lane;
    D = 130: four."""
    l, r = F.saturating_pair(W, H, D, d_star)
    kw = F.saturating_params(bs)
    ref = M.sgm(l, r, D, **kw)
    print(f"[sgm-fuzz] saturating {W}x{H}x{D}: model max L_r {ref['max_l']}  max S {int(ref['S'].max())}")
    assert ref["max_l"] == 65535 and int(ref["S"].max()) == 8 * 65535 == 524280
    with psm.DispEst(l, r, D) as de:
        for u in (10, 99, 0):
            best, minS, unique, d16 = M.select(ref["S"], u)
            _, valid = M.consistency(best, minS, unique, d16, 1)
            ru = dict(ref, disp=np.where(valid, d16, M.INVALID).astype(np.int16), valid=valid)
            n = differing(f"saturating {W}x{H}x{D} bs {bs} uniqueness {u}", de, ru, de.SGBM_GPU(uniqueness_ratio=u, **kw))
            assert not any(n.values()), (n, where(de, ru))


@pytest.mark.parametrize("W,H,D", F.HIGH_FLOOR_CASES)
def test_minimum_of_s_above_2_pow_18(psm, W, H, D):
    """The saturating pairs reach the largest S, but their winner's S is small: a packed key with 18 bits for S would still pick
    the right d there.  Here the winner's own S is at and above 2^18 (test_fuzz_inputs.py holds the pair to that): with the
    tests off every pixel shows best and the sub-pixel step, which read minS back from the key; at the default ratio every
    pixel has a rival by the true minS and the map is -16 throughout."""
    l, r = F.high_floor_case(W, H, D)
    with psm.DispEst(l, r, D) as de:
        for extra in (dict(uniqueness_ratio=0, disp12_max_diff=-1), dict(), dict(uniqueness_ratio=50, disp12_max_diff=0)):
            kw = dict(F.HIGH_FLOOR_PARAMS, **extra)
            ref = M.sgm(l, r, D, **kw)
            n = differing(f"high floor {W}x{H}x{D} {extra}", de, ref, de.SGBM_GPU(**kw))
            assert not any(n.values()), (n, where(de, ref))


@pytest.mark.parametrize("kind,W,H,D,seed", F.TIE_CASES)
def test_ties_on_the_device(psm, kind, W, H, D, seed):
    """Constant pairs, exact shifts and periodic stripes: the lowest-d rule in the low byte of the packed key, minS = 0 in the
    uniqueness test, den clamped to 1 - under both costs, with and without the uniqueness test."""
    l, r = F.tie_pair(kind, W, H, D, seed)
    with psm.DispEst(l, r, D) as de:
        for kw in (dict(), dict(pre_filter_cap=63), dict(uniqueness_ratio=0, disp12_max_diff=-1), dict(pre_filter_cap=15, uniqueness_ratio=99)):
            ref = model(l, r, D, kw)
            n = differing(f"{kind} {W}x{H}x{D} {kw}", de, ref, de.SGBM_GPU(**kw))
            assert not any(n.values()), (n, where(de, ref))


@pytest.mark.parametrize("W,H,D,seed", F.FLOAT_CASES)
def test_float_pairs_with_values_outside_the_bytes(psm, W, H, D, seed):
    """rint, not floor(x + 0.5); saturation at both ends; NaN -> 0: the float pair gives the model's result on the float images,
    which is the device's own result on quantise(pair) uploaded as bytes."""
    rng = np.random.default_rng(seed)
    l, r = F.sgm_content("synth", W, H, D, rng)
    lf, rf = F.float_pair(l, r, rng)
    lq, rq = M.quantise(lf), M.quantise(rf)
    assert np.count_nonzero(lq != l) > 0
    with psm.DispEst(lf, rf, D) as df, psm.DispEst(lq, rq, D) as dq:
        for kw in (dict(), dict(pre_filter_cap=63), dict(block_size=1, uniqueness_ratio=0)):
            ref = model(lf, rf, D, kw)
            mf, mq = df.SGBM_GPU(**kw), dq.SGBM_GPU(**kw)
            n = differing(f"float {W}x{H}x{D} {kw}", df, ref, mf)
            assert not any(n.values()), (n, where(df, ref))
            assert np.array_equal(mf, mq)
            for a, b in zip(df.sgm_costs(), dq.sgm_costs()):
                assert np.array_equal(a, b)
            if "pre_filter_cap" in kw:
                assert np.array_equal(df.sgm_prefiltered(0), dq.sgm_prefiltered(0)) and np.array_equal(df.sgm_prefiltered(1), dq.sgm_prefiltered(1))


@pytest.mark.parametrize("W,H,D,kinds,seed", F.sgm_batches(8, 31337))
def test_random_batches(psm, W, H, D, kinds, seed):
    """Pairs of different kinds in one set of launches, the settings shared: every context equals the model and its own single
    call."""
    from primestereomatch_amd import dispest
    pairs, kw, speckle = F.sgm_batch_case(W, H, D, kinds, seed)
    skw = dict(kw, speckle_window_size=speckle[0], speckle_range=speckle[1])
    des = [psm.DispEst(l, r, D) for l, r in pairs]
    try:
        maps = dispest.sgbm_batch(des, **skw)
        for kind, (l, r), de, disp in zip(kinds, pairs, des, maps):
            ref = model(l, r, D, kw)
            n = differing(f"batch of {len(kinds)} {W}x{H}x{D} {kind} {kw} speckle {speckle}", de, ref, disp, speckle)
            assert not any(n.values()), (n, where(de, ref))
            with psm.DispEst(l, r, D) as one:
                assert np.array_equal(one.SGBM_GPU(**skw), disp)
                for a, b in zip(one.sgm_costs(), de.sgm_costs()):
                    assert np.array_equal(a, b)
                if speckle[0]:
                    assert np.array_equal(one.sgm_speckle_sizes(), de.sgm_speckle_sizes())
                if "pre_filter_cap" in kw:
                    assert np.array_equal(one.sgm_prefiltered(0), de.sgm_prefiltered(0)) and np.array_equal(one.sgm_prefiltered(1), de.sgm_prefiltered(1))
    finally:
        for de in des:
            de.close()
