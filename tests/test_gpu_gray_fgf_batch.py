"""-m gpu: psm_gray_compute_fgf_batch (dispest.gray_batch(subsample_rate=s), harness.compute_gray_batch) - the launches of
psm_gray_compute_fgf with the pair on a grid axis, the kernels reading every member's buffers through the device table of ctxs[0].
There is no tolerance anywhere: np.array_equal on maps, planes and volumes compared as bit patterns against
tests/gray_fgf_model.py and against single calls on fresh contexts.  Members are always pair(kind, W, H, seed=i) of
tests/test_gpu_gray.py with distinct seeds and every member is compared with its own model: a kernel that reads a neighbour's record
or scratch cannot pass."""
import ctypes as C

import numpy as np
import pytest

import gray_fgf_model as F
from test_gpu_gray import check_maps, same_bits
from test_gpu_gray_batch import Members, arr
from test_gpu_gray_fgf import fpair, want_maps

pytestmark = pytest.mark.gpu

RATES = (2, 4, 8)
W, H, D = 67, 45, 16


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def check_batch(psm, des, s, seeds, name="", kind="noise"):
    """one batch of the members' own pairs; every member's returned and device maps against its model"""
    ps = [fpair(kind, W, H, i) for i in seeds]
    got = psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps], subsample_rate=s)
    for i, (de, sd) in enumerate(zip(des, seeds)):
        check_maps(f"{name} s={s} member {i}/{len(des)} (seed {sd})", [m.copy() for m in got[i]], want_maps(kind, W, H, D, s, sd))
        check_maps(f"{name} member {i}: download_maps", de.download_maps(), want_maps(kind, W, H, D, s, sd))


def raw_batch(psm, des, ls, rs, stride=0, depth=0, rate=4, lmaps=None, rmaps=None, map_stride=0, n=None):
    lib = psm.capi.load()
    hs = (C.c_void_p * len(des))(*[None if d is None else d._h for d in des])
    return lib.psm_gray_compute_fgf_batch(hs, len(des) if n is None else n, ls, rs, stride, depth, rate, lmaps, rmaps, map_stride)


@pytest.fixture(scope="module")
def singles(psm):
    """member seed -> (maps, guidance, q, model) of its own single call at s = 4 on a fresh context: computed once, shared"""
    out = {}
    for seed in range(8):
        l, r = fpair("noise", W, H, seed)
        with psm.DispEst.blank(H, W, D) as de:
            maps = [m.copy() for m in de.Gray_GPU(l, r, subsample_rate=4)]
            out[seed] = (maps, de.gray_fgf_guidance(1), *de.gray_fgf_volume(1, 0, D, want_model=True))
    return out


# --------------------------------------------------------------------------------------------------------------- the pair axis

@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_pair_axis(psm, singles, n):
    """n = 1 is the table form of one pair.  Every member against its own model and its own single call: maps and hook planes."""
    s = 4
    with Members(psm, n, W, H, D) as des:
        check_batch(psm, des, s, range(n), name="in order")
        for i, de in enumerate(des):
            maps, guid, q, model = singles[i]
            check_maps(f"member {i} against its single call", de.download_maps(), maps)
            assert same_bits(de.gray_fgf_guidance(1), guid), i
            gq, gm = de.gray_fgf_volume(1, 0, D, want_model=True)
            assert same_bits(gq, q) and same_bits(gm, model), i
            l, r = fpair("noise", W, H, i)
            assert same_bits(guid, F.Side(l, r, 1, s).planes()), i
            wq, wm = F.volume(l, r, 1, s, 0, D, want_model=True)
            assert same_bits(gq, wq) and same_bits(gm, wm), i
        check_batch(psm, des[::-1], s, range(10, 10 + n), name="reversed")      # ctxs[0], the table's owner, changes


@pytest.mark.parametrize("s", [2, 8])
def test_the_other_rates(psm, s):
    with Members(psm, 3, W, H, D) as des:
        check_batch(psm, des, s, range(3))
        for i in (0, 2):
            l, r = fpair("noise", W, H, i)
            assert same_bits(des[i].gray_fgf_guidance(0), F.Side(l, r, 0, s).planes())
            assert same_bits(des[i].gray_fgf_volume(0, 1, D), F.volume(l, r, 0, s, 1, D))


def test_f32_contents(psm):
    s = 4
    kinds = ["float", "binary", "constant float"]
    ps = [fpair(k, W, H, i) for i, k in enumerate(kinds)]
    with Members(psm, 3, W, H, D) as des:
        got = psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps], subsample_rate=s)
        for i, k in enumerate(kinds):
            check_maps(f"f32 member {i} ({k})", got[i], want_maps(k, W, H, D, s, i))


# ---------------------------------------------------------------------------------------------------------------------- state

def test_a_member_with_a_pending_map_download(psm):
    """member 1's maps of an earlier call are on their way to the host when the batch is enqueued: the batch's launches, which write
    the same buffer, wait for the copy"""
    s = 4
    with Members(psm, 3, W, H, D) as des:
        check_batch(psm, des, s, range(3))
        des[1].download_maps_async()
        ps = [fpair("noise", W, H, i) for i in (5, 6, 7)]
        psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps], download=False, subsample_rate=s)
        check_maps("the pending download", des[1].download_maps_wait(), want_maps("noise", W, H, D, s, 1))
        for i, de in enumerate(des):
            check_maps(f"member {i} behind it", de.download_maps(), want_maps("noise", W, H, D, s, 5 + i))


def test_a_second_batch_shares_the_first_contexts_table(psm):
    """des[0] owns the table: a batch of (des[0], others) after (des[0], des[1], des[2]) rewrites it; then the first again; a batch
    of the full-resolution form in between uses the same table and records"""
    s = 4
    with Members(psm, 5, W, H, D) as des:
        check_batch(psm, des[:3], s, (0, 1, 2), name="first")
        check_batch(psm, [des[0], des[3], des[4]], s, (3, 4, 5), name="second")
        check_maps("a member of the first batch meanwhile", des[1].download_maps(), want_maps("noise", W, H, D, s, 1))
        check_batch(psm, des[:3], 2, (6, 7, 8), name="first again, another rate")
        from test_gpu_gray import pair, want_maps as want_gray
        ps = [pair("noise", W, H, i) for i in range(3)]
        got = psm.gray_batch(des[:3], [p[0] for p in ps], [p[1] for p in ps])
        for i in range(3):
            check_maps(f"full-resolution batch member {i}", got[i], want_gray("noise", W, H, D, i))
        with pytest.raises(psm.capi.PsmError, match="psm_gray_fgf_guidance: the planes belong to psm_gray_compute "):
            des[1].gray_fgf_guidance(0)
        check_batch(psm, des[:3], s, (0, 1, 2), name="fgf behind it")


def test_async_and_profile(psm):
    s = 4
    with Members(psm, 2, W, H, D) as des:
        for de in des:
            de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
            de.set_option(psm.capi.PSM_OPT_PROFILE, 1)
        ps = [fpair("noise", W, H, i) for i in range(2)]
        assert psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps], download=False, subsample_rate=s) == [None] * 2
        for i in (1, 0):
            check_maps(f"async member {i}", des[i].download_maps(), want_maps("noise", W, H, D, s, i))
        for de in des:
            de.synchronize()
        assert 0.0 < des[0].gray_time() < 1000.0
        with pytest.raises(psm.capi.PsmError, match="psm_gray_time: .*not timed"):
            des[1].gray_time()


def test_harness_batch_gives_the_single_records(psm):
    from primestereomatch_amd import harness
    pairs = [fpair("shifted", W, H, i) for i in range(3)]
    outs = harness.compute_gray_batch(pairs, D, lr_check=True, fill=True, subsample_rate=4)
    for i, out in enumerate(outs):
        one = harness.compute_gray(pairs[i][0], pairs[i][1], D, lr_check=True, fill=True, subsample_rate=4)
        for k in ("lDisMap_raw", "rDisMap_raw", "lValid", "rValid", "lDisMap", "rDisMap"):
            assert np.array_equal(out[k], one[k]), (i, k)
        check_maps(f"pair {i}", (out["lDisMap_raw"], out["rDisMap_raw"]), want_maps("shifted", W, H, D, 4, i))


# ------------------------------------------------------------------------------------------------------------------- refusals

def test_refusals(psm):
    n, s = 3, 4
    capi = psm.capi
    lib = capi.load()
    ps = [fpair("noise", W, H, i) for i in range(n)]
    ls, rs = arr([p[0] for p in ps]), arr([p[1] for p in ps])
    ls4, rs4 = arr([p[0] for p in ps] + [ps[0][0]]), arr([p[1] for p in ps] + [ps[0][1]])
    lms = [np.zeros((H, W), np.uint8) for _ in range(n + 1)]
    rms = [np.zeros((H, W), np.uint8) for _ in range(n + 1)]
    with Members(psm, n, W, H, D) as des:
        check_batch(psm, des, s, (10, 11, 12))
        before = [want_maps("noise", W, H, D, s, i) for i in (10, 11, 12)]

        def refused(words, members, l=ls, r=rs, stride=0, depth=0, rate=s, map_stride=0, count=None, null=False):
            k = len(members)
            assert raw_batch(psm, members, l, r, stride, depth, rate, arr(lms[:k]), arr(rms[:k]), map_stride, n=count) != 0
            msg = capi.last_error(None if null else members[0]._h)
            assert "psm_gray_compute_fgf_batch" in msg and all(w in msg for w in words), msg
            for i, de in enumerate(des):
                check_maps(f"{words}: the previous maps of member {i} stay current", de.download_maps(), before[i])

        assert lib.psm_gray_compute_fgf_batch(None, n, ls, rs, 0, 0, s, None, None, 0) != 0 and "psm_gray_compute_fgf_batch" in capi.last_error(None)
        refused(["n 0"], des, count=0, null=True)
        refused(["4097"], des, count=4097)
        refused(["context 1", "NULL"], [des[0], None, des[2]])
        refused(["context 2", "twice"], [des[0], des[1], des[0]])
        refused(["NULL"], des, l=None)
        refused(["context 1", "NULL"], des, l=arr([ps[0][0], None, ps[2][0]]))
        refused(["depth", "7"], des, depth=7)
        refused(["stride", str(W - 1)], des, stride=W - 1)
        refused(["map stride", str(W - 1)], des, map_stride=W - 1)
        for rate in (0, 3, 16):
            refused(["subsample_rate", str(rate), "{2,4,8}"], des, rate=rate)
        with psm.DispEst.blank(H, W, D, dtype="u8") as odd:
            refused(["context 3", "8-bit"], des + [odd], l=ls4, r=rs4)
        with psm.DispEst.blank(H, W + 1, D) as odd:
            refused(["context 3", "geometry"], des + [odd], l=ls4, r=rs4)
        des[2].set_rows(4, 8)
        refused(["context 2", "row stripe"], des)
        des[2].set_rows(0, 0)
        assert not any(m.any() for m in lms + rms)                            # nothing was written to the caller's maps either
        check_batch(psm, des, s, range(n), name="and the call works again")
    # too small for the rate: 40 x 12 at s = 8 (12 / 8 = 1 is not above 8 / 8)
    small = [fpair("noise", 40, 12, i) for i in range(2)]
    with Members(psm, 2, 40, 12, D) as des:
        assert raw_batch(psm, des, arr([p[0] for p in small]), arr([p[1] for p in small]), rate=8) != 0
        msg = capi.last_error(des[0]._h)
        assert "psm_gray_compute_fgf_batch: 40x12 too small for subsample_rate 8" in msg, msg
