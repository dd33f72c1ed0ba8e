"""-m gpu: psm_gray_compute_batch (dispest.gray_batch, harness.compute_gray_batch) - the launches of psm_gray_compute with the pair
on a grid axis, the kernels reading every member's buffers through the device table of ctxs[0].  There is no tolerance anywhere:
np.array_equal on maps, planes and volumes compared as bit patterns against tests/gray_model.py and against single calls on fresh
contexts.  Members are always pair(kind, W, H, seed=i) of tests/test_gpu_gray.py with distinct seeds and every member is compared
with its own model: a kernel that reads a neighbour's record or scratch cannot pass.  The shapes are the smallest at which each
seam of the kernels (test_gpu_gray.py's list) can go wrong with the pair on the grid."""
import ctypes as C

import numpy as np
import pytest

import gray_model as M
import score_model as SC
from test_gpu_gray import check_maps, pair, same_bits, want_maps
from test_gpu_wls import hip_runtime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


class Members:
    """n blank objects of one geometry"""

    def __init__(self, psm, n, W, H, D, **kw):
        self.des = [psm.DispEst.blank(H, W, D, **kw) for _ in range(n)]

    def __enter__(self):
        return self.des

    def __exit__(self, *exc):
        for d in self.des:
            d.close()


def pairs_of(kinds, W, H, seeds=None):
    seeds = range(len(kinds)) if seeds is None else seeds
    return [pair(k, W, H, s) for k, s in zip(kinds, seeds)]


def check_batch(psm, des, kinds, W, H, D, seeds=None, name=""):
    """one batch of the members' own pairs; every member's returned and device maps against its model"""
    seeds = list(range(len(kinds))) if seeds is None else list(seeds)
    ps = pairs_of(kinds, W, H, seeds)
    got = psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps])
    for i, (de, k, s) in enumerate(zip(des, kinds, seeds)):
        check_maps(f"{name} {W}x{H}x{D} member {i}/{len(des)} ({k} {s})", [m.copy() for m in got[i]], want_maps(k, W, H, D, s))
        check_maps(f"{name} member {i}: download_maps", de.download_maps(), want_maps(k, W, H, D, s))


def arr(items):
    return (C.c_void_p * len(items))(*[None if x is None else (x if isinstance(x, int) else x.ctypes.data) for x in items])


def raw_batch(psm, des, ls, rs, stride=0, depth=0, lmaps=None, rmaps=None, map_stride=0, n=None):
    lib = psm.capi.load()
    hs = (C.c_void_p * len(des))(*[None if d is None else d._h for d in des])
    return lib.psm_gray_compute_batch(hs, len(des) if n is None else n, ls, rs, stride, depth, lmaps, rmaps, map_stride)


# --------------------------------------------------------------------------------------------------------------- the pair axis

@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_pair_axis(psm, n):
    """n = 1 is the table form of one pair.  Then the same contexts in reverse order with other pairs: ctxs[0], the table's owner,
    changes between calls on the same contexts."""
    W, H, D = 67, 45, 16
    with Members(psm, n, W, H, D) as des:
        check_batch(psm, des, ["noise"] * n, W, H, D, name="in order")
        check_batch(psm, des[::-1], ["noise"] * n, W, H, D, seeds=range(10, 10 + n), name="reversed")
        check_batch(psm, des, ["noise"] * n, W, H, D, name="in order again")


@pytest.mark.parametrize("W,H,D", [(8, 8, 2), (57, 17, 3), (113, 33, 34), (70, 9, 66)])
def test_kernel_seams(psm, W, H, D):
    """one live slot of four | second strip of one column, second segment of one row | three strips, a second chunk of one slice |
    three chunks"""
    with Members(psm, 3, W, H, D) as des:
        check_batch(psm, des, ["noise"] * 3, W, H, D)


# -------------------------------------------------------------------------------------------------------------------- content

def test_u8_contents(psm):
    W, H, D = 67, 21, 16
    with Members(psm, 3, W, H, D) as des:
        check_batch(psm, des, ["noise", "shifted", "constant"], W, H, D)
        assert np.all(des[2].lDisMap == 1) and np.all(des[2].rDisMap == 1)      # exact ties go to the lowest candidate


def test_f32_contents(psm, oracle):
    """+-1024 floats, exact ties everywhere, and a float copy of a u8 pair in one batch"""
    W, H, D = 67, 21, 16
    u = pair("noise", W, H, 2)
    ps = [pair("float", W, H, 0), pair("binary", W, H, 1), (oracle.u8_to_f32(u[0]), oracle.u8_to_f32(u[1]))]
    wants = [want_maps("float", W, H, D, 0), want_maps("binary", W, H, D, 1), want_maps("noise", W, H, D, 2)]
    with Members(psm, 3, W, H, D) as des:
        got = psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps])
        for i, (g, w) in enumerate(zip(got, wants)):
            check_maps(f"f32 member {i}", g, w)
        for i in (0, 2):
            assert same_bits(des[i].gray_guidance(1), M.Side(ps[i][0], ps[i][1], 1).planes())


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_padded_strides_and_null_maps(psm, oracle, dtype):
    W, H, D, n = 65, 21, 9, 3
    src = [pair("noise", W, H, i) for i in range(n)]
    if dtype == np.float32:
        src = [(oracle.u8_to_f32(l), oracle.u8_to_f32(r)) for l, r in src]
    pads = [[np.full((H, W + 7), 200, dtype) for _ in range(2)] for _ in range(n)]      # junk behind every row
    for pd, s in zip(pads, src):
        pd[0][:, :W], pd[1][:, :W] = s
    stride = (W + 7) * np.dtype(dtype).itemsize
    depth = int(dtype == np.float32)
    wants = [want_maps("noise", W, H, D, i) for i in range(n)]
    with Members(psm, n, W, H, D) as des:
        lms = [np.full((H, W + 5), 255, np.uint8) for _ in range(n)]
        rms = [np.full((H, W + 5), 255, np.uint8) for _ in range(n)]
        ls, rs = arr([p[0] for p in pads]), arr([p[1] for p in pads])
        assert raw_batch(psm, des, ls, rs, stride, depth, arr(lms), arr(rms), W + 5) == 0, psm.capi.last_error(des[0]._h)
        for i in range(n):
            check_maps(f"padded rows, member {i}", (lms[i][:, :W], rms[i][:, :W]), wants[i])
            assert np.all(lms[i][:, W:] == 255) and np.all(rms[i][:, W:] == 255)
        # lmaps NULL: the right maps alone; then some entries NULL on both sides
        rms2 = [np.full((H, W), 255, np.uint8) for _ in range(n)]
        assert raw_batch(psm, des[::-1], arr([p[0] for p in pads[::-1]]), arr([p[1] for p in pads[::-1]]), stride, depth, None, arr(rms2[::-1]), 0) == 0
        for i in range(n):
            assert np.array_equal(rms2[i], wants[i][1]), i
        lms3 = [np.full((H, W), 255, np.uint8) for _ in range(n)]
        rms3 = [np.full((H, W), 255, np.uint8) for _ in range(n)]
        assert raw_batch(psm, des, ls, rs, stride, depth, arr([lms3[0], None, lms3[2]]), arr([None, rms3[1], None]), W) == 0
        assert np.array_equal(lms3[0], wants[0][0]) and np.array_equal(lms3[2], wants[2][0]) and np.array_equal(rms3[1], wants[1][1])
        assert np.all(lms3[1] == 255) and np.all(rms3[0] == 255) and np.all(rms3[2] == 255)
        for i, de in enumerate(des):
            check_maps(f"the device maps of member {i}", de.download_maps(), wants[i])


# ---------------------------------------------------------------------------------------------------------------------- hooks

def test_hooks_behind_a_batch(psm):
    """the planes and the chunk scratch the hooks read are the member's own; (1, 34) and (30, 36) straddle a chunk edge"""
    W, H, D, n = 70, 19, 70, 3
    ps = [pair("noise", W, H, i) for i in range(n)]
    with Members(psm, n, W, H, D) as des:
        before = [[m.copy() for m in got] for got in psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps])]
        for i in (0, 1, 2):                                                   # first, middle, last
            l, r = ps[i]
            for side in (0, 1):
                got, want = des[i].gray_guidance(side), M.Side(l, r, side).planes()
                for k, nm in enumerate(("I", "G", "mI", "inv")):
                    assert same_bits(got[k], want[k]), (i, side, nm)
                wq, wab = M.volume(l, r, side, 0, D, want_ab=True)
                for d0, d1 in ((1, 34), (30, 36)):
                    q, ab = des[i].gray_volume(side, d0, d1, want_ab=True)
                    assert same_bits(q, wq[d0:d1]), ("q", i, side, d0, d1, int(np.count_nonzero(q != wq[d0:d1])))
                    assert same_bits(ab, wab[d0:d1]), ("ab", i, side, d0, d1)
        for i, de in enumerate(des):
            check_maps(f"member {i}: maps untouched by the hooks", de.download_maps(), before[i])
            check_maps(f"member {i}", before[i], want_maps("noise", W, H, D, i))


# ------------------------------------------------------------------------------------------------------------------- the plan

def test_the_plans_seam(psm):
    """672 x 400 x 17, n = 2: a single call runs 24-row segments there (1 632 waves: one round of the 2 048 a 256-CU device holds).
    The built planner counts both pairs' waves: 16 rows 3 rounds x 23 steps = 69, 24 rows 2 x 31 = 62, 32 rows 2 x 39 = 78, 48 rows
    1 x 55 = 55, 64 rows 71 - it picks 48 (8 full segments and one of 16 rows; by the arithmetic of gray_plan, which has no
    reader on the host).  The maps equal the model either way."""
    W, H, D = 672, 400, 17
    with Members(psm, 2, W, H, D) as des:
        check_batch(psm, des, ["shifted"] * 2, W, H, D)


# ---------------------------------------------------------------------------------------------------------- the committed pairs

@pytest.fixture(scope="module")
def green(golden):
    out = []
    for name in ("cones", "teddy"):
        p = golden(f"{name}_pair.npz")
        out.append((np.ascontiguousarray(p["l_bgr"][:, :, 1]), np.ascontiguousarray(p["r_bgr"][:, :, 1]), p))
    return out


def test_committed_pairs_equal_two_single_calls(psm, green):
    """(test_gpu_gray.py holds the single calls to the model)"""
    H, W = green[0][0].shape
    singles = []
    for gl, gr, _ in green:
        with psm.DispEst.blank(H, W, 64) as de:
            singles.append([m.copy() for m in de.Gray_GPU(gl, gr)])
    with Members(psm, 2, W, H, 64) as des:
        got = psm.gray_batch(des, [g[0] for g in green], [g[1] for g in green])
        for name, g, s in zip(("cones", "teddy"), got, singles):
            check_maps(name, g, s)
    assert not np.array_equal(singles[0][0], singles[1][0])


def test_harness_batch_gives_the_single_records(psm, green):
    from primestereomatch_amd import harness
    pairs = [(g[0], g[1]) for g in green]
    gts, masks = [g[2]["gt_l"] for g in green], [g[2]["occl"] for g in green]
    for tail in (False, True):
        outs = harness.compute_gray_batch(pairs, 64, gts, masks, lr_check=True, fill=True, device_tail=tail)
        for i, out in enumerate(outs):
            one = harness.compute_gray(pairs[i][0], pairs[i][1], 64, gts[i], masks[i], lr_check=True, fill=True, device_tail=tail)
            for k in ("lDisMap_raw", "rDisMap_raw", "lValid", "rValid", "lDisMap", "rDisMap"):
                assert np.array_equal(out[k], one[k]), (tail, i, k)
            assert out["bad_pixels"] == one["bad_pixels"] and out["bp_percent"] == one["bp_percent"] and out["gray_ms"] > 0.0


# ---------------------------------------------------------------------------------------------------------------------- state

Q = np.array([[1.0, 0, 0, -30.0], [0, 1.0, 0, -20.0], [0, 0, 0, 700.0], [0, 0, 1.0 / 120.0, 0]])


def tail_of(de, gt):
    """the stages that run behind the call, and everything they leave"""
    out = {}
    de.set_score_params(4, 1, 0)
    de.set_truth(gt)
    rec = de.Score_GPU(SC.GIF)
    out.update({f"score.{k}": np.asarray(rec[k]) for k in SC.RECORD_KEYS})
    de.setReprojection(Q)
    out["kept"] = np.asarray(de.Reproject_GPU(0, 3))                          # PSM_DEPTH_GIF; PSM_DEPTH_XYZ | PSM_DEPTH_Z
    xyz, z = de.reprojected()
    out["xyz"], out["z"] = xyz.view(np.uint32).copy(), z.view(np.uint32).copy()
    de.LRCheck_GPU()
    out["lValid"], out["rValid"] = de.lValid.copy(), de.rValid.copy()
    de.FillInv_GPU()
    out["lFill"], out["rFill"] = de.lDisMap.copy(), de.rDisMap.copy()
    return out


def test_the_tail_behind_a_member(psm):
    W, H, D, n = 131, 40, 16, 3
    ps = [pair("shifted", W, H, i) for i in range(n)]
    gts = [np.random.default_rng(40 + i).integers(0, 4 * D, (H, W), dtype=np.uint8) for i in range(n)]
    singles = []
    for (l, r), gt in zip(ps, gts):
        with psm.DispEst.blank(H, W, D) as de:
            de.Gray_GPU(l, r)
            singles.append(tail_of(de, gt))
    with Members(psm, n, W, H, D) as des:
        psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps], download=False)
        with pytest.raises(psm.capi.PsmError, match="psm_fill_invalid"):      # no mask of these maps yet, as behind a single call
            des[1].FillInv_GPU()
        for i in (2, 0, 1):
            got = tail_of(des[i], gts[i])
            assert got.keys() == singles[i].keys()
            for k in got:
                assert np.array_equal(got[k], singles[i][k]), (i, k)
        assert int(np.count_nonzero(singles[0]["lValid"])) not in (0, W * H)      # (the L-R check had something to decide)
    # ... and the L-R check and the fill of all members in shared launches
    with Members(psm, n, W, H, D) as des:
        psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps], download=False)
        psm.post_process_batch(des, lr_check=True, fill=True)
        for i, de in enumerate(des):
            for k, v in (("lValid", de.lValid), ("rValid", de.rValid), ("lFill", de.lDisMap), ("rFill", de.rDisMap)):
                assert np.array_equal(v, singles[i][k]), (i, k)


def test_a_member_with_a_colour_result(psm):
    """member 1 holds an uploaded colour pair and a finished, still pending colour result: behind the batch it downloads the same
    volume, selects the same maps, and its next colour sequence is what it was."""
    from primestereomatch_amd import synth
    W, H, D = 128, 48, 40
    l, r, _ = synth.make_pair(W, H, D, seed=1)
    gs = [(np.ascontiguousarray(synth.make_pair(W, H, D, seed=s)[0][:, :, 1]), np.ascontiguousarray(synth.make_pair(W, H, D, seed=s)[1][:, :, 1]))
          for s in (1, 2, 3)]
    wants = [M.maps(gl, gr, D) for gl, gr in gs]
    with psm.DispEst(l, r, D) as ref:                                         # the same steps without any gray call
        ref.CostConst_GPU(); ref.CostFilter_GPU(); ref.DispSelect_GPU()
        ref_maps = [ref.lDisMap.copy(), ref.rDisMap.copy()]
        ref_vol = ref.download_volume(0)
    des = [psm.DispEst.blank(H, W, D), psm.DispEst(l, r, D), psm.DispEst.blank(H, W, D)]
    try:
        des[1].CostConst_GPU(); des[1].CostFilter_GPU()                       # the filtered result is pending as packed minima
        got = psm.gray_batch(des, [g[0] for g in gs], [g[1] for g in gs])
        for i in range(3):
            check_maps(f"member {i}", got[i], wants[i])
        des[1].DispSelect_GPU()
        check_maps("the pending colour result behind the batch", (des[1].lDisMap, des[1].rDisMap), ref_maps)
        assert same_bits(des[1].download_volume(0), ref_vol)
        got = psm.gray_batch(des[::-1], [g[0] for g in gs[::-1]], [g[1] for g in gs[::-1]])
        check_maps("gray behind a colour select", got[1], wants[1])
        des[1].CostConst_GPU(); des[1].CostFilter_GPU(); des[1].DispSelect_GPU()
        check_maps("the next colour sequence", (des[1].lDisMap, des[1].rDisMap), ref_maps)
    finally:
        for d in des:
            d.close()


def test_alone_between_two_batches_and_release(psm):
    W, H, D, n = 67, 45, 16, 3
    with Members(psm, n, W, H, D) as des:
        check_batch(psm, des, ["noise"] * n, W, H, D)
        l, r = pair("shifted", W, H, 7)
        check_maps("member 1 alone", des[1].Gray_GPU(l, r), want_maps("shifted", W, H, D, 7))
        assert same_bits(des[1].gray_guidance(0), M.Side(l, r, 0).planes())
        for i in (0, 2):                                                      # nothing of the others changed
            check_maps(f"member {i} meanwhile", des[i].download_maps(), want_maps("noise", W, H, D, i))
        check_batch(psm, des, ["noise"] * n, W, H, D, seeds=(3, 4, 5), name="batched again")
        des[1].release_scratch()                                              # its buffers go, and come back at other addresses
        with pytest.raises(psm.capi.PsmError, match="psm_gray_guidance: no pair"):
            des[1].gray_guidance(0)
        check_batch(psm, des, ["noise"] * n, W, H, D, seeds=(6, 7, 8), name="after member 1's release")
        des[0].release_scratch()                                              # the table's owner: the table goes too
        check_batch(psm, des, ["noise"] * n, W, H, D, name="after member 0's release")
        assert same_bits(des[1].gray_guidance(1), M.Side(*pair("noise", W, H, 1), 1).planes())


def test_async_on_every_member(psm):
    W, H, D, n = 131, 70, 33, 3
    ps = [pair("noise", W, H, i) for i in range(n)]
    with Members(psm, n, W, H, D) as des:
        for de in des:
            de.set_option(psm.capi.PSM_OPT_ASYNC, 1)
        assert psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps], download=False) == [None] * n
        for i in (1, 2, 0):
            check_maps(f"async member {i}", des[i].download_maps(), want_maps("noise", W, H, D, i))
        for de in des:
            de.synchronize()


def test_members_on_streams_of_their_own(psm):
    W, H, D, n = 67, 45, 16, 3
    hip = hip_runtime()
    streams = [C.c_void_p() for _ in range(n)]
    with Members(psm, n, W, H, D) as des:
        for de, s in zip(des, streams):
            assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0            # hipStreamNonBlocking
            de.set_stream(s.value)
        check_batch(psm, des, ["noise"] * n, W, H, D)
        check_batch(psm, des[::-1], ["shifted"] * n, W, H, D)
        for i, de in enumerate(des):                                          # later work on a member's stream comes behind the batch
            de.LRCheck_GPU()
        for de in des:
            de.set_stream(None)
            de.synchronize()
        for s in streams:
            assert hip.hipStreamDestroy(s) == 0


def test_profile_time_is_context_0s(psm):
    W, H, D = 67, 45, 16
    with Members(psm, 2, W, H, D) as des:
        check_batch(psm, des, ["noise"] * 2, W, H, D)
        with pytest.raises(psm.capi.PsmError, match="psm_gray_time"):
            des[0].gray_time()
        des[0].set_option(psm.capi.PSM_OPT_PROFILE, 1)
        des[1].set_option(psm.capi.PSM_OPT_PROFILE, 1)
        check_batch(psm, des, ["noise"] * 2, W, H, D)
        assert 0.0 < des[0].gray_time() < 1000.0
        with pytest.raises(psm.capi.PsmError, match="psm_gray_time: .*not timed"):
            des[1].gray_time()


# ------------------------------------------------------------------------------------------------------------------- refusals

def test_refusals(psm):
    W, H, D, n = 40, 12, 16, 3
    capi = psm.capi
    lib = capi.load()
    ps = [pair("noise", W, H, i) for i in range(n)]
    ls, rs = arr([p[0] for p in ps]), arr([p[1] for p in ps])
    ls4, rs4 = arr([p[0] for p in ps] + [ps[0][0]]), arr([p[1] for p in ps] + [ps[0][1]])
    lms = [np.zeros((H, W), np.uint8) for _ in range(n + 1)]
    rms = [np.zeros((H, W), np.uint8) for _ in range(n + 1)]
    with Members(psm, n, W, H, D) as des:
        before = [[m.copy() for m in got]
                  for got in psm.gray_batch(des, [pair("shifted", W, H, i)[0] for i in range(n)], [pair("shifted", W, H, i)[1] for i in range(n)])]

        def refused(words, members, l=ls, r=rs, stride=0, depth=0, map_stride=0, count=None, null=False):
            k = len(members)
            assert raw_batch(psm, members, l, r, stride, depth, arr(lms[:k]), arr(rms[:k]), map_stride, n=count) != 0
            msg = capi.last_error(None if null else members[0]._h)
            assert "psm_gray_compute_batch" in msg and all(w in msg for w in words), msg
            for i, de in enumerate(des):
                check_maps(f"{words}: the previous maps of member {i} stay current", de.download_maps(), before[i])

        assert lib.psm_gray_compute_batch(None, n, ls, rs, 0, 0, None, None, 0) != 0 and "psm_gray_compute_batch" in capi.last_error(None)
        refused(["n 0"], des, count=0, null=True)
        refused(["4097"], des, count=4097)
        refused(["context 1", "NULL"], [des[0], None, des[2]])
        refused(["context 2", "twice"], [des[0], des[1], des[0]])
        refused(["NULL"], des, l=None)
        refused(["NULL"], des, r=None)
        refused(["context 1", "NULL"], des, l=arr([ps[0][0], None, ps[2][0]]))
        refused(["context 2", "NULL"], des, r=arr([ps[0][1], ps[1][1], None]))
        refused(["depth", "7"], des, depth=7)
        refused(["stride", str(W - 1)], des, stride=W - 1)
        refused(["stride", str(4 * W - 4)], des, stride=4 * W - 4, depth=1)
        refused(["map stride", str(W - 1)], des, map_stride=W - 1)
        for kw, words in (({"dtype": "u8"}, ["context 3", "8-bit"]), ({"d_range": (0, 8)}, ["context 3", "disparity shard"]),
                          ({"d_stride": (1, 2)}, ["context 3", "disparity shard"])):
            with psm.DispEst.blank(H, W, D, **kw) as odd:
                refused(words, des + [odd], l=ls4, r=rs4)
        for shape, words in (((H, W + 1, D), ["context 3", "geometry"]), ((H + 1, W, D), ["context 3", "geometry"]),
                             ((H, W, D + 1), ["context 3", "geometry"])):
            with psm.DispEst.blank(*shape) as odd:
                refused(words, des + [odd], l=ls4, r=rs4)
        des[1].set_option(capi.PSM_OPT_FLAGS, capi.PSM_FLAG_TWO_PHASE_OFF)
        refused(["context 1", "options"], des)
        des[1].set_option(capi.PSM_OPT_FLAGS, 0)
        des[2].set_rows(4, 8)
        refused(["context 2", "row stripe"], des)
        des[2].set_rows(0, 0)
        assert not any(m.any() for m in lms + rms)                            # nothing was written to the caller's maps either
        check_batch(psm, des, ["noise"] * n, W, H, D, name="and the call works again")
