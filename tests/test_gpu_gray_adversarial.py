"""-m gpu: the one-channel guided-filter path - psm_gray_compute, psm_gray_compute_fgf and their batch entries - on the pairs of
tests/gray_inputs.py: NaN of either sign, +-inf and overflowing values planted in both planes, planes that are wholly NaN, exact
ties across the 32-slice chunk seams, and minima below zero.  Every input is a call the API accepts: psm_api_gray.cpp looks at no
value.  tests/test_gray_inputs.py holds the inputs to the conditions that keep these tests from passing vacuously.

The contract: a NaN q is never a candidate, a pixel with no candidate is 0 - oracle.wta's strict <, which
tests/gray_model.py::wta_running restates.  There is no tolerance: np.array_equal on maps; planes and volumes are the model's bits
wherever the model's value is not a NaN (+-inf and the sign of a zero count) and NaN exactly where the model's is.  The sign and
payload of a NaN are free - x86 forms 0xFFC00000 for inf - inf where gfx950 forms 0x7FC00000, and neither is this project's
contract - but they are counted and printed: a NaN with the sign bit set is the one whose WTA key sorts below every finite cost.
"""
import numpy as np
import pytest

import gray_inputs as GI
from test_gpu_gray import check_maps
from test_gpu_gray_batch import Members

pytestmark = pytest.mark.gpu

FORMS = GI.FORMS


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def blank(psm, kind, s):
    W, H, D = GI.size(kind, s)
    return psm.DispEst.blank(H, W, D)


def run(de, l, r, s, **kw):
    return de.Gray_GPU(l, r, subsample_rate=s, **kw)


def check_planes(name, got, want):
    """the model's bits where the model is not NaN, NaN exactly where it is -> (device NaNs, of them with the sign bit set)"""
    assert got.shape == want.shape and got.dtype == np.float32, name
    g, w, gn, wn = bits(got), bits(want), np.isnan(got), np.isnan(want)
    n, neg, wneg = int(np.count_nonzero(gn)), int(np.count_nonzero(gn & (g >> 31 == 1))), int(np.count_nonzero(wn & (w >> 31 == 1)))
    print(f"[gray-adv] {name}: device NaNs {n}, with the sign bit set {neg}  (model: {int(np.count_nonzero(wn))}, {wneg})")
    assert np.array_equal(gn, wn), (name, "NaN in other places than the model's", int(np.count_nonzero(gn != wn)), np.argwhere(gn != wn)[:8].tolist())
    assert np.array_equal(g[~wn], w[~wn]), (name, int(np.count_nonzero(g[~wn] != w[~wn])))
    return n, neg


# -------------------------------------------------------------------------------------------------------------------------- maps

@pytest.mark.parametrize("s", FORMS)
@pytest.mark.parametrize("kind", GI.KINDS)
def test_maps(psm, kind, s):
    l, r = GI.pair(kind, s)
    want = GI.maps(kind, s)
    with blank(psm, kind, s) as de:
        got = [m.copy() for m in run(de, l, r, s)]
        check_maps(f"{kind} s={s}", got, want)
        check_maps(f"{kind} s={s} download_maps", de.download_maps(), want)
    if kind == "all_slices":
        assert not got[0].any() and not got[1].any()                  # no candidate anywhere: 0


# ----------------------------------------------------------------------------------------------------------------- storing hooks

def hook_ranges(D):
    return [(30, 36), (1, D)]                                         # across the chunk edge 32 | 33; every candidate


@pytest.mark.parametrize("s", FORMS)
@pytest.mark.parametrize("kind", ["all", "periodic", "nan_neg", "overflow"])
def test_storing_hooks(psm, kind, s):
    """q, a, b (the Fast Guided Filter: q, a, b, blur(a), blur(b)) of both sides.  nan_neg answers whether the sign of an input NaN
    reaches q on the device, overflow what sign the device's own inf - inf has; `all` has both."""
    l, r = GI.pair(kind, s)
    D = GI.size(kind, s)[2]
    names = ("a", "b") if s == 0 else ("a", "b", "blur(a)", "blur(b)")
    with blank(psm, kind, s) as de:
        before = [m.copy() for m in run(de, l, r, s)]
        for side in (0, 1):
            wq, wm = GI.volume(kind, s, side)
            for d0, d1 in hook_ranges(D):
                q, m = de.gray_volume(side, d0, d1, want_ab=True) if s == 0 else de.gray_fgf_volume(side, d0, d1, want_model=True)
                tag = f"{kind} s={s} side {side} [{d0},{d1})"
                check_planes(f"{tag} q", q, wq[d0:d1])
                for k, nm in enumerate(names):
                    check_planes(f"{tag} {nm}", m[:, k], wm[d0:d1, k])
        check_maps("maps untouched by the hooks", de.download_maps(), before)
        check_maps(f"{kind} s={s}", before, GI.maps(kind, s))


# --------------------------------------------------------------------------------------------------------------------- seam ties

@pytest.mark.parametrize("s", FORMS)
@pytest.mark.parametrize("kind", list(GI.TIE))
def test_exact_ties_across_chunk_seams_go_to_the_lowest_d(psm, kind, s):
    """The slices 3 and 35 (and 67) are the same bits in at least a quarter of the pixels and arrive in different launches: their
    keys differ in the low word alone.  The same pair as bytes 0 / 255 converts to the same float planes."""
    l, r = GI.pair(kind, s)
    want = GI.maps(kind, s)
    with blank(psm, kind, s) as de:
        got = [m.copy() for m in run(de, l, r, s)]
        check_maps(f"{kind} s={s}", got, want)
        for side in (0, 1):
            tie = GI.ties(kind, s, side)
            assert 4 * int(np.count_nonzero(tie)) >= tie.size
            assert np.all(got[side][tie] <= 3), (kind, s, side, np.unique(got[side][tie]).tolist())
        check_maps(f"{kind} s={s} as bytes", run(de, *GI.as_bytes(kind, s), s), want)


# ----------------------------------------------------------------------------------------------------------------------- batches

@pytest.fixture(scope="module")
def single(psm):
    """(kind, s, seed, like) -> the maps of its own single call on a fresh context: computed once, shared"""
    cache = {}

    def get(kind, s, seed=0, like=None):
        key = (kind, s, seed, like)
        if key not in cache:
            with blank(psm, like or kind, s) as de:
                cache[key] = tuple(m.copy() for m in run(de, *GI.pair(kind, s, seed, like), s))
                for m in cache[key]:
                    m.setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("s", [0, 4])
@pytest.mark.parametrize("kind", ["all", "periodic"])
def test_batch_members_keep_to_themselves(psm, single, kind, s):
    """n = 3: the adversarial pair between two clean pairs of other seeds.  Every member against its own model and its own single
    call: a NaN in one member's scratch or key plane reaches no neighbour."""
    W, H, D = GI.size(kind, s)
    members = [("clean", s, 1, kind), (kind, s, 0, None), ("clean", s, 2, kind)]
    ps = [GI.pair(*m) for m in members]
    with Members(psm, 3, W, H, D) as des:
        for rnd in (0, 1):                                            # twice: the second batch finds the first one's keys and scratch
            got = psm.gray_batch(des, [p[0] for p in ps], [p[1] for p in ps], subsample_rate=s)
            for i, (m, de) in enumerate(zip(members, des)):
                name = f"{kind} s={s} round {rnd} member {i} ({m[0]})"
                check_maps(name, [g.copy() for g in got[i]], GI.maps(*m))
                check_maps(name + " download_maps", de.download_maps(), GI.maps(*m))
                check_maps(name + " against its single call", got[i], single(*m))
        # the hooks of a clean neighbour, whose slots sit beside the adversarial member's
        wq, wm = GI.volume(*members[2][:2], 1, members[2][2], members[2][3])
        q, m = des[2].gray_volume(1, 30, 36, want_ab=True) if s == 0 else des[2].gray_fgf_volume(1, 30, 36, want_model=True)
        assert check_planes("a clean neighbour's q", q, wq[30:36])[0] == 0
        assert check_planes("a clean neighbour's model planes", m, wm[30:36])[0] == 0


# ---------------------------------------------------------------------------------------------------------------------- the tail

@pytest.mark.parametrize("s", FORMS)
def test_lr_check_and_fill_behind_the_all_pair(psm, oracle, s):
    """all-zero regions are what a NaN plane leaves behind"""
    lm, rm = GI.maps("all", s)
    assert (lm == 0).any() and (rm == 0).any()
    lv, rv = oracle.lr_check(lm, rm)
    with blank(psm, "all", s) as de:
        run(de, *GI.pair("all", s), s, download=False)
        de.LRCheck_GPU()
        assert np.array_equal(de.lValid, lv) and np.array_equal(de.rValid, rv)
        de.FillInv_GPU()
        assert np.array_equal(de.lDisMap, oracle.fill_inv(lm, lv)) and np.array_equal(de.rDisMap, oracle.fill_inv(rm, rv))


# ------------------------------------------------------------------------------------------------------------------------- reuse

@pytest.mark.parametrize("s", FORMS)
def test_a_clean_pair_after_nan_planes_on_one_context(psm, s):
    """stale keys or scratch of the NaN planes would show in the clean pair's maps"""
    clean = ("clean", s, 3, "all_slices")
    with blank(psm, "all_slices", s) as de:
        for kind in ("all_slices", "left_nan"):
            check_maps(f"{kind} s={s}", run(de, *GI.pair(kind, s), s), GI.maps(kind, s))
            check_maps(f"clean behind {kind} s={s}", run(de, *GI.pair(*clean), s), GI.maps(*clean))
            q = de.gray_volume(0, 30, 36) if s == 0 else de.gray_fgf_volume(0, 30, 36)
            assert check_planes(f"clean behind {kind} s={s} q", q, GI.volume(clean[0], s, 0, clean[2], clean[3])[0][30:36])[0] == 0
