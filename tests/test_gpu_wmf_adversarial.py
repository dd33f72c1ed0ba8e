"""-m gpu: psm_wgt_median on the adversarial inputs of tests/wmf_inputs.py, every map np.array_equal to oracle.wgt_median - 0
differing pixels, no tolerance.  Three properties the device forms rest on and smooth random maps never exercise:

* the ORDER of the fp32 additions into the histogram and the total (knife_edge: windows whose two bins have equal real sums);
* DENORMAL weights and sums (denormal_windows: windows whose every voting weight is one);
* leaving the sweeps WITHOUT a fixed point (domino: chains that need hundreds of synchronous sweeps against a cap of 96);

and the seams: D around the 64-bin words (129: three words), counts of invalid pixels around WM_LANE_MIN = 8192 and around a
multiple of 64, windows without a vote, images the window wraps onto itself, several calls on one context.
tests/test_wmf_inputs.py holds the inputs to what they claim (on the CPU)."""
import numpy as np
import pytest

import wmf_inputs as G

pytestmark = pytest.mark.gpu

FLAGS = G.FORMS                        # sweeps (0) | no_cache | dataflow | fallback (two sweeps, then the dataflow form)
SEED_KNIFE, SEED_DENORMAL = 5, 6       # (tests/test_wmf_inputs.py checks these very inputs)
CAP = 96


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@pytest.fixture(scope="module")
def expected(oracle):
    """oracle.wgt_median of both maps of an input, computed once per input (the forms share it); never written to."""
    cache = {}

    def get(key, inp, D):
        if key not in cache:
            cache[key] = tuple(oracle.wgt_median(oracle.u8_to_f32(inp.img[s]), inp[1 + s], inp[3 + s], D, right=bool(s)) for s in (0, 1))
            for m in cache[key]:
                m.setflags(write=False)
        return cache[key]
    return get


def _filter(psm, inp, D, flags):
    """-> (left map, right map, sweeps, evaluations) of one psm_wgt_median on a fresh context"""
    from primestereomatch_amd import capi
    with psm.DispEst(inp.img[0], inp.img[1], D) as de:
        de.set_option(capi.PSM_OPT_FLAGS, flags)
        de.upload_maps(inp.lmap, inp.rmap, inp.lvalid, inp.rvalid)
        de.WgtMedian_GPU()
        sweeps, evals = de.wgt_median_stats()
        return de.lDisMap.copy(), de.rDisMap.copy(), sweeps, evals


def _check_stats(form, sweeps):
    if form == "dataflow":
        assert sweeps == [-1, -1]
    else:
        assert all(s == -1 or 1 <= s <= CAP for s in sweeps), sweeps


def _at(m, pix):
    return m[pix[:, 0], pix[:, 1]]


# ------------------------------------------------------------------------------------------ 1. order and denormals

PROPERTY_CASES = [("wave", 0)] + [(form, G.BULK_ROWS) for form in sorted(FLAGS)]      # short lists: wave form | long: the four forms


@pytest.mark.parametrize("form,bulk", PROPERTY_CASES, ids=[f"{f}-bulk{b}" for f, b in PROPERTY_CASES])
@pytest.mark.parametrize("H,W,D", G.KNIFE_CASES)
@pytest.mark.parametrize("kind", ["knife_edge", "denormal_windows"])
def test_order_and_denormal_sensitive_windows(psm, expected, kind, H, W, D, form, bulk):
    """knife_edge: every listed pixel's result changes under another order of the 361 additions (reversed rows, reversed columns
    or a balanced tree - the model says which, tests/test_wmf_inputs.py prints the counts).  denormal_windows: every listed
    pixel's result becomes 0 if a denormal weight or sum is flushed.  Without the bulk rows the lists are short (40 pixels per
    side: k_wm_eval_w); with them the first sweep evaluates the listed pixels one per lane (k_wm_eval), with the weight
    cache and without it; then the dataflow form and the two-sweep fall-back.  D = 64, 129, 256: one, three and four words of
    bins (256 on a wider image: a context takes no D above its width)."""
    gen, seed = (G.knife_edge, SEED_KNIFE) if kind == "knife_edge" else (G.denormal_windows, SEED_DENORMAL)
    inp = gen(H, W, D, seed, bulk)
    el, er = expected((kind, D, bulk), inp, D)
    gl, gr, sweeps, evals = _filter(psm, inp, D, FLAGS.get(form, 0))
    ninv = int((inp.lvalid == 0).sum()), int((inp.rvalid == 0).sum())
    bad = [int((_at(g, p) != _at(e, p)).sum()) for g, e, p in ((gl, el, inp.pixels[0]), (gr, er, inp.pixels[1]))]
    print(f"[wmf-adv] {kind} D={D} {form} bulk={bulk}: {len(inp.pixels[0])} + {len(inp.pixels[1])} sensitive pixels checked, {bad[0]} + {bad[1]} "
          f"of them wrong; whole maps: {int((gl != el).sum())} + {int((gr != er).sum())} wrong of {ninv[0]} + {ninv[1]} filtered; "
          f"sweeps {sweeps}, evaluations {evals}")
    assert min(len(p) for p in inp.pixels) >= 8
    assert (ninv[0] >= 8192 and ninv[1] >= 8192) == (bulk > 0)
    prop = "the order of the additions" if kind == "knife_edge" else "denormal weights / sums"
    assert bad == [0, 0], f"{prop}: {bad} of the sensitive pixels differ from the oracle"
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    _check_stats(form, sweeps)
    if kind == "denormal_windows":
        assert _at(gl, inp.pixels[0]).all() and _at(gr, inp.pixels[1]).all()          # (0 is what flushing gives)


# ------------------------------------------------------------------------------------------ 2. chains

@pytest.mark.parametrize("form", ["sweeps", "no_cache"])
@pytest.mark.parametrize("name", sorted(G.DOMINO_CASES))
def test_domino_chains(psm, expected, name, form):
    """Maps whose synchronous iteration needs 196 .. 395 sweeps (tests/test_wmf_inputs.py) against the cap of 96: either the sweeps
    get to the fixed point in time - a device sweep sees changes of its own, so how far it gets depends on timing - or the input is
    restored and the dataflow form runs (-1).  Which of the two happened is printed, not asserted; the maps are the oracle's
    either way."""
    inp = G.domino(*G.DOMINO_CASES[name])
    el, er = expected(("domino", name), inp, 16)
    gl, gr, sweeps, evals = _filter(psm, inp, 16, FLAGS[form])
    what = ["fell back to the dataflow form" if s == -1 else f"fixed point after {s} sweeps" for s in sweeps]
    print(f"[wmf-adv] domino {name} {form}: left {what[0]}, right {what[1]}; evaluations {evals}; "
          f"wrong pixels {int((gl != el).sum())} + {int((gr != er).sum())} of {int((inp.lvalid == 0).sum())} per side")
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    _check_stats(form, sweeps)
    assert not np.array_equal(el, inp.lmap)


@pytest.mark.parametrize("form", ["sweeps", "no_cache"])
def test_domino_control_needs_few_sweeps(psm, expected, form):
    """Period 2: b holds the majority of every window from the start, every pixel flips in the first sweep."""
    inp = G.domino(*G.DOMINO_CONTROL)
    el, er = expected(("domino", "control"), inp, 16)
    gl, gr, sweeps, evals = _filter(psm, inp, 16, FLAGS[form])
    print(f"[wmf-adv] domino control {form}: sweeps {sweeps}, evaluations {evals}")
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    assert all(1 <= s <= 3 for s in sweeps), sweeps


# ------------------------------------------------------------------------------------------ 3. windows without a vote

@pytest.mark.parametrize("form,D", [(f, 64) for f in sorted(FLAGS)] + [("sweeps", 2), ("dataflow", 2)])
def test_windows_without_a_vote(psm, expected, form, D):
    inp = G.zero_windows(*G.ZERO_GEO, D, 3)
    el, er = expected(("zero", D), inp, D)
    gl, gr, sweeps, evals = _filter(psm, inp, D, FLAGS[form])
    print(f"[wmf-adv] zero_windows D={D} {form}: {len(inp.pixels[0])} + {len(inp.pixels[1])} pixels with an empty window; sweeps {sweeps}")
    assert min(len(p) for p in inp.pixels) >= 8
    assert not _at(gl, inp.pixels[0]).any() and not _at(gr, inp.pixels[1]).any(), "sumWgt = 0: the result is 0"
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    _check_stats(form, sweeps)


# ------------------------------------------------------------------------------------------ 4. counts at the seams

@pytest.mark.parametrize("form", ["sweeps", "no_cache"])
@pytest.mark.parametrize("nl,nr", G.COUNTS)
def test_counts_of_invalid_pixels_at_the_seams(psm, expected, nl, nr, form):
    """WM_LANE_MIN = 8192 decides lane or wave form (and, for the pair, cache or not); the cache is laid out in blocks of 64 pixels
    (8192 and 8256 fill their last block, 8193 and 8257 start a new one with one pixel); a side without an invalid pixel beside
    one exactly at the threshold."""
    H, W, D = G.COUNTED_GEO
    inp = G.counted_invalid(H, W, D, 11, nl, nr)
    el, er = expected(("counted", nl, nr), inp, D)
    gl, gr, sweeps, evals = _filter(psm, inp, D, FLAGS[form])
    print(f"[wmf-adv] invalid {nl} / {nr} {form}: sweeps {sweeps}, evaluations {evals}")
    assert int((inp.lvalid == 0).sum()) == nl and int((inp.rvalid == 0).sum()) == nr
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    assert all(1 <= s <= CAP for s in sweeps), sweeps
    for n, e in zip((nl, nr), evals):
        assert (e == 0) if n == 0 else (e >= n)


# ------------------------------------------------------------------------------------------ 5. geometries

@pytest.mark.parametrize("W,H,D,frac,form,seed", G.geometry_cases(), ids=lambda v: str(v))
def test_small_and_seam_geometries(psm, expected, W, H, D, frac, form, seed):
    inp = G.random_case(W, H, D, frac, seed)
    el, er = expected(("geo", W, H, D, frac, seed), inp, D)
    gl, gr, sweeps, evals = _filter(psm, inp, D, FLAGS[form])
    print(f"[wmf-adv] {W}x{H} D={D} invalid {frac} {form}: sweeps {sweeps}, evaluations {evals}, wrong {int((gl != el).sum())} + {int((gr != er).sum())}")
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    _check_stats(form, sweeps)


# ------------------------------------------------------------------------------------------ 6. one context, several calls

@pytest.mark.parametrize("form", ["sweeps", "no_cache"])
def test_one_context_several_calls(psm, oracle, form):
    """400 invalid pixels per side, then 12000 (the cache is allocated), then 400 (it is held but not used), then the first input
    again - every result the oracle's: nothing of a call (lists, stamps, slots, counters, the cache) reaches the next.  Then two
    filter calls without an upload between them: the second filters the first's output with the same mask."""
    from primestereomatch_amd import capi
    H, W, D = G.COUNTED_GEO
    seq = [G.counted_invalid(H, W, D, 21, 400, 400, 1), G.counted_invalid(H, W, D, 21, 12000, 12000, 2),
           G.counted_invalid(H, W, D, 21, 400, 400, 3), G.counted_invalid(H, W, D, 21, 400, 400, 1)]
    first = seq[0]
    f = [oracle.u8_to_f32(first.img[s]) for s in (0, 1)]
    with psm.DispEst(first.img[0], first.img[1], D) as de:
        de.set_option(capi.PSM_OPT_FLAGS, FLAGS[form])
        for i, inp in enumerate(seq):
            assert np.array_equal(inp.img, first.img)                       # (one image pair: drawn from the seed, the maps from the map seed)
            de.upload_maps(inp.lmap, inp.rmap, inp.lvalid, inp.rvalid)
            de.WgtMedian_GPU()
            sweeps, evals = de.wgt_median_stats()
            print(f"[wmf-adv] call {i} ({form}): sweeps {sweeps}, evaluations {evals}")
            assert np.array_equal(de.lDisMap, oracle.wgt_median(f[0], inp.lmap, inp.lvalid, D, right=False)), i
            assert np.array_equal(de.rDisMap, oracle.wgt_median(f[1], inp.rmap, inp.rvalid, D, right=True)), i
        once = de.lDisMap.copy(), de.rDisMap.copy()
        de.WgtMedian_GPU()
        assert np.array_equal(de.lDisMap, oracle.wgt_median(f[0], once[0], first.lvalid, D, right=False))
        assert np.array_equal(de.rDisMap, oracle.wgt_median(f[1], once[1], first.rvalid, D, right=True))
        twice = de.lDisMap.copy(), de.rDisMap.copy()
        de.WgtMedian_GPU()
        assert np.array_equal(de.lDisMap, oracle.wgt_median(f[0], twice[0], first.lvalid, D, right=False))
        assert np.array_equal(de.rDisMap, oracle.wgt_median(f[1], twice[1], first.rvalid, D, right=True))
