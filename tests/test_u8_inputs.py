"""CPU: the numpy statement of the 8-bit mode (tests/u8_model.py) equals the oracle on every case of tests/u8_inputs.py, every
generator reaches the edge it was written for, and each mutant of the model is seen by the cases meant for it - so a device
that equals the oracle on these cases (tests/test_gpu_u8_adversarial.py) cannot hold one of those readings."""
import ctypes as C

import numpy as np
import pytest

import u8_inputs as I
import u8_model as M

SIDES = (("ql", "lvol", "lkeys", "raw_l"), ("qr", "rvol", "rkeys", "raw_r"))


@pytest.fixture(scope="module")
def models(oracle):
    """The canonical model of every case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            c = I.BY_NAME[name]
            cache[name] = M.pipeline(oracle, c.l, c.r, c.D) if c.vols is None else M.from_raw(oracle, c.l, c.r, *c.vols)
        return cache[name]
    return get


def edge_counts(m):
    """Per side: the counts of u8_model.edges over the whole filtered volume."""
    return [{k: int(v.sum()) for k, v in M.edges(M.scaled(m[q])).items()} for q, _, _, _ in SIDES]


def tie_counts(m, S):
    tied = cross = 0
    for _, vol, _, _ in SIDES:
        t, c = M.tie_masks(m[vol], S)
        tied += int(t.sum())
        cross += int((t & c).sum())
    return tied, cross


def mutant_counts(oracle, c, m):
    """Elements of (raw volumes, filtered volumes, keys) that each mutant changes on case c."""
    out = {}
    for name in ("fma", "floor", "wrap"):
        if name == "fma":
            if c.vols is not None:
                out[name] = (0, 0, 0)
                continue
            raw = M.raw_volumes(c.l, c.r, c.D, "fma")
            if all(np.array_equal(a, m[k]) for a, k in zip(raw, ("raw_l", "raw_r"))):
                out[name] = (0, 0, 0)
                continue
            mm = M.from_raw(oracle, c.l, c.r, *raw)
        else:
            mm = {"raw_l": m["raw_l"], "raw_r": m["raw_r"], "lvol": M.quant(m["ql"], name), "rvol": M.quant(m["qr"], name)}
            mm["lkeys"], mm["rkeys"] = M.keys_of(mm["lvol"]), M.keys_of(mm["rvol"])
        out[name] = tuple(sum(int((mm[s[i]] != m[s[i]]).sum()) for s in SIDES) for i in (3, 1, 2))
    return out


def table_line(oracle, c, m):
    e = edge_counts(m)
    n = 2 * c.W * c.H
    t5, x5 = tie_counts(m, 5)
    _, x8 = tie_counts(m, 8)
    mu = mutant_counts(oracle, c, m)
    sat = 100.0 * sum(int((m[k] == 255).sum()) for k in ("raw_l", "raw_r")) / (n * c.D)
    return ("%-22s over %d/%d under %d/%d half_even %d/%d half_odd %d/%d ties %.0f%% cross5 %d cross8 %d fma %s floor %s wrap %s raw255 %.0f%%"
            % (c.name, e[0]["over"], e[1]["over"], e[0]["under"], e[1]["under"], e[0]["half_even"], e[1]["half_even"],
               e[0]["half_odd"], e[1]["half_odd"], 100.0 * t5 / n, x5, x8, *("/".join(map(str, mu[k])) for k in ("fma", "floor", "wrap")), sat))


def test_case_table(oracle, models, capsys):
    """Prints the table that u8_inputs.py records (pytest -s); asserts nothing but that every case can be measured."""
    lines = [table_line(oracle, c, models(c.name)) for c in I.CASES]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert len(lines) == len(I.CASES)


def test_shapes_take_both_seed_strides():
    rows, pixels, below, above = I.seed_stride_rule()
    assert (below, above) == (5, 8)
    assert I.SMALL[1] < rows <= I.TALL[1]
    assert all(c.W * c.H < pixels for c in I.CASES)
    assert {c.H >= rows for c in I.CASES if c.family == "tie"} == {False, True}
    assert {c.H >= rows for c in I.CASES if c.family == "half"} == {False, True}


@pytest.mark.parametrize("name", [c.name for c in I.IMAGE_CASES])
def test_model_equals_oracle(oracle, models, name):
    c, m = I.BY_NAME[name], models(name)
    ref = oracle.pipeline_u8(c.l, c.r, c.D, threads=8, want_volumes=True, want_raw=True)
    for k in ("raw_l", "raw_r", "lvol", "rvol", "ldisp", "rdisp"):
        assert np.array_equal(m[k], ref[k]), k
    assert np.array_equal(M.keys_of(ref["lvol"]), m["lkeys"]) and np.array_equal(M.keys_of(ref["rvol"]), m["rkeys"])


@pytest.mark.parametrize("name", [c.name for c in I.UPLOAD_CASES])
def test_uploaded_model_equals_the_oracles_pieces(oracle, models, name):
    """An uploaded volume has no oracle pipeline: the filter is the oracle's, the quantisation the model's (equal to the oracle's
    on every image case above), and the model's WTA equals psmo_wta_u8."""
    c, m = I.BY_NAME[name], models(name)
    for vol, disp in (("lvol", "ldisp"), ("rvol", "rdisp")):
        out = np.empty((c.H, c.W), np.uint8)
        v = np.ascontiguousarray(m[vol])
        oracle.lib().psmo_wta_u8(v.ctypes.data_as(C.c_void_p), c.D, c.H, c.W, out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(out, m[disp])
        assert np.array_equal(M.unpack(m[vol[0] + "keys"]), m[disp])


def test_all_255_is_exact_and_the_first_slice_wins(models):
    m = models("up_all255")
    for q, vol, _, _ in SIDES:
        assert (M.scaled(m[q]) == 255).all() and (m[vol] == 255).all()
    assert (m["ldisp"] == 1).all() and (m["rdisp"] == 1).all()


@pytest.mark.parametrize("name", ["table_black", "table_white"])
def test_table_holds_every_pair_on_each_side(name):
    """Slice 1 - a slice that the WTA reads - meets all 65 536 pairs (clr / 3, grd) in the left and in the right volume, and its
    raw costs are a plain statement of the cost line."""
    c = I.BY_NAME[name]
    pl, pr = M.planes(c.l), M.planes(c.r)
    for base, other, right in ((pl, pr, False), (pr, pl, True)):
        clr, grd = M.cost_terms(base, other, 1, right)
        assert len(set((clr * 256 + grd).ravel().tolist())) == 65536
        expect = np.trunc(np.float32(0.9) * clr.astype(np.float32) + (np.float32(1) - np.float32(0.9)) * grd.astype(np.float32))
        assert np.array_equal(M.cost(clr, grd), expect.astype(np.uint8))


def test_extrapolation_leaves_the_range_on_both_ends_of_each_side(models):
    tot = [{"over": 0, "under": 0}, {"over": 0, "under": 0}]
    for c in I.IMAGE_CASES:
        for s, e in enumerate(edge_counts(models(c.name))):
            tot[s]["over"] += e["over"]
            tot[s]["under"] += e["under"]
    for s in range(2):
        assert tot[s]["over"] >= 5 and tot[s]["under"] >= 5, tot
    # ... and the family written for it does so alone
    fam = [edge_counts(models(c.name)) for c in I.IMAGE_CASES if c.family == "extrap"]
    for s in range(2):
        assert sum(e[s]["over"] for e in fam) >= 5 and sum(e[s]["under"] for e in fam) >= 5


def test_saturated_costs(models):
    """Equal pixels of a binary image and its inverse differ by 255 in every channel, and where their gradients differ by 255 too
    the cost line gives trunc(229.5 + 25.5) = 255: a fifth of the volume, far beyond the 238 that uniform noise reaches."""
    m = models("sat_binary_inverse")
    for raw in ("raw_l", "raw_r"):
        assert (m[raw] == 255).mean() >= 0.15
    m = models("sat_channel_noise")
    assert (m["raw_l"] == 255).any() and (m["raw_l"] == 0).any()


@pytest.mark.parametrize("cases", [[c for c in I.IMAGE_CASES if c.family == "half"], [c for c in I.UPLOAD_CASES if "stripes" in c.name]],
                         ids=["image_form", "uploaded_form"])
def test_exact_halves_of_both_parities(models, cases):
    assert cases
    even = sum(e["half_even"] for c in cases for e in edge_counts(models(c.name)))
    odd = sum(e["half_odd"] for c in cases for e in edge_counts(models(c.name)))
    assert even >= 100 and odd >= 100, (even, odd)


@pytest.mark.parametrize("name", [c.name for c in I.CASES if c.family == "tie"] + ["up_repeated_min"])
def test_ties_on_the_winning_value(models, name):
    c, m = I.BY_NAME[name], models(name)
    rows, _, below, above = I.seed_stride_rule()
    tied, _ = tie_counts(m, below)
    assert 2 * tied >= 2 * c.W * c.H, tied                   # at least half the pixels of both maps


@pytest.mark.parametrize("S", [5, 8])
def test_ties_meet_a_seed_slice_and_a_key_slice(models, S):
    """Among the tied pixels some hold the winning value in a slice with local index = 0 mod S and in one that has not - in the
    cases whose height makes the forced two-phase selection take that S."""
    rows, _, below, above = I.seed_stride_rule()
    assert S in (below, above)
    cases = [c for c in I.CASES if c.family == "tie" and (c.H < rows) == (S == below)]
    assert cases
    for c in cases:
        assert tie_counts(models(c.name), S)[1] >= 1, c.name


MUTANT_CASES = {"fma": ["table_black", "table_white"],
                "floor": ["half_100x24", "half_96x208", "up_stripes_100x24", "up_stripes_96x208"],
                "wrap": [c.name for c in I.CASES if c.family == "extrap"]}


@pytest.mark.parametrize("mutant", sorted(MUTANT_CASES))
def test_every_mutant_is_seen(oracle, models, mutant):
    """On each case meant for it the mutant changes a volume AND the keys: what the GPU tests compare."""
    for name in MUTANT_CASES[mutant]:
        raw, vol, keys = mutant_counts(oracle, I.BY_NAME[name], models(name))[mutant]
        assert raw + vol >= 1 and keys >= 1, (name, raw, vol, keys)
    if mutant == "fma":       # a fact of fp32: 471 of the 65 536 pairs truncate differently with the product fused, (12, 2) among them
        c, g = np.divmod(np.arange(65536), 256)
        differ = M.cost(c, g) != M.cost(c, g, "fma")
        assert int(differ.sum()) == 471 and differ[12 * 256 + 2]
