"""CPU: the generators and references of tests/fgf_inputs.py held to the conditions that keep the Fast Guided Filter tests on the
device (tests/test_gpu_fgf_seams.py) from being vacuous: that the case list reaches every strip, segment, block and chunk form of
the launches of psm_fgf.hip, that the composed reference is psmo_pipeline_fgf, and that each adversarial volume has, in the
reference, the property it was built for."""
import numpy as np
import pytest

import fgf_inputs as G
import fuzz_inputs as F


def test_the_case_list_is_a_function_of_nothing():
    assert G.cases() == G.cases() and G.refusal_cases() == G.refusal_cases()
    for c in G.cases()[::9]:
        (al, ar), (bl, br) = G.content(c), G.content(c)
        assert np.array_equal(al, bl) and np.array_equal(ar, br)
        assert al.shape == (c[2], c[1], 3) and al.dtype == np.uint8
    for s in G.RATES:
        a, b = G.adversarial_volume("nan", s), G.adversarial_volume("nan", s)
        assert np.array_equal(a, b, equal_nan=True)


def test_the_case_list_holds_every_required_form():
    cases = G.cases()
    assert G.missing(cases) == []
    assert len({c[1:5] for c in cases}) == len(cases)                   # no geometry twice
    for c in cases:
        _, W, H, D, s, kind, _ = c
        assert W >= 8 and H >= 8 and 2 <= D <= W and not G.refused(W, H, s), c
        assert W * H * D <= 400_000, c                                  # a few ms on the device, well under a second in the oracle
    # the table is no tautology: without its group of cases an entry is missed
    for tag, name in (("strips", "three strips"), ("segments", "three segments"), ("x-blocks", "two x-blocks of the 4-pixel kernels, one live thread in the second"),
                      ("strips x segments", "two strips and two segments, 16-byte rows")):
        assert {n for n, _ in G.missing([c for c in cases if c[0] != tag])} >= {name}, tag
    assert any(n.startswith("D = 65") for n, _ in G.missing([c for c in cases if c[0] != "chunks"]))
    assert any(n.startswith("small") for n, _ in G.missing(G.seam_cases()))


def test_grid_restates_the_launch_arithmetic():
    """Known answers worked out by hand from launch_fgf_model / launch_fgf_apply[_wta] (psm_fgf.hip)."""
    g = G.grid(1920, 1080, 256, 4)           # ws 480 -> 8 strips of 60; nsegs 4 -> seg 68 -> 4 segments, the last 270 - 204 = 66 rows
    assert (g["ws"], g["hs"], g["strips"], g["last_strip"], g["segs"], g["seg"], g["last_seg"]) == (480, 270, 8, 60, 4, 68, 66)
    assert (g["fused"], g["xblocks"], g["chunks"]) == (True, 2, 8)
    assert g["apply4"] == (4, 2, 2) and g["apply_wta"] == (2, 0, 0)       # yshift 2 | 0; 1080 + 2 = 4 * 270.5 -> 271 blocks, 2 rows below
    g = G.grid(504, 104, 3, 8)               # ws 63 = 62 + 1, hs 13 = 12 + 1
    assert (g["strips"], g["last_strip"], g["segs"], g["seg"], g["last_seg"]) == (2, 1, 2, 12, 1)
    g = G.grid(450, 375, 64, 2)              # W % 4 = 2: k_fgf_apply, 256 columns per block
    assert (g["fused"], g["xblocks"], g["strips"], g["segs"], g["seg"]) == (False, 2, 5, 6, 36)
    g = G.grid(1028, 10, 2, 2)
    assert (g["xblocks"], g["chunks"], g["apply4"], g["apply_wta"]) == (2, 1, (2, 1, 1), (2, 1, 1))
    g = G.grid(44, 41, 2, 4)                 # apply4<4>: rows -2 .. 41 in 11 blocks: 2 above, 1 below; apply_wta<2>: 21 blocks, 1 below
    assert g["apply4"] == (4, 2, 1) and g["apply_wta"] == (2, 0, 1)
    for s, k in ((2, 9), (4, 5), (8, 3)):
        assert G.strip_width(s) == 64 - (k - 1) and G.grid(40, 8 * k * s, 2, s)["seg"] == 4 * k


def test_what_the_existing_cases_left_out():
    """The gap this list closes, from the same arithmetic: the shapes of test_gpu_fgf.py's parity test and the golden pairs (450 x
    375) have one strip at s = 8 and at most two at s = 4, and no last segment shorter than the radius."""
    old = [(64, 48, 9), (70, 45, 6), (61, 37, 5), (161, 120, 20), (450, 375, 64)]
    for s in G.RATES:
        gs = [G.grid(W, H, D, s) for W, H, D in old]
        assert max(g["strips"] for g in gs) == {2: 5, 4: 2, 8: 1}[s]
        assert all(g["xblocks"] == 1 or not g["fused"] for g in gs)
        assert all(g["segs"] == 1 or g["last_seg"] > G.radius(s) for g in gs)


def test_nn_idx_is_what_the_oracle_reads(oracle):
    rng = np.random.default_rng(3)
    for s in G.RATES:
        for H, W in ((24, 40), (23, 43), (17, 19)):
            img = rng.random((H, W, 3), dtype=np.float32)
            setup = oracle.fgf_setup(img, s)
            assert np.array_equal(setup[1], img[:, :, 1][np.ix_(G.nn_idx(H, s), G.nn_idx(W, s))])


@pytest.mark.parametrize("W,H,D,s", [(64, 48, 5, 4), (45, 37, 4, 2), (70, 45, 3, 8), (10, 17, 3, 2), (19, 12, 2, 4), (16, 23, 3, 8), (247, 24, 2, 4)])
def test_the_composed_reference_is_the_pipeline(oracle, W, H, D, s):
    l, r = F.sgm_content("half_flat", W, H, D, np.random.default_rng(W * H))
    a = G.reference(l, r, D, s)
    b = oracle.pipeline_fgf(l, r, D, s=s, threads=3, want_volumes=True)
    for k in ("lvol", "rvol", "ldisp", "rdisp"):
        assert np.array_equal(a[k], b[k]), k
    # the float pair byte / 255 is the same pair; a shard's reference is the slices of the whole one
    c = G.reference(oracle.u8_to_f32(l), oracle.u8_to_f32(r), D, s, d_range=(1, D))
    assert np.array_equal(c["lvol"], b["lvol"][1:]) and np.array_equal(c["rvol"], b["rvol"][1:]) and "ldisp" not in c
    q, m = G.reference_uploaded(l, b["rvol"], s)
    assert q.shape == (D, H, W) and np.array_equal(m, oracle.wta(q))


def test_refusal_cases_sit_on_both_sides_of_the_bound(oracle):
    from primestereomatch_amd import synth
    seen = set()
    for W, H, s, no in G.refusal_cases():
        assert G.refused(W, H, s) == no and W >= 8 and H >= 8
        R = G.radius(s)
        small = min(W // s, H // s)
        assert small == (R if no or (W, H) == (8, 8) else R + 1) or (W, H) == (8, 8)
        seen.add((s, no, "W" if W // s <= H // s else "H"))
        l, r, _ = synth.make_pair(W, H, 2, seed=1)
        if no:                                             # the oracle draws the line where the library does
            with pytest.raises(ValueError):
                oracle.pipeline_fgf(l, r, 2, s=s)
        else:
            oracle.pipeline_fgf(l, r, 2, s=s)
    assert seen >= {(s, no, ax) for s in G.RATES for no in (True, False) for ax in "WH"}


@pytest.mark.parametrize("W,H,D,s,seed", G.FLOAT_CASES)
def test_float_pairs_keep_what_tells_the_readings_apart(W, H, D, s, seed):
    lf, rf = G.float_pair(W, H, D, seed)
    halves = F.half_products()
    for f in (lf, rf):
        assert f.dtype == np.float32 and f.shape == (H, W, 3) and np.isfinite(f).all()
        assert (f < 0).any() and (f > 1).any() and (np.signbit(f) & (f == 0)).any() and np.isin(f, halves).any()
    assert not G.refused(W, H, s)


def test_the_repeats_sit_inside_a_chunk_and_across_the_seams():
    pairs = {(a // 32, b // 32) for a, b in G.REPEATS}
    assert pairs == {(0, 1), (0, 2), (1, 2), (1, 1), (2, 2)}           # both seams, first against last, and ties within one thread's loop


def _refs(name, s):
    l, _ = G.adversarial_guidance()
    vol = G.adversarial_volume(name, s)
    return vol, *G.reference_uploaded(l, vol, s)


@pytest.mark.parametrize("s", G.RATES)
@pytest.mark.parametrize("T", G.REPEATS)
def test_repeated_slices_tie_exactly_and_the_lower_wins(oracle, T, s):
    vol, q, m = _refs(f"repeats-{T[0]}-{T[1]}", s)
    assert vol.shape == (G.ADV_D, G.ADV_H, G.ADV_W) and G.grid(G.ADV_W, G.ADV_H, G.ADV_D, s)["chunks"] == 3
    assert np.array_equal(q[T[0]], q[T[1]])
    others = np.delete(q, T, axis=0)[1:]                               # (d = 0 is no candidate)
    gap = float((others - q[T[0]]).min())
    print(f"[fgf-inputs] repeats {T} s={s}: gap to the other slices {gap:.6f}")
    assert gap > 0.99
    assert (m == min(T)).all()


@pytest.mark.parametrize("s", G.RATES)
def test_negative_slice_wins_with_a_negative_cost(oracle, s):
    vol, q, m = _refs("negative", s)
    neg = (G.NEGATIVE_D,) + tuple(d for d, _ in G.NEGATIVE_OTHERS)
    assert sorted(d // 32 for d in neg) == [0, 1, 2]                     # one negative slice in each chunk
    assert (m == G.NEGATIVE_D).all() and (q[list(neg)] < 0).all() and (np.delete(q, neg, axis=0) > 0).all()
    assert all((q[d] - q[G.NEGATIVE_D]).min() > 0.99 for d, _ in G.NEGATIVE_OTHERS)
    # keys that order negative floats by their raw bits pick the one nearest zero
    raw = q[list(neg)].view(np.int32).astype(np.int64)
    assert (np.array(neg)[raw.argmin(axis=0)] == G.NEGATIVE_OTHERS[0][0]).all()


@pytest.mark.parametrize("s", G.RATES)
def test_subnormal_slice_stays_subnormal_and_wins(oracle, s):
    vol, q, m = _refs("subnormal", s)
    tiny = np.finfo(np.float32).tiny
    a, b = q[G.SUBNORMAL_D], q[G.SUBNORMAL_OTHER]
    n = int(np.count_nonzero((a > 0) & (a < tiny)))
    print(f"[fgf-inputs] subnormal s={s}: {n} of {a.size} pixels of the filtered slice subnormal and not zero")
    assert n == a.size and (b > a).all() and (b < tiny).all()
    assert (np.delete(q, (G.SUBNORMAL_D, G.SUBNORMAL_OTHER), axis=0) >= 0.99).all()
    assert (m == G.SUBNORMAL_D).all()
    # flushed to zero the two slices tie and the lower one wins: the map tells
    flushed = q.copy()
    flushed[np.abs(flushed) < tiny] = 0
    assert (oracle.wta(flushed) == G.SUBNORMAL_OTHER).all()


@pytest.mark.parametrize("s", G.RATES)
def test_nan_volume_reaches_the_filter_and_the_map(oracle, s):
    vol, q, m = _refs("nan", s)
    yi, xi = G.nn_idx(G.ADV_H, s), G.nn_idx(G.ADV_W, s)
    for ys, xs in G.nan_pixels(s):                                      # the special values sit on pixels the subsampling reads
        assert np.isin(ys, yi).all() and np.isin(xs, xi).all()
    sampled = vol[:, yi][:, :, xi]
    assert np.isnan(sampled[G.NAN_SLICE]).all() and np.isnan(sampled[:, 0, 0]).all()
    assert 1 <= np.isnan(sampled[G.NAN_WINNER]).sum() - 1 <= 2 and np.isnan(sampled[G.NAN_SECOND]).sum() == 1
    all_nan = np.isnan(q[1:]).all(axis=0)
    assert np.isnan(q[G.NAN_SLICE]).all()
    assert all_nan.any() and not all_nan.all() and np.array_equal(m == 0, all_nan)           # no candidate: the map keeps 0
    under = np.isnan(q[G.NAN_WINNER]) & ~np.isnan(q[G.NAN_SECOND])
    huge = q[G.NAN_HUGE]
    print(f"[fgf-inputs] nan s={s}: {int(all_nan.sum())} pixels without a candidate, {int(under.sum())} under the patch alone, winners "
          f"{sorted(set(m.ravel().tolist()))}; slice {G.NAN_HUGE}: {int(np.isnan(huge).sum())} NaN, {int(np.isinf(huge).sum())} inf")
    assert under.any() and (m != G.NAN_SLICE).all()
    free = ~np.isnan(q[G.NAN_WINNER])
    not_huge = m != G.NAN_HUGE                                          # (where slice 60 came out -inf it wins: the reference decides)
    assert (m[free & not_huge] == G.NAN_WINNER).all() and (m[under & not_huge] == G.NAN_SECOND).all()
    assert (m[under] == G.NAN_SECOND).any()
    assert (m[free] == G.NAN_WINNER).any()
    assert not np.isfinite(huge).all()                                  # its products did overflow
