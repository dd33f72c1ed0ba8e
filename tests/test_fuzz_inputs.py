"""CPU: the generators of tests/fuzz_inputs.py held to the conditions that keep the sweeps on the device
(tests/test_gpu_sgm_fuzz.py, tests/test_gpu_jwmf_fuzz.py) from being vacuous.  Everything here is checked on the numpy models alone:
that a saturating pair reaches the packing bound of the select kernel, that a stripes pair has exact ties of S, that a float pair
holds the values that tell rint from floor(x + 0.5), on which side of the identity / k-means switch a JointWMF image falls."""
import numpy as np
import pytest

import fuzz_inputs as F
import jwmf_model as J
import sgm_bt_model as B
import sgm_model as M


def two_smallest_equal(S):
    s = np.sort(S.astype(np.int64), axis=2)
    return int(np.count_nonzero(s[:, :, 0] == s[:, :, 1]))


def test_the_generators_are_functions_of_their_seeds():
    assert F.sad_cases() == F.sad_cases() and F.bt_cases() == F.bt_cases() and F.jw_cases() == F.jw_cases()
    assert F.sgm_batches(8, 5) == F.sgm_batches(8, 5) and F.jwmf_batches(6, 5) == F.jwmf_batches(6, 5)
    assert F.sgm_geometries(10, 1) != F.sgm_geometries(10, 2)
    for g in F.sad_cases()[:6]:
        a, b = F.sgm_case(*g), F.sgm_case(*g)
        assert a[0] == b[0] and a[3:] == b[3:] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for c in F.jw_cases()[:6]:
        (al, ar), am = F.jwmf_build(c)
        (bl, br), bm = F.jwmf_build(c)
        assert np.array_equal(al, bl, equal_nan=True) and np.array_equal(ar, br, equal_nan=True) and np.array_equal(am, bm)


@pytest.mark.parametrize("cases", [F.sad_cases, F.bt_cases], ids=["sad", "bt"])
def test_geometry_lists_hold_every_seam(cases):
    geo = cases()
    assert 30 <= len(geo) <= 40 + len(F.REQUIRED)
    for W, H, D, _ in geo:
        assert 2 <= D <= min(W, 256) and W >= 8 and H >= 8 and W * H * D <= F.VOXELS
    for name, has, _ in F.REQUIRED:
        assert any(has(W, H, D) for W, H, D, _ in geo), name
    assert any(W == D for W, H, D, _ in geo)
    kinds = {F.sgm_case(*g, bt=cases is F.bt_cases)[0] for g in geo}
    assert kinds == set(F.SGM_KINDS), kinds                   # every content kind is drawn somewhere


def test_an_empty_draw_gets_every_required_geometry():
    geo = F.sgm_geometries(0, 1)
    assert geo and {g[:3] for g in geo} <= {fallback for _, _, fallback in F.REQUIRED}      # (a fallback may serve two entries)
    for name, has, fallback in F.REQUIRED:
        assert has(*fallback) and any(has(*g[:3]) for g in geo), name


def test_drawn_settings_are_accepted_by_the_model():
    seen = set()
    for i in range(200):
        kw, gray, speckle = F.sgm_settings(np.random.default_rng(i), bt=bool(i & 1))
        cap = kw.pop("pre_filter_cap", 0)
        bs, P1, P2, u, m = M.resolve_params(3, **kw)            # (what psm_sgm_set_params checks, whatever pair the compute takes)
        M.resolve_params(1, **kw)                               # a gray pair passes with room to spare
        assert (cap > 0) == bool(i & 1)
        seen.add(("bound", P2 == 65535 - bs * bs * 3 * 255))
        seen.add(("equal", P1 == P2))
        seen.add(("speckle", speckle[0] > 0))
    assert {("bound", True), ("equal", True), ("speckle", True), ("speckle", False)} <= seen


@pytest.mark.parametrize("W,H,D,d_star,bs", F.SATURATING_CASES)
def test_saturating_pairs_reach_the_packing_bound_in_the_model(W, H, D, d_star, bs):
    """max L_r = 65535 and max S = 8 * 65535 = 524280 < 2^19: the largest sum psm_sgm_set_params admits, the value the packed key
    (S << 8 | d) of k_sgm_select has to hold.  One channel (197115) and 120 x 100 (323595) do not get there."""
    l, r = F.saturating_pair(W, H, D, d_star)
    ref = M.sgm(l, r, D, **F.saturating_params(bs))
    near = int(np.count_nonzero(ref["S"] > (1 << 19) - 4096))
    print(f"[fuzz] saturating {W}x{H}x{D} d* {d_star} bs {bs}: max L_r {ref['max_l']}  max S {int(ref['S'].max())}  "
          f"voxels within 4096 of 2^19: {near}")
    assert ref["max_l"] == 65535
    assert int(ref["S"].max()) == 8 * 65535 == 524280
    assert near > 0


def test_saturating_pair_costs_are_0_or_255_ch_by_parity():
    l, r = F.saturating_pair(30, 8, 7, 3)
    c = M.pixel_cost(l, r, 7)
    x = np.arange(30)[None, :, None]
    d = np.arange(7)[None, None, :]
    inside = x - np.maximum(d, 3) >= 0                         # both reads unclamped
    want = np.where((d - 3) % 2 == 0, 0, 765)
    assert np.array_equal(c[inside & np.ones_like(c, bool)], np.broadcast_to(want, c.shape)[inside & np.ones_like(c, bool)])
    g = F.saturating_pair(30, 8, 7, 3, ch=1)
    assert g[0].shape == (8, 30) and np.array_equal(g[0], l[:, :, 0]) and np.array_equal(g[1], r[:, :, 0])


@pytest.mark.parametrize("W,H,D", F.HIGH_FLOOR_CASES)
def test_high_floor_pairs_put_the_minimum_of_s_above_2_pow_18(W, H, D):
    """The winner's S itself at and above 2^18: a select key with 18 bits for S decodes another minS at the first kind of pixel
    and picks another d at the second.  Without the uniqueness and consistency tests every pixel shows its d16."""
    l, r = F.high_floor_case(W, H, D)
    ref = M.sgm(l, r, D, uniqueness_ratio=0, disp12_max_diff=-1, **F.HIGH_FLOOR_PARAMS)
    S = ref["S"].astype(np.int64)
    above = int(np.count_nonzero(S.min(axis=2) >= 1 << 18))
    straddle = int(np.count_nonzero((S.min(axis=2) < 1 << 18) & (S.max(axis=2) >= 1 << 18)))
    print(f"[fuzz] high floor {W}x{H}x{D}: pixels with min S >= 2^18: {above}, with S on both sides of 2^18: {straddle}, of {W * H}; "
          f"max S {int(S.max())}, {len(np.unique(ref['disp']))} distinct map values")
    assert above > W * H // 4 and straddle > W * H // 8 and int(S.max()) < 1 << 19
    assert ref["valid"].all() and len(np.unique(ref["disp"])) > D
    wrapped = np.argmin(S & ((1 << 18) - 1), axis=2)                 # what 18 bits would select
    assert np.count_nonzero(wrapped != ref["best"]) > 0
    assert not M.sgm(l, r, D, **F.HIGH_FLOOR_PARAMS)["valid"].any()  # at the default ratio every pixel has a rival: the map is -16


def test_select_of_the_model_is_what_sgm_returns():
    """test_gpu_sgm_fuzz.py runs a saturating pair at three uniqueness ratios on one run of the model: select + consistency
    recomputed from S for another ratio is M.sgm at that ratio."""
    l, r = F.saturating_pair(40, 20, 7, 3)
    kw = F.saturating_params(1)
    ref = M.sgm(l, r, 7, **kw)
    for u in (99, 0):
        best, minS, unique, d16 = M.select(ref["S"], u)
        _, valid = M.consistency(best, minS, unique, d16, 1)
        assert np.array_equal(np.where(valid, d16, M.INVALID).astype(np.int16), M.sgm(l, r, 7, uniqueness_ratio=u, **kw)["disp"])


@pytest.mark.parametrize("kind,W,H,D,seed", F.TIE_CASES)
def test_tie_cases_in_the_models(kind, W, H, D, seed):
    """What the models say about the degenerate pairs test_ties_on_the_device uploads.
    constant, SAD: S is 0 everywhere, every pixel ties over all of D, the map is 0 everywhere (best 0 by the lowest-d rule, no d
    has S (100 - u) < 0, den clamped to 1 is never used at best 0).  constant, Birchfield-Tomasi: the border columns of the
    planes are ft, so S is not 0 - but the map is 0 everywhere too.  stripes: pixels whose two smallest S are equal, under both
    costs.  shift: the model's own result, no property claimed."""
    l, r = F.tie_pair(kind, W, H, D, seed)
    sad, bt = M.sgm(l, r, D), B.sgm(l, r, D, pre_filter_cap=63)
    ties = two_smallest_equal(sad["S"]), two_smallest_equal(bt["S"])
    print(f"[fuzz] {kind} {W}x{H}x{D}: pixels whose two smallest S tie: SAD {ties[0]}  BT {ties[1]};  max S {int(sad['S'].max())} / "
          f"{int(bt['S'].max())};  valid {sad['valid'].mean():.3f} / {bt['valid'].mean():.3f}")
    if kind == "constant":
        assert not sad["S"].any() and not sad["C"].any() and ties[0] == W * H
        assert not sad["disp"].any() and sad["valid"].all()
        assert bt["S"].any() and not bt["disp"].any()
    if kind == "stripes":
        assert ties[0] > 0 and ties[1] > 0
        assert np.array_equal(l[0], l[-1]) and len(np.unique(l[0].reshape(-1, 3), axis=0)) in (2, 3, 4, 8)
    if kind == "shift":
        assert any(np.array_equal(r, F._shifted(l, k)) for k in range(D))


def test_half_products_are_exact_ties_of_the_rounding():
    h = F.half_products()
    p = h * np.float32(255.0)
    assert p.dtype == np.float32 and len(h) >= 128
    assert np.array_equal(p - np.floor(p), np.full(len(h), 0.5, np.float32))
    q = M.quantise(h)
    assert np.array_equal(q % 2, np.zeros(len(h), np.uint8))                   # ties to even ...
    assert np.count_nonzero(q != np.floor(p + np.float32(0.5))) >= 64          # ... which floor(x + 0.5) misses on every odd k + 1


def scalar_quantise(img):
    """saturate_cast<uchar>(cvRound(f * 255.0f)) element by element: the product in fp32, Python's round (ties to even), explicit
    clamping, NaN -> 0."""
    out = np.empty(img.size, np.uint8)
    for i, f in enumerate(img.reshape(-1)):
        with np.errstate(invalid="ignore"):
            p = float(np.float32(f) * np.float32(255.0))
        if p != p:
            out[i] = 0
        elif p == float("inf"):
            out[i] = 255
        elif p == float("-inf"):
            out[i] = 0
        else:
            out[i] = min(max(round(p), 0), 255)
    return out.reshape(img.shape)


@pytest.mark.parametrize("W,H,D,seed", F.FLOAT_CASES)
def test_float_pairs_hold_every_class_and_quantise_as_the_scalar_loop(W, H, D, seed):
    rng = np.random.default_rng(seed)
    l, r = F.sgm_content("synth", W, H, D, rng)
    for f, u in zip(F.float_pair(l, r, rng), (l, r)):
        assert f.dtype == np.float32 and f.shape == u.shape
        with np.errstate(invalid="ignore"):
            p = f * np.float32(255.0)
        finite = np.isfinite(p)
        halves = finite & (p - np.floor(np.where(finite, p, 0)) == 0.5)
        counts = dict(half=int(halves.sum()), negative=int((f < 0).sum()), above_1=int((f > 1).sum()), inf=int(np.isposinf(f).sum()),
                      minus_inf=int(np.isneginf(f).sum()), nan=int(np.isnan(f).sum()), minus_0=int((np.signbit(f) & (f == 0)).sum()))
        print(f"[fuzz] float image {W}x{H}: {counts}")
        assert all(v > 0 for v in counts.values()), counts
        q = M.quantise(f)
        assert np.array_equal(q, scalar_quantise(f))
        plain = ~halves & finite & (f >= 0) & (f <= 1)
        assert np.count_nonzero(q != u) > 0 and np.count_nonzero(plain) > f.size // 2
        # rint, not floor(x + 0.5): the two differ on this very image
        assert np.count_nonzero(q[halves] != np.floor(p[halves] + np.float32(0.5))) > 0


def test_jwmf_cases_fall_on_the_side_of_the_switch_they_are_meant_for():
    cases = F.jw_cases()
    assert 41 <= len(cases) <= 60
    for field in (0, 1):                                                        # both directions around every multiple of JW_TILE
        assert set(F.JW_EDGE) <= {c[field] for c in cases}
    assert {c[2] for c in cases} == set(range(1, 17)) and {1, 2, 3, 16, 255, 256} <= {c[3] for c in cases}
    assert {"u8", "f32"} == {c[4] for c in cases}
    keys_seen, many, sides = set(), 0, {"identity": 0, "kmeans": 0}
    for case in cases:
        W, H, radius, nc, depth, ik, mk, sigma, seed = case
        assert 1 <= radius <= 16 and 1 <= nc <= 256 and ik[0] != ik[1] and mk[0] != mk[1] and sigma in F.JW_SIGMAS
        imgs, maps = F.jwmf_build(case)
        for img, kind, dmap in zip(imgs, ik, maps):
            assert img.shape == (H, W, 3) and img.dtype == (np.float32 if depth == "f32" else np.uint8)
            assert dmap.shape == (H, W) and dmap.dtype == np.uint8
            m = J.clustering_of(img, nc)
            n = len(m["samples"])
            keys_seen.add(kind)
            many += 1024 < n < 2048
            if kind == "palette_n":
                assert n == nc and m["iterations"] == 0, case
            elif kind == "palette_n1":
                assert n == nc + 1 and m["iterations"] > 1, case
            elif kind == "two":
                assert n == 2
            assert (n <= nc) == (m["iterations"] == 0)
            if n > nc:
                assert m["iterations"] > 1 and len(m["centres"]) == nc
            sides["identity" if n <= nc else "kmeans"] += 1
    print(f"[fuzz] JointWMF sides: {sides}, with 1024 < keys < 2048: {many}")
    assert keys_seen == set(F.JW_IMAGES) and many >= 1 and min(sides.values()) >= 10
    assert {c[7] for c in cases} == set(F.JW_SIGMAS)
    assert {k for c in cases for k in c[6]} == set(F.JW_MAPS)
    m = J.clustering_of(F.jwmf_build(F.JW_MANY_KEYS)[0][0], 256)
    assert 1024 < len(m["samples"]) < 2048 and m["iterations"] > 1


def test_jwmf_maps_leave_radix_digits_empty():
    rng = np.random.default_rng(3)
    assert len(np.unique(F.jwmf_map("constant", 17, 9, rng))) == 1
    assert set(np.unique(F.jwmf_map("extremes", 17, 9, rng))) == {0, 255}
    assert len(np.unique(F.jwmf_map("nibble", 17, 9, rng) >> 4)) == 1
    assert len(np.unique(F.jwmf_map("ramp", 60, 40, rng))) == 256


def test_the_sigmas_do_what_they_are_there_for():
    cen = J.key_xyz(np.array([0, 1, 64, 4096 + 65, 63 * 4096 + 63 * 64 + 63])).astype(np.float32)
    small, large = J.quantise(J.weight_table(cen, 0.05)), J.quantise(J.weight_table(cen, 1e6))
    off = ~np.eye(len(cen), dtype=bool)
    assert not small[off].any() and np.all(np.diag(small) == 1 << 48)           # integer centres: every cross-cluster weight is 0
    assert np.all(large[:4, :4] == 1 << 48) and np.all(large >= (1 << 48) - (1 << 25))


def test_the_first_batches_mix_what_they_promise():
    W, H, D, kinds, seed = F.sgm_batches(8, 99)[0]
    assert kinds == ("saturating", "constant", "noise")
    pairs, kw, speckle = F.sgm_batch_case(W, H, D, kinds, seed)
    assert len(pairs) == 3 and not np.ptp(pairs[1][0].reshape(-1, 3), axis=0).any()
    assert all(len(set(b[3])) == len(b[3]) for b in F.sgm_batches(8, 99))
    batch = F.jwmf_batches(6, 99)[0]
    assert [host for _, host in batch] == [(False, False), (False, False), (True, True)]
    its = [[J.clustering_of(img, case[3])["iterations"] for img in F.jwmf_build(case)[0]] for case, _ in batch[:2]]
    assert its[0] == [0, 0] and all(i > 1 for i in its[1]), its
    for b in F.jwmf_batches(6, 99):
        assert 2 <= len(b) <= 4 and len({c[:5] + (c[7],) for c, _ in b}) == 1
