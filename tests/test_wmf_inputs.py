"""CPU: tests/wmf_model.py held to the oracle, and the generators of tests/wmf_inputs.py held to the conditions without which
tests/test_gpu_wmf_adversarial.py would prove nothing: that a knife-edge window really changes its result with the order of the
additions, a denormal window with flushing, that a domino map really needs more sweeps than the device's cap, that a count of
invalid pixels is exact and that the seams of the geometry list are all there."""
import numpy as np
import pytest

import wmf_inputs as G
import wmf_model as M

SEED_KNIFE, SEED_DENORMAL = 5, 6          # (the seeds test_gpu_wmf_adversarial.py uploads)


def _oracle_maps(oracle, inp, D):
    return [oracle.wgt_median(oracle.u8_to_f32(inp.img[s]), inp[1 + s], inp[3 + s], D, right=bool(s)) for s in (0, 1)]


def test_the_model_forms_the_oracles_float_image(oracle):
    img = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    assert np.array_equal(G.to_f32(img), oracle.u8_to_f32(img))


@pytest.mark.parametrize("right", [False, True])
def test_evaluate_is_the_oracle_for_isolated_pixels(oracle, right):
    """Raster order, nothing flushed: the oracle's result at pixels that have no other invalid pixel in their window - on an image
    smaller than the window in one direction, too (the taps wrap onto the same pixels)."""
    for (h, w, D) in ((40, 50, 32), (12, 60, 9), (9, 9, 5)):
        rng = np.random.default_rng(h * w)
        f = G.to_f32(G.smooth_image(h, w, rng))
        dis = rng.integers(0, D, (h, w)).astype(np.uint8)
        pix = np.array([(5, 5), (5, 30), (30, 10), (0, 0), (h - 1, w - 1)])
        pix = pix[(pix[:, 0] < h) & (pix[:, 1] < w)][: 1 if min(h, w) < 19 else None]
        valid = np.ones((h, w), np.uint8)
        valid[pix[:, 0], pix[:, 1]] = 0
        want = oracle.wgt_median(f, dis, valid, D, right=right)[pix[:, 0], pix[:, 1]]
        assert np.array_equal(M.evaluate(f, dis, pix, D, right), want)
        for order in M.ORDERS[1:]:                     # smooth random content is not order-sensitive: the other orders agree here
            assert np.array_equal(M.evaluate(f, dis, pix, D, right, order), want)


def test_tap_orders_are_permutations():
    for o in M.ORDERS:
        assert sorted(M.tap_order(o)) == list(range(M.TAPS))
    assert M.tap_order("rows_reversed")[0] == M.TAPS - 19 and M.tap_order("cols_reversed")[0] == 18
    with pytest.raises(ValueError):
        M.tap_order("columns_first")


def test_the_generators_are_functions_of_their_arguments():
    assert G.wm_geometries(24, 3) == G.wm_geometries(24, 3) != G.wm_geometries(24, 4)
    for gen, args in ((G.knife_edge, (40, 60, 16, 1)), (G.denormal_windows, (40, 60, 16, 1)), (G.zero_windows, (70, 70, 7, 1)),
                      (G.counted_invalid, (20, 30, 9, 1, 7, 0)), (G.random_case, (19, 9, 5, 0.5, 1))):
        a = gen(*args)
        b = gen.__wrapped__(*args)
        assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))
        assert all(np.array_equal(x, y) for x, y in zip(a.pixels, b.pixels))
        assert not a.lmap.flags.writeable                  # a cached result cannot be changed under the next test


def _check_bulk(inp, bulk, H, W):
    """the bulk rows carry >= 8192 invalid pixels per side and stay more than 9 rows from every cell, counting through the wrap"""
    HH = inp.lmap.shape[0]
    assert HH == H + bulk + (G.GAP if bulk else 0)
    cells = G.cell_centres(H, W)
    for v in (inp.lvalid, inp.rvalid):
        rows = np.flatnonzero((v[H:] == 0).any(axis=1)) + H
        assert (bulk == 0) == (len(rows) == 0)
        if bulk:
            assert int((v[H:] == 0).sum()) >= 8192
            dist = np.abs(rows[:, None] - cells[None, :, 0])
            assert int(np.minimum(dist, HH - dist).min()) > 2 * M.R          # no bulk pixel in a cell's window, no cell in a bulk pixel's
        assert int((v[:H] == 0).sum()) == len(cells) == 4 * (W // G.CELL) >= 40


@pytest.mark.parametrize("bulk", [0, G.BULK_ROWS])
@pytest.mark.parametrize("H,W,D", G.KNIFE_CASES)
def test_knife_edge_windows_depend_on_the_order_of_the_additions(oracle, H, W, D, bulk):
    inp = G.knife_edge(H, W, D, SEED_KNIFE, bulk)
    _check_bulk(inp, bulk, H, W)
    want = _oracle_maps(oracle, inp, D)
    for s, name in ((0, "left"), (1, "right")):
        assert int(inp[1 + s].max()) < D
        pix = inp.pixels[s]
        f = G.to_f32(inp.img[s])
        raster = M.evaluate(f, inp[1 + s], pix, D, s)
        assert np.array_equal(raster, want[s][pix[:, 0], pix[:, 1]])          # the model in raster order is the oracle ...
        other = {o: M.evaluate(f, inp[1 + s], pix, D, s, o) for o in M.ORDERS[1:]}
        differs = {o: int((v != raster).sum()) for o, v in other.items()}
        walk = int(((other["rows_reversed"] != raster) | (other["cols_reversed"] != raster)).sum())
        print(f"[wmf-inputs] knife_edge D={D} bulk={bulk} {name}: {len(pix)} of {4 * (W // G.CELL)} windows order-sensitive; differing from raster order: "
              f"{differs}; under a reversed walk: {walk}")
        assert len(pix) >= 8                                                  # ... and another order is not, at every listed pixel
        assert all(any(other[o][k] != raster[k] for o in other) for k in range(len(pix)))
        # a reversed walk (what a kernel that splits the window between lanes or runs its rows backwards would do) must be
        # among what is told apart, not only the balanced tree
        assert walk >= 8
        assert set(np.unique(raster)) <= set(np.unique(inp[1 + s][:H]))


@pytest.mark.parametrize("bulk", [0, G.BULK_ROWS])
@pytest.mark.parametrize("H,W,D", G.KNIFE_CASES)
def test_denormal_windows_depend_on_denormals(oracle, H, W, D, bulk):
    inp = G.denormal_windows(H, W, D, SEED_DENORMAL, bulk)
    _check_bulk(inp, bulk, H, W)
    want = _oracle_maps(oracle, inp, D)
    for s, name in ((0, "left"), (1, "right")):
        assert int(inp[1 + s].max()) < D
        pix = inp.pixels[s]
        assert len(pix) == 4 * (W // G.CELL)                                  # no cell may be dropped
        f = G.to_f32(inp.img[s])
        q, wts = M.window(f, pix, s)
        votes = inp[1 + s].reshape(-1)[q] != 0
        assert votes.sum(axis=0).min() == M.TAPS - 1
        assert (wts[votes] < M.F32_MIN).all()                                 # every voting weight: a denormal or 0
        nonzero = (votes & (wts > 0)).sum(axis=0)
        kept = M.evaluate(f, inp[1 + s], pix, D, s)
        flushed = M.evaluate(f, inp[1 + s], pix, D, s, flush=True)
        print(f"[wmf-inputs] denormal_windows D={D} bulk={bulk} {name}: {int((kept != flushed).sum())} of {len(pix)} pixels differ when "
              f"denormals are flushed; denormal voters per window {int(nonzero.min())} .. {int(nonzero.max())}")
        assert np.array_equal(kept, want[s][pix[:, 0], pix[:, 1]])
        assert (kept != flushed).all() and not flushed.any() and nonzero.min() >= 2
        for o in M.ORDERS[1:]:                                                # (sums of denormals are exact: no order changes them)
            assert np.array_equal(M.evaluate(f, inp[1 + s], pix, D, s, o), kept)


@pytest.mark.parametrize("name", sorted(G.DOMINO_CASES))
def test_domino_maps_need_more_sweeps_than_the_cap(oracle, name):
    """The device gives up after 96 sweeps.  A device sweep sees some of its own changes, so it may need fewer than the synchronous
    model; at least 150 here on both sides leaves room for that."""
    inp = G.domino(*G.DOMINO_CASES[name])
    want = _oracle_maps(oracle, inp, 16)
    for s in (0, 1):
        n, fixed = M.jacobi_sweeps(G.to_f32(inp.img[s]), inp[1 + s], inp[3 + s], 16, s, cap=2000)
        ninv = int((inp[3 + s] == 0).sum())
        print(f"[wmf-inputs] domino {name} side {s}: {n} synchronous sweeps, {ninv} invalid pixels, "
              f"{int((want[s] != inp[1 + s]).sum())} of them change")
        assert np.array_equal(fixed, want[s])
        assert n >= 150
        assert (ninv >= 8192) == name.startswith("lane")
        assert np.array_equal(want[s][inp[3 + s] == 0], np.full(ninv, G.DOMINO_CASES[name][5], np.uint8))      # every domino falls


def test_domino_control_has_no_chain(oracle):
    inp = G.domino(*G.DOMINO_CONTROL)
    want = _oracle_maps(oracle, inp, 16)
    for s in (0, 1):
        n, fixed = M.jacobi_sweeps(G.to_f32(inp.img[s]), inp[1 + s], inp[3 + s], 16, s, cap=96)
        assert np.array_equal(fixed, want[s]) and 1 <= n <= 3
        assert not np.array_equal(fixed, inp[1 + s])          # (the pixels do flip - at once)
        assert M.jacobi_sweeps(G.to_f32(inp.img[s]), inp[1 + s], inp[3 + s], 16, s, cap=1)[0] == -1       # the cap is honoured


def test_jacobi_sweeps_reach_the_in_place_map_on_random_content(oracle):
    rng = np.random.default_rng(8)
    h, w, D = 30, 44, 24
    f = G.to_f32(G.smooth_image(h, w, rng))
    dis = rng.integers(0, D, (h, w)).astype(np.uint8)
    valid = (rng.random((h, w)) > 0.6).astype(np.uint8)
    for right in (False, True):
        n, fixed = M.jacobi_sweeps(f, dis, valid, D, right, cap=200)
        assert n > 1 and np.array_equal(fixed, oracle.wgt_median(f, dis, valid, D, right=right))
    assert M.jacobi_sweeps(f, dis, np.ones_like(valid), D, False, cap=5)[0] == 1


@pytest.mark.parametrize("D", [64, 2])
def test_zero_windows_have_pixels_without_a_vote(oracle, D):
    inp = G.zero_windows(*G.ZERO_GEO, D, 3)
    want = _oracle_maps(oracle, inp, D)
    for s in (0, 1):
        pix = inp.pixels[s]
        m = inp[1 + s]
        print(f"[wmf-inputs] zero_windows D={D} side {s}: {len(pix)} invalid pixels with an all-zero window")
        B = G.BLOCK
        assert len(pix) >= 8 and int(m.max()) < D and not m[:B, :B].any() and m[:B, B:2 * B].all() and not m[B:2 * B, :B].any()
        assert not want[s][:B, :B].any() and want[s][B:2 * B, :B].any()          # the guarded block stays 0, the plain one does not
        assert not want[s][pix[:, 0], pix[:, 1]].any()
        assert not M.evaluate(G.to_f32(inp.img[s]), m, pix, D, s).any()
        assert 0 < int((inp[3 + s] == 0).sum()) < m.size
        assert ((m == 0) & (inp[3 + s] != 0)).any() and ((m != 0) & (inp[3 + s] == 0)).any()      # valid and invalid in both kinds of region


def test_counted_invalid_counts_exactly():
    Hc, Wc, D = G.COUNTED_GEO
    assert {c[0] for c in G.COUNTS} >= {8191, 8192, 8193, 8256, 8257} and (8191, 8193) in G.COUNTS and (0, 8192) in G.COUNTS
    for nl, nr in G.COUNTS:
        inp = G.counted_invalid(Hc, Wc, D, 11, nl, nr)
        assert int((inp.lvalid == 0).sum()) == nl and int((inp.rvalid == 0).sum()) == nr
        assert int(inp.lmap.max()) < D and int(inp.rmap.max()) < D
        assert set(np.unique(inp.lvalid)) <= {0, 1}
    a, b = G.counted_invalid(Hc, Wc, D, 11, 400, 400, 1), G.counted_invalid(Hc, Wc, D, 11, 400, 400, 2)
    assert np.array_equal(a.img, b.img) and not np.array_equal(a.lmap, b.lmap) and not np.array_equal(a.lvalid, b.lvalid)


def test_geometry_list_holds_every_seam():
    geo = G.geometry_cases()
    assert 24 <= len(geo) <= 24 + len(G.REQUIRED)
    for Wg, Hg, D, frac, form, seed in geo:
        assert 9 <= Wg and 9 <= Hg and 2 <= D <= min(Wg, 256) and frac in G.FRACS and form in G.FORMS
        inp = G.random_case(Wg, Hg, D, frac, seed)
        assert inp.lmap.shape == (Hg, Wg) and int(inp.lmap.max()) < D and int(inp.rmap.max()) < D
        if frac == 1.0:
            assert not inp.lvalid.any() and not inp.rvalid.any()
    for name, has, _ in G.REQUIRED:
        assert any(has(*g[:3]) for g in geo), name
    assert {g[3] for g in geo} == set(G.FRACS) and {g[4] for g in geo} == set(G.FORMS)
    assert any(g[0] < 19 and g[1] < 19 for g in geo) and any(g[0] == g[2] for g in geo)
    empty = G.wm_geometries(0, 1)
    for name, has, fallback in G.REQUIRED:
        assert has(*fallback) and any(has(*g[:3]) for g in empty), name
