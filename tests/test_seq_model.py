"""The generator of tests/seq_model.py held to its conditions over the committed seed list, on the CPU: these are conditions, not
measurements - they fail when an op leaves the vocabulary, a seed is dropped or a bias of the generator is lost, which is what
keeps tests/test_gpu_sequences.py looking where it is meant to look."""
import collections

import numpy as np
import pytest

import seq_model as S


@pytest.fixture(scope="module")
def walks():
    return [S.generate(seed) for seed in S.SEEDS]


def ops(walk):
    return [st for st in walk.steps if st.kind != "read"]


def test_same_seed_same_walk(walks):
    assert len(S.SEEDS) == 40 and len(set(S.SEEDS)) == 40
    for seed, w in zip(S.SEEDS, walks):
        again = S.generate(seed)
        assert [st.key() for st in again.steps] == [st.key() for st in w.steps], seed
        assert (again.shape, again.dtype) == (w.shape, w.dtype)
    assert len({tuple(st.key() for st in w.steps) for w in walks}) == len(walks)


def test_every_walk_replays_on_the_shadow(walks):
    for w in walks:
        n = 0
        for i, st, world, want in S.replay(w):
            n += 1
            if st.kind == "read":
                assert want is not None and all(e is not None for e in want[:1]), (w.seed, i, st)
        assert n == len(w.steps)


def test_every_op_kind_occurs(walks):
    count = collections.Counter(st.kind for w in walks for st in ops(w))
    print(sorted(count.items(), key=lambda kv: kv[1]))
    assert set(count) == set(S.OP_KINDS)
    for kind in S.OP_KINDS:
        assert count[kind] >= 10, (kind, count[kind])
    done = collections.Counter(st.kind for w in walks for st in ops(w) if st.refused is None)
    for kind in S.OP_KINDS:                          # ... and not only as a refusal
        assert done[kind] >= 5, (kind, done[kind])


def test_every_reader_occurs(walks):
    count = collections.Counter(st.args["what"] for w in walks for st in w.steps if st.kind == "read")
    print(dict(count))
    for what in ("download_maps", "download_valid", "sgm_disparity", "sgm_costs", "sgm_speckle_sizes", "score_maps", "download_images",
                 "jwmf_clusters"):
        assert count[what] >= 5, (what, count[what])


def test_foreign_writers_inside_the_early_map_window(walks):
    """Between a single-phase CostFilter and that context's next DispSelect: every writer of the map buffer other than the filter at
    least twice, carried out, not refused; JointWMF never (it has no maps to filter there), and at least twice outside."""
    inside = collections.Counter(st.kind for w in walks for st in ops(w) if st.window and st.refused is None)
    print(dict(inside))
    for kind in S.MAP_WRITERS:
        assert inside[kind] >= 2, (kind, inside[kind])
    assert inside["disp_select"] + inside["select_async"] >= 20          # the windows are closed by a select, which must then deliver
    outside = collections.Counter(st.kind for w in walks for st in ops(w) if not st.window and st.refused is None)
    for kind in S.JWMF_OPS:
        assert inside[kind] == 0 and outside[kind] >= 2, (kind, inside[kind], outside[kind])
        assert not any(st.window for w in walks for st in ops(w) if st.kind == kind)


def test_the_window_is_the_shadows(walks):
    """Step.window is what the shadow says at that step: open after a single-phase filter of fresh lazy costs, closed by a select, new
    costs, a new pair, another filter."""
    for w in walks:
        for i, st, world, _ in S.replay(w):
            if st.kind == "cost_filter" and st.refused is None:
                c = world.ctxs[st.ctx]
                assert c.window == (c.filt_rows == c.rows and c.lazy and not (c.flags & S.STORE) and not (c.flags & S.TWO_PHASE_ON
                                                                                                         and not c.flags & S.TWO_PHASE_OFF))
            if st.kind in ("disp_select", "select_async", "cost_const", "images", "float", "frame") and st.refused is None:
                assert not world.ctxs[st.ctx].window


def test_refusals_are_a_minority_and_name_a_call(walks):
    for w in walks:
        o = ops(w)
        refused = [st for st in o if st.refused is not None]
        assert 4 * len(refused) <= len(o), (w.seed, len(refused), len(o))
        for st in refused:
            assert st.refused.startswith("psm_")
    assert sum(st.refused is not None for w in walks for st in ops(w)) >= 40      # ... but they are there


def test_every_walk_compares_maps_and_an_sgm_result(walks):
    for w in walks:
        reads = collections.Counter(st.args["what"] for st in w.steps if st.kind == "read")
        assert reads["download_maps"] >= 3, (w.seed, dict(reads))
        assert reads["sgm_disparity"] + reads["sgm_costs"] >= 1, (w.seed, dict(reads))


def test_dtypes_modes_and_stripes(walks):
    assert {w.dtype for w in walks} == {"f32", "u8"}
    assert {w.shape for w in walks} == set(S.SHAPES)
    assert all(w.shape == S.SHAPES[0] for w in walks if w.dtype == "u8")
    on = off = striped = 0
    for w in walks:
        seen = set()
        for i, st, world, _ in S.replay(w):
            if st.kind == "cost_filter" and st.refused is None:
                c = world.ctxs[st.ctx]
                seen.add("on" if c.flags & S.TWO_PHASE_ON and not c.flags & S.TWO_PHASE_OFF else "off" if c.flags & S.TWO_PHASE_OFF else "")
                if c.filt_rows is not None:
                    seen.add("striped")
        on, off, striped = on + ("on" in seen), off + ("off" in seen), striped + ("striped" in seen)
    print(f"walks with a forced two-phase filter {on}, forced single-phase {off}, striped {striped} of {len(walks)}")
    assert 5 * on >= len(walks) and 5 * off >= len(walks) and 5 * striped >= len(walks)


def test_batches_name_subsets_in_any_order(walks):
    subsets = collections.Counter(st.ctx for w in walks for st in ops(w) if not isinstance(st.ctx, int))
    assert {len(c) for c in subsets} == {1, 2, 3}
    assert any(list(c) != sorted(c) for c in subsets)


def test_expressions_evaluate(oracle):
    """One walk of either shape through Refs: every value a reader compares exists, has the context's shape and comes out of the
    cache the second time."""
    for seed in (0, 1):
        w = S.generate(seed)
        data = S.Data(w.shape, seed)
        R = S.Refs(data, oracle, ("test", w.shape, seed))
        W, H, D = w.shape
        for i, st, world, want in S.replay(w):
            if st.kind != "read":
                continue
            what = st.args["what"]
            if what == "jwmf_clusters":
                for e in want[0]:
                    cen, lok, it = R(e)
                    assert cen.shape[1] == 3 and lok.shape == (64 ** 3,)
                continue
            v = R(want[0])
            assert R(want[0]) is v
            if what in ("download_maps", "download_valid", "download_images"):
                assert v[0].shape[:2] == (H, W) and v[0].dtype == np.uint8
            elif what in ("sgm_disparity", "sgm_costs"):
                nd = S.sgm_range(want[0], D)[1]
                assert v["d16"].shape == (H, W) and v["S"].shape == (H, W, nd)
    data = S.Data(S.SHAPES[0], 0)
    assert data.pairs[S.RECT][0].shape == (S.SHAPES[0][1], S.SHAPES[0][0], 3)
    lf, _ = data.float_pair(1)
    assert np.array_equal(lf, oracle.u8_to_f32(np.ascontiguousarray(data.pairs[1][0])))
