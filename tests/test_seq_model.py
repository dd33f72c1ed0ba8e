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


OLD_WALKS_SHA256 = "71ee35508fde7dd7d6ff8216063dad941cc3d52a242dfb22e8d49a79cdc0eb4e"


def test_the_forty_old_walks_are_what_they_were(walks):
    """sha256 over repr of every step key of the walks of SEEDS in order, computed with the model as it was before the tail
    vocabulary: a second vocabulary re-deals none of them."""
    import hashlib
    h = hashlib.sha256()
    for w in walks:
        for st in w.steps:
            h.update(repr(st.key()).encode())
    assert h.hexdigest() == OLD_WALKS_SHA256
    assert len(S.OP_KINDS) == 37 and not set(S.NEW_KINDS) & set(S.OP_KINDS)


# ------------------------------------------------------------------------------------------------------ the tail vocabulary

@pytest.fixture(scope="module")
def tails():
    return [S.generate(seed, vocabulary="tail") for seed in S.TAIL_SEEDS]


def timeline(walk):
    """[(index, step, shadow before the step, shadow after it, the names read right behind it per context)] of the ops of a walk"""
    import copy
    out, before = [], S.World(walk.shape, walk.dtype)
    for i, st, world, _ in S.replay(walk):
        if st.kind == "read":
            out[-1][4].setdefault(st.ctx, set()).add(st.args["what"])
            continue
        out.append((i, st, before, copy.deepcopy(world), {}))
        before = out[-1][3]
    return out


@pytest.fixture(scope="module")
def lines(tails):
    return [timeline(w) for w in tails]


def named(st):
    return (st.ctx,) if isinstance(st.ctx, int) else tuple(st.ctx)


def test_tail_same_seed_same_walk(tails):
    assert len(S.TAIL_SEEDS) == 24 and len(set(S.TAIL_SEEDS)) == 24
    for seed, w in zip(S.TAIL_SEEDS, tails):
        again = S.generate(seed, vocabulary="tail")
        assert [st.key() for st in again.steps] == [st.key() for st in w.steps], seed
        assert (again.shape, again.dtype) == (w.shape, w.dtype)
        assert len(ops(w)) <= S.STEPS + 8 and set(st.kind for st in ops(w)) <= set(S.TAIL_KINDS)
    assert len({tuple(st.key() for st in w.steps) for w in tails}) == len(tails)
    assert {w.shape for w in tails} == set(S.SHAPES) and {w.dtype for w in tails} == {"f32", "u8"}


def test_every_tail_walk_replays_on_the_shadow(tails):
    for w in tails:
        n = 0
        for i, st, world, want in S.replay(w):
            n += 1
            if st.kind == "read":
                assert want is not None and want[0] is not None, (w.seed, i, st)
        assert n == len(w.steps)


def test_every_new_op_kind_and_reader_occurs(tails, lines):
    count = collections.Counter(st.kind for w in tails for st in ops(w))
    done = collections.Counter(st.kind for w in tails for st in ops(w) if st.refused is None)
    print(sorted(count.items(), key=lambda kv: kv[1]))
    for kind in S.NEW_KINDS:
        assert count[kind] >= 10 and done[kind] >= 5, (kind, count[kind], done[kind])
    reads = collections.Counter(st.args["what"] for w in tails for st in w.steps if st.kind == "read")
    print(dict(reads))
    for what in S.NEW_READERS:
        assert reads[what] >= 10, (what, reads[what])
    # the score record and planes under the SGM sources while publishing is on
    published = collections.Counter()
    for line in lines:
        for i, st, before, after, reads_ in line:
            if st.kind in ("score", "score_batch") and st.refused is None and st.args["source"] != S.GIF:
                published[st.args["source"]] += sum(after.ctxs[c].wls_pub and "score_maps" in reads_.get(c, ()) for c in named(st))
    assert published[S.SGM] >= 5 and published[S.SGM_INT] >= 5, published


def test_the_new_ops_draw_from_their_sets(tails, lines):
    o = [st for w in tails for st in ops(w)]
    assert {st.args["source"] for st in o if st.kind in ("wls", "wls_async", "wls_batch") and st.refused is None} == {"gif", "gifm", "sgm"}
    assert {st.args["source"] for st in o if st.kind in ("reproject", "reproject_async", "reproject_batch") and st.refused is None} == {"gif", "gifm", "sgm"}
    assert {st.args["outs"] for st in o if st.kind.startswith("reproject") and "outs" in st.args and st.refused is None} == set(range(1, 8))
    assert {st.args["stages"] for st in o if st.kind == "pp_batch" and st.refused is None} == set(S.PP_STAGES)
    assert {(st.args["lam"], st.args["sigma"], st.args["iterations"]) for st in o if st.kind == "wls_params"} == set(S.WLS_PARAMS)
    assert {p[2] for p in S.WLS_PARAMS} == {1, 2, 3, 4} and S.WLS_PARAMS[0] == S.WLS_DEFAULT
    assert {(st.args["q"], st.args["zr"]) for st in o if st.kind == "reproject_q"} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {st.args["on"] for st in o if st.kind == "wls_publish" and st.refused is None} == {True, False}
    assert {st.args["mseed"] is None for st in o if st.kind == "hook_map"} == {True, False}
    for kind in ("wls_batch", "reproject_batch", "pp_batch"):
        subsets = {st.ctx for st in o if st.kind == kind and st.refused is None}
        assert {len(c) for c in subsets} == {1, 2, 3} and any(list(c) != sorted(c) for c in subsets), kind
    # a batch whose members differ in lambda and sigma; one refused because the iterations differ
    mixed = refused_iters = 0
    for line in lines:
        for i, st, before, after, _ in line:
            if st.kind == "wls_batch":
                pars = {before.ctxs[c].wls_par for c in st.ctx}
                mixed += st.refused is None and len(pars) > 1
                refused_iters += st.refused is not None and len({p[2] for p in pars}) > 1
    assert mixed >= 5 and refused_iters >= 1, (mixed, refused_iters)
    import depth_model as DM
    s3 = [[float(S.q_matrix(q)[3] @ np.array([0.0, 0.0, d, 1.0])) for d in (0.0, 1.0)] for q in (0, 1)]
    assert s3[0][0] != 0.0 and s3[1][0] == 0.0 and s3[1][1] != 0.0 and S.Q_CROPS[0] != (0, 0)
    assert S.Z_RANGES[0] == (0.0, DM.FLT_MAX)


def test_tail_refusals_are_a_minority_and_name_a_call(tails):
    for w in tails:
        o = ops(w)
        refused = [st for st in o if st.refused is not None]
        assert 4 * len(refused) <= len(o), (w.seed, len(refused), len(o))
        for st in refused:
            assert st.refused.startswith("psm_")
    assert sum(st.refused is not None for w in tails for st in ops(w)) >= 24


# ---- the interleavings: each a predicate of one walk's timeline, true in at least three walks ----
SGM_READERS = {"score": "score_maps", "score_batch": "score_maps", "reproject": "reprojected", "reproject_batch": "reprojected"}


def sgm_source_runs(line, only=("score", "score_batch", "reproject", "reproject_batch")):
    """(step, context, shadow before) of every carried-out run of an SGM source of psm_score / psm_reproject that is read behind it"""
    for i, st, before, after, reads in line:
        if st.kind in only and st.refused is None and st.args["source"] in ("sgm", S.SGM, S.SGM_INT):
            for c in named(st):
                if SGM_READERS[st.kind] in reads.get(c, ()):
                    yield st, c, before.ctxs[c]


def hook_over_a_published_result(line):
    """... the hook wins; the same again after the hook is dropped: the published map, read with its own invalid value"""
    hooked = set()
    for st, c, b in sgm_source_runs(line):
        if b.wls_pub and b.wls is not None:
            if b.hook is not None:
                hooked.add(c)
            elif c in hooked:
                return True
    return False


def stale_invalid_value(line):
    return any(b.wls_pub and b.wls is not None and b.hook is None and b.sgm is not None and (b.sgm[4] - 1) * 16 != b.wls[2]
               for st, c, b in sgm_source_runs(line, ("reproject", "reproject_batch")))


def hook_invalid_follows_the_setting(line):
    return any(b.hook is not None and b.hook[2] != (b.range_set[0] - 1) * 16 for st, c, b in sgm_source_runs(line, ("reproject", "reproject_batch")))


def stage_runs(line, stage):
    """per context: the carried-out runs of the WLS ("wls") or reprojection ("reproject") stage that are read behind them, and the
    other carried-out ops of that context, in order: [(step, shadow before, shadow after)]"""
    per = {c: [] for c in range(S.NCTX)}
    for i, st, before, after, reads in line:
        if st.refused is None:
            for c in named(st):
                if is_run(st, stage) and not st.kind.endswith("_async") and ("wls_planes" if stage == "wls" else "reprojected") not in reads.get(c, ()):
                    continue
                per[c].append((st, before.ctxs[c], after.ctxs[c]))
    return per


def is_run(st, stage):
    return st.kind in (stage, stage + "_async", stage + "_batch")


def rerun_after_release(line):
    for stage in ("wls", "reproject"):
        for c, seq in stage_runs(line, stage).items():
            state = 0
            for st, b, a in seq:
                if is_run(st, stage):
                    if state == 2:
                        return True
                    state = 1
                elif st.kind == "release_scratch" and state == 1:
                    state = 2
    return False


def weight_table_reload(line):
    """sigma A, a run, sigma B, a run, sigma A again, a run - on one context"""
    for c, seq in stage_runs(line, "wls").items():
        sig = [a.wls[4][1] for st, b, a in seq if is_run(st, "wls")]
        sig = [s for j, s in enumerate(sig) if j == 0 or s != sig[j - 1]]
        if any(sig[j] == sig[j + 2] for j in range(len(sig) - 2)):
            return True
    return False


def guide_follows_the_pair(line):
    for c, seq in stage_runs(line, "wls").items():
        last, new_pair = None, False
        for st, b, a in seq:
            if st.kind in ("images", "float", "frame"):
                new_pair = True
            elif is_run(st, "wls") and a.wls[3][1] != "gray":
                if last is not None and new_pair and last != a.wls[3]:
                    return True
                last, new_pair = a.wls[3], False
    return False


def staged_pair_not_adopted(line):
    """images_async between a wls_async (a reproject_async with the cloud) and its wait; the wait is carried out and read"""
    open_ = {}
    for i, st, before, after, reads in line:
        if st.refused is not None or not isinstance(st.ctx, int):
            continue
        c = st.ctx
        if st.kind == "wls_async" or (st.kind == "reproject_async" and st.args["outs"] & S.CLOUD):
            open_[c] = [st.kind, False]
        elif st.kind in ("images_async", "frame_async") and c in open_:
            open_[c][1] = True
        elif st.kind in ("wls_wait", "reproject_wait") and c in open_:
            kind, staged = open_.pop(c)
            if kind[:3] == st.kind[:3] and staged and after.ctxs[c].staged is not None and ("wls_planes" if kind[0] == "w" else "cloud") in reads.get(c, ()):
                return True
        elif st.kind in ("cost_const", "images", "float", "frame", "release_scratch", "wls", "reproject"):
            open_.pop(c, None)
    return False


def gray_guide(line):
    """sgbm_gray, then WLS (SGM) and a cloud under its plane; later a 3-channel sgbm and the same again under the pair"""
    for c in range(S.NCTX):
        seen = set()
        for i, st, before, after, reads in line:
            if st.refused is not None or c not in named(st) or st.args.get("source") != "sgm":
                continue
            a = after.ctxs[c]
            three = a.sgm is not None and not isinstance(a.sgm[1], tuple)
            if st.kind in ("wls", "wls_batch") and "wls_planes" in reads.get(c, ()):
                kind = a.wls[3][1]
                if kind == "gray":
                    seen.add("wg")
                elif three and {"wg", "cg"} <= seen:
                    seen.add("wp")
            if st.kind in ("reproject", "reproject_batch") and st.args["outs"] & S.CLOUD and "cloud" in reads.get(c, ()):
                kind = a.depth[0][5][1]
                if kind == "gray":
                    seen.add("cg")
                elif three and {"wg", "cg"} <= seen:
                    seen.add("cp")
        if {"wg", "cg", "wp", "cp"} <= seen:
            return True
    return False


def table_ownership(line):
    """a context is ctxs[0] of one batch of the new kinds and a later member of another of that kind; and a member list not sorted"""
    owned, later, unsorted_ = {}, False, False
    for i, st, before, after, reads in line:
        if st.kind in ("wls_batch", "reproject_batch", "pp_batch") and st.refused is None:
            later = later or any(c in owned.get(st.kind, ()) for c in st.ctx[1:])
            owned.setdefault(st.kind, set()).add(st.ctx[0])
            unsorted_ = unsorted_ or list(st.ctx) != sorted(st.ctx)
    return later and unsorted_


def batch_against_single_calls(line):
    """pp_batch on a context whose maps came from sgbm_select or upload_maps, read by download_maps and download_valid"""
    seen = set()
    for i, st, before, after, reads in line:
        if st.kind == "pp_batch" and st.refused is None:
            for c in st.ctx:
                root = before.ctxs[c].maps
                while root[0] in ("fill", "wm"):
                    root = root[1]
                if root[0] in ("sgmaps", "up") and "download_maps" in reads.get(c, ()):
                    seen.add("maps")
                    if "download_valid" in reads.get(c, ()):
                        seen.add("valid")
    return seen == {"maps", "valid"}


INTERLEAVINGS = (hook_over_a_published_result, stale_invalid_value, hook_invalid_follows_the_setting, rerun_after_release,
                 weight_table_reload, guide_follows_the_pair, staged_pair_not_adopted, gray_guide, table_ownership, batch_against_single_calls)


@pytest.mark.parametrize("pred", INTERLEAVINGS, ids=lambda f: f.__name__)
def test_interleavings(lines, tails, pred):
    hits = [w.seed for w, line in zip(tails, lines) if pred(line)]
    print(pred.__name__, hits)
    assert len(hits) >= 3, hits


def test_tail_models_have_void_and_dense_results_and_both_kinds_of_dropped_pixels(oracle, tails):
    """On the model, over the tail walks: a WLS result with void pixels and one without; a cloud that drops pixels by the z-range and
    one that drops them because s_3 == 0.  (Only results whose source is cheap to evaluate are looked at: the hook plane and
    uploaded maps.)"""
    import depth_model as DM
    seen = set()
    for w in tails:
        if {"void", "dense", "range", "s3"} <= seen:
            break
        R = S.Refs(S.Data(w.shape, w.seed), oracle, ("test", w.shape, w.seed))
        for i, st, world, want in S.replay(w):
            if st.kind != "read" or st.args["what"] not in ("wls_planes", "cloud"):
                continue
            e = want[0]
            src = e[1]
            cheap = src[1][0] in ("hook", "up") and (src[0] != "gif" or len(src) < 3 or src[2] is None or src[2][0] == "upmask")
            if st.args["what"] == "cloud":
                cheap = cheap and (e[2] is None or isinstance(e[2], int) or e[2][0] == "upmask")
            if not cheap:
                continue
            v = R(e)
            if st.args["what"] == "wls_planes":
                void = v["q"].view(np.uint32) == 0x7FC00000
                assert np.array_equal(void, v["disp"] == e[2])
                seen.add("void" if void.any() else "dense")
            else:
                void = v["xyz"].view(np.uint32)[..., 2] == DM.VOID_BITS
                if src[0] == "gif":
                    d, missing = DM.gif_disparity(R(src[1])[0], R(e[2])[0] if e[2] is not None else None)
                else:
                    d16 = R(src[1])["d16"]
                    d, missing = d16 * 0.0625, d16 == e[2]
                if (void & ~missing).any():
                    assert e[3] == 1 and (d[void & ~missing] == 0).all()
                    seen.add("s3")
                if len(v["cloud"]) < int((~void).sum()):
                    seen.add("range")
    assert {"void", "dense", "range", "s3"} <= seen, seen


def test_expressions_evaluate(oracle):
    """One walk of either shape and vocabulary through Refs: every value a reader compares exists, has the context's shape and comes
    out of the cache the second time."""
    import depth_model as DM
    for seed in S.TAIL_SEEDS[:2]:
        w = S.generate(seed, vocabulary="tail")
        R = S.Refs(S.Data(w.shape, seed), oracle, ("test", w.shape, seed))
        W, H, D = w.shape
        new = collections.Counter()
        for i, st, world, want in S.replay(w):
            if st.kind != "read" or st.args["what"] not in S.NEW_READERS:
                continue
            v = R(want[0])
            assert R(want[0]) is v
            new[st.args["what"]] += 1
            if st.args["what"] == "wls_planes":
                assert v["disp"].shape == (H, W) and v["disp"].dtype == np.int16 and v["tab"].shape == (256,)
                assert all(v[k].shape == (H, W) and v[k].dtype == np.float32 for k in ("q", "num", "den"))
            else:
                assert v["xyz"].shape == (H, W, 3) and v["z"].shape == (H, W) and v["cloud"].dtype == DM.POINT and len(v["cloud"]) <= W * H
        assert len(new) == 3, (seed, new)
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
