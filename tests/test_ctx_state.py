"""The records a context keeps between calls of the C ABI (primestereomatch_amd/csrc/psm_state.h: what stands for a volume side,
what the current results are, which image pair is current and which is on its way) walked without a context or a device:
tests/ctx_state_probe.cpp puts their transitions behind ctypes and is built here with the host compiler - the header includes nothing
of HIP.  The same file with its own main is also built as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer and run."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NOTHING, KEYS, FGF = 0, 1, 2
# the five states of a side: (lazy, pending, subsample rate)
RECIPE, REAL, RECIPE_KEYS, REAL_KEYS, MODELS = (1, NOTHING, 0), (0, NOTHING, 0), (1, KEYS, 0), (0, KEYS, 0), (0, FGF, 4)
FIVE = [RECIPE, REAL, RECIPE_KEYS, REAL_KEYS, MODELS]
NEW_COSTS, COSTS_BUILT, TO_KEYS, TO_FGF, TO_MEMORY, ASK = range(6)
STALE, FILTERED, COVER, MAPS_WRITTEN, MASK_WRITTEN, TAKE_EARLY, FORGET_EARLY, MAPS_GONE, KEYS_COMPLETE, KEYS_GONE, NEW = range(11)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ctx_state") / "ctx_state_probe.so")
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", os.path.join(HERE, "ctx_state_probe.cpp"), "-o", so],
                   check=True)
    return ctypes.CDLL(so)


def side(probe, state, op, arg=0):
    st = (ctypes.c_int * 3)(*state)
    return tuple(st), probe.side_step(st, op, arg), tuple(st)


def res(probe, st, op, a=0, b=0, e=0):
    buf = (ctypes.c_int * 7)(*st)
    ret = probe.res_step(buf, op, a, b, e)
    return list(buf), ret


def test_side_transitions_stay_inside_the_table(probe):
    # what each move makes of each state: new costs replace everything; built costs keep what is pending; keys keep whatever the
    # costs were and replace models; models and memory leave no recipe and nothing else pending
    want = {
        (NEW_COSTS, 1): lambda s: RECIPE,
        (NEW_COSTS, 0): lambda s: REAL,
        (COSTS_BUILT, 0): lambda s: (0, s[1], s[2]),
        (TO_KEYS, 0): lambda s: (s[0], KEYS, 0),
        (TO_FGF, 2): lambda s: (0, FGF, 2),
        (TO_FGF, 8): lambda s: (0, FGF, 8),
        (TO_MEMORY, 0): lambda s: REAL,
    }
    for state, ((op, arg), f) in itertools.product(FIVE, want.items()):
        _, q, got = side(probe, state, op, arg)
        assert got == f(state), (state, op, arg)
        assert (got[0], got[1], 4 if got[1] == FGF else got[2]) in FIVE, (state, op, arg)     # no sixth state
        lazy, keys, fgf, real, fresh = (bool(q >> i & 1) for i in range(5))
        assert not (keys and fgf)                                  # keys and models are never pending together
        assert (lazy, keys, fgf) == (bool(got[0]), got[1] == KEYS, got[1] == FGF) and q >> 5 & 1
        assert real == (got == REAL) and fresh == (got == RECIPE)
        assert not (fgf and lazy)                                  # models stand for the volume: nothing of it is a recipe
    assert side(probe, (0, NOTHING, 0), ASK)[2] == REAL            # (what VolSide{} and a new image pair give)


def test_results_mask_rows_and_early_map(probe):
    H = 60
    new, _ = res(probe, [0] * 7, NEW)
    assert new == [0, 0, 0, 0, 0, 0, 0]
    # a mask never outlives its maps, whatever happens in whatever order
    rng = np.random.default_rng(3)
    st = new
    for _ in range(4000):
        op = int(rng.integers(0, 10))
        y0 = int(rng.integers(0, H)); y1 = int(rng.integers(y0 + 1, H + 1))
        before = st
        st, ret = res(probe, st, op, y0 if op != KEYS_COMPLETE else int(rng.integers(0, 2)), y1, int(rng.integers(0, 3)))
        assert not (st[1] and not st[0]), (op, st)
        if op == MAPS_WRITTEN:
            assert st[:2] == [1, 0]                                # new maps: the old mask does not describe them
        if op in (STALE, FILTERED, MAPS_GONE):
            assert st[:2] == [0, 0]
        if op == MASK_WRITTEN:
            assert st[1] == before[0]
        if op in (STALE, FORGET_EARLY, TAKE_EARLY):
            assert st[6] == 0
        if op not in (FILTERED, COVER):
            assert st[4:6] == before[4:6]                          # only a filter and `cover` say which rows
        if op not in (KEYS_COMPLETE, KEYS_GONE):
            assert st[2:4] == before[2:4]
    # maps written for the whole image after a stripe
    st, _ = res(probe, new, FILTERED, 20, 40, 1)
    assert st[4:6] == [20, 40] and not probe.rows_whole(H, *st[4:6])
    st, _ = res(probe, st, COVER, 0, H)
    st, _ = res(probe, st, MAPS_WRITTEN)
    assert st[:2] == [1, 0] and st[4:6] == [0, H] and probe.rows_whole(H, *st[4:6])
    # the early map: recorded by the filter call whose reduction filled it, taken once, and only for that buffer
    st, _ = res(probe, new, FILTERED, 0, H, 1)
    assert st[6] == 1
    st, hit = res(probe, st, TAKE_EARLY, e=1)
    assert hit == 1 and st[6] == 0
    assert res(probe, st, TAKE_EARLY, e=1)[1] == 0                 # once
    st, _ = res(probe, new, FILTERED, 0, H, 1)
    assert res(probe, st, TAKE_EARLY, e=2) == (st[:6] + [0], 0)    # another buffer: no hit, and forgotten
    for op, args in ((STALE, ()), (FILTERED, (0, H, 0)), (FORGET_EARLY, ())):      # a later filter without one, new costs, an upload
        assert res(probe, st, op, *args)[0][6] == 0
    for op in (MAPS_WRITTEN, MASK_WRITTEN, COVER, KEYS_COMPLETE, KEYS_GONE, MAPS_GONE):
        assert res(probe, st, op, 0, H)[0][6] == 1                 # (nothing else touches it)
    # keys: per side, gone together
    st, _ = res(probe, new, KEYS_COMPLETE, 1)
    assert st[2:4] == [0, 1]
    st, _ = res(probe, st, KEYS_COMPLETE, 0)
    assert st[2:4] == [1, 1] and res(probe, st, KEYS_GONE)[0][2:4] == [0, 0]


def test_pending_minima_keep_their_rows_across_foreign_maps(probe):
    """Maps written by someone else than the select (psm_upload_maps, psm_gather_rows_ctx, the SGM stage) cover the whole image; the
    minima a striped filter left pending still cover the stripe, and so do the maps a later select makes of them."""
    H = 60
    for stripe in ((20, 40), (0, 7), (0, H)):
        y = (ctypes.c_int * 4)()
        probe.rows_across_foreign_maps(*stripe, 0, H, y)
        assert tuple(y) == (0, H, *stripe)
        assert probe.rows_whole(H, y[2], y[3]) == (stripe == (0, H))


# ---- the image pair and the staged one (psm::PairState): st = (depth, next depth, slot, range pending, inside) ----
UPLOADED, STAGED, ADOPTED, NEXT_SLOT, RANGE_ARRIVED, NEW_PAIR, ASK_PAIR = range(7)
NONE, U8, F32 = -1, 0, 1


def pair(probe, st, op, a=0, b=0):
    buf = (ctypes.c_int * 5)(*st)
    ret = probe.pair_step(buf, op, a, b)
    return tuple(buf), ret


def reachable_pairs(probe):
    fresh, _ = pair(probe, (0,) * 5, NEW_PAIR)
    moves = [(UPLOADED, d, i) for d in (U8, F32) for i in (0, 1)] + [(STAGED, U8, 0), (STAGED, F32, 1)] + \
            [(ADOPTED, i, 0) for i in (0, 1)] + [(NEXT_SLOT, 0, 0), (RANGE_ARRIVED, 0, 0)]
    seen, todo = {fresh}, [fresh]
    while todo:
        st = todo.pop()
        for m in moves:
            nxt, _ = pair(probe, st, *m)
            if nxt not in seen:
                seen.add(nxt)
                todo.append(nxt)
    return fresh, sorted(seen)


def test_pair_transitions_from_every_reachable_state(probe):
    fresh, states = reachable_pairs(probe)
    assert fresh == (NONE, NONE, 0, 0, 1)
    assert len(states) > 20 and all(s[2] in (0, 1) for s in states)
    for st in states:
        staged_before = st[1] >= 0
        assert pair(probe, st, ASK_PAIR) == (st, int(staged_before) | ((st[1] if staged_before else st[0]) + 1) << 1)
        # a blocking upload leaves no staged pair and no pending range
        for depth, inside in itertools.product((U8, F32), (0, 1)):
            got, q = pair(probe, st, UPLOADED, depth, inside)
            assert got == (depth, NONE, st[2], 0, inside) and q == (depth + 1) << 1
        # staging twice without adopting keeps the second pair's depth and its pending mark only
        for (d1, p1), (d2, p2) in itertools.product(((U8, 0), (F32, 1)), repeat=2):
            once, _ = pair(probe, st, STAGED, d1, p1)
            twice, q = pair(probe, once, STAGED, d2, p2)
            assert twice == (st[0], d2, st[2], p2, st[4]) and q == 1 | (d2 + 1) << 1
            # ... which the adoption makes current, with the answer it is given
            for inside in (0, 1):
                assert pair(probe, twice, ADOPTED, inside)[0] == (d2, NONE, st[2], 0, inside)
        # adopt with nothing staged changes nothing
        if not staged_before:
            for inside in (0, 1):
                assert pair(probe, st, ADOPTED, inside)[0] == st
        # a staged pair given up (the next one is about to overwrite its slot) leaves none; the range arriving changes the pending
        # mark alone; the slot flips and nothing else moves
        assert pair(probe, st, STAGED, NONE, 0)[0] == (st[0], NONE, st[2], 0, st[4])
        assert pair(probe, st, RANGE_ARRIVED)[0] == st[:3] + (0,) + st[4:]
        assert pair(probe, st, NEXT_SLOT) == (st[:2] + (st[2] ^ 1,) + st[3:], st[2] ^ 1)


def test_pair_slot_alternates_from_a_fresh_record(probe):
    st, _ = pair(probe, (0,) * 5, NEW_PAIR)
    slots = []
    for _ in range(6):
        st, slot = pair(probe, st, NEXT_SLOT)
        slots.append(slot)
    assert slots == [1, 0, 1, 0, 1, 0]                             # as `stage_slot ^= 1` gave them


def test_depth_at_the_next_construct_is_the_batch_rule(probe):
    """psm_compute_batch compared its members' depths with a nested conditional over the staged and the current depth of the member
    and of context 0; the accessor answers the same on all 3 x 3 combinations of (none, 8-bit, float), for both contexts."""
    def at_construct(depth, nxt):
        return (pair(probe, (depth, nxt, 0, 0, 1), ASK_PAIR)[1] >> 1) - 1

    depths = (NONE, U8, F32)
    for raw, nxt, raw0, nxt0 in itertools.product(depths, repeat=4):
        ref0 = nxt0 if nxt0 >= 0 else raw0
        refused = (nxt != ref0) if nxt >= 0 else (raw != ref0)     # the conditional as it stood
        assert (at_construct(raw, nxt) != at_construct(raw0, nxt0)) == refused, (raw, nxt, raw0, nxt0)


def test_probe_runs_clean_under_sanitizers(tmp_path):
    """The probe as a stand-alone program with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer: it walks
    the records' transitions natively and must report nothing."""
    exe = str(tmp_path / "ctx_state_probe_san")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-DPROBE_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "ctx_state_probe.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    assert run.stdout.startswith("60000 steps, rows 0 60 20 40, whole 1")

