"""What the host driver of the weighted median decides without the device for the maps of several pairs (psm_post_process_batch;
WmSched, wm_cache_plan in primestereomatch_amd/csrc/psm_wm_sched.h): the groups of sweeps of m = 2 n maps and their form, when a
map is finished, which maps are left to the dataflow form, and the call-wide cache decision.  tests/wm_sched_probe.cpp plays the
device to the schedule behind ctypes and is built here with the host compiler.  The rules are stated here a second time, in
Python.  A single pair is the same schedule with m = 2: tests/test_wm_sched.py holds it against the single call's model."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "wm_sched_probe.cpp")
TWO_SWEEPS, NO_CACHE = 8388608, 16777216          # PSM_FLAG_WMF_TWO_SWEEPS, PSM_FLAG_WMF_NO_CACHE (include/primesm_hip.h)
CAP, LANE_MIN, WPIX = 96, 8192, 19 * 20
NCNT = 2 * (CAP + 2)
GIB = 1 << 30
SIZES = (2, 4, 6, 16)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("wm_batch_sched") / "wm_sched_probe.so")
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.wm_probe_cache.restype = ctypes.c_ulonglong
    assert (lib.wm_probe_ncnt(), lib.wm_probe_cap(), lib.wm_probe_lane_min(), lib.wm_probe_wpix()) == (NCNT, CAP, LANE_MIN, WPIX)
    return lib


# ---- the rules ----
def model_run(table, flags):
    """table: [m][NCNT] counters as a whole call leaves them -> (groups [(begin, end, short form)], snapshots [(slot, extent)],
    done [m], tail [m], sweeps [m], evaluations [m])."""
    m = len(table)
    cap = 2 if flags & TWO_SWEEPS else 96
    done, tail, upto, pin = [0] * m, [0] * m, [0, 0], [None, None]
    sweeps, evals = [-1] * m, [0] * m              # a map that is not finished: the dataflow form reports -1 and 0
    groups, snaps = [], []
    sw = 0

    def launch_group(slot):
        nonlocal sw
        short = all(tail[s] or done[s] for s in range(m))          # the one-launch wave form only when EVERY map is short or finished
        end = min(sw + (8 if short else 2), cap)
        groups.append((sw, end, int(short)))
        sw = end
        pin[slot] = [list(t[:2 * sw + 1]) + [0] * (NCNT - 2 * sw - 1) for t in table]
        upto[slot] = sw

    launch_group(0)
    g = 0
    while True:
        more = sw < cap
        if more:
            launch_group((g + 1) & 1)              # queued before this group's counters are looked at
        h, seen = pin[g & 1], upto[g & 1]
        snaps.append((g & 1, seen))
        for s in range(m):
            if done[s]:
                continue
            ev = 0
            for k in range(seen):
                ev += h[s][2 * k]
                if h[s][2 * k + 1] == 0:           # the first sweep that changed nothing: the fixed point
                    done[s], sweeps[s], evals[s] = 1, k + 1, ev
                    break
            tail[s] = int(seen < cap and h[s][2 * seen] < LANE_MIN)
        if all(done) or not more:                  # every map done, or the cap reached
            break
        g += 1
    return groups, snaps, done, tail, sweeps, evals


def model_cache(n0, avail, flags):
    """-> floats of all sides' weights, 0: no cache.  One decision for the batch."""
    limit = min(12 * GIB, avail // 2)
    tot = sum((n + 63) // 64 * 64 * WPIX for n in n0)
    if not any(n >= LANE_MIN for n in n0) or tot * 4 > limit or flags & NO_CACHE:
        return 0
    return tot


# ---- the header through the probe ----
def probe_run(probe, table, flags):
    t = np.ascontiguousarray(table, dtype=np.int32)
    m = t.shape[0]
    assert t.shape == (m, NCNT)
    room = CAP + 8
    groups, snaps = (ctypes.c_int * (3 * room))(), (ctypes.c_int * (2 * room))()
    ns = ctypes.c_int()
    done, tail, sweeps, evals = (ctypes.c_int * m)(), (ctypes.c_int * m)(), (ctypes.c_int * m)(), (ctypes.c_longlong * m)()
    tp = t.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    ng = probe.wm_probe_run(tp, m, ctypes.c_uint(flags), groups, room, snaps, ctypes.byref(ns), done, tail, sweeps, evals)
    assert ng <= room and ns.value <= room
    return ([(groups[3 * i], groups[3 * i + 1], groups[3 * i + 2]) for i in range(ng)],
            [(snaps[2 * i], snaps[2 * i + 1]) for i in range(ns.value)], list(done), list(tail), list(sweeps), list(evals))


def counters(active, changed):
    """One map's counters of a call whose sweep k evaluates active[k] pixels and changes changed[k] of them; a sweep that changes
    nothing leaves empty lists behind it (as does a list that is empty)."""
    t = [0] * NCNT
    live = True
    for k in range(CAP + 1):
        a = active[min(k, len(active) - 1)] if live else 0
        t[2 * k] = a
        if k == CAP:
            break
        c = min(changed[min(k, len(changed) - 1)], a) if live else 0
        t[2 * k + 1] = c
        live = live and c > 0
    return t


EMPTY = counters([0], [0])


def both(probe, table, flags=0):
    """The model and the schedule: every group (begin, end, form), every snapshot, done, tail, sweeps and evals equal."""
    want = model_run([list(map(int, t)) for t in table], flags)
    got = probe_run(probe, table, flags)
    assert got == want
    return got


@pytest.mark.parametrize("m", SIZES)
def test_all_maps_empty(probe, m):
    groups, snaps, done, tail, sweeps, evals = both(probe, [EMPTY] * m)
    assert groups == [(0, 2, 0), (2, 4, 0)]                   # the second group was queued before the first was looked at
    assert snaps == [(0, 2)] and sweeps == [1] * m and evals == [0] * m and done == [1] * m


@pytest.mark.parametrize("m", SIZES)
def test_one_map_of_eleven_sweeps_beside_empty_ones(probe, m):
    act = [20000, 15000, 12000, 9000, 5000, 3000, 900, 300, 60, 12, 3]
    busy = counters(act, [a // 2 + 1 for a in act[:10]] + [0])
    for at in (0, m - 1):
        table = [EMPTY] * m
        table[at] = busy
        groups, snaps, done, tail, sweeps, evals = both(probe, table)
        assert sweeps[at] == 11 and evals[at] == sum(act)
        assert all(sweeps[s] == 1 and evals[s] == 0 for s in range(m) if s != at)
        # the list going into sweep 4 is the first short one; the snapshot that shows it is behind sweep 3, read with sweeps 4 and 5 queued
        assert [g for g in groups if g[2]] == [(6, 14, 1), (14, 22, 1)]
        assert snaps[-1] == (1, 14)                           # the fixed point is seen in the group that holds sweep 10


@pytest.mark.parametrize("m", SIZES)
def test_the_form_changes_two_groups_late_and_only_for_all_maps(probe, m):
    act = [30000, 20000, 10000] + [5000 - 50 * k for k in range(40)]
    t = counters(act, [a // 3 + 1 for a in act[:30]] + [0])
    groups, snaps, done, tail, sweeps, evals = both(probe, [t] * m)
    assert t[2 * 3] < LANE_MIN <= t[2 * 2]                    # short after the third sweep
    assert groups[:4] == [(0, 2, 0), (2, 4, 0), (4, 6, 0), (6, 14, 1)]
    assert [e for _, e in snaps[:4]] == [2, 4, 6, 14]
    assert sweeps == [31] * m and evals == [sum(act[:31])] * m
    # one map whose lists stay long keeps every group in the long form, for all maps
    long_act = [30000] * 12
    stays = counters(long_act, [100] * 11 + [0])
    groups, _, _, _, sweeps, _ = both(probe, [t] * (m - 1) + [stays])
    assert sweeps[-1] == 12 and sweeps[0] == 31
    assert all(not short for b, e, short in groups if b < 12)


@pytest.mark.parametrize("m", SIZES)
def test_one_map_never_stops_the_others_finish_at_sweep_three(probe, m):
    never = counters([9000], [1])
    three = counters([700, 90, 4], [60, 3, 0])
    for at in (0, m // 2, m - 1):
        table = [three] * m
        table[at] = never
        groups, snaps, done, tail, sweeps, evals = both(probe, table)
        assert groups[-1][1] == 96 and snaps[-1][1] == 96 and sum(e - b for b, e, _ in groups) == 96
        assert not any(short for _, _, short in groups)        # 9000 pixels: never the wave form
        assert [s for s in range(m) if not done[s]] == [at]    # only that map is left for the dataflow form
        assert sweeps[at] == -1 and evals[at] == 0
        assert all(sweeps[s] == 3 and evals[s] == 794 for s in range(m) if s != at)


@pytest.mark.parametrize("m", SIZES)
def test_cap_of_two(probe, m):
    inside = counters([500, 20], [7, 0])
    beyond = counters([500, 20, 3], [7, 2, 0])
    table = [inside if s % 2 == 0 else beyond for s in range(m)]
    groups, snaps, done, tail, sweeps, evals = both(probe, table, TWO_SWEEPS)
    assert groups == [(0, 2, 0)] and snaps == [(0, 2)]
    assert sweeps == [2 if s % 2 == 0 else -1 for s in range(m)] and evals == [520 if s % 2 == 0 else 0 for s in range(m)]
    assert both(probe, table, 0)[4] == [2 if s % 2 == 0 else 3 for s in range(m)]      # (without the flag all finish)
    assert both(probe, [EMPTY] * m, TWO_SWEEPS)[0] == [(0, 2, 0)]


def random_map(rng):
    """Active counts that fall, a first zero change at a random sweep or none."""
    start = int(rng.choice([0, 5, 300, 8191, 8192, 8193, 40000, 2000000]))
    decay = rng.uniform(0.3, 1.0)
    stop = int(rng.integers(0, CAP + 4)) if rng.random() < 0.8 else None
    act, chg, a = [], [], start
    for k in range(CAP + 1):
        act.append(a)
        chg.append(0 if k == stop else int(rng.integers(1, a + 1)) if a else 0)
        a = int(a * decay) if rng.random() < 0.9 else a
    return counters(act, chg)


@pytest.mark.parametrize("m", SIZES)
def test_random_tables(probe, m):
    rng = np.random.default_rng(20261 + m)
    forms, fall_backs = set(), 0
    for i in range(200):
        table = [random_map(rng) for _ in range(m)]
        flags = TWO_SWEEPS if i % 10 == 9 else 0
        groups, snaps, done, tail, sweeps, evals = both(probe, table, flags)
        forms |= {short for _, _, short in groups}
        fall_backs += sweeps.count(-1)
        for s in range(m):
            assert (sweeps[s] > 0) == bool(done[s])
            if sweeps[s] > 0:
                assert table[s][2 * sweeps[s] - 1] == 0 and all(table[s][2 * k + 1] for k in range(sweeps[s] - 1))
                assert evals[s] == sum(table[s][0:2 * sweeps[s]:2])
    assert forms == {0, 1} and fall_backs > 5                  # (the tables reach every branch)


def cache(probe, n0, avail, flags=0):
    m = len(n0)
    need = (ctypes.c_ulonglong * m)()
    got = probe.wm_probe_cache((ctypes.c_int * m)(*n0), m, ctypes.c_ulonglong(avail), ctypes.c_uint(flags), need)
    assert got == model_cache(n0, avail, flags), (n0, avail, flags)
    assert list(need) == [(n + 63) // 64 * 64 * WPIX for n in n0]
    return got


@pytest.mark.parametrize("m", SIZES)
def test_cache_decision_at_the_seams(probe, m):
    big = 1 << 60
    # a side at 8191 / 8192 invalid pixels: no cache while every list is short, and with one side at LANE_MIN ALL sides get theirs
    assert cache(probe, [LANE_MIN - 1] * m, big) == 0
    for at in (0, m - 1):
        n0 = [LANE_MIN - 1] * m
        n0[at] = LANE_MIN
        assert cache(probe, n0, big) == m * LANE_MIN * WPIX
        n0 = [0] * m
        n0[at] = LANE_MIN
        assert cache(probe, n0, big) == LANE_MIN * WPIX
    # the flag
    assert cache(probe, [10000] * m, big, NO_CACHE) == 0 and cache(probe, [10000] * m, big, TWO_SWEEPS) == m * 10048 * WPIX
    # half of what is available, on either side of equality
    tot = m * 10048 * WPIX
    assert cache(probe, [10000] * m, 8 * tot) == tot
    assert cache(probe, [10000] * m, 8 * tot - 1) == 0
    assert cache(probe, [10000] * m, 0) == 0
    # 12 GiB: the last total block count that fits, and one block over - wherever the block is added
    blocks = 12 * GIB // (64 * WPIX * 4)
    share = [blocks // m + (1 if s < blocks % m else 0) for s in range(m)]
    assert sum(share) == blocks and min(share) * 64 >= LANE_MIN
    assert cache(probe, [b * 64 for b in share], big) == blocks * 64 * WPIX
    for at in (0, m - 1):
        over = [b * 64 for b in share]
        over[at] += 1                                          # (one pixel more: one block of 64 more)
        assert cache(probe, over, big) == 0
        assert cache(probe, over, big, NO_CACHE) == 0
    rng = np.random.default_rng(5 + m)
    for _ in range(1000):
        n0 = [int(v) for v in rng.choice([0, 63, 64, LANE_MIN - 1, LANE_MIN, 100000, 1500000], m) + rng.integers(0, 3, m)]
        cache(probe, n0, int(rng.integers(0, 40 * GIB)), int(rng.choice([0, NO_CACHE])))


def test_probe_as_a_program_under_sanitizers(tmp_path):
    """The same probe source as a program of its own (its main walks seeded random tables of 2, 4, 6 and 16 maps through the
    schedule, the cache decision and the layout), built with the address and undefined-behaviour sanitizers: it must report nothing."""
    exe = str(tmp_path / "wm_sched_probe")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DWM_SCHED_PROBE_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "1500"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.startswith("1500 tables")
