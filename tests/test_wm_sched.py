"""What the host driver of the plain weighted median decides without the device (primestereomatch_amd/csrc/psm_wm_sched.h: the
groups of sweeps and their form, when a map is finished, the weight cache, the layout of the sweep block), without a context or a
device: tests/wm_sched_probe.cpp plays the device to the schedule behind ctypes and is built here with the host compiler - the
header includes nothing of HIP.  The rules are stated here a second time, in Python, as psm_wgt_median had them in its body before
the header existed, for the two maps of a single pair (the header's one schedule and one cache decision with m = 2; more maps:
tests/test_wm_batch_sched.py); launches, snapshots and statistics must be equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "wm_sched_probe.cpp")
TWO_SWEEPS, NO_CACHE = 8388608, 16777216          # PSM_FLAG_WMF_TWO_SWEEPS, PSM_FLAG_WMF_NO_CACHE (include/primesm_hip.h)
CAP, LANE_MIN, WPIX = 96, 8192, 19 * 20
NCNT = 2 * (CAP + 2)                               # counters per map: cnt[2k] active, cnt[2k + 1] changed, cnt[2k + 2] the next list
GIB = 1 << 30


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("wm_sched") / "wm_sched_probe.so")
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.wm_probe_cache.restype = ctypes.c_ulonglong
    assert (lib.wm_probe_ncnt(), lib.wm_probe_cap(), lib.wm_probe_lane_min(), lib.wm_probe_wpix()) == (NCNT, CAP, LANE_MIN, WPIX)
    return lib


# ---- the rules, as the driver's loop had them ----
def model_run(table, flags):
    """table: [2][NCNT] counters as a whole call leaves them -> (launches [(sweep, short form)], snapshots [(slot, extent)],
    sweeps [2], evaluations [2])."""
    cap = 2 if flags & TWO_SWEEPS else 96
    done, tail, upto, pin = [False, False], [False, False], [0, 0], [None, None]
    sweeps, evals = [-1, -1], [0, 0]               # a map that is not finished: the dataflow form reports -1 and 0
    launches, snaps = [], []
    sw = 0

    def launch_group(slot):
        nonlocal sw
        short = (tail[0] or done[0]) and (tail[1] or done[1])
        end = min(sw + (8 if short else 2), cap)
        launches.extend((k, int(short)) for k in range(sw, end))
        sw = end
        # what the device has written when the snapshot behind sweep sw - 1 is taken: cnt[0 .. 2 sw]
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
        for s in range(2):
            if done[s]:
                continue
            ev = 0
            for k in range(seen):
                ev += h[s][2 * k]
                if h[s][2 * k + 1] == 0:
                    done[s], sweeps[s], evals[s] = True, k + 1, ev
                    break
            tail[s] = seen < cap and h[s][2 * seen] < LANE_MIN
        if (done[0] and done[1]) or not more:
            break
        g += 1
    return launches, snaps, sweeps, evals


def model_cache(n0, avail, flags):
    """-> (floats of the cache or 0, first float of the right side)."""
    limit = min(12 * GIB, avail // 2)
    need = [(n + 63) // 64 * 64 * WPIX for n in n0]
    tot = 0 if n0[0] < LANE_MIN and n0[1] < LANE_MIN else need[0] + need[1]
    return (tot if tot and tot * 4 <= limit and not flags & NO_CACHE else 0), need[0]


def model_layout(HW):
    """-> ({name: (offset, bytes)} of every part of the block, bytes to allocate)."""
    nb = (HW + 255) // 256 * 256
    per_side = 4 * nb + 6 * nb * 4
    parts = {}
    for s in range(2):
        b = s * per_side
        ip = b + 4 * nb
        for i, name in enumerate(("orig", "newv", "chgb", "rowany")):
            parts[name, s] = (b + i * nb, nb)
        for i, name in enumerate(("stamp", "list0", "list1", "chg", "slot_of", "inv")):
            parts[name, s] = (ip + i * nb * 4, nb * 4)
    return parts, 2 * per_side


# ---- the header through the probe ----
def probe_run(probe, table, flags):
    t = np.ascontiguousarray(table, dtype=np.int32)
    assert t.shape == (2, NCNT)
    room = CAP + 8
    groups, snaps = (ctypes.c_int * (3 * room))(), (ctypes.c_int * (2 * room))()
    ns, sweeps, evals = ctypes.c_int(), (ctypes.c_int * 2)(), (ctypes.c_longlong * 2)()
    done, tail = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    ng = probe.wm_probe_run(t.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 2, ctypes.c_uint(flags), groups, room, snaps, ctypes.byref(ns),
                            done, tail, sweeps, evals)
    assert ng <= room and ns.value <= room
    assert [bool(d) for d in done] == [s > 0 for s in sweeps]
    # (the probe reports groups {begin, end, form}: every sweep of a group is launched in the group's form)
    launches = [(k, groups[3 * i + 2]) for i in range(ng) for k in range(groups[3 * i], groups[3 * i + 1])]
    return launches, [(snaps[2 * i], snaps[2 * i + 1]) for i in range(ns.value)], list(sweeps), list(evals)


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
    want = model_run([list(map(int, t)) for t in table], flags)
    got = probe_run(probe, table, flags)
    assert got == want
    return got


def test_both_maps_empty(probe):
    launches, snaps, sweeps, evals = both(probe, [EMPTY, EMPTY])
    assert launches == [(0, 0), (1, 0), (2, 0), (3, 0)]      # the second group was queued before the first was looked at
    assert snaps == [(0, 2)] and sweeps == [1, 1] and evals == [0, 0]


@pytest.mark.parametrize("side", [0, 1])
def test_one_map_empty_beside_eleven_sweeps(probe, side):
    act = [20000, 15000, 12000, 9000, 5000, 3000, 900, 300, 60, 12, 3]
    busy = counters(act, [a // 2 + 1 for a in act[:10]] + [0])
    table = [EMPTY, EMPTY]
    table[side] = busy
    launches, snaps, sweeps, evals = both(probe, table)
    assert sweeps[side] == 11 and evals[side] == sum(act) and sweeps[1 - side] == 1 and evals[1 - side] == 0
    # the list going into sweep 4 is the first short one; the snapshot that shows it is behind sweep 3, read with sweeps 4 and 5 queued
    assert [k for k, short in launches if short] == list(range(6, 22))
    assert snaps[-1] == (1, 14)                               # the fixed point is seen in the group that holds sweep 10


def test_short_lists_change_the_form_two_groups_later(probe):
    act = [30000, 20000, 10000] + [5000 - 50 * k for k in range(40)]
    t = counters(act, [a // 3 + 1 for a in act[:30]] + [0])
    launches, snaps, sweeps, evals = both(probe, [t, t])
    assert t[2 * 3] < LANE_MIN <= t[2 * 2]                    # short after the third sweep
    assert launches[:8] == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 1), (7, 1)]
    assert [e for _, e in snaps[:4]] == [2, 4, 6, 14]         # groups of two, then of eight
    assert sweeps == [31, 31] and evals == [sum(act[:31])] * 2


def test_a_map_that_never_stops_falls_back(probe):
    never = counters([9000], [1])
    launches, snaps, sweeps, evals = both(probe, [never, EMPTY])
    assert [k for k, _ in launches] == list(range(96)) and snaps[-1][1] == 96
    assert sweeps == [-1, 1] and evals == [0, 0]
    launches, _, sweeps, _ = both(probe, [never, never])
    assert len(launches) == 96 and sweeps == [-1, -1]
    assert not any(short for _, short in launches)            # 9000 pixels: never the wave form


def test_cap_of_two(probe):
    inside = counters([500, 20], [7, 0])
    beyond = counters([500, 20, 3], [7, 2, 0])
    launches, snaps, sweeps, evals = both(probe, [inside, beyond], TWO_SWEEPS)
    assert launches == [(0, 0), (1, 0)] and snaps == [(0, 2)]
    assert sweeps == [2, -1] and evals == [520, 0]
    assert both(probe, [beyond, inside], 0)[2] == [3, 2]      # (without the flag both finish)
    assert both(probe, [EMPTY, EMPTY], TWO_SWEEPS)[0] == [(0, 0), (1, 0)]


def random_table(rng):
    """Active counts that fall, a first zero change at a random sweep or none."""
    table = []
    for _ in range(2):
        start = int(rng.choice([0, 5, 300, 8191, 8192, 8193, 40000, 2000000]))
        decay = rng.uniform(0.3, 1.0)
        stop = int(rng.integers(0, CAP + 4)) if rng.random() < 0.8 else None
        act, chg, a = [], [], start
        for k in range(CAP + 1):
            act.append(a)
            chg.append(0 if k == stop else int(rng.integers(1, a + 1)) if a else 0)
            a = int(a * decay) if rng.random() < 0.9 else a
        table.append(counters(act, chg))
    return table


def test_random_tables(probe):
    rng = np.random.default_rng(20260)
    forms, fall_backs = set(), 0
    for i in range(2500):
        table = random_table(rng)
        flags = TWO_SWEEPS if i % 10 == 9 else 0
        launches, snaps, sweeps, evals = both(probe, table, flags)
        forms |= {short for _, short in launches}
        fall_backs += sweeps.count(-1)
        for s in range(2):
            if sweeps[s] > 0:
                assert table[s][2 * sweeps[s] - 1] == 0 and all(table[s][2 * k + 1] for k in range(sweeps[s] - 1))
                assert evals[s] == sum(table[s][0:2 * sweeps[s]:2])
    assert forms == {0, 1} and fall_backs > 50                # (the tables reach every branch)


def cache(probe, n0, avail, flags=0):
    need = (ctypes.c_ulonglong * 2)()
    floats = probe.wm_probe_cache((ctypes.c_int * 2)(*n0), 2, ctypes.c_ulonglong(avail), ctypes.c_uint(flags), need)
    assert floats in (0, need[0] + need[1])
    assert (floats, need[0]) == model_cache(n0, avail, flags), (n0, avail, flags)      # (the right side begins behind the left side's need)
    return floats, need[0]


def test_cache_decision(probe):
    big = 1 << 60
    # no cache while both lists are short; from LANE_MIN on either side both maps are cached
    assert cache(probe, (LANE_MIN - 1, LANE_MIN - 1), big)[0] == 0
    assert cache(probe, (LANE_MIN, 0), big) == (LANE_MIN * WPIX, LANE_MIN * WPIX)
    assert cache(probe, (0, LANE_MIN), big) == (LANE_MIN * WPIX, 0)
    assert cache(probe, (LANE_MIN - 1, LANE_MIN), big)[0] == 2 * LANE_MIN * WPIX
    # whole blocks of 64 pixels per side; the right side begins behind the left side's blocks
    assert cache(probe, (10000, 1), big) == ((10048 + 64) * WPIX, 10048 * WPIX)
    assert cache(probe, (10048, 64), big) == ((10048 + 64) * WPIX, 10048 * WPIX)
    assert cache(probe, (10049, 65), big) == ((10112 + 128) * WPIX, 10112 * WPIX)
    # the flag
    assert cache(probe, (10000, 10000), big, NO_CACHE)[0] == 0 and cache(probe, (10000, 10000), big, TWO_SWEEPS)[0] > 0
    # half of what is available, on either side of equality
    tot = 2 * 10048 * WPIX
    assert cache(probe, (10000, 10000), 8 * tot)[0] == tot
    assert cache(probe, (10000, 10000), 8 * tot + 1)[0] == tot
    assert cache(probe, (10000, 10000), 8 * tot - 1)[0] == 0
    assert cache(probe, (10000, 10000), 0)[0] == 0
    # 12 GiB: a block of 64 pixels is 97 280 bytes, which does not divide it - the last block count that fits, and the next
    blocks = 12 * GIB // (64 * WPIX * 4)
    fits, over = blocks * 64, (blocks + 1) * 64
    assert fits * WPIX * 4 <= 12 * GIB < over * WPIX * 4
    for n0 in ((fits, 0), (0, fits), (blocks // 2 * 64, (blocks - blocks // 2) * 64)):
        assert cache(probe, n0, big)[0] == fits * WPIX
    for n0 in ((over, 0), (0, over), (fits, 1), (fits - 63, 65)):
        assert cache(probe, n0, big)[0] == 0
    assert cache(probe, (fits, 0), 24 * GIB)[0] == fits * WPIX and cache(probe, (fits, 0), 2 * fits * WPIX * 4 - 2)[0] == 0
    rng = np.random.default_rng(5)
    for _ in range(3000):
        n0 = tuple(int(v) for v in rng.choice([0, 63, 64, LANE_MIN - 1, LANE_MIN, 100000, 3000000, 6000000], 2) + rng.integers(0, 3, 2))
        cache(probe, n0, int(rng.integers(0, 40 * GIB)), int(rng.choice([0, NO_CACHE])))


@pytest.mark.parametrize("W,H", [(9, 9), (111, 233), (1920, 1080)])
def test_block_layout(probe, W, H):
    HW = W * H
    out = (ctypes.c_ulonglong * 21)()
    probe.wm_probe_layout(ctypes.c_ulonglong(HW), out)
    names = ("orig", "newv", "chgb", "rowany", "stamp", "list0", "list1", "chg", "slot_of", "inv")
    parts, nbytes = model_layout(HW)
    got = {(n, s): out[10 * s + i] for s in range(2) for i, n in enumerate(names)}
    assert got == {k: off for k, (off, _) in parts.items()}
    assert out[20] == nbytes
    # every part inside the allocation, none overlapping another; ints on int boundaries, every part on a 256-byte one (the seed
    # writes 16 bytes per lane); the counters are no longer in the block (they lie with the call's first context)
    spans = sorted((got[k], got[k] + parts[k][1], k) for k in parts)
    assert spans[0][0] == 0 and spans[-1][1] == nbytes
    for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
        assert a1 <= b0, (ka, kb)
    for (n, s), off in got.items():
        assert parts[n, s][1] >= (HW if n in names[:4] else HW * 4)
        assert n in names[:4] or off % 4 == 0
        assert off % 256 == 0


def test_probe_as_a_program_under_sanitizers(tmp_path):
    """The same probe source as a program of its own (its main walks seeded random tables through the schedule, the cache decision
    and the layout), built with the address and undefined-behaviour sanitizers: it must report nothing."""
    exe = str(tmp_path / "wm_sched_probe")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DWM_SCHED_PROBE_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "3000"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.startswith("3000 tables")
