"""CPU: the liveness predicate of the select forms (primestereomatch_amd/csrc/psm_live.h) against the oracle's filtered volumes,
and the planner's count of live work items.

A voxel of the left volume takes the d-invariant border cost where x < d (src/CVC.cpp:135-146), of the right volume where
x >= W - d; the guided filter (src/CVF.cpp:72-165) reads input columns x-8 .. x+6 under output column x.  Once all of them are
border columns a slice repeats the one below it bit for bit, and DispSel::CVSelect (src/DispSel.cpp:96-104) takes the lowest d
on ties: such a (column group, slice) work item cannot change a map, and k_cvf_pc does not run it.  The predicate is the
library's own (psm_debug_pc_dead); the volumes are the oracle's, float and 8-bit."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    l = C.CDLL(capi.LIB_PATH)
    l.psm_debug_pc_dead.restype = C.c_int
    l.psm_debug_pc_items.restype = C.c_int
    l.psm_debug_pc_group_items.restype = C.c_int
    return l


def random_pair(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def volumes(oracle):
    """{(W, H, D, dtype): (left volume, right volume)} as integer bit patterns [D][H][W] - computed once."""
    out = {}
    for W, H, D in ((140, 37, 100), (230, 40, 128)):
        l, r = random_pair(W, H, seed=W)
        f = oracle.pipeline_f32(l, r, D, threads=8, want_volumes=True)
        u = oracle.pipeline_u8(l, r, D, threads=8, want_volumes=True)
        out[W, H, D, "f32"] = (f["lvol"].view(np.uint32), f["rvol"].view(np.uint32))
        out[W, H, D, "u8"] = (u["lvol"], u["rvol"])
    return out


# the slices a context owns: (first global disparity, stride)
OWNED = [(0, 1), (60, 1), (0, 4), (1, 4)]


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("W,H,D", [(140, 37, 100), (230, 40, 128)])
def test_dead_slices_repeat_the_slice_below_and_the_predicate_is_tight(lib, volumes, W, H, D, dtype):
    vols = volumes[W, H, D, dtype]
    checked = 0
    for cols in (107, 50):
        ngroups = -(-W // cols)
        for d_begin, dstep in OWNED:
            owned = list(range(d_begin, D, dstep))
            for side in (0, 1):
                vol = vols[side]
                for g in range(ngroups):
                    xf, xl = g * cols, min(W - 1, g * cols + cols - 1)
                    first_dead = first_equal = None
                    for i, dg in enumerate(owned):
                        dprev = owned[i - 1] if i else -1
                        dead = lib.psm_debug_pc_dead(side, xf, g * cols + cols - 1, W, dg, dprev)
                        equal = i > 0 and np.array_equal(vol[dg][:, xf:xl + 1], vol[dprev][:, xf:xl + 1])
                        if i == 0:
                            assert dead == (dg == 0), "a context's first slice is live unless it is d = 0"
                        if dead and dg != 0:
                            assert equal, (cols, d_begin, dstep, side, g, dg, dprev)
                            checked += 1
                            if first_dead is None:
                                first_dead = dg
                        if equal and first_equal is None:
                            first_equal = dg
                    if g in (0, ngroups - 1):       # tight: not one slice later than the volumes allow
                        assert first_dead == first_equal, (cols, d_begin, dstep, side, g, first_dead, first_equal)
    assert checked > 100


def test_predicate_constants(lib):
    dead = lib.psm_debug_pc_dead
    W = 1920
    # left volume, group 0 of the wide layout (x = 0 .. 106): dead once the slice below is at d >= 106 + 7
    assert not dead(0, 0, 106, W, 113, 112) and dead(0, 0, 106, W, 114, 113)
    # right volume, last group of the wide layout (x = 1819 .. 1919, x' = 100 at its first column): from 100 + 9
    assert not dead(1, 1819, 1925, W, 109, 108) and dead(1, 1819, 1925, W, 110, 109)
    # d = 0 is never a candidate; a first slice is live wherever it lies; a strided context's slice below is dstep away
    assert dead(0, 0, 106, W, 0, -1) and dead(1, 0, 106, W, 0, -1)
    assert not dead(0, 0, 106, W, 250, -1) and not dead(1, 1819, 1925, W, 250, -1)
    assert not dead(0, 0, 106, W, 116, 112) and dead(0, 0, 106, W, 117, 113)
    # column 0 alone: the reflected window reaches input column 7
    assert not dead(0, 0, 0, W, 8, 7) and dead(0, 0, 0, W, 9, 8)
    assert not dead(0, 0, 1, W, 8, 7) and dead(0, 0, 1, W, 9, 8)


def items(lib, W, rows, nsl, form, d_begin=0, dstep=1, sel=0, step=1):
    out = (C.c_int * 12)()
    assert lib.psm_debug_pc_items(W, rows, nsl, form, d_begin, dstep, sel, step, out) == 0
    keys = ("ngroups", "nsegs", "DC", "cols", "live_l", "live_r", "all", "slices_l", "slices_r", "blocks", "first", "_")
    return dict(zip(keys, out))


STORE, PLANES, KEYS = 0, 1, 2


def test_planner_counts_live_items_at_1080p_256(lib):
    """1920 x 1080 x 256, two-phase selection with every 8th slice through the planes: 398 of the 2 x 18 x 256 (column group,
    slice) combinations are dead - left group 0 from d = 114 (142) and group 1 from d = 221 (35), right group 17 from d = 110 (146)
    and group 16 from d = 217 (39), d = 0 in all 36."""
    p = items(lib, 1920, 1080, 32, PLANES, sel=1, step=8)
    k = items(lib, 1920, 1080, 224, KEYS, sel=2, step=8)
    assert p["ngroups"] == k["ngroups"] == 18 and p["cols"] == 107
    assert p["all"] * p["DC"] >= 18 * 32 and k["all"] == 18 * 224
    live = p["slices_l"] + p["slices_r"] + k["slices_l"] + k["slices_r"]
    assert live == 9216 - 398
    assert p["slices_l"] + k["slices_l"] == 18 * 256 - (142 + 35 + 18)
    assert p["slices_r"] + k["slices_r"] == 18 * 256 - (146 + 39 + 18)
    # one slice per item in the key form: the items the kernel enumerates are exactly the live slices
    assert (k["live_l"], k["live_r"]) == (k["slices_l"], k["slices_r"])
    assert k["blocks"] >= k["nsegs"] * max(k["live_l"], k["live_r"])
    # the storing form skips nothing
    s = items(lib, 1920, 1080, 256, STORE)
    assert s["live_l"] == s["live_r"] == s["all"] == s["slices_l"] == s["ngroups"] * 256


def test_layouts_of_the_side_order_shapes(lib):
    """The shapes of tests/test_gpu_parity.py::test_right_side_first as the planner cuts their two-volume plane launch: one wide
    column group; the narrow layout with three groups; the wide layout with two groups and more than one chunk, whatever the
    device (DC <= 16 < 20 slices)."""
    a, b, c = items(lib, 61, 21, 4, PLANES), items(lib, 120, 24, 9, PLANES), items(lib, 200, 33, 20, PLANES)
    assert (a["cols"], a["ngroups"]) == (107, 1)
    assert (b["cols"], b["ngroups"]) == (50, 3)
    assert (c["cols"], c["ngroups"]) == (107, 2) and c["DC"] < 20


@pytest.mark.parametrize("W", [150, 200, 300, 450, 1920])
@pytest.mark.parametrize("d_begin,dstep,nsl_all", [(0, 1, 128), (96, 1, 32), (1, 4, 32), (0, 4, 32), (200, 1, 56), (0, 1, 1)])
def test_enumerated_items_are_the_live_slices(lib, W, d_begin, dstep, nsl_all):
    """The counts the kernel's decode runs on (closed form) against the predicate asked slice by slice, for the launches of a
    two-phase selection (every 8th slice / the others) and of a single phase."""
    n1 = -(-nsl_all // 8)
    for form, nsl, sel, step in ((KEYS, nsl_all - n1, 2, 8), (KEYS, n1, 1, 8), (KEYS, nsl_all, 0, 1)):
        if nsl < 1:
            continue
        k = items(lib, W, 40, nsl, form, d_begin, dstep, sel, step)
        assert (k["live_l"], k["live_r"]) == (k["slices_l"], k["slices_r"]), (form, nsl, sel)


def sel_index(sel, step, j):
    """Slice j of a launch -> local slice of the context (PcSel)."""
    return j * step if sel == 1 else ((j // (step - 1)) * step + j % (step - 1) + 1 if sel == 2 else j)


@pytest.mark.parametrize("W", [150, 200, 300, 450, 1920])
@pytest.mark.parametrize("d_begin,dstep,nsl_all", [(0, 1, 128), (96, 1, 32), (1, 4, 32), (0, 4, 32), (200, 1, 56), (0, 1, 1), (0, 1, 256)])
def test_plane_form_table_names_exactly_the_chunks_with_a_live_slice(lib, W, d_begin, dstep, nsl_all):
    """k_cvf_pc writes a chunk's records only where the chunk keeps a slice, and k_chunk_min reads the chunks the launch's item
    table names for the record's column group: per volume and group the table's range must be exactly the chunks that hold a
    slice the predicate calls live - one more and k_chunk_min reads records nobody wrote, one fewer and a candidate is lost."""
    dead = lib.psm_debug_pc_dead
    n1 = -(-nsl_all // 8)
    for nsl, sel, step in ((n1, 1, 8), (nsl_all, 0, 1)):
        p = items(lib, W, 40, nsl, PLANES, d_begin, dstep, sel, step)
        DC, cols = p["DC"], p["cols"]
        total = [0, 0]
        for side in (0, 1):
            for g in range(p["ngroups"]):
                want = []
                for ch in range(-(-nsl // DC)):
                    for j in range(ch * DC, min(nsl, ch * DC + DC)):
                        i = sel_index(sel, step, j)
                        dprev = d_begin + (i - 1) * dstep if i > 0 else -1
                        if not dead(side, g * cols, g * cols + cols - 1, W, d_begin + i * dstep, dprev):
                            want.append(ch)
                            break
                out = (C.c_int * 2)()
                assert lib.psm_debug_pc_group_items(W, 40, nsl, PLANES, d_begin, dstep, sel, step, side, g, out) == 0
                assert list(range(out[0], out[0] + out[1])) == want, (nsl, sel, side, g, DC, out[0], out[1], want)
                total[side] += len(want)
        assert (p["live_l"], p["live_r"]) == tuple(total)
