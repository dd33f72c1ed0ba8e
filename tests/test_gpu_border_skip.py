"""-m gpu: the select forms of k_cvf_pc skip the (column group, slice) work items whose slices only repeat the border cost
(primestereomatch_amd/csrc/psm_live.h; tests/test_border_skip.py holds the argument against the oracle's volumes).  Nothing may
change: maps and packed minima (min cost, lowest d: src/DispSel.cpp:96-104) are the oracle's bit for bit - at widths where most
of a volume's slices are dead, in both layouts, with one and two launches, in 8-bit mode, on a row stripe, on contiguous and
strided disparity shards and in a batch."""
import ctypes as C

import numpy as np
import pytest

from shard_model import pack_keys

pytestmark = pytest.mark.gpu
H = 40


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def device_keys(de):
    hip = C.CDLL("libamdhip64.so")
    ptr, nbytes = de.partial_keys()
    out = np.empty((2, de.hei, de.wid), np.int64)
    de.synchronize()
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
    return out


def keys_of(vol, ds=None):
    """Packed minima of a filtered volume [D][H][W] over the slices ds (default: all): strict '<' in ascending d, d = 0 never a
    candidate, NaN never wins; no candidate: key(+inf, 0)."""
    ds = [d for d in (range(vol.shape[0]) if ds is None else ds) if d != 0]
    v = vol[ds].astype(np.float32)
    v = np.where(np.isnan(v), np.float32(np.inf), v)
    i = np.argmin(v, axis=0)                         # (the first minimum: the lowest d)
    cost = np.take_along_axis(v, i[None], 0)[0]
    d = np.where(np.isinf(cost), 0, np.asarray(ds, np.int64)[i])
    return pack_keys(cost, d)


def random_pair(W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's results per (W, D, dtype, pair seed), computed once."""
    cache = {}

    def get(W, D, dtype="f32", seed=None, pair=None):
        key = (W, D, dtype, seed)
        if key not in cache:
            l, r = pair if pair is not None else random_pair(W, W + D if seed is None else seed)
            fn = oracle.pipeline_f32 if dtype == "f32" else oracle.pipeline_u8
            cache[key] = (l, r, fn(l, r, D, threads=8, want_volumes=True))
        return cache[key]
    return get


def run(psm, l, r, D, dtype="f32", **kw):
    with psm.DispEst(l, r, D, dtype=dtype, **kw) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        return de.lDisMap.copy(), de.rDisMap.copy(), device_keys(de)


def same_as_oracle(out, ref, rows=slice(None)):
    lm, rm, keys = out
    assert np.array_equal(lm[rows], ref["ldisp"][rows]) and np.array_equal(rm[rows], ref["rdisp"][rows])
    assert np.array_equal(keys[0][rows], keys_of(ref["lvol"])[rows]) and np.array_equal(keys[1][rows], keys_of(ref["rvol"])[rows])


# width, D: 200 x 128 two-phase, both launches skip, the right volume's last group (x = 107 .. 199) dead from d = 102 and its first
# from d = 209 > D; 200 x 64 planes only; 300 x 128 left: only group 0 has dead slices (from d = 114), right: the last group
# (x = 214 .. 299) dead from d = 95; 150: the narrow layout, 3 groups of 50
@pytest.mark.parametrize("W,D", [(200, 128), (200, 64), (300, 128), (150, 128), (150, 64)])
def test_maps_and_keys_equal_the_oracle(psm, refs, W, D):
    l, r, ref = refs(W, D)
    same_as_oracle(run(psm, l, r, D), ref)


def test_8bit_mode(psm, refs):
    l, r, ref = refs(200, 128, "u8")
    same_as_oracle(run(psm, l, r, 128, "u8"), ref)


def test_row_stripe(psm, refs):
    l, r, ref = refs(200, 128)
    with psm.DispEst(l, r, 128) as de:
        de.set_rows(8, 30)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        same_as_oracle((de.lDisMap, de.rDisMap, device_keys(de)), ref, slice(8, 30))


def test_contiguous_shard_keeps_its_first_slice(psm, refs):
    """d = 96 .. 127: for the left volume's group 0 (dead from d = 114 in the whole range) and most of the right volume every
    slice but the first repeats it - the first one carries the value and must survive."""
    l, r, ref = refs(200, 128)
    with psm.DispEst(l, r, 128, d_range=(96, 128)) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_partial()
        keys = device_keys(de)
    for s, v in enumerate(("lvol", "rvol")):
        assert np.array_equal(keys[s], keys_of(ref[v], range(96, 128)))
    shards = []
    for a, b in ((0, 96), (96, 128)):
        de = psm.DispEst(l, r, 128, d_range=(a, b))
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_partial()
        shards.append(de)
    shards[0].DispSelect_merge_ctx(shards)
    assert np.array_equal(shards[0].lDisMap, ref["ldisp"]) and np.array_equal(shards[0].rDisMap, ref["rdisp"])
    for de in shards:
        de.close()


def test_strided_shards(psm, refs):
    l, r, ref = refs(200, 128)
    shards = []
    for g in range(4):
        de = psm.DispEst(l, r, 128, 8, True, d_stride=(g, 4))
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_partial()
        shards.append(de)
    keys = device_keys(shards[1])                    # d = 1, 5, 9, ...
    for s, v in enumerate(("lvol", "rvol")):
        assert np.array_equal(keys[s], keys_of(ref[v], range(1, 128, 4)))
    shards[0].DispSelect_merge_ctx(shards)
    assert np.array_equal(shards[0].lDisMap, ref["ldisp"]) and np.array_equal(shards[0].rDisMap, ref["rdisp"])
    allk = np.stack([device_keys(de) for de in shards]).min(axis=0)
    assert np.array_equal(allk[0], keys_of(ref["lvol"])) and np.array_equal(allk[1], keys_of(ref["rvol"]))
    for de in shards:
        de.close()


def test_batch_of_two_pairs(psm, refs):
    from primestereomatch_amd.dispest import compute_batch
    cases = [refs(200, 128), refs(200, 128, seed=7)]
    des = [psm.DispEst(l, r, 128) for l, r, _ in cases]
    try:
        compute_batch(des)
        for de, (_, _, ref) in zip(des, cases):
            lm, rm = de.download_maps()
            same_as_oracle((lm, rm, device_keys(de)), ref)
    finally:
        for de in des:
            de.close()


def test_white_borders_pin_the_first_all_border_slice(psm, refs):
    """Left image white in its first 130 columns, right image white in its last 130: the border cost there is 0, the minimum, and
    the winner of a pixel is the first slice whose whole window is border - the very slice below the first dead one.  A predicate
    that drops one slice too many changes the maps."""
    l, r = random_pair(200, 11)
    l, r = l.copy(), r.copy()
    l[:, :130] = 255
    r[:, 70:] = 255
    _, _, ref = refs(200, 128, seed="white", pair=(l, r))
    # (the pair is adversarial only if border slices do win there)
    assert (ref["ldisp"][:, :100] > 8).mean() > 0.5 and (ref["rdisp"][:, 100:] > 8).mean() > 0.5
    same_as_oracle(run(psm, l, r, 128), ref)
    _, _, ref8 = refs(200, 128, "u8", seed="white", pair=(l, r))
    same_as_oracle(run(psm, l, r, 128, "u8"), ref8)


@pytest.mark.parametrize("W,lw,rw,xl,dl,xr,dr", [(200, 120, 80, 106, 113, None, None), (150, 60, 60, 49, 56, 100, 58)])
def test_white_borders_at_the_edge_of_a_column_group(psm, refs, W, lw, rw, xl, dl, xr, dr):
    """The same construction sized to a column group: in the last column of the left volume's group 0 (first column of the right
    volume's last group) the oracle's winner is the very slice whose successor is the group's first dead one."""
    l, r = random_pair(W, 11)
    l, r = l.copy(), r.copy()
    l[:, :lw] = 255
    r[:, W - rw:] = 255
    for dtype in ("f32", "u8"):
        _, _, ref = refs(W, 128, dtype, seed=("white", lw), pair=(l, r))
        assert (ref["ldisp"][:, xl] == dl).all() and (xr is None or (ref["rdisp"][:, xr] == dr).all())
        same_as_oracle(run(psm, l, r, 128, dtype), ref)
