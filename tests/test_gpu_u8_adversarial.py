"""-m gpu: the 8-bit char mode against the oracle on the adversarial cases of tests/u8_inputs.py, through every form the mode
has - 0 differing elements in the packed minima (min q8, lowest d), the maps and, where a form holds them, the raw and the
filtered volumes.  Maps alone would not do: the fused-multiply-add reading of the cost line changes 1 236 keys of the cost table and
not one pixel of its maps (tests/test_u8_inputs.py).

The forms: the default select path (k_cvf_pc<U8>, one phase), the forced two-phase selection (S = 5 below 200 rows, S = 8 from
there), the storing path (k_cvc_u8 -> float copy -> storing kernel -> k_f32_to_u8 -> k_wta_u8), the direct kernel variant, one side
at a time, a batch per geometry, row stripes cut inside a band, contiguous and strided disparity shards, and uploaded 8-bit
volumes.  No form refuses an 8-bit context."""
import numpy as np
import pytest

import u8_inputs as I
import u8_model as M
from test_gpu_border_skip import device_keys, keys_of

pytestmark = pytest.mark.gpu
IMAGE = [c.name for c in I.IMAGE_CASES]
TWO_PHASE_ON = 1048576


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@pytest.fixture(scope="module")
def refs(oracle):
    """Per case, computed once: the oracle's raw and filtered volumes, maps and the packed minima of its filtered volumes.  An
    uploaded volume has no oracle pipeline: the oracle's guided filter, then the quantisation and WTA that test_u8_inputs.py
    holds against the oracle's."""
    cache = {}

    def get(name):
        if name not in cache:
            c = I.BY_NAME[name]
            if c.vols is None:
                ref = oracle.pipeline_u8(c.l, c.r, c.D, threads=8, want_volumes=True, want_raw=True)
            else:
                ref = M.from_raw(oracle, c.l, c.r, *c.vols)
            ref["lkeys"], ref["rkeys"] = keys_of(ref["lvol"]), keys_of(ref["rvol"])
            cache[name] = ref
        return cache[name]
    return get


def differing(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a != b).sum())


def check(what, ref, maps=None, keys=None, raw=None, vols=None, rows=slice(None)):
    """0 differing elements in everything the form handed over."""
    diff = {}
    if keys is not None:
        diff["lkeys"], diff["rkeys"] = differing(keys[0][rows], ref["lkeys"][rows]), differing(keys[1][rows], ref["rkeys"][rows])
    if maps is not None:
        diff["ldisp"], diff["rdisp"] = differing(maps[0][rows], ref["ldisp"][rows]), differing(maps[1][rows], ref["rdisp"][rows])
    if raw is not None:
        diff["raw_l"], diff["raw_r"] = differing(raw[0], ref["raw_l"]), differing(raw[1], ref["raw_r"])
    if vols is not None:
        diff["lvol"], diff["rvol"] = differing(vols[0], ref["lvol"]), differing(vols[1], ref["rvol"])
    assert not any(diff.values()), (what, diff)


def context(psm, c, flags=0, **kw):
    from primestereomatch_amd import capi
    de = psm.DispEst(c.l, c.r, c.D, dtype="u8", **kw)
    if flags:
        de.set_option(capi.PSM_OPT_FLAGS, flags)
    return de


def select_all(de):
    """Maps, then the packed minima (a select form left them behind already; a stored volume goes through the 8-bit WTA again)."""
    de.DispSelect_GPU()
    maps = de.lDisMap.copy(), de.rDisMap.copy()
    de.DispSelect_partial()
    return maps, device_keys(de)


@pytest.mark.parametrize("name", IMAGE)
def test_default_path(psm, refs, name):
    c = I.BY_NAME[name]
    with context(psm, c) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        check(name, refs(name), maps=(de.lDisMap, de.rDisMap), keys=device_keys(de))


@pytest.mark.parametrize("name", IMAGE)
def test_forced_two_phase(psm, refs, name):
    from primestereomatch_amd import capi
    c = I.BY_NAME[name]
    with context(psm, c, TWO_PHASE_ON) as de:
        de.set_option(capi.PSM_OPT_PROFILE, 2)
        de.filter_launch_times()
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        forms = [f for _, f in de.filter_launch_times()]
        # the minima planes of every S-th slice, then the key plane for the rest; the table's 3 slices have one seed slice, d = 0,
        # which is never a candidate: that phase has no work item and starts no kernel
        assert forms == ([1, 2] if c.D > I.seed_stride(c.H) else [2]), forms
        check(name, refs(name), maps=(de.lDisMap, de.rDisMap), keys=device_keys(de))


@pytest.mark.parametrize("name", IMAGE)
def test_storing_path(psm, refs, name):
    from primestereomatch_amd import capi
    c = I.BY_NAME[name]
    with context(psm, c, capi.PSM_FLAG_STORE_FILTERED) as de:
        de.CostConst_GPU()
        raw = de.download_volume(0), de.download_volume(1)   # k_cvc_u8
        de.CostFilter_GPU()
        vols = de.download_volume(0), de.download_volume(1)
        maps, keys = select_all(de)
        check(name, refs(name), maps=maps, keys=keys, raw=raw, vols=vols)


@pytest.mark.parametrize("name", IMAGE)
def test_direct_kernel_variant(psm, refs, name):
    from primestereomatch_amd import capi
    c = I.BY_NAME[name]
    with context(psm, c) as de:
        de.set_option(capi.PSM_OPT_KERNEL_VARIANT, 1)
        de.CostConst_GPU(); de.CostFilter_GPU()
        vols = de.download_volume(0), de.download_volume(1)
        maps, keys = select_all(de)
        check(name, refs(name), maps=maps, keys=keys, vols=vols)


@pytest.mark.parametrize("name", IMAGE)
def test_one_side_at_a_time(psm, refs, name):
    c = I.BY_NAME[name]
    with context(psm, c) as de:
        de.CostConst_GPU()
        de.CostFilter_side(1); de.DispSelect_partial_side(1)
        de.CostFilter_side(0); de.DispSelect_partial_side(0)
        keys = device_keys(de)
        de.DispSelect_merge_ctx([de])
        check(name, refs(name), maps=(de.lDisMap, de.rDisMap), keys=keys)


@pytest.mark.parametrize("geometry", [I.SMALL, I.TALL, I.TABLE], ids=lambda g: "%dx%dx%d" % g)
@pytest.mark.parametrize("flags", [0, TWO_PHASE_ON], ids=["default", "two_phase"])
def test_batch_of_one_geometry(psm, refs, geometry, flags):
    from primestereomatch_amd.dispest import compute_batch
    cases = [c for c in I.IMAGE_CASES if (c.W, c.H, c.D) == geometry]
    assert len(cases) >= 2
    des = [context(psm, c, flags) for c in cases]
    try:
        compute_batch(des)
        for de, c in zip(des, cases):
            lm, rm = de.download_maps()
            check(c.name, refs(c.name), maps=(lm, rm), keys=device_keys(de))
    finally:
        for de in des:
            de.close()


def stripe_bounds(c):
    """Three stripes whose cuts fall inside a band of the half cases (12 and 16 rows) and on no multiple of 4."""
    return [(0, c.H // 3 + 1), (c.H // 3 + 1, 2 * c.H // 3 + 3), (2 * c.H // 3 + 3, c.H)]


@pytest.mark.parametrize("name", I.SUBSET)
@pytest.mark.parametrize("flags", [0, TWO_PHASE_ON], ids=["default", "two_phase"])
def test_row_stripes(psm, refs, name, flags):
    c, ref = I.BY_NAME[name], refs(name)
    assert all(y % 4 and y % 12 and y % 16 for y, _ in stripe_bounds(c)[1:])
    des = [context(psm, c, flags) for _ in range(3)]
    try:
        for de, (y0, y1) in zip(des, stripe_bounds(c)):
            de.set_rows(y0, y1)
            de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
            check((name, y0, y1), ref, maps=(de.lDisMap, de.rDisMap), keys=device_keys(de), rows=slice(y0, y1))
        des[0].gather_rows_ctx(des)
        check(name, ref, maps=(des[0].lDisMap, des[0].rDisMap))
    finally:
        for de in des:
            de.close()


def shard_check(psm, c, ref, flags, shards_kw, owned):
    """Every shard's minima are those of its own slices; merged, the maps and the minima of all slices."""
    des = [context(psm, c, flags, **kw) for kw in shards_kw]
    try:
        keys = []
        for de, ds in zip(des, owned):
            de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_partial()
            k = device_keys(de)
            assert differing(k[0], keys_of(ref["lvol"], ds)) == 0 and differing(k[1], keys_of(ref["rvol"], ds)) == 0, (c.name, ds)
            keys.append(k)
        des[0].DispSelect_merge_ctx(des)
        check(c.name, ref, maps=(des[0].lDisMap, des[0].rDisMap), keys=np.stack(keys).min(axis=0))
    finally:
        for de in des:
            de.close()


@pytest.mark.parametrize("name", I.SUBSET)
@pytest.mark.parametrize("flags", [0, TWO_PHASE_ON], ids=["default", "two_phase"])
def test_contiguous_disparity_shards(psm, refs, name, flags):
    c = I.BY_NAME[name]
    cut = 5 if c.D >= 6 else 2                               # 12 slices: 0 .. 4 and 5 .. 11; the table's 3: 0 .. 1 and 2
    bounds = [(0, cut), (cut, c.D)]
    shard_check(psm, c, refs(name), flags, [{"d_range": b} for b in bounds], [range(*b) for b in bounds])


@pytest.mark.parametrize("name", I.SUBSET)
@pytest.mark.parametrize("flags", [0, TWO_PHASE_ON], ids=["default", "two_phase"])
def test_strided_disparity_shards(psm, refs, name, flags):
    c = I.BY_NAME[name]
    G = 3 if c.D >= 6 else 2
    shard_check(psm, c, refs(name), flags, [{"d_stride": (g, G)} for g in range(G)], [range(g, c.D, G) for g in range(G)])


@pytest.mark.parametrize("name", [c.name for c in I.UPLOAD_CASES])
def test_uploaded_volumes(psm, refs, name):
    c, ref = I.BY_NAME[name], refs(name)
    with context(psm, c) as de:
        de.upload_volume(0, c.vols[0]); de.upload_volume(1, c.vols[1])
        de.CostFilter_GPU()
        maps, keys = select_all(de)
        vols = de.download_volume(0), de.download_volume(1)
        check(name, ref, maps=maps, keys=keys, vols=vols)
    if name == "up_all255":                                  # the start value 256: a volume of 255 selects d = 1, not 0
        assert (maps[0] == 1).all() and (maps[1] == 1).all()
