"""-m gpu: the Fast Guided Filter path (psm_cost_filter_fgf, psm_fgf.hip) at the seams of its launches, on images smaller than a
blur window and on adversarial content, against the CPU oracle (cases, contents and references: tests/fgf_inputs.py, held to their
own conditions on the CPU by tests/test_fgf_inputs.py).  Volumes and maps are the oracle's bits - np.array_equal, no tolerance
anywhere in this file; only the NaN volumes compare with equal_nan, and their maps exactly.

What the fixed shapes of test_gpu_fgf.py, the sweep of test_gpu_fuzz.py and the golden pairs do not reach and this file does:
  * two strips of blur4_march at s = 8, three at s = 4, a strip of a single column at every rate
  * a last row segment shorter than the blur radius (one row), three segments against volumes, strips and segments together
  * a second x-block of k_fgf_apply4 / k_fgf_apply_wta (W = 1028: one live thread), five of k_fgf_apply
  * row blocks of the 4-pixel kernels hanging over the image at either end for every H % 4
  * images whose subsampled width or height lies in [R + 1, 2 R], R = 8 / s: every window reflects at both ends
  * noise, binary, constant and half-flat pairs; float pairs outside [0, 1]
  * exact ties between slices of different 32-slice chunks, negative and subnormal costs, NaN and overflow through the fused
    upsample + winner-takes-all and its 64-bit atomicMin
  * disparity shards (d_begin != 0 inside k_fgf_model's own cost) at the strip and segment seams"""
import numpy as np
import pytest

import fgf_inputs as G

pytestmark = pytest.mark.gpu

LAZY, STORE, MATERIALISE = 0, 4096, 128          # PSM_OPT_FLAGS: 0 | PSM_FLAG_FGF_STORE | PSM_FLAG_MATERIALISE_COSTS


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    assert (capi.PSM_FLAG_FGF_STORE, capi.PSM_FLAG_MATERIALISE_COSTS) == (STORE, MATERIALISE)
    import primestereomatch_amd as P
    return P


def first_diff(a, b, nan_equal=False):
    """-> the first differing index of two arrays as a list ((d, y, x) of volumes, (y, x) of maps), None when there is none"""
    ne = a != b
    if nan_equal:
        ne &= ~(np.isnan(a) & np.isnan(b))
    w = np.argwhere(ne)
    return w[0].tolist() if len(w) else None


def differing(name, got, ref, nan_equal=False):
    """got, ref: dicts of arrays under the same keys -> {key: count of differing elements}, printed; asserts there is none and names
    the first differing (d, y, x) of each key otherwise."""
    n, first = {}, {}
    for k in got:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (name, k, got[k].shape, ref[k].shape)
        eq = got[k] == ref[k]
        if nan_equal and got[k].dtype.kind == "f":
            eq |= np.isnan(got[k]) & np.isnan(ref[k])
        n[k] = int(eq.size - np.count_nonzero(eq))
        if n[k]:
            first[k] = first_diff(got[k], ref[k], nan_equal)
    print(f"[fgf-seams] {name}: differing elements {n}")
    assert not first, (name, n, {k: (v, got[k][tuple(v)], ref[k][tuple(v)]) for k, v in first.items()})
    for k in got:        # (the statement itself, beside the count)
        assert np.array_equal(got[k], ref[k], equal_nan=nan_equal and got[k].dtype.kind == "f"), (name, k)


def run_pair(psm, l, r, D, s, flags, name, ref):
    """CostConst -> CostFilter_FGF -> DispSelect under `flags`; the maps are compared BEFORE any volume is downloaded (flags 0 and
    16-byte rows: the filtered volume is virtual and the fused upsample + WTA made them), the volumes after."""
    from primestereomatch_amd import capi
    with psm.DispEst(l, r, D) as de:
        de.set_option(capi.PSM_OPT_FLAGS, flags)
        de.setSubsampleRate(s)
        de.CostConst_GPU()
        de.CostFilter_FGF_GPU()
        de.DispSelect_GPU()
        differing(f"{name} flags {flags} maps", {"ldisp": de.lDisMap, "rdisp": de.rDisMap}, ref)
        differing(f"{name} flags {flags} volumes", {"lvol": de.download_volume(0), "rvol": de.download_volume(1)}, ref)
        de.DispSelect_GPU()                      # the selection of the volumes now in memory
        differing(f"{name} flags {flags} maps of the stored volumes", {"ldisp": de.lDisMap, "rdisp": de.rDisMap}, ref)


def run_case(psm, case):
    tag, W, H, D, s, kind, seed = case
    l, r = G.content(case)
    ref = G.reference(l, r, D, s)
    g = G.grid(W, H, D, s)
    name = (f"{tag} {W}x{H}x{D} s={s} {kind} (strips {g['strips']}, segments {g['segs']} last {g['last_seg']}, x-blocks {g['xblocks']} "
            f"{'fused' if g['fused'] else 'k_fgf_apply'}, chunks {g['chunks']})")
    for flags in (LAZY, STORE, MATERIALISE):
        run_pair(psm, l, r, D, s, flags, name, ref)


def _id(case):
    return f"{case[0].replace(' ', '_')}-{case[1]}x{case[2]}x{case[3]}-s{case[4]}-{case[5]}"


@pytest.mark.parametrize("case", G.seam_cases(), ids=_id)
def test_seam_cases(psm, case):
    run_case(psm, case)


@pytest.mark.parametrize("case", G.small_cases(), ids=_id)
def test_small_images(psm, case):
    """Subsampled width and / or height in [R + 1, 2 R]: r101s folds once, and that is exact down to R + 1."""
    run_case(psm, case)


@pytest.mark.parametrize("W,H,s,refused", G.refusal_cases())
def test_small_images_refusal_boundary(psm, W, H, s, refused):
    """Subsampled size R is refused ("too small"), R + 1 runs and equals the oracle; a refused call leaves the context usable."""
    from primestereomatch_amd import synth
    D = 2
    l, r, _ = synth.make_pair(W, H, D, seed=W + H + s)
    with psm.DispEst(l, r, D) as de:
        de.setSubsampleRate(s)
        de.CostConst_GPU()
        if refused:
            with pytest.raises(RuntimeError, match="too small"):
                de.CostFilter_FGF_GPU()
            de.CostFilter_GPU()                  # the full filter takes any 8 x 8 image
            de.DispSelect_GPU()
            assert de.lDisMap.shape == (H, W)
            return
        de.CostFilter_FGF_GPU()
        de.DispSelect_GPU()
        ref = G.reference(l, r, D, s)
        differing(f"boundary {W}x{H} s={s}", {"ldisp": de.lDisMap, "rdisp": de.rDisMap, "lvol": de.download_volume(0),
                                               "rvol": de.download_volume(1)}, ref)


@pytest.mark.parametrize("W,H,s", G.STRIPS_AND_SEGMENTS)
def test_disparity_shards_at_the_seams(psm, W, H, s):
    """Two d_range shards of a case with two strips and two segments, cut at a random slice and at slice 32 (the chunk seam):
    DispSelect_partial + DispSelect_merge_ctx give the whole pair's maps, and each shard's volume is the reference's slices -
    the second shard builds its costs with d_begin != 0 inside k_fgf_model."""
    D = 40
    g = G.grid(W, H, D, s)
    assert g["strips"] >= 2 and g["segs"] >= 2 and g["last_seg"] == 1 and g["fused"]
    rng = np.random.default_rng(W + s)
    l, r = G.F.sgm_content("noise" if s == 4 else "synth", W, H, D, rng)
    ref = G.reference(l, r, D, s)
    for cut in (int(rng.integers(1, 32)), 32):
        shards = [psm.DispEst(l, r, D, d_range=(0, cut)), psm.DispEst(l, r, D, d_range=(cut, D))]
        try:
            for sh in shards:
                sh.setSubsampleRate(s)
                sh.CostConst_GPU()
                sh.CostFilter_FGF_GPU()
                sh.DispSelect_partial()
            shards[0].DispSelect_merge_ctx(shards)
            differing(f"shards {W}x{H}x{D} s={s} cut {cut} maps", {"ldisp": shards[0].lDisMap, "rdisp": shards[0].rDisMap}, ref)
            for sh, (d0, d1) in zip(shards, ((0, cut), (cut, D))):
                differing(f"shards {W}x{H}x{D} s={s} slices {d0}..{d1}", {"lvol": sh.download_volume(0), "rvol": sh.download_volume(1)},
                          {"lvol": ref["lvol"][d0:d1], "rvol": ref["rvol"][d0:d1]})
        finally:
            for sh in shards:
                sh.close()


@pytest.fixture(scope="module")
def adversarial_refs():
    """(name, s) -> (volume, {"lvol", "rvol", "ldisp", "rdisp"}): computed once, shared, never written to"""
    cache = {}

    def get(name, s):
        if (name, s) not in cache:
            l, r = G.adversarial_guidance()
            vol = G.adversarial_volume(name, s)
            (lq, lm), (rq, rm) = G.reference_uploaded(l, vol, s), G.reference_uploaded(r, vol, s)
            cache[name, s] = (vol, {"lvol": lq, "rvol": rq, "ldisp": lm, "rdisp": rm})
        return cache[name, s]
    return get


@pytest.mark.parametrize("s", G.RATES)
@pytest.mark.parametrize("name", G.ADVERSARIAL)
def test_adversarial_volumes(psm, adversarial_refs, name, s):
    """Uploaded volumes (fgf_inputs.adversarial_volume) on both sides: ties across the chunk merge (the lower slice wins), a negative
    winner, a subnormal winner that a flush to zero would lose, NaN slices, patches and pixels and overflowing products."""
    from primestereomatch_amd import capi
    l, r = G.adversarial_guidance()
    vol, ref = adversarial_refs(name, s)
    nan = name == "nan"
    for flags in (LAZY, STORE):
        with psm.DispEst(l, r, G.ADV_D) as de:
            de.set_option(capi.PSM_OPT_FLAGS, flags)
            de.setSubsampleRate(s)
            de.upload_volume(0, vol)
            de.upload_volume(1, vol)
            de.CostFilter_FGF_GPU()
            de.DispSelect_GPU()
            differing(f"adversarial {name} s={s} flags {flags} maps", {"ldisp": de.lDisMap, "rdisp": de.rDisMap}, ref)
            differing(f"adversarial {name} s={s} flags {flags} volumes", {"lvol": de.download_volume(0), "rvol": de.download_volume(1)},
                      ref, nan_equal=nan)


@pytest.mark.parametrize("W,H,D,s,seed", G.FLOAT_CASES)
def test_float_pairs(psm, W, H, D, s, seed):
    """Float images that are no byte / 255 (values below 0 and above 1, -0.0, exact .5 products): the reference is the composed one
    on the float images themselves."""
    lf, rf = G.float_pair(W, H, D, seed)
    ref = G.reference(lf, rf, D, s)
    for flags in (LAZY, STORE, MATERIALISE):
        run_pair(psm, lf, rf, D, s, flags, f"float pair {W}x{H}x{D} s={s}", ref)
