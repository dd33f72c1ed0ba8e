"""-m gpu: psm_joint_wmf, the joint weighted median of the reference's live PP::processDM (src/PP.cpp:402-424), against the
numpy model tests/jwmf_model.py - clustering (label_of_key, centres, iterations) and both maps bit for bit."""
import json
import os

import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jwmf_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def _device(P, l, r, lmap, rmap, D=8, radius=0, n_clusters=0, clusters=None, options=()):
    with P.DispEst(l, r, D) as de:
        for o, v in options:
            de.set_option(o, v)
        de.upload_maps(lmap, rmap)
        for s, cl in enumerate(clusters or ()):
            if cl is not None:
                de.set_jwmf_clusters(s, *cl)
        de.JointWMF_GPU(radius, 0.0, n_clusters, 0)
        de.synchronize()
        return de.lDisMap.copy(), de.rDisMap.copy(), [de.jwmf_clusters(s) for s in (0, 1)]


def _check_clusters(dev, img, n_clusters=256):
    cen, lok, it = dev
    m = M.clustering_of(img, n_clusters)
    assert it == m["iterations"]
    assert np.array_equal(cen, m["centres"])
    assert np.array_equal(lok, m["lok"])
    return m


def _random_pair(W, H, seed, depth):
    rng = np.random.default_rng(seed)
    l = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lm = rng.integers(0, 256, (H, W), dtype=np.uint8)
    rm = rng.integers(0, 256, (H, W), dtype=np.uint8)
    if depth == "f32":       # the harness's float images (u8 * (1/255.0f)) plus values that saturate / round
        l = l.astype(np.float32) * np.float32(1 / 255.0)
        r = r.astype(np.float32) * np.float32(1 / 255.0)
        l[0, 0] = (-0.5, 1.7, 0.50196)
    return l, r, lm, rm


@pytest.mark.parametrize("W,H", [(8, 8), (9, 11), (33, 17)])
@pytest.mark.parametrize("radius", [1, 4, 9, 16])
@pytest.mark.parametrize("n_clusters", [1, 16, 256])
def test_small_equal_model(psm, W, H, radius, n_clusters):
    depth = ("u8", "f32")[(W + radius + n_clusters) % 2]
    l, r, lm, rm = _random_pair(W, H, W * 1000 + H * 10 + radius, depth)
    dl, dr, cl = _device(psm, l, r, lm, rm, radius=radius, n_clusters=n_clusters)
    for img, dmap, out, dev in ((l, lm, dl, cl[0]), (r, rm, dr, cl[1])):
        m = _check_clusters(dev, img, n_clusters)
        wq = M.quantise(M.weight_table(m["centres"]))
        assert np.array_equal(out, M.median(dmap, m["F"], wq, radius))


def test_bring_your_own_clusters(psm):
    W, H = 70, 45
    l, r, lm, rm = _random_pair(W, H, 7, "u8")
    rng = np.random.default_rng(8)
    n = 200
    cen = (rng.random((n, 3)) * 63).astype(np.float32)
    lok = rng.integers(0, n, 64 ** 3).astype(np.uint8)
    dl, dr, cl = _device(psm, l, r, lm, rm, radius=5, clusters=[(cen, lok), None])
    assert np.array_equal(cl[0][0], cen) and np.array_equal(cl[0][1], lok) and cl[0][2] == 0
    assert np.array_equal(dl, M.joint_wmf(lm, l, 5, clusters=(cen, lok)))
    _check_clusters(cl[1], r)
    assert np.array_equal(dr, M.joint_wmf(rm, r, 5))
    # a label outside the clustering is refused
    from primestereomatch_amd import capi
    with psm.DispEst(l, r, 16) as de:
        bad = lok.copy()
        bad[5] = n
        with pytest.raises(capi.PsmError):
            de.set_jwmf_clusters(0, cen, bad)


def _golden(name):
    """The committed pair, oracle maps and JointWMF fixture (scripts/make_jwmf_fixtures.py: the model's clustering and maps)."""
    pair = dict(np.load(os.path.join(GOLDEN, f"{name}_pair.npz")))
    gold = dict(np.load(os.path.join(GOLDEN, f"{name}_oracle_d64.1.npz")))
    fx = dict(np.load(os.path.join(GOLDEN, f"{name}_jwmf.npz")))
    return pair, gold, fx


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_middlebury_equal_fixture(psm, name):
    pair, gold, fx = _golden(name)
    dl, dr, cl = _device(psm, pair["l_bgr"], pair["r_bgr"], gold["ldisp"], gold["rdisp"], D=64)
    for s, out in ((0, dl), (1, dr)):
        k = "lr"[s]
        assert cl[s][2] == int(fx[f"{k}_iterations"]), (name, s)
        assert np.array_equal(cl[s][0], fx[f"{k}_centres"]) and np.array_equal(cl[s][1], fx[f"{k}_lok"]), (name, s)
        assert np.array_equal(out, fx[f"{k}map"]), (name, s, int(np.count_nonzero(out != fx[f"{k}map"])))
    print(f"{name}: {int(fx['l_iterations'])} / {int(fx['r_iterations'])} Lloyd iterations")


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_harness_joint_wmf_bp(psm, name):
    """harness.compute(joint_wmf=True) scores the filtered left map, as StereoMatch::compute does after PostProcess."""
    from primestereomatch_amd import harness
    pair, gold, fx = _golden(name)
    out = harness.compute(pair["l_bgr"], pair["r_bgr"], 64, gt=pair["gt_l"], mask=pair["occl"], scale_factor=4, joint_wmf=True)
    raw = harness.compute(pair["l_bgr"], pair["r_bgr"], 64, gt=pair["gt_l"], mask=pair["occl"], scale_factor=4)
    assert np.array_equal(out["lDisMap_raw"], gold["ldisp"])
    assert np.array_equal(out["lDisMap"], fx["lmap"]) and np.array_equal(out["rDisMap"], fx["rmap"])
    bp = harness.error_vs_ground_truth(fx["lmap"], pair["gt_l"], pair["occl"], 64, 4, 4)[0]
    assert out["bp_percent"] == bp
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))[name.capitalize()]
    assert raw["bad_pixels"] == man["bad_pixels_thr4_nonocc"]
    print(f"{name}: %BP raw {raw['bp_percent']:.2f} -> JointWMF {out['bp_percent']:.2f}")


@pytest.mark.parametrize("W,H,D", [(1280, 720, 128), (1920, 1080, 256)])
def test_synthetic_large(psm, W, H, D):
    """Clustering of both images equal to the model's (tests/golden/synthetic_jwmf_clusters.npz) bit for bit; both maps
    equal to the model's median on the first, middle and last rows plus 3000 random pixels."""
    from primestereomatch_amd import synth
    fx = np.load(os.path.join(GOLDEN, "synthetic_jwmf_clusters.npz"))
    l, r, _ = synth.make_pair(W, H, D, seed=3)
    rng = np.random.default_rng(W)
    lm = rng.integers(0, D, (H, W), dtype=np.uint8)
    rm = rng.integers(0, D, (H, W), dtype=np.uint8)
    dl, dr, cl = _device(psm, l, r, lm, rm, D=D)
    ys = np.concatenate([np.repeat([0, H // 2, H - 1], W), rng.integers(0, H, 3000)])
    xs = np.concatenate([np.tile(np.arange(W), 3), rng.integers(0, W, 3000)])
    for k, img, dmap, out, (cen, lok, it) in (("l", l, lm, dl, cl[0]), ("r", r, rm, dr, cl[1])):
        p = f"s{W}x{H}_{k}"
        assert it == int(fx[f"{p}_iterations"]) and np.array_equal(cen, fx[f"{p}_centres"]) and np.array_equal(lok, fx[f"{p}_lok"]), p
        ref = M.median(dmap, lok[M.keys_of(M.feature_u8(img))], M.quantise(M.weight_table(cen)), 9, pixels=(ys, xs))
        assert np.array_equal(out[ys, xs], ref[ys, xs])
        print(f"{W}x{H} {k}: {it} Lloyd iterations")


@pytest.fixture(scope="module")
def reading(tmp_path_factory):
    return M.load_reading(str(tmp_path_factory.mktemp("jwmf_reading")))


def test_pin_palette_pair_equals_reading(psm, reading):
    """The pin: a 450 x 375 pair with at most 256 distinct 6-bit keys (where every clustering is the identity, so the
    reference's result does not depend on its RNG) through the whole pipeline - CostConst, CostFilter, DispSelect,
    JointWMF - equals the serial reading of the reference's filterCore (tests/jwmf_reading.c) on every pixel outside the
    near-tie rule."""
    from primestereomatch_amd import synth
    W, H, D = 450, 375, 64
    l, r, _ = synth.make_pair(W, H, D, seed=12)
    l, r = (((im // 43) * 43 + 21).astype(np.uint8) for im in (l, r))      # 6 levels per channel: <= 216 keys
    with psm.DispEst(l, r, D) as de:
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        raw = de.lDisMap.copy(), de.rDisMap.copy()
        de.JointWMF_GPU()
        out = de.lDisMap.copy(), de.rDisMap.copy()
        cl = [de.jwmf_clusters(s) for s in (0, 1)]
    total = 0
    for s, img in ((0, l), (1, r)):
        ref, nf = M.reading_identity(reading, img, raw[s])
        assert 0 < nf <= 216 and cl[s][2] == 0 and len(cl[s][0]) == nf
        m = M.clustering_of(img)
        w = M.weight_table(m["centres"])
        diff = np.argwhere(out[s] != ref)
        for y, x in diff:
            assert M.near_tie(raw[s], m["F"], w, 9, y, x, int(ref[y, x]), int(out[s][y, x])), (s, y, x)
        assert np.count_nonzero(out[s] != raw[s]) > 0
        total += len(diff)
        print(f"pin side {s}: {nf} keys, {len(diff)} of {W * H} pixels differ from the reading, all near-ties")


def test_host_clusters_async_and_reuse(psm):
    """Host clusters on both sides under PSM_OPT_ASYNC; a second call on the same pair reuses the clustering and the tables
    (one PSM_K_JWMF bracket: planes + median) and gives the same maps."""
    from primestereomatch_amd import capi
    W, H = 80, 50
    l, r, lm, rm = _random_pair(W, H, 21, "u8")
    rng = np.random.default_rng(22)
    cls = [((rng.random((n, 3)) * 63).astype(np.float32), rng.integers(0, n, 64 ** 3).astype(np.uint8)) for n in (37, 256)]
    refs = [M.joint_wmf(d, im, 9, clusters=c) for d, im, c in ((lm, l, cls[0]), (rm, r, cls[1]))]
    with psm.DispEst(l, r, 16) as de:
        de.set_option(capi.PSM_OPT_ASYNC, 1)
        de.upload_maps(lm, rm)
        for s in (0, 1):
            de.set_jwmf_clusters(s, *cls[s])
        de.JointWMF_GPU()
        de.synchronize()
        assert np.array_equal(de.lDisMap, refs[0]) and np.array_equal(de.rDisMap, refs[1])
    with psm.DispEst(l, r, 16) as de:
        de.upload_maps(lm, rm)
        de.JointWMF_GPU()
        first = de.lDisMap.copy(), de.rDisMap.copy()
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        de.reset_kernel_times()
        de.upload_maps(lm, rm)
        de.JointWMF_GPU()
        assert de.kernel_time_ms(capi.PSM_K_JWMF)[1] == 1
        assert np.array_equal(de.lDisMap, first[0]) and np.array_equal(de.rDisMap, first[1])
        # another sigma: same clustering, new tables
        de.upload_maps(lm, rm)
        de.JointWMF_GPU(sigma=10.0)
        assert de.kernel_time_ms(capi.PSM_K_JWMF)[1] == 2
        cen, lok, _ = de.jwmf_clusters(0)
        assert np.array_equal(de.lDisMap, M.joint_wmf(lm, l, 9, sigma=10.0, clusters=(cen, lok)))


def test_async_option_and_stripe_refusal(psm):
    from primestereomatch_amd import capi, synth
    W, H, D = 96, 40, 16
    l, r, _ = synth.make_pair(W, H, D, seed=5)
    lm, rm = np.random.default_rng(1).integers(0, D, (2, H, W), dtype=np.uint8)
    ref_l, ref_r = M.joint_wmf(lm, l), M.joint_wmf(rm, r)
    dl, dr, _ = _device(psm, l, r, lm, rm, options=[(capi.PSM_OPT_ASYNC, 1)])
    assert np.array_equal(dl, ref_l) and np.array_equal(dr, ref_r)
    with psm.DispEst(l, r, D) as de:
        de.set_rows(0, H // 2)
        de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
        with pytest.raises(capi.PsmError, match="stripe"):
            de.JointWMF_GPU()
        with pytest.raises(capi.PsmError):
            de.JointWMF_GPU(radius=17)


def test_merged_root(psm, oracle):
    """On the root after psm_disp_merge_ctx: the merged maps filtered with the root's images."""
    from primestereomatch_amd import synth
    W, H, D = 120, 50, 20
    l, r, _ = synth.make_pair(W, H, D, seed=6)
    ref = oracle.pipeline_f32(l, r, D, threads=8)
    shards = [psm.DispEst(l, r, D, d_range=rg) for rg in ((0, 9), (9, 20))]
    try:
        for s in shards:
            s.CostConst_GPU(); s.CostFilter_GPU(); s.DispSelect_partial()
        shards[0].DispSelect_merge_ctx(shards)
        assert np.array_equal(shards[0].lDisMap, ref["ldisp"])
        shards[0].JointWMF_GPU()
        assert np.array_equal(shards[0].lDisMap, M.joint_wmf(ref["ldisp"], l))
        assert np.array_equal(shards[0].rDisMap, M.joint_wmf(ref["rdisp"], r))
    finally:
        for s in shards:
            s.close()


def _chain_img(W, H, k):
    """Image k of the generator tests/test_gpu_jwmf_batch.py uses (its model chains at 33 x 17, 4 clusters: k = 7: 11 Lloyd
    iterations, k = 22: 51)."""
    return np.random.default_rng(1000 + k).integers(0, 256, (H, W, 3), dtype=np.uint8)


def test_single_call_bracket_count(psm):
    """PSM_K_JWMF brackets of a single call that clusters, the batch's formula: keys, seeding, one per group of 16 Lloyd
    iterations until every image has converged, clusters, median - both images of the call in the same launches."""
    from primestereomatch_amd import capi
    W, H, nc, radius = 33, 17, 4, 4
    short, long_ = _chain_img(W, H, 7), _chain_img(W, H, 22)
    rng = np.random.default_rng(5)
    pal = rng.integers(0, 256, (3, 3), dtype=np.uint8)
    ident = pal[rng.integers(0, 3, (H, W))], pal[rng.integers(0, 3, (H, W))]
    lm, rm = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    host = (rng.random((7, 3)) * 63).astype(np.float32), rng.integers(0, 7, 64 ** 3).astype(np.uint8)

    def run(l, r, clusters=()):
        with psm.DispEst(l, r, 8) as de:
            de.upload_maps(lm, rm)
            for s, cl in enumerate(clusters):
                if cl is not None:
                    de.set_jwmf_clusters(s, *cl)
            de.set_option(capi.PSM_OPT_PROFILE, 1)
            de.reset_kernel_times()
            de.JointWMF_GPU(radius, 0.0, nc, 0)
            return de.kernel_time_ms(capi.PSM_K_JWMF)[1], [de.jwmf_clusters(s)[2] for s in (0, 1)]

    its = [M.clustering_of(im, nc)["iterations"] for im in (short, long_)]
    assert 0 < its[0] <= 16 and its[1] > 32, its
    for l, r in ((short, long_), (long_, short)):
        n, got = run(l, r)
        assert sorted(got) == its
        print("two k-means images:", n, got)
        assert n == 2 + -(-max(its) // 16) + 2
    n, got = run(*ident)
    print("two identity images:", n, got)
    assert got == [0, 0] and n == 2 + 0 + 2
    n, got = run(short, long_, (None, host))
    print("host clusters on the long side:", n, got)
    assert got == [its[0], 0] and n == 2 + 1 + 2


def test_jwmf_only_async_frame_loop(psm):
    """construct(i) (adopts pair i); setInputImages_async(pair i + 1); JointWMF of uploaded maps with pair i as the feature images -
    no guided filter in between, PSM_OPT_ASYNC on.  The stage forms its keys and cluster planes from the image slots and records that
    it has read them (images_read), so the copy into the slot of two frames ago is ordered behind it.  Every frame's maps must be the
    model's for THAT frame's pair.  This guards the mark and the bookkeeping around it; it cannot see a missing ordering even by
    chance: psm_upload_maps blocks, and clustering a new pair synchronises the host several times inside psm_joint_wmf, so the host
    has caught up with the device well before the next upload is issued.  The proof is the code: one function, called by every
    reader."""
    from primestereomatch_amd import capi
    W, H, D, radius, nc, frames = 67, 45, 16, 4, 16, 5
    data = [_random_pair(W, H, 300 + i, "u8") for i in range(frames)]
    with psm.DispEst(data[0][0], data[0][1], D) as de:
        de.set_option(capi.PSM_OPT_ASYNC, 1)
        de.setInputImages_async(*data[0][:2])
        for i, (l, r, lm, rm) in enumerate(data):
            de.CostConst_GPU()
            if i + 1 < frames:
                de.setInputImages_async(*data[i + 1][:2])
            de.upload_maps(lm, rm)
            de.JointWMF_GPU(radius, 0.0, nc, 0)
            de.synchronize()
            assert np.array_equal(de.lDisMap, M.joint_wmf(lm, l, radius, n_clusters=nc)), i
            assert np.array_equal(de.rDisMap, M.joint_wmf(rm, r, radius, n_clusters=nc)), i


def test_reclustering_after_a_parameter_change(psm):
    """Another n_clusters on a clustered pair clusters both sides again, and the first parameters after that once more: a
    kept clustering is one made with the call's own parameters."""
    from primestereomatch_amd import capi
    W, H, radius = 33, 17, 4
    l, r, lm, rm = _random_pair(W, H, 31, "u8")
    with psm.DispEst(l, r, 8) as de:
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        seen = []
        for nc in (16, 5, 16):
            de.upload_maps(lm, rm)
            de.reset_kernel_times()
            de.JointWMF_GPU(radius, 0.0, nc, 0)
            assert de.kernel_time_ms(capi.PSM_K_JWMF)[1] > 1          # (1: planes + median alone, a clustering kept)
            for s, img, dmap, out in ((0, l, lm, de.lDisMap), (1, r, rm, de.rDisMap)):
                m = _check_clusters(de.jwmf_clusters(s), img, nc)
                assert m["iterations"] > 0 and len(m["centres"]) == nc
                assert np.array_equal(out, M.median(dmap, m["F"], M.quantise(M.weight_table(m["centres"])), radius))
            seen.append(de.jwmf_clusters(0)[0].copy())
        assert np.array_equal(seen[0], seen[2]) and seen[0].shape != seen[1].shape
