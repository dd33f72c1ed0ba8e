"""-m gpu: the joint weighted median of several pairs in one set of launches (psm_joint_wmf_batch, dispest.joint_wmf_batch) against
the numpy model tests/jwmf_model.py and against the single call - clusterings (centres, label_of_key, iterations) and both maps of
every context, 0 differing elements everywhere.  Each test recomputes the model's Lloyd iteration counts and asserts the
precondition it relies on (where the counts fall relative to the group of 16 iterations between two looks at the flags)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jwmf_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
JW_GROUP = 16          # psm_api_jwmf.cpp: Lloyd iterations between two looks at the convergence flags


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


@functools.lru_cache(maxsize=None)
def _img(W, H, k):
    a = np.random.default_rng(1000 + k).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _maps(W, H, k):
    a = np.random.default_rng(2000 + k).integers(0, 256, (2, H, W), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _model(W, H, k, n_clusters, max_iter=10000):
    """The model's clustering of image k (computed once, shared, left unchanged)."""
    return M.clustering_of(_img(W, H, k), n_clusters, max_iter)


def _as_f32(img):
    return img.astype(np.float32) * np.float32(1 / 255.0)


def _objects(P, pairs, maps, D=8):
    """(max_disp only sizes the volumes, which the filter never touches; psm_upload_maps takes any byte, as tests/test_gpu_jwmf.py
    relies on too - a context refuses max_disp above its width, so 256 is not available at these sizes)"""
    des = [P.DispEst(l, r, D) for l, r in pairs]
    for d, (lm, rm) in zip(des, maps):
        d.upload_maps(lm, rm)
    return des


def _close(des):
    for d in des:
        d.close()


def _check_side(de, side, m, dmap, radius, out):
    cen, lok, it = de.jwmf_clusters(side)
    assert it == m["iterations"]
    assert np.array_equal(cen, m["centres"])
    assert np.array_equal(lok, m["lok"])
    ref = M.median(dmap, m["F"], M.quantise(M.weight_table(m["centres"])), radius)
    assert int(np.count_nonzero(out != ref)) == 0


def _batch_equals_model_and_singles(P, W, H, ks_l, ks_r, n_clusters, radius, max_iter=0):
    """Contexts i = 0..n-1 hold (image ks_l[i], image ks_r[i]); the batch against the model, then against n single calls."""
    from primestereomatch_amd import dispest
    mi = max_iter or 10000
    n = len(ks_l)
    pairs = [(_img(W, H, a), _img(W, H, b)) for a, b in zip(ks_l, ks_r)]
    maps = [_maps(W, H, i) for i in range(n)]
    des = _objects(P, pairs, maps)
    try:
        assert dispest.joint_wmf_batch(des, radius, 0.0, n_clusters, max_iter) is None
        got = []
        for i, d in enumerate(des):
            for s, k in ((0, ks_l[i]), (1, ks_r[i])):
                _check_side(d, s, _model(W, H, k, n_clusters, mi), maps[i][s], radius, (d.lDisMap, d.rDisMap)[s])
            got.append((d.lDisMap.copy(), d.rDisMap.copy(), [d.jwmf_clusters(s) for s in (0, 1)]))
    finally:
        _close(des)
    singles = _objects(P, pairs, maps)
    try:
        for d, g in zip(singles, got):
            d.JointWMF_GPU(radius, 0.0, n_clusters, max_iter)
            assert np.array_equal(d.lDisMap, g[0]) and np.array_equal(d.rDisMap, g[1])
            for s in (0, 1):
                cen, lok, it = d.jwmf_clusters(s)
                assert it == g[2][s][2] and np.array_equal(cen, g[2][s][0]) and np.array_equal(lok, g[2][s][1])
    finally:
        _close(singles)


def test_group_seams_and_frozen_images(psm):
    """Images that converge inside the first group, exactly at its end and in the second group, in one batch."""
    W, H, nc = 33, 17, 4
    its = [_model(W, H, k, nc)["iterations"] for k in range(8)]
    print("iterations", its)
    assert any(i == JW_GROUP for i in its) and any(i < JW_GROUP for i in its) and any(i > JW_GROUP for i in its), its
    _batch_equals_model_and_singles(psm, W, H, [0, 1, 2, 3], [4, 5, 6, 7], nc, 4)


def test_several_groups_apart(psm):
    """One image needs groups the others sit through frozen."""
    W, H, nc = 40, 30, 4
    its = [_model(W, H, k, nc)["iterations"] for k in range(4)]
    print("iterations", its)
    assert max(its) >= 3 * JW_GROUP and min(its) < 2 * JW_GROUP, its
    _batch_equals_model_and_singles(psm, W, H, [0, 1], [2, 3], nc, 9)


@pytest.mark.parametrize("depth", ["u8", "f32"])
@pytest.mark.parametrize("order", ["short-left", "short-right"])
@pytest.mark.parametrize("W,H,nc,k_short,k_long", [(33, 17, 4, 7, 22), (70, 45, 8, 20, 9)])
def test_unequal_chains_in_one_single_call(psm, W, H, nc, k_short, k_long, order, depth):
    """One image of a single call converges inside the first group of iterations, the other needs more than two groups;
    max_iter 1, 16 and 17 cut one or both chains at and next to the group's end (a cut image reports max_iter)."""
    full = [_model(W, H, k, nc)["iterations"] for k in (k_short, k_long)]
    print("iterations", full)
    assert 0 < full[0] <= JW_GROUP and full[1] > 2 * JW_GROUP, full
    ks = (k_short, k_long) if order == "short-left" else (k_long, k_short)
    pair = tuple(_img(W, H, k) for k in ks)
    if depth == "f32":
        pair = tuple(_as_f32(im) for im in pair)
    maps, radius = _maps(W, H, 50), 4
    for max_iter in (0, 1, 16, 17):
        (de,) = _objects(psm, [pair], [maps])
        try:
            de.JointWMF_GPU(radius, 0.0, nc, max_iter)
            for s, k in enumerate(ks):
                m = _model(W, H, k, nc, max_iter or 10000)
                assert m["iterations"] == min(_model(W, H, k, nc)["iterations"], max_iter or 10000)
                _check_side(de, s, m, maps[s], radius, (de.lDisMap, de.rDisMap)[s])
        finally:
            _close([de])


def test_max_iter_cuts_some_images(psm):
    W, H, nc, cap = 33, 17, 4, 18
    its = [_model(W, H, k, nc)["iterations"] for k in range(8)]
    assert any(i <= cap for i in its) and any(i > cap for i in its), its
    for k in range(8):
        assert _model(W, H, k, nc, cap)["iterations"] == min(its[k], cap)
    _batch_equals_model_and_singles(psm, W, H, [0, 1, 2, 3], [4, 5, 6, 7], nc, 4, max_iter=cap)


@pytest.mark.parametrize("W,H,radius,depth", [(9, 11, 1, "u8"), (9, 11, 16, "u8"), (33, 17, 1, "u8"), (33, 17, 16, "u8"),
                                              (9, 11, 16, "f32"), (33, 17, 1, "f32")])
def test_identity_and_kmeans_in_one_batch(psm, W, H, radius, depth):
    """Context 1 holds a 12-colour pair (every key its own cluster, 0 iterations), contexts 0 and 2 random pairs (k-means)."""
    from primestereomatch_amd import dispest
    nc = 16
    rng = np.random.default_rng(5)
    pal = rng.integers(0, 256, (12, 3), dtype=np.uint8)
    pl, pr = pal[rng.integers(0, 12, (H, W))], pal[rng.integers(0, 12, (H, W))]
    imgs = [(_img(W, H, 0), _img(W, H, 1)), (pl, pr), (_img(W, H, 2), _img(W, H, 3))]
    ms = [[M.clustering_of(im, nc) for im in pair] for pair in imgs]
    assert [m["iterations"] for m in ms[1]] == [0, 0] and all(m["iterations"] > 0 for i in (0, 2) for m in ms[i])
    maps = [_maps(W, H, 10 + i) for i in range(3)]
    pairs = [tuple(_as_f32(im) for im in pair) for pair in imgs] if depth == "f32" else imgs
    des = _objects(psm, pairs, maps)
    try:
        dispest.joint_wmf_batch(des, radius, 0.0, nc, 0)
        for i, d in enumerate(des):
            for s in (0, 1):
                _check_side(d, s, ms[i][s], maps[i][s], radius, (d.lDisMap, d.rDisMap)[s])
    finally:
        _close(des)


def test_sides_that_sit_out(psm):
    from primestereomatch_amd import capi, dispest
    W, H, radius = 70, 45, 5
    pairs = [(_img(W, H, 2 * i), _img(W, H, 2 * i + 1)) for i in range(3)]
    maps = [_maps(W, H, 20 + i) for i in range(3)]
    rng = np.random.default_rng(8)
    host = [((rng.random((n, 3)) * 63).astype(np.float32), rng.integers(0, n, 64 ** 3).astype(np.uint8)) for n in (200, 37, 256, 5, 64, 128)]
    des = _objects(psm, pairs, maps)
    try:
        des[0].set_jwmf_clusters(0, *host[0])                      # context 0: the host's clusters on the left
        des[1].JointWMF_GPU(radius)                                # context 1: clustered by a single call on this pair already
        before = [des[1].jwmf_clusters(s) for s in (0, 1)]
        des[1].upload_maps(*maps[1])
        des[0].set_option(capi.PSM_OPT_PROFILE, 1)
        des[0].reset_kernel_times()
        dispest.joint_wmf_batch(des, radius)
        # m = 3 images (context 0's right, context 2's two): one group of brackets, whatever the number of contexts
        brackets = des[0].kernel_time_ms(capi.PSM_K_JWMF)[1]
        des[0].set_option(capi.PSM_OPT_PROFILE, 0)
        for s in (0, 1):
            cen, lok, it = des[1].jwmf_clusters(s)
            assert it == before[s][2] and it > 0 and np.array_equal(cen, before[s][0]) and np.array_equal(lok, before[s][1])
        cen, lok, it = des[0].jwmf_clusters(0)
        assert it == 0 and np.array_equal(cen, host[0][0]) and np.array_equal(lok, host[0][1])
        its = []
        for i, d in enumerate(des):
            for s in (0, 1):
                cl = host[0] if (i, s) == (0, 0) else None
                ref = M.joint_wmf(maps[i][s], pairs[i][s], radius, clusters=cl)
                assert int(np.count_nonzero((d.lDisMap, d.rDisMap)[s] != ref)) == 0, (i, s)
                its.append(d.jwmf_clusters(s)[2])
        groups = -(-max(its[1], its[4], its[5]) // JW_GROUP)
        assert brackets == 2 + groups + 2, (brackets, its)         # keys, seeding, the groups, clusters, median
        # host clusters on all six sides, asynchronous: no image to cluster, nothing to wait for
        for i, d in enumerate(des):
            d.setInputImages(*pairs[i])
            for s in (0, 1):
                d.set_jwmf_clusters(s, *host[2 * i + s])
            d.upload_maps(*maps[i])
        des[0].set_option(capi.PSM_OPT_ASYNC, 1)
        dispest.joint_wmf_batch(des, radius)
        des[0].synchronize()
        for i, d in enumerate(des):
            for s in (0, 1):
                ref = M.joint_wmf(maps[i][s], pairs[i][s], radius, clusters=host[2 * i + s])
                assert int(np.count_nonzero((d.lDisMap, d.rDisMap)[s] != ref)) == 0, (i, s)
    finally:
        _close(des)


def test_batch_of_one_and_reuse(psm):
    from primestereomatch_amd import capi, dispest
    W, H, nc, radius = 33, 17, 16, 4
    pair, maps = (_img(W, H, 0), _img(W, H, 1)), _maps(W, H, 30)
    a, b = _objects(psm, [pair, pair], [maps, maps])
    try:
        dispest.joint_wmf_batch([a], radius, 0.0, nc, 0)
        b.JointWMF_GPU(radius, 0.0, nc, 0)
        assert np.array_equal(a.lDisMap, b.lDisMap) and np.array_equal(a.rDisMap, b.rDisMap)
        first = a.lDisMap.copy(), a.rDisMap.copy()
        cl = [a.jwmf_clusters(s) for s in (0, 1)]
        for s in (0, 1):
            cen, lok, it = b.jwmf_clusters(s)
            assert it == cl[s][2] and it > 0 and np.array_equal(cen, cl[s][0]) and np.array_equal(lok, cl[s][1])
        # a later single call on the batch's member: clustering and tables reused (one bracket: planes + median)
        a.set_option(capi.PSM_OPT_PROFILE, 1)
        a.reset_kernel_times()
        a.upload_maps(*maps)
        a.JointWMF_GPU(radius, 0.0, nc, 0)
        assert a.kernel_time_ms(capi.PSM_K_JWMF)[1] == 1
        assert np.array_equal(a.lDisMap, first[0]) and np.array_equal(a.rDisMap, first[1])
        assert [a.jwmf_clusters(s)[2] for s in (0, 1)] == [cl[0][2], cl[1][2]]
        # ... and a later batch on it too
        a.reset_kernel_times()
        a.upload_maps(*maps)
        dispest.joint_wmf_batch([a], radius, 0.0, nc, 0)
        assert a.kernel_time_ms(capi.PSM_K_JWMF)[1] == 1
        assert np.array_equal(a.lDisMap, first[0]) and np.array_equal(a.rDisMap, first[1])
    finally:
        _close([a, b])


def test_refusals_leave_the_maps(psm):
    from primestereomatch_amd import capi, dispest, synth
    W, H, D = 96, 40, 16
    l, r, _ = synth.make_pair(W, H, D, seed=5)
    l2, r2, _ = synth.make_pair(W + 1, H, D, seed=5)
    maps = [np.random.default_rng(40 + i).integers(0, D, (2, H, W), dtype=np.uint8) for i in range(2)]
    des = _objects(psm, [(l, r), (r, l)], maps, D=D)
    bad = {}
    try:
        dispest.joint_wmf_batch(des)
        earlier = [(d.lDisMap.copy(), d.rDisMap.copy()) for d in des]
        clusters = [[d.jwmf_clusters(s) for s in (0, 1)] for d in des]
        bad["width"] = psm.DispEst(l2, r2, D)
        bad["width"].upload_maps(*np.zeros((2, H, W + 1), np.uint8))
        bad["depth"] = psm.DispEst(_as_f32(l), _as_f32(r), D)
        bad["depth"].upload_maps(*maps[0])
        bad["no maps"] = psm.DispEst(l, r, D)
        bad["stripe"] = psm.DispEst(l, r, D)
        bad["stripe"].set_rows(0, H // 2)
        bad["stripe"].CostConst_GPU(); bad["stripe"].CostFilter_GPU(); bad["stripe"].DispSelect_GPU()
        cases = [("twice", des + [des[0]], {}), ("width", des + [bad["width"]], {}), ("depth", des + [bad["depth"]], {}),
                 ("no maps", des + [bad["no maps"]], {}), ("stripe", des + [bad["stripe"]], {}),
                 ("radius", des, {"radius": 17}), ("n_clusters", des, {"n_clusters": 257})]
        for name, members, kw in cases:
            with pytest.raises(capi.PsmError, match="joint_wmf_batch"):
                dispest.joint_wmf_batch(members, **kw)
            for d, e, cl in zip(des, earlier, clusters):
                lm, rm = d.download_maps()
                assert np.array_equal(lm, e[0]) and np.array_equal(rm, e[1]), name
                for s in (0, 1):
                    cen, lok, it = d.jwmf_clusters(s)
                    assert it == cl[s][2] and np.array_equal(cen, cl[s][0]) and np.array_equal(lok, cl[s][1]), name
        lib = capi.load()
        import ctypes as C
        arr = (C.c_void_p * 2)(des[0]._h, None)
        assert lib.psm_joint_wmf_batch(arr, 2, 0, 0.0, 0, 0) != 0
        assert lib.psm_joint_wmf_batch(arr, 0, 0, 0.0, 0, 0) != 0 and lib.psm_joint_wmf_batch(arr, 4097, 0, 0.0, 0, 0) != 0
    finally:
        _close(des + list(bad.values()))


def test_middlebury_through_the_harness(psm):
    from primestereomatch_amd import dispest, harness
    names = ["cones", "teddy"]
    pair = [dict(np.load(os.path.join(GOLDEN, f"{n}_pair.npz"))) for n in names]
    gold = [dict(np.load(os.path.join(GOLDEN, f"{n}_oracle_d64.1.npz"))) for n in names]
    fx = [dict(np.load(os.path.join(GOLDEN, f"{n}_jwmf.npz"))) for n in names]
    outs = harness.compute_batch([(p["l_bgr"], p["r_bgr"]) for p in pair], 64, [p["gt_l"] for p in pair], [p["occl"] for p in pair],
                                 joint_wmf=True)
    assert len(outs) == 2
    for n, p, g, f, out in zip(names, pair, gold, fx, outs):
        assert np.array_equal(out["lDisMap_raw"], g["ldisp"]) and np.array_equal(out["rDisMap_raw"], g["rdisp"]), n
        assert int(np.count_nonzero(out["lDisMap"] != f["lmap"])) == 0 and int(np.count_nonzero(out["rDisMap"] != f["rmap"])) == 0, n
        assert out["bp_percent"] == harness.error_vs_ground_truth(f["lmap"], p["gt_l"], p["occl"], 64, 4, 4)[0], n
        print(f"{n}: %BP after JointWMF {out['bp_percent']:.2f}")
    des = _objects(psm, [(p["l_bgr"], p["r_bgr"]) for p in pair], [(g["ldisp"], g["rdisp"]) for g in gold], D=64)
    try:
        dispest.joint_wmf_batch(des)
        for n, f, d in zip(names, fx, des):
            for s, k in ((0, "l"), (1, "r")):
                cen, lok, it = d.jwmf_clusters(s)
                assert it == int(f[f"{k}_iterations"]), (n, s)
                assert np.array_equal(cen, f[f"{k}_centres"]) and np.array_equal(lok, f[f"{k}_lok"]), (n, s)
                assert np.array_equal((d.lDisMap, d.rDisMap)[s], f[f"{k}map"]), (n, s)
        print("Lloyd iterations", [[d.jwmf_clusters(s)[2] for s in (0, 1)] for d in des])
    finally:
        _close(des)
