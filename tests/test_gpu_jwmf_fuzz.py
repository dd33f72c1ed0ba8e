"""-m gpu seeded sweep of the joint weighted median (psm_joint_wmf, psm_joint_wmf_batch) against the numpy model
tests/jwmf_model.py: the clustering (iterations, centres, label_of_key) and both maps of every context, 0 differing elements
everywhere.  The cases come from tests/fuzz_inputs.py (their conditions are held by tests/test_fuzz_inputs.py on the CPU):

  * sizes around JW_TILE = 16 in both directions, every radius 1 .. 16, n_clusters such as 2, 3, 255 and anything between
  * images with exactly n_clusters and n_clusters + 1 distinct keys (the identity / k-means switch), two colours, and random
    bytes with more than 1024 keys (chunk = 2 in jw_seed, the last owner's partial chunk)
  * maps with one value, only 0 and 255, one high nibble, a ramp: the two radix passes with empty digits
  * a sigma that sends every cross-cluster weight to 0, and one that sends every weight to (nearly) 2^48
  * float images with values outside [0, 1], infinities and NaN
  * the left and the right side of a context always of different kinds"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_inputs as F  # noqa: E402
import jwmf_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def sigma_of(sigma):
    return sigma or 25.5                               # 0: the reference's value


def check_side(name, de, side, img, dmap, case, host=None):
    """One side of a context after the filter: its clustering against the model's (or the host's own), its map against the
    model's median -> the count of differing map elements, asserted 0."""
    W, H, radius, nc, depth, ik, mk, sigma, seed = case
    cen, lok, it = de.jwmf_clusters(side)
    if host is None:
        m = M.clustering_of(img, nc)
        assert it == m["iterations"], (name, it, m["iterations"])
        assert np.array_equal(cen, m["centres"]), name
        assert np.array_equal(lok, m["lok"]), name
        centres, Fp = m["centres"], m["F"]
    else:
        assert it == 0 and np.array_equal(cen, host[0]) and np.array_equal(lok, host[1]), name
        centres, Fp = host[0], host[1][M.keys_of(M.feature_u8(img))]
    ref = M.median(dmap, Fp, M.quantise(M.weight_table(centres, sigma_of(sigma))), radius)
    out = (de.lDisMap, de.rDisMap)[side]
    n = int(np.count_nonzero(out != ref))
    print(f"[jwmf-fuzz] {name} side {side} ({ik[side]}, {mk[side]}): {len(centres)} clusters, {it} iterations, "
          f"{int(np.count_nonzero(ref != dmap))} pixels changed, differing elements {n}")
    assert n == 0, (name, np.argwhere(out != ref)[:8].tolist())
    return out.copy(), (cen, lok, it)


@pytest.mark.parametrize("case", F.jw_cases(), ids=lambda c: f"{c[0]}x{c[1]}-r{c[2]}-n{c[3]}-{c[4]}-{c[5][0]}-{c[5][1]}-{c[6][0]}-{c[6][1]}-s{c[7]:g}")
def test_random_cases(psm, case):
    W, H, radius, nc, depth, ik, mk, sigma, seed = case
    imgs, maps = F.jwmf_build(case)
    with psm.DispEst(imgs[0], imgs[1], 8) as de:       # (max_disp only sizes the volumes, which the filter never touches)
        de.upload_maps(*maps)
        de.JointWMF_GPU(radius, sigma, nc, 0)
        de.synchronize()
        for side in (0, 1):
            check_side(f"{W}x{H} r {radius} n {nc} {depth} sigma {sigma:g}", de, side, imgs[side], maps[side], case)


@pytest.mark.parametrize("batch", F.jwmf_batches(6, 2718), ids=lambda b: f"{len(b)}of{b[0][0][0]}x{b[0][0][1]}-r{b[0][0][2]}-n{b[0][0][3]}-{b[0][0][4]}")
def test_random_batches(psm, batch):
    """2 to 4 contexts of one geometry with kinds of their own, some sides with clusters from the host: every context equals the
    model and its own single call."""
    from primestereomatch_amd import dispest
    W, H, radius, nc, depth, _, _, sigma, _ = batch[0][0]
    built = [F.jwmf_build(case) for case, _ in batch]
    hosts = [[F.host_clusters(case[8] + side) if flag else None for side, flag in enumerate(host)] for case, host in batch]

    def contexts():
        des = [psm.DispEst(imgs[0], imgs[1], 8) for imgs, _ in built]
        for de, (_, maps), hs in zip(des, built, hosts):
            de.upload_maps(*maps)
            for side, h in enumerate(hs):
                if h is not None:
                    de.set_jwmf_clusters(side, *h)
        return des

    des = contexts()
    try:
        dispest.joint_wmf_batch(des, radius, sigma, nc, 0)
        got = [[check_side(f"batch of {len(batch)} context {i}", de, side, built[i][0][side], built[i][1][side], batch[i][0], hosts[i][side])
                for side in (0, 1)] for i, de in enumerate(des)]
    finally:
        for de in des:
            de.close()
    singles = contexts()
    try:
        for de, g in zip(singles, got):
            de.JointWMF_GPU(radius, sigma, nc, 0)
            de.synchronize()
            for side in (0, 1):
                cen, lok, it = de.jwmf_clusters(side)
                out, (bcen, blok, bit) = g[side]
                assert np.array_equal((de.lDisMap, de.rDisMap)[side], out)
                assert it == bit and np.array_equal(cen, bcen) and np.array_equal(lok, blok)
    finally:
        for de in singles:
            de.close()
