"""CPU: the model of psm_joint_wmf (tests/jwmf_model.py) against a serial restatement of the reference's own method
(tests/jwmf_reading.c: filterCore's column scan with the float balanceWeight and its necklace order).  Equal on every pixel
except near-ties: where they differ, some disparity between the two answers balances the window to within 1e-3, so the
reference's float walk decides by its own rounding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jwmf_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="session")
def reading(tmp_path_factory):
    return M.load_reading(str(tmp_path_factory.mktemp("jwmf_reading")))


def _compare(reading, dmap, F, w, r, what):
    ref = M.reading_core(reading, dmap, F, w, r)
    mod = M.median(dmap, F, M.quantise(w), r)
    diff = np.argwhere(ref != mod)
    for y, x in diff:
        assert M.near_tie(dmap, F, w, r, y, x, int(ref[y, x]), int(mod[y, x])), (what, y, x, ref[y, x], mod[y, x])
    print(f"{what}: {len(diff)} of {dmap.size} pixels differ, all near-ties")
    return len(diff)


@pytest.mark.parametrize("W,H,r,n", [(8, 8, 9, 256), (9, 11, 16, 16), (33, 17, 4, 16), (40, 30, 1, 3), (64, 48, 9, 256)])
def test_model_equals_reading_random(reading, W, H, r, n):
    rng = np.random.default_rng(W + H + r)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    d = rng.integers(0, 256, (H, W), dtype=np.uint8)
    m = M.clustering_of(img, n)
    _compare(reading, d, m["F"], M.weight_table(m["centres"]), r, f"{W}x{H} r={r} n={n}")


def test_model_equals_reading_uniform_colour(reading):
    """One cluster: all weights 1, exact ties everywhere the window holds as many taps on either side."""
    img = np.full((12, 10, 3), 40, np.uint8)
    d = np.where(np.arange(10)[None, :] % 2 == 0, 3, 9).astype(np.uint8).repeat(12, 0)
    m = M.clustering_of(img)
    assert _compare(reading, d, m["F"], M.weight_table(m["centres"]), 2, "uniform") == 0


@pytest.mark.parametrize("name", ["cones", "teddy"])
def test_model_equals_reading_middlebury(reading, name):
    """The committed fixtures' clustering (tests/golden/<name>_jwmf.npz) on the committed oracle maps, both sides."""
    pair = np.load(os.path.join(GOLDEN, f"{name}_pair.npz"))
    gold = np.load(os.path.join(GOLDEN, f"{name}_oracle_d64.1.npz"))
    fx = np.load(os.path.join(GOLDEN, f"{name}_jwmf.npz"))
    for s, img, dmap in (("l", pair["l_bgr"], gold["ldisp"]), ("r", pair["r_bgr"], gold["rdisp"])):
        F = fx[f"{s}_lok"][M.keys_of(img)]
        w = M.weight_table(fx[f"{s}_centres"])
        _compare(reading, dmap, F, w, 9, f"{name} {s}")
        assert np.array_equal(M.median(dmap, F, M.quantise(w), 9), fx[f"{s}map"])


def test_reading_identity_matches_model(reading):
    """A palette image (at most 256 keys): the reading's own keys, identity clustering and expf table, then the scan."""
    rng = np.random.default_rng(11)
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    img = pal[rng.integers(0, 256, (50, 60))]
    d = rng.integers(0, 64, (50, 60), dtype=np.uint8)
    out, nf = M.reading_identity(reading, img, d)
    m = M.clustering_of(img)
    assert nf == len(m["samples"]) and m["iterations"] == 0
    mod = M.joint_wmf(d, img)
    w = M.weight_table(m["centres"])
    for y, x in np.argwhere(out != mod):
        assert M.near_tie(d, m["F"], w, 9, y, x, int(out[y, x]), int(mod[y, x]))
    # more than 256 keys: the reading refuses (its clustering would be the reference's random one)
    assert M.reading_identity(reading, rng.integers(0, 256, (40, 40, 3), dtype=np.uint8), d[:40, :40])[1] == -1
