"""CPU: the model of psm_joint_wmf (tests/jwmf_model.py) against the definition in Python integers, its clustering's
properties, and the binding of the new entry points (include/primesm_hip.h <-> capi.py)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jwmf_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("W,H,r,n", [(8, 8, 3, 4), (9, 11, 2, 256), (7, 9, 16, 1), (12, 5, 1, 16), (10, 10, 4, 3)])
def test_median_equals_brute_force(W, H, r, n):
    rng = np.random.default_rng(W * H + r)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    d = rng.integers(0, 256, (H, W), dtype=np.uint8)
    m = M.clustering_of(img, n)
    wq = M.quantise(M.weight_table(m["centres"]))
    assert np.array_equal(M.median(d, m["F"], wq, r), M.brute_median(d, m["F"], wq, r))


def test_exact_ties_take_the_lower_value():
    """Uniform colour: every weight is 1 (2^48).  Columns alternate 10 / 20: a clipped window with as many 10s as 20s is an
    exact tie (2 * W(<=10) == W(total)), which the rule W(<=c) >= W(>c) resolves to 10."""
    H, W, r = 6, 6, 1
    img = np.full((H, W, 3), 77, np.uint8)
    d = np.where(np.arange(W)[None, :] % 2 == 0, 10, 20).astype(np.uint8).repeat(H, 0)
    m = M.clustering_of(img)
    assert len(m["samples"]) == 1 and m["iterations"] == 0
    wq = M.quantise(M.weight_table(m["centres"]))
    assert wq[0, 0] == 1 << 48
    out = M.median(d, m["F"], wq, r)
    assert np.array_equal(out, M.brute_median(d, m["F"], wq, r))
    assert out[0, 0] == 10 and out[3, 0] == 10      # window columns 0, 1: as many 10s as 20s - a tie
    assert out[3, 2] == 20 and out[3, 1] == 10      # columns 1..3: 20, 10, 20; columns 0..2: 10, 20, 10


def test_feature_of_float_images_recovers_the_bytes():
    """convertTo(CV_8UC3, 255) of u8 * (1/255.0f) gives the bytes back; out-of-range values saturate."""
    v = np.arange(256, dtype=np.uint8).reshape(1, -1, 1).repeat(3, 2)
    f = v.astype(np.float32) * np.float32(1 / 255.0)
    assert np.array_equal(M.feature_u8(f), v)
    odd = np.array([[[-0.5, 1.7, np.nan]]], np.float32)
    assert M.feature_u8(odd).tolist() == [[[0, 255, 0]]]


def test_weight_table_is_the_reference_formula():
    cen = np.array([[0, 0, 0], [1.5, 2, 3], [63, 63, 63]], np.float32)
    w = M.weight_table(cen)
    assert w.dtype == np.float32 and np.array_equal(w, w.T) and np.all(np.diag(w) == 1)
    ns = np.float32(np.float32(25.5) / np.float32(256)) * np.float32(64)
    div = np.float32(1) / (np.float32(2) * ns * ns)
    assert w[0, 1] == np.float32(M.expf(float(-np.float32(np.float32(2.25 + 4) + 9) * div)))
    assert w[0, 2] == 0                     # exp(-146.5) underflows
    assert M.quantise(w)[0, 1] == int(np.rint(np.float64(w[0, 1]) * 2.0 ** 48))


def test_clustering_identity_when_few_keys():
    rng = np.random.default_rng(3)
    pal = rng.integers(0, 256, (200, 3), dtype=np.uint8)
    img = pal[rng.integers(0, 200, (40, 50))]
    m = M.clustering_of(img)
    assert m["iterations"] == 0 and len(m["centres"]) == len(m["samples"]) <= 200
    assert np.array_equal(m["labels"], np.arange(len(m["samples"])))
    assert np.array_equal(m["centres"], M.key_xyz(m["samples"]).astype(np.float32))


def test_clustering_deterministic_fixed_point():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)
    a, b = M.clustering_of(img, 64), M.clustering_of(img, 64)
    assert a["iterations"] == b["iterations"] and np.array_equal(a["centres"], b["centres"]) and np.array_equal(a["lok"], b["lok"])
    assert len(a["centres"]) == 64 and 0 < a["iterations"] < 10000
    xyz = M.key_xyz(a["samples"]).astype(np.float32)
    assert np.array_equal(M._assign(xyz, a["centres"]), a["labels"])
    # max_iter bounds the Lloyd loop
    c = M.clustering_of(img, 64, max_iter=2)
    assert c["iterations"] == 2


def test_cones_left_clustering_as_recorded():
    """The default clustering of the Cones left image: 31 109 distinct keys, 77 Lloyd assignments to the fixed point."""
    pair = np.load(os.path.join(ROOT, "tests", "golden", "cones_pair.npz"))
    m = M.clustering_of(pair["l_bgr"])
    assert len(m["samples"]) == 31109 and len(m["centres"]) == 256
    assert m["iterations"] == 77


def test_entry_points_declared_and_bound():
    from primestereomatch_amd import capi, harness
    hdr = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"PSM_K_JWMF = 12, PSM_K_COUNT = 13", hdr)
    assert capi.PSM_K_JWMF == 12
    names = {n for n, _, _ in capi.SYMBOLS}
    assert {"psm_joint_wmf", "psm_joint_wmf_set_clusters", "psm_joint_wmf_clusters"} <= names
    for n in ("psm_joint_wmf", "psm_joint_wmf_set_clusters", "psm_joint_wmf_clusters"):
        assert re.search(r"\bint %s\(" % n, hdr)
    assert inspect.signature(harness.compute).parameters["joint_wmf"].default is False
