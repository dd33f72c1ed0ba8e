"""CPU-only checks of tests/wls_model.py, the definition of the WLS smoothing stage (psm_wls_filter): the Thomas recurrence against a
dense solve, the cases whose answer is known without arithmetic, and what the filter does to the committed SGM maps of Cones and
Teddy."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import wls_model as M
from conftest import GOLDEN


def rnd(seed):
    return np.random.default_rng(seed)


def dense_pass(x, lw):
    """(I + A) u = x for every line: A the weighted graph Laplacian of the line's links, solved densely in float64"""
    L, N = x.shape
    u = np.empty((L, N))
    for i in range(L):
        A = np.eye(N)
        for n in range(N - 1):
            w = lw[i, n]
            A[n, n] += w
            A[n + 1, n + 1] += w
            A[n, n + 1] -= w
            A[n + 1, n] -= w
        u[i] = np.linalg.solve(A, x[i])
    return u


@pytest.mark.parametrize("W,H", ((9, 8), (8, 13)))
def test_the_recurrence_in_float64_equals_a_dense_solve_of_every_pass(W, H):
    """The condition number of I + lam_t A is at most 1 + 4 lam_0, about 1.2e4 at the defaults, so the Thomas error is about
    3e-12 of the largest element; the bound sits four orders above that."""
    r = rnd(W)
    guide = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    guide[:, : W // 2] //= 64                                    # half of the image with strong links
    v = r.integers(0, 16 * 64, (H, W)).astype(np.int16)
    v[r.random((H, W)) < 0.3] = -16
    kh, kv = M.links(guide)
    tab = M.table(M.DEFAULTS["sigma"]).astype(np.float64)
    pl = M.start(v, -16).astype(np.float64)
    ref = pl.copy()
    for lam_t in M.lambdas(M.DEFAULTS["lam"], M.DEFAULTS["iterations"]):
        lam_t = np.float64(lam_t)
        lwh, lwv = lam_t * tab[kh[:, :-1]], lam_t * tab[kv[:-1, :].T]
        pl = M.solve_lines(pl, lwh, np.float64)
        ref = np.stack([dense_pass(p, lwh) for p in ref])
        assert np.abs(pl - ref).max() <= 1e-9 * np.abs(ref).max()
        pl = M.solve_lines(pl.transpose(0, 2, 1), lwv, np.float64).transpose(0, 2, 1)
        ref = np.stack([dense_pass(p.T, lwv).T for p in ref])
        assert np.abs(pl - ref).max() <= 1e-9 * np.abs(ref).max()
    whole = M.smooth(v, -16, guide, dtype=np.float64)             # the same passes as smooth() runs them
    assert np.abs(whole - ref).max() <= 1e-9 * np.abs(ref).max()


def test_the_table_and_the_lambdas():
    tab = M.table(1.5)
    assert tab.dtype == np.float32 and tab.shape == (256,) and tab[0] == 1.0 and (np.diff(tab) <= 0).all()
    assert tab[1] == np.float32(math.exp(-1 / 1.5)) and tab[255] == 0.0 and 0.0 < tab[140] < np.finfo(np.float32).tiny      # subnormal weights exist
    for T in (1, 2, 3, 4):
        lams = M.lambdas(8000.0, T)
        assert len(lams) == T and all(isinstance(v, np.float32) for v in lams)
        assert abs(float(sum(float(v) for v in lams)) - 4000.0) < 1e-3            # they sum to lambda / 2 ...
        assert all(abs(float(a) / float(b) - 4.0) < 1e-6 for a, b in zip(lams, lams[1:]))      # ... and fall by 4


def test_a_line_of_one_pixel_is_the_identity():
    x = rnd(1).normal(size=(2, 5, 1)).astype(np.float32)
    u = M.solve_lines(x, np.zeros((5, 0), np.float32))
    assert np.array_equal(u.view(np.uint32), x.view(np.uint32))
    v = np.array([[7, -16, 300, -32768, 32767]], np.int16).T      # a 1 x 5 ... and a 5 x 1 image through the whole filter
    for img in (v, v.T.copy()):
        out = M.wls(img, -16, np.zeros(img.shape + (3,), np.uint8), iterations=1)
        assert out["disp"].shape == img.shape


def test_an_all_invalid_map_gives_all_inv():
    g = rnd(2).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    for inv in (-16, 64, -64):
        out = M.wls(np.full((9, 11), inv, np.int16), inv, g)
        assert (out["disp"] == inv).all() and (out["q"].view(np.uint32) == M.VOID_BITS).all() and (out["den"] == 0).all()


def test_one_valid_pixel_on_a_flat_guide_gives_its_value_everywhere():
    v = np.full((12, 17), -16, np.int16)
    v[5, 9] = 555
    out = M.wls(v, -16, np.full((12, 17, 3), 90, np.uint8))
    assert (out["disp"] == 555).all() and (out["den"] > 0).all()
    assert np.abs(out["den"].sum() - 1.0) < 1e-3                   # the passes preserve mass


def test_a_wall_in_the_guide_gives_inv_beyond_it():
    H, W = 10, 24
    g = np.full((H, W, 3), 90, np.uint8)
    g[:, :14, 1], g[:, 14:, 1] = 0, 255                            # a 0 / 255 step in one channel: tab[255] == 0
    v = np.full((H, W), -16, np.int16)
    v[:, :14] = rnd(3).integers(0, 900, (H, 14))
    out = M.wls(v, -16, g)
    assert (out["disp"][:, 14:] == -16).all() and (out["disp"][:, :14] != -16).all()
    assert (out["den"][:, 14:] == 0).all()
    gray = g[..., 1]                                               # the same wall as a one-channel guide
    assert np.array_equal(M.wls(v, -16, gray)["disp"], out["disp"])


def test_the_extremes_stay_in_range():
    g = np.full((9, 14, 3), 7, np.uint8)
    r = rnd(4)
    for inv in (-16, 64):
        for ext in (32767, -32768):
            v = np.where(r.random((9, 14)) < 0.3, inv, ext).astype(np.int16)
            out = M.wls(v, inv, g)
            assert out["disp"].dtype == np.int16 and (out["disp"] != inv).all()
            assert (out["disp"] == (32767 if ext > 0 else inv + 1)).all()       # clamped to inv + 1 from below: never taken for a hole
        mixed = r.choice(np.array([-32768, 32767, inv], np.int16), (9, 14))
        out = M.wls(mixed, inv, g)
        assert out["disp"].min() >= inv + 1 and out["disp"].max() <= 32767


def test_the_gif_source_and_the_rounded_reading():
    lmap = np.array([[0, 1, 63, 255]], np.uint8)
    v, inv = M.gif_source(lmap)
    assert inv == -16 and v.tolist() == [[0, 16, 1008, 4080]]
    v, _ = M.gif_source(lmap, np.array([[255, 0, 1, 0]], np.uint8))
    assert v.tolist() == [[0, -16, 1008, -16]]
    assert M.rounded_u8(np.array([-16, 0, 7, 8, 23, 24, 32767], np.int16)).tolist() == [0, 0, 0, 1, 1, 2, 255]


@pytest.mark.parametrize("name", ("cones", "teddy"))
def test_golden_sgm_maps_with_the_defaults(golden, name):
    from primestereomatch_amd import harness
    p, g, want = golden(f"{name}_pair.npz"), golden(f"{name}_sgm.npz"), golden(f"{name}_wls.npz")
    out = M.wls(g["disp"], -16, p["l_bgr"])
    assert np.array_equal(out["disp"], want["disp"])
    metric = lambda m: harness.error_vs_ground_truth(m, p["gt_l"], p["occl"], 64, 4, 4)[0]
    bp_int = metric(np.maximum(g["disp"], 0) >> 4)
    bp_wls = metric(M.rounded_u8(out["disp"]))
    print(name, "bp_percent_int", bp_int, "bp_percent_wls", bp_wls, "void", int((out["disp"] == -16).sum()))
    assert bp_wls < bp_int                                          # (Cones 5.56 < 9.20, Teddy 11.94 < 13.90)
    assert bp_wls == float(want["bp_percent_wls"])
    void = int((out["disp"] == -16).sum())
    assert void == int(want["void"]) and void < 0.01 * out["disp"].size      # (395 and 336 of 168 750)
    assert (g["disp"] == -16).mean() > 0.09                         # ... of the 9 to 10 % the SGM map had
    man = json.load(open(os.path.join(GOLDEN, "manifest_wls.json")))[name.capitalize()]["wls"]
    assert man["sha256"]["disp"] == hashlib.sha256(out["disp"].tobytes()).hexdigest()
    assert man["sha256"]["q"] == hashlib.sha256(out["q"].tobytes()).hexdigest()
    assert (man["lambda"], man["sigma"], man["iterations"]) == (8000.0, 1.5, 3) and man["void"] == void
