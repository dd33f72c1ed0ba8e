"""CPU-only checks of the surface of the score stage (psm_score: display maps and the error metric on the device): the built
library exports the symbols, capi declares them and the record, the argument checks answer without a device and carry messages,
the Python layers reach the calls, and the C++ host (DispEst::Score, psm_demo's score option) still builds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("psm_score_set_truth", "psm_score_clear_truth", "psm_score_set_params", "psm_score", "psm_score_wait",
         "psm_score_download", "psm_score_batch", "psm_score_time", "psm_score_upload_sgm_map")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_library_exports_the_symbols(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}\b", out), name
    for kernel in ("k_sc_minmax", "k_sc_score"):                   # the stage's own device code is in the library
        assert kernel.encode() in open(built.LIB_PATH, "rb").read()


def test_capi_declares_them_and_the_record(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    for name in NAMES:
        assert decl[name][0] is C.c_int and hasattr(built.load(), name)
    assert decl["psm_score"][1] == [C.c_void_p, C.c_int, C.POINTER(built.Score)]
    assert decl["psm_score_set_params"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_int]
    # struct psm_score { int32 min_val, max_val; uint32 pixels, bad; uint64 err_sum; int32 unit; uint32 flags; }
    assert [(n, C.sizeof(t)) for n, t in built.Score._fields_] == [("min_val", 4), ("max_val", 4), ("pixels", 4), ("bad", 4),
                                                                    ("err_sum", 8), ("unit", 4), ("flags", 4)]
    assert C.sizeof(built.Score) == 32 and built.Score.err_sum.offset == 16
    assert (built.PSM_SCORE_GIF, built.PSM_SCORE_SGM, built.PSM_SCORE_SGM_INT) == (0, 1, 2)
    assert (built.PSM_MASK_NONE, built.PSM_MASK_NONOCC, built.PSM_MASK_DISC, built.PSM_SCORE_FLAT) == (0, 1, 2, 1)
    rec = built.Score(min_val=-16, max_val=1000, pixels=200, bad=50, err_sum=300, unit=3, flags=0).as_dict()
    assert rec["bp_percent"] == 25.0 and rec["avg_err"] == (300 / 200) / 3
    assert built.Score(pixels=4, bad=1, err_sum=9, unit=0).as_dict()["avg_err"] == 0.0


def test_null_context_is_refused_with_a_message(built):
    lib = built.load()
    rec = built.Score()
    calls = {
        "psm_score_set_truth": (None, None, None, 0), "psm_score_clear_truth": (None,), "psm_score_set_params": (None, 4, 4, 1),
        "psm_score": (None, 0, C.byref(rec)), "psm_score_wait": (None, C.byref(rec)),
        "psm_score_download": (None, None, None, None, 0), "psm_score_time": (None, None),
        "psm_score_upload_sgm_map": (None, None, 0),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        msg = built.last_error(None)
        assert msg.startswith(name + ":") and "NULL" in msg, (name, msg)
    assert lib.psm_score_batch(None, 3, 0, None) != 0 and "psm_score_batch" in built.last_error(None)
    arr = (C.c_void_p * 2)(None, None)
    assert lib.psm_score_batch(arr, 2, 0, None) != 0 and "psm_score_batch" in built.last_error(None)


def test_out_of_range_parameters_are_refused_without_a_device(built):
    """(on a context the same messages are psm_last_error(ctx)'s: tests/test_gpu_score.py)"""
    lib = built.load()
    for ok in ((1, 0, 0), (255, 255, 2), (4, 4, 1)):
        assert lib.psm_score_set_params(None, *ok) != 0 and "NULL" in built.last_error(None)      # in range: only the context is missing
    for bad in (0, -1, 256, 1 << 20):
        assert lib.psm_score_set_params(None, bad, 4, 1) != 0
        msg = built.last_error(None)
        assert "scale_factor" in msg and str(bad) in msg and "[1, 255]" in msg
    for bad in (-1, 256):
        assert lib.psm_score_set_params(None, 4, bad, 1) != 0
        msg = built.last_error(None)
        assert "error_threshold" in msg and str(bad) in msg and "[0, 255]" in msg
    for bad in (-1, 3):
        assert lib.psm_score_set_params(None, 4, 4, bad) != 0
        msg = built.last_error(None)
        assert "mask_mode" in msg and str(bad) in msg and "PSM_MASK_DISC" in msg


class _Recorder:
    """stands where the loaded library stands in a DispEst: every psm_* call is recorded and succeeds; psm_score leaves the
    record of an 8 x 12 image with nothing wrong"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args[1:]))
            if name == "psm_score":
                args[2]._obj.pixels, args[2]._obj.unit = 96, 1
            return 0
        return call


def _fake(dispest, maxDis=64, W=12, H=8):
    de = object.__new__(dispest.DispEst)
    de._lib, de._h, de.wid, de.hei, de.maxDis, de.options = _Recorder(), 1, W, H, maxDis, {}
    return de


def test_the_python_layer_reaches_the_calls(built):
    from primestereomatch_amd import dispest
    de = _fake(dispest)
    gt = np.zeros((8, 12), np.uint8)
    de.set_truth(gt, gt)
    de.set_score_params(3, 7, built.PSM_MASK_DISC)
    rec = de.Score_GPU(built.PSM_SCORE_SGM)
    assert (rec["pixels"], rec["bp_percent"], rec["avg_err"]) == (96, 0.0, 0.0)
    assert set(rec) >= {"min_val", "max_val", "pixels", "bad", "err_sum", "unit", "flags", "bp_percent", "avg_err"}
    l, e = de.score_maps()
    assert l.shape == e.shape == (8, 12) and l.dtype == np.uint8 and len(de.score_maps(right=True)) == 3
    names = [n for n, _ in de._lib.calls]
    assert names[:3] == ["psm_score_set_truth", "psm_score_set_params", "psm_score"] and "psm_score_download" in names
    assert ("psm_score_set_params", (3, 7, 2)) in de._lib.calls
    with pytest.raises(ValueError):
        de.set_truth(np.zeros((8, 13), np.uint8))
    with pytest.raises(ValueError):
        de.upload_sgm_map(np.zeros((8, 12), np.uint8))
    assert dispest.score_batch([]) == []
    p = inspect.signature(dispest.FrameRing.__init__).parameters
    assert p["truth"].default is None and p["scale_factor"].default == 4 and p["error_threshold"].default == 4


def test_the_harness_keeps_the_numpy_tail_as_the_default(built):
    from primestereomatch_amd import harness
    for f in (harness.compute, harness.compute_batch, harness.compute_sgbm, harness.compute_sgbm_batch):
        assert inspect.signature(f).parameters["device_tail"].default is False
        assert "device_tail" in f.__doc__


def test_the_header_declares_the_stage():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"int psm_score\(psm_ctx \*ctx, int source, struct psm_score \*out\);", text)
    assert re.search(r"struct psm_score \{\s*int32_t min_val, max_val;.*?uint32_t pixels, bad;.*?uint64_t err_sum;.*?int32_t unit;.*?uint32_t flags;",
                     text, flags=re.S)
    for phrase in ("PSM_SCORE_GIF = 0, PSM_SCORE_SGM = 1, PSM_SCORE_SGM_INT = 2", "PSM_MASK_NONE = 0, PSM_MASK_NONOCC = 1, PSM_MASK_DISC = 2",
                   "PSM_SCORE_FLAT", "survive psm_release_scratch", "tests/score_model.py"):
        assert phrase in text, phrase


def test_host_demo_builds_with_the_stage(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    hdr = open(os.path.join(host, "DispEst.h")).read()
    for decl in ("setGroundTruth(const Mat", "setScoreParams(int", "int Score(int source"):
        assert decl in hdr
    blob = open(demo, "rb").read()
    assert b"psm_score_set_truth" in blob and b"Avg Err" in blob                          # hipUtil binds the symbols by name
