"""CPU-only checks of the surface of the SGM stage's disparity range (psm_sgm_set_range): the built library exports the symbol,
capi declares it, the argument checks answer without a device and name the accepted ranges, the Python keywords reach the call,
the header says what is not OpenCV's, and the C++ host (which binds the symbol and carries DispEst::setSGBMRange) still builds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAME = "psm_sgm_set_range"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_library_exports_the_symbol(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bT {NAME}\b", out)


def test_capi_declares_it(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    res, args = decl[NAME]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int]
    assert hasattr(built.load(), NAME)


def test_null_and_bad_values_are_refused_without_a_device(built):
    """(on a context the same messages are psm_last_error(ctx)'s: tests/test_gpu_sgm_range.py)"""
    lib = built.load()
    for ok in ((0, 0), (-1024, 1024), (1024, 2), (-7, 300)):
        assert lib.psm_sgm_set_range(None, *ok) != 0
        assert NAME in built.last_error(None) and "NULL" in built.last_error(None)
    for bad in (-1025, 1025, -(1 << 20), 1 << 20):
        assert lib.psm_sgm_set_range(None, bad, 64) != 0
        msg = built.last_error(None)
        assert NAME in msg and "min_disparity" in msg and str(bad) in msg and "[-1024, 1024]" in msg
    for bad in (-1, 1, 1025, 1 << 20):
        assert lib.psm_sgm_set_range(None, 0, bad) != 0
        msg = built.last_error(None)
        assert NAME in msg and "num_disparities" in msg and str(bad) in msg and "[2, 1024]" in msg and "max_disp" in msg


class _Recorder:
    """stands where the loaded library stands in a DispEst: every psm_* call is recorded and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args[1:]))
            return 0
        return call


def _fake(dispest, maxDis=64, W=12, H=8):
    de = object.__new__(dispest.DispEst)
    de._lib, de._h, de.wid, de.hei, de.maxDis = _Recorder(), 1, W, H, maxDis
    return de


def test_the_python_keywords_reach_the_call(built):
    from primestereomatch_amd import dispest
    for f in (dispest.DispEst.SGBM_GPU, dispest.sgbm_batch):
        p = inspect.signature(f).parameters
        assert p["min_disparity"].default == 0 and p["num_disparities"].default == 0
    de = _fake(dispest)
    disp = de.SGBM_GPU(min_disparity=-7, num_disparities=300)
    assert disp.shape == (8, 12) and disp.dtype == np.int16
    names = [n for n, _ in de._lib.calls]
    assert (NAME, (-7, 300)) in de._lib.calls and names.index(NAME) < names.index("psm_sgm_compute")
    Cv, Sv = de.sgm_costs()
    assert Cv.shape == Sv.shape == (8, 12, 300)                                          # sized by the range, not by maxDis
    del de._lib.calls[:]
    de.SGBM_GPU()
    assert (NAME, (0, 0)) in de._lib.calls                                               # the setting is the call's: the default again
    assert de.sgm_costs()[0].shape == (8, 12, 64)
    assert dispest.sgbm_batch([], min_disparity=3, num_disparities=512) == []


def test_the_batch_sets_every_object(built, monkeypatch):
    from primestereomatch_amd import dispest
    des = [_fake(dispest) for _ in range(3)]
    monkeypatch.setattr(dispest, "sgm_compute_batch", lambda ds: None)
    maps = dispest.sgbm_batch(des, min_disparity=5, num_disparities=1024)
    assert len(maps) == 3
    for de in des:
        assert (NAME, (5, 1024)) in de._lib.calls and de.sgm_costs()[1].shape == (8, 12, 1024)


def test_the_harness_forwards_the_keywords(built):
    from primestereomatch_amd import harness
    for f in (harness.compute_sgbm, harness.compute_sgbm_batch):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(f).parameters.values())
    assert "min_disparity" in harness.compute_sgbm.__doc__


def test_the_header_declares_it_and_says_what_is_not_opencvs():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"int psm_sgm_set_range\(psm_ctx \*ctx, int min_disparity, int num_disparities\);", text)
    block = text[text.index("minDisparity and numDisparities"):text.index("int psm_sgm_set_range(")]
    for phrase in ("[-1024, 1024]", "[2, 1024]", "(min_disparity - 1) * 16", "Not OpenCV's convention", "keeps all columns", "unpinned"):
        assert phrase in block, phrase


def test_the_models_bounds_are_the_librarys(built):
    import sgm_range_model as R
    lib = built.load()
    assert lib.psm_sgm_set_range(None, R.MAX_MIN + 1, 0) != 0 and "min_disparity" in built.last_error(None)
    assert lib.psm_sgm_set_range(None, R.MAX_MIN, R.MAX_D) != 0 and "NULL" in built.last_error(None)   # in range: only the context is missing
    assert lib.psm_sgm_set_range(None, 0, R.MAX_D + 1) != 0 and "num_disparities" in built.last_error(None)


def test_host_demo_builds_with_the_range(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    assert "setSGBMRange(int" in open(os.path.join(host, "DispEst.h")).read()
    assert NAME.encode() in open(demo, "rb").read()                                       # hipUtil binds the symbol by name
