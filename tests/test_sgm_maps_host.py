"""CPU-only checks of the surface of psm_sgm_select_maps / _batch / psm_sgm_maps_time: the built library exports the symbols, capi
declares them, NULL contexts are refused without a device with messages that name the call, the Python keywords reach the calls in
order, compute_sgbm's defaults add no key, the header states the range condition and what is untouched, and the C++ host (which
binds the symbols and carries DispEst::SGBMSelect) still builds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = {"psm_sgm_select_maps": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
         "psm_sgm_select_maps_batch": [C.POINTER(C.c_void_p), C.c_int],
         "psm_sgm_maps_time": [C.c_void_p, C.POINTER(C.c_double)]}


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


def test_capi_declares_them(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    for name, args in NAMES.items():
        assert decl[name] == (C.c_int, args), name
        assert hasattr(built.load(), name)


def test_null_contexts_are_refused_without_a_device(built):
    lib = built.load()
    assert lib.psm_sgm_select_maps(None, None, None, 0) != 0
    assert "psm_sgm_select_maps" in built.last_error(None) and "NULL" in built.last_error(None)
    assert lib.psm_sgm_maps_time(None, None) != 0
    assert "psm_sgm_maps_time" in built.last_error(None) and "NULL" in built.last_error(None)
    assert lib.psm_sgm_select_maps_batch(None, 1) != 0
    assert "psm_sgm_select_maps_batch" in built.last_error(None)
    arr = (C.c_void_p * 2)(None, None)
    for n in (2, 0, -1):
        assert lib.psm_sgm_select_maps_batch(arr, n) != 0
        assert "psm_sgm_select_maps_batch" in built.last_error(None)


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
    de.lDisMap, de.rDisMap = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    de.lValid, de.rValid = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    de.options = {}
    return de


def test_the_python_calls_reach_the_library_in_order(built, monkeypatch):
    from primestereomatch_amd import dispest
    assert inspect.signature(dispest.DispEst.SGBMSelect_GPU).parameters["download"].default is True
    de = _fake(dispest)
    de.SGBM_GPU()
    maps = de.SGBMSelect_GPU()
    assert maps[0] is de.lDisMap and maps[1] is de.rDisMap
    de.LRCheck_GPU(); de.FillInv_GPU(); de.WgtMedian_GPU()
    names = [n for n, _ in de._lib.calls]
    order = [names.index(n) for n in ("psm_sgm_compute", "psm_sgm_select_maps", "psm_lr_check", "psm_fill_invalid", "psm_wgt_median")]
    assert order == sorted(order)
    call = de._lib.calls[names.index("psm_sgm_select_maps")]
    assert call[1][0] is not None and call[1][1] is not None and call[1][2] == 12      # both maps, the row pitch
    del de._lib.calls[:]
    assert de.SGBMSelect_GPU(download=False) is None
    assert de._lib.calls == [("psm_sgm_select_maps", (None, None, 0))]
    assert de.sgm_maps_time() == 0.0 and de._lib.calls[-1][0] == "psm_sgm_maps_time"
    assert dispest.sgbm_select_batch([]) is None
    seen = []
    monkeypatch.setattr(dispest.capi, "check", lambda rc, h=None, what="": seen.append(what))
    dispest.sgbm_select_batch([_fake(dispest), _fake(dispest)])
    assert seen == ["sgbm_select_batch"]
    import primestereomatch_amd as P
    assert "sgbm_select_batch" in P.__all__


def test_the_harness_takes_the_keywords_and_its_defaults_add_no_key(built, monkeypatch):
    from primestereomatch_amd import dispest, harness
    for f in (harness.compute_sgbm, harness.compute_sgbm_batch):
        p = inspect.signature(f).parameters
        assert p["post_process"].default is False and p["joint_wmf"].default is False
    assert "lDisMap_pp" in harness.compute_sgbm.__doc__ and "bp_percent_pp" in harness.compute_sgbm.__doc__

    fakes = []

    class Fake(dispest.DispEst):
        def __init__(self, l, r, d, *a, **k):
            self.__dict__.update(_fake(dispest, d, l.shape[1], l.shape[0]).__dict__)
            fakes.append(self)

        def sgm_disparity(self):                                   # (a map with a range: the display conversion divides by it)
            return (np.arange(self.hei * self.wid, dtype=np.int16).reshape(self.hei, self.wid) % 8) * 16

        def sgm_times(self):
            return (0.0, 0.0, 0.0)

        def close(self):
            pass

    monkeypatch.setattr(harness, "DispEst", Fake)
    img = np.zeros((8, 12, 3), np.uint8)
    gt = np.zeros((8, 12), np.uint8)
    plain = harness.compute_sgbm(img, img, 8, gt)
    assert sorted(plain) == ["avg_err", "bad_pixels", "bp_percent", "bp_percent_int", "cost_ms", "disp16", "lDispMap", "paths_ms", "select_ms"]
    assert "psm_sgm_select_maps" not in [n for n, _ in fakes[-1]._lib.calls]
    out = harness.compute_sgbm(img, img, 8, gt, post_process=True)
    assert sorted(set(out) - set(plain)) == ["avg_err_pp", "bp_percent_pp", "lDisMap_pp"]
    names = [n for n, _ in fakes[-1]._lib.calls]
    order = [names.index(n) for n in ("psm_sgm_compute", "psm_sgm_select_maps", "psm_lr_check", "psm_fill_invalid", "psm_wgt_median")]
    assert order == sorted(order) and "psm_joint_wmf" not in names
    harness.compute_sgbm(img, img, 8, gt, joint_wmf=True)
    names = [n for n, _ in fakes[-1]._lib.calls]
    order = [names.index(n) for n in ("psm_sgm_select_maps", "psm_lr_check", "psm_joint_wmf")]
    assert order == sorted(order) and "psm_wgt_median" not in names and "psm_fill_invalid" not in names


def test_the_header_states_the_range_condition_and_what_is_untouched():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"int psm_sgm_select_maps\(psm_ctx \*ctx, uint8_t \*lmap, uint8_t \*rmap, size_t stride\);", text)
    assert re.search(r"int psm_sgm_select_maps_batch\(psm_ctx \*const \*ctxs, int n\);", text)
    assert re.search(r"int psm_sgm_maps_time\(psm_ctx \*ctx, double \*ms\);", text)
    block = text[text.index("The 8-bit maps of both views from the SGM stage"):text.index("int psm_sgm_select_maps(")]
    for phrase in ("tests/sgm_maps_model.py", "0 <= dmin and dmin + D <= max_disp", "lowest k on ties", "Untouched", "untouched",
                   "psm_upload_maps", "disparity shard", "row stripe", "stride < W", "psm_release_scratch", "no global atomics"):
        assert phrase in block, phrase
    assert "n * 96 bytes" in text and "n * 88 bytes" not in text


def test_host_demo_builds_with_the_maps(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    text = open(os.path.join(host, "DispEst.h")).read()
    assert "int SGBMSelect();" in text and "SGBMSelectBatch(" in text
    blob = open(demo, "rb").read()
    for name in NAMES:
        assert name.encode() in blob                                                      # hipUtil binds the symbols by name
