"""CPU-only checks of the surface of the WLS smoothing stage (psm_wls_filter: edge-aware smoothing of the sub-pixel disparity map on
the device): the built library exports the symbols and holds the kernels, capi declares them, the argument checks answer without
a device and carry messages, the Python layers reach the calls, and the C++ host (DispEst::WLS_GPU, psm_demo's --wls option) still
builds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("psm_wls_set_params", "psm_wls_filter", "psm_wls_wait", "psm_wls_download", "psm_wls_download_table", "psm_wls_time",
         "psm_wls_publish")


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
    blob = open(built.LIB_PATH, "rb").read()
    for kernel in ("k_wls_init", "k_wls_rows", "k_wls_cols"):      # the stage's own device code
        assert kernel.encode() in blob, kernel


def test_capi_declares_them(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    for name in NAMES:
        assert decl[name][0] is C.c_int and hasattr(built.load(), name)
    assert decl["psm_wls_set_params"][1] == [C.c_void_p, C.c_float, C.c_float, C.c_int]
    assert decl["psm_wls_filter"][1] == [C.c_void_p, C.c_int, C.c_int]
    assert decl["psm_wls_download"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    assert decl["psm_wls_publish"][1] == [C.c_void_p, C.c_int]
    assert (built.PSM_WLS_GIF, built.PSM_WLS_SGM, built.PSM_WLS_USE_MASK) == (0, 1, 1)
    assert built.PSM_WLS_VOID == 0x7FC00000


def test_null_context_is_refused_with_a_message(built):
    lib = built.load()
    calls = {
        "psm_wls_set_params": (None, 8000.0, 1.5, 3), "psm_wls_filter": (None, 1, 0), "psm_wls_wait": (None,),
        "psm_wls_download": (None, None, None, None, None, 0), "psm_wls_download_table": (None, None), "psm_wls_time": (None, None),
        "psm_wls_publish": (None, 1),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        msg = built.last_error(None)
        assert msg.startswith(name + ":") and "NULL" in msg, (name, msg)


def test_out_of_range_parameters_are_refused_without_a_device(built):
    """(on a context the same messages are psm_last_error(ctx)'s: tests/test_gpu_wls.py)"""
    lib = built.load()
    for ok in ((8000.0, 1.5, 3), (1e-6, 1e-6, 1), (1e30, 1e30, 4)):      # in range: only the context is missing
        assert lib.psm_wls_set_params(None, *ok) != 0 and "NULL context" in built.last_error(None)
    for bad, word in (((0.0, 1.5, 3), "lambda"), ((-8000.0, 1.5, 3), "lambda"), ((np.nan, 1.5, 3), "lambda"), ((np.inf, 1.5, 3), "lambda"),
                      ((8000.0, 0.0, 3), "sigma"), ((8000.0, -1.5, 3), "sigma"), ((8000.0, np.nan, 3), "sigma"), ((8000.0, np.inf, 3), "sigma"),
                      ((8000.0, 1.5, 0), "iterations 0"), ((8000.0, 1.5, 5), "iterations 5"), ((8000.0, 1.5, -3), "iterations -3")):
        assert lib.psm_wls_set_params(None, *bad) != 0
        msg = built.last_error(None)
        assert msg.startswith("psm_wls_set_params:") and word in msg and "NULL" not in msg, msg
    for args, word in (((2, 0), "source 2"), ((-1, 0), "source -1"), ((0, 2), "flag bits 0x2"), ((1, 1), "PSM_WLS_USE_MASK")):
        assert lib.psm_wls_filter(None, *args) != 0
        msg = built.last_error(None)
        assert msg.startswith("psm_wls_filter:") and word in msg and "NULL" not in msg, msg


class _Recorder:
    """stands where the loaded library stands in a DispEst: every psm_* call is recorded and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args[1:]))
            return 0
        return call


def _fake(dispest, maxDis=8, W=12, H=8):
    de = object.__new__(dispest.DispEst)
    de._lib, de._h, de.wid, de.hei, de.maxDis, de.options = _Recorder(), 1, W, H, maxDis, {}
    return de


def test_the_python_layer_reaches_the_calls(built):
    from primestereomatch_amd import dispest
    de = _fake(dispest)
    de.setWLS(lam=100.0, sigma=2.5, iterations=2)
    de.WLS_GPU()
    de.WLS_GPU(built.PSM_WLS_GIF, use_mask=True)
    de.wls_wait()
    disp = de.wls_map()
    q, num, den = de.wls_planes()
    tab = de.wls_table()
    de.wls_publish()
    de.wls_publish(False)
    de.wls_time()
    assert disp.shape == (8, 12) and disp.dtype == np.int16 and tab.shape == (256,) and tab.dtype == np.float32
    assert all(a.shape == (8, 12) and a.dtype == np.float32 for a in (q, num, den))
    calls = de._lib.calls
    assert [n for n, _ in calls] == ["psm_wls_set_params", "psm_wls_filter", "psm_wls_filter", "psm_wls_wait", "psm_wls_download",
                                     "psm_wls_download", "psm_wls_download_table", "psm_wls_publish", "psm_wls_publish", "psm_wls_time"]
    assert calls[0][1] == (100.0, 2.5, 2) and calls[1][1] == (built.PSM_WLS_SGM, 0) and calls[2][1] == (built.PSM_WLS_GIF, built.PSM_WLS_USE_MASK)
    assert calls[4][1][1:4] == (None, None, None) and calls[4][1][0] is not None          # wls_map: the int16 map alone
    assert calls[5][1][0] is None and all(p is not None for p in calls[5][1][1:4])        # wls_planes: the three float planes
    assert calls[7][1] == (1,) and calls[8][1] == (0,)
    p = inspect.signature(dispest.DispEst.setWLS).parameters
    assert (p["lam"].default, p["sigma"].default, p["iterations"].default) == (8000.0, 1.5, 3)


def test_the_harness_keeps_wls_off_by_default(built):
    from primestereomatch_amd import harness
    p = inspect.signature(harness.compute_sgbm).parameters
    assert p["wls"].default is None and "wls" in harness.compute_sgbm.__doc__ and "bp_percent_wls" in harness.compute_sgbm.__doc__
    # the option's own steps, on a recorder: parameters, filter, publish, download - and the rounded reading of the metric
    from primestereomatch_amd import dispest
    de = _fake(dispest, maxDis=8)
    de.wls_map = lambda: np.array([[7, 8, 23, 24, -16, 4095, 32767, 0] * 2] * 8, np.int16)[:, :12]
    out = {}
    gt = np.zeros((8, 12), np.uint8)
    harness._wls(de, out, {"lam": 5.0}, 8, gt, None, 1, 0)
    assert [n for n, _ in de._lib.calls] == ["psm_wls_set_params", "psm_wls_filter", "psm_wls_publish"]
    assert de._lib.calls[0][1] == (5.0, 1.5, 3) and de._lib.calls[1][1] == (built.PSM_WLS_SGM, 0) and de._lib.calls[2][1] == (1,)
    assert set(out) == {"wls16", "bp_percent_wls"} and out["wls16"].dtype == np.int16
    # columns up to maxDis are not scored; the scored three hold 8, 23, 24 -> 1, 1, 2, all off the truth 0
    assert out["bp_percent_wls"] == 100.0 * (3 * 8) / 96
    out = {}
    harness._wls(de, out, {}, 8, None, None, 1, 0)
    assert set(out) == {"wls16"}


def test_the_header_and_the_documents_carry_the_definition():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"int psm_wls_filter\(psm_ctx \*ctx, int source, int flags\);", text)
    assert re.search(r"int psm_wls_download\(psm_ctx \*ctx, int16_t \*disp, float \*q, float \*num, float \*den, size_t stride_bytes\);", text)
    for phrase in ("PSM_WLS_GIF = 0, PSM_WLS_SGM = 1", "PSM_WLS_USE_MASK = 1", "0x7FC00000", "tests/wls_model.py", "r = 1.0f / m",
                   "0x1p-64f", "exp(-(double)k / (double)sigma)", "4^(T-1-t)", "unpinned"):
        assert phrase in text, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for phrase in ("psm_wls_filter", "k_wls_rows", "k_wls_cols", "WLS_PITCH", "psm_wls_publish", "tests/wls_model.py"):
        assert phrase in design, phrase
    assert "psm_wls_filter" in open(os.path.join(ROOT, "README.md")).read()
    tab = open(os.path.join(ROOT, "primestereomatch_amd", "csrc", "psm_wls_tab.h")).read()
    assert "hip" not in tab.replace("free of HIP", "").lower() and "std::exp" in tab       # host only


def test_host_demo_builds_with_the_stage(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    hdr = open(os.path.join(host, "DispEst.h")).read()
    for decl in ("int setWLS(float lambda", "int WLS_GPU(int source", "int WLSPublish(bool on)", "int WLSWait()", "int wlsTime(double *ms)"):
        assert decl in hdr
    blob = open(demo, "rb").read()
    assert b"psm_wls_filter" in blob and b"psm_wls_publish" in blob and b"--wls" in blob      # hipUtil binds the symbols by name
