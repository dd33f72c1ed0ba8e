"""CPU-only checks of the surface of the graded confidence of the WLS smoothing stage (PSM_WLS_CONFIDENCE): the built library exports
the three symbols and holds the two kernels, capi declares them, the argument checks of psm_wls_set_confidence and of the flag
answer without a device, the Python layers reach the calls, and the header and documents carry the definition."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("psm_wls_set_confidence", "psm_wls_download_confidence", "psm_wls_conf_time")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_library_exports_the_symbols_and_holds_the_kernels(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}\b", out), name
    blob = open(built.LIB_PATH, "rb").read()
    for kernel in ("k_sgm_right16", "k_wls_conf", "k_wls_init_conf", "k_wls_init"):
        assert kernel.encode() in blob, kernel


def test_capi_declares_them(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    for name in NAMES:
        assert decl[name][0] is C.c_int and hasattr(built.load(), name)
    assert decl["psm_wls_set_confidence"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    assert decl["psm_wls_download_confidence"][1] == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    assert (built.PSM_WLS_USE_MASK, built.PSM_WLS_CONFIDENCE, built.PSM_WLS_CONF_LR, built.PSM_WLS_CONF_VAR) == (1, 2, 1, 2)


def test_refusals_that_need_no_device(built):
    lib = built.load()
    for name, args in (("psm_wls_set_confidence", (None, 3, 24, 2, 8)), ("psm_wls_download_confidence", (None, None, 0, None, 0)),
                       ("psm_wls_conf_time", (None, None))):
        assert getattr(lib, name)(*args) != 0, name
        msg = built.last_error(None)
        assert msg.startswith(name + ":") and "NULL" in msg, (name, msg)
    for ok in ((1, 1, 1, 0), (2, 32767, 4, 16), (3, 24, 2, 8)):        # in range: only the context is missing
        assert lib.psm_wls_set_confidence(None, *ok) != 0 and "NULL context" in built.last_error(None)
    for bad, word in (((0, 24, 2, 8), "terms 0"), ((4, 24, 2, 8), "terms 4"), ((-1, 24, 2, 8), "terms -1"), ((3, 0, 2, 8), "lr_thresh 0"),
                      ((3, 32768, 2, 8), "lr_thresh 32768"), ((3, 24, 0, 8), "radius 0"), ((3, 24, 5, 8), "radius 5"),
                      ((3, 24, 2, -1), "var_shift -1"), ((3, 24, 2, 17), "var_shift 17")):
        assert lib.psm_wls_set_confidence(None, *bad) != 0
        msg = built.last_error(None)
        assert msg.startswith("psm_wls_set_confidence:") and word in msg and "NULL" not in msg, msg
    # the flag: known, but not with the GIF source; the next bit is unknown
    for args, word in (((0, 2), "PSM_WLS_CONFIDENCE"), ((0, 3), "PSM_WLS_CONFIDENCE"), ((1, 4), "unknown flag bits 0x4"), ((1, 6), "unknown flag bits 0x4")):
        assert lib.psm_wls_filter(None, *args) != 0
        msg = built.last_error(None)
        assert msg.startswith("psm_wls_filter:") and word in msg and "NULL" not in msg, msg
    assert lib.psm_wls_filter(None, 1, 2) != 0 and "NULL context" in built.last_error(None)      # accepted as far as the arguments go


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args[1:]))
            return 0
        return call


def _fake(dispest, W=12, H=8):
    de = object.__new__(dispest.DispEst)
    de._lib, de._h, de.wid, de.hei, de.maxDis, de.options = _Recorder(), 1, W, H, 8, {}
    return de


def test_the_python_layer_reaches_the_calls(built):
    from primestereomatch_amd import dispest, harness
    de = _fake(dispest)
    de.WLS_GPU()
    de.WLS_GPU(confidence={})
    de.WLS_GPU(confidence={"terms": built.PSM_WLS_CONF_VAR, "radius": 4})
    conf, r16 = de.download_wls_confidence()
    conf2, none = de.download_wls_confidence(right=False)
    de.wls_conf_time()
    assert conf.shape == r16.shape == conf2.shape == (8, 12) and conf.dtype == np.uint8 and r16.dtype == np.int16 and none is None
    calls = de._lib.calls
    assert [n for n, _ in calls] == ["psm_wls_filter", "psm_wls_set_confidence", "psm_wls_filter", "psm_wls_set_confidence", "psm_wls_filter",
                                     "psm_wls_download_confidence", "psm_wls_download_confidence", "psm_wls_conf_time"]
    assert calls[0][1] == (built.PSM_WLS_SGM, 0)                       # without the option nothing changes
    assert calls[1][1] == (3, 24, 2, 8) and calls[2][1] == (built.PSM_WLS_SGM, built.PSM_WLS_CONFIDENCE)
    assert calls[3][1] == (2, 24, 4, 8)
    assert calls[6][1][2] is None
    p = inspect.signature(dispest.DispEst.setWLSConfidence).parameters
    assert tuple(p[k].default for k in ("terms", "lr_thresh", "radius", "var_shift")) == (3, 24, 2, 8)
    assert inspect.signature(dispest.wls_batch).parameters["confidence"].default is None
    # the harness: "confidence" in the wls dict is the option, the rest setWLS's
    de = _fake(dispest)
    de.wls_map = lambda: np.zeros((8, 12), np.int16)
    harness._wls(de, {}, {"lam": 5.0, "confidence": {"lr_thresh": 30}}, 8, None, None, 1, 0)
    assert [n for n, _ in de._lib.calls] == ["psm_wls_set_params", "psm_wls_set_confidence", "psm_wls_filter", "psm_wls_publish"]
    assert de._lib.calls[0][1] == (5.0, 1.5, 3) and de._lib.calls[1][1] == (3, 30, 2, 8) and de._lib.calls[2][1] == (built.PSM_WLS_SGM, built.PSM_WLS_CONFIDENCE)


def test_the_header_and_the_documents_carry_the_definition():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert "int psm_wls_set_confidence(psm_ctx *ctx, int terms, int lr_thresh, int radius, int var_shift);" in text
    assert "int psm_wls_download_confidence(psm_ctx *ctx, uint8_t *conf, size_t conf_stride, int16_t *right16, size_t right_stride_bytes);" in text
    assert "int psm_wls_conf_time(psm_ctx *ctx, double *ms);" in text
    for phrase in ("PSM_WLS_USE_MASK = 1, PSM_WLS_CONFIDENCE = 2", "PSM_WLS_CONF_LR = 1, PSM_WLS_CONF_VAR = 2", "tests/wls_conf_model.py",
                   "Out of scope", "(n^2 << var_shift)", "(dmin - 1) 16"):
        assert phrase in text, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for phrase in ("PSM_WLS_CONFIDENCE", "k_sgm_right16", "k_wls_conf", "tests/wls_conf_model.py"):
        assert phrase in design, phrase
    assert "PSM_WLS_CONFIDENCE" in open(os.path.join(ROOT, "README.md")).read()
    assert "PSM_WLS_CONFIDENCE" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_host_demo_carries_the_option(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    hdr = open(os.path.join(host, "DispEst.h")).read()
    assert "int setWLSConfidence(int terms" in hdr
    blob = open(os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo"), "rb").read()
    assert b"psm_wls_set_confidence" in blob and b"--wls-conf" in blob
