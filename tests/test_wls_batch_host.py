"""CPU-only checks of the surface of the batch entry of the WLS smoothing stage (psm_wls_filter_batch: psm_wls_filter of several
contexts in one set of launches): the built library exports the symbol and holds the batch kernels, capi declares the call, the
argument checks answer without a device and carry messages, the Python layers reach the call, and the C++ host
(DispEst::WLSBatch) still builds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAME = "psm_wls_filter_batch"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_library_exports_the_symbol_and_holds_the_kernels(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bT {NAME}\b", out)
    # every kernel is a template over the record source: both instantiations - the record by value (RecVal<WlsPair, 1>, the single
    # call) and the device table (const WlsPair *, the batch) - are in the symbol table and in the code object
    blob = open(built.LIB_PATH, "rb").read()
    for kernel in ("k_wls_init", "k_wls_rows", "k_wls_cols"):
        stem = rf"_ZN3psm{len(kernel)}{kernel}I"
        by_value = re.search(rf"\bV ({stem}NS_6RecValINS_7WlsPairELi1EEEEEv\w+)$", out, re.M)
        table = re.search(rf"\bV ({stem}PKNS_7WlsPairEEEv\w+)$", out, re.M)
        assert by_value and table, kernel
        assert by_value.group(1) != table.group(1)
        for sym in (by_value.group(1), table.group(1)):
            assert (sym + ".kd").encode() in blob, sym


def test_capi_declares_it(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    assert decl[NAME][0] is C.c_int and hasattr(built.load(), NAME)
    assert decl[NAME][1] == [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]


def test_bad_arguments_are_refused_without_a_device(built):
    lib = built.load()
    none = (C.c_void_p * 2)(None, None)
    for args, words in (((None, 1, built.PSM_WLS_SGM, 0), ("NULL",)), ((none, 0, built.PSM_WLS_SGM, 0), ("n 0",)),
                        ((none, -3, built.PSM_WLS_SGM, 0), ("n -3",)), ((none, 2, built.PSM_WLS_SGM, 0), ("context 0", "NULL")),
                        ((none, 2, 2, 0), ("source 2",)), ((none, 2, -1, 0), ("source -1",)), ((None, 0, 0, 2), ("flag bits 0x2",)),
                        ((none, 2, built.PSM_WLS_SGM, built.PSM_WLS_USE_MASK), ("PSM_WLS_USE_MASK", "SGM source"))):
        assert lib.psm_wls_filter_batch(*args) != 0, args
        msg = built.last_error(None)
        assert msg.startswith(NAME + ":"), msg
        for w in words:
            assert w in msg, (w, msg)


class _Recorder:
    """stands where the loaded library stands in a DispEst: every psm_* call is recorded and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _fake(dispest, lib, h, maxDis=8, W=12, H=8):
    de = object.__new__(dispest.DispEst)
    de._lib, de._h, de.wid, de.hei, de.maxDis, de.options = lib, h, W, H, maxDis, {}
    return de


def test_the_python_layer_reaches_the_call(built):
    import primestereomatch_amd as P
    from primestereomatch_amd import dispest
    assert P.wls_batch is dispest.wls_batch and "wls_batch" in P.__all__
    assert dispest.wls_batch([]) == []
    lib = _Recorder()
    des = [_fake(dispest, lib, h) for h in (11, 22, 33)]
    maps = dispest.wls_batch(des)
    assert len(maps) == 3 and all(m.shape == (8, 12) and m.dtype == np.int16 for m in maps)
    assert [n for n, _ in lib.calls] == [NAME, "psm_wls_download", "psm_wls_download", "psm_wls_download"]
    arr, n, source, flags = lib.calls[0][1]
    assert list(arr) == [11, 22, 33] and (n, source, flags) == (3, built.PSM_WLS_SGM, 0)
    assert [a[0] for _, a in lib.calls[1:]] == [11, 22, 33]                          # every object's own map
    lib.calls.clear()
    dispest.wls_batch(des[:2], built.PSM_WLS_GIF, use_mask=True)
    assert lib.calls[0][1][1:] == (2, built.PSM_WLS_GIF, built.PSM_WLS_USE_MASK)
    lib.calls.clear()
    des[0].options[built.PSM_OPT_ASYNC] = 1                                          # asynchronous: nothing is downloaded
    assert dispest.wls_batch(des) is None and [n for n, _ in lib.calls] == [NAME]
    p = inspect.signature(dispest.wls_batch).parameters
    assert p["source"].default == built.PSM_WLS_SGM and p["use_mask"].default is False


def test_the_hosts_keep_the_new_options_off_by_default(built):
    from primestereomatch_amd import dispest, harness
    p = inspect.signature(harness.compute_sgbm_batch).parameters
    assert p["wls"].default is None and p["depth"].default is False
    assert "wls" in harness.compute_sgbm_batch.__doc__ and "depth" in harness.compute_sgbm_batch.__doc__
    p = inspect.signature(dispest.FrameRing.__init__).parameters
    assert p["wls"].default is None and p["wls"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "wls" in dispest.FrameRing.__init__.__doc__
    # compute_sgbm_batch's wls= steps, on a recorder: every object's parameters, one batch call, every object published
    lib = _Recorder()
    des = [_fake(dispest, lib, h) for h in (5, 6)]
    outs = [{}, {}]
    gt = np.zeros((8, 12), np.uint8)
    harness._wls_batch(des, outs, {"lam": 5.0}, 8, [gt, None], None, 1, 0)
    names = [n for n, _ in lib.calls]
    assert names == ["psm_wls_set_params"] * 2 + [NAME] + ["psm_wls_download"] * 2 + ["psm_wls_publish"] * 2
    assert lib.calls[0][1] == (5, 5.0, 1.5, 3) and lib.calls[1][1] == (6, 5.0, 1.5, 3)
    assert lib.calls[5][1] == (5, 1) and lib.calls[6][1] == (6, 1)
    assert set(outs[0]) == {"wls16", "bp_percent_wls"} and set(outs[1]) == {"wls16"}
    # ... and depth=False adds nothing and calls nothing
    lib.calls.clear()
    harness._reproject_batch(des, outs, False, built.PSM_DEPTH_SGM)
    assert lib.calls == [] and set(outs[1]) == {"wls16"}


def test_the_header_and_the_documents_carry_the_call():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"int psm_wls_filter_batch\(psm_ctx \*const \*ctxs, int n, int source, int flags\);", text)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for phrase in (NAME, "k_wls_init", "k_wls_rows", "k_wls_cols", "WlsPair", "Recs<WlsPair>"):
        assert phrase in design, phrase
    assert NAME in open(os.path.join(ROOT, "README.md")).read()
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_host_demo_builds_with_the_batch_entry(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    hdr = open(os.path.join(host, "DispEst.h")).read()
    assert "static int WLSBatch(DispEst *const *des, int n, int source = PSM_WLS_SGM, int flags = 0);" in hdr
    assert NAME.encode() in open(demo, "rb").read()                                  # hipUtil binds the symbol by name
