"""CPU-only checks of the post-processing batch's surface (psm_post_process_batch): the header declares it and its stage bits, the
built library exports it, capi declares it, the argument checks that need no device answer without one, the Python wrappers handle
the empty list, and the C++ host (which binds the symbol and carries DispEst::PostProcessBatch) still builds."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_header_declares_the_symbol_and_the_stages():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"^int psm_post_process_batch\(psm_ctx \*const \*ctxs, int n, int stages\);", text, re.M)
    for name, value in (("PSM_PP_LR_CHECK", 1), ("PSM_PP_FILL", 2), ("PSM_PP_WGT_MEDIAN", 4)):
        assert re.search(rf"^#define {name}\s+{value}$", text, re.M), name


def test_library_exports_the_symbol(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT psm_post_process_batch\b", out)
    assert re.search(r"\bT psm_download_valid\b", out)


def test_capi_declares_it(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    res, args = decl["psm_post_process_batch"]
    assert res is C.c_int and args == [C.POINTER(C.c_void_p), C.c_int, C.c_int]
    assert hasattr(built.load(), "psm_post_process_batch")
    assert (built.PSM_PP_LR_CHECK, built.PSM_PP_FILL, built.PSM_PP_WGT_MEDIAN) == (1, 2, 4)


def test_null_arguments_are_refused_without_a_device(built):
    lib = built.load()
    assert lib.psm_post_process_batch(None, 0, 7) != 0
    assert "psm_post_process_batch" in built.last_error(None)
    arr = (C.c_void_p * 2)(None, None)
    assert lib.psm_post_process_batch(arr, 2, 7) != 0
    assert "psm_post_process_batch" in built.last_error(None)
    assert lib.psm_post_process_batch(arr, -1, 1) != 0
    assert "psm_post_process_batch" in built.last_error(None)
    assert lib.psm_download_valid(None, None, None, 0) != 0


def test_empty_list(built):
    import primestereomatch_amd as P
    from primestereomatch_amd import dispest, harness
    assert dispest.post_process_batch([]) is None
    assert dispest.post_process_batch([], lr_check=False, fill=True, median=True, download=False) is None
    assert P.post_process_batch is dispest.post_process_batch
    assert "post_process_batch" in P.__all__
    assert harness.compute_batch([], process_dm=True) == []


def test_host_demo_builds_with_the_batch(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    assert "PostProcessBatch" in open(os.path.join(host, "DispEst.h")).read()
    assert b"psm_post_process_batch" in open(demo, "rb").read()          # hipUtil binds the symbol by name
