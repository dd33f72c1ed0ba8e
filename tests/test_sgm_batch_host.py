"""CPU-only checks of the SGM batch's surface (psm_sgm_compute_batch): the built library exports it, capi declares it, the
argument checks that need no device answer without one, the Python wrapper handles the empty list, and the C++ host (which binds
the symbol and carries DispEst::SGBMBatch) still builds."""
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


def test_library_exports_the_symbol(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT psm_sgm_compute_batch\b", out)


def test_capi_declares_it(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    assert "psm_sgm_compute_batch" in decl
    res, args = decl["psm_sgm_compute_batch"]
    assert res is C.c_int and args == [C.POINTER(C.c_void_p), C.c_int]
    assert hasattr(built.load(), "psm_sgm_compute_batch")


def test_null_arguments_are_refused_without_a_device(built):
    lib = built.load()
    assert lib.psm_sgm_compute_batch(None, 0) != 0
    assert "psm_sgm_compute_batch" in built.last_error(None)
    arr = (C.c_void_p * 2)(None, None)
    assert lib.psm_sgm_compute_batch(arr, 2) != 0
    assert lib.psm_sgm_compute_batch(arr, -1) != 0


def test_empty_list(built):
    import primestereomatch_amd as P
    from primestereomatch_amd import dispest, harness
    assert dispest.sgbm_batch([]) == []
    assert dispest.sgbm_batch([], pre_filter_cap=63, speckle_window_size=100, speckle_range=32) == []
    assert P.sgbm_batch is dispest.sgbm_batch
    assert harness.compute_sgbm_batch([]) == []


def test_host_demo_builds_with_the_batch(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    assert "SGBMBatch" in open(os.path.join(host, "DispEst.h")).read()
    assert b"psm_sgm_compute_batch" in open(demo, "rb").read()          # hipUtil binds the symbol by name
