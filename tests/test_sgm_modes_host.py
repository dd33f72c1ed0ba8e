"""CPU-only checks of the surface of the SGM stage's modes (psm_sgm_set_mode): the built library exports the symbol, capi declares
it, the argument checks answer without a device and name the accepted values, the Python wrappers know the four names, and the
C++ host (which binds the symbol and carries DispEst::setSGBMMode) still builds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

SETTERS = ("psm_sgm_set_mode",)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_library_exports_the_symbols(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SETTERS:
        assert re.search(rf"\bT {name}\b", out)


def test_capi_declares_them(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    for name in SETTERS:
        res, args = decl[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_int]
        assert hasattr(built.load(), name)


def test_null_and_bad_values_are_refused_without_a_device(built):
    """(on a context the same messages are psm_last_error(ctx)'s: tests/test_gpu_sgm_modes.py)"""
    lib = built.load()
    for name in SETTERS:
        assert getattr(lib, name)(None, 1) != 0
        assert name in built.last_error(None) and "NULL" in built.last_error(None)
    for bad in (-1, 4, 1 << 20):
        assert lib.psm_sgm_set_mode(None, bad) != 0
        msg = built.last_error(None)
        assert "psm_sgm_set_mode" in msg and str(bad) in msg
        assert all(w in msg for w in ("0: MODE_SGBM", "1: MODE_HH", "2: MODE_SGBM_3WAY", "3: MODE_HH4"))


def test_python_wrappers_know_the_names(built):
    from primestereomatch_amd import dispest
    import sgm_mode_model as MM
    assert dispest.SGM_MODES == MM.VALUES
    assert [dispest.sgm_mode(m) for m in ("sgbm", "hh", "3way", "hh4", 2)] == [0, 1, 2, 3, 2]
    with pytest.raises(ValueError, match="hh8"):
        dispest.sgm_mode("hh8")
    for f in (dispest.DispEst.SGBM_GPU, dispest.sgbm_batch):
        p = inspect.signature(f).parameters
        assert p["mode"].default == "hh"
    assert dispest.sgbm_batch([], mode="3way") == []


def test_header_enum_holds_opencvs_values():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    for name, value in (("PSM_SGM_MODE_SGBM", 0), ("PSM_SGM_MODE_HH", 1), ("PSM_SGM_MODE_SGBM_3WAY", 2), ("PSM_SGM_MODE_HH4", 3)):
        assert re.search(rf"\b{name} = {value}\b", text)


def test_host_demo_builds_with_the_modes(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    header = open(os.path.join(host, "DispEst.h")).read()
    assert "setSGBMMode(int" in header
    blob = open(demo, "rb").read()
    for name in SETTERS:
        assert name.encode() in blob                                     # hipUtil binds the symbols by name
