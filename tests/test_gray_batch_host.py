"""CPU-only checks of the gray batch's surface (psm_gray_compute_batch): the header declares it, the built library exports it, capi
declares it, the argument checks that need no device answer without one, the Python wrappers handle the empty list, and the C++
host (which binds the symbol and carries DispEst::GrayBatch) still builds."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

NAME = "psm_gray_compute_batch"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_header_declares_the_prototype():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    proto = (r"^int psm_gray_compute_batch\(psm_ctx \*const \*ctxs, int n, const void \*const \*ls, const void \*const \*rs, "
             r"size_t stride_bytes, int depth,\s+uint8_t \*const \*lmaps, uint8_t \*const \*rmaps, size_t map_stride\);")
    assert re.search(proto, text, re.M)
    # the stage's paragraph no longer lists batches among what it leaves out
    scope = re.search(r"Out of scope:([^/]*)\*/\s*int psm_gray_compute\(", text)
    assert scope and "batch" not in scope.group(1)


def test_library_exports_the_symbol(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bT {NAME}\b", out)
    assert re.search(r"\bT psm_gray_compute\b", out)


def test_capi_declares_it(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    res, args = decl[NAME]
    pp = C.POINTER(C.c_void_p)
    assert res is C.c_int and args == [pp, C.c_int, pp, pp, C.c_size_t, C.c_int, pp, pp, C.c_size_t]
    assert hasattr(built.load(), NAME)


def test_null_arguments_are_refused_without_a_device(built):
    lib = built.load()
    fn = getattr(lib, NAME)
    planes = (C.c_void_p * 2)(None, None)
    for ctxs, n in ((None, 2), ((C.c_void_p * 2)(None, None), 0), ((C.c_void_p * 2)(None, None), -1), ((C.c_void_p * 2)(None, None), 2)):
        lib.psm_gray_compute(None, None, None, 0, 0, None, None, 0)          # (another call's message in the slot first)
        assert fn(ctxs, n, planes, planes, 0, 0, None, None, 0) != 0
        assert NAME in built.last_error(None), (n, built.last_error(None))


def test_empty_list(built):
    import primestereomatch_amd as P
    from primestereomatch_amd import dispest, harness
    assert dispest.gray_batch([], []) == [] and dispest.gray_batch([], [], []) == []
    assert dispest.gray_batch([], [], [], download=False) == []
    assert P.gray_batch is dispest.gray_batch
    assert "gray_batch" in P.__all__
    assert harness.compute_gray_batch([]) == []
    assert harness.compute_gray_batch([], 64, None, None, lr_check=True, fill=True, device_tail=True) == []


def test_host_demo_builds_with_the_batch(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    assert "GrayBatch" in open(os.path.join(host, "DispEst.h")).read()
    assert NAME.encode() in open(demo, "rb").read()          # hipUtil binds the symbol by name
