"""CPU-only checks of the JointWMF batch's surface (psm_joint_wmf_batch): the built library exports it, capi declares it, the
argument checks that need no device answer without one, the Python wrappers handle the empty list, and the C++ host (which binds
the symbol and carries DispEst::JointWMFBatch) still builds."""
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
    assert re.search(r"\bT psm_joint_wmf_batch\b", out)


def test_capi_declares_it(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    assert "psm_joint_wmf_batch" in decl
    res, args = decl["psm_joint_wmf_batch"]
    assert res is C.c_int and args == [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_float, C.c_int, C.c_int]
    assert hasattr(built.load(), "psm_joint_wmf_batch")


def test_null_arguments_are_refused_without_a_device(built):
    lib = built.load()
    assert lib.psm_joint_wmf_batch(None, 0, 0, 0.0, 0, 0) != 0
    assert "psm_joint_wmf_batch" in built.last_error(None)
    arr = (C.c_void_p * 2)(None, None)
    assert lib.psm_joint_wmf_batch(arr, 2, 0, 0.0, 0, 0) != 0
    assert "psm_joint_wmf_batch" in built.last_error(None)
    assert lib.psm_joint_wmf_batch(arr, -1, 0, 0.0, 0, 0) != 0
    assert "psm_joint_wmf_batch" in built.last_error(None)


def test_empty_list(built):
    import primestereomatch_amd as P
    from primestereomatch_amd import dispest, harness
    assert dispest.joint_wmf_batch([]) is None
    assert dispest.joint_wmf_batch([], radius=4, sigma=10.0, n_clusters=16, max_iter=5) is None
    assert P.joint_wmf_batch is dispest.joint_wmf_batch
    assert "joint_wmf_batch" in P.__all__
    assert harness.compute_batch([]) == []
    assert harness.compute_batch([], joint_wmf=True) == []


def test_host_demo_builds_with_the_batch(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    assert "JointWMFBatch" in open(os.path.join(host, "DispEst.h")).read()
    assert b"psm_joint_wmf_batch" in open(demo, "rb").read()          # hipUtil binds the symbol by name
