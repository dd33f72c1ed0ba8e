"""CPU-only checks of the surface of the reprojection stage (psm_reproject: cv::reprojectImageTo3D and the point cloud on the
device): the built library exports the symbols and holds the kernels, capi declares them and the 16-byte record, the argument
checks answer without a device and carry messages, the Python layers reach the calls, and the C++ host (DispEst::Reproject,
psm_demo's --ply option) still builds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("psm_reproject_set_q", "psm_reproject_set_range", "psm_reproject", "psm_reproject_wait", "psm_reproject_download",
         "psm_reproject_download_cloud", "psm_reproject_batch", "psm_reproject_time")
EYE = (C.c_double * 16)(*np.eye(4).reshape(-1))


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
    # the stage's own device code: every kernel is a template over the record source, and both instantiations - the record by
    # value (RecVal<DpArgs, 1>) and the device table (const DpArgs *) - are in the symbol table and in the code object
    blob = open(built.LIB_PATH, "rb").read()
    for kernel in ("k_dp_count", "k_dp_scan", "k_dp_pack"):
        stem = rf"_ZN3psm{len(kernel)}{kernel}I"
        by_value = re.search(rf"\bV ({stem}NS_6RecValINS_6DpArgsELi1EEEEEv\w+)$", out, re.M)
        table = re.search(rf"\bV ({stem}PKNS_6DpArgsEEEv\w+)$", out, re.M)
        assert by_value and table, kernel
        assert by_value.group(1) != table.group(1)
        for sym in (by_value.group(1), table.group(1)):
            assert (sym + ".kd").encode() in blob, sym


def test_capi_declares_them_and_the_record(built):
    decl = {name: (res, args) for name, res, args in built.SYMBOLS}
    for name in NAMES:
        assert decl[name][0] is C.c_int and hasattr(built.load(), name)
    pu = C.POINTER(C.c_uint32)
    assert decl["psm_reproject"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_int, pu]
    assert decl["psm_reproject_set_q"][1] == [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int]
    assert decl["psm_reproject_set_range"][1] == [C.c_void_p, C.c_float, C.c_float]
    assert decl["psm_reproject_download_cloud"][1] == [C.c_void_p, C.c_void_p, C.c_uint32, pu]
    assert decl["psm_reproject_batch"][1] == [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, pu]
    dt = built.point_dtype()
    assert dt.itemsize == 16 and dt.names == ("x", "y", "z", "b", "g", "r", "a")
    assert [dt.fields[k][1] for k in dt.names] == [0, 4, 8, 12, 13, 14, 15]
    assert C.sizeof(built.Point) == 16 and built.Point.b.offset == 12 and built.Point.a.offset == 15
    assert (built.PSM_DEPTH_GIF, built.PSM_DEPTH_SGM) == (0, 1)
    assert (built.PSM_DEPTH_XYZ, built.PSM_DEPTH_Z, built.PSM_DEPTH_CLOUD, built.PSM_DEPTH_USE_MASK) == (1, 2, 4, 1)
    assert built.PSM_DEPTH_VOID == 0x7FC00000


def test_null_context_is_refused_with_a_message(built):
    lib = built.load()
    n = C.c_uint32()
    calls = {
        "psm_reproject_set_q": (None, EYE, 0, 0), "psm_reproject_set_range": (None, 0.0, 1.0),
        "psm_reproject": (None, 0, 4, 0, C.byref(n)), "psm_reproject_wait": (None, C.byref(n)),
        "psm_reproject_download": (None, None, None, 0), "psm_reproject_download_cloud": (None, None, 0, C.byref(n)),
        "psm_reproject_time": (None, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        msg = built.last_error(None)
        assert msg.startswith(name + ":") and "NULL" in msg, (name, msg)
    assert lib.psm_reproject_batch(None, 3, 0, 4, 0, None) != 0 and built.last_error(None).startswith("psm_reproject_batch:")
    arr = (C.c_void_p * 2)(None, None)
    assert lib.psm_reproject_batch(arr, 2, 0, 4, 0, None) != 0 and built.last_error(None).startswith("psm_reproject_batch:")


def test_out_of_range_parameters_are_refused_without_a_device(built):
    """(on a context the same messages are psm_last_error(ctx)'s: tests/test_gpu_depth.py)"""
    lib = built.load()
    n = C.c_uint32()
    for crop in ((0, 0), (-32768, 32767), (32767, -32768)):      # in range: only the context is missing
        assert lib.psm_reproject_set_q(None, EYE, *crop) != 0 and "NULL context" in built.last_error(None)
    for crop in ((-32769, 0), (0, 32768), (1 << 20, 0)):
        assert lib.psm_reproject_set_q(None, EYE, *crop) != 0
        msg = built.last_error(None)
        assert msg.startswith("psm_reproject_set_q:") and "crop" in msg and "[-32768, 32767]" in msg and "NULL" not in msg
    for at, bad in ((0, np.inf), (7, -np.inf), (15, np.nan)):
        q = np.eye(4).reshape(-1)
        q[at] = bad
        assert lib.psm_reproject_set_q(None, (C.c_double * 16)(*q), 0, 0) != 0
        msg = built.last_error(None)
        assert msg.startswith("psm_reproject_set_q:") and f"Q[{at // 4}][{at % 4}]" in msg and "finite" in msg
    assert lib.psm_reproject_set_q(None, None, 0, 0) != 0 and "NULL Q" in built.last_error(None)
    for ok in ((0.0, 1.0), (-np.inf, np.inf), (-1.0, 0.0)):
        assert lib.psm_reproject_set_range(None, *ok) != 0 and "NULL context" in built.last_error(None)
    for bad in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan)):
        assert lib.psm_reproject_set_range(None, *bad) != 0
        msg = built.last_error(None)
        assert msg.startswith("psm_reproject_set_range:") and "z_min" in msg and "NULL" not in msg
    for args, word in (((2, 4, 0), "source 2"), ((-1, 4, 0), "source -1"), ((0, 0, 0), "outputs == 0"), ((0, 8, 0), "output bits 0x8"),
                       ((0, 4, 2), "flag bits 0x2"), ((1, 4, 1), "PSM_DEPTH_USE_MASK")):
        assert lib.psm_reproject(None, *args, C.byref(n)) != 0
        msg = built.last_error(None)
        assert msg.startswith("psm_reproject:") and word in msg and "NULL" not in msg, msg


class _Recorder:
    """stands where the loaded library stands in a DispEst: every psm_* call is recorded and succeeds; psm_reproject keeps 5
    pixels, psm_reproject_download_cloud writes 5 records"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args[1:]))
            if name in ("psm_reproject", "psm_reproject_wait"):
                args[-1]._obj.value = 5
            if name == "psm_reproject_download_cloud":
                args[3]._obj.value = 5
            return 0
        return call


def _fake(dispest, maxDis=8, W=12, H=8):
    de = object.__new__(dispest.DispEst)
    de._lib, de._h, de.wid, de.hei, de.maxDis, de.options = _Recorder(), 1, W, H, maxDis, {}
    return de


def test_the_python_layer_reaches_the_calls(built):
    from primestereomatch_amd import dispest, rectify
    de = _fake(dispest)
    de.setReprojection(np.eye(4), crop=(3, 4), z_range=(0.5, 9.0))
    assert de.Reproject_GPU(built.PSM_DEPTH_SGM, built.PSM_DEPTH_XYZ | built.PSM_DEPTH_CLOUD) == 5
    xyz, z = de.reprojected()
    assert xyz.shape == (8, 12, 3) and xyz.dtype == np.float32 and z is None
    cl = de.cloud()
    assert cl.shape == (5,) and cl.dtype == built.point_dtype()
    names = [n for n, _ in de._lib.calls]
    assert names == ["psm_reproject_set_q", "psm_reproject_set_range", "psm_reproject", "psm_reproject_download",
                     "psm_reproject_download_cloud"]
    assert de._lib.calls[0][1][1:] == (3, 4) and de._lib.calls[1][1] == (0.5, 9.0)
    assert de._lib.calls[2][1][:3] == (1, 5, 0)
    de.Reproject_GPU(built.PSM_DEPTH_GIF, built.PSM_DEPTH_Z, use_mask=True)
    assert de._lib.calls[-1][1][:3] == (0, 2, 1)
    with pytest.raises(ValueError):
        de.setReprojection(np.eye(3))
    assert dispest.reproject_batch([]) == []
    assert dispest.reproject_batch([de], built.PSM_DEPTH_GIF, built.PSM_DEPTH_CLOUD) == [0] and de._lib.calls[-1][0] == "psm_reproject_batch"
    p = inspect.signature(dispest.FrameRing.__init__).parameters
    assert p["reproject"].default == 0
    assert hasattr(dispest.FrameRing, "setReprojection") and hasattr(dispest.FrameRing, "push_async")
    # a rectification that carries Q sets the reprojection too, with the crop's origin
    de = _fake(dispest)
    xy, fr = np.zeros((8, 12, 2), np.int16), np.zeros((8, 12), np.uint16)
    rect = rectify.Rectification((xy, xy), (fr, fr), 12, 8)                  # (the fields Q and crop have defaults)
    assert rect.Q is None and rect.crop == (0, 0, 12, 8)
    de.setRectification(rect)
    assert "psm_reproject_set_q" not in [n for n, _ in de._lib.calls]
    rect = rectify.Rectification((xy, xy), (fr, fr), 40, 30, (5, 6, 12, 8), np.eye(4))
    de.setRectification(rect)
    assert [a[1:] for n, a in de._lib.calls if n == "psm_reproject_set_q"] == [(5, 6)]


def test_the_harness_keeps_depth_off_by_default_and_writes_ply(built, tmp_path):
    from primestereomatch_amd import harness
    for f in (harness.compute, harness.compute_sgbm):
        assert inspect.signature(f).parameters["depth"].default is False
        assert "depth" in f.__doc__
    cloud = np.zeros(3, built.point_dtype())
    cloud["x"], cloud["y"], cloud["z"] = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]
    cloud["b"], cloud["g"], cloud["r"], cloud["a"] = [1, 2, 3], [4, 5, 6], [7, 8, 9], 255
    path = tmp_path / "c.ply"
    harness.write_ply(str(path), cloud)
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n")
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\n")
    assert head.count(b"property float") == 3 and head.count(b"property uchar") == 3 and b"element face" not in head
    v = np.frombuffer(body, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    assert v.shape == (3,) and v["p"].tolist() == [[1, 4, 7], [2, 5, 8], [3, 6, 9]] and v["c"].tolist() == [[7, 4, 1], [8, 5, 2], [9, 6, 3]]
    harness.write_ply(str(path), cloud[:0])
    assert b"element vertex 0\n" in path.read_bytes()


def test_the_header_and_the_documents_carry_the_definition():
    text = open(os.path.join(ROOT, "include", "primesm_hip.h")).read()
    assert re.search(r"int psm_reproject\(psm_ctx \*ctx, int source, int outputs, int flags, uint32_t \*count\);", text)
    for phrase in ("PSM_DEPTH_GIF = 0, PSM_DEPTH_SGM = 1", "PSM_DEPTH_XYZ = 1, PSM_DEPTH_Z = 2, PSM_DEPTH_CLOUD = 4", "PSM_DEPTH_USE_MASK = 1",
                   "0x7FC00000", "tests/depth_model.py", "r = 1.0 / s_3", "unpinned"):
        assert phrase in text, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for phrase in ("psm_reproject", "private_segment_fixed_size", "unpinned", "k_dp_scan"):
        assert phrase in design, phrase
    assert "camProps.Q" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "psm_reproject" in open(os.path.join(ROOT, "README.md")).read()


def test_host_demo_builds_with_the_stage(built):
    host = os.path.join(ROOT, "primestereomatch_amd", "host")
    subprocess.run(["make", "-C", host], check=True, capture_output=True)
    demo = os.path.join(ROOT, "primestereomatch_amd", "lib", "psm_demo")
    assert os.path.exists(demo)
    hdr = open(os.path.join(host, "DispEst.h")).read()
    for decl in ("int setReprojection(const double Q[16]", "int Reproject(int source", "cloud() const"):
        assert decl in hdr
    blob = open(demo, "rb").read()
    assert b"psm_reproject_download_cloud" in blob and b"--ply" in blob and b"binary_little_endian" in blob      # hipUtil binds the symbols by name
