"""Host-side quantities of the image pair path of ONE build (argv[1]: the root to import the package from): wall time per call of
psm_upload_pair_async and psm_upload_pair_rectified_async in a running frame loop at 450 x 375 x 64 and 1920 x 1080 x 256, and of
psm_sgm_compute (launch to synchronise) at 450 x 375 x 64 in a context that has uploaded asynchronously.  One JSON line."""
import ctypes as C
import json
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np  # noqa: E402

import primestereomatch_amd as P  # noqa: E402
from primestereomatch_amd import capi  # noqa: E402
from primestereomatch_amd.rectify import Rectification  # noqa: E402

capi.load()
assert os.path.abspath(capi.LIB_PATH).startswith(root), capi.LIB_PATH
vp = C.c_void_p
out = {"root": root}
rng = np.random.default_rng(0)


def loop(de, upload, frames=28, skip=6):
    ts = []
    for i in range(frames):
        de.CostConst_GPU()
        t0 = time.perf_counter()
        rc = upload()
        ts.append(time.perf_counter() - t0)
        assert rc == 0
        de.CostFilter_GPU()
        de.DispSelect_device()
        if i > 0:
            de.download_maps_wait()
        de.download_maps_async()
    de.download_maps_wait()
    de.synchronize()
    return round(float(np.median(ts[skip:])) * 1e6, 2)


for name, (W, H, D) in (("450x375", (450, 375, 64)), ("1920x1080", (1920, 1080, 256))):
    l = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    with P.DispEst(l, r, D) as de:
        de.set_option(capi.PSM_OPT_ASYNC, 1)
        out[f"upload_async_us_{name}"] = loop(
            de, lambda: de._lib.psm_upload_pair_async(de._h, vp(l.ctypes.data), vp(r.ctypes.data), 3, l.strides[0], capi.PSM_IMG_U8))
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).astype(np.int16)
    fr = np.full((H, W), 16 * 32 + 16, np.uint16)
    rect = Rectification((xy, xy), (fr, fr), W, H, (0, 0, W, H))
    with P.DispEst(l, r, D) as de:
        de.set_option(capi.PSM_OPT_ASYNC, 1)
        de.setRectification(rect)
        out[f"upload_rectified_async_us_{name}"] = loop(
            de, lambda: de._lib.psm_upload_pair_rectified_async(de._h, vp(l.ctypes.data), vp(r.ctypes.data), 3, l.strides[0]))

W, H, D = 450, 375, 64
l = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
r = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
with P.DispEst(l, r, D) as de:
    de.setInputImages_async(l, r)
    de.CostConst_GPU()
    de.SGBM_GPU()
    ts = []
    for i in range(30):
        t0 = time.perf_counter()
        de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
        ts.append(time.perf_counter() - t0)
    out["sgm_compute_ms_450x375x64"] = round(float(np.median(ts[5:])) * 1e3, 4)
print(json.dumps(out))
