"""Times the reprojection stage (psm_reproject: cv::reprojectImageTo3D and the point cloud on the device) beside its two yardsticks:
one JSON line per size, source and output set, and the same lines into profiles/depth_bench.txt.

  kernels_ms    device time of the launches of one psm_reproject (PSM_OPT_PROFILE: k_dp_count, k_dp_scan, and k_dp_pack with the
                cloud); best of --reps
  call_ms       the synchronous call on the host clock (launches, the 4-byte count's copy, the wait); best of --reps
  floor_ms      the bytes the output set moves - the source map read once per launch that computes points, the dense planes
                written, the left image read and the kept records written - at the copy ceiling profiles/sgm_bench.txt records
  model_ms      the numpy model (tests/depth_model.py) on this machine's host, one thread, planes and cloud; mean of --host-reps
  batch8        (450 x 375 only) the same output sets for 8 contexts in one psm_reproject_batch: kernels_ms of the batch and per pair

The maps are random with one pixel in eight missing; the range keeps about half of the rest, so the cloud is neither empty nor
full.  Usage: python scripts/depth_bench.py [--reps N] [--host-reps N] [--only WxH]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((450, 375, 64), (1280, 720, 128), (1920, 1080, 256))
FALLBACK_CEILING_TBS = 6.29


def copy_ceiling_tbs():
    """The copy ceiling profiles/sgm_bench.txt records (TB/s)."""
    try:
        m = re.search(r'"copy_ceiling_TBps": ([0-9.]+)', open(os.path.join(ROOT, "profiles", "sgm_bench.txt")).read())
        return float(m.group(1)) if m else FALLBACK_CEILING_TBS
    except OSError:
        return FALLBACK_CEILING_TBS


def fixture_q():
    from primestereomatch_amd import rectify
    return rectify.read_opencv_yaml(os.path.join(ROOT, "tests", "golden", "zed_extrinsics.yml"))["Q"]


def inputs(W, H, D, seed):
    rng = np.random.default_rng(seed)
    lmap = rng.integers(1, D, (H, W), dtype=np.uint8)
    valid = (rng.random((H, W)) >= 0.125).astype(np.uint8) * 255
    d16 = rng.integers(16, 16 * D, (H, W)).astype(np.int16)
    d16[valid == 0] = -16
    left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return lmap, valid, d16, left


def z_range(Q, D):
    """(z_min, z_max] that keeps the disparities above D / 2: about half of the pixels that are not missing"""
    return 0.0, float(Q[2, 3] / (Q[3, 2] * (D / 2.0)))


def floor_ms(W, H, source, outputs, kept, ceiling_tbs, capi):
    n = W * H
    src = 2 * n                                                       # the int16 map, or the u8 map and its u8 mask
    b = src
    if outputs & capi.PSM_DEPTH_XYZ:
        b += 12 * n
    if outputs & capi.PSM_DEPTH_Z:
        b += 4 * n
    if outputs & capi.PSM_DEPTH_CLOUD:
        b += src + 3 * n + 16 * kept                                  # the pack launch reads the map again, and the image
    return b / (ceiling_tbs * 1e12) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import depth_model as M
    import primestereomatch_amd as P
    from primestereomatch_amd import capi, dispest
    Q = fixture_q()
    ceiling = copy_ceiling_tbs()
    sets = (("xyz", capi.PSM_DEPTH_XYZ), ("z", capi.PSM_DEPTH_Z), ("cloud", capi.PSM_DEPTH_CLOUD),
            ("xyz+z+cloud", capi.PSM_DEPTH_XYZ | capi.PSM_DEPTH_Z | capi.PSM_DEPTH_CLOUD))
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    emit({"what": "depth_bench", "copy_ceiling_tbs": ceiling, "reps": a.reps})
    for W, H, D in SIZES:
        if a.only and a.only != f"{W}x{H}":
            continue
        lmap, valid, d16, left = inputs(W, H, D, 1)
        zr = z_range(Q, D)
        model = {}
        for name, dm in (("gif", M.gif_disparity(lmap, valid)), ("sgm", M.sgm_disparity(d16))):
            t = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                M.reproject(*dm, Q, (0, 0), zr, left)
                t.append((time.perf_counter() - t0) * 1e3)
            model[name] = round(float(np.mean(t)), 2)
        with P.DispEst(left, left, D) as de:
            de.set_option(capi.PSM_OPT_PROFILE, 1)
            de.setReprojection(Q, (0, 0), zr)
            de.upload_maps(lmap, lmap, valid, valid)
            de.upload_sgm_map(d16)
            for sname, source, mask in (("gif", capi.PSM_DEPTH_GIF, True), ("sgm", capi.PSM_DEPTH_SGM, False)):
                for oname, outputs in sets:
                    kept = de.Reproject_GPU(source, outputs, use_mask=mask)      # (first use: the stage's scratch)
                    kern, call = [], []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        de.Reproject_GPU(source, outputs, use_mask=mask)
                        call.append((time.perf_counter() - t0) * 1e3)
                        kern.append(de.reproject_time())
                    emit({"size": f"{W}x{H}", "source": sname, "outputs": oname, "kept": kept, "kernels_ms": round(min(kern), 4),
                          "call_ms": round(min(call), 4), "floor_ms": round(floor_ms(W, H, source, outputs, kept, ceiling, capi), 4),
                          "model_ms": model[sname]})
        if (W, H) == (450, 375):
            des = [P.DispEst(left, left, D) for _ in range(8)]
            try:
                des[0].set_option(capi.PSM_OPT_PROFILE, 1)
                for i, d in enumerate(des):
                    li, vi, di, _ = inputs(W, H, D, 10 + i)
                    d.setReprojection(Q, (0, 0), zr)
                    d.upload_maps(li, li, vi, vi)
                    d.upload_sgm_map(di)
                for sname, source, mask in (("gif", capi.PSM_DEPTH_GIF, True), ("sgm", capi.PSM_DEPTH_SGM, False)):
                    for oname, outputs in sets:
                        dispest.reproject_batch(des, source, outputs, use_mask=mask)
                        kern = []
                        for _ in range(a.reps):
                            dispest.reproject_batch(des, source, outputs, use_mask=mask)
                            kern.append(des[0].reproject_time())
                        emit({"size": f"{W}x{H}", "batch": 8, "source": sname, "outputs": oname, "kernels_ms": round(min(kern), 4),
                              "kernels_ms_per_pair": round(min(kern) / 8, 4)})
            finally:
                for d in des:
                    d.close()
    with open(os.path.join(ROOT, "profiles", "depth_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
