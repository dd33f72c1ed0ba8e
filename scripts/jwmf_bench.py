"""Times psm_joint_wmf (the device JointWMF post-filter) per image pair: one JSON line per size.

  whole_ms      the call with the default clustering (device k-means, host looks at its convergence flag)
  median_ms     the call with both clusterings set by the host: weight tables, cluster planes and the median kernel
  (every timed call is on a freshly uploaded pair: the library keeps a pair's clustering and tables between calls)
  cluster_ms    the difference: keys, samples, k-means++ seeding and Lloyd iterations of both images
  kernels_ms    device time of the PSM_K_JWMF launches of one default call (PSM_OPT_PROFILE 1)
  cpu_reading_ms  CPU baseline: one thread running tests/jwmf_reading.c - a serial port of the reference's filterCore column
                scan (not the reference binary) - on both maps with the device's clustering (k-means not included)

Usage: python scripts/jwmf_bench.py [--reps N] [--only NAME] [--no-cpu-baseline]"""
import argparse
import json
import os
import sys
import time

import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jwmf_model as M  # noqa: E402


def _pairs():
    from primestereomatch_amd import synth
    z = np.load(os.path.join(ROOT, "tests", "golden", "cones_pair.npz"))
    yield "cones_450x375", z["l_bgr"], z["r_bgr"], 64
    for W, H, D in ((1280, 720, 128), (1920, 1080, 256)):
        l, r, _ = synth.make_pair(W, H, D, seed=3)
        yield f"synthetic_{W}x{H}", l, r, D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="run only the pair whose name contains this")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    a = ap.parse_args()
    reading = None if a.no_cpu_baseline else M.load_reading(tempfile.mkdtemp())
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    for name, l, r, D in _pairs():
        if a.only and a.only not in name:
            continue
        H, W = l.shape[:2]
        rng = np.random.default_rng(0)
        lm, rm = rng.integers(0, D, (2, H, W), dtype=np.uint8)
        with P.DispEst(l, r, D) as de:
            def once(cl=None):
                de.setInputImages(l, r)                          # a new pair: no clustering or table survives
                if cl is not None:
                    for s in (0, 1):
                        de.set_jwmf_clusters(s, cl[s][0], cl[s][1])
                de.upload_maps(lm, rm)
                t = time.perf_counter()
                de.JointWMF_GPU()
                de.synchronize()
                return (time.perf_counter() - t) * 1e3
            once()                                               # warm-up (allocations)
            whole = min(once() for _ in range(a.reps))
            de.set_option(capi.PSM_OPT_PROFILE, 1)
            de.reset_kernel_times()
            once()
            kms, nk = de.kernel_time_ms(capi.PSM_K_JWMF)
            de.set_option(capi.PSM_OPT_PROFILE, 0)
            cl = [de.jwmf_clusters(s) for s in (0, 1)]
            once(cl)
            med = min(once(cl) for _ in range(a.reps))
        line = {"pair": name, "W": W, "H": H, "whole_ms": round(whole, 3), "median_ms": round(med, 3),
                "cluster_ms": round(whole - med, 3), "lloyd_iterations": [cl[0][2], cl[1][2]],
                "kernels_ms": round(kms, 3), "kernel_launches": nk}
        if reading is not None:
            t = time.perf_counter()
            for s, img, dmap in ((0, l, lm), (1, r, rm)):
                M.reading_core(reading, dmap, cl[s][1][M.keys_of(img)], M.weight_table(cl[s][0]), 9)
            cpu = (time.perf_counter() - t) * 1e3
            line.update({"cpu_reading_ms": round(cpu, 1), "speedup_median": round(cpu / med, 1),
                         "speedup_whole": round(cpu / whole, 1)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
