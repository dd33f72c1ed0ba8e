"""Times the WLS smoothing stage (psm_wls_filter: the Fast Global Smoother over the int16 disparity map) beside the numpy model: one
JSON line per size and iteration count, and the same lines into profiles/wls_bench.txt.

  kernels_ms    device time of the 1 + 2 T launches of one psm_wls_filter (PSM_OPT_PROFILE: k_wls_init, k_wls_rows, k_wls_cols);
                best of --reps
  call_ms       the synchronous call on the host clock; best of --reps
  ns_per_step   kernels_ms over the steps one lane walks in a call, T * 2 * (W + H) (a forward and a back sweep of every row
                pass and every column pass): constant over the sizes if the serial chain binds
  gbps          the bytes all passes move (about 250 per pixel at T = 3: bytes_per_pixel) over kernels_ms: near the copy
                ceiling if the bytes bind
  model_ms      the numpy model (tests/wls_model.py) on this machine's host, one thread; mean of --host-reps

The maps are random with 30 % missing, the guide is a smooth image with edges.  Usage: python scripts/wls_bench.py [--reps N]
[--host-reps N] [--only WxH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((450, 375, 64), (1280, 720, 128), (1920, 1080, 256))


def inputs(W, H, D, seed):
    rng = np.random.default_rng(seed)
    d16 = rng.integers(16, 16 * D, (H, W)).astype(np.int16)
    d16[rng.random((H, W)) < 0.3] = -16
    yy, xx = np.mgrid[0:H, 0:W]
    base = (96 + 40 * np.sin(xx / 37.0) + 30 * np.cos(yy / 23.0) + 50 * ((xx // 160 + yy // 120) % 2))[..., None]
    left = np.clip(base + rng.integers(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)
    return d16, left


def bytes_per_pixel(T):
    """k_wls_init: the map, the guide and its two neighbours (cached), num, den, kh, kv; a pass: forward reads num, den, a link
    byte and writes cp, np, dp, back reads those and writes num, den; the last column pass also writes q and the int16 map"""
    return (2 + 3 + 8 + 2) + T * 2 * (9 + 12 + 12 + 8) + 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import wls_model as M
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    emit({"what": "wls_bench", "reps": a.reps, "lambda": 8000.0, "sigma": 1.5})
    for W, H, D in SIZES:
        if a.only and a.only != f"{W}x{H}":
            continue
        d16, left = inputs(W, H, D, 1)
        with P.DispEst(left, left, D) as de:
            de.set_option(capi.PSM_OPT_PROFILE, 1)
            de.upload_sgm_map(d16)
            for T in (1, 3):
                t = []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    model = M.wls(d16, -16, left, iterations=T)
                    t.append((time.perf_counter() - t0) * 1e3)
                de.setWLS(iterations=T)
                de.WLS_GPU(capi.PSM_WLS_SGM)                             # (first use: the stage's planes)
                same = bool(np.array_equal(de.wls_map(), model["disp"]))
                kern, call = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    de.WLS_GPU(capi.PSM_WLS_SGM)
                    call.append((time.perf_counter() - t0) * 1e3)
                    kern.append(de.wls_time())
                ms = min(kern)
                emit({"size": f"{W}x{H}", "iterations": T, "kernels_ms": round(ms, 4), "call_ms": round(min(call), 4),
                      "ns_per_step": round(ms * 1e6 / (T * 2 * (W + H)), 1), "bytes_per_pixel": bytes_per_pixel(T),
                      "gbps": round(bytes_per_pixel(T) * W * H / (ms * 1e-3) / 1e9, 1), "model_ms": round(float(np.mean(t)), 1),
                      "void": int((model["disp"] == -16).sum()), "equals_model": same})
    with open(os.path.join(ROOT, "profiles", "wls_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
