"""Times psm_joint_wmf (the device JointWMF post-filter) per image pair: one JSON line per size.

  whole_ms      the call with the default clustering (device k-means, host looks at its convergence flag)
  median_ms     the call with both clusterings set by the host: weight tables, cluster planes and the median kernel
  (every timed call is on a freshly uploaded pair: the library keeps a pair's clustering and tables between calls)
  cluster_ms    the difference: keys, samples, k-means++ seeding and Lloyd iterations of both images
  kernels_ms    device time of the PSM_K_JWMF launches of one default call (PSM_OPT_PROFILE 1)
  cpu_reading_ms  CPU baseline: one thread running tests/jwmf_reading.c - a serial port of the reference's filterCore column
                scan (not the reference binary) - on both maps with the device's clustering (k-means not included)

--batch N[,N...]: instead of the above, several pairs per call (psm_joint_wmf_batch) beside the same pairs through single calls
one after the other: one JSON line per size and N - N at 450 x 375 (Cones, Teddy and synthetic pairs of that size), --batch-720p
(default 4) at 1280 x 720.  The pairs differ (a batch waits for its slowest clustering chain; flips of one image have the same
keys and so the same chain).  Every timed call is on freshly uploaded pairs, the maps stay on the device in both forms, the host
clock ends behind a synchronise, every shape is warmed first; best of --reps, *_spread_ms: max - min of the repetitions.
  single_whole_ms / batch_whole_ms      per pair, default clustering
  single_median_ms / batch_median_ms    per pair, clusterings set by the host (no k-means: tables, planes, median)
  batch_kernels_ms, batch_kernel_launches   PSM_K_JWMF of ctxs[0] over one default batch call (PSM_OPT_PROFILE 1)

Usage: python scripts/jwmf_bench.py [--reps N] [--only NAME] [--no-cpu-baseline] [--batch N[,N...]] [--batch-720p N]"""
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


def _batch_pairs(W, H, D, n):
    """n different pairs of one size: at 450 x 375 Cones and Teddy first, synthetic seeds behind them."""
    from primestereomatch_amd import synth
    out = []
    if (W, H) == (450, 375):
        for name in ("cones", "teddy"):
            z = np.load(os.path.join(ROOT, "tests", "golden", f"{name}_pair.npz"))
            out.append((z["l_bgr"], z["r_bgr"]))
    seed = 3
    while len(out) < n:
        l, r, _ = synth.make_pair(W, H, D, seed=seed)
        out.append((l, r))
        seed += 1
    return out[:n]


def _batch(W, H, D, N, reps):
    import primestereomatch_amd as P
    from primestereomatch_amd import capi, dispest
    pairs = _batch_pairs(W, H, D, N)
    rng = np.random.default_rng(0)
    maps = [rng.integers(0, D, (2, H, W), dtype=np.uint8) for _ in range(N)]
    des = [P.DispEst(l, r, D) for l, r in pairs]
    try:
        def fresh(cl):
            for i, d in enumerate(des):
                d.setInputImages(*pairs[i])                      # a new pair: no clustering or table survives
                if cl is not None:
                    for s in (0, 1):
                        d.set_jwmf_clusters(s, cl[i][s][0], cl[i][s][1])
                d.upload_maps(*maps[i])
            for d in des:
                d.synchronize()

        def singles(cl=None):
            fresh(cl)
            t = time.perf_counter()
            for d in des:
                d._ck(d._lib.psm_joint_wmf(d._h, 0, 0.0, 0, 0, None, None, 0), "joint_wmf")
            for d in des:
                d.synchronize()
            return (time.perf_counter() - t) * 1e3 / N

        def batch(cl=None):
            fresh(cl)
            t = time.perf_counter()
            dispest.joint_wmf_batch_device(des)
            for d in des:
                d.synchronize()
            return (time.perf_counter() - t) * 1e3 / N

        singles()                                                # warm-up (allocations), both forms
        ref = [tuple(m.copy() for m in d.download_maps()) for d in des]
        cl = [[d.jwmf_clusters(s) for s in (0, 1)] for d in des]
        batch()
        same = all(np.array_equal(a, b) for d, r in zip(des, ref) for a, b in zip(d.download_maps(), r))
        same = same and all(d.jwmf_clusters(s)[2] == cl[i][s][2] for i, d in enumerate(des) for s in (0, 1))
        ts, tb = [singles() for _ in range(reps)], [batch() for _ in range(reps)]
        des[0].set_option(capi.PSM_OPT_PROFILE, 1)
        des[0].reset_kernel_times()
        batch()
        kms, nk = des[0].kernel_time_ms(capi.PSM_K_JWMF)
        des[0].set_option(capi.PSM_OPT_PROFILE, 0)
        singles(cl), batch(cl)
        ms, mb = [singles(cl) for _ in range(reps)], [batch(cl) for _ in range(reps)]
    finally:
        for d in des:
            d.close()
    r3 = lambda v: round(v, 3)
    print(json.dumps({"batch": f"{W}x{H}", "N": N, "reps": reps, "same_maps_and_iterations": bool(same),
                      "single_whole_ms": r3(min(ts)), "single_whole_spread_ms": r3(max(ts) - min(ts)),
                      "batch_whole_ms": r3(min(tb)), "batch_whole_spread_ms": r3(max(tb) - min(tb)),
                      "whole_ratio": r3(min(tb) / min(ts)),
                      "single_median_ms": r3(min(ms)), "single_median_spread_ms": r3(max(ms) - min(ms)),
                      "batch_median_ms": r3(min(mb)), "batch_median_spread_ms": r3(max(mb) - min(mb)),
                      "median_ratio": r3(min(mb) / min(ms)),
                      "lloyd_iterations": [[c[0][2], c[1][2]] for c in cl],
                      "batch_kernels_ms": r3(kms), "batch_kernel_launches": nk}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="run only the pair whose name contains this")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--batch", default=None, help="N[,N...]: time psm_joint_wmf_batch at these batch sizes (450 x 375) beside the singles")
    ap.add_argument("--batch-720p", type=int, default=4, help="with --batch: the batch size at 1280 x 720 (0: skip)")
    a = ap.parse_args()
    if a.batch:
        for N in [int(v) for v in a.batch.split(",")]:
            _batch(450, 375, 64, N, a.reps)
        if a.batch_720p > 0:
            _batch(1280, 720, 128, a.batch_720p, a.reps)
        return
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
