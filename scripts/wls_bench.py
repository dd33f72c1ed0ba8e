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

--batch: psm_wls_filter_batch instead - T = 3 and T = 1, 450 x 375 in batches of 1, 2, 4 and 8, 1280 x 720 of 1, 2 and 4,
1920 x 1080 of 1 and 2, every member with a map of its own; the lines are appended to profiles/wls_bench.txt as a new block.

  batch_ms_per_pair     device time of the 1 + 2 T launches of one psm_wls_filter_batch (PSM_OPT_PROFILE on its first context:
                        the instantiations of k_wls_init, k_wls_rows, k_wls_cols over the device table - k_wls_*_b in the blocks
                        recorded before they were templates) over the number of pairs; best of --reps
  singles_ms_per_pair   the same number of psm_wls_filter calls one after the other: the sum of their kernels_ms over the number
                        of pairs (the gaps between the calls are not in it); best of --reps
  single_ms             the single call of context 0 alone: kernels_ms of the default mode, the figure to set against the
                        parent commit's
  batch_call_ms_per_pair, singles_call_ms_per_pair   the same two on the host clock, synchronous calls
  ns_per_step           batch_ms (of the whole batch) over T * 2 * (W + H): what one step of the chain costs when n chains run
                        side by side - constant over n while the chain binds, growing once the device is full

--conf: PSM_WLS_CONFIDENCE - the two launches the graded confidence adds (k_sgm_right16, k_wls_conf), on the SGM stage's own result
of a synthetic pair (synth.make_pair) at 450 x 375 x 64, 1280 x 720 x 128 and 1920 x 1080 x 256; the lines are appended to
profiles/wls_bench.txt as a new block.  All device ms between events (PSM_OPT_PROFILE), best of --reps.

  conf_ms_both, conf_ms_lr, conf_ms_var   psm_wls_conf_time with both terms (k_sgm_right16 + k_wls_conf), with the L-R term alone
                        (k_sgm_right16 + k_wls_conf without its window), with the variance term alone (k_wls_conf alone, without
                        its gather of right16)
  sgm_maps_ms           k_sgm_maps of the same S in the same session (psm_sgm_maps_time): it reads S once and scatters the same
                        keys, so it is the yardstick of k_sgm_right16; right16_over_maps = (conf_ms_both - conf_ms_var) / sgm_maps_ms
                        bounds the ratio from above (the difference also holds k_wls_conf's gather of right16)
  s_floor_ms            S read once at the 6.29 TB/s copy ceiling of profiles/sgm_bench.txt
  flagged_ms, unflagged_ms   psm_wls_time of the whole call with and without the flag (T = 3)
  equals_model          450 x 375 only: disp, conf and right16 equal tests/wls_conf_model.py

The maps are random with 30 % missing, the guide is a smooth image with edges.  Usage: python scripts/wls_bench.py [--reps N]
[--host-reps N] [--only WxH] [--batch | --conf]"""
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
BATCHES = {(450, 375): (1, 2, 4, 8), (1280, 720): (1, 2, 4), (1920, 1080): (1, 2)}


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


def batch_bench(a, emit):
    import wls_model as M
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    emit({"what": "wls_bench --batch", "reps": a.reps, "lambda": 8000.0, "sigma": 1.5})
    for W, H, D in SIZES:
        if a.only and a.only != f"{W}x{H}":
            continue
        ns = BATCHES[(W, H)]
        pairs = [inputs(W, H, D, 1 + i) for i in range(max(ns))]
        des = [P.DispEst(left, left, 16) for _, left in pairs]         # (the stage reads no volume: the contexts' own D is small)
        try:
            for de, (d16, _) in zip(des, pairs):
                de.set_option(capi.PSM_OPT_PROFILE, 1)
                de.upload_sgm_map(d16)
            for T in (3, 1):
                for de in des:
                    de.setWLS(iterations=T)
                models = [M.wls(d16, -16, left, iterations=T)["disp"] for d16, left in pairs[:2]]
                for n in ns:
                    maps = P.wls_batch(des[:n])                         # (first use: the planes, the table of the records)
                    same = all(bool(np.array_equal(m, w)) for m, w in zip(maps, models))
                    batch, batch_call, singles, singles_call, single = [], [], [], [], []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        P.wls_batch(des[:n])
                        batch_call.append((time.perf_counter() - t0) * 1e3)
                        batch.append(des[0].wls_time())
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        for de in des[:n]:
                            de.WLS_GPU(capi.PSM_WLS_SGM)
                        singles_call.append((time.perf_counter() - t0) * 1e3)
                        each = [de.wls_time() for de in des[:n]]
                        singles.append(sum(each))
                        single.append(each[0])
                    ms = min(batch)
                    emit({"size": f"{W}x{H}", "iterations": T, "n": n, "batch_ms_per_pair": round(ms / n, 4),
                          "singles_ms_per_pair": round(min(singles) / n, 4), "single_ms": round(min(single), 4),
                          "batch_call_ms_per_pair": round(min(batch_call) / n, 4),
                          "singles_call_ms_per_pair": round(min(singles_call) / n, 4),
                          "ns_per_step": round(ms * 1e6 / (T * 2 * (W + H)), 1),
                          "gbps": round(n * bytes_per_pixel(T) * W * H / (ms * 1e-3) / 1e9, 1), "equals_model": same})
        finally:
            for de in des:
                de.close()


def conf_bench(a, emit):
    import wls_conf_model as CM
    import primestereomatch_amd as P
    from primestereomatch_amd import capi, synth
    emit({"what": "wls_bench --conf", "reps": a.reps, "lambda": 8000.0, "sigma": 1.5, "iterations": 3, **CM.DEFAULTS})
    for W, H, D in SIZES:
        if a.only and a.only != f"{W}x{H}":
            continue
        l, r, _ = synth.make_pair(W, H, D, seed=0)
        with P.DispEst(l, r, D) as de:
            de.set_option(capi.PSM_OPT_PROFILE, 1)
            m16 = de.SGBM_GPU()
            de.setWLS()

            def best(conf, what):
                t = []
                for _ in range(a.reps + 1):                             # (the first run allocates)
                    de.WLS_GPU(capi.PSM_WLS_SGM, confidence=conf)
                    t.append(what())
                return min(t[1:])

            both = best({}, de.wls_conf_time)
            flagged = best({}, de.wls_time)
            same = None
            if (W, H) == (450, 375):
                import depth_model as DM
                got = {"disp": de.wls_map()}
                got["conf"], got["right16"] = de.download_wls_confidence()
                model = CM.wls(m16, -16, DM.quantise(l), S=de.sgm_costs()[1], dmin=0)
                same = all(bool(np.array_equal(got[k], model[k])) for k in got)
            lr = best({"terms": capi.PSM_WLS_CONF_LR}, de.wls_conf_time)
            var = best({"terms": capi.PSM_WLS_CONF_VAR}, de.wls_conf_time)
            unflagged = best(None, de.wls_time)
            maps = []
            for _ in range(a.reps):
                de.SGBMSelect_GPU(download=False)
                maps.append(de.sgm_maps_time())
            floor = W * H * D * 4 / 6.29e12 * 1e3
            emit({"size": f"{W}x{H}x{D}", "conf_ms_both": round(both, 4), "conf_ms_lr": round(lr, 4), "conf_ms_var": round(var, 4),
                  "sgm_maps_ms": round(min(maps), 4), "right16_over_maps": round((both - var) / min(maps), 2), "s_floor_ms": round(floor, 4),
                  "flagged_ms": round(flagged, 4), "unflagged_ms": round(unflagged, 4), "void_in": int((m16 == -16).sum()), "equals_model": same})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--conf", action="store_true")
    a = ap.parse_args()
    import wls_model as M
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    if a.batch or a.conf:
        (conf_bench if a.conf else batch_bench)(a, emit)
        with open(os.path.join(ROOT, "profiles", "wls_bench.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
        return
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
