#!/usr/bin/env python3
"""Timing of the semi-global matching stage (psm_sgm_compute: k_sgm_cost, 8 x k_sgm_path, k_sgm_select + k_sgm_check).
One JSON line per configuration on stdout and, with --out, appended to that file (profiles/sgm_bench.txt).

Configurations: 450 x 375 x 64 (the Cones pair, tests/golden), 1280 x 720 x 128 and 1920 x 1080 x 256 (synth.make_pair).
Per configuration, in one process: --warmup computes, then --runs computes under PSM_OPT_PROFILE 1; reported are the medians of
the three kernel-group times of psm_sgm_times (hipEvents on the stream) and of their sum, the bytes the design moves by its own
accounting (per element of the padded volumes, Dp = D rounded up to 4: C written once, 2 B; per direction C read, 2 B, S read
and written, 8 B - the first direction only writes; S read once by the selection, 4 B: 82 B; plus the images and the planes),
those bytes over the total as a fraction of the part's measured copy ceiling (6.29 TB/s, float4 copy), and the device memory
the stage holds.  --model: also time the numpy model (tests/sgm_model.py) on the same pair, for scale; --model-only does just
that and needs no GPU (the large pairs take minutes and gigabytes).

--min-disparity M, --num-disparities N (psm_sgm_set_range): the same record over the disparities M .. M + N - 1 instead of
0 .. D - 1, N up to 1024 whatever the configuration's D (the context keeps max_disp = min(D, 256)); the configurations 1080p512,
1080p1024 and 4k512 (1920 x 1080 x 512 / x 1024, 3840 x 2160 x 512) set N themselves.  Dp is then N rounded up to 8 (N > 256) or
16 (N > 512), and "valid" means != (M - 1) * 16.

--mode: StereoSGBM's reduced modes beside hh - modes_bench below.

The speckle filter (psm_sgm_set_speckle; k_spk_runs, k_spk_merge, k_spk_count, k_spk_apply): every configuration is timed twice in
the same process, with the filter off (the record above, unchanged) and on at the reference's (100, 32) - "speckle_ms", the median
of psm_sgm_speckle_time, and the three group times of those runs as "*_ms_speckle_on".  --speckle-maps: also two 1920 x 1080
maps through psm_sgm_filter_speckles at (-16, 100, 512): a serpentine (the whole image one path) and a constant map.

The prefiltered Birchfield-Tomasi cost (psm_sgm_set_prefilter; k_sgm_prefilter, k_sgm_bt_rows, k_sgm_bt_cols): every configuration
is timed a third time in the same process at pre_filter_cap 63 with the filter off - the three group times as "*_ms_cap63" (the
cost group holds the prefilter), their ratio to the SAD cost group, and the 12 W H bytes of planes the stage then holds.

--census W,H: the census cost (psm_sgm_set_census; k_sgm_census, k_sgm_census_cost): every configuration is timed once more in the
same process with that window, at pre_filter_cap 0 with the filter off - the three group times as "*_ms_census" (the cost group
holds the census transform), the cost group over the SAD and the Birchfield-Tomasi cost groups of the same process, the 16 W H
bytes of codes the stage then holds, and the floor of the cost group - C written once, 2 W H Dp bytes at the copy ceiling - over
its time.  With --batch the census cost is a third setting beside pre_filter_cap 0 and 63; --num-disparities works as ever.

--batch N[,N...]: instead of the above, several pairs per launch (psm_sgm_compute_batch).  Per configuration (450 x 375 x 64 and
1280 x 720 x 128 at the batch sizes given; 1920 x 1080 x 256, 3.2 GB per context, at those of them that are 2 or 4), at
pre_filter_cap 0 and 63 with the speckle filter on at (100, 32): per-pair ms of the three groups and of the filter for the batch
(psm_sgm_times / psm_sgm_speckle_time of its first context over N), beside the same N contexts run one after another through
psm_sgm_compute in the same process (the mean of their own times), hipEvents, median of --runs after --warmup, and the wall time
per pair of both.  --reps R: the whole pair of measurements R times, singles and batch alternating - the spread between the
repetitions is what a difference has to exceed.

--maps: instead of the above, the 8-bit maps of both views (psm_sgm_select_maps; k_sgm_maps) beside the group it is measured
against.  Per configuration (SAD cost, the configuration's D, filter off), --reps times over: --warmup rounds, then --runs rounds
of psm_sgm_compute, psm_sgm_select_maps with the maps left on the device, and the post-processing chain behind them (psm_lr_check,
psm_fill_invalid, psm_wgt_median, maps left on the device).  Reported per repetition: the medians of psm_sgm_times' third number
(select + check: the same S read once, one wave per pixel), of psm_sgm_maps_time and of the chain's wall time; over the
repetitions their medians and, as "*_spread", the smallest and largest - what a difference has to exceed - and the bytes the
launch moves (S once, 4 B per element of the padded volume, 2 B per pixel written) over its time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING = 6.29e12          # B/s
CONFIGS = {"cones": (450, 375, 64), "720p": (1280, 720, 128), "1080p": (1920, 1080, 256),
           "1080p512": (1920, 1080, 512), "1080p1024": (1920, 1080, 1024), "4k512": (3840, 2160, 512)}       # above 256: through the range


def the_pair(name):
    W, H, D = CONFIGS[name]
    if name == "cones":
        z = np.load(os.path.join(ROOT, "tests", "golden", "cones_pair.npz"))
        return z["l_bgr"], z["r_bgr"]
    from primestereomatch_amd import synth
    return synth.make_pair(W, H, D, seed=0)[:2]


def accounting(W, H, D):
    Dp = (D + 3) // 4 * 4 if D <= 256 else ((D + 7) // 8 * 8 if D <= 512 else (D + 15) // 16 * 16)
    vox = W * H * Dp
    moved = vox * (2 + 8 * 10 - 4 + 4) + W * H * (2 * 3 + 4 + 4 + 2 + 4 + 4 + 2 + 2)   # images; disp2 fill, atomics, probes; pre, out
    held = vox * 6 + W * H * (4 + 2 + 2)
    return Dp, moved, held


def model_seconds(l, r, D):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sgm_model as M
    t0 = time.perf_counter()
    M.sgm(l, r, D)
    return time.perf_counter() - t0


def speckle_maps(runs, warmup, out):
    """The filter alone on 1080p maps an SGM run never produces: device ms of its four launches, median of `runs`."""
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    W, H = 1920, 1080
    serp = np.full((H, W), 2000, np.int16)
    serp[0::2] = 160
    serp[1::4, W - 1] = 160
    serp[3::4, 0] = 160
    blank = np.zeros((H, W, 3), np.uint8)
    with P.DispEst(blank, blank, 2) as de:
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        for name, m in (("serpentine", serp), ("constant", np.full((H, W), 160, np.int16))):
            t = []
            for i in range(warmup + runs):
                de.filter_speckles(m, -16, 100, 512)
                if i >= warmup:
                    t.append(de.sgm_speckle_time())
            rec = {"bench": "speckle", "map": name, "W": W, "H": H, "args": [-16, 100, 512], "runs": runs, "warmup": warmup,
                   "speckle_ms": round(float(np.median(t)), 4), "speckle_ms_min_max": [round(min(t), 4), round(max(t), 4)],
                   "largest_component": int(de.sgm_speckle_sizes().max())}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")


def batch_pairs(name, n):
    """n pairs of the configuration's size: Cones and Teddy alternating at their size, synth pairs of n seeds elsewhere."""
    W, H, D = CONFIGS[name]
    if name == "cones":
        zs = [np.load(os.path.join(ROOT, "tests", "golden", f"{k}_pair.npz")) for k in ("cones", "teddy")]
        return [(zs[i % 2]["l_bgr"], zs[i % 2]["r_bgr"]) for i in range(n)]
    from primestereomatch_amd import synth
    return [synth.make_pair(W, H, D, seed=i)[:2] for i in range(n)]


def batch_bench(a):
    import primestereomatch_amd as P
    from primestereomatch_amd import capi, dispest
    if capi.device_count() < 1:
        raise SystemExit("sgm_bench: no HIP device visible")
    sizes = sorted({int(v) for v in a.batch.split(",")})
    for name in a.configs.split(","):
        W, H, D = CONFIGS[name]
        ns = [n for n in sizes if name != "1080p" or n in (2, 4)]
        if not ns:
            continue
        des = [P.DispEst(l, r, D) for l, r in batch_pairs(name, max(ns))]
        try:
            for de in des:
                de.set_option(capi.PSM_OPT_PROFILE, 1)
            for cap, census in [(0, None), (63, None)] + ([(0, a.census)] if a.census else []):
                kw = dict(pre_filter_cap=cap, census=census, speckle_window_size=100, speckle_range=32)
                for n in ns:
                    sub = des[:n]

                    def singles():
                        t, wall = [], []
                        for i in range(a.warmup + a.runs):
                            w0 = time.perf_counter()
                            for de in sub:
                                de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
                            w = (time.perf_counter() - w0) * 1e3 / n
                            if i >= a.warmup:
                                wall.append(w)
                                t.append(np.mean([list(de.sgm_times()) + [de.sgm_speckle_time()] for de in sub], axis=0))
                        return np.median(np.array(t), axis=0), float(np.median(wall))

                    def batch():
                        t, wall = [], []
                        for i in range(a.warmup + a.runs):
                            w0 = time.perf_counter()
                            dispest.sgm_compute_batch(sub)
                            w = (time.perf_counter() - w0) * 1e3 / n
                            if i >= a.warmup:
                                wall.append(w)
                                t.append(np.array(list(sub[0].sgm_times()) + [sub[0].sgm_speckle_time()]) / n)
                        return np.median(np.array(t), axis=0), float(np.median(wall))

                    maps1 = [de.SGBM_GPU(**kw) for de in sub]                      # (sets the parameters of every context)
                    same = all(np.array_equal(x, y) for x, y in zip(maps1, dispest.sgbm_batch(sub, **kw)))
                    for rep_i in range(a.reps):
                        s_t, s_w = singles()
                        b_t, b_w = batch()
                        rec = {"bench": "sgm_batch", "config": name, "W": W, "H": H, "D": D, "pre_filter_cap": cap, "speckle": [100, 32],
                               "batch": n, "rep": rep_i, "runs": a.runs, "warmup": a.warmup, "maps_equal_singles": bool(same)}
                        if census:
                            rec["census"] = list(census)
                        for tag, t, w in (("singles", s_t, s_w), ("batch", b_t, b_w)):
                            rec[tag + "_per_pair_ms"] = {"cost": round(float(t[0]), 4), "paths": round(float(t[1]), 4), "select": round(float(t[2]), 4),
                                                         "speckle": round(float(t[3]), 4), "total": round(float(t.sum()), 4), "wall": round(w, 4)}
                        rec["batch_over_singles_total"] = round(float(b_t.sum() / s_t.sum()), 3)
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if a.out:
                            with open(a.out, "a") as f:
                                f.write(line + "\n")
        finally:
            for de in des:
                de.close()


def modes_bench(a):
    """--mode M[,M...] [--batch N]: the reduced modes (psm_sgm_set_mode) on one context per configuration, in one process.  Per
    repetition (--reps) the sequence hh, then every mode in turn; per entry --warmup computes, then the medians of psm_sgm_times
    over --runs computes.  One record per (configuration, rep, mode) with the three groups, the paths group over hh's of the same
    repetition and, at the Cones size, bp_percent_int of Cones / Teddy.  With --batch N the same for a batch of N pairs, per
    pair."""
    import primestereomatch_amd as P
    from primestereomatch_amd import capi, dispest, harness
    if capi.device_count() < 1:
        raise SystemExit("sgm_bench: no HIP device visible")
    modes = a.mode.split(",")
    n = int(a.batch) if a.batch else 1
    for name in a.configs.split(","):
        W, H, D = CONFIGS[name]
        des = [P.DispEst(l, r, D) for l, r in batch_pairs(name, max(n, 2 if name == "cones" else 1))]
        try:
            sub = des[:n]
            sub[0].set_option(capi.PSM_OPT_PROFILE, 1)
            bp = {}
            if name == "cones":                                     # des[0]: Cones, des[1]: Teddy
                for k, de in zip(("cones", "teddy"), des):
                    z = np.load(os.path.join(ROOT, "tests", "golden", f"{k}_pair.npz"))
                    for mode in ["hh"] + modes:
                        d16 = de.SGBM_GPU(mode=mode)
                        bp[k, mode] = round(float(harness.error_vs_ground_truth(np.maximum(d16, 0) >> 4, z["gt_l"], z["occl"], D, 4)[0]), 2)

            def timed(mode):
                dispest.sgbm_batch(sub, mode=mode)                                     # (sets every context; the first warm-up)
                t = []
                for i in range(a.warmup + a.runs):
                    if n == 1:
                        sub[0]._ck(sub[0]._lib.psm_sgm_compute(sub[0]._h), "psm_sgm_compute")
                    else:
                        dispest.sgm_compute_batch(sub)
                    if i >= a.warmup:
                        t.append(np.array(sub[0].sgm_times()) / n)
                return np.median(np.array(t), axis=0)

            for rep_i in range(a.reps):
                hh = timed("hh")
                for mode, t in [("hh", hh)] + [(mode, timed(mode)) for mode in modes]:
                    rec = {"bench": "sgm_modes", "config": name, "W": W, "H": H, "D": D, "batch": n, "rep": rep_i, "runs": a.runs,
                           "warmup": a.warmup, "mode": mode, "cost_ms": round(float(t[0]), 4),
                           "paths_ms": round(float(t[1]), 4), "select_ms": round(float(t[2]), 4),
                           "paths_over_hh": round(float(t[1] / hh[1]), 3), "total_over_hh": round(float(t.sum() / hh.sum()), 3)}
                    if bp:
                        rec["bp_percent_int"] = {k: bp[k, mode] for k in ("cones", "teddy")}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if a.out:
                        with open(a.out, "a") as f:
                            f.write(line + "\n")
        finally:
            for de in des:
                de.close()


def maps_bench(a):
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("sgm_bench: no HIP device visible")
    for name in a.configs.split(","):
        W, H, D = CONFIGS[name]
        if D > 256:
            continue                                               # (the maps are 8-bit)
        l, r = the_pair(name)
        Dp = (D + 3) & ~3
        sel, maps, chain = [], [], []
        with P.DispEst(l, r, D) as de:
            de.set_option(capi.PSM_OPT_PROFILE, 1)
            lib, h = de._lib, de._h

            def round_():
                de._ck(lib.psm_sgm_compute(h), "psm_sgm_compute")
                de._ck(lib.psm_sgm_select_maps(h, None, None, 0), "psm_sgm_select_maps")
                w0 = time.perf_counter()
                de._ck(lib.psm_lr_check(h, None, None, 0), "psm_lr_check")
                de._ck(lib.psm_fill_invalid(h, None, None, 0), "psm_fill_invalid")
                de._ck(lib.psm_wgt_median(h, None, None, 0), "psm_wgt_median")
                de.synchronize()
                return de.sgm_times()[2], de.sgm_maps_time(), (time.perf_counter() - w0) * 1e3

            de.SGBM_GPU()
            for _ in range(a.reps):
                for _ in range(a.warmup):
                    round_()
                t = np.array([round_() for _ in range(a.runs)])
                m = np.median(t, axis=0)
                sel.append(float(m[0])); maps.append(float(m[1])); chain.append(float(m[2]))
        moved = 4 * W * H * Dp + 2 * W * H
        rec = {"bench": "sgm_maps", "config": name, "W": W, "H": H, "D": D, "runs": a.runs, "warmup": a.warmup, "reps": a.reps}
        for key, v in (("select_ms", sel), ("maps_ms", maps), ("chain_wall_ms", chain)):
            rec[key] = round(float(np.median(v)), 4)
            rec[key + "_spread"] = [round(min(v), 4), round(max(v), 4)]
        rec.update({"maps_over_select": round(rec["maps_ms"] / rec["select_ms"], 3), "maps_bytes_moved": int(moved),
                    "maps_fraction_of_copy_ceiling": round(moved / COPY_CEILING * 1e3 / rec["maps_ms"], 4)})
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cones,720p,1080p")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--model-only", action="store_true")
    ap.add_argument("--speckle-maps", action="store_true")
    ap.add_argument("--batch", default=None, help="N[,N...]: time psm_sgm_compute_batch at these batch sizes beside the singles")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--mode", default=None, help="M[,M...] of sgbm, 3way, hh4: time these modes beside hh (modes_bench)")
    ap.add_argument("--min-disparity", type=int, default=0, help="psm_sgm_set_range: the first disparity")
    ap.add_argument("--num-disparities", type=int, default=0, help="psm_sgm_set_range: their number, up to 1024 (0: the configuration's D)")
    ap.add_argument("--census", default=None, help="W,H: also time the census cost with this window (psm_sgm_set_census)")
    ap.add_argument("--maps", action="store_true", help="time psm_sgm_select_maps beside the select group and the chain behind it (maps_bench)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 1
    a.census = tuple(int(v) for v in a.census.split(",")) if a.census else None
    if a.census and a.mode:
        raise SystemExit("sgm_bench: --census goes with the plain record and with --batch")
    if (a.mode or a.batch) and (a.min_disparity or a.num_disparities):
        raise SystemExit("sgm_bench: --min-disparity / --num-disparities go with the plain record only")
    if a.maps:
        return maps_bench(a)
    if a.mode:
        return modes_bench(a)
    if a.batch:
        return batch_bench(a)
    for name in a.configs.split(","):
        W, H, D = CONFIGS[name]
        l, r = the_pair(name)
        maxdis = min(D, 256)
        nd = a.num_disparities or (D if D > 256 else 0)
        D = nd or D
        rng = dict(min_disparity=a.min_disparity, num_disparities=nd) if nd or a.min_disparity else {}
        invalid = (a.min_disparity - 1) * 16
        Dp, moved, held = accounting(W, H, D)
        rec = {"bench": "sgm", "config": name, "W": W, "H": H, "D": D, "Dp": Dp}
        if rng:
            rec["range"] = [a.min_disparity, nd]
        if not a.model_only:
            import primestereomatch_amd as P
            from primestereomatch_amd import capi
            if capi.device_count() < 1:
                raise SystemExit("sgm_bench: no HIP device visible")
            with P.DispEst(l, r, maxdis) as de:
                de.set_option(capi.PSM_OPT_PROFILE, 1)
                for _ in range(a.warmup):
                    de.SGBM_GPU(**rng)
                t, wall = [], []
                for _ in range(a.runs):
                    w0 = time.perf_counter()
                    de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")
                    wall.append((time.perf_counter() - w0) * 1e3)
                    t.append(de.sgm_times())
                disp = de.sgm_disparity()
                for _ in range(a.warmup):
                    de.SGBM_GPU(speckle_window_size=100, speckle_range=32, **rng)
                ts, tk = [], []
                for _ in range(a.runs):
                    de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")      # (the setting holds)
                    ts.append(de.sgm_times())
                    tk.append(de.sgm_speckle_time())
                removed = int(np.count_nonzero(de.sgm_disparity() != disp))
                for _ in range(a.warmup):
                    de.SGBM_GPU(pre_filter_cap=63, **rng)
                tb = []
                for _ in range(a.runs):
                    de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")      # (the setting holds)
                    tb.append(de.sgm_times())
                valid_bt = float((de.sgm_disparity() != invalid).mean())
                tc = []
                if a.census:
                    for _ in range(a.warmup):
                        de.SGBM_GPU(census=a.census, **rng)
                    for _ in range(a.runs):
                        de._ck(de._lib.psm_sgm_compute(de._h), "psm_sgm_compute")      # (the setting holds)
                        tc.append(de.sgm_times())
                    valid_census = float((de.sgm_disparity() != invalid).mean())
            t = np.array(t)
            meds = np.median(np.array(ts), axis=0)
            medb = np.median(np.array(tb), axis=0)
            med = np.median(t, axis=0)
            total = float(np.median(t.sum(axis=1)))
            rec.update({"runs": a.runs, "warmup": a.warmup, "cost_ms": round(float(med[0]), 4), "paths_ms": round(float(med[1]), 4),
                        "select_ms": round(float(med[2]), 4), "total_ms": round(total, 4), "total_ms_min_max": [round(float(t.sum(axis=1).min()), 4), round(float(t.sum(axis=1).max()), 4)],
                        "wall_ms_median": round(float(np.median(wall)), 4), "bytes_moved": int(moved),
                        "fraction_of_copy_ceiling": round(moved / COPY_CEILING * 1e3 / total, 4), "copy_ceiling_TBps": COPY_CEILING / 1e12,
                        "device_bytes_held": int(held), "valid_fraction": round(float((disp != invalid).mean()), 4),
                        "speckle_ms": round(float(np.median(tk)), 4), "speckle_ms_min_max": [round(min(tk), 4), round(max(tk), 4)],
                        "cost_ms_speckle_on": round(float(meds[0]), 4), "paths_ms_speckle_on": round(float(meds[1]), 4),
                        "select_ms_speckle_on": round(float(meds[2]), 4), "speckle_pixels_removed": removed,
                        "cost_ms_cap63": round(float(medb[0]), 4), "paths_ms_cap63": round(float(medb[1]), 4),
                        "select_ms_cap63": round(float(medb[2]), 4), "cost_cap63_over_sad": round(float(medb[0] / med[0]), 2),
                        "cost_cap63_over_paths": round(float(medb[0] / medb[1]), 3), "prefiltered_bytes_held": 12 * W * H,
                        "valid_fraction_cap63": round(valid_bt, 4)})
            if tc:
                medc = np.median(np.array(tc), axis=0)
                floor_ms = 2 * W * H * Dp / COPY_CEILING * 1e3
                rec.update({"census": list(a.census), "cost_ms_census": round(float(medc[0]), 4), "paths_ms_census": round(float(medc[1]), 4),
                            "select_ms_census": round(float(medc[2]), 4), "cost_census_over_sad": round(float(medc[0] / med[0]), 2),
                            "cost_census_over_cap63": round(float(medc[0] / medb[0]), 2), "census_bytes_held": 16 * W * H,
                            "cost_census_floor_ms": round(floor_ms, 4), "cost_census_fraction_of_floor": round(float(floor_ms / medc[0]), 3),
                            "valid_fraction_census": round(valid_census, 4)})
        if a.model or a.model_only:
            rec["numpy_model_s"] = round(model_seconds(l, r, D), 2)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    if a.speckle_maps and not a.model_only:
        speckle_maps(a.runs, a.warmup, a.out)


if __name__ == "__main__":
    main()
