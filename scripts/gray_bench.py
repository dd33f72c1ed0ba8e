#!/usr/bin/env python3
"""Timing of the guided-filter path over a one-channel pair (psm_gray_compute: k_gray_prep, per chunk k_gray_ab + k_gray_q, k_merge)
beside the only thing a mono user could run before it: the unchanged colour default path (psm_cost_construct + psm_cost_filter +
psm_disp_select) on the tripled plane.  One JSON line per configuration on stdout and, with --out, appended to that file
(profiles/gray_bench.txt).

Configurations: 450 x 375 x 64 (the green planes of the Cones pair, tests/golden), 1280 x 720 x 128 and 1920 x 1080 x 256 (the green
planes of synth.make_pair).  Per configuration, in one process and one session: --warmup rounds, then --runs rounds that alternate
the two paths; reported are the best and the median of
  gray_ms        psm_gray_time: device events around the launches of the call (PSM_OPT_PROFILE; the upload of the two planes, which the
                 call completes first, lies outside - as the upload of the colour pair lies outside the colour figure)
  gray_call_ms   device events on the stream around the whole call, upload included
  colour_ms      device events on the stream around construct + filter + select of the tripled pair, maps left on the device
and gray_ms over colour_ms (best over best).  The maps of the gray call are left on the device too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"cones": (450, 375, 64), "720p": (1280, 720, 128), "1080p": (1920, 1080, 256)}


def the_planes(name):
    W, H, D = CONFIGS[name]
    if name == "cones":
        z = np.load(os.path.join(ROOT, "tests", "golden", "cones_pair.npz"))
        l, r = z["l_bgr"], z["r_bgr"]
    else:
        from primestereomatch_amd import synth
        l, r = synth.make_pair(W, H, D, seed=0)[:2]
    return np.ascontiguousarray(l[:, :, 1]), np.ascontiguousarray(r[:, :, 1])


def bench(torch, name, warmup, runs):
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    W, H, D = CONFIGS[name]
    gl, gr = the_planes(name)
    l3, r3 = (np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) for g in (gl, gr))
    stream = torch.cuda.Stream()
    with P.DispEst.blank(H, W, D) as dg, P.DispEst(l3, r3, D) as dc:
        for d in (dg, dc):
            d.set_stream(stream.cuda_stream)
            d.set_option(capi.PSM_OPT_ASYNC, 1)
        dg.set_option(capi.PSM_OPT_PROFILE, 1)

        def events(run):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            run()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        def gray():
            dg.Gray_GPU(gl, gr, download=False)

        def colour():
            dc.CostConst_GPU()
            dc.CostFilter_GPU()
            dc._ck(dc._lib.psm_disp_select(dc._h, None, None, 0), "disp_select")

        for _ in range(warmup):
            events(gray)
            events(colour)
        g_ms, gc_ms, c_ms = [], [], []
        for _ in range(runs):
            gc_ms.append(events(gray))
            g_ms.append(dg.gray_time())
            c_ms.append(events(colour))
        gmaps = [m.copy() for m in dg.download_maps()]
        cmaps = [m.copy() for m in dc.download_maps()]
    rec = {"config": name, "size": f"{W}x{H}x{D}", "warmup": warmup, "runs": runs}
    for key, v in (("gray_ms", g_ms), ("gray_call_ms", gc_ms), ("colour_ms", c_ms)):
        rec[key] = {"best": round(min(v), 4), "median": round(float(np.median(v)), 4)}
    rec["gray_over_colour"] = round(min(g_ms) / min(c_ms), 4)
    rec["maps_differ_percent"] = round(100.0 * float(np.mean(gmaps[0] != cmaps[0])), 2)      # two different filters: for scale only
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS), help="default: all three")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    from primestereomatch_amd import capi
    capi.load()
    if capi.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("gray_bench: no HIP device visible (there is no CPU path to time)")
    for name in a.config or ["cones", "720p", "1080p"]:
        line = json.dumps(bench(torch, name, a.warmup, a.runs))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
