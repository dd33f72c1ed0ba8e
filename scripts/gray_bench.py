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
and gray_ms over colour_ms (best over best).  The maps of the gray call are left on the device too.

--batch: psm_gray_compute_batch beside a loop of single calls instead.  Per configuration (default: cones, and 720p with a batch of
4 alone) and per batch size 1 / 2 / 4 / 8, device ms per pair (psm_gray_time of the batch's first context over n) beside the per-pair
device ms of a loop of 8 psm_gray_compute calls on 8 contexts (the sum of their psm_gray_time over 8), and the single call's device
ms at all three configurations.  Every build of the library measured - this tree's, and with --parent-lib another build's (the
parent commit's, which has no batch: its loop of single calls and its single calls alone) - runs in child processes of its own,
through ctypes on the few symbols both builds have, --rounds times in alternation; a child warms up, then repeats --runs times.
Reported per build: the best and the median over all of its repeats, and the spread of its rounds' bests (max - min).  The block
is printed as JSON lines and, with --out, appended to that file.

--fgf S: psm_gray_compute_fgf at subsample rate S (2, 4 or 8) instead.  Per configuration, in one process and one session, --warmup
rounds, then --runs rounds that alternate three paths; reported are the best and the median of
  fgf_ms         psm_gray_time of psm_gray_compute_fgf: device events around its launches
  colour_fgf_ms  device events on the stream around the unchanged colour FGF path - psm_cost_construct + psm_cost_filter_fgf +
                 psm_disp_select - on the tripled plane: the only fast mode a mono user had before, and the yardstick
  gray_ms        psm_gray_time of psm_gray_compute, the full-resolution one-channel filter
and fgf_ms over colour_fgf_ms (best over best).  Then, at 450 x 375 x 64, psm_gray_compute_fgf_batch: device ms per pair in
batches of 2 / 4 / 8 (psm_gray_time of the first context over n) beside a loop of 8 single calls on 8 contexts, alternating."""
import argparse
import ctypes as C
import functools
import json
import os
import subprocess
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


# ---- --fgf ---------------------------------------------------------------------------------------------------------------
def fgf_bench(torch, name, s, warmup, runs):
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    W, H, D = CONFIGS[name]
    gl, gr = the_planes(name)
    l3, r3 = (np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) for g in (gl, gr))
    stream = torch.cuda.Stream()
    with P.DispEst.blank(H, W, D) as df, P.DispEst.blank(H, W, D) as dg, P.DispEst(l3, r3, D) as dc:
        for d in (df, dg, dc):
            d.set_stream(stream.cuda_stream)
            d.set_option(capi.PSM_OPT_ASYNC, 1)
        df.set_option(capi.PSM_OPT_PROFILE, 1)
        dg.set_option(capi.PSM_OPT_PROFILE, 1)
        dc.setSubsampleRate(s)

        def colour():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            dc.CostConst_GPU()
            dc.CostFilter_FGF_GPU()
            dc._ck(dc._lib.psm_disp_select(dc._h, None, None, 0), "disp_select")
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        def fgf():
            df.Gray_GPU(gl, gr, download=False, subsample_rate=s)
            return df.gray_time()

        def gray():
            dg.Gray_GPU(gl, gr, download=False)
            return dg.gray_time()

        paths = {"fgf_ms": fgf, "colour_fgf_ms": colour, "gray_ms": gray}
        for _ in range(warmup):
            for f in paths.values():
                f()
        res = {k: [] for k in paths}
        for _ in range(runs):
            for k, f in paths.items():
                res[k].append(f())
        fmaps = [m.copy() for m in df.download_maps()]
        cmaps = [m.copy() for m in dc.download_maps()]
    rec = {"config": name, "size": f"{W}x{H}x{D}", "fgf": s, "warmup": warmup, "runs": runs}
    for key, v in res.items():
        rec[key] = {"best": round(min(v), 4), "median": round(float(np.median(v)), 4)}
    rec["fgf_over_colour_fgf"] = round(min(res["fgf_ms"]) / min(res["colour_fgf_ms"]), 4)
    rec["maps_differ_percent"] = round(100.0 * float(np.mean(fmaps[0] != cmaps[0])), 2)      # one plane against three equal ones: for scale only
    return rec


def fgf_batch_bench(name, s, warmup, runs):
    """ms per pair: batches of 2 / 4 / 8 beside a loop of LOOP single calls, alternating"""
    import primestereomatch_amd as P
    from primestereomatch_amd import capi
    W, H, D = CONFIGS[name]
    gl, gr = the_planes(name)
    planes = [(np.ascontiguousarray(np.roll(gl, k, axis=0)), np.ascontiguousarray(np.roll(gr, k, axis=0))) for k in range(LOOP)]
    des = [P.DispEst.blank(H, W, D) for _ in range(LOOP)]
    try:
        for d in des:
            d.set_option(capi.PSM_OPT_PROFILE, 1)

        def loop():
            ms = 0.0
            for d, (l, r) in zip(des, planes):
                d.Gray_GPU(l, r, download=False, subsample_rate=s)
                ms += d.gray_time()
            return ms / LOOP

        def batch(n):
            P.gray_batch(des[:n], [p[0] for p in planes[:n]], [p[1] for p in planes[:n]], download=False, subsample_rate=s)
            return des[0].gray_time() / n

        forms = {f"loop{LOOP}": loop}
        for n in (2, 4, 8):
            forms[f"batch{n}"] = functools.partial(batch, n)
        for _ in range(warmup):
            for f in forms.values():
                f()
        res = {k: [] for k in forms}
        for _ in range(runs):
            for k, f in forms.items():
                res[k].append(f())
    finally:
        for d in des:
            d.close()
    rec = {"block": "fgf batch", "unit": "device ms per pair", "config": name, "size": f"{W}x{H}x{D}", "fgf": s, "warmup": warmup, "runs": runs}
    for k, v in res.items():
        rec[k] = {"best": round(min(v), 4), "median": round(float(np.median(v)), 4)}
    return rec


# ---- --batch -------------------------------------------------------------------------------------------------------------
BATCH_SIZES = (1, 2, 4, 8)
LOOP = 8


def _bind(path):
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib = C.CDLL(path)
    for name, args in (("psm_create", [C.POINTER(vp), i, i, i, i, i]), ("psm_set_option", [vp, i, i]), ("psm_synchronize", [vp]),
                       ("psm_gray_compute", [vp, vp, vp, sz, i, vp, vp, sz]), ("psm_gray_time", [vp, C.POINTER(C.c_double)])):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, i
    lib.psm_destroy.argtypes, lib.psm_destroy.restype = [vp], None
    lib.psm_last_error.argtypes, lib.psm_last_error.restype = [vp], C.c_char_p
    if hasattr(lib, "psm_gray_compute_batch"):
        pp = C.POINTER(vp)
        lib.psm_gray_compute_batch.argtypes, lib.psm_gray_compute_batch.restype = [pp, i, pp, pp, sz, i, pp, pp, sz], i
    return lib


def worker(path, names, warmup, runs):
    """one build of the library in this process: {key: [ms per pair, one per repeat]}"""
    lib = _bind(path)
    out = {}

    def ck(rc, h=None):
        if rc:
            raise SystemExit("gray_bench worker: " + (lib.psm_last_error(h) or b"?").decode())

    def time_of(h):
        ms = C.c_double()
        ck(lib.psm_gray_time(h, C.byref(ms)), h)
        return ms.value

    for name in names:
        W, H, D = CONFIGS[name]
        gl, gr = the_planes(name)
        planes = [(np.ascontiguousarray(np.roll(gl, k, axis=0)), np.ascontiguousarray(np.roll(gr, k, axis=0))) for k in range(LOOP)]
        nctx = LOOP if name != "1080p" else 1
        hs = []
        for _ in range(nctx):
            h = C.c_void_p()
            ck(lib.psm_create(C.byref(h), W, H, D, 0, 0))
            ck(lib.psm_set_option(h, 2, 1), h)                                # PSM_OPT_PROFILE
            hs.append(h)

        def single(k):
            l, r = planes[k]
            ck(lib.psm_gray_compute(hs[k], l.ctypes.data, r.ctypes.data, 0, 0, None, None, 0), hs[k])
            return time_of(hs[k])

        def batch(n):
            arr = (C.c_void_p * n)(*[h.value for h in hs[:n]])
            ls = (C.c_void_p * n)(*[p[0].ctypes.data for p in planes[:n]])
            rs = (C.c_void_p * n)(*[p[1].ctypes.data for p in planes[:n]])
            ck(lib.psm_gray_compute_batch(arr, n, ls, rs, 0, 0, None, None, 0), hs[0])
            return time_of(hs[0]) / n

        sizes = [n for n in BATCH_SIZES if hasattr(lib, "psm_gray_compute_batch") and (name == "cones" or (name == "720p" and n == 4))]
        def loop():
            return sum(single(k) for k in range(LOOP)) / LOOP

        # two phases, each warmed up by itself, the forms of a phase alternating: the single calls, the same sequence in every
        # build (what follows a batch is not what follows a single call) - then, in a build that has it, the batches beside the loop
        phases = [{f"{name}.single": lambda: single(0)}]
        if nctx == LOOP:
            phases[0][f"{name}.loop{LOOP}"] = loop
        if sizes:
            phases.append({f"{name}.loop{LOOP}_beside_batches": loop})
            for n in sizes:
                phases[1][f"{name}.batch{n}"] = functools.partial(batch, n)
        for runs_of in phases:
            for _ in range(warmup):
                for f in runs_of.values():
                    f()
            res = {k: [] for k in runs_of}
            for _ in range(runs):
                for k, f in runs_of.items():
                    res[k].append(f())
            out.update(res)
        for h in hs:
            lib.psm_destroy(h)
    return out


def batch_bench(a):
    from primestereomatch_amd import capi
    builds = [("this", capi.LIB_PATH)] + ([("parent", os.path.abspath(a.parent_lib))] if a.parent_lib else [])
    names = a.config or ["cones", "720p", "1080p"]
    rounds = {tag: [] for tag, _ in builds}
    for _ in range(a.rounds):
        for tag, path in builds:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", path, "--warmup", str(a.warmup), "--runs", str(a.runs)]
            for n in names:
                cmd += ["--config", n]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"gray_bench: the child of build '{tag}' ended with {p.returncode}: {p.stderr[-2000:]}")
            rounds[tag].append(json.loads(p.stdout.strip().splitlines()[-1]))
    lines = [json.dumps({"block": "batch", "unit": "device ms per pair", "rounds": a.rounds, "warmup": a.warmup, "runs": a.runs,
                         "builds": [t for t, _ in builds], "loop": LOOP})]
    for tag, _ in builds:
        for key in rounds[tag][0]:
            per_round = [r[key] for r in rounds[tag]]
            allv = [v for r in per_round for v in r]
            bests = [min(r) for r in per_round]
            name, form = key.split(".")
            lines.append(json.dumps({"build": tag, "config": name, "size": "x".join(map(str, CONFIGS[name])), "form": form,
                                     "best": round(min(allv), 4), "median": round(float(np.median(allv)), 4),
                                     "spread_of_round_bests": round(max(bests) - min(bests), 4), "worst": round(max(allv), 4)}))
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", action="store_true", help="psm_gray_compute_batch beside a loop of single calls")
    ap.add_argument("--fgf", type=int, choices=(2, 4, 8), help="psm_gray_compute_fgf at this rate beside the colour FGF path and psm_gray_compute")
    ap.add_argument("--parent-lib", help="--batch: another build of libprimesm_hip.so to measure in alternation (single calls only)")
    ap.add_argument("--rounds", type=int, default=2, help="--batch: child processes per build")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS), help="default: all three")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.worker:
        print(json.dumps(worker(a.worker, a.config or ["cones"], a.warmup, a.runs)), flush=True)
        return
    if a.batch:
        return batch_bench(a)
    import torch
    from primestereomatch_amd import capi
    capi.load()
    if capi.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("gray_bench: no HIP device visible (there is no CPU path to time)")
    names = a.config or ["cones", "720p", "1080p"]
    if a.fgf:
        lines = (json.dumps(fgf_bench(torch, name, a.fgf, a.warmup, a.runs)) for name in names)
        if "cones" in names:
            lines = list(lines) + [json.dumps(fgf_batch_bench("cones", a.fgf, a.warmup, a.runs))]
    else:
        lines = (json.dumps(bench(torch, name, a.warmup, a.runs)) for name in names)
    for line in lines:
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
