"""Times PP::processDM's own sequence - lrCheck, fillInv, wgtMedian - per image pair, as n single-call sequences one after the
other (psm_lr_check, psm_fill_invalid, psm_wgt_median per context) and as one psm_post_process_batch of the same n contexts: one
JSON line per size and n.

Inputs: the maps of Cones, Teddy and their mirrored / upside-down variants after psm_compute_batch at 450 x 375 x 64 (n = 2, 4, 8),
and synthetic pairs at 1280 x 720 x 128 (n = 4).  Every timed sequence starts from freshly uploaded maps; the maps stay on the
device in both forms.  All contexts run on one stream; *_ms is the time between two events on it around the calls (the median
synchronises with the host, so the host's looks at the counters are inside), *_wall_ms the host clock behind a synchronise; best of
--reps, *_spread_ms: max - min of the repetitions.  sweeps: per pair [left, right] of the last repetition (-1: the dataflow form).

--singles-only: the singles leg alone; it uses no entry point newer than psm_wgt_median, so with --tree it runs against the package
of another checkout (a build of the parent commit) in the same session - the reference point of the comparison.

Usage: python scripts/pp_bench.py [--reps N] [--batch N[,N...]] [--batch-720p N] [--singles-only] [--tree PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(golden, W, H, D, n):
    """n different pairs of one size: at 450 x 375 Cones and Teddy, mirrored (the views swap) and upside down; else synthetic seeds."""
    out = []
    if (W, H) == (450, 375):
        base = []
        for name in ("cones", "teddy"):
            z = np.load(os.path.join(golden, f"{name}_pair.npz"))
            base.append((z["l_bgr"], z["r_bgr"]))
        for flip_v in (False, True):
            for mirror in (False, True):
                for l, r in base:
                    if mirror:
                        l, r = r[:, ::-1], l[:, ::-1]
                    if flip_v:
                        l, r = l[::-1], r[::-1]
                    out.append((np.ascontiguousarray(l), np.ascontiguousarray(r)))
    else:
        from primestereomatch_amd import synth
        for seed in range(3, 3 + n):
            l, r, _ = synth.make_pair(W, H, D, seed=seed)
            out.append((l, r))
    return out[:n]


def _bench(torch, golden, W, H, D, N, reps, singles_only):
    import primestereomatch_amd as P
    from primestereomatch_amd import dispest
    pairs = _pairs(golden, W, H, D, N)
    stream = torch.cuda.Stream()
    des = [P.DispEst(l, r, D) for l, r in pairs]
    try:
        for d in des:
            d.set_stream(stream.cuda_stream)
        dispest.compute_batch(des)
        raw = [tuple(m.copy() for m in d.download_maps()) for d in des]
        invalid = [[int((v == 0).sum()) for v in d.download_valid()] for d in des]      # (the L-R check of the raw maps)

        def timed(run):
            for d, (lm, rm) in zip(des, raw):
                d.upload_maps(lm, rm)
            for d in des:
                d.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            a.record(stream)
            run()
            b.record(stream)
            b.synchronize()
            wall = (time.perf_counter() - t) * 1e3
            return a.elapsed_time(b) / N, wall / N

        def singles():
            for d in des:
                d._ck(d._lib.psm_lr_check(d._h, None, None, 0), "lr_check")
                d._ck(d._lib.psm_fill_invalid(d._h, None, None, 0), "fill_invalid")
                d._ck(d._lib.psm_wgt_median(d._h, None, None, 0), "wgt_median")

        def batch():
            dispest.post_process_batch(des, lr_check=True, fill=True, median=True, download=False)

        timed(singles)                                           # warm-up (allocations)
        ref = [tuple(m.copy() for m in d.download_maps()) for d in des]
        ts = [timed(singles) for _ in range(reps)]
        line = {"size": f"{W}x{H}x{D}", "N": N, "reps": reps,
                "invalid_per_map": invalid,
                "single_ms": round(min(t[0] for t in ts), 3), "single_spread_ms": round(max(t[0] for t in ts) - min(t[0] for t in ts), 3),
                "single_wall_ms": round(min(t[1] for t in ts), 3),
                "single_sweeps": [d.wgt_median_stats()[0] for d in des]}
        if not singles_only:
            timed(batch)
            same = all(np.array_equal(a, b) for d, r in zip(des, ref) for a, b in zip(d.download_maps(), r))
            tb = [timed(batch) for _ in range(reps)]
            line.update({"same_maps": bool(same),
                         "batch_ms": round(min(t[0] for t in tb), 3), "batch_spread_ms": round(max(t[0] for t in tb) - min(t[0] for t in tb), 3),
                         "batch_wall_ms": round(min(t[1] for t in tb), 3),
                         "batch_sweeps": [d.wgt_median_stats()[0] for d in des],
                         "ratio": round(min(t[0] for t in tb) / min(t[0] for t in ts), 3)})
            ts2 = [timed(singles) for _ in range(reps)]          # the singles again, behind the batches: the session's drift
            line["single_again_ms"] = round(min(t[0] for t in ts2), 3)
    finally:
        for d in des:
            d.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", default="2,4,8", help="N[,N...]: the batch sizes at 450 x 375")
    ap.add_argument("--batch-720p", type=int, default=4, help="the batch size at 1280 x 720 (0: skip)")
    ap.add_argument("--singles-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package (and built library) is timed")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch                                                 # (first: the library then binds to the HIP runtime torch loaded)
    torch.cuda.init()
    golden = os.path.join(ROOT, "tests", "golden")
    print(json.dumps({"tree": os.path.relpath(tree, ROOT), "singles_only": a.singles_only}), flush=True)
    for N in [int(v) for v in a.batch.split(",") if v]:
        _bench(torch, golden, 450, 375, 64, N, a.reps, a.singles_only)
    if a.batch_720p > 0:
        _bench(torch, golden, 1280, 720, 128, a.batch_720p, a.reps, a.singles_only)


if __name__ == "__main__":
    main()
