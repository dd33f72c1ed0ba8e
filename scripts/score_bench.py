"""Times the score stage (psm_score: display maps and the error metric on the device) beside the numpy tail it stands for: one
JSON line per size, and the same lines into profiles/score_bench.txt.

  gif_kernels_ms / sgm_kernels_ms   device time of the launches of one psm_score (PSM_OPT_PROFILE): k_sc_score, and for the SGM
                                    source k_sc_minmax + k_sc_score; best of --reps
  gif_call_ms / sgm_call_ms         the synchronous call on the host clock (launches, the 24-byte record's copy, the wait)
  gif_host_ms / sgm_host_ms         the numpy tail on this machine's host, one thread: harness.error_vs_ground_truth and
                                    harness._finish_sgbm on maps that are already on the host; mean of --host-reps
  ring_plain_ms / ring_scored_ms    FrameRing (2 frames in flight) per frame without and with a truth, three runs each of
                                    --frames frames: the list of the three means; the plain runs are what the parent commit runs
  ring_plain_spread_ms              max - min of the three plain runs: with gif_kernels_ms the margin inside which the frame loop
                                    counts as having absorbed the stage

The maps scored are random (the stage's cost does not depend on their values); the SGM map is placed with the test hook.
Usage: python scripts/score_bench.py [--reps N] [--host-reps N] [--frames N] [--only WxH] [--no-ring]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((450, 375, 64), (1280, 720, 128), (1920, 1080, 256))


def _stage(W, H, D, reps, host_reps):
    import primestereomatch_amd as P
    from primestereomatch_amd import capi, harness
    rng = np.random.default_rng(1)
    maps = rng.integers(0, D, (2, H, W), dtype=np.uint8)
    d16 = rng.integers(-16, 16 * D, (H, W)).astype(np.int16)
    gt = rng.integers(0, 256, (H, W), dtype=np.uint8)
    mask = rng.choice(np.array([0, 255], np.uint8), (H, W))
    z = np.zeros((H, W, 3), np.uint8)
    out = {}
    with P.DispEst(z, z, D) as de:
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        de.set_truth(gt, mask)
        de.upload_maps(maps[0], maps[1])
        de.upload_sgm_map(d16)
        for name, source in (("gif", capi.PSM_SCORE_GIF), ("sgm", capi.PSM_SCORE_SGM)):
            de.Score_GPU(source)                             # (first use: the stage's scratch)
            kern, call = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                rec = de.Score_GPU(source)
                call.append((time.perf_counter() - t0) * 1e3)
                kern.append(de.score_time())
            out[f"{name}_kernels_ms"], out[f"{name}_call_ms"] = round(min(kern), 4), round(min(call), 4)
            out[f"{name}_bad"] = rec["bad"]
    t = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        harness._finish({"lDisMap": maps[0]}, D, gt, mask, 4, 4, False)
        t.append((time.perf_counter() - t0) * 1e3)
    out["gif_host_ms"] = round(float(np.mean(t)), 3)
    t = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        harness._finish_sgbm({"disp16": d16}, D, gt, mask, 4, 4, False)
        t.append((time.perf_counter() - t0) * 1e3)
    out["sgm_host_ms"] = round(float(np.mean(t)), 3)
    return out


def _ring(W, H, D, frames):
    import primestereomatch_amd as P
    from primestereomatch_amd import synth
    l, r, _ = synth.make_pair(W, H, D, seed=3)
    rng = np.random.default_rng(2)
    truth = (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.choice(np.array([0, 255], np.uint8), (H, W)))

    def run(**kw):
        with P.FrameRing(l, r, D, frames=2, **kw) as ring:
            for _ in range(4):                               # warm: buffers, code objects
                ring.push(l, r)
            ring.flush()
            t0 = time.perf_counter()
            for _ in range(frames):
                ring.push(l, r)
            ring.flush()
            return (time.perf_counter() - t0) * 1e3 / frames

    plain, scored = [], []
    for _ in range(3):                                       # alternately, so drift hits both alike
        plain.append(round(run(), 4))
        scored.append(round(run(truth=truth), 4))
    return {"ring_plain_ms": plain, "ring_scored_ms": scored, "ring_plain_spread_ms": round(max(plain) - min(plain), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-ring", action="store_true")
    a = ap.parse_args()
    lines = []
    for W, H, D in SIZES:
        if a.only and a.only != f"{W}x{H}":
            continue
        rec = {"size": f"{W}x{H}x{D}"}
        rec.update(_stage(W, H, D, a.reps, a.host_reps))
        if not a.no_ring:
            rec.update(_ring(W, H, D, a.frames))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "score_bench.txt"), "w") as f:
        f.write("# scripts/score_bench.py: the score stage beside the numpy tail; ms\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
