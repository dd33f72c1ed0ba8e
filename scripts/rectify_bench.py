#!/usr/bin/env python3
"""Timing of the device rectification (psm_upload_pair_rectified[_async], k_rectify).  One JSON line on stdout.

For each configuration (the reference's ZED calibration, tests/golden/zed_*.yml, at 1280 x 720 per eye and scaled by 1.5 to
1920 x 1080 per eye; the centred crop 960 x 512 resp. 1440 x 768):
  kernel   device time of k_rectify from the hipEvents of PSM_OPT_PROFILE 1 around every launch (warmed, --launches of them),
           its byte count (maps 6 B + output 3 B per output pixel + every source pixel a tap touches, 3 B, once) and that
           count over the part's measured copy rate (k_box8: 4.9 TB/s) as a fraction of the kernel time
  loop     step time of the overlapped frame loop - construct(i); upload(i + 1); filter(i); select(i); maps downloaded
           asynchronously - over --frames frames, fed (a) the raw side-by-side frame through psm_upload_pair_rectified_async and
           (b) the pair rectified beforehand through psm_upload_pair_async (what a host had to do before), alternating in one
           process, --repeats times each: median and spread (max - min), and the host time spent inside the upload call
Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 4.9e12      # B/s, k_box8


def footprint_bytes(rect):
    n = 0
    x, y, w, h = rect.crop
    for s in range(2):
        m = rect.map_xy[s][y:y + h, x:x + w].astype(np.int64)
        hit = np.zeros((rect.src_h + 3, rect.src_w + 3), bool)          # (a margin of one takes the taps outside)
        for dy in (0, 1):
            for dx in (0, 1):
                yy = np.clip(m[..., 1] + dy, -1, rect.src_h) + 1
                xx = np.clip(m[..., 0] + dx, -1, rect.src_w) + 1
                hit[yy, xx] = True
        n += int(np.count_nonzero(hit[1:rect.src_h + 1, 1:rect.src_w + 1])) * 3
    return n


def run_loop(de, frames, upload, n):
    """-> (ms per step, host ms per upload call)"""
    upload(de, frames[0])
    de.synchronize()
    host = 0.0
    have_prev = False
    t0 = time.perf_counter()
    for i in range(n):
        de.CostConst_GPU()
        if i + 1 < n:
            h0 = time.perf_counter()
            upload(de, frames[(i + 1) % len(frames)])
            host += time.perf_counter() - h0
        de.CostFilter_GPU()
        de.DispSelect_device()
        if have_prev:
            de.download_maps_wait()
        de.download_maps_async()
        have_prev = True
    de.download_maps_wait()
    de.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, host * 1e3 / max(1, n - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-disp", type=int, default=64)
    ap.add_argument("--dtype", default="f32")
    a = ap.parse_args()

    import primestereomatch_amd as P
    from primestereomatch_amd import capi, rectify, synth
    if capi.device_count() < 1:
        raise SystemExit("rectify_bench: no HIP device visible")
    cal = rectify.load_calibration(os.path.join(ROOT, "tests", "golden", "zed_intrinsics.yml"), os.path.join(ROOT, "tests", "golden", "zed_extrinsics.yml"))
    out = {"bench": "rectify", "max_disp": a.max_disp, "dtype": a.dtype, "launches": a.launches, "frames": a.frames, "repeats": a.repeats,
           "copy_rate_TBps": COPY_RATE / 1e12, "configs": []}
    for scale, (w, h), crop in ((1.0, (1280, 720), (160, 104, 960, 512)), (1.5, (1920, 1080), (240, 156, 1440, 768))):
        rect = rectify.Rectification.from_calibration(rectify.scale_calibration(cal, scale), w, h, crop)
        vframes = [np.ascontiguousarray(np.concatenate(synth.make_pair(w, h, a.max_disp, seed=s)[:2], axis=1)) for s in (0, 1)]
        blank = np.zeros((crop[3], crop[2], 3), np.uint8)
        npix = crop[2] * crop[3]
        nbytes = 2 * npix * (6 + 3) + footprint_bytes(rect)
        cfg = {"frame": [2 * w, h], "crop": list(crop), "bytes": nbytes}
        with P.DispEst(blank, blank, a.max_disp, dtype=a.dtype) as de:
            de.setRectification(rect)
            # ---- kernel ----
            for _ in range(10):
                de.setInputFrame(vframes[0])
            de.set_option(capi.PSM_OPT_PROFILE, 1)
            de.reset_kernel_times()
            for i in range(a.launches):
                de.setInputFrame(vframes[i & 1])
            ms, n = de.kernel_time_ms(capi.PSM_K_PREP)
            assert n == a.launches, (n, a.launches)
            de.set_option(capi.PSM_OPT_PROFILE, 0)
            k_us = ms * 1e3 / n
            cfg["kernel_us"] = round(k_us, 3)
            cfg["bytes_over_copy_rate_us"] = round(nbytes / COPY_RATE * 1e6, 3)
            cfg["fraction_of_copy_rate"] = round(nbytes / COPY_RATE * 1e6 / k_us, 4)
            # the pairs a host without this feature would upload: rectified beforehand
            pairs = []
            for f in vframes:
                de.setInputFrame(f)
                pairs.append(tuple(x.copy() for x in de.download_images()))
            # ---- loop ----
            de.set_option(capi.PSM_OPT_ASYNC, 1)
            forms = {"rectified_async": (vframes, lambda d, f: d.setInputFrame_async(f)),
                     "prerectified_async": (pairs, lambda d, p: d.setInputImages_async(p[0], p[1]))}
            for name, (src, up) in forms.items():       # warm both
                run_loop(de, src, up, 4)
            res = {k: [] for k in forms}
            for _ in range(a.repeats):
                for name, (src, up) in forms.items():   # alternating
                    res[name].append(run_loop(de, src, up, a.frames))
            for name, v in res.items():
                steps = sorted(x[0] for x in v)
                cfg[name] = {"step_ms_median": round(steps[len(steps) // 2], 4), "step_ms_spread": round(steps[-1] - steps[0], 4),
                             "step_ms_all": [round(x[0], 4) for x in v], "host_upload_call_ms": round(float(np.median([x[1] for x in v])), 4)}
            cfg["step_growth_ms"] = round(cfg["rectified_async"]["step_ms_median"] - cfg["prerectified_async"]["step_ms_median"], 4)
        out["configs"].append(cfg)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
