"""One process of the parent / tree comparison for score, reproject and SGM map select: python scripts/tail_run_speed.py ROOT LABEL OUT
ROOT: the checkout whose package (and built library) is measured.  One JSON line to OUT and stdout.
Per size: device ms of the launches (the stage's _time getter, best of REPS) and the synchronous call on the host clock (best of
REPS), as scripts/score_bench.py, depth_bench.py and sgm_bench.py --maps take them; the host time per call of 200 back-to-back
calls under PSM_OPT_ASYNC (us, RUNS repetitions); at 450x375 the batch entries at n = 8."""
import json
import os
import sys
import time

import numpy as np

ROOT, LABEL, OUT = os.path.abspath(sys.argv[1]), sys.argv[2], sys.argv[3]
sys.path.insert(0, ROOT)
import primestereomatch_amd as P                                   # noqa: E402
from primestereomatch_amd import capi, dispest, rectify            # noqa: E402

assert os.path.abspath(P.__file__).startswith(ROOT + os.sep), P.__file__
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = rectify.read_opencv_yaml(os.path.join(HERE, "tests", "golden", "zed_extrinsics.yml"))["Q"]
SIZES = ((450, 375, 64), (1920, 1080, 256))
REPS, RUNS, CALLS, NB = 20, 6, 200, 8


def best(call, dev):
    call()
    k, c = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        c.append((time.perf_counter() - t0) * 1e3)
        k.append(dev())
    return round(min(k), 4), round(min(c), 4)


def async_us(de, call):
    de.set_option(capi.PSM_OPT_ASYNC, 1)
    out = []
    for _ in range(RUNS):
        de.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            rc = call()
        t = time.perf_counter() - t0
        assert rc == 0, capi.last_error(de._h)
        de.synchronize()
        out.append(round(t * 1e6 / CALLS, 3))
    de.set_option(capi.PSM_OPT_ASYNC, 0)
    return out


def inputs(W, H, D, seed):
    g = np.random.default_rng(seed)
    maps = g.integers(1, D, (2, H, W), dtype=np.uint8)
    d16 = g.integers(-16, 16 * D, (H, W)).astype(np.int16)
    gt = g.integers(0, 256, (H, W), dtype=np.uint8)
    mask = g.choice(np.array([0, 255], np.uint8), (H, W))
    l, r = g.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    return maps, d16, gt, mask, l, r


def prepare(de, maps, d16, gt, mask):
    de.set_option(capi.PSM_OPT_PROFILE, 1)
    de.set_truth(gt, mask)
    de.setReprojection(Q)
    de.upload_sgm_map(d16)
    de.upload_maps(maps[0], maps[1])


def single(W, H, D):
    maps, d16, gt, mask, l, r = inputs(W, H, D, 1)
    rec = {}
    with P.DispEst(l, r, D) as de:
        lib, h = de._lib, de._h
        prepare(de, maps, d16, gt, mask)
        for name, src in (("gif", capi.PSM_SCORE_GIF), ("sgm", capi.PSM_SCORE_SGM)):
            rec[f"score_{name}_kernels_ms"], rec[f"score_{name}_call_ms"] = best(lambda: de.Score_GPU(src), de.score_time)
        rec["score_async_us"] = async_us(de, lambda: lib.psm_score(h, capi.PSM_SCORE_GIF, None))
        every = capi.PSM_DEPTH_XYZ | capi.PSM_DEPTH_Z | capi.PSM_DEPTH_CLOUD
        for name, outs in (("all", every), ("cloud", capi.PSM_DEPTH_CLOUD)):
            rec[f"depth_{name}_kernels_ms"], rec[f"depth_{name}_call_ms"] = best(lambda: de.Reproject_GPU(capi.PSM_DEPTH_SGM, outs), de.reproject_time)
        rec["depth_async_us"] = async_us(de, lambda: lib.psm_reproject(h, capi.PSM_DEPTH_SGM, capi.PSM_DEPTH_CLOUD, 0, None))
        de.upload_sgm_map(None)
        de.SGBM_GPU()
        rec["maps_kernels_ms"], rec["maps_call_ms"] = best(lambda: de.SGBMSelect_GPU(download=False), de.sgm_maps_time)
        rec["maps_async_us"] = async_us(de, lambda: lib.psm_sgm_select_maps(h, None, None, 0))
    return rec


def batch(W, H, D):
    des, rec = [], {}
    try:
        for i in range(NB):
            maps, d16, gt, mask, l, r = inputs(W, H, D, 10 + i)
            de = P.DispEst(l, r, D)
            des.append(de)
            prepare(de, maps, d16, gt, mask)
        rec["score_batch_kernels_ms"], rec["score_batch_call_ms"] = best(lambda: dispest.score_batch(des, capi.PSM_SCORE_GIF), des[0].score_time)
        rec["depth_batch_kernels_ms"], rec["depth_batch_call_ms"] = best(
            lambda: dispest.reproject_batch(des, capi.PSM_DEPTH_SGM, capi.PSM_DEPTH_CLOUD), des[0].reproject_time)
        for de in des:
            de.upload_sgm_map(None)
        dispest.sgbm_batch(des)
        rec["maps_batch_kernels_ms"], rec["maps_batch_call_ms"] = best(lambda: dispest.sgbm_select_batch(des), des[0].sgm_maps_time)
    finally:
        for de in des:
            de.close()
    return rec


def main():
    res = {"label": LABEL, "lib": os.path.relpath(capi.LIB_PATH, HERE)}
    for W, H, D in SIZES:
        res[f"{W}x{H}x{D}"] = single(W, H, D)
    W, H, D = SIZES[0]
    res[f"{W}x{H}x{D} n={NB}"] = batch(W, H, D)
    line = json.dumps(res)
    print(line, flush=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
