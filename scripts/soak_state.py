"""Randomised soak of the CONTEXT STATE MACHINE (not part of the test suite): one context lives through a random sequence of
new image pairs, row stripes, tuning flags and readers of intermediate results; after every filter + select the maps of the
current stripe must equal the oracle's for the current pair.  The suite's version is tests/test_gpu_sequences.py with the shadow
of tests/seq_model.py: every stage, three contexts, every reader against the models; this script stays as the open-ended soak of
the guided-filter path at random geometries.
    python scripts/soak_state.py [seconds] [seed]
    python scripts/soak_state.py --episodes N [seed]     (the same N episodes for a seed on every build: for comparing two)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import primestereomatch_amd as P          # noqa: E402
from primestereomatch_amd import capi, synth   # noqa: E402
import psm_oracle_py as O                 # noqa: E402

SAFE_FLAGS = [0, 0, 0, 1048576, 2097152]     # compatible with row stripes
ANY_FLAGS = SAFE_FLAGS + [128, 8192, 8192 | 128]


def episode(rng, idx):
    W = int(rng.integers(8, 260)); H = int(rng.integers(8, 80))
    D = int(rng.integers(2, min(W, 140) + 1)) if rng.random() < 0.3 else int(rng.integers(2, min(W, 24) + 1))
    dtype = "u8" if rng.random() < 0.25 else "f32"
    pairs = [synth.make_pair(W, H, D, seed=int(rng.integers(0, 1 << 16)))[:2] for _ in range(3)]
    pipe = O.pipeline_u8 if dtype == "u8" else O.pipeline_f32
    small = D <= 16                              # volumes are held (and compared) for few slices only
    refs = [pipe(l, r, D, threads=8, want_volumes=(dtype == "f32" and small), want_raw=small) for l, r in pairs]
    fgf_rates = [s for s in (2, 4, 8) if W // s > 8 // s and H // s > 8 // s] if dtype == "f32" else []
    fgf_refs = {}
    log = [f"episode {idx}: {W}x{H} D={D} {dtype}"]
    cur, pend = 0, None
    y0, y1 = 0, H
    with P.DispEst(pairs[0][0], pairs[0][1], D, dtype=dtype) as de:
        for step in range(int(rng.integers(4, 12))):
            op = rng.choice(["frame", "frame", "frame", "images", "images_async", "rows", "flags", "volume", "pp", "frame_async",
                             "fgf", "upvol", "sides"])
            if op == "images":
                cur = int(rng.integers(0, 3))
                pend = None                     # a blocking upload supersedes a staged pair
                de.setInputImages(*pairs[cur]); log.append(f"images {cur}")
                continue
            if op == "images_async":            # staged for the NEXT CostConst (psm_upload_pair_async)
                pend = int(rng.integers(0, 3))
                de.setInputImages_async(*pairs[pend]); log.append(f"images_async {pend}")
                continue
            if op == "rows":
                if rng.random() < 0.4:
                    y0, y1 = 0, H
                else:
                    y0 = int(rng.integers(0, H)); y1 = int(rng.integers(y0 + 1, H + 1))
                de.set_rows(y0, y1); log.append(f"rows {y0},{y1}")
                if (y0, y1) != (0, H):          # stripes need the default select form: back to a compatible flag set
                    de.set_option(capi.PSM_OPT_FLAGS, int(rng.choice(SAFE_FLAGS)))
                continue
            if op == "flags":
                fl = int(rng.choice(SAFE_FLAGS if (y0, y1) != (0, H) else ANY_FLAGS))
                if dtype == "u8" and fl == 8192:
                    fl = 0
                de.set_option(capi.PSM_OPT_FLAGS, fl); log.append(f"flags {fl}")
                continue
            if pend is not None:                # CostConst adopts the staged pair
                cur, pend = pend, None
            ref = refs[cur]
            if op == "fgf" and fgf_rates and (y0, y1) == (0, H):      # Fast Guided Filter (+ select, + a slice of its volume)
                s = int(rng.choice(fgf_rates))
                if (cur, s) not in fgf_refs:
                    fgf_refs[cur, s] = O.pipeline_fgf(*pairs[cur], D, s=s, threads=8, want_volumes=small)
                fref = fgf_refs[cur, s]
                de.setSubsampleRate(s)
                de.CostConst_GPU(); de.CostFilter_FGF_GPU(); de.DispSelect_GPU()
                log.append(f"fgf s={s} pair {cur}")
                if not (np.array_equal(de.lDisMap, fref["ldisp"]) and np.array_equal(de.rDisMap, fref["rdisp"])):
                    return False, " | ".join(log)
                if small:
                    d, side = int(rng.integers(0, D)), int(rng.integers(0, 2))
                    log.append(f"fgf volume side {side} slice {d}")
                    if not np.array_equal(de.download_volume(side, d, d + 1)[0], fref["rvol" if side else "lvol"][d]):
                        return False, " | ".join(log)
                continue
            if op == "upvol" and small:         # some slices uploaded over fresh costs: the others must be the real costs
                side, d0 = int(rng.integers(0, 2)), int(rng.integers(0, D))
                n = int(rng.integers(1, D - d0 + 1))
                patch = np.full((n, H, W), 64, np.uint8) if dtype == "u8" else np.full((n, H, W), 0.25, np.float32)
                de.CostConst_GPU()
                de.upload_volume(side, patch, d0=d0)
                log.append(f"upvol pair {cur} side {side} slices {d0}..{d0 + n}")
                exp = ref["raw_r" if side else "raw_l"].copy()
                exp[d0:d0 + n] = patch
                if not (np.array_equal(de.download_volume(side), exp) and
                        np.array_equal(de.download_volume(1 - side), ref["raw_l" if side else "raw_r"])):
                    return False, " | ".join(log)
                continue
            if op == "frame_async":             # maps through psm_download_maps_async / _wait
                de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_device()
                de.download_maps_async(); de.download_maps_wait()
            elif op == "sides" and (y0, y1) == (0, H):      # one side at a time in place of CostFilter_GPU
                de.CostConst_GPU(); de.CostFilter_side(0); de.CostFilter_side(1); de.DispSelect_GPU()
                log.append("sides")
            else:
                de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
            log.append(f"frame pair {cur} rows {y0},{y1}")
            if not (np.array_equal(de.lDisMap[y0:y1], ref["ldisp"][y0:y1]) and np.array_equal(de.rDisMap[y0:y1], ref["rdisp"][y0:y1])):
                return False, " | ".join(log)
            if op == "volume" and "lvol" in ref:
                d = int(rng.integers(0, D))
                log.append(f"volume slice {d}")
                if not np.array_equal(de.download_volume(int(rng.integers(0, 2)) * 0, d, d + 1)[0], ref["lvol"][d]):
                    return False, " | ".join(log)
            if op == "pp" and (y0, y1) == (0, H):
                de.LRCheck_GPU()
                lv, rv = O.lr_check(ref["ldisp"], ref["rdisp"])
                de.FillInv_GPU()
                log.append("pp")
                if not (np.array_equal(de.lValid, lv) and np.array_equal(de.lDisMap, O.fill_inv(ref["ldisp"], lv))):
                    return False, " | ".join(log)
    return True, log[0]


def main():
    args = sys.argv[1:]
    episodes = None
    if args and args[0] == "--episodes":
        episodes, args = int(args[1]), [0] + args[2:]
    secs = float(args[0]) if args else 60.0
    seed = int(args[1]) if len(args) > 1 else 1
    O.build()
    rng = np.random.default_rng(seed)
    t0 = time.time(); n = bad = 0
    while (n < episodes) if episodes is not None else (time.time() - t0 < secs):
        try:
            ok, desc = episode(rng, n)
        except Exception as e:
            ok, desc = False, f"episode {n}: EXCEPTION {type(e).__name__}: {str(e)[:300]}"
        n += 1
        if not ok:
            bad += 1
            print("FAIL", desc, flush=True)
    print(f"soak_state: {n} episodes in {time.time() - t0:.0f} s, {bad} failures (seed {seed})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
