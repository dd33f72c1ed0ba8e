"""Writes tests/golden/{cones,teddy}_wls_conf.npz and manifest_wls_conf.json: what the confidence-weighted WLS smoothing
(tests/wls_conf_model.py, the defaults) makes of the committed Cones / Teddy pairs - S recomputed by tests/sgm_model.sgm at D = 64.
The npz hold three planes only - disp int16, conf uint8, right16 int16 - compressed; the manifest their SHA-256, the bad-pixel
figure of the rounded reading and the void count.  tests/test_wls_conf_model.py pins the model to them.

    python scripts/make_wls_conf_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden")


def record(name):
    import sgm_model
    import wls_conf_model as CM
    import wls_model
    from primestereomatch_amd import harness

    p = np.load(os.path.join(GOLDEN, f"{name}_pair.npz"))
    o = sgm_model.sgm(p["l_bgr"], p["r_bgr"], 64)
    out = CM.wls(o["disp"], -16, p["l_bgr"], S=o["S"], dmin=0)
    planes = {k: out[k] for k in ("disp", "conf", "right16")}
    bp = harness.error_vs_ground_truth(wls_model.rounded_u8(out["disp"]), p["gt_l"], p["occl"], 64, 4, 4)[0]
    np.savez_compressed(os.path.join(GOLDEN, f"{name}_wls_conf.npz"), **planes)
    return {"bp_percent_wls_conf": float(bp), "void": int((out["disp"] == -16).sum()), **CM.DEFAULTS, **wls_model.DEFAULTS,
            "sha256": {k: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for k, a in planes.items()}}


def main():
    man = {name.capitalize(): {"wls_conf": record(name)} for name in ("cones", "teddy")}
    with open(os.path.join(GOLDEN, "manifest_wls_conf.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(man, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
