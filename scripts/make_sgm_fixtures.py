"""Generate the semi-global matching fixtures from the numpy model (tests/sgm_model.py), CPU only:

  tests/golden/{cones,teddy}_sgm.npz   D = 64, default parameters: the final int16 map `disp`, `best` (uint8), the validity mask
                                       `valid` (uint8) and the SHA-256 of the volumes C (uint16) and S (uint32), both [H][W][D]

  python scripts/make_sgm_fixtures.py      (a few seconds per pair)
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sgm_model as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    for name in ("cones", "teddy"):
        pair = np.load(os.path.join(GOLDEN, f"{name}_pair.npz"))
        o = M.sgm(pair["l_bgr"], pair["r_bgr"], 64)
        path = os.path.join(GOLDEN, f"{name}_sgm.npz")
        np.savez_compressed(path, disp=o["disp"], best=o["best"], valid=o["valid"].astype(np.uint8),
                            sha_C=np.array(sha(o["C"])), sha_S=np.array(sha(o["S"])))
        print(name, os.path.getsize(path), "bytes; valid", float(o["valid"].mean()), flush=True)


if __name__ == "__main__":
    main()
