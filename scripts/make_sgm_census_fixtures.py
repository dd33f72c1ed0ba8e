"""Generate the fixtures of the SGM stage's census cost from the numpy model (tests/sgm_census_model.py), CPU only:

  tests/golden/{cones,teddy}_sgm_census.npz   D = 64, census window 9 x 7, other parameters default: the final int16 map `disp`,
                                              `best` (uint8), the validity mask `valid` (uint8), the SHA-256 of the volumes C
                                              (uint16) and S (uint32), both [H][W][D], and of the code planes of both images
                                              (uint64 [H][W])

  python scripts/make_sgm_census_fixtures.py      (a few seconds per pair)
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sgm_census_model as Z  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    for name in ("cones", "teddy"):
        pair = np.load(os.path.join(GOLDEN, f"{name}_pair.npz"))
        o = Z.sgm(pair["l_bgr"], pair["r_bgr"], 0, 64, census=(9, 7))
        path = os.path.join(GOLDEN, f"{name}_sgm_census.npz")
        np.savez_compressed(path, disp=o["disp"], best=o["best"], valid=o["valid"].astype(np.uint8),
                            sha_C=np.array(sha(o["C"])), sha_S=np.array(sha(o["S"])),
                            sha_codes_l=np.array(sha(o["codes"][0])), sha_codes_r=np.array(sha(o["codes"][1])))
        print(name, os.path.getsize(path), "bytes; valid", int(o["valid"].sum()), "max C", int(o["C"].max()), "max S", int(o["S"].max()),
              "max L_r", o["max_l"], "sha C", sha(o["C"])[:16], "S", sha(o["S"])[:16], "map", sha(o["disp"])[:16], flush=True)


if __name__ == "__main__":
    main()
