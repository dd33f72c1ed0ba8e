"""Generate the JointWMF fixtures of tests/test_gpu_jwmf.py from the numpy model (tests/jwmf_model.py), CPU only:

  tests/golden/{cones,teddy}_jwmf.npz      the model's default clustering of both images (label_of_key, centres, Lloyd
                                           iterations) and its filtered maps of the committed *_oracle_d64 maps (r = 9)
  tests/golden/synthetic_jwmf_clusters.npz the model's default clustering of both images of synth.make_pair(W, H, D, seed=3)
                                           at 1280x720x128 and 1920x1080x256

  python scripts/make_jwmf_fixtures.py      (several minutes: the model's k-means is plain numpy)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jwmf_model as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _clusters(prefix, img):
    m = M.clustering_of(img)
    return m, {f"{prefix}_lok": m["lok"], f"{prefix}_centres": m["centres"], f"{prefix}_iterations": np.int64(m["iterations"])}


def main():
    for name in ("cones", "teddy"):
        pair = np.load(os.path.join(GOLDEN, f"{name}_pair.npz"))
        gold = np.load(os.path.join(GOLDEN, f"{name}_oracle_d64.1.npz"))
        out = {}
        for side, img, dmap in (("l", pair["l_bgr"], gold["ldisp"]), ("r", pair["r_bgr"], gold["rdisp"])):
            m, d = _clusters(side, img)
            out.update(d)
            out[f"{side}map"] = M.median(dmap, m["F"], M.quantise(M.weight_table(m["centres"])), 9)
        np.savez_compressed(os.path.join(GOLDEN, f"{name}_jwmf.npz"), **out)
        print(name, out["l_iterations"], out["r_iterations"], flush=True)
    from primestereomatch_amd import synth
    out = {}
    for W, H, D in ((1280, 720, 128), (1920, 1080, 256)):
        l, r, _ = synth.make_pair(W, H, D, seed=3)
        for side, img in (("l", l), ("r", r)):
            out.update(_clusters(f"s{W}x{H}_{side}", img)[1])
        print(W, H, out[f"s{W}x{H}_l_iterations"], out[f"s{W}x{H}_r_iterations"], flush=True)
    np.savez_compressed(os.path.join(GOLDEN, "synthetic_jwmf_clusters.npz"), **out)


if __name__ == "__main__":
    main()
