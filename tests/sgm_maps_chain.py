"""What the tests of psm_sgm_select_maps share: the post-processing chain of the oracle (oracle/psm_oracle_py.py) on a pair of 8-bit
maps, and the reference's bad-pixel count of each step - the CPU prototype the feature was measured with."""
from __future__ import annotations

import numpy as np

# Cones / Teddy, SAD cost, D = 64, non-occluded mask, scale 4, threshold 4, out of 168 750 pixels: bad pixels of the left map
# after WTA, + lrCheck + fillInv, + wgtMedian (measured on the models: tests/sgm_model.py -> tests/sgm_maps_model.py -> the oracle)
SAD_COUNTS = {"cones": (8380, 7460, 6759), "teddy": (17659, 16196, 15662)}
PIXELS = 168750


def chain(O, l_bgr, lmap, rmap, max_disp):
    """lrCheck -> fillInv -> wgtMedian of the oracle on (lmap, rmap).  -> dict of the intermediate maps and masks."""
    lv, rv = O.lr_check(lmap, rmap)
    lf, rf = O.fill_inv(lmap, lv), O.fill_inv(rmap, rv)
    img = O.u8_to_f32(np.ascontiguousarray(l_bgr))
    return {"lvalid": lv, "rvalid": rv, "lfill": lf, "rfill": rf, "lmed": O.wgt_median(img, lf, lv, max_disp), "img_l": img}


def bad_pixels(O, disp, gt, mask, max_disp, scale=4, thr=4):
    return O.eval_bad_pixels(disp, gt, mask, max_disp, scale, thr)[0]
