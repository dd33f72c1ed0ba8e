"""-m gpu: whose _time getter answers after a batch - the profile bracket (psm::Bracket, csrc/psm_ctx.h) of psm_score,
psm_reproject and psm_sgm_select_maps, as tests/test_gpu_wls_batch.py::test_profile_time_is_context_0s has it for psm_wls_filter.
A batch records the events of its first context alone, so that context's getter answers and every other member's refuses; a
context that gave its scratch back (psm_release_scratch: the events go with it) refuses, and so does one whose last call ran with
PSM_OPT_PROFILE off.  8 x 8 contexts, the smallest a context takes; the results themselves are other files' subject."""
import ctypes as C
import math

import numpy as np
import pytest

import depth_model as DM

pytestmark = pytest.mark.gpu

W, H, D = 8, 8, 4
Q = DM.q_from_projections([[700.0, 0, 30.0, 0], [0, 700.0, 20.0, 0], [0, 0, 1, 0]], [[700.0, 0, 30.0, -84000.0], [0, 700.0, 20.0, 0], [0, 0, 1, 0]])


@pytest.fixture(scope="module")
def psm():
    from primestereomatch_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no HIP device visible"
    import primestereomatch_amd as P
    return P


def score_stage(psm):
    from primestereomatch_amd import dispest
    maps = np.random.default_rng(1).integers(0, D, (2, H, W), dtype=np.uint8)
    return dict(prepare=lambda de: de.upload_maps(*maps),
                batch=lambda des: dispest.score_batch(des, psm.capi.PSM_SCORE_GIF),
                single=lambda de: de.Score_GPU(psm.capi.PSM_SCORE_GIF),
                time=lambda de: de.score_time(), getter="psm_score_time",
                refusal="psm_score_time: the last psm_score was not timed (PSM_OPT_PROFILE)")


def reproject_stage(psm):
    from primestereomatch_amd import dispest
    lmap = np.random.default_rng(2).integers(0, D, (H, W), dtype=np.uint8)

    def prepare(de):
        de.setReprojection(Q)
        de.upload_maps(lmap, lmap)
    return dict(prepare=prepare,
                batch=lambda des: dispest.reproject_batch(des, psm.capi.PSM_DEPTH_GIF, psm.capi.PSM_DEPTH_Z),
                single=lambda de: de.Reproject_GPU(psm.capi.PSM_DEPTH_GIF, psm.capi.PSM_DEPTH_Z),
                time=lambda de: de.reproject_time(), getter="psm_reproject_time",
                refusal="psm_reproject_time: the last psm_reproject was not timed (PSM_OPT_PROFILE)")


def maps_stage(psm):
    from primestereomatch_amd import dispest
    return dict(prepare=lambda de: de.SGBM_GPU(),                                 # (psm_release_scratch gives the SGM result back)
                batch=dispest.sgbm_select_batch,
                single=lambda de: de.SGBMSelect_GPU(download=False),
                time=lambda de: de.sgm_maps_time(), getter="psm_sgm_maps_time",
                refusal="psm_sgm_maps_time: the last psm_sgm_select_maps was not timed (PSM_OPT_PROFILE), or there is none")


def refused(psm, de, stage):
    rc = getattr(de._lib, stage["getter"])(de._h, C.byref(C.c_double()))
    assert rc != 0 and psm.capi.last_error(de._h) == stage["refusal"], (rc, psm.capi.last_error(de._h))


@pytest.mark.parametrize("make", (score_stage, reproject_stage, maps_stage))
def test_only_context_0_of_a_batch_is_timed(psm, make):
    stage = make(psm)
    profile = psm.capi.PSM_OPT_PROFILE
    l, r = np.random.default_rng(3).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    des = [psm.DispEst(l, r, D) for _ in range(2)]
    try:
        for de in des:
            de.set_option(profile, 1)
            stage["prepare"](de)
        stage["batch"](des)
        ms = stage["time"](des[0])
        assert math.isfinite(ms) and ms >= 0.0
        refused(psm, des[1], stage)                                               # a member's own bracket recorded nothing
        des[0].release_scratch()                                                  # the events went with the scratch
        refused(psm, des[0], stage)
        stage["prepare"](des[0])
        stage["single"](des[0])                                                   # a single call under the option is timed again ...
        ms = stage["time"](des[0])
        assert math.isfinite(ms) and ms >= 0.0
        des[0].set_option(profile, 0)
        stage["single"](des[0])                                                   # ... and one without it is not
        refused(psm, des[0], stage)
    finally:
        for de in des:
            de.close()
