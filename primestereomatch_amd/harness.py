"""Headless counterpart of StereoMatch::compute's accelerator branch (src/StereoMatch.cpp:193-311):
set the pair, run the four timed stages through the DispEst mirror, scale the maps for display and
score the left map against ground truth exactly as the reference does.  ("next" row 2 of SURVEY.md 8f.)
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import dispest
from .dispest import DispEst, reproject_batch, sgbm_batch, score_batch, sgbm_select_batch, wls_batch

MASK_NONE, MASK_NONOCC, MASK_DISC = 0, 1, 2   # include/StereoMatch.h


def error_vs_ground_truth(lDisMap, gt, mask, maxDis, scale_factor, error_threshold=4):
    """src/StereoMatch.cpp:248,275-309.  Returns (%BP, avg_err, num_bad_pixels, error map)."""
    # SMDE->lDisMap.convertTo(lDispMap, CV_8U, scale_factor)
    lDispMap = np.clip(lDisMap.astype(np.int32) * int(scale_factor), 0, 255).astype(np.uint8)
    e = np.abs(lDispMap.astype(np.int32) - np.asarray(gt, np.uint8).astype(np.int32))   # cv::absdiff
    e[:, :maxDis + 1] = 0                                    # eDispMap(Rect(0,0,maxDis+1,rows)) = 0
    unit = 127 // maxDis                                     # CHAR_MAX/maxDis, integer division
    e[e <= error_threshold * unit] = 0                       # THRESH_TOZERO
    if mask is not None:                                     # eDispMap.mul(errMask, 1/255.f)
        m = np.asarray(mask, np.uint8).astype(np.float64)
        e = np.rint(e * m * float(np.float32(1 / 255.0))).astype(np.int32)
    e = np.clip(e, 0, 255).astype(np.uint8)
    avg_err = float(e.mean()) / unit if unit else 0.0
    bad = int(np.count_nonzero(e))
    return 100.0 * bad / e.size, avg_err, bad, e


def compute(l_bgr, r_bgr, maxDis=64, gt=None, mask=None, scale_factor=4, error_threshold=4, threads=8,
            dtype="f32", post_process=True, verbose=False, subsample_rate=0, process_dm=False, joint_wmf=False, device_tail=False,
            depth=False):
    """One frame of STEREO_GIF on the accelerator path.  l_bgr/r_bgr: H x W x 3 uint8 (imread order).
    subsample_rate 0: full guided filter (CostFilter_GPU, the reference's 'm' branch); 2/4/8: the Fast Guided
    Filter variant (CostFilter_FGF, the snapshot's live branch, src/StereoMatch.cpp:213) on the device.
    process_dm: after the L-R check run the rest of PP::processDM's plain sequence on the device - fillInv, then wgtMedian
    on the pixels the check rejected (src/PP.cpp:405-410; lrCheck and fillInv are commented out in the snapshot's live
    processDM, wgtMedian is its dead-code predecessor of JointWMF) - the maps before it stay in lDisMap_raw / rDisMap_raw.
    joint_wmf: then run the snapshot's live processDM body, JointWMF::filter on both maps (src/PP.cpp:417-422), on the device
    (DispEst.JointWMF_GPU) and score the filtered left map, as StereoMatch::compute does after PostProcess
    (src/StereoMatch.cpp:225-311); the selected maps stay in lDisMap_raw / rDisMap_raw.
    device_tail: the display map and the error metric come from the device (DispEst.Score_GPU) instead of the numpy tail below -
    the same record, key for key.
    depth: False, the default: nothing is added.  Else the Q of cv::stereoRectify (4 x 4), or a dict {"Q", "crop": (x, y),
    "z_range": (z_min, z_max), "use_mask": bool}: the final left map is reprojected on the device (DispEst.Reproject_GPU) and the
    record gains xyz (H x W x 3 float32), z (H x W float32) and cloud (capi.point_dtype() records)."""
    out = {}
    lFrame = np.ascontiguousarray(l_bgr)
    rFrame = np.ascontiguousarray(r_bgr)
    if dtype == "f32":
        # lFrame.convertTo(lFrame, CV_32F, 1/255.0f) (src/StereoMatch.cpp:193-197)
        lFrame = lFrame.astype(np.float32) * np.float32(1 / 255.0)
        rFrame = rFrame.astype(np.float32) * np.float32(1 / 255.0)
    with DispEst(lFrame, rFrame, maxDis, threads, True, dtype=dtype) as SMDE:
        SMDE.setInputImages(lFrame, rFrame)
        _run_stages(SMDE, out, threads, subsample_rate, post_process, process_dm, joint_wmf)
        tail = _device_tail([SMDE], [gt], [mask], scale_factor, error_threshold, capi.PSM_SCORE_GIF)[0] if device_tail else None
        _reproject(SMDE, out, depth, capi.PSM_DEPTH_GIF)
    return _finish(out, maxDis, gt, mask, scale_factor, error_threshold, verbose, tail)


def compute_batch(pairs, maxDis=64, gts=None, masks=None, scale_factor=4, error_threshold=4, dtype="f32", post_process=True,
                  joint_wmf=False, verbose=False, device_tail=False, process_dm=False):
    """compute() for a list of (l_bgr, r_bgr) uint8 pairs of one size in shared launches: the reference's loop over pairs and
    datasets (src/main.cpp:64-73, src/StereoMatch.cpp:528-609) on the live STEREO_GIF branch.  dispest.compute_batch (CostConst +
    CostFilter + DispSelect of all pairs), then the L-R check of all pairs when post_process, then dispest.joint_wmf_batch when
    joint_wmf (the live processDM body on every pair's maps, the clustering chains of all images side by side).  gts / masks: one
    per pair (or None).  -> a list of compute's records; the stage times are each object's (a batch's wall time is charged to
    every member).  device_tail: display maps and metric of all pairs from the device in one set of launches (dispest.score_batch).
    process_dm: compute()'s - after the L-R check the rest of PP::processDM's plain sequence, fillInv and wgtMedian, of all pairs in
    shared launches (dispest.post_process_batch; the sweep chains of all maps side by side); the maps before it stay in
    lDisMap_raw / rDisMap_raw.  The L-R check of post_process goes through the same entry: the same bits."""
    if not pairs:
        return []
    frames = []
    for l, r in pairs:
        l, r = np.ascontiguousarray(l), np.ascontiguousarray(r)
        if dtype == "f32":
            l, r = l.astype(np.float32) * np.float32(1 / 255.0), r.astype(np.float32) * np.float32(1 / 255.0)
        frames.append((l, r))
    des = [DispEst(l, r, maxDis, 8, True, dtype=dtype) for l, r in frames]
    outs = [{} for _ in des]
    try:
        dispest.compute_batch(des)
        for d, out in zip(des, outs):
            d.download_maps()
            if joint_wmf or process_dm:
                out["lDisMap_raw"], out["rDisMap_raw"] = d.lDisMap.copy(), d.rDisMap.copy()
        if post_process or process_dm:
            # (one call: the fill and the median leave the masks as the L-R check wrote them)
            dispest.post_process_batch(des, lr_check=True, fill=process_dm, median=process_dm)
            for d, out in zip(des, outs):
                out["lValid"], out["rValid"] = d.lValid.copy(), d.rValid.copy()
        if joint_wmf:
            dispest.joint_wmf_batch(des)
        for d, out in zip(des, outs):
            out["cvc_ms"] = d.stage_time_us(capi.PSM_STAGE_CVC) / 1000
            out["cvf_ms"] = d.stage_time_us(capi.PSM_STAGE_CVF) / 1000
            out["dispsel_ms"] = d.stage_time_us(capi.PSM_STAGE_DISPSEL) / 1000
            out["pp_ms"] = d.stage_time_us(capi.PSM_STAGE_PP) / 1000
            out["lDisMap"], out["rDisMap"] = d.lDisMap.copy(), d.rDisMap.copy()
        tails = _device_tail(des, gts, masks, scale_factor, error_threshold, capi.PSM_SCORE_GIF) if device_tail else [None] * len(des)
    finally:
        for d in des:
            d.close()
    return [_finish(out, maxDis, gts[i] if gts else None, masks[i] if masks else None, scale_factor, error_threshold, verbose, tails[i])
            for i, out in enumerate(outs)]


def compute_video(vFrame, rectification, maxDis=64, gt=None, mask=None, scale_factor=4, error_threshold=4, threads=8,
                  dtype="f32", post_process=True, verbose=False, subsample_rate=0, process_dm=False, joint_wmf=False):
    """One frame of the DE_VIDEO branch of StereoMatch::compute (src/StereoMatch.cpp:138-153) followed by the stages of compute():
    vFrame is the camera's side-by-side frame (src_h x 2 src_w x 3 uint8), split into its eyes without a copy, rectified with
    `rectification` (rectify.Rectification) and cropped on the device.  The rectified pair comes back as lFrame / rFrame.
    The device keeps the pair 8-bit (float contexts scale it by 1/255 themselves), where the reference converts to float on
    the host (src/StereoMatch.cpp:193-198) - the same values."""
    out = {}
    w, h = rectification.crop[2], rectification.crop[3]
    blank = np.zeros((h, w, 3), np.uint8)
    with DispEst(blank, blank, maxDis, threads, True, dtype=dtype) as SMDE:
        SMDE.setRectification(rectification)
        SMDE.setInputFrame(vFrame)
        out["lFrame"], out["rFrame"] = SMDE.download_images()
        _run_stages(SMDE, out, threads, subsample_rate, post_process, process_dm, joint_wmf)
    return _finish(out, maxDis, gt, mask, scale_factor, error_threshold, verbose)


def compute_sgbm(l_bgr, r_bgr, maxDis=64, gt=None, mask=None, scale_factor=4, error_threshold=4, verbose=False, device_tail=False,
                 post_process=False, joint_wmf=False, depth=False, wls=None, **params):
    """One frame of STEREO_SGBM (src/StereoMatch.cpp:169-187, 275-309) on the device: l_bgr / r_bgr H x W x 3, uint8 or float32
    scaled by 1/255 (quantised on the device as lFrame.convertTo(lFrame, CV_8U, 255) does); params: DispEst.SGBM_GPU's, forwarded
    as they are - the reference's whole configuration is pre_filter_cap=63, speckle_window_size=100, speckle_range=32 (the
    defaults: SAD cost, no speckle filter), census=(win_w, win_h) selects the census cost; min_disparity / num_disparities choose another range than [0, maxDis), up to 1024
    disparities (the display conversion works from the map's own minimum and maximum).
    -> disp16 (imgDisparity16S), lDispMap (the display map), the reference's error metric on it, and bp_percent_int.
    device_tail: display map and both metrics from the device (DispEst.Score_GPU, PSM_SCORE_SGM and PSM_SCORE_SGM_INT).
    post_process: afterwards the stage's 8-bit maps of both views (DispEst.SGBMSelect_GPU) go through the post-processing chain of
    the GIF path on the device - LRCheck, FillInv, WgtMedian; joint_wmf: JointWMF in place of the latter two - and the record
    gains lDisMap_pp, the filtered left map, and (with gt) bp_percent_pp / avg_err_pp, the metric of compute() on it - from
    Score_GPU(PSM_SCORE_GIF) under device_tail.  The range must lie inside [0, maxDis).  Off, the default: no key is added.
    depth: compute()'s, on the int16 map (PSM_DEPTH_SGM: sixteenths of a disparity, the invalid pixels missing).
    wls: None, the default: nothing is added.  Else a dict of DispEst.setWLS's parameters ({}: lam 8000, sigma 1.5, iterations
    3): the int16 map goes through the WLS smoothing on the device (DispEst.WLS_GPU) and is published, so that depth= gives the
    cloud of the filtered map; the record gains wls16, the filtered map, and (with gt) bp_percent_wls - bp_percent_int's metric on
    its rounded reading min((max(v, 0) + 8) >> 4, 255).  The key "confidence" of the dict is not setWLS's: a dict of
    DispEst.setWLSConfidence's parameters ({}: both terms, 24, 2, 8) - the solve then starts with the graded confidence
    (PSM_WLS_CONFIDENCE: the L-R consistency of the stage's summed costs and the variance of the map around the pixel)."""
    out = {}
    lFrame, rFrame = np.ascontiguousarray(l_bgr), np.ascontiguousarray(r_bgr)
    with DispEst(lFrame, rFrame, maxDis, 8, True) as SMDE:
        SMDE.set_option(capi.PSM_OPT_PROFILE, 1)
        d16 = out["disp16"] = SMDE.SGBM_GPU(**params)
        out["cost_ms"], out["paths_ms"], out["select_ms"] = SMDE.sgm_times()
        if params.get("speckle_window_size", 0) > 0:
            out["speckle_ms"] = SMDE.sgm_speckle_time()
        tail = _device_tail_sgbm([SMDE], [gt], [mask], scale_factor, error_threshold)[0] if device_tail else None
        if wls is not None:
            _wls(SMDE, out, wls, maxDis, gt, mask, scale_factor, error_threshold)
        _reproject(SMDE, out, depth, capi.PSM_DEPTH_SGM)
        if post_process or joint_wmf:
            SMDE.SGBMSelect_GPU()
            _post_process_sgbm([SMDE], [out], [gt], [mask], scale_factor, error_threshold, joint_wmf, device_tail)
    return _finish_sgbm(out, maxDis, gt, mask, scale_factor, error_threshold, verbose, tail)


def compute_gray(gl, gr, maxDis=64, gt=None, mask=None, scale_factor=4, error_threshold=4, lr_check=True, fill=False,
                 device_tail=False, verbose=False, subsample_rate=0):
    """One frame of STEREO_GIF for a monochrome pair: gl / gr are H x W planes, uint8 or float32 scaled by 1/255, and go through
    the one-channel guided filter in one call (DispEst.Gray_GPU; no colour pair is staged).  lr_check: the L-R check behind it
    (lValid / rValid); fill: fillInv after it - the selected maps then stay in lDisMap_raw / rDisMap_raw.  The tail stages that
    read the image (wgtMedian, JointWMF) need a colour pair and are not offered.  device_tail: compute()'s.  subsample_rate 2, 4
    or 8: the Fast Guided Filter (FastGuidedFilterMono) in place of the full-resolution filter.
    -> compute()'s record with gray_ms, the device time of the call; of the stage times cvf_ms repeats it, the others are 0."""
    out = {}
    gl, gr = np.asarray(gl), np.asarray(gr)
    with DispEst.blank(gl.shape[0], gl.shape[1], maxDis) as SMDE:
        SMDE.set_option(capi.PSM_OPT_PROFILE, 1)
        SMDE.Gray_GPU(gl, gr, subsample_rate=subsample_rate)
        out["gray_ms"] = SMDE.gray_time()
        if lr_check or fill:
            SMDE.LRCheck_GPU()
            out["lValid"], out["rValid"] = SMDE.lValid.copy(), SMDE.rValid.copy()
        if fill:
            out["lDisMap_raw"], out["rDisMap_raw"] = SMDE.lDisMap.copy(), SMDE.rDisMap.copy()
            SMDE.FillInv_GPU()
        out["lDisMap"], out["rDisMap"] = SMDE.lDisMap.copy(), SMDE.rDisMap.copy()
        tail = _device_tail([SMDE], [gt], [mask], scale_factor, error_threshold, capi.PSM_SCORE_GIF)[0] if device_tail else None
    for k in ("cvc_ms", "cvf_ms", "dispsel_ms", "pp_ms"):
        out[k] = 0.0
    out["cvf_ms"] = out["gray_ms"]
    return _finish(out, maxDis, gt, mask, scale_factor, error_threshold, verbose, tail)


def compute_gray_batch(pairs, maxDis=64, gts=None, masks=None, scale_factor=4, error_threshold=4, lr_check=True, fill=False,
                       device_tail=False, verbose=False, subsample_rate=0):
    """compute_gray for a list of (gl, gr) monochrome pairs of one size and one depth (all uint8, or all float32) in shared
    launches (dispest.gray_batch): the reference's loop over pairs and datasets (src/main.cpp:64-73).  gts / masks: one per pair (or
    None).  lr_check / fill: compute_gray's, the stages of all pairs in shared launches (dispest.post_process_batch); device_tail:
    display maps and metrics of all pairs from the device (dispest.score_batch); subsample_rate: compute_gray's.
    -> a list of compute_gray's records; gray_ms is the batch's device time divided by the number of pairs."""
    pairs = [(np.asarray(gl), np.asarray(gr)) for gl, gr in pairs]
    if not pairs:
        return []
    hei, wid = pairs[0][0].shape
    des = [DispEst.blank(hei, wid, maxDis) for _ in pairs]
    outs = [{} for _ in pairs]
    try:
        des[0].set_option(capi.PSM_OPT_PROFILE, 1)
        dispest.gray_batch(des, [p[0] for p in pairs], [p[1] for p in pairs], subsample_rate=subsample_rate)
        ms = des[0].gray_time() / len(des)
        if lr_check or fill:
            dispest.post_process_batch(des, lr_check=True)
            for d, out in zip(des, outs):
                out["lValid"], out["rValid"] = d.lValid.copy(), d.rValid.copy()
        if fill:
            for d, out in zip(des, outs):
                out["lDisMap_raw"], out["rDisMap_raw"] = d.lDisMap.copy(), d.rDisMap.copy()
            dispest.post_process_batch(des, lr_check=False, fill=True)
        for d, out in zip(des, outs):
            out["lDisMap"], out["rDisMap"] = d.lDisMap.copy(), d.rDisMap.copy()
        tails = _device_tail(des, gts, masks, scale_factor, error_threshold, capi.PSM_SCORE_GIF) if device_tail else [None] * len(des)
    finally:
        for d in des:
            d.close()
    for i, out in enumerate(outs):
        out["gray_ms"] = ms
        for k in ("cvc_ms", "dispsel_ms", "pp_ms"):
            out[k] = 0.0
        out["cvf_ms"] = ms
        outs[i] = _finish(out, maxDis, gts[i] if gts else None, masks[i] if masks else None, scale_factor, error_threshold, verbose,
                          tails[i])
    return outs


def _wls_split(wls):
    """the wls= dict -> (setWLS's parameters, the "confidence" dict or None)"""
    params = {k: v for k, v in wls.items() if k != "confidence"}
    return params, wls.get("confidence")


def _wls(SMDE, out, wls, maxDis, gt, mask, scale_factor, error_threshold):
    """compute_sgbm's wls= option: the filtered map of the object's int16 map into the record, published to the SGM sources."""
    params, conf = _wls_split(wls)
    SMDE.setWLS(**params)
    if conf is None:
        SMDE.WLS_GPU(capi.PSM_WLS_SGM)
    else:
        SMDE.WLS_GPU(capi.PSM_WLS_SGM, confidence=conf)
    SMDE.wls_publish(True)
    w16 = out["wls16"] = SMDE.wls_map()
    if gt is not None:
        rounded = np.minimum((np.maximum(w16.astype(np.int32), 0) + 8) >> 4, 255)
        out["bp_percent_wls"] = error_vs_ground_truth(rounded, gt, mask, maxDis, scale_factor, error_threshold)[0]


def _reproject(SMDE, out, depth, source):
    """compute's depth= option: the planes and the cloud of the object's current result into the record."""
    if depth is False or depth is None:
        return
    opt = depth if isinstance(depth, dict) else {"Q": depth}
    SMDE.setReprojection(opt["Q"], opt.get("crop", (0, 0)), opt.get("z_range"))
    outputs = capi.PSM_DEPTH_XYZ | capi.PSM_DEPTH_Z | capi.PSM_DEPTH_CLOUD
    SMDE.Reproject_GPU(source, outputs, use_mask=bool(opt.get("use_mask", False)) and source == capi.PSM_DEPTH_GIF)
    out["xyz"], out["z"] = SMDE.reprojected()
    out["cloud"] = SMDE.cloud()


def _wls_batch(des, outs, wls, maxDis, gts, masks, scale_factor, error_threshold):
    """compute_sgbm_batch's wls= option: _wls for every object, the smoothing of all maps in shared launches."""
    params, conf = _wls_split(wls)
    for d in des:
        d.setWLS(**params)
    maps = wls_batch(des, capi.PSM_WLS_SGM) if conf is None else wls_batch(des, capi.PSM_WLS_SGM, confidence=conf)
    for i, (d, out, w16) in enumerate(zip(des, outs, maps)):
        d.wls_publish(True)
        out["wls16"] = w16
        gt, mask = (gts[i] if gts else None), (masks[i] if masks else None)
        if gt is not None:
            rounded = np.minimum((np.maximum(w16.astype(np.int32), 0) + 8) >> 4, 255)
            out["bp_percent_wls"] = error_vs_ground_truth(rounded, gt, mask, maxDis, scale_factor, error_threshold)[0]


def _reproject_batch(des, outs, depth, source):
    """compute_sgbm_batch's depth= option: _reproject for every object (depth: one setting for all, or a list with one per object),
    the planes and clouds of all of them from shared launches."""
    if depth is False or depth is None:
        return
    depths = list(depth) if isinstance(depth, (list, tuple)) else [depth] * len(des)
    opts = [dp if isinstance(dp, dict) else {"Q": dp} for dp in depths]
    for d, opt in zip(des, opts):
        d.setReprojection(opt["Q"], opt.get("crop", (0, 0)), opt.get("z_range"))
    use_mask = bool(opts[0].get("use_mask", False)) and source == capi.PSM_DEPTH_GIF
    reproject_batch(des, source, capi.PSM_DEPTH_XYZ | capi.PSM_DEPTH_Z | capi.PSM_DEPTH_CLOUD, use_mask=use_mask)
    for d, out in zip(des, outs):
        out["xyz"], out["z"] = d.reprojected()
        out["cloud"] = d.cloud()


def write_ply(path, cloud):
    """A point cloud (capi.point_dtype() records: DispEst.cloud()) as a binary little-endian PLY file, vertices only: x, y, z as
    float, red, green, blue as uchar."""
    cloud = np.asarray(cloud)
    rec = np.empty(cloud.shape[0], np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    for k in ("x", "y", "z"):
        rec[k] = cloud[k]
    rec["red"], rec["green"], rec["blue"] = cloud["r"], cloud["g"], cloud["b"]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % rec.shape[0])
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def _post_process_sgbm(des, outs, gts, masks, scale_factor, error_threshold, joint_wmf, device_tail):
    """The chain behind SGBMSelect_GPU on every object's device maps, and its keys of the record: lDisMap_pp and the metric on it."""
    if len(des) > 1:      # (several objects: the chain of all pairs in shared launches - the same bits)
        dispest.post_process_batch(des, lr_check=True, fill=not joint_wmf, median=not joint_wmf)
    else:
        for d in des:
            d.LRCheck_GPU()
            if not joint_wmf:
                d.FillInv_GPU()
                d.WgtMedian_GPU()
    if joint_wmf and len(des) == 1:
        des[0].JointWMF_GPU()
    elif joint_wmf:
        dispest.joint_wmf_batch(des)
    tails = _device_tail(des, gts, masks, scale_factor, error_threshold, capi.PSM_SCORE_GIF) if device_tail else [None] * len(des)
    for i, (d, out) in enumerate(zip(des, outs)):
        out["lDisMap_pp"] = d.lDisMap.copy()
        gt, mask = (gts[i] if gts else None), (masks[i] if masks else None)
        if gt is None:
            continue
        if tails[i] is not None:
            out["bp_percent_pp"], out["avg_err_pp"] = tails[i][1]["bp_percent"], tails[i][1]["avg_err"]
        else:
            out["bp_percent_pp"], out["avg_err_pp"] = error_vs_ground_truth(out["lDisMap_pp"], gt, mask, d.maxDis, scale_factor,
                                                                             error_threshold)[:2]


def compute_sgbm_batch(pairs, maxDis=64, gts=None, masks=None, scale_factor=4, error_threshold=4, verbose=False, device_tail=False,
                       post_process=False, joint_wmf=False, depth=False, wls=None, **params):
    """compute_sgbm for a list of (l_bgr, r_bgr) pairs of one size and depth in shared launches (dispest.sgbm_batch): the
    reference's loop over pairs and datasets (src/main.cpp:64-73, src/StereoMatch.cpp:528-609).  gts / masks: one per pair (or
    None).  -> a list of compute_sgbm's records; the times are the batch's divided by the number of pairs.  device_tail: display
    maps and both metrics of all pairs from the device (dispest.score_batch).  post_process / joint_wmf: compute_sgbm's, the maps of
    all pairs from one launch (dispest.sgbm_select_batch).  wls / depth: compute_sgbm's, for every pair - the smoothing of all int16
    maps in one set of launches (dispest.wls_batch), published, then with depth the planes and clouds of all pairs in one more
    (dispest.reproject_batch, PSM_DEPTH_SGM); depth may be a list with one entry per pair.  The defaults add nothing."""
    pairs = [(np.ascontiguousarray(l), np.ascontiguousarray(r)) for l, r in pairs]
    if not pairs:
        return []
    des = [DispEst(l, r, maxDis, 8, True) for l, r in pairs]
    try:
        des[0].set_option(capi.PSM_OPT_PROFILE, 1)
        maps = sgbm_batch(des, **params)
        times = [t / len(des) for t in des[0].sgm_times()]
        spk = des[0].sgm_speckle_time() / len(des) if params.get("speckle_window_size", 0) > 0 else None
        tails = _device_tail_sgbm(des, gts, masks, scale_factor, error_threshold) if device_tail else [None] * len(des)
        pps = [{} for _ in des]
        if wls is not None:
            _wls_batch(des, pps, wls, maxDis, gts, masks, scale_factor, error_threshold)
        _reproject_batch(des, pps, depth, capi.PSM_DEPTH_SGM)
        if post_process or joint_wmf:
            sgbm_select_batch(des)
            _post_process_sgbm(des, pps, gts, masks, scale_factor, error_threshold, joint_wmf, device_tail)
    finally:
        for d in des:
            d.close()
    outs = []
    for i, d16 in enumerate(maps):
        out = {"disp16": d16, "cost_ms": times[0], "paths_ms": times[1], "select_ms": times[2]}
        out.update(pps[i])
        if spk is not None:
            out["speckle_ms"] = spk
        outs.append(_finish_sgbm(out, maxDis, gts[i] if gts else None, masks[i] if masks else None, scale_factor, error_threshold,
                                 verbose, tails[i]))
    return outs


def _device_tail(des, gts, masks, scale_factor, error_threshold, source):
    """The display map and the error record of every object's current result from the device: truth and parameters to each
    object, one score_batch -> [(display map, record)]."""
    for i, d in enumerate(des):
        gt, mask = (gts[i] if gts else None), (masks[i] if masks else None)
        d.set_score_params(scale_factor, error_threshold, MASK_NONOCC if mask is not None else MASK_NONE)
        if gt is not None:
            d.set_truth(np.asarray(gt, np.uint8), None if mask is None else np.asarray(mask, np.uint8))
        else:
            d.clear_truth()
    recs = score_batch(des, source)
    return [(d.score_maps()[0], rec) for d, rec in zip(des, recs)]


def _device_tail_sgbm(des, gts, masks, scale_factor, error_threshold):
    """... of STEREO_SGBM: the reference's min-max display conversion and its metric, then the integer-disparity figure."""
    tails = _device_tail(des, gts, masks, scale_factor, error_threshold, capi.PSM_SCORE_SGM)
    ints = score_batch(des, capi.PSM_SCORE_SGM_INT)
    return [(disp, rec, rint) for (disp, rec), rint in zip(tails, ints)]


def _from_record(out, rec):
    out.update({"bp_percent": rec["bp_percent"], "avg_err": rec["avg_err"], "bad_pixels": rec["bad"]})


def _finish_sgbm(out, maxDis, gt, mask, scale_factor, error_threshold, verbose, tail=None):
    if tail is not None:
        out["lDispMap"] = tail[0]
        if gt is not None:
            _from_record(out, tail[1])
            out["bp_percent_int"] = tail[2]["bp_percent"]
        return _report_sgbm(out, gt, verbose)
    d16 = out["disp16"]
    # minMaxLoc(imgDisparity16S, &minVal, &maxVal); imgDisparity16S.convertTo(lDispMap, CV_8U, 255/(maxVal - minVal));
    # lDispMap = (lDispMap/4) * scale_factor.  OpenCV's rounding of both steps: the factor is formed in double, but convertTo of a
    # 16-bit source multiplies in fp32 - saturate_cast<uchar>(cvRound((float)v * (float)alpha)), cvRound = ties to even, negative
    # products (the invalid -16) saturate to 0; Mat / 4 on CV_8U is convertTo(CV_8U, 0.25): cvRound(v * 0.25f), ties to even
    # again (10 / 4 -> 2, 14 / 4 -> 4); * scale_factor saturates at 255.  There is no offset: minVal is not subtracted.
    v = d16.astype(np.float32)
    alpha = np.float32(255.0 / (float(d16.max()) - float(d16.min())))
    m8 = np.clip(np.rint(v * alpha), 0, 255).astype(np.float32)
    m8 = np.clip(np.rint(m8 * np.float32(0.25)), 0, 255)
    out["lDispMap"] = np.clip(m8 * scale_factor, 0, 255).astype(np.uint8)
    if gt is not None:
        # the metric of :275-309 on the display map as it is (it already carries scale_factor)
        bp, avg, bad, _ = error_vs_ground_truth(out["lDispMap"], gt, mask, maxDis, 1, error_threshold)
        out.update({"bp_percent": bp, "avg_err": avg, "bad_pixels": bad})
        # The figure to compare with the GIF path: the same metric on the integer disparity max(d16, 0) >> 4 scaled like the GIF
        # maps.  bp_percent above is NOT comparable - the reference stretches the SGBM map by 255 / (maxVal - minVal) of the
        # frame at hand (min-max scaling, then / 4), so its grey levels are not disparity * scale_factor.
        out["bp_percent_int"] = error_vs_ground_truth(np.maximum(d16, 0) >> 4, gt, mask, maxDis, scale_factor, error_threshold)[0]
    return _report_sgbm(out, gt, verbose)


def _report_sgbm(out, gt, verbose):
    if verbose:
        print("STEREO SGBM Times:")
        print("Cost Time:\t %4.3f ms\nPaths Time:\t %4.3f ms\nSelect Time:\t %4.3f ms" % (out["cost_ms"], out["paths_ms"], out["select_ms"]))
        if "speckle_ms" in out:
            print("Speckle Time:\t %4.3f ms" % out["speckle_ms"])
        if gt is not None:
            print("%%BP = %.2f%% \t Avg Err = %.2f" % (out["bp_percent"], out["avg_err"]))
    return out


def _run_stages(SMDE, out, threads, subsample_rate, post_process, process_dm, joint_wmf):
    SMDE.setThreads(threads)
    SMDE.setSubsampleRate(subsample_rate or 4)
    SMDE.CostConst_GPU()
    if subsample_rate:
        SMDE.CostFilter_FGF_GPU()
    else:
        SMDE.CostFilter_GPU()
    SMDE.DispSelect_GPU()
    if post_process or process_dm:
        SMDE.LRCheck_GPU()
        out["lValid"], out["rValid"] = SMDE.lValid.copy(), SMDE.rValid.copy()
    if process_dm:
        out["lDisMap_raw"], out["rDisMap_raw"] = SMDE.lDisMap.copy(), SMDE.rDisMap.copy()
        SMDE.FillInv_GPU()
        SMDE.WgtMedian_GPU()
    if joint_wmf:
        out.setdefault("lDisMap_raw", SMDE.lDisMap.copy())
        out.setdefault("rDisMap_raw", SMDE.rDisMap.copy())
        SMDE.JointWMF_GPU()
    out["cvc_ms"] = SMDE.stage_time_us(capi.PSM_STAGE_CVC) / 1000
    out["cvf_ms"] = SMDE.stage_time_us(capi.PSM_STAGE_CVF) / 1000
    out["dispsel_ms"] = SMDE.stage_time_us(capi.PSM_STAGE_DISPSEL) / 1000
    out["pp_ms"] = SMDE.stage_time_us(capi.PSM_STAGE_PP) / 1000
    out["lDisMap"], out["rDisMap"] = SMDE.lDisMap.copy(), SMDE.rDisMap.copy()


def _finish(out, maxDis, gt, mask, scale_factor, error_threshold, verbose, tail=None):
    if tail is not None:
        out["lDispMap"] = tail[0]
        if gt is not None:
            _from_record(out, tail[1])
    else:
        out["lDispMap"] = np.clip(out["lDisMap"].astype(np.int32) * scale_factor, 0, 255).astype(np.uint8)
        if gt is not None:
            bp, avg, bad, emap = error_vs_ground_truth(out["lDisMap"], gt, mask, maxDis, scale_factor, error_threshold)
            out.update({"bp_percent": bp, "avg_err": avg, "bad_pixels": bad})
    if verbose:
        print("STEREO GIF Module Times:")
        print("CVC Time:\t %4.2f ms" % out["cvc_ms"])
        print("CVF Time:\t %4.2f ms" % out["cvf_ms"])
        print("DispSel Time:\t %4.2f ms" % out["dispsel_ms"])
        print("PP Time:\t %4.2f ms" % out["pp_ms"])
        if gt is not None:
            print("%%BP = %.2f%% \t Avg Err = %.2f" % (out["bp_percent"], out["avg_err"]))
    return out
