"""Python mirror of the reference's `DispEst` accelerator interface (include/DispEst.h:21-51,
src/DispEst.cpp:272-328) on top of the C ABI.  Method names, argument meaning and return
conventions follow the reference so that tests read like calls into the reference:

    de = DispEst(l, r, maxDis, threads, useHIP=True)
    de.setInputImages(l, r); de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_GPU()
    de.lDisMap, de.rDisMap            # H x W uint8

The C++ twin (primestereomatch_amd/host/DispEst.h) is what a C++ host links; this class exists
for the Python tests and bench.  No CPU path lives here: without the HIP library and a GPU the
constructor raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

MAX_CPU_THREADS = 8  # include/ComFunc.h:52


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class DispEst:
    _sgm_d = 0                               # the disparities of the last SGBM_GPU (0: none yet - maxDis)
    _gray_rate = 0                               # the subsample rate of the last Gray_GPU / gray_batch (0: the full-resolution filter)
    _sgm_ch = 3                                  # the channels of the pair the last SGBM_GPU ran on (1: its gray= pair)

    def __init__(self, l, r, d: int, t: int = 8, ocl: bool = True, *, dtype: str = "f32",
                 device: int = 0, d_range=None, d_stride=None):
        """l, r: H x W x 3 images (uint8 as loaded by imread, or float32 scaled by 1/255 as
        StereoMatch::compute hands them over, src/StereoMatch.cpp:193-198); d: maxDis;
        t: host threads (kept for interface parity; unused by the GPU path); ocl: must be true
        (the accelerator path is the only one this package implements).
        dtype: "f32" | "u8" (8-bit char mode).  d_range=(d_begin,d_end): disparity shard."""
        if not ocl:
            raise capi.PsmError("DispEst: only the accelerator ('m' / OCL_DE) path exists in this package")
        l = np.asarray(l)
        r = np.asarray(r)
        if l.shape != r.shape or l.dtype != r.dtype:
            # src/DispEst.cpp:21-29: exits on mismatching types
            raise ValueError("DE: Error - Left & Right images are of different types.")
        if l.ndim != 3 or l.shape[2] != 3:
            raise ValueError("DispEst: images must be H x W x 3")
        self._create(int(l.shape[0]), int(l.shape[1]), d, t, dtype, device, d_range, d_stride)
        self.setInputImages(l, r)

    @classmethod
    def blank(cls, hei: int, wid: int, d: int, t: int = 8, *, dtype: str = "f32", device: int = 0, d_range=None, d_stride=None):
        """A DispEst of the given size without an image pair: what Gray_GPU and SGBM_GPU(gray=...) need, which bring their own
        one-channel planes.  Every method that reads the staged colour pair is refused until setInputImages has run."""
        self = cls.__new__(cls)
        self._create(int(hei), int(wid), d, t, dtype, device, d_range, d_stride)
        return self

    def _create(self, hei, wid, d, t, dtype, device, d_range, d_stride):
        self.hei, self.wid = hei, wid
        self.maxDis = int(d)
        self.threads = int(t)
        self.useOCL = True
        self.subsample_rate = 4
        self._lib = capi.load()
        self._dtype = capi.PSM_U8 if dtype == "u8" else capi.PSM_F32
        self._h = C.c_void_p()
        self.options = {}
        d0, d1 = (0, self.maxDis) if d_range is None else (int(d_range[0]), int(d_range[1]))
        self.d_begin, self.d_end = d0, d1
        if d_stride is not None:
            # strided ownership (psm_create_shard_strided): this object holds the slices d_stride[0], + d_stride[1], ... < maxDis
            self.d_begin, self.d_end = int(d_stride[0]), self.maxDis
            rc = self._lib.psm_create_shard_strided(C.byref(self._h), self.wid, self.hei, self.maxDis, int(d_stride[0]), int(d_stride[1]),
                                                    self._dtype, int(device))
        else:
            rc = self._lib.psm_create_shard(C.byref(self._h), self.wid, self.hei, self.maxDis, d0, d1,
                                            self._dtype, int(device))
        if rc != 0:
            self._h = C.c_void_p()
            raise capi.PsmError("DispEst: " + capi.last_error(None))
        self.lDisMap = np.zeros((self.hei, self.wid), np.uint8)
        self.rDisMap = np.zeros((self.hei, self.wid), np.uint8)
        self.lValid = np.zeros((self.hei, self.wid), np.uint8)
        self.rValid = np.zeros((self.hei, self.wid), np.uint8)

    # ---- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.psm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc, what):
        capi.check(rc, self._h, what)

    # ---- reference interface ---------------------------------------------------------------
    def setInputImages(self, l, r) -> int:
        l = np.ascontiguousarray(l)
        r = np.ascontiguousarray(r)
        assert l.dtype == r.dtype  # src/DispEst.cpp:166
        if l.shape != (self.hei, self.wid, 3) or r.shape != l.shape:
            raise ValueError("setInputImages: image size differs from the one DispEst was built for")
        if l.dtype == np.uint8:
            depth = capi.PSM_IMG_U8
        elif l.dtype == np.float32:
            depth = capi.PSM_IMG_F32
        else:
            raise ValueError("setInputImages: images must be uint8 or float32")
        self._ck(self._lib.psm_upload_pair(self._h, _ptr(l), _ptr(r), 3, l.strides[0], depth),
                 "setInputImages")
        return 0

    def setThreads(self, newThreads: int) -> int:
        if newThreads > MAX_CPU_THREADS:  # src/DispEst.cpp:172-179
            return -1
        self.threads = int(newThreads)
        return 0

    def setSubsampleRate(self, newRate: int) -> None:
        self.subsample_rate = int(newRate)

    def CostConst_GPU(self) -> int:
        self._ck(self._lib.psm_cost_construct(self._h), "CostConst_GPU")
        return 0

    def CostFilter_GPU(self) -> int:
        self._ck(self._lib.psm_cost_filter(self._h), "CostFilter_GPU")
        return 0

    def CostFilter_FGF_GPU(self) -> int:
        """DispEst::CostFilter_FGF (src/DispEst.cpp:281-296) on the device: FastGuidedFilterColor with
        r = GIF_R_WIN, eps = GIF_EPS and s = subsample_rate (setSubsampleRate; default 4)."""
        self._ck(self._lib.psm_cost_filter_fgf(self._h, int(self.subsample_rate)), "CostFilter_FGF_GPU")
        return 0

    def DispSelect_GPU(self) -> int:
        self._ck(self._lib.psm_disp_select(self._h, _ptr(self.lDisMap), _ptr(self.rDisMap), self.wid),
                 "DispSelect_GPU")
        return 0

    # ---- the second algorithm: STEREO_SGBM (src/StereoMatch.cpp:169-187) ----------------------
    def SGBM_GPU(self, block_size: int = 0, P1: int = 0, P2: int = 0, uniqueness_ratio: int = 10, disp12_max_diff: int = 1,
                 gray=None, speckle_window_size: int = 0, speckle_range: int = 0, pre_filter_cap: int = 0, mode="hh",
                 min_disparity: int = 0, num_disparities: int = 0, census=None):
        """ssgbm->compute(lFrame, rFrame, imgDisparity16S) on the device over the pair setInputImages staged, with the
        parameters of setupOpenCVSGBM (src/StereoMatch.cpp:639-660) as defaults (0: blockSize 5, P1 = 8 ch bs^2, P2 = 32 ch bs^2).
        -> H x W int16: disparity * 16, -16 where invalid.  An independent stage (psm_sgm_compute): the maps, masks and volumes
        of the other methods are untouched.  gray = (l, r): run on that H x W uint8 pair instead (CV_8UC1 frames).
        speckle_window_size > 0: the map goes through StereoSGBM's last step, filterSpeckles(map, -16, speckle_window_size,
        16 * speckle_range) (the reference: 100, 32); 0, the default: off - the setting is this call's, not the object's.
        pre_filter_cap in 1 .. 63: StereoSGBM's pixel cost, Birchfield-Tomasi over Sobel-prefiltered images (psm_sgm_set_prefilter;
        the reference: 63); 0, the default: SAD - this call's setting too.
        mode: ssgbm->setMode, "sgbm", "hh" (the default: all eight directions), "3way", "hh4" or OpenCV's integer
        (psm_sgm_set_mode) - this call's setting as well.
        min_disparity, num_disparities: StereoSGBM::create's first two arguments (psm_sgm_set_range) - the disparities
        min_disparity .. min_disparity + num_disparities - 1, num_disparities in 2 .. 1024 whatever maxDis is, or 0, the default:
        maxDis; invalid pixels are then (min_disparity - 1) * 16.  This call's setting as well.
        census = (win_w, win_h), both odd, 3 .. 9 by 3 .. 7: the pixel cost is the Hamming distance of census codes
        (psm_sgm_set_census), which does not change when the two cameras differ in gain or exposure; None or (0, 0), the default:
        off - this call's setting too.  Refused together with pre_filter_cap > 0."""
        self._ck(self._lib.psm_sgm_set_census(self._h, *census_window(census)), "SGBM_GPU")
        self._ck(self._lib.psm_sgm_set_mode(self._h, sgm_mode(mode)), "SGBM_GPU")
        self._ck(self._lib.psm_sgm_set_range(self._h, int(min_disparity), int(num_disparities)), "SGBM_GPU")
        self._sgm_d = int(num_disparities) or self.maxDis
        self._ck(self._lib.psm_sgm_set_prefilter(self._h, int(pre_filter_cap)), "SGBM_GPU")
        self._ck(self._lib.psm_sgm_set_speckle(self._h, int(speckle_window_size), int(speckle_range)), "SGBM_GPU")
        self._ck(self._lib.psm_sgm_set_params(self._h, int(block_size), int(P1), int(P2), int(uniqueness_ratio),
                                              int(disp12_max_diff)), "SGBM_GPU")
        self._sgm_ch = 3 if gray is None else 1
        if gray is None:
            self._ck(self._lib.psm_sgm_compute(self._h), "SGBM_GPU")
        else:
            l, r = (np.ascontiguousarray(a) for a in gray)
            if l.shape != (self.hei, self.wid) or r.shape != l.shape or l.dtype != np.uint8 or r.dtype != np.uint8:
                raise ValueError("SGBM_GPU: gray must be two H x W uint8 images of the size DispEst was built for")
            self._ck(self._lib.psm_sgm_compute_gray(self._h, _ptr(l), _ptr(r), l.strides[0]), "SGBM_GPU")
        return self.sgm_disparity()

    def sgm_disparity(self):
        """The int16 map of the last SGBM_GPU (synchronises)."""
        disp = np.empty((self.hei, self.wid), np.int16)
        self._ck(self._lib.psm_sgm_download_disparity(self._h, _ptr(disp), disp.strides[0]), "sgm_disparity")
        return disp

    def sgm_costs(self):
        """Test hook: (C uint16, S uint32), both [H][W][D], of the last SGBM_GPU - D its num_disparities, or maxDis."""
        D = self._sgm_d or self.maxDis
        Cv = np.empty((self.hei, self.wid, D), np.uint16)
        Sv = np.empty((self.hei, self.wid, D), np.uint32)
        self._ck(self._lib.psm_sgm_download_costs(self._h, 0, _ptr(Cv)), "sgm_costs")
        self._ck(self._lib.psm_sgm_download_costs(self._h, 1, _ptr(Sv)), "sgm_costs")
        return Cv, Sv

    def sgm_prefiltered(self, side: int):
        """Test hook: the prefiltered planes [H][W][2 ch] uint8 (P_0 .. P_{ch-1}, Q_0 .. Q_{ch-1}) of the left (side 0) or right
        (1) image in the last SGBM_GPU, which must have run with pre_filter_cap > 0; ch: 3, or 1 for a gray pair."""
        planes = np.empty((self.hei, self.wid, 6), np.uint8)           # (room for either channel count)
        self._ck(self._lib.psm_sgm_download_prefiltered(self._h, int(side), _ptr(planes)), "sgm_prefiltered")
        ch = self._sgm_ch
        return planes.reshape(-1)[:self.hei * self.wid * 2 * ch].reshape(self.hei, self.wid, 2 * ch).copy()

    def sgm_census(self, side: int):
        """Test hook: the census codes [H][W] uint64 of the left (side 0) or right (1) image in the last SGBM_GPU, which must have
        run with census=(win_w, win_h)."""
        codes = np.empty((self.hei, self.wid), np.uint64)
        self._ck(self._lib.psm_sgm_download_census(self._h, int(side), _ptr(codes)), "sgm_census")
        return codes

    def sgm_times(self):
        """(cost, paths, select + check) device ms of the last SGBM_GPU; needs PSM_OPT_PROFILE."""
        ms = (C.c_double * 3)()
        self._ck(self._lib.psm_sgm_times(self._h, ms), "sgm_times")
        return tuple(ms)

    def filter_speckles(self, disp, new_val: int, max_speckle_size: int, max_diff: int):
        """cv::filterSpeckles(disp, newVal, maxSpeckleSize, maxDiff) on the device (psm_sgm_filter_speckles): disp H x W int16 of
        the size DispEst was built for -> the filtered copy.  Components of at most max_speckle_size pixels (4-neighbours, values
        != new_val, |difference| <= max_diff) become new_val.  The results of SGBM_GPU are untouched."""
        disp = np.asarray(disp)
        if disp.shape != (self.hei, self.wid) or disp.dtype != np.int16:
            raise ValueError("filter_speckles: disp must be an H x W int16 map of the size DispEst was built for")
        out = np.array(disp, order="C", copy=True)
        self._ck(self._lib.psm_sgm_filter_speckles(self._h, _ptr(out), out.strides[0], int(new_val), int(max_speckle_size),
                                                   int(max_diff)), "filter_speckles")
        return out

    def sgm_speckle_sizes(self):
        """Test hook: H x W int32, the size of every pixel's component in the last speckle filter run (SGBM_GPU with the filter
        on, or filter_speckles); 0 where the pixel was new_val on input."""
        sizes = np.empty((self.hei, self.wid), np.int32)
        self._ck(self._lib.psm_sgm_download_speckle_sizes(self._h, _ptr(sizes), sizes.strides[0]), "sgm_speckle_sizes")
        return sizes

    def sgm_speckle_time(self):
        """Device ms of the speckle filter's launches in the last SGBM_GPU (or filter_speckles); needs PSM_OPT_PROFILE."""
        ms = C.c_double()
        self._ck(self._lib.psm_sgm_speckle_time(self._h, C.byref(ms)), "sgm_speckle_time")
        return ms.value

    def SGBMSelect_GPU(self, download: bool = True):
        """psm_sgm_select_maps: the 8-bit maps of both views from the S of the last SGBM_GPU (sgbm_batch) into the object's device
        maps, where LRCheck_GPU, FillInv_GPU, WgtMedian_GPU, JointWMF_GPU, Score_GPU(PSM_SCORE_GIF) and download_maps() find
        them: the left map is the winner-takes-all disparity of S, the right map Hirschmueller's search along the epipolar line
        in the same S (tests/sgm_maps_model.py).  The range is the one that SGBM_GPU ran with; it must lie inside [0, maxDis).
        The int16 map, sgm_costs() and the guided-filter path's volumes are untouched.  -> (lDisMap, rDisMap); download=False:
        the maps stay on the device, None."""
        if download:
            self._ck(self._lib.psm_sgm_select_maps(self._h, _ptr(self.lDisMap), _ptr(self.rDisMap), self.wid), "SGBMSelect_GPU")
            return self.lDisMap, self.rDisMap
        self._ck(self._lib.psm_sgm_select_maps(self._h, None, None, 0), "SGBMSelect_GPU")
        return None

    # ---- the guided-filter path over a one-channel pair (psm_gray_compute) --------------------------
    def Gray_GPU(self, gl, gr, download: bool = True, subsample_rate: int = 0):
        """Cost build, one-channel guided filter and winner-takes-all of the monochrome pair (gl, gr) - two H x W planes, uint8 or
        float32 (uint8 is scaled by 1/255 as setInputImages scales) - in one call; the definition is tests/gray_model.py.  The maps
        land in the object's device maps, where LRCheck_GPU, FillInv_GPU, Score_GPU(PSM_SCORE_GIF), Reproject_GPU and
        download_maps() find them; the staged colour pair, the volumes and whatever CostFilter_GPU left pending are untouched.
        subsample_rate 2, 4 or 8: the Fast Guided Filter in place of the full-resolution one (psm_gray_compute_fgf,
        FastGuidedFilterMono; the definition is tests/gray_fgf_model.py); 0: every bit as without the argument.
        -> (lDisMap, rDisMap); download=False: the maps stay on the device, None."""
        gl, gr = np.asarray(gl), np.asarray(gr)
        if gl.shape != (self.hei, self.wid) or gr.shape != gl.shape or gl.dtype != gr.dtype:
            raise ValueError("Gray_GPU: gl, gr must be two H x W planes of one type and of the size DispEst was built for")
        if gl.dtype == np.uint8:
            depth = capi.PSM_IMG_U8
        elif gl.dtype == np.float32:
            depth = capi.PSM_IMG_F32
        else:
            raise ValueError("Gray_GPU: planes must be uint8 or float32")
        if gl.strides[1] != gl.itemsize or gr.strides != gl.strides or gl.strides[0] < self.wid * gl.itemsize:
            gl, gr = np.ascontiguousarray(gl), np.ascontiguousarray(gr)      # (rows with a pitch go as they are)
        lm, rm = (_ptr(self.lDisMap), _ptr(self.rDisMap)) if download else (None, None)
        if subsample_rate:
            self._ck(self._lib.psm_gray_compute_fgf(self._h, _ptr(gl), _ptr(gr), gl.strides[0], depth, int(subsample_rate), lm, rm,
                                                    self.wid if download else 0), "Gray_GPU")
        else:
            self._ck(self._lib.psm_gray_compute(self._h, _ptr(gl), _ptr(gr), gl.strides[0], depth, lm, rm, self.wid if download else 0),
                     "Gray_GPU")
        self._gray_rate = int(subsample_rate)
        return (self.lDisMap, self.rDisMap) if download else None

    def gray_guidance(self, side: int):
        """Test hook: [4][H][W] float32 - I, G, mI, inv - of `side` of the last Gray_GPU's pair."""
        planes = np.empty((4, self.hei, self.wid), np.float32)
        self._ck(self._lib.psm_gray_guidance(self._h, int(side), _ptr(planes)), "gray_guidance")
        return planes

    def gray_volume(self, side: int, d0: int = 0, d1: int | None = None, want_ab: bool = False):
        """Test hook: the filtered slices [d0, d1) of `side` of the last Gray_GPU's pair through the storing form of its kernels:
        q [d1-d0][H][W] float32, and - want_ab - ab [d1-d0][2][H][W], the planes a and b of every slice."""
        d1 = self.maxDis if d1 is None else int(d1)
        n = max(d1 - int(d0), 0)
        q = np.empty((n, self.hei, self.wid), np.float32)
        ab = np.empty((n, 2, self.hei, self.wid), np.float32) if want_ab else None
        self._ck(self._lib.psm_gray_volume(self._h, int(side), int(d0), d1, _ptr(q), _ptr(ab)), "gray_volume")
        return (q, ab) if want_ab else q

    def gray_fgf_guidance(self, side: int):
        """Test hook: [3][H/s][W/s] float32 - Is, mI, den - of `side` of the last Gray_GPU(subsample_rate=s)'s pair."""
        s = self._gray_rate or 1
        planes = np.empty((3, self.hei // s, self.wid // s), np.float32)
        self._ck(self._lib.psm_gray_fgf_guidance(self._h, int(side), _ptr(planes)), "gray_fgf_guidance")
        return planes

    def gray_fgf_volume(self, side: int, d0: int = 0, d1: int | None = None, want_model: bool = False):
        """Test hook: the filtered slices [d0, d1) of `side` of the last Gray_GPU(subsample_rate=s)'s pair through the storing form
        of its kernels: q [d1-d0][H][W] float32, and - want_model - [d1-d0][4][H/s][W/s]: a, b, blur(a), blur(b) of every slice."""
        s = self._gray_rate or 1
        d1 = self.maxDis if d1 is None else int(d1)
        n = max(d1 - int(d0), 0)
        q = np.empty((n, self.hei, self.wid), np.float32)
        model = np.empty((n, 4, self.hei // s, self.wid // s), np.float32) if want_model else None
        self._ck(self._lib.psm_gray_fgf_volume(self._h, int(side), int(d0), d1, _ptr(q), _ptr(model)), "gray_fgf_volume")
        return (q, model) if want_model else q

    def gray_time(self):
        """Device ms of the launches of the last Gray_GPU; needs PSM_OPT_PROFILE."""
        ms = C.c_double()
        self._ck(self._lib.psm_gray_time(self._h, C.byref(ms)), "gray_time")
        return ms.value

    def sgm_maps_time(self):
        """Device ms of the launch of the last SGBMSelect_GPU (sgbm_select_batch: of all pairs, on its first object); needs
        PSM_OPT_PROFILE."""
        ms = C.c_double()
        self._ck(self._lib.psm_sgm_maps_time(self._h, C.byref(ms)), "sgm_maps_time")
        return ms.value

    # ---- score: display maps and the error metric on the device (src/StereoMatch.cpp:181-185, 248-249, 275-309) ----
    def set_truth(self, gt, mask=None):
        """The dataset's ground truth and (optional) error mask, H x W uint8 each: uploaded once, kept until replaced or
        clear_truth() (psm_score_set_truth)."""
        gt = np.asarray(gt)
        mask = None if mask is None else np.asarray(mask)
        for a in (gt, mask):
            if a is not None and (a.shape != (self.hei, self.wid) or a.dtype != np.uint8):
                raise ValueError("set_truth: gt and mask must be H x W uint8 planes of the size DispEst was built for")
        if mask is not None and (mask.strides != gt.strides or gt.strides[1] != 1):
            gt, mask = np.ascontiguousarray(gt), np.ascontiguousarray(mask)
        elif gt.strides[1] != 1:
            gt = np.ascontiguousarray(gt)
        self._ck(self._lib.psm_score_set_truth(self._h, _ptr(gt), _ptr(mask), gt.strides[0]), "set_truth")

    def clear_truth(self):
        self._ck(self._lib.psm_score_clear_truth(self._h), "clear_truth")

    def set_score_params(self, scale_factor: int = 4, error_threshold: int = 4, mask_mode: int = capi.PSM_MASK_NONOCC):
        """scale_factor 1..255, error_threshold 0..255, mask_mode capi.PSM_MASK_NONE | PSM_MASK_NONOCC | PSM_MASK_DISC
        (psm_score_set_params; a new object: 4, 4, NONOCC)."""
        self._ck(self._lib.psm_score_set_params(self._h, int(scale_factor), int(error_threshold), int(mask_mode)),
                 "set_score_params")

    def Score_GPU(self, source: int = capi.PSM_SCORE_GIF):
        """psm_score: the display map(s) and the reference's error record of the current result, on the device.  source:
        capi.PSM_SCORE_GIF (the current 8-bit maps), PSM_SCORE_SGM (the int16 map of the last SGBM_GPU through the reference's
        min-max display conversion) or PSM_SCORE_SGM_INT (its integer disparities scaled like the GIF maps).
        -> dict: the record's integers (min_val, max_val, pixels, bad, err_sum, unit, flags) and bp_percent / avg_err derived from
        them; under PSM_OPT_ASYNC None - score_wait() collects the record."""
        rec = capi.Score()
        self._ck(self._lib.psm_score(self._h, int(source), C.byref(rec)), "Score_GPU")
        return None if self.options.get(capi.PSM_OPT_ASYNC) else rec.as_dict()

    def score_wait(self):
        """The record of the Score_GPU enqueued under PSM_OPT_ASYNC."""
        rec = capi.Score()
        self._ck(self._lib.psm_score_wait(self._h, C.byref(rec)), "score_wait")
        return rec.as_dict()

    def score_maps(self, right: bool = False):
        """(left display, error plane) of the last Score_GPU, H x W uint8 each; right=True: (left, right, error) - the right
        display exists for PSM_SCORE_GIF only."""
        l, e = np.empty((self.hei, self.wid), np.uint8), np.empty((self.hei, self.wid), np.uint8)
        r = np.empty((self.hei, self.wid), np.uint8) if right else None
        self._ck(self._lib.psm_score_download(self._h, _ptr(l), _ptr(r), _ptr(e), self.wid), "score_maps")
        return (l, r, e) if right else (l, e)

    def score_time(self):
        """Device ms of the launches of the last Score_GPU (score_batch: of all pairs, on its first object); needs PSM_OPT_PROFILE."""
        ms = C.c_double()
        self._ck(self._lib.psm_score_time(self._h, C.byref(ms)), "score_time")
        return ms.value

    def upload_sgm_map(self, disp):
        """Test hook (psm_score_upload_sgm_map): the SGM sources of Score_GPU read this H x W int16 map from now on; None: the
        map of the last SGBM_GPU again."""
        if disp is None:
            self._ck(self._lib.psm_score_upload_sgm_map(self._h, None, 0), "upload_sgm_map")
            return
        disp = np.ascontiguousarray(disp)
        if disp.shape != (self.hei, self.wid) or disp.dtype != np.int16:
            raise ValueError("upload_sgm_map: disp must be an H x W int16 map of the size DispEst was built for")
        self._ck(self._lib.psm_score_upload_sgm_map(self._h, _ptr(disp), disp.strides[0]), "upload_sgm_map")

    # ---- reproject: from disparity to depth on the device (cv::reprojectImageTo3D with the Q of src/StereoMatch.cpp:456-458) ----
    _depth_outputs = 0                           # the outputs of the last Reproject_GPU (reproject_batch)

    def setReprojection(self, Q, crop=(0, 0), z_range=None):
        """Q: the 4 x 4 matrix of cv::stereoRectify (rectify.load_calibration(...)["Q"], or rectify.q_from_projections); crop: the
        (x, y) of this object's image inside the rectified one (the cropBox of src/StereoMatch.cpp:474-481; an (x, y, w, h) box
        is taken by its first two); z_range = (z_min, z_max): the cloud keeps z_min < z <= z_max (None: unchanged; a new
        object: (0, FLT_MAX)).  psm_reproject_set_q / psm_reproject_set_range."""
        q = np.ascontiguousarray(Q, dtype=np.float64)
        if q.size != 16:
            raise ValueError("setReprojection: Q must hold 4 x 4 values")
        self._ck(self._lib.psm_reproject_set_q(self._h, q.ctypes.data_as(C.POINTER(C.c_double)), int(crop[0]), int(crop[1])),
                 "setReprojection")
        if z_range is not None:
            self._ck(self._lib.psm_reproject_set_range(self._h, float(z_range[0]), float(z_range[1])), "setReprojection")

    def Reproject_GPU(self, source: int = capi.PSM_DEPTH_GIF, outputs: int = capi.PSM_DEPTH_CLOUD, use_mask: bool = False):
        """psm_reproject: the points of the current result, on the device.  source: capi.PSM_DEPTH_GIF (the current left 8-bit
        map; use_mask: pixels the current L-R mask marks invalid are missing) or PSM_DEPTH_SGM (the int16 map of the last
        SGBM_GPU); outputs: any of capi.PSM_DEPTH_XYZ | PSM_DEPTH_Z | PSM_DEPTH_CLOUD.  -> the number of kept pixels; under
        PSM_OPT_ASYNC None - reproject_wait() collects it.  reprojected() and cloud() download the results."""
        n = C.c_uint32()
        flags = capi.PSM_DEPTH_USE_MASK if use_mask else 0
        self._ck(self._lib.psm_reproject(self._h, int(source), int(outputs), flags, C.byref(n)), "Reproject_GPU")
        self._depth_outputs = int(outputs)
        return None if self.options.get(capi.PSM_OPT_ASYNC) else int(n.value)

    def reproject_wait(self):
        """The count of the Reproject_GPU enqueued under PSM_OPT_ASYNC."""
        n = C.c_uint32()
        self._ck(self._lib.psm_reproject_wait(self._h, C.byref(n)), "reproject_wait")
        return int(n.value)

    def reprojected(self):
        """The dense planes of the last Reproject_GPU: (xyz H x W x 3 float32 or None, z H x W float32 or None) - what its
        outputs named.  Void pixels hold the bit pattern capi.PSM_DEPTH_VOID (a NaN)."""
        xyz = np.empty((self.hei, self.wid, 3), np.float32) if self._depth_outputs & capi.PSM_DEPTH_XYZ else None
        z = np.empty((self.hei, self.wid), np.float32) if self._depth_outputs & capi.PSM_DEPTH_Z else None
        self._ck(self._lib.psm_reproject_download(self._h, _ptr(xyz), _ptr(z), 0), "reprojected")
        return xyz, z

    def cloud(self):
        """The point cloud of the last Reproject_GPU (with PSM_DEPTH_CLOUD): a structured array of capi.point_dtype() - x, y,
        z, b, g, r, a - the kept pixels in raster order."""
        rec = np.empty(self.hei * self.wid, capi.point_dtype())
        n = C.c_uint32()
        self._ck(self._lib.psm_reproject_download_cloud(self._h, _ptr(rec), rec.size, C.byref(n)), "cloud")
        return rec[:n.value].copy()

    def reproject_time(self):
        """Device ms of the launches of the last Reproject_GPU (reproject_batch: of all pairs, on its first object); needs
        PSM_OPT_PROFILE."""
        ms = C.c_double()
        self._ck(self._lib.psm_reproject_time(self._h, C.byref(ms)), "reproject_time")
        return ms.value

    # ---- WLS smoothing of the sub-pixel map (psm_wls_filter; the definition is tests/wls_model.py) ----
    def setWLS(self, lam: float = 8000.0, sigma: float = 1.5, iterations: int = 3):
        """psm_wls_set_params: lambda > 0, sigma > 0, iterations in 1..4 (a new object: 8000, 1.5, 3)."""
        self._ck(self._lib.psm_wls_set_params(self._h, float(lam), float(sigma), int(iterations)), "setWLS")

    def setWLSConfidence(self, terms: int = capi.PSM_WLS_CONF_LR | capi.PSM_WLS_CONF_VAR, lr_thresh: int = 24, radius: int = 2,
                         var_shift: int = 8):
        """psm_wls_set_confidence: the terms (capi.PSM_WLS_CONF_LR | PSM_WLS_CONF_VAR) and parameters of the graded confidence
        WLS_GPU(confidence=...) starts with - lr_thresh in 1..32767 (16ths), radius in 1..4, var_shift in 0..16."""
        self._ck(self._lib.psm_wls_set_confidence(self._h, int(terms), int(lr_thresh), int(radius), int(var_shift)), "setWLSConfidence")

    def WLS_GPU(self, source: int = capi.PSM_WLS_SGM, use_mask: bool = False, confidence=None):
        """psm_wls_filter: the confidence-weighted, edge-aware global smoothing (Fast Global Smoother) of the int16 map of the last
        SGBM_GPU (capi.PSM_WLS_SGM) or of the current left 8-bit map times 16 (PSM_WLS_GIF; use_mask: pixels the current L-R mask
        marks invalid are missing), guided by the left image: the holes are filled, the sixteenths stay.  Under PSM_OPT_ASYNC
        wls_wait() waits for it.  wls_map() and wls_planes() download the results; wls_publish() hands the map to the SGM
        sources of Score_GPU and Reproject_GPU.
        confidence: None, the default: every valid pixel starts with the weight 1.  Else a dict of setWLSConfidence's parameters
        ({}: both terms, 24, 2, 8; PSM_WLS_SGM only): they are set, and the solve starts with the graded confidence of
        tests/wls_conf_model.py (PSM_WLS_CONFIDENCE) - download_wls_confidence() gives its planes."""
        flags = capi.PSM_WLS_USE_MASK if use_mask else 0
        if confidence is not None:
            self.setWLSConfidence(**confidence)
            flags |= capi.PSM_WLS_CONFIDENCE
        self._ck(self._lib.psm_wls_filter(self._h, int(source), flags), "WLS_GPU")

    def download_wls_confidence(self, right: bool = True):
        """The planes of the last WLS_GPU(confidence=...): (conf H x W uint8, right16 H x W int16 - the right view's map in 16ths;
        None with right=False, which a run without the L-R term needs)."""
        conf = np.empty((self.hei, self.wid), np.uint8)
        r16 = np.empty((self.hei, self.wid), np.int16) if right else None
        self._ck(self._lib.psm_wls_download_confidence(self._h, _ptr(conf), 0, _ptr(r16) if right else None, 0), "download_wls_confidence")
        return conf, r16

    def wls_conf_time(self):
        """Device ms of the two launches the confidence adds to the last WLS_GPU; needs PSM_OPT_PROFILE."""
        ms = C.c_double()
        self._ck(self._lib.psm_wls_conf_time(self._h, C.byref(ms)), "wls_conf_time")
        return ms.value

    def wls_wait(self):
        """Wait for the WLS_GPU enqueued under PSM_OPT_ASYNC."""
        self._ck(self._lib.psm_wls_wait(self._h), "wls_wait")

    def wls_map(self):
        """The filtered map of the last WLS_GPU: H x W int16 in 16ths, with the invalid value of the map it came from."""
        disp = np.empty((self.hei, self.wid), np.int16)
        self._ck(self._lib.psm_wls_download(self._h, _ptr(disp), None, None, None, 0), "wls_map")
        return disp

    def wls_planes(self):
        """The float planes of the last WLS_GPU: (q, num, den), H x W float32 each - the quotient (void pixels hold the bit
        pattern capi.PSM_WLS_VOID, a NaN) and the working planes as the last pass left them."""
        q, num, den = (np.empty((self.hei, self.wid), np.float32) for _ in range(3))
        self._ck(self._lib.psm_wls_download(self._h, None, _ptr(q), _ptr(num), _ptr(den), 0), "wls_planes")
        return q, num, den

    def wls_table(self):
        """The 256 weights the last WLS_GPU read on the device."""
        tab = np.empty(256, np.float32)
        self._ck(self._lib.psm_wls_download_table(self._h, _ptr(tab)), "wls_table")
        return tab

    def wls_publish(self, on: bool = True):
        """psm_wls_publish: while on, the SGM sources of Score_GPU / Reproject_GPU (and their batches) read the map of the last
        WLS_GPU instead of the SGM stage's."""
        self._ck(self._lib.psm_wls_publish(self._h, 1 if on else 0), "wls_publish")

    def wls_time(self):
        """Device ms of the launches of the last WLS_GPU; needs PSM_OPT_PROFILE."""
        ms = C.c_double()
        self._ck(self._lib.psm_wls_time(self._h, C.byref(ms)), "wls_time")
        return ms.value

    # ---- extensions beyond the reference surface --------------------------------------------
    def LRCheck_GPU(self) -> int:
        """PP lrCheck (src/PP.cpp:17-50) on the device -> lValid / rValid."""
        self._ck(self._lib.psm_lr_check(self._h, _ptr(self.lValid), _ptr(self.rValid), self.wid),
                 "LRCheck_GPU")
        return 0

    def LRCheck_device(self):
        """PP lrCheck with the validity masks left on the device (bench: D2H excluded from the timed region)."""
        self._ck(self._lib.psm_lr_check(self._h, None, None, 0), "LRCheck_device")

    def download_valid(self):
        """The validity masks of the last LRCheck (psm_lr_check is idempotent on unchanged maps: run again, with download)."""
        self.LRCheck_GPU()
        return self.lValid, self.rValid

    def FillInv_GPU(self) -> int:
        """PP fillInv (src/PP.cpp:52-143) on the device; updates lDisMap / rDisMap."""
        self._ck(self._lib.psm_fill_invalid(self._h, _ptr(self.lDisMap), _ptr(self.rDisMap), self.wid),
                 "FillInv_GPU")
        return 0

    def WgtMedian_GPU(self) -> int:
        """PP wgtMedian (src/PP.cpp:145-247) on the device, for the pixels LRCheck_GPU marked invalid; updates
        lDisMap / rDisMap.  Same result as the reference's sequential in-place form."""
        self._ck(self._lib.psm_wgt_median(self._h, _ptr(self.lDisMap), _ptr(self.rDisMap), self.wid), "WgtMedian_GPU")
        return 0

    def JointWMF_GPU(self, radius: int = 0, sigma: float = 0.0, n_clusters: int = 0, max_iter: int = 0) -> int:
        """The reference's live post-filter: PP::processDM = JointWMF::filter on both maps with the 8-bit colour images
        (src/PP.cpp:402-424) on the device; updates lDisMap / rDisMap, the valid masks stay as they are.  0: the
        reference's radius 9, sigma 25.5, 256 clusters, 10000 k-means iterations.  PostProcess_GPU is unchanged."""
        self._ck(self._lib.psm_joint_wmf(self._h, int(radius), float(sigma), int(n_clusters), int(max_iter),
                                         _ptr(self.lDisMap), _ptr(self.rDisMap), self.wid), "JointWMF_GPU")
        return 0

    def set_jwmf_clusters(self, side: int, centres, label_of_key):
        """Bring-your-own clustering of one side for JointWMF_GPU: centres [n, 3] (6-bit B, G, R), label_of_key [64**3]."""
        cen = np.ascontiguousarray(centres, dtype=np.float32).reshape(-1, 3)
        lok = np.ascontiguousarray(label_of_key, dtype=np.uint8).reshape(-1)
        if lok.size != 64 ** 3:
            raise ValueError("label_of_key must hold 64**3 entries")
        self._ck(self._lib.psm_joint_wmf_set_clusters(self._h, int(side), int(cen.shape[0]), _ptr(cen), _ptr(lok)),
                 "set_jwmf_clusters")

    def jwmf_clusters(self, side: int):
        """-> (centres [n, 3] float32, label_of_key [64**3] uint8, iterations) of the clustering JointWMF_GPU used."""
        import ctypes as C
        n, it = C.c_int(), C.c_int()
        cen = np.zeros((256, 3), np.float32)
        lok = np.zeros(64 ** 3, np.uint8)
        self._ck(self._lib.psm_joint_wmf_clusters(self._h, int(side), C.byref(n), _ptr(cen), _ptr(lok), C.byref(it)),
                 "jwmf_clusters")
        return cen[:n.value].copy(), lok, it.value

    def wgt_median_stats(self):
        """(sweeps, evaluations) of the last WgtMedian_GPU per map [left, right]; sweeps = -1: the dataflow form ran."""
        import ctypes as C
        sw, ev = (C.c_int * 2)(), (C.c_longlong * 2)()
        self._ck(self._lib.psm_wgt_median_stats(self._h, sw, ev), "wgt_median_stats")
        return list(sw), list(ev)

    def upload_maps(self, lmap=None, rmap=None, lvalid=None, rvalid=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8) for a in (lmap, rmap, lvalid, rvalid)]
        for a in arrs:
            assert a is None or a.shape == (self.hei, self.wid)
        self._ck(self._lib.psm_upload_maps(self._h, *[_ptr(a) for a in arrs], self.wid), "upload_maps")

    def set_option(self, option: int, value: int):
        self._ck(self._lib.psm_set_option(self._h, int(option), int(value)), "set_option")
        self.options[int(option)] = int(value)           # (what was accepted, for callers that inspect a context)

    def set_stream(self, stream_ptr: int | None):
        self._ck(self._lib.psm_set_stream(self._h, C.c_void_p(stream_ptr or 0)), "set_stream")

    def release_scratch(self):
        """Give back the on-first-use scratch (weighted-median cache, minima planes, exchange buffers); see psm_release_scratch."""
        self._ck(self._lib.psm_release_scratch(self._h), "release_scratch")

    def synchronize(self):
        self._ck(self._lib.psm_synchronize(self._h), "synchronize")

    def DispSelect_partial(self, dev_keys_ptr: int | None = None):
        self._ck(self._lib.psm_disp_select_partial(self._h, C.c_void_p(dev_keys_ptr or 0)),
                 "DispSelect_partial")

    def CostFilter_side(self, side: int):
        self._ck(self._lib.psm_cost_filter_side(self._h, int(side)), "CostFilter_side")

    def DispSelect_partial_side(self, side: int, dev_keys_ptr: int | None = None):
        self._ck(self._lib.psm_disp_select_partial_side(self._h, int(side), C.c_void_p(dev_keys_ptr or 0)),
                 "DispSelect_partial_side")

    def set_key_buffer(self, dev_keys_ptr: int | None):
        """The packed minima of the following frames go straight into this device buffer (2*H*W int64); None: own buffer."""
        self._ck(self._lib.psm_set_key_buffer(self._h, C.c_void_p(dev_keys_ptr or 0)), "set_key_buffer")

    def partial_keys(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self._lib.psm_partial_keys(self._h, C.byref(p), C.byref(n)), "partial_keys")
        return p.value, n.value

    def DispSelect_merge(self, dev_keys_all_ptr: int, nranks: int, download: bool = True):
        self._ck(self._lib.psm_disp_merge(self._h, C.c_void_p(dev_keys_all_ptr), int(nranks),
                                          _ptr(self.lDisMap) if download else None,
                                          _ptr(self.rDisMap) if download else None, self.wid),
                 "DispSelect_merge")

    def DispSelect_merge_ctx(self, shards, download: bool = True):
        """Single-process exchange: merge the partial keys of `shards` (DispEst objects)."""
        arr = (C.c_void_p * len(shards))(*[s._h for s in shards])
        self._ck(self._lib.psm_disp_merge_ctx(self._h, arr, len(shards),
                                              _ptr(self.lDisMap) if download else None,
                                              _ptr(self.rDisMap) if download else None, self.wid),
                 "DispSelect_merge_ctx")

    def set_rows(self, y_begin: int = 0, y_end: int = 0):
        """Row stripe: CostFilter_GPU / DispSelect* compute output rows [y_begin, y_end) of the whole image only (all
        slices, both volumes, identical values); (0, 0): whole image.  Call before CostFilter_GPU."""
        self._ck(self._lib.psm_set_rows(self._h, int(y_begin), int(y_end)), "set_rows")

    def set_map_buffer(self, dev_maps_ptr: int | None, whole: bool = False):
        """The device maps [2][H][W] uint8 live in this device buffer (>= 2*H*W + 4 bytes) from now on; None: own buffer.
        whole: the buffer already holds both complete maps of the current frame."""
        self._ck(self._lib.psm_set_map_buffer(self._h, C.c_void_p(dev_maps_ptr or 0), int(whole)), "set_map_buffer")

    def gather_rows_ctx(self, stripes, download: bool = True):
        """Single-process exchange of the row-stripe sharding: the stripe rows of every context's maps -> this context."""
        arr = (C.c_void_p * len(stripes))(*[s._h for s in stripes])
        self._ck(self._lib.psm_gather_rows_ctx(self._h, arr, len(stripes),
                                               _ptr(self.lDisMap) if download else None,
                                               _ptr(self.rDisMap) if download else None, self.wid),
                 "gather_rows_ctx")

    def DispSelect_device(self):
        """WTA with the maps left on the device (bench: D2H excluded from the timed region)."""
        self._ck(self._lib.psm_disp_select(self._h, None, None, 0), "DispSelect_device")

    def download_maps(self):
        self._ck(self._lib.psm_download_maps(self._h, _ptr(self.lDisMap), _ptr(self.rDisMap), self.wid),
                 "download_maps")
        return self.lDisMap, self.rDisMap

    # ---- frame loop: the PCIe legs next to the kernels (src/main.cpp:64-73) ----
    def setInputImages_async(self, l, r) -> int:
        """The NEXT frame's pair: staged and copied on the copy stream while the current frame computes; the next
        CostConst_GPU adopts it."""
        l = np.ascontiguousarray(l)
        r = np.ascontiguousarray(r)
        if l.shape != (self.hei, self.wid, 3) or r.shape != l.shape or l.dtype != r.dtype:
            raise ValueError("setInputImages_async: image size / type differs from the one DispEst was built for")
        depth = capi.PSM_IMG_U8 if l.dtype == np.uint8 else capi.PSM_IMG_F32
        self._ck(self._lib.psm_upload_pair_async(self._h, _ptr(l), _ptr(r), 3, l.strides[0], depth), "setInputImages_async")
        return 0

    # ---- video mode: the camera frame is rectified and cropped on the device (src/StereoMatch.cpp:138-153) ----
    def setRectification(self, rect) -> int:
        """rect: rectify.Rectification whose crop has this object's size.  The maps go to the device once."""
        x, y, w, h = rect.crop
        if (w, h) != (self.wid, self.hei):
            raise ValueError("setRectification: the crop's size differs from the one DispEst was built for")
        for side in (capi.PSM_LEFT, capi.PSM_RIGHT):
            xy = np.ascontiguousarray(rect.map_xy[side], dtype=np.int16)
            fr = np.ascontiguousarray(rect.map_frac[side], dtype=np.uint16)
            if xy.ndim != 3 or xy.shape[2] != 2 or fr.shape != xy.shape[:2]:
                raise ValueError("setRectification: maps must be [h, w, 2] int16 and [h, w] uint16")
            self._ck(self._lib.psm_rectify_set_maps(self._h, side, _ptr(xy), _ptr(fr), xy.shape[1], xy.shape[0], int(rect.src_w),
                                                    int(rect.src_h), int(x), int(y)), "setRectification")
        self._rect_src = (int(rect.src_h), int(rect.src_w))
        if getattr(rect, "Q", None) is not None:             # the calibration's Q came along: the object can reproject as well
            self.setReprojection(rect.Q, crop=(x, y))
        return 0

    def clearRectification(self):
        self._ck(self._lib.psm_rectify_clear(self._h), "clearRectification")
        self._rect_src = None

    def _eyes(self, vFrame, who):
        """The two halves of a side-by-side frame as pointers into it (the cv::Mat ROIs of src/StereoMatch.cpp:138-139: no copy)."""
        src = getattr(self, "_rect_src", None)
        if src is None:
            raise capi.PsmError(f"{who}: no rectification set (setRectification)")
        v = np.asarray(vFrame)
        if v.dtype != np.uint8:
            raise ValueError(f"{who}: the frame must be uint8 (float frames are not remapped)")
        if v.ndim != 3 or v.shape != (src[0], 2 * src[1], 3):
            raise ValueError(f"{who}: the frame must be {src[0]} x {2 * src[1]} x 3 (two eyes side by side)")
        if v.strides[2] != 1 or v.strides[1] != 3:
            v = np.ascontiguousarray(v)
        base = v.ctypes.data
        return v, C.c_void_p(base), C.c_void_p(base + 3 * src[1]), v.strides[0]

    def setInputFrame(self, vFrame) -> int:
        """vFrame: the camera's side-by-side frame, src_h x 2 src_w x 3 uint8, unrectified; the pair the object holds afterwards is
        remap(eye, maps, INTER_LINEAR)(cropBox) of both eyes."""
        v, l, r, stride = self._eyes(vFrame, "setInputFrame")
        self._ck(self._lib.psm_upload_pair_rectified(self._h, l, r, 3, stride), "setInputFrame")
        return 0

    def setInputFrame_async(self, vFrame) -> int:
        """setInputFrame for the NEXT frame (as setInputImages_async): copy and remap run on the copy stream while the current
        frame computes; the next CostConst_GPU adopts the pair."""
        v, l, r, stride = self._eyes(vFrame, "setInputFrame_async")
        self._ck(self._lib.psm_upload_pair_rectified_async(self._h, l, r, 3, stride), "setInputFrame_async")
        return 0

    def download_images(self):
        """The current 8-bit pair as staged on the device -> (l, r) H x W x 3 uint8 (the reference's leftInputImg / rightInputImg)."""
        l = np.empty((self.hei, self.wid, 3), np.uint8)
        r = np.empty((self.hei, self.wid, 3), np.uint8)
        self._ck(self._lib.psm_download_images(self._h, _ptr(l), _ptr(r), l.strides[0]), "download_images")
        return l, r

    def download_maps_async(self):
        self._ck(self._lib.psm_download_maps_async(self._h), "download_maps_async")

    def download_maps_wait(self):
        self._ck(self._lib.psm_download_maps_wait(self._h, _ptr(self.lDisMap), _ptr(self.rDisMap), self.wid), "download_maps_wait")
        return self.lDisMap, self.rDisMap

    def filter_launch_times(self, max_launches: int = 4096):
        """PSM_OPT_PROFILE 2: [(ms, form)] of every launch of the fused filter kernel since the last call (form 1 = minima
        planes, 2 = key plane, 0 = storing), from time stamps the kernel takes itself; resets the record."""
        ms = (C.c_double * max_launches)()
        form = (C.c_int * max_launches)()
        n = C.c_int()
        self._ck(self._lib.psm_filter_launch_times(self._h, ms, form, max_launches, C.byref(n)), "filter_launch_times")
        return [(ms[i], form[i]) for i in range(n.value)]

    def _vdtype(self):
        return np.uint8 if self._dtype == capi.PSM_U8 else np.float32

    def download_volume(self, side: int, d0: int | None = None, d1: int | None = None):
        d0 = self.d_begin if d0 is None else d0
        d1 = self.d_end if d1 is None else d1
        out = np.empty((d1 - d0, self.hei, self.wid), self._vdtype())
        self._ck(self._lib.psm_download_volume(self._h, side, d0, d1, _ptr(out)), "download_volume")
        return out

    def upload_volume(self, side: int, vol, d0: int | None = None):
        vol = np.ascontiguousarray(vol, dtype=self._vdtype())
        d0 = self.d_begin if d0 is None else d0
        assert vol.shape[1:] == (self.hei, self.wid)
        self._ck(self._lib.psm_upload_volume(self._h, side, d0, d0 + vol.shape[0], _ptr(vol)),
                 "upload_volume")

    def filter_stage_a(self, side: int):
        self._ck(self._lib.psm_filter_stage_a(self._h, side), "filter_stage_a")

    def download_ab(self, d0: int | None = None, d1: int | None = None):
        d0 = self.d_begin if d0 is None else d0
        d1 = self.d_end if d1 is None else d1
        out = np.empty((d1 - d0, self.hei, self.wid, 4), np.float32)
        self._ck(self._lib.psm_download_ab(self._h, d0, d1, _ptr(out)), "download_ab")
        return out

    def download_guidance(self, side: int):
        out = np.empty((14, self.hei, self.wid), np.float32)
        self._ck(self._lib.psm_download_guidance(self._h, side, _ptr(out)), "download_guidance")
        return out

    def box8_volume(self, side: int, download: bool = True):
        out = np.empty((self.d_end - self.d_begin, self.hei, self.wid), np.float32) if download else None
        self._ck(self._lib.psm_box8_volume(self._h, side, _ptr(out)), "box8_volume")
        return out

    def stage_time_us(self, stage: int) -> float:
        v = C.c_double()
        self._ck(self._lib.psm_stage_time_us(self._h, stage, C.byref(v)), "stage_time_us")
        return v.value

    def kernel_time_ms(self, kernel: int):
        v, n = C.c_double(), C.c_int()
        self._ck(self._lib.psm_kernel_time_ms(self._h, kernel, C.byref(v), C.byref(n)), "kernel_time_ms")
        return v.value, n.value

    def reset_kernel_times(self):
        self._ck(self._lib.psm_reset_kernel_times(self._h), "reset_kernel_times")


def compute_batch(des):
    """CostConst_GPU + CostFilter_GPU + DispSelect (maps left on the device) of several DispEst objects of one geometry in
    shared launches (psm_compute_batch): the reference's loop over pairs / datasets (src/main.cpp:64-73,
    src/StereoMatch.cpp:556-607) as one grid.  Every object afterwards behaves as after the three single-pair calls
    (download_maps(), LRCheck_GPU(), download_volume(), ...)."""
    des = list(des)
    if not des:
        return
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    capi.check(des[0]._lib.psm_compute_batch(arr, len(des)), des[0]._h, "compute_batch")


SGM_MODES = {"sgbm": 0, "hh": 1, "3way": 2, "hh4": 3}       # ssgbm->setMode: OpenCV's enum values


def sgm_mode(mode):
    """A mode name of SGM_MODES, or its integer (passed on as it is: psm_sgm_set_mode refuses what it does not know)."""
    if isinstance(mode, str):
        if mode not in SGM_MODES:
            raise ValueError(f"mode {mode!r} not in {sorted(SGM_MODES)}")
        return SGM_MODES[mode]
    return int(mode)


def census_window(census):
    """SGBM_GPU's census=: None is (0, 0), off; a pair is passed on as it is (psm_sgm_set_census refuses what it does not know)."""
    if census is None:
        return 0, 0
    win_w, win_h = census
    return int(win_w), int(win_h)


def sgbm_batch(des, block_size: int = 0, P1: int = 0, P2: int = 0, uniqueness_ratio: int = 10, disp12_max_diff: int = 1,
               speckle_window_size: int = 0, speckle_range: int = 0, pre_filter_cap: int = 0, mode="hh", min_disparity: int = 0,
               num_disparities: int = 0, census=None):
    """SGBM_GPU of several DispEst objects of one geometry in shared launches (psm_sgm_compute_batch): the parameters (SGBM_GPU's,
    without gray=) are set on every object, each object's own staged pair goes through the stage, -> the list of H x W int16 maps.
    Every object afterwards behaves as after its own SGBM_GPU (sgm_costs(), sgm_prefiltered(), sgm_census(), sgm_speckle_sizes(), ...); the
    times of the batch are des[0]'s (sgm_times(), sgm_speckle_time() under PSM_OPT_PROFILE)."""
    des = list(des)
    if not des:
        return []
    for d in des:
        d._ck(d._lib.psm_sgm_set_census(d._h, *census_window(census)), "sgbm_batch")
        d._ck(d._lib.psm_sgm_set_mode(d._h, sgm_mode(mode)), "sgbm_batch")
        d._ck(d._lib.psm_sgm_set_range(d._h, int(min_disparity), int(num_disparities)), "sgbm_batch")
        d._sgm_d = int(num_disparities) or d.maxDis
        d._ck(d._lib.psm_sgm_set_prefilter(d._h, int(pre_filter_cap)), "sgbm_batch")
        d._ck(d._lib.psm_sgm_set_speckle(d._h, int(speckle_window_size), int(speckle_range)), "sgbm_batch")
        d._ck(d._lib.psm_sgm_set_params(d._h, int(block_size), int(P1), int(P2), int(uniqueness_ratio), int(disp12_max_diff)),
              "sgbm_batch")
        d._sgm_ch = 3
    sgm_compute_batch(des)
    return [d.sgm_disparity() for d in des]


def sgm_compute_batch(des):
    """psm_sgm_compute_batch with the objects' parameters as they are (sgbm_batch sets them first)."""
    des = list(des)
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    capi.check(des[0]._lib.psm_sgm_compute_batch(arr, len(des)), des[0]._h, "sgm_compute_batch")


def sgbm_select_batch(des):
    """SGBMSelect_GPU(download=False) of several DispEst objects of one geometry in one launch (psm_sgm_select_maps_batch): each
    object's S becomes its own device maps; every object afterwards behaves as after its own call (download_maps(),
    LRCheck_GPU(), ...).  The results must share one disparity range."""
    des = list(des)
    if not des:
        return
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    capi.check(des[0]._lib.psm_sgm_select_maps_batch(arr, len(des)), des[0]._h, "sgbm_select_batch")


def joint_wmf_batch(des, radius: int = 0, sigma: float = 0.0, n_clusters: int = 0, max_iter: int = 0):
    """JointWMF_GPU of several DispEst objects of one geometry in shared launches (psm_joint_wmf_batch): each object's device maps
    are filtered with its own pair (the parameters: JointWMF_GPU's), the clustering chains of all images side by side; then every
    object's lDisMap / rDisMap are refreshed (download_maps).  Every object afterwards behaves as after its own JointWMF_GPU
    (jwmf_clusters(), a later JointWMF_GPU on the same pair reuses the clustering)."""
    des = list(des)
    if not des:
        return
    joint_wmf_batch_device(des, radius, sigma, n_clusters, max_iter)
    for d in des:
        d.download_maps()


def joint_wmf_batch_device(des, radius: int = 0, sigma: float = 0.0, n_clusters: int = 0, max_iter: int = 0):
    """psm_joint_wmf_batch alone: the filtered maps stay on the device (asynchronous under PSM_OPT_ASYNC on des[0] when no image
    needs the device k-means)."""
    des = list(des)
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    capi.check(des[0]._lib.psm_joint_wmf_batch(arr, len(des), int(radius), float(sigma), int(n_clusters), int(max_iter)),
               des[0]._h, "joint_wmf_batch")


def post_process_batch(des, lr_check: bool = True, fill: bool = False, median: bool = False, download: bool = True):
    """The named stages of PP::processDM's own sequence - LRCheck_GPU, FillInv_GPU, WgtMedian_GPU, in that order - of several DispEst
    objects of one geometry in shared launches (psm_post_process_batch): each object's device maps and masks with its own pair, the
    sweep chains of all maps side by side.  Every object afterwards behaves as after its own calls (wgt_median_stats() answers per
    object); download: every object's lDisMap / rDisMap / lValid / rValid receive its results."""
    des = list(des)
    if not des:
        return
    stages = (capi.PSM_PP_LR_CHECK if lr_check else 0) | (capi.PSM_PP_FILL if fill else 0) | (capi.PSM_PP_WGT_MEDIAN if median else 0)
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    capi.check(des[0]._lib.psm_post_process_batch(arr, len(des), stages), des[0]._h, "post_process_batch")
    if download:
        for d in des:
            d.download_maps()
            d._ck(d._lib.psm_download_valid(d._h, _ptr(d.lValid), _ptr(d.rValid), d.wid), "post_process_batch")


def score_batch(des, source: int = capi.PSM_SCORE_GIF):
    """Score_GPU of several DispEst objects of one geometry in one set of launches (psm_score_batch): each object's current result
    against its own truth -> the list of Score_GPU's dicts.  Every object afterwards behaves as after its own Score_GPU
    (score_maps()); under PSM_OPT_ASYNC on des[0]: None, every object's score_wait() collects its record."""
    des = list(des)
    if not des:
        return []
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    recs = (capi.Score * len(des))()
    capi.check(des[0]._lib.psm_score_batch(arr, len(des), int(source), recs), des[0]._h, "score_batch")
    return None if des[0].options.get(capi.PSM_OPT_ASYNC) else [r.as_dict() for r in recs]


def reproject_batch(des, source: int = capi.PSM_DEPTH_GIF, outputs: int = capi.PSM_DEPTH_CLOUD, use_mask: bool = False):
    """Reproject_GPU of several DispEst objects of one geometry in one set of launches (psm_reproject_batch): each object's current
    result with its own Q, crop and range -> the list of counts.  Every object afterwards behaves as after its own Reproject_GPU
    (reprojected(), cloud()); under PSM_OPT_ASYNC on des[0]: None, every object's reproject_wait() collects its count."""
    des = list(des)
    if not des:
        return []
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    counts = (C.c_uint32 * len(des))()
    flags = capi.PSM_DEPTH_USE_MASK if use_mask else 0
    capi.check(des[0]._lib.psm_reproject_batch(arr, len(des), int(source), int(outputs), flags, counts), des[0]._h, "reproject_batch")
    for d in des:
        d._depth_outputs = int(outputs)
    return None if des[0].options.get(capi.PSM_OPT_ASYNC) else [int(v) for v in counts]


def wls_batch(des, source: int = capi.PSM_WLS_SGM, use_mask: bool = False, confidence=None):
    """WLS_GPU of several DispEst objects of one geometry and one iteration count in one set of launches (psm_wls_filter_batch):
    each object's map with its own guide, lambda and sigma (setWLS) -> the list of filtered H x W int16 maps.  Every object
    afterwards behaves as after its own WLS_GPU (wls_map(), wls_planes(), wls_publish()); under PSM_OPT_ASYNC on des[0]: None,
    every object's wls_wait() waits for it.  wls_time() of des[0] is the batch's (PSM_OPT_PROFILE).  confidence: WLS_GPU's - one
    dict for every object, or a sequence of one dict per object (the terms and parameters may differ between them)."""
    des = list(des)
    if not des:
        return []
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    flags = capi.PSM_WLS_USE_MASK if use_mask else 0
    if confidence is not None:
        per = [confidence] * len(des) if isinstance(confidence, dict) else list(confidence)
        if len(per) != len(des):
            raise ValueError(f"wls_batch: {len(per)} confidence dicts for {len(des)} objects")
        for d, k in zip(des, per):
            d.setWLSConfidence(**k)
        flags |= capi.PSM_WLS_CONFIDENCE
    capi.check(des[0]._lib.psm_wls_filter_batch(arr, len(des), int(source), flags), des[0]._h, "wls_batch")
    return None if des[0].options.get(capi.PSM_OPT_ASYNC) else [d.wls_map() for d in des]


def gray_batch(des, gls=(), grs=(), download: bool = True, subsample_rate: int = 0):
    """Gray_GPU of several DispEst objects of one geometry in one set of launches (psm_gray_compute_batch): object i takes the
    monochrome pair (gls[i], grs[i]) - H x W planes, all uint8 or all float32.  Every object afterwards behaves as after its own
    Gray_GPU (LRCheck_GPU, Score_GPU(PSM_SCORE_GIF), download_maps(), the gray_* hooks).  -> the list of (lDisMap, rDisMap) of the
    objects; download=False: the maps stay on the device, a list of None.  gray_time() of des[0] is the batch's
    (PSM_OPT_PROFILE).  subsample_rate 2, 4 or 8: Gray_GPU(subsample_rate=...) of every object (psm_gray_compute_fgf_batch)."""
    des, gls, grs = list(des), [np.asarray(g) for g in gls], [np.asarray(g) for g in grs]
    if len(gls) != len(des) or len(grs) != len(des):
        raise ValueError("gray_batch: one (gl, gr) pair per object")
    if not des:
        return []
    shape, dtype = (des[0].hei, des[0].wid), gls[0].dtype
    if dtype == np.uint8:
        depth = capi.PSM_IMG_U8
    elif dtype == np.float32:
        depth = capi.PSM_IMG_F32
    else:
        raise ValueError("gray_batch: planes must be uint8 or float32")
    if any(g.shape != shape or g.dtype != dtype for g in gls + grs):
        raise ValueError("gray_batch: every plane must be H x W, of one type and of the size the objects were built for")
    row = shape[1] * gls[0].itemsize
    if any(g.strides != gls[0].strides for g in gls + grs) or gls[0].strides[1] != gls[0].itemsize or gls[0].strides[0] < row:
        gls, grs = [np.ascontiguousarray(g) for g in gls], [np.ascontiguousarray(g) for g in grs]      # (one pitch for the call)
    n = len(des)
    arr = (C.c_void_p * n)(*[d._h for d in des])
    ls = (C.c_void_p * n)(*[g.ctypes.data for g in gls])
    rs = (C.c_void_p * n)(*[g.ctypes.data for g in grs])
    lm = (C.c_void_p * n)(*[d.lDisMap.ctypes.data for d in des]) if download else None
    rm = (C.c_void_p * n)(*[d.rDisMap.ctypes.data for d in des]) if download else None
    if subsample_rate:
        capi.check(des[0]._lib.psm_gray_compute_fgf_batch(arr, n, ls, rs, gls[0].strides[0], depth, int(subsample_rate), lm, rm,
                                                          shape[1] if download else 0), des[0]._h, "gray_batch")
    else:
        capi.check(des[0]._lib.psm_gray_compute_batch(arr, n, ls, rs, gls[0].strides[0], depth, lm, rm, shape[1] if download else 0),
                   des[0]._h, "gray_batch")
    for d in des:
        d._gray_rate = int(subsample_rate)
    return [(d.lDisMap, d.rDisMap) if download else None for d in des]


def share_streams(des):
    """The DispEst objects of a batch run on one compute stream and one copy stream each way (psm_share_streams) - call once
    before a frame loop over batches."""
    des = list(des)
    if not des:
        return
    arr = (C.c_void_p * len(des))(*[d._h for d in des])
    capi.check(des[0]._lib.psm_share_streams(arr, len(des)), des[0]._h, "share_streams")


class FrameRing:
    """The reference's frame loop (src/main.cpp:64-73: one compute() per frame) with `frames` frames in the device's queues: F
    contexts of one geometry, each on its own stream, take the frames of a stream in turn.  While frame i runs, frame i + 1 is
    already queued behind it on another stream, so a frame's short kernels (image preparation, guidance, reduction, merge) and the
    half-empty last round of its fused launch run beside the next frame's fused kernel instead of alone.  Results are those of
    the single-context calls, bit for bit (every context is an ordinary DispEst).  Measured on MI355X (profiles/r05): -13 % per
    frame at 1280 x 720 x 128, -24 % at 450 x 375 x 64, nothing at 1920 x 1080 x 256 (there the fused launches fill the chip).

        ring = FrameRing(l0, r0, maxDis, frames=2)
        for l, r in stream:
            done = ring.push(l, r)          # maps of the frame pushed `frames` calls earlier (None while the ring fills)
        for lm, rm in ring.flush(): ...     # the frames still in flight, oldest first
    """

    def __init__(self, l, r, d: int, frames: int = 2, *, dtype: str = "f32", device: int = 0, lr_check: bool = False,
                 seg_rows: int = 0, truth=None, scale_factor: int = 4, error_threshold: int = 4, reproject: int = 0, wls=None):
        """Every context is told PSM_OPT_FRAMES_IN_FLIGHT = frames: the planner of the fused launches then cuts them for a shared
        device (450 x 375 x 64: 0.207 ms per frame against 0.22-0.23 without the hint; no result changes).  seg_rows > 0:
        PSM_OPT_SEG_ROWS of every context on top of that (round 5's first finding - one segment per launch, seg_rows = image height
        - is what the hint replaced: profiles/r05/exp_plan_model.txt).
        truth = (gt, mask or None): every frame's left map is scored against it on the device behind its last stage (Score_GPU,
        PSM_SCORE_GIF, with scale_factor / error_threshold); push / flush then return (lmap, rmap, score) instead of (lmap, rmap).
        reproject = outputs (capi.PSM_DEPTH_*): every frame's left map is reprojected on the device behind its last stage
        (Reproject_GPU, PSM_DEPTH_GIF; under lr_check with its mask) once setReprojection - or setRectification with a
        rectification that carries Q - has told the ring its Q; push / flush then return one more element: the cloud if the
        outputs name it alone, else the dict {"xyz", "z", "cloud"} of what they name.
        wls = a dict of DispEst.setWLS's parameters ({}: lam 8000, sigma 1.5, iterations 3): every frame's left map goes through the
        WLS smoothing on the device behind its last stage (WLS_GPU, PSM_WLS_GIF; under lr_check with its mask); push / flush then
        return one more element, the last: the filtered H x W int16 map in 16ths.  (The dict's key "confidence", WLS_GPU's option, is
        passed through with it - and refused by the library, whose confidence belongs to the SGM source.)"""
        if frames < 1:
            raise ValueError("FrameRing: frames must be >= 1")
        self.ctx = [DispEst(l, r, d, dtype=dtype, device=device) for _ in range(frames)]
        for c in self.ctx:
            c.set_option(capi.PSM_OPT_ASYNC, 1)
            c.set_option(capi.PSM_OPT_FRAMES_IN_FLIGHT, frames)      # the planner cuts the launches for `frames` pairs at a time
            if seg_rows > 0:
                c.set_option(capi.PSM_OPT_SEG_ROWS, int(seg_rows))
        self._n = 0
        self._busy = [False] * frames
        self._lrc = lr_check
        self._score = truth is not None
        self._depth = int(reproject)
        self._wls = wls is not None
        self._wls_conf = wls.get("confidence") if self._wls else None
        if self._wls:
            for c in self.ctx:
                c.setWLS(**{k: v for k, v in wls.items() if k != "confidence"})
        if self._score:
            for c in self.ctx:
                c.set_truth(truth[0], truth[1])
                c.set_score_params(scale_factor, error_threshold,
                                   capi.PSM_MASK_NONOCC if truth[1] is not None else capi.PSM_MASK_NONE)

    def setRectification(self, rect):
        """Every context of the ring rectifies the frames push_frame gives it (DispEst.setRectification)."""
        for c in self.ctx:
            c.setRectification(rect)

    def setReprojection(self, Q, crop=(0, 0), z_range=None):
        """Every context of the ring reprojects with this Q, crop and range (DispEst.setReprojection)."""
        for c in self.ctx:
            c.setReprojection(Q, crop, z_range)

    def push(self, l, r):
        return self._push(lambda c: c.setInputImages(l, r))

    def push_async(self, l, r):
        """push with the pair travelling on the context's copy stream (DispEst.setInputImages_async): the call returns once the
        images are in page-locked staging memory, and the frame's first kernel waits for the copy on the device."""
        return self._push(lambda c: c.setInputImages_async(l, r))

    def push_frame(self, vFrame):
        """push for a side-by-side camera frame: rectified and cropped on the device (DispEst.setInputFrame)."""
        return self._push(lambda c: c.setInputFrame(vFrame))

    def _push(self, set_input):
        i = self._n % len(self.ctx)
        self._n += 1
        c = self.ctx[i]
        out = None
        if self._busy[i]:
            out = self._collect(c)
        set_input(c)
        c.CostConst_GPU()
        c.CostFilter_GPU()
        c.DispSelect_device()
        if self._lrc:
            c.LRCheck_device()
        c.download_maps_async()
        if self._score:
            c.Score_GPU(capi.PSM_SCORE_GIF)      # (behind the download's start: the copy of the maps does not wait for the score)
        if self._depth:
            c.Reproject_GPU(capi.PSM_DEPTH_GIF, self._depth, use_mask=self._lrc)
        if self._wls:
            c.WLS_GPU(capi.PSM_WLS_GIF, use_mask=self._lrc, confidence=self._wls_conf)
        self._busy[i] = True
        return out

    def _collect(self, c):
        out = tuple(m.copy() for m in c.download_maps_wait())
        if self._score:
            out += (c.score_wait(),)
        if self._depth:
            c.reproject_wait()
            if self._depth == capi.PSM_DEPTH_CLOUD:
                out += (c.cloud(),)
            else:
                xyz, z = c.reprojected()
                out += ({"xyz": xyz, "z": z, "cloud": c.cloud() if self._depth & capi.PSM_DEPTH_CLOUD else None},)
        if self._wls:
            c.wls_wait()
            out += (c.wls_map(),)
        return out

    def flush(self):
        out = []
        F = len(self.ctx)
        for k in range(F):
            i = (self._n + k) % F
            if self._busy[i]:
                out.append(self._collect(self.ctx[i]))
                self._busy[i] = False
        return out

    def close(self):
        for c in self.ctx:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

