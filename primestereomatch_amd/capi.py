"""ctypes loader for libprimesm_hip.so - the C ABI declared in include/primesm_hip.h.

This is the Python-side "hipUtil": it dlopen()s the HIP library at run time the way the
reference's oclUtil JIT-loads its .cl files (src/oclUtil.cpp:438-496).  There is NO CPU
fallback: if the library is missing or no GPU is present the calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libprimesm_hip.so")

# enums of include/primesm_hip.h
PSM_F32, PSM_U8 = 0, 1
PSM_IMG_U8, PSM_IMG_F32 = 0, 1
PSM_LEFT, PSM_RIGHT = 0, 1
PSM_STAGE_CVC, PSM_STAGE_CVF, PSM_STAGE_DISPSEL, PSM_STAGE_PP = 0, 1, 2, 3
(PSM_K_PREP, PSM_K_CVC, PSM_K_GUIDE, PSM_K_CVF_A, PSM_K_CVF_B, PSM_K_WTA, PSM_K_MERGE, PSM_K_BOX,
 PSM_K_LRC, PSM_K_CVF_F, PSM_K_FGF, PSM_K_WMF, PSM_K_JWMF) = range(13)
(PSM_OPT_ASYNC, PSM_OPT_KERNEL_VARIANT, PSM_OPT_PROFILE, PSM_OPT_SEG_ROWS, PSM_OPT_WAVES, PSM_OPT_FLAGS, PSM_OPT_GRAPH,
 PSM_OPT_GATHER_STAGED, PSM_OPT_FRAMES_IN_FLIGHT) = range(9)
# enum psm_flag (PSM_OPT_FLAGS bits)
PSM_FLAG_MATERIALISE_COSTS, PSM_FLAG_FGF_STORE, PSM_FLAG_STORE_FILTERED = 128, 4096, 8192
PSM_FLAG_TWO_PHASE_ON, PSM_FLAG_TWO_PHASE_OFF = 1048576, 2097152
PSM_FLAG_WMF_DATAFLOW, PSM_FLAG_WMF_TWO_SWEEPS, PSM_FLAG_WMF_NO_CACHE = 4194304, 8388608, 16777216
PSM_FLAG_F32_TOL = 33554432
# psm_post_process_batch: the stages
PSM_PP_LR_CHECK, PSM_PP_FILL, PSM_PP_WGT_MEDIAN = 1, 2, 4
PSM_FLAG_FMA_SOLVE = 67108864
# the score stage: sources, mask modes (include/StereoMatch.h), record flags
PSM_SCORE_GIF, PSM_SCORE_SGM, PSM_SCORE_SGM_INT = 0, 1, 2
PSM_MASK_NONE, PSM_MASK_NONOCC, PSM_MASK_DISC = 0, 1, 2
PSM_SCORE_FLAT = 1
# the reprojection stage: sources, outputs, flags
PSM_DEPTH_GIF, PSM_DEPTH_SGM = 0, 1
PSM_DEPTH_XYZ, PSM_DEPTH_Z, PSM_DEPTH_CLOUD = 1, 2, 4
PSM_DEPTH_USE_MASK = 1
PSM_DEPTH_VOID = 0x7FC00000          # the bit pattern of a void pixel in the dense planes
# the WLS smoothing stage: sources, flags
PSM_WLS_GIF, PSM_WLS_SGM = 0, 1
PSM_WLS_USE_MASK, PSM_WLS_CONFIDENCE = 1, 2
PSM_WLS_CONF_LR, PSM_WLS_CONF_VAR = 1, 2   # the terms of the graded confidence (psm_wls_set_confidence)
PSM_WLS_VOID = 0x7FC00000            # the bit pattern of a void pixel in the float plane


class Score(C.Structure):
    """struct psm_score: the integers of the error record; the two figures are derived from them in double."""
    _fields_ = [("min_val", C.c_int32), ("max_val", C.c_int32), ("pixels", C.c_uint32), ("bad", C.c_uint32),
                ("err_sum", C.c_uint64), ("unit", C.c_int32), ("flags", C.c_uint32)]

    def as_dict(self):
        d = {name: int(getattr(self, name)) for name, _ in self._fields_}
        d["bp_percent"] = 100.0 * d["bad"] / d["pixels"]
        d["avg_err"] = (d["err_sum"] / d["pixels"]) / d["unit"] if d["unit"] else 0.0
        return d


def point_dtype():
    """The 16-byte record of the point cloud (psm_reproject_download_cloud): float x, y, z; uint8 b, g, r, a (a = 255)."""
    import numpy as np
    return np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])


class Point(C.Structure):
    """The same record for ctypes callers."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("b", C.c_uint8), ("g", C.c_uint8), ("r", C.c_uint8),
                ("a", C.c_uint8)]


# every symbol include/primesm_hip.h declares: (name, restype, argtypes)
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
_pi, _pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
_pu = C.POINTER(C.c_uint32)
SYMBOLS = [
    ("psm_device_count", _i, []),
    ("psm_create", _i, [C.POINTER(_vp), _i, _i, _i, _i, _i]),
    ("psm_create_shard", _i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i, _i]),
    ("psm_create_shard_strided", _i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i, _i]),
    ("psm_destroy", None, [_vp]),
    ("psm_last_error", C.c_char_p, [_vp]),
    ("psm_set_option", _i, [_vp, _i, _i]),
    ("psm_set_stream", _i, [_vp, _vp]),
    ("psm_synchronize", _i, [_vp]),
    ("psm_release_scratch", _i, [_vp]),
    ("psm_upload_pair", _i, [_vp, _vp, _vp, _i, _sz, _i]),
    ("psm_upload_pair_async", _i, [_vp, _vp, _vp, _i, _sz, _i]),
    ("psm_cost_construct", _i, [_vp]),
    ("psm_cost_filter", _i, [_vp]),
    ("psm_cost_filter_side", _i, [_vp, _i]),
    ("psm_cost_filter_fgf", _i, [_vp, _i]),
    ("psm_disp_select", _i, [_vp, _vp, _vp, _sz]),
    ("psm_disp_select_partial_side", _i, [_vp, _i, _vp]),
    ("psm_disp_select_partial", _i, [_vp, _vp]),
    ("psm_set_key_buffer", _i, [_vp, _vp]),
    ("psm_partial_keys", _i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    ("psm_disp_merge", _i, [_vp, _vp, _i, _vp, _vp, _sz]),
    ("psm_disp_merge_ctx", _i, [_vp, C.POINTER(_vp), _i, _vp, _vp, _sz]),
    ("psm_compute_batch", _i, [C.POINTER(_vp), _i]),
    ("psm_share_streams", _i, [C.POINTER(_vp), _i]),
    ("psm_download_maps", _i, [_vp, _vp, _vp, _sz]),
    ("psm_download_maps_async", _i, [_vp]),
    ("psm_download_maps_wait", _i, [_vp, _vp, _vp, _sz]),
    ("psm_lr_check", _i, [_vp, _vp, _vp, _sz]),
    ("psm_fill_invalid", _i, [_vp, _vp, _vp, _sz]),
    ("psm_wgt_median", _i, [_vp, _vp, _vp, _sz]),
    ("psm_wgt_median_stats", _i, [_vp, _vp, _vp]),
    ("psm_post_process_batch", _i, [C.POINTER(_vp), _i, _i]),
    ("psm_download_valid", _i, [_vp, _vp, _vp, _sz]),
    ("psm_joint_wmf", _i, [_vp, _i, C.c_float, _i, _i, _vp, _vp, _sz]),
    ("psm_joint_wmf_set_clusters", _i, [_vp, _i, _i, _vp, _vp]),
    ("psm_joint_wmf_clusters", _i, [_vp, _i, _pi, _vp, _vp, _pi]),
    ("psm_joint_wmf_batch", _i, [C.POINTER(_vp), _i, _i, C.c_float, _i, _i]),
    ("psm_set_rows", _i, [_vp, _i, _i]),
    ("psm_set_map_buffer", _i, [_vp, _vp, _i]),
    ("psm_gather_rows_ctx", _i, [_vp, _vp, _i, _vp, _vp, _sz]),
    ("psm_gather_staged_legs", _i, [_vp]),
    ("psm_upload_maps", _i, [_vp, _vp, _vp, _vp, _vp, _sz]),
    ("psm_download_volume", _i, [_vp, _i, _i, _i, _vp]),
    ("psm_upload_volume", _i, [_vp, _i, _i, _i, _vp]),
    ("psm_filter_stage_a", _i, [_vp, _i]),
    ("psm_download_ab", _i, [_vp, _i, _i, _vp]),
    ("psm_download_guidance", _i, [_vp, _i, _vp]),
    ("psm_box8_volume", _i, [_vp, _i, _vp]),
    ("psm_stage_time_us", _i, [_vp, _i, _pd]),
    ("psm_kernel_time_ms", _i, [_vp, _i, _pd, _pi]),
    ("psm_reset_kernel_times", _i, [_vp]),
    ("psm_filter_launch_times", _i, [_vp, _pd, _pi, _i, _pi]),
    ("psm_get_info", _i, [_vp, _pi, _pi, _pi, _pi, _pi, _pi, _pi]),
    ("psm_rectify_build_maps", _i, [_pd, _pd, _i, _pd, _pd, _i, _i, _vp, _vp]),
    ("psm_rectify_set_maps", _i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    ("psm_rectify_clear", _i, [_vp]),
    ("psm_upload_pair_rectified", _i, [_vp, _vp, _vp, _i, _sz]),
    ("psm_upload_pair_rectified_async", _i, [_vp, _vp, _vp, _i, _sz]),
    ("psm_download_images", _i, [_vp, _vp, _vp, _sz]),
    ("psm_sgm_set_params", _i, [_vp, _i, _i, _i, _i, _i]),
    ("psm_sgm_compute", _i, [_vp]),
    ("psm_sgm_compute_gray", _i, [_vp, _vp, _vp, _sz]),
    ("psm_sgm_download_disparity", _i, [_vp, _vp, _sz]),
    ("psm_sgm_download_costs", _i, [_vp, _i, _vp]),
    ("psm_sgm_times", _i, [_vp, _pd]),
    ("psm_sgm_set_speckle", _i, [_vp, _i, _i]),
    ("psm_sgm_filter_speckles", _i, [_vp, _vp, _sz, _i, _i, _i]),
    ("psm_sgm_download_speckle_sizes", _i, [_vp, _vp, _sz]),
    ("psm_sgm_speckle_time", _i, [_vp, _pd]),
    ("psm_sgm_set_prefilter", _i, [_vp, _i]),
    ("psm_sgm_download_prefiltered", _i, [_vp, _i, _vp]),
    ("psm_sgm_compute_batch", _i, [C.POINTER(_vp), _i]),
    ("psm_sgm_set_mode", _i, [_vp, _i]),
    ("psm_sgm_set_range", _i, [_vp, _i, _i]),
    ("psm_sgm_set_census", _i, [_vp, _i, _i]),
    ("psm_sgm_download_census", _i, [_vp, _i, _vp]),
    ("psm_sgm_select_maps", _i, [_vp, _vp, _vp, _sz]),
    ("psm_sgm_select_maps_batch", _i, [C.POINTER(_vp), _i]),
    ("psm_sgm_maps_time", _i, [_vp, _pd]),
    ("psm_score_set_truth", _i, [_vp, _vp, _vp, _sz]),
    ("psm_score_clear_truth", _i, [_vp]),
    ("psm_score_set_params", _i, [_vp, _i, _i, _i]),
    ("psm_score", _i, [_vp, _i, C.POINTER(Score)]),
    ("psm_score_wait", _i, [_vp, C.POINTER(Score)]),
    ("psm_score_download", _i, [_vp, _vp, _vp, _vp, _sz]),
    ("psm_score_batch", _i, [C.POINTER(_vp), _i, _i, C.POINTER(Score)]),
    ("psm_score_time", _i, [_vp, _pd]),
    ("psm_score_upload_sgm_map", _i, [_vp, _vp, _sz]),
    ("psm_reproject_set_q", _i, [_vp, _pd, _i, _i]),
    ("psm_reproject_set_range", _i, [_vp, C.c_float, C.c_float]),
    ("psm_reproject", _i, [_vp, _i, _i, _i, _pu]),
    ("psm_reproject_wait", _i, [_vp, _pu]),
    ("psm_reproject_download", _i, [_vp, _vp, _vp, _sz]),
    ("psm_reproject_download_cloud", _i, [_vp, _vp, C.c_uint32, _pu]),
    ("psm_reproject_batch", _i, [C.POINTER(_vp), _i, _i, _i, _i, _pu]),
    ("psm_reproject_time", _i, [_vp, _pd]),
    ("psm_wls_set_params", _i, [_vp, C.c_float, C.c_float, _i]),
    ("psm_wls_filter", _i, [_vp, _i, _i]),
    ("psm_wls_filter_batch", _i, [C.POINTER(_vp), _i, _i, _i]),
    ("psm_wls_wait", _i, [_vp]),
    ("psm_wls_download", _i, [_vp, _vp, _vp, _vp, _vp, _sz]),
    ("psm_wls_download_table", _i, [_vp, _vp]),
    ("psm_wls_time", _i, [_vp, _pd]),
    ("psm_wls_publish", _i, [_vp, _i]),
    ("psm_wls_set_confidence", _i, [_vp, _i, _i, _i, _i]),
    ("psm_wls_download_confidence", _i, [_vp, _vp, _sz, _vp, _sz]),
    ("psm_wls_conf_time", _i, [_vp, _pd]),
    ("psm_gray_compute", _i, [_vp, _vp, _vp, _sz, _i, _vp, _vp, _sz]),
    ("psm_gray_compute_batch", _i, [C.POINTER(_vp), _i, C.POINTER(_vp), C.POINTER(_vp), _sz, _i, C.POINTER(_vp), C.POINTER(_vp), _sz]),
    ("psm_gray_compute_fgf", _i, [_vp, _vp, _vp, _sz, _i, _i, _vp, _vp, _sz]),
    ("psm_gray_compute_fgf_batch", _i, [C.POINTER(_vp), _i, C.POINTER(_vp), C.POINTER(_vp), _sz, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _sz]),
    ("psm_gray_fgf_guidance", _i, [_vp, _i, _vp]),
    ("psm_gray_fgf_volume", _i, [_vp, _i, _i, _i, _vp, _vp]),
    ("psm_gray_time", _i, [_vp, _pd]),
    ("psm_gray_guidance", _i, [_vp, _i, _vp]),
    ("psm_gray_volume", _i, [_vp, _i, _i, _i, _vp, _vp]),
]

_lib = None


class PsmError(RuntimeError):
    """A C-ABI call returned non-zero (the reference's `_cl` methods return 1 on failure)."""


def load(path: str | None = None):
    """dlopen the HIP library and bind every declared symbol.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("PRIMESM_HIP_LIB") or LIB_PATH   # same override as the C++ hipUtil
    if not os.path.exists(p):
        raise PsmError(
            f"{p} not found: build it with `make -C primestereomatch_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(p)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    if path is None:
        _lib = lib
    return lib


def device_count() -> int:
    return int(load().psm_device_count())


def last_error(handle=None) -> str:
    s = load().psm_last_error(handle)
    return s.decode("utf-8", "replace") if s else ""


def check(rc: int, handle=None, what: str = ""):
    if rc != 0:
        raise PsmError(f"{what or 'psm call'} failed: {last_error(handle)}")
