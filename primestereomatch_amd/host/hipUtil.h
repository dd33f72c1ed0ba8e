// hipUtil.h - run-time loader of libprimesm_hip.so.  Takes the place of the reference's oclUtil
// (include/oclUtil.h:47-152, src/oclUtil.cpp): where oclUtil polls OpenCL devices, creates the
// context/queue and JIT-builds the .cl programs, hipUtil dlopen()s the prebuilt HIP library and
// binds the C ABI of include/primesm_hip.h, so the host program has no link-time HIP dependency.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/primesm_hip.h"

namespace psm {

struct HipApi {
    // one pointer per entry point of include/primesm_hip.h that the DispEst mirror uses
    int (*device_count)(void) = nullptr;
    int (*create_shard)(psm_ctx **, int, int, int, int, int, int, int) = nullptr;
    void (*destroy)(psm_ctx *) = nullptr;
    const char *(*last_error)(const psm_ctx *) = nullptr;
    int (*set_option)(psm_ctx *, int, int) = nullptr;
    int (*upload_pair)(psm_ctx *, const void *, const void *, int, size_t, int) = nullptr;
    int (*upload_pair_async)(psm_ctx *, const void *, const void *, int, size_t, int) = nullptr;
    int (*download_maps_async)(psm_ctx *) = nullptr;
    int (*download_maps_wait)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*cost_construct)(psm_ctx *) = nullptr;
    int (*cost_filter)(psm_ctx *) = nullptr;
    int (*cost_filter_fgf)(psm_ctx *, int) = nullptr;
    int (*disp_select)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*disp_select_partial)(psm_ctx *, void *) = nullptr;
    int (*disp_merge_ctx)(psm_ctx *, psm_ctx *const *, int, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*set_rows)(psm_ctx *, int, int) = nullptr;
    int (*gather_rows_ctx)(psm_ctx *, psm_ctx *const *, int, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*lr_check)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*fill_invalid)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*wgt_median)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*joint_wmf)(psm_ctx *, int, float, int, int, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*joint_wmf_set_clusters)(psm_ctx *, int, int, const float *, const uint8_t *) = nullptr;
    int (*stage_time_us)(psm_ctx *, int, double *) = nullptr;
    int (*compute_batch)(psm_ctx *const *, int) = nullptr;
    int (*download_maps)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    // video mode: rectification on the device
    int (*rectify_build_maps)(const double *, const double *, int, const double *, const double *, int, int, int16_t *, uint16_t *) = nullptr;
    int (*rectify_set_maps)(psm_ctx *, int, const int16_t *, const uint16_t *, int, int, int, int, int, int) = nullptr;
    int (*rectify_clear)(psm_ctx *) = nullptr;
    int (*upload_pair_rectified)(psm_ctx *, const void *, const void *, int, size_t) = nullptr;
    int (*upload_pair_rectified_async)(psm_ctx *, const void *, const void *, int, size_t) = nullptr;
    int (*download_images)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    // the second algorithm: semi-global matching
    int (*sgm_set_params)(psm_ctx *, int, int, int, int, int) = nullptr;
    int (*sgm_compute)(psm_ctx *) = nullptr;
    int (*sgm_compute_gray)(psm_ctx *, const uint8_t *, const uint8_t *, size_t) = nullptr;
    int (*sgm_download_disparity)(psm_ctx *, int16_t *, size_t) = nullptr;
    int (*sgm_times)(psm_ctx *, double *) = nullptr;
    int (*sgm_set_speckle)(psm_ctx *, int, int) = nullptr;
    int (*sgm_filter_speckles)(psm_ctx *, int16_t *, size_t, int, int, int) = nullptr;
    int (*sgm_download_speckle_sizes)(psm_ctx *, int32_t *, size_t) = nullptr;
    int (*sgm_speckle_time)(psm_ctx *, double *) = nullptr;
    int (*sgm_set_prefilter)(psm_ctx *, int) = nullptr;
    int (*sgm_compute_batch)(psm_ctx *const *, int) = nullptr;
    int (*sgm_set_mode)(psm_ctx *, int) = nullptr;
    int (*sgm_set_range)(psm_ctx *, int, int) = nullptr;
    int (*sgm_set_census)(psm_ctx *, int, int) = nullptr;
    int (*sgm_select_maps)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*sgm_select_maps_batch)(psm_ctx *const *, int) = nullptr;
    int (*sgm_maps_time)(psm_ctx *, double *) = nullptr;
    int (*joint_wmf_batch)(psm_ctx *const *, int, int, float, int, int) = nullptr;
    int (*post_process_batch)(psm_ctx *const *, int, int) = nullptr;
    int (*download_valid)(psm_ctx *, uint8_t *, uint8_t *, size_t) = nullptr;
    // score: display maps and the error metric against ground truth
    int (*score_set_truth)(psm_ctx *, const uint8_t *, const uint8_t *, size_t) = nullptr;
    int (*score_set_params)(psm_ctx *, int, int, int) = nullptr;
    int (*score)(psm_ctx *, int, struct psm_score *) = nullptr;
    int (*score_download)(psm_ctx *, uint8_t *, uint8_t *, uint8_t *, size_t) = nullptr;
    // reproject: from disparity to depth, the point cloud
    int (*reproject_set_q)(psm_ctx *, const double *, int, int) = nullptr;
    int (*reproject_set_range)(psm_ctx *, float, float) = nullptr;
    int (*reproject)(psm_ctx *, int, int, int, uint32_t *) = nullptr;
    int (*reproject_download)(psm_ctx *, float *, float *, size_t) = nullptr;
    int (*reproject_download_cloud)(psm_ctx *, void *, uint32_t, uint32_t *) = nullptr;
    // WLS smoothing of the sub-pixel map
    int (*wls_set_params)(psm_ctx *, float, float, int) = nullptr;
    int (*wls_filter)(psm_ctx *, int, int) = nullptr;
    int (*wls_filter_batch)(psm_ctx *const *, int, int, int) = nullptr;
    int (*wls_wait)(psm_ctx *) = nullptr;
    int (*wls_download)(psm_ctx *, int16_t *, float *, float *, float *, size_t) = nullptr;
    int (*wls_time)(psm_ctx *, double *) = nullptr;
    int (*wls_publish)(psm_ctx *, int) = nullptr;
    int (*wls_set_confidence)(psm_ctx *, int, int, int, int) = nullptr;
    int (*wls_download_confidence)(psm_ctx *, uint8_t *, size_t, int16_t *, size_t) = nullptr;
    int (*wls_conf_time)(psm_ctx *, double *) = nullptr;
    // the guided-filter path over a one-channel pair
    int (*gray_compute)(psm_ctx *, const void *, const void *, size_t, int, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*gray_compute_batch)(psm_ctx *const *, int, const void *const *, const void *const *, size_t, int, uint8_t *const *, uint8_t *const *,
                              size_t) = nullptr;
    int (*gray_time)(psm_ctx *, double *) = nullptr;
    int (*gray_compute_fgf)(psm_ctx *, const void *, const void *, size_t, int, int, uint8_t *, uint8_t *, size_t) = nullptr;
    int (*gray_compute_fgf_batch)(psm_ctx *const *, int, const void *const *, const void *const *, size_t, int, int, uint8_t *const *,
                                  uint8_t *const *, size_t) = nullptr;
};

class hipUtil {
public:
    // Loads the library once per process.  path == nullptr: $PRIMESM_HIP_LIB, then
    // libprimesm_hip.so next to the executable's ../lib, then the dynamic linker's search path.
    // Returns false (and keeps error()) if the library or a symbol is missing.
    static bool load(const char *path = nullptr);
    static bool loaded();
    static const HipApi &api();
    static const std::string &error();
    // Replaces openCLdevicepoll() (src/oclUtil.cpp:18-135): number of usable devices, 0 if the
    // library cannot be loaded or no GPU is present.
    static int hipDevicePoll();
};

}  // namespace psm
