#include "hipUtil.h"

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>

namespace psm {
namespace {
void *g_handle = nullptr;
HipApi g_api;
std::string g_error;

template <typename F>
bool bind(F &fn, const char *name)
{
    fn = reinterpret_cast<F>(dlsym(g_handle, name));
    if (!fn) {
        g_error = std::string("hipUtil: symbol ") + name + " missing from libprimesm_hip.so";
        return false;
    }
    return true;
}
}  // namespace

bool hipUtil::load(const char *path)
{
    if (g_handle) return true;
    const char *cands[3] = {path, std::getenv("PRIMESM_HIP_LIB"), "libprimesm_hip.so"};
    for (const char *c : cands) {
        if (!c || !*c) continue;
        g_handle = dlopen(c, RTLD_NOW | RTLD_LOCAL);
        if (g_handle) break;
        g_error = std::string("hipUtil: dlopen(") + c + ") failed: " + dlerror();
    }
    if (!g_handle) {
        fprintf(stderr, "%s\n", g_error.c_str());
        return false;
    }
    bool ok = bind(g_api.device_count, "psm_device_count") && bind(g_api.create_shard, "psm_create_shard") &&
              bind(g_api.destroy, "psm_destroy") && bind(g_api.last_error, "psm_last_error") &&
              bind(g_api.set_option, "psm_set_option") && bind(g_api.upload_pair, "psm_upload_pair") &&
              bind(g_api.upload_pair_async, "psm_upload_pair_async") && bind(g_api.download_maps_async, "psm_download_maps_async") &&
              bind(g_api.download_maps_wait, "psm_download_maps_wait") &&
              bind(g_api.cost_construct, "psm_cost_construct") && bind(g_api.cost_filter, "psm_cost_filter") &&
              bind(g_api.cost_filter_fgf, "psm_cost_filter_fgf") &&
              bind(g_api.disp_select, "psm_disp_select") && bind(g_api.disp_select_partial, "psm_disp_select_partial") &&
              bind(g_api.disp_merge_ctx, "psm_disp_merge_ctx") && bind(g_api.set_rows, "psm_set_rows") && bind(g_api.gather_rows_ctx, "psm_gather_rows_ctx") &&
              bind(g_api.lr_check, "psm_lr_check") && bind(g_api.fill_invalid, "psm_fill_invalid") &&
              bind(g_api.wgt_median, "psm_wgt_median") && bind(g_api.joint_wmf, "psm_joint_wmf") &&
              bind(g_api.joint_wmf_set_clusters, "psm_joint_wmf_set_clusters") &&
              bind(g_api.stage_time_us, "psm_stage_time_us") && bind(g_api.compute_batch, "psm_compute_batch") &&
              bind(g_api.download_maps, "psm_download_maps") && bind(g_api.rectify_build_maps, "psm_rectify_build_maps") &&
              bind(g_api.rectify_set_maps, "psm_rectify_set_maps") && bind(g_api.rectify_clear, "psm_rectify_clear") &&
              bind(g_api.upload_pair_rectified, "psm_upload_pair_rectified") &&
              bind(g_api.upload_pair_rectified_async, "psm_upload_pair_rectified_async") && bind(g_api.download_images, "psm_download_images") &&
              bind(g_api.sgm_set_params, "psm_sgm_set_params") && bind(g_api.sgm_compute, "psm_sgm_compute") &&
              bind(g_api.sgm_compute_gray, "psm_sgm_compute_gray") && bind(g_api.sgm_download_disparity, "psm_sgm_download_disparity") &&
              bind(g_api.sgm_times, "psm_sgm_times") && bind(g_api.sgm_set_speckle, "psm_sgm_set_speckle") &&
              bind(g_api.sgm_filter_speckles, "psm_sgm_filter_speckles") &&
              bind(g_api.sgm_download_speckle_sizes, "psm_sgm_download_speckle_sizes") && bind(g_api.sgm_speckle_time, "psm_sgm_speckle_time") &&
              bind(g_api.sgm_set_prefilter, "psm_sgm_set_prefilter") && bind(g_api.sgm_compute_batch, "psm_sgm_compute_batch") &&
              bind(g_api.sgm_set_mode, "psm_sgm_set_mode") && bind(g_api.sgm_set_range, "psm_sgm_set_range") &&
              bind(g_api.sgm_set_census, "psm_sgm_set_census") && bind(g_api.sgm_select_maps, "psm_sgm_select_maps") &&
              bind(g_api.sgm_select_maps_batch, "psm_sgm_select_maps_batch") && bind(g_api.sgm_maps_time, "psm_sgm_maps_time") &&
              bind(g_api.joint_wmf_batch, "psm_joint_wmf_batch") && bind(g_api.post_process_batch, "psm_post_process_batch") &&
              bind(g_api.download_valid, "psm_download_valid") && bind(g_api.score_set_truth, "psm_score_set_truth") &&
              bind(g_api.score_set_params, "psm_score_set_params") && bind(g_api.score, "psm_score") &&
              bind(g_api.score_download, "psm_score_download") && bind(g_api.reproject_set_q, "psm_reproject_set_q") &&
              bind(g_api.reproject_set_range, "psm_reproject_set_range") && bind(g_api.reproject, "psm_reproject") &&
              bind(g_api.reproject_download, "psm_reproject_download") && bind(g_api.reproject_download_cloud, "psm_reproject_download_cloud") &&
              bind(g_api.wls_set_params, "psm_wls_set_params") && bind(g_api.wls_filter, "psm_wls_filter") && bind(g_api.wls_wait, "psm_wls_wait") &&
              bind(g_api.wls_download, "psm_wls_download") && bind(g_api.wls_time, "psm_wls_time") && bind(g_api.wls_publish, "psm_wls_publish") &&
              bind(g_api.wls_set_confidence, "psm_wls_set_confidence") && bind(g_api.wls_download_confidence, "psm_wls_download_confidence") &&
              bind(g_api.wls_conf_time, "psm_wls_conf_time") &&
              bind(g_api.wls_filter_batch, "psm_wls_filter_batch") && bind(g_api.gray_compute, "psm_gray_compute") &&
              bind(g_api.gray_compute_batch, "psm_gray_compute_batch") && bind(g_api.gray_time, "psm_gray_time") &&
              bind(g_api.gray_compute_fgf, "psm_gray_compute_fgf") && bind(g_api.gray_compute_fgf_batch, "psm_gray_compute_fgf_batch");
    if (!ok) {
        fprintf(stderr, "%s\n", g_error.c_str());
        dlclose(g_handle);
        g_handle = nullptr;
    }
    return ok;
}

bool hipUtil::loaded() { return g_handle != nullptr; }
const HipApi &hipUtil::api() { return g_api; }
const std::string &hipUtil::error() { return g_error; }

int hipUtil::hipDevicePoll()
{
    if (!load()) return 0;
    return g_api.device_count();
}

}  // namespace psm
