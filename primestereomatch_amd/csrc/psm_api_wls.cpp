// psm_api_wls.cpp - psm_wls_filter: edge-aware WLS smoothing of a sub-pixel disparity map behind the C ABI - the confidence-weighted
// global smoothing users of cv::StereoSGBM apply at this point (cv::ximgproc::DisparityWLSFilter), by Min et al.'s Fast Global
// Smoother: it fills the holes of the int16 map from their surroundings, keeps depth edges on image edges and keeps the sixteenths.
// Kernels: psm_wls.hip.  The definition is tests/wls_model.py / DESIGN.md 13.  An independent stage, as psm_score and psm_reproject
// are: it reads the context's current result - the int16 map of the SGM stage (or the hook plane), or the left 8-bit map and its
// mask through psm::Results - and the left image of the pair, and writes its own planes (psm::WlsState).  psm_wls_publish lets the
// SGM sources of psm_score and psm_reproject read its result instead of the SGM stage's.
#include "psm_ctx.h"
#include "psm_wls_tab.h"

#include <cmath>

using namespace psm;

namespace psm {

void wls_free(psm_ctx *c)
{
    WlsState &w = c->wls;
    (void)hipFree(w.work); w.work = nullptr;
    (void)hipFree(w.links); w.links = nullptr;
    (void)hipFree(w.out); w.out = nullptr;
    (void)hipFree(w.q); w.q = nullptr;
    (void)hipFree(w.tab); w.tab = nullptr;
    w.tab_sigma = 0.0f;
    for (hipEvent_t *e : {&w.ev_done, &w.ev[0], &w.ev[1]}) {
        if (*e) (void)hipEventDestroy(*e);
        *e = nullptr;
    }
    w.have = w.pending = w.timed = w.publish = false;
}

}  // namespace psm

namespace {

constexpr int WLS_FLAGS_ALL = PSM_WLS_USE_MASK;

// what psm_wls_filter refuses about the call's own arguments (no context needed) ...
int check_call(psm_ctx *e, const char *who, int source, int flags)
{
    if (source != PSM_WLS_GIF && source != PSM_WLS_SGM) return fail(e, "%s: source %d not in {0: PSM_WLS_GIF, 1: PSM_WLS_SGM}", who, source);
    if (flags & ~WLS_FLAGS_ALL) return fail(e, "%s: unknown flag bits 0x%x", who, flags & ~WLS_FLAGS_ALL);
    if ((flags & PSM_WLS_USE_MASK) && source != PSM_WLS_GIF)
        return fail(e, "%s: PSM_WLS_USE_MASK with the SGM source (the L-R mask belongs to the 8-bit maps)", who);
    return 0;
}

// ... and about the context
int check_ctx(psm_ctx *c, const char *who, int source, int flags)
{
    if (source == PSM_WLS_GIF) {
        if (!c->res.maps) return fail(c, "%s: no disparity maps computed (PSM_WLS_GIF)", who);
        if (stripe_only(c)) return fail(c, "%s: the maps hold this context's row stripe only (gather the stripes first)", who);
        if ((flags & PSM_WLS_USE_MASK) && !c->res.mask) return fail(c, "%s: PSM_WLS_USE_MASK without a current L-R mask (psm_lr_check)", who);
    } else if (!sgm_stage_exists(c)) {
        return fail(c, "%s: no SGM result (psm_sgm_compute) for the SGM source", who);
    }
    if (!colour_of(c, source == PSM_WLS_SGM).img)
        return fail(c, "%s: no current image pair (psm_upload_pair: the left image guides the smoothing)", who);
    return 0;
}

int ensure_buffers(psm_ctx *c)
{
    WlsState &w = c->wls;
    const size_t HW = (size_t)c->W * c->H;
    if (!w.work) PSM_HIP(c, hipMalloc((void **)&w.work, 5 * HW * sizeof(float)));
    if (!w.links) PSM_HIP(c, hipMalloc((void **)&w.links, 2 * HW));
    if (!w.out) PSM_HIP(c, hipMalloc((void **)&w.out, HW * sizeof(int16_t)));
    if (!w.q) PSM_HIP(c, hipMalloc((void **)&w.q, HW * sizeof(unsigned)));
    if (!w.tab) PSM_HIP(c, hipMalloc((void **)&w.tab, WLS_TAB * sizeof(float)));
    if (!w.ev_done) PSM_HIP(c, hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
    if (c->opt_profile)
        for (hipEvent_t &e : w.ev)
            if (!e) PSM_HIP(c, hipEventCreate(&e));
    return 0;
}

WlsArgs wls_args(const psm_ctx *c, int source, int flags)
{
    const WlsState &w = c->wls;
    const size_t HW = (size_t)c->W * c->H;
    const Colour col = colour_of(c, source == PSM_WLS_SGM);
    WlsArgs a = {};
    a.map = c->maps;
    a.valid = (flags & PSM_WLS_USE_MASK) ? c->valid : nullptr;
    a.d16 = sgm_stage_map(c);
    a.img = col.img;
    a.num = w.work; a.den = w.work + HW;
    a.cp = w.work + 2 * HW; a.np = w.work + 3 * HW; a.dp = w.work + 4 * HW;
    a.kh = w.links; a.kv = w.links + HW;
    a.tab = w.tab;
    a.out = w.out;
    a.q = w.q;
    a.W = c->W; a.H = c->H; a.source = source;
    a.invalid = source == PSM_WLS_GIF ? -16 : sgm_stage_invalid(c);
    a.depth = col.depth; a.ch = col.ch;
    return a;
}

// the planes of the last run, complete: an asynchronous run is waited for on the way
int result_ready(psm_ctx *c, const char *who)
{
    if (!c->wls.have) return fail(c, "%s: no psm_wls_filter ran (or its planes were released)", who);
    if (bind(c)) return 1;
    PSM_HIP(c, hipEventSynchronize(c->wls.ev_done));
    return 0;
}

}  // namespace

extern "C" {

int psm_wls_set_params(psm_ctx *c, float lambda, float sigma, int iterations)
{
    if (!std::isfinite(lambda) || !(lambda > 0.0f)) return fail(c, "psm_wls_set_params: lambda %g is not a finite positive number", (double)lambda);
    if (!std::isfinite(sigma) || !(sigma > 0.0f)) return fail(c, "psm_wls_set_params: sigma %g is not a finite positive number", (double)sigma);
    if (iterations < 1 || iterations > WLS_MAX_ITERS) return fail(c, "psm_wls_set_params: iterations %d outside [1, %d]", iterations, WLS_MAX_ITERS);
    if (!c) return fail(nullptr, "psm_wls_set_params: NULL context");
    c->wls.lambda = lambda;
    c->wls.sigma = sigma;
    c->wls.iters = iterations;
    return 0;
}

int psm_wls_filter(psm_ctx *c, int source, int flags)
{
    const char *who = "psm_wls_filter";
    if (check_call(c, who, source, flags)) return 1;
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_ctx(c, who, source, flags)) return 1;
    if (bind(c)) return 1;
    if (ensure_buffers(c)) return 1;
    WlsState &w = c->wls;
    if (w.tab_sigma != w.sigma) {
        // (the copy out of tab_host of an earlier run has executed: a pageable source is staged before the call returns)
        wls_table(w.sigma, w.tab_host);
        w.tab_sigma = 0.0f;
        PSM_HIP(c, hipMemcpyAsync(w.tab, w.tab_host, sizeof w.tab_host, hipMemcpyHostToDevice, c->stream));
        w.tab_sigma = w.sigma;
    }
    const bool timed = c->opt_profile != 0;
    const WlsArgs a = wls_args(c, source, flags);
    w.have = w.pending = w.timed = false;       // (every check and allocation lies before this: the planes are about to be rewritten)
    if (timed) PSM_HIP(c, hipEventRecord(w.ev[0], c->stream));
    launch_wls_init(c->stream, a);
    for (int t = 0; t < w.iters; ++t) {
        const float lam = wls_lambda(w.lambda, w.iters, t);
        launch_wls_rows(c->stream, a, lam);
        launch_wls_cols(c->stream, a, lam, t == w.iters - 1);
    }
    if (check_launch(c, "k_wls_init, k_wls_rows, k_wls_cols")) return 1;
    if (timed) PSM_HIP(c, hipEventRecord(w.ev[1], c->stream));
    if (colour_of(c, source == PSM_WLS_SGM).slots && images_read(c, c->stream)) return 1;      // k_wls_init read the pair's left image
    PSM_HIP(c, hipEventRecord(w.ev_done, c->stream));
    w.have = true;
    w.invalid = a.invalid;
    w.timed = timed;
    w.pending = c->opt_async != 0;
    if (c->opt_async) return 0;
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int psm_wls_wait(psm_ctx *c)
{
    if (!c) return fail(nullptr, "psm_wls_wait: NULL context");
    if (!c->wls.pending) return fail(c, "psm_wls_wait: no asynchronous psm_wls_filter started");
    if (result_ready(c, "psm_wls_wait")) return 1;
    c->wls.pending = false;
    return 0;
}

int psm_wls_download(psm_ctx *c, int16_t *disp, float *q, float *num, float *den, size_t stride_bytes)
{
    if (!c) return fail(nullptr, "psm_wls_download: NULL context");
    const size_t row = (size_t)c->W * sizeof(float);
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row || stride_bytes % 4) return fail(c, "psm_wls_download: stride %zu: a multiple of 4, at least the row size %zu", stride_bytes, row);
    if (result_ready(c, "psm_wls_download")) return 1;
    const WlsState &w = c->wls;
    const size_t HW = (size_t)c->W * c->H;
    if (disp && d2h_rows(c, disp, w.out, row / 2, stride_bytes / 2, c->H)) return 1;
    if (q && d2h_rows(c, q, w.q, row, stride_bytes, c->H)) return 1;
    if (num && d2h_rows(c, num, w.work, row, stride_bytes, c->H)) return 1;
    if (den && d2h_rows(c, den, w.work + HW, row, stride_bytes, c->H)) return 1;
    return 0;
}

int psm_wls_download_table(psm_ctx *c, float tab[256])
{
    if (!c) return fail(nullptr, "psm_wls_download_table: NULL context");
    if (!tab) return fail(c, "psm_wls_download_table: NULL pointer");
    if (result_ready(c, "psm_wls_download_table")) return 1;
    return d2h_rows(c, tab, c->wls.tab, WLS_TAB * sizeof(float), WLS_TAB * sizeof(float), 1);
}

int psm_wls_time(psm_ctx *c, double *ms)
{
    if (!c) return fail(nullptr, "psm_wls_time: NULL context");
    if (!ms) return fail(c, "psm_wls_time: NULL pointer");
    if (!c->wls.have || !c->wls.timed) return fail(c, "psm_wls_time: the last psm_wls_filter was not timed (PSM_OPT_PROFILE)");
    if (bind(c)) return 1;
    PSM_HIP(c, hipEventSynchronize(c->wls.ev[1]));
    float t = 0.f;
    PSM_HIP(c, hipEventElapsedTime(&t, c->wls.ev[0], c->wls.ev[1]));
    *ms = t;
    return 0;
}

int psm_wls_publish(psm_ctx *c, int on)
{
    if (!c) return fail(nullptr, "psm_wls_publish: NULL context");
    if (on && !c->wls.have) return fail(c, "psm_wls_publish: no psm_wls_filter ran (or its planes were released)");
    c->wls.publish = on != 0;
    return 0;
}

}  // extern "C"
