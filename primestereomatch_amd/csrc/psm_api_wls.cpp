// psm_api_wls.cpp - psm_wls_filter: edge-aware WLS smoothing of a sub-pixel disparity map behind the C ABI - the confidence-weighted
// global smoothing users of cv::StereoSGBM apply at this point (cv::ximgproc::DisparityWLSFilter), by Min et al.'s Fast Global
// Smoother: it fills the holes of the int16 map from their surroundings, keeps depth edges on image edges and keeps the sixteenths.
// Kernels: psm_wls.hip.  The definition is tests/wls_model.py / DESIGN.md 13.  An independent stage, as psm_score and psm_reproject
// are: it reads the context's current result - the int16 map of the SGM stage (or the hook plane), or the left 8-bit map and its
// mask through psm::Results - and the left image of the pair, and writes its own planes (psm::WlsState).  psm_wls_publish lets the
// SGM sources of psm_score and psm_reproject read its result instead of the SGM stage's.
// psm_wls_filter_batch: the same launches for the maps of several contexts at once, the context on a grid axis of its own.
// PSM_WLS_CONFIDENCE (psm_wls_set_confidence; tests/wls_conf_model.py): wls_run puts k_sgm_right16 and k_wls_conf ahead of them and
// the solve starts with a graded confidence instead of one bit per pixel.
#include "psm_ctx.h"
#include "psm_wls_tab.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

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
    table_free(w.pairs);
    if (w.ev_done) (void)hipEventDestroy(w.ev_done);
    w.ev_done = nullptr;
    bracket_free(w.prof);
    (void)hipFree(w.conf); w.conf = nullptr;
    (void)hipFree(w.r16); w.r16 = nullptr;
    bracket_free(w.conf_prof);
    w.have_conf = 0;
    w.have = w.pending = w.publish = false;
}

}  // namespace psm

namespace {

constexpr int WLS_FLAGS_ALL = PSM_WLS_USE_MASK | PSM_WLS_CONFIDENCE;

// what psm_wls_filter refuses about the call's own arguments (no context needed) ...
int check_call(psm_ctx *e, const char *who, int source, int flags)
{
    if (source != PSM_WLS_GIF && source != PSM_WLS_SGM) return fail(e, "%s: source %d not in {0: PSM_WLS_GIF, 1: PSM_WLS_SGM}", who, source);
    if (flags & ~WLS_FLAGS_ALL) return fail(e, "%s: unknown flag bits 0x%x", who, flags & ~WLS_FLAGS_ALL);
    if ((flags & PSM_WLS_USE_MASK) && source != PSM_WLS_GIF)
        return fail(e, "%s: PSM_WLS_USE_MASK with the SGM source (the L-R mask belongs to the 8-bit maps)", who);
    if ((flags & PSM_WLS_CONFIDENCE) && source != PSM_WLS_SGM)
        return fail(e, "%s: flag bits 0x%x (PSM_WLS_CONFIDENCE) with the GIF source (the confidence is made of the SGM stage's map and costs)", who,
                    PSM_WLS_CONFIDENCE);
    return 0;
}

int check_conf_params(psm_ctx *e, const char *who, int terms, int lr_thresh, int radius, int var_shift)
{
    if (terms < 1 || terms > (PSM_WLS_CONF_LR | PSM_WLS_CONF_VAR)) return fail(e, "%s: terms %d not in {1: PSM_WLS_CONF_LR, 2: PSM_WLS_CONF_VAR, 3: both}", who, terms);
    if (lr_thresh < 1 || lr_thresh > 32767) return fail(e, "%s: lr_thresh %d outside [1, 32767]", who, lr_thresh);
    if (radius < 1 || radius > WLS_CONF_RMAX) return fail(e, "%s: radius %d outside [1, %d]", who, radius, WLS_CONF_RMAX);
    if (var_shift < 0 || var_shift > 16) return fail(e, "%s: var_shift %d outside [0, 16]", who, var_shift);
    return 0;
}

// ... and about one context; e: the context that receives the message (a batch: its first; who names the member)
int check_ctx(psm_ctx *e, const psm_ctx *c, const char *who, int source, int flags)
{
    if (source == PSM_WLS_GIF) {
        if (!c->res.maps) return fail(e, "%s: no disparity maps computed (PSM_WLS_GIF)", who);
        if (stripe_only(c)) return fail(e, "%s: the maps hold this context's row stripe only (gather the stripes first)", who);
        if ((flags & PSM_WLS_USE_MASK) && !c->res.mask) return fail(e, "%s: PSM_WLS_USE_MASK without a current L-R mask (psm_lr_check)", who);
    } else if (!sgm_stage_exists(c)) {
        return fail(e, "%s: no SGM result (psm_sgm_compute) for the SGM source", who);
    }
    if (!colour_of(c, source == PSM_WLS_SGM).img)
        return fail(e, "%s: no current image pair (psm_upload_pair: the left image guides the smoothing)", who);
    if ((flags & PSM_WLS_CONFIDENCE) && (c->wls.conf_terms & PSM_WLS_CONF_LR)) {
        // the L-R term reads the S the map was selected from: the last psm_sgm_compute*'s of this context, with that result's range
        // (with the hook plane off, sgm_stage_exists above has answered for a compute that never ran or was released: S lives and
        // dies with the map)
        const SgmState &g = c->sgm;
        if (c->score.hook_on)
            return fail(e, "%s: flag bits 0x%x (PSM_WLS_CONFIDENCE): the L-R term while the plane of psm_score_upload_sgm_map is on (the summed costs do not belong to it)",
                        who, PSM_WLS_CONFIDENCE);
        if (g.res_d < 1 || g.res_d > SGM_DMAX || g.res_dmin < -SGM_DMAX || g.res_dmin > SGM_DMAX)
            return fail(e, "%s: the result's range (min_disparity %d, %d disparities) is outside what k_sgm_right16 serves", who, g.res_dmin, g.res_d);
        if ((size_t)c->W * sizeof(unsigned) > WLS_R16_LDS_MAX)
            return fail(e, "%s: width %d: a row's keys (%zu bytes) exceed the %zu bytes of LDS a workgroup takes", who, c->W, (size_t)c->W * sizeof(unsigned),
                        WLS_R16_LDS_MAX);
    }
    return 0;
}

int ensure_buffers(psm_ctx *c, int flags)
{
    WlsState &w = c->wls;
    const size_t HW = (size_t)c->W * c->H;
    if (!w.work) PSM_HIP(c, hipMalloc((void **)&w.work, 5 * HW * sizeof(float)));
    if (!w.links) PSM_HIP(c, hipMalloc((void **)&w.links, 2 * HW));
    if (!w.out) PSM_HIP(c, hipMalloc((void **)&w.out, HW * sizeof(int16_t)));
    if (!w.q) PSM_HIP(c, hipMalloc((void **)&w.q, HW * sizeof(unsigned)));
    if (!w.tab) PSM_HIP(c, hipMalloc((void **)&w.tab, WLS_TAB * sizeof(float)));
    if (!w.ev_done) PSM_HIP(c, hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
    if (flags & PSM_WLS_CONFIDENCE) {
        if (!w.conf) PSM_HIP(c, hipMalloc((void **)&w.conf, HW));
        if (!w.r16) PSM_HIP(c, hipMalloc((void **)&w.r16, HW * sizeof(int16_t)));
        if (bracket_events(c, w.conf_prof)) return 1;
    }
    return bracket_events(c, w.prof);
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
    a.conf = (flags & PSM_WLS_CONFIDENCE) ? w.conf : nullptr;
    return a;
}

// the member's own terms and parameters, and - the L-R term - the S of its SGM result with that result's range
WlsConf wls_conf_args(const psm_ctx *c, int flags)
{
    WlsConf k = {};
    if (!(flags & PSM_WLS_CONFIDENCE)) return k;
    const WlsState &w = c->wls;
    k.r16 = w.r16; k.conf = w.conf;
    k.terms = w.conf_terms; k.thresh = w.conf_thresh; k.radius = w.conf_radius; k.shift = w.conf_shift;
    if (k.terms & PSM_WLS_CONF_LR) {
        k.S = c->sgm.S;
        k.D = c->sgm.res_d; k.Dp = sgm_dp(c->sgm.res_d); k.dmin = c->sgm.res_dmin;
    }
    return k;
}

// the planes of the last run, complete: an asynchronous run is waited for on the way
int result_ready(psm_ctx *c, const char *who)
{
    if (!c->wls.have) return fail(c, "%s: no psm_wls_filter ran (or its planes were released)", who);
    if (bind(c)) return 1;
    PSM_HIP(c, hipEventSynchronize(c->wls.ev_done));
    return 0;
}

// the member's weight table on the device is that of its sigma: uploaded on its own stream, only when sigma changed
int table_current(psm_ctx *c)
{
    WlsState &w = c->wls;
    if (w.tab_sigma == w.sigma) return 0;
    // (the copy out of tab_host of an earlier run has executed: a pageable source is staged before the call returns)
    wls_table(w.sigma, w.tab_host);
    w.tab_sigma = 0.0f;
    PSM_HIP(c, hipMemcpyAsync(w.tab, w.tab_host, sizeof w.tab_host, hipMemcpyHostToDevice, c->stream));
    w.tab_sigma = w.sigma;
    return 0;
}

// The host sequence of psm_wls_filter (its one context, the record by value) and of psm_wls_filter_batch (batch: the same kernels
// over the device table of ctxs[0]), the arguments and every context checked: 1 + 2 T launches on
// ctxs[0]'s stream.  T is ctxs[0]'s: the batch's.
int wls_run(const char *who, psm_ctx *const *ctxs, int n, int source, int flags, bool batch)
{
    psm_ctx *c0 = ctxs[0];
    if (bind(c0)) return 1;
    hipStream_t s = c0->stream;
    const int T = c0->wls.iters;

    // ---- buffers, events and the table's memory: before any launch ----
    for (int i = 0; i < n; ++i)
        if (ensure_buffers(ctxs[i], flags)) return member_failed(c0, who, i, ctxs[i]);
    if (batch_events(c0, ctxs, n)) return 1;
    std::vector<WlsPair> tab((size_t)n);
    for (int i = 0; i < n; ++i) {
        tab[i].a = wls_args(ctxs[i], source, flags);
        tab[i].c = wls_conf_args(ctxs[i], flags);
        for (int t = 0; t < T; ++t) tab[i].lam[t] = wls_lambda(ctxs[i]->wls.lambda, T, t);
    }
    bool fresh = false;
    if (batch && table_reserve(c0, c0->wls.pairs, tab.data(), tab.size() * sizeof(WlsPair), &fresh)) return 1;
    const Recs<WlsPair> q{tab.data(), batch ? (const WlsPair *)c0->wls.pairs.dev : nullptr, n};

    // ---- every context's earlier work (the map to filter, its weight table, a single psm_wls_filter) is ordered before the shared launches ----
    for (int i = 0; i < n; ++i)
        if (table_current(ctxs[i])) return member_failed(c0, who, i, ctxs[i]);
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, c0->wls.pairs, tab.data(), tab.size() * sizeof(WlsPair))) return 1;

    for (int i = 0; i < n; ++i) {
        WlsState &w = ctxs[i]->wls;
        w.have = w.pending = w.prof.timed = w.conf_prof.timed = false;   // (every check and allocation lies before this: the planes are about to be rewritten)
    }
    if (bracket_open(c0, c0->wls.prof, s)) return 1;
    if (flags & PSM_WLS_CONFIDENCE) {                // the confidence bytes of every member, from its map and - the L-R term - its S
        int dp_max = 0;
        for (const WlsPair &p : tab) dp_max = std::max(dp_max, p.c.Dp);
        if (bracket_open(c0, c0->wls.conf_prof, s)) return 1;
        if (dp_max) launch_sgm_right16(s, q, dp_max);
        launch_wls_conf(s, q);
        if (bracket_close(c0, c0->wls.conf_prof, s)) return 1;
    }
    launch_wls_init(s, q);
    for (int t = 0; t < T; ++t) {
        launch_wls_rows(s, q, t);
        launch_wls_cols(s, q, t, t == T - 1);
    }
    if (check_launch(c0, "k_sgm_right16, k_wls_conf, k_wls_init, k_wls_rows, k_wls_cols")) return 1;
    if (bracket_close(c0, c0->wls.prof, s)) return 1;

    // ---- every context is now where its own psm_wls_filter would have left it; only context 0 counts as timed ----
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if (colour_of(c, source == PSM_WLS_SGM).slots && images_read(c, s)) return member_failed(c0, who, i, c);   // k_wls_init read the pair's left image
        PSM_HIP(c0, hipEventRecord(c->wls.ev_done, s));
    }
    if (batch_fork(c0, ctxs, n)) return 1;
    for (int i = 0; i < n; ++i) {
        WlsState &w = ctxs[i]->wls;
        w.have = true;
        w.invalid = tab[i].a.invalid;
        w.have_conf = tab[i].c.terms;
        w.pending = c0->opt_async != 0;
    }
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(s));
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

int psm_wls_set_confidence(psm_ctx *c, int terms, int lr_thresh, int radius, int var_shift)
{
    if (check_conf_params(c, "psm_wls_set_confidence", terms, lr_thresh, radius, var_shift)) return 1;
    if (!c) return fail(nullptr, "psm_wls_set_confidence: NULL context");
    c->wls.conf_terms = terms;
    c->wls.conf_thresh = lr_thresh;
    c->wls.conf_radius = radius;
    c->wls.conf_shift = var_shift;
    return 0;
}

int psm_wls_filter(psm_ctx *c, int source, int flags)
{
    const char *who = "psm_wls_filter";
    if (check_call(c, who, source, flags)) return 1;
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_ctx(c, c, who, source, flags)) return 1;
    return wls_run(who, &c, 1, source, flags, false);
}

// The launches of psm_wls_filter with the context on a grid axis of its own.  Planes, table and parameters stay per context; the
// kernels reach them through a device table ctxs[0] owns.  Every context ends where its own psm_wls_filter would have left it.
int psm_wls_filter_batch(psm_ctx *const *ctxs, int n, int source, int flags)
{
    const char *who = "psm_wls_filter_batch";
    psm_ctx *c0 = ctxs && n >= 1 ? ctxs[0] : nullptr;
    if (check_call(c0, who, source, flags)) return 1;
    if (!ctxs) return fail(nullptr, "%s: NULL ctxs", who);
    if (n < 1) return fail(nullptr, "%s: n %d below 1", who, n);
    if (!c0) return fail(nullptr, "%s: context 0 is NULL", who);
    if (n > 4096) return fail(c0, "%s: %d contexts (at most 4096 per call)", who, n);
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        const psm_ctx *c = ctxs[i];
        if (c->W != c0->W || c->H != c0->H || c->device != c0->device)
            return fail(c0, "%s: context %d has another width / height / device than context 0", who, i);
        if (c->wls.iters != c0->wls.iters)
            return fail(c0, "%s: context %d has iterations %d, context 0 has %d (the launches are the batch's; lambda and sigma may differ)", who, i,
                        c->wls.iters, c0->wls.iters);
        char member[64];
        snprintf(member, sizeof member, "%s: context %d", who, i);
        if (check_ctx(c0, c, member, source, flags)) return 1;
    }
    return wls_run(who, ctxs, n, source, flags, true);
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

int psm_wls_download_confidence(psm_ctx *c, uint8_t *conf, size_t conf_stride, int16_t *right16, size_t right_stride_bytes)
{
    const char *who = "psm_wls_download_confidence";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    const size_t row = (size_t)c->W;
    if (conf_stride == 0) conf_stride = row;
    if (right_stride_bytes == 0) right_stride_bytes = 2 * row;
    if (conf_stride < row) return fail(c, "%s: conf_stride %zu below the row size %zu", who, conf_stride, row);
    if (right_stride_bytes < 2 * row || right_stride_bytes % 2) return fail(c, "%s: right_stride_bytes %zu: a multiple of 2, at least the row size %zu", who, right_stride_bytes, 2 * row);
    if (result_ready(c, who)) return 1;
    const WlsState &w = c->wls;
    if (!w.have_conf) return fail(c, "%s: the last psm_wls_filter ran without PSM_WLS_CONFIDENCE", who);
    if (right16 && !(w.have_conf & PSM_WLS_CONF_LR)) return fail(c, "%s: the last psm_wls_filter ran without the L-R term: there is no right map", who);
    if (conf && d2h_rows(c, conf, w.conf, row, conf_stride, c->H)) return 1;
    if (right16 && d2h_rows(c, right16, w.r16, 2 * row, right_stride_bytes, c->H)) return 1;
    return 0;
}

int psm_wls_conf_time(psm_ctx *c, double *ms)
{
    if (!c) return fail(nullptr, "psm_wls_conf_time: NULL context");
    return bracket_ms(c, c->wls.conf_prof, c->wls.have && c->wls.have_conf, "psm_wls_conf_time",
                      "the last psm_wls_filter was not timed (PSM_OPT_PROFILE) or ran without PSM_WLS_CONFIDENCE", ms);
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
    return bracket_ms(c, c->wls.prof, c->wls.have, "psm_wls_time", "the last psm_wls_filter was not timed (PSM_OPT_PROFILE)", ms);
}

int psm_wls_publish(psm_ctx *c, int on)
{
    if (!c) return fail(nullptr, "psm_wls_publish: NULL context");
    if (on && !c->wls.have) return fail(c, "psm_wls_publish: no psm_wls_filter ran (or its planes were released)");
    c->wls.publish = on != 0;
    return 0;
}

}  // extern "C"
