// psm_api_score.cpp - psm_score: the steps of StereoMatch::compute behind the maps - the display conversion of either algorithm
// (src/StereoMatch.cpp:181-185, 248-249) and the error metric against ground truth (:275-309) - on the device, behind the C ABI.
// Kernels: psm_score.hip.  The definition is tests/score_model.py / DESIGN.md 11.  An independent stage: it reads the context's
// current result - the maps through psm::Results, the int16 map of the SGM stage - and writes its own planes (psm::ScoreState).
// psm_score_batch: the same launches for the results of several contexts at once, the context on a grid axis of its own.  Both
// entries check their arguments and enqueue through score_run.
#include "psm_ctx.h"

#include <cstdio>
#include <cstring>

using namespace psm;

namespace psm {

void score_free(psm_ctx *c, bool truth)
{
    ScoreState &q = c->score;
    (void)hipFree(q.planes); q.planes = nullptr;
    (void)hipFree(q.cnt); q.cnt = nullptr;
    if (q.pin) (void)hipHostFree(q.pin);
    q.pin = nullptr;
    if (q.ev_done) (void)hipEventDestroy(q.ev_done);
    q.ev_done = nullptr;
    bracket_free(q.prof);
    table_free(q.tab);
    q.source = -1;
    q.pending = false;
    if (truth) {
        (void)hipFree(q.gt); q.gt = nullptr;
        (void)hipFree(q.mask); q.mask = nullptr;
        (void)hipFree(q.hook); q.hook = nullptr;
        q.have_truth = q.have_mask = q.hook_on = false;
    }
}

}  // namespace psm

namespace {

bool is_sgm(int source) { return source == PSM_SCORE_SGM || source == PSM_SCORE_SGM_INT; }
bool use_mask(const ScoreState &q) { return q.have_truth && q.have_mask && q.mask_mode != PSM_MASK_NONE; }

// what psm_score refuses about one context; e: the context that receives the message (a batch: its first; who names the member)
int check_source(psm_ctx *e, const psm_ctx *c, const char *who, int source)
{
    if (source != PSM_SCORE_GIF && !is_sgm(source))
        return fail(e, "%s: source %d not in {0: PSM_SCORE_GIF, 1: PSM_SCORE_SGM, 2: PSM_SCORE_SGM_INT}", who, source);
    if (source == PSM_SCORE_GIF) {
        if (!c->res.maps) return fail(e, "%s: no disparity maps computed (PSM_SCORE_GIF)", who);
        if (stripe_only(c)) return fail(e, "%s: the maps hold this context's row stripe only (gather the stripes first)", who);
    } else if (!sgm_source_exists(c)) {
        return fail(e, "%s: no SGM result (psm_sgm_compute) for an SGM source", who);
    }
    return 0;
}

int ensure_scratch(psm_ctx *c)
{
    ScoreState &q = c->score;
    const size_t HW = (size_t)c->W * c->H;
    if (!q.planes) PSM_HIP(c, hipMalloc((void **)&q.planes, 3 * HW));
    if (!q.cnt) PSM_HIP(c, hipMalloc((void **)&q.cnt, sizeof(ScCnt)));
    if (!q.pin) PSM_HIP(c, hipHostMalloc((void **)&q.pin, sizeof(ScCnt), hipHostMallocDefault));
    if (!q.ev_done) PSM_HIP(c, hipEventCreateWithFlags(&q.ev_done, hipEventDisableTiming));
    return bracket_events(c, q.prof);
}

// the context's buffers (ensure_scratch) as the kernels take them: a single call's record, an entry of a batch's table
ScPair score_pair(const psm_ctx *c)
{
    const ScoreState &q = c->score;
    return ScPair{c->maps, sgm_source_map(c), q.have_truth ? q.gt : nullptr, use_mask(q) ? q.mask : nullptr, q.planes, q.cnt};
}

ScArgs score_args(const psm_ctx *c)
{
    const ScoreState &q = c->score;
    ScArgs a;
    a.W = c->W; a.H = c->H; a.D = c->D;
    a.scale = q.scale;
    a.thr = q.thr * (127 / c->D);
    a.disc = q.mask_mode == PSM_MASK_DISC;
    return a;
}

// the record of a context from the counters in its page-locked slot (their copy has executed)
void fill_record(const psm_ctx *c, struct psm_score *out)
{
    const ScoreState &q = c->score;
    const bool mm = q.source == PSM_SCORE_SGM;
    out->min_val = mm ? q.pin->mn + SC_MN_BIAS : 0;
    out->max_val = mm ? q.pin->mx - SC_MX_BIAS : 0;
    out->pixels = (uint32_t)((size_t)c->W * c->H);
    out->bad = q.pin->bad;
    out->err_sum = q.pin->sum;
    out->unit = q.unit;
    out->flags = mm && out->min_val == out->max_val ? PSM_SCORE_FLAT : 0u;
}

// The host sequence of psm_score (its one context, the record by value) and of psm_score_batch (batch: the same kernels over the
// device table of ctxs[0]), the arguments and every context checked: one or two launches on ctxs[0]'s stream.  Every context ends
// where its own psm_score would have left it, its counters in its page-locked slot (fill_record) unless the call is asynchronous.
int score_run(const char *who, psm_ctx *const *ctxs, int n, int source, bool batch)
{
    psm_ctx *c0 = ctxs[0];
    if (bind(c0)) return 1;
    hipStream_t s = c0->stream;
    ScoreState &t = c0->score;

    // ---- buffers, events and the table's memory: before any launch ----
    for (int i = 0; i < n; ++i)
        if (ensure_scratch(ctxs[i])) return member_failed(c0, who, i, ctxs[i]);
    if (batch_events(c0, ctxs, n)) return 1;
    std::vector<ScPair> tab((size_t)n);
    for (int i = 0; i < n; ++i) tab[i] = score_pair(ctxs[i]);
    bool fresh = false;
    if (batch && table_reserve(c0, t.tab, tab.data(), tab.size() * sizeof(ScPair), &fresh)) return 1;
    const Recs<ScPair> recs{tab.data(), batch ? (const ScPair *)t.tab.dev : nullptr, n};

    // ---- every context's earlier work (the result to score, a single psm_score) is ordered before the shared launches ----
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, t.tab, tab.data(), tab.size() * sizeof(ScPair))) return 1;

    for (int i = 0; i < n; ++i) {
        ScoreState &q = ctxs[i]->score;
        q.source = -1;                          // (every check and allocation lies before this: the planes are about to be rewritten)
        q.pending = q.prof.timed = false;
        PSM_HIP(c0, hipMemsetAsync(q.cnt, 0, sizeof(ScCnt), s));
    }
    const ScArgs a = score_args(c0);
    if (bracket_open(c0, t.prof, s)) return 1;
    if (source == PSM_SCORE_SGM) launch_sc_minmax(s, a, recs);
    launch_sc_score(s, source, a, recs);
    if (check_launch(c0, "k_sc_minmax, k_sc_score")) return 1;
    if (bracket_close(c0, t.prof, s)) return 1;

    // ---- every context is now where its own psm_score would have left it; only context 0 counts as timed ----
    for (int i = 0; i < n; ++i) {
        ScoreState &q = ctxs[i]->score;
        PSM_HIP(c0, hipMemcpyAsync(q.pin, q.cnt, sizeof(ScCnt), hipMemcpyDeviceToHost, s));
        PSM_HIP(c0, hipEventRecord(q.ev_done, s));
    }
    if (batch_fork(c0, ctxs, n)) return 1;
    for (int i = 0; i < n; ++i) {
        ScoreState &q = ctxs[i]->score;
        q.source = source;
        q.unit = 127 / ctxs[i]->D;
        q.pending = c0->opt_async != 0;
    }
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(s));
    return 0;
}

}  // namespace

extern "C" {

int psm_score_set_truth(psm_ctx *c, const uint8_t *gt, const uint8_t *mask, size_t stride_bytes)
{
    if (!c) return fail(nullptr, "psm_score_set_truth: NULL context");
    if (!gt) return fail(c, "psm_score_set_truth: NULL ground truth (psm_score_clear_truth removes one)");
    const size_t row = (size_t)c->W;
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row) return fail(c, "psm_score_set_truth: stride %zu < width %d", stride_bytes, c->W);
    if (bind(c)) return 1;
    ScoreState &q = c->score;
    if (!q.gt) PSM_HIP(c, hipMalloc((void **)&q.gt, row * c->H));
    if (mask && !q.mask) PSM_HIP(c, hipMalloc((void **)&q.mask, row * c->H));
    q.have_truth = q.have_mask = false;
    if (h2d_rows(c, q.gt, gt, row, stride_bytes, c->H)) return 1;
    if (mask && h2d_rows(c, q.mask, mask, row, stride_bytes, c->H)) return 1;
    PSM_HIP(c, hipStreamSynchronize(c->stream));      // the copy reads caller memory (psm_upload_pair)
    q.have_truth = true;
    q.have_mask = mask != nullptr;
    return 0;
}

int psm_score_clear_truth(psm_ctx *c)
{
    if (!c) return fail(nullptr, "psm_score_clear_truth: NULL context");
    c->score.have_truth = c->score.have_mask = false;      // (the planes stay for the next truth)
    return 0;
}

int psm_score_set_params(psm_ctx *c, int scale_factor, int error_threshold, int mask_mode)
{
    if (scale_factor < 1 || scale_factor > 255)             // (without a context the message is psm_last_error(NULL)'s)
        return fail(c, "psm_score_set_params: scale_factor %d outside [1, 255]", scale_factor);
    if (error_threshold < 0 || error_threshold > 255) return fail(c, "psm_score_set_params: error_threshold %d outside [0, 255]", error_threshold);
    if (mask_mode != PSM_MASK_NONE && mask_mode != PSM_MASK_NONOCC && mask_mode != PSM_MASK_DISC)
        return fail(c, "psm_score_set_params: mask_mode %d not in {0: PSM_MASK_NONE, 1: PSM_MASK_NONOCC, 2: PSM_MASK_DISC}", mask_mode);
    if (!c) return fail(nullptr, "psm_score_set_params: NULL context");
    c->score.scale = scale_factor;
    c->score.thr = error_threshold;
    c->score.mask_mode = mask_mode;
    return 0;
}

int psm_score(psm_ctx *c, int source, struct psm_score *out)
{
    if (!c) return fail(nullptr, "psm_score: NULL context");
    if (check_source(c, c, "psm_score", source)) return 1;
    if (!out && !c->opt_async) return fail(c, "psm_score: NULL record (only PSM_OPT_ASYNC leaves it to psm_score_wait)");
    if (score_run("psm_score", &c, 1, source, false)) return 1;
    if (!c->opt_async) fill_record(c, out);
    return 0;
}

int psm_score_wait(psm_ctx *c, struct psm_score *out)
{
    if (!c) return fail(nullptr, "psm_score_wait: NULL context");
    if (!out) return fail(c, "psm_score_wait: NULL record");
    if (!c->score.pending) return fail(c, "psm_score_wait: no asynchronous psm_score started");
    if (bind(c)) return 1;
    PSM_HIP(c, hipEventSynchronize(c->score.ev_done));
    c->score.pending = false;
    fill_record(c, out);
    return 0;
}

int psm_score_download(psm_ctx *c, uint8_t *ldisp, uint8_t *rdisp, uint8_t *emap, size_t stride)
{
    if (!c) return fail(nullptr, "psm_score_download: NULL context");
    if (stride == 0) stride = (size_t)c->W;
    if (stride < (size_t)c->W) return fail(c, "psm_score_download: stride %zu < width %d", stride, c->W);
    const ScoreState &q = c->score;
    if (q.source < 0) return fail(c, "psm_score_download: no psm_score ran (or its planes were released)");
    if (rdisp && q.source != PSM_SCORE_GIF) return fail(c, "psm_score_download: a right display map exists for PSM_SCORE_GIF only");
    if (bind(c)) return 1;
    const size_t HW = (size_t)c->W * c->H;
    if (copy_maps_out(c, q.planes, ldisp, rdisp, stride)) return 1;
    return copy_maps_out(c, q.planes + 2 * HW, emap, nullptr, stride);
}

// The launches of psm_score with the context on a grid axis of its own (score_run).  Buffers stay per context; the kernels reach
// them through a device table ctxs[0] owns.
int psm_score_batch(psm_ctx *const *ctxs, int n, int source, struct psm_score *outs)
{
    const char *who = "psm_score_batch";
    if (!ctxs || n < 1 || !ctxs[0]) return fail(nullptr, "%s: bad arguments", who);
    psm_ctx *c0 = ctxs[0];
    if (n > 4096) return fail(c0, "%s: %d contexts (at most 4096 per call)", who, n);
    if (!outs && !c0->opt_async) return fail(c0, "%s: NULL records (only PSM_OPT_ASYNC leaves them to psm_score_wait)", who);
    const ScoreState &q0 = c0->score;
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        psm_ctx *c = ctxs[i];
        if (c->W != c0->W || c->H != c0->H || c->D != c0->D || c->device != c0->device)
            return fail(c0, "%s: context %d has another width / height / max_disp / device than context 0", who, i);
        char member[64];
        snprintf(member, sizeof member, "%s: context %d", who, i);
        if (check_source(c0, c, member, source)) return 1;
        const ScoreState &q = c->score;
        if (q.scale != q0.scale || q.thr != q0.thr || q.mask_mode != q0.mask_mode)
            return fail(c0, "%s: context %d has other score parameters (psm_score_set_params) than context 0", who, i);
        if (q.have_truth != q0.have_truth)
            return fail(c0, "%s: context %d has %s ground truth, context 0 has %s (psm_score_set_truth: on all contexts or on none)", who, i,
                        q.have_truth ? "a" : "no", q0.have_truth ? "one" : "none");
        if (use_mask(q) != use_mask(q0))
            return fail(c0, "%s: context %d has %s mask, context 0 has %s (on all contexts or on none)", who, i, use_mask(q) ? "a" : "no",
                        use_mask(q0) ? "one" : "none");
    }
    if (score_run(who, ctxs, n, source, true)) return 1;
    for (int i = 0; i < n && !c0->opt_async; ++i) fill_record(ctxs[i], &outs[i]);
    return 0;
}

int psm_score_time(psm_ctx *c, double *ms)
{
    if (!c) return fail(nullptr, "psm_score_time: NULL context");
    return bracket_ms(c, c->score.prof, c->score.source >= 0, "psm_score_time", "the last psm_score was not timed (PSM_OPT_PROFILE)", ms);
}

int psm_score_upload_sgm_map(psm_ctx *c, const int16_t *disp, size_t stride_bytes)
{
    if (!c) return fail(nullptr, "psm_score_upload_sgm_map: NULL context");
    ScoreState &q = c->score;
    if (!disp) { q.hook_on = false; return 0; }
    const size_t row = (size_t)c->W * sizeof(int16_t);
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row) return fail(c, "psm_score_upload_sgm_map: stride %zu < row size %zu", stride_bytes, row);
    if (bind(c)) return 1;
    if (!q.hook) PSM_HIP(c, hipMalloc((void **)&q.hook, row * c->H));
    q.hook_on = false;
    if (h2d_rows(c, q.hook, disp, row, stride_bytes, c->H)) return 1;
    PSM_HIP(c, hipStreamSynchronize(c->stream));      // the copy reads caller memory
    q.hook_on = true;
    return 0;
}

}  // extern "C"
