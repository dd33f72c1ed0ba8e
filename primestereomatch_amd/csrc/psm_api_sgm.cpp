// psm_api_sgm.cpp - semi-global matching behind the C ABI: the STEREO_SGBM branch of StereoMatch::compute (ssgbm->compute(lFrame,
// rFrame, imgDisparity16S), src/StereoMatch.cpp:169-187) with the parameters of setupOpenCVSGBM (:639-660), on the device
// (psm_sgm.hip).  An independent stage: it reads the staged images and writes its own buffers (psm::SgmState) - volumes, maps,
// masks, keys and the records of psm_state.h never see it.  The definition is tests/sgm_model.py / DESIGN.md 10.  The last step
// of ssgbm->compute, the speckle filter (speckleWindowSize 100, speckleRange 32 there), is psm_speckle.hip: on the stage's map when
// psm_sgm_set_speckle turned it on, on a caller's map in psm_sgm_filter_speckles (tests/speckle_model.py).  The pixel cost is SAD
// (pre_filter_cap 0, a new context's setting) or, after psm_sgm_set_prefilter, StereoSGBM's Sobel-prefiltered Birchfield-Tomasi
// cost as tests/sgm_bt_model.py defines it (the reference: preFilterCap 63), or, after psm_sgm_set_census, the Hamming distance
// of census codes (tests/sgm_census_model.py).  Unpinned in all of it: a live cv::StereoSGBM.
// psm_sgm_compute_batch: the same launches for the pairs of several contexts at once, the pair on a grid axis of its own.
// psm_sgm_select_maps / _batch: the one place where the stage meets the rest - the context's two current 8-bit maps (psm::Results)
// from S, so that the post-processing and score stages run behind it (tests/sgm_maps_model.py).
// Single pairs and batches share the launch sequence (enqueue), the record of a pair's buffers (pair_of), the name of the pixel
// cost (cost_kind) and what a context forgets ahead of the launches and holds behind them (forget, mark); the entry points keep
// what differs - argument checks, the gray upload, a batch's cross-context checks, stream ordering and table.  The map select's
// two entries keep their checks and share the whole sequence (maps_run).
#include "psm_ctx.h"

#include <cstdio>
#include <cstring>

using namespace psm;

namespace psm {

void sgm_free(psm_ctx *c)
{
    SgmState &g = c->sgm;
    (void)hipFree(g.C); g.C = nullptr;
    (void)hipFree(g.S); g.S = nullptr;
    (void)hipFree(g.disp2); g.disp2 = nullptr;
    (void)hipFree(g.pre); g.pre = nullptr;
    (void)hipFree(g.out); g.out = nullptr;
    (void)hipFree(g.spk_label); g.spk_label = nullptr;
    (void)hipFree(g.spk_size); g.spk_size = nullptr;
    for (uint8_t *&p : g.gray) { (void)hipFree(p); p = nullptr; }
    for (uint8_t *&p : g.pf) { (void)hipFree(p); p = nullptr; }
    g.pf_ch = 0;
    for (uint64_t *&p : g.cen) { (void)hipFree(p); p = nullptr; }
    g.cen_have = false;
    for (hipEvent_t &e : g.ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    table_free(g.tab);
    bracket_free(g.maps);
    g.have = g.timed = g.spk_have = false;
    g.spk_t0 = -1;
    g.vol_dp = g.res_d = g.res_dmin = g.res_ch = 0;
}

}  // namespace psm

namespace {

// the disparities of the stage: psm_sgm_set_range's, or the context's max_disp; index k stands for the disparity dmin + k
inline int sgm_d(const psm_ctx *c) { return c->sgm.nd ? c->sgm.nd : c->D; }
inline int sgm_dp(const psm_ctx *c) { return psm::sgm_dp(sgm_d(c)); }
inline int sgm_invalid(const psm_ctx *c) { return (c->sgm.dmin - 1) * 16; }

// the conditions on the parameters for a pair of `ch` channels; *p1 / *p2: 0 resolved to the default
int check_params(psm_ctx *c, const char *who, int ch, int bs, int *p1, int *p2, int u)
{
    if (bs != 1 && bs != 3 && bs != 5 && bs != 7) return fail(c, "%s: block_size %d not in {1, 3, 5, 7}", who, bs);
    if (*p1 < 0 || *p2 < 0) return fail(c, "%s: P1 %d, P2 %d: 0 < P1 <= P2 required (0: the default)", who, *p1, *p2);
    if (*p1 == 0) *p1 = 8 * ch * bs * bs;
    if (*p2 == 0) *p2 = 32 * ch * bs * bs;
    if (*p1 > *p2) return fail(c, "%s: P1 %d > P2 %d (0 < P1 <= P2 required)", who, *p1, *p2);
    if ((long long)bs * bs * ch * 255 + *p2 > 65535)
        return fail(c, "%s: block_size^2 * channels * 255 + P2 = %lld > 65535 (a path cost must fit 16 bits)", who, (long long)bs * bs * ch * 255 + *p2);
    if (u < 0 || u >= 100) return fail(c, "%s: uniqueness_ratio %d outside [0, 100)", who, u);
    return 0;
}

// e: the context that receives the message (a batch: its first; who then names the member)
int check_ctx(psm_ctx *e, const psm_ctx *c, const char *who)
{
    if (c->Dloc != c->D || strided(c)) return fail(e, "%s: a disparity shard holds part of the range (the paths need every disparity of a pixel)", who);
    if (c->march.yend > c->march.ybeg) return fail(e, "%s: a row stripe is in force (psm_set_rows): the paths cross the whole image", who);
    if (sgm_d(c) < 2) return fail(e, "%s: max_disp %d < 2", who, sgm_d(c));
    return 0;
}

// the census cost and the prefilter exclude each other: a compute that finds both set is refused before it touches anything
int check_cost(psm_ctx *e, const psm_ctx *c, const char *who)
{
    const SgmState &g = c->sgm;
    if (g.cen_w > 0 && g.cap > 0)
        return fail(e, "%s: census window %d x %d (psm_sgm_set_census) and pre_filter_cap %d (psm_sgm_set_prefilter) are both set: one pixel cost at a time",
                    who, g.cen_w, g.cen_h, g.cap);
    return 0;
}

// ... and which one a context that passed is set to: the only place that reads the two settings for it.  Buffers, arguments,
// launchers, the kernel names of check_launch and the marks of a result all go by this.
enum class SgmCost { SAD, BT, CENSUS };
SgmCost cost_kind(const SgmState &g) { return g.cen_w > 0 ? SgmCost::CENSUS : (g.cap > 0 ? SgmCost::BT : SgmCost::SAD); }

int ensure_speckle_planes(psm_ctx *c)
{
    SgmState &g = c->sgm;
    const size_t HW = (size_t)c->W * c->H;
    if (!g.spk_label) PSM_HIP(c, hipMalloc((void **)&g.spk_label, HW * sizeof(unsigned)));
    if (!g.spk_size) PSM_HIP(c, hipMalloc((void **)&g.spk_size, HW * sizeof(unsigned)));
    return 0;
}

// everything a compute of this context's settings touches, the events of a timed one included
int ensure_buffers(psm_ctx *c)
{
    SgmState &g = c->sgm;
    const size_t HW = (size_t)c->W * c->H, V = HW * sgm_dp(c);
    if ((g.C || g.S) && g.vol_dp != sgm_dp(c)) {
        // another range's volumes: nothing may still read them (a batch runs on its first context's stream), and the result in
        // them is gone; a table that names them is compared against the new pointers by psm_sgm_compute_batch
        PSM_HIP(c, hipDeviceSynchronize());
        (void)hipFree(g.C); g.C = nullptr;
        (void)hipFree(g.S); g.S = nullptr;
        g.have = g.timed = false;
    }
    g.vol_dp = sgm_dp(c);
    if (!g.C) PSM_HIP(c, hipMalloc((void **)&g.C, V * sizeof(uint16_t)));
    if (!g.S) PSM_HIP(c, hipMalloc((void **)&g.S, V * sizeof(uint32_t)));
    if (!g.disp2) PSM_HIP(c, hipMalloc((void **)&g.disp2, HW * sizeof(uint32_t)));
    if (!g.pre) PSM_HIP(c, hipMalloc((void **)&g.pre, HW * sizeof(int16_t)));
    if (!g.out) PSM_HIP(c, hipMalloc((void **)&g.out, HW * sizeof(int16_t)));
    switch (cost_kind(g)) {
    case SgmCost::BT:
        for (uint8_t *&p : g.pf)
            if (!p) PSM_HIP(c, hipMalloc((void **)&p, HW * 6));
        break;
    case SgmCost::CENSUS:
        for (uint64_t *&p : g.cen)
            if (!p) PSM_HIP(c, hipMalloc((void **)&p, HW * sizeof(uint64_t)));
        break;
    case SgmCost::SAD: break;
    }
    if (g.spk_window > 0 && ensure_speckle_planes(c)) return 1;
    if (c->opt_profile)
        for (hipEvent_t &e : g.ev)
            if (!e) PSM_HIP(c, hipEventCreate(&e));
    return 0;
}

// One pair's buffers (ensure_buffers) as the kernels take them: the record a single call passes by value and a batch's device table
// holds.  l, r: the staged pair, or psm_sgm_compute_gray's.
SgmPair pair_of(const psm_ctx *c, const void *l, const void *r)
{
    const SgmState &g = c->sgm;
    SgmPair p{{l, r}, g.C, g.S, g.disp2, g.pre, g.out, {nullptr, nullptr}, nullptr, nullptr, c->maps};
    switch (cost_kind(g)) {
    case SgmCost::BT: p.pf[0] = g.pf[0]; p.pf[1] = g.pf[1]; break;
    case SgmCost::CENSUS: p.pf[0] = (uint8_t *)g.cen[0]; p.pf[1] = (uint8_t *)g.cen[1]; break;      // the code planes travel in the pf slots
    case SgmCost::SAD: break;
    }
    if (g.spk_window > 0) { p.spk_label = g.spk_label; p.spk_size = g.spk_size; }
    return p;
}

// the context's settings as the kernels take them
SgmArgs sgm_args(const psm_ctx *c, int depth, int ch, int p1, int p2)
{
    const SgmState &g = c->sgm;
    SgmArgs a = {};
    a.depth = depth; a.ch = ch;
    a.W = c->W; a.H = c->H; a.D = sgm_d(c); a.Dp = sgm_dp(c);
    a.dmin = g.dmin; a.invalid = sgm_invalid(c);
    a.bs = g.bs; a.P1 = p1; a.P2 = p2; a.u = g.u; a.m = g.m;
    if (cost_kind(g) == SgmCost::BT) a.ft = (g.cap > 15 ? g.cap : 15) | 1;
    a.cw = g.cen_w; a.chh = g.cen_h;
    return a;
}

// the filter's settings as the kernels take them
SpkArgs speckle_args(const psm_ctx *c, int new_val, int max_size, long long max_diff)
{
    SpkArgs a;
    a.W = c->W; a.H = c->H;
    a.new_val = new_val; a.max_size = max_size;
    a.max_diff = (int)(max_diff > 65535 ? 65535 : max_diff);      // (two int16 values differ by 65535 at most)
    return a;
}

// The speckle filter in place on stream s - on the `out` maps of the pairs of q, with their planes: four launches, nothing read
// back.  timed: the event behind them is c's ev[4] (the one ahead is already recorded).
int enqueue_speckle(psm_ctx *c, hipStream_t s, const SpkArgs &a, const Recs<SgmPair> &q, bool timed)
{
    launch_speckle(s, a, q);
    if (check_launch(c, "k_spk_*")) return 1;
    if (timed) PSM_HIP(c, hipEventRecord(c->sgm.ev[4], s));
    return 0;
}

// ahead of a compute's launches a context forgets its previous result (every check and allocation lies before this) ...
void forget(SgmState &g)
{
    g.have = g.timed = false;
    g.spk_t0 = -1;
    g.pf_ch = 0;
    g.cen_have = false;
    if (g.spk_window > 0) g.spk_have = false;             // (with the filter off, the sizes of an earlier run stay readable)
}

// ... and behind them it holds the result of this cost on `ch` channels over the D disparities from dmin on; timed: its own events
// bracketed them
void mark(SgmState &g, SgmCost kind, int ch, int dmin, int D, bool timed)
{
    g.have = true;
    g.res_d = D;
    g.res_dmin = dmin;
    g.res_ch = ch;
    g.timed = timed;
    g.pf_ch = kind == SgmCost::BT ? ch : 0;
    g.cen_have = kind == SgmCost::CENSUS;
    if (g.spk_window > 0) {
        g.spk_have = true;
        g.spk_t0 = timed ? 3 : -1;
    }
}

// The launches of a compute, for a single pair and for a batch alike: disp2 reset, the cost group, the mode's directions, select
// and check, the speckle filter if it is on - on stream s, with c's settings, events (PSM_OPT_PROFILE) and error slot.  q:
// the single pair's record (by value), or the n pairs of a batch's device table, c being the batch's first context.  `a` brings the
// scalars.  What the two deliberately do differently:
//   - a single pair resets disp2 with hipMemsetAsync, a batch with k_sgm_fill (one launch for the n planes);
//   - a batch is bracketed by its first context's events only: that context alone counts as timed (psm_sgm_compute_batch);
//   - psm_sgm_compute_gray comes with ch 1 in `a`, which has also resolved its P1 / P2 defaults (check_params);
//   - a batch reports a member's allocation failure on its first context, as "...: context i: <the member's message>" - by its
//     caller, as every check and allocation: nothing here can fail but a launch or an event.
// readers: the n contexts whose image slots the pairs are (null: psm_sgm_compute_gray's own planes) - behind the launches, outside
// the brackets of psm_sgm_times, each records that its images have been read (the cost group reads them; the paths, the select
// and the speckle filter read C, S and the maps).
int enqueue(psm_ctx *c, hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q, psm_ctx *const *readers)
{
    static const char *const cost_kernels[3] = {"k_sgm_cost", "k_sgm_prefilter, k_sgm_bt_*", "k_sgm_census, k_sgm_census_cost"};
    SgmState &g = c->sgm;
    const SgmCost kind = cost_kind(g);
    const bool timed = c->opt_profile != 0;
    const int n = q.n;
    // disp2 starts every frame as "nothing lands here"
    if (q.dev) launch_sgm_fill_batch(s, a, q.dev, n);
    else PSM_HIP(c, hipMemsetAsync(q.host[0].disp2, 0xff, (size_t)a.W * a.H * sizeof(uint32_t), s));
    if (timed) PSM_HIP(c, hipEventRecord(g.ev[0], s));
    switch (kind) {
    case SgmCost::SAD: launch_sgm_cost(s, a, q); break;
    case SgmCost::BT: launch_sgm_cost_bt(s, a, q); break;
    case SgmCost::CENSUS: launch_sgm_cost_census(s, a, q); break;
    }
    if (check_launch(c, cost_kernels[(int)kind])) return 1;
    if (timed) PSM_HIP(c, hipEventRecord(g.ev[1], s));
    // the directions of the mode in table order; the first launch stores S, so no sum of an earlier frame or mode survives
    for (int i = 0; i < SGM_MODE_NDIR[g.mode]; ++i) {
        const int *r = SGM_DIRS[SGM_MODE_DIRS[g.mode][i]];
        launch_sgm_path(s, a, r[0], r[1], i == 0, q);
    }
    if (check_launch(c, "k_sgm_path")) return 1;
    if (timed) PSM_HIP(c, hipEventRecord(g.ev[2], s));
    launch_sgm_select(s, a, q);
    if (check_launch(c, "k_sgm_select")) return 1;
    if (timed) PSM_HIP(c, hipEventRecord(g.ev[3], s));
    if (g.spk_window > 0) {
        // filterSpeckles(disp, (minDisparity - 1) * 16, speckleWindowSize, 16 * speckleRange), as StereoSGBM ends
        if (enqueue_speckle(c, s, speckle_args(c, a.invalid, g.spk_window, 16ll * g.spk_range), q, timed)) return 1;
    }
    for (int i = 0; readers && i < n; ++i)
        if (images_read(readers[i], s)) return member_failed(c, "the SGM stage", i, readers[i]);
    return 0;
}

// The records of a batch's device table (psm_sgm_compute_batch, psm_sgm_select_maps_batch): c0->sgm.tab, DESIGN.md 4.7
std::vector<SgmPair> pairs_of(psm_ctx *const *ctxs, int n)
{
    std::vector<SgmPair> tab((size_t)n);
    for (int i = 0; i < n; ++i) tab[i] = pair_of(ctxs[i], ctxs[i]->pair.raw[0], ctxs[i]->pair.raw[1]);
    return tab;
}

// psm_sgm_select_maps / _batch: what context c must be for the call `who`; e: the context that receives the message
int check_maps(psm_ctx *e, const psm_ctx *c, const char *who)
{
    const SgmState &g = c->sgm;
    if (c->Dloc != c->D || strided(c)) return fail(e, "%s: a disparity shard holds part of the range (the SGM stage does not run on it)", who);
    if (c->march.yend > c->march.ybeg) return fail(e, "%s: a row stripe is in force (psm_set_rows): the maps are whole-image maps", who);
    if (!g.have) return fail(e, "%s: no SGM result (psm_sgm_compute; psm_release_scratch gives it back)", who);
    if (g.res_dmin < 0 || g.res_dmin + g.res_d > c->D || g.res_dmin + g.res_d > 256)
        return fail(e, "%s: the result's range (min_disparity %d, %d disparities) is not inside [0, max_disp %d): the 8-bit maps hold the disparities 0 .. max_disp - 1, at most 256",
                    who, g.res_dmin, g.res_d, c->D);
    if (sgm_maps_lds_bytes(c->W) > SGM_MAPS_LDS_MAX)
        return fail(e, "%s: width %d: a row's keys and bytes (%zu bytes) exceed the %zu bytes of LDS a workgroup takes", who, c->W,
                    sgm_maps_lds_bytes(c->W), SGM_MAPS_LDS_MAX);
    return 0;
}

// the result of a context as k_sgm_maps takes it: its own range (mark), not the current setting's
SgmArgs maps_args(const psm_ctx *c)
{
    const SgmState &g = c->sgm;
    SgmArgs a = {};
    a.W = c->W; a.H = c->H; a.D = g.res_d; a.Dp = psm::sgm_dp(g.res_d);
    a.dmin = g.res_dmin;
    return a;
}

// behind the launch a context is where psm_upload_maps(l, r, NULL, NULL) leaves it: whole-image maps, no mask, no early map; the
// volume sides, the packed minima and whatever the guided-filter path has pending are not touched
void maps_selected(psm_ctx *c)
{
    forget_early(c->res);
    cover(c->res, whole_image(c));
    maps_written(c->res);
}

// The host sequence of psm_sgm_select_maps (its one context, the record by value) and of psm_sgm_select_maps_batch (batch: the same
// kernel over the device table of ctxs[0]), every context checked: one launch on ctxs[0]'s stream.  Every context ends where its
// own psm_sgm_select_maps would have left it.  The single entry has its copy_maps_out behind this function, which is why the
// closing synchronisation is the entries'.
int maps_run(psm_ctx *const *ctxs, int n, bool batch)
{
    psm_ctx *c0 = ctxs[0];
    if (bind(c0)) return 1;
    hipStream_t s = c0->stream;
    SgmState &g0 = c0->sgm;

    // ---- events and the table's memory: before anything is ordered or launched ----
    if (batch_events(c0, ctxs, n)) return 1;
    if (bracket_events(c0, g0.maps)) return 1;
    const std::vector<SgmPair> tab = pairs_of(ctxs, n);      // (pair_of: maps = c->maps)
    bool fresh = false;
    if (batch && table_reserve(c0, g0.tab, tab.data(), tab.size() * sizeof(SgmPair), &fresh)) return 1;
    const Recs<SgmPair> recs{tab.data(), batch ? (const SgmPair *)g0.tab.dev : nullptr, n};

    // ---- every context's earlier work (its compute, downloads of its maps) is ordered before the shared launch ----
    for (int i = 0; i < n; ++i)
        if (ctxs[i]->ev_down) PSM_HIP(c0, hipStreamWaitEvent(s, ctxs[i]->ev_down, 0));       // (maps_writable, for the stream that writes)
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, g0.tab, tab.data(), tab.size() * sizeof(SgmPair))) return 1;

    // ---- the launch; then every context is where its own psm_sgm_select_maps would have left it - only context 0 counts as timed ----
    for (int i = 0; i < n; ++i) ctxs[i]->sgm.maps.timed = false;
    if (bracket_open(c0, g0.maps, s)) return 1;
    launch_sgm_maps(s, maps_args(c0), recs);
    if (check_launch(c0, "k_sgm_maps")) return 1;
    if (bracket_close(c0, g0.maps, s)) return 1;
    if (batch_fork(c0, ctxs, n)) return 1;
    for (int i = 0; i < n; ++i) maps_selected(ctxs[i]);
    return 0;
}

// a single pair of `ch` channels through the stage on the context's stream (psm_sgm_compute: the context's image slots;
// psm_sgm_compute_gray: planes of its own)
int compute_one(psm_ctx *c, const char *who, const void *l, const void *r, int depth, int ch, bool slots)
{
    SgmState &g = c->sgm;
    int p1 = g.p1, p2 = g.p2;
    if (check_params(c, who, ch, g.bs, &p1, &p2, g.u)) return 1;
    if (ensure_buffers(c)) return 1;
    const SgmArgs a = sgm_args(c, depth, ch, p1, p2);
    const SgmPair p = pair_of(c, l, r);
    forget(g);
    if (enqueue(c, c->stream, a, Recs<SgmPair>{&p, nullptr, 1}, slots ? &c : nullptr)) return 1;
    mark(g, cost_kind(g), ch, a.dmin, a.D, c->opt_profile != 0);
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace

extern "C" {

int psm_sgm_set_params(psm_ctx *c, int block_size, int p1, int p2, int uniqueness_ratio, int disp12_max_diff)
{
    if (!c) return 1;
    const int bs = block_size ? block_size : 5;
    int q1 = p1, q2 = p2;
    if (check_params(c, "psm_sgm_set_params", 3, bs, &q1, &q2, uniqueness_ratio)) return 1;      // (the staged pair has 3 channels)
    SgmState &g = c->sgm;
    g.bs = bs; g.p1 = p1; g.p2 = p2; g.u = uniqueness_ratio; g.m = disp12_max_diff;
    return 0;
}

int psm_sgm_set_speckle(psm_ctx *c, int speckle_window_size, int speckle_range)
{
    if (!c) return 1;
    if (speckle_window_size < 0 || speckle_range < 0)
        return fail(c, "psm_sgm_set_speckle: speckle_window_size %d, speckle_range %d: negative", speckle_window_size, speckle_range);
    c->sgm.spk_window = speckle_window_size;
    c->sgm.spk_range = speckle_range;
    return 0;
}

int psm_sgm_set_prefilter(psm_ctx *c, int pre_filter_cap)
{
    if (!c) return 1;
    if (pre_filter_cap < 0 || pre_filter_cap > 63)
        return fail(c, "psm_sgm_set_prefilter: pre_filter_cap %d outside [0, 63] (0: the SAD cost)", pre_filter_cap);
    c->sgm.cap = pre_filter_cap;
    return 0;
}

int psm_sgm_set_census(psm_ctx *c, int win_w, int win_h)
{
    const bool off = win_w == 0 && win_h == 0;             // (without a context the message is psm_last_error(NULL)'s)
    if (!off && (win_w < 3 || win_w > SGM_CEN_MAXW || win_h < 3 || win_h > SGM_CEN_MAXH || win_w % 2 == 0 || win_h % 2 == 0))
        return fail(c, "psm_sgm_set_census: window %d x %d: both odd, width in [3, %d], height in [3, %d], or (0, 0) for off", win_w, win_h,
                    SGM_CEN_MAXW, SGM_CEN_MAXH);
    if (!c) return fail(nullptr, "psm_sgm_set_census: NULL context");
    c->sgm.cen_w = win_w;
    c->sgm.cen_h = win_h;
    return 0;
}

int psm_sgm_set_mode(psm_ctx *c, int mode)
{
    if (mode < 0 || mode > 3)                  // (without a context the message is psm_last_error(NULL)'s)
        return fail(c, "psm_sgm_set_mode: mode %d not in {0: MODE_SGBM, 1: MODE_HH, 2: MODE_SGBM_3WAY, 3: MODE_HH4}", mode);
    if (!c) return fail(nullptr, "psm_sgm_set_mode: NULL context");
    c->sgm.mode = mode;
    return 0;
}

int psm_sgm_set_range(psm_ctx *c, int min_disparity, int num_disparities)
{
    if (min_disparity < -1024 || min_disparity > 1024)      // (without a context the message is psm_last_error(NULL)'s)
        return fail(c, "psm_sgm_set_range: min_disparity %d outside [-1024, 1024]", min_disparity);
    if (num_disparities != 0 && (num_disparities < 2 || num_disparities > SGM_DMAX))
        return fail(c, "psm_sgm_set_range: num_disparities %d neither 0 (the context's max_disp) nor in [2, %d]", num_disparities, SGM_DMAX);
    if (!c) return fail(nullptr, "psm_sgm_set_range: NULL context");
    c->sgm.dmin = min_disparity;
    c->sgm.nd = num_disparities;
    return 0;
}

int psm_sgm_compute(psm_ctx *c)
{
    if (!c) return 1;
    if (check_ctx(c, c, "psm_sgm_compute") || check_cost(c, c, "psm_sgm_compute")) return 1;
    const PairSlots &p = c->pair;
    if (p.st.depth < 0) return fail(c, "psm_sgm_compute: no image pair (psm_upload_pair)");
    if (bind(c)) return 1;
    return compute_one(c, "psm_sgm_compute", p.raw[0], p.raw[1], p.st.depth, 3, true);
}

int psm_sgm_compute_gray(psm_ctx *c, const uint8_t *l, const uint8_t *r, size_t stride_bytes)
{
    if (!c) return 1;
    if (check_ctx(c, c, "psm_sgm_compute_gray") || check_cost(c, c, "psm_sgm_compute_gray")) return 1;
    if (!l || !r) return fail(c, "psm_sgm_compute_gray: NULL image");
    const size_t row = (size_t)c->W;
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row) return fail(c, "psm_sgm_compute_gray: stride %zu < row size %zu", stride_bytes, row);
    if (bind(c)) return 1;
    SgmState &g = c->sgm;
    const uint8_t *src[2] = {l, r};
    for (int s = 0; s < 2; ++s) {
        if (!g.gray[s]) PSM_HIP(c, hipMalloc((void **)&g.gray[s], row * c->H));
        if (h2d_rows(c, g.gray[s], src[s], row, stride_bytes, c->H)) return 1;
    }
    PSM_HIP(c, hipStreamSynchronize(c->stream));      // the copy reads caller memory (psm_upload_pair)
    return compute_one(c, "psm_sgm_compute_gray", g.gray[0], g.gray[1], PSM_IMG_U8, 1, false);
}

// The launches of psm_sgm_compute with the pair on a grid axis of its own: n x (H, W or W + H - 1) one-wave paths per path launch
// instead of one pair's 375 to 824 on 1024 SIMDs ("several pairs per launch").  Buffers stay per context; the kernels
// reach them through a device table ctxs[0] owns.  Every context ends where its own psm_sgm_compute would have left it.
int psm_sgm_compute_batch(psm_ctx *const *ctxs, int n)
{
    const char *who = "psm_sgm_compute_batch";
    if (!ctxs || n < 1 || !ctxs[0]) return fail(nullptr, "%s: bad arguments", who);
    psm_ctx *c0 = ctxs[0];
    if (n > 4096) return fail(c0, "%s: %d pairs (at most 4096 per call)", who, n);
    const SgmState &g0 = c0->sgm;
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        psm_ctx *c = ctxs[i];
        if (c->W != c0->W || c->H != c0->H || c->D != c0->D || c->device != c0->device)
            return fail(c0, "%s: context %d has another width / height / max_disp / device than context 0", who, i);
        char member[64];
        snprintf(member, sizeof member, "%s: context %d", who, i);
        if (check_ctx(c0, c, member) || check_cost(c0, c, member)) return 1;
        if (c->pair.st.depth < 0) return fail(c0, "%s: context %d has no image pair (psm_upload_pair)", who, i);
        if (c->pair.st.depth != c0->pair.st.depth) return fail(c0, "%s: context %d holds images of another depth than context 0", who, i);
        const SgmState &g = c->sgm;
        if (g.bs != g0.bs || g.p1 != g0.p1 || g.p2 != g0.p2 || g.u != g0.u || g.m != g0.m)
            return fail(c0, "%s: context %d has other parameters (psm_sgm_set_params) than context 0", who, i);
        if (g.cap != g0.cap) return fail(c0, "%s: context %d has another pre_filter_cap (%d) than context 0 (%d)", who, i, g.cap, g0.cap);
        if (g.cen_w != g0.cen_w || g.cen_h != g0.cen_h)
            return fail(c0, "%s: context %d has another census window (%d x %d) than context 0 (%d x %d)", who, i, g.cen_w, g.cen_h, g0.cen_w, g0.cen_h);
        if (g.mode != g0.mode) return fail(c0, "%s: context %d has another mode (%d) than context 0 (%d)", who, i, g.mode, g0.mode);
        if (g.dmin != g0.dmin || sgm_d(c) != sgm_d(c0))
            return fail(c0, "%s: context %d has another disparity range (min %d, %d disparities) than context 0 (min %d, %d)", who, i, g.dmin,
                        sgm_d(c), g0.dmin, sgm_d(c0));
        if (g.spk_window != g0.spk_window || g.spk_range != g0.spk_range)
            return fail(c0, "%s: context %d has another speckle window / range (%d, %d) than context 0 (%d, %d)", who, i, g.spk_window,
                        g.spk_range, g0.spk_window, g0.spk_range);
    }
    int p1 = g0.p1, p2 = g0.p2;
    if (check_params(c0, who, 3, g0.bs, &p1, &p2, g0.u)) return 1;      // (every context's: they are context 0's)
    if (bind(c0)) return 1;
    hipStream_t s = c0->stream;

    // ---- buffers, events and the table's memory: before any launch, and before any context forgets its previous result ----
    for (int i = 0; i < n; ++i)
        if (ensure_buffers(ctxs[i])) return member_failed(c0, who, i, ctxs[i]);
    if (batch_events(c0, ctxs, n)) return 1;
    DevTable &t = c0->sgm.tab;
    const std::vector<SgmPair> tab = pairs_of(ctxs, n);
    bool fresh = false;
    if (table_reserve(c0, t, tab.data(), tab.size() * sizeof(SgmPair), &fresh)) return 1;

    // ---- every context's earlier work (uploads, a single compute, downloads) is ordered before the shared launches ----
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, t, tab.data(), tab.size() * sizeof(SgmPair))) return 1;

    // ---- the launches; then every context is where its own psm_sgm_compute would have left it - only context 0 counts as timed ----
    const SgmArgs a = sgm_args(c0, c0->pair.st.depth, 3, p1, p2);
    for (int i = 0; i < n; ++i) forget(ctxs[i]->sgm);
    if (enqueue(c0, s, a, Recs<SgmPair>{tab.data(), (const SgmPair *)t.dev, n}, ctxs)) return 1;
    if (batch_fork(c0, ctxs, n)) return 1;
    for (int i = 0; i < n; ++i) mark(ctxs[i]->sgm, cost_kind(g0), 3, a.dmin, a.D, i == 0 && c0->opt_profile != 0);
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(s));
    return 0;
}

// The 8-bit maps of both views from the S of the last compute, into the context's map buffer (k_sgm_maps, tests/sgm_maps_model.py):
// one launch; the int16 map, C, S, disp2 and the speckle planes are read-only or untouched.
int psm_sgm_select_maps(psm_ctx *c, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    const char *who = "psm_sgm_select_maps";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_maps(c, c, who)) return 1;
    if (stride != 0 && stride < (size_t)c->W) return fail(c, "%s: stride %zu < width %d", who, stride, c->W);
    if (maps_run(&c, 1, false)) return 1;
    if (copy_maps_out(c, c->maps, lmap, rmap, stride)) return 1;
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ... of the n contexts ctxs[0..n) in one launch on ctxs[0]'s stream (maps_run), ordered as psm_sgm_compute_batch's
int psm_sgm_select_maps_batch(psm_ctx *const *ctxs, int n)
{
    const char *who = "psm_sgm_select_maps_batch";
    if (!ctxs || n < 1 || !ctxs[0]) return fail(nullptr, "%s: bad arguments", who);
    psm_ctx *c0 = ctxs[0];
    if (n > 4096) return fail(c0, "%s: %d pairs (at most 4096 per call)", who, n);
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        psm_ctx *c = ctxs[i];
        if (c->W != c0->W || c->H != c0->H || c->D != c0->D || c->device != c0->device)
            return fail(c0, "%s: context %d has another width / height / max_disp / device than context 0", who, i);
        char member[64];
        snprintf(member, sizeof member, "%s: context %d", who, i);
        if (check_maps(c0, c, member)) return 1;
        if (c->sgm.res_dmin != c0->sgm.res_dmin || c->sgm.res_d != c0->sgm.res_d)
            return fail(c0, "%s: the result of context %d has another disparity range (min %d, %d disparities) than context 0's (min %d, %d)", who, i,
                        c->sgm.res_dmin, c->sgm.res_d, c0->sgm.res_dmin, c0->sgm.res_d);
    }
    if (maps_run(ctxs, n, true)) return 1;
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(c0->stream));
    return 0;
}

int psm_sgm_maps_time(psm_ctx *c, double *ms)
{
    if (!c) return fail(nullptr, "psm_sgm_maps_time: NULL context");
    return bracket_ms(c, c->sgm.maps, true, "psm_sgm_maps_time", "the last psm_sgm_select_maps was not timed (PSM_OPT_PROFILE), or there is none", ms);
}

int psm_sgm_download_disparity(psm_ctx *c, int16_t *disp, size_t stride_bytes)
{
    if (!c) return 1;
    if (!disp) return fail(c, "psm_sgm_download_disparity: NULL map");
    if (!c->sgm.have) return fail(c, "psm_sgm_download_disparity: no result (psm_sgm_compute)");
    const size_t row = (size_t)c->W * sizeof(int16_t);
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row) return fail(c, "psm_sgm_download_disparity: stride %zu < row size %zu", stride_bytes, row);
    if (bind(c)) return 1;
    return d2h_rows(c, disp, c->sgm.out, row, stride_bytes, c->H);
}

int psm_sgm_download_costs(psm_ctx *c, int which, void *host)
{
    if (!c) return 1;
    if (!host) return fail(c, "psm_sgm_download_costs: NULL buffer");
    if (which != 0 && which != 1) return fail(c, "psm_sgm_download_costs: which %d (0: C as u16, 1: S as u32)", which);
    if (!c->sgm.have) return fail(c, "psm_sgm_download_costs: no result (psm_sgm_compute)");
    if (bind(c)) return 1;
    const size_t HW = (size_t)c->W * c->H, Dp = psm::sgm_dp(c->sgm.res_d), D = c->sgm.res_d, el = which ? sizeof(uint32_t) : sizeof(uint16_t);
    std::vector<uint8_t> dev(HW * Dp * el);
    PSM_HIP(c, hipMemcpyAsync(dev.data(), which ? (const void *)c->sgm.S : (const void *)c->sgm.C, dev.size(), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t p = 0; p < HW; ++p) memcpy((uint8_t *)host + p * D * el, dev.data() + p * Dp * el, D * el);      // the host layout has no padding
    return 0;
}

int psm_sgm_download_prefiltered(psm_ctx *c, int side, uint8_t *planes)
{
    if (!c) return 1;
    if (!planes) return fail(c, "psm_sgm_download_prefiltered: NULL buffer");
    if (side != 0 && side != 1) return fail(c, "psm_sgm_download_prefiltered: side %d (0: left, 1: right)", side);
    if (!c->sgm.have || c->sgm.pf_ch == 0)
        return fail(c, "psm_sgm_download_prefiltered: the last psm_sgm_compute prefiltered nothing (psm_sgm_set_prefilter), or there is none");
    if (bind(c)) return 1;
    PSM_HIP(c, hipMemcpyAsync(planes, c->sgm.pf[side], (size_t)c->W * c->H * 2 * c->sgm.pf_ch, hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int psm_sgm_download_census(psm_ctx *c, int side, uint64_t *codes)
{
    if (!c) return 1;
    if (!codes) return fail(c, "psm_sgm_download_census: NULL buffer");
    if (side != 0 && side != 1) return fail(c, "psm_sgm_download_census: side %d (0: left, 1: right)", side);
    if (!c->sgm.have || !c->sgm.cen_have)
        return fail(c, "psm_sgm_download_census: the last psm_sgm_compute ran another pixel cost (psm_sgm_set_census), or there is none");
    if (bind(c)) return 1;
    PSM_HIP(c, hipMemcpyAsync(codes, c->sgm.cen[side], (size_t)c->W * c->H * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int psm_sgm_times(psm_ctx *c, double ms[3])
{
    if (!c) return 1;
    if (!ms) return fail(c, "psm_sgm_times: NULL array");
    if (!c->sgm.have || !c->sgm.timed) return fail(c, "psm_sgm_times: the last psm_sgm_compute was not timed (PSM_OPT_PROFILE)");
    if (bind(c)) return 1;
    PSM_HIP(c, hipEventSynchronize(c->sgm.ev[3]));
    for (int i = 0; i < 3; ++i) {
        float t = 0.f;
        PSM_HIP(c, hipEventElapsedTime(&t, c->sgm.ev[i], c->sgm.ev[i + 1]));
        ms[i] = t;
    }
    return 0;
}

int psm_sgm_filter_speckles(psm_ctx *c, int16_t *disp, size_t stride_bytes, int new_val, int max_speckle_size, int max_diff)
{
    if (!c) return 1;
    if (!disp) return fail(c, "psm_sgm_filter_speckles: NULL map");
    if (new_val < -32768 || new_val > 32767) return fail(c, "psm_sgm_filter_speckles: new_val %d is no int16 value", new_val);
    if (max_speckle_size < 0) return fail(c, "psm_sgm_filter_speckles: max_speckle_size %d negative", max_speckle_size);
    if (max_diff < 0) return fail(c, "psm_sgm_filter_speckles: max_diff %d negative", max_diff);
    const size_t row = (size_t)c->W * sizeof(int16_t);
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row) return fail(c, "psm_sgm_filter_speckles: stride %zu < row size %zu", stride_bytes, row);
    if (bind(c)) return 1;
    SgmState &g = c->sgm;
    const bool timed = c->opt_profile != 0;
    if (timed)
        for (int i = 4; i < 6; ++i)
            if (!g.ev[i]) PSM_HIP(c, hipEventCreate(&g.ev[i]));
    // the map lives in a plane of this call: the stage's own map and volumes are not touched, and the filter holds no more than
    // its 8 W H bytes between calls
    int16_t *map = nullptr;
    PSM_HIP(c, hipMalloc((void **)&map, row * c->H));
    int rc = h2d_rows(c, map, disp, row, stride_bytes, c->H);
    if (!rc && timed) rc = hipEventRecord(g.ev[5], c->stream) != hipSuccess ? fail(c, "psm_sgm_filter_speckles: hipEventRecord") : 0;
    if (!rc) rc = ensure_speckle_planes(c);
    if (!rc) {
        SgmPair p = {};
        p.out = map; p.spk_label = g.spk_label; p.spk_size = g.spk_size;
        g.spk_have = false;
        g.spk_t0 = -1;
        rc = enqueue_speckle(c, c->stream, speckle_args(c, new_val, max_speckle_size, max_diff), Recs<SgmPair>{&p, nullptr, 1}, timed);
        if (!rc) {
            g.spk_have = true;
            g.spk_t0 = timed ? 5 : -1;
        }
    }
    // the filter has run before anything is written to the caller's map: a failure up to here leaves it untouched
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(c, "psm_sgm_filter_speckles: hipStreamSynchronize");
    if (!rc) rc = d2h_rows(c, disp, map, row, stride_bytes, c->H);
    (void)hipFree(map);
    return rc;
}

int psm_sgm_download_speckle_sizes(psm_ctx *c, int32_t *sizes, size_t stride_bytes)
{
    if (!c) return 1;
    if (!sizes) return fail(c, "psm_sgm_download_speckle_sizes: NULL plane");
    if (!c->sgm.spk_have) return fail(c, "psm_sgm_download_speckle_sizes: no filter run (psm_sgm_set_speckle + psm_sgm_compute, psm_sgm_filter_speckles)");
    const size_t row = (size_t)c->W * sizeof(int32_t);
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row) return fail(c, "psm_sgm_download_speckle_sizes: stride %zu < row size %zu", stride_bytes, row);
    if (bind(c)) return 1;
    return d2h_rows(c, sizes, c->sgm.spk_size, row, stride_bytes, c->H);
}

int psm_sgm_speckle_time(psm_ctx *c, double *ms)
{
    if (!c) return 1;
    if (!ms) return fail(c, "psm_sgm_speckle_time: NULL pointer");
    if (!c->sgm.spk_have || c->sgm.spk_t0 < 0)
        return fail(c, "psm_sgm_speckle_time: the last compute did not run the speckle filter, or was not timed (psm_sgm_set_speckle, PSM_OPT_PROFILE)");
    if (bind(c)) return 1;
    PSM_HIP(c, hipEventSynchronize(c->sgm.ev[4]));
    float t = 0.f;
    PSM_HIP(c, hipEventElapsedTime(&t, c->sgm.ev[c->sgm.spk_t0], c->sgm.ev[4]));
    *ms = t;
    return 0;
}

}  // extern "C"
