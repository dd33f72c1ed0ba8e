// psm_api_pp.cpp - the post-processing rows behind the C ABI: lrCheck, fillInv and the plain weighted
// median of PP::processDM (src/PP.cpp:17-247,405-410) on the device maps of the last DispSelect.  The reference runs these
// on the CPU; here they sit behind the same boundary so that the maps never leave the device between the stages.
// The weighted median keeps its scratch in psm::WmState (psm_ctx.h; wm_free); the layout of its sweep block, the schedule of its
// sweeps and its cache decision are psm_wm_sched.h, which tests/test_wm_sched.py checks on the host against a model of the rules.
// psm_post_process_batch runs the three stages for several contexts in shared launches: the same steps, the pair on a grid axis of
// its own, the members' records in a device table of the batch's first context (psm::WmBatch) and one schedule for all their maps
// (WmBatchSched; tests/test_wm_batch_sched.py).
#include "psm_ctx.h"

using namespace psm;

// ---- The plain weighted median: psm::WmState between calls, WmRun within a call of the sweep form ----
namespace psm {

void wm_free(psm_ctx *c, bool all)
{
    WmState &m = c->wm;
    (void)hipFree(m.wts); m.wts = nullptr; m.wts_n = 0;
    (void)hipFree(m.block); m.block = nullptr;
    (void)hipFree(m.flow); m.flow = nullptr;
    WmBatch &b = c->wmb;                   // (as the first of a psm_post_process_batch: rebuilt by the next such call)
    table_free(b.tab);
    (void)hipFree(b.cnt); b.cnt = nullptr;
    if (b.pin) { (void)hipHostFree(b.pin); b.pin = nullptr; }
    b.cap = 0;
    if (!all) return;
    if (m.pin) { (void)hipHostFree(m.pin); m.pin = nullptr; }
    for (hipEvent_t &e : m.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    for (hipEvent_t &e : b.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

// The row-dataflow form of wgtMedian: exact for any input, but as sequential as the reference wherever invalid pixels chain
static int wgt_median_dataflow(psm_ctx *c, int side)
{
    const size_t HW = (size_t)c->W * c->H, nn = (size_t)c->H * (c->W + 1);
    if (!c->wm.flow) PSM_HIP(c, hipMalloc((void **)&c->wm.flow, (nn + c->H + 1) * sizeof(int)));
    int *nxt = c->wm.flow, *prog = nxt + nn, *err = prog + c->H;
    PSM_HIP(c, hipMemsetAsync(err, 0, sizeof(int), c->stream));
    {
        Prof p(c, PSM_K_WMF);
        launch_wgt_median(c->stream, c->maps + side * HW, c->valid + side * HW, c->g[side].g1, c->W, c->H, c->D, side, nxt, prog, err);
    }
    if (check_launch(c, "wgt_median")) return 1;
    int herr = 0;
    PSM_HIP(c, hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    if (herr) {
        // the kernel gave up on unfinished rows: the in-place maps are partially filtered - not results
        maps_gone(c->res);
        return fail(c, "psm_wgt_median: row pipeline stalled (watchdog); the device maps are no longer valid - select again");
    }
    return 0;
}

// The parallel form: sweeps to the fixed point of the in-place recursion (psm_pp.hip), both maps side by side
struct WmRun {
    WmPair pr;             // the parts of the block, as the kernels take them
    int *cnt;              // the counters of both maps
    size_t snap;           // ints per snapshot of them
    bool cached = false;   // both maps have their weight cache
};

// the block, the page-locked snapshots and the events, on first use; r: what the block holds where
static int wm_scratch(psm_ctx *c, WmRun &r)
{
    WmState &m = c->wm;
    const size_t HW = (size_t)c->W * c->H;
    const WmLayout l = wm_layout(HW);
    if (!m.block) PSM_HIP(c, hipMalloc((void **)&m.block, l.bytes));
    if (!m.pin) PSM_HIP(c, hipHostMalloc((void **)&m.pin, 2 * l.snap * sizeof(int), hipHostMallocDefault));
    for (hipEvent_t &e : m.ev)
        if (!e) PSM_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    auto ints = [&](size_t at) { return reinterpret_cast<int *>(m.block + at); };
    for (int s = 0; s < 2; ++s) {
        const WmSideAt &at = l.s[s];
        WmSide &a = r.pr.s[s];
        a.cur = c->maps + s * HW; a.valid = c->valid + s * HW; a.g1 = c->g[s].g1;
        a.orig = m.block + at.orig; a.newv = m.block + at.newv; a.chgb = m.block + at.chgb; a.rowany = m.block + at.rowany;
        a.stamp = ints(at.stamp); a.list[0] = ints(at.list[0]); a.list[1] = ints(at.list[1]); a.chg = ints(at.chg);
        a.slot_of = ints(at.slot_of); a.inv = ints(at.inv); a.cnt = ints(at.cnt); a.wts = nullptr;
    }
    r.cnt = ints(l.cnt); r.snap = l.snap;
    return 0;
}

// The weight cache (wm_cache_plan), grown on demand, and the pass that fills it
static int wm_cache(psm_ctx *c, WmRun &r)
{
    WmState &m = c->wm;
    size_t mem_free = 0, mem_total = 0, avail = SIZE_MAX;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) avail = mem_free + m.wts_n * sizeof(float);   // (what we hold already counts as available to us)
    else (void)hipGetLastError();
    // (the counts of invalid pixels through the same page-locked snapshot the sweeps use: one small kernel, no copy engine; the
    // host reads them next, so this one snapshot is waited for)
    launch_copy_bytes(c->stream, m.pin, r.cnt, r.snap * sizeof(int));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    const int n0[2] = {wm_active(wm_counters(m.pin, 0), 0), wm_active(wm_counters(m.pin, 1), 0)};
    const WmCachePlan plan = wm_cache_plan(n0, avail, c->march.flags);
    if (!plan.floats) return 0;
    if (m.wts_n < plan.floats) {
        (void)hipFree(m.wts); m.wts = nullptr; m.wts_n = 0;
        if (hipMalloc((void **)&m.wts, plan.floats * sizeof(float)) == hipSuccess) m.wts_n = plan.floats;
        else (void)hipGetLastError();           // no memory for it: recompute, as without the cache
    }
    if (m.wts_n < plan.floats) return 0;
    r.cached = true;
    Prof p(c, PSM_K_WMF);
    for (int s = 0; s < 2; ++s) {
        WmSide &a = r.pr.s[s];
        float *wts = s ? m.wts + plan.right : m.wts;
        a.wts = wts;
        if (n0[s]) launch_wm_weights(c->stream, c->g[s].g1, c->W, c->H, s, a.inv, a.cnt, n0[s], wts, a.slot_of);
    }
    return 0;
}

// the schedule's next group of sweeps, and behind it the snapshot of the counters into `slot`
static int wm_launch_group(psm_ctx *c, const WmRun &r, WmSched &sch, int slot)
{
    const WmGroup g = sch.next_group();
    {
        Prof p(c, PSM_K_WMF);
        // (a map that has reached its fixed point has empty lists from then on: its half of a launch returns at once)
        for (int sw = g.begin; sw < g.end; ++sw) launch_wm_sweep(c->stream, r.pr, c->W, c->H, c->D, sw, r.cached, g.short_lists);
    }
    if (check_launch(c, "wgt_median (sweeps)")) return 1;
    // (a kernel writing the page-locked snapshot: a copy-engine transfer in the stream stalls it for ~60 us)
    launch_copy_bytes(c->stream, c->wm.pin + slot * r.snap, r.cnt, r.snap * sizeof(int));
    PSM_HIP(c, hipEventRecord(c->wm.ev[slot], c->stream));
    sch.launched(g, slot);
    return 0;
}

static int wm_sweeps(psm_ctx *c, const WmRun &r, WmSched &sch)
{
    if (wm_launch_group(c, r, sch, 0)) return 1;
    for (int g = 0;; ++g) {
        if (sch.more() && wm_launch_group(c, r, sch, (g + 1) & 1)) return 1;      // (queued before this group's counters are looked at)
        PSM_HIP(c, hipEventSynchronize(c->wm.ev[g & 1]));
        if (!sch.read(g & 1, c->wm.pin + (g & 1) * r.snap)) break;
    }
#ifdef PSM_EXPERIMENTS
    if (getenv("PSM_WM_TRACE")) {      // per sweep: pixels evaluated / changed (both maps)
        std::vector<int> hc(2 * WM_NCNT);
        PSM_HIP(c, hipMemcpy(hc.data(), r.cnt, hc.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int s = 0; s < 2; ++s) {
            const int *cnt = wm_counters(hc.data(), s);
            fprintf(stderr, "[wm] side %d:", s);
            for (int k = 0; k < sch.sw && k < WM_SWEEP_CAP; ++k) fprintf(stderr, " %d/%d", wm_active(cnt, k), wm_changed(cnt, k));
            fprintf(stderr, "\n");
        }
    }
#endif
    return 0;
}

// ---- The three stages for the members of a batch (psm_post_process_batch): the single call's steps, each launch
// once for all pairs through the device table of c0 ----
struct WmBatchRun {
    psm_ctx *c0;
    psm_ctx *const *ctxs;
    int n;
    const PpPair *dt;      // the device table
    size_t snap;           // ints per snapshot: the counters of all 2 n maps
    bool cached = false;
};

// the counters of all maps and their page-locked snapshots, for at least `maps` maps; the events
static int wm_batch_block(psm_ctx *c0, size_t maps)
{
    WmBatch &b = c0->wmb;
    if (b.cap < maps) {
        PSM_HIP(c0, hipStreamSynchronize(c0->stream));     // (kernels of an earlier call may still count in the old block)
        (void)hipFree(b.cnt); b.cnt = nullptr;
        if (b.pin) { (void)hipHostFree(b.pin); b.pin = nullptr; }
        b.cap = 0;
        PSM_HIP(c0, hipMalloc((void **)&b.cnt, maps * WM_NCNT * sizeof(int)));
        PSM_HIP(c0, hipHostMalloc((void **)&b.pin, 2 * maps * WM_NCNT * sizeof(int), hipHostMallocDefault));
        b.cap = maps;
    }
    for (hipEvent_t &e : b.ev)
        if (!e) PSM_HIP(c0, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return 0;
}

// The batch-wide cache decision (wm_batch_cache_plan) and the pass that fills every side's weights.  recs: the table's records, which
// gain their wts here; *changed: they did, and the table must be uploaded again before the next launch.
static int wm_batch_cache(WmBatchRun &r, std::vector<PpPair> &recs, bool *changed)
{
    psm_ctx *c0 = r.c0;
    WmBatch &b = c0->wmb;
    const int m = 2 * r.n;
    size_t mem_free = 0, mem_total = 0, avail = SIZE_MAX;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) {
        avail = mem_free;
        for (int i = 0; i < r.n; ++i) avail += r.ctxs[i]->wm.wts_n * sizeof(float);     // (what the members hold already counts as available)
    } else (void)hipGetLastError();
    launch_copy_bytes(c0->stream, b.pin, b.cnt, r.snap * sizeof(int));
    PSM_HIP(c0, hipStreamSynchronize(c0->stream));
    std::vector<int> n0((size_t)m);
    for (int i = 0; i < m; ++i) n0[i] = wm_active(wm_counters(b.pin, i), 0);
    if (!wm_batch_cache_plan(n0.data(), m, avail, c0->march.flags)) return 0;
    bool fits = true;
    for (int i = 0; i < r.n && fits; ++i) {
        WmState &w = r.ctxs[i]->wm;
        const size_t need = wm_side_need(n0[2 * i]) + wm_side_need(n0[2 * i + 1]);
        if (w.wts_n < need) {
            (void)hipFree(w.wts); w.wts = nullptr; w.wts_n = 0;
            if (hipMalloc((void **)&w.wts, need * sizeof(float)) == hipSuccess) w.wts_n = need;
            else { (void)hipGetLastError(); fits = false; }     // no memory for it: the whole batch recomputes, as without the cache
        }
    }
    if (!fits) return 0;
    for (int i = 0; i < r.n; ++i) {
        WmState &w = r.ctxs[i]->wm;
        recs[i].wm.s[0].wts = w.wts;
        recs[i].wm.s[1].wts = w.wts + wm_side_need(n0[2 * i]);
    }
    r.cached = true;
    *changed = true;
    return 0;
}

static int wm_batch_launch_group(WmBatchRun &r, WmBatchSched &sch, int slot)
{
    psm_ctx *c0 = r.c0;
    const WmGroup g = sch.next_group();
    {
        Prof p(c0, PSM_K_WMF);
        for (int sw = g.begin; sw < g.end; ++sw) launch_wm_sweep_b(c0->stream, r.dt, r.n, c0->W, c0->H, c0->D, sw, r.cached, g.short_lists);
    }
    if (check_launch(c0, "post_process_batch (sweeps)")) return 1;
    launch_copy_bytes(c0->stream, c0->wmb.pin + slot * r.snap, c0->wmb.cnt, r.snap * sizeof(int));
    PSM_HIP(c0, hipEventRecord(c0->wmb.ev[slot], c0->stream));
    sch.launched(g, slot);
    return 0;
}

static int wm_batch_sweeps(WmBatchRun &r, WmBatchSched &sch)
{
    psm_ctx *c0 = r.c0;
    if (wm_batch_launch_group(r, sch, 0)) return 1;
    for (int g = 0;; ++g) {
        if (sch.more() && wm_batch_launch_group(r, sch, (g + 1) & 1)) return 1;
        PSM_HIP(c0, hipEventSynchronize(c0->wmb.ev[g & 1]));
        if (!sch.read(g & 1, c0->wmb.pin + (g & 1) * r.snap)) break;
    }
    return 0;
}

}  // namespace psm

extern "C" {

int psm_post_process_batch(psm_ctx *const *ctxs, int n, int stages)
{
    const char *who = "psm_post_process_batch";
    if (!ctxs || n < 1 || !ctxs[0]) return fail(nullptr, "%s: bad arguments", who);
    psm_ctx *c0 = ctxs[0];
    if (n > 4096) return fail(c0, "%s: %d pairs (at most 4096 per call)", who, n);
    const int all_stages = PSM_PP_LR_CHECK | PSM_PP_FILL | PSM_PP_WGT_MEDIAN;
    if (!stages || (stages & ~all_stages)) return fail(c0, "%s: stages %d name none of, or more than, PSM_PP_LR_CHECK | PSM_PP_FILL | PSM_PP_WGT_MEDIAN", who, stages);
    const bool lrc = stages & PSM_PP_LR_CHECK, fill = stages & PSM_PP_FILL, med = stages & PSM_PP_WGT_MEDIAN;
    const unsigned wmf_bits = PSM_FLAG_WMF_DATAFLOW | PSM_FLAG_WMF_NO_CACHE | PSM_FLAG_WMF_TWO_SWEEPS;
    // ---- refused before anything is allocated, ordered or launched ----
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        const psm_ctx *c = ctxs[i];
        if (c->W != c0->W || c->H != c0->H || c->D != c0->D || c->device != c0->device)
            return fail(c0, "%s: context %d has another geometry / max_disp / device than context 0", who, i);
        if ((c->march.flags & wmf_bits) != (c0->march.flags & wmf_bits))
            return fail(c0, "%s: context %d has other weighted-median flags than context 0", who, i);
        if (c->pair.st.depth != c0->pair.st.depth) return fail(c0, "%s: context %d holds images of another depth than context 0", who, i);
        if (!c->res.maps) return fail(c0, "%s: context %d has no disparity maps", who, i);
        if (stripe_only(c)) return fail(c0, "%s: the maps of context %d hold its row stripe only (gather the stripes first)", who, i);
        if (!lrc && !c->res.mask) return fail(c0, "%s: context %d has no current mask (psm_lr_check, or PSM_PP_LR_CHECK among the stages)", who, i);
        if (med && !c->have_images) return fail(c0, "%s: context %d has no image pair uploaded (colour weights)", who, i);
        if (med && (c->W < 9 || c->H < 9))
            return fail(c0, "%s: context %d: image %dx%d smaller than the 19x19 window's wrap allows", who, i, c->W, c->H);
    }
    if (bind(c0)) return 1;
    const double t0 = now_us();
    const int W = c0->W, H = c0->H;
    const size_t HW = (size_t)W * H;
    hipStream_t s = c0->stream;
    const bool sweeps = med && !(c0->march.flags & PSM_FLAG_WMF_DATAFLOW);

    // ---- scratch, events and the table's memory: before any launch (growing synchronises) ----
    std::vector<PpPair> recs((size_t)n);
    WmBatchRun r{c0, ctxs, n, nullptr, 2 * (size_t)n * WM_NCNT};
    if (sweeps && wm_batch_block(c0, 2 * (size_t)n)) return 1;
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        PpPair &p = recs[i];
        memset(&p, 0, sizeof p);                 // (padding too: table_reserve compares bytes)
        if (sweeps) {
            WmRun own;
            if (wm_scratch(c, own)) return member_failed(c0, who, i, c);
            p.wm = own.pr;
            for (int sd = 0; sd < 2; ++sd) p.wm.s[sd].cnt = c0->wmb.cnt + (2 * (size_t)i + sd) * WM_NCNT;
        } else {
            for (int sd = 0; sd < 2; ++sd) { p.wm.s[sd].cur = c->maps + sd * HW; p.wm.s[sd].valid = c->valid + sd * HW; }
        }
        p.lv = c->valid; p.rv = c->valid + HW;
    }
    if (batch_events(c0, ctxs, n)) return 1;
    bool fresh = false;
    const size_t tab_bytes = recs.size() * sizeof(PpPair);
    if (table_reserve(c0, c0->wmb.tab, recs.data(), tab_bytes, &fresh)) return 1;
    r.dt = (const PpPair *)c0->wmb.tab.dev;

    // ---- every member's earlier work is ordered before the shared launches; the planes the weights read ----
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if ((fill || med) && maps_writable(c)) return member_failed(c0, who, i, c);
        if (med && ensure_planes(c, whole_image(c), Rows{})) return member_failed(c0, who, i, c);
        if (sweeps) for (int sd = 0; sd < 2; ++sd) recs[i].wm.s[sd].g1 = c->g[sd].g1;      // (allocated by ensure_planes at the latest)
    }
    if (sweeps) fresh = fresh || c0->wmb.tab.host.size() != tab_bytes || memcmp(c0->wmb.tab.host.data(), recs.data(), tab_bytes) != 0;
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, c0->wmb.tab, recs.data(), tab_bytes)) return 1;

    if (lrc) {
        {
            Prof p(c0, PSM_K_LRC);
            launch_lr_check_b(s, r.dt, n, W, H);
        }
        if (check_launch(c0, "post_process_batch (lr_check)")) return 1;
        for (int i = 0; i < n; ++i) mask_written(ctxs[i]->res);
    }
    if (fill) {
        {
            Prof p(c0, PSM_K_LRC);
            launch_fill_inv_b(s, r.dt, n, W, H);
        }
        if (check_launch(c0, "post_process_batch (fill_inv)")) return 1;
    }
    if (med) {
        WmBatchSched sch(2 * n, c0->march.flags);
        if (sweeps) {
            PSM_HIP(c0, hipMemsetAsync(c0->wmb.cnt, 0, r.snap * sizeof(int), s));
            launch_wm_seed_b(s, r.dt, n, W, H);
            bool changed = false;
            if (wm_batch_cache(r, recs, &changed)) return 1;
            if (changed) {
                // (every side's wts: the records differ from the table the seed read - which the host has waited for)
                if (table_upload(c0, c0->wmb.tab, recs.data(), tab_bytes)) return 1;
                int n_max = 0;
                for (int i = 0; i < 2 * n; ++i) { const int v = wm_active(wm_counters(c0->wmb.pin, i), 0); if (v > n_max) n_max = v; }
                Prof p(c0, PSM_K_WMF);
                launch_wm_weights_b(s, r.dt, n, W, H, n_max);
            }
            if (wm_batch_sweeps(r, sch)) return 1;
            for (int q = 0; q < 2 * n; ++q)
                if (!sch.done[q]) PSM_HIP(c0, hipMemcpyAsync(ctxs[q / 2]->maps + (q & 1) * HW, recs[q / 2].wm.s[q & 1].orig, HW, hipMemcpyDeviceToDevice, s));
        }
        // maps that left the sweeps at the cap (or every map: PSM_FLAG_WMF_DATAFLOW): the dataflow form, one by one, on c0's stream
        for (int q = 0; q < 2 * n; ++q) {
            psm_ctx *c = ctxs[q / 2];
            if (!sch.done[q]) {
                hipStream_t own = c->stream;
                c->stream = s;
                const int bad = wgt_median_dataflow(c, q & 1);
                c->stream = own;
                if (bad) return member_failed(c0, who, q / 2, c);
            }
            c->wm.sweeps[q & 1] = sch.sweeps[q]; c->wm.evals[q & 1] = sch.evals[q];
        }
    }
    if (batch_fork(c0, ctxs, n)) return 1;
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(s));      // (the median has waited for its snapshots either way)
    const double dt_us = now_us() - t0;
    for (int i = 0; i < n; ++i) ctxs[i]->stage_us[PSM_STAGE_PP] = dt_us;
    return 0;
}

int psm_lr_check(psm_ctx *c, uint8_t *lvalid, uint8_t *rvalid, size_t stride)
{
    if (!c) return 1;
    if (!c->res.maps) return fail(c, "psm_lr_check: no disparity maps computed");
    if (stripe_only(c)) return fail(c, "psm_lr_check: the maps hold this context's row stripe only (gather the stripes first)");
    if (bind(c)) return 1;
    const double t0 = now_us();
    const size_t HW = (size_t)c->W * c->H;
    {
        Prof p(c, PSM_K_LRC);
        launch_lr_check(c->stream, c->maps, c->maps + HW, c->W, c->H, c->valid, c->valid + HW);
    }
    if (check_launch(c, "lr_check")) return 1;
    mask_written(c->res);
    if (copy_maps_out(c, c->valid, lvalid, rvalid, stride)) return 1;
    return end_stage(c, PSM_STAGE_PP, t0);
}

int psm_fill_invalid(psm_ctx *c, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    if (!c->res.mask) return fail(c, "psm_fill_invalid: needs disparity maps and psm_lr_check");
    if (bind(c) || maps_writable(c)) return 1;
    const double t0 = now_us();
    const size_t HW = (size_t)c->W * c->H;
    {
        Prof p(c, PSM_K_LRC);
        launch_fill_inv(c->stream, c->maps, c->valid, HW, c->W, c->H);
    }
    if (check_launch(c, "fill_inv")) return 1;
    // the mask stays current: it still says which pixels the L-R check rejected, which is what the next stage of
    // PP::processDM (wgtMedian, src/PP.cpp:405-410) filters
    if (copy_maps_out(c, c->maps, lmap, rmap, stride)) return 1;
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    c->stage_us[PSM_STAGE_PP] += now_us() - t0;
    return 0;
}

int psm_wgt_median(psm_ctx *c, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    if (!c->res.mask) return fail(c, "psm_wgt_median: needs disparity maps and psm_lr_check");
    if (!c->have_images) return fail(c, "psm_wgt_median: no image pair uploaded (colour weights)");
    if (c->W < 9 || c->H < 9) return fail(c, "psm_wgt_median: image %dx%d smaller than the 19x19 window's wrap allows", c->W, c->H);
    if (bind(c) || maps_writable(c)) return 1;
    const double t0 = now_us();
    if (ensure_planes(c, whole_image(c), Rows{})) return 1;
    const size_t HW = (size_t)c->W * c->H;
    WmSched sch(c->march.flags);
    if (!(c->march.flags & PSM_FLAG_WMF_DATAFLOW)) {      // (PSM_FLAG_WMF_DATAFLOW: the dataflow form only)
        WmRun r;
        if (wm_scratch(c, r)) return 1;
        PSM_HIP(c, hipMemsetAsync(r.cnt, 0, r.snap * sizeof(int), c->stream));
        launch_wm_seed(c->stream, r.pr, c->W, c->H);     // all invalid pixels = the first sweep's lists; input copies; per-pixel state zeroed
        if (wm_cache(c, r) || wm_sweeps(c, r, sch)) return 1;
        // no fixed point within the cap (long chains of pixels that keep flipping each other): start over from the input with the
        // dataflow form, which is exact for any input
        for (int s = 0; s < 2; ++s)
            if (!sch.done[s]) PSM_HIP(c, hipMemcpyAsync(c->maps + s * HW, r.pr.s[s].orig, HW, hipMemcpyDeviceToDevice, c->stream));
    }
    for (int s = 0; s < 2; ++s) {
        if (!sch.done[s] && wgt_median_dataflow(c, s)) return 1;
        c->wm.sweeps[s] = sch.sweeps[s]; c->wm.evals[s] = sch.evals[s];
    }
    if (copy_maps_out(c, c->maps, lmap, rmap, stride)) return 1;
    c->stage_us[PSM_STAGE_PP] += now_us() - t0;
    return 0;
}

int psm_download_valid(psm_ctx *c, uint8_t *lvalid, uint8_t *rvalid, size_t stride)
{
    if (!c) return 1;
    if (!c->res.mask) return fail(c, "psm_download_valid: no current mask (psm_lr_check)");
    if (bind(c)) return 1;
    return copy_maps_out(c, c->valid, lvalid, rvalid, stride);
}

int psm_wgt_median_stats(psm_ctx *c, int *sweeps, long long *evals)
{
    if (!c) return 1;
    for (int s = 0; s < 2; ++s) {
        if (sweeps) sweeps[s] = c->wm.sweeps[s];
        if (evals) evals[s] = c->wm.evals[s];
    }
    return 0;
}

int psm_upload_maps(psm_ctx *c, const uint8_t *lmap, const uint8_t *rmap, const uint8_t *lvalid, const uint8_t *rvalid, size_t stride)
{
    if (!c) return 1;
    if (stride == 0) stride = c->W;
    if (stride < (size_t)c->W) return fail(c, "psm_upload_maps: stride %zu < width %d", stride, c->W);
    if (bind(c) || maps_writable(c)) return 1;
    forget_early(c->res);
    const size_t HW = (size_t)c->W * c->H;
    const uint8_t *src[4] = {lmap, rmap, lvalid, rvalid};
    uint8_t *dst[4] = {c->maps, c->maps + HW, c->valid, c->valid + HW};
    for (int i = 0; i < 4; ++i)
        if (src[i] && h2d_rows(c, dst[i], src[i], (size_t)c->W, stride, c->H)) return 1;
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    if (lmap && rmap) { cover(c->res, whole_image(c)); maps_written(c->res); }   // whole maps
    if (lvalid && rvalid) mask_written(c->res);                                  // (of the maps in the buffer: none without them)
    return 0;
}

}  // extern "C"
