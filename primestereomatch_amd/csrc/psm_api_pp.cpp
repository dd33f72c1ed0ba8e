// psm_api_pp.cpp - the post-processing rows behind the C ABI: lrCheck, fillInv and the plain weighted
// median of PP::processDM (src/PP.cpp:17-247,405-410) on the device maps of the last DispSelect.  The reference runs these
// on the CPU; here they sit behind the same boundary so that the maps never leave the device between the stages.
// psm_lr_check, psm_fill_invalid, psm_wgt_median and psm_post_process_batch are one launch sequence (pp_enqueue): the pair lies on
// a grid axis of its own, whether the call has one or many.  A context keeps the median's scratch in psm::WmState (psm_ctx.h;
// wm_free); the counters of all maps of a call, their snapshots and - for several pairs - the device table of the records lie with
// the call's first context (psm::WmBatch).  The layout of the sweep block, the schedule of the sweeps and the cache decision are
// psm_wm_sched.h, which tests/test_wm_sched.py and tests/test_wm_batch_sched.py check on the host against a model of the rules.
#include "psm_ctx.h"

#include <cstring>
#include <string>

using namespace psm;

// ---- The plain weighted median: psm::WmState and psm::WmBatch between calls, WmRun within a call ----
namespace psm {

void wm_free(psm_ctx *c, bool all)
{
    WmState &m = c->wm;
    (void)hipFree(m.wts); m.wts = nullptr; m.wts_n = 0;
    (void)hipFree(m.block); m.block = nullptr;
    (void)hipFree(m.flow); m.flow = nullptr;
    WmBatch &b = c->wmb;                   // (as the first context of a call: rebuilt by the next such call)
    table_free(b.tab);
    (void)hipFree(b.cnt); b.cnt = nullptr;
    if (b.pin) { (void)hipHostFree(b.pin); b.pin = nullptr; }
    b.cap = 0;
    if (!all) return;
    for (hipEvent_t &e : b.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

// The row-dataflow form of wgtMedian: exact for any input, but as sequential as the reference wherever invalid pixels chain
static int wgt_median_dataflow(psm_ctx *c, int side, const char *who)
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
        return fail(c, "%s: row pipeline stalled (watchdog); the device maps are no longer valid - select again", who);
    }
    return 0;
}

// The parallel form: sweeps to the fixed point of the in-place recursion (psm_pp.hip), the maps of all pairs side by side
struct WmRun {
    const char *who;               // the entry, for the messages
    psm_ctx *c0;
    psm_ctx *const *ctxs;
    int n;
    std::vector<PpPair> recs;      // the pairs' records as the host fills them
    PpRecs q;                      // ... as the launches take them: by value (n == 1) or through c0's device table
    size_t snap;                   // ints per snapshot: the counters of all 2 n maps
    bool cached = false;           // every map has its weight cache
};

// the launch check behind a step of the entry `who`: the stage as the entry's name behind "psm_" has it, and the step
static int pp_launched(psm_ctx *c0, const char *who, const char *what)
{
    if (hipPeekAtLastError() == hipSuccess) return 0;
    return check_launch(c0, (std::string(who + 4) + " (" + what + ")").c_str());
}

// a context's sweep block, on first use; pr: what the block holds where (cnt, g1 and wts are the caller's)
static int wm_scratch(psm_ctx *c, WmPair &pr)
{
    WmState &m = c->wm;
    const size_t HW = (size_t)c->W * c->H;
    const WmLayout l = wm_layout(HW);
    if (!m.block) PSM_HIP(c, hipMalloc((void **)&m.block, l.bytes));
    auto ints = [&](size_t at) { return reinterpret_cast<int *>(m.block + at); };
    for (int s = 0; s < 2; ++s) {
        const WmSideAt &at = l.s[s];
        WmSide &a = pr.s[s];
        a.cur = c->maps + s * HW; a.valid = c->valid + s * HW; a.g1 = c->g[s].g1;
        a.orig = m.block + at.orig; a.newv = m.block + at.newv; a.chgb = m.block + at.chgb; a.rowany = m.block + at.rowany;
        a.stamp = ints(at.stamp); a.list[0] = ints(at.list[0]); a.list[1] = ints(at.list[1]); a.chg = ints(at.chg);
        a.slot_of = ints(at.slot_of); a.inv = ints(at.inv); a.cnt = nullptr; a.wts = nullptr;
    }
    return 0;
}

// the counters of all maps and their page-locked snapshots, for at least `maps` maps; the events
static int wm_counter_block(psm_ctx *c0, size_t maps)
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

// The call-wide cache decision (wm_cache_plan), every member's weights grown on demand, and the pass that fills them.  The records
// gain their wts here: a device table is uploaded again before the pass reads it.
static int wm_cache(WmRun &r)
{
    psm_ctx *c0 = r.c0;
    WmBatch &b = c0->wmb;
    const int m = 2 * r.n;
    size_t mem_free = 0, mem_total = 0, avail = SIZE_MAX;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) {
        avail = mem_free;
        for (int i = 0; i < r.n; ++i) avail += r.ctxs[i]->wm.wts_n * sizeof(float);     // (what the members hold already counts as available)
    } else (void)hipGetLastError();
    // (the counts of invalid pixels through the same page-locked snapshot the sweeps use: one small kernel, no copy engine; the
    // host reads them next, so this one snapshot is waited for)
    launch_copy_bytes(c0->stream, b.pin, b.cnt, r.snap * sizeof(int));
    PSM_HIP(c0, hipStreamSynchronize(c0->stream));
    std::vector<int> n0((size_t)m);
    int n_max = 0;
    for (int i = 0; i < m; ++i) {
        n0[i] = wm_active(wm_counters(b.pin, i), 0);
        if (n0[i] > n_max) n_max = n0[i];
    }
    if (!wm_cache_plan(n0.data(), m, avail, c0->march.flags)) return 0;
    for (int i = 0; i < r.n; ++i) {
        WmState &w = r.ctxs[i]->wm;
        const size_t need = wm_side_need(n0[2 * i]) + wm_side_need(n0[2 * i + 1]);
        if (w.wts_n < need) {
            (void)hipFree(w.wts); w.wts = nullptr; w.wts_n = 0;
            if (hipMalloc((void **)&w.wts, need * sizeof(float)) == hipSuccess) w.wts_n = need;
            else { (void)hipGetLastError(); return 0; }     // no memory for it: the whole call recomputes, as without the cache
        }
    }
    for (int i = 0; i < r.n; ++i) {
        WmState &w = r.ctxs[i]->wm;
        r.recs[i].wm.s[0].wts = w.wts;
        r.recs[i].wm.s[1].wts = w.wts + wm_side_need(n0[2 * i]);
    }
    r.cached = true;
    // (every side's wts: the records differ from the table the seed read - which the host has waited for)
    if (r.q.dev && table_upload(c0, b.tab, r.recs.data(), r.recs.size() * sizeof(PpPair))) return 1;
    Prof p(c0, PSM_K_WMF);
    launch_wm_weights(c0->stream, r.q, c0->W, c0->H, n_max);
    return 0;
}

// the schedule's next group of sweeps, and behind it the snapshot of the counters into `slot`
static int wm_launch_group(const WmRun &r, WmSched &sch, int slot)
{
    psm_ctx *c0 = r.c0;
    const WmGroup g = sch.next_group();
    {
        Prof p(c0, PSM_K_WMF);
        // (a map that has reached its fixed point has empty lists from then on: its share of a launch returns at once)
        for (int sw = g.begin; sw < g.end; ++sw) launch_wm_sweep(c0->stream, r.q, c0->W, c0->H, c0->D, sw, r.cached, g.short_lists);
    }
    if (pp_launched(c0, r.who, "sweeps")) return 1;
    // (a kernel writing the page-locked snapshot: a copy-engine transfer in the stream stalls it for ~60 us)
    launch_copy_bytes(c0->stream, c0->wmb.pin + slot * r.snap, c0->wmb.cnt, r.snap * sizeof(int));
    PSM_HIP(c0, hipEventRecord(c0->wmb.ev[slot], c0->stream));
    sch.launched(g, slot);
    return 0;
}

static int wm_sweeps(const WmRun &r, WmSched &sch)
{
    psm_ctx *c0 = r.c0;
    if (wm_launch_group(r, sch, 0)) return 1;
    for (int g = 0;; ++g) {
        if (sch.more() && wm_launch_group(r, sch, (g + 1) & 1)) return 1;      // (queued before this group's counters are looked at)
        PSM_HIP(c0, hipEventSynchronize(c0->wmb.ev[g & 1]));
        if (!sch.read(g & 1, c0->wmb.pin + (g & 1) * r.snap)) break;
    }
#ifdef PSM_EXPERIMENTS
    if (getenv("PSM_WM_TRACE")) {      // per sweep: pixels evaluated / changed (every map; map 2 i + s: side s of pair i)
        std::vector<int> hc(r.snap);
        PSM_HIP(c0, hipMemcpy(hc.data(), c0->wmb.cnt, hc.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int s = 0; s < 2 * r.n; ++s) {
            const int *cnt = wm_counters(hc.data(), s);
            fprintf(stderr, "[wm] side %d:", s);
            for (int k = 0; k < sch.sw && k < WM_SWEEP_CAP; ++k) fprintf(stderr, " %d/%d", wm_active(cnt, k), wm_changed(cnt, k));
            fprintf(stderr, "\n");
        }
    }
#endif
    return 0;
}

// The stages of `stages` (PSM_PP_*) on the maps of the n contexts of one call, in the order of PP::processDM: the only statement of
// the tail's preconditions, its allocation order, the join, the table upload, the launches, their Prof brackets and launch checks,
// the median's group loop, cache pass, copy-back of unfinished maps and dataflow fall-back, wm.sweeps / wm.evals, mask_written and
// the fork.  who: the entry's name in the messages; single: the entry is one of the three single-pair ones.  Every launch takes all
// pairs, the pair on grid.z; buffers stay per context (WmState), but for the counters of all 2 n maps, which lie in one block of
// ctxs[0] (WmBatch) so that one fill clears and one small kernel snapshots them.  The median's sweeps follow one schedule for all
// maps (WmSched) and one cache decision (wm_cache_plan); a map that leaves the sweeps at the cap - or every map, under
// PSM_FLAG_WMF_DATAFLOW - starts over from its input with the dataflow form, one by one.  Every context of a batch ends where its
// own single calls would have left it.
// What differs between a single call and a batch, and nothing else:
//   - n == 1 (either entry): the PpPair record goes to the kernels by value in the kernarg, so such a call neither allocates nor
//     uploads a device table; n > 1: the records are uploaded as ctxs[0]'s table (table_reserve / table_upload), again once the
//     cache has set their wts;
//   - n > 1 only: the other contexts' streams are ordered before and behind the shared launches by events (batch_events,
//     batch_join and batch_fork do nothing for n == 1);
//   - the single entries name "this context" where a batch names "context i" (the launch checks and the watchdog name the stage by
//     the entry either way), and psm_fill_invalid and psm_wgt_median take the current mask as their word that the maps are whole,
//     as they always have (a batch looks at the rows itself);
//   - the single entries only: copy_maps_out behind this function, by the entry itself (which is why the closing synchronisation
//     and the stage time are the entries').
static int pp_enqueue(const char *who, bool single, psm_ctx *const *ctxs, int n, int stages)
{
    psm_ctx *c0 = ctxs[0];
    const bool lrc = stages & PSM_PP_LR_CHECK, fill = stages & PSM_PP_FILL, med = stages & PSM_PP_WGT_MEDIAN;
    const unsigned wmf_bits = PSM_FLAG_WMF_DATAFLOW | PSM_FLAG_WMF_NO_CACHE | PSM_FLAG_WMF_TWO_SWEEPS;
    // ---- refused before anything is allocated, ordered or launched ----
    auto name = [&](int i) { return single ? std::string("this context") : "context " + std::to_string(i); };
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        const psm_ctx *c = ctxs[i];
        if (c->W != c0->W || c->H != c0->H || c->D != c0->D || c->device != c0->device)
            return fail(c0, "%s: %s has another geometry / max_disp / device than context 0", who, name(i).c_str());
        if ((c->march.flags & wmf_bits) != (c0->march.flags & wmf_bits))
            return fail(c0, "%s: %s has other weighted-median flags than context 0", who, name(i).c_str());
        if (c->pair.st.depth != c0->pair.st.depth) return fail(c0, "%s: %s holds images of another depth than context 0", who, name(i).c_str());
        if (!c->res.maps) return fail(c0, "%s: %s has no disparity maps", who, name(i).c_str());
        if ((lrc || !single) && stripe_only(c)) return fail(c0, "%s: the maps of %s hold its row stripe only (gather the stripes first)", who, name(i).c_str());
        if (!lrc && !c->res.mask)
            return fail(c0, "%s: %s has no current mask (psm_lr_check%s)", who, name(i).c_str(), single ? "" : ", or PSM_PP_LR_CHECK among the stages");
        if (med && !c->have_images) return fail(c0, "%s: %s has no image pair uploaded (colour weights)", who, name(i).c_str());
        if (med && (c->W < 9 || c->H < 9))
            return fail(c0, "%s: %s: image %dx%d smaller than the 19x19 window's wrap allows", who, name(i).c_str(), c->W, c->H);
    }
    if (bind(c0)) return 1;
    const int W = c0->W, H = c0->H;
    const size_t HW = (size_t)W * H;
    hipStream_t s = c0->stream;
    const bool sweeps = med && !(c0->march.flags & PSM_FLAG_WMF_DATAFLOW);      // (PSM_FLAG_WMF_DATAFLOW: the dataflow form only)
    const bool table = n > 1;

    // ---- scratch, events and the table's memory: before any launch (growing synchronises) ----
    WmRun r{who, c0, ctxs, n, std::vector<PpPair>((size_t)n), PpRecs{}, 2 * (size_t)n * WM_NCNT};
    if (sweeps && wm_counter_block(c0, 2 * (size_t)n)) return 1;
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        PpPair &p = r.recs[i];
        memset(&p, 0, sizeof p);                 // (padding too: table_reserve compares bytes)
        if (sweeps) {
            if (wm_scratch(c, p.wm)) return member_failed(c0, who, i, c);
            for (int sd = 0; sd < 2; ++sd) p.wm.s[sd].cnt = c0->wmb.cnt + (2 * (size_t)i + sd) * WM_NCNT;
        } else {
            for (int sd = 0; sd < 2; ++sd) { p.wm.s[sd].cur = c->maps + sd * HW; p.wm.s[sd].valid = c->valid + sd * HW; }
        }
        p.lv = c->valid; p.rv = c->valid + HW;
    }
    if (batch_events(c0, ctxs, n)) return 1;
    bool fresh = false;
    const size_t tab_bytes = r.recs.size() * sizeof(PpPair);
    if (table && table_reserve(c0, c0->wmb.tab, r.recs.data(), tab_bytes, &fresh)) return 1;
    r.q = PpRecs{r.recs.data(), table ? (const PpPair *)c0->wmb.tab.dev : nullptr, n};

    // ---- every member's earlier work is ordered before the shared launches; the planes the weights read ----
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if ((fill || med) && maps_writable(c)) return member_failed(c0, who, i, c);
        if (med && ensure_planes(c, whole_image(c), Rows{})) return member_failed(c0, who, i, c);
        if (sweeps) for (int sd = 0; sd < 2; ++sd) r.recs[i].wm.s[sd].g1 = c->g[sd].g1;      // (allocated by ensure_planes at the latest)
    }
    if (table && sweeps) fresh = fresh || c0->wmb.tab.host.size() != tab_bytes || memcmp(c0->wmb.tab.host.data(), r.recs.data(), tab_bytes) != 0;
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, c0->wmb.tab, r.recs.data(), tab_bytes)) return 1;

    if (lrc) {
        {
            Prof p(c0, PSM_K_LRC);
            launch_lr_check(s, r.q, W, H);
        }
        if (pp_launched(c0, who, "lr_check")) return 1;
        for (int i = 0; i < n; ++i) mask_written(ctxs[i]->res);
    }
    if (fill) {
        {
            Prof p(c0, PSM_K_LRC);
            launch_fill_inv(s, r.q, W, H);
        }
        if (pp_launched(c0, who, "fill_inv")) return 1;
        // the masks stay current: they still say which pixels the L-R check rejected, which is what the next stage of
        // PP::processDM (wgtMedian, src/PP.cpp:405-410) filters
    }
    if (med) {
        WmSched sch(2 * n, c0->march.flags);
        if (sweeps) {
            PSM_HIP(c0, hipMemsetAsync(c0->wmb.cnt, 0, r.snap * sizeof(int), s));
            launch_wm_seed(s, r.q, W, H);     // all invalid pixels = the first sweep's lists; input copies; per-pixel state zeroed
            if (wm_cache(r) || wm_sweeps(r, sch)) return 1;
            // no fixed point within the cap (long chains of pixels that keep flipping each other): start over from the input with the
            // dataflow form, which is exact for any input
            for (int q = 0; q < 2 * n; ++q)
                if (!sch.done[q]) PSM_HIP(c0, hipMemcpyAsync(ctxs[q / 2]->maps + (q & 1) * HW, r.recs[q / 2].wm.s[q & 1].orig, HW, hipMemcpyDeviceToDevice, s));
        }
        // maps that left the sweeps at the cap (or every map: PSM_FLAG_WMF_DATAFLOW): the dataflow form, one by one, on c0's stream
        for (int q = 0; q < 2 * n; ++q) {
            psm_ctx *c = ctxs[q / 2];
            if (!sch.done[q]) {
                hipStream_t own = c->stream;
                c->stream = s;
                const int bad = wgt_median_dataflow(c, q & 1, who);
                c->stream = own;
                if (bad) return member_failed(c0, who, q / 2, c);
            }
            c->wm.sweeps[q & 1] = sch.sweeps[q]; c->wm.evals[q & 1] = sch.evals[q];
        }
    }
    return batch_fork(c0, ctxs, n);
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
    const double t0 = now_us();
    if (pp_enqueue(who, false, ctxs, n, stages)) return 1;
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(c0->stream));      // (the median has waited for its snapshots either way)
    const double dt_us = now_us() - t0;
    for (int i = 0; i < n; ++i) ctxs[i]->stage_us[PSM_STAGE_PP] = dt_us;
    return 0;
}

int psm_lr_check(psm_ctx *c, uint8_t *lvalid, uint8_t *rvalid, size_t stride)
{
    if (!c) return 1;
    const double t0 = now_us();
    if (pp_enqueue("psm_lr_check", true, &c, 1, PSM_PP_LR_CHECK)) return 1;
    if (copy_maps_out(c, c->valid, lvalid, rvalid, stride)) return 1;
    return end_stage(c, PSM_STAGE_PP, t0);
}

int psm_fill_invalid(psm_ctx *c, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    const double t0 = now_us();
    if (pp_enqueue("psm_fill_invalid", true, &c, 1, PSM_PP_FILL)) return 1;
    if (copy_maps_out(c, c->maps, lmap, rmap, stride)) return 1;
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    c->stage_us[PSM_STAGE_PP] += now_us() - t0;
    return 0;
}

int psm_wgt_median(psm_ctx *c, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    const double t0 = now_us();
    if (pp_enqueue("psm_wgt_median", true, &c, 1, PSM_PP_WGT_MEDIAN)) return 1;
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
