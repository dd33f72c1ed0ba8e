// psm_api_batch.cpp - several stereo pairs of one geometry per launch.  The reference's use on Middlebury-size data is a
// loop over pairs / datasets (src/main.cpp:64-73, src/StereoMatch.cpp:556-607): one 450 x 375 x 64 pair is 1 280 workgroups -
// 1.7 rounds of the chip's resident slots - behind four launches at their latency floor.  psm_compute_batch runs
// DispEst::CostConst_GPU + CostFilter_GPU + DispSelect_GPU (src/DispEst.cpp:272-276,299-308,323-328) of n contexts in shared
// launches: one k_prep, one k_guide_march, one k_cvf_pc grid with blockIdx.z = pair (two in the two-phase form), one
// reduction.  Every context stays a complete context: its maps, minima, validity masks, post-processing and volume readers
// behave as after the three single-pair calls, and the results are the same bits.
#include "psm_ctx.h"

#include <cstring>

using namespace psm;

// What the batch entry points share - psm_compute_batch, psm_sgm_compute_batch, psm_sgm_select_maps_batch,
// psm_joint_wmf_batch, psm_score_batch.  c0 is the batch's first context: it owns the table, the shared launches run on its
// stream, and it receives every message.
namespace psm {

int batch_member(psm_ctx *c0, const char *who, psm_ctx *const *ctxs, int i)
{
    if (!ctxs[i]) return fail(c0, "%s: context %d is NULL", who, i);
    for (int j = 0; j < i; ++j)
        if (ctxs[j] == ctxs[i]) return fail(c0, "%s: context %d appears twice", who, i);
    return 0;
}

int member_failed(psm_ctx *c0, const char *who, int i, const psm_ctx *c)
{
    return c == c0 ? 1 : fail(c0, "%s: context %d: %s", who, i, c->err.c_str());
}

// The device table of the members' records is uploaded again only when a record changed (*fresh: `recs` differ from the host
// copy; the comparison is bytewise, so a record's padding can report a change that is none - one upload too many, never one too
// few).  table_reserve makes room for a fresh table and is the part to call before anything is ordered or launched: growing
// synchronises c0's stream, whose kernels may still read the old table.
int table_reserve(psm_ctx *c0, DevTable &t, const void *recs, size_t bytes, bool *fresh)
{
    *fresh = t.host.size() != bytes || memcmp(t.host.data(), recs, bytes) != 0;
    if (*fresh && t.cap < bytes) {
        PSM_HIP(c0, hipStreamSynchronize(c0->stream));
        (void)hipFree(t.dev);
        if (t.pin) (void)hipHostFree(t.pin);
        t.dev = t.pin = nullptr;
        t.cap = 0;
        t.host.clear();                      // (should an allocation below fail, the next call must not take the old table for current)
        PSM_HIP(c0, hipMalloc((void **)&t.dev, bytes));
        PSM_HIP(c0, hipHostMalloc((void **)&t.pin, 2 * bytes, hipHostMallocDefault));
        t.cap = bytes;
    }
    for (hipEvent_t &e : t.ev)
        if (!e) PSM_HIP(c0, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return 0;
}

// The copy of a fresh table, on c0's stream: stream-ordered behind the previous call's kernels, which still read the old table (it
// changes with every frame of a loop whose image slots alternate), and out of one of two page-locked slots (a pageable source
// would make the "asynchronous" copy wait for the stream to drain) - a slot is rewritten only after the copy that read it has
// executed.  The host copy is adopted last: a table that did not get under way is not taken for current by the next call.
int table_upload(psm_ctx *c0, DevTable &t, const void *recs, size_t bytes)
{
    const int slot = t.slot ^= 1;
    PSM_HIP(c0, hipEventSynchronize(t.ev[slot]));
    uint8_t *pin = t.pin + (size_t)slot * t.cap;
    memcpy(pin, recs, bytes);
    t.host.clear();                          // (from here to the end the device copy is neither the old table for certain nor the new one)
    PSM_HIP(c0, hipMemcpyAsync(t.dev, pin, bytes, hipMemcpyHostToDevice, c0->stream));
    PSM_HIP(c0, hipEventRecord(t.ev[slot], c0->stream));
    t.host.assign((const uint8_t *)recs, (const uint8_t *)recs + bytes);
    return 0;
}

void table_free(DevTable &t)
{
    (void)hipFree(t.dev);
    if (t.pin) (void)hipHostFree(t.pin);
    for (hipEvent_t &e : t.ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    t.dev = t.pin = nullptr;
    t.cap = 0;
    t.host.clear();
}

// The stream ordering around the shared launches.  batch_events: the events of the two below, before any launch; batch_join:
// every member's earlier work on a stream of its own is ordered before what follows on c0's; batch_fork: what was enqueued on c0's
// stream is ordered before every such member's later work.  Members on c0's stream (shared streams, a batch of one) need neither.
int batch_events(psm_ctx *c0, psm_ctx *const *ctxs, int n)
{
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if (c->stream == c0->stream) continue;
        if (!c->ev_batch) PSM_HIP(c0, hipEventCreateWithFlags(&c->ev_batch, hipEventDisableTiming));
        if (!c0->ev_batch) PSM_HIP(c0, hipEventCreateWithFlags(&c0->ev_batch, hipEventDisableTiming));
    }
    return 0;
}

int batch_join(psm_ctx *c0, psm_ctx *const *ctxs, int n)
{
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if (c->stream == c0->stream) continue;
        PSM_HIP(c0, hipEventRecord(c->ev_batch, c->stream));
        PSM_HIP(c0, hipStreamWaitEvent(c0->stream, c->ev_batch, 0));
    }
    return 0;
}

int batch_fork(psm_ctx *c0, psm_ctx *const *ctxs, int n)
{
    bool recorded = false;
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if (c->stream == c0->stream) continue;
        if (!recorded) PSM_HIP(c0, hipEventRecord(c0->ev_batch, c0->stream));
        recorded = true;
        PSM_HIP(c0, hipStreamWaitEvent(c->stream, c0->ev_batch, 0));
    }
    return 0;
}

}  // namespace psm

extern "C" int psm_compute_batch(psm_ctx *const *ctxs, int n)
{
    if (!ctxs || n < 1 || !ctxs[0]) return fail(nullptr, "psm_compute_batch: bad arguments");
    psm_ctx *c0 = ctxs[0];
    if (n > 4096) return fail(c0, "psm_compute_batch: %d pairs (at most 4096 per call)", n);
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, "psm_compute_batch", ctxs, i)) return 1;
        psm_ctx *c = ctxs[i];
        if (c->W != c0->W || c->H != c0->H || c->D != c0->D || c->d0 != c0->d0 || c->d1 != c0->d1 || c->dtype != c0->dtype || c->device != c0->device)
            return fail(c0, "psm_compute_batch: context %d has another geometry / type / device than context 0", i);
        if (c->opt_variant != 0 || (c->march.flags & (PSM_FLAG_STORE_FILTERED | PSM_FLAG_MATERIALISE_COSTS)))
            return fail(c0, "psm_compute_batch: context %d asks for a storing form (the batch runs the default select path)", i);
        if (c->march.flags != c0->march.flags || c->march.seg_rows != c0->march.seg_rows || c->march.dstep != c0->march.dstep)
            return fail(c0, "psm_compute_batch: context %d has other options than context 0", i);
        // the batched launches exist in the bit-exact form only: a silently ignored flag would break "same maps as the three
        // single-pair calls" (which DO run the tolerance form with this flag)
        if (c->march.flags & (PSM_FLAG_F32_TOL | PSM_FLAG_FMA_SOLVE))
            return fail(c0, "psm_compute_batch: context %d asks for PSM_FLAG_F32_TOL / PSM_FLAG_FMA_SOLVE (single-pair entry points only)", i);
        if (c->march.yend > c->march.ybeg) return fail(c0, "psm_compute_batch: context %d is restricted to a row stripe", i);
        if (!c->have_images && !pair_staged(c->pair.st)) return fail(c0, "psm_compute_batch: context %d has no image pair", i);
        if (depth_at_construct(c->pair.st) != depth_at_construct(c0->pair.st))      // (a staged pair is adopted below)
            return fail(c0, "psm_compute_batch: context %d holds images of another depth than context 0", i);
    }
    if (bind(c0)) return 1;
    const double t0 = now_us();
    // Refused before any context has changed.  Float images staged asynchronously bring their range with them; only the IMAGES
    // matter: the batch rebuilds the costs from them, as psm_cost_construct does before it forgets an uploaded volume's range.
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        bool ok = true;
        if (next_pair_inside(c, &ok)) return member_failed(c0, "psm_compute_batch", i, c);
        if (!ok) return fail(c0, "psm_compute_batch: the float images of context %d are outside the select forms' domain (2^-10 .. 2^10)%s", i,
                             pair_staged(c->pair.st) ? "" : "; use the single-pair entry points");
    }
    const int W = c0->W, H = c0->H, Dloc = c0->Dloc;
    hipStream_t s = c0->stream;

    // ---- plan, scratch and events (before any launch: growing a scratch buffer synchronises its context's stream) ----
    const SelPlan sp = select_plan(c0, n, true);
    for (int i = 0; i < n; ++i)
        if (ensure_gf_scratch(ctxs[i], sp.scratch_bytes)) return fail(c0, "psm_compute_batch: %s", ctxs[i]->err.c_str());
    if (batch_events(c0, ctxs, n)) return 1;

    // ---- every context's earlier work (uploads, downloads of its maps) is ordered before the shared launches ----
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        hipStream_t own = c->stream;
        c->stream = s;                       // (adopt_staged_pair / maps_writable make `s` wait for the copy streams' events)
        const int bad = adopt_staged_pair(c) || maps_writable(c);
        c->stream = own;
        if (bad) return fail(c0, "psm_compute_batch: %s", c->err.c_str());
    }
    if (batch_join(c0, ctxs, n)) return 1;

    // ---- the table of the pairs' pointers: built here, since adopt_staged_pair swapped the image slots ----
    std::vector<PcPair> tab((size_t)n);
    for (int i = 0; i < n; ++i) tab[i] = pc_pair(ctxs[i]);
    bool fresh = false;
    if (table_reserve(c0, c0->batch_tab, tab.data(), tab.size() * sizeof(PcPair), &fresh)) return 1;
    if (fresh && table_upload(c0, c0->batch_tab, tab.data(), tab.size() * sizeof(PcPair))) return 1;
    const Recs<PcPair> q = {tab.data(), (const PcPair *)c0->batch_tab.dev, n};

    const int depth = c0->pair.st.depth;
    const size_t row = (size_t)W * 3 * (depth == PSM_IMG_F32 ? 4 : 1);
    const bool u8 = c0->dtype == PSM_U8;
    const bool whole = Dloc == c0->D;        // every slice here: the maps are final (else: packed minima for psm_disp_merge)
    double t1 = t0;
    auto enqueue = [&]() -> int {
        // ---- CostConst: CVC::preprocess of every image (the cost volumes stay virtual) - float mode: inside the guidance launch ----
        if (u8) {
            Prof p(c0, PSM_K_PREP);
            launch_prep(s, q, row, depth == PSM_IMG_F32, W, 0, H, false);
            launch_prep(s, q, row, depth == PSM_IMG_F32, W, 0, H, true);
        }
        t1 = now_us();
        // ---- CostFilter: guidance of every image, the fused select kernel over every pair, the reduction ----
        {
            Prof p(c0, PSM_K_GUIDE);
            launch_guidance(s, q, W, H, 0, H, false, u8 ? 0 : (depth == PSM_IMG_F32 ? 2 : 1), row);
        }
        if (enqueue_select(c0, q, sp)) return 1;
        if (sp.two_phase && whole) {
            Prof p(c0, PSM_K_MERGE);
            launch_merge_batch(s, q, W, H);
        }
        return check_launch(c0, "batch (prep, guidance, fused select filter, reduction)");
    };
#ifdef PSM_EXPERIMENTS      // (PSM_OPT_GRAPH: experiment builds only - the replay measured slower than the plain launches)
    if (c0->opt_graph && c0->opt_profile == 0) {
        // One graph per frame: the kernels read every pair through the device table (whose ADDRESS is all the graph holds), so the
        // captured launches stay valid while the batch size, the geometry and the options do - also across new image pairs.
        const long long sig[8] = {n, (long long)(size_t)q.dev, c0->march.flags, c0->march.seg_rows, depth, Dloc, c0->d0, (long long)W << 32 | H};
        if (!c0->batch_graph || memcmp(sig, c0->graph_sig, sizeof sig) != 0) {
            if (c0->batch_graph) { (void)hipGraphExecDestroy(c0->batch_graph); c0->batch_graph = nullptr; }
            hipGraph_t g = nullptr;
            PSM_HIP(c0, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const int bad = enqueue();
            const hipError_t e = hipStreamEndCapture(s, &g);
            if (bad || e != hipSuccess) {
                if (g) (void)hipGraphDestroy(g);
                return bad ? 1 : fail(c0, "psm_compute_batch: graph capture failed: %s", hipGetErrorString(e));
            }
            const hipError_t ei = hipGraphInstantiate(&c0->batch_graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ei != hipSuccess) { c0->batch_graph = nullptr; return fail(c0, "psm_compute_batch: hipGraphInstantiate failed: %s", hipGetErrorString(ei)); }
            memcpy(c0->graph_sig, sig, sizeof sig);
        }
        PSM_HIP(c0, hipGraphLaunch(c0->batch_graph, s));
        t1 = now_us();
    } else
#endif
    if (enqueue()) return 1;
    for (int i = 0; i < n; ++i)
        if (images_read(ctxs[i], s)) return member_failed(c0, "psm_compute_batch", i, ctxs[i]);
    const double t2 = now_us();

    // ---- every context is now where psm_cost_construct + psm_cost_filter + psm_disp_select(ctx, NULL, NULL, 0) leave it ----
    if (batch_fork(c0, ctxs, n)) return 1;
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        c->g1_rows = c->guid_rows = whole_image(c);
        c->have_cost = true;
        c->vol_domain_ok[0] = c->vol_domain_ok[1] = true;      // (the costs are those of the images again, as after psm_cost_construct)
        for (VolSide &v : c->vside) { new_costs(v, true); filtered_to_keys(v); }
        stale(c->res);
        keys_gone(c->res);
        filtered(c->res, whole_image(c), nullptr);             // (the batch wrote the maps itself: no early map to take)
        if (whole) maps_written(c->res);
        else { keys_complete(c->res, 0); keys_complete(c->res, 1); }   // (a disparity shard: its minima are what psm_disp_merge_ctx takes)
    }
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(s));
    const double t3 = now_us();
    for (int i = 0; i < n; ++i) {      // the batch's wall time, split like the reference's three stage timers
        ctxs[i]->stage_us[PSM_STAGE_CVC] = t1 - t0;
        ctxs[i]->stage_us[PSM_STAGE_CVF] = t2 - t1;
        ctxs[i]->stage_us[PSM_STAGE_DISPSEL] = t3 - t2;
    }
    return 0;
}
