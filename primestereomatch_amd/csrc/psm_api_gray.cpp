// psm_api_gray.cpp - the guided-filter path over a one-channel pair behind the C ABI: cost build, one-channel guided filter and
// winner-takes-all of two host planes in one call (psm_gray_compute; psm_gray.hip), the reading of GuidedFilter_cv (src/CVF.cpp:72-165)
// that FastGuidedFilter's dispatch on I.channels() intends (src/fastguidedfilter.cpp:38-49,89-119).  The definition is
// tests/gray_model.py / DESIGN.md 14.  An independent stage like the SGM one: it stages its own planes and writes its own buffers
// (psm::GrayState); it meets the rest where psm_sgm_select_maps does - the context's two current 8-bit maps (psm::Results) - so the
// L-R check, the fill, psm_score, the downloads and psm_reproject run behind it.  The image pair slots, the volume sides and the
// packed minima of the colour path never see it.
// No volume exists: per chunk of gray_plan().dc slices k_gray_ab leaves {a, b} in the chunk scratch and k_gray_q folds q into the
// stage's key plane; k_gray_merge turns the keys into the maps.  The test hooks run the storing form of the same kernels.
// psm_gray_compute_batch: the same launches for the pairs of several contexts at once, the pair on a grid axis - one host sequence,
// gray_run, of which the single call is the n = 1 with the record by value.
// psm_gray_compute_fgf / _batch: the same sequence with a subsample rate - FastGuidedFilterMono (src/fastguidedfilter.cpp:89-119;
// psm_gray_fgf.hip, tests/gray_fgf_model.py): its prep launch, per chunk model, smooth and apply + select on planes
// of the subsampled size, the same key plane, merge, state and timer.  Rate 0 is psm_gray_compute.
#include "psm_ctx.h"

#include <algorithm>
#include <cstdio>
#include <vector>

using namespace psm;

namespace psm {

void gray_free(psm_ctx *c)
{
    GrayState &g = c->gray;
    for (int s = 0; s < 2; ++s) {
        (void)hipFree(g.raw[s]); g.raw[s] = nullptr;
        (void)hipFree(g.ig[s]); g.ig[s] = nullptr;
        (void)hipFree(g.mv[s]); g.mv[s] = nullptr;
    }
    (void)hipFree(g.ab); g.ab = nullptr;
    (void)hipFree(g.keys); g.keys = nullptr;
    for (int s = 0; s < 2; ++s) { (void)hipFree(g.fsm[s]); g.fsm[s] = nullptr; }
    (void)hipFree(g.fab); g.fab = nullptr;
    (void)hipFree(g.fmab); g.fmab = nullptr;
    g.fsm_cap = g.fab_cap = 0;
    g.rate = 0;
    table_free(g.pairs);
    bracket_free(g.prof);
    g.depth = -1;
}

}  // namespace psm

namespace {

// what a context must be for the stage; who: the call; e: the context that receives the message (a batch: its first; who names the
// member)
int check_ctx(psm_ctx *e, const psm_ctx *c, const char *who)
{
    if (c->dtype == PSM_U8) return fail(e, "%s: an 8-bit context (PSM_U8): the one-channel filter is a float-mode stage", who);
    if (c->Dloc != c->D || strided(c)) return fail(e, "%s: a disparity shard holds part of the range (the stage selects over every disparity)", who);
    if (c->march.yend > c->march.ybeg) return fail(e, "%s: a row stripe is in force (psm_set_rows): the maps are whole-image maps", who);
    return 0;
}

// fp: the plan of a psm_gray_compute_fgf, which needs the subsampled planes in place of mv and ab; null: psm_gray_compute
int ensure_buffers(psm_ctx *c, const GrayPlan &pl, const GrayFgfPlan *fp)
{
    GrayState &g = c->gray;
    const size_t HW = (size_t)c->W * c->H;
    for (int s = 0; s < 2; ++s) {
        if (!g.raw[s]) PSM_HIP(c, hipMalloc(&g.raw[s], HW * sizeof(float)));
        if (!g.ig[s]) PSM_HIP(c, hipMalloc((void **)&g.ig[s], HW * sizeof(float2)));
        if (!fp && !g.mv[s]) PSM_HIP(c, hipMalloc((void **)&g.mv[s], HW * sizeof(float2)));
    }
    if (!fp && !g.ab) PSM_HIP(c, hipMalloc((void **)&g.ab, 2 * (size_t)pl.dc * HW * sizeof(float2)));
    if (!g.keys) PSM_HIP(c, hipMalloc((void **)&g.keys, 2 * HW * sizeof(long long)));
    if (!fp) return 0;
    const size_t n = (size_t)fp->ws * fp->hs, nab = 2 * (size_t)fp->dc * n;
    if (g.fsm_cap < n) {      // (a lower rate than any before: hipFree waits for whatever still reads the planes)
        g.depth = -1;
        for (int s = 0; s < 2; ++s) { (void)hipFree(g.fsm[s]); g.fsm[s] = nullptr; }
        g.fsm_cap = 0;
        for (int s = 0; s < 2; ++s) PSM_HIP(c, hipMalloc((void **)&g.fsm[s], n * sizeof(float4)));
        g.fsm_cap = n;
    }
    if (g.fab_cap < nab) {
        g.depth = -1;
        (void)hipFree(g.fab); g.fab = nullptr;
        (void)hipFree(g.fmab); g.fmab = nullptr;
        g.fab_cap = 0;
        PSM_HIP(c, hipMalloc((void **)&g.fab, nab * sizeof(float2)));
        PSM_HIP(c, hipMalloc((void **)&g.fmab, nab * sizeof(float2)));
        g.fab_cap = nab;
    }
    return 0;
}

GrayPair pair_of(const psm_ctx *c)
{
    const GrayState &g = c->gray;
    return GrayPair{{g.raw[0], g.raw[1]}, {g.ig[0], g.ig[1]}, {g.mv[0], g.mv[1]}, g.ab, g.keys, c->maps, {g.fsm[0], g.fsm[1]}, g.fab, g.fmab};
}

// The host sequence of psm_gray_compute (its one context, the record by value) and of psm_gray_compute_batch (batch: the same
// kernels over the device table of ctxs[0]), the arguments and every context checked: 2 + 2 ceil((D - 1) / dc) launches on ctxs[0]'s
// stream whatever n is.  ls, rs, lmaps, rmaps: per member (the map arrays, or an entry, may be null).
// rate: 0, or the subsample rate of psm_gray_compute_fgf / _batch (checked): 2 + 3 ceil((D - 1) / dc) launches.
int gray_run(const char *who, psm_ctx *const *ctxs, int n, const void *const *ls, const void *const *rs, size_t stride_bytes, int depth,
             uint8_t *const *lmaps, uint8_t *const *rmaps, size_t map_stride, bool batch, int rate)
{
    psm_ctx *c0 = ctxs[0];
    if (bind(c0)) return 1;
    hipStream_t s = c0->stream;
    const int W = c0->W, H = c0->H, D = c0->D;
    const size_t row = (size_t)W * (depth == PSM_IMG_F32 ? sizeof(float) : 1);
    const GrayPlan pl = gray_plan(W, H, D, n);
    const GrayFgfPlan fp = rate ? gray_fgf_plan(W, H, D, rate, n) : GrayFgfPlan{};

    // ---- buffers, events and the table's memory: before anything is ordered or launched ----
    for (int i = 0; i < n; ++i)
        if (ensure_buffers(ctxs[i], pl, rate ? &fp : nullptr)) return member_failed(c0, who, i, ctxs[i]);
    if (bracket_events(c0, c0->gray.prof) || batch_events(c0, ctxs, n)) return 1;
    std::vector<GrayPair> tab((size_t)n);
    for (int i = 0; i < n; ++i) tab[i] = pair_of(ctxs[i]);
    bool fresh = false;
    if (batch && table_reserve(c0, c0->gray.pairs, tab.data(), tab.size() * sizeof(GrayPair), &fresh)) return 1;
    const Recs<GrayPair> q{tab.data(), batch ? (const GrayPair *)c0->gray.pairs.dev : nullptr, n};

    // ---- the pairs, each on its member's stream: the planes of an earlier call are gone from here on ----
    for (int i = 0; i < n; ++i) {
        GrayState &g = ctxs[i]->gray;
        g.depth = -1;
        g.prof.timed = false;
    }
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        const void *src[2] = {ls[i], rs[i]};
        for (int k = 0; k < 2; ++k)
            if (h2d_rows(c, c->gray.raw[k], src[k], row, stride_bytes, H)) return member_failed(c0, who, i, c);
    }
    for (int i = 0; i < n; ++i) PSM_HIP(c0, hipStreamSynchronize(ctxs[i]->stream));      // the copies read caller memory (psm_upload_pair)

    // ---- every member's earlier work (a download of its maps, the copy of its pair) is ordered before the shared launches ----
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        hipStream_t own = c->stream;
        c->stream = s;                       // (maps_writable makes `s` wait for the member's download)
        const int bad = maps_writable(c);
        c->stream = own;
        if (bad) return member_failed(c0, who, i, c);
    }
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, c0->gray.pairs, tab.data(), tab.size() * sizeof(GrayPair))) return 1;

    // ---- the launches: guidance and empty keys, the chunks of the slices 1 .. D - 1 (d = 0 is never a candidate), the maps ----
    if (bracket_open(c0, c0->gray.prof, s)) return 1;
    if (rate) {
        launch_grayf_prep(s, q, fp, W, H, depth == PSM_IMG_F32);
        if (check_launch(c0, "k_grayf_prep")) return 1;
        for (int d = 1; d < D; d += fp.dc) launch_grayf_chunk(s, q, fp, W, H, d, std::min(D, d + fp.dc));
        if (check_launch(c0, "k_grayf_model, k_grayf_smooth, k_grayf_apply")) return 1;
    } else {
        launch_gray_prep(s, q, pl, W, H, depth == PSM_IMG_F32);
        if (check_launch(c0, "k_gray_prep")) return 1;
        for (int d = 1; d < D; d += pl.dc) launch_gray_chunk(s, q, pl, W, H, d, std::min(D, d + pl.dc));
        if (check_launch(c0, "k_gray_ab, k_gray_q")) return 1;
    }
    launch_gray_merge(s, q, W, H);
    if (check_launch(c0, "k_gray_merge")) return 1;
    if (bracket_close(c0, c0->gray.prof, s)) return 1;

    // ---- every context is where psm_sgm_select_maps leaves it: whole-image maps, no mask, no early map; the volume sides, the
    // packed minima and whatever the colour path has pending are not touched.  Only context 0 counts as timed ----
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        c->gray.depth = depth;
        c->gray.rate = rate;
        forget_early(c->res);
        cover(c->res, whole_image(c));
        maps_written(c->res);
    }
    if (batch_fork(c0, ctxs, n)) return 1;
    for (int i = 0; i < n; ++i)
        if (copy_maps_out(ctxs[i], ctxs[i]->maps, lmaps ? lmaps[i] : nullptr, rmaps ? rmaps[i] : nullptr, map_stride)) return member_failed(c0, who, i, ctxs[i]);
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(s));
    return 0;
}

// the hooks: the planes of a psm_gray_compute (fgf: of a psm_gray_compute_fgf) must exist
int check_hook(psm_ctx *c, const char *who, int side, bool fgf = false)
{
    if (check_ctx(c, c, who)) return 1;
    if (c->gray.depth < 0) return fail(c, "%s: no pair (%s; psm_release_scratch gives it back)", who, fgf ? "psm_gray_compute_fgf" : "psm_gray_compute");
    if (fgf != (c->gray.rate != 0))
        return fail(c, "%s: the planes belong to %s (the last call of the stage)", who, c->gray.rate ? "psm_gray_compute_fgf" : "psm_gray_compute");
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "%s: bad side %d", who, side);
    return 0;
}

// what both single entries check of the call's arguments; *stride_bytes 0 becomes the packed row
int check_call(psm_ctx *c, const char *who, const void *l, const void *r, size_t *stride_bytes, int depth, size_t map_stride)
{
    if (!l || !r) return fail(c, "%s: NULL image", who);
    if (depth != PSM_IMG_U8 && depth != PSM_IMG_F32) return fail(c, "%s: unknown depth %d", who, depth);
    const size_t row = (size_t)c->W * (depth == PSM_IMG_F32 ? sizeof(float) : 1);
    if (*stride_bytes == 0) *stride_bytes = row;
    if (*stride_bytes < row) return fail(c, "%s: stride %zu < row size %zu", who, *stride_bytes, row);
    if (map_stride != 0 && map_stride < (size_t)c->W) return fail(c, "%s: map stride %zu < width %d", who, map_stride, c->W);
    return 0;
}

// the rate of psm_gray_compute_fgf / _batch on a context of c's size: psm_cost_filter_fgf's bounds
int check_rate(psm_ctx *c, const char *who, int rate)
{
    if (rate != 2 && rate != 4 && rate != 8) return fail(c, "%s: subsample_rate %d not in {2,4,8}", who, rate);
    if (c->W / rate <= 8 / rate || c->H / rate <= 8 / rate) return fail(c, "%s: %dx%d too small for subsample_rate %d", who, c->W, c->H, rate);
    return 0;
}

// the batch entries' checks: the members, then the call's arguments; rate: of psm_gray_compute_fgf_batch, else null
int check_batch(const char *who, psm_ctx *const *ctxs, int n, const void *const *ls, const void *const *rs, size_t *stride_bytes, int depth,
                size_t map_stride, const int *rate)
{
    if (!ctxs) return fail(nullptr, "%s: NULL ctxs", who);
    if (n < 1) return fail(nullptr, "%s: n %d below 1", who, n);
    psm_ctx *c0 = ctxs[0];
    if (!c0) return fail(nullptr, "%s: context 0 is NULL", who);
    if (n > 4096) return fail(c0, "%s: %d contexts (at most 4096 per call)", who, n);
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        const psm_ctx *c = ctxs[i];
        char member[64];
        snprintf(member, sizeof member, "%s: context %d", who, i);
        if (check_ctx(c0, c, member)) return 1;
        if (c->W != c0->W || c->H != c0->H || c->D != c0->D || c->d0 != c0->d0 || c->d1 != c0->d1 || c->dtype != c0->dtype || c->device != c0->device)
            return fail(c0, "%s: context %d has another geometry / type / device than context 0", who, i);
        if (c->march.flags != c0->march.flags || c->march.seg_rows != c0->march.seg_rows || c->march.dstep != c0->march.dstep)
            return fail(c0, "%s: context %d has other options than context 0", who, i);
    }
    if (!ls || !rs) return fail(c0, "%s: NULL image arrays", who);
    for (int i = 0; i < n; ++i)
        if (!ls[i] || !rs[i]) return fail(c0, "%s: context %d: NULL image", who, i);
    if (depth != PSM_IMG_U8 && depth != PSM_IMG_F32) return fail(c0, "%s: unknown depth %d", who, depth);
    const size_t row = (size_t)c0->W * (depth == PSM_IMG_F32 ? sizeof(float) : 1);
    if (*stride_bytes == 0) *stride_bytes = row;
    if (*stride_bytes < row) return fail(c0, "%s: stride %zu < row size %zu", who, *stride_bytes, row);
    if (map_stride != 0 && map_stride < (size_t)c0->W) return fail(c0, "%s: map stride %zu < width %d", who, map_stride, c0->W);
    return rate ? check_rate(c0, who, *rate) : 0;
}

}  // namespace

extern "C" {

int psm_gray_compute(psm_ctx *c, const void *l, const void *r, size_t stride_bytes, int depth, uint8_t *lmap, uint8_t *rmap, size_t map_stride)
{
    const char *who = "psm_gray_compute";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_ctx(c, c, who) || check_call(c, who, l, r, &stride_bytes, depth, map_stride)) return 1;
    return gray_run(who, &c, 1, &l, &r, stride_bytes, depth, &lmap, &rmap, map_stride, false, 0);
}

// psm_gray_compute with FastGuidedFilterMono in place of the full-resolution filter: the same sequence with the rate
int psm_gray_compute_fgf(psm_ctx *c, const void *l, const void *r, size_t stride_bytes, int depth, int subsample_rate, uint8_t *lmap, uint8_t *rmap,
                         size_t map_stride)
{
    const char *who = "psm_gray_compute_fgf";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_ctx(c, c, who) || check_call(c, who, l, r, &stride_bytes, depth, map_stride) || check_rate(c, who, subsample_rate)) return 1;
    return gray_run(who, &c, 1, &l, &r, stride_bytes, depth, &lmap, &rmap, map_stride, false, subsample_rate);
}

// The launches of psm_gray_compute with the pair on a grid axis.  Planes, chunk scratch and keys stay per context; the kernels
// reach them through a device table ctxs[0] owns.  Every context ends where its own psm_gray_compute would have left it.
int psm_gray_compute_batch(psm_ctx *const *ctxs, int n, const void *const *ls, const void *const *rs, size_t stride_bytes, int depth,
                           uint8_t *const *lmaps, uint8_t *const *rmaps, size_t map_stride)
{
    const char *who = "psm_gray_compute_batch";
    if (check_batch(who, ctxs, n, ls, rs, &stride_bytes, depth, map_stride, nullptr)) return 1;
    return gray_run(who, ctxs, n, ls, rs, stride_bytes, depth, lmaps, rmaps, map_stride, true, 0);
}

int psm_gray_compute_fgf_batch(psm_ctx *const *ctxs, int n, const void *const *ls, const void *const *rs, size_t stride_bytes, int depth,
                               int subsample_rate, uint8_t *const *lmaps, uint8_t *const *rmaps, size_t map_stride)
{
    const char *who = "psm_gray_compute_fgf_batch";
    if (check_batch(who, ctxs, n, ls, rs, &stride_bytes, depth, map_stride, &subsample_rate)) return 1;
    return gray_run(who, ctxs, n, ls, rs, stride_bytes, depth, lmaps, rmaps, map_stride, true, subsample_rate);
}

int psm_gray_guidance(psm_ctx *c, int side, float *planes)
{
    const char *who = "psm_gray_guidance";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_hook(c, who, side)) return 1;
    if (!planes) return fail(c, "%s: NULL buffer", who);
    if (bind(c)) return 1;
    const size_t HW = (size_t)c->W * c->H;
    std::vector<float2> ig(HW), mv(HW);
    PSM_HIP(c, hipMemcpyAsync(ig.data(), c->gray.ig[side], HW * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipMemcpyAsync(mv.data(), c->gray.mv[side], HW * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < HW; ++i) {
        planes[i] = ig[i].x; planes[HW + i] = ig[i].y;
        planes[2 * HW + i] = mv[i].x; planes[3 * HW + i] = mv[i].y;
    }
    return 0;
}

int psm_gray_volume(psm_ctx *c, int side, int d0, int d1, float *q, float *ab)
{
    const char *who = "psm_gray_volume";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_hook(c, who, side)) return 1;
    if (d0 < 0 || d1 > c->D || d0 >= d1) return fail(c, "%s: slices [%d,%d) not inside [0,%d)", who, d0, d1, c->D);
    if (!q) return fail(c, "%s: NULL buffer", who);
    if (bind(c)) return 1;
    const GrayPlan pl = gray_plan(c->W, c->H, c->D);
    const GrayPair p = pair_of(c);
    const size_t HW = (size_t)c->W * c->H;
    float *qdev = nullptr;
    PSM_HIP(c, hipMalloc((void **)&qdev, (size_t)pl.dc * HW * sizeof(float)));
    std::vector<float2> abh(ab ? (size_t)pl.dc * HW : 0);
    int rc = 0;
    // chunk by chunk through the storing form; the chunks begin at d0
    for (int d = d0; d < d1 && !rc; d += pl.dc) {
        const int e = std::min(d1, d + pl.dc);
        const size_t n = (size_t)(e - d) * HW;
        launch_gray_chunk_store(c->stream, p, pl, c->W, c->H, side, d, e, qdev);
        rc = check_launch(c, "k_gray_ab, k_gray_q");
        if (!rc && hipMemcpyAsync(q + (size_t)(d - d0) * HW, qdev, n * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = fail(c, "%s: hipMemcpyAsync", who);
        if (!rc && ab && hipMemcpyAsync(abh.data(), c->gray.ab + (size_t)side * pl.dc * HW, n * sizeof(float2), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = fail(c, "%s: hipMemcpyAsync", who);
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(c, "%s: hipStreamSynchronize", who);
        for (size_t i = 0; ab && !rc && i < n; ++i) {      // [slice][2][H][W]: the plane a, then the plane b
            const size_t z = i / HW, px = i - z * HW;
            float *dst = ab + ((size_t)(d - d0) + z) * 2 * HW;
            dst[px] = abh[i].x; dst[HW + px] = abh[i].y;
        }
    }
    (void)hipFree(qdev);
    return rc;
}

int psm_gray_fgf_guidance(psm_ctx *c, int side, float *planes)
{
    const char *who = "psm_gray_fgf_guidance";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_hook(c, who, side, true)) return 1;
    if (!planes) return fail(c, "%s: NULL buffer", who);
    if (bind(c)) return 1;
    const size_t n = (size_t)(c->W / c->gray.rate) * (c->H / c->gray.rate);
    std::vector<float4> sm(n);
    PSM_HIP(c, hipMemcpyAsync(sm.data(), c->gray.fsm[side], n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        planes[i] = sm[i].x; planes[n + i] = sm[i].y; planes[2 * n + i] = sm[i].z;
    }
    return 0;
}

int psm_gray_fgf_volume(psm_ctx *c, int side, int d0, int d1, float *q, float *model)
{
    const char *who = "psm_gray_fgf_volume";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_hook(c, who, side, true)) return 1;
    if (d0 < 0 || d1 > c->D || d0 >= d1) return fail(c, "%s: slices [%d,%d) not inside [0,%d)", who, d0, d1, c->D);
    if (!q) return fail(c, "%s: NULL buffer", who);
    if (bind(c)) return 1;
    const GrayFgfPlan fp = gray_fgf_plan(c->W, c->H, c->D, c->gray.rate);
    const GrayPair p = pair_of(c);
    const size_t HW = (size_t)c->W * c->H, n = (size_t)fp.ws * fp.hs;
    float *qdev = nullptr;
    PSM_HIP(c, hipMalloc((void **)&qdev, (size_t)fp.dc * HW * sizeof(float)));
    std::vector<float2> abh(model ? (size_t)fp.dc * n : 0), mabh(abh.size());
    int rc = 0;
    // chunk by chunk through the storing form; the chunks begin at d0
    for (int d = d0; d < d1 && !rc; d += fp.dc) {
        const int e = std::min(d1, d + fp.dc);
        const size_t nq = (size_t)(e - d) * HW, nm = (size_t)(e - d) * n, off = (size_t)side * fp.dc * n;
        launch_grayf_chunk_store(c->stream, p, fp, c->W, c->H, side, d, e, qdev);
        rc = check_launch(c, "k_grayf_model, k_grayf_smooth, k_grayf_apply");
        if (!rc && hipMemcpyAsync(q + (size_t)(d - d0) * HW, qdev, nq * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = fail(c, "%s: hipMemcpyAsync", who);
        if (!rc && model && (hipMemcpyAsync(abh.data(), c->gray.fab + off, nm * sizeof(float2), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                             hipMemcpyAsync(mabh.data(), c->gray.fmab + off, nm * sizeof(float2), hipMemcpyDeviceToHost, c->stream) != hipSuccess))
            rc = fail(c, "%s: hipMemcpyAsync", who);
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(c, "%s: hipStreamSynchronize", who);
        for (size_t i = 0; model && !rc && i < nm; ++i) {      // [slice][4][hs][ws]: a, b, blur(a), blur(b)
            const size_t z = i / n, px = i - z * n;
            float *dst = model + ((size_t)(d - d0) + z) * 4 * n;
            dst[px] = abh[i].x; dst[n + px] = abh[i].y;
            dst[2 * n + px] = mabh[i].x; dst[3 * n + px] = mabh[i].y;
        }
    }
    (void)hipFree(qdev);
    return rc;
}

int psm_gray_time(psm_ctx *c, double *ms)
{
    if (!c) return fail(nullptr, "psm_gray_time: NULL context");
    return bracket_ms(c, c->gray.prof, c->gray.depth >= 0, "psm_gray_time", "the last psm_gray_compute / psm_gray_compute_fgf was not timed (PSM_OPT_PROFILE), or there is none", ms);
}

}  // extern "C"
