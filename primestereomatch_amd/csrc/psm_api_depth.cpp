// psm_api_depth.cpp - psm_reproject: from disparity to depth behind the C ABI - cv::reprojectImageTo3D of the current result with
// the Q of cv::stereoRectify (the reference computes it at src/StereoMatch.cpp:456-458 and drops it) and the ordered, compacted,
// coloured point cloud.  Kernels: psm_depth.hip.  The definition is tests/depth_model.py / DESIGN.md 12.  An independent stage, as
// psm_score is: it reads the context's current result - the left map and its mask through psm::Results, the int16 map the SGM
// sources of psm_score read - and the left image of the pair, and writes its own planes (psm::DepthState).
// psm_reproject_batch: the same launches for the results of several contexts at once, the context on a grid axis of its own.  Both
// entries check their arguments and enqueue through reproject_run.
#include "psm_ctx.h"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace psm;

namespace psm {

void depth_free(psm_ctx *c)
{
    DepthState &q = c->depth;
    (void)hipFree(q.xyz); q.xyz = nullptr;
    (void)hipFree(q.z); q.z = nullptr;
    (void)hipFree(q.cloud); q.cloud = nullptr;
    (void)hipFree(q.tiles); q.tiles = nullptr;
    (void)hipFree(q.cnt); q.cnt = nullptr;
    if (q.pin) (void)hipHostFree(q.pin);
    q.pin = nullptr;
    if (q.ev_done) (void)hipEventDestroy(q.ev_done);
    q.ev_done = nullptr;
    bracket_free(q.prof);
    table_free(q.tab);
    q.outputs = 0;
    q.pending = false;
}

}  // namespace psm

namespace {

constexpr int DEPTH_OUTPUTS_ALL = PSM_DEPTH_XYZ | PSM_DEPTH_Z | PSM_DEPTH_CLOUD;

// what psm_reproject refuses about the call's own arguments (no context needed) ...
int check_call(psm_ctx *e, const char *who, int source, int outputs, int flags)
{
    if (source != PSM_DEPTH_GIF && source != PSM_DEPTH_SGM) return fail(e, "%s: source %d not in {0: PSM_DEPTH_GIF, 1: PSM_DEPTH_SGM}", who, source);
    if (outputs == 0) return fail(e, "%s: outputs == 0 (PSM_DEPTH_XYZ | PSM_DEPTH_Z | PSM_DEPTH_CLOUD: at least one)", who);
    if (outputs & ~DEPTH_OUTPUTS_ALL) return fail(e, "%s: unknown output bits 0x%x", who, outputs & ~DEPTH_OUTPUTS_ALL);
    if (flags & ~PSM_DEPTH_USE_MASK) return fail(e, "%s: unknown flag bits 0x%x", who, flags & ~PSM_DEPTH_USE_MASK);
    if ((flags & PSM_DEPTH_USE_MASK) && source != PSM_DEPTH_GIF)
        return fail(e, "%s: PSM_DEPTH_USE_MASK with an SGM source (the L-R mask belongs to the 8-bit maps)", who);
    return 0;
}

// ... and about one context; e: the context that receives the message (a batch: its first; who names the member)
int check_ctx(psm_ctx *e, const psm_ctx *c, const char *who, int source, int outputs, int flags)
{
    if (!c->depth.have_q) return fail(e, "%s: no Q set (psm_reproject_set_q)", who);
    if (source == PSM_DEPTH_GIF) {
        if (!c->res.maps) return fail(e, "%s: no disparity maps computed (PSM_DEPTH_GIF)", who);
        if (stripe_only(c)) return fail(e, "%s: the maps hold this context's row stripe only (gather the stripes first)", who);
        if ((flags & PSM_DEPTH_USE_MASK) && !c->res.mask) return fail(e, "%s: PSM_DEPTH_USE_MASK without a current L-R mask (psm_lr_check)", who);
    } else if (!sgm_source_exists(c)) {
        return fail(e, "%s: no SGM result (psm_sgm_compute) for an SGM source", who);
    }
    if ((outputs & PSM_DEPTH_CLOUD) && !colour_of(c, source == PSM_DEPTH_SGM).img)
        return fail(e, "%s: PSM_DEPTH_CLOUD without a current image pair (psm_upload_pair: the records take their colours from it)", who);
    return 0;
}

int ensure_scratch(psm_ctx *c, int outputs)
{
    DepthState &q = c->depth;
    const size_t HW = (size_t)c->W * c->H;
    if ((outputs & PSM_DEPTH_XYZ) && !q.xyz) PSM_HIP(c, hipMalloc((void **)&q.xyz, 12 * HW));
    if ((outputs & PSM_DEPTH_Z) && !q.z) PSM_HIP(c, hipMalloc((void **)&q.z, 4 * HW));
    if ((outputs & PSM_DEPTH_CLOUD) && !q.cloud) PSM_HIP(c, hipMalloc((void **)&q.cloud, 16 * HW));
    if (!q.tiles) PSM_HIP(c, hipMalloc((void **)&q.tiles, 2 * (size_t)dp_tiles(c->W, c->H) * sizeof(unsigned)));
    if (!q.cnt) PSM_HIP(c, hipMalloc((void **)&q.cnt, sizeof(unsigned)));
    if (!q.pin) PSM_HIP(c, hipHostMalloc((void **)&q.pin, sizeof(unsigned), hipHostMallocDefault));
    if (!q.ev_done) PSM_HIP(c, hipEventCreateWithFlags(&q.ev_done, hipEventDisableTiming));
    return bracket_events(c, q.prof);
}

// the context's buffers (ensure_scratch) and parameters as the kernels take them: the kernel argument, or an entry of a batch's table
DpArgs depth_args(const psm_ctx *c, int source, int outputs, int flags)
{
    const DepthState &q = c->depth;
    const Colour col = colour_of(c, source == PSM_DEPTH_SGM);
    DpArgs a = {};
    a.map = c->maps;
    a.valid = (flags & PSM_DEPTH_USE_MASK) ? c->valid : nullptr;
    a.d16 = sgm_source_map(c);
    a.img = col.img;
    a.xyz = (outputs & PSM_DEPTH_XYZ) ? q.xyz : nullptr;
    a.z = (outputs & PSM_DEPTH_Z) ? q.z : nullptr;
    a.cloud = (outputs & PSM_DEPTH_CLOUD) ? q.cloud : nullptr;
    a.tile_cnt = q.tiles;
    a.tile_off = q.tiles + dp_tiles(c->W, c->H);
    a.total = q.cnt;
    memcpy(a.Q, q.Q, sizeof a.Q);
    a.crop_x = q.crop_x; a.crop_y = q.crop_y;
    a.z_min = q.z_min; a.z_max = q.z_max;
    a.invalid = sgm_source_invalid(c);
    a.depth = col.depth; a.ch = col.ch;
    return a;
}

// the count of the last run, its copy having executed
int count_of(psm_ctx *c, uint32_t *count)
{
    PSM_HIP(c, hipEventSynchronize(c->depth.ev_done));
    *count = *c->depth.pin;
    return 0;
}

// The host sequence of psm_reproject (its one context, the record by value) and of psm_reproject_batch (batch: the same kernels
// over the device table of ctxs[0]), the arguments and every context checked: two or three launches on ctxs[0]'s stream.  Every
// context ends where its own psm_reproject would have left it, its count in its page-locked slot unless the call is asynchronous.
int reproject_run(const char *who, psm_ctx *const *ctxs, int n, int source, int outputs, int flags, bool batch)
{
    psm_ctx *c0 = ctxs[0];
    if (bind(c0)) return 1;
    hipStream_t s = c0->stream;
    DepthState &t = c0->depth;
    const bool cloud = (outputs & PSM_DEPTH_CLOUD) != 0;

    // ---- buffers, events and the table's memory: before any launch ----
    for (int i = 0; i < n; ++i)
        if (ensure_scratch(ctxs[i], outputs)) return member_failed(c0, who, i, ctxs[i]);
    if (batch_events(c0, ctxs, n)) return 1;
    std::vector<DpArgs> tab((size_t)n);
    for (int i = 0; i < n; ++i) tab[i] = depth_args(ctxs[i], source, outputs, flags);
    bool fresh = false;
    if (batch && table_reserve(c0, t.tab, tab.data(), tab.size() * sizeof(DpArgs), &fresh)) return 1;
    const Recs<DpArgs> recs{tab.data(), batch ? (const DpArgs *)t.tab.dev : nullptr, n};

    // ---- every context's earlier work (the result to reproject, a single psm_reproject) is ordered before the shared launches ----
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, t.tab, tab.data(), tab.size() * sizeof(DpArgs))) return 1;

    for (int i = 0; i < n; ++i) {
        DepthState &q = ctxs[i]->depth;
        q.outputs = 0;                          // (every check and allocation lies before this: the planes are about to be rewritten)
        q.pending = q.prof.timed = false;
        PSM_HIP(c0, hipMemsetAsync(q.cnt, 0, sizeof(unsigned), s));
    }
    const DpGeom g{c0->W, c0->H, source};
    if (bracket_open(c0, t.prof, s)) return 1;
    launch_dp_count(s, g, recs);
    launch_dp_scan(s, g, recs);
    if (cloud) launch_dp_pack(s, g, recs);
    if (check_launch(c0, "k_dp_count, k_dp_scan, k_dp_pack")) return 1;
    if (bracket_close(c0, t.prof, s)) return 1;

    // ---- every context is now where its own psm_reproject would have left it; only context 0 counts as timed ----
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if (cloud && colour_of(c, source == PSM_DEPTH_SGM).slots && images_read(c, s)) return member_failed(c0, who, i, c);   // k_dp_pack read the pair's left image
        PSM_HIP(c0, hipMemcpyAsync(c->depth.pin, c->depth.cnt, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        PSM_HIP(c0, hipEventRecord(c->depth.ev_done, s));
    }
    if (batch_fork(c0, ctxs, n)) return 1;
    for (int i = 0; i < n; ++i) {
        ctxs[i]->depth.outputs = outputs;
        ctxs[i]->depth.pending = c0->opt_async != 0;
    }
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(s));
    return 0;
}

}  // namespace

extern "C" {

int psm_reproject_set_q(psm_ctx *c, const double Q[16], int crop_x, int crop_y)
{
    if (!Q) return fail(c, "psm_reproject_set_q: NULL Q");      // (without a context the messages are psm_last_error(NULL)'s)
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(Q[i])) return fail(c, "psm_reproject_set_q: Q[%d][%d] is not finite", i / 4, i % 4);
    if (crop_x < -32768 || crop_x > 32767 || crop_y < -32768 || crop_y > 32767)
        return fail(c, "psm_reproject_set_q: crop (%d, %d) outside [-32768, 32767]", crop_x, crop_y);
    if (!c) return fail(nullptr, "psm_reproject_set_q: NULL context");
    DepthState &q = c->depth;
    memcpy(q.Q, Q, sizeof q.Q);
    q.crop_x = crop_x; q.crop_y = crop_y;
    q.have_q = true;
    return 0;
}

int psm_reproject_set_range(psm_ctx *c, float z_min, float z_max)
{
    if (!(z_min < z_max))                                       // (NaN compares false)
        return fail(c, "psm_reproject_set_range: z_min %g is not below z_max %g (or one of them is NaN)", (double)z_min, (double)z_max);
    if (!c) return fail(nullptr, "psm_reproject_set_range: NULL context");
    c->depth.z_min = z_min;
    c->depth.z_max = z_max;
    return 0;
}

int psm_reproject(psm_ctx *c, int source, int outputs, int flags, uint32_t *count)
{
    const char *who = "psm_reproject";
    if (check_call(c, who, source, outputs, flags)) return 1;
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_ctx(c, c, who, source, outputs, flags)) return 1;
    if (!count && !c->opt_async) return fail(c, "%s: NULL count (only PSM_OPT_ASYNC leaves it to psm_reproject_wait)", who);
    if (reproject_run(who, &c, 1, source, outputs, flags, false)) return 1;
    if (!c->opt_async) *count = *c->depth.pin;
    return 0;
}

int psm_reproject_wait(psm_ctx *c, uint32_t *count)
{
    if (!c) return fail(nullptr, "psm_reproject_wait: NULL context");
    if (!count) return fail(c, "psm_reproject_wait: NULL count");
    if (!c->depth.pending) return fail(c, "psm_reproject_wait: no asynchronous psm_reproject started");
    if (bind(c)) return 1;
    if (count_of(c, count)) return 1;
    c->depth.pending = false;
    return 0;
}

int psm_reproject_download(psm_ctx *c, float *xyz, float *z, size_t stride_bytes)
{
    if (!c) return fail(nullptr, "psm_reproject_download: NULL context");
    const size_t row = (size_t)c->W * sizeof(float);
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row || stride_bytes % 4) return fail(c, "psm_reproject_download: stride %zu: a multiple of 4, at least the row size %zu", stride_bytes, row);
    const DepthState &q = c->depth;
    if (!q.outputs) return fail(c, "psm_reproject_download: no psm_reproject ran (or its planes were released)");
    if (xyz && !(q.outputs & PSM_DEPTH_XYZ)) return fail(c, "psm_reproject_download: the last psm_reproject had no PSM_DEPTH_XYZ among its outputs");
    if (z && !(q.outputs & PSM_DEPTH_Z)) return fail(c, "psm_reproject_download: the last psm_reproject had no PSM_DEPTH_Z among its outputs");
    if (bind(c)) return 1;
    if (xyz && d2h_rows(c, xyz, q.xyz, 3 * row, 3 * stride_bytes, c->H)) return 1;
    if (z && d2h_rows(c, z, q.z, row, stride_bytes, c->H)) return 1;
    return 0;
}

int psm_reproject_download_cloud(psm_ctx *c, void *records, uint32_t max_records, uint32_t *written)
{
    if (!c) return fail(nullptr, "psm_reproject_download_cloud: NULL context");
    const DepthState &q = c->depth;
    if (!q.outputs) return fail(c, "psm_reproject_download_cloud: no psm_reproject ran (or its planes were released)");
    if (!(q.outputs & PSM_DEPTH_CLOUD)) return fail(c, "psm_reproject_download_cloud: the last psm_reproject had no PSM_DEPTH_CLOUD among its outputs");
    if (bind(c)) return 1;
    uint32_t n = 0;
    if (count_of(c, &n)) return 1;
    if (max_records < n) return fail(c, "psm_reproject_download_cloud: max_records %u below the count %u", max_records, n);
    if (n && !records) return fail(c, "psm_reproject_download_cloud: NULL records");
    if (n) {
        PSM_HIP(c, hipMemcpyAsync(records, q.cloud, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
        PSM_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (written) *written = n;
    return 0;
}

// The launches of psm_reproject with the context on a grid axis of its own (reproject_run).  Buffers and parameters stay per
// context; the kernels reach them through a device table ctxs[0] owns.
int psm_reproject_batch(psm_ctx *const *ctxs, int n, int source, int outputs, int flags, uint32_t *counts)
{
    const char *who = "psm_reproject_batch";
    if (!ctxs || n < 1 || !ctxs[0]) return fail(nullptr, "%s: bad arguments", who);
    psm_ctx *c0 = ctxs[0];
    if (n > 4096) return fail(c0, "%s: %d contexts (at most 4096 per call)", who, n);
    if (check_call(c0, who, source, outputs, flags)) return 1;
    if (!counts && !c0->opt_async) return fail(c0, "%s: NULL counts (only PSM_OPT_ASYNC leaves them to psm_reproject_wait)", who);
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        psm_ctx *c = ctxs[i];
        if (c->W != c0->W || c->H != c0->H || c->device != c0->device)
            return fail(c0, "%s: context %d has another width / height / device than context 0", who, i);
        char member[64];
        snprintf(member, sizeof member, "%s: context %d", who, i);
        if (check_ctx(c0, c, member, source, outputs, flags)) return 1;
    }
    if (reproject_run(who, ctxs, n, source, outputs, flags, true)) return 1;
    for (int i = 0; i < n && !c0->opt_async; ++i) counts[i] = *ctxs[i]->depth.pin;
    return 0;
}

int psm_reproject_time(psm_ctx *c, double *ms)
{
    if (!c) return fail(nullptr, "psm_reproject_time: NULL context");
    return bracket_ms(c, c->depth.prof, c->depth.outputs != 0, "psm_reproject_time", "the last psm_reproject was not timed (PSM_OPT_PROFILE)", ms);
}

}  // extern "C"
