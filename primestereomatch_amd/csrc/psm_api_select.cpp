// psm_api_select.cpp - DispSelect behind the C ABI: the two u8 maps, the packed per-pixel minima a sharded job exchanges,
// row stripes and disparity shards, and the D2H leg of the maps.  Replaces DispSel_cl::CVSelect
// (src/DispSel_cl.cpp:69-140) as called by DispEst::DispSelect_GPU (src/DispEst.cpp:323-328); arithmetic of
// DispSel::CVSelect (src/DispSel.cpp:83-109).
#include "psm_ctx.h"

#include <cstring>

using namespace psm;

namespace psm {

// Two [H][W] planes in a page-locked buffer into the caller's (pageable, possibly strided) rows: the row stride the caller
// means (0: packed rows), refused when it is shorter than a row, and the copy
static int rows_out(psm_ctx *c, size_t &stride, const uint8_t *pin = nullptr, uint8_t *lmap = nullptr, uint8_t *rmap = nullptr)
{
    const size_t W = (size_t)c->W, HW = W * c->H;
    if (stride == 0) stride = W;
    if (stride < W) return fail(c, "map stride %zu < width %d", stride, c->W);
    uint8_t *dst[2] = {lmap, rmap};
    for (int s = 0; s < 2 && pin; ++s) {
        if (!dst[s]) continue;
        const uint8_t *src = pin + s * HW;
        if (stride == W) memcpy(dst[s], src, HW);
        else for (int y = 0; y < c->H; ++y) memcpy(dst[s] + (size_t)y * stride, src + (size_t)y * W, W);
    }
    return 0;
}

int copy_maps_out(psm_ctx *c, const uint8_t *dev, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    const size_t HW = (size_t)c->W * c->H;
    if (rows_out(c, stride)) return 1;          // (the stride alone: nothing is started for one that is refused)
    if (!lmap && !rmap) return 0;
    // device -> page-locked bounce buffer (one DMA at link speed) -> the caller's (pageable, possibly strided) rows.
    // A direct copy into pageable memory took 6-16 ms for two 1080p maps; this way it is ~0.5 ms.
    if (!c->pinned && hipHostMalloc((void **)&c->pinned, 2 * HW, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        c->pinned = nullptr;
    }
    if (!c->pinned) {   // no page-locked memory: plain copies
        if (lmap) PSM_HIP(c, hipMemcpy2DAsync(lmap, stride, dev, c->W, c->W, c->H, hipMemcpyDeviceToHost, c->stream));
        if (rmap) PSM_HIP(c, hipMemcpy2DAsync(rmap, stride, dev + HW, c->W, c->W, c->H, hipMemcpyDeviceToHost, c->stream));
        PSM_HIP(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    if (lmap && rmap) PSM_HIP(c, hipMemcpyAsync(c->pinned, dev, 2 * HW, hipMemcpyDeviceToHost, c->stream));
    else if (lmap) PSM_HIP(c, hipMemcpyAsync(c->pinned, dev, HW, hipMemcpyDeviceToHost, c->stream));
    else PSM_HIP(c, hipMemcpyAsync(c->pinned + HW, dev + HW, HW, hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    return rows_out(c, stride, c->pinned, lmap, rmap);
}

}  // namespace psm

namespace {

// WTA of one side into keys_s (may be NULL) and / or map_s (may be NULL).  A side whose Fast-Guided-Filter result is
// still virtual is selected straight from the smoothed models (upsample + linear model + argmin in one pass).
int wta_side(psm_ctx *c, int s, long long *keys_s, uint8_t *map_s)
{
    const size_t HW = (size_t)c->W * c->H;
    Prof p(c, PSM_K_WTA);
    long long *const cur = c->keys_cur + s * HW, *const k = keys_s ? keys_s : cur;
    switch (c->vside[s].pending) {
    case VolSide::KEYS:         // the select-mode filter already reduced this side: `cur` holds the packed minima over the local slices
        if (k != cur) PSM_HIP(c, hipMemcpyAsync(k, cur, HW * sizeof(long long), hipMemcpyDeviceToDevice, c->stream));
        if (map_s) launch_merge(c->stream, cur, HW, 1, (int)HW, map_s);
        break;
    case VolSide::FGF:
        launch_fgf_apply_wta(c->stream, c->g[s].g1, c->W, c->H, c->Dloc, c->d0, pending_fgf(c->vside[s]), c->fgf_mab[s], k);
        if (map_s) launch_merge(c->stream, k, HW, 1, (int)HW, map_s);
        break;
    case VolSide::NOTHING:      // (real memory: wta_ready)
        if (c->dtype == PSM_U8) launch_wta_u8(c->stream, (const uint8_t *)c->vol[s], c->W, c->H, c->d0, c->Dloc, keys_s, map_s);
        else launch_wta(c->stream, (const float *)c->vol[s], c->W, c->H, c->d0, c->Dloc, keys_s, map_s);
        break;
    }
    return 0;
}

int wta_launch(psm_ctx *c, long long *keys, uint8_t *maps)
{
    const size_t HW = (size_t)c->W * c->H;
    // the map buffer may still be the source of an asynchronous download of the previous frame
    if (maps && maps_writable(c)) return 1;
    // a side that is not the select filter's packed minima was selected from a whole volume: its map is whole
    const bool both_keys = pending_keys(c->vside[0]) && pending_keys(c->vside[1]);
    if (!both_keys) cover(c->res, whole_image(c));
    else cover_filtered(c->res);                  // (maps uploaded, gathered or selected by the SGM stage in between covered the whole image)
    if (both_keys && !keys && maps) {             // both sides already reduced to keys: one launch for both maps
        if (take_early(c->res, maps)) return 0;   // ... unless the filter's reduction wrote them already (once: post-processing rewrites the maps in place)
        Prof p(c, PSM_K_WTA);
        launch_merge(c->stream, c->keys_cur, 2 * HW, 1, (int)(2 * HW), maps);
        return check_launch(c, "wta");
    }
    for (int s = 0; s < 2; ++s)
        if (wta_side(c, s, keys ? keys + s * HW : nullptr, maps ? maps + s * HW : nullptr)) return 1;
    return check_launch(c, "wta");
}

// the volume a WTA is about to read: real data, or a virtual result (consumed without materialising it)
int wta_ready(psm_ctx *c, int side)
{
    return c->vside[side].pending != VolSide::NOTHING ? 0 : materialize(c, side);
}

}  // namespace

extern "C" {

int psm_disp_select(psm_ctx *c, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    if (c->Dloc != c->D) return fail(c, "psm_disp_select: context holds slices [%d,%d) of %d; use psm_disp_select_partial + psm_disp_merge", c->d0, c->d1, c->D);
    if (!c->have_cost) return fail(c, "psm_disp_select: no cost volume");
    if (bind(c)) return 1;
    const double t0 = now_us();
    if (wta_ready(c, 0) || wta_ready(c, 1)) return 1;
    if (wta_launch(c, nullptr, c->maps)) return 1;
    maps_written(c->res);
    if (copy_maps_out(c, c->maps, lmap, rmap, stride)) return 1;
    return end_stage(c, PSM_STAGE_DISPSEL, t0);
}

int psm_disp_select_partial(psm_ctx *c, void *dev_keys)
{
    if (!c) return 1;
    if (!c->have_cost) return fail(c, "psm_disp_select_partial: no cost volume");
    if (bind(c)) return 1;
    const double t0 = now_us();
    if (wta_ready(c, 0) || wta_ready(c, 1)) return 1;
    if (wta_launch(c, dev_keys ? (long long *)dev_keys : c->keys_cur, nullptr)) return 1;
    if (!dev_keys) { keys_complete(c->res, 0); keys_complete(c->res, 1); }
    return end_stage(c, PSM_STAGE_DISPSEL, t0);
}

int psm_disp_select_partial_side(psm_ctx *c, int side, void *dev_keys_side)
{
    if (!c) return 1;
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "psm_disp_select_partial_side: bad side %d", side);
    if (!c->have_cost) return fail(c, "psm_disp_select_partial_side: no cost volume");
    if (bind(c)) return 1;
    const double t0 = now_us();
    if (wta_ready(c, side)) return 1;
    const size_t HW = (size_t)c->W * c->H;
    long long *keys = dev_keys_side ? (long long *)dev_keys_side : c->keys_cur + side * HW;
    if (wta_side(c, side, keys, nullptr)) return 1;
    if (check_launch(c, "wta")) return 1;
    if (!dev_keys_side) keys_complete(c->res, side);
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    c->stage_us[PSM_STAGE_DISPSEL] = (side == PSM_LEFT ? 0.0 : c->stage_us[PSM_STAGE_DISPSEL]) + (now_us() - t0);
    return 0;
}

int psm_set_rows(psm_ctx *c, int y_begin, int y_end)
{
    if (!c) return 1;
    // (takes effect with the next psm_cost_filter; minima / maps already computed keep describing the stripe they were made
    // for - Results::rows, recorded when they were filtered)
    if (y_begin == 0 && (y_end == 0 || y_end == c->H)) {   // whole image
        c->march.ybeg = c->march.yend = 0;
        return 0;
    }
    if (y_begin < 0 || y_end > c->H || y_begin >= y_end) return fail(c, "psm_set_rows: bad stripe [%d,%d) of %d rows", y_begin, y_end, c->H);
    c->march.ybeg = y_begin;
    c->march.yend = y_end;
    return 0;
}

int psm_set_map_buffer(psm_ctx *c, void *dev_maps, int whole)
{
    if (!c) return 1;
    uint8_t *m = dev_maps ? (uint8_t *)dev_maps : c->maps_own;
    if (m != c->maps) maps_gone(c->res);
    forget_early(c->res);
    c->maps = m;
    if (whole) {    // the caller filled the buffer with both complete maps of the current frame (e.g. gathered row stripes)
        cover(c->res, whole_image(c));
        maps_written(c->res);
    }
    return 0;
}

// One leg of the single-process exchange (psm_gather_rows_ctx / psm_disp_merge_ctx): n bytes of context s (its stream already
// synchronised) into root's memory, ordered on root's stream.  Same device: a device copy.  Other device: a peer copy when
// hipDeviceCanAccessPeer(root, s) says the two can reach each other (xGMI / PCIe P2P), else - or with PSM_OPT_GATHER_STAGED, the
// test hook for exactly this path on a one-GPU box - through a page-locked bounce buffer of root: device -> host on s's device,
// host -> device on root's stream (two buffers used alternately: the next leg's device -> host copy overlaps this leg's host -> device
// copy, a slot is refilled only after the copy out of it has executed - the slow but always available way).
static int gather_leg(psm_ctx *root, void *dst, psm_ctx *s, const void *src, size_t n)
{
    bool staged = root->opt_gather_staged != 0;
    if (!staged && s->device != root->device) {
        signed char &ok = root->peer_ok[s->device & 63];      // asked once per device pair, not on every leg of every frame
        if (ok < 0) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, root->device, s->device) != hipSuccess) { can = 0; (void)hipGetLastError(); }
            ok = can ? 1 : 0;
        }
        staged = !ok;
    }
    if (!staged) {
        if (s->device == root->device) PSM_HIP(root, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, root->stream));
        else PSM_HIP(root, hipMemcpyPeerAsync(dst, root->device, src, s->device, n, root->stream));
        return 0;
    }
    const int k = root->xfer_slot;
    root->xfer_slot ^= 1;
    if (!root->ev_xfer[k]) PSM_HIP(root, hipEventCreateWithFlags(&root->ev_xfer[k], hipEventDisableTiming));
    else PSM_HIP(root, hipEventSynchronize(root->ev_xfer[k]));    // the copy out of this slot (two legs ago) has executed
    if (root->xfer_pin_bytes[k] < n) {
        if (root->xfer_pin[k]) (void)hipHostFree(root->xfer_pin[k]);
        root->xfer_pin[k] = nullptr;
        root->xfer_pin_bytes[k] = 0;
        PSM_HIP(root, hipHostMalloc((void **)&root->xfer_pin[k], n, hipHostMallocPortable));    // (portable: both devices copy to / from it)
        root->xfer_pin_bytes[k] = n;
    }
    (void)hipSetDevice(s->device);
    const hipError_t e = hipMemcpy(root->xfer_pin[k], src, n, hipMemcpyDeviceToHost);    // (blocking: the slot is complete when it returns)
    (void)hipSetDevice(root->device);
    if (e != hipSuccess) return fail(root, "exchange leg (device %d -> host): %s", s->device, hipGetErrorString(e));
    PSM_HIP(root, hipMemcpyAsync(dst, root->xfer_pin[k], n, hipMemcpyHostToDevice, root->stream));
    PSM_HIP(root, hipEventRecord(root->ev_xfer[k], root->stream));
    ++root->gather_staged_legs;
    return 0;
}

// ... first: everything context s has enqueued on its stream (on its device) has executed
static int sync_other(psm_ctx *root, psm_ctx *s)
{
    (void)hipSetDevice(s->device);
    PSM_HIP(root, hipStreamSynchronize(s->stream));
    (void)hipSetDevice(root->device);
    return 0;
}

int psm_gather_rows_ctx(psm_ctx *root, psm_ctx *const *stripes, int nstripes, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!root) return 1;
    if (!stripes || nstripes < 1) return fail(root, "psm_gather_rows_ctx: bad arguments");
    std::vector<char> covered((size_t)root->H, 0);
    // (which rows a context's maps hold: the stripe they were FILTERED with - Results::rows -, not what psm_set_rows says now)
    for (int i = 0; i < nstripes; ++i) {
        const psm_ctx *s = stripes[i];
        if (!s || s->W != root->W || s->H != root->H || s->D != root->D || s->dtype != root->dtype)
            return fail(root, "psm_gather_rows_ctx: stripe %d does not belong to this job", i);
        if (!s->res.maps) return fail(root, "psm_gather_rows_ctx: stripe %d has no maps for this frame (call psm_disp_select first)", i);
        for (int y = s->res.rows.y0; y < s->res.rows.y1; ++y) {
            if (covered[y]) return fail(root, "psm_gather_rows_ctx: row %d is held by more than one stripe", y);
            covered[y] = 1;
        }
    }
    for (int y = 0; y < root->H; ++y)
        if (!covered[y]) return fail(root, "psm_gather_rows_ctx: no stripe holds row %d", y);
    if (bind(root) || maps_writable(root)) return 1;
    const size_t HW = (size_t)root->W * root->H;
    for (int i = 0; i < nstripes; ++i) {
        psm_ctx *s = stripes[i];
        if (s == root) continue;
        if (sync_other(root, s)) return 1;                  // the stripe's maps must be complete before they are read
        const size_t o = (size_t)s->res.rows.y0 * root->W, n = (size_t)(s->res.rows.y1 - s->res.rows.y0) * root->W;
        for (int side = 0; side < 2; ++side)
            if (gather_leg(root, root->maps + side * HW + o, s, s->maps + side * HW + o, n)) return 1;
    }
    cover(root->res, whole_image(root));      // the root's maps are whole now
    forget_early(root->res);                  // (a single-phase filter of the root's own, not selected yet, no longer finds its maps there)
    maps_written(root->res);
    if (copy_maps_out(root, root->maps, lmap, rmap, stride)) return 1;
    if (!root->opt_async) PSM_HIP(root, hipStreamSynchronize(root->stream));
    return 0;
}

int psm_gather_staged_legs(const psm_ctx *root) { return root ? root->gather_staged_legs : -1; }

int psm_set_key_buffer(psm_ctx *c, void *dev_keys)
{
    if (!c) return 1;
    long long *k = dev_keys ? (long long *)dev_keys : c->keys;
    if (k != c->keys_cur && (pending_keys(c->vside[0]) || pending_keys(c->vside[1])))
        return fail(c, "psm_set_key_buffer: the current minima are still pending in the previous buffer (call before psm_cost_filter)");
    c->keys_cur = k;
    return 0;
}

int psm_partial_keys(psm_ctx *c, void **dev_keys, size_t *bytes)
{
    if (!c) return 1;
    if (dev_keys) *dev_keys = c->keys_cur;
    if (bytes) *bytes = 2 * (size_t)c->W * c->H * sizeof(long long);
    return 0;
}

int psm_disp_merge(psm_ctx *c, const void *dev_keys_all, int nranks, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    if (!dev_keys_all || nranks < 1) return fail(c, "psm_disp_merge: bad arguments");
    if (bind(c)) return 1;
    const double t0 = now_us();
    const size_t n = 2 * (size_t)c->W * c->H;
    if (maps_writable(c)) return 1;
    {
        Prof p(c, PSM_K_MERGE);
        launch_merge(c->stream, (const long long *)dev_keys_all, n, nranks, (int)n, c->maps);
    }
    if (check_launch(c, "merge")) return 1;
    // (the merged keys are those of this job's shards, filtered under the stripe this context recorded - Results::rows
    // stay as psm_cost_filter left them: stripes of disparity shards merge to a stripe)
    forget_early(c->res);                     // (as above: the merged maps replaced what the context's own filter had put there)
    maps_written(c->res);
    if (copy_maps_out(c, c->maps, lmap, rmap, stride)) return 1;
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    c->stage_us[PSM_STAGE_DISPSEL] += now_us() - t0;
    return 0;
}

int psm_disp_merge_ctx(psm_ctx *root, psm_ctx *const *shards, int nshards, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!root) return 1;
    if (!shards || nshards < 1) return fail(root, "psm_disp_merge_ctx: bad arguments");
    const size_t bytes = 2 * (size_t)root->W * root->H * sizeof(long long);
    std::vector<char> covered((size_t)root->D, 0);
    for (int i = 0; i < nshards; ++i) {
        const psm_ctx *s = shards[i];
        if (!s || s->W != root->W || s->H != root->H || s->D != root->D || s->dtype != root->dtype)
            return fail(root, "psm_disp_merge_ctx: shard %d does not belong to this job", i);
        if (!(s->res.keys[0] && s->res.keys[1]))
            return fail(root, "psm_disp_merge_ctx: shard %d has no partial minima for this frame (call psm_disp_select_partial(ctx, NULL) first)", i);
        if (!(s->res.rows == shards[0]->res.rows))
            return fail(root, "psm_disp_merge_ctx: shard %d was filtered under another row stripe than shard 0", i);
        for (int d = s->d0; d < s->d1; d += s->march.dstep) {       // (a strided shard holds d0, d0 + dstep, ...)
            if (covered[d]) return fail(root, "psm_disp_merge_ctx: slice %d is held by more than one shard", d);
            covered[d] = 1;
        }
    }
    for (int d = 0; d < root->D; ++d)
        if (!covered[d]) return fail(root, "psm_disp_merge_ctx: no shard holds slice %d", d);
    if (bind(root)) return 1;
    if (root->gather_ranks < nshards) {
        PSM_HIP(root, hipStreamSynchronize(root->stream));
        (void)hipFree(root->gather);
        root->gather = nullptr;
        root->gather_ranks = 0;
        PSM_HIP(root, hipMalloc((void **)&root->gather, bytes * nshards));
        root->gather_ranks = nshards;
    }
    for (int i = 0; i < nshards; ++i) {
        psm_ctx *s = shards[i];
        if (sync_other(root, s)) return 1;      // the shard's partial WTA must have finished before its keys are read
        if (gather_leg(root, (char *)root->gather + bytes * i, s, s->keys_cur, bytes)) return 1;
    }
    // the merged maps cover what the shards' minima cover
    cover(root->res, shards[0]->res.rows);
    return psm_disp_merge(root, root->gather, nshards, lmap, rmap, stride);
}

int psm_download_maps(psm_ctx *c, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    if (!c->res.maps) return fail(c, "psm_download_maps: no disparity maps computed");
    if (bind(c)) return 1;
    return copy_maps_out(c, c->maps, lmap, rmap, stride);
}

// Frame loop: the D2H leg of frame i next to the kernels of frame i+1.  psm_download_maps_async starts the copy of the
// current maps into page-locked memory on the copy stream (after the kernels that produce them, before any later kernel
// overwrites them); psm_download_maps_wait hands them to the caller.  One download may be in flight.
int psm_download_maps_async(psm_ctx *c)
{
    if (!c) return 1;
    if (!c->res.maps) return fail(c, "psm_download_maps_async: no disparity maps computed");
    if (bind(c)) return 1;
    const size_t HW = (size_t)c->W * c->H;
    if (!c->copy_stream) PSM_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->down_stream) c->down_stream = c->copy_stream;
    for (hipEvent_t *e : {&c->ev_maps, &c->ev_down})
        if (!*e) PSM_HIP(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    if (!c->pinned2) PSM_HIP(c, hipHostMalloc((void **)&c->pinned2, 2 * HW, hipHostMallocDefault));
    PSM_HIP(c, hipEventRecord(c->ev_maps, c->stream));
    PSM_HIP(c, hipStreamWaitEvent(c->down_stream, c->ev_maps, 0));
    if (((uintptr_t)c->maps & 15) == 0 && 2 * HW <= PSM_COPY_KERNEL_MAX) {     // small maps: a kernel writing page-locked host memory (k_copy16; see psm_upload_pair_async)
        launch_copy_bytes(c->down_stream, c->pinned2, c->maps, 2 * HW);
        if (check_launch(c, "download (copy kernel)")) return 1;
    } else PSM_HIP(c, hipMemcpyAsync(c->pinned2, c->maps, 2 * HW, hipMemcpyDeviceToHost, c->down_stream));
    PSM_HIP(c, hipEventRecord(c->ev_down, c->down_stream));
    return 0;
}

int psm_download_maps_wait(psm_ctx *c, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    if (!c->ev_down || !c->pinned2) return fail(c, "psm_download_maps_wait: no asynchronous download started");
    if (rows_out(c, stride)) return 1;
    if (bind(c)) return 1;
    PSM_HIP(c, hipEventSynchronize(c->ev_down));
    return rows_out(c, stride, c->pinned2, lmap, rmap);
}

}  // extern "C"
