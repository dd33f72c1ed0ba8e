// psm_api_gray.cpp - the guided-filter path over a one-channel pair behind the C ABI: cost build, one-channel guided filter and
// winner-takes-all of two host planes in one call (psm_gray_compute; psm_gray.hip), the reading of GuidedFilter_cv (src/CVF.cpp:72-165)
// that FastGuidedFilter's dispatch on I.channels() intends (src/fastguidedfilter.cpp:38-49,89-119).  The definition is
// tests/gray_model.py / DESIGN.md 14.  An independent stage like the SGM one: it stages its own planes and writes its own buffers
// (psm::GrayState); it meets the rest where psm_sgm_select_maps does - the context's two current 8-bit maps (psm::Results) - so the
// L-R check, the fill, psm_score, the downloads and psm_reproject run behind it.  The image pair slots, the volume sides and the
// packed minima of the colour path never see it.
// No volume exists: per chunk of gray_plan().dc slices k_gray_ab leaves {a, b} in the chunk scratch and k_gray_q folds q into the
// stage's key plane; launch_merge turns the keys into the maps.  The test hooks run the storing form of the same kernels.
#include "psm_ctx.h"

#include <algorithm>
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
    bracket_free(g.prof);
    g.depth = -1;
}

}  // namespace psm

namespace {

// what a context must be for the stage; who: the call
int check_ctx(psm_ctx *c, const char *who)
{
    if (c->dtype == PSM_U8) return fail(c, "%s: an 8-bit context (PSM_U8): the one-channel filter is a float-mode stage", who);
    if (c->Dloc != c->D || strided(c)) return fail(c, "%s: a disparity shard holds part of the range (the stage selects over every disparity)", who);
    if (c->march.yend > c->march.ybeg) return fail(c, "%s: a row stripe is in force (psm_set_rows): the maps are whole-image maps", who);
    return 0;
}

int ensure_buffers(psm_ctx *c, const GrayPlan &pl)
{
    GrayState &g = c->gray;
    const size_t HW = (size_t)c->W * c->H;
    for (int s = 0; s < 2; ++s) {
        if (!g.raw[s]) PSM_HIP(c, hipMalloc(&g.raw[s], HW * sizeof(float)));
        if (!g.ig[s]) PSM_HIP(c, hipMalloc((void **)&g.ig[s], HW * sizeof(float2)));
        if (!g.mv[s]) PSM_HIP(c, hipMalloc((void **)&g.mv[s], HW * sizeof(float2)));
    }
    if (!g.ab) PSM_HIP(c, hipMalloc((void **)&g.ab, 2 * (size_t)pl.dc * HW * sizeof(float2)));
    if (!g.keys) PSM_HIP(c, hipMalloc((void **)&g.keys, 2 * HW * sizeof(long long)));
    return 0;
}

GrayPair pair_of(const psm_ctx *c)
{
    const GrayState &g = c->gray;
    return GrayPair{{g.raw[0], g.raw[1]}, {g.ig[0], g.ig[1]}, {g.mv[0], g.mv[1]}, g.ab, g.keys};
}

// the hooks: the planes of a psm_gray_compute must exist
int check_hook(psm_ctx *c, const char *who, int side)
{
    if (check_ctx(c, who)) return 1;
    if (c->gray.depth < 0) return fail(c, "%s: no pair (psm_gray_compute; psm_release_scratch gives it back)", who);
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "%s: bad side %d", who, side);
    return 0;
}

}  // namespace

extern "C" {

int psm_gray_compute(psm_ctx *c, const void *l, const void *r, size_t stride_bytes, int depth, uint8_t *lmap, uint8_t *rmap, size_t map_stride)
{
    const char *who = "psm_gray_compute";
    if (!c) return fail(nullptr, "%s: NULL context", who);
    if (check_ctx(c, who)) return 1;
    if (!l || !r) return fail(c, "%s: NULL image", who);
    if (depth != PSM_IMG_U8 && depth != PSM_IMG_F32) return fail(c, "%s: unknown depth %d", who, depth);
    const size_t row = (size_t)c->W * (depth == PSM_IMG_F32 ? sizeof(float) : 1);
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row) return fail(c, "%s: stride %zu < row size %zu", who, stride_bytes, row);
    if (map_stride != 0 && map_stride < (size_t)c->W) return fail(c, "%s: map stride %zu < width %d", who, map_stride, c->W);
    if (bind(c)) return 1;
    GrayState &g = c->gray;
    const GrayPlan pl = gray_plan(c->W, c->H, c->D);
    if (ensure_buffers(c, pl) || bracket_events(c, g.prof)) return 1;

    // ---- the pair: the planes of an earlier call are gone from here on ----
    g.depth = -1;
    g.prof.timed = false;
    const void *src[2] = {l, r};
    for (int s = 0; s < 2; ++s)
        if (h2d_rows(c, g.raw[s], src[s], row, stride_bytes, c->H)) return 1;
    PSM_HIP(c, hipStreamSynchronize(c->stream));      // the copy reads caller memory (psm_upload_pair)

    // ---- the launches: guidance and empty keys, the chunks of the slices 1 .. D - 1 (d = 0 is never a candidate), the maps ----
    if (maps_writable(c)) return 1;
    const GrayPair p = pair_of(c);
    const size_t HW = (size_t)c->W * c->H;
    if (bracket_open(c, g.prof, c->stream)) return 1;
    launch_gray_prep(c->stream, p, pl, c->W, c->H, depth == PSM_IMG_F32);
    if (check_launch(c, "k_gray_prep")) return 1;
    for (int d = 1; d < c->D; d += pl.dc) launch_gray_chunk(c->stream, p, pl, c->W, c->H, 0, 2, d, std::min(c->D, d + pl.dc), nullptr);
    if (check_launch(c, "k_gray_ab, k_gray_q")) return 1;
    launch_merge(c->stream, g.keys, 2 * HW, 1, (int)(2 * HW), c->maps);
    if (check_launch(c, "k_merge")) return 1;
    if (bracket_close(c, g.prof, c->stream)) return 1;

    // ---- the context is where psm_sgm_select_maps leaves it: whole-image maps, no mask, no early map; the volume sides, the
    // packed minima and whatever the colour path has pending are not touched ----
    g.depth = depth;
    forget_early(c->res);
    cover(c->res, whole_image(c));
    maps_written(c->res);
    if (copy_maps_out(c, c->maps, lmap, rmap, map_stride)) return 1;
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
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
        launch_gray_chunk(c->stream, p, pl, c->W, c->H, side, 1, d, e, qdev);
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

int psm_gray_time(psm_ctx *c, double *ms)
{
    if (!c) return fail(nullptr, "psm_gray_time: NULL context");
    return bracket_ms(c, c->gray.prof, c->gray.depth >= 0, "psm_gray_time", "the last psm_gray_compute was not timed (PSM_OPT_PROFILE), or there is none", ms);
}

}  // extern "C"
