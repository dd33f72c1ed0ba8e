// psm_api_filter.cpp - CostConst and CostFilter behind the C ABI: what stays virtual (lazy cost volumes, the filtered
// volume as packed per-pixel minima or low-resolution FGF models), which form of the fused kernel runs, and how a virtual
// volume becomes real when something other than the WTA reads it.  Replaces CVC_cl::buildCV (src/CVC_cl.cpp:95-210) and
// CVF_cl::preprocess / filterCV (src/CVF_cl.cpp) as called by DispEst::CostConst_GPU / CostFilter_GPU
// (src/DispEst.cpp:272-276,299-308); the FGF entry follows DispEst::CostFilter_FGF (src/DispEst.cpp:281-296).
#include "psm_ctx.h"

#include <cstring>
#include <utility>

using namespace psm;

namespace psm {

// The float volumes are allocated on first use: the default path (lazy costs + select-mode filter) never touches them.
int ensure_vol(psm_ctx *c, int side)
{
    if (c->vol[side]) return 0;
    const size_t V = (size_t)c->W * c->H * c->Dloc;
    PSM_HIP(c, hipMalloc(&c->vol[side], V * velem(c)));
    return 0;
}

// The 16 B/voxel (a0,a1,a2,b) scratch is only needed by psm_filter_stage_a, the direct variant and psm_box8_volume
int ensure_ab(psm_ctx *c)
{
    if (c->ab) return 0;
    const size_t V = (size_t)c->W * c->H * c->Dloc;
    PSM_HIP(c, hipMalloc((void **)&c->ab, V * sizeof(float4)));
    return 0;
}

// second float volume for the fused filter when it has to READ a materialised cost volume (out of place)
int ensure_spare(psm_ctx *c)
{
    if (c->spare) return 0;
    const size_t V = (size_t)c->W * c->H * c->Dloc;
    PSM_HIP(c, hipMalloc((void **)&c->spare, V * sizeof(float)));
    return 0;
}

unsigned long long *next_pc_stamp(psm_ctx *c)
{
    if (c->opt_profile != 2) return nullptr;
    if (!c->pc_ts) {
        if (hipMalloc((void **)&c->pc_ts, 3 * (size_t)PC_TS_SLOTS * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            c->pc_ts = nullptr;
            return nullptr;
        }
        (void)hipMemsetAsync(c->pc_ts, 0xff, PC_TS_SLOTS * sizeof(unsigned long long), c->stream);
        (void)hipMemsetAsync(c->pc_ts + PC_TS_SLOTS, 0, 2 * PC_TS_SLOTS * sizeof(unsigned long long), c->stream);
        c->pc_ts_n = 0;
    }
    if (c->pc_ts_n >= PC_TS_SLOTS) return nullptr;        // (read them with psm_filter_launch_times to start over)
    return c->pc_ts + c->pc_ts_n++;
}

// a virtual Fast-Guided-Filter result becomes a real volume
int fgf_flush(psm_ctx *c, int side)
{
    const int sub = pending_fgf(c->vside[side]);
    if (!sub) return 0;
    if (ensure_vol(c, side)) return 1;
    {
        Prof p(c, PSM_K_FGF);
        launch_fgf_apply(c->stream, (float *)c->vol[side], c->g[side].g1, c->W, c->H, c->Dloc, sub, c->fgf_mab[side]);
    }
    in_memory(c->vside[side]);
    return check_launch(c, "fgf (upsample)");
}

// chunk planes of the select-mode fused kernel
int ensure_gf_scratch(psm_ctx *c, size_t bytes)
{
    if (c->gf_scratch && c->gf_scratch_bytes >= bytes) return 0;
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->gf_scratch);
    c->gf_scratch = nullptr;
    c->gf_scratch_bytes = 0;
    PSM_HIP(c, hipMalloc(&c->gf_scratch, bytes));
    c->gf_scratch_bytes = bytes;
    return 0;
}

PcPair pc_pair(const psm_ctx *c)
{
    PcPair p;
    memset(&p, 0, sizeof p);             // (psm_compute_batch compares table entries bytewise)
    for (int k = 0; k < 2; ++k) { p.raw[k] = c->pair.raw[k]; p.g[k] = c->g[k]; p.p4[k] = c->p4[k]; }
    p.scratch = c->gf_scratch;
    p.keys = c->keys_cur;
    p.maps = c->maps;
    return p;
}

// Bring g1 (and the 8-bit planes) of the rows g1_need and the guidance g2..g4 of the rows guid_need up to date with the current
// pair - an empty need asks for nothing; guid_need lies inside g1_need.  The one place that compares need with record, picks
// the launches and updates the record: float contexts that miss both take ONE launch, k_guide_march forming the image planes
// itself from the staged images (planarise + scale + gray + x-gradient, then the guidance of the same rows - a stripe: 4 rows
// more either side than it needs); everything else takes k_prep (+ k_prep_u8) and / or the guidance kernel on the g1 planes.
// The kernels are row-independent, so a row stripe prepares its own rows only and every later need they do not cover
// prepares again.
int ensure_planes(psm_ctx *c, Rows g1_need, Rows guid_need)
{
    const bool need_g1 = !c->g1_rows.covers(g1_need), need_guid = !c->guid_rows.covers(guid_need);
    if (!need_g1 && !need_guid) return 0;
    const bool f32_img = c->pair.st.depth == PSM_IMG_F32;
    const size_t row = (size_t)c->W * 3 * (f32_img ? 4 : 1);
    const PcPair pair = pc_pair(c);
    const Recs<PcPair> q = {&pair, nullptr, 1};
    if (need_g1 && need_guid && c->dtype == PSM_F32) {
        {
            Prof p(c, PSM_K_GUIDE);
            launch_guidance(c->stream, q, c->W, c->H, g1_need.y0, g1_need.y1, fma_solve(c), f32_img ? 2 : 1, row);
        }
        if (check_launch(c, "prep + guidance") || images_read(c, c->stream)) return 1;
        guid_need = g1_need;
    } else {
        if (need_g1) {
            for (int u8 = 0; u8 < (c->dtype == PSM_U8 ? 2 : 1); ++u8) {   // both images per launch: g1, then the byte planes of an 8-bit context
                Prof p(c, PSM_K_PREP);
                launch_prep(c->stream, q, row, f32_img, c->W, g1_need.y0, g1_need.y1, u8 != 0);
            }
            if (check_launch(c, "prep") || images_read(c, c->stream)) return 1;
        }
        if (need_guid) {
            {
                Prof p(c, PSM_K_GUIDE);
                launch_guidance(c->stream, q, c->W, c->H, guid_need.y0, guid_need.y1, fma_solve(c));
            }
            if (check_launch(c, "guidance")) return 1;
        }
    }
    if (need_g1) c->g1_rows = g1_need;
    if (need_guid) c->guid_rows = guid_need;
    return 0;
}

// npairs / batch: see pc_plan_select.  The geometry, options and slices are the context's (a batch: those of its first context).
SelPlan select_plan(const psm_ctx *c, int npairs, bool batch)
{
    const March &m = c->march;
    SelPlan sp;
    // Two-phase selection (default from 112 local slices up - measured: -10 % at 1080p x 256, -13 % at 4K x 256, -4 % at
    // 720p x 128, worse at 64 slices and below; PSM_FLAG_TWO_PHASE_ON / _OFF force it for any Dloc >= 2 / disable it): every
    // S-th slice goes through the minima planes -> k_chunk_min -> keys; the other slices then run against that seeded key
    // plane (key form: one key load per voxel, an atomic only where a slice beats the current minimum - rare after the
    // seeding), so they write no planes and need no reduction.  S = pc_seed_stride: 8 since round 6 (5, and 4 from 4 Mpixel up,
    // while the key loads came from the memory side).
    sp.two_phase = !(m.flags & PSM_FLAG_TWO_PHASE_OFF) && c->Dloc >= 2 && (c->Dloc >= 112 || (m.flags & PSM_FLAG_TWO_PHASE_ON));
    sp.S = sp.two_phase ? pc_seed_stride(c->W, m.rows(c->H), c->dtype == PSM_U8) : 1;
    sp.n1 = (c->Dloc + sp.S - 1) / sp.S;
    sp.n2 = c->Dloc - sp.n1;
    // The reduction is the last thing that touches the keys: when the pair holds every slice and one phase runs, it writes the maps
    // (the low byte of each key) in the same pass.  After two phases a batch merges its maps itself (k_merge_batch), a single
    // context leaves them to psm_disp_select.
    sp.maps = c->Dloc == c->D && !sp.two_phase;
    sp.scratch_bytes = 2 * pc_plan_select(m, c->W, c->H, sp.n1, PC_PLANES, npairs, batch).scratch_bytes();
    return sp;
}

// Plane form (all slices, or every S-th) -> reduction -> key form (the others) for the pairs q on c's stream, with c's brackets
// and launch stamps.  Every pair's scratch holds sp.scratch_bytes.
int enqueue_select(psm_ctx *c, const Recs<PcPair> &q, const SelPlan &sp)
{
    const bool u8 = c->dtype == PSM_U8;
    {
        Prof p(c, PSM_K_CVF_F);
        launch_cvf_select2(c->stream, c->march, q, u8, c->W, c->H, sp.n1, c->d0, next_pc_stamp(c), sp.two_phase ? 1 : 0, sp.S);
    }
    // (a single context's maps may still be the source of the last frame's download; a batch waited for its contexts' before the table)
    if (sp.maps && !q.dev && maps_writable(c)) return 1;
    {
        Prof p(c, PSM_K_WTA);
        launch_chunk_min2sides(c->stream, c->march, q, c->W, c->H, sp.n1, sp.maps, c->d0, sp.two_phase ? 1 : 0, sp.S);
    }
    if (sp.n2 > 0) {
        Prof p(c, PSM_K_CVF_F);
        launch_cvf_select_keys2(c->stream, c->march, q, u8, c->W, c->H, sp.n2, c->d0, next_pc_stamp(c), 2, sp.S);
    }
    return 0;
}

}  // namespace psm

namespace {

// The context's pair as a one-volume launch of the fused filter and its reduction see it: `side` first - its guidance and byte
// planes in [0], the other image's in [1] -, its chunk planes at the start of the scratch, its own key plane.
PcPair pc_pair_side(const psm_ctx *c, int side)
{
    PcPair p = pc_pair(c);
    if (side) { std::swap(p.g[0], p.g[1]); std::swap(p.p4[0], p.p4[1]); }
    if (p.keys) p.keys += side * (size_t)c->W * c->H;
    return p;
}

// the recipe carried out: the unfiltered costs of `side` written to vol[side]
int build_costs(psm_ctx *c, int side)
{
    if (ensure_vol(c, side)) return 1;
    Prof p(c, PSM_K_CVC);
    // buildCV_right is called with the images swapped (src/DispEst.cpp:217,260)
    if (c->dtype == PSM_U8) launch_cvc_u8(c->stream, c->p4[side], c->p4[1 - side], (uint8_t *)c->vol[side], c->W, c->H, c->d0, c->Dloc, side);
    else launch_cvc(c->stream, c->g[side].g1, c->g[1 - side].g1, (float *)c->vol[side], c->W, c->H, c->d0, c->Dloc, side, 0, c->H);
    costs_built(c->vside[side]);
    return 0;
}

// 8-bit mode: the float copy of the 8-bit volume of `side` that the storing kernels work on (re-quantised afterwards)
int u8_to_fvol(psm_ctx *c, int side)
{
    const size_t V = (size_t)c->W * c->H * c->Dloc;
    if (!c->fvol) PSM_HIP(c, hipMalloc((void **)&c->fvol, V * sizeof(float)));
    launch_u8_to_f32(c->stream, (const uint8_t *)c->vol[side], c->fvol, V);
    return 0;
}

// The storing form of the fused filter: `side` filtered into a real volume, from whatever its costs currently are (what
// psm_download_volume etc. see; the default path never runs it).  Needs the planes of the whole image.
//   float, costs virtual:  built on the fly inside the kernel; nothing is read from vol[side], so the result goes straight into it
//   float, costs in vol[side]:  out of place into `spare`, which then becomes vol[side] (ping-pong)
//   8-bit:  costs built if they are virtual; float copy -> kernel (out of place) -> re-quantised into vol[side]
int filter_stored(psm_ctx *c, int side)
{
    const bool u8 = c->dtype == PSM_U8;
    if (ensure_vol(c, side)) return 1;
    if (u8 && costs_lazy(c->vside[side]) && build_costs(c, side)) return 1;
    const bool lazy = costs_lazy(c->vside[side]);
    if (u8 && u8_to_fvol(c, side)) return 1;
    if (!lazy && ensure_spare(c)) return 1;
    const float *in = lazy ? nullptr : u8 ? c->fvol : (const float *)c->vol[side];
    float *out = lazy ? (float *)c->vol[side] : c->spare;
    const PcPair one = pc_pair_side(c, side);
    {
        Prof p(c, PSM_K_CVF_F);
        launch_cvf_fused(c->stream, c->march, Recs<PcPair>{&one, nullptr, 1}, in, out, c->W, c->H, c->Dloc, 0, c->H, c->d0, lazy ? 1 + side : 0,
                         next_pc_stamp(c));
    }
    if (u8) launch_f32_to_u8(c->stream, out, (uint8_t *)c->vol[side], (size_t)c->W * c->H * c->Dloc);   // q8 = sat_u8(rintf(q * 255))
    else if (!lazy) std::swap(*(float **)&c->vol[side], c->spare);
    in_memory(c->vside[side]);                   // vol[side] now holds real (filtered) data
    return check_launch(c, "cvf (fused, storing form)");
}

}  // namespace

namespace psm {

// make sure the whole volume of `side` (unfiltered, or filtered by psm_cost_filter / psm_cost_filter_fgf) is in memory
int materialize(psm_ctx *c, int side)
{
    PSM_NOT_STRIDED(c, "materialising a cost volume");
    if (fgf_flush(c, side)) return 1;
    if (all_real(c->vside[side])) return 0;
    // (a row-stripe filter leaves only its own rows of the planes behind)
    if (ensure_planes(c, whole_image(c), whole_image(c))) return 1;
    // the guided-filter result exists only as WTA keys: run the same fused kernel again, this time storing q
    if (pending_keys(c->vside[side])) return filter_stored(c, side);
    // the costs exist only as a recipe: build them
    return build_costs(c, side) || check_launch(c, "cvc (materialize)");
}

}  // namespace psm

namespace {

// One volume, select form: the fused kernel in "select" mode - the WTA over the local slices runs inside the filter, the filtered
// volume stays virtual (8-bit mode: with costs built on the fly only)
int filter_side_select(psm_ctx *c, int side)
{
    const int W = c->W, H = c->H;
    const bool lazy = costs_lazy(c->vside[side]), sel8 = c->dtype == PSM_U8;
    const PcPlan pl = pc_plan(W, c->march.rows(H), c->Dloc, c->march.seg_rows, PC_PLANES);
    if (ensure_gf_scratch(c, pl.scratch_bytes())) return 1;
    const PcPair one = pc_pair_side(c, side);      // (after the scratch exists: the record carries it)
    const Recs<PcPair> q = {&one, nullptr, 1};
    {
        Prof p(c, PSM_K_CVF_F);
        launch_cvf_select(c->stream, c->march, q, lazy ? nullptr : (const float *)c->vol[side], sel8, W, H, c->Dloc, c->d0, lazy ? 1 + side : 0,
                          next_pc_stamp(c));
    }
    {
        Prof p(c, PSM_K_WTA);
        launch_chunk_min(c->stream, c->march, q, W, H, c->Dloc);
    }
    filtered_to_keys(c->vside[side]);
    return check_launch(c, "cvf (fused, select mode)");
}

// One volume, stage A alone (psm_filter_stage_a) or the direct variant: they read a real cost volume (8-bit mode: its float copy,
// re-quantised after stage B)
int filter_side_direct(psm_ctx *c, int side, bool stage_b)
{
    if (fma_solve(c))
        return fail(c, "PSM_FLAG_FMA_SOLVE: stage A alone (psm_filter_stage_a) and the direct kernel variant exist in the canonical arithmetic only");
    if (materialize(c, side) || ensure_ab(c)) return 1;
    const bool u8 = c->dtype == PSM_U8;
    if (u8 && u8_to_fvol(c, side)) return 1;
    float *fv = u8 ? c->fvol : (float *)c->vol[side];
    {
        Prof p(c, PSM_K_CVF_A);
        launch_cvf_a(c->stream, c->opt_variant, c->march, fv, c->ab, c->g[side], c->W, c->H, c->Dloc, 0, c->H);
    }
    if (stage_b) {          // (direct variant only: the marching stage B lives in the fused kernel)
        {
            Prof p(c, PSM_K_CVF_B);
            launch_cvf_b_direct(c->stream, c->ab, fv, c->g[side], c->W, c->H, c->Dloc);
        }
        if (u8) launch_f32_to_u8(c->stream, fv, (uint8_t *)c->vol[side], (size_t)c->W * c->H * c->Dloc);
    }
    return check_launch(c, "cvf");
}

// One volume: the path for cost volumes that exist in memory (psm_upload_volume, PSM_FLAG_MATERIALISE_COSTS), for the storing
// form (PSM_FLAG_STORE_FILTERED, or images / volumes outside the select forms' domain), the direct variant and for stage A alone.
int filter_side(psm_ctx *c, int side, bool stage_b)
{
    PSM_NOT_STRIDED(c, "filtering one side / a materialised volume / the storing form");
    forget_early(c->res);                // (the keys under an early map are about to change)
    // (the guidance of BOTH images the first time either side asks: the other side's call then finds it)
    if (ensure_planes(c, whole_image(c), whole_image(c))) return 1;
    if (fgf_flush(c, side)) return 1;
    if (pending_keys(c->vside[side]) && materialize(c, side)) return 1;   // filtering an already filtered (virtual) volume: make it real first
    if (!stage_b || c->opt_variant != 0) return filter_side_direct(c, side, stage_b);
    const bool select_form = (c->dtype == PSM_F32 || costs_lazy(c->vside[side])) && !(c->march.flags & PSM_FLAG_STORE_FILTERED) && scaled_forms_ok(c);
    return select_form ? filter_side_select(c, side) : filter_stored(c, side);
}

// Both volumes per launch: guidance of both images, select-mode fused filter of both volumes, chunk reduction of both - five
// launches per frame instead of twelve.  The default path (costs built on the fly, both sides fresh).
bool can_filter_both(const psm_ctx *c)
{
    return c->opt_variant == 0 && !(c->march.flags & PSM_FLAG_STORE_FILTERED) && scaled_forms_ok(c) && fresh_lazy(c->vside[0]) && fresh_lazy(c->vside[1]);
}

// The results are those of the stripe in force NOW, whatever psm_set_rows says later; sp.maps: psm_disp_select has no kernel left to launch.
int filter_both(psm_ctx *c)
{
    // (after a lazy psm_cost_construct in a float context: image planes AND guidance in one launch, straight from the staged images)
    const PlaneRows need = stripe_planes(c);
    if (ensure_planes(c, need.g1, need.guid)) return 1;
    const SelPlan sp = select_plan(c, 1, false);
    if (ensure_gf_scratch(c, sp.scratch_bytes)) return 1;
    const PcPair pair = pc_pair(c);
    if (enqueue_select(c, Recs<PcPair>{&pair, nullptr, 1}, sp)) return 1;
    for (VolSide &v : c->vside) filtered_to_keys(v);
    filtered(c->res, stripe_rows(c), sp.maps ? c->maps : nullptr);
    return check_launch(c, sp.two_phase ? "cvf (fused, select mode, two phases, both volumes)" : "cvf (fused, select mode, both volumes)");
}

}  // namespace

extern "C" {

int psm_cost_construct(psm_ctx *c)
{
    if (!c) return 1;
    if (bind(c)) return 1;
    if (adopt_staged_pair(c)) return 1;
    if (!c->have_images) return fail(c, "psm_cost_construct: no image pair uploaded");
    const double t0 = now_us();
    // Lazy cost volume: when the fused filter will consume the costs (marching kernels, PSM_FLAG_MATERIALISE_COSTS not set)
    // they are built inside that kernel and never written to HBM.
    // (8-bit mode: lazy only when the select-mode kernel will consume the costs - its storing form reads a float copy)
    const bool lazy = c->opt_variant == 0 && !(c->march.flags & PSM_FLAG_MATERIALISE_COSTS) &&
                      (c->dtype == PSM_F32 || !(c->march.flags & PSM_FLAG_STORE_FILTERED));
    if (!lazy) PSM_NOT_STRIDED(c, "psm_cost_construct with materialised costs");
    // Every call starts the planes afresh, also when the pair has not changed: a frame does all of its work.
    c->g1_rows = c->guid_rows = Rows{};
    // CVC::preprocess belongs to this stage (src/DispEst.cpp:232-233): the rows a stripe with lazy costs reads, else the whole image.
    // In a float context it is lazy too (round 6): with the cost volume virtual, the first thing that needs the image planes is the
    // guidance precompute of psm_cost_filter - and k_guide_march forms them itself from the staged images (one launch instead of
    // k_prep + k_guide_march: ensure_planes).  (Not with frames in flight on other streams - PSM_OPT_FRAMES_IN_FLIGHT: the merged
    // launch carries the conversions in all three waves of its workgroups and stretches beside another frame's VALU-bound fused
    // kernel - 450 x 375 x 64, two frames in flight: 0.226 ms against 0.211 with k_prep + k_guide_march; alone it is 0.270 vs 0.279.)
    const bool lazy_prep = lazy && c->dtype == PSM_F32 && c->march.inflight <= 1;
    if (!lazy_prep && ensure_planes(c, lazy ? stripe_planes(c).g1 : whole_image(c), Rows{})) return 1;
    c->vol_domain_ok[0] = c->vol_domain_ok[1] = true;   // (uploaded volumes are gone; the costs now follow from the images)
    for (int s = 0; s < 2; ++s) {
        if (!lazy && build_costs(c, s)) return 1;
        new_costs(c->vside[s], lazy);                   // a new cost volume replaces whatever was pending
    }
    if (check_launch(c, "cvc")) return 1;
    c->have_cost = true;
    stale(c->res);
    keys_gone(c->res);
    return end_stage(c, PSM_STAGE_CVC, t0);
}

int psm_cost_filter(psm_ctx *c)
{
    if (!c) return 1;
    if (!c->have_cost) return fail(c, "psm_cost_filter: no cost volume (call psm_cost_construct or psm_upload_volume)");
    if (!c->have_images) return fail(c, "psm_cost_filter: no image pair uploaded (guidance)");
    if (bind(c)) return 1;
    const double t0 = now_us();
    // preprocess L, filter L, preprocess R, filter R (src/DispEst.cpp:302-305)
    const bool striped = c->march.yend > c->march.ybeg;
    if (can_filter_both(c)) {
        if (filter_both(c)) return 1;
    } else {
        if (striped) return fail(c, "psm_cost_filter: a row stripe (psm_set_rows) needs the default select form of the filter "
                                    "(no variant / storing flag, cost volumes not materialised, images / volumes inside the select forms' domain)");
        for (int s = 0; s < 2; ++s)
            if (filter_side(c, s, true)) return 1;
        filtered(c->res, whole_image(c), nullptr);
    }
    return end_stage(c, PSM_STAGE_CVF, t0);
}

int psm_cost_filter_side(psm_ctx *c, int side)
{
    if (!c) return 1;
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "psm_cost_filter_side: bad side %d", side);
    if (!c->have_cost) return fail(c, "psm_cost_filter_side: no cost volume");
    if (!c->have_images) return fail(c, "psm_cost_filter_side: no image pair uploaded (guidance)");
    if (c->march.yend > c->march.ybeg) return fail(c, "psm_cost_filter_side: row stripes (psm_set_rows) go through psm_cost_filter");
    if (bind(c)) return 1;
    const double t0 = now_us();
    if (filter_side(c, side, true)) return 1;
    filtered(c->res, whole_image(c), nullptr);
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    c->stage_us[PSM_STAGE_CVF] = (side == PSM_LEFT ? 0.0 : c->stage_us[PSM_STAGE_CVF]) + (now_us() - t0);
    return 0;
}

int psm_cost_filter_fgf(psm_ctx *c, int sub)
{
    if (!c) return 1;
    if (c->dtype != PSM_F32) return fail(c, "psm_cost_filter_fgf: float contexts only");
    if (sub != 2 && sub != 4 && sub != 8) return fail(c, "psm_cost_filter_fgf: subsample_rate %d not in {2,4,8}", sub);
    if (!c->have_cost) return fail(c, "psm_cost_filter_fgf: no cost volume (call psm_cost_construct or psm_upload_volume)");
    if (!c->have_images) return fail(c, "psm_cost_filter_fgf: no image pair uploaded (guidance)");
    // (the low-resolution models of a stripe would need their own halo arithmetic; a striped host filters whole images here)
    if (c->march.yend > c->march.ybeg) return fail(c, "psm_cost_filter_fgf: row stripes (psm_set_rows) are not supported by the Fast Guided Filter path");
    PSM_NOT_STRIDED(c, "psm_cost_filter_fgf");
    const int ws = c->W / sub, hs = c->H / sub, rad = 8 / sub;
    if (ws <= rad || hs <= rad) return fail(c, "psm_cost_filter_fgf: %dx%d too small for subsample_rate %d", c->W, c->H, sub);
    if (bind(c)) return 1;
    const double t0 = now_us();
    if (ensure_planes(c, whole_image(c), Rows{})) return 1;
    // small planes: ism, msm, v1 (float4), v2 (float2) per pixel; ab (scratch) and one mab per side (float4) per small voxel
    const size_t n = (size_t)ws * hs, need = n * (3 * sizeof(float4) + sizeof(float2)) + 3 * n * c->Dloc * sizeof(float4);
    if (fgf_flush(c, 0) || fgf_flush(c, 1)) return 1;   // filtering an already FGF-filtered volume: make it real first
    for (int side = 0; side < 2; ++side)
        if (pending_keys(c->vside[side]) && materialize(c, side)) return 1;
    if (c->fgf_bytes < need) {
        PSM_HIP(c, hipStreamSynchronize(c->stream));
        (void)hipFree(c->fgf);
        c->fgf = nullptr;
        c->fgf_bytes = 0;
        PSM_HIP(c, hipMalloc(&c->fgf, need));
        c->fgf_bytes = need;
    }
    float4 *ism = (float4 *)c->fgf, *msm = ism + n, *v1 = msm + n, *ab = v1 + n;
    c->fgf_mab[0] = ab + n * c->Dloc;
    c->fgf_mab[1] = c->fgf_mab[0] + n * c->Dloc;
    float2 *v2 = (float2 *)(c->fgf_mab[1] + n * c->Dloc);
    // PSM_FLAG_FGF_STORE: always write the filtered volume (default: it stays virtual until something other than the WTA reads it)
    const bool keep_virtual = fgf_can_fuse_wta(c->W) && !(c->march.flags & PSM_FLAG_FGF_STORE);
    // left volume with the left image as guidance, then the right one (src/DispEst.cpp:283-295)
    for (int side = 0; side < 2; ++side) {
        // a virtual (lazy) cost volume stays virtual: the filter samples 1/sub^2 of it straight from the g1 planes
        const int mode = costs_lazy(c->vside[side]) ? 1 + side : 0;
        Prof p(c, PSM_K_FGF);
        launch_fgf_setup(c->stream, c->g[side].g1, c->W, c->H, sub, ism, msm, v1, v2);
        launch_fgf_model(c->stream, (const float *)c->vol[side], c->g[side].g1, c->g[1 - side].g1, c->W, c->H, c->Dloc, c->d0, sub, mode,
                         msm, v1, v2, ab, c->fgf_mab[side]);
        if (keep_virtual) { filtered_to_fgf(c->vside[side], sub); continue; }   // (vol[side] stands for it, allocated or not: VolSide)
        if (ensure_vol(c, side)) return 1;
        launch_fgf_apply(c->stream, (float *)c->vol[side], c->g[side].g1, c->W, c->H, c->Dloc, sub, c->fgf_mab[side]);
        in_memory(c->vside[side]);
    }
    if (check_launch(c, "cvf (fast guided filter)")) return 1;
    filtered(c->res, whole_image(c), nullptr);
    return end_stage(c, PSM_STAGE_CVF, t0);
}

int psm_filter_stage_a(psm_ctx *c, int side)
{
    if (!c) return 1;
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "psm_filter_stage_a: bad side %d", side);
    if (!c->have_cost || !c->have_images) return fail(c, "psm_filter_stage_a: needs images and a cost volume");
    if (bind(c)) return 1;
    if (filter_side(c, side, false)) return 1;
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
