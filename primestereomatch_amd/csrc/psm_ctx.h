// psm_ctx.h - the context behind the C ABI of libprimesm_hip.so (include/primesm_hip.h) and the helpers its
// translation units share.  Internal to the library:
//   psm_api_core.cpp    context life cycle, options, uploads / downloads, timers; the image pair slots (psm::PairSlots): the
//                       staging steps of the asynchronous uploads, adoption of the staged pair, the mark that the images were read
//   psm_api_filter.cpp  CostConst / CostFilter: which plane rows are current (ensure_planes), what is built lazily, which form
//                       of the fused kernel runs, materialisation
//   psm_api_select.cpp  DispSelect: maps, packed minima, row stripes and disparity shards
//   psm_api_pp.cpp      post-processing: L-R check, invalid fill, weighted median of one context or of several in shared
//                       launches (psm_post_process_batch) - one launch sequence, pp_enqueue (psm::WmState, psm::WmBatch; the sweep
//                       schedule, block layout and cache decision are the host-only psm_wm_sched.h)
//   psm_api_batch.cpp   several Middlebury-size pairs per launch (psm_compute_batch); what every batch entry point shares: the
//                       device table of the members' records (psm::DevTable), the join and fork of the members' streams, the
//                       member checks
//   psm_api_jwmf.cpp    JointWMF: the joint weighted median of the reference's live post-filter (psm_joint_wmf), and of the
//                       maps of several contexts in shared launches (psm_joint_wmf_batch)
//   psm_api_rectify.cpp video mode: remap + crop of the camera frame into the staged image slot (psm_upload_pair_rectified)
//   psm_api_sgm.cpp     semi-global matching over the staged pair, the reference's STEREO_SGBM branch (psm_sgm_compute), and
//                       over the pairs of several contexts in shared launches (psm_sgm_compute_batch) - one launch sequence,
//                       enqueue; the 8-bit maps of both views from its S (psm_sgm_select_maps, _batch) - one sequence, maps_run
//   psm_api_score.cpp   display maps and the error metric against ground truth of the current result (psm_score), and of the
//                       results of several contexts in shared launches (psm_score_batch) - one sequence, score_run
//   psm_api_depth.cpp   from disparity to depth: cv::reprojectImageTo3D of the current result and the compacted point cloud
//                       (psm_reproject), and of the results of several contexts in shared launches (psm_reproject_batch) - one
//                       sequence, reproject_run
//   psm_api_gray.cpp    the guided-filter path over a one-channel pair: one-channel fused filter and selection of host planes
//                       (psm_gray_compute), of the pairs of several contexts in shared launches (psm_gray_compute_batch) - one
//                       sequence, gray_run -, its test hooks and timer (psm::GrayState)
//   psm_api_wls.cpp     edge-aware WLS smoothing of the sub-pixel int16 map (psm_wls_filter), of the maps of several contexts in
//                       shared launches (psm_wls_filter_batch) - one sequence, wls_run - and the switch that lets the SGM sources
//                       of psm_score / psm_reproject read its result (psm_wls_publish)
// The last four bracket their launches for PSM_OPT_PROFILE with one psm::Bracket each (bracket_* below).
// Takes the place of the reference's oclUtil + CVC_cl / CVF_cl / DispSel_cl host wrappers
// (src/oclUtil.cpp, src/CVC_cl.cpp, src/CVF_cl.cpp, src/DispSel_cl.cpp).
// What a context knows about its volumes, results and image pairs between calls - psm::VolSide per side, psm::Results,
// psm::PairState - lives in psm_state.h with the only functions that change it.
#pragma once
#include "../../include/primesm_hip.h"
#include "psm_kernels.h"
#include "psm_state.h"

#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace psm {

struct KernelTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0.0;
    int launches = 0;
};

// psm_share_streams: the contexts of a batch run on ONE main stream and ONE copy stream each way instead of three streams per
// context (the runtime multiplexes streams onto a few hardware queues; with 8 contexts' 24 streams every asynchronous copy cost
// 0.2 ms of host time).  Owned jointly: the last context to go destroys the streams.
struct StreamSet {
    hipStream_t main = nullptr, up = nullptr, down = nullptr;
    int refs = 0;
};

// The device table of the members' records of a batch entry point, owned by the batch's first context and written
// by table_reserve / table_upload / table_free (psm_api_batch.cpp) alone.  Bytes: the records' type is the launch site's cast.
struct DevTable {
    uint8_t *dev = nullptr;
    uint8_t *pin = nullptr;                        // page-locked staging: two slots of `cap` bytes, used alternately
    std::vector<uint8_t> host;                     // the records the device copy holds (empty: none)
    size_t cap = 0;                                // bytes
    int slot = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};         // the copy out of a slot has executed (the host may refill it)
};

// PSM_OPT_PROFILE around one launch sequence - score_run, reproject_run, maps_run, wls_run: two events on its stream, and whether
// the last sequence recorded them (a batch records its first context's alone: only that context counts as timed).  Written by the
// bracket_* functions below alone, but for the `timed = false` of a sequence's forget step.
struct Bracket {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;
};

// psm_sgm_compute (psm_api_sgm.cpp): parameters, the stage's own device buffers (allocated on first use, reused from frame to
// frame) and the events of psm_sgm_times.  Nothing else in the context reads or writes any of it.
struct SgmState {
    int bs = 5, p1 = 0, p2 = 0, u = 10, m = 1;     // p1 / p2 0: the default for the pair's channel count
    int mode = 1;                                  // psm_sgm_set_mode: the row of SGM_MODE_DIRS; 1: MODE_HH, all eight directions
    int dmin = 0, nd = 0;                          // psm_sgm_set_range: minDisparity, numDisparities; nd 0: the context's max_disp
    int vol_dp = 0;                                // the Dp C and S are allocated for (another range's: freed and allocated again)
    int res_d = 0;                                 // the D of the result in them (psm_sgm_download_costs)
    int res_dmin = 0;                              // ... and its minDisparity (psm_sgm_select_maps: psm_sgm_set_range may have been called since)
    int res_ch = 0;                                // ... and the channels of the pair it ran on (1: psm_sgm_compute_gray's planes `gray`)
    uint16_t *C = nullptr;
    uint32_t *S = nullptr;
    uint32_t *disp2 = nullptr;
    int16_t *pre = nullptr, *out = nullptr;
    uint8_t *gray[2] = {nullptr, nullptr};         // psm_sgm_compute_gray: its 1-channel pair
    bool have = false;                             // a map and volumes of a compute exist
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [0..3]: psm_sgm_times; [4]: behind the speckle filter; [5]: ahead of a psm_sgm_filter_speckles
    bool timed = false;                            // ... and its launches were bracketed (PSM_OPT_PROFILE)
    // the speckle filter (psm_sgm_set_speckle, psm_sgm_filter_speckles; psm_speckle.hip): 8 W H bytes, allocated when first used
    int spk_window = 0, spk_range = 0;             // window 0: off
    unsigned *spk_label = nullptr, *spk_size = nullptr;
    bool spk_have = false;                         // spk_size holds the component sizes of a filter run
    int spk_t0 = -1;                               // the event ahead of the last filter run's launches (3 or 5); -1: it was not timed
    // the prefiltered Birchfield-Tomasi cost (psm_sgm_set_prefilter): 12 W H bytes, allocated when first used
    int cap = 0;                                   // pre_filter_cap; 0: the SAD cost
    uint8_t *pf[2] = {nullptr, nullptr};           // the planes of both images, [H][W][2 ch] bytes (room for ch 3)
    int pf_ch = 0;                                 // the channels of the planes the last compute wrote; 0: it wrote none
    // the census cost (psm_sgm_set_census): 16 W H bytes, allocated when first used
    int cen_w = 0, cen_h = 0;                      // the window; (0, 0): off
    uint64_t *cen[2] = {nullptr, nullptr};         // the code planes of both images, [H][W]
    bool cen_have = false;                         // the last compute wrote them
    DevTable tab;                                  // psm_sgm_compute_batch, psm_sgm_select_maps_batch (this context as the first): SgmPair records
    Bracket maps;                                  // psm_sgm_select_maps: around its launch (psm_sgm_maps_time)
};

// JointWMF (psm_api_jwmf.cpp): what a side's clustering of the current pair is.  Written by its three transitions alone; each makes
// the whole record anew, so none can leave the device weight table of an earlier clustering standing as current.
struct JwClust {
    bool have = false, user = false;               // a clustering exists (run or set) / ... and the host set it (psm_joint_wmf_set_clusters)
    int nf = 0, iters = 0;
    int n_clusters = 0, max_iter = 0;              // the parameters of the device k-means that made it
    std::vector<float> centres;
    bool tab_ok = false;                           // the device weight table is that of this clustering with sigma tab_sigma
    float tab_sigma = 0.f;
    // clustering adopted from the device k-means / clustering set by host / clustering gone: with the image pair, or because the
    // side's lok, labels or centres buffers are about to be rewritten
    void adopted(int nf_, int it, int nc, int mi, const float *cen) { *this = JwClust{true, false, nf_, it, nc, mi, {cen, cen + 3 * (size_t)nf_}}; }
    void set_by_host(int nf_, const float *cen) { *this = JwClust{true, true, nf_, 0, 0, 0, {cen, cen + 3 * (size_t)nf_}}; }
    void gone() { *this = JwClust{}; }
};

// psm_joint_wmf, psm_joint_wmf_batch (psm_api_jwmf.cpp; this context as the first of the call): `block`: the Lloyd states and centres
// of the images to cluster side by side, `pin` the page-locked memory the host reads them in.  A call of several contexts also has
// the device table: room for 2 n JwImg records (the images to cluster), behind them the 2 n JwSide records of the map sides.
struct JwBatch {
    DevTable tab;
    uint8_t *block = nullptr, *pin = nullptr;      // [cap] x {int state[4]}, then [cap] x {float centres[JW_NF_MAX][3]}
    size_t cap = 0;                                // images
};

// The plain weighted median (pp_enqueue, psm_api_pp.cpp): a context's own scratch of the two forms, allocated on first use, and what
// the last call reports.  Freed by wm_free alone.
struct WmState {
    int *flow = nullptr;                           // the dataflow form: nxt[H][W+1], prog[H], err[1]
    uint8_t *block = nullptr;                      // the sweep form: both sides' state (wm_layout, psm_wm_sched.h)
    float *wts = nullptr;                          // ... the 19 x 19 window weights of every invalid pixel (formed once per call, read by every evaluation)
    size_t wts_n = 0;                              // floats
    int sweeps[2] = {0, 0};                        // last call: sweeps until the fixed point (-1: dataflow form), evaluations
    long long evals[2] = {0, 0};
};

// The post-processing tail with this context as the first of the call (pp_enqueue; a single call's only one): the per-sweep counters
// of all 2 n maps in one block, so that one fill clears and one copy kernel snapshots them all into `pin` (two slots: a group's
// counters are read while the next group runs), and - n > 1 - the device table of the members' PpPair records.  Every other buffer
// of the median stays the member's own (WmState).  Freed by wm_free alone.
struct WmBatch {
    DevTable tab;
    int *cnt = nullptr;                            // [cap] x WM_NCNT counters, map 2 i + s: side s of member i
    int *pin = nullptr;                            // page-locked snapshots of them: two slots of cap x WM_NCNT ints
    size_t cap = 0;                                // maps
    hipEvent_t ev[2] = {nullptr, nullptr};         // the snapshot into a slot has executed
};

// psm_score (psm_api_score.cpp): parameters, the dataset's truth (kept until replaced or cleared), and the stage's scratch -
// display and error planes, counters, their page-locked slot - allocated on first use and given back by psm_release_scratch.
struct ScoreState {
    int scale = 4, thr = 4, mask_mode = PSM_MASK_NONOCC;
    uint8_t *gt = nullptr, *mask = nullptr;        // [H][W] each; have_mask: the last psm_score_set_truth brought one
    bool have_truth = false, have_mask = false;
    int16_t *hook = nullptr;                       // psm_score_upload_sgm_map: the plane; hook_on: the SGM sources read it
    bool hook_on = false;
    uint8_t *planes = nullptr;                     // [3][H][W]: left display, right display, error plane
    ScCnt *cnt = nullptr, *pin = nullptr;          // the counters and the page-locked slot their copy lands in
    hipEvent_t ev_done = nullptr;                  // ... that copy has executed
    Bracket prof;                                  // PSM_OPT_PROFILE: around the launches
    int source = -1;                               // of the last psm_score (-1: none: the planes hold nothing)
    int unit = 0;                                  // ... and its 127 / max_disp
    bool pending = false;                          // a record is on its way to `pin` (psm_score_wait)
    DevTable tab;                                  // psm_score_batch (this context as the first of a batch): ScPair records
};

// psm_reproject (psm_api_depth.cpp): parameters (they survive psm_release_scratch) and the stage's scratch - the dense planes and
// the cloud (each allocated when first asked for), the tiles' counts and offsets, the count and its page-locked slot.
struct DepthState {
    double Q[16] = {};
    bool have_q = false;
    int crop_x = 0, crop_y = 0;
    float z_min = 0.0f, z_max = 3.402823466e+38f;  // FLT_MAX
    unsigned *xyz = nullptr, *z = nullptr;         // [H][W][3], [H][W] float bit patterns
    uint4 *cloud = nullptr;                        // [H W] records
    unsigned *tiles = nullptr;                     // [2][dp_tiles]: counts, offsets
    unsigned *cnt = nullptr, *pin = nullptr;       // the count and the page-locked slot its copy lands in
    hipEvent_t ev_done = nullptr;                  // ... that copy has executed
    Bracket prof;                                  // PSM_OPT_PROFILE: around the launches
    int outputs = 0;                               // of the last psm_reproject (0: none: the planes hold nothing)
    bool pending = false;                          // a count is on its way to `pin` (psm_reproject_wait)
    DevTable tab;                                  // psm_reproject_batch (this context as the first of a batch): DpArgs records
};

// psm_wls_filter (psm_api_wls.cpp): parameters (they survive psm_release_scratch) and the stage's planes, allocated on first use
// and given back by psm_release_scratch - 35 bytes per pixel: the working planes, the 12 bytes of the forward sweeps, the link
// indices, the result - and 3 more under PSM_WLS_CONFIDENCE.
struct WlsState {
    float lambda = 8000.0f, sigma = 1.5f;
    int iters = 3;
    float *work = nullptr;                         // [5][H][W]: num, den; cp, np, dp of a pass's forward sweep
    uint8_t *links = nullptr;                      // [2][H][W]: kh, kv
    int16_t *out = nullptr;                        // [H][W]: the filtered map
    unsigned *q = nullptr;                         // [H][W]: the quotient's bit patterns
    float *tab = nullptr;                          // [256] on the device; tab_sigma: the sigma it was formed with (0: none yet)
    float tab_host[256] = {};                      // ... and the host's copy the upload reads
    float tab_sigma = 0.0f;
    hipEvent_t ev_done = nullptr;                  // behind the last launch (psm_wls_wait)
    Bracket prof;                                  // PSM_OPT_PROFILE: around the launches
    bool have = false;                             // the planes hold the result of a filter run
    int invalid = 0;                               // ... and its invalid value
    bool pending = false;                          // an asynchronous run has not been waited for (psm_wls_wait)
    bool publish = false;                          // psm_wls_publish: the SGM sources of psm_score / psm_reproject read `out`
    DevTable pairs;                                // psm_wls_filter_batch (this context as the first of a batch): WlsPair records
    // PSM_WLS_CONFIDENCE (psm_wls_set_confidence: the parameters survive psm_release_scratch too): 3 more bytes per pixel,
    // allocated when first used
    int conf_terms = PSM_WLS_CONF_LR | PSM_WLS_CONF_VAR, conf_thresh = 24, conf_radius = 2, conf_shift = 8;
    uint8_t *conf = nullptr;                       // [H][W]: the confidence bytes
    int16_t *r16 = nullptr;                        // [H][W]: the right view's map in 16ths
    int have_conf = 0;                             // the terms the last run's planes were made with (0: it had no flag)
    Bracket conf_prof;                             // PSM_OPT_PROFILE: around the two launches ahead of k_wls_init (psm_wls_conf_time)
};

// psm_gray_compute (psm_api_gray.cpp): the stage's own device buffers - the pair's planes, 16 bytes of guidance per pixel and side,
// the chunk scratch, the key plane - allocated on first use and given back by gray_free alone.  Nothing else in the context reads
// or writes any of it; the stage meets the rest in the map buffer and psm::Results only.
struct GrayState {
    void *raw[2] = {nullptr, nullptr};             // the pair's planes [H][W], room for floats
    float2 *ig[2] = {nullptr, nullptr};            // {I, G}
    float2 *mv[2] = {nullptr, nullptr};            // {mI, 1 / (var + eps)}
    float2 *ab = nullptr;                          // [2][gray_plan().dc][H][W] {a, b} of one chunk of slices
    long long *keys = nullptr;                     // [2][H][W]: this stage's packed minima (ctx->keys belongs to the colour path)
    int depth = -1;                                // PSM_IMG_* of the last call's pair, which the planes hold; -1: none
    // psm_gray_compute_fgf: the subsampled planes, allocated on its first use and grown when a call needs more (a lower rate)
    float4 *fsm[2] = {nullptr, nullptr};           // [hs][ws] {Is, mI, den, 0}
    float2 *fab = nullptr, *fmab = nullptr;        // [2][gray_fgf_plan().dc][hs][ws] {a, b} and {blur(a), blur(b)} of one chunk of slices
    size_t fsm_cap = 0, fab_cap = 0;               // elements of each fsm plane; of fab and of fmab
    int rate = 0;                                  // the call the planes belong to: 0 psm_gray_compute, else the rate of psm_gray_compute_fgf
    Bracket prof;                                  // PSM_OPT_PROFILE: around the launches (psm_gray_time)
    DevTable pairs;                                // psm_gray_compute_batch (this context as the first of a batch): GrayPair records
};

// The image pair every frame starts with, and the second slot the next frame travels into (psm_upload_pair_async,
// psm_upload_pair_rectified_async).  `st` is changed by its transitions (psm_state.h) alone, the rest by the functions declared
// under "the image pair slots" below.
struct PairSlots {
    PairState st;
    void *raw[2] = {nullptr, nullptr};             // the current pair: the interleaved host images, raw_bytes each
    void *raw_next[2] = {nullptr, nullptr};        // the slot a staged pair travels into (swapped with raw when adopted), on first use
    size_t raw_bytes = 0;
    uint8_t *pin_up = nullptr;                     // page-locked staging of the plain asynchronous form (2 slots x 2 images, used alternately), on first use
    hipEvent_t ev_stage[2] = {nullptr, nullptr};   // the copy out of staging slot st.slot (pin_up's or rect_pin's) has executed: the host may refill it
    // ev_up: the staged pair is complete in raw_next; ev_free: recorded behind every launch sequence that reads raw (images_read) -
    // what the copy stream waits for before it overwrites raw_next, the current pair of two frames ago
    hipEvent_t ev_up = nullptr, ev_free = nullptr;
};
}  // namespace psm

struct psm_ctx {
    psm_ctx() { for (signed char &p : peer_ok) p = -1; }
    int W = 0, H = 0, D = 0, d0 = 0, d1 = 0, Dloc = 0, dtype = PSM_F32, device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t copy_stream = nullptr;  // psm_upload_pair_async / psm_download_maps_async: PCIe legs next to the kernels
    hipStream_t down_stream = nullptr;  // ... the D2H leg's stream: copy_stream unless the context shares a StreamSet
    psm::StreamSet *shared = nullptr;   // psm_share_streams
    hipEvent_t ev_maps = nullptr, ev_down = nullptr;

    // device memory (DESIGN.md "HBM layout")
    psm::PairSlots pair;                // the staged image pair, the slot of the next one and their events
    psm::Guidance g[2] = {};
    void *vol[2] = {nullptr, nullptr};  // [Dloc][H][W] float (PSM_F32) or uint8 (PSM_U8)
    float *fvol = nullptr;              // PSM_U8 only: float work volume of one side
    float *spare = nullptr;             // PSM_F32: output volume of the fused filter (ping-pong with vol[side])
    float4 *ab = nullptr;               // [Dloc][H][W] {a0,a1,a2,b}; also box8 output
    long long *keys = nullptr;          // [2][H][W]
    long long *keys_cur = nullptr;      // where the packed minima go: `keys`, or the caller's buffer (psm_set_key_buffer)
    long long *gather = nullptr;        // [gather_ranks][2][H][W], psm_disp_merge_ctx
    int gather_ranks = 0;
    // page-locked bounce buffers of the single-process exchange when two devices cannot reach each other (gather_leg): two slots
    // used alternately - the device -> host copy of leg i + 1 runs while the host -> device copy of leg i is still in flight; a
    // slot is refilled only after the copy out of it has executed (ev_xfer)
    uint8_t *xfer_pin[2] = {nullptr, nullptr};
    size_t xfer_pin_bytes[2] = {0, 0};
    hipEvent_t ev_xfer[2] = {nullptr, nullptr};
    int xfer_slot = 0;
    signed char peer_ok[64];            // hipDeviceCanAccessPeer(this device, d), asked once per device (-1: not asked yet)
    int gather_staged_legs = 0;         // legs that went through the bounce buffers since the context was created (psm_gather_staged_legs: tests)
    uint8_t *maps = nullptr;            // [2][H][W]: maps_own, or the caller's buffer (psm_set_map_buffer)
    uint8_t *maps_own = nullptr;
    psm::Results res;                   // which of maps / valid / keys_cur are the current frame's, and for which rows (psm_state.h)
    uint8_t *valid = nullptr;           // [2][H][W]
    uint8_t *pinned = nullptr;          // [2][H][W] page-locked bounce buffer for map / mask downloads (on first use)
    uint8_t *pinned2 = nullptr;         // second bounce buffer: psm_download_maps_async of frame i while frame i-1 is being read
    psm::WmState wm;
    psm::WmBatch wmb;
    // psm_joint_wmf (psm_api_jwmf.cpp): one device block for both sides (psm::JwScratch), allocated on first use
    uint8_t *jw = nullptr;
    psm::JwClust jw_cl[2];
    unsigned long long *jw_pin = nullptr;  // page-locked staging of the two integer tables (on first use)
    hipEvent_t ev_jw[2] = {nullptr, nullptr};   // ... the copy out of a side's staging has executed
    psm::JwBatch jwb;
    // psm_upload_pair_rectified (psm_api_rectify.cpp): the W x H crop window of a side's CV_16SC2 maps, uploaded once by
    // psm_rectify_set_maps; the unrectified source frames (both eyes, packed rows) per staging slot and their page-locked staging,
    // allocated on first use
    uint32_t *rect_xy[2] = {nullptr, nullptr};   // [H][W] {int16 x, int16 y}
    uint16_t *rect_fr[2] = {nullptr, nullptr};   // [H][W] fy * 32 + fx
    int rect_src_w[2] = {0, 0}, rect_src_h[2] = {0, 0};
    uint8_t *rect_src[2] = {nullptr, nullptr};
    uint8_t *rect_pin = nullptr;
    size_t rect_src_bytes = 0;                   // bytes of one eye in a slot (16-byte multiple) the buffers were allocated for
    psm::SgmState sgm;
    psm::ScoreState score;
    psm::DepthState depth;
    psm::WlsState wls;
    psm::GrayState gray;
    uint8_t *p4[2] = {nullptr, nullptr};  // PSM_U8 only: {c0,c1,c2,grad} words
    // What stands for vol[side] (psm_state.h): costs that are a recipe, a filtered volume pending as packed minima or as FGF models.
    // The WTA consumes either form directly; any other reader makes the volume real first (materialize()).
    psm::VolSide vside[2];
    // The rows of the planes that are those of the current image pair (empty: none; [0, H): the whole image; a row stripe
    // leaves its own rows behind).  Brought up to date by ensure_planes alone.
    psm::Rows g1_rows;                    // g1 (and the 8-bit planes p4) of both images
    psm::Rows guid_rows;                  // g2..g4 of both images
    void *gf_scratch = nullptr;         // chunk planes of the select-mode kernel (PcPlan::scratch_bytes)
    size_t gf_scratch_bytes = 0;
    unsigned long long *pc_ts = nullptr;  // PSM_OPT_PROFILE 2: {first start, last end} device time stamps per k_cvf_pc launch
    int pc_ts_n = 0;                      // launches stamped since the last reset (slots: PC_TS_SLOTS)
    psm::DevTable batch_tab;            // psm_compute_batch (this context as the first of a batch): PcPair records
    hipEvent_t ev_batch = nullptr;      // a batch entry point's join and fork (batch_join, batch_fork)
    // PSM_OPT_GRAPH: the launches of a batch captured once as a hipGraph and replayed while nothing they depend on changes
    hipGraphExec_t batch_graph = nullptr;
    long long graph_sig[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float4 *fgf_mab[2] = {nullptr, nullptr};
    void *fgf = nullptr;                // psm_cost_filter_fgf scratch (small planes), fgf_bytes long
    size_t fgf_bytes = 0;

    bool have_images = false, have_cost = false;

    // Domain of the scaled window sums (select forms of the fused kernel carry the 1/64 of both box filters as one 2^-12 at the
    // end: bit-identical to the per-sum scaling only while no intermediate under- or overflows).  8-bit images are always
    // inside; float images (non-zero |I| within 2^-10 .. 2^10) and uploaded cost volumes (2^-60 .. 2^60) are measured on the
    // device when they arrive; outside, psm_cost_filter runs the storing form (the oracle's arithmetic op for op) + k_wta.
    // (The images' answer is pair.st.inside.)
    bool vol_domain_ok[2] = {true, true};
    unsigned *range_dev = nullptr;      // [4][2] exponent ranges (current pair, staged pair, volume L, volume R), on first use
    unsigned *range_pin = nullptr;      // page-locked copy

    // options
    int opt_async = 0, opt_variant = 0, opt_profile = 0, opt_graph = 0, opt_gather_staged = 0;
    psm::March march = {0, 4, 0};

    double stage_us[PSM_STAGE_COUNT] = {0, 0, 0, 0};
    psm::KernelTimer timers[PSM_K_COUNT];
    std::vector<hipEvent_t> event_pool;
    std::string err;
};

namespace psm {

int fail(psm_ctx *c, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define PSM_HIP(c, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return psm::fail((c), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

double now_us();
hipEvent_t get_event(psm_ctx *c);
int check_launch(psm_ctx *c, const char *what);
int end_stage(psm_ctx *c, int stage, double t0);
int bind(psm_ctx *c);
inline size_t velem(const psm_ctx *c) { return c->dtype == PSM_U8 ? 1 : 4; }
// Call before anything on c->stream writes c->maps: the buffer may still be the source of an asynchronous download
// (psm_download_maps_async on the copy stream) - the writer waits for that copy on the device, the host never blocks.
inline int maps_writable(psm_ctx *c)
{
    if (c->ev_down) PSM_HIP(c, hipStreamWaitEvent(c->stream, c->ev_down, 0));
    return 0;
}

// The profile bracket of a launch sequence (psm::Bracket).  events: before anything is ordered or launched, its events exist while
// PSM_OPT_PROFILE is set; open / close: around the launches on stream s - c is the context whose option decides, a batch's first;
// ms: what the stage's _time getter answers - `have`: the result the bracket belongs to still exists, `not_timed`: the getter's
// refusal; free: with the stage's scratch.
inline int bracket_events(psm_ctx *c, Bracket &b)
{
    if (c->opt_profile)
        for (hipEvent_t &e : b.ev)
            if (!e) PSM_HIP(c, hipEventCreate(&e));
    return 0;
}
inline int bracket_open(psm_ctx *c, Bracket &b, hipStream_t s)
{
    b.timed = false;
    if (c->opt_profile) PSM_HIP(c, hipEventRecord(b.ev[0], s));
    return 0;
}
inline int bracket_close(psm_ctx *c, Bracket &b, hipStream_t s)
{
    if (c->opt_profile) PSM_HIP(c, hipEventRecord(b.ev[1], s));
    b.timed = c->opt_profile != 0;
    return 0;
}
inline int bracket_ms(psm_ctx *c, const Bracket &b, bool have, const char *who, const char *not_timed, double *ms)
{
    if (!ms) return fail(c, "%s: NULL pointer", who);
    if (!have || !b.timed) return fail(c, "%s: %s", who, not_timed);
    if (bind(c)) return 1;
    PSM_HIP(c, hipEventSynchronize(b.ev[1]));
    float t = 0.f;
    PSM_HIP(c, hipEventElapsedTime(&t, b.ev[0], b.ev[1]));
    *ms = t;
    return 0;
}
inline void bracket_free(Bracket &b)
{
    for (hipEvent_t &e : b.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    b.timed = false;
}

// RAII bracket of one kernel launch with hipEvents on the launch stream (PSM_OPT_PROFILE 1); s: that stream if it is not the
// context's (the rectification of a pair staged on the copy stream)
struct Prof {
    psm_ctx *c;
    int k;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    Prof(psm_ctx *c_, int k_, hipStream_t s_ = nullptr) : c(c_), k(k_), s(s_ ? s_ : c_->stream)
    {
        if (c->opt_profile == 1) {
            a = get_event(c);
            b = a ? get_event(c) : nullptr;
            if (a && !b) { c->event_pool.push_back(a); a = nullptr; }
            if (a) (void)hipEventRecord(a, s);
        }
    }
    ~Prof()
    {
        if (a) {
            (void)hipEventRecord(b, s);
            c->timers[k].pending.emplace_back(a, b);
        }
    }
};

// psm_api_core.cpp
int h2d_rows(psm_ctx *c, void *dst, const void *src, size_t row, size_t stride, int rows);   // host rows -> packed device rows
// packed device rows -> host rows `stride` bytes apart, on the context's stream and complete on return; rows that are packed on
// the host as well (stride == row) are the copy's own destination
inline int d2h_rows(psm_ctx *c, void *dst, const void *src, size_t row, size_t stride, int rows)
{
    std::vector<uint8_t> packed(stride == row ? 0 : row * rows);
    PSM_HIP(c, hipMemcpyAsync(stride == row ? dst : packed.data(), src, row * rows, hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    if (stride != row)
        for (int y = 0; y < rows; ++y) memcpy((uint8_t *)dst + (size_t)y * stride, packed.data() + (size_t)y * row, row);
    return 0;
}

// psm_api_core.cpp: the image pair slots (psm::PairSlots)
void pair_slots_free(psm_ctx *c);
void adopt_new_pair(psm_ctx *c);                 // a new image pair is current: nothing derived from the previous one survives
// a blocking upload has filled raw: it supersedes a staged pair, adopts the new one and sets the domain flag
inline void pair_uploaded(psm_ctx *c, int depth, bool inside) { uploaded(c->pair.st, depth, inside); adopt_new_pair(c); }
// The staging sequence of the two asynchronous forms, all on the copy stream.  They differ in where they record ev_stage[slot]
// relative to their wait for ev_free, and in what runs between send and commit.
//   begin:  a pair staged before is given up (raw_next is about to be overwritten); copy stream, ev_up, ev_free, (pin: pin_up,)
//           raw_next - each on first use; the next staging slot; its event is created, or waited for on the host: the copy out of
//           the slot issued TWO uploads ago is over
//   pack:   the caller's rows into a page-locked destination
//   send:   `bytes` from a page-locked source to the device - up to PSM_COPY_KERNEL_MAX by the copy kernel, else by a copy engine
//           (the form checks the launch)
//   commit: ev_up behind what the form enqueued; the pair is staged
int stage_begin(psm_ctx *c, bool pin, int *slot);
void stage_pack(void *dst, const void *src, size_t row, size_t stride, int rows);
void stage_send(psm_ctx *c, void *dst, const void *pinned, size_t bytes);
int stage_commit(psm_ctx *c, int depth, bool range_pending);
// Is the pair the next psm_cost_construct will find - the staged one, else the current one - inside the select forms' domain?  Waits
// on the host for a range still on its way; asking again is free.
int next_pair_inside(psm_ctx *c, bool *inside);
int adopt_staged_pair(psm_ctx *c);               // the staged pair becomes the current one (psm_cost_construct, psm_compute_batch)
// Behind the last launch of a sequence on stream s that reads c's raw: the slot may be overwritten once the stream gets here.  A
// context that never uploaded asynchronously has no ev_free and records nothing.
inline int images_read(psm_ctx *c, hipStream_t s)
{
    if (c->pair.ev_free) PSM_HIP(c, hipEventRecord(c->pair.ev_free, s));
    return 0;
}

// The plane rows a filter reads: the whole image, or - a psm_set_rows stripe [y0, y1) being in force - what the select form of
// the fused kernel touches for it: the guidance of the model rows y0 - 4 .. y1 + 2 (rounded to +- 4), and the image planes of
// the rows y0 - 8 .. y1 + 7 (the costs of those model rows, +- 4 for their box sums, and their guidance).
struct PlaneRows { Rows g1, guid; };
inline Rows whole_image(const psm_ctx *c) { return whole_image(c->H); }
inline bool stripe_only(const psm_ctx *c) { return !(c->res.rows == whole_image(c)); }   // the current minima / maps cover a row stripe
inline Rows stripe_rows(const psm_ctx *c) { return c->march.yend > c->march.ybeg ? Rows{c->march.ybeg, c->march.yend} : whole_image(c); }   // psm_set_rows
inline PlaneRows stripe_planes(const psm_ctx *c)
{
    const int H = c->H, a = c->march.ybeg, b = c->march.yend;
    if (b <= a) return {whole_image(c), whole_image(c)};
    return {Rows{a > 8 ? a - 8 : 0, b + 8 < H ? b + 8 : H}, Rows{a > 4 ? a - 4 : 0, b + 4 < H ? b + 4 : H}};
}
// psm_api_filter.cpp
int ensure_planes(psm_ctx *c, Rows g1_need, Rows guid_need);   // an empty need: those planes are not asked for
int ensure_vol(psm_ctx *c, int side);
int ensure_ab(psm_ctx *c);
int ensure_spare(psm_ctx *c);
int fgf_flush(psm_ctx *c, int side);
int materialize(psm_ctx *c, int side);
int ensure_gf_scratch(psm_ctx *c, size_t bytes);
// The select path of the default product path - fused select filter of both volumes, reduction - for one pair (psm_cost_filter)
// or the pairs of a batch (psm_compute_batch)
PcPair pc_pair(const psm_ctx *c);                // the context's pair as the launchers see it (an entry of the batch table)
struct SelPlan {
    bool two_phase;
    int S, n1, n2;          // the plane form runs n1 slices (every S-th; one phase: all, S = 1), the key form the other n2
    bool maps;              // the reduction writes the maps
    size_t scratch_bytes;   // chunk planes per pair (both volumes)
};
SelPlan select_plan(const psm_ctx *c, int npairs, bool batch);
int enqueue_select(psm_ctx *c, const Recs<PcPair> &q, const SelPlan &sp);
// PSM_FLAG_FMA_SOLVE applies to float mode only (8-bit contexts never carry the bit: psm_set_option)
inline bool fma_solve(const psm_ctx *c) { return c->dtype == PSM_F32 && (c->march.flags & PSM_FLAG_FMA_SOLVE) != 0; }
// psm_create_shard_strided: the slices of such a context exist in the select forms of the fused kernel only
inline bool strided(const psm_ctx *c) { return c->march.dstep != 1; }
#define PSM_NOT_STRIDED(c, what)                                                                                               \
    do {                                                                                                                        \
        if (psm::strided(c)) return psm::fail((c), "%s: a strided disparity shard (psm_create_shard_strided) runs the default select path only", (what)); \
    } while (0)
inline bool scaled_forms_ok(const psm_ctx *c) { return c->pair.st.inside && c->vol_domain_ok[0] && c->vol_domain_ok[1]; }
constexpr int PSM_IMG_EXP = 10, PSM_VOL_EXP = 60;
constexpr size_t PSM_COPY_KERNEL_MAX = (size_t)2 << 20;     // asynchronous PCIe legs up to this size go through k_copy16 instead of the copy engines
unsigned long long *next_pc_stamp(psm_ctx *c);   // slot of the next k_cvf_pc launch (NULL unless PSM_OPT_PROFILE 2)

// psm_api_batch.cpp: what the batch entry points share.  c0: the batch's first context, which owns the table,
// whose stream the shared launches run on and which receives every message.
int batch_member(psm_ctx *c0, const char *who, psm_ctx *const *ctxs, int i);    // ctxs[i] is a context, and none of ctxs[0..i)
int member_failed(psm_ctx *c0, const char *who, int i, const psm_ctx *c);        // the error of member i as the batch's: returns 1
int table_reserve(psm_ctx *c0, DevTable &t, const void *recs, size_t bytes, bool *fresh);
int table_upload(psm_ctx *c0, DevTable &t, const void *recs, size_t bytes);
void table_free(DevTable &t);
int batch_events(psm_ctx *c0, psm_ctx *const *ctxs, int n);
int batch_join(psm_ctx *c0, psm_ctx *const *ctxs, int n);
int batch_fork(psm_ctx *c0, psm_ctx *const *ctxs, int n);
// psm_api_rectify.cpp
void rectify_free(psm_ctx *c, bool maps);        // the source slots and their staging; maps: the device maps too
// psm_api_jwmf.cpp
void jwmf_batch_free(psm_ctx *c);                // what the context holds as the first of a psm_joint_wmf_batch
// psm_api_sgm.cpp
void sgm_free(psm_ctx *c);                       // the stage's buffers and events (its parameters stay)
// psm_api_pp.cpp
void wm_free(psm_ctx *c, bool all);              // the weighted median's scratch, counters, snapshots and table; all: its events too
// psm_api_score.cpp
void score_free(psm_ctx *c, bool truth);         // the stage's scratch and events; truth: the uploaded truth, mask and hook map too
// The int16 map the SGM source of psm_wls_filter reads - the plane of psm_score_upload_sgm_map while it is on, else the last
// psm_sgm_compute*'s - and the invalid value of the range it belongs to (the hook plane: the current setting's) ...
inline const int16_t *sgm_stage_map(const psm_ctx *c) { return c->score.hook_on ? c->score.hook : c->sgm.out; }
inline int sgm_stage_invalid(const psm_ctx *c) { return ((c->score.hook_on ? c->sgm.dmin : c->sgm.res_dmin) - 1) * 16; }
inline bool sgm_stage_exists(const psm_ctx *c) { return c->sgm.have || c->score.hook_on; }
// ... and the one the SGM sources of psm_score and psm_reproject read: the same, or - psm_wls_publish being on and no hook plane -
// the result of the last psm_wls_filter with the invalid value it was made with
inline bool wls_published(const psm_ctx *c) { return c->wls.publish && c->wls.have && !c->score.hook_on; }
inline const int16_t *sgm_source_map(const psm_ctx *c) { return wls_published(c) ? c->wls.out : sgm_stage_map(c); }
inline int sgm_source_invalid(const psm_ctx *c) { return wls_published(c) ? c->wls.invalid : sgm_stage_invalid(c); }
inline bool sgm_source_exists(const psm_ctx *c) { return wls_published(c) || sgm_stage_exists(c); }
// psm_api_depth.cpp
void depth_free(psm_ctx *c);                     // the stage's scratch and events (its parameters stay)
// The left image the colours of psm_reproject's cloud come from, and the guide of psm_wls_filter: the current pair's, or - an SGM
// source whose result psm_sgm_compute_gray made - that call's left plane; img null: there is none.  slots: it lies in the image
// pair slots (the read mark applies)
struct Colour {
    const void *img;
    int depth, ch;
    bool slots;
};
inline Colour colour_of(const psm_ctx *c, bool sgm_source)
{
    const SgmState &g = c->sgm;
    if (sgm_source && g.have && g.res_ch == 1 && g.gray[0]) return Colour{g.gray[0], PSM_IMG_U8, 1, false};
    if (c->pair.st.depth < 0) return Colour{nullptr, 0, 3, false};
    return Colour{c->pair.raw[0], c->pair.st.depth, 3, true};
}
// psm_api_wls.cpp
void wls_free(psm_ctx *c);                       // the stage's planes and events (its parameters stay); publishing is switched off
// psm_api_gray.cpp
void gray_free(psm_ctx *c);                      // the stage's buffers and events: no pair of a psm_gray_compute is left
// psm_api_select.cpp: copy_maps_out - two [H][W] planes on the device to the caller's rows
int copy_maps_out(psm_ctx *c, const uint8_t *dev, uint8_t *lmap, uint8_t *rmap, size_t stride);

}  // namespace psm
