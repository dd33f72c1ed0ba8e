// psm_kernels.h - launcher interface between the C-ABI layer (psm_api_*.cpp) and the gfx950
// kernels (psm_kernels.hip, psm_pc.hip, psm_fgf.hip, psm_pp.hip).  Internal to libprimesm_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "psm_live.h"
#include "psm_wm_sched.h"
#include "psm_wls_tab.h"

namespace psm {

// Per-pixel guidance of one side, packed for 16-byte lane loads (DESIGN.md "HBM layout").
//   g1[y][x] = { I0, I1, I2, GrdX }            I_c = image channel c (c0=B), GrdX = x-gradient of gray
//   g2[y][x] = { mI0, mI1, mI2, 1/DET }        mI_c = box(I_c)
//   g3[y][x] = { A00, A01, A02, A11 }          A_rc = the distinct adjugate entries of Sigma+eps*I
//   g4[y][x] = { A12, A22 }
struct Guidance {
    float4 *g1;
    float4 *g2;
    float4 *g3;
    float2 *g4;
};

struct March {       // geometry of the marching kernels
    int seg_rows;    // output rows per y-segment (0 = auto)
    int waves;       // waves (= disparity slices) per workgroup: 1,2,4,8
    int flags;       // PSM_OPT_FLAGS (include/primesm_hip.h)
    int dstep = 1;            // psm_create_shard_strided: local slice i is the global disparity d_begin + i * dstep (select forms only)
    int inflight = 1;         // PSM_OPT_FRAMES_IN_FLIGHT: pairs other contexts filter at the same time on their own streams (a planning hint only)
    int ybeg = 0, yend = 0;   // row stripe of the select-form filter (psm_set_rows): output rows [ybeg, yend) of the whole
                              // image; yend <= ybeg: all rows
    int y0(int H) const { (void)H; return yend > ybeg ? ybeg : 0; }
    int y1(int H) const { return yend > ybeg ? yend : H; }
    int rows(int H) const { return y1(H) - y0(H); }
};

// ---- batched launches: B stereo pairs of one geometry share every launch of the default path (psm_compute_batch; the
// reference's use on Middlebury-size data is a loop over pairs, src/main.cpp:64-73) ----
struct PcPair {                  // one pair's buffers: what a single call passes by value, an entry of a batch's device table (Recs below)
    const void *raw[2];          // staged interleaved images (left, right)
    Guidance g[2];
    uint8_t *p4[2];              // 8-bit char mode: {c0,c1,c2,grad} byte planes (else null)
    void *scratch;               // chunk planes of the select kernel (both sides)
    long long *keys;             // [2][H][W] packed minima
    uint8_t *maps;               // [2][H][W]
};                               // (a one-volume launch of the fused filter and its reduction: that volume's side in [0], its keys [H][W])
// ---- record sources: what every stage with a batch entry (the default path - prep, guidance, fused select filter, reduction -,
// post-processing tail, JointWMF, SGM and speckle, score, depth, WLS) shares ----
// The n records R of one launch as the host filled them, the record on a grid axis.  dev == nullptr: the records of a single call
// travel by value in the kernarg (RecVal: one record; the two of JointWMF's single pair); else the kernels read the n records of the
// device table at dev.  Either way the index is uniform per workgroup: scalar loads ahead of one body.  Every kernel of these stages
// is one template over the two sources, S = RecVal<R, N> or RecTab<R>, and rec(src, i) is record i of either.
template <typename R> struct Recs { const R *host, *dev; int n; };
template <typename R, int N = 1> struct RecVal { R r[N]; };
template <typename R> using RecTab = const R *;
template <typename R> __device__ __forceinline__ const R &rec(const R *tab, unsigned i) { return tab[i]; }
template <typename R, int N> __device__ __forceinline__ const R &rec(const RecVal<R, N> &v, unsigned i) { return v.r[N == 1 ? 0 : i]; }
// A pointer a kernel reads from the table is a flat pointer to the compiler (one that arrives as a kernel argument is known to be
// global): every access through it would become a flat_* instruction, which counts on vmcnt and lgkmcnt at once and makes the
// body wait for everything in flight (k_sgm_path over the table with flat accesses: 0.44 ms for a batch of one Cones pair against
// 0.38 ms).  Reading the record's slot as one that holds a global pointer gives the table instantiations the global_* instructions
// of the by-value ones (a cast of the loaded value to global and back is folded away before it can tell anyone).
template <typename T>
__device__ __forceinline__ T *sgm_global(T *const &slot) { return (T *)*(__attribute__((address_space(1))) T *const *)(const void *)&slot; }
// one launch of a kernel over either source: its two instantiations, the grid with q.n on the record's axis
template <typename T> struct RecArg { using type = T; };
template <typename R, int N, typename... A>
void rec_launch(hipStream_t st, void (*kv)(RecVal<R, N>, A...), void (*kt)(const R *, A...), dim3 grid, dim3 block, size_t lds, const Recs<R> &q,
                typename RecArg<A>::type... rest)
{
    if (q.dev) {
        hipLaunchKernelGGL(kt, grid, block, lds, st, q.dev, rest...);
        return;
    }
    RecVal<R, N> v;
    for (int i = 0; i < N; ++i) v.r[i] = q.host[i < q.n ? i : q.n - 1];
    hipLaunchKernelGGL(kv, grid, block, lds, st, v, rest...);
}
// ... of a kernel that takes the call's scalars H ahead of the source (SGM, speckle, score: the argument order of their earlier entries)
template <typename H, typename R, int N, typename... A>
void rec_launch(hipStream_t st, void (*kv)(H, RecVal<R, N>, A...), void (*kt)(H, const R *, A...), dim3 grid, dim3 block, size_t lds, const H &head,
                const Recs<R> &q, typename RecArg<A>::type... rest)
{
    if (q.dev) {
        hipLaunchKernelGGL(kt, grid, block, lds, st, head, q.dev, rest...);
        return;
    }
    RecVal<R, N> v;
    for (int i = 0; i < N; ++i) v.r[i] = q.host[i < q.n ? i : q.n - 1];
    hipLaunchKernelGGL(kv, grid, block, lds, st, head, v, rest...);
}

// the default path's two sources: its kernels are templates over S = PcVal (120 bytes of kernarg) or PcTab
using PcVal = RecVal<PcPair>;
using PcTab = RecTab<PcPair>;
void launch_merge_batch(hipStream_t s, const Recs<PcPair> &q, int W, int H);   // keys -> maps of every pair of a batch's table

// device <-> page-locked host copy as a kernel (both pointers 16-byte aligned)
void launch_copy_bytes(hipStream_t s, void *dst, const void *src, size_t bytes);
// biased-exponent range of n floats: out[0] = max, out[1] = min over the non-zero values (initialise out to {0, 255})
void launch_range_f32(hipStream_t s, const float *p, size_t n, unsigned *out);
// staged images (raw, row pitch `pitch`) -> rows [y0, y1) of g1 (planarise, scale, gray, x-gradient) of both images of every pair in
// q, one launch.  u8_planes: the launch of 8-bit char mode instead - the {c0,c1,c2,grad} byte planes p4, the same word also into
// g1[..].w (bit pattern) of the image's g1 plane: after the launch that writes g1
void launch_prep(hipStream_t s, const Recs<PcPair> &q, size_t pitch, int depth_f32, int W, int y0, int y1, bool u8_planes);
// g1 -> g2,g3,g4 of both images of every pair in q, one launch ([ybeg, yend): rows of g2..g4 to produce, yend <= ybeg: all).
// fma: PSM_FLAG_FMA_SOLVE - minors and DET in their fused forms.  src 1 / 2: image preparation (launch_prep) in the same launch
// from the pairs' staged 8-bit / float images (raw, row pitch `pitch`) - the g1 rows [ybeg, yend) are written from them
void launch_guidance(hipStream_t s, const Recs<PcPair> &q, int W, int H, int ybeg, int yend, bool fma, int src = 0, size_t pitch = 0);
// cost volume slices [d_begin, d_begin+Dloc) of one side.  base: g1 of the side's own image.
void launch_cvc(hipStream_t s, const float4 *g1_base, const float4 *g1_other, float *vol, int W, int H,
                int d_begin, int Dloc, int right, int ybeg, int yend);
// Stage A of the guided filter alone (the debug entry psm_filter_stage_a; tests compare (a0,a1,a2,b) with the oracle's
// intermediates).  variant 0 = marching, 1 = direct per-voxel.  [ybeg, yend): output rows of this launch (the arithmetic
// always refers to the full H-row planes).  Stage B alone exists in the direct formulation only (cross-check).
void launch_cvf_a(hipStream_t s, int variant, March m, const float *vol, float4 *ab, Guidance g, int W,
                  int H, int Dloc, int ybeg, int yend);
void launch_cvf_b_direct(hipStream_t s, const float4 *ab, float *vol, Guidance g, int W, int H, int Dloc);
// fused stage A+B: vin -> vout (distinct buffers), output rows [ybeg, yend) within [4, H-3)
// cvc_mode 0: read the cost slices from vin; 1/2: build the left/right costs on the fly from the g1 planes
// One volume per launch: q is one record (by value, q.dev == nullptr) that carries the volume's own side FIRST - g[0] its
// guidance, g[1].g1 the other image; likewise launch_cvf_select below.
void launch_cvf_fused(hipStream_t s, March m, const Recs<PcPair> &q, const float *vin, float *vout, int W, int H, int Dloc,
                      int ybeg, int yend, int d_begin, int cvc_mode, unsigned long long *ts = nullptr);
// The same kernel with the winner-takes-all fused in ("select" forms): the filtered volume is never written.
//   plane form: per pixel the running minimum over chunks of DC slices in scratch planes -> launch_chunk_min* -> packed WTA keys
//   key form:   64-bit atomicMin on a key plane that already holds good bounds (second phase of the two-phase selection)
struct PcDev { int nxcd = 0, cus_per_xcd = 0; };
PcDev pc_dev();                                                  // of the device the calling thread is bound to
enum { PC_STORE = 0, PC_PLANES = 1, PC_KEYS = 2, PC_BOTH = 4 };  // forms of pc_plan (PC_BOTH: both volumes per launch)
struct PcPlan {
    int ngroups, nsegs, seg_rows, DC, nchunks, nbmax, nxcd;
    int cols;                                                    // output columns per column group (107; 50 in the narrow layout; 96 storing form)
    bool narrow;                                                 // two-wave workgroups (one producer + one consumer wave)
    size_t rec_per_chunk;                                        // records per chunk plane
    int rec_bytes;                                               // bytes per record (costs + disparities)
    size_t scratch_bytes() const { return rec_per_chunk * (size_t)nchunks * rec_bytes; }
};
PcPlan pc_plan(int W, int rows, int Dloc, int seg_rows_opt, int form, int batch = 1, int inflight = 1);   // batch: pairs per launch (psm_compute_batch); inflight: March::inflight
// pc_plan of the two-volume select launches (form PC_PLANES / PC_KEYS) of npairs pairs; batch: the pairs of psm_compute_batch
PcPlan pc_plan_select(March m, int W, int H, int Dloc, int form, int npairs, bool batch);
int pc_seed_stride(int W, int rows, bool u8);                     // S of the two-phase selection: every S-th slice seeds the key plane (rows: of the stripe being filtered)
// ts (may be NULL): slot of this launch in a buffer of 3 x PC_TS_SLOTS 64-bit words {first workgroup start | last workgroup
// end | form} in ticks of the device's constant-rate clock (PSM_OPT_PROFILE 2, psm_filter_launch_times)
constexpr int PC_TS_SLOTS = 4096;
// one volume per launch (costs read from vin, cvc_mode 0, or built on the fly, 1 / 2; u8: 8-bit char mode): the first side of q's
// one record - its byte planes p4[0] against p4[1], its chunk planes at the start of the record's scratch
void launch_cvf_select(hipStream_t s, March m, const Recs<PcPair> &q, const float *vin, bool u8, int W, int H, int Dloc, int d_begin,
                       int cvc_mode, unsigned long long *ts = nullptr);
// ... its reduction, over the same record: the chunk planes in q's scratch -> q's keys (one volume's: [H][W])
void launch_chunk_min(hipStream_t s, March m, const Recs<PcPair> &q, int W, int H, int Dloc);
// both volumes of every pair in q per launch (costs on the fly; u8: 8-bit char mode): the left volume is filtered with the guidance
// g[0] of the left image, the right one with g[1]; keys / maps: [2][H][W] per pair; grid z = pair (a single pair: 1).  Dloc slices,
// which ones: (sel, step) - 0: all, 1: every step-th, 2: the others.
// ... plane form: chunk planes in each pair's scratch (2 x pc_plan_select(..., PC_PLANES, ...).scratch_bytes())
void launch_cvf_select2(hipStream_t s, March m, const Recs<PcPair> &q, bool u8, int W, int H, int Dloc, int d_begin, unsigned long long *ts,
                        int sel, int step);
// ... their reduction to each pair's keys; to_maps: the maps as well
// d_begin, (sel, step): as given to launch_cvf_select2 - chunks it did not walk (psm_live.h) are not read
void launch_chunk_min2sides(hipStream_t s, March m, const Recs<PcPair> &q, int W, int H, int Dloc, bool to_maps, int d_begin, int sel, int step);
// ... key form: continues from the minima each pair's keys hold (the second phase of the two-phase selection)
void launch_cvf_select_keys2(hipStream_t s, March m, const Recs<PcPair> &q, bool u8, int W, int H, int Dloc, int d_begin,
                             unsigned long long *ts, int sel, int step);
// plain 8x8 box filter of every slice (the north-star kernel in isolation)
void launch_box8(hipStream_t s, int variant, March m, const float *vol, float *out, int W, int H, int Dloc);
// WTA over local slices -> packed keys (keys != NULL) and/or final map (map != NULL)
void launch_wta(hipStream_t s, const float *vol, int W, int H, int d_begin, int Dloc, long long *keys,
                uint8_t *map);
// min over nranks key planes -> map
void launch_merge(hipStream_t s, const long long *keys_all, size_t rank_stride, int nranks, int n,
                  uint8_t *map);
// (the left-right check and the fill of invalid pixels: with the post-processing tail below, PpRecs)

// weighted-median post-filter of one map, in place, with the reference's raster-order semantics (psm_pp.hip).
// nxt: scratch of H*(W+1) ints, prog: H ints, err: 1 int (set to 1 if the dataflow watchdog fired)
void launch_wgt_median(hipStream_t s, uint8_t *dis, const uint8_t *valid, const float4 *g1, int W, int H, int maxDis, int right,
                       int *nxt, int *prog, int *err);
// parallel form (sweeps to the fixed point of the in-place recursion; psm_pp.hip)
// (WM_LANE_MIN, WM_WROW, WM_WPIX, the sweep cap and the counters' accessors: psm_wm_sched.h)
// One map's share of the sweep state.  Sweep k (0-based) evaluates the list act = k ? list[(k + 1) & 1] : inv, whose length is
// cnt[2k]; it leaves the number of changed pixels in cnt[2k + 1], the changed pixels in chg, and the next sweep's list in
// list[k & 1] / cnt[2k + 2]; cnt[0] is the number of invalid pixels (inv).  Both maps go through every launch side by side
// (blockIdx.y): below the first sweeps a kernel is a few hundred waves, and the two maps are independent.
struct WmSide {
    uint8_t *cur;                 // the map, filtered in place
    const uint8_t *valid;
    const float4 *g1;
    uint8_t *orig, *newv, *chgb, *rowany;      // input copy, new values of changed pixels, byte maps of the gather form
    int *stamp, *list[2], *chg, *slot_of, *inv, *cnt;
    const float *wts;             // weight cache of this map (null: none, or an empty map)
};
struct WmPair { WmSide s[2]; };
// One pair of the post-processing tail (psm_lr_check, psm_fill_invalid, psm_wgt_median, psm_post_process_batch) as its kernels find
// it, the pair on blockIdx.z and the side on blockIdx.y: the sweep state of its two maps - of which the L-R check and the fill read
// cur and valid alone - and the masks as the L-R check writes them.  A side's cnt lies in the counter block of the call's first
// context, the counters of all maps one behind the other; wts of every side is set when the call is cached.
struct PpPair {
    WmPair wm;
    uint8_t *lv, *rv;
};
// The records of one call (Recs above): a single pair travels by value (256 bytes of kernarg), several through the device table.
using PpRecs = Recs<PpPair>;
using PpVal = RecVal<PpPair>;
using PpTab = const PpPair *__restrict__;      // (RecTab<PpPair> with the qualifier the tail's kernels were written and measured with)
void launch_lr_check(hipStream_t s, const PpRecs &q, int W, int H);       // left-right check of the two maps of every pair -> lv, rv
void launch_fill_inv(hipStream_t s, const PpRecs &q, int W, int H);       // fill of the invalid pixels of every map in place
void launch_wm_seed(hipStream_t s, const PpRecs &q, int W, int H);        // (the counters of all maps are zero: the caller's memset)
void launch_wm_weights(hipStream_t s, const PpRecs &q, int W, int H, int n_max);   // n_max: an upper bound of the invalid pixels of any side
void launch_wm_sweep(hipStream_t s, const PpRecs &q, int W, int H, int maxDis, int sw, bool cached, bool tail);

// ---- Fast Guided Filter variant (psm_fgf.hip); sub = subsample rate, small planes are (H/sub) x (W/sub) ----
// g1 -> subsampled guidance ism, its means msm and the inverse covariance planes v1 = {irr,irg,irb,igg}, v2 = {igb,ibb}
void launch_fgf_setup(hipStream_t s, const float4 *g1, int W, int H, int sub, float4 *ism, float4 *msm, float4 *v1, float2 *v2);
// First half of the filter for Dloc slices: subsampled cost (cvc_mode 0: read from vol; 1/2: left/right costs of the
// sampled pixels built from the g1 planes) -> linear models -> smoothed models mab (Dloc*(H/sub)*(W/sub) float4;
// ab: scratch of the same size).
void launch_fgf_model(hipStream_t s, const float *vol, const float4 *g1, const float4 *g1_other, int W, int H, int Dloc, int d_begin,
                      int sub, int cvc_mode, const float4 *msm, const float4 *v1, const float2 *v2, float4 *ab, float4 *mab);
// Second half: bilinear upsampling of mab + q = a.I + b, written to vol ...
void launch_fgf_apply(hipStream_t s, float *vol, const float4 *g1, int W, int H, int Dloc, int sub, const float4 *mab);
// ... or consumed on the fly by the WTA: keys[H*W] receives the packed (cost, d) minimum over the local slices and the
// filtered volume is never written (needs fgf_can_fuse_wta(W))
bool fgf_can_fuse_wta(int W);
void launch_fgf_apply_wta(hipStream_t s, const float4 *g1, int W, int H, int Dloc, int d_begin, int sub, const float4 *mab,
                          long long *keys);

// ---- 8-bit char mode ----  (the {c0,c1,c2,grad} byte planes: launch_prep)
void launch_cvc_u8(hipStream_t s, const uint8_t *base4, const uint8_t *other4, uint8_t *vol, int W, int H,
                   int d_begin, int Dloc, int right);
void launch_u8_to_f32(hipStream_t s, const uint8_t *src, float *dst, size_t n);
void launch_f32_to_u8(hipStream_t s, const float *src, uint8_t *dst, size_t n);
void launch_wta_u8(hipStream_t s, const uint8_t *vol, int W, int H, int d_begin, int Dloc, long long *keys,
                   uint8_t *map);

// psm_jwmf.hip: the joint weighted median (psm_joint_wmf, psm_api_jwmf.cpp)
constexpr int JW_KEYS = 1 << 18;       // 6-bit B, G, R colour keys
constexpr int JW_NF_MAX = 256;         // clusters at most; the integer weight table of a side is [JW_NF_MAX][JW_NF_MAX]
constexpr int JW_RMAX = 16;            // window radius at most: (2r+1)^2 <= 1089 taps, every integer sum < 2^59
struct JwSide {
    const void *img;                   // staged interleaved B,G,R image (PSM_IMG_U8 bytes or PSM_IMG_F32 floats)
    const uint8_t *lok;                // cluster of every key [JW_KEYS]
    uint8_t *F;                        // cluster plane [H][W]
    const uint8_t *din;                // input map [H][W]
    const unsigned long long *wq;      // rint(w * 2^48) [JW_NF_MAX][JW_NF_MAX]
    uint8_t *out;                      // filtered map [H][W]
};
// One image to cluster.  Buffers are the context's own (JwScratch), but for state and centres: those lie side by side in a block of
// the call's first context (JwBatch), so the host reads all of them in one copy.
struct JwImg {
    const void *img;
    unsigned *bits, *samples, *kt, *d2t;
    int *labels, *sums;
    int *state;                        // {changed, converged, iterations, sample count}
    float *centres;                    // [JW_NF_MAX][3]
    uint8_t *lok;
    int n, nf;                         // sample count and clusters: known once the samples have been counted
};
// The records (R: JwImg, JwSide) of one launch (Recs above): the n <= 2 records of a single pair travel by value
template <typename R> using JwRecs = Recs<R>;
template <typename R> using JwVal = RecVal<R, 2>;
void launch_jw_keys(hipStream_t s, const JwRecs<JwImg> &im, int depth, size_t HW);           // clears the bitmaps first
void launch_jw_compact(hipStream_t s, const JwRecs<JwImg> &im);
void launch_jw_identity(hipStream_t s, const JwRecs<JwImg> &im, int n_clusters);             // the images with n <= n_clusters
void launch_jw_seed(hipStream_t s, const JwRecs<JwImg> &im, int n_clusters, unsigned long long seed);   // ... the others; leaves the Lloyd state ready
void launch_jw_lloyd(hipStream_t s, const JwRecs<JwImg> &im, int n_max, int it);             // one Lloyd iteration (assignment + update) of every image
void launch_jw_lok(hipStream_t s, const JwRecs<JwImg> &im, int n_max);                       // clears the tables first
void launch_jw_plane(hipStream_t s, const JwRecs<JwSide> &sides, int depth, size_t HW);
void launch_jw_median(hipStream_t s, const JwRecs<JwSide> &sides, int W, int H, int r);

// psm_rectify.hip: remap (CV_16SC2 maps, INTER_LINEAR, constant border 0) + crop of both eyes (psm_api_rectify.cpp)
struct RectSide {
    const uint8_t *src;                // unrectified eye image, interleaved B,G,R rows of `pitch` bytes (8 readable bytes behind the last)
    const uint32_t *xy;                // crop window of the map: {int16 x, int16 y} per output pixel, [npix]
    const uint16_t *fr;                // ... fy * 32 + fx
    uint32_t *out;                     // staged image slot: npix interleaved B,G,R pixels, written as ndw whole dwords
};
struct RectArgs {
    RectSide s[2];
    int npix, ndw;                     // W * H of the context; (3 * npix + 3) / 4
    int src_w, src_h;
    unsigned pitch;
};
void launch_rectify(hipStream_t s, const RectArgs &a);

// psm_sgm.hip: semi-global matching over the staged pair (psm_sgm_compute, psm_api_sgm.cpp)
// The scalars of one call - a single pair's or a batch's; the pair's buffers are its SgmPair
struct SgmArgs {
    int depth, ch;                     // of the staged images: PSM_IMG_U8 bytes or PSM_IMG_F32 floats, interleaved `ch` channels
    int W, H, D, Dp;                   // Dp: elements per pixel, sgm_dp(D)
    int dmin, invalid;                 // psm_sgm_set_range: index k in [0, D) is the disparity dmin + k; invalid = (dmin - 1) * 16
    int bs, P1, P2, u, m;
    int ft;                            // the prefiltered Birchfield-Tomasi cost (launch_sgm_cost_bt only; psm_sgm_set_prefilter): max(pre_filter_cap, 15) | 1
    int cw, chh;                       // the census cost (launch_sgm_cost_census only; psm_sgm_set_census): the window
};
// One pair's buffers: what a single call passes by value and what a batch's device table (psm_sgm_compute_batch) holds per pair,
// indexed with the pair number (blockIdx.z).  The horizontal block sums Hs of the Birchfield-Tomasi cost, u16 [H][W][Dp], lie in
// the memory of S (free until the first direction stores it).
struct SgmPair {
    const void *img[2];                // staged images
    uint16_t *C;                       // block costs [H][W][Dp]
    uint32_t *S;                       // summed path costs [H][W][Dp]
    uint32_t *disp2;                   // [H][W] packed minima (minS << KB | best index) landing on the right image's pixel, KB = sgm_kb(Dp); all ones: none
    int16_t *pre, *out;                // [H][W] d16 (or `invalid`: not unique) before the consistency test / the final map
    uint8_t *pf[2];                    // the prefiltered planes of both images, [H][W][2 ch] bytes: P_0 .. P_{ch-1}, Q_0 .. Q_{ch-1}; with the census
                                       // cost the code planes, [H][W] uint64 (the two costs exclude each other); null with the SAD cost
    unsigned *spk_label, *spk_size;    // the speckle filter's planes (SpkArgs below); null with the filter off
    uint8_t *maps;                     // the map buffer [2][H][W] k_sgm_maps writes: the context's (psm_sgm_select_maps, _batch)
};
// one pixel of a staged image as a dword of `ch` bytes (depth 0: bytes, PSM_IMG_U8); float images are quantised as lFrame.convertTo(lFrame, CV_8U, 255) does
// (src/StereoMatch.cpp:174-177): saturate(rint(f * 255.0f)), ties to even
__device__ __forceinline__ unsigned sgm_px(const void *img, int depth, int ch, size_t idx)
{
    unsigned v = 0;
    for (int k = 0; k < ch; ++k) {
        unsigned b;
        if (depth == 0) b = ((const uint8_t *)img)[idx * ch + k];
        else b = (unsigned)fminf(fmaxf(rintf(__fmul_rn(((const float *)img)[idx * ch + k], 255.0f)), 0.0f), 255.0f);
        v |= b << (8 * k);
    }
    return v;
}
constexpr int SGM_DIRS[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};   // (dy, dx)
// the directions a mode sums (psm_sgm_set_mode; the values are OpenCV's enum): the first SGM_MODE_NDIR[mode] entries of its row, as
// indices into SGM_DIRS, launched in this order - the first one stores S.  Every reduced mode begins with the two row directions.
constexpr int SGM_MODE_NDIR[4] = {5, 8, 3, 4};
constexpr int SGM_MODE_DIRS[4][8] = {{0, 1, 2, 4, 5}, {0, 1, 2, 3, 4, 5, 6, 7}, {0, 1, 2}, {0, 1, 2, 3}};   // SGBM, HH, SGBM_3WAY, HH4
// The widest range (psm_sgm_set_range).  Up to 256 disparities a pixel's Dp is D rounded up to 4 elements, as ever; above, to the
// 8 or 16 disparities a lane of k_sgm_path holds, so that a lane's vector is whole and 16-byte aligned in both volumes.
constexpr int SGM_DMAX = 1024;
inline int sgm_dp(int D) { return D <= 256 ? (D + 3) & ~3 : (D <= 512 ? (D + 7) & ~7 : (D + 15) & ~15); }
// bits of the disparity index below S in the packed minima of k_sgm_select: 8 as ever up to Dp 256, 10 above (S < 2^19: 29 bits)
__host__ __device__ inline int sgm_kb(int Dp) { return Dp > 256 ? 10 : 8; }
constexpr int SGM_BT_TX = 128;         // k_sgm_bt_rows: output pixels of a row per workgroup
constexpr int SGM_BT_YS = 32;          // k_sgm_bt_cols: output rows per thread
constexpr int SGM_CEN_TX = 32;         // k_sgm_census: the pixels of a workgroup's tile, columns ...
constexpr int SGM_CEN_TY = 8;          // ... and rows
constexpr int SGM_CEN_MAXW = 9;        // the widest census window (psm_sgm_set_census): 9 x 7 - 1 = 62 bits
constexpr int SGM_CEN_MAXH = 7;
// q: the pair of a single call, or the n pairs of a batch's device table (grid z = pair)
void launch_sgm_cost(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q);
void launch_sgm_cost_bt(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q);       // k_sgm_prefilter, k_sgm_bt_rows, k_sgm_bt_cols: the same C
void launch_sgm_cost_census(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q);   // k_sgm_census, k_sgm_census_cost: the same C
void launch_sgm_path(hipStream_t s, const SgmArgs &a, int dy, int dx, bool first, const Recs<SgmPair> &q);   // S = L_r (first) or S += L_r
void launch_sgm_select(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q);        // k_sgm_select + k_sgm_check (disp2 all ones before)
void launch_sgm_fill_batch(hipStream_t s, const SgmArgs &a, const SgmPair *tab, int n);   // disp2 of every pair all ones
// k_sgm_maps: the 8-bit maps of both views from S into every pair's `maps` [2][H][W]; of `a` it reads W, H, D, Dp and dmin >= 0,
// D <= 256.  One workgroup per row with sgm_maps_lds_bytes(W) of dynamic LDS, which must not exceed
// SGM_MAPS_LDS_MAX.
constexpr size_t SGM_MAPS_LDS_MAX = 65536;
size_t sgm_maps_lds_bytes(int W);
void launch_sgm_maps(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q);

// psm_speckle.hip: cv::filterSpeckles on an int16 map, in place (psm_sgm_set_speckle, psm_sgm_filter_speckles).  The planes are an
// SgmPair's: out, the map [H][W], filtered in place; spk_label [H][W], union-find parents - a pixel index of the same component, <=
// the pixel's own; all ones: a new_val pixel; spk_size [H][W], run lengths at run heads, then component sizes at roots, in the end
// every pixel's component size
struct SpkArgs {
    int W, H;
    int new_val, max_size, max_diff;   // max_diff <= 65535
};
// k_spk_runs, k_spk_merge, k_spk_count, k_spk_apply; q: as above
void launch_speckle(hipStream_t s, const SpkArgs &a, const Recs<SgmPair> &q);

// psm_score.hip: the display maps and the reference's error record of the current result (psm_score, psm_api_score.cpp)
// The counters of one pair, zeroed on the stream ahead of the launches.  mn / mx hold the int16 map's minimum - 32767 (<= 0) and
// maximum + 32768 (>= 0): zero is then the identity of both atomics, and one memset prepares all of it.
struct ScCnt {
    int mn, mx;
    unsigned bad, pad;
    unsigned long long sum;
};
constexpr int SC_MN_BIAS = 32767, SC_MX_BIAS = 32768;
enum { SC_GIF = 0, SC_SGM = 1, SC_SGM_INT = 2 };       // PSM_SCORE_* (include/primesm_hip.h)
// One pair's pointers: a single call's by value, an entry of a batch's device table (psm_score_batch; blockIdx.y = pair)
struct ScPair {
    const uint8_t *maps;               // SC_GIF: [2][H][W], the context's current maps
    const int16_t *d16;                // SC_SGM, SC_SGM_INT: [H][W], the map of the last compute
    const uint8_t *gt, *mask;          // [H][W] each; gt null: nothing is scored; mask null: step 5 of the metric is left out
    uint8_t *planes;                   // [3][H][W]: left display, right display (SC_GIF only), error plane
    ScCnt *cnt;
};
struct ScArgs {                        // the scalars of one call
    int W, H, D;
    int scale, thr;                    // scale_factor; error_threshold * unit: errors up to it count as none
    int disc;                          // PSM_MASK_DISC: mask values up to 254 count as 0
};
void launch_sc_minmax(hipStream_t s, const ScArgs &a, const Recs<ScPair> &q);   // k_sc_minmax: cnt->mn, cnt->mx of d16
void launch_sc_score(hipStream_t s, int source, const ScArgs &a, const Recs<ScPair> &q);   // k_sc_score<source>: planes, cnt->bad, cnt->sum

// psm_depth.hip: cv::reprojectImageTo3D of the current result and the compacted point cloud (psm_reproject, psm_api_depth.cpp)
enum { DP_GIF = 0, DP_SGM = 1 };                       // PSM_DEPTH_* (include/primesm_hip.h)
constexpr int DP_TILE = 256;                           // pixels (in raster order) of a workgroup: one count per tile
constexpr int DP_SCAN = 256;                           // threads of the scan's single workgroup; thread t takes ceil(tiles / DP_SCAN) consecutive tiles
__host__ __device__ inline int dp_tiles(int W, int H) { return (int)(((size_t)W * H + DP_TILE - 1) / DP_TILE); }
// One pair: its pointers and its own parameters.  A single call passes the record as the kernel argument; a batch's device table
// holds one per pair, indexed with the pair number (blockIdx.y).  What a batch shares travels in DpGeom.
struct DpArgs {
    const uint8_t *map;                // DP_GIF: [H][W], the left 8-bit map
    const uint8_t *valid;              // PSM_DEPTH_USE_MASK: [H][W], the left validity bytes; else null
    const int16_t *d16;                // DP_SGM: [H][W]
    const void *img;                   // the left image of the colour pair (k_dp_pack only)
    unsigned *xyz, *z;                 // [H][W][3], [H][W] float bit patterns; null: not asked for
    uint4 *cloud;                      // [H W] records; null: not asked for
    unsigned *tile_cnt, *tile_off;     // [dp_tiles]: kept pixels per tile, and their exclusive sums
    unsigned *total;                   // the count
    double Q[16];
    int crop_x, crop_y;
    float z_min, z_max;
    int invalid;                       // DP_SGM: the map's invalid value
    int depth, ch;                     // of img: PSM_IMG_*, 3 or 1 channels
};
struct DpGeom { int W, H, source; };
void launch_dp_count(hipStream_t s, const DpGeom &g, const Recs<DpArgs> &q);   // k_dp_count: dense planes, tile_cnt
void launch_dp_scan(hipStream_t s, const DpGeom &g, const Recs<DpArgs> &q);    // k_dp_scan: tile_off, total
void launch_dp_pack(hipStream_t s, const DpGeom &g, const Recs<DpArgs> &q);    // k_dp_pack: cloud

// psm_wls.hip: edge-aware WLS smoothing of an int16 map in 16ths, Min et al.'s Fast Global Smoother (psm_wls_filter, psm_api_wls.cpp)
enum { WLS_GIF = 0, WLS_SGM = 1 };                     // PSM_WLS_* (include/primesm_hip.h)
constexpr int WLS_LINES = 64;                          // lines of a wave: one lane owns one line and walks it
constexpr int WLS_STEPS = 64;                          // row pass: the steps of a tile that travels through LDS
constexpr int WLS_PITCH = WLS_STEPS + 1;               // ... dwords between the lines of a tile in LDS: the transposed ds_read_b32 / ds_write_b32
                                                       //     of a 32-lane half then touch 32 different banks ((a / 4) mod 32)
constexpr int WLS_ROW_THREADS = 256;                   // ... threads of a workgroup: four waves move the tile, the first one walks it
constexpr int WLS_CHUNK = 8;                           // steps whose loads - global in the column pass, LDS in the row pass - are issued ahead of the chain
constexpr int WLS_TILE = 256;                          // k_wls_init: pixels (in raster order) of a workgroup
constexpr unsigned WLS_VOID = 0x7FC00000u;             // what a void pixel holds in the float plane: stored, never computed
struct WlsArgs {
    const uint8_t *map;                // WLS_GIF: [H][W], the left 8-bit map
    const uint8_t *valid;              // PSM_WLS_USE_MASK: [H][W], the left validity bytes; else null
    const int16_t *d16;                // WLS_SGM: [H][W]
    const void *img;                   // the guide: the left image of the colour pair
    float *num, *den;                  // [H][W] each: the working planes
    float *cp, *np, *dp;               // [H][W] each: what the forward sweep of a pass leaves for its back sweep
    uint8_t *kh, *kv;                  // [H][W] each: the link indices to the right and downwards
    const float *tab;                  // [256]: exp(-k / sigma)
    int16_t *out;                      // [H][W]: the filtered map
    unsigned *q;                       // [H][W]: the quotient's bit patterns
    int W, H, source;
    int invalid;                       // the invalid value of the source map, and of the result
    int depth, ch;                     // of img: PSM_IMG_*, 3 or 1 channels
    const uint8_t *conf;               // PSM_WLS_CONFIDENCE: [H][W], the confidence bytes k_wls_conf wrote - num = conf * v, den = conf; else null
};
// PSM_WLS_CONFIDENCE (tests/wls_conf_model.py): what the two launches ahead of k_wls_init read of a member - its own terms and
// parameters, and, with the L-R term, the S of its SGM result with the range that result has.  terms 0: the call has no flag.
enum { WLS_CONF_LR = 1, WLS_CONF_VAR = 2 };            // PSM_WLS_CONF_* (include/primesm_hip.h)
constexpr int WLS_CONF_RMAX = 4;                       // the widest radius of the variance window
constexpr int WLS_CONF_TX = 64, WLS_CONF_TY = 4;       // k_wls_conf: the pixels of a workgroup's tile - a wave per row, the lane as x: every LDS
                                                       // instruction of a wave reads 64 consecutive dwords, whatever the pitch
constexpr int WLS_R16_WAVES = 8;                       // k_sgm_right16: waves of a row's workgroup
constexpr size_t WLS_R16_LDS_MAX = 65536;              // ... whose W keys of 4 bytes must fit
struct WlsConf {
    const uint32_t *S;                 // [H][W][Dp]: the summed path costs of the member's SGM result (L-R term only)
    int16_t *r16;                      // [H][W]: the right view's map in 16ths, k_sgm_right16's
    uint8_t *conf;                     // [H][W]: the confidence bytes, k_wls_conf's
    int terms, thresh, radius, shift;
    int D, Dp, dmin;                   // of S
};
__host__ __device__ inline int wls_groups(int lines) { return (lines + WLS_LINES - 1) / WLS_LINES; }
// One call's record - psm_wls_filter's, or a member's of a batch (psm_wls_filter_batch) - and the lambdas of its passes: lambda and
// sigma are the member's own, the number of passes is the batch's.  A single call passes it by value; a batch's device table holds
// one per member, indexed with the member number (blockIdx.y).  W and H are the same in all records of a call.
struct WlsPair {
    WlsArgs a;
    float lam[WLS_MAX_ITERS];          // wls_lambda(lambda, T, t), t < T; the rest 0
    WlsConf c;                         // PSM_WLS_CONFIDENCE; else zeros
};
// k_sgm_right16: r16 of every member with the L-R term (the others' workgroups return at once); one workgroup per image row with
// 4 W bytes of dynamic LDS (<= WLS_R16_LDS_MAX); dp_max: the largest Dp among those members (the per-lane count of the launch)
void launch_sgm_right16(hipStream_t s, const Recs<WlsPair> &q, int dp_max);
void launch_wls_conf(hipStream_t s, const Recs<WlsPair> &q);                   // k_wls_conf: conf from the source map and r16
void launch_wls_init(hipStream_t s, const Recs<WlsPair> &q);                   // k_wls_init: num, den, kh, kv; a.conf of q.host[0] non-null: the weighted start
void launch_wls_rows(hipStream_t s, const Recs<WlsPair> &q, int t);            // k_wls_rows: pass t over every row
void launch_wls_cols(hipStream_t s, const Recs<WlsPair> &q, int t, bool last);   // k_wls_cols: ... every column; last: and the quotient, out and q

// psm_gray.hip: the one-channel guided filter over a one-channel pair (psm_gray_compute, psm_api_gray.cpp)
constexpr int GRAY_COLS = 56;                          // output columns of a wave's strip
constexpr int GRAY_DC_MAX = 32;                        // slices of a chunk at most
constexpr size_t GRAY_SCRATCH_MAX = (size_t)1 << 30;   // bytes of the chunk scratch at most (but four slices always fit)
struct GrayPair {                                      // one pair's buffers: a single call's by value, an entry of a batch's device table (psm_gray_compute_batch)
    const void *raw[2];                // the pair's planes [H][W]: bytes (PSM_IMG_U8) or floats (PSM_IMG_F32)
    float2 *ig[2];                     // [H][W] {I, G}: the plane and its x-gradient
    float2 *mv[2];                     // [H][W] {mI, 1 / (var + eps)}
    float2 *ab;                        // the chunk scratch [2][dc][H][W] {a, b}
    long long *keys;                   // [2][H][W] packed minima of this stage (not the colour path's)
    uint8_t *maps;                     // [2][H][W]: the context's map buffer (k_gray_merge)
    // psm_gray_compute_fgf (psm_gray_fgf.hip) alone; hs = H / s, ws = W / s
    float4 *fsm[2];                    // [hs][ws] {Is, mI, den, 0}: the subsampled guidance
    float2 *fab;                       // the chunk scratch [2][dc][hs][ws] {a, b}
    float2 *fmab;                      // ... and [2][dc][hs][ws] {blur(a), blur(b)}
};
struct GrayPlan { int nstrips, nsegs, seg_rows, dc; };   // strips of GRAY_COLS columns, segments of seg_rows rows, slices per chunk
// for the device the calling thread is bound to (pc_dev); n: the pairs that share every launch - seg_rows alone depends on it
GrayPlan gray_plan(int W, int H, int D, int n = 1);
// q: the pair of a single call, or the n pairs of a batch's device table (grid z = pair; k_gray_ab, k_gray_q: pair * 2 + side)
void launch_gray_prep(hipStream_t s, const Recs<GrayPair> &q, const GrayPlan &g, int W, int H, bool f32);   // k_gray_prep: ig, mv of both sides; keys = no candidate
// k_gray_ab, k_gray_q over the slices [dbeg, dend) (at most g.dc) of both sides of every pair: {a, b} into each pair's ab, minima into its keys
void launch_gray_chunk(hipStream_t s, const Recs<GrayPair> &q, const GrayPlan &g, int W, int H, int dbeg, int dend);
// ... the storing form (the test hooks'), one side of one pair by value: q into qvol [dend - dbeg][H][W]; {a, b} of the slices are in p.ab
void launch_gray_chunk_store(hipStream_t s, const GrayPair &p, const GrayPlan &g, int W, int H, int side, int dbeg, int dend, float *qvol);
void launch_gray_merge(hipStream_t s, const Recs<GrayPair> &q, int W, int H);   // k_gray_merge: keys -> maps of every pair

// psm_gray_fgf.hip: FastGuidedFilterMono over a one-channel pair (psm_gray_compute_fgf, psm_api_gray.cpp)
struct GrayFgfPlan { int sub, k, ws, hs, nstrips, nsegs, seg, dc; };   // rate, taps, subsampled size; strips of 64 - 2 (k / 2) columns, segments of seg rows, slices per chunk
// n: the pairs that share every launch - seg alone depends on it (and on D)
GrayFgfPlan gray_fgf_plan(int W, int H, int D, int sub, int n = 1);
// k_grayf_prep: ig and fsm of both sides of every pair; keys = no candidate
void launch_grayf_prep(hipStream_t s, const Recs<GrayPair> &q, const GrayFgfPlan &g, int W, int H, bool f32);
// k_grayf_model, k_grayf_smooth, k_grayf_apply over the slices [dbeg, dend) (at most g.dc) of both sides of every pair: minima into its keys
void launch_grayf_chunk(hipStream_t s, const Recs<GrayPair> &q, const GrayFgfPlan &g, int W, int H, int dbeg, int dend);
// ... the storing form (the test hooks'), one side of one pair by value: q into qvol [dend - dbeg][H][W]; the model planes of the slices are in p.fab, p.fmab
void launch_grayf_chunk_store(hipStream_t s, const GrayPair &p, const GrayFgfPlan &g, int W, int H, int side, int dbeg, int dend, float *qvol);

}  // namespace psm
