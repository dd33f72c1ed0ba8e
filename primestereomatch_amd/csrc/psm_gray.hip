// psm_gray.hip - the one-channel guided filter of psm_gray_compute (psm_api_gray.cpp): GuidedFilter_cv (src/CVF.cpp:72-165) read for
// a one-channel guide, in the structure of FastGuidedFilterMono (src/fastguidedfilter.cpp:89-119), over costs that are myCostGrd
// (src/CVC.cpp:18-39) with the colour sum over one channel.  The definition is tests/gray_model.py; every kernel here evaluates it
// bit for bit (fp32 operations rounded one by one, IEEE division, the box filter in the tree order of psm_dev.h).
//   k_gray_prep   one launch per call: {I, G} and {mI, 1 / (var + eps)} of both sides, and the key plane's "no candidate yet"
//   k_gray_ab     a chunk of slices of one or both sides: costs on the fly from {I, G}, box(p), box(I p) -> {a, b} into the chunk
//                 scratch [side][slice of the chunk][H][W]
//   k_gray_q      the same chunk: box(a), box(b) -> q = box(b) + box(a) I -> the packed minimum of the wave's NS slices into the
//                 key plane (64-bit atomic minimum behind a plain read of the plane: a stale key only costs a redundant atomic), or -
//                 STORE, the test hooks' instantiation of the same body - q itself into a chunk of floats
//   k_gray_merge  the key planes -> the 8-bit maps
// Every kernel is one template over the record source S (psm_kernels.h): the GrayPair of psm_gray_compute by value, or the device
// table of the members of a psm_gray_compute_batch, the pair on grid z (k_gray_merge: y).  The index is uniform per workgroup, so
// the record's pointers arrive by scalar loads ahead of a body that is the same in both.
// No volume exists in memory: the scratch holds one chunk, GRAY_DC_MAX slices at most whatever D is.
// One wave marches a strip of GRAY_COLS output columns down a segment of rows, as the kernels of psm_kernels.hip do: lane l holds the
// input column r101(x0 - 4 + l), hsum8 leaves the window sum of output column x0 + l in lane l < 56, and a sliding vertical tree
// (vstep) turns the row sums of the rows y - 4 .. y + 3 into output row y; a segment costs 7 rows of run-in.  A wave carries NS
// slices side by side, so the side's own {I, G} row, the guidance and the indices are loaded and formed once for all of them, and -
// k_gray_q - one atomic stands for NS slices.
#include "psm_kernels.h"
#include "psm_dev.h"

#include <algorithm>

namespace psm {

namespace {

// slices a wave carries.  The kernels are bound by their instruction count, not by occupancy: at 1080p x 256 with chunks of 8 slices
// and segments of 48 rows one slice per wave (92 VGPRs, five waves per SIMD) took 12.4 ms and two (142, three waves) 9.0 ms; with
// chunks of 32 and segments of 64 rows two slices in k_gray_ab took 7.5 ms and four (228, two waves) 6.6 ms - what a wave shares
// between its slices (rows, indices, guidance, the atomic) is that much of a step
constexpr int GRAY_NS = 4;

struct GrayPos {
    int lane, x0, cs, xo, xoc, y0, y1, n, ybase;
    bool ovalid;
};
__device__ __forceinline__ GrayPos gray_pos(int W, int H, int nstrips, int seg_rows)
{
    GrayPos p;
    const int strip = blockIdx.x % nstrips, seg = blockIdx.x / nstrips;
    p.lane = threadIdx.x & 63;
    p.x0 = strip * GRAY_COLS;
    p.cs = r101c(p.x0 - 4 + p.lane, W);
    p.xo = p.x0 + p.lane;
    p.xoc = min(p.xo, W - 1);
    p.ovalid = p.lane < GRAY_COLS && p.xo < W;
    p.y0 = seg * seg_rows;
    p.y1 = min(H, p.y0 + seg_rows);
    p.n = (p.y1 - p.y0) + 7;                           // steps: step s feeds image row ybase + s and leaves output row ybase + s - 3
    p.ybase = p.y0 - 4;
    return p;
}
#define PSM_GRAY_LANE_IDX()                            \
    const int i1 = ((pos.lane + 1) & 63) << 2;         \
    const int i2 = ((pos.lane + 2) & 63) << 2;         \
    const int i4 = ((pos.lane + 4) & 63) << 2;         \
    (void)i1; (void)i2
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (The pointers of a record are read where they are used, each as a global pointer - sgm_global, psm_kernels.h - and with the side
// as the index into the record itself: a copy of the record indexed by the side would be an array in private memory.)
// grid z of k_gray_ab / k_gray_q: pair * 2 + side of a launch over both sides; the one workgroup layer of a launch over one side
// (the storing form: a single pair) is z = 0, the side side0
__device__ __forceinline__ int gray_z_side(int side0) { return side0 + (blockIdx.z & 1); }
__device__ __forceinline__ unsigned gray_z_pair() { return blockIdx.z >> 1; }

// ---- guidance ---------------------------------------------------------------------------------
template <bool F32>
__device__ __forceinline__ float gray_px(const void *raw, size_t idx)
{   // PSM_IMG_U8: (float)u8 * (1 / 255.0f), as psm_upload_pair converts (src/StereoMatch.cpp:195-196); PSM_IMG_F32: as it is
    if (F32) return ((const float *)raw)[idx];
    return __fmul_rn((float)((const uint8_t *)raw)[idx], 1 / 255.0f);
}

struct GrayPrepSide {                  // one side of a pair as k_gray_prep finds it
    const void *raw;
    float2 *ig, *mv;
    long long *keys;                   // the side's [H][W]
};

template <bool F32, int K>
__device__ __forceinline__ void gray_prep_step(const GrayPrepSide &p, const GrayPos &pos, int W, int H, int i, VTree &t0, VTree &t1, int i1, int i2,
                                               int i4, int im1)
{
    const int step = i + K;
    const float I = gray_px<F32>(p.raw, (size_t)r101c(pos.ybase + step, H) * W + pos.cs);
    // G = I(x + 1) - I(x - 1) with REFLECT_101: the lanes l + 1 / l - 1 hold exactly those columns
    const float G = __fsub_rn(rol1(I), lane_get(I, im1));
    const int xi = pos.x0 - 4 + pos.lane;
    if (step >= 4 && step < pos.n - 3 && pos.lane >= 4 && pos.lane < 4 + GRAY_COLS && xi < W)
        p.ig[(size_t)(pos.ybase + step) * W + xi] = make_float2(I, G);
    const float mI = box_out(vstep<K>(t0, hsum8(I, i1, i2, i4)));
    const float mII = box_out(vstep<K>(t1, hsum8(__fmul_rn(I, I), i1, i2, i4)));
    const float var = __fsub_rn(mII, __fmul_rn(mI, mI));
    const float inv = __fdiv_rn(1.0f, __fadd_rn(var, 0.0001f));      // GIF_EPS, include/ComFunc.h:50; the 1 x 1 case of src/CVF.cpp:120-132
    if (step >= 7 && step < pos.n && pos.ovalid) {
        const size_t o = (size_t)(pos.ybase + step - 3) * W + pos.xo;
        p.mv[o] = make_float2(mI, inv);
        p.keys[o] = pack_key_f32(__builtin_inff(), 0);      // no candidate: (+inf, 0), oracle.wta's start
    }
}

template <typename S, bool F32>
__global__ __launch_bounds__(64) void k_gray_prep(S src, int W, int H, int nstrips, int seg_rows)
{
    const GrayPair &pr = rec(src, blockIdx.z);
    const int side = blockIdx.y;
    const GrayPrepSide p = {sgm_global(pr.raw[side]), sgm_global(pr.ig[side]), sgm_global(pr.mv[side]), sgm_global(pr.keys) + (size_t)side * H * W};
    const GrayPos pos = gray_pos(W, H, nstrips, seg_rows);
    PSM_GRAY_LANE_IDX();
    const int im1 = ((pos.lane + 63) & 63) << 2;
    VTree t0 = {}, t1 = {};
    for (int i = 0; i < pos.n; i += 4) {
        gray_prep_step<F32, 0>(p, pos, W, H, i, t0, t1, i1, i2, i4, im1);
        gray_prep_step<F32, 1>(p, pos, W, H, i, t0, t1, i1, i2, i4, im1);
        gray_prep_step<F32, 2>(p, pos, W, H, i, t0, t1, i1, i2, i4, im1);
        gray_prep_step<F32, 3>(p, pos, W, H, i, t0, t1, i1, i2, i4, im1);
    }
}

// ---- p -> {a, b} -------------------------------------------------------------------------------
// The slices a wave carries: slot cz0 + s of the chunk is the disparity dbeg + cz0 + s; beyond dend the slot is dead (computed on
// the last live disparity, never stored).
template <int NS> struct GrayAbIn {
    float2 ig[4], mv[4], og[NS][4];
};

template <int NS, int K>
__device__ __forceinline__ void gray_ab_step(const GrayAbIn<NS> &in, const GrayPos &pos, int W, int i, VTree (&t)[NS][2], const bool (&border)[NS], bool anyb,
                                             const bool (&live)[NS], float2 *const (&out)[NS], int i1, int i2, int i4)
{
    const int step = i + K;
    const float I = in.ig[K].x, G = in.ig[K].y;
    const float w1 = __fsub_rn(1.0f, 0.9f);
    // myCostGrd(lC, lG), src/CVC.cpp:30-39: BC_32F is the double 1.0
    float cb = 0.0f;
    if (anyb) cb = __fadd_rn(__fmul_rn(0.9f, (float)fabs(__dsub_rn((double)I, 1.0))), __fmul_rn(w1, (float)fabs(__dsub_rn((double)G, 1.0))));
    const float mI = in.mv[K].x, inv = in.mv[K].y;
    const bool st = step >= 7 && step < pos.n && pos.ovalid;
    const unsigned o = (unsigned)(pos.ybase + step - 3) * (unsigned)W + (unsigned)pos.xo;      // (used under st alone)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        // myCostGrd(lC, rC, lG, rG), src/CVC.cpp:18-27, one channel
        const float ci = __fadd_rn(__fmul_rn(0.9f, fabsf(__fsub_rn(I, in.og[s][K].x))), __fmul_rn(w1, fabsf(__fsub_rn(G, in.og[s][K].y))));
        const float c = border[s] ? cb : ci;
        const float mp = box_out(vstep<K>(t[s][0], hsum8(c, i1, i2, i4)));
        const float mIp = box_out(vstep<K>(t[s][1], hsum8(__fmul_rn(I, c), i1, i2, i4)));
        const float cov = __fsub_rn(mIp, __fmul_rn(mI, mp));
        const float a = __fmul_rn(inv, cov);
        const float b = __fsub_rn(mp, __fmul_rn(a, mI));
        if (st && live[s]) out[s][o] = make_float2(a, b);
    }
}

template <typename S, int NS>
__global__ __launch_bounds__(64) void k_gray_ab(S src, int W, int H, int nstrips, int seg_rows, int side0, int dbeg, int dend, int dc)
{
    const GrayPair &p = rec(src, gray_z_pair());
    const int side = gray_z_side(side0);
    const GrayPos pos = gray_pos(W, H, nstrips, seg_rows);
    PSM_GRAY_LANE_IDX();
    const size_t HW = (size_t)H * W;
    const float2 *__restrict__ IG = sgm_global(p.ig[side]), *__restrict__ OG = sgm_global(p.ig[side ^ 1]), *__restrict__ MV = sgm_global(p.mv[side]);
    float2 *const AB = sgm_global(p.ab);
    bool border[NS], live[NS];
    int pc[NS];
    float2 *out[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int cz = blockIdx.y * NS + s;
        live[s] = dbeg + cz < dend;
        const int d = live[s] ? dbeg + cz : dend - 1;
        // left volume: the partner is x - d in the right image, border x < d; right volume: x + d in the left image, border
        // x >= W - d (src/CVC.cpp:122-179 with the swapped arguments)
        const int xp = side ? pos.cs + d : pos.cs - d;
        border[s] = side ? xp >= W : xp < 0;
        pc[s] = clampi(xp, 0, W - 1);
        out[s] = AB + ((size_t)side * dc + min(cz, dc - 1)) * HW;
    }
    // no lane of most waves sees a border column: the border cost (two double differences) is formed only where one does
    bool anyl = false;
#pragma unroll
    for (int s = 0; s < NS; ++s) anyl = anyl || border[s];
    const bool anyb = __any(anyl) != 0;
    VTree t[NS][2] = {};
    GrayAbIn<NS> nx;
    auto issue = [&](GrayAbIn<NS> &r, int i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // (32-bit element offsets: W H < 2^27, psm_create - a scalar base and one VGPR offset per load)
            const unsigned row = (unsigned)r101c(pos.ybase + i + k, H) * (unsigned)W;
            r.ig[k] = IG[row + (unsigned)pos.cs];
#pragma unroll
            for (int s = 0; s < NS; ++s) r.og[s][k] = OG[row + (unsigned)pc[s]];
            r.mv[k] = MV[(unsigned)clampi(pos.ybase + i + k - 3, 0, H - 1) * (unsigned)W + (unsigned)pos.xoc];
        }
    };
    issue(nx, 0);
    for (int i = 0; i < pos.n; i += 4) {
        const GrayAbIn<NS> cu = nx;
        issue(nx, i + 4);      // the next four rows are in flight while these four compute
        gray_ab_step<NS, 0>(cu, pos, W, i, t, border, anyb, live, out, i1, i2, i4);
        gray_ab_step<NS, 1>(cu, pos, W, i, t, border, anyb, live, out, i1, i2, i4);
        gray_ab_step<NS, 2>(cu, pos, W, i, t, border, anyb, live, out, i1, i2, i4);
        gray_ab_step<NS, 3>(cu, pos, W, i, t, border, anyb, live, out, i1, i2, i4);
    }
}

// ---- {a, b} -> q -> keys ------------------------------------------------------------------------
template <int NS> struct GrayQIn {
    float I[4];
    float2 ab[NS][4];
};

template <int NS, bool STORE, int K>
__device__ __forceinline__ void gray_q_step(const GrayQIn<NS> &in, const GrayPos &pos, int W, int i, VTree (&t)[NS][2], const int (&d)[NS],
                                            const bool (&live)[NS], float *const (&qout)[NS], long long *keys, int i1, int i2, int i4)
{
    const int step = i + K;
    const bool st = step >= 7 && step < pos.n && pos.ovalid;
    const unsigned o = (unsigned)(pos.ybase + step - 3) * (unsigned)W + (unsigned)pos.xo;      // (used under st alone)
    float bq = __builtin_inff();
    int bd = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float ma = box_out(vstep<K>(t[s][0], hsum8(in.ab[s][K].x, i1, i2, i4)));
        const float mb = box_out(vstep<K>(t[s][1], hsum8(in.ab[s][K].y, i1, i2, i4)));
        const float q = __fadd_rn(mb, __fmul_rn(ma, in.I[K]));      // src/CVF.cpp:157-163, one channel
        if (STORE) {
            if (st && live[s]) qout[s][o] = q;
        } else {
            // d = 0 is never a candidate (src/DispSel.cpp:96); ascending slots, strict <: the lower disparity keeps an exact tie.
            // The wave's slices meet as floats, not as keys: a NaN q fails the compare whatever its sign, so it never wins - as a
            // key, a NaN with the sign bit set (an input 0xFFC00000 carried through, or the device's own 0 * inf) sorts below
            // every finite cost.  What reaches the key plane is never a NaN: (+inf, 0) where no slice was a candidate.
            // (Two selects, no branch: && here became a scalar branch per slice and cost 4 % of the call.)
            const bool take = (q < bq) & live[s] & (d[s] > 0);
            bq = take ? q : bq;
            bd = take ? d[s] : bd;
        }
    }
    if (!STORE && st) {
        const long long best = pack_key_f32(bq, bd);      // across waves and chunks the key's low word lets the lower d win a tie
        if (best < keys[o]) (void)__hip_atomic_fetch_min(keys + o, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <typename S, int NS, bool STORE>
__global__ __launch_bounds__(64) void k_gray_q(S src, float *qvol, int W, int H, int nstrips, int seg_rows, int side0, int dbeg, int dend, int dc)
{
    const GrayPair &p = rec(src, gray_z_pair());
    const int side = gray_z_side(side0);
    const GrayPos pos = gray_pos(W, H, nstrips, seg_rows);
    PSM_GRAY_LANE_IDX();
    const size_t HW = (size_t)H * W;
    const float2 *__restrict__ IG = sgm_global(p.ig[side]);
    const float2 *const AB = sgm_global(p.ab);
    long long *const keys = sgm_global(p.keys) + (size_t)side * HW;
    bool live[NS];
    int d[NS];
    const float2 *ab[NS];
    float *qout[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int cz = blockIdx.y * NS + s, czc = min(cz, dc - 1);
        live[s] = dbeg + cz < dend;
        d[s] = dbeg + cz;
        ab[s] = AB + ((size_t)side * dc + czc) * HW;
        qout[s] = STORE ? qvol + (size_t)czc * HW : nullptr;      // (the storing form runs one side per launch)
    }
    VTree t[NS][2] = {};
    GrayQIn<NS> nx;
    auto issue = [&](GrayQIn<NS> &r, int i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned row = (unsigned)r101c(pos.ybase + i + k, H) * (unsigned)W;
#pragma unroll
            for (int s = 0; s < NS; ++s) r.ab[s][k] = ab[s][row + (unsigned)pos.cs];
            r.I[k] = IG[(unsigned)clampi(pos.ybase + i + k - 3, 0, H - 1) * (unsigned)W + (unsigned)pos.xoc].x;
        }
    };
    issue(nx, 0);
    for (int i = 0; i < pos.n; i += 4) {
        const GrayQIn<NS> cu = nx;
        issue(nx, i + 4);
        gray_q_step<NS, STORE, 0>(cu, pos, W, i, t, d, live, qout, keys, i1, i2, i4);
        gray_q_step<NS, STORE, 1>(cu, pos, W, i, t, d, live, qout, keys, i1, i2, i4);
        gray_q_step<NS, STORE, 2>(cu, pos, W, i, t, d, live, qout, keys, i1, i2, i4);
        gray_q_step<NS, STORE, 3>(cu, pos, W, i, t, d, live, qout, keys, i1, i2, i4);
    }
}

// ---- keys -> maps: both sides of every pair, the pair on grid y ----------------------------------
template <typename S>
__global__ __launch_bounds__(256) void k_gray_merge(S src, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GrayPair &p = rec(src, blockIdx.y);
    sgm_global(p.maps)[i] = (uint8_t)((unsigned long long)sgm_global(p.keys)[i] & 0xffull);
}

using GrayVal = RecVal<GrayPair>;
using GrayTab = RecTab<GrayPair>;

}  // namespace

GrayPlan gray_plan(int W, int H, int D, int n)
{
    GrayPlan g;
    g.nstrips = (W + GRAY_COLS - 1) / GRAY_COLS;
    // the chunk: as many slices as keep both sides' {a, b} planes within GRAY_SCRATCH_MAX, a multiple of GRAY_NS, up to GRAY_DC_MAX
    // (the more slices a launch carries the less its tail weighs: 1080p x 256 took 9.0 ms with chunks of 8, 7.7 ms with 32)
    const size_t per_slice = 2 * (size_t)W * H * sizeof(float2);
    int dc = (int)std::min<size_t>(GRAY_SCRATCH_MAX / per_slice, (size_t)GRAY_DC_MAX);
    dc = std::max(GRAY_NS, dc - dc % GRAY_NS);
    g.dc = dc;
    // Rows per segment.  A segment costs 7 rows of run-in, a launch runs its waves in rounds of as many as the device holds (two
    // per SIMD at these kernels' 210 to 230 VGPRs), and a wave takes seg_rows + 7 steps: the segment length with the least
    // rounds x steps for a full chunk, the longer one on a tie.  Measured at 1080p x 256 (35 strips, 8 groups of 4 slices, 2 sides):
    // 64 rows 6.6 ms, 128 rows 7.3 ms; at 450 x 375 x 64: 16 rows 0.223, 32 rows 0.205, 64 rows 0.238 ms - the order this gives.
    // The n pairs of a batch share the launch: its waves are those of all of them.
    const PcDev dev = pc_dev();
    const long long slots = std::max(1, 2 * 4 * dev.nxcd * dev.cus_per_xcd);
    const int groups = (std::max(1, std::min(dc, D - 1)) + GRAY_NS - 1) / GRAY_NS;
    static const int segs[] = {16, 24, 32, 48, 64, 96, 128};
    long long best = -1;
    for (int sr : segs) {
        const long long waves = (long long)g.nstrips * ((H + sr - 1) / sr) * 2 * groups * std::max(1, n);
        const long long cost = ((waves + slots - 1) / slots) * (sr + 7);
        if (best < 0 || cost <= best) { best = cost; g.seg_rows = sr; }
    }
    g.nsegs = (H + g.seg_rows - 1) / g.seg_rows;
    return g;
}

void launch_gray_prep(hipStream_t s, const Recs<GrayPair> &q, const GrayPlan &g, int W, int H, bool f32)
{
    // the guidance runs once per pair: short segments, so that its one launch fills the device
    const int seg_rows = 16, nsegs = (H + seg_rows - 1) / seg_rows;
    const dim3 grid(g.nstrips * nsegs, 2, q.n);
    if (f32) rec_launch(s, k_gray_prep<GrayVal, true>, k_gray_prep<GrayTab, true>, grid, dim3(64), 0, q, W, H, g.nstrips, seg_rows);
    else rec_launch(s, k_gray_prep<GrayVal, false>, k_gray_prep<GrayTab, false>, grid, dim3(64), 0, q, W, H, g.nstrips, seg_rows);
}

void launch_gray_chunk(hipStream_t s, const Recs<GrayPair> &q, const GrayPlan &g, int W, int H, int dbeg, int dend)
{
    const int groups = (dend - dbeg + GRAY_NS - 1) / GRAY_NS;
    const dim3 grid(g.nstrips * g.nsegs, groups, 2 * q.n);
    float *const none = nullptr;
    rec_launch(s, k_gray_ab<GrayVal, GRAY_NS>, k_gray_ab<GrayTab, GRAY_NS>, grid, dim3(64), 0, q, W, H, g.nstrips, g.seg_rows, 0, dbeg, dend, g.dc);
    rec_launch(s, k_gray_q<GrayVal, GRAY_NS, false>, k_gray_q<GrayTab, GRAY_NS, false>, grid, dim3(64), 0, q, none, W, H, g.nstrips, g.seg_rows, 0, dbeg,
               dend, g.dc);
}

void launch_gray_chunk_store(hipStream_t s, const GrayPair &p, const GrayPlan &g, int W, int H, int side, int dbeg, int dend, float *qvol)
{
    const int groups = (dend - dbeg + GRAY_NS - 1) / GRAY_NS;
    const dim3 grid(g.nstrips * g.nsegs, groups, 1);
    const GrayVal v{{p}};
    hipLaunchKernelGGL((k_gray_ab<GrayVal, GRAY_NS>), grid, dim3(64), 0, s, v, W, H, g.nstrips, g.seg_rows, side, dbeg, dend, g.dc);
    hipLaunchKernelGGL((k_gray_q<GrayVal, GRAY_NS, true>), grid, dim3(64), 0, s, v, qvol, W, H, g.nstrips, g.seg_rows, side, dbeg, dend, g.dc);
}

void launch_gray_merge(hipStream_t s, const Recs<GrayPair> &q, int W, int H)
{
    const int n = 2 * W * H;
    rec_launch(s, k_gray_merge<GrayVal>, k_gray_merge<GrayTab>, dim3((n + 255) / 256, q.n), dim3(256), 0, q, n);
}

}  // namespace psm
