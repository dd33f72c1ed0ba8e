// psm_gray_fgf.hip - FastGuidedFilterMono (src/fastguidedfilter.cpp:89-119) of psm_gray_compute_fgf (psm_api_gray.cpp): the guided
// filter of psm_gray.hip on planes subsampled by s (nearest neighbour), its box shrunk to k = 2 (8 / s) + 1 taps of cv::blur, the two
// smoothed model planes upsampled bilinearly before the linear model is applied at full resolution.  The definition is
// tests/gray_fgf_model.py; every kernel here evaluates it bit for bit (fp32 operations rounded one by one, IEEE division, the fp64
// tap sums of cv::blur in their order - blur4_march, psm_fgf_dev.h).
//   k_grayf_prep    one launch per call: {I, G} of both sides at full resolution and the key plane's "no candidate yet" (its first
//                   blocks), the subsampled guidance {Is, mI, den} of both sides by direct k x k windows (its last blocks)
//   k_grayf_model   a chunk of slices of one or both sides, small grid: the cost of the sampled pixel on the fly from {I, G} - no
//                   full-resolution cost exists -, blur(p), blur(Is p) -> {a, b} into the chunk scratch [side][slot][hs][ws].  The
//                   march carries four planes per lane: a wave carries two slices, (p_d, Is p_d, p_d+1, Is p_d+1)
//   k_grayf_smooth  the same chunk: blur(a), blur(b) of two slices per wave -> {mean_a, mean_b}
//   k_grayf_apply   full resolution, 4 pixels x RB rows per thread: bilinear weights and guidance in registers across the chunk's
//                   slices, q = up(mean_a) I + up(mean_b), a running strict-< minimum in the thread and one 64-bit atomic minimum
//                   per pixel and chunk into the gray key plane behind a plain read of it (k_gray_q's form), or - STORE, the test
//                   hooks' instantiation of the same body - q itself into a chunk of floats
// then k_gray_merge (psm_gray.hip).  Every kernel is one template over the record source S (psm_kernels.h), the pair on grid z
// (with the side: pair * 2 + side, as k_gray_ab has it).  The scratch holds one chunk, GRAY_DC_MAX slices at most whatever D is.
#include "psm_kernels.h"
#include "psm_dev.h"
#include "psm_fgf_dev.h"

#include <algorithm>

namespace psm {

namespace {

__device__ __forceinline__ int fz_side(int side0) { return side0 + (blockIdx.z & 1); }
__device__ __forceinline__ unsigned fz_pair() { return blockIdx.z >> 1; }

template <bool F32>
__device__ __forceinline__ float grayf_px(const void *raw, size_t idx)
{   // PSM_IMG_U8: (float)u8 * (1 / 255.0f), as psm_upload_pair converts; PSM_IMG_F32: as it is (k_gray_prep's reading)
    if (F32) return ((const float *)raw)[idx];
    return __fmul_rn((float)((const uint8_t *)raw)[idx], 1 / 255.0f);
}

// ---- prep ---------------------------------------------------------------------------------------
// blocks [0, nfull): one full-resolution pixel per thread; blocks [nfull, ..): one subsampled pixel per thread
template <typename S, bool F32, int K>
__global__ __launch_bounds__(256) void k_grayf_prep(S src, int W, int H, int ws, int hs, int nfull)
{
    const GrayPair &p = rec(src, blockIdx.z);
    const int side = blockIdx.y;
    const void *raw = sgm_global(p.raw[side]);
    if ((int)blockIdx.x < nfull) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= W * H) return;
        const int y = i / W, x = i - y * W;
        const size_t row = (size_t)y * W;
        const float I = grayf_px<F32>(raw, row + x);
        // G = I(x + 1) - I(x - 1) with REFLECT_101 (tests/gray_model.py: gradient)
        const float G = __fsub_rn(grayf_px<F32>(raw, row + r101c(x + 1, W)), grayf_px<F32>(raw, row + r101c(x - 1, W)));
        sgm_global(p.ig[side])[i] = make_float2(I, G);
        sgm_global(p.keys)[(size_t)side * H * W + i] = pack_key_f32(__builtin_inff(), 0);      // no candidate: (+inf, 0), oracle.wta's start
        return;
    }
    const int j = ((int)blockIdx.x - nfull) * 256 + threadIdx.x;
    if (j >= ws * hs) return;
    const int ys = j / ws, xs = j - ys * ws;
    constexpr int R = K / 2;
    int X[K];
#pragma unroll
    for (int i = 0; i < K; ++i) X[i] = nn_src(r101s(xs + i - R, ws), ws, W);
    double a1 = 0.0, a2 = 0.0;
    for (int jj = -R; jj <= R; ++jj) {
        const size_t row = (size_t)nn_src(r101s(ys + jj, hs), hs, H) * W;
        double h1 = 0.0, h2 = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float v = grayf_px<F32>(raw, row + X[i]);
            h1 = __dadd_rn(h1, (double)v);
            h2 = __dadd_rn(h2, (double)__fmul_rn(v, v));
        }
        a1 = __dadd_rn(a1, h1);
        a2 = __dadd_rn(a2, h2);
    }
    const double scale = 1.0 / (K * K);
    const float mI = (float)(a1 * scale), mII = (float)(a2 * scale);
    // var_I + eps, src/fastguidedfilter.cpp:104-105: the double eps is added to a CV_32F plane in float
    const float den = __fadd_rn(__fsub_rn(mII, __fmul_rn(mI, mI)), 0.0001f);
    const float Is = grayf_px<F32>(raw, (size_t)nn_src(ys, hs, H) * W + X[R]);
    sgm_global(p.fsm[side])[j] = make_float4(Is, mI, den, 0.f);
}

// ---- p -> {a, b} at the subsampled size -----------------------------------------------------------
// The two slices of a wave: the slots cz, cz + 1 of the chunk are the disparities dbeg + cz, + 1; beyond dend the second slot is
// dead (computed on the first one's disparity, never stored).
template <typename S, int K>
__global__ __launch_bounds__(64) void k_grayf_model(S src, int W, int H, int ws, int hs, int nstrips, int seg, int side0, int dbeg, int dend, int dc)
{
    __shared__ float4 lds[2 * 64];
    const GrayPair &p = rec(src, fz_pair());
    const int side = fz_side(side0);
    const int strip = blockIdx.x % nstrips, sgi = blockIdx.x / nstrips;
    const int ybeg = sgi * seg, yend = ybeg + seg < hs ? ybeg + seg : hs;
    const float2 *__restrict__ IG = sgm_global(p.ig[side]), *__restrict__ OG = sgm_global(p.ig[side ^ 1]);
    const float4 *__restrict__ SM = sgm_global(p.fsm[side]);
    const int cz = blockIdx.y * 2;
    const bool live1 = dbeg + cz + 1 < dend;
    const int d0 = dbeg + cz, d1 = live1 ? d0 + 1 : d0;
    const size_t n = (size_t)hs * ws;
    float2 *const out0 = sgm_global(p.fab) + ((size_t)side * dc + cz) * n, *const out1 = out0 + n;      // (dc is even: slot cz + 1 exists)
    constexpr int R = K / 2, OUTW = 64 - 2 * R;
    // the full-resolution column of this lane's subsampled column, fixed for the whole march, and its partners: left volume x - d
    // in the right image, border x < d; right volume x + d in the left image, border x >= W - d (src/CVC.cpp:122-179)
    const int X = nn_src(r101s(strip * OUTW - R + (int)threadIdx.x, ws), ws, W);
    const int xp0 = side ? X + d0 : X - d0, xp1 = side ? X + d1 : X - d1;
    const bool border0 = side ? xp0 >= W : xp0 < 0, border1 = side ? xp1 >= W : xp1 < 0;
    const int pc0 = min(max(xp0, 0), W - 1), pc1 = min(max(xp1, 0), W - 1);
    const float w1 = __fsub_rn(1.0f, 0.9f);
    auto load = [&](int ys, int) -> float4 {
        const unsigned row = (unsigned)nn_src(ys, hs, H) * (unsigned)W;      // (32-bit element offsets: W H < 2^27, psm_create)
        const float2 own = IG[row + (unsigned)X], o0 = OG[row + (unsigned)pc0], o1 = OG[row + (unsigned)pc1];
        const float I = own.x, G = own.y;
        // myCostGrd(lC, lG), src/CVC.cpp:30-39 (BC_32F is the double 1.0), and myCostGrd(lC, rC, lG, rG), src/CVC.cpp:18-27, one channel
        const float cb = __fadd_rn(__fmul_rn(0.9f, (float)fabs(__dsub_rn((double)I, 1.0))), __fmul_rn(w1, (float)fabs(__dsub_rn((double)G, 1.0))));
        const float c0 = border0 ? cb : __fadd_rn(__fmul_rn(0.9f, fabsf(__fsub_rn(I, o0.x))), __fmul_rn(w1, fabsf(__fsub_rn(G, o0.y))));
        const float c1 = border1 ? cb : __fadd_rn(__fmul_rn(0.9f, fabsf(__fsub_rn(I, o1.x))), __fmul_rn(w1, fabsf(__fsub_rn(G, o1.y))));
        return make_float4(c0, __fmul_rn(I, c0), c1, __fmul_rn(I, c1));
    };
    auto finish = [&](int y, int x, float4 mean) {
        const unsigned o = (unsigned)y * (unsigned)ws + (unsigned)x;
        const float4 g = SM[o];
        const float mI = g.y, den = g.z;
        // src/fastguidedfilter.cpp:110-112: a = cov_Ip / (var_I + eps), the per-voxel quotient; b = mean_p - a mean_I
        const float a0 = __fdiv_rn(__fsub_rn(mean.y, __fmul_rn(mI, mean.x)), den);
        out0[o] = make_float2(a0, __fsub_rn(mean.x, __fmul_rn(a0, mI)));
        if (live1) {
            const float a1 = __fdiv_rn(__fsub_rn(mean.w, __fmul_rn(mI, mean.z)), den);
            out1[o] = make_float2(a1, __fsub_rn(mean.z, __fmul_rn(a1, mI)));
        }
    };
    blur4_march<K>(ws, hs, strip, ybeg, yend, lds, load, finish);
}

// ---- {a, b} -> {blur(a), blur(b)} -----------------------------------------------------------------
template <typename S, int K>
__global__ __launch_bounds__(64) void k_grayf_smooth(S src, int ws, int hs, int nstrips, int seg, int side0, int dbeg, int dend, int dc)
{
    __shared__ float4 lds[2 * 64];
    const GrayPair &p = rec(src, fz_pair());
    const int side = fz_side(side0);
    const int strip = blockIdx.x % nstrips, sgi = blockIdx.x / nstrips;
    const int ybeg = sgi * seg, yend = ybeg + seg < hs ? ybeg + seg : hs;
    const int cz = blockIdx.y * 2;
    const bool live1 = dbeg + cz + 1 < dend;
    const size_t n = (size_t)hs * ws, base = ((size_t)side * dc + cz) * n;
    // a dead second slot repeats the first one's planes (its own hold whatever an earlier chunk left)
    const float2 *__restrict__ in0 = sgm_global(p.fab) + base, *__restrict__ in1 = live1 ? in0 + n : in0;
    float2 *const out0 = sgm_global(p.fmab) + base, *const out1 = out0 + n;
    auto load = [&](int ys, int xs) -> float4 {
        const unsigned o = (unsigned)ys * (unsigned)ws + (unsigned)xs;
        const float2 u = in0[o], v = in1[o];
        return make_float4(u.x, u.y, v.x, v.y);
    };
    auto finish = [&](int y, int x, float4 mean) {
        const unsigned o = (unsigned)y * (unsigned)ws + (unsigned)x;
        out0[o] = make_float2(mean.x, mean.y);
        if (live1) out1[o] = make_float2(mean.z, mean.w);
    };
    blur4_march<K>(ws, hs, strip, ybeg, yend, lds, load, finish);
}

// ---- upsample + linear model + selection ----------------------------------------------------------
// k_fgf_apply_wta's scheme (psm_fgf.hip) on two planes and for any W: the thread's four columns are clamped to the row for the
// loads and guarded for the stores.  Row blocks start at y = RB by - yshift; consecutive rows use the same pair of model rows or
// the next one (uniform over the block: sy advances by 0 or 1 per row and the new sy is the old sy1).
template <typename S, bool STORE, int RB>
__global__ __launch_bounds__(256) void k_grayf_apply(S src, float *qvol, int W, int H, int ws, int hs, int yshift, int side0, int dbeg, int dend, int dc)
{
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4, y0 = (int)blockIdx.y * RB - yshift;
    if (x0 >= W) return;
    const GrayPair &p = rec(src, fz_pair());
    const int side = fz_side(side0);
    const size_t HW = (size_t)H * W, n = (size_t)hs * ws;
    const float2 *__restrict__ IG = sgm_global(p.ig[side]);
    const float2 *__restrict__ MAB = sgm_global(p.fmab) + (size_t)side * dc * n;
    long long *const keys = sgm_global(p.keys) + (size_t)side * HW;
    unsigned oa[4], ob[4];      // the two model columns of each pixel
    float a0[4], a1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int ca;
        lin_src(min(x0 + j, W - 1), ws, W, ca, a1[j]);
        oa[j] = (unsigned)ca;
        ob[j] = (unsigned)(ca + 1 < ws ? ca + 1 : ws - 1);
        a0[j] = __fsub_rn(1.f, a1[j]);
    }
    float gI[RB][4];
    int sy[RB], sy1[RB];
    float b0[RB], b1[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        int y = y0 + r;
        y = y < 0 ? 0 : (y < H ? y : H - 1);      // rows outside the image are skipped below; clamped here to stay in range
#pragma unroll
        for (int j = 0; j < 4; ++j) gI[r][j] = IG[(unsigned)y * (unsigned)W + (unsigned)min(x0 + j, W - 1)].x;
        lin_src(y, hs, H, sy[r], b1[r]);
        sy1[r] = sy[r] + 1 < hs ? sy[r] + 1 : hs - 1;
        b0[r] = __fsub_rn(1.f, b1[r]);
    }
    float mc[RB][4];
    int md[RB][4];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) { mc[r][j] = __builtin_inff(); md[r][j] = 0; }
    auto lerp2 = [](float2 s0, float w0, float2 s1, float w1) -> float2 {      // S0 w0 + S1 w1 per component, fp32, no FMA
        return make_float2(__fadd_rn(__fmul_rn(s0.x, w0), __fmul_rn(s1.x, w1)), __fadd_rn(__fmul_rn(s0.y, w0), __fmul_rn(s1.y, w1)));
    };
    for (int d = dbeg; d < dend; ++d) {
        const float2 *__restrict__ mrow = MAB + (size_t)(d - dbeg) * n;
        auto hrow = [&](int row, float2 *U) {      // row pass of cv::resize INTER_LINEAR: S[sx] (1 - fx) + S[sx + 1] fx
            const unsigned ro = (unsigned)row * (unsigned)ws;
#pragma unroll
            for (int j = 0; j < 4; ++j) U[j] = lerp2(mrow[ro + oa[j]], a0[j], mrow[ro + ob[j]], a1[j]);
        };
        float2 Ua[4], Ub[4];
        hrow(sy[0], Ua);
        hrow(sy1[0], Ub);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if (r > 0 && sy[r] != sy[r - 1]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) Ua[j] = Ub[j];
                hrow(sy1[r], Ub);
            }
            const bool yin = y0 + r >= 0 && y0 + r < H;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 u = lerp2(Ua[j], b0[r], Ub[j], b1[r]);      // column pass
                const float q = __fadd_rn(__fmul_rn(u.x, gI[r][j]), u.y);      // src/fastguidedfilter.cpp:118: mean_a.mul(I) + mean_b
                if (STORE) {
                    if (yin && x0 + j < W) qvol[(size_t)(d - dbeg) * HW + (size_t)(y0 + r) * W + x0 + j] = q;
                } else if (q < mc[r][j]) {      // ascending d, strict <: the lower disparity keeps an exact tie; a NaN never wins
                    mc[r][j] = q; md[r][j] = d;
                }
            }
        }
    }
    if (STORE) return;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        if (y0 + r < 0 || y0 + r >= H) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= W) continue;
            const size_t o = (size_t)(y0 + r) * W + x0 + j;
            const long long key = pack_key_f32(mc[r][j], md[r][j]);
            if (key < keys[o]) (void)__hip_atomic_fetch_min(keys + o, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

using GrayVal = RecVal<GrayPair>;
using GrayTab = RecTab<GrayPair>;

}  // namespace

GrayFgfPlan gray_fgf_plan(int W, int H, int D, int sub, int n)
{
    GrayFgfPlan g;
    g.sub = sub;
    g.k = 2 * (8 / sub) + 1;
    g.ws = W / sub;
    g.hs = H / sub;
    const int outw = 64 - 2 * (g.k / 2);
    g.nstrips = (g.ws + outw - 1) / outw;
    // the chunk: as many slices as keep both sides' {a, b} and {blur(a), blur(b)} within GRAY_SCRATCH_MAX, an even count (a wave
    // carries two slices), up to GRAY_DC_MAX
    const size_t per_slice = 2 * 2 * (size_t)g.ws * g.hs * sizeof(float2);
    int dc = (int)std::min<size_t>(GRAY_SCRATCH_MAX / per_slice, (size_t)GRAY_DC_MAX);
    g.dc = std::max(2, dc - dc % 2);
    // rows per marching segment: enough workgroups to fill the device, at least 4 k rows each (a segment costs k - 1 rows of run-in)
    const int groups = (std::max(1, std::min(g.dc, D - 1)) + 1) / 2;
    const long long per_seg = (long long)g.nstrips * groups * 2 * std::max(1, n);
    const int want = (int)std::max<long long>(1, (4096 + per_seg - 1) / per_seg);
    g.seg = std::min(g.hs, std::max(4 * g.k, (g.hs + want - 1) / want));
    g.nsegs = (g.hs + g.seg - 1) / g.seg;
    return g;
}

void launch_grayf_prep(hipStream_t s, const Recs<GrayPair> &q, const GrayFgfPlan &g, int W, int H, bool f32)
{
    const int nfull = (W * H + 255) / 256, nsub = (g.ws * g.hs + 255) / 256;
    const dim3 grid(nfull + nsub, 2, q.n);
#define PSM_GRAYF_PREP(F, K) rec_launch(s, k_grayf_prep<GrayVal, F, K>, k_grayf_prep<GrayTab, F, K>, grid, dim3(256), 0, q, W, H, g.ws, g.hs, nfull)
    if (f32) {
        if (g.k == 3) PSM_GRAYF_PREP(true, 3); else if (g.k == 5) PSM_GRAYF_PREP(true, 5); else PSM_GRAYF_PREP(true, 9);
    } else {
        if (g.k == 3) PSM_GRAYF_PREP(false, 3); else if (g.k == 5) PSM_GRAYF_PREP(false, 5); else PSM_GRAYF_PREP(false, 9);
    }
#undef PSM_GRAYF_PREP
}

namespace {

// Rows per thread: four at s = 4 and 8, where the four rows of a block share one pair of model rows whenever H is a multiple of s
// (yshift puts the block on them), so a slice costs a thread two row passes for sixteen outputs; two at s = 2, where four rows
// would need three.  Measured at 1280 x 720 x 128 and 1920 x 1080 x 256 (ms per call, two | four rows): s = 4 0.650 | 0.601 and
// 1.82 | 1.61, s = 8 0.572 | 0.522 and 1.56 | 1.35 - although four rows hold 228 VGPRs (two waves per SIMD) against 130 (three).
// Requesting slice d + 1's model rows ahead of slice d's outputs, as k_fgf_apply4 does, changed nothing at two rows (0.652,
// 1.83; 162 VGPRs) and cost 6 to 27 % at four (260 VGPRs): the loads are not what the kernel waits for.
dim3 apply_grid(const GrayFgfPlan &g, int W, int H, int z, int &yshift, int &rb)
{
    rb = g.sub >= 4 ? 4 : 2;
    yshift = (g.sub / 2) % rb;
    return dim3(((W + 3) / 4 + 255) / 256, (H + yshift + rb - 1) / rb, z);
}

}  // namespace

void launch_grayf_chunk(hipStream_t s, const Recs<GrayPair> &q, const GrayFgfPlan &g, int W, int H, int dbeg, int dend)
{
    const dim3 gs(g.nstrips * g.nsegs, (dend - dbeg + 1) / 2, 2 * q.n);
#define PSM_GRAYF_K(K)                                                                                                                            \
    do {                                                                                                                                          \
        rec_launch(s, k_grayf_model<GrayVal, K>, k_grayf_model<GrayTab, K>, gs, dim3(64), 0, q, W, H, g.ws, g.hs, g.nstrips, g.seg, 0, dbeg, dend, g.dc); \
        rec_launch(s, k_grayf_smooth<GrayVal, K>, k_grayf_smooth<GrayTab, K>, gs, dim3(64), 0, q, g.ws, g.hs, g.nstrips, g.seg, 0, dbeg, dend, g.dc);   \
    } while (0)
    if (g.k == 3) PSM_GRAYF_K(3); else if (g.k == 5) PSM_GRAYF_K(5); else PSM_GRAYF_K(9);
#undef PSM_GRAYF_K
    int yshift, rb;
    const dim3 ga = apply_grid(g, W, H, 2 * q.n, yshift, rb);
    float *const none = nullptr;
    if (rb == 4)
        rec_launch(s, k_grayf_apply<GrayVal, false, 4>, k_grayf_apply<GrayTab, false, 4>, ga, dim3(256), 0, q, none, W, H, g.ws, g.hs, yshift, 0, dbeg, dend, g.dc);
    else
        rec_launch(s, k_grayf_apply<GrayVal, false, 2>, k_grayf_apply<GrayTab, false, 2>, ga, dim3(256), 0, q, none, W, H, g.ws, g.hs, yshift, 0, dbeg, dend, g.dc);
}

void launch_grayf_chunk_store(hipStream_t s, const GrayPair &p, const GrayFgfPlan &g, int W, int H, int side, int dbeg, int dend, float *qvol)
{
    const dim3 gs(g.nstrips * g.nsegs, (dend - dbeg + 1) / 2, 1);
    const GrayVal v{{p}};
#define PSM_GRAYF_K(K)                                                                                                                         \
    do {                                                                                                                                       \
        hipLaunchKernelGGL((k_grayf_model<GrayVal, K>), gs, dim3(64), 0, s, v, W, H, g.ws, g.hs, g.nstrips, g.seg, side, dbeg, dend, g.dc);  \
        hipLaunchKernelGGL((k_grayf_smooth<GrayVal, K>), gs, dim3(64), 0, s, v, g.ws, g.hs, g.nstrips, g.seg, side, dbeg, dend, g.dc);       \
    } while (0)
    if (g.k == 3) PSM_GRAYF_K(3); else if (g.k == 5) PSM_GRAYF_K(5); else PSM_GRAYF_K(9);
#undef PSM_GRAYF_K
    int yshift, rb;
    const dim3 ga = apply_grid(g, W, H, 1, yshift, rb);
    if (rb == 4) hipLaunchKernelGGL((k_grayf_apply<GrayVal, true, 4>), ga, dim3(256), 0, s, v, qvol, W, H, g.ws, g.hs, yshift, side, dbeg, dend, g.dc);
    else hipLaunchKernelGGL((k_grayf_apply<GrayVal, true, 2>), ga, dim3(256), 0, s, v, qvol, W, H, g.ws, g.hs, yshift, side, dbeg, dend, g.dc);
}

}  // namespace psm
