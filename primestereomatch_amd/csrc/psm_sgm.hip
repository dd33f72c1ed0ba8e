// psm_sgm.hip - semi-global matching, the reference's second algorithm (STEREO_SGBM: ssgbm->compute, src/StereoMatch.cpp:169-187,
// configured by setupOpenCVSGBM, :639-660) as four kernels over the staged 8-bit pair.  All arithmetic is integer; the definition
// is tests/sgm_model.py, the device equals it element for element:
//   k_sgm_cost    C(x,y,d) = sum over the bs x bs block (replicated edge) of sum_ch |L[y][x] - R[y][max(x-d,0)]|        u16 [y][x][d]
//   k_sgm_path    one scan direction r: L_r(p,d) = C(p,d) + min(L_r(p-r,d), L_r(p-r,d+-1)+P1, m+P2) - m, m = min_k L_r(p-r,k);
//                 S += L_r (the first direction stores)                                                                   u32 [y][x][d]
//   k_sgm_select  argmin_d S (lowest d), uniqueness, sub-pixel d16, disp2[y][x-best] = min (minS << 8 | best)
//   k_sgm_check   the disp12MaxDiff test of every pixel against disp2 of its row -> int16 map, -16 where invalid
//   k_sgm_maps    (psm_sgm_select_maps, its own launch) the 8-bit maps of both views from S: argmin_d S(x, d) and argmin_d S(xr + d, d)
// psm_sgm_set_range (tests/sgm_range_model.py): index k in [0, D), D <= 1024, stands for the disparity dmin + k - the right column
// is clamp(x - dmin - k, 0, W - 1), d16, the landing column and the probes carry dmin, invalid is (dmin - 1) * 16.  Above 256
// disparities the cost kernels walk their tile once per 256 of them, a lane of k_sgm_path / k_sgm_select holds 8 or 16.
// d is innermost in both volumes (Dp = D rounded up to 4 elements per pixel): the disparities of a pixel are one contiguous read
// whatever the walking direction.  The speckle filter StereoSGBM ends with is psm_speckle.hip (psm_sgm_set_speckle).  StereoSGBM's
// own pixel cost, Birchfield-Tomasi over Sobel-prefiltered images (psm_sgm_set_prefilter, tests/sgm_bt_model.py), writes the same
// C through k_sgm_prefilter, k_sgm_bt_rows and k_sgm_bt_cols below; the census cost (psm_sgm_set_census, tests/sgm_census_model.py)
// through k_sgm_census and k_sgm_census_cost.  Unpinned: agreement with a live cv::StereoSGBM.
#include "psm_kernels.h"

#include <type_traits>

namespace psm {

constexpr int SGM_INF = 1 << 28;
constexpr int SGM_TX = 32;         // k_sgm_cost: output pixels of a row per workgroup
constexpr int SGM_U = 8;           // k_sgm_path: steps whose loads are issued together, ahead of the dependent chain

// DPP moves with `old` for the lanes that have no source (bound_ctrl off): row_shr:n 0x110 + n, wave_shl:1 0x130 (lane l <- l + 1),
// wave_shr:1 0x138 (lane l <- l - 1)
template <int CTRL>
__device__ __forceinline__ int sgm_dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false); }

// minimum over the wave, in every lane: four row_shr steps leave a row's minimum in its lane 15, the four rows meet in SGPRs
__device__ __forceinline__ int sgm_wave_min(int v)
{
    v = min(v, sgm_dpp<0x111>(0x7fffffff, v));
    v = min(v, sgm_dpp<0x112>(0x7fffffff, v));
    v = min(v, sgm_dpp<0x114>(0x7fffffff, v));
    v = min(v, sgm_dpp<0x118>(0x7fffffff, v));
    return min(min(__builtin_amdgcn_readlane(v, 15), __builtin_amdgcn_readlane(v, 31)),
               min(__builtin_amdgcn_readlane(v, 47), __builtin_amdgcn_readlane(v, 63)));
}

// (sgm_px, one pixel of a staged image as a dword of its bytes: psm_kernels.h - the reprojection stage's colours read it too)
__device__ __forceinline__ int sgm_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// Every kernel below is one body (sgm_*) behind an entry that is a template over the record source S (psm_kernels.h, Recs): the pair
// of a single call by value, or pair blockIdx.z of a batch's device table (psm_sgm_compute_batch).  The entry assembles what the body
// takes - the call's scalars and the pair's pointers, read as global ones; the pair number is uniform per workgroup, so these are
// scalar loads ahead of an unchanged body.  All index arithmetic stays inside a pair.
struct SgmRun : SgmArgs, SgmPair {
    uint16_t *Hs;                      // horizontal block sums [H][W][Dp], in the memory of S (free until the first direction stores it)
};
template <typename S>
__device__ __forceinline__ SgmRun sgm_run(const S &src, const SgmArgs &a, unsigned pair)
{
    const SgmPair &p = rec(src, pair);
    SgmRun r;
    static_cast<SgmArgs &>(r) = a;
    r.img[0] = sgm_global(p.img[0]); r.img[1] = sgm_global(p.img[1]);
    r.C = sgm_global(p.C); r.S = sgm_global(p.S); r.disp2 = sgm_global(p.disp2); r.pre = sgm_global(p.pre); r.out = sgm_global(p.out);
    r.pf[0] = sgm_global(p.pf[0]); r.pf[1] = sgm_global(p.pf[1]);
    r.spk_label = r.spk_size = nullptr;                  // (the speckle filter's: psm_speckle.hip)
    r.maps = sgm_global(p.maps);
    r.Hs = (uint16_t *)r.S;
    return r;
}
using SgmV = RecVal<SgmPair>;
using SgmT = RecTab<SgmPair>;

// One workgroup per SGM_TX pixels of one row, one thread per disparity.  The BS rows of both images the block needs go to LDS as
// one dword per pixel (v_sad_u8 then takes the 1 or 3 channels of a tap in one instruction); a thread walks x with its d fixed:
// the left tap is a broadcast, the right taps of neighbouring lanes are neighbouring dwords, the stores of a wave are 128
// contiguous bytes.  Column sums of the last BS columns stay in registers.
// WIDE (D > 256): 256 threads, a thread takes the disparities d, d + 256, ... in turn; the staged right span is NL + D - 1 columns
// either way (static LDS: 29.7 KB at BS 7 when WIDE), and holds the clamped columns: a tap's index needs no clamp of its own.
template <int BS, bool WIDE>
__device__ __forceinline__ void sgm_cost(const SgmRun &a)
{
    constexpr int HALF = BS / 2, NL = SGM_TX + BS - 1, NR = NL + (WIDE ? SGM_DMAX : 256) - 1;
    __shared__ unsigned sl[BS][NL], sr[BS][NR];
    const int y = blockIdx.y, x0 = blockIdx.x * SGM_TX;
    int d = threadIdx.x;
    const int cx_min = sgm_clamp(x0 - HALF, a.W);
    const int rbase = cx_min - a.dmin - (a.D - 1);        // image column of sr[.][0] (before the clamp)
    const int nr = NL + a.D - 1;
    for (int i = threadIdx.x; i < BS * NL; i += blockDim.x) {
        const int j = i / NL, s = i - j * NL;
        sl[j][s] = sgm_px(a.img[0], a.depth, a.ch, (size_t)sgm_clamp(y + j - HALF, a.H) * a.W + sgm_clamp(x0 - HALF + s, a.W));
    }
    for (int i = threadIdx.x; i < BS * nr; i += blockDim.x) {
        const int j = i / nr, k = i - j * nr;
        sr[j][k] = sgm_px(a.img[1], a.depth, a.ch, (size_t)sgm_clamp(y + j - HALF, a.H) * a.W + sgm_clamp(rbase + k, a.W));
    }
    __syncthreads();
    if (d >= a.Dp) return;
    do {
        const bool real = d < a.D;
        const int kd = a.D - 1 - (real ? d : 0) - cx_min;     // column cx, index d: sr[.][cx - cx_min + D - 1 - d], inside [0, nr)
        unsigned v[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) v[i] = 0;
        for (int s = 0; s < NL; ++s) {
            const int k = sgm_clamp(x0 - HALF + s, a.W) + kd;
            unsigned col = 0;
#pragma unroll
            for (int j = 0; j < BS; ++j) col = __builtin_amdgcn_sad_u8(sl[j][s], sr[j][k], col);
#pragma unroll
            for (int i = 0; i + 1 < BS; ++i) v[i] = v[i + 1];
            v[BS - 1] = col;
            const int x = x0 + s - (BS - 1);
            if (s >= BS - 1 && x < a.W) {
                unsigned sum = 0;
#pragma unroll
                for (int i = 0; i < BS; ++i) sum += v[i];
                a.C[((size_t)y * a.W + x) * a.Dp + d] = (uint16_t)(real ? sum : 0u);
            }
        }
    } while (WIDE && (d += 256) < a.Dp);
}

template <int BS, bool WIDE, typename S>
__global__ __launch_bounds__(256) void k_sgm_cost(SgmArgs a, S src) { sgm_cost<BS, WIDE>(sgm_run(src, a, blockIdx.z)); }

// ---- the prefiltered Birchfield-Tomasi cost (psm_sgm_set_prefilter, tests/sgm_bt_model.py): the same C by three kernels -------
//   k_sgm_prefilter  both images -> their 2 ch planes per pixel (x-Sobel clipped to [0, 2 ft], the intensity; ft in the border columns)
//   k_sgm_bt_rows    c(x,y,d) and its horizontal sum over the block's columns (replicated edge) -> Hs u16 [y][x][d], in S's memory
//   k_sgm_bt_cols    the vertical sum of Hs over the block's rows (replicated edge), marching down the rows -> C
// Every c is evaluated once (the bs - 1 columns two neighbouring tiles of SGM_BT_TX columns share: twice): a Birchfield-Tomasi
// tap is ~13 packed operations per pair of planes, not the one v_sad_u8 k_sgm_cost repeats per block row.

// k_sgm_prefilter: one thread per pixel of one image (blockIdx.z = 2 pair + side); a float image is quantised here, once
__device__ __forceinline__ void sgm_prefilter(const SgmRun &a, int side)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    const void *img = a.img[side];
    const int ch = a.ch, ft = a.ft;
    uint8_t *out = a.pf[side] + ((size_t)y * a.W + x) * (2 * ch);
    if (x == 0 || x == a.W - 1) {
        for (int i = 0; i < 2 * ch; ++i) out[i] = (uint8_t)ft;
        return;
    }
    const int rows[3] = {max(y - 1, 0), y, min(y + 1, a.H - 1)};
    unsigned w[3], e[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        w[j] = sgm_px(img, a.depth, ch, (size_t)rows[j] * a.W + x - 1);
        e[j] = sgm_px(img, a.depth, ch, (size_t)rows[j] * a.W + x + 1);
    }
    const unsigned centre = sgm_px(img, a.depth, ch, (size_t)y * a.W + x);
    for (int k = 0; k < ch; ++k) {
        int g = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) g += (j == 1 ? 2 : 1) * ((int)((e[j] >> (8 * k)) & 255u) - (int)((w[j] >> (8 * k)) & 255u));
        out[k] = (uint8_t)(min(max(g, -ft), ft) + ft);
        out[ch + k] = (uint8_t)((centre >> (8 * k)) & 255u);
    }
}

// (the side's planes go to slot 0 ahead of the body: an index that is known at compile time keeps the assembled record in registers)
template <typename S>
__global__ __launch_bounds__(256) void k_sgm_prefilter(SgmArgs a, S src)
{
    SgmRun r = sgm_run(src, a, blockIdx.z >> 1);
    if (blockIdx.z & 1) { r.img[0] = r.img[1]; r.pf[0] = r.pf[1]; }
    sgm_prefilter(r, 0);
}

// Two adjacent planes of a pixel travel as the two 16-bit lanes of a dword (planes 2p, 2p + 1: pair p), so that one packed
// instruction (v_pk_sub_i16, v_pk_max_i16, v_pk_min_i16) serves both; every value is in [-255, 255].
typedef short sgm_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ sgm_s2 sgm_as_s2(unsigned v) { return __builtin_bit_cast(sgm_s2, v); }
__device__ __forceinline__ unsigned sgm_as_u(sgm_s2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ unsigned sgm_bt_pair(const uint8_t *p) { return (unsigned)p[0] | ((unsigned)p[1] << 16); }

// pixel cx of a plane row ([W][2 NP] bytes) -> dst[(3 p + q) * stride], q = 0: the values, 1: lo, 2: hi (the half-sample bounds)
template <int NP>
__device__ __forceinline__ void sgm_bt_stage(const uint8_t *row, int W, int cx, unsigned *dst, int stride)
{
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const uint8_t *q = row + ((size_t)cx * NP + p) * 2;
        const unsigned v = sgm_bt_pair(q);
        const unsigned vl = cx > 0 ? ((v + sgm_bt_pair(q - 2 * NP)) >> 1) & 0x00ff00ffu : v;          // (a lane's sum <= 510: no carry)
        const unsigned vr = cx < W - 1 ? ((v + sgm_bt_pair(q + 2 * NP)) >> 1) & 0x00ff00ffu : v;
        const sgm_s2 s = sgm_as_s2(v), sl = sgm_as_s2(vl), sr = sgm_as_s2(vr);
        dst[(3 * p) * stride] = v;
        dst[(3 * p + 1) * stride] = sgm_as_u(__builtin_elementwise_min(s, __builtin_elementwise_min(sl, sr)));
        dst[(3 * p + 2) * stride] = sgm_as_u(__builtin_elementwise_max(s, __builtin_elementwise_max(sl, sr)));
    }
}

// One workgroup per SGM_BT_TX pixels of one row, one thread per disparity, as k_sgm_cost - but one image row only: a thread walks
// x with its d fixed, evaluates c(x, y, d) once and keeps the last BS of them in registers.  LDS holds, per pixel and pair of
// planes, the values and both bounds of the left tile and of the part of the right row the tile's disparities reach; the left
// operands are broadcasts, the right ones of neighbouring lanes neighbouring dwords.  NP pairs of planes: ch = NP (1 or 3); plane
// i has shift 0 below ch (P), 2 from ch on (Q).  The sums go to Hs, or to C itself when BS is 1 (a 1 x 1 block has no vertical sum).
// WIDE: as k_sgm_cost (static LDS: 46.5 KB at BS 7, NP 3).
template <int BS, int NP, bool WIDE>
__device__ __forceinline__ void sgm_bt_rows(const SgmRun &a)
{
    uint16_t *const out = BS == 1 ? a.C : a.Hs;
    constexpr int HALF = BS / 2, NL = SGM_BT_TX + BS - 1, NR = NL + (WIDE ? SGM_DMAX : 256) - 1, NQ = 3 * NP;
    __shared__ unsigned sl[NQ][NL], sr[NQ][NR];
    const int y = blockIdx.y, x0 = blockIdx.x * SGM_BT_TX;
    int d = threadIdx.x;
    const int cx_min = sgm_clamp(x0 - HALF, a.W);
    const int rbase = cx_min - a.dmin - (a.D - 1);        // image column of sr[.][0] (before the clamp)
    const int nr = NL + a.D - 1;
    const uint8_t *rowl = a.pf[0] + (size_t)y * a.W * (2 * NP), *rowr = a.pf[1] + (size_t)y * a.W * (2 * NP);
    for (int i = threadIdx.x; i < NL; i += blockDim.x) sgm_bt_stage<NP>(rowl, a.W, sgm_clamp(x0 - HALF + i, a.W), &sl[0][i], NL);
    for (int i = threadIdx.x; i < nr; i += blockDim.x) sgm_bt_stage<NP>(rowr, a.W, sgm_clamp(rbase + i, a.W), &sr[0][i], NR);
    __syncthreads();
    if (d >= a.Dp) return;
    const int ns = min(NL, a.W - x0 + BS - 1);            // the steps up to the row's last pixel
    const sgm_s2 zero = {0, 0};
    do {
        const bool real = d < a.D;
        const int kd = a.D - 1 - (real ? d : 0) - cx_min;     // column cx, index d: sr[.][cx - cx_min + D - 1 - d], inside [0, nr)
        unsigned v[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) v[i] = 0;
        for (int s = 0; s < ns; ++s) {
            const int k = sgm_clamp(x0 - HALF + s, a.W) + kd;
            unsigned col = 0;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const sgm_s2 u = sgm_as_s2(sl[3 * p][s]), lu = sgm_as_s2(sl[3 * p + 1][s]), hu = sgm_as_s2(sl[3 * p + 2][s]);
                const sgm_s2 w = sgm_as_s2(sr[3 * p][k]), lw = sgm_as_s2(sr[3 * p + 1][k]), hw = sgm_as_s2(sr[3 * p + 2][k]);
                const sgm_s2 c0 = __builtin_elementwise_max(__builtin_elementwise_max(u - hw, lw - u), zero);
                const sgm_s2 c1 = __builtin_elementwise_max(__builtin_elementwise_max(w - hu, lu - w), zero);
                const unsigned m = sgm_as_u(__builtin_elementwise_min(c0, c1));
                constexpr int CH = NP;
                const int s0 = 2 * p >= CH ? 2 : 0, s1 = 2 * p + 1 >= CH ? 2 : 0;
                col += ((m & 0xffffu) >> s0) + (m >> (16 + s1));
            }
#pragma unroll
            for (int i = 0; i + 1 < BS; ++i) v[i] = v[i + 1];
            v[BS - 1] = col;
            if (s >= BS - 1) {
                unsigned sum = 0;
#pragma unroll
                for (int i = 0; i < BS; ++i) sum += v[i];
                out[((size_t)y * a.W + (x0 + s - (BS - 1))) * a.Dp + d] = (uint16_t)(real ? sum : 0u);
            }
        }
    } while (WIDE && (d += 256) < a.Dp);
}

template <int BS, int NP, bool WIDE, typename S>
__global__ __launch_bounds__(256) void k_sgm_bt_rows(SgmArgs a, S src) { sgm_bt_rows<BS, NP, WIDE>(sgm_run(src, a, blockIdx.z)); }

// The vertical sum: a thread holds four adjacent disparities of one pixel column (8 bytes: Dp is a multiple of 4) and marches
// down SGM_BT_YS rows; the last BS rows of Hs stay in registers, a step is one load, one add, one subtract and one store.  Two
// 16-bit sums share a dword: every result is at most 65535 (psm_sgm_set_params), and the 32-bit arithmetic is exact modulo 2^32,
// so no carry survives between the halves.  Only the BS - 1 rows two segments share are loaded twice.
template <int BS>
__device__ __forceinline__ void sgm_bt_cols(const SgmRun &a)
{
    constexpr int HALF = BS / 2;
    const size_t rowq = (size_t)a.W * a.Dp / 4;           // uint2 per row
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rowq) return;
    const int y0 = blockIdx.y * SGM_BT_YS, y1 = min(y0 + SGM_BT_YS, a.H);
    const uint2 *src = (const uint2 *)a.Hs + e;
    uint2 *dst = (uint2 *)a.C + e;
    uint2 ring[BS], sum = make_uint2(0u, 0u);
#pragma unroll
    for (int j = 0; j < BS; ++j) {
        ring[j] = src[(size_t)sgm_clamp(y0 - HALF + j, a.H) * rowq];
        sum.x += ring[j].x; sum.y += ring[j].y;
    }
    dst[(size_t)y0 * rowq] = sum;
    for (int y = y0 + 1; y < y1; y += BS) {
#pragma unroll
        for (int r = 0; r < BS; ++r) {
            if (y + r < y1) {
                const uint2 n = src[(size_t)sgm_clamp(y + r + HALF, a.H) * rowq];
                sum.x += n.x - ring[r].x; sum.y += n.y - ring[r].y;
                ring[r] = n;
                dst[(size_t)(y + r) * rowq] = sum;
            }
        }
    }
}

template <int BS, typename S> __global__ __launch_bounds__(256) void k_sgm_bt_cols(SgmArgs a, S src) { sgm_bt_cols<BS>(sgm_run(src, a, blockIdx.z)); }

// ---- the census cost (psm_sgm_set_census, tests/sgm_census_model.py): the same C by two kernels ---------------------------------
//   k_sgm_census       both images -> their code planes T [H][W] uint64: bit i is "tap i of the win_w x win_h window is darker than
//                      the centre" on the gray plane, the taps in raster order with the centre skipped, the plane replicated
//   k_sgm_census_cost  C(x,y,k) = the bs x bs box sum (replicated edge) of popcount(T_L[y][x] ^ T_R[y][xr])

// the gray value of one staged pixel: the byte, or (1868 B + 9617 G + 4899 R + 8192) >> 14 of the staged order B, G, R
__device__ __forceinline__ unsigned sgm_gray(const void *img, int depth, int ch, size_t idx)
{
    const unsigned v = sgm_px(img, depth, ch, idx);
    return ch == 1 ? v : (1868u * (v & 255u) + 9617u * ((v >> 8) & 255u) + 4899u * (v >> 16) + 8192u) >> 14;
}

// One workgroup per tile of SGM_CEN_TX x SGM_CEN_TY pixels of one image (blockIdx.z = 2 pair + side), one pixel per
// thread.  The tile's gray values with the window's halo go to LDS as bytes (a float image is quantised here, once); the clamp of
// a tap is done there.  The two dwords of a code are built separately - a tap sets a bit of one of them - and leave as one 8-byte
// store.
__device__ __forceinline__ void sgm_census(const SgmRun &a, int side)
{
    constexpr int LW = SGM_CEN_TX + SGM_CEN_MAXW - 1, LH = SGM_CEN_TY + SGM_CEN_MAXH - 1;
    __shared__ uint8_t sg[LH * LW];
    const int hx = a.cw / 2, hy = a.chh / 2, lw = SGM_CEN_TX + 2 * hx, lh = SGM_CEN_TY + 2 * hy;      // lw <= LW, lh <= LH
    const int x0 = blockIdx.x * SGM_CEN_TX, y0 = blockIdx.y * SGM_CEN_TY;
    const void *img = side ? a.img[1] : a.img[0];             // (no index: the argument record stays in registers)
    for (int i = threadIdx.x; i < lh * lw; i += blockDim.x) {
        const int j = i / lw, s = i - j * lw;
        sg[i] = (uint8_t)sgm_gray(img, a.depth, a.ch, (size_t)sgm_clamp(y0 - hy + j, a.H) * a.W + sgm_clamp(x0 - hx + s, a.W));
    }
    __syncthreads();
    const int tx = threadIdx.x % SGM_CEN_TX, ty = threadIdx.x / SGM_CEN_TX;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;
    const unsigned centre = sg[(ty + hy) * lw + tx + hx];
    unsigned lo = 0, hi = 0;
    int i = 0;
    for (int dy = 0; dy <= 2 * hy; ++dy) {
        const uint8_t *row = sg + (ty + dy) * lw + tx;
        for (int dx = 0; dx <= 2 * hx; ++dx) {
            if (dy == hy && dx == hx) continue;
            const unsigned bit = row[dx] < centre;
            if (i < 32) lo |= bit << i;
            else hi |= bit << (i - 32);
            ++i;
        }
    }
    ((uint2 *)(side ? a.pf[1] : a.pf[0]))[(size_t)y * a.W + x] = make_uint2(lo, hi);
}

template <typename S>
__global__ __launch_bounds__(256) void k_sgm_census(SgmArgs a, S src) { sgm_census(sgm_run(src, a, blockIdx.z >> 1), blockIdx.z & 1); }

// k_sgm_cost's shape: one workgroup per SGM_TX pixels of one row, one thread per disparity; the BS rows of both code planes go to
// LDS as 8-byte words, the left tap is a broadcast, the right taps of neighbouring lanes are neighbouring words; where k_sgm_cost
// has one v_sad_u8 with its accumulator this has two XORs and two v_bcnt_u32_b32, whose second operand takes the running sum.
// Column sums of the last BS columns stay in registers.  Above 256 disparities the 256 threads take the disparities in passes of
// 256 and the right span is staged again for every pass: NL + 255 columns whatever D is (static LDS: 18.1 KB at BS 7, where one
// span for all 1024 disparities would be 61.5 KB and leave a CU one workgroup).
template <int BS>
__device__ __forceinline__ void sgm_census_cost(const SgmRun &a)
{
    constexpr int HALF = BS / 2, NL = SGM_TX + BS - 1, NR = NL + 255;
    __shared__ uint2 sl[BS][NL], sr[BS][NR];
    const uint2 *tl = (const uint2 *)a.pf[0], *tr = (const uint2 *)a.pf[1];
    const int y = blockIdx.y, x0 = blockIdx.x * SGM_TX;
    const int cx_min = sgm_clamp(x0 - HALF, a.W);
    for (int i = threadIdx.x; i < BS * NL; i += blockDim.x) {
        const int j = i / NL, s = i - j * NL;
        sl[j][s] = tl[(size_t)sgm_clamp(y + j - HALF, a.H) * a.W + sgm_clamp(x0 - HALF + s, a.W)];
    }
    for (int db = 0; db < a.Dp; db += 256) {                  // the pass over the indices db .. de - 1 (db < D: Dp - D < 16)
        const int de = min(a.D, db + 256);
        const int rbase = cx_min - a.dmin - (de - 1);         // image column of sr[.][0] (before the clamp)
        const int nr = NL + (de - db) - 1;
        if (db) __syncthreads();                              // the previous pass has read its span
        for (int i = threadIdx.x; i < BS * nr; i += blockDim.x) {
            const int j = i / nr, k = i - j * nr;
            sr[j][k] = tr[(size_t)sgm_clamp(y + j - HALF, a.H) * a.W + sgm_clamp(rbase + k, a.W)];
        }
        __syncthreads();
        const int d = db + threadIdx.x;
        if (d >= a.Dp) continue;
        const bool real = d < a.D;
        const int kd = de - 1 - (real ? d : db) - cx_min;     // column cx, index d: sr[.][cx - cx_min + de - 1 - d], inside [0, nr)
        unsigned v[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) v[i] = 0;
        for (int s = 0; s < NL; ++s) {
            const int k = sgm_clamp(x0 - HALF + s, a.W) + kd;
            unsigned col = 0;
#pragma unroll
            for (int j = 0; j < BS; ++j) {
                const uint2 l = sl[j][s], r = sr[j][k];
                col = __builtin_popcount(l.x ^ r.x) + col;
                col = __builtin_popcount(l.y ^ r.y) + col;
            }
#pragma unroll
            for (int i = 0; i + 1 < BS; ++i) v[i] = v[i + 1];
            v[BS - 1] = col;
            const int x = x0 + s - (BS - 1);
            if (s >= BS - 1 && x < a.W) {
                unsigned sum = 0;
#pragma unroll
                for (int i = 0; i < BS; ++i) sum += v[i];
                a.C[((size_t)y * a.W + x) * a.Dp + d] = (uint16_t)(real ? sum : 0u);
            }
        }
    }
}

template <int BS, typename S> __global__ __launch_bounds__(256) void k_sgm_census_cost(SgmArgs a, S src) { sgm_census_cost<BS>(sgm_run(src, a, blockIdx.z)); }

// NV adjacent disparities per lane: what a lane moves per pixel, and U, the steps of k_sgm_path whose loads are issued together.
// NV U is constant from NV 4 on: the look-ahead of the wide forms (NV 8, 16: Dp up to 512, 1024) holds the 2 U (NV / 2 + NV) = 96
// dwords of NV 4, not 192 or 384 - the registers the longer vectors need go to lq, c, l and s instead.
template <int N> struct alignas(16) SgmQ { uint4 q[N]; };
template <int NV> struct SgmVec;
template <> struct SgmVec<1> { using C = unsigned short; using S = unsigned; static constexpr int U = SGM_U; };
template <> struct SgmVec<2> { using C = unsigned; using S = uint2; static constexpr int U = SGM_U; };
template <> struct SgmVec<4> { using C = uint2; using S = uint4; static constexpr int U = SGM_U; };
template <> struct SgmVec<8> { using C = uint4; using S = SgmQ<2>; static constexpr int U = SGM_U / 2; };
template <> struct SgmVec<16> { using C = SgmQ<2>; using S = SgmQ<4>; static constexpr int U = SGM_U / 4; };
__device__ __forceinline__ void sgm_unpack(unsigned short v, int *o) { o[0] = v; }
__device__ __forceinline__ void sgm_unpack(unsigned v, int *o) { o[0] = v & 0xffffu; o[1] = v >> 16; }
__device__ __forceinline__ void sgm_unpack(uint2 v, int *o) { o[0] = v.x & 0xffffu; o[1] = v.x >> 16; o[2] = v.y & 0xffffu; o[3] = v.y >> 16; }
__device__ __forceinline__ void sgm_unpack(uint4 v, int *o) { sgm_unpack(make_uint2(v.x, v.y), o); sgm_unpack(make_uint2(v.z, v.w), o + 4); }
__device__ __forceinline__ void sgm_unpack(const SgmQ<2> &v, int *o) { sgm_unpack(v.q[0], o); sgm_unpack(v.q[1], o + 8); }
__device__ __forceinline__ void sgm_unpack_s(unsigned v, unsigned *o) { o[0] = v; }
__device__ __forceinline__ void sgm_unpack_s(uint2 v, unsigned *o) { o[0] = v.x; o[1] = v.y; }
__device__ __forceinline__ void sgm_unpack_s(uint4 v, unsigned *o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
template <int N> __device__ __forceinline__ void sgm_unpack_s(const SgmQ<N> &v, unsigned *o)
{
#pragma unroll
    for (int i = 0; i < N; ++i) sgm_unpack_s(v.q[i], o + 4 * i);
}
__device__ __forceinline__ void sgm_pack_s(const unsigned *o, unsigned &v) { v = o[0]; }
__device__ __forceinline__ void sgm_pack_s(const unsigned *o, uint2 &v) { v = make_uint2(o[0], o[1]); }
__device__ __forceinline__ void sgm_pack_s(const unsigned *o, uint4 &v) { v = make_uint4(o[0], o[1], o[2], o[3]); }
template <int N> __device__ __forceinline__ void sgm_pack_s(const unsigned *o, SgmQ<N> &v)
{
#pragma unroll
    for (int i = 0; i < N; ++i) sgm_pack_s(o + 4 * i, v.q[i]);
}

// the paths of direction (dy, dx): one per pixel whose predecessor lies outside the image
__host__ __device__ inline int sgm_npaths(int W, int H, int dy, int dx) { return dy == 0 ? H : (dx == 0 ? W : W + H - 1); }

// One wave per path, lane l holds the disparities l * NV .. l * NV + NV - 1 of the previous pixel, normalised (L - m: their
// minimum is 0), so a step is L = C + min(Lq(d), Lq(d-1) + P1, Lq(d+1) + P1, P2); d+-1 is a register except at the lane's edges
// (two DPP moves), m the DPP minimum over the wave.  The recurrence is one dependent chain; C and S do not depend on it, so the
// loads of SGM_U steps are issued together, one batch ahead of the one the chain is walking.  The body of the main loop has no
// branch: the compiler then waits for exactly the loads a step needs (s_waitcnt vmcnt(n)) - with a branch per step it waited for
// everything in flight, the previous step's store included, and a step cost a store round trip (measured: 1080p x 256, 13.6 ms for
// the eight directions in that form).  Loads past the end of a path read its last pixel again; FIRST: the first direction of a
// frame stores S instead of adding to it; ALL: every lane holds disparities below Dp (Dp = 64 NV) and stores without a predicate.
// Within a direction every voxel lies on exactly one path and the launches of a frame follow each other on one stream: S is
// updated with plain loads and stores, no atomics.
template <int NV, bool FIRST, bool ALL>
__device__ __forceinline__ void sgm_path(const SgmRun &a, int dy, int dx)
{
    using CV = typename SgmVec<NV>::C;
    using SV = typename SgmVec<NV>::S;
    constexpr int U = SgmVec<NV>::U;
    const int lane = threadIdx.x & 63;
    const int path = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (path >= sgm_npaths(a.W, a.H, dy, dx)) return;             // (wave-uniform)
    const int xs = dx > 0 ? 0 : a.W - 1, ys = dy > 0 ? 0 : a.H - 1;        // where a path enters the image
    int x, y;
    if (dy == 0) { x = xs; y = path; }
    else if (dx == 0 || path < a.W) { x = path; y = ys; }
    else { x = xs; y = ys + dy * (path - a.W + 1); }
    const int lx = dx == 0 ? a.H : (dx > 0 ? a.W - x : x + 1), ly = dy == 0 ? a.W : (dy > 0 ? a.H - y : y + 1);
    const int len = min(lx, ly);
    const int d0 = lane * NV;
    const bool act = ALL || d0 < a.Dp;
    const long long step = ((long long)dy * a.W + dx) * a.Dp;
    const long long off = ((long long)y * a.W + x) * a.Dp + (act ? d0 : 0);      // the path's first pixel (lanes past Dp: lane 0's
                                                                                 // address - they load what they never use)
    int lq[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) lq[k] = d0 + k < a.D ? 0 : SGM_INF;
    CV cv[2][U];
    SV sv[2][U];
    auto load = [&](CV (&cb)[U], SV (&sb)[U], int i) {             // the loads of steps i .. i + U - 1
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long o = off + min(i + u, len - 1) * step;
            cb[u] = *(const CV *)(a.C + o);
            if (!FIRST) sb[u] = *(const SV *)(a.S + o);
        }
    };
    auto run = [&](const CV (&cb)[U], const SV (&sb)[U], int i, auto full) {      // ... and their part of the chain
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (decltype(full)::value || i + u < len) {
                int c[NV], l[NV];
                unsigned s[NV] = {};
                sgm_unpack(cb[u], c);
                if (!FIRST) sgm_unpack_s(sb[u], s);
                const int left = sgm_dpp<0x138>(SGM_INF, lq[NV - 1]), right = sgm_dpp<0x130>(SGM_INF, lq[0]);
                int lmin = SGM_INF;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int lo = (k ? lq[k - 1] : left) + a.P1, hi = (k + 1 < NV ? lq[k + 1] : right) + a.P1;
                    const int t = min(min(lq[k], lo), min(hi, a.P2));
                    l[k] = d0 + k < a.D ? c[k] + t : SGM_INF;
                    lmin = min(lmin, l[k]);
                }
                const int m = sgm_wave_min(lmin);
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const bool real = d0 + k < a.D;
                    s[k] += real ? (unsigned)l[k] : 0u;
                    lq[k] = real ? l[k] - m : SGM_INF;
                }
                if (act) {
                    SV o;
                    sgm_pack_s(s, o);
                    *(SV *)(a.S + off + (i + u) * step) = o;
                }
            }
        }
    };
    load(cv[0], sv[0], 0);
    int i = 0;
    for (; i + 2 * U <= len; i += 2 * U) {
        load(cv[1], sv[1], i + U);
        run(cv[0], sv[0], i, std::true_type{});
        load(cv[0], sv[0], i + 2 * U);
        run(cv[1], sv[1], i + U, std::true_type{});
    }
    load(cv[1], sv[1], i + U);                                        // fewer than 2 U steps are left
    run(cv[0], sv[0], i, std::false_type{});
    run(cv[1], sv[1], i + U, std::false_type{});
}

// a batch: n x (H, W or W + H - 1) one-wave paths per launch - what hides a path's dependent chain is other pairs' waves on the same SIMD
template <int NV, bool FIRST, bool ALL, typename S>
__global__ __launch_bounds__(256) void k_sgm_path(SgmArgs a, S src, int dy, int dx) { sgm_path<NV, FIRST, ALL>(sgm_run(src, a, blockIdx.z), dy, dx); }

// One wave per pixel: the packed (S << KB | d) minimum over the wave is argmin with the lowest d on ties (S < 2^19: at most
// 8 * 65535 = 524280, which tests/test_gpu_sgm_fuzz.py::test_saturating_pairs_reach_the_packing_bound reaches).  KB is 8 up to 256
// disparities, 10 above (29 bits).  d is the index; the disparity is dmin + d in d16 and in the landing column.
template <int NV>
__device__ __forceinline__ void sgm_select(const SgmRun &a)
{
    using SV = typename SgmVec<NV>::S;
    constexpr int KB = NV > 4 ? 10 : 8;                            // = sgm_kb(Dp): NV > 4 is Dp > 256
    const int lane = threadIdx.x & 63;
    const int pix = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= a.W * a.H) return;                                 // (wave-uniform)
    const int d0 = lane * NV;
    const unsigned *Sp = a.S + (size_t)pix * a.Dp;
    unsigned s[NV] = {};
    if (d0 < a.Dp) sgm_unpack_s(*(const SV *)(Sp + d0), s);
    int key = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (d0 + k < a.D) key = min(key, (int)((s[k] << KB) | (unsigned)(d0 + k)));
    const int kmin = sgm_wave_min(key);
    const int best = kmin & ((1 << KB) - 1), minS = kmin >> KB;
    bool rival = false;                                            // a disparity further than 1 from best within the uniqueness margin
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int d = d0 + k;
        rival |= d < a.D && (d < best - 1 || d > best + 1) && (int)s[k] * (100 - a.u) < minS * 100;
    }
    const bool unique = !__any(rival);
    if (lane != 0) return;
    int d16 = (a.dmin + best) * 16;
    if (best > 0 && best < a.D - 1) {
        const int sm = (int)Sp[best - 1], sp = (int)Sp[best + 1];
        const int den = max(sm + sp - 2 * minS, 1);
        const int num = (sm - sp) * 16 + den, dd = 2 * den;
        int q = num / dd;
        if (num % dd != 0 && num < 0) --q;                         // floor
        d16 += q;
    }
    a.pre[pix] = (int16_t)(unique ? d16 : a.invalid);
    const int y = pix / a.W, x = pix - y * a.W, xl = x - (a.dmin + best);
    if (unique && xl >= 0 && xl < a.W) atomicMin(a.disp2 + (size_t)y * a.W + xl, (unsigned)kmin);
}

template <int NV, typename S> __global__ __launch_bounds__(256) void k_sgm_select(SgmArgs a, S src) { sgm_select<NV>(sgm_run(src, a, blockIdx.z)); }

// a packed minimum's disparity: dmin + its index bits (mask)
__device__ __forceinline__ bool sgm_bad_probe(const unsigned *row, int W, int xq, int dq, int m, int dmin, unsigned mask)
{
    if (xq < 0 || xq >= W) return false;
    const unsigned k = row[xq];
    if (k == 0xffffffffu) return false;
    const int t = dmin + (int)(k & mask) - dq;
    return (t < 0 ? -t : t) > m;
}

__device__ __forceinline__ void sgm_check(const SgmRun &a)
{
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.W * a.H) return;
    int v = a.pre[pix];
    if (v != a.invalid && a.m >= 0) {
        const int y = pix / a.W, x = pix - y * a.W;
        const unsigned *row = a.disp2 + (size_t)y * a.W;
        const unsigned mask = (1u << sgm_kb(a.Dp)) - 1u;
        const int da = v >> 4, db = (v + 15) >> 4;                 // (arithmetic shifts: floor, also of a negative d16)
        if (sgm_bad_probe(row, a.W, x - da, da, a.m, a.dmin, mask) && sgm_bad_probe(row, a.W, x - db, db, a.m, a.dmin, mask)) v = a.invalid;
    }
    a.out[pix] = (int16_t)v;
}

template <typename S> __global__ __launch_bounds__(256) void k_sgm_check(SgmArgs a, S src) { sgm_check(sgm_run(src, a, blockIdx.z)); }

// disp2 of every pair of a batch: "nothing lands here" (the single pair's is a hipMemsetAsync)
__global__ __launch_bounds__(256) void k_sgm_fill(SgmArgs a, const SgmPair *tab)
{
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix < a.W * a.H) sgm_global(tab[blockIdx.z].disp2)[pix] = 0xffffffffu;
}

void launch_sgm_fill_batch(hipStream_t s, const SgmArgs &a, const SgmPair *tab, int n)
{
    hipLaunchKernelGGL(k_sgm_fill, dim3((a.W * a.H + 255) / 256, 1, n), dim3(256), 0, s, a, tab);
}

// one thread per disparity up to 256 of them; above, 256 threads that each take every 256th (the WIDE forms)
static unsigned sgm_cost_threads(int D) { return D > 256 ? 256u : (unsigned)((D + 63) / 64 * 64); }

// The run-time block size (1, 3, 5 or 7: psm_sgm_set_params) and `wide` as the kernels' template arguments: f(BS, WIDE) with two
// std::integral_constant values
template <typename F>
static void sgm_with_bs(int bs, bool wide, F f)
{
    auto g = [&](auto b) {
        if (wide) f(b, std::true_type{});
        else f(b, std::false_type{});
    };
    switch (bs) {
    case 1: g(std::integral_constant<int, 1>{}); break;
    case 3: g(std::integral_constant<int, 3>{}); break;
    case 5: g(std::integral_constant<int, 5>{}); break;
    default: g(std::integral_constant<int, 7>{}); break;
    }
}

// one launch over the pairs of q (psm_kernels.h, rec_launch): the pairs - times `per`, the images of a pair - on grid axis z
template <typename... A>
static void sgm_launch(hipStream_t s, void (*kv)(SgmArgs, SgmV, A...), void (*kt)(SgmArgs, SgmT, A...), dim3 grid, dim3 block, const SgmArgs &a,
                       const Recs<SgmPair> &q, int per, A... rest)
{
    rec_launch(s, kv, kt, dim3(grid.x, grid.y, (unsigned)(per * q.n)), block, 0, a, q, rest...);
}

void launch_sgm_cost(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q)
{
    const dim3 grid((a.W + SGM_TX - 1) / SGM_TX, a.H), block(sgm_cost_threads(a.D));
    sgm_with_bs(a.bs, a.D > 256, [&](auto bs, auto wide) {
        constexpr int BS = decltype(bs)::value;
        constexpr bool WIDE = decltype(wide)::value;
        sgm_launch(s, k_sgm_cost<BS, WIDE, SgmV>, k_sgm_cost<BS, WIDE, SgmT>, grid, block, a, q, 1);
    });
}

void launch_sgm_cost_bt(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q)
{
    sgm_launch(s, k_sgm_prefilter<SgmV>, k_sgm_prefilter<SgmT>, dim3((a.W + 255) / 256, a.H), dim3(256), a, q, 2);
    const dim3 grid((a.W + SGM_BT_TX - 1) / SGM_BT_TX, a.H), block(sgm_cost_threads(a.D));
    sgm_with_bs(a.bs, a.D > 256, [&](auto bs, auto wide) {
        constexpr int BS = decltype(bs)::value;
        constexpr bool WIDE = decltype(wide)::value;
        if (a.ch == 1) sgm_launch(s, k_sgm_bt_rows<BS, 1, WIDE, SgmV>, k_sgm_bt_rows<BS, 1, WIDE, SgmT>, grid, block, a, q, 1);
        else sgm_launch(s, k_sgm_bt_rows<BS, 3, WIDE, SgmV>, k_sgm_bt_rows<BS, 3, WIDE, SgmT>, grid, block, a, q, 1);
        if constexpr (BS > 1) {
            const size_t rowq = (size_t)a.W * a.Dp / 4;
            sgm_launch(s, k_sgm_bt_cols<BS, SgmV>, k_sgm_bt_cols<BS, SgmT>, dim3((unsigned)((rowq + 255) / 256), (a.H + SGM_BT_YS - 1) / SGM_BT_YS), dim3(256), a, q, 1);
        }
    });
}

void launch_sgm_cost_census(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q)
{
    sgm_launch(s, k_sgm_census<SgmV>, k_sgm_census<SgmT>, dim3((a.W + SGM_CEN_TX - 1) / SGM_CEN_TX, (a.H + SGM_CEN_TY - 1) / SGM_CEN_TY),
               dim3(SGM_CEN_TX * SGM_CEN_TY), a, q, 2);
    const dim3 grid((a.W + SGM_TX - 1) / SGM_TX, a.H), block(sgm_cost_threads(a.D));
    sgm_with_bs(a.bs, false, [&](auto bs, auto) {              // (one form whatever D is: the passes are the kernel's own)
        constexpr int BS = decltype(bs)::value;
        sgm_launch(s, k_sgm_census_cost<BS, SgmV>, k_sgm_census_cost<BS, SgmT>, grid, block, a, q, 1);
    });
}

// lanes hold 1, 2, 4, 8 or 16 disparities, the smallest count that covers Dp with 64 lanes: f(NV) with a std::integral_constant
template <typename F>
static void sgm_with_nv(int Dp, F f)
{
    if (Dp <= 64) f(std::integral_constant<int, 1>{});
    else if (Dp <= 128) f(std::integral_constant<int, 2>{});
    else if (Dp <= 256) f(std::integral_constant<int, 4>{});
    else if (Dp <= 512) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

void launch_sgm_path(hipStream_t s, const SgmArgs &a, int dy, int dx, bool first, const Recs<SgmPair> &q)
{
    const dim3 grid((sgm_npaths(a.W, a.H, dy, dx) + 3) / 4), block(256);
    sgm_with_nv(a.Dp, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        const bool all = a.Dp == 64 * NV;
        if (first && all) sgm_launch(s, k_sgm_path<NV, true, true, SgmV>, k_sgm_path<NV, true, true, SgmT>, grid, block, a, q, 1, dy, dx);
        else if (first) sgm_launch(s, k_sgm_path<NV, true, false, SgmV>, k_sgm_path<NV, true, false, SgmT>, grid, block, a, q, 1, dy, dx);
        else if (all) sgm_launch(s, k_sgm_path<NV, false, true, SgmV>, k_sgm_path<NV, false, true, SgmT>, grid, block, a, q, 1, dy, dx);
        else sgm_launch(s, k_sgm_path<NV, false, false, SgmV>, k_sgm_path<NV, false, false, SgmT>, grid, block, a, q, 1, dy, dx);
    });
}

void launch_sgm_select(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q)
{
    const int HW = a.W * a.H;
    sgm_with_nv(a.Dp, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        sgm_launch(s, k_sgm_select<NV, SgmV>, k_sgm_select<NV, SgmT>, dim3((HW + 3) / 4), dim3(256), a, q, 1);
    });
    sgm_launch(s, k_sgm_check<SgmV>, k_sgm_check<SgmT>, dim3((HW + 255) / 256), dim3(256), a, q, 1);
}

// ---- the 8-bit maps of both views from S (psm_sgm_select_maps, tests/sgm_maps_model.py) -----------------------------------------
//   left   lmap[y][x]  = dmin + argmin_k S[y][x][k], lowest k: k_sgm_select's `best`, nothing else of it
//   right  rmap[y][xr] = dmin + k of the smallest (S[y][xr + dmin + k][k], k) over the k with xr + dmin + k < W; 0 where there is none
// The right view's candidates lie on a diagonal of S (stride Dp + 1 elements): gathered, a wave would touch 64 cache lines for 64
// values.  S is read as k_sgm_select reads it instead - a pixel's disparities across the lanes of a wave - and the minimum is
// SCATTERED: a workgroup owns one image row, holds the row's right keys in LDS (4 W bytes, all ones to begin with), and for
// every left pixel x each lane takes the LDS minimum (ds_min_u32, no return value) of (S << 8 | k) into slot x - dmin - k.
// Minima commute: the keys do not depend on the order the waves arrive in.  The wave minimum of the same keys is the left map's
// entry; it waits in LDS too (W bytes), and after a barrier the workgroup writes both rows of bytes coalesced.  S is read once.
// Lane l holds the NV indices l, l + 64, .. (NV dword loads of 256 contiguous bytes each), not NV adjacent ones: the 64 lanes of
// one LDS instruction then go to 64 consecutive slots, and the 32 lanes the LDS serves together to 32 different banks (bank =
// dword address mod 32).  With adjacent indices per lane the lanes of an instruction would lie NV slots apart - 2 or 4 lanes
// per bank.  KB is 8: the call exists up to 256 disparities (S < 2^19: a key has 27 bits and never equals the all-ones start).
// The waves of a workgroup take every SGM_MAPS_WAVES-th pixel of the row, U pixels' loads issued ahead of their minima.
constexpr int SGM_MAPS_WAVES = 8, SGM_MAPS_U = 4;

template <int NV>
__device__ __forceinline__ void sgm_maps(const SgmRun &a, uint8_t *maps)
{
    extern __shared__ unsigned sgm_maps_lds[];
    unsigned *rkey = sgm_maps_lds;                                 // [W] the right view's packed minima
    uint8_t *lrow = (uint8_t *)(rkey + a.W);                       // [W] the left map's row
    const int y = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < a.W; i += SGM_MAPS_WAVES * 64) rkey[i] = 0xffffffffu;
    __syncthreads();
    const unsigned *Srow = a.S + (size_t)y * a.W * a.Dp;
    for (int x0 = wave; x0 < a.W; x0 += SGM_MAPS_WAVES * SGM_MAPS_U) {      // (wave-uniform)
        // The body has no branch, so that the compiler waits for exactly the loads a pixel needs (k_sgm_path above): what takes no
        // part - a lane past D, a landing column left of the image, a pixel past the row's end - loads a clamped address and
        // brings the all-ones key, which changes no minimum, to a slot inside the row.
        unsigned s[SGM_MAPS_U][NV];
#pragma unroll
        for (int u = 0; u < SGM_MAPS_U; ++u) {
            const unsigned *Sp = Srow + (size_t)min(x0 + u * SGM_MAPS_WAVES, a.W - 1) * a.Dp;
#pragma unroll
            for (int j = 0; j < NV; ++j) s[u][j] = Sp[min(j * 64 + lane, a.Dp - 1)];
        }
        int lv = 0;                                                // lane u: the left map's entry of pixel u
#pragma unroll
        for (int u = 0; u < SGM_MAPS_U; ++u) {
            const int x = x0 + u * SGM_MAPS_WAVES;
            int lkey = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int k = j * 64 + lane;
                const bool real = k < a.D && x < a.W;              // (the padding elements of Dp take no part)
                const unsigned key = (s[u][j] << 8) | (unsigned)k;
                lkey = min(lkey, real ? (int)key : 0x7fffffff);
                const int xr = x - a.dmin - k;                     // the landing column: < W for a real key, as dmin, k >= 0
                atomicMin(rkey + min(xr >= 0 ? xr : -xr - 1, a.W - 1), real && xr >= 0 ? key : 0xffffffffu);
            }
            const int kmin = sgm_wave_min(lkey);
            lv = lane == u ? a.dmin + (kmin & 255) : lv;
        }
        const int xl = x0 + lane * SGM_MAPS_WAVES;
        if (lane < SGM_MAPS_U && xl < a.W) lrow[xl] = (uint8_t)lv;
    }
    __syncthreads();
    uint8_t *lo = maps + (size_t)y * a.W, *ro = lo + (size_t)a.W * a.H;
    for (int i = threadIdx.x; i < a.W; i += SGM_MAPS_WAVES * 64) {
        const unsigned k = rkey[i];
        lo[i] = lrow[i];
        ro[i] = k == 0xffffffffu ? (uint8_t)0 : (uint8_t)(a.dmin + (int)(k & 255u));
    }
}

template <int NV, typename S>
__global__ __launch_bounds__(SGM_MAPS_WAVES * 64) void k_sgm_maps(SgmArgs a, S src)
{
    const SgmRun r = sgm_run(src, a, blockIdx.z);
    sgm_maps<NV>(r, r.maps);
}

size_t sgm_maps_lds_bytes(int W) { return (size_t)W * 5; }

// one workgroup per image row, the pair on grid axis z
void launch_sgm_maps(hipStream_t s, const SgmArgs &a, const Recs<SgmPair> &q)
{
    const dim3 block(SGM_MAPS_WAVES * 64);
    const size_t lds = sgm_maps_lds_bytes(a.W);
    auto go = [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        rec_launch(s, k_sgm_maps<NV, SgmV>, k_sgm_maps<NV, SgmT>, dim3(a.H, 1, q.n), block, lds, a, q);
    };
    if (a.Dp <= 64) go(std::integral_constant<int, 1>{});
    else if (a.Dp <= 128) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 4>{});
}

}  // namespace psm
