// psm_wls.hip - edge-aware WLS smoothing of an int16 disparity map in 16ths on the device (psm_wls_filter, psm_api_wls.cpp): the
// confidence-weighted global smoothing of cv::ximgproc::DisparityWLSFilter's kind by Min et al.'s Fast Global Smoother -
// separable tridiagonal solves along rows and columns, guided by the left image.  It follows no library's convention: the
// definition is tests/wls_model.py, the device equals it in every bit.  fp32, every operation rounded on its own
// (the file is built without contraction), IEEE division, subnormals kept.
// Launches, whatever the data - 1 + 2 T of them, for one pair or for the pairs of a batch (the same kernels, the member on grid
// axis y, its record - pointers, table, the lambdas of its passes - by value or in a device table):
//   k_wls_init  one pixel per lane: num and den from the source map, the link indices kh and kv from the guide
//   k_wls_rows  one pass over every row.  One lane owns one line and walks it, a wave holds WLS_LINES lines.  Lanes a row pitch
//               apart would fetch a cache line per lane and step, so the WLS_LINES x WLS_STEPS tiles travel through LDS: the four
//               waves of the workgroup load them with the lane as x and store them the same way, the first wave reads and
//               writes them transposed, the lane as the row (WLS_PITCH: free of bank conflicts).  The forward sweep leaves
//               cp, np, dp in the scratch planes, the back sweep takes the tiles in reverse and writes num and den
//   k_wls_cols  one pass over every column: the lane is x, so its walk is coalesced as it stands; the loads of WLS_CHUNK steps are
//               in flight ahead of the chain.  The last one forms the quotient, the int16 map and the float plane in its back sweep
// No atomics, no workgroup waits for another (the order between the launches is the stream's), no scratch memory.  The chain of a
// step - multiply, subtract, divide, multiply - is the definition's and is not reordered.
#include "psm_kernels.h"

namespace psm {

// one step of the forward sweep: am = a[n] (the c of the step before; 0 at n = 0), c = c[n] (0 at n = N - 1); cp, np, dp arrive as
// those of n - 1 (0 at n = 0: the products are +0 and the differences the definition's b[0] and num[0]) and leave as those of n
__device__ __forceinline__ void wls_forward(float am, float c, float v, float d, float &cp, float &np, float &dp)
{
    const float b = __fsub_rn(__fsub_rn(1.0f, am), c);
    const float m = __fsub_rn(b, __fmul_rn(cp, am));
    const float r = __fdiv_rn(1.0f, m);
    cp = __fmul_rn(c, r);
    np = __fmul_rn(__fsub_rn(v, __fmul_rn(np, am)), r);
    dp = __fmul_rn(__fsub_rn(d, __fmul_rn(dp, am)), r);
}

// The record of a workgroup from either source S (psm_kernels.h, Recs) - a single call's by value, or member blockIdx.y of a batch's
// device table - with the pointers in it read as global ones.  The index is uniform, so the record arrives through scalar loads
// ahead of the body.
template <typename S>
__device__ __forceinline__ WlsArgs wls_pair(const S &src)
{
    const WlsArgs &p = rec(src, blockIdx.y).a;
    WlsArgs a = p;
    a.map = sgm_global(p.map); a.valid = sgm_global(p.valid); a.d16 = sgm_global(p.d16); a.img = sgm_global(p.img);
    a.num = sgm_global(p.num); a.den = sgm_global(p.den); a.cp = sgm_global(p.cp); a.np = sgm_global(p.np); a.dp = sgm_global(p.dp);
    a.kh = sgm_global(p.kh); a.kv = sgm_global(p.kv); a.tab = sgm_global(p.tab); a.out = sgm_global(p.out); a.q = sgm_global(p.q);
    return a;
}

__device__ __forceinline__ void wls_init(WlsArgs a)
{
    const size_t N = (size_t)a.W * a.H, i = (size_t)blockIdx.x * WLS_TILE + threadIdx.x;
    if (i >= N) return;
    const int y = (int)(i / a.W), x = (int)(i - (size_t)y * a.W);
    int v;
    bool valid;
    if (a.source == WLS_GIF) {
        v = (int)a.map[i] * 16;
        valid = !(a.valid && a.valid[i] == 0);
    } else {
        v = a.d16[i];
        valid = v != a.invalid;
    }
    a.num[i] = valid ? (float)v : 0.0f;
    a.den[i] = valid ? 1.0f : 0.0f;
    const unsigned g = sgm_px(a.img, a.depth, a.ch, i);
    const unsigned gr = x < a.W - 1 ? sgm_px(a.img, a.depth, a.ch, i + 1) : g;
    const unsigned gd = y < a.H - 1 ? sgm_px(a.img, a.depth, a.ch, i + a.W) : g;
    int kh = 0, kv = 0;
    for (int k = 0; k < a.ch; ++k) {
        const int p = (g >> (8 * k)) & 255;
        kh = max(kh, abs(p - (int)((gr >> (8 * k)) & 255)));
        kv = max(kv, abs(p - (int)((gd >> (8 * k)) & 255)));
    }
    a.kh[i] = (uint8_t)kh;
    a.kv[i] = (uint8_t)kv;
}

// The tile of the rows y0 .. y0 + WLS_LINES and the columns x0 .. x0 + WLS_STEPS between three global planes and the three LDS
// planes, the lane as x: wave w moves the rows w, w + 4, ...  load: plane 2 is formed from the link indices as lw = lam * tab[kh].
// All global loads of a thread are issued before the first LDS write, so a tile costs one trip to memory, not one per row; rows
// below the image repeat its last row (nobody reads their lines).
template <bool LOAD, bool LINKS>
__device__ __forceinline__ void wls_tile_move(float (*sh)[WLS_LINES * WLS_PITCH], const float *tab, float lam, float *p0, float *p1, float *p2,
                                              const uint8_t *kh, int W, int H, int y0, int x0)
{
    constexpr int WAVES = WLS_ROW_THREADS / 64, ROWS = WLS_LINES / WAVES;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, x = x0 + lane;
    if (x >= W) return;
    if (LOAD) {
        float r0[ROWS], r1[ROWS], r2[ROWS];
        unsigned k[ROWS];
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            const size_t i = (size_t)min(y0 + w + q * WAVES, H - 1) * W + x;
            r0[q] = p0[i];
            r1[q] = p1[i];
            if (LINKS) k[q] = kh[i];
            else r2[q] = p2[i];
        }
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            const int s = (w + q * WAVES) * WLS_PITCH + lane;
            sh[0][s] = r0[q];
            sh[1][s] = r1[q];
            sh[2][s] = LINKS ? __fmul_rn(lam, tab[k[q]]) : r2[q];
        }
    } else {
        for (int r = w; r < WLS_LINES; r += WAVES) {
            const int y = y0 + r;
            if (y >= H) break;
            const size_t i = (size_t)y * W + x;
            const int s = r * WLS_PITCH + lane;
            p0[i] = sh[0][s];
            p1[i] = sh[1][s];
            if (p2) p2[i] = sh[2][s];
        }
    }
}

__device__ __forceinline__ void wls_rows(WlsArgs a, float lam)
{
    __shared__ float sh[3][WLS_LINES * WLS_PITCH];
    __shared__ float tab[256];
    const int W = a.W, H = a.H, y0 = blockIdx.x * WLS_LINES;
    const int lane = threadIdx.x & 63;
    const bool walker = threadIdx.x < 64 && y0 + lane < H;      // the first wave: lane = row
    const int tiles = (W + WLS_STEPS - 1) / WLS_STEPS;
    float *const line = &sh[0][0] + lane * WLS_PITCH;
    constexpr int PLANE = WLS_LINES * WLS_PITCH;
    tab[threadIdx.x] = a.tab[threadIdx.x];
    __syncthreads();

    // ---- forward: num, den, lw -> np, dp, cp ----
    float am = 0.0f, cp = 0.0f, np = 0.0f, dp = 0.0f;
    for (int t = 0; t < tiles; ++t) {
        const int x0 = t * WLS_STEPS, n = min(WLS_STEPS, W - x0);
        wls_tile_move<true, true>(sh, tab, lam, a.num, a.den, nullptr, a.kh, W, H, y0, x0);
        __syncthreads();
        if (walker) {
            // WLS_CHUNK steps at a time: their LDS reads ahead of the chain, their writes behind it
            for (int j0 = 0; j0 < n; j0 += WLS_CHUNK) {
                float v[WLS_CHUNK], d[WLS_CHUNK], l[WLS_CHUNK];
#pragma unroll
                for (int k = 0; k < WLS_CHUNK; ++k) {
                    const int j = min(j0 + k, WLS_STEPS - 1);
                    v[k] = line[j]; d[k] = line[PLANE + j]; l[k] = line[2 * PLANE + j];
                }
#pragma unroll
                for (int k = 0; k < WLS_CHUNK; ++k) {
                    if (j0 + k < n) {
                        const float c = x0 + j0 + k < W - 1 ? -l[k] : 0.0f;
                        wls_forward(am, c, v[k], d[k], cp, np, dp);
                        v[k] = np; d[k] = dp; l[k] = cp;
                        am = c;
                    }
                }
#pragma unroll
                for (int k = 0; k < WLS_CHUNK; ++k) {
                    if (j0 + k < n) {
                        const int j = j0 + k;
                        line[j] = v[k]; line[PLANE + j] = d[k]; line[2 * PLANE + j] = l[k];
                    }
                }
            }
        }
        __syncthreads();
        wls_tile_move<false, false>(sh, tab, lam, a.np, a.dp, a.cp, nullptr, W, H, y0, x0);
        __syncthreads();
    }

    // ---- back: np, dp, cp -> num, den ----
    float un = 0.0f, ud = 0.0f;
    for (int t = tiles - 1; t >= 0; --t) {
        const int x0 = t * WLS_STEPS, n = min(WLS_STEPS, W - x0);
        wls_tile_move<true, false>(sh, tab, lam, a.np, a.dp, a.cp, nullptr, W, H, y0, x0);
        __syncthreads();
        if (walker) {
            for (int j0 = ((n - 1) / WLS_CHUNK) * WLS_CHUNK; j0 >= 0; j0 -= WLS_CHUNK) {
                float v[WLS_CHUNK], d[WLS_CHUNK], l[WLS_CHUNK];
#pragma unroll
                for (int k = 0; k < WLS_CHUNK; ++k) {
                    const int j = min(j0 + k, WLS_STEPS - 1);
                    v[k] = line[j]; d[k] = line[PLANE + j]; l[k] = line[2 * PLANE + j];
                }
#pragma unroll
                for (int k = WLS_CHUNK - 1; k >= 0; --k) {
                    if (j0 + k < n) {
                        if (x0 + j0 + k == W - 1) {
                            un = v[k];
                            ud = d[k];
                        } else {
                            un = __fsub_rn(v[k], __fmul_rn(l[k], un));
                            ud = __fsub_rn(d[k], __fmul_rn(l[k], ud));
                        }
                        v[k] = un; d[k] = ud;
                    }
                }
#pragma unroll
                for (int k = 0; k < WLS_CHUNK; ++k) {
                    if (j0 + k < n) {
                        line[j0 + k] = v[k]; line[PLANE + j0 + k] = d[k];
                    }
                }
            }
        }
        __syncthreads();
        wls_tile_move<false, false>(sh, tab, lam, a.num, a.den, nullptr, nullptr, W, H, y0, x0);
        __syncthreads();
    }
}

// WLS_CHUNK steps of a column's forward sweep from row y0; FULL: all of them lie inside the image (no step is conditional, so the
// table look-ups stay ahead of the chain)
template <bool FULL>
__device__ __forceinline__ void wls_cols_forward(const WlsArgs &a, const float *tab, float lam, int x, int y0, const float (&v)[WLS_CHUNK],
                                                 const float (&d)[WLS_CHUNK], const unsigned (&k)[WLS_CHUNK], float &am, float &cp, float &np, float &dp)
{
    const int W = a.W, H = a.H;
    float lw[WLS_CHUNK];
#pragma unroll
    for (int j = 0; j < WLS_CHUNK; ++j) lw[j] = __fmul_rn(lam, tab[k[j]]);
#pragma unroll
    for (int j = 0; j < WLS_CHUNK; ++j) {
        const int y = y0 + j;
        if (FULL || y < H) {
            const float c = y < H - 1 ? -lw[j] : 0.0f;
            wls_forward(am, c, v[j], d[j], cp, np, dp);
            const size_t i = (size_t)y * W + x;
            a.cp[i] = cp; a.np[i] = np; a.dp[i] = dp;
            am = c;
        }
    }
}

__device__ __forceinline__ bool wls_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void wls_cols(WlsArgs a, float lam, int last)
{
    __shared__ float tab[256];
    const int W = a.W, H = a.H, x = blockIdx.x * WLS_LINES + threadIdx.x;
    for (int k = threadIdx.x; k < 256; k += WLS_LINES) tab[k] = a.tab[k];
    __syncthreads();
    if (x >= W) return;

    // ---- forward: the loads of the next WLS_CHUNK steps are issued ahead of this chunk's chain ----
    float v[WLS_CHUNK], d[WLS_CHUNK], v2[WLS_CHUNK], d2[WLS_CHUNK];
    unsigned k[WLS_CHUNK], k2[WLS_CHUNK];
#pragma unroll
    for (int j = 0; j < WLS_CHUNK; ++j) {
        const size_t i = (size_t)min(j, H - 1) * W + x;
        v[j] = a.num[i]; d[j] = a.den[i]; k[j] = a.kv[i];
    }
    float am = 0.0f, cp = 0.0f, np = 0.0f, dp = 0.0f;
    for (int y0 = 0; y0 < H; y0 += WLS_CHUNK) {
#pragma unroll
        for (int j = 0; j < WLS_CHUNK; ++j) {
            const size_t i = (size_t)min(y0 + WLS_CHUNK + j, H - 1) * W + x;
            v2[j] = a.num[i]; d2[j] = a.den[i]; k2[j] = a.kv[i];
        }
        if (y0 + WLS_CHUNK <= H) wls_cols_forward<true>(a, tab, lam, x, y0, v, d, k, am, cp, np, dp);
        else wls_cols_forward<false>(a, tab, lam, x, y0, v, d, k, am, cp, np, dp);
#pragma unroll
        for (int j = 0; j < WLS_CHUNK; ++j) { v[j] = v2[j]; d[j] = d2[j]; k[j] = k2[j]; }
    }

    // ---- back: the same with cp, np, dp, from the last row upwards ----
    const float lo = (float)(a.invalid + 1);
    float c1[WLS_CHUNK], c2[WLS_CHUNK];
    const int top = ((H - 1) / WLS_CHUNK) * WLS_CHUNK;      // the first row of the last chunk
#pragma unroll
    for (int j = 0; j < WLS_CHUNK; ++j) {
        const size_t i = (size_t)min(top + j, H - 1) * W + x;
        v[j] = a.np[i]; d[j] = a.dp[i]; c1[j] = a.cp[i];
    }
    float un = 0.0f, ud = 0.0f;
    for (int y0 = top; y0 >= 0; y0 -= WLS_CHUNK) {
#pragma unroll
        for (int j = 0; j < WLS_CHUNK; ++j) {
            const size_t i = (size_t)max(y0 - WLS_CHUNK + j, 0) * W + x;
            v2[j] = a.np[i]; d2[j] = a.dp[i]; c2[j] = a.cp[i];
        }
#pragma unroll
        for (int j = WLS_CHUNK - 1; j >= 0; --j) {
            const int y = y0 + j;
            if (y < H) {
                if (y == H - 1) {
                    un = v[j];
                    ud = d[j];
                } else {
                    un = __fsub_rn(v[j], __fmul_rn(c1[j], un));
                    ud = __fsub_rn(d[j], __fmul_rn(c1[j], ud));
                }
                const size_t i = (size_t)y * W + x;
                a.num[i] = un; a.den[i] = ud;
                if (last) {
                    const float q = __fdiv_rn(un, ud);
                    const bool good = ud >= 0x1p-64f && wls_finite(q);
                    a.q[i] = good ? __float_as_uint(q) : WLS_VOID;
                    a.out[i] = good ? (int16_t)(int)fminf(fmaxf(rintf(q), lo), 32767.0f) : (int16_t)a.invalid;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < WLS_CHUNK; ++j) { v[j] = v2[j]; d[j] = d2[j]; c1[j] = c2[j]; }
    }
}

// The lambda of pass t is the record's own lam[t]: every member of a batch has its own lambda and sigma.
template <typename S> __global__ __launch_bounds__(WLS_TILE) void k_wls_init(S src) { wls_init(wls_pair(src)); }
template <typename S>
__global__ __launch_bounds__(WLS_ROW_THREADS) void k_wls_rows(S src, int t) { wls_rows(wls_pair(src), rec(src, blockIdx.y).lam[t]); }
template <typename S>
__global__ __launch_bounds__(WLS_LINES) void k_wls_cols(S src, int t, int last) { wls_cols(wls_pair(src), rec(src, blockIdx.y).lam[t], last); }

using WlsV = RecVal<WlsPair>;
using WlsT = RecTab<WlsPair>;

void launch_wls_init(hipStream_t s, const Recs<WlsPair> &q)
{
    const WlsArgs &a = q.host[0].a;
    const unsigned blocks = (unsigned)(((size_t)a.W * a.H + WLS_TILE - 1) / WLS_TILE);
    rec_launch(s, k_wls_init<WlsV>, k_wls_init<WlsT>, dim3(blocks, (unsigned)q.n), dim3(WLS_TILE), 0, q);
}

void launch_wls_rows(hipStream_t s, const Recs<WlsPair> &q, int t)
{
    rec_launch(s, k_wls_rows<WlsV>, k_wls_rows<WlsT>, dim3((unsigned)wls_groups(q.host[0].a.H), (unsigned)q.n), dim3(WLS_ROW_THREADS), 0, q, t);
}

void launch_wls_cols(hipStream_t s, const Recs<WlsPair> &q, int t, bool last)
{
    rec_launch(s, k_wls_cols<WlsV>, k_wls_cols<WlsT>, dim3((unsigned)wls_groups(q.host[0].a.W), (unsigned)q.n), dim3(WLS_LINES), 0, q, t, last ? 1 : 0);
}

}  // namespace psm
