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
// Under PSM_WLS_CONFIDENCE two launches lie ahead of them - k_sgm_right16, k_wls_conf (below: the graded confidence of
// tests/wls_conf_model.py) - and k_wls_init starts with num = conf * v, den = conf.
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
    a.conf = sgm_global(p.conf);
    return a;
}
template <typename S>
__device__ __forceinline__ WlsConf wls_conf_of(const S &src)
{
    const WlsConf &p = rec(src, blockIdx.y).c;
    WlsConf c = p;
    c.S = sgm_global(p.S); c.r16 = sgm_global(p.r16); c.conf = sgm_global(p.conf);
    return c;
}

// ---- PSM_WLS_CONFIDENCE: the two launches ahead of k_wls_init (tests/wls_conf_model.py) -----------------------------
//   k_sgm_right16  the right view's sub-pixel map in 16ths from S, built the way k_sgm_maps is (psm_sgm.hip): a workgroup owns one
//                  image row and holds the row's W right keys in LDS, all ones to begin with; S is read once, a pixel's
//                  disparities across the lanes of a wave (lane l holds the indices l, l + 64, ..: the 64 lanes of one LDS
//                  instruction go to 64 consecutive slots), and every lane takes the LDS minimum of (S << 10 | k) - 29 bits, as
//                  S < 2^19: never the all-ones start - into slot x - dmin - k.  The body has no branch: what takes no part (a lane
//                  past D, a landing column left OR right of the image - dmin may be negative -, a pixel past the row's end) loads
//                  a clamped address and brings the all-ones key to a mirrored, clamped slot inside the row.  After the barrier a
//                  thread takes right pixels: the neighbours Sm, Sp on the candidate's diagonal by two gathered loads of the row
//                  just read (L2), the sub-pixel step with k_sgm_select's expressions, one coalesced int16 store.
//   k_wls_conf     the confidence byte of every pixel: a tile of the int16 map with a halo of WLS_CONF_RMAX goes through LDS as
//                  dwords (an invalid or outside pixel as WLS_NONE); a wave is one row of the tile with the lane as x, so every
//                  LDS read of a wave is of 64 consecutive dwords.  Window sums in 64-bit integers, one 64-bit division per pixel.
// No atomics on global memory, no workgroup waits for another, no scratch memory.
constexpr int WLS_NONE = (int)0x80000000;

template <int NV>
__device__ __forceinline__ void sgm_right16(const WlsConf &c, int W, int y)
{
    extern __shared__ unsigned wls_r16_keys[];                     // [W] the right view's packed minima
    constexpr int U = NV > 4 ? 2 : 4;                              // pixels whose loads are issued ahead of their minima
    constexpr int T = WLS_R16_WAVES * 64;
    unsigned *rkey = wls_r16_keys;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < W; i += T) rkey[i] = 0xffffffffu;
    __syncthreads();
    const unsigned *Srow = c.S + (size_t)y * W * c.Dp;
    for (int x0 = wave; x0 < W; x0 += WLS_R16_WAVES * U) {         // (wave-uniform)
        unsigned s[U][NV];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned *Sp = Srow + (size_t)min(x0 + u * WLS_R16_WAVES, W - 1) * c.Dp;
#pragma unroll
            for (int j = 0; j < NV; ++j) s[u][j] = Sp[min(j * 64 + lane, c.Dp - 1)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int x = x0 + u * WLS_R16_WAVES;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int k = j * 64 + lane;
                const bool real = k < c.D && x < W;                // (the padding elements of Dp take no part)
                const unsigned key = (s[u][j] << 10) | (unsigned)k;
                const int xr = x - c.dmin - k;                     // the landing column: on either side of the image with dmin < 0
                const int xm = xr < 0 ? -xr - 1 : (xr >= W ? 2 * W - 1 - xr : xr);
                atomicMin(rkey + min(max(xm, 0), W - 1), real && xr >= 0 && xr < W ? key : 0xffffffffu);
            }
        }
    }
    __syncthreads();
    int16_t *out = c.r16 + (size_t)y * W;
    const int rinv = (c.dmin - 1) * 16;
    for (int i = threadIdx.x; i < W; i += T) {
        const unsigned key = rkey[i];
        const bool none = key == 0xffffffffu;
        const int k = (int)(key & 1023u), s0 = (int)(key >> 10), xl = i + c.dmin + k;
        const bool inner = k > 0 && k < c.D - 1 && xl - 1 >= 0 && xl + 1 < W;
        const int km = min(max(k - 1, 0), c.D - 1), kp = min(k + 1, c.D - 1);
        const int sm = (int)Srow[(size_t)min(max(xl - 1, 0), W - 1) * c.Dp + km];
        const int sp = (int)Srow[(size_t)min(max(xl + 1, 0), W - 1) * c.Dp + kp];
        const int den = max(sm + sp - 2 * s0, 1);
        const int num = (sm - sp) * 16 + den, dd = 2 * den;
        int q = num / dd;
        if (num % dd != 0 && num < 0) --q;                         // floor
        out[i] = (int16_t)(none ? rinv : (c.dmin + k) * 16 + (inner ? q : 0));
    }
}

template <int NV, typename S>
__global__ __launch_bounds__(WLS_R16_WAVES * 64) void k_sgm_right16(S src)
{
    const WlsConf c = wls_conf_of(src);
    if (!(c.terms & WLS_CONF_LR)) return;                          // (uniform: a member without the L-R term takes no part)
    sgm_right16<NV>(c, rec(src, blockIdx.y).a.W, blockIdx.x);
}

__device__ __forceinline__ void wls_conf(const WlsArgs &a, const WlsConf &c)
{
    constexpr int R = WLS_CONF_RMAX, LW = WLS_CONF_TX + 2 * R, LH = WLS_CONF_TY + 2 * R;
    __shared__ int tile[LH * LW];
    const int W = a.W, H = a.H, tx = (W + WLS_CONF_TX - 1) / WLS_CONF_TX;
    const int y0 = (int)(blockIdx.x / tx) * WLS_CONF_TY, x0 = (int)(blockIdx.x % tx) * WLS_CONF_TX;
    for (int e = threadIdx.x; e < LH * LW; e += WLS_CONF_TX * WLS_CONF_TY) {
        const int gy = y0 - R + e / LW, gx = x0 - R + e % LW;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const int v = a.d16[(size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)];
        tile[e] = inside && v != a.invalid ? v : WLS_NONE;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, row = threadIdx.x >> 6, x = x0 + lane, y = y0 + row;
    if (x >= W || y >= H) return;
    const int *centre = tile + (row + R) * LW + lane + R;
    const int v = *centre;
    const bool valid = v != WLS_NONE;
    unsigned cvar = 255, clr = 255;
    if (c.terms & WLS_CONF_VAR) {                                  // (uniform)
        unsigned n = 0;
        int s = 0;                                                 // |s| <= 81 * 2^15
        unsigned long long ss = 0;                                 // <= 81 * 2^30
        for (int dy = -c.radius; dy <= c.radius; ++dy)
            for (int dx = -c.radius; dx <= c.radius; ++dx) {
                const int t = centre[dy * LW + dx];
                const bool ok = t != WLS_NONE;
                n += ok ? 1u : 0u;
                s += ok ? t : 0;
                ss += ok ? (unsigned)(t * t) : 0u;
            }
        const unsigned long long m = (unsigned long long)n * ss - (unsigned long long)((long long)s * s);   // n ss >= s^2 (Cauchy-Schwarz)
        const unsigned long long den = max((unsigned long long)(n * n) << c.shift, 1ull);                   // (n = 0: the centre is invalid)
        cvar = 255u - (unsigned)min(255ull * m / den, 255ull);
    }
    if (c.terms & WLS_CONF_LR) {
        const int vv = valid ? v : 0, xq = x - ((vv + 8) >> 4);
        const int r = c.r16[(size_t)y * W + min(max(xq, 0), W - 1)];
        const bool ok = xq >= 0 && xq < W && r != (c.dmin - 1) * 16;
        clr = ok ? 255u - min((unsigned)abs(vv - r) * 255u / (unsigned)c.thresh, 255u) : 0u;
    }
    c.conf[(size_t)y * W + x] = (uint8_t)(valid ? (cvar * clr + 127u) / 255u : 0u);
}

template <typename S> __global__ __launch_bounds__(WLS_CONF_TX * WLS_CONF_TY) void k_wls_conf(S src) { wls_conf(wls_pair(src), wls_conf_of(src)); }

// CONF (PSM_WLS_CONFIDENCE, the SGM source): the start is weighted with the bytes of k_wls_conf, which are 0 in the invalid pixels -
// den = (float)conf, num = (float)conf * (float)v, one exact multiply.  The instantiation without it is the stage's as it ever was.
template <bool CONF>
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
    if (CONF) {
        const float c = (float)a.conf[i];
        a.num[i] = __fmul_rn(c, (float)v);
        a.den[i] = c;
    } else {
        a.num[i] = valid ? (float)v : 0.0f;
        a.den[i] = valid ? 1.0f : 0.0f;
    }
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
template <typename S> __global__ __launch_bounds__(WLS_TILE) void k_wls_init(S src) { wls_init<false>(wls_pair(src)); }
template <typename S> __global__ __launch_bounds__(WLS_TILE) void k_wls_init_conf(S src) { wls_init<true>(wls_pair(src)); }
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
    if (a.conf) rec_launch(s, k_wls_init_conf<WlsV>, k_wls_init_conf<WlsT>, dim3(blocks, (unsigned)q.n), dim3(WLS_TILE), 0, q);
    else rec_launch(s, k_wls_init<WlsV>, k_wls_init<WlsT>, dim3(blocks, (unsigned)q.n), dim3(WLS_TILE), 0, q);
}

void launch_sgm_right16(hipStream_t s, const Recs<WlsPair> &q, int dp_max)
{
    const WlsArgs &a = q.host[0].a;
    const dim3 grid((unsigned)a.H, (unsigned)q.n), block(WLS_R16_WAVES * 64);
    const size_t lds = (size_t)a.W * sizeof(unsigned);
    auto go = [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        rec_launch(s, k_sgm_right16<NV, WlsV>, k_sgm_right16<NV, WlsT>, grid, block, lds, q);
    };
    if (dp_max <= 64) go(std::integral_constant<int, 1>{});
    else if (dp_max <= 128) go(std::integral_constant<int, 2>{});
    else if (dp_max <= 256) go(std::integral_constant<int, 4>{});
    else if (dp_max <= 512) go(std::integral_constant<int, 8>{});
    else go(std::integral_constant<int, 16>{});
}

void launch_wls_conf(hipStream_t s, const Recs<WlsPair> &q)
{
    const WlsArgs &a = q.host[0].a;
    const unsigned tiles = (unsigned)((a.W + WLS_CONF_TX - 1) / WLS_CONF_TX) * (unsigned)((a.H + WLS_CONF_TY - 1) / WLS_CONF_TY);
    rec_launch(s, k_wls_conf<WlsV>, k_wls_conf<WlsT>, dim3(tiles, (unsigned)q.n), dim3(WLS_CONF_TX * WLS_CONF_TY), 0, q);
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
