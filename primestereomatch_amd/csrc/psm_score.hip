// psm_score.hip - the last steps of StereoMatch::compute on the device (psm_score, psm_api_score.cpp): the display conversion of the
// maps (src/StereoMatch.cpp:181-185 for STEREO_SGBM, :248-249 for STEREO_GIF) and the error metric against ground truth (:275-309).
// All integer, or IEEE operations with one defined rounding; the definition is tests/score_model.py, the device
// equals it element for element and counter for counter.
//   k_sc_minmax         minMaxLoc of the int16 map: per-wave minimum / maximum, one atomicMin / atomicMax per wave
//   k_sc_score<source>  one pass: display value(s) of 4 adjacent pixels per lane, |display - gt|, the left columns, the threshold,
//                       the mask multiply; display and error planes out, `bad` and `err_sum` reduced per wave, one atomicAdd each
// The SGM source forms alpha = (float)(255.0 / (max - min)) from the counters k_sc_minmax left: no host round trip in between.
#include "psm_kernels.h"

namespace psm {

// DPP row_shr:n (0x110 + n) with `old` for the lanes that have no source, as psm_sgm.hip's sgm_dpp
template <int CTRL>
__device__ __forceinline__ int sc_dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false); }

// Over the wave, in every lane: four row_shr steps leave a row's result in its lane 15, the four rows meet in SGPRs.  Every lane of
// the wave must be active (the callers keep lanes without work alive with the identity).
__device__ __forceinline__ int sc_wave_min(int v)
{
    v = min(v, sc_dpp<0x111>(0x7fffffff, v));
    v = min(v, sc_dpp<0x112>(0x7fffffff, v));
    v = min(v, sc_dpp<0x114>(0x7fffffff, v));
    v = min(v, sc_dpp<0x118>(0x7fffffff, v));
    return min(min(__builtin_amdgcn_readlane(v, 15), __builtin_amdgcn_readlane(v, 31)),
               min(__builtin_amdgcn_readlane(v, 47), __builtin_amdgcn_readlane(v, 63)));
}
__device__ __forceinline__ int sc_wave_max(int v) { return -sc_wave_min(-v); }      // (callers stay inside +-2^31 - 1)
__device__ __forceinline__ int sc_wave_sum(int v)
{
    v += sc_dpp<0x111>(0, v);
    v += sc_dpp<0x112>(0, v);
    v += sc_dpp<0x114>(0, v);
    v += sc_dpp<0x118>(0, v);
    return __builtin_amdgcn_readlane(v, 15) + __builtin_amdgcn_readlane(v, 31) + __builtin_amdgcn_readlane(v, 47) +
           __builtin_amdgcn_readlane(v, 63);
}

// What a body takes: the call's scalars and the pointers of one pair, read as global ones, from either record source S
// (psm_kernels.h, Recs) - a single call's pair by value, or pair blockIdx.y of a batch's device table
struct ScRun : ScArgs, ScPair {};
template <typename S>
__device__ __forceinline__ ScRun sc_run(const S &src, const ScArgs &a, unsigned pair)
{
    const ScPair &p = rec(src, pair);
    ScRun r;
    static_cast<ScArgs &>(r) = a;
    r.maps = sgm_global(p.maps); r.d16 = sgm_global(p.d16); r.gt = sgm_global(p.gt); r.mask = sgm_global(p.mask);
    r.planes = sgm_global(p.planes); r.cnt = sgm_global(p.cnt);
    return r;
}

// ---- k_sc_minmax: the map is one run of W H int16 values on an 8-byte boundary; a lane takes 4 of them per step ----
__device__ __forceinline__ void sc_minmax(const ScRun &a)
{
    const int n = a.W * a.H, n4 = n >> 2;
    int mn = 0x7fff, mx = -0x8000;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int2 q = ((const int2 *)a.d16)[i];
        const int v0 = (short)(q.x & 0xffff), v1 = q.x >> 16, v2 = (short)(q.y & 0xffff), v3 = q.y >> 16;
        mn = min(mn, min(min(v0, v1), min(v2, v3)));
        mx = max(mx, max(max(v0, v1), max(v2, v3)));
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < n - 4 * n4) {
        const int v = a.d16[4 * n4 + threadIdx.x];
        mn = min(mn, v);
        mx = max(mx, v);
    }
    mn = sc_wave_min(mn);
    mx = sc_wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&a.cnt->mn, mn - SC_MN_BIAS);
        atomicMax(&a.cnt->mx, mx + SC_MX_BIAS);
    }
}

template <typename S> __global__ __launch_bounds__(256) void k_sc_minmax(ScArgs a, S src) { sc_minmax(sc_run(src, a, blockIdx.y)); }

// ---- k_sc_score ----
// n (1..4) bytes at p as one dword, byte k the pixel x + k.  Rows are W bytes long, so p sits on no particular boundary: the whole
// group goes as one dword access through memcpy (the target reads global memory at any alignment), a row's last, shorter group
// byte by byte - nothing past the plane's end is touched.
__device__ __forceinline__ unsigned sc_load4(const uint8_t *p, int n)
{
    unsigned v = 0;
    if (n == 4) __builtin_memcpy(&v, p, 4);
    else for (int k = 0; k < n; ++k) v |= (unsigned)p[k] << (8 * k);
    return v;
}
__device__ __forceinline__ void sc_store4(uint8_t *p, unsigned v, int n)
{
    if (n == 4) __builtin_memcpy(p, &v, 4);
    else for (int k = 0; k < n; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
__device__ __forceinline__ void sc_load4x16(const int16_t *p, int n, int v[4])
{
    v[0] = v[1] = v[2] = v[3] = 0;
    if (n == 4) {
        int2 q;
        __builtin_memcpy(&q, p, 8);
        v[0] = (short)(q.x & 0xffff); v[1] = q.x >> 16; v[2] = (short)(q.y & 0xffff); v[3] = q.y >> 16;
    } else for (int k = 0; k < n; ++k) v[k] = p[k];
}
__device__ __forceinline__ int sc_sat_u8(float r) { return (int)fminf(fmaxf(r, 0.0f), 255.0f); }
// convertTo(CV_8U, scale_factor) of an 8-bit value
__device__ __forceinline__ unsigned sc_scale(unsigned v, int scale) { return min(v * (unsigned)scale, 255u); }
__device__ __forceinline__ unsigned sc_scale4(unsigned v, int scale)
{
    return sc_scale(v & 255u, scale) | sc_scale((v >> 8) & 255u, scale) << 8 | sc_scale((v >> 16) & 255u, scale) << 16 |
           sc_scale(v >> 24, scale) << 24;
}

// One lane per 4 adjacent pixels of a row, ceil(W / 4) lanes per row, the rows one behind the other.
template <int SRC>
__device__ __forceinline__ void sc_score(const ScRun &a)
{
    const int G = (a.W + 3) >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    int bad = 0, sum = 0;
    if (t < G * a.H) {
        const int y = t / G, x = (t - y * G) * 4;
        const int n = min(4, a.W - x);
        const size_t HW = (size_t)a.W * a.H, at = (size_t)y * a.W + x;
        unsigned p;
        if (SRC == SC_GIF) {
            p = sc_scale4(sc_load4(a.maps + at, n), a.scale);
            sc_store4(a.planes + HW + at, sc_scale4(sc_load4(a.maps + HW + at, n), a.scale), n);
        } else {
            int v[4];
            sc_load4x16(a.d16 + at, n, v);
            p = 0;
            if (SRC == SC_SGM) {
                // convertTo(CV_8U, 255 / (maxVal - minVal)) multiplies in fp32 by the factor formed in fp64; Mat / 4 is convertTo(CV_8U,
                // 0.25); both round to nearest even and saturate.  A flat map has no factor: alpha 0, an all-zero display.
                const int mn = a.cnt->mn + SC_MN_BIAS, mx = a.cnt->mx - SC_MX_BIAS;
                const float alpha = mx == mn ? 0.0f : (float)(255.0 / ((double)mx - (double)mn));
                for (int k = 0; k < 4; ++k) {
                    const int m = sc_sat_u8(rintf(__fmul_rn((float)v[k], alpha)));
                    const int q = sc_sat_u8(rintf(__fmul_rn((float)m, 0.25f)));
                    p |= sc_scale((unsigned)q, a.scale) << (8 * k);
                }
            } else {
                for (int k = 0; k < 4; ++k) p |= sc_scale((unsigned)min(max(v[k], 0) >> 4, 255), a.scale) << (8 * k);
            }
        }
        sc_store4(a.planes + at, p, n);
        unsigned e4 = 0;
        if (a.gt) {
            const unsigned g = sc_load4(a.gt + at, n), m = a.mask ? sc_load4(a.mask + at, n) : 0u;
            constexpr double INV255 = (double)(1.0f / 255.0f);      // eDispMap.mul(errMask, 1 / 255.f): the factor is a float
            for (int k = 0; k < n; ++k) {
                int e = abs((int)((p >> (8 * k)) & 255u) - (int)((g >> (8 * k)) & 255u));
                if (x + k <= a.D || e <= a.thr) e = 0;
                if (a.mask) {
                    int w = (int)((m >> (8 * k)) & 255u);
                    if (a.disc && w <= 254) w = 0;
                    e = (int)fmin(fmax(rint(__dmul_rn((double)(e * w), INV255)), 0.0), 255.0);
                }
                e4 |= (unsigned)e << (8 * k);
                bad += e != 0;
                sum += e;
            }
        }
        sc_store4(a.planes + 2 * HW + at, e4, n);
    }
    // (every lane of the workgroup arrives here: 4 pixels of at most 255 each per lane, 65280 per wave)
    bad = sc_wave_sum(bad);
    sum = sc_wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && bad) {
        atomicAdd(&a.cnt->bad, (unsigned)bad);
        atomicAdd(&a.cnt->sum, (unsigned long long)sum);
    }
}

template <int SRC, typename S> __global__ __launch_bounds__(256) void k_sc_score(ScArgs a, S src) { sc_score<SRC>(sc_run(src, a, blockIdx.y)); }

using ScV = RecVal<ScPair>;
using ScT = RecTab<ScPair>;

void launch_sc_minmax(hipStream_t s, const ScArgs &a, const Recs<ScPair> &q)
{
    const int n4 = (a.W * a.H) >> 2, blocks = (n4 + 255) / 256;
    rec_launch(s, k_sc_minmax<ScV>, k_sc_minmax<ScT>, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)q.n), dim3(256), 0, a, q);      // (a lane of a large map takes several steps)
}

void launch_sc_score(hipStream_t s, int source, const ScArgs &a, const Recs<ScPair> &q)
{
    const dim3 grid((unsigned)((((a.W + 3) >> 2) * a.H + 255) / 256), (unsigned)q.n), block(256);
    switch (source) {
    case SC_GIF: rec_launch(s, k_sc_score<SC_GIF, ScV>, k_sc_score<SC_GIF, ScT>, grid, block, 0, a, q); break;
    case SC_SGM: rec_launch(s, k_sc_score<SC_SGM, ScV>, k_sc_score<SC_SGM, ScT>, grid, block, 0, a, q); break;
    default: rec_launch(s, k_sc_score<SC_SGM_INT, ScV>, k_sc_score<SC_SGM_INT, ScT>, grid, block, 0, a, q); break;
    }
}

}  // namespace psm
