// psm_depth.hip - from disparity to depth on the device (psm_reproject, psm_api_depth.cpp): cv::reprojectImageTo3D of the current
// result with the Q of cv::stereoRectify (the reference computes it at src/StereoMatch.cpp:456-458 and drops it), and the ordered,
// compacted, coloured point cloud.  fp64 with every product and sum rounded on its own; the definition is tests/depth_model.py
// (DESIGN.md 12), the device equals it in every bit.
// One pixel per lane, the pixels in raster order, DP_TILE of them per workgroup.  Three launches whatever the data:
//   k_dp_count  the point of every pixel; the dense planes if asked for; the keep predicate through __ballot and a popcount into
//               one count per tile
//   k_dp_scan   a single workgroup: the exclusive sums of the tiles' counts, and the total
//   k_dp_pack   the point again; a kept lane's slot is its tile's offset + the counts of the tile's earlier waves + the kept lanes
//               below it in its wave (mbcnt of the ballot); the record leaves as one 16-byte store
// No workgroup waits for another: the order between the launches is the stream's.  No atomics; every word of shared state is
// written by exactly one lane of one launch.
#include "psm_kernels.h"

namespace psm {

// The pair of a workgroup from either record source S (psm_kernels.h, Recs) - a single call's by value, or pair blockIdx.y of a batch's
// device table - with its pointers read as global ones
template <typename S>
__device__ __forceinline__ DpArgs dp_pair(const S &src)
{
    const DpArgs &p = rec(src, blockIdx.y);
    DpArgs a = p;
    a.map = sgm_global(p.map); a.valid = sgm_global(p.valid); a.d16 = sgm_global(p.d16); a.img = sgm_global(p.img);
    a.xyz = sgm_global(p.xyz); a.z = sgm_global(p.z); a.cloud = sgm_global(p.cloud);
    a.tile_cnt = sgm_global(p.tile_cnt); a.tile_off = sgm_global(p.tile_off); a.total = sgm_global(p.total);
    return a;
}

constexpr unsigned DP_VOID = 0x7FC00000u;              // what a void pixel holds in the dense planes: stored, never computed

struct DpPoint {
    unsigned b[3];                                     // the bit patterns of the stored floats
    bool keep;                                         // the pixel has a record in the cloud
};

__device__ __forceinline__ bool dp_finite(double v) { return ((unsigned)__double2hiint(v) & 0x7ff00000u) != 0x7ff00000u; }

// pixel i (in raster order) of the pair
__device__ __forceinline__ DpPoint dp_point(const DpArgs &a, const DpGeom &g, int i)
{
    const int y = i / g.W, x = i - y * g.W;
    double d;
    bool missing;
    if (g.source == DP_GIF) {
        d = (double)a.map[i];
        missing = a.valid && a.valid[i] == 0;
    } else {
        const int v = a.d16[i];
        d = __dmul_rn((double)v, 0.0625);
        missing = v == a.invalid;
    }
    const double xf = (double)(x + a.crop_x), yf = (double)(y + a.crop_y);
    double s[4];
    for (int k = 0; k < 4; ++k)
        s[k] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.Q[4 * k], xf), __dmul_rn(a.Q[4 * k + 1], yf)), __dmul_rn(a.Q[4 * k + 2], d)), a.Q[4 * k + 3]);
    const double r = 1.0 / s[3];                       // IEEE division: correctly rounded, +-inf for +-0
    bool isvoid = missing;
    float f[3];
    for (int k = 0; k < 3; ++k) {
        const double p = __dmul_rn(s[k], r);
        isvoid = isvoid || !dp_finite(p);
        f[k] = __double2float_rn(p);
    }
    DpPoint pt;
    for (int k = 0; k < 3; ++k) pt.b[k] = isvoid ? DP_VOID : __float_as_uint(f[k]);
    pt.keep = !isvoid && f[2] > a.z_min && f[2] <= a.z_max;
    return pt;
}

// the kept pixels of the workgroup's four waves, in every lane, through LDS; b: this wave's ballot
__device__ __forceinline__ void dp_wave_counts(unsigned long long b, unsigned wc[4])
{
    __shared__ unsigned sh[DP_TILE / 64];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (unsigned)__popcll(b);
    __syncthreads();
    for (int w = 0; w < DP_TILE / 64; ++w) wc[w] = sh[w];
}

__device__ __forceinline__ void dp_count(const DpArgs &a, const DpGeom &g)
{
    const int N = g.W * g.H, i = blockIdx.x * DP_TILE + threadIdx.x;
    bool keep = false;
    if (i < N) {
        const DpPoint pt = dp_point(a, g, i);
        if (a.xyz)
            for (int k = 0; k < 3; ++k) a.xyz[(size_t)3 * i + k] = pt.b[k];
        if (a.z) a.z[i] = pt.b[2];
        keep = pt.keep;
    }
    unsigned wc[4];
    dp_wave_counts(__ballot(keep), wc);
    if (threadIdx.x == 0) a.tile_cnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// thread t owns the tiles [t K, (t + 1) K), K = ceil(T / DP_SCAN): their sum, the workgroup's scan of the sums, their offsets
__device__ __forceinline__ void dp_scan(const DpArgs &a, const DpGeom &g)
{
    __shared__ unsigned sh[DP_SCAN];
    const int T = dp_tiles(g.W, g.H), K = (T + DP_SCAN - 1) / DP_SCAN, t = threadIdx.x;
    const int t0 = min(t * K, T), t1 = min(t0 + K, T);
    unsigned sum = 0;
    for (int k = t0; k < t1; ++k) sum += a.tile_cnt[k];
    sh[t] = sum;
    __syncthreads();
    for (int o = 1; o < DP_SCAN; o <<= 1) {
        const unsigned u = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += u;
        __syncthreads();
    }
    unsigned off = sh[t] - sum;
    for (int k = t0; k < t1; ++k) {
        a.tile_off[k] = off;
        off += a.tile_cnt[k];
    }
    if (t == DP_SCAN - 1) *a.total = sh[t];
}

__device__ __forceinline__ void dp_pack(const DpArgs &a, const DpGeom &g)
{
    const int N = g.W * g.H, i = blockIdx.x * DP_TILE + threadIdx.x;
    DpPoint pt;
    pt.keep = false;
    if (i < N) pt = dp_point(a, g, i);
    const unsigned long long b = __ballot(pt.keep);
    unsigned wc[4];
    dp_wave_counts(b, wc);
    if (pt.keep) {
        unsigned slot = a.tile_off[blockIdx.x] + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        for (unsigned w = 0; w < (threadIdx.x >> 6); ++w) slot += wc[w];
        unsigned px = sgm_px(a.img, a.depth, a.ch, (size_t)i);
        if (a.ch == 1) px *= 0x010101u;                // a one-channel pair: the byte three times
        a.cloud[slot] = make_uint4(pt.b[0], pt.b[1], pt.b[2], px | 0xff000000u);
    }
}

template <typename S> __global__ __launch_bounds__(DP_TILE) void k_dp_count(S src, DpGeom g) { dp_count(dp_pair(src), g); }
template <typename S> __global__ __launch_bounds__(DP_SCAN) void k_dp_scan(S src, DpGeom g) { dp_scan(dp_pair(src), g); }
template <typename S> __global__ __launch_bounds__(DP_TILE) void k_dp_pack(S src, DpGeom g) { dp_pack(dp_pair(src), g); }

using DpV = RecVal<DpArgs>;
using DpT = RecTab<DpArgs>;

void launch_dp_count(hipStream_t s, const DpGeom &g, const Recs<DpArgs> &q)
{
    rec_launch(s, k_dp_count<DpV>, k_dp_count<DpT>, dim3((unsigned)dp_tiles(g.W, g.H), (unsigned)q.n), dim3(DP_TILE), 0, q, g);
}

void launch_dp_scan(hipStream_t s, const DpGeom &g, const Recs<DpArgs> &q)
{
    rec_launch(s, k_dp_scan<DpV>, k_dp_scan<DpT>, dim3(1u, (unsigned)q.n), dim3(DP_SCAN), 0, q, g);
}

void launch_dp_pack(hipStream_t s, const DpGeom &g, const Recs<DpArgs> &q)
{
    rec_launch(s, k_dp_pack<DpV>, k_dp_pack<DpT>, dim3((unsigned)dp_tiles(g.W, g.H), (unsigned)q.n), dim3(DP_TILE), 0, q, g);
}

}  // namespace psm
