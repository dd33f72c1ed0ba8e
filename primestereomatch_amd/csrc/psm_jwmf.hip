// psm_jwmf.hip - the joint weighted median of the reference's live PP::processDM (src/PP.cpp:402-424 -> JointWMF::filter,
// include/JointWMF.h) on gfx950, computed per pixel from its definition:
//
//   feature    the 8-bit colour image; keys (c0>>2, c1>>2, c2>>2), c0 = B         (JointWMF.h:546-567)
//   samples    the distinct keys in ascending order                                (JointWMF.h:575-582)
//   clusters   identity when there are at most nF samples; otherwise k-means++ seeding from a fixed splitmix64 stream
//              and Lloyd iterations (the reference's cv::kmeans, JointWMF.h:587-613, draws from an unreproducible RNG)
//   median     the smallest c with 2 * W(<=c) >= W(total) over the clipped (2r+1)^2 window, W summed as the exact
//              integers rint(w * 2^48) of the weight table w[F(p)][F(q)]      (the balanceWeight rule, JointWMF.h:272-315)
//
// The reference's column scan with its joint histogram and necklace tables (filterCore, JointWMF.h:173-410) is a serial
// speed-up of that definition; nothing of it is used here.  The weight table itself is formed on the host with libm expf
// (psm_api_jwmf.cpp), so it is the reference's float table bit for bit.
//
// One launch sequence for a single pair and for several (psm_joint_wmf, psm_joint_wmf_batch): every kernel is one body (jw_*)
// behind one entry k_jw_*<S>, which has the image to cluster (JwImg) or the map side (JwSide) on a grid axis of its own and is
// templated over where the records come from - S (psm_kernels.h, Recs) - JwVal<R>: the at most two records of a single pair by value in
// the kernarg; RecTab<R>: the device table of a batch.  All sums are exact integers: a body's result does not depend on the grid it runs in.
#include "psm_kernels.h"

#include <algorithm>

namespace psm {

namespace {

constexpr int JW_SEED_THREADS = 1024;
constexpr int JW_TILE = 16;                // median: 16 x 16 output pixels per workgroup, one lane each
constexpr int JW_HALO_MAX = JW_TILE + 2 * JW_RMAX;

__device__ __forceinline__ unsigned key_u8(unsigned b, unsigned g, unsigned r) { return ((b >> 2) << 12) | ((g >> 2) << 6) | (r >> 2); }

// convertTo(CV_8UC3, 255) of a float image: saturate(rint(v * 255)) (PP.cpp:417-419); NaN -> 0
__device__ __forceinline__ unsigned feat_f32(float v)
{
    const float f = rintf(__fmul_rn(v, 255.0f));
    return f > 0.f ? (unsigned)fminf(f, 255.f) : 0u;
}

__device__ __forceinline__ unsigned key_at(const void *img, int depth, size_t p)
{
    if (depth == 0) {
        const uint8_t *q = (const uint8_t *)img + 3 * p;
        return key_u8(q[0], q[1], q[2]);
    }
    const float *q = (const float *)img + 3 * p;
    return key_u8(feat_f32(q[0]), feat_f32(q[1]), feat_f32(q[2]));
}

__device__ __forceinline__ void key_xyz(unsigned k, int &x, int &y, int &z) { x = (int)(k >> 12); y = (int)((k >> 6) & 63); z = (int)(k & 63); }

// the two record sources (psm_kernels.h, Recs) of the images and of the map sides; a record's pointers are read as global ones (sgm_global)
using ImgV = JwVal<JwImg>;
using ImgT = RecTab<JwImg>;
using SideV = JwVal<JwSide>;
using SideT = RecTab<JwSide>;

// presence of every key of one image: one bit per key in a 2^18-bit map
__device__ __forceinline__ void jw_keys(const void *img, int depth, size_t HW, unsigned *bits)
{
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (size_t)gridDim.x * blockDim.x) {
        const unsigned k = key_at(img, depth, p);
        const unsigned m = 1u << (k & 31);
        if (!(bits[k >> 5] & m)) atomicOr(&bits[k >> 5], m);
    }
}

template <typename S> __global__ void k_jw_keys(S src, int depth, size_t HW)
{
    const JwImg &r = rec(src, blockIdx.y);
    jw_keys(sgm_global(r.img), depth, HW, sgm_global(r.bits));
}

// the key bitmap (what 0) or the key -> cluster table (what 1) of every image to zero, 16 bytes per lane
template <typename S> __global__ void k_jw_clear(S src, int what)
{
    const JwImg &r = rec(src, blockIdx.y);
    uint4 *p = what ? (uint4 *)sgm_global(r.lok) : (uint4 *)sgm_global(r.bits);
    const size_t n = (what ? (size_t)JW_KEYS : (size_t)JW_KEYS / 8) / 16;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}

// inclusive block scan of one 64-bit value per thread (blockDim.x = 64 * waves <= 1024)
__device__ unsigned long long block_scan_u64(unsigned long long v, unsigned long long *wsum)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0;
        for (int i = 0; i < nw; ++i) { const unsigned long long t = wsum[i]; wsum[i] = a; a += t; }
        wsum[nw] = a;
    }
    __syncthreads();
    v += wsum[wv];
    return v;
}

// ordered compaction of the key bitmap into the ascending sample list (one workgroup of 1024 threads, 8 words each)
__device__ __forceinline__ void jw_compact(const unsigned *bits, unsigned *samples, int *n_out)
{
    __shared__ unsigned long long wsum[17];
    const int w0 = threadIdx.x * (JW_KEYS / 32 / 1024);
    unsigned cnt = 0;
    for (int i = 0; i < JW_KEYS / 32 / 1024; ++i) cnt += __popc(bits[w0 + i]);
    const unsigned long long incl = block_scan_u64(cnt, wsum);
    unsigned o = (unsigned)(incl - cnt);
    for (int i = 0; i < JW_KEYS / 32 / 1024; ++i) {
        unsigned b = bits[w0 + i];
        while (b) {
            const int j = __ffs(b) - 1;
            b &= b - 1;
            samples[o++] = (unsigned)((w0 + i) * 32 + j);
        }
    }
    if (threadIdx.x == blockDim.x - 1) *n_out = (int)incl;
}

template <typename S> __global__ void __launch_bounds__(1024) k_jw_compact(S src)
{
    const JwImg &r = rec(src, blockIdx.x);
    jw_compact(sgm_global(r.bits), sgm_global(r.samples), sgm_global(r.state) + 3);
}

// every sample its own cluster
__device__ __forceinline__ void jw_identity(const unsigned *samples, int n, float *centres, int *labels)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int x, y, z;
    key_xyz(samples[i], x, y, z);
    centres[3 * i] = (float)x; centres[3 * i + 1] = (float)y; centres[3 * i + 2] = (float)z;
    labels[i] = i;
}

// the images with at most n_clusters samples; such an image counts as converged from the start (the Lloyd entries skip it)
template <typename S> __global__ void k_jw_identity(S src, int n_clusters)
{
    const JwImg &r = rec(src, blockIdx.y);
    if (r.n > n_clusters) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) sgm_global(r.state)[1] = 1;
    jw_identity(sgm_global(r.samples), r.n, sgm_global(r.centres), sgm_global(r.labels));
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long &s)
{
    s += 0x9E3779B97F4A7C15ull;
    unsigned long long z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// k-means++ seeding in one workgroup: thread t owns the samples [t*chunk, (t+1)*chunk) (kept transposed in kt / d2t so the
// rounds read coalesced); per round a block scan of the owners' D^2 sums finds the owner of the draw, which walks its chunk.
// Seeds are samples: D^2 and all prefix sums are integers, so the choice is exact.
__device__ __forceinline__ void jw_seed(const unsigned *samples, int n, int nf, unsigned long long seed, float *centres, unsigned *kt,
                                        unsigned *d2t)
{
    __shared__ unsigned long long wsum[17];
    __shared__ unsigned long long s_r;
    __shared__ int s_pick;
    const int t = threadIdx.x, T = JW_SEED_THREADS;
    const int chunk = (n + T - 1) / T;
    for (int k = 0; k < chunk; ++k) {
        const int i = t * chunk + k;
        kt[(size_t)k * T + t] = i < n ? samples[i] : 0u;
    }
    unsigned long long rng = seed;
    if (t == 0) {
        s_pick = (int)(splitmix64(rng) % (unsigned long long)n);
    }
    __syncthreads();
    int lim = n - t * chunk;
    lim = lim < 0 ? 0 : (lim > chunk ? chunk : lim);
    for (int round = 0;; ++round) {
        const int j = s_pick;
        int cx, cy, cz;
        key_xyz(samples[j], cx, cy, cz);
        if (t == 0) { centres[3 * round] = (float)cx; centres[3 * round + 1] = (float)cy; centres[3 * round + 2] = (float)cz; }
        if (round + 1 == nf) break;
        unsigned long long sum = 0;
        for (int k = 0; k < lim; ++k) {
            int x, y, z;
            key_xyz(kt[(size_t)k * T + t], x, y, z);
            const unsigned d = (unsigned)((x - cx) * (x - cx) + (y - cy) * (y - cy) + (z - cz) * (z - cz));
            const size_t a = (size_t)k * T + t;
            const unsigned m = round == 0 ? d : min(d2t[a], d);
            d2t[a] = m;
            sum += m;
        }
        const unsigned long long incl = block_scan_u64(sum, wsum);
        if (t == 0) s_r = splitmix64(rng) % wsum[T / 64];       // (the total: > 0 while fewer than n samples are seeds)
        __syncthreads();
        const unsigned long long r = s_r;
        if (incl - sum <= r && r < incl) {                         // the owner of the first prefix > r
            unsigned long long run = incl - sum;
            for (int k = 0; k < lim; ++k) {
                run += d2t[(size_t)k * T + t];
                if (run > r) { s_pick = t * chunk + k; break; }
            }
        }
        __syncthreads();
    }
}

// one workgroup per image with more than n_clusters samples, every image from the same seed; behind the seeding the workgroup
// makes the image's Lloyd state ready: labels -1 (the first assignment changes every label), sums 0 (the state block is zero from
// the start of the call)
template <typename S> __global__ void __launch_bounds__(JW_SEED_THREADS) k_jw_seed(S src, int n_clusters, unsigned long long seed)
{
    const JwImg &r = rec(src, blockIdx.x);
    if (r.n <= n_clusters) return;
    jw_seed(sgm_global(r.samples), r.n, r.nf, seed, sgm_global(r.centres), sgm_global(r.kt), sgm_global(r.d2t));
    int *labels = sgm_global(r.labels), *sums = sgm_global(r.sums);
    for (int i = threadIdx.x; i < r.n; i += JW_SEED_THREADS) labels[i] = -1;
    for (int i = threadIdx.x; i < JW_NF_MAX * 4; i += JW_SEED_THREADS) sums[i] = 0;
}

// Lloyd assignment: nearest centre in fp32 ((t0*t0 + t1*t1) + t2*t2, no contraction), ties to the lower index; integer
// sums and counts of the new clusters; st[0] counts the samples whose label changed.  st[1] != 0: converged, nothing to do.
__device__ __forceinline__ void jw_assign(const unsigned *samples, int n, int nf, const float *centres, int *labels, int *sums, int *st)
{
    __shared__ float c[JW_NF_MAX * 3];
    __shared__ int acc[JW_NF_MAX * 4];
    if (st[1]) return;
    for (int i = threadIdx.x; i < nf * 3; i += blockDim.x) c[i] = centres[i];
    for (int i = threadIdx.x; i < nf * 4; i += blockDim.x) acc[i] = 0;
    __syncthreads();
    int changed = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int x, y, z;
        key_xyz(samples[i], x, y, z);
        const float fx = (float)x, fy = (float)y, fz = (float)z;
        float best = 0.f;
        int bi = 0;
        for (int k = 0; k < nf; ++k) {
            const float t0 = __fsub_rn(fx, c[3 * k]), t1 = __fsub_rn(fy, c[3 * k + 1]), t2 = __fsub_rn(fz, c[3 * k + 2]);
            const float d = __fadd_rn(__fadd_rn(__fmul_rn(t0, t0), __fmul_rn(t1, t1)), __fmul_rn(t2, t2));
            if (k == 0 || d < best) { best = d; bi = k; }
        }
        changed += labels[i] != bi;
        labels[i] = bi;
        atomicAdd(&acc[4 * bi], x);
        atomicAdd(&acc[4 * bi + 1], y);
        atomicAdd(&acc[4 * bi + 2], z);
        atomicAdd(&acc[4 * bi + 3], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nf * 4; i += blockDim.x)
        if (acc[i]) atomicAdd(&sums[i], acc[i]);
    for (int o = 32; o; o >>= 1) changed += __shfl_xor(changed, o, 64);
    if ((threadIdx.x & 63) == 0 && changed) atomicAdd(&st[0], changed);
}

// the image on grid axis y, x sized for the largest image (an image's workgroups beyond its samples add nothing)
template <typename S> __global__ void __launch_bounds__(256) k_jw_assign(S src)
{
    const JwImg &r = rec(src, blockIdx.y);
    jw_assign(sgm_global(r.samples), r.n, r.nf, sgm_global(r.centres), sgm_global(r.labels), sgm_global(r.sums), sgm_global(r.state));
}

// Lloyd update (one workgroup): no label changed in iteration `it` -> converged after it + 1 assignments (st[1], st[2]);
// otherwise every non-empty cluster moves to its integer sums / count (fp32, exact operands, correctly rounded).
__device__ __forceinline__ void jw_update(int nf, float *centres, int *sums, int *st, int it)
{
    if (st[1]) return;
    const int changed = st[0];
    if (changed) {
        for (int k = threadIdx.x; k < nf; k += blockDim.x) {
            const int cnt = sums[4 * k + 3];
            if (cnt)
                for (int d = 0; d < 3; ++d) centres[3 * k + d] = __fdiv_rn((float)sums[4 * k + d], (float)cnt);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nf * 4; i += blockDim.x) sums[i] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        st[0] = 0;
        if (!changed) { st[1] = 1; st[2] = it + 1; }
    }
}

template <typename S> __global__ void __launch_bounds__(256) k_jw_update(S src, int it)
{
    const JwImg &r = rec(src, blockIdx.x);
    jw_update(r.nf, sgm_global(r.centres), sgm_global(r.sums), sgm_global(r.state), it);
}

__device__ __forceinline__ void jw_lok(const unsigned *samples, int n, const int *labels, uint8_t *lok)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lok[samples[i]] = (uint8_t)labels[i];
}

template <typename S> __global__ void k_jw_lok(S src)
{
    const JwImg &r = rec(src, blockIdx.y);
    jw_lok(sgm_global(r.samples), r.n, sgm_global(r.labels), sgm_global(r.lok));
}

// per-pixel cluster plane of both sides: F = label_of_key[key]
__device__ __forceinline__ void jw_plane(const JwSide &s, int depth, size_t HW)
{
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (size_t)gridDim.x * blockDim.x)
        s.F[p] = s.lok[key_at(s.img, depth, p)];
}

// a map side's record: of the device table, its pointers read as global ones (sgm_global, psm_kernels.h); of the kernarg, as it is
__device__ __forceinline__ JwSide jw_side(SideT tab, unsigned i)
{
    const JwSide &t = rec(tab, i);
    return JwSide{sgm_global(t.img), sgm_global(t.lok), sgm_global(t.F), sgm_global(t.din), sgm_global(t.wq), sgm_global(t.out)};
}
__device__ __forceinline__ const JwSide &jw_side(const SideV &v, unsigned i) { return rec(v, i); }

template <typename S> __global__ void k_jw_plane(S src, int depth, size_t HW) { jw_plane(jw_side(src, blockIdx.y), depth, HW); }

// The weighted median of both maps: one lane per output pixel of a 16 x 16 tile, the (disparity, cluster) pairs of the tile
// and its halo staged in LDS.  Two radix passes over 16 bins each (high nibble, then the low nibble inside the chosen high
// bin), every lane with its own 64-bit bins in LDS (bin-major, lane-minor: a lane's bins never share a bank with another
// lane's).  The sums are exact integers: the result does not depend on their order.
__device__ __forceinline__ void jw_median(const JwSide &s, int W, int H, int r)
{
    __shared__ unsigned short tile[JW_HALO_MAX * JW_HALO_MAX];
    __shared__ unsigned long long bins[16][256];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * JW_TILE, y0 = blockIdx.y * JW_TILE;
    const int tw = JW_TILE + 2 * r;
    const int ty0 = y0 - r, tx0 = x0 - r;
    for (int i = tid; i < tw * tw; i += 256) {
        const int yy = ty0 + i / tw, xx = tx0 + i % tw;
        unsigned short v = 0;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const size_t p = (size_t)yy * W + xx;
            v = (unsigned short)(s.din[p] | (s.F[p] << 8));
        }
        tile[i] = v;
    }
    for (int b = 0; b < 16; ++b) bins[b][tid] = 0;
    __syncthreads();
    const int x = x0 + (tid & (JW_TILE - 1)), y = y0 + tid / JW_TILE;
    if (x >= W || y >= H) return;                   // (no barrier below)
    const unsigned long long *wrow = s.wq + (size_t)(tile[(y - ty0) * tw + (x - tx0)] >> 8) * JW_NF_MAX;   // w[F(p)][.]
    const int ya = max(0, y - r) - ty0, yb = min(H - 1, y + r) - ty0;
    const int xa = max(0, x - r) - tx0, xb = min(W - 1, x + r) - tx0;
    for (int yy = ya; yy <= yb; ++yy)
        for (int xx = xa; xx <= xb; ++xx) {
            const unsigned v = tile[yy * tw + xx];
            bins[(v & 255) >> 4][tid] += wrow[v >> 8];
        }
    unsigned long long tot = 0;
    for (int b = 0; b < 16; ++b) tot += bins[b][tid];
    unsigned long long acc = 0;
    int h = 15;
    for (int b = 0; b < 16; ++b) {
        const unsigned long long a2 = acc + bins[b][tid];
        if (2 * a2 >= tot) { h = b; break; }
        acc = a2;
    }
    for (int b = 0; b < 16; ++b) bins[b][tid] = 0;
    for (int yy = ya; yy <= yb; ++yy)
        for (int xx = xa; xx <= xb; ++xx) {
            const unsigned v = tile[yy * tw + xx];
            if (((v & 255) >> 4) == (unsigned)h) bins[v & 15][tid] += wrow[v >> 8];
        }
    int l = 15;
    for (int b = 0; b < 16; ++b) {
        const unsigned long long a2 = acc + bins[b][tid];
        if (2 * a2 >= tot) { l = b; break; }
        acc = a2;
    }
    s.out[(size_t)y * W + x] = (uint8_t)(16 * h + l);
}

template <typename S> __global__ void __launch_bounds__(256) k_jw_median(S src, int W, int H, int r) { jw_median(jw_side(src, blockIdx.z), W, H, r); }

// grid x of the kernels that stride over the pixels of an image (keys, planes)
unsigned pixel_blocks(size_t HW) { return (unsigned)std::min<size_t>(std::max<size_t>((HW + 255) / 256, 1), 2048); }

}  // namespace

void launch_jw_keys(hipStream_t st, const JwRecs<JwImg> &im, int depth, size_t HW)
{
    rec_launch(st, k_jw_clear<ImgV>, k_jw_clear<ImgT>, dim3(JW_KEYS / 8 / 16 / 256, im.n), dim3(256), 0, im, 0);
    rec_launch(st, k_jw_keys<ImgV>, k_jw_keys<ImgT>, dim3(pixel_blocks(HW), im.n), dim3(256), 0, im, depth, HW);
}

void launch_jw_compact(hipStream_t st, const JwRecs<JwImg> &im)
{
    rec_launch(st, k_jw_compact<ImgV>, k_jw_compact<ImgT>, dim3(im.n), dim3(1024), 0, im);
}

void launch_jw_identity(hipStream_t st, const JwRecs<JwImg> &im, int n_clusters)
{
    rec_launch(st, k_jw_identity<ImgV>, k_jw_identity<ImgT>, dim3((n_clusters + 255) / 256, im.n), dim3(256), 0, im, n_clusters);
}

void launch_jw_seed(hipStream_t st, const JwRecs<JwImg> &im, int n_clusters, unsigned long long seed)
{
    rec_launch(st, k_jw_seed<ImgV>, k_jw_seed<ImgT>, dim3(im.n), dim3(JW_SEED_THREADS), 0, im, n_clusters, seed);
}

void launch_jw_lloyd(hipStream_t st, const JwRecs<JwImg> &im, int n_max, int it)
{
    rec_launch(st, k_jw_assign<ImgV>, k_jw_assign<ImgT>, dim3(std::min((n_max + 255) / 256, 512), im.n), dim3(256), 0, im);
    rec_launch(st, k_jw_update<ImgV>, k_jw_update<ImgT>, dim3(im.n), dim3(256), 0, im, it);
}

void launch_jw_lok(hipStream_t st, const JwRecs<JwImg> &im, int n_max)
{
    rec_launch(st, k_jw_clear<ImgV>, k_jw_clear<ImgT>, dim3(64, im.n), dim3(256), 0, im, 1);
    rec_launch(st, k_jw_lok<ImgV>, k_jw_lok<ImgT>, dim3((n_max + 255) / 256, im.n), dim3(256), 0, im);
}

void launch_jw_plane(hipStream_t st, const JwRecs<JwSide> &sides, int depth, size_t HW)
{
    rec_launch(st, k_jw_plane<SideV>, k_jw_plane<SideT>, dim3(pixel_blocks(HW), sides.n), dim3(256), 0, sides, depth, HW);
}

void launch_jw_median(hipStream_t st, const JwRecs<JwSide> &sides, int W, int H, int r)
{
    rec_launch(st, k_jw_median<SideV>, k_jw_median<SideT>, dim3((W + JW_TILE - 1) / JW_TILE, (H + JW_TILE - 1) / JW_TILE, sides.n), dim3(256), 0, sides, W, H, r);
}

}  // namespace psm

