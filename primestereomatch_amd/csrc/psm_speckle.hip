// psm_speckle.hip - the speckle filter of the semi-global matching stage: cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff)
// on an int16 map, which StereoSGBM runs on its final map when speckleWindowSize > 0 (setupOpenCVSGBM, src/StereoMatch.cpp:639-660:
// 100, 32 -> newVal -16, maxSpeckleSize 100, maxDiff 512).  The definition (tests/speckle_model.py) is order-free:
//   vertices  the pixels with img != newVal
//   edges     4-neighbours p, q, both vertices, |img[p] - img[q]| <= maxDiff (the difference in 32 bits)
//   result    every pixel of a connected component of at most maxSpeckleSize pixels becomes newVal, every other pixel stays
// Connected components by union-find over the pixel grid, four launches whatever the data (no pass count, no host read-back):
//   k_spk_runs    label[p] = index of the first pixel of p's horizontal run (SPK_NONE for newVal pixels), size[head] = run length
//   k_spk_merge   every vertical edge (p, p - W) joins the sets of its two ends: atomicMin on the larger root
//   k_spk_count   every run head that is not its set's root: label[head] = root, atomicAdd(size[root], run length)
//   k_spk_apply   map[p] = size[root of p] <= maxSpeckleSize ? newVal : map[p]; size[p] = size[root of p] (0 for newVal pixels)
// A label is the index of a pixel of the same set that is not larger than the pixel's own index, and a label only ever decreases:
// every chain p, label[p], label[label[p]] ... is strictly decreasing, so every loop below ends on its own.
#include "psm_kernels.h"

namespace psm {

constexpr unsigned SPK_NONE = 0xffffffffu;

__device__ __forceinline__ bool spk_conn(int a, int b, int md)
{
    const int d = a - b;                          // int16 values in 32 bits: 32767 - (-32768) does not wrap
    return (d < 0 ? -d : d) <= md;
}

// The root of x's tree as this thread sees it.  Labels are read with plain loads: inside k_spk_merge other workgroups, on other
// XCDs, lower labels at the same time, and a load may return an older parent.  Correctness does not depend on it: an old parent
// is still a pixel of the same set (sets only grow) with a smaller index, so what find returns is always a member of x's set that
// was a root at some time; whether it still is, the atomicMin in spk_union decides - its return value is authoritative.
__device__ __forceinline__ unsigned spk_find(const unsigned *label, unsigned x)
{
    unsigned l;
    while ((l = label[x]) < x) x = l;             // (strictly decreasing: at most x steps)
    return x;
}

// Joins the sets of a and b.  The larger of the two roots receives the smaller one; if the atomicMin finds that it was no root any
// more (its label `old` is already below itself), its label is now min(old, lo) and the set of `old` and the set of `lo` still have
// to be joined: continue with that pair.  The larger root of the pair strictly decreases from round to round (old < hi, lo < hi),
// which bounds the loop; no thread waits for another.
__device__ __forceinline__ void spk_union(unsigned *label, unsigned a, unsigned b)
{
    for (;;) {
        a = spk_find(label, a);
        b = spk_find(label, b);
        if (a == b) return;
        const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
        const unsigned old = atomicMin(label + hi, lo);
        if (old == hi) return;                    // hi was a root, now it hangs below lo
        a = old;
        b = lo;
    }
}

// What a body takes: the call's scalars and the planes of one pair - map [H][W], filtered in place; label and size as psm_kernels.h
// has them (SgmPair's out, spk_label, spk_size)
struct SpkRun : SpkArgs {
    int16_t *map;
    unsigned *label, *size;
};

// One wave per row, 64 pixels at a time.  A pixel starts a run if it is a vertex and does not connect to its left neighbour; the
// ballot of the starts and a bit scan give every lane its run's first pixel, a run that began in an earlier piece is carried in
// `carry`.  The last pixel of a run writes the run's length to size[head].  All horizontal structure is flat before the first
// atomic is issued.
__device__ __forceinline__ void spk_runs(const SpkRun &a)
{
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= a.H) return;                                           // (wave-uniform)
    const int16_t *row = a.map + (size_t)y * a.W;
    const unsigned base = (unsigned)y * (unsigned)a.W;
    int carry = 0;                                                  // first pixel of the run that reaches the piece's left edge
    for (int x0 = 0; x0 < a.W; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < a.W;
        const int v = in ? row[x] : a.new_val;
        const bool vert = in && v != a.new_val;
        bool left = false, right = false;                           // connects to the left / right neighbour
        if (vert && x > 0) { const int l = row[x - 1]; left = l != a.new_val && spk_conn(v, l, a.max_diff); }
        if (vert && x + 1 < a.W) { const int r = row[x + 1]; right = r != a.new_val && spk_conn(v, r, a.max_diff); }
        const unsigned long long starts = __ballot(vert && !left);
        const unsigned long long below = starts & (~0ull >> (63 - lane));       // starts at or left of this lane
        const int head = below ? x0 + 63 - __builtin_clzll(below) : carry;
        if (vert) {
            a.label[base + x] = base + (unsigned)head;
            if (!right) a.size[base + head] = (unsigned)(x - head + 1);
        } else if (in) {
            a.label[base + x] = SPK_NONE;
        }
        carry = __builtin_amdgcn_readlane(head, 63);
    }
}

// One thread per pixel below the first row: its edge to the pixel above.  Skipped when the left neighbour is in the same run, has
// an edge of its own to the pixel above it and that pixel is in the same run as ours above: the edge would join the same two runs.
__device__ __forceinline__ void spk_merge(const SpkRun &a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y + 1;
    if (x >= a.W) return;
    const size_t p = (size_t)y * a.W + x;
    const int v = a.map[p], u = a.map[p - a.W];
    if (v == a.new_val || u == a.new_val || !spk_conn(v, u, a.max_diff)) return;
    if (x > 0) {
        const int l = a.map[p - 1], ul = a.map[p - a.W - 1];
        if (l != a.new_val && ul != a.new_val && spk_conn(l, v, a.max_diff) && spk_conn(ul, u, a.max_diff) && spk_conn(l, ul, a.max_diff)) return;
    }
    spk_union(a.label, (unsigned)p, (unsigned)(p - a.W));
}

// One thread per pixel, run heads act.  After k_spk_merge the labels are final (a launch of its own on the same stream), so find
// gives the true root; writing it back only shortens chains other threads walk (either value leads to the same root).  Only roots
// receive adds and only heads that are no roots read their own size: a size is an exact integer sum, whatever the arrival order.
__device__ __forceinline__ void spk_count(const SpkRun &a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    const size_t p = (size_t)y * a.W + x;
    const int v = a.map[p];
    if (v == a.new_val) return;
    if (x > 0) { const int l = a.map[p - 1]; if (l != a.new_val && spk_conn(v, l, a.max_diff)) return; }
    const unsigned r = spk_find(a.label, (unsigned)p);
    if (r == (unsigned)p) return;
    a.label[p] = r;
    atomicAdd(a.size + r, a.size[p]);
}

// One thread per pixel.  size[p] is rewritten in place with the size of p's component: the only entries other threads read here
// are those of roots, and a root writes the value it already holds.
__device__ __forceinline__ void spk_apply(const SpkRun &a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    const size_t p = (size_t)y * a.W + x;
    const unsigned h = a.label[p];
    unsigned s = 0;
    if (h != SPK_NONE) {
        s = a.size[spk_find(a.label, h)];
        if (s <= (unsigned)a.max_size) a.map[p] = (int16_t)a.new_val;
    }
    a.size[p] = s;
}

// Every kernel is its body behind an entry that is a template over the record source S (psm_kernels.h, Recs): the pair of a single
// call by value, or - several maps of one size per launch (psm_sgm_compute_batch) - pair blockIdx.z of the device table; its planes
// are read as global pointers (uniform per workgroup).  Labels and sizes are pixel indices within a pair's own planes.
template <typename S>
__device__ __forceinline__ SpkRun spk_run(const S &src, const SpkArgs &a, unsigned pair)
{
    const SgmPair &p = rec(src, pair);
    SpkRun r;
    static_cast<SpkArgs &>(r) = a;
    r.map = sgm_global(p.out); r.label = sgm_global(p.spk_label); r.size = sgm_global(p.spk_size);
    return r;
}
template <typename S> __global__ __launch_bounds__(256) void k_spk_runs(SpkArgs a, S src) { spk_runs(spk_run(src, a, blockIdx.z)); }
template <typename S> __global__ __launch_bounds__(256) void k_spk_merge(SpkArgs a, S src) { spk_merge(spk_run(src, a, blockIdx.z)); }
template <typename S> __global__ __launch_bounds__(256) void k_spk_count(SpkArgs a, S src) { spk_count(spk_run(src, a, blockIdx.z)); }
template <typename S> __global__ __launch_bounds__(256) void k_spk_apply(SpkArgs a, S src) { spk_apply(spk_run(src, a, blockIdx.z)); }

void launch_speckle(hipStream_t s, const SpkArgs &a, const Recs<SgmPair> &q)
{
    using V = RecVal<SgmPair>;
    using T = RecTab<SgmPair>;
    const unsigned n = (unsigned)q.n;
    const dim3 block(256), rows((a.W + 255) / 256, a.H, n);
    rec_launch(s, k_spk_runs<V>, k_spk_runs<T>, dim3((a.H + 3) / 4, 1, n), block, 0, a, q);
    if (a.H > 1) rec_launch(s, k_spk_merge<V>, k_spk_merge<T>, dim3(rows.x, a.H - 1, n), block, 0, a, q);
    rec_launch(s, k_spk_count<V>, k_spk_count<T>, rows, block, 0, a, q);
    rec_launch(s, k_spk_apply<V>, k_spk_apply<T>, rows, block, 0, a, q);
}

}  // namespace psm
