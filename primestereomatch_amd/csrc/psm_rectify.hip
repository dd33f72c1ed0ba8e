// psm_rectify.hip - k_rectify: cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) with CV_16SC2 fixed-point maps, followed by the crop,
// for both eyes of a camera frame in one launch - the first thing StereoMatch::compute does to a frame in video mode
// (src/StereoMatch.cpp:149-153).  Writes the interleaved B,G,R bytes straight into the context's staged image slot, in the layout
// psm_upload_pair leaves there.  Integer arithmetic with an exact definition:
//   (mx, my) = map_xy, fx = frac & 31, fy = frac >> 5, w00 = (32-fx)(32-fy)*32 ... (sum 2^15),
//   out = (w00*S(my,mx) + w01*S(my,mx+1) + w10*S(my+1,mx) + w11*S(my+1,mx+1) + 2^14) >> 15, a tap outside the source reads 0.
#include "psm_kernels.h"

namespace psm {

// the two horizontally adjacent taps of one source row: 6 bytes from an arbitrary byte address as one unaligned 8-byte load
// (the source slot is allocated with 8 spare bytes behind the last pixel)
__device__ __forceinline__ unsigned long long rect_load6(const uint8_t *p)
{
    unsigned long long v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// one tap on its own (border columns): 3 bytes, or 0 outside the source
__device__ __forceinline__ unsigned long long rect_tap(const uint8_t *src, size_t pitch, int x, int y, int src_w, int src_h)
{
    if ((unsigned)x >= (unsigned)src_w || (unsigned)y >= (unsigned)src_h) return 0ull;
    const uint8_t *p = src + (size_t)y * pitch + 3 * (size_t)x;
    return (unsigned long long)(p[0] | (p[1] << 8) | (p[2] << 16));
}

// One workgroup per tile of 256 consecutive pixels of the output's row-major order (a 256 x 1 tile that wraps at the end of a
// row): its 768 bytes start on a dword whatever the image width is, which a two-dimensional tile's rows do not (W * 3 is odd
// for odd W).  One pixel per lane; the source is read through L1 / L2 with two 8-byte loads per lane - the maps are smooth, so
// the lanes of a wave read overlapping bytes of two or three source rows; arbitrary maps are as correct, only slower.  The
// 3-byte pixels of four neighbouring lanes become three dwords through one quad DPP move; every store is a whole dword, 192
// contiguous bytes per wave.  blockIdx.y: side.
__global__ __launch_bounds__(256) void k_rectify(RectArgs a)
{
    const RectSide sd = a.s[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    unsigned v = 0;
    if (idx < a.npix) {
        const unsigned m = sd.xy[idx];
        const int mx = (short)(m & 0xffffu), my = (int)m >> 16;
        const unsigned f = sd.fr[idx];
        const int fx = f & 31, fy = (f >> 5) & 31;
        const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
        unsigned long long t0, t1;          // bytes 0..2: tap (row, mx), bytes 3..5: tap (row, mx + 1)
        if ((unsigned)mx < (unsigned)(a.src_w - 1)) {       // both columns inside: the rows decide
            const uint8_t *p = sd.src + (size_t)(my < 0 ? 0 : my) * a.pitch + 3 * (size_t)mx;
            t0 = (unsigned)my < (unsigned)a.src_h ? rect_load6(p) : 0ull;
            t1 = (unsigned)(my + 1) < (unsigned)a.src_h ? rect_load6(my < 0 ? p : p + a.pitch) : 0ull;
        } else {
            t0 = rect_tap(sd.src, a.pitch, mx, my, a.src_w, a.src_h) | (rect_tap(sd.src, a.pitch, mx + 1, my, a.src_w, a.src_h) << 24);
            t1 = rect_tap(sd.src, a.pitch, mx, my + 1, a.src_w, a.src_h) | (rect_tap(sd.src, a.pitch, mx + 1, my + 1, a.src_w, a.src_h) << 24);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int s00 = (int)(t0 >> (8 * ch)) & 255, s01 = (int)(t0 >> (24 + 8 * ch)) & 255;
            const int s10 = (int)(t1 >> (8 * ch)) & 255, s11 = (int)(t1 >> (24 + 8 * ch)) & 255;
            const int o = (w00 * s00 + w01 * s01 + w10 * s10 + w11 * s11 + (1 << 14)) >> 15;      // FixedPtCast<int, uchar, 15>
            v |= (unsigned)o << (8 * ch);
        }
    }
    // lane j of a quad <- its right neighbour's pixel (quad_perm [1,2,3,3]); lanes 0..2 of the quad hold the quad's 3 dwords
    const unsigned nxt = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xF9, 0xf, 0xf, true);
    const int j = threadIdx.x & 3;
    const int dw = (idx >> 2) * 3 + j;
    if (j < 3 && dw < a.ndw) sd.out[dw] = (v >> (8 * j)) | (nxt << (24 - 8 * j));
}

void launch_rectify(hipStream_t s, const RectArgs &a)
{
    hipLaunchKernelGGL(k_rectify, dim3((a.npix + 255) / 256, 2), dim3(256), 0, s, a);
}

}  // namespace psm
