// psm_fgf_dev.h - the device functions the two Fast Guided Filter files share (psm_fgf.hip: FastGuidedFilterColor; psm_gray_fgf.hip:
// FastGuidedFilterMono): the index maps of cv::resize and the marching cv::blur of four planes.
// Canonical OpenCV semantics (oracle/psm_oracle.h "CVF, Fast Guided Filter variant"):
//   INTER_NN:      src index = min(floor(x * ifx), size-1), ifx = 1 / ((size/s) / (double)size)
//   cv::blur k x k: taps -k/2..+k/2, REFLECT_101, fp64 sums (x taps left to right, then y taps top to
//                  bottom), (float)(sum * (1.0/(k*k)))
//   INTER_LINEAR:  fx = (float)((dx+0.5)*scale-0.5); sx = floor(fx); fx -= sx; clamped at both ends;
//                  row pass S[sx]*(1-fx) + S[sx+1]*fx, then column pass, fp32, no FMA
#pragma once
#include <hip/hip_runtime.h>

namespace psm {

__device__ __forceinline__ int r101s(int k, int n)
{
    k = k < 0 ? -k : k;
    k = k >= n ? 2 * (n - 1) - k : k;
    return k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
}
__device__ __forceinline__ int nn_src(int x, int dsize, int ssize)
{   // cv::resize INTER_NN source index
    const double ifx = 1. / ((double)dsize / ssize);
    int sx = (int)floor(x * ifx);
    return sx < ssize - 1 ? sx : ssize - 1;
}
__device__ __forceinline__ void lin_src(int d, int ssize, int dsize, int &sx, float &f)
{   // cv::resize INTER_LINEAR source index and weight of the second tap
    const double scale = (double)ssize / dsize;
    f = (float)((d + 0.5) * scale - 0.5);
    sx = (int)floorf(f);
    f = __fsub_rn(f, (float)sx);
    if (sx < 0) { f = 0.f; sx = 0; }
    if (sx >= ssize - 1) { f = 0.f; sx = ssize - 1; }
}

// ---- separable k x k mean of four planes (one float4 per pixel), marching down the rows -------------
// One 64-lane workgroup owns OUTW = 64 - 2R output columns (+R halo lanes each side, reflected) of one slice and
// the rows [ybeg, yend).  Summation order = cv::blur's: x taps left to right (fp64), then y taps top to bottom.
template <int K, class Load, class Finish>
__device__ __forceinline__ void blur4_march(int ws, int hs, int strip, int ybeg, int yend, float4 *lds, Load load, Finish finish)
{
    constexpr int R = K / 2, OUTW = 64 - 2 * R;
    const int lane = threadIdx.x;
    const int x = strip * OUTW - R + lane;
    const int xc = r101s(x, ws);
    const bool out_lane = lane >= R && lane < 64 - R && x < ws;
    const double scale = 1.0 / (K * K);
    int tap[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        int l = lane - R + i;
        tap[i] = l < 0 ? 0 : (l > 63 ? 63 : l);
    }
    double ring[K][4];
#pragma unroll
    for (int u = 0; u < K; ++u) ring[u][0] = ring[u][1] = ring[u][2] = ring[u][3] = 0.0;
    int par = 0;
    for (int yy0 = ybeg - R; yy0 < yend + R; yy0 += K) {
#pragma unroll
        for (int u = 0; u < K; ++u) {
            const int yy = yy0 + u;
            if (yy < yend + R) {  // uniform over the workgroup
                lds[par * 64 + lane] = load(r101s(yy, hs), xc);
                __syncthreads();
                double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const float4 t = lds[par * 64 + tap[i]];
                    h0 = __dadd_rn(h0, (double)t.x);
                    h1 = __dadd_rn(h1, (double)t.y);
                    h2 = __dadd_rn(h2, (double)t.z);
                    h3 = __dadd_rn(h3, (double)t.w);
                }
                ring[u][0] = h0; ring[u][1] = h1; ring[u][2] = h2; ring[u][3] = h3;
                par ^= 1;
                if (yy >= ybeg + R) {  // rows yy-2R .. yy are in the ring, oldest in slot u+1
                    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
                    for (int j = 1; j <= K; ++j) {
                        const int sl = (u + j) % K;
                        a0 = __dadd_rn(a0, ring[sl][0]);
                        a1 = __dadd_rn(a1, ring[sl][1]);
                        a2 = __dadd_rn(a2, ring[sl][2]);
                        a3 = __dadd_rn(a3, ring[sl][3]);
                    }
                    if (out_lane)
                        finish(yy - R, x, make_float4((float)(a0 * scale), (float)(a1 * scale), (float)(a2 * scale), (float)(a3 * scale)));
                }
            }
        }
    }
}

}  // namespace psm
