// psm_api_rectify.cpp - video mode behind the C ABI: the camera frame goes to the device unrectified, k_rectify (psm_rectify.hip)
// remaps and crops both eyes into the context's staged image slot, psm_cost_construct adopts the pair as if psm_upload_pair[_async]
// had put it there.  Replaces remap(..., INTER_LINEAR) + lFrame_rec(cropBox) of StereoMatch::compute's DE_VIDEO branch
// (src/StereoMatch.cpp:149-153); psm_rectify_build_maps restates initUndistortRectifyMap(..., CV_16SC2, ...) (src/StereoMatch.cpp:464-466)
// for hosts without OpenCV.
#include "psm_ctx.h"

#include <cmath>
#include <cstring>

using namespace psm;

namespace psm {

void rectify_free(psm_ctx *c, bool maps)
{
    for (int k = 0; k < 2; ++k) {
        (void)hipFree(c->rect_src[k]); c->rect_src[k] = nullptr;
        if (maps) {
            (void)hipFree(c->rect_xy[k]); c->rect_xy[k] = nullptr;
            (void)hipFree(c->rect_fr[k]); c->rect_fr[k] = nullptr;
            c->rect_src_w[k] = c->rect_src_h[k] = 0;
        }
    }
    if (c->rect_pin) (void)hipHostFree(c->rect_pin);
    c->rect_pin = nullptr;
    c->rect_src_bytes = 0;
}

}  // namespace psm

namespace {

// what both upload forms check; *eye: bytes of one eye in a source slot (16-byte multiple)
int check_rect_args(psm_ctx *c, const char *who, const void *l, const void *r, int channels, size_t *stride_bytes, size_t *row, size_t *eye)
{
    if (!l || !r) return fail(c, "%s: NULL image", who);
    if (channels != 3) return fail(c, "%s: %d channels (3 required, B,G,R interleaved)", who, channels);
    for (int s = 0; s < 2; ++s)
        if (!c->rect_xy[s]) return fail(c, "%s: no rectification maps for the %s side (psm_rectify_set_maps)", who, s ? "right" : "left");
    if (c->rect_src_w[0] != c->rect_src_w[1] || c->rect_src_h[0] != c->rect_src_h[1])
        return fail(c, "%s: the source sizes of the two sides differ (%d x %d left, %d x %d right)", who, c->rect_src_w[0], c->rect_src_h[0],
                    c->rect_src_w[1], c->rect_src_h[1]);
    *row = (size_t)c->rect_src_w[0] * 3;
    if (*stride_bytes == 0) *stride_bytes = *row;
    if (*stride_bytes < *row) return fail(c, "%s: stride %zu < row size %zu", who, *stride_bytes, *row);
    *eye = (*row * c->rect_src_h[0] + 15) & ~(size_t)15;
    return 0;
}

// source slots for eyes of `eye` bytes: both device slots (8 readable bytes behind the last pixel: k_rectify's 8-byte loads) and,
// pinned: the page-locked staging of the asynchronous form (2 slots)
int ensure_src(psm_ctx *c, size_t eye, bool pinned)
{
    if (c->rect_src_bytes != eye) {
        if (psm_synchronize(c)) return 1;
        rectify_free(c, false);
    }
    for (int k = 0; k < 2; ++k)
        if (!c->rect_src[k]) PSM_HIP(c, hipMalloc((void **)&c->rect_src[k], 2 * eye + 16));
    if (pinned && !c->rect_pin) PSM_HIP(c, hipHostMalloc((void **)&c->rect_pin, 4 * eye, hipHostMallocDefault));
    c->rect_src_bytes = eye;
    return 0;
}

int enqueue_rectify(psm_ctx *c, hipStream_t stream, const uint8_t *src, size_t eye, void *const out[2])
{
    RectArgs a;
    for (int s = 0; s < 2; ++s) a.s[s] = RectSide{src + s * eye, c->rect_xy[s], c->rect_fr[s], (uint32_t *)out[s]};
    a.npix = c->W * c->H;
    a.ndw = (3 * a.npix + 3) / 4;         // (the image slots hold W * H * 12 bytes: the last dword's spare bytes are inside)
    a.src_w = c->rect_src_w[0];
    a.src_h = c->rect_src_h[0];
    a.pitch = (unsigned)a.src_w * 3;
    {
        Prof p(c, PSM_K_PREP, stream);
        launch_rectify(stream, a);
    }
    return check_launch(c, "k_rectify");
}

inline int sat16(long long v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : (int)v); }
// cvRound of a finite double into int (ties to even: the default rounding mode), saturated
inline int round_sat(double v)
{
    if (v <= -2147483648.0) return INT32_MIN;
    if (v >= 2147483647.0) return INT32_MAX;
    return (int)std::nearbyint(v);
}

}  // namespace

extern "C" {

int psm_rectify_build_maps(const double M[9], const double *dist, int n_dist, const double R[9], const double P[12], int map_w, int map_h,
                           int16_t *map_xy, uint16_t *map_frac)
{
    if (!M || !R || !P || !map_xy || !map_frac || (n_dist && !dist)) return fail(nullptr, "psm_rectify_build_maps: NULL argument");
    if (map_w < 1 || map_h < 1) return fail(nullptr, "psm_rectify_build_maps: bad map size %d x %d", map_w, map_h);
    if (n_dist != 0 && n_dist != 4 && n_dist != 5 && n_dist != 8 && n_dist != 12 && n_dist != 14)
        return fail(nullptr, "psm_rectify_build_maps: %d distortion coefficients (0, 4, 5, 8, 12 or 14)", n_dist);
    double k[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};       // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tx ty
    for (int i = 0; i < n_dist; ++i) k[i] = dist[i];
    if (k[12] != 0.0 || k[13] != 0.0) return fail(nullptr, "psm_rectify_build_maps: a tilted sensor model (tau_x, tau_y != 0) is not supported");
    // iR = inv(P[:, :3] * R): cofactors over the determinant
    double A[3][3], iR[3][3], C[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = (P[4 * i] * R[j] + P[4 * i + 1] * R[3 + j]) + P[4 * i + 2] * R[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            C[i][j] = A[(i + 1) % 3][(j + 1) % 3] * A[(i + 2) % 3][(j + 2) % 3] - A[(i + 1) % 3][(j + 2) % 3] * A[(i + 2) % 3][(j + 1) % 3];
    const double det = (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2];
    if (det == 0.0 || !std::isfinite(det)) return fail(nullptr, "psm_rectify_build_maps: P[:, :3] * R is singular");
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) iR[i][j] = C[j][i] / det;
    const double fx = M[0], fy = M[4], u0 = M[2], v0 = M[5];
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7], s1 = k[8], s2 = k[9], s3 = k[10], s4 = k[11];
    for (int v = 0; v < map_h; ++v)
        for (int u = 0; u < map_w; ++u) {
            const double du = (double)u, dv = (double)v;
            const double X = (iR[0][0] * du + iR[0][1] * dv) + iR[0][2];
            const double Y = (iR[1][0] * du + iR[1][1] * dv) + iR[1][2];
            const double Z = (iR[2][0] * du + iR[2][1] * dv) + iR[2][2];
            const double x = X / Z, y = Y / Z;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = (2 * x) * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = (((x * kr + p1 * _2xy) + p2 * (r2 + 2 * x2)) + s1 * r2) + (s2 * r2) * r2;
            const double yd = (((y * kr + p1 * (r2 + 2 * y2)) + p2 * _2xy) + s3 * r2) + (s4 * r2) * r2;
            const double mu = fx * xd + u0, mv = fy * yd + v0;
            const size_t o = (size_t)v * map_w + u;
            if (!std::isfinite(mu) || !std::isfinite(mv)) {          // every tap outside
                map_xy[2 * o] = map_xy[2 * o + 1] = -32768;
                map_frac[o] = 0;
                continue;
            }
            const int iu = round_sat(mu * 32.0), iv = round_sat(mv * 32.0);
            map_xy[2 * o] = (int16_t)sat16(iu >> 5);
            map_xy[2 * o + 1] = (int16_t)sat16(iv >> 5);
            map_frac[o] = (uint16_t)((iv & 31) * 32 + (iu & 31));
        }
    return 0;
}

int psm_rectify_set_maps(psm_ctx *c, int side, const int16_t *map_xy, const uint16_t *map_frac, int map_w, int map_h, int src_w, int src_h,
                         int crop_x, int crop_y)
{
    if (!c) return 1;
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "psm_rectify_set_maps: bad side %d", side);
    if (!map_xy || !map_frac) return fail(c, "psm_rectify_set_maps: NULL map");
    if (map_w < 1 || map_h < 1) return fail(c, "psm_rectify_set_maps: bad map size %d x %d", map_w, map_h);
    if (src_w < 2 || src_h < 1 || src_w > 32767 || src_h > 32767) return fail(c, "psm_rectify_set_maps: source size %d x %d outside [2, 32767] x [1, 32767]", src_w, src_h);
    if (crop_x < 0 || crop_y < 0 || (long long)crop_x + c->W > map_w || (long long)crop_y + c->H > map_h)
        return fail(c, "psm_rectify_set_maps: crop %d x %d at (%d, %d) outside the %d x %d maps", c->W, c->H, crop_x, crop_y, map_w, map_h);
    for (size_t i = 0, n = (size_t)map_w * map_h; i < n; ++i)
        if (map_frac[i] >= 1024)
            return fail(c, "psm_rectify_set_maps: map_frac %u at (%zu, %zu) >= 1024 (INTER_BITS = 5: fy * 32 + fx)", (unsigned)map_frac[i], i % map_w, i / map_w);
    if (bind(c)) return 1;
    if (psm_synchronize(c)) return 1;            // (a rectification in flight may still read the previous maps)
    const size_t HW = (size_t)c->W * c->H;
    if (!c->rect_xy[side]) PSM_HIP(c, hipMalloc((void **)&c->rect_xy[side], HW * sizeof(uint32_t)));
    if (!c->rect_fr[side]) PSM_HIP(c, hipMalloc((void **)&c->rect_fr[side], HW * sizeof(uint16_t)));
    // the crop window only, packed on the host (hipMemcpy2D is slow for rows that are no multiple of 4 bytes: h2d_rows)
    std::vector<uint32_t> xy(HW);
    std::vector<uint16_t> fr(HW);
    for (int y = 0; y < c->H; ++y) {
        const size_t o = (size_t)(crop_y + y) * map_w + crop_x;
        memcpy(xy.data() + (size_t)y * c->W, map_xy + 2 * o, (size_t)c->W * 4);
        memcpy(fr.data() + (size_t)y * c->W, map_frac + o, (size_t)c->W * 2);
    }
    PSM_HIP(c, hipMemcpy(c->rect_xy[side], xy.data(), HW * sizeof(uint32_t), hipMemcpyHostToDevice));
    PSM_HIP(c, hipMemcpy(c->rect_fr[side], fr.data(), HW * sizeof(uint16_t), hipMemcpyHostToDevice));
    c->rect_src_w[side] = src_w;
    c->rect_src_h[side] = src_h;
    return 0;
}

int psm_rectify_clear(psm_ctx *c)
{
    if (!c) return 1;
    if (psm_synchronize(c)) return 1;
    rectify_free(c, true);
    (void)hipGetLastError();
    return 0;
}

int psm_upload_pair_rectified(psm_ctx *c, const void *l, const void *r, int channels, size_t stride_bytes)
{
    if (!c) return 1;
    size_t row = 0, eye = 0;
    if (check_rect_args(c, "psm_upload_pair_rectified", l, r, channels, &stride_bytes, &row, &eye)) return 1;
    if (bind(c)) return 1;
    if (ensure_src(c, eye, false)) return 1;
    if (c->copy_stream) PSM_HIP(c, hipStreamSynchronize(c->copy_stream));     // (a staged frame's k_rectify may still read slot 0)
    const void *src[2] = {l, r};
    for (int s = 0; s < 2; ++s)
        if (h2d_rows(c, c->rect_src[0] + s * eye, src[s], row, stride_bytes, c->rect_src_h[0])) return 1;
    if (enqueue_rectify(c, c->stream, c->rect_src[0], eye, c->pair.raw)) return 1;
    PSM_HIP(c, hipStreamSynchronize(c->stream));      // the copy reads caller memory (psm_upload_pair)
    pair_uploaded(c, PSM_IMG_U8, true);
    return 0;
}

// psm_upload_pair_async with the rectification behind the copy, both on the copy stream: the frame is copied into page-locked
// staging before the call returns, travels into the slot's device source buffer and is remapped into the second image slot; ev_up
// is recorded behind the kernel, so the next psm_cost_construct adopts a finished pair.
int psm_upload_pair_rectified_async(psm_ctx *c, const void *l, const void *r, int channels, size_t stride_bytes)
{
    if (!c) return 1;
    size_t row = 0, eye = 0;
    if (check_rect_args(c, "psm_upload_pair_rectified_async", l, r, channels, &stride_bytes, &row, &eye)) return 1;
    if (bind(c)) return 1;
    if (ensure_src(c, eye, true)) return 1;
    int slot = 0;
    if (stage_begin(c, false, &slot)) return 1;
    uint8_t *stage = c->rect_pin + (size_t)slot * 2 * eye;
    const void *src[2] = {l, r};
    for (int s = 0; s < 2; ++s) stage_pack(stage + s * eye, src[s], row, stride_bytes, c->rect_src_h[0]);
    stage_send(c, c->rect_src[slot], stage, 2 * eye);                        // both eyes, one copy
    if (check_launch(c, "upload (copy kernel)")) return 1;
    PSM_HIP(c, hipEventRecord(c->pair.ev_stage[slot], c->copy_stream));            // the staging slot is free again once the copy is over
    // raw_next was the current pair two frames ago: the launches that read it (images_read records ev_free behind them) must be over
    // before the kernel writes there (the copy above touches the source slot only and need not wait)
    PSM_HIP(c, hipStreamWaitEvent(c->copy_stream, c->pair.ev_free, 0));
    if (enqueue_rectify(c, c->copy_stream, c->rect_src[slot], eye, c->pair.raw_next)) return 1;
    return stage_commit(c, PSM_IMG_U8, false);
}

int psm_download_images(psm_ctx *c, uint8_t *l, uint8_t *r, size_t stride_bytes)
{
    if (!c) return 1;
    if (!l || !r) return fail(c, "psm_download_images: NULL image");
    if (!c->have_images) return fail(c, "psm_download_images: no current image pair (a staged pair becomes current in psm_cost_construct)");
    if (c->pair.st.depth != PSM_IMG_U8) return fail(c, "psm_download_images: the current pair is a float pair (8-bit pairs only)");
    const size_t row = (size_t)c->W * 3;
    if (stride_bytes == 0) stride_bytes = row;
    if (stride_bytes < row) return fail(c, "psm_download_images: stride %zu < row size %zu", stride_bytes, row);
    if (bind(c)) return 1;
    return d2h_rows(c, l, c->pair.raw[0], row, stride_bytes, c->H) || d2h_rows(c, r, c->pair.raw[1], row, stride_bytes, c->H);
}

}  // extern "C"
