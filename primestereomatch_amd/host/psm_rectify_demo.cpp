// psm_rectify_demo - headless counterpart of the DE_VIDEO branch of StereoMatch::compute (src/StereoMatch.cpp:138-153) through the
// C++ mirror: a raw side-by-side camera frame and the CV_16SC2 maps of both cameras in, the rectified + cropped images and the
// disparity maps out.
//   psm_rectify_demo <frame.raw> <src_w> <src_h> <maps_prefix> <map_w> <map_h> <crop_x> <crop_y> <W> <H> <maxDis> <out_prefix> [f32|u8] [frames] [ring]
// frame.raw: src_h rows of 2 * src_w B,G,R pixels (left eye | right eye).  Maps: <maps_prefix>_l_xy.raw / _r_xy.raw (int16
// [map_h][map_w][2]) and <maps_prefix>_l_frac.raw / _r_frac.raw (uint16 [map_h][map_w]).
// Writes <out>_limg.raw / _rimg.raw (H x W x 3: setRectification + setInputFrame + downloadImages) and <out>_ldisp.raw /
// _rdisp.raw (the stage calls).
// frames > 0: additionally that many frames through DispEst::computeVideoFrame (the frame rectified on the copy stream while
//             the previous one computes), last maps to <out>_ldisp_loop.raw / _rdisp_loop.raw
// ring > 0:   additionally that many frames through FrameRing::push_frame (two objects), every delivered frame's maps checked
//             against the blocking run, last maps to <out>_ldisp_ring.raw / _rdisp_ring.raw
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "DispEst.h"

template <typename T>
static bool slurp(const std::string &path, std::vector<T> &buf, size_t n)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    buf.resize(n);
    size_t got = fread(buf.data(), sizeof(T), n, f);
    fclose(f);
    return got == n;
}
static bool dump(const std::string &path, const unsigned char *p, size_t n)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    size_t put = fwrite(p, 1, n, f);
    fclose(f);
    return put == n;
}

int main(int argc, char **argv)
{
    if (argc < 13) {
        fprintf(stderr, "usage: %s frame.raw src_w src_h maps_prefix map_w map_h crop_x crop_y W H maxDis out_prefix [f32|u8] [frames] [ring]\n", argv[0]);
        return 2;
    }
    const int src_w = atoi(argv[2]), src_h = atoi(argv[3]);
    const std::string maps = argv[4];
    const int map_w = atoi(argv[5]), map_h = atoi(argv[6]), crop_x = atoi(argv[7]), crop_y = atoi(argv[8]);
    const int W = atoi(argv[9]), H = atoi(argv[10]), D = atoi(argv[11]);
    const std::string out = argv[12];
    const int dtype = (argc > 13 && !strcmp(argv[13], "u8")) ? PSM_U8 : PSM_F32;
    const int frames = argc > 14 ? atoi(argv[14]) : 0;
    const int nring = argc > 15 ? atoi(argv[15]) : 0;
    if (src_w < 1 || src_h < 1 || map_w < 1 || map_h < 1 || W < 1 || H < 1) {
        fprintf(stderr, "psm_rectify_demo: bad sizes\n");
        return 2;
    }
    std::vector<unsigned char> frame;
    std::vector<int16_t> xy[2];
    std::vector<uint16_t> fr[2];
    const size_t MN = (size_t)map_w * map_h;
    if (!slurp(argv[1], frame, (size_t)src_h * 2 * src_w * 3) || !slurp(maps + "_l_xy.raw", xy[0], 2 * MN) || !slurp(maps + "_r_xy.raw", xy[1], 2 * MN) ||
        !slurp(maps + "_l_frac.raw", fr[0], MN) || !slurp(maps + "_r_frac.raw", fr[1], MN)) {
        fprintf(stderr, "psm_rectify_demo: cannot read the frame or the maps\n");
        return 2;
    }
    int gotDev = psm::hipUtil::hipDevicePoll();  // src/main.cpp:29 openCLdevicepoll()
    if (gotDev <= 0) {
        fprintf(stderr, "psm_rectify_demo: no HIP device / library (%s)\n", psm::hipUtil::error().c_str());
        return 3;
    }
    psm::Mat vFrame(src_h, 2 * src_w, 3, psm::PSM_8U, frame.data());
    psm::Rectification rect;
    for (int s = 0; s < 2; ++s) {
        rect.map_xy[s] = xy[s].data();
        rect.map_frac[s] = fr[s].data();
    }
    rect.map_w = map_w; rect.map_h = map_h; rect.src_w = src_w; rect.src_h = src_h; rect.crop_x = crop_x; rect.crop_y = crop_y;

    psm::Mat blank = psm::Mat::zeros(H, W, 3, psm::PSM_8U);
    psm::DispEst SMDE(blank, blank, D, 8, gotDev > 0, 1, dtype);
    if (!SMDE.ok()) return 4;
    if (SMDE.setRectification(rect) || SMDE.setInputFrame(vFrame)) return 5;
    psm::Mat lImg, rImg;
    if (SMDE.downloadImages(&lImg, &rImg)) return 5;
    if (SMDE.CostConst_GPU() || SMDE.CostFilter_GPU() || SMDE.DispSelect_GPU()) return 5;
    const size_t HW = (size_t)W * H;
    bool ok = dump(out + "_limg.raw", lImg.data, HW * 3) && dump(out + "_rimg.raw", rImg.data, HW * 3) &&
              dump(out + "_ldisp.raw", SMDE.lDisMap.data, HW) && dump(out + "_rdisp.raw", SMDE.rDisMap.data, HW);
    printf("Rectified:\t %d x %d frame -> 2 x %d x %d at (%d, %d)\n", 2 * src_w, src_h, W, H, crop_x, crop_y);
    std::vector<uint8_t> kl(SMDE.lDisMap.data, SMDE.lDisMap.data + HW), kr(SMDE.rDisMap.data, SMDE.rDisMap.data + HW);
    if (ok && frames > 0) {
        if (SMDE.setInputFrame(vFrame)) return 5;
        for (int i = 0; i < frames; ++i)
            if (SMDE.computeVideoFrame(i + 1 < frames ? &vFrame : nullptr, i > 0)) return 5;
        if (SMDE.finishFrames()) return 5;
        const bool same = !memcmp(SMDE.lDisMap.data, kl.data(), HW) && !memcmp(SMDE.rDisMap.data, kr.data(), HW);
        printf("Frame loop:\t %d frames, maps %s\n", frames, same ? "equal the blocking run's" : "DIFFER");
        ok = same && dump(out + "_ldisp_loop.raw", SMDE.lDisMap.data, HW) && dump(out + "_rdisp_loop.raw", SMDE.rDisMap.data, HW);
    }
    if (ok && nring > 0) {
        psm::FrameRing ring(blank, blank, D, 2, dtype);
        if (!ring.ok() || ring.setRectification(rect)) return 5;
        psm::Mat ol = psm::Mat::zeros(H, W, 1, psm::PSM_8U), orr = psm::Mat::zeros(H, W, 1, psm::PSM_8U);
        int delivered = 0;
        bool same = true;
        for (int i = 0; i < nring + 2 && same; ++i) {
            const int got = i < nring ? ring.push_frame(vFrame, &ol, &orr) : ring.flush(&ol, &orr);
            if (got < 0) return 5;
            if (got == 1) {
                ++delivered;
                same = !memcmp(ol.data, kl.data(), HW) && !memcmp(orr.data, kr.data(), HW);
            }
        }
        same = same && delivered == nring && ring.flush(&ol, &orr) == 0;
        printf("Frame ring:\t %d frames through 2 objects, %d delivered, maps %s\n", nring, delivered, same ? "equal the blocking run's" : "DIFFER");
        ok = same && dump(out + "_ldisp_ring.raw", ol.data, HW) && dump(out + "_rdisp_ring.raw", orr.data, HW);
    }
    return ok ? 0 : 6;
}
