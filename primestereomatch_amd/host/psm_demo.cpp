// psm_demo - headless counterpart of the reference's StereoMatch::compute accelerator branch
// (src/StereoMatch.cpp:193-262): raw B,G,R uint8 pair in, four timed stages, raw uint8 maps out.
//   psm_demo <left.raw> <right.raw> <W> <H> <maxDis> <out_prefix> [ndev] [f32|u8] [float_input] [fgf_rate] [pp] [frames] [batch] [ring] [sgbm|sgbm_ref|sgbm_census|-] [gt.raw] [mask.raw|-] [pp]
// gt.raw (the 16th argument; W x H bytes, mask.raw likewise): the left map - after pp, if given - is scored on the device
// (DispEst::Score: scale_factor 4, error_threshold 4, the non-occluded mask if one is given) and the reference's line
// "%BP = ... Avg Err = ..." (src/StereoMatch.cpp:306) is printed from the device record; the display map and the error plane go to
// <out>_ldisp_disp.raw / <out>_edisp.raw; together with sgbm / sgbm_ref the same for the SGBM map (<out>_sgbm_disp.raw)
// sgbm: the 15th argument, the word "sgbm": additionally run the second algorithm (DispEst::SGBM_GPU: the STEREO_SGBM branch,
// src/StereoMatch.cpp:169-187) on the pair, print its three device times and dump the int16 map as <out>_sgbm16.raw (the SAD
// cost, no speckle filter); the word "sgbm_ref": the same with the whole configuration of setupOpenCVSGBM (:639-660) -
// preFilterCap 63, speckleWindowSize 100, speckleRange 32 - and the filter's time as a fourth line; the word "sgbm_census": the
// settings of sgbm with the census cost over a 9 x 7 window (DispEst::setSGBMCensus), nothing else changed
// pp: the 19th argument, the word "pp", with one of the sgbm words: the stage's 8-bit maps (DispEst::SGBMSelect) then go through
// lrCheck, fillInv and wgtMedian on the device; the filtered left map is dumped as <out>_sgbm_pp_ldisp.raw and, with gt.raw, scored
// like a GIF map (its %BP line)
// ring > 0: additionally push that many frames of the pair through a psm::FrameRing of two objects (two frames in flight, each
// object told PSM_OPT_FRAMES_IN_FLIGHT = 2), check every delivered frame's maps against the single-pair run, dump <out>_ldisp_ring.raw
// batch > 1: additionally run that many copies of the pair as ONE batch (DispEst::computeBatch -> psm_compute_batch: the
// reference's loop over pairs as shared launches), check every copy's maps against the single-pair run, dump <out>_ldisp_batch.raw;
// together with sgbm / sgbm_ref: also that many copies through DispEst::SGBMBatch (psm_sgm_compute_batch), every copy's int16
// map checked against the single run's
// frames > 0: additionally run that many frames of the pair through DispEst::computeFrame (asynchronous upload of the next
// pair / download of the previous maps: the frame loop of src/main.cpp:64-73), dump its last maps as <out>_ldisp_loop.raw and
// print the time per frame
// fgf_rate 0 (default): CostFilter_GPU; 2/4/8: CostFilter_FGF_GPU with that subsample rate
// pp 1: after the left-right check also fillInv + wgtMedian (the stages of PP::processDM, src/PP.cpp:405-410); the
//       post-processed maps go to <out_prefix>_ldisp_pp.raw / _rdisp_pp.raw
// pp 2: instead JointWMF on the device (JointWMF_GPU: the live body of processDM, src/PP.cpp:417-422), same output files
// --ply FILE (anywhere on the line; optionally --q q00,q01,...,q33: the 16 entries of cv::stereoRectify's Q, row-major): the left
// map - without the pixels the L-R check rejected; after pp, if given, all of it - is reprojected on the device (DispEst::Reproject) and the
// coloured point cloud written to FILE as a binary little-endian PLY.  Without --q: a pinhole camera of focal length W pixels with the
// principal point in the image centre and baseline 1 (depths in baselines)
// --wls (anywhere on the line; with one of the sgbm words): the int16 map then goes through the WLS smoothing on the device
// (DispEst::WLS_GPU: lambda 8000, sigma 1.5, 3 iterations) - the holes filled, the sixteenths kept; its device time is printed, the
// filtered map dumped as <out>_sgbm_wls16.raw and, with gt.raw, scored as integer disparities beside the unfiltered map's figure;
// with --ply a second cloud, that of the filtered map, goes to FILE with ".wls.ply" appended
// --wls-conf: --wls with the graded confidence (PSM_WLS_CONFIDENCE: both terms, lr_thresh 24, radius 2, var_shift 8) at the start of the
// solve; the device time of the two launches it adds is printed too
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "DispEst.h"

static bool slurp(const char *path, std::vector<unsigned char> &buf, size_t n)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    buf.resize(n);
    size_t got = fread(buf.data(), 1, n, f);
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

static bool write_ply(const char *path, const std::vector<psm::DispEst::Point> &cloud)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n", cloud.size());
    bool ok = true;
    for (const psm::DispEst::Point &p : cloud) {
        const float xyz[3] = {p.x, p.y, p.z};
        const unsigned char rgb[3] = {p.r, p.g, p.b};
        ok = ok && fwrite(xyz, sizeof xyz, 1, f) == 1 && fwrite(rgb, sizeof rgb, 1, f) == 1;
    }
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    // the two named options are taken off the line first; the positional arguments keep their places
    const char *ply_path = nullptr, *q_text = nullptr;
    bool wls = false, wls_conf = false;
    std::vector<char *> args;
    for (int i = 0; i < argc; ++i) {
        if (!strcmp(argv[i], "--ply") && i + 1 < argc) ply_path = argv[++i];
        else if (!strcmp(argv[i], "--q") && i + 1 < argc) q_text = argv[++i];
        else if (!strcmp(argv[i], "--wls")) wls = true;
        else if (!strcmp(argv[i], "--wls-conf")) wls = wls_conf = true;
        else args.push_back(argv[i]);
    }
    argc = (int)args.size();
    argv = args.data();
    if (argc < 7) {
        fprintf(stderr, "usage: %s left.raw right.raw W H maxDis out_prefix [ndev] [f32|u8] [float_input] [fgf_rate] [pp] [frames] [batch] [ring] [sgbm|sgbm_ref|sgbm_census|-] [gt.raw] [mask.raw|-] [pp]\n", argv[0]);
        return 2;
    }
    const int W = atoi(argv[3]), H = atoi(argv[4]), D = atoi(argv[5]);
    const std::string out = argv[6];
    const int ndev = argc > 7 ? atoi(argv[7]) : 1;
    const int dtype = (argc > 8 && !strcmp(argv[8], "u8")) ? PSM_U8 : PSM_F32;
    const bool float_input = argc > 9 && atoi(argv[9]) != 0;
    const int fgf_rate = argc > 10 ? atoi(argv[10]) : 0;
    const int pp = argc > 11 ? atoi(argv[11]) : 0;
    const int frames = argc > 12 ? atoi(argv[12]) : 0;
    const int batch = argc > 13 ? atoi(argv[13]) : 0;
    const int nring = argc > 14 ? atoi(argv[14]) : 0;
    const bool sgbm_ref = argc > 15 && !strcmp(argv[15], "sgbm_ref");
    const bool sgbm_census = argc > 15 && !strcmp(argv[15], "sgbm_census");
    const bool sgbm = sgbm_ref || sgbm_census || (argc > 15 && !strcmp(argv[15], "sgbm"));
    const char *gt_path = argc > 16 ? argv[16] : nullptr;
    const char *mask_path = argc > 17 && strcmp(argv[17], "-") ? argv[17] : nullptr;
    const bool sgbm_pp = sgbm && argc > 18 && !strcmp(argv[18], "pp");
    std::vector<unsigned char> lraw, rraw, gtraw, maskraw;
    if (gt_path && (!slurp(gt_path, gtraw, (size_t)W * H) || (mask_path && !slurp(mask_path, maskraw, (size_t)W * H)))) {
        fprintf(stderr, "psm_demo: cannot read the ground truth / mask\n");
        return 2;
    }
    if (!slurp(argv[1], lraw, (size_t)W * H * 3) || !slurp(argv[2], rraw, (size_t)W * H * 3)) {
        fprintf(stderr, "psm_demo: cannot read the input pair\n");
        return 2;
    }
    int gotDev = psm::hipUtil::hipDevicePoll();  // src/main.cpp:29 openCLdevicepoll()
    if (gotDev <= 0) {
        fprintf(stderr, "psm_demo: no HIP device / library (%s)\n", psm::hipUtil::error().c_str());
        return 3;
    }
    psm::Mat l(H, W, 3, psm::PSM_8U, lraw.data()), r(H, W, 3, psm::PSM_8U, rraw.data());
    std::vector<float> lf, rf;
    if (float_input) {  // src/StereoMatch.cpp:195-196 convertTo(CV_32F, 1/255.0f)
        lf.resize(lraw.size());
        rf.resize(rraw.size());
        const float alpha = 1 / 255.0f;
        for (size_t i = 0; i < lraw.size(); ++i) {
            lf[i] = (float)lraw[i] * alpha;
            rf[i] = (float)rraw[i] * alpha;
        }
        l = psm::Mat(H, W, 3, psm::PSM_32F, lf.data());
        r = psm::Mat(H, W, 3, psm::PSM_32F, rf.data());
    }
    psm::DispEst SMDE(l, r, D, 8, gotDev > 0, ndev, dtype);
    if (!SMDE.ok()) return 4;
    SMDE.setInputImages(l, r);
    SMDE.setThreads(8);
    SMDE.setSubsampleRate(fgf_rate ? fgf_rate : 4);
    int rc = 0;
    rc |= SMDE.CostConst_GPU();
    rc |= fgf_rate ? SMDE.CostFilter_FGF_GPU() : SMDE.CostFilter_GPU();
    rc |= SMDE.DispSelect_GPU();
    rc |= SMDE.PostProcess_GPU();        // (L-R validity only: the maps stay the raw WTA maps; ProcessDM_GPU below is the commented-out sequence of processDM)
    if (rc) return 5;
    printf("STEREO GIF Module Times:\nCVC Time:\t %4.2f ms\nCVF Time:\t %4.2f ms\nDispSel Time:\t %4.2f ms\nPP Time:\t %4.2f ms\n",
           SMDE.stageTimeUs(PSM_STAGE_CVC) / 1000, SMDE.stageTimeUs(PSM_STAGE_CVF) / 1000,
           SMDE.stageTimeUs(PSM_STAGE_DISPSEL) / 1000, SMDE.stageTimeUs(PSM_STAGE_PP) / 1000);
    bool ok = dump(out + "_ldisp.raw", SMDE.lDisMap.data, (size_t)W * H) && dump(out + "_rdisp.raw", SMDE.rDisMap.data, (size_t)W * H) &&
              dump(out + "_lvalid.raw", SMDE.lValid.data, (size_t)W * H) && dump(out + "_rvalid.raw", SMDE.rValid.data, (size_t)W * H);
    if (ok && pp) {
        if (pp == 2 ? SMDE.JointWMF_GPU() : SMDE.ProcessDM_GPU()) return 5;   // pp 1: lrCheck + fillInv + wgtMedian (src/PP.cpp:405-410,
                                                                              // commented out in the reference); pp 2: JointWMF
        ok = dump(out + "_ldisp_pp.raw", SMDE.lDisMap.data, (size_t)W * H) && dump(out + "_rdisp_pp.raw", SMDE.rDisMap.data, (size_t)W * H);
    }
    if (ok && gt_path) {
        psm::Mat gt(H, W, 1, psm::PSM_8U, gtraw.data()), mask(H, W, 1, psm::PSM_8U, maskraw.data()), disp, emap;
        struct psm_score rec;
        if (SMDE.setGroundTruth(gt, mask_path ? &mask : nullptr) || SMDE.setScoreParams(4, 4, mask_path ? PSM_MASK_NONOCC : PSM_MASK_NONE) ||
            SMDE.Score(PSM_SCORE_GIF, &rec, &disp, &emap))
            return 5;
        printf("%%BP = %.2f%% \t Avg Err = %.2f\n", psm::DispEst::scoreBP(rec), psm::DispEst::scoreAvgErr(rec));
        ok = dump(out + "_ldisp_disp.raw", disp.data, (size_t)W * H) && dump(out + "_edisp.raw", emap.data, (size_t)W * H);
    }
    double Q[16] = {1, 0, 0, -0.5 * W, 0, 1, 0, -0.5 * H, 0, 0, 0, (double)W, 0, 0, 1, 0};
    if (ok && ply_path) {
        if (q_text) {
            const char *p = q_text;
            for (int i = 0; i < 16; ++i) {
                char *end = nullptr;
                Q[i] = strtod(p, &end);
                if (end == p || (i < 15 && *end != ',')) { fprintf(stderr, "psm_demo: --q wants 16 numbers separated by commas\n"); return 2; }
                p = end + 1;
            }
        }
        uint32_t count = 0;
        if (SMDE.setReprojection(Q) || SMDE.Reproject(PSM_DEPTH_GIF, &count, pp == 0)) return 5;
        printf("Point cloud:\t %u of %d pixels kept -> %s\n", count, W * H, ply_path);
        ok = write_ply(ply_path, SMDE.cloud());
    }
    if (ok && frames > 0 && ndev == 1 && !fgf_rate) {
        SMDE.setInputImages(l, r);
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < frames; ++i)
            if (SMDE.computeFrame(i + 1 < frames ? &l : nullptr, i + 1 < frames ? &r : nullptr, i > 0)) return 5;
        if (SMDE.finishFrames()) return 5;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("Frame loop:	 %d frames, %4.3f ms per frame (H2D of every pair and D2H of every pair of maps included)\n", frames, ms / frames);
        ok = dump(out + "_ldisp_loop.raw", SMDE.lDisMap.data, (size_t)W * H) && dump(out + "_rdisp_loop.raw", SMDE.rDisMap.data, (size_t)W * H);
    }
    if (ok && batch > 1 && ndev == 1 && !fgf_rate) {
        std::vector<std::vector<uint8_t>> keep(2);
        keep[0].assign(SMDE.lDisMap.data, SMDE.lDisMap.data + (size_t)W * H);      // (frames > 0: the loop's maps = the same pair's)
        keep[1].assign(SMDE.rDisMap.data, SMDE.rDisMap.data + (size_t)W * H);
        std::vector<psm::DispEst *> des;
        for (int b = 0; b < batch; ++b) des.push_back(new psm::DispEst(l, r, D, 8, true, 1, dtype));
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = psm::DispEst::computeBatch(des.data(), batch);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        bool same = rc == 0;
        for (int b = 0; b < batch && same && !pp; ++b)
            same = !memcmp(des[b]->lDisMap.data, keep[0].data(), (size_t)W * H) && !memcmp(des[b]->rDisMap.data, keep[1].data(), (size_t)W * H);
        printf("Batch:\t %d pairs in one set of launches, %4.3f ms (first call, maps downloaded), maps %s\n", batch, ms, same ? "equal the single-pair run's" : "DIFFER");
        ok = same && dump(out + "_ldisp_batch.raw", des[batch - 1]->lDisMap.data, (size_t)W * H) && dump(out + "_rdisp_batch.raw", des[batch - 1]->rDisMap.data, (size_t)W * H);
        for (auto *d : des) delete d;
    }
    if (ok && nring > 0 && ndev == 1 && !fgf_rate && !pp) {
        std::vector<uint8_t> kl(SMDE.lDisMap.data, SMDE.lDisMap.data + (size_t)W * H), kr(SMDE.rDisMap.data, SMDE.rDisMap.data + (size_t)W * H);
        psm::FrameRing ring(l, r, D, 2, dtype);
        if (!ring.ok()) return 5;
        psm::Mat ol = psm::Mat::zeros(H, W, 1, psm::PSM_8U), orr = psm::Mat::zeros(H, W, 1, psm::PSM_8U);
        int delivered = 0;
        bool same = true;
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < nring + 2 && same; ++i) {
            const int got = i < nring ? ring.push(l, r, &ol, &orr) : ring.flush(&ol, &orr);
            if (got < 0) return 5;
            if (got == 1) {
                ++delivered;
                same = !memcmp(ol.data, kl.data(), (size_t)W * H) && !memcmp(orr.data, kr.data(), (size_t)W * H);
            }
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        same = same && delivered == nring && ring.flush(&ol, &orr) == 0;
        printf("Frame ring:\t %d frames through 2 objects, %4.3f ms per frame (H2D and D2H of every frame included), %d delivered, maps %s\n", nring,
               ms / nring, delivered, same ? "equal the single-pair run's" : "DIFFER");
        ok = same && dump(out + "_ldisp_ring.raw", ol.data, (size_t)W * H) && dump(out + "_rdisp_ring.raw", orr.data, (size_t)W * H);
    }
    if (ok && sgbm) {
        std::vector<int16_t> d16;
        double ms[3] = {0, 0, 0};
        SMDE.setInputImages(l, r);
        if (sgbm_ref && (SMDE.setSGBMPreFilterCap(63) || SMDE.setSGBMSpeckle(100, 32))) return 5;
        if (sgbm_census && SMDE.setSGBMCensus(9, 7)) return 5;
        if (SMDE.setOption(PSM_OPT_PROFILE, 1) || SMDE.SGBM_GPU(d16) || SMDE.sgbmTimes(ms)) return 5;
        printf("STEREO SGBM Times:\nCost Time:\t %4.3f ms\nPaths Time:\t %4.3f ms\nSelect Time:\t %4.3f ms\n", ms[0], ms[1], ms[2]);
        if (sgbm_ref) {
            double spk = 0;
            if (SMDE.sgbmSpeckleTime(&spk)) return 5;
            printf("Speckle Time:\t %4.3f ms\n", spk);
        }
        ok = dump(out + "_sgbm16.raw", (const unsigned char *)d16.data(), d16.size() * sizeof(int16_t));
        if (ok && gt_path) {      // (the truth is already on the device)
            psm::Mat disp;
            struct psm_score rec;
            if (SMDE.Score(PSM_SCORE_SGM, &rec, &disp, nullptr)) return 5;
            printf("%%BP = %.2f%% \t Avg Err = %.2f\n", psm::DispEst::scoreBP(rec), psm::DispEst::scoreAvgErr(rec));
            ok = dump(out + "_sgbm_disp.raw", disp.data, (size_t)W * H);
        }
        if (ok && wls) {          // the sub-pixel map through the WLS smoothing; published, the SGM sources of Score and Reproject read it
            std::vector<int16_t> w16;
            double wms = 0;
            struct psm_score before, after;
            if (gt_path && SMDE.Score(PSM_SCORE_SGM_INT, &before, nullptr, nullptr)) return 5;
            if (SMDE.setWLS() || SMDE.setWLSConfidence() || SMDE.WLS_GPU(PSM_WLS_SGM, false, &w16, nullptr, wls_conf) || SMDE.wlsTime(&wms) ||
                SMDE.WLSPublish(true))
                return 5;
            printf("WLS Time:\t %4.3f ms\n", wms);
            if (wls_conf) {
                double cms = 0;
                if (SMDE.wlsConfTime(&cms)) return 5;
                printf("... of which the graded confidence:\t %4.3f ms\n", cms);
            }
            ok = dump(out + "_sgbm_wls16.raw", (const unsigned char *)w16.data(), w16.size() * sizeof(int16_t));
            if (ok && gt_path) {
                if (SMDE.Score(PSM_SCORE_SGM_INT, &after, nullptr, nullptr)) return 5;
                printf("SGBM integer disparities: %%BP = %.2f%%, WLS-filtered: %%BP = %.2f%%\n", psm::DispEst::scoreBP(before), psm::DispEst::scoreBP(after));
            }
            if (ok && ply_path) {
                uint32_t count = 0;
                const std::string path = std::string(ply_path) + ".wls.ply";
                if (SMDE.setReprojection(Q) || SMDE.Reproject(PSM_DEPTH_SGM, &count)) return 5;
                printf("Point cloud (WLS):\t %u of %d pixels kept -> %s\n", count, W * H, path.c_str());
                ok = write_ply(path.c_str(), SMDE.cloud());
            }
            if (SMDE.WLSPublish(false)) return 5;
        }
        if (ok && sgbm_pp) {      // the stage's 8-bit maps through the post-processing chain of the GIF path, scored like its maps
            if (SMDE.SGBMSelect() || SMDE.LRCheck_GPU() || SMDE.FillInvalid_GPU() || SMDE.WgtMedian_GPU()) return 5;
            ok = dump(out + "_sgbm_pp_ldisp.raw", SMDE.lDisMap.data, (size_t)W * H);
            if (ok && gt_path) {
                struct psm_score rec;
                if (SMDE.Score(PSM_SCORE_GIF, &rec, nullptr, nullptr)) return 5;
                printf("SGBM post-processed (lrCheck, fillInv, wgtMedian): %%BP = %.2f%% \t Avg Err = %.2f\n", psm::DispEst::scoreBP(rec),
                       psm::DispEst::scoreAvgErr(rec));
            }
        }
        if (ok && batch > 1 && ndev == 1) {
            std::vector<psm::DispEst *> des;
            bool set = true;
            for (int b = 0; b < batch; ++b) {
                des.push_back(new psm::DispEst(l, r, D, 8, true, 1, dtype));
                set = set && des[b]->ok() && !(sgbm_ref && (des[b]->setSGBMPreFilterCap(63) || des[b]->setSGBMSpeckle(100, 32))) &&
                      !(sgbm_census && des[b]->setSGBMCensus(9, 7));
            }
            std::vector<std::vector<int16_t>> maps;
            double bms[3] = {0, 0, 0};
            const int rcb = !set || des[0]->setOption(PSM_OPT_PROFILE, 1) || psm::DispEst::SGBMBatch(des.data(), batch, maps) || des[0]->sgbmTimes(bms);
            bool same = rcb == 0;
            for (int b = 0; b < batch && same; ++b) same = maps[b] == d16;
            printf("SGBM batch:\t %d pairs in one set of launches, per pair %4.3f ms cost, %4.3f ms paths, %4.3f ms select, maps %s\n", batch,
                   bms[0] / batch, bms[1] / batch, bms[2] / batch, same ? "equal the single run's" : "DIFFER");
            ok = same;
            for (auto *d : des) delete d;
        }
    }
    return ok ? 0 : 6;
}
