#include "DispEst.h"

#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace psm {

DispEst::DispEst(Mat l, Mat r, const int d, int t, bool ocl, int ndev, int dtype)
    : lImg(l), rImg(r), maxDis(d), threads(t), useOCL(ocl)
{
    hei = lImg.rows;
    wid = lImg.cols;
    if (lImg.type() != rImg.type()) {  // src/DispEst.cpp:21-29
        printf("DE: Error - Left & Right images are of different types.\n");
        exit(1);
    }
    lDisMap = Mat::zeros(hei, wid, 1, PSM_8U);
    rDisMap = Mat::zeros(hei, wid, 1, PSM_8U);
    lValid = Mat::zeros(hei, wid, 1, PSM_8U);
    rValid = Mat::zeros(hei, wid, 1, PSM_8U);
    if (!useOCL) return;
    if (!hipUtil::load()) {
        useOCL = false;
        return;
    }
    const HipApi &api = hipUtil::api();
    int have = api.device_count();
    if (ndev < 1) ndev = 1;
    // PSM_HOST_LOGICAL_STRIPES=1: more stripes than devices are allowed, the contexts then share devices (tests on one GPU)
    const char *logical = std::getenv("PSM_HOST_LOGICAL_STRIPES");
    const bool share = logical && *logical && *logical != '0' && have > 0;
    if (ndev > have && !share) ndev = have;
    if (ndev > hei) ndev = hei;
    // several devices: one context per device on a stripe of the image rows - all disparities of both volumes, so the WTA
    // finishes on the device and only finished map rows are gathered (psm_gather_rows_ctx).  Stripes of R = ceil(H / ndev)
    // rows, aligned at multiples of R (the same bounds as the rank-per-GPU host, primestereomatch_amd/stripes.py: a gathered
    // [ndev][2][R][W] buffer is the image); devices past the last non-empty stripe stay unused.
    const int R = (hei + ndev - 1) / ndev;
    while (ndev > 1 && (ndev - 1) * R >= hei) --ndev;
    for (int g = 0; g < ndev; ++g) {
        psm_ctx *c = nullptr;
        const int ya = g * R, yb = ya + R < hei ? ya + R : hei;
        y0s.push_back(ya);
        y1s.push_back(yb);
        if (api.create_shard(&c, wid, hei, maxDis, 0, maxDis, dtype, g % have) != 0 ||
            (ndev > 1 && api.set_rows(c, ya, yb) != 0)) {
            fprintf(stderr, "DispEst: %s\n", api.last_error(c));
            if (c) api.destroy(c);
            for (psm_ctx *p : ctx) api.destroy(p);
            ctx.clear();
            useOCL = false;
            return;
        }
        if (ndev > 1) api.set_option(c, PSM_OPT_ASYNC, 1);  // the stripes run concurrently
        ctx.push_back(c);
    }
    setInputImages(lImg, rImg);
}

DispEst::~DispEst(void)
{
    if (hipUtil::loaded())
        for (psm_ctx *p : ctx) hipUtil::api().destroy(p);
}

int DispEst::setInputImages(Mat leftImg, Mat rightImg)
{
    assert(leftImg.type() == rightImg.type());  // src/DispEst.cpp:166
    lImg = leftImg;
    rImg = rightImg;
    int rc = 0;
    for (psm_ctx *c : ctx)
        rc |= hipUtil::api().upload_pair(c, lImg.data, rImg.data, lImg.channels, lImg.step,
                                         lImg.depth == PSM_32F ? PSM_IMG_F32 : PSM_IMG_U8);
    return rc;
}

int DispEst::setRectification(const Rectification &rect)
{
    if (ctx.empty()) return 1;
    int rc = 0;
    for (psm_ctx *c : ctx)
        for (int s = 0; s < 2 && !rc; ++s) {
            rc = hipUtil::api().rectify_set_maps(c, s, rect.map_xy[s], rect.map_frac[s], rect.map_w, rect.map_h, rect.src_w, rect.src_h,
                                                 rect.crop_x, rect.crop_y);
            if (rc) fprintf(stderr, "DispEst: %s\n", hipUtil::api().last_error(c));
        }
    rect_src_w = rc ? 0 : rect.src_w;
    rect_src_h = rc ? 0 : rect.src_h;
    return rc;
}

bool DispEst::frameOk(const Mat &v) const
{
    if (rect_src_w > 0 && v.data && v.depth == PSM_8U && v.channels == 3 && v.rows == rect_src_h && v.cols == 2 * rect_src_w) return true;
    fprintf(stderr, "DispEst: setInputFrame needs setRectification first and a %d x %d CV_8UC3 side-by-side frame\n", 2 * rect_src_w, rect_src_h);
    return false;
}

int DispEst::setInputFrame(const Mat &vFrame)
{
    if (ctx.empty() || !frameOk(vFrame)) return 1;
    int rc = 0;       // the two eyes: ROIs of the frame (same pitch, the right one 3 * src_w bytes further)
    for (psm_ctx *c : ctx) rc |= hipUtil::api().upload_pair_rectified(c, vFrame.data, vFrame.data + 3 * (size_t)rect_src_w, 3, vFrame.step);
    return rc;
}

int DispEst::downloadImages(Mat *l, Mat *r)
{
    if (ctx.empty() || !l || !r) return 1;
    for (Mat *m : {l, r})
        if (!m->data || m->rows != hei || m->cols != wid || m->channels != 3 || m->depth != PSM_8U) *m = Mat::zeros(hei, wid, 3, PSM_8U);
    if (l->step != r->step) return 1;
    return hipUtil::api().download_images(ctx[0], l->data, r->data, l->step);
}

int DispEst::setThreads(unsigned int newThreads)
{
    if (newThreads > MAX_CPU_THREADS) return -1;  // src/DispEst.cpp:172-179
    threads = newThreads;
    return 0;
}

int DispEst::CostConst_GPU()
{
    if (ctx.empty()) return 1;
    int rc = 0;
    for (psm_ctx *c : ctx) rc |= hipUtil::api().cost_construct(c);
    return rc;
}

int DispEst::CostFilter_GPU()
{
    if (ctx.empty()) return 1;
    int rc = 0;
    if (whole_on_first && ctx.size() > 1) rc |= hipUtil::api().set_rows(ctx[0], y0s[0], y1s[0]);   // back to stripes
    whole_on_first = false;
    for (psm_ctx *c : ctx) rc |= hipUtil::api().cost_filter(c);
    return rc;
}

int DispEst::CostFilter_FGF_GPU()
{
    if (ctx.empty()) return 1;
    // the Fast Guided Filter path has no row stripes (its low-resolution models would need their own halo arithmetic, and
    // it is 3x cheaper than the full filter anyway): the first device filters the whole image, the others sit this frame out
    int rc = 0;
    if (ctx.size() > 1) rc |= hipUtil::api().set_rows(ctx[0], 0, 0);
    whole_on_first = ctx.size() > 1;
    rc |= hipUtil::api().cost_filter_fgf(ctx[0], (int)subsample_rate);
    return rc;
}

int DispEst::DispSelect_GPU()
{
    if (ctx.empty()) return 1;
    const HipApi &api = hipUtil::api();
    if (ctx.size() == 1 || whole_on_first) return api.disp_select(ctx[0], lDisMap.data, rDisMap.data, lDisMap.step);
    int rc = 0;
    for (psm_ctx *c : ctx) rc |= api.disp_select(c, nullptr, nullptr, 0);
    rc |= api.gather_rows_ctx(ctx[0], ctx.data(), (int)ctx.size(), lDisMap.data, rDisMap.data, lDisMap.step);
    return rc;
}

int DispEst::setOption(int option, int value)
{
    if (ctx.empty()) return 1;
    int rc = 0;
    for (psm_ctx *c : ctx) rc |= hipUtil::api().set_option(c, option, value);
    return rc;
}

int DispEst::LRCheck_GPU()
{
    if (ctx.empty()) return 1;
    return hipUtil::api().lr_check(ctx[0], lValid.data, rValid.data, lValid.step);
}

int DispEst::PostProcess_GPU()
{   // The reference's call (src/DispEst.cpp:338-344) runs PP::processDM, whose LIVE body is the CPU JointWMF (out of scope) with
    // lrCheck / fillInv / wgtMedian commented out (src/PP.cpp:405-412).  What the accelerator side contributes to this stage is
    // the L-R check: lValid / rValid are filled, lDisMap / rDisMap stay the raw WTA maps (a caller that reads them afterwards
    // gets what DispSelect_GPU left).  The commented-out sequence as a whole: ProcessDM_GPU().
    return LRCheck_GPU();
}

int DispEst::ProcessDM_GPU()
{   // the sequence PP::processDM's source spells out but does not run (src/PP.cpp:405-410): lrCheck, fillInv, wgtMedian - all on
    // the device; lDisMap / rDisMap are REPLACED by the filled, weighted-median-filtered maps
    if (ctx.empty()) return 1;
    const HipApi &api = hipUtil::api();
    int rc = api.lr_check(ctx[0], lValid.data, rValid.data, lValid.step);
    if (!rc) rc = api.fill_invalid(ctx[0], nullptr, nullptr, 0);
    if (!rc) rc = api.wgt_median(ctx[0], lDisMap.data, rDisMap.data, lDisMap.step);
    return rc;
}

int DispEst::FillInvalid_GPU()
{
    if (ctx.empty()) return 1;
    return hipUtil::api().fill_invalid(ctx[0], lDisMap.data, rDisMap.data, lDisMap.step);
}

int DispEst::WgtMedian_GPU()
{
    if (ctx.empty()) return 1;
    return hipUtil::api().wgt_median(ctx[0], lDisMap.data, rDisMap.data, lDisMap.step);
}

int DispEst::JointWMF_GPU()
{
    if (ctx.empty()) return 1;
    return hipUtil::api().joint_wmf(ctx[0], 0, 0.f, 0, 0, lDisMap.data, rDisMap.data, lDisMap.step);
}

int DispEst::setGroundTruth(const Mat &gt, const Mat *mask)
{
    if (ctx.empty()) return 1;
    if (gt.rows != hei || gt.cols != wid || gt.channels != 1 || gt.depth != PSM_8U ||
        (mask && (mask->rows != hei || mask->cols != wid || mask->channels != 1 || mask->depth != PSM_8U || mask->step != gt.step))) {
        fprintf(stderr, "DE: setGroundTruth wants H x W CV_8UC1 planes of one step\n");
        return 1;
    }
    return hipUtil::api().score_set_truth(ctx[0], gt.data, mask ? mask->data : nullptr, gt.step);
}

int DispEst::setScoreParams(int scaleFactor, int errorThreshold, int maskMode)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().score_set_params(ctx[0], scaleFactor, errorThreshold, maskMode);
}

int DispEst::Score(int source, struct psm_score *rec, Mat *lDisp, Mat *eDisp)
{
    if (ctx.empty() || !rec) return 1;
    if (hipUtil::api().score(ctx[0], source, rec)) return 1;      // (several devices: ctx[0] holds the gathered maps)
    for (Mat *m : {lDisp, eDisp})
        if (m && (m->rows != hei || m->cols != wid || m->channels != 1 || m->depth != PSM_8U)) *m = Mat::zeros(hei, wid, 1, PSM_8U);
    if (!lDisp && !eDisp) return 0;
    return hipUtil::api().score_download(ctx[0], lDisp ? lDisp->data : nullptr, nullptr, eDisp ? eDisp->data : nullptr,
                                         lDisp ? lDisp->step : eDisp->step);
}

int DispEst::setReprojection(const double Q[16], int cropX, int cropY, float zMin, float zMax)
{
    if (ctx.empty()) return 1;
    if (hipUtil::api().reproject_set_q(ctx[0], Q, cropX, cropY)) return 1;
    return zMin < zMax ? hipUtil::api().reproject_set_range(ctx[0], zMin, zMax) : 0;
}

int DispEst::Reproject(int source, uint32_t *count, bool useMask, Mat *xyz, Mat *z)
{
    if (ctx.empty() || !count) return 1;
    const int outputs = PSM_DEPTH_CLOUD | (xyz ? PSM_DEPTH_XYZ : 0) | (z ? PSM_DEPTH_Z : 0);
    if (hipUtil::api().reproject(ctx[0], source, outputs, useMask ? PSM_DEPTH_USE_MASK : 0, count)) return 1;      // (several devices: ctx[0] holds the gathered maps)
    if (xyz && (xyz->rows != hei || xyz->cols != wid || xyz->channels != 3 || xyz->depth != PSM_32F)) *xyz = Mat::zeros(hei, wid, 3, PSM_32F);
    if (z && (z->rows != hei || z->cols != wid || z->channels != 1 || z->depth != PSM_32F)) *z = Mat::zeros(hei, wid, 1, PSM_32F);
    // (the planes of Mat::zeros are packed; psm_reproject_download takes one stride for both: that of z)
    if (xyz && hipUtil::api().reproject_download(ctx[0], (float *)xyz->data, nullptr, xyz->step / 3)) return 1;
    if (z && hipUtil::api().reproject_download(ctx[0], nullptr, (float *)z->data, z->step)) return 1;
    cloud_.resize(*count);
    uint32_t written = 0;
    static_assert(sizeof(Point) == 16, "the cloud's record is 16 bytes");
    if (hipUtil::api().reproject_download_cloud(ctx[0], cloud_.data(), *count, &written) || written != *count) return 1;
    return 0;
}

int DispEst::setWLS(float lambda, float sigma, int iterations)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().wls_set_params(ctx[0], lambda, sigma, iterations);
}

int DispEst::setWLSConfidence(int terms, int lrThresh, int radius, int varShift)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().wls_set_confidence(ctx[0], terms, lrThresh, radius, varShift);
}

int DispEst::wlsConfidence(std::vector<uint8_t> *conf, std::vector<int16_t> *right16)
{
    if (ctx.empty()) return 1;
    if (conf) conf->resize((size_t)hei * wid);
    if (right16) right16->resize((size_t)hei * wid);
    return hipUtil::api().wls_download_confidence(ctx[0], conf ? conf->data() : nullptr, 0, right16 ? right16->data() : nullptr, 0);
}

int DispEst::wlsConfTime(double *ms) { return ctx.empty() ? 1 : hipUtil::api().wls_conf_time(ctx[0], ms); }

int DispEst::WLS_GPU(int source, bool useMask, std::vector<int16_t> *disp16, Mat *q, bool confidence)
{
    if (ctx.empty()) return 1;
    if (hipUtil::api().wls_filter(ctx[0], source, (useMask ? PSM_WLS_USE_MASK : 0) | (confidence ? PSM_WLS_CONFIDENCE : 0))) return 1;      // (several devices: ctx[0] holds the gathered maps)
    if (disp16) {
        disp16->resize((size_t)hei * wid);
        if (hipUtil::api().wls_download(ctx[0], disp16->data(), nullptr, nullptr, nullptr, 0)) return 1;
    }
    if (q && (q->rows != hei || q->cols != wid || q->channels != 1 || q->depth != PSM_32F)) *q = Mat::zeros(hei, wid, 1, PSM_32F);
    if (q && hipUtil::api().wls_download(ctx[0], nullptr, (float *)q->data, nullptr, nullptr, q->step)) return 1;
    return 0;
}

int DispEst::WLSWait() { return ctx.empty() ? 1 : hipUtil::api().wls_wait(ctx[0]); }
int DispEst::WLSPublish(bool on) { return ctx.empty() ? 1 : hipUtil::api().wls_publish(ctx[0], on ? 1 : 0); }
int DispEst::wlsTime(double *ms) { return ctx.empty() ? 1 : hipUtil::api().wls_time(ctx[0], ms); }

int DispEst::setSGBMParams(int blockSize, int P1, int P2, int uniquenessRatio, int disp12MaxDiff)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_set_params(ctx[0], blockSize, P1, P2, uniquenessRatio, disp12MaxDiff);
}

int DispEst::SGBM_GPU(std::vector<int16_t> &disp16)
{
    if (ctx.size() != 1) {
        fprintf(stderr, "DispEst: SGBM_GPU runs on single-device objects only\n");
        return 1;
    }
    disp16.resize((size_t)hei * wid);
    return hipUtil::api().sgm_compute(ctx[0]) || hipUtil::api().sgm_download_disparity(ctx[0], disp16.data(), 0);
}

int DispEst::SGBMSelect()
{
    if (ctx.size() != 1) {
        fprintf(stderr, "DispEst: SGBMSelect runs on single-device objects only\n");
        return 1;
    }
    return hipUtil::api().sgm_select_maps(ctx[0], lDisMap.data, rDisMap.data, lDisMap.step);
}

int DispEst::sgbmMapsTime(double *ms)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_maps_time(ctx[0], ms);
}

int DispEst::grayRun(const Mat &gl, const Mat &gr, int rate)
{
    const char *who = rate ? "GrayFGF_GPU" : "Gray_GPU";
    if (ctx.size() != 1) {
        fprintf(stderr, "DispEst: %s runs on single-device objects only\n", who);
        return 1;
    }
    if (gl.channels != 1 || gr.channels != 1 || gl.rows != hei || gl.cols != wid || gr.rows != hei || gr.cols != wid || gl.depth != gr.depth ||
        gl.step != gr.step) {
        fprintf(stderr, "DispEst: %s wants two one-channel Mats of the object's size, of one depth and step\n", who);
        return 1;
    }
    const int depth = gl.depth == PSM_32F ? PSM_IMG_F32 : PSM_IMG_U8;
    if (rate) return hipUtil::api().gray_compute_fgf(ctx[0], gl.data, gr.data, gl.step, depth, rate, lDisMap.data, rDisMap.data, lDisMap.step);
    return hipUtil::api().gray_compute(ctx[0], gl.data, gr.data, gl.step, depth, lDisMap.data, rDisMap.data, lDisMap.step);
}

int DispEst::Gray_GPU(const Mat &gl, const Mat &gr) { return grayRun(gl, gr, 0); }

int DispEst::GrayFGF_GPU(const Mat &gl, const Mat &gr)
{
    if (subsample_rate != 2 && subsample_rate != 4 && subsample_rate != 8) {
        fprintf(stderr, "DispEst: GrayFGF_GPU: subsample_rate %u not in {2,4,8}\n", subsample_rate);
        return 1;
    }
    return grayRun(gl, gr, (int)subsample_rate);
}

int DispEst::grayTime(double *ms)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().gray_time(ctx[0], ms);
}

int DispEst::setSGBMSpeckle(int speckleWindowSize, int speckleRange)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_set_speckle(ctx[0], speckleWindowSize, speckleRange);
}

int DispEst::setSGBMPreFilterCap(int preFilterCap)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_set_prefilter(ctx[0], preFilterCap);
}

int DispEst::setSGBMMode(int mode)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_set_mode(ctx[0], mode);
}

int DispEst::setSGBMRange(int minDisparity, int numDisparities)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_set_range(ctx[0], minDisparity, numDisparities);
}

int DispEst::setSGBMCensus(int winW, int winH)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_set_census(ctx[0], winW, winH);
}

int DispEst::sgbmSpeckleTime(double *ms)
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_speckle_time(ctx[0], ms);
}

int DispEst::sgbmTimes(double ms[3])
{
    if (ctx.empty()) return 1;
    return hipUtil::api().sgm_times(ctx[0], ms);
}

int DispEst::computeFrame(const Mat *nextL, const Mat *nextR, bool have_prev)
{
    if (ctx.size() != 1) return 1;           // (a multi-device host gathers stripes: use the stage calls)
    const HipApi &api = hipUtil::api();
    psm_ctx *c = ctx[0];
    int rc = api.cost_construct(c);
    if (nextL && nextR)
        rc |= api.upload_pair_async(c, nextL->data, nextR->data, nextL->channels, nextL->step,
                                    nextL->depth == PSM_32F ? PSM_IMG_F32 : PSM_IMG_U8);
    rc |= api.cost_filter(c);
    rc |= api.disp_select(c, nullptr, nullptr, 0);
    if (have_prev) rc |= api.download_maps_wait(c, lDisMap.data, rDisMap.data, lDisMap.step);
    rc |= api.download_maps_async(c);
    return rc;
}

int DispEst::computeVideoFrame(const Mat *next, bool have_prev)
{
    if (ctx.size() != 1 || (next && !frameOk(*next))) return 1;
    const HipApi &api = hipUtil::api();
    psm_ctx *c = ctx[0];
    int rc = api.cost_construct(c);
    if (next) rc |= api.upload_pair_rectified_async(c, next->data, next->data + 3 * (size_t)rect_src_w, 3, next->step);
    rc |= api.cost_filter(c);
    rc |= api.disp_select(c, nullptr, nullptr, 0);
    if (have_prev) rc |= api.download_maps_wait(c, lDisMap.data, rDisMap.data, lDisMap.step);
    rc |= api.download_maps_async(c);
    return rc;
}

int DispEst::finishFrames()
{
    if (ctx.size() != 1) return 1;
    return hipUtil::api().download_maps_wait(ctx[0], lDisMap.data, rDisMap.data, lDisMap.step);
}

int DispEst::computeBatch(DispEst *const *des, int n)
{
    if (!des || n < 1) return 1;
    std::vector<psm_ctx *> cs;
    for (int i = 0; i < n; ++i) {
        if (!des[i] || des[i]->ctx.size() != 1) return 1;      // (a multi-device object shards ONE pair; batches are per device)
        cs.push_back(des[i]->ctx[0]);
    }
    const HipApi &api = hipUtil::api();
    int rc = api.compute_batch(cs.data(), n);
    for (int i = 0; i < n && !rc; ++i)
        rc |= api.download_maps(cs[i], des[i]->lDisMap.data, des[i]->rDisMap.data, des[i]->lDisMap.step);
    return rc;
}

int DispEst::SGBMBatch(DispEst *const *des, int n, std::vector<std::vector<int16_t>> &disp16)
{
    if (!des || n < 1) return 1;
    std::vector<psm_ctx *> cs;
    for (int i = 0; i < n; ++i) {
        if (!des[i] || des[i]->ctx.size() != 1) {
            fprintf(stderr, "DispEst: SGBMBatch runs on single-device objects only\n");
            return 1;
        }
        cs.push_back(des[i]->ctx[0]);
    }
    const HipApi &api = hipUtil::api();
    int rc = api.sgm_compute_batch(cs.data(), n);
    disp16.resize(rc ? 0 : (size_t)n);
    for (int i = 0; i < n && !rc; ++i) {
        disp16[i].resize((size_t)des[i]->wid * des[i]->hei);
        rc |= api.sgm_download_disparity(cs[i], disp16[i].data(), 0);
    }
    return rc;
}

int DispEst::SGBMSelectBatch(DispEst *const *des, int n)
{
    if (!des || n < 1) return 1;
    std::vector<psm_ctx *> cs;
    for (int i = 0; i < n; ++i) {
        if (!des[i] || des[i]->ctx.size() != 1) {
            fprintf(stderr, "DispEst: SGBMSelectBatch runs on single-device objects only\n");
            return 1;
        }
        cs.push_back(des[i]->ctx[0]);
    }
    const HipApi &api = hipUtil::api();
    int rc = api.sgm_select_maps_batch(cs.data(), n);
    for (int i = 0; i < n && !rc; ++i) rc |= api.download_maps(cs[i], des[i]->lDisMap.data, des[i]->rDisMap.data, des[i]->lDisMap.step);
    return rc;
}

int DispEst::JointWMFBatch(DispEst *const *des, int n, int radius, float sigma, int n_clusters, int max_iter)
{
    if (!des || n < 1) return 1;
    std::vector<psm_ctx *> cs;
    for (int i = 0; i < n; ++i) {
        if (!des[i] || des[i]->ctx.size() != 1) {
            fprintf(stderr, "DispEst: JointWMFBatch runs on single-device objects only\n");
            return 1;
        }
        cs.push_back(des[i]->ctx[0]);
    }
    const HipApi &api = hipUtil::api();
    int rc = api.joint_wmf_batch(cs.data(), n, radius, sigma, n_clusters, max_iter);
    for (int i = 0; i < n && !rc; ++i)
        rc |= api.download_maps(cs[i], des[i]->lDisMap.data, des[i]->rDisMap.data, des[i]->lDisMap.step);
    return rc;
}

int DispEst::PostProcessBatch(DispEst *const *des, int n, int stages)
{
    if (!des || n < 1) return 1;
    std::vector<psm_ctx *> cs;
    for (int i = 0; i < n; ++i) {
        if (!des[i] || des[i]->ctx.size() != 1) {
            fprintf(stderr, "DispEst: PostProcessBatch runs on single-device objects only\n");
            return 1;
        }
        cs.push_back(des[i]->ctx[0]);
    }
    const HipApi &api = hipUtil::api();
    int rc = api.post_process_batch(cs.data(), n, stages);
    for (int i = 0; i < n && !rc; ++i) {
        rc |= api.download_maps(cs[i], des[i]->lDisMap.data, des[i]->rDisMap.data, des[i]->lDisMap.step);
        rc |= api.download_valid(cs[i], des[i]->lValid.data, des[i]->rValid.data, des[i]->lValid.step);
    }
    return rc;
}

int DispEst::WLSBatch(DispEst *const *des, int n, int source, int flags)
{
    if (!des || n < 1) return 1;
    std::vector<psm_ctx *> cs;
    for (int i = 0; i < n; ++i) {
        if (!des[i] || des[i]->ctx.size() != 1) {
            fprintf(stderr, "DispEst: WLSBatch runs on single-device objects only\n");
            return 1;
        }
        cs.push_back(des[i]->ctx[0]);
    }
    return hipUtil::api().wls_filter_batch(cs.data(), n, source, flags);
}

int DispEst::GrayBatch(DispEst *const *des, int n, const Mat *gls, const Mat *grs) { return grayBatchRun(des, n, gls, grs, 0, "GrayBatch"); }

int DispEst::GrayFGFBatch(DispEst *const *des, int n, const Mat *gls, const Mat *grs)
{
    if (!des || n < 1 || !des[0]) return 1;
    const unsigned int s = des[0]->subsample_rate;
    if (s != 2 && s != 4 && s != 8) {
        fprintf(stderr, "DispEst: GrayFGFBatch: subsample_rate %u not in {2,4,8}\n", s);
        return 1;
    }
    return grayBatchRun(des, n, gls, grs, (int)s, "GrayFGFBatch");
}

int DispEst::grayBatchRun(DispEst *const *des, int n, const Mat *gls, const Mat *grs, int rate, const char *who)
{
    if (!des || n < 1 || !gls || !grs) return 1;
    std::vector<psm_ctx *> cs;
    std::vector<const void *> ls, rs;
    std::vector<uint8_t *> lm, rm;
    for (int i = 0; i < n; ++i) {
        if (!des[i] || des[i]->ctx.size() != 1) {
            fprintf(stderr, "DispEst: %s runs on single-device objects only\n", who);
            return 1;
        }
        const DispEst &d = *des[i];
        for (const Mat *m : {&gls[i], &grs[i]})
            if (m->channels != 1 || m->rows != d.hei || m->cols != d.wid || m->depth != gls[0].depth || m->step != gls[0].step) {
                fprintf(stderr, "DispEst: %s wants one-channel Mats of the objects' size, of one depth and step\n", who);
                return 1;
            }
        if (d.lDisMap.step != des[0]->lDisMap.step || d.rDisMap.step != des[0]->lDisMap.step) return 1;
        cs.push_back(d.ctx[0]);
        ls.push_back(gls[i].data);
        rs.push_back(grs[i].data);
        lm.push_back(d.lDisMap.data);
        rm.push_back(d.rDisMap.data);
    }
    const int depth = gls[0].depth == PSM_32F ? PSM_IMG_F32 : PSM_IMG_U8;
    if (rate)
        return hipUtil::api().gray_compute_fgf_batch(cs.data(), n, ls.data(), rs.data(), gls[0].step, depth, rate, lm.data(), rm.data(),
                                                     des[0]->lDisMap.step);
    return hipUtil::api().gray_compute_batch(cs.data(), n, ls.data(), rs.data(), gls[0].step, depth, lm.data(), rm.data(), des[0]->lDisMap.step);
}

double DispEst::stageTimeUs(int stage) const
{
    double us = 0;
    if (!ctx.empty()) hipUtil::api().stage_time_us(ctx[0], stage, &us);
    return us;
}

// ---- FrameRing ----
FrameRing::FrameRing(Mat l, Mat r, int d, int frames, int dtype)
{
    if (frames < 1) return;
    for (int i = 0; i < frames; ++i) {
        DispEst *de = new DispEst(l, r, d, MAX_CPU_THREADS, true, 1, dtype);
        if (!de->ok() || de->setOption(PSM_OPT_ASYNC, 1) || de->setOption(PSM_OPT_FRAMES_IN_FLIGHT, frames)) {
            delete de;
            for (DispEst *o : ring) delete o;
            ring.clear();
            return;
        }
        ring.push_back(de);
    }
    busy.assign(frames, 0);
}

FrameRing::~FrameRing()
{
    for (DispEst *o : ring) delete o;
}

int FrameRing::setOption(int option, int value)
{
    int rc = 0;
    for (DispEst *o : ring) rc |= o->setOption(option, value);
    return rc;
}

int FrameRing::deliver(int i, Mat *outL, Mat *outR)
{   // the maps of object i's last frame have been on their way since its push: wait for them, hand them over
    DispEst *de = ring[i];
    if (hipUtil::api().download_maps_wait(de->ctx[0], de->lDisMap.data, de->rDisMap.data, de->lDisMap.step)) return -1;
    busy[i] = 0;
    const size_t row = (size_t)de->wid;
    for (int y = 0; y < de->hei; ++y) {
        if (outL && outL->data) memcpy(outL->ptr<unsigned char>(y), de->lDisMap.ptr<unsigned char>(y), row);
        if (outR && outR->data) memcpy(outR->ptr<unsigned char>(y), de->rDisMap.ptr<unsigned char>(y), row);
    }
    return 1;
}

int FrameRing::setRectification(const Rectification &rect)
{
    if (ring.empty()) return -1;
    int rc = 0;
    for (DispEst *o : ring) rc |= o->setRectification(rect);
    return rc;
}

int FrameRing::push(const Mat &l, const Mat &r, Mat *outL, Mat *outR) { return push_any(&l, &r, nullptr, outL, outR); }
int FrameRing::push_frame(const Mat &vFrame, Mat *outL, Mat *outR) { return push_any(nullptr, nullptr, &vFrame, outL, outR); }

int FrameRing::push_any(const Mat *l, const Mat *r, const Mat *vFrame, Mat *outL, Mat *outR)
{
    if (ring.empty()) return -1;
    const HipApi &api = hipUtil::api();
    const int i = (int)(pushed % (long long)ring.size());
    int got = 0;
    if (busy[i]) {
        got = deliver(i, outL, outR);
        if (got < 0) return got;
        ++flushed;
    }
    DispEst *de = ring[i];
    psm_ctx *c = de->ctx[0];
    if (vFrame) {
        if (!de->frameOk(*vFrame)) return -1;
        if (api.upload_pair_rectified_async(c, vFrame->data, vFrame->data + 3 * (size_t)de->rect_src_w, 3, vFrame->step)) return -1;
    } else if (api.upload_pair_async(c, l->data, r->data, l->channels, l->step, l->depth == PSM_32F ? PSM_IMG_F32 : PSM_IMG_U8)) return -1;
    if (api.cost_construct(c) || api.cost_filter(c) || api.disp_select(c, nullptr, nullptr, 0) || api.download_maps_async(c)) return -1;
    busy[i] = 1;
    ++pushed;
    return got;
}

int FrameRing::flush(Mat *outL, Mat *outR)
{
    if (ring.empty()) return -1;
    while (flushed < pushed) {
        const int i = (int)(flushed % (long long)ring.size());
        ++flushed;
        if (busy[i]) return deliver(i, outL, outR);
    }
    return 0;
}

}  // namespace psm
