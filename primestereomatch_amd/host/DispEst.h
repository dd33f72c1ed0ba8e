// DispEst.h - C++ host-side mirror of the reference's DispEst class (include/DispEst.h:21-109)
// for the accelerator ('m' / OCL_DE) compute mode, on top of the C ABI of libprimesm_hip.so.
//
// Kept from the reference: constructor signature (l, r, d, t, useAccel), setInputImages /
// setThreads / setSubsampleRate, CostConst_GPU / CostFilter_GPU / DispSelect_GPU /
// PostProcess_GPU, the public outputs lDisMap / rDisMap (8-bit, one byte per pixel), `int`
// returns with 0 = ok (the reference's *_GPU methods always return 0, src/DispEst.cpp:272-328;
// here a failing device call returns 1 and prints, like the _cl wrappers).
// cv::Mat is replaced by the POD view psm::Mat below because OpenCV is not part of this build;
// field names follow cv::Mat (rows, cols, data, step).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hipUtil.h"

namespace psm {

enum { PSM_8U = 0, PSM_32F = 1 };  // cv depth codes the path uses (CV_8U, CV_32F)

struct Mat {
    int rows = 0, cols = 0, channels = 0, depth = PSM_8U;
    size_t step = 0;  // bytes per row
    unsigned char *data = nullptr;
    std::vector<unsigned char> store;  // owning storage when created with create()

    Mat() {}
    Mat(int r, int c, int ch, int dp, void *ext, size_t stp = 0)
        : rows(r), cols(c), channels(ch), depth(dp), step(stp ? stp : (size_t)c * ch * (dp == PSM_32F ? 4 : 1)),
          data((unsigned char *)ext) {}
    static Mat zeros(int r, int c, int ch, int dp)
    {
        Mat m;
        m.rows = r; m.cols = c; m.channels = ch; m.depth = dp;
        m.step = (size_t)c * ch * (dp == PSM_32F ? 4 : 1);
        m.store.assign(m.step * r, 0);
        m.data = m.store.data();
        return m;
    }
    int type() const { return depth * 8 + channels; }
    template <typename T> T *ptr(int y) { return (T *)(data + step * y); }
    template <typename T> const T *ptr(int y) const { return (const T *)(data + step * y); }
};

#define MAX_CPU_THREADS 8  // include/ComFunc.h:52

// Video mode (src/StereoMatch.cpp:138-153,464-466): the CV_16SC2 maps of both cameras (mapl / mapr: dense map_h x map_w, [..][2]
// int16 and uint16; from initUndistortRectifyMap or psm_rectify_build_maps), the size of the eye images they index and the
// origin of cropBox in the rectified image (its size is the DispEst object's).  The maps are copied to the device by
// setRectification; the host arrays need not outlive the call.
struct Rectification {
    const int16_t *map_xy[2] = {nullptr, nullptr};
    const uint16_t *map_frac[2] = {nullptr, nullptr};
    int map_w = 0, map_h = 0, src_w = 0, src_h = 0, crop_x = 0, crop_y = 0;
};

class DispEst {
public:
    // l, r: H x W x 3 images, cv::imread channel order, CV_8U or CV_32F (already scaled by
    // 1/255.0f, src/StereoMatch.cpp:193-198).  d: maxDis; t: host threads (interface parity);
    // ocl: accelerator available (the reference's gotOCLDev).  ndev > 1: the first ndev devices of this process each
    // take a stripe of ceil(H / ndev) output rows of both maps (all disparities of both volumes: the WTA finishes on the
    // device, only finished map rows are gathered - psm_set_rows / psm_gather_rows_ctx).
    DispEst(Mat l, Mat r, const int d, int t, bool ocl, int ndev = 1, int dtype = PSM_F32);
    ~DispEst(void);

    Mat lDisMap;
    Mat rDisMap;
    Mat lValid;
    Mat rValid;

    int setInputImages(Mat l, Mat r);
    // Video mode: after setRectification, setInputFrame takes the camera's side-by-side frame (src_h x 2 src_w, CV_8UC3), splits
    // it by pointer arithmetic - lFrame = vFrame(Rect(0, 0, cols/2, rows)), rFrame = vFrame(Rect(cols/2, ...)), no copy - and the
    // device remaps (INTER_LINEAR) and crops both eyes; the pair the object then holds is the rectified, cropped one
    // (downloadImages: H x W CV_8UC3 Mats).  Replaces src/StereoMatch.cpp:138-153.
    int setRectification(const Rectification &rect);
    int setInputFrame(const Mat &vFrame);
    int downloadImages(Mat *l, Mat *r);
    int setThreads(unsigned int newThreads);
    void setSubsampleRate(unsigned int newRate) { subsample_rate = newRate; }

    int CostConst_GPU();
    int CostFilter_GPU();
    int CostFilter_FGF_GPU();  // DispEst::CostFilter_FGF (src/DispEst.cpp:281-296) on the device, s = subsample_rate
    int DispSelect_GPU();
    // DispEst::PostProcess_GPU (src/DispEst.cpp:338-344) calls PP::processDM, whose live body is the CPU JointWMF (third-party, out
    // of scope: SURVEY.md 2) with lrCheck / fillInv / wgtMedian commented out (src/PP.cpp:405-412).  PostProcess_GPU here runs the
    // L-R check ONLY: lValid / rValid are filled, lDisMap / rDisMap stay the raw WTA maps (as in rounds 1-4; round 5 briefly made
    // it run all three stages - callers reading raw maps after it got filtered ones).  ProcessDM_GPU() is that commented-out
    // sequence - lrCheck, fillInv, wgtMedian - on the device: afterwards lDisMap / rDisMap hold the filled, filtered maps.
    int PostProcess_GPU();
    int ProcessDM_GPU();
    int LRCheck_GPU();         // lrCheck (src/PP.cpp:17-50): lValid / rValid; the maps stay untouched
    int FillInvalid_GPU();     // fillInv (src/PP.cpp:52-143): fills the pixels the last L-R check marked invalid
    // wgtMedian (src/PP.cpp:145-247) for the pixels the last L-R check marked invalid; same result as the reference's sequential
    // in-place form
    int WgtMedian_GPU();
    // The live body of PP::processDM (src/PP.cpp:417-422): JointWMF::filter on both maps, on the device (psm_joint_wmf with the
    // reference's radius, sigma and cluster count); lDisMap / rDisMap receive the filtered maps.  PostProcess_GPU is unchanged.
    int JointWMF_GPU();

    // The second algorithm, STEREO_SGBM: ssgbm->compute(lFrame, rFrame, imgDisparity16S) (src/StereoMatch.cpp:169-187) on the device
    // over the pair setInputImages gave, CV_8U or CV_32F (quantised on the device as convertTo(CV_8U, 255) does); the parameters
    // are those of setupOpenCVSGBM (:639-660) unless setSGBMParams changed them (0: the default of the first three).  disp16:
    // H x W int16 (imgDisparity16S, packed rows) - disparity * 16, -16 where invalid; resized by the call.  Independent of the GIF stages: lDisMap / rDisMap and
    // the masks stay as they are.  Single-device objects only (the paths cross the whole image).  sgbmTimes: device ms of the
    // block costs, the paths and select + check of the last call, if setOption(PSM_OPT_PROFILE, 1) was in force.
    int setSGBMParams(int blockSize, int P1, int P2, int uniquenessRatio, int disp12MaxDiff);
    int SGBM_GPU(std::vector<int16_t> &disp16);
    int sgbmTimes(double ms[3]);
    // The step StereoSGBM ends with: filterSpeckles(disp16, -16, speckleWindowSize, 16 * speckleRange) on the map of every following
    // SGBM_GPU (setupOpenCVSGBM: 100, 32).  Window 0, the setting of a new object: off.  sgbmSpeckleTime: device ms of the filter in
    // the last timed SGBM_GPU.
    int setSGBMSpeckle(int speckleWindowSize, int speckleRange);
    int sgbmSpeckleTime(double *ms);
    // StereoSGBM's pixel cost for every following SGBM_GPU: Birchfield-Tomasi over Sobel-prefiltered images, preFilterCap in 1 .. 63
    // (setupOpenCVSGBM: 63).  0, the setting of a new object: the SAD cost.
    int setSGBMPreFilterCap(int preFilterCap);
    // ssgbm->setMode for every following SGBM_GPU (the reference's `m` key, src/main.cpp:114-168): PSM_SGM_MODE_SGBM (0),
    // PSM_SGM_MODE_HH (1, the setting of a new object: all eight directions), PSM_SGM_MODE_SGBM_3WAY (2), PSM_SGM_MODE_HH4 (3) -
    // OpenCV's enum values.  SGBMBatch wants one mode on all its objects.
    int setSGBMMode(int mode);
    // StereoSGBM::create's minDisparity and numDisparities for every following SGBM_GPU (psm_sgm_set_range): the disparities
    // minDisparity .. minDisparity + numDisparities - 1, minDisparity in [-1024, 1024], numDisparities in [2, 1024] or 0, the
    // setting of a new object: maxDis.  Invalid pixels of the map are (minDisparity - 1) * 16.  SGBMBatch wants one range on all
    // its objects.
    int setSGBMRange(int minDisparity, int numDisparities);
    // The census cost for every following SGBM_GPU (psm_sgm_set_census): the Hamming distance of census codes over a winW x winH
    // window, both odd, 3 .. 9 by 3 .. 7 - unchanged when the two cameras differ in gain or exposure.  (0, 0), the setting of a new
    // object: off.  Refused by SGBM_GPU together with a preFilterCap > 0.  SGBMBatch wants one window on all its objects.
    int setSGBMCensus(int winW, int winH);
    // The 8-bit maps of both views from the summed path costs of the last SGBM_GPU (psm_sgm_select_maps): lDisMap - the
    // winner-takes-all disparity - and rDisMap - the search along the epipolar line in the same costs - are filled and become the
    // object's device maps, so LRCheck_GPU, FillInvalid_GPU, WgtMedian_GPU, JointWMF_GPU and Score(PSM_SCORE_GIF) run behind the
    // SGBM stage as behind DispSelect_GPU.  The range of that SGBM_GPU must lie inside [0, maxDis); the int16 map and the GIF
    // stages' volumes are untouched.  sgbmMapsTime: device ms of the launch under PSM_OPT_PROFILE.
    int SGBMSelect();
    int sgbmMapsTime(double *ms);
    // The GIF stages for a monochrome pair in one call (psm_gray_compute): gl, gr are H x W one-channel Mats of the object's size,
    // CV_8U or CV_32F (scaled by 1/255.0f already) - cost build, the one-channel guided filter (FastGuidedFilter's dispatch on
    // I.channels(), src/fastguidedfilter.cpp:38-49) and the selection; lDisMap / rDisMap are filled and become the object's device
    // maps, so LRCheck_GPU, FillInvalid_GPU and Score(PSM_SCORE_GIF) run behind it.  The pair of setInputImages, the volumes and
    // whatever CostFilter_GPU left pending are untouched (an object built for mono frames alone is given blank colour Mats).
    // Single-device objects only.  grayTime: device ms of the call under PSM_OPT_PROFILE.
    int Gray_GPU(const Mat &gl, const Mat &gr);
    int grayTime(double *ms);
    // ... with the Fast Guided Filter in place of the full-resolution one (psm_gray_compute_fgf: FastGuidedFilterMono,
    // src/fastguidedfilter.cpp:89-119), s = subsample_rate (setSubsampleRate: 2, 4 or 8) - to Gray_GPU what CostFilter_FGF_GPU is to
    // CostFilter_GPU.  Everything else is Gray_GPU's.
    int GrayFGF_GPU(const Mat &gl, const Mat &gr);

    // The steps of StereoMatch::compute behind the maps, on the device (psm_score): setGroundTruth uploads the dataset's ground truth
    // and (mask non-NULL) error mask once, H x W CV_8UC1 each; setScoreParams: scale_factor, error_threshold, PSM_MASK_NONE / NONOCC /
    // DISC (a new object: 4, 4, NONOCC).  Score writes the display map of `source` - PSM_SCORE_GIF: the current lDisMap as
    // convertTo(CV_8U, scale_factor) makes it (src/StereoMatch.cpp:248); PSM_SCORE_SGM: the map of the last SGBM_GPU through minMaxLoc,
    // convertTo, / 4, * scale_factor (:181-185); PSM_SCORE_SGM_INT: its integer disparities scaled like the GIF maps - and the error
    // record of :275-309 against the truth; lDisp / eDisp (may be NULL; resized) receive the display map and the error plane.
    // scoreBP / scoreAvgErr: the two figures of the reference's "%BP = ... Avg Err = ..." line from the record's integers.
    int setGroundTruth(const Mat &gt, const Mat *mask);
    int setScoreParams(int scaleFactor, int errorThreshold, int maskMode);
    int Score(int source, struct psm_score *rec, Mat *lDisp = nullptr, Mat *eDisp = nullptr);
    static double scoreBP(const struct psm_score &r) { return 100.0 * r.bad / r.pixels; }
    static double scoreAvgErr(const struct psm_score &r) { return r.unit ? ((double)r.err_sum / r.pixels) / r.unit : 0.0; }
    // From disparity to depth on the device (psm_reproject): cv::reprojectImageTo3D with the Q of cv::stereoRectify - the
    // reference's camProps.Q (src/StereoMatch.cpp:456-458) - and the compacted, coloured point cloud.  setReprojection: Q (16
    // doubles, row-major), the (x, y) of this object's image inside the rectified one (the cropBox of :474-481), and the range
    // z_min < z <= z_max the cloud keeps (zMin >= zMax: the range stays as it is; a new object: (0, FLT_MAX)).  Reproject: `source`
    // PSM_DEPTH_GIF (the current lDisMap; useMask: without the pixels the L-R check rejected) or PSM_DEPTH_SGM (the map of the
    // last SGBM_GPU); *count: the kept pixels; xyz (H x W CV_32FC3) / z (H x W CV_32FC1) receive the dense planes if given;
    // cloud() then holds the records of the kept pixels in raster order.
    struct Point { float x, y, z; uint8_t b, g, r, a; };
    int setReprojection(const double Q[16], int cropX = 0, int cropY = 0, float zMin = 0.f, float zMax = 0.f);
    int Reproject(int source, uint32_t *count, bool useMask = false, Mat *xyz = nullptr, Mat *z = nullptr);
    const std::vector<Point> &cloud() const { return cloud_; }
    // WLS smoothing of the sub-pixel map on the device (psm_wls_filter): the confidence-weighted, edge-aware global smoothing users
    // of cv::StereoSGBM apply behind it (cv::ximgproc::DisparityWLSFilter's kind, by the Fast Global Smoother), guided by the left
    // image - the holes of the int16 map are filled from their surroundings, the sixteenths stay.  setWLS: lambda > 0, sigma > 0,
    // iterations in 1..4 (a new object: 8000, 1.5, 3).  WLS_GPU: `source` PSM_WLS_SGM (the map of the last SGBM_GPU) or PSM_WLS_GIF
    // (the current lDisMap times 16; useMask: without the pixels the L-R check rejected); disp16 (H x W int16, in 16ths) and q
    // (H x W CV_32FC1, the unrounded quotient) receive the result if given.  WLSWait: behind a WLS_GPU under PSM_OPT_ASYNC.
    // WLSPublish(true): Score and Reproject with an SGM source read the filtered map from now on - the way to a dense cloud that
    // keeps the sixteenths.  wlsTime: device ms of the launches under PSM_OPT_PROFILE.
    int setWLS(float lambda = 8000.f, float sigma = 1.5f, int iterations = 3);
    int WLS_GPU(int source, bool useMask = false, std::vector<int16_t> *disp16 = nullptr, Mat *q = nullptr, bool confidence = false);
    // The graded confidence (PSM_WLS_CONFIDENCE, PSM_WLS_SGM only; the definition is tests/wls_conf_model.py): with `confidence` WLS_GPU
    // - and WLSBatch with the flag - starts the solve with a confidence byte per pixel from the L-R consistency of the SGM stage's
    // summed costs and the variance of the map around the pixel.  setWLSConfidence: terms PSM_WLS_CONF_LR | PSM_WLS_CONF_VAR,
    // lr_thresh in 1..32767 (16ths), radius in 1..4, var_shift in 0..16 (a new object: both, 24, 2, 8).  wlsConfidence: the planes
    // of the last such run (either may be null; right16 needs the L-R term).  wlsConfTime: device ms of the two launches it adds.
    int setWLSConfidence(int terms = PSM_WLS_CONF_LR | PSM_WLS_CONF_VAR, int lrThresh = 24, int radius = 2, int varShift = 8);
    int wlsConfidence(std::vector<uint8_t> *conf, std::vector<int16_t> *right16);
    int wlsConfTime(double *ms);
    int WLSWait();
    int WLSPublish(bool on);
    int wlsTime(double *ms);

    // Frame loop (src/main.cpp:64-73) with the PCIe legs next to the kernels (single-device hosts): one call per frame -
    // CostConst (adopts the pair staged by the previous call), stages `next` pair (may be NULL at the end of the stream: its
    // Mats are free again on return), CostFilter, DispSelect on the device, hands over the PREVIOUS frame's maps in
    // lDisMap / rDisMap (have_prev: there was one) and starts this frame's download.  finishFrames() returns the last maps.
    int computeFrame(const Mat *nextL, const Mat *nextR, bool have_prev);
    // ... the same loop in video mode: `next` is the next side-by-side camera frame (setInputFrame's argument), rectified on the
    // copy stream behind its H2D copy
    int computeVideoFrame(const Mat *next, bool have_prev);
    int finishFrames();

    // Several pairs of one geometry per launch (the reference loops over pairs / datasets, src/main.cpp:64-73,
    // src/StereoMatch.cpp:556-607): CostConst_GPU + CostFilter_GPU + DispSelect_GPU of n single-device DispEst objects in shared
    // launches (psm_compute_batch); every object's lDisMap / rDisMap receive its maps.
    static int computeBatch(DispEst *const *des, int n);
    // ... and the second algorithm: SGBM_GPU of n single-device objects of one geometry and one set of SGBM settings in shared
    // launches (psm_sgm_compute_batch); disp16[i]: object i's H x W int16 map, as SGBM_GPU returns it.  Every object is afterwards
    // where its own SGBM_GPU would have left it; sgbmTimes / sgbmSpeckleTime of des[0] report the batch.
    static int SGBMBatch(DispEst *const *des, int n, std::vector<std::vector<int16_t>> &disp16);
    // SGBMSelect of n such objects in one launch (psm_sgm_select_maps_batch); every object's lDisMap / rDisMap receive its maps.
    static int SGBMSelectBatch(DispEst *const *des, int n);
    // ... and the live post-filter: JointWMF_GPU of n single-device objects of one geometry in shared launches (psm_joint_wmf_batch;
    // 0: the reference's radius, sigma, cluster count and iteration limit), each object's device maps with its own pair - after
    // computeBatch, say, with or without the L-R check between; every object's lDisMap / rDisMap receive its filtered maps.
    static int JointWMFBatch(DispEst *const *des, int n, int radius = 0, float sigma = 0, int n_clusters = 0, int max_iter = 0);
    // ... and PP::processDM's own sequence: the stages named in `stages` (PSM_PP_LR_CHECK | PSM_PP_FILL | PSM_PP_WGT_MEDIAN, run in
    // that order) of n single-device objects of one geometry in shared launches (psm_post_process_batch), the sweep chains of all
    // maps side by side; every object's lDisMap / rDisMap / lValid / rValid receive its results.
    static int PostProcessBatch(DispEst *const *des, int n, int stages);
    // ... and the WLS smoothing: WLS_GPU(source, flags & PSM_WLS_USE_MASK) of n single-device objects of one geometry and one
    // iteration count in one set of launches (psm_wls_filter_batch), each object's map with its own guide, lambda and sigma.
    // Every object is afterwards where its own WLS_GPU would have left it (WLSPublish, WLSWait under PSM_OPT_ASYNC on des[0]);
    // wlsTime of des[0] reports the batch.
    static int WLSBatch(DispEst *const *des, int n, int source = PSM_WLS_SGM, int flags = 0);
    // ... and the monochrome path: Gray_GPU(gls[i], grs[i]) of n single-device objects of one geometry in one set of launches
    // (psm_gray_compute_batch); the 2 n Mats are one-channel, of the objects' size and of one depth and step.  Every object's
    // lDisMap / rDisMap are filled and it is afterwards where its own Gray_GPU would have left it; grayTime of des[0] reports the
    // batch.
    static int GrayBatch(DispEst *const *des, int n, const Mat *gls, const Mat *grs);
    // ... GrayFGF_GPU of the n objects (psm_gray_compute_fgf_batch), at the subsample_rate of des[0]
    static int GrayFGFBatch(DispEst *const *des, int n, const Mat *gls, const Mat *grs);

    // psm_set_option on every device's context (PSM_OPT_FLAGS: e.g. PSM_FLAG_FMA_SOLVE - the maps of a reference binary built for an
    // FMA target -, PSM_OPT_SEG_ROWS, PSM_OPT_GATHER_STAGED, PSM_OPT_FRAMES_IN_FLIGHT ...; include/primesm_hip.h).  0 = ok.
    int setOption(int option, int value);

    bool ok() const { return !ctx.empty(); }
    double stageTimeUs(int stage) const;

private:
    friend class FrameRing;
    Mat lImg, rImg;
    int hei, wid, maxDis, threads;
    bool useOCL;
    unsigned int subsample_rate = 4;
    int grayRun(const Mat &gl, const Mat &gr, int rate);      // Gray_GPU (rate 0) and GrayFGF_GPU
    static int grayBatchRun(DispEst *const *des, int n, const Mat *gls, const Mat *grs, int rate, const char *who);
    std::vector<psm_ctx *> ctx;  // one per device (row stripes of ceil(H / ndev) rows)
    std::vector<int> y0s, y1s;   // their stripes
    int rect_src_w = 0, rect_src_h = 0;   // setRectification: the eye images' size
    std::vector<Point> cloud_;            // Reproject: the records of the last call
    bool frameOk(const Mat &vFrame) const;
    bool whole_on_first = false; // the last filter ran on ctx[0] over the whole image (Fast Guided Filter path: no stripes)
};

// The frame loop of src/main.cpp:64-73 (one compute() per frame) with `frames` frames in the device's queues: that many DispEst
// objects of one geometry, each with its own streams, take the frames of a stream in turn, so a frame's short launches and the
// half-empty tail of its fused launch run beside the next frame's fused kernel (the Python
// form is primestereomatch_amd.FrameRing).  Every object is told PSM_OPT_FRAMES_IN_FLIGHT = frames.  The maps are those of the
// single-object calls, bit for bit.  Single-device objects only.
class FrameRing {
public:
    FrameRing(Mat l, Mat r, int d, int frames = 2, int dtype = PSM_F32);
    ~FrameRing();
    bool ok() const { return !ring.empty(); }
    int frames() const { return (int)ring.size(); }
    // Queues the pair (l, r).  Once the ring is full this first hands over the maps of the frame pushed frames() calls earlier:
    // outL / outR (H x W, 8-bit, may be NULL to drop them) are filled and 1 is returned; 0 = no maps yet; < 0 = a device call failed.
    int push(const Mat &l, const Mat &r, Mat *outL, Mat *outR);
    // Video mode: setRectification on every object of the ring, then push_frame instead of push with the side-by-side frame.
    int setRectification(const Rectification &rect);
    int push_frame(const Mat &vFrame, Mat *outL, Mat *outR);
    // The frames still in flight, oldest first, one per call: 1 = maps delivered, 0 = none left, < 0 = error.
    int flush(Mat *outL, Mat *outR);
    int setOption(int option, int value);      // on every object of the ring

private:
    int deliver(int i, Mat *outL, Mat *outR);
    int push_any(const Mat *l, const Mat *r, const Mat *vFrame, Mat *outL, Mat *outR);
    std::vector<DispEst *> ring;
    std::vector<char> busy;
    long long pushed = 0, flushed = 0;
};

}  // namespace psm
