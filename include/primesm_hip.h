/*
 * primesm_hip.h - C ABI of libprimesm_hip.so: the MI355X (gfx950) implementation of the
 * PRiMEStereoMatch DispEst hot path (CVC cost build -> CVF guided-image-filter aggregation
 * -> DispSel WTA) that takes the place of the reference's OpenCL side.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository).  Conventions are those of the reference's `_cl` classes:
 *   - every function returns 0 on success and non-zero on failure (CVC_cl::buildCV,
 *     src/CVC_cl.cpp:185-210); the message is available from psm_last_error();
 *   - calls are synchronous on return unless PSM_OPT_ASYNC is set (the reference issues
 *     clFinish after each launch, src/CVC_cl.cpp:193);
 *   - the caller owns host memory, the context owns all device memory
 *     (DispEst owns memoryObjects[12], src/DispEst.cpp:88-128,159-160);
 *   - a context is used from one thread at a time (the reference calls from a single
 *     worker thread, src/main.cpp:42,64-73).
 * Plain pointers and sizes only; no C++/torch types cross this boundary.  The library is
 * meant to be dlopen()ed by the host program (hipUtil in primestereomatch_amd/host takes
 * the place of oclUtil) the way the reference defers .cl compilation to run time
 * (src/oclUtil.cpp:438-496).
 */
#ifndef PRIMESM_HIP_H
#define PRIMESM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSM_ABI_VERSION 1

typedef struct psm_ctx psm_ctx;

/* element type of the cost volume ("float mode" / "8-bit char mode") */
enum { PSM_F32 = 0, PSM_U8 = 1 };
/* element type of host images handed to psm_upload_pair.  PSM_IMG_F32 images are used as they are (the reference hands
 * DispEst images already scaled by 1/255, src/StereoMatch.cpp:195-198).  The default (select) forms of psm_cost_filter carry the
 * 1/64 of the box filters as one exact power of two at the end, which is bit-identical to the reference's per-sum scaling while
 * no intermediate under- or overflows: float images whose non-zero magnitudes leave 2^-10 .. 2^10 (measured on the device when
 * they arrive) make psm_cost_filter run its storing form - the reference's arithmetic op for op, ~25 % slower - automatically. */
enum { PSM_IMG_U8 = 0, PSM_IMG_F32 = 1 };
/* volume side: the reference's buffers CV_LCV / CV_RCV (include/ComFunc.h:65) */
enum { PSM_LEFT = 0, PSM_RIGHT = 1 };
/* stages, in the order StereoMatch::compute times them (src/StereoMatch.cpp:225-242) */
enum { PSM_STAGE_CVC = 0, PSM_STAGE_CVF = 1, PSM_STAGE_DISPSEL = 2, PSM_STAGE_PP = 3,
       PSM_STAGE_COUNT = 4 };
/* kernels whose device time can be queried with psm_kernel_time_ms() */
enum { PSM_K_PREP = 0, PSM_K_CVC = 1, PSM_K_GUIDE = 2, PSM_K_CVF_A = 3, PSM_K_CVF_B = 4,
       PSM_K_WTA = 5, PSM_K_MERGE = 6, PSM_K_BOX = 7, PSM_K_LRC = 8, PSM_K_CVF_F = 9, PSM_K_FGF = 10, PSM_K_WMF = 11,
       PSM_K_JWMF = 12, PSM_K_COUNT = 13 };
/* options for psm_set_option */
enum {
    PSM_OPT_ASYNC = 0,          /* 1: stage calls only enqueue; use psm_synchronize()        */
    PSM_OPT_KERNEL_VARIANT = 1, /* 0: marching kernels (default), 1: direct per-voxel kernels */
    PSM_OPT_PROFILE = 2,        /* 1: bracket every kernel launch with hipEvents (psm_kernel_time_ms); 2: the fused filter
                                   kernel stamps its own start / end instead (psm_filter_launch_times) */
    PSM_OPT_SEG_ROWS = 3,       /* rows per y-segment of the marching kernels (0 = auto)      */
    PSM_OPT_WAVES = 4,          /* waves (disparity slices) per workgroup: 1,2,4,8            */
    PSM_OPT_FLAGS = 5,          /* PSM_FLAG_* bits below; no flag but PSM_FLAG_F32_TOL / PSM_FLAG_FMA_SOLVE changes any result */
    PSM_OPT_GRAPH = 6,          /* retired: 1 is refused by the product library (hipGraph replay of a batch's launches measured slower
                                   than the launches themselves on this runtime; experiment builds keep it), 0 is accepted */
    PSM_OPT_GATHER_STAGED = 7,  /* 1 (on the ROOT context): psm_gather_rows_ctx / psm_disp_merge_ctx move every stripe / shard through
                                   page-locked host memory instead of device / peer copies - what they do on their own between two
                                   devices for which hipDeviceCanAccessPeer says no; the option forces that path (test hook) */
    PSM_OPT_FRAMES_IN_FLIGHT = 8 /* F >= 1 (default 1): this context is one of F contexts of the same geometry whose frames are
                                   filtered at the same time, each on its own stream (the frame loop of src/main.cpp:64-73 with F
                                   frames queued).  A hint for the planner of the fused launches only - how the work is cut into
                                   segments and chunks; no result changes */
};

/* PSM_OPT_FLAGS bits.  The default (0) is the product path: cost volumes and filtered volumes stay virtual, the fused
 * kernel runs CVC + CVF + WTA in one pass (two phases from 112 local slices up).  The flags select the forms that
 * materialise a volume - what a host that reads volumes gets anyway, on demand - and test hooks. */
enum psm_flag {
    PSM_FLAG_MATERIALISE_COSTS = 128,   /* psm_cost_construct always writes the cost volumes (default: they stay virtual
                                           and the fused filter builds the costs on the fly; any other reader
                                           materialises them first) */
    PSM_FLAG_FGF_STORE = 4096,          /* psm_cost_filter_fgf always writes the filtered volumes (default: they stay
                                           virtual - low-resolution models - and the WTA consumes those directly) */
    PSM_FLAG_STORE_FILTERED = 8192,     /* psm_cost_filter always writes the filtered volumes (storing form of the fused
                                           kernel + a separate WTA; default: select forms, packed per-pixel minima) */
    PSM_FLAG_TWO_PHASE_ON = 1048576,    /* force / disable the two-phase selection of psm_cost_filter (default: on from */
    PSM_FLAG_TWO_PHASE_OFF = 2097152,   /* 112 local slices - every 8th (short stripes, large 8-bit images: 5th) slice through minima planes, the rest against
                                           the seeded key plane) */
    PSM_FLAG_WMF_DATAFLOW = 4194304,    /* psm_wgt_median runs its row-dataflow form only */
    PSM_FLAG_WMF_TWO_SWEEPS = 8388608,  /* ... at most 2 sweeps of its parallel form (test hook for the fall-back) */
    PSM_FLAG_WMF_NO_CACHE = 16777216,   /* ... without the cache of window weights (1.5 KB of device memory per invalid pixel):
                                           every evaluation forms its weights itself; same maps */
    PSM_FLAG_F32_TOL = 33554432,        /* float mode, default (select) path of psm_cost_filter: the TOLERANCE form of the fused kernel -
                                           level 1 of its horizontal window sums in fp32 instead of fp64 (fewer four-cycle
                                           instructions).  The ONLY flag that changes results: filtered costs within 1e-4 of
                                           the default form's (measured: <= 4e-5, no disparity changed on the test pairs), not
                                           bit-identical.  The storing form (psm_download_volume ...) stays exact; 8-bit mode
                                           ignores the flag.  Off by default. */
    PSM_FLAG_FMA_SOLVE = 67108864,      /* float mode: the 3x3 solve of the guided filter (src/CVF.cpp:129-147) with the fused
                                           multiply-adds GCC's default -ffp-contract=fast forms on an FMA target (the ARM boards
                                           the reference ran on): every x*y - z*w of the minors and of DET and every s + x*y of
                                           the three accumulations is one fma.  Bit-identical to the oracle's reading
                                           PSMO_VAR_FMA_SOLVE of those lines (maps, minima and filtered volumes); within 4e-4 of
                                           the default (the canon: the same lines compiled without contraction, e.g. x86-64).
                                           Applies to psm_cost_filter (select and storing forms); psm_compute_batch, the FGF
                                           variant and 8-bit mode refuse / ignore it.  Off by default. */
    PSM_FLAGS_ALL = 128 | 4096 | 8192 | 1048576 | 2097152 | 4194304 | 8388608 | 16777216 | 33554432 | 67108864
};

/* Number of usable HIP devices; 0 if none.  Replaces openCLdevicepoll()
 * (src/oclUtil.cpp:18-135) whose result StereoMatch receives as gotOCLDev
 * (src/main.cpp:29,37). */
int psm_device_count(void);

/* Create a context for W x H images and disparities [0, max_disp): device selection,
 * stream, the device buffers of enum buff_id (8 image/gradient planes, 2 volumes, 2 maps;
 * include/ComFunc.h:65, src/DispEst.cpp:88-128) and the CVF intermediates
 * (src/CVF_cl.cpp:115-159).  Replaces createContext/createCommandQueue/clCreateBuffer and
 * the three `_cl` constructors (src/DispEst.cpp:57-140).
 * dtype: PSM_F32 | PSM_U8.  8 <= W,H; 1 <= max_disp <= 256 (maps are 8-bit,
 * src/DispSel.cpp:105). */
int psm_create(psm_ctx **out, int width, int height, int max_disp, int dtype, int device);

/* As psm_create, for one rank of a disparity-sharded job: this context holds only the
 * slices d in [d_begin, d_end) of both volumes.  0 <= d_begin < d_end <=
 * max_disp. */
int psm_create_shard(psm_ctx **out, int width, int height, int max_disp, int d_begin, int d_end,
                     int dtype, int device);
/* The same job cut the other way (round 6): this context holds the slices d_first, d_first + d_step, d_first + 2 d_step, ... <
 * max_disp of both volumes - rank g of G owns d = g (mod G).  A rank's slices then span the whole disparity range, so the
 * slices that seed its key plane bound EVERY pixel's minimum and the two-phase selection works on a shard as it does on the
 * whole volume (a contiguous shard's seeds bound little: most pixels' minima lie in other ranks' slices).  The merge
 * (psm_disp_merge / psm_disp_merge_ctx: a signed minimum of packed keys) does not care how the slices were dealt
 * (DispSel::CVSelect, src/DispSel.cpp:96-104, is a minimum over d in any order with ties to the lowest d).  Such a context
 * runs the default select path only: CostConst / CostFilter / psm_disp_select_partial; everything that reads or writes a
 * volume refuses it.  0 <= d_first < max_disp, d_step >= 1 (1: the contiguous shard [d_first, max_disp)). */
int psm_create_shard_strided(psm_ctx **out, int width, int height, int max_disp, int d_first, int d_step,
                             int dtype, int device);

/* Releases everything the context owns (DispEst::~DispEst, src/DispEst.cpp:143-162). */
void psm_destroy(psm_ctx *ctx);

/* Last error text of this context (ctx == NULL: last creation error).  Replaces
 * checkSuccess/errorNumberToString (include/oclUtil.h:63-71, src/oclUtil.cpp:582-683). */
const char *psm_last_error(const psm_ctx *ctx);

int psm_set_option(psm_ctx *ctx, int option, int value);
/* Run all work of this context on an existing hipStream_t (NULL = the context's own). */
int psm_set_stream(psm_ctx *ctx, void *hip_stream);
int psm_synchronize(psm_ctx *ctx);
/* Give back the device / page-locked memory the context allocated ON FIRST USE and that holds no state between calls: the
 * weighted median's sweep scratch and weight cache (1.5 KB per invalid pixel), the minima planes of the fused filter, the gather /
 * bounce buffers of the single-process exchange, the 8-bit storing path's float work volume.  Synchronises the context first;
 * everything is allocated again by the call that needs it.  Maps, minima, volumes and images are untouched.  (The reference
 * allocates its CVF intermediates per call, src/CVF_cl.cpp:115-159; this library keeps them - this is how a long-running host
 * gets the memory back without destroying the context.) */
int psm_release_scratch(psm_ctx *ctx);

/* Copy a stereo pair to the device and planarise it.  Replaces the host half of
 * CVC_cl::buildCV (split + 8x map/memcpy, src/CVC_cl.cpp:95-160) and
 * DispEst::setInputImages (src/DispEst.cpp:164-170).  l, r: H rows of W interleaved
 * `channels`(=3, cv::imread order B,G,R) pixels, row pitch stride_bytes.
 * depth PSM_IMG_U8: values are scaled by 1/255.0f on the device exactly as
 * convertTo(CV_32F, 1/255.0f) does (src/StereoMatch.cpp:195-196); PSM_IMG_F32: used as is. */
int psm_upload_pair(psm_ctx *ctx, const void *l, const void *r, int channels, size_t stride_bytes,
                    int depth);

/* DispEst::CostConst_GPU (src/DispEst.cpp:272-276) == CVC_cl::buildCV: gray + x-gradient
 * of both images (CVC::preprocess arithmetic, src/CVC.cpp:41-46 - no +0.5) and both cost
 * volumes (CVC::buildCV_left/right arithmetic, src/CVC.cpp:122-179).  In the default float path all of it is lazy: the cost
 * volumes stay virtual (the fused filter builds the costs on the fly) and - since round 6 - so does the image preparation (the
 * guidance launch of psm_cost_filter forms gray and gradient itself); the call then only adopts the pair and resets the frame's
 * state.  Whatever reads the image planes or a volume earlier gets them prepared / materialised on demand. */
int psm_cost_construct(psm_ctx *ctx);

/* DispEst::CostFilter_GPU (src/DispEst.cpp:299-308) == CVF_cl::preprocess + filterCV for
 * the left then the right volume, with the arithmetic of CVF::preprocess and
 * GuidedFilter_cv (src/CVF.cpp:44-165).  Filters both volumes in place. */
int psm_cost_filter(psm_ctx *ctx);

/* One half of psm_cost_filter: preprocess + filter of volume `side` only (the reference runs the two
 * halves back to back, src/DispEst.cpp:302-305).  Lets a sharded host start exchanging the left
 * minima while the right volume is still being filtered. */
int psm_cost_filter_side(psm_ctx *ctx, int side);

/* DispEst::CostFilter_FGF (src/DispEst.cpp:281-296): the Fast Guided Filter variant of the aggregation,
 * FastGuidedFilterColor(I, GIF_R_WIN, GIF_EPS, subsample_rate) per slice (src/fastguidedfilter.cpp:124-209),
 * left then right volume, in place.  subsample_rate in {2, 4, 8} (the reference's default is 4,
 * src/DispEst.cpp:19); PSM_F32 contexts only; width/subsample_rate and height/subsample_rate must exceed
 * the blur radius 8/subsample_rate.  The reference has this on the CPU only ('m' mode has no FGF kernel). */
int psm_cost_filter_fgf(psm_ctx *ctx, int subsample_rate);

/* DispEst::DispSelect_GPU (src/DispEst.cpp:323-328) == DispSel_cl::CVSelect
 * (src/DispSel_cl.cpp:69-140) with DispSel::CVSelect arithmetic (src/DispSel.cpp:83-109).
 * lmap/rmap: H rows of W bytes, row pitch `stride` (cv::Mat lDisMap/rDisMap, CV_8UC1).
 * Either may be NULL: the maps then stay on the device (psm_download_maps).
 * Only valid on an unsharded context. */
int psm_disp_select(psm_ctx *ctx, uint8_t *lmap, uint8_t *rmap, size_t stride);

/* Sharded DispSel, step 1: local argmin over this context's slices with the global
 * semantics (d = 0 never a candidate, strict '<', lowest d wins ties).  Writes one packed
 * 64-bit key per pixel and side, keys[side][y][x] = (ordered(cost) << 32 | d) ^ (1<<63), so
 * that a signed 64-bit minimum over ranks selects (min cost, then lowest d).
 * dev_keys: DEVICE pointer to 2*H*W int64 (e.g. a torch tensor handed to RCCL), or NULL to
 * use the context's own buffer (psm_partial_keys). */
int psm_disp_select_partial(psm_ctx *ctx, void *dev_keys);
/* The same for one side only: dev_keys_side = DEVICE pointer to H*W int64 (NULL: the context's buffer). */
int psm_disp_select_partial_side(psm_ctx *ctx, int side, void *dev_keys_side);
/* Let the context write its packed minima (both sides, 2*H*W int64) straight into a caller-owned DEVICE buffer - e.g. the
 * torch tensor a collective is about to reduce - instead of its own (NULL: back to its own).  Call before
 * psm_cost_filter of the frame whose minima should land there; psm_disp_select_partial(ctx, NULL) and psm_disp_merge
 * then use that buffer.  Saves the device-to-device copy of the keys per frame on a sharded host. */
int psm_set_key_buffer(psm_ctx *ctx, void *dev_keys);
/* Device pointer / size of the context's current key buffer. */
int psm_partial_keys(psm_ctx *ctx, void **dev_keys, size_t *bytes);
/* Sharded DispSel, step 2: dev_keys_all = DEVICE pointer to nranks consecutive key buffers
 * (the all-gather result, rank-major).  Produces the two final maps as psm_disp_select. */
int psm_disp_merge(psm_ctx *ctx, const void *dev_keys_all, int nranks, uint8_t *lmap,
                   uint8_t *rmap, size_t stride);

/* Single-process form of the exchange step: `shards` are nshards contexts of one job (on the
 * same or on different devices) whose psm_disp_select_partial has run; their key planes are
 * copied (device copy; peer copy across devices; through page-locked host memory when the two
 * devices have no peer access) into `root`'s gather buffer and merged there.  This is
 * what a C++ host that drives several GPUs from one process uses instead of RCCL, and what
 * the single-GPU "logical shard" tests use. */
int psm_disp_merge_ctx(psm_ctx *root, psm_ctx *const *shards, int nshards, uint8_t *lmap,
                       uint8_t *rmap, size_t stride);

int psm_download_maps(psm_ctx *ctx, uint8_t *lmap, uint8_t *rmap, size_t stride);

/* ---- frame loop (src/main.cpp:64-73: one pair after the other; the reference's stage timers include the copies,
 * src/StereoMatch.cpp:227-237): the PCIe legs next to the kernels ----
 * psm_upload_pair_async: as psm_upload_pair, but for the NEXT frame: the images are copied to page-locked staging memory
 * before the call returns (the caller's buffers are free again) and travel on the context's copy stream into a second image
 * slot while the current frame is being computed; the next psm_cost_construct adopts that pair (its kernels wait for the
 * copy on the device) - so it is called right after psm_cost_construct of the current frame:
 *   psm_cost_construct(i); psm_upload_pair_async(pair i+1); psm_cost_filter(i); psm_disp_select(i, NULL, NULL, 0);
 *   psm_download_maps_async(); psm_download_maps_wait(...)   <- typically one frame later: the maps of frame i-1
 * psm_download_maps_async starts the D2H copy of the current maps (after the kernels that produce them, before any
 * later kernel overwrites them) and returns; psm_download_maps_wait blocks until they have arrived and hands them over
 * (lmap / rmap as psm_download_maps).  One upload and one download may be in flight. */
int psm_upload_pair_async(psm_ctx *ctx, const void *l, const void *r, int channels, size_t stride_bytes, int depth);
int psm_download_maps_async(psm_ctx *ctx);
int psm_download_maps_wait(psm_ctx *ctx, uint8_t *lmap, uint8_t *rmap, size_t stride);

/* ---- video mode (the DE_VIDEO branch of StereoMatch::compute, src/StereoMatch.cpp:138-153): the camera frame is rectified and
 * cropped on the device.  The arithmetic is that of cv::remap(src, dst, map1, map2, INTER_LINEAR) with CV_16SC2 / CV_16UC1 maps,
 * the default BORDER_CONSTANT with value 0, 8-bit 3-channel images, followed by dst(cropBox) - stated exactly:
 * for an output pixel (x, y) of a side, (mx, my) = map_xy[crop_y + y][crop_x + x], f = map_frac[crop_y + y][crop_x + x],
 * fx = f & 31, fy = f >> 5: w00 = (32-fx)(32-fy)*32, w01 = fx(32-fy)*32, w10 = (32-fx)fy*32, w11 = fx*fy*32 (their sum is 2^15),
 * out = (w00*S(my, mx) + w01*S(my, mx+1) + w10*S(my+1, mx) + w11*S(my+1, mx+1) + 2^14) >> 15 per channel, where a tap outside the
 * src_w x src_h eye image reads 0, each tap on its own.
 *
 * psm_rectify_build_maps: host only, needs no device and no context (ctx-less errors: psm_last_error(NULL)) -
 * initUndistortRectifyMap(M, D, R, P, Size(map_w, map_h), CV_16SC2, map1, map2) (src/StereoMatch.cpp:464-466) restated in double,
 * every pixel from its own (u, v): iR = inv(P[:, :3] * R) by cofactors over the determinant, [X Y Z] = iR * [u v 1], x = X/Z,
 * y = Y/Z, the rational radial + tangential + thin-prism model (dist: k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4 [tx ty]]]], n_dist 0,
 * 4, 5, 8, 12 or 14; tx, ty != 0 refused), u' = fx * xd + cx, iu = rint(32 u') (ties to even), map_xy = saturate_int16(iu >> 5),
 * map_frac = (iv & 31) * 32 + (iu & 31); a non-finite coordinate gives map_xy = (-32768, -32768), map_frac = 0 (every tap outside).
 * map_xy: [map_h][map_w][2], map_frac: [map_h][map_w]. */
int psm_rectify_build_maps(const double M[9], const double *dist, int n_dist, const double R[9], const double P[12],
                           int map_w, int map_h, int16_t *map_xy, uint16_t *map_frac);
/* The maps of one side (dense, as above; every map_frac < 1024) for the following rectified uploads.  The eye images they index are
 * src_w x src_h (2 <= src_w, 1 <= src_h, both <= 32767; the same for both sides); the context's W x H window of the maps starts
 * at (crop_x, crop_y) - lFrame_rec(cropBox).  The window is copied to the device once; the host arrays are free on return. */
int psm_rectify_set_maps(psm_ctx *ctx, int side, const int16_t *map_xy, const uint16_t *map_frac, int map_w, int map_h,
                         int src_w, int src_h, int crop_x, int crop_y);
/* Forget the maps of both sides and free everything the rectified uploads allocated. */
int psm_rectify_clear(psm_ctx *ctx);
/* As psm_upload_pair / psm_upload_pair_async with depth PSM_IMG_U8, but l / r are the UNRECTIFIED eye images: src_h rows of src_w
 * B,G,R pixels, pitch stride_bytes (0: packed).  The two halves of a side-by-side frame are l = frame, r = frame + 3 * src_w with
 * the frame's pitch (the cv::Mat ROIs of src/StereoMatch.cpp:138-139: no copy).  The pair the context adopts is the rectified,
 * cropped one - contexts of either dtype, shards, row stripes and psm_compute_batch see an ordinary 8-bit pair.  One kernel launch
 * per frame, timed under PSM_K_PREP, outside the four stage timers (remap sits before cvc_time in the reference).  The asynchronous
 * form keeps the contract of psm_upload_pair_async: the caller's buffers are free on return, two staging slots, one upload in
 * flight, adopted by the next psm_cost_construct. */
int psm_upload_pair_rectified(psm_ctx *ctx, const void *l, const void *r, int channels, size_t stride_bytes);
int psm_upload_pair_rectified_async(psm_ctx *ctx, const void *l, const void *r, int channels, size_t stride_bytes);
/* The context's CURRENT 8-bit pair as it is staged on the device (what the reference shows as leftInputImg / rightInputImg):
 * H rows of W B,G,R pixels each, pitch stride_bytes (0: packed).  A pair staged by an asynchronous upload becomes current in
 * psm_cost_construct.  Float pairs are refused. */
int psm_download_images(psm_ctx *ctx, uint8_t *l, uint8_t *r, size_t stride_bytes);

/* ---- semi-global matching: the reference's second algorithm, the STEREO_SGBM branch of StereoMatch::compute
 * (ssgbm->compute(lFrame, rFrame, imgDisparity16S), src/StereoMatch.cpp:169-187) with the configuration of setupOpenCVSGBM
 * (:639-660): minDisparity 0, numDisparities = the context's max_disp (any value in [2, 256]; psm_sgm_set_range: another minimum,
 * up to 1024 disparities), blockSize 5, P1 = 8 ch bs^2,
 * P2 = 32 ch bs^2, disp12MaxDiff 1, uniquenessRatio 10, eight paths (MODE_HH).  All integer; the definition (DESIGN.md section 10,
 * tests/sgm_model.py) is Hirschmueller's recurrence under OpenCV's parameter names, and the device equals it element for element:
 *   pixel cost  c(x,y,d) = sum_ch |L[y][x][ch] - R[y][max(x-d, 0)][ch]|, or the prefiltered Birchfield-Tomasi cost, or the
 *               census cost - below
 *   block cost  C = the bs x bs box sum of c(.,.,d), the plane replicated at the image edge (u16)
 *   paths       L_r(p,d) = C(p,d) + min(L_r(p-r,d), L_r(p-r,d-1)+P1, L_r(p-r,d+1)+P1, m+P2) - m, m = min_k L_r(p-r,k); L_r = C where
 *               p-r is outside; r = (dy,dx) in (0,+-1), (+-1,0), (+-1,+-1); S = sum_r L_r (u32, exact)
 *   select      best = argmin_d S (lowest d on ties); not unique if some d, |d-best| > 1, has S(d)(100-u) < minS 100;
 *               0 < best < D-1: den = max(S(best-1)+S(best+1)-2 minS, 1), d16 = 16 best + floor(((S(best-1)-S(best+1)) 16 + den) / (2 den))
 *   consistency disp2[y][x-best] = best of the smallest (minS, best) among the unique pixels landing there; with m >= 0 a pixel is
 *               rejected if the probes (x-da, da), da = d16 >> 4, and (x-db, db), db = (d16+15) >> 4, both find a disp2 that
 *               differs from the probe's disparity by more than m
 *   output      int16, d16 (disparity * 16) or -16 where not unique or rejected (OpenCV's (minDisparity - 1) * 16)
 *   speckles    optional (psm_sgm_set_speckle), StereoSGBM's last step: cv::filterSpeckles on the output map - below
 * A float pair (PSM_IMG_F32) is quantised as lFrame.convertTo(lFrame, CV_8U, 255) does (:174-177): saturate(rint(f * 255.0f)).
 * Every field of setupOpenCVSGBM is built; the pixel cost of a new context is SAD, StereoSGBM's own cost (preFilterCap 63 in the
 * reference) is selected by psm_sgm_set_prefilter.  Unpinned: agreement with a live cv::StereoSGBM (neither OpenCV nor its
 * source was available) - what is built is the definition stated here and in the models under tests/.
 *
 * psm_sgm_set_params: block_size in {1, 3, 5, 7}; 0 < P1 <= P2; block_size^2 * channels * 255 + P2 <= 65535; uniqueness_ratio in
 * [0, 100); disp12_max_diff < 0 turns the consistency test off.  0 for any of the first three: the default above. */
int psm_sgm_set_params(psm_ctx *ctx, int block_size, int p1, int p2, int uniqueness_ratio, int disp12_max_diff);
/* Runs the stage on the context's stream over the pair psm_upload_pair* staged (either depth); synchronous on return unless
 * PSM_OPT_ASYNC.  An independent stage: it reads the staged images only and writes its own buffers - 6 * W * H * Dp bytes of
 * volumes (Dp = the number of disparities D rounded up to 4; above 256 to 8, above 512 to 16 - D is max_disp or psm_sgm_set_range's)
 * and 8 * W * H of planes, plus 12 * W * H of prefiltered planes once a compute ran with
 * pre_filter_cap > 0 and 16 * W * H of census codes once one ran with a census window, allocated on first use, reused from frame to frame, given back by psm_release_scratch and psm_destroy.  Volumes, maps, masks and minima of the other entry points are untouched: it may be
 * called anywhere between them.  Refused on disparity shards, under a row stripe, and when nothing has been uploaded. */
int psm_sgm_compute(psm_ctx *ctx);
/* The same for a 1-channel 8-bit pair (CV_8UC1 frames): H rows of W bytes, pitch stride_bytes (0: packed).  The pair is copied to
 * buffers of the stage and used by this call only (the caller's memory is free on return); the staged colour pair is untouched. */
int psm_sgm_compute_gray(psm_ctx *ctx, const uint8_t *l, const uint8_t *r, size_t stride_bytes);
/* The left map of the last compute (imgDisparity16S): H rows of W int16, pitch stride_bytes (0: packed).  Synchronises. */
int psm_sgm_download_disparity(psm_ctx *ctx, int16_t *disp, size_t stride_bytes);
/* Test hook: the volumes of the last compute as dense host arrays [H][W][D], D the number of disparities that compute ran with
 * (max_disp, or psm_sgm_set_range's) - which 0: C as uint16, 1: S as uint32. */
int psm_sgm_download_costs(psm_ctx *ctx, int which, void *host);
/* With PSM_OPT_PROFILE set during the last compute: device time in ms of its block-cost launches (everything up to C, the
 * prefilter or the census transform included), its eight path launches and its select + check launches (a getter of its own: the PSM_K_* and PSM_STAGE_* tables stay as they are). */
int psm_sgm_times(psm_ctx *ctx, double ms[3]);

/* StereoSGBM's modes (ssgbm->setMode, the reference's `m` key: src/main.cpp:22,114-168): the set of directions step "paths" sums.
 * Everything else above is untouched.  (dy, dx) is the step from the predecessor p-r to p; the values are OpenCV's enum:
 *   PSM_SGM_MODE_SGBM       (0, 1), (0, -1), (1, 0), (1, 1), (1, -1): OpenCV's single top-down pass plus the right-to-left row path
 *                           it forms during selection
 *   PSM_SGM_MODE_HH         all eight - a new context's setting: psm_sgm_compute is what it is without this function
 *   PSM_SGM_MODE_SGBM_3WAY  (0, 1), (0, -1), (1, 0)
 *   PSM_SGM_MODE_HH4        (0, 1), (0, -1), (1, 0), (-1, 0)   (the reference's key does not reach it; OpenCV's enum has it)
 * The paths cross the whole image in every mode: OpenCV cuts the 3-way image into stripes by thread count and restarts its paths
 * in each, which is not built.  The definition is tests/sgm_mode_model.py; agreement with a live cv::StereoSGBM stays unpinned in
 * every mode.  S is at most (directions) * 65535 < 2^19 as before.  Any other value is refused.  The setting holds until changed;
 * psm_sgm_compute, _compute_gray and _compute_batch launch the mode's directions in the order above, the first one stores S;
 * psm_sgm_times' second number covers the mode's path launches.  psm_sgm_compute_batch refuses contexts whose modes differ. */
enum { PSM_SGM_MODE_SGBM = 0, PSM_SGM_MODE_HH = 1, PSM_SGM_MODE_SGBM_3WAY = 2, PSM_SGM_MODE_HH4 = 3 };
int psm_sgm_set_mode(psm_ctx *ctx, int mode);

/* The first two arguments of StereoSGBM::create, minDisparity and numDisparities (the reference passes mindisparity, ndisparities):
 * the stage's D = num_disparities indices k in [0, D) stand for the disparities min_disparity + k.  min_disparity in [-1024, 1024];
 * num_disparities 0: the context's max_disp (a new context's setting), else any value in [2, 1024] - independent of max_disp and
 * of the width, because every case is defined by the clamp below.  With (0, 0), or without this function, psm_sgm_compute,
 * _compute_gray and _compute_batch are bit for bit what they are above.  The definition is tests/sgm_range_model.py:
 *   pixel cost   the right column is xr = clamp(x - (min_disparity + k), 0, W - 1), on BOTH sides (a negative disparity reaches past
 *                the right edge), in the SAD cost and in step "cost" of the Birchfield-Tomasi cost; planes, bounds and border
 *                columns are unchanged
 *   block cost, paths, sum, select   over k as above; d16 = 16 (min_disparity + best_k) + sub, sub only for 0 < best_k < D - 1
 *   consistency  a unique pixel lands at column x - (min_disparity + best_k) if that is inside [0, W); disp2 holds the disparity
 *                min_disparity + best_k of the smallest (minS, best_k) landing there, "nothing landed" is a state of its own
 *                (-1 can be a disparity); the probes da = d16 >> 4, db = (d16 + 15) >> 4 are floors, also of a negative d16
 *   output       d16, or invalid = (min_disparity - 1) * 16 where not unique or rejected; the speckle filter, when on, runs with
 *                newVal = invalid.  |sub| <= 8: a valid value never equals invalid.  16 (min_disparity + D - 1) + 8 <= 32767 and
 *                invalid >= -32768 hold inside the ranges above; S <= 8 * 65535 as before.
 * Not OpenCV's convention: OpenCV leaves the columns outside [max(maxD, 0), W + min(minD, 0)) invalid, the stage keeps all columns,
 * as it does without a range.  Agreement with a live cv::StereoSGBM stays unpinned.
 * The setting holds until changed.  The volumes follow it: a compute whose D needs another Dp than the volumes have frees and
 * allocates C and S again (6 * W * H * Dp bytes: 1920 x 1080 x 512 is 6.4 GB, 3840 x 2160 x 512 25.5 GB) and the previous result
 * is gone from that moment; psm_release_scratch and psm_destroy work as ever.  psm_sgm_compute_batch refuses contexts whose ranges
 * differ.  Values outside the ranges are refused; with a NULL context the message is psm_last_error(NULL)'s.  The guided-filter path
 * (psm_cost_construct ... psm_post_process) keeps max_disp <= 256: its maps are 8-bit. */
int psm_sgm_set_range(psm_ctx *ctx, int min_disparity, int num_disparities);

/* StereoSGBM's pixel cost: the Birchfield-Tomasi cost over Sobel-prefiltered images (tests/sgm_bt_model.py; all integer, the
 * device equals it element for element).  pre_filter_cap = cap, 1 <= cap <= 63, ft = max(cap, 15) | 1; images are the 8-bit pair
 * (a float pair is quantised first), ch in {1, 3}:
 *   planes   2 ch per image, [H][W] bytes each, over the whole image; yn = max(y-1, 0), ys = min(y+1, H-1); for 1 <= x <= W-2:
 *              g = 2 (I[y][x+1] - I[y][x-1]) + (I[yn][x+1] - I[yn][x-1]) + (I[ys][x+1] - I[ys][x-1])   on channel k
 *              P_k[y][x] = min(max(g, -ft), ft) + ft,  Q_k[y][x] = I[y][x][k]
 *            for x = 0 and x = W-1 BOTH P_k and Q_k are ft (OpenCV presets the border columns of all its row buffers).
 *            Order P_0 .. P_{ch-1}, Q_0 .. Q_{ch-1}; P planes have shift 0, Q planes shift 2.
 *   bounds   of a plane row a: al = x > 0 ? (a[x] + a[x-1]) / 2 : a[x], ar = x < W-1 ? (a[x] + a[x+1]) / 2 : a[x] (floor),
 *            lo(a, x) = min(a[x], al, ar), hi(a, x) = max(a[x], al, ar)
 *   cost     xr = max(x - d, 0); per plane, U of the left image, V of the right: u = U[y][x], v = V[y][xr],
 *            c0 = max(0, u - hi(V, xr), lo(V, xr) - u), c1 = max(0, v - hi(U, x), lo(U, x) - v),
 *            c(x,y,d) = sum over the planes of min(c0, c1) >> shift
 * Per channel c is at most 2 ft + 63 <= 189 < 255: the conditions of psm_sgm_set_params hold as they are.  Block cost, paths,
 * selection, consistency test and speckle filter are unchanged.  Not OpenCV's: the stage keeps all columns and xr = max(x-d, 0)
 * where OpenCV leaves the leftmost numDisparities columns invalid.
 *
 * psm_sgm_set_prefilter: 0 (a new context's setting): SAD - psm_sgm_compute / psm_sgm_compute_gray are what they are without this
 * function.  1 .. 63: every following compute uses the cost above.  Other values are refused.  The setting holds until changed;
 * psm_sgm_set_params and psm_sgm_set_speckle do not reset it. */
int psm_sgm_set_prefilter(psm_ctx *ctx, int pre_filter_cap);
/* Test hook: the prefiltered planes of the last compute, side 0: left, 1: right, as [H][W][2 ch] bytes in the plane order above.
 * Refused when the last compute ran with pre_filter_cap 0, or there is none.  Synchronises. */
int psm_sgm_download_prefiltered(psm_ctx *ctx, int side, uint8_t *planes);

/* A third pixel cost: the Hamming distance of census transforms (tests/sgm_census_model.py; all integer, the device equals it
 * element for element).  SAD and Birchfield-Tomasi compare intensities and break when the two cameras differ in gain, exposure or
 * vignetting; a census code keeps only the order of a pixel's neighbourhood, which any increasing map of the intensities leaves
 * as it is.  Window win_w x win_h, both odd, 3 <= win_w <= 9, 3 <= win_h <= 7 (win_w win_h - 1 <= 62 bits: one uint64 per pixel);
 * images are the 8-bit pair (a float pair is quantised first), ch in {1, 3}:
 *   gray     g [H][W]: ch 1: the byte; ch 3, staged order B, G, R: g = (1868 B + 9617 G + 4899 R + 8192) >> 14 (the stage's own
 *            definition; the coefficients sum to 16384, so g <= 255)
 *   code     T [H][W] uint64: the taps (dy, dx) in raster order, dy from -(win_h / 2) up, dx from -(win_w / 2) up, the centre
 *            skipped, tap i = 0, 1, ...: bit i (bit 0 the least significant) is 1 iff
 *            g[clamp(y + dy, 0, H - 1)][clamp(x + dx, 0, W - 1)] < g[y][x], strictly (a tap equal to the centre gives 0); the
 *            plane is replicated at the image edge; the bits above win_w win_h - 2 are 0
 *   cost     c(x,y,k) = popcount(T_L[y][x] ^ T_R[y][xr]), xr = clamp(x - (min_disparity + k), 0, W - 1): the range's right column,
 *            max(x - d, 0) with the default range, as for the other two costs
 * c <= win_w win_h - 1 <= 62, C <= 49 * 62 = 3038: the conditions of psm_sgm_set_params hold as they are, and P1 / P2 default to
 * 8 ch bs^2 / 32 ch bs^2 with ch the pair's channels whatever the cost.  Block cost, paths, selection, consistency test and
 * speckle filter are unchanged.  No library's convention, like the other two costs.
 *
 * psm_sgm_set_census: (0, 0) (a new context's setting): off - psm_sgm_compute, _compute_gray and _compute_batch are bit for bit
 * what they are without this function.  A window as above: every following compute uses the cost above.  Anything else is
 * refused; with a NULL context the message is psm_last_error(NULL)'s.  The setting holds until changed; no other setter resets
 * it, it resets none, and no setter depends on call order.  A compute that finds a window and pre_filter_cap > 0 both set is
 * refused (the message names both; in a batch also the index): nothing is enqueued, the previous result stays readable.
 * psm_sgm_compute_batch refuses contexts whose windows differ.  The two code planes are 16 * W * H bytes per context, allocated
 * by the first census compute, given back by psm_release_scratch and psm_destroy; psm_sgm_times counts the census launches in
 * its first number. */
int psm_sgm_set_census(psm_ctx *ctx, int win_w, int win_h);
/* Test hook: the codes of the last compute, side 0: left, 1: right, as [H][W] uint64.  Refused when the last compute ran another
 * cost, or there is none.  Synchronises. */
int psm_sgm_download_census(psm_ctx *ctx, int side, uint64_t *codes);

/* The speckle filter, the step StereoSGBM ends with when speckleWindowSize > 0 (the reference: 100, with speckleRange 32):
 * cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on a CV_16SC1 map.  Its definition (tests/speckle_model.py) is free of
 * any visiting order:
 *   vertices  the pixels with img != newVal
 *   edges     4-neighbours p, q, both vertices, |img[p] - img[q]| <= maxDiff (the difference taken in 32 bits; chains connect:
 *             0, 512, 1024 side by side are one component at maxDiff 512)
 *   result    every pixel of a connected component of AT MOST maxSpeckleSize pixels becomes newVal, every other pixel is unchanged
 * On the device: union-find over the pixel grid in four launches whatever the data (psm_speckle.hip), all integer, the result
 * equals the definition element for element.  It holds 8 * W * H bytes, allocated when first used, given back by
 * psm_release_scratch and psm_destroy.
 *
 * psm_sgm_set_speckle: window 0 (a new context's setting): off - psm_sgm_compute / psm_sgm_compute_gray are what they are without
 * this function.  window > 0: every following compute ends with filterSpeckles(map, -16, window, 16 * range) on its output map,
 * after the disp12_max_diff test, on the stream (asynchronous computes stay asynchronous); C and S are not touched.  Negative
 * values are refused.  The setting holds until changed; psm_sgm_set_params does not reset it. */
int psm_sgm_set_speckle(psm_ctx *ctx, int speckle_window_size, int speckle_range);
/* cv::filterSpeckles on the caller's map, in place: H rows of W int16, pitch stride_bytes (0: packed).  new_val: any int16 value;
 * max_speckle_size >= 0 (0 changes nothing); max_diff >= 0.  The map goes through a device plane of this call; the last compute's
 * map, C and S are untouched.  Synchronises on return.  Needs no staged pair and reads nothing else of the context: valid on
 * disparity shards and under a row stripe too. */
int psm_sgm_filter_speckles(psm_ctx *ctx, int16_t *disp, size_t stride_bytes, int new_val, int max_speckle_size, int max_diff);
/* Test hook: for the last filter run (a compute with the filter on, or psm_sgm_filter_speckles) the size of every pixel's
 * component, 0 where the pixel was new_val on input: H rows of W int32, pitch stride_bytes (0: packed).  Synchronises. */
int psm_sgm_download_speckle_sizes(psm_ctx *ctx, int32_t *sizes, size_t stride_bytes);
/* Device time in ms of the filter's four launches in the last compute, which must have been timed (PSM_OPT_PROFILE) and have run
 * the filter; psm_sgm_times keeps its three numbers.  A psm_sgm_filter_speckles under PSM_OPT_PROFILE is timed the same way
 * (the copies of the map excluded) and then is what this reports. */
int psm_sgm_speckle_time(psm_ctx *ctx, double *ms);

/* psm_sgm_compute of the n contexts ctxs[0..n) in shared launches: every kernel of the stage - cost, prefilter + Birchfield-Tomasi
 * cost or census + census cost, the eight paths, select, check, the four of the speckle filter - runs once with the pair on a grid axis of its own, so a
 * path launch has n x (H, W or W + H - 1) one-wave paths instead of one pair's.  The reference's use on Middlebury-size data is a
 * loop over pairs and datasets (src/main.cpp:64-73, src/StereoMatch.cpp:528-609); there the stage is bound by the waves it has in
 * flight, not by bytes.  Measured at 450 x 375 x 64 with the reference's configuration
 * (cap 63, speckle 100 / 32): 0.569 ms per pair one context after the other, 0.276 ms per pair in a batch of 8 (0.356 in a batch
 * of 2); at 1280 x 720 x 128 0.98 of the singles in a batch of 8, at 1920 x 1080 x 256 0.96 in a batch of 4.
 * Each context holds its own pair, exactly the one its own psm_sgm_compute would read at that moment, and afterwards is exactly
 * where that call would have left it: psm_sgm_download_disparity / _costs / _prefiltered / _census / _speckle_sizes, a later single
 * psm_sgm_compute and psm_sgm_filter_speckles work per context and return the same bits.  Volumes, maps, masks and minima of the
 * other entry points are untouched; the call may stand anywhere between them.
 * The contexts must agree on width, height, max_disp and device, on the depth of the staged pair (a float pair is quantised on the
 * device, as ever) and on every setting of psm_sgm_set_params, psm_sgm_set_prefilter, psm_sgm_set_census, psm_sgm_set_speckle,
 * psm_sgm_set_mode and psm_sgm_set_range.  Refused otherwise,
 * and for NULL or repeated contexts, n < 1 or n > 4096, a context without a pair, a disparity shard, a row stripe in force and
 * parameters psm_sgm_set_params would refuse: psm_last_error(ctxs[0]) names the offending index, nothing has been enqueued, and
 * every context's previous result is still readable.
 * The launches run on ctxs[0]'s stream, after everything already queued on the other contexts' streams and before anything queued
 * on them later; synchronous on return unless ctxs[0] has PSM_OPT_ASYNC.  Contexts under psm_share_streams work as they are.
 * Buffers stay per context (allocated on first use, given back by psm_release_scratch / psm_destroy); the kernels reach them
 * through a device table of n * 96 bytes (the census code planes take the slots of the prefiltered planes: a batch has one cost)
 * that ctxs[0] owns and uploads again only when an entry changed.  With PSM_OPT_PROFILE on
 * ctxs[0], psm_sgm_times(ctxs[0]) and psm_sgm_speckle_time(ctxs[0]) report the batch's launches; the other contexts count as not
 * timed.  psm_sgm_compute_gray has no batch form: it takes host pointers and stages them itself. */
int psm_sgm_compute_batch(psm_ctx *const *ctxs, int n);

/* The 8-bit maps of both views from the SGM stage, so that everything that works on the context's current maps - psm_lr_check,
 * psm_fill_invalid, psm_wgt_median, psm_joint_wmf, psm_score(PSM_SCORE_GIF), psm_download_maps* - runs behind the stage as it runs
 * behind psm_disp_select.  The definition is tests/sgm_maps_model.py, all integer; the device equals it element for element.  For
 * the summed path costs S [H][W][D] of the last psm_sgm_compute / _compute_gray / _compute_batch of the context, computed with
 * the range (dmin, D) - index k stands for the disparity dmin + k:
 *   left   lmap[y][x]  = dmin + argmin_k S[y][x][k], the lowest k on ties: the winner-takes-all disparity.  The uniqueness test,
 *                        the sub-pixel step and the disp12_max_diff test play no part: psm_lr_check validates these maps.
 *   right  rmap[y][xr] = dmin + k of the smallest (S[y][xr + dmin + k][k], k) over the k in [0, D) with xr + dmin + k < W, the
 *                        lowest k on ties - Hirschmueller's D_m(q) = argmin_d S(q.x + d, q.y, d), the search along the epipolar
 *                        line in the same S; 0 in a column without a candidate (the last dmin columns).
 * Range condition: the call is defined for 0 <= dmin and dmin + D <= max_disp (<= 256) only - the maps are bytes and index the
 * max_disp bins of the weighted medians.  The range is the one the RESULT was computed with, whatever psm_sgm_set_range has been
 * told since.  One launch (k_sgm_maps) that reads S once; no global atomics.
 * Both maps go to the context's map buffer (psm_disp_select's, or the caller's after psm_set_map_buffer).  Afterwards the context
 * is exactly where psm_upload_maps(ctx, l, r, NULL, NULL, 0) leaves it: whole-image maps are current, there is no mask
 * (psm_fill_invalid and the medians are refused until a new psm_lr_check), and the guided-filter path keeps what it had - volumes,
 * packed minima and anything pending are untouched, a later psm_disp_select yields the guided-filter maps again.  Untouched as
 * well, bit for bit: the int16 map, C, S, the consistency plane, the speckle planes and everything psm_sgm_download_* returns.
 * lmap / rmap: H rows of W bytes, pitch `stride` (0: packed); either may be NULL (the results stay on the device).  On the
 * context's stream; synchronous on return unless PSM_OPT_ASYNC is set.
 * Refused - psm_last_error names the call and the numbers, nothing has been enqueued, the previous maps are still current - for a
 * NULL context (psm_last_error(NULL)), a context without an SGM result (never computed, or given back by psm_release_scratch), a
 * result whose range violates the range condition (so every result with more disparities than the image has columns: psm_create
 * wants max_disp <= width), a disparity shard, a row stripe in force and stride < W. */
int psm_sgm_select_maps(psm_ctx *ctx, uint8_t *lmap, uint8_t *rmap, size_t stride);
/* psm_sgm_select_maps of the n contexts ctxs[0..n) in one launch, the pair on a grid axis of its own; the maps stay on the device
 * (psm_download_maps).  On ctxs[0]'s stream, ordered as psm_sgm_compute_batch's launches: after everything already queued on the
 * other contexts' streams, before anything queued on them later; synchronous on return unless ctxs[0] has PSM_OPT_ASYNC.  The
 * contexts must agree on width, height, max_disp and device and on the range (dmin, D) of their results; every context must pass
 * the single call's conditions.  Refused otherwise and for NULL or repeated contexts, n < 1 or n > 4096: psm_last_error(ctxs[0])
 * names the offending index, nothing has been enqueued.  Every context ends where its own psm_sgm_select_maps would have left
 * it, with the same bits.  The kernels reach the buffers through psm_sgm_compute_batch's device table, which for this carries
 * every context's map buffer. */
int psm_sgm_select_maps_batch(psm_ctx *const *ctxs, int n);
/* Device time in ms of the launch of the last psm_sgm_select_maps, which must have run under PSM_OPT_PROFILE (a batch: of all
 * pairs, on its first context; the other contexts count as not timed). */
int psm_sgm_maps_time(psm_ctx *ctx, double *ms);

/* "next" row: PP lrCheck on the device (src/PP.cpp:17-50) on the maps of the last
 * psm_disp_select/psm_disp_merge.  lvalid/rvalid: H x W bytes (0/1), pitch `stride`; either
 * may be NULL (results stay on the device). */
int psm_lr_check(psm_ctx *ctx, uint8_t *lvalid, uint8_t *rvalid, size_t stride);

/* "next" row: PP fillInv on the device (src/PP.cpp:52-143): every pixel the last psm_lr_check
 * marked invalid takes the smaller disparity of its nearest valid left/right neighbours in the row.
 * Modifies the device maps in place; lmap/rmap (optional) receive them. */
int psm_fill_invalid(psm_ctx *ctx, uint8_t *lmap, uint8_t *rmap, size_t stride);

/* "next" row: the plain weighted-median post-filter, wgtMedian (src/PP.cpp:145-247; constants MED_SZ 19, SIG_CLR 0.1,
 * SIG_DIS 9, include/PP.h:12-14), on the device maps of the last psm_disp_select/psm_disp_merge, for the pixels the
 * last psm_lr_check marked invalid (the sequence of PP::processDM: lrCheck, fillInv, wgtMedian, src/PP.cpp:405-410).
 * Left map with the left image and the squared distances (:169-175), right map with the right image and the
 * square-rooted ones (:216-224).  Same result as the reference's single-threaded form: the map is filtered in place in
 * raster order, a filtered pixel sees the filtered pixels before it.  Run as parallel sweeps to the fixed point of that
 * recursion (every sweep evaluates all pixels whose earlier window taps changed; it stops, at the reference's map, when
 * a sweep changes nothing); falls back to a row-dataflow pipeline with the reference's own dependency chain if 96
 * sweeps do not reach it (PSM_OPT_FLAGS 4194304: dataflow form only).
 * Needs W, H >= 9 (the reference's modulo wrap is undefined below that).  lmap/rmap (optional) receive the maps.
 * Device memory: from 8192 invalid pixels per map the 19 x 19 window weights of every invalid pixel are formed once and kept
 * for the sweeps - 1.5 KB per invalid pixel (0.6 GB per 1080p map at 20 % invalid), held by the context until psm_destroy;
 * above 12 GB (or half of the device's free memory) for the pair, or when the allocation fails, the evaluations form their
 * weights themselves (slower, same maps).
 * Always synchronises with the host, PSM_OPT_ASYNC or not: the number of sweeps depends on the data (the host reads the
 * device's per-sweep counters), so the call returns with the filtered maps complete. */
int psm_wgt_median(psm_ctx *ctx, uint8_t *lmap, uint8_t *rmap, size_t stride);
/* What the last psm_wgt_median did, per map {left, right}: sweeps until the fixed point (-1: dataflow form) and pixel
 * evaluations in total.  Either pointer may be NULL.  The maps are a function of the input alone (the unique fixed point of the
 * in-place recursion); these two numbers are not - a changed pixel is visible to evaluations still running in its sweep, so how
 * many evaluations (and, on dense maps, sweeps) a call needs can differ from run to run. */
int psm_wgt_median_stats(psm_ctx *ctx, int sweeps[2], long long evals[2]);

/* PP::processDM's own sequence - lrCheck, fillInv, wgtMedian (src/PP.cpp:17-247,405-410) - of the n contexts ctxs[0..n) in shared
 * launches: the stages named in `stages` run in the reference's order, every launch once with the pair on a grid axis of its own.
 * The reference's use on Middlebury-size data is a loop over pairs and datasets (src/main.cpp:64-73, src/StereoMatch.cpp:528-609),
 * and a single psm_wgt_median is a chain of 20 - 40 small sweeps, each one to four launches near the launch floor, with the device
 * nearly idle; the chains of different maps are independent, so here the sweeps of all 2 n maps run side by side: one seed launch,
 * one weights launch, one set of launches per sweep and one look at the counters of all maps per group of sweeps.  A map that has
 * reached its fixed point has empty lists while the others go on; a group takes the one-launch wave form only when every map's list
 * is short or finished; maps that leave the sweeps at the cap of 96 are restored and take the dataflow form one by one.
 * Measured: DESIGN.md 4.5.
 * Each context uses its own device maps (from psm_disp_select, psm_compute_batch, psm_disp_merge, psm_upload_maps), its own mask
 * and its own current pair, and afterwards is exactly where its own psm_lr_check(ctx, NULL, NULL, 0), psm_fill_invalid(ctx, NULL,
 * NULL, 0) and psm_wgt_median(ctx, NULL, NULL, 0) - those of the named stages - would have left it: the same maps and masks bit for
 * bit (no result depends on a grid's shape: the kernels stride over their lists, and the median's map is the unique fixed point of
 * the in-place recursion), the same result state, and psm_wgt_median_stats answering per context (-1 for a map that went to the
 * dataflow form; sweeps and evaluations may differ from run to run as they may in the single call).  The maps stay on the device:
 * psm_download_maps[_async] per context reads them.
 * The contexts must agree on width, height, max_disp, device, the depth of the image pair and the weighted-median bits of
 * PSM_OPT_FLAGS (4194304 dataflow only, 16777216 no cache, 8388608 two sweeps).  Refused otherwise, and for NULL or repeated
 * contexts, n < 1 or n > 4096, stages naming none or an unknown stage, a context without maps or with stripe-only maps, without a
 * current mask when PSM_PP_LR_CHECK is not among the stages, and - the median being asked for - without an image pair or with W or
 * H below 9: psm_last_error(ctxs[0]) names the offending index, nothing has been enqueued, and every context is as before.
 * The weight cache is decided for the batch as a whole, since a launch takes every map one way: cached when at least one of the
 * 2 n maps has 8192 invalid pixels, the needs of all maps together stay within psm_wgt_median's bound and no flag forbids it; then
 * every map's weights are formed, in its own context's buffer.  The maps are the same either way.
 * The launches run on ctxs[0]'s stream, after everything already queued on the other contexts' streams (a pending
 * psm_download_maps_async of their maps included) and before anything queued on them later.  Without the median the call never
 * synchronises with the host under PSM_OPT_ASYNC on ctxs[0]; with it, it synchronises as psm_wgt_median does.  Contexts under
 * psm_share_streams work as they are.
 * Buffers stay per context (allocated on first use); the kernels reach them through a device table of n * 256 bytes that ctxs[0]
 * owns and uploads from page-locked memory only when an entry changed, and the per-sweep counters of all 2 n maps lie in one block of
 * ctxs[0] (n * 1568 bytes, and twice as much page-locked memory), so one small copy kernel snapshots all of them.  PSM_STAGE_PP
 * of every context receives the batch's wall time; with PSM_OPT_PROFILE 1 on ctxs[0], PSM_K_LRC / PSM_K_WMF of ctxs[0] count the
 * batch's launches. */
/* (below) The validity masks of the current maps as the last psm_lr_check, psm_post_process_batch or psm_upload_maps left them, to
 * the caller's rows (stride 0: packed).  Needs a current mask.  Complete on return. */
#define PSM_PP_LR_CHECK   1
#define PSM_PP_FILL       2
#define PSM_PP_WGT_MEDIAN 4
int psm_post_process_batch(psm_ctx *const *ctxs, int n, int stages);
int psm_download_valid(psm_ctx *ctx, uint8_t *lvalid, uint8_t *rvalid, size_t stride);

/* The live post-filter of the reference: PP::processDM runs JointWMF::filter on both maps with the 8-bit colour image as
 * the feature (src/PP.cpp:402-424, include/JointWMF.h), which is what PostProcess_GPU / PostProcess_CPU compute
 * (src/DispEst.cpp:330-344).  Filters the context's device maps in place (lDisMap = JointWMF::filter(...)), the left map
 * with the left image and the right map with the right image; the valid masks are untouched.  Per pixel: the smallest
 * disparity c with W(<=c) >= W(>c) over the clipped (2*radius+1)^2 window, W summing w[F(p)][F(q)] for the colour clusters
 * F of the centre and the tap; the sums are exact integers rint(w * 2^48) (equal to the reference's float
 * walk except where its own rounding decides, |W(<=c) - W(>c)| ~ 1e-4).  Clusters of a side: those psm_joint_wmf_set_clusters
 * gave for the current pair; otherwise every distinct 6-bit colour key is its own cluster when there are at most n_clusters
 * of them (the reference's result for any RNG state), else a deterministic k-means (k-means++ seeding from a fixed
 * splitmix64 stream, Lloyd iterations in fp32 until no label changes or max_iter).
 * radius 1..16, sigma > 0, n_clusters 1..256, max_iter >= 1; 0 or a negative value selects the reference's value
 * (9 = MED_SZ/2, 25.5, 256, 10000).  Refuses stripe-only maps.  lmap/rmap (optional) receive the filtered maps.
 * Synchronises with the host when the device k-means runs (the host reads the sample counts and the convergence flags);
 * it runs once per pair and (n_clusters, max_iter), the images of both sides in the same launches, as a psm_joint_wmf_batch of
 * this one context would run them.  With clusters set for both sides, or on a later call for the same pair,
 * it is asynchronous under PSM_OPT_ASYNC (the weight tables are formed once per clustering and sigma and copied from
 * page-locked memory).  Kernel time: PSM_K_JWMF; stage PSM_STAGE_PP. */
int psm_joint_wmf(psm_ctx *ctx, int radius, float sigma, int n_clusters, int max_iter, uint8_t *lmap, uint8_t *rmap, size_t stride);
/* Bring-your-own clustering for one side (PSM_LEFT / PSM_RIGHT) of the current pair: n_clusters (1..256) centres
 * [n][3] (B, G, R order of the 6-bit keys) and label_of_key[64*64*64] (index (B>>2)*4096 + (G>>2)*64 + (R>>2), values
 * < n_clusters).  Holds until the next pair is adopted; psm_joint_wmf then ignores its n_clusters / max_iter for that side. */
int psm_joint_wmf_set_clusters(psm_ctx *ctx, int side, int n_clusters, const float *centres, const uint8_t *label_of_key);
/* The clustering the last psm_joint_wmf used for a side (or the one set for it): *n_clusters, centres [n][3] (room for
 * 256 x 3), label_of_key [64^3] (keys absent from the image: 0 unless set), *iterations (Lloyd assignments; 0: identity or
 * set by the host).  Any output pointer may be NULL. */
int psm_joint_wmf_clusters(psm_ctx *ctx, int side, int *n_clusters, float *centres, uint8_t *label_of_key, int *iterations);

/* psm_joint_wmf of the n contexts ctxs[0..n) in shared launches: every kernel of the stage runs once with the image to cluster or
 * the map side on a grid axis of its own.  The reference's use on Middlebury-size data is a loop over pairs and datasets
 * (src/main.cpp:64-73, src/StereoMatch.cpp:528-609), and in a single call nearly all the time is one image's clustering chain - one
 * seeding workgroup, two small launches per Lloyd iteration - with the rest of the device idle; the chains of different images are
 * independent, so here they run side by side (one seeding workgroup per image in one launch, one pair of launches per Lloyd
 * iteration for all images, one look at all convergence flags per 16 iterations; an image that has converged is frozen by its
 * own flag while the others go on), and the median is one grid over the 2 n map sides.  Measured: DESIGN.md 9.
 * The parameters are psm_joint_wmf's, with the same "0 selects the reference's value" rule and the same ranges.  The filtered maps
 * stay on the device: psm_download_maps[_async] per context reads them, as after psm_compute_batch.
 * Each context uses its own state - its own current pair (the feature images) and its own device maps (from psm_disp_select,
 * psm_compute_batch, psm_disp_merge, psm_upload_maps, or after psm_lr_check / psm_fill_invalid) - and afterwards is exactly where
 * its own psm_joint_wmf(ctx, ..., NULL, NULL, 0) would have left it: the same maps bit for bit (every sum of the stage is an exact
 * integer, so no result depends on the grid's shape), the same clustering - psm_joint_wmf_clusters answers per context, a later
 * single psm_joint_wmf on the same pair reuses clustering and tables - and the same weight tables.
 * A side whose clustering the host set (psm_joint_wmf_set_clusters), or that an earlier call made with the same (n_clusters,
 * max_iter), takes no part in the k-means, exactly as in psm_joint_wmf: the images to cluster are m <= 2 n.  With m = 0 the call
 * never synchronises with the host and is asynchronous under PSM_OPT_ASYNC on ctxs[0]; with m > 0 it synchronises as the single
 * call does (the sample counts, the convergence flags of all images once per 16 iterations, the centres).
 * The contexts must agree on width, height, device and the depth of the staged pair.  Refused otherwise, and for NULL or repeated
 * contexts, n < 1 or n > 4096, a context without maps or without an image pair, stripe-only maps, and radius or n_clusters out of
 * range: psm_last_error(ctxs[0]) names the offending index, nothing has been enqueued, and every context's maps and clustering
 * are as before.
 * The launches run on ctxs[0]'s stream, after everything already queued on the other contexts' streams (a pending
 * psm_download_maps_async of their maps included) and before anything queued on them later; synchronous on return unless ctxs[0]
 * has PSM_OPT_ASYNC.  Contexts under psm_share_streams work as they are.
 * Buffers stay per context (allocated on first use); with n > 1 the kernels reach them through a device table of n * 272 bytes that
 * ctxs[0] owns and uploads from page-locked memory only when an entry changed (n = 1: in the kernel arguments), and the Lloyd states and centres of the m images lie in a
 * block of ctxs[0] (n * 6176 bytes, and as much page-locked memory), so one copy reads all of them.  PSM_STAGE_PP of every
 * context receives the batch's wall time; with PSM_OPT_PROFILE 1 on ctxs[0], PSM_K_JWMF of ctxs[0] counts the batch's launches. */
int psm_joint_wmf_batch(psm_ctx *const *ctxs, int n, int radius, float sigma, int n_clusters, int max_iter);

/* ---- second sharding axis: row stripes (SURVEY.md 8e asks for shards of the path; the filter's vertical support is
 * bounded - 8 rows of costs either side - so a stripe of output rows needs nothing from another stripe) ----
 * psm_set_rows restricts psm_cost_filter (select form) and psm_disp_select* of this context to the output rows
 * [y_begin, y_end) of the whole image - all D slices (or this context's slices) of both volumes, identical values to
 * the unrestricted run; the image pair is uploaded whole (borders reflect at the true image border).  Rows outside the
 * stripe of the maps / minima are undefined.  (0, 0) or (0, H): whole image again.  Takes effect with the next psm_cost_filter.
 * With G contexts / ranks on stripes [H*g/G, H*(g+1)/G) no minima are exchanged at all: the only exchange is the
 * gather of the finished map rows (2*W*H bytes in total) - psm_gather_rows_ctx in one process, an all-gather of the
 * stripes between ranks (bench.py).  The post-processing entry points refuse stripe-only maps. */
int psm_set_rows(psm_ctx *ctx, int y_begin, int y_end);
/* The disparity maps [2][H][W] (uint8) of this context live in dev_maps (device memory of this context's GPU, at least
 * 2*W*H + 4 bytes) from now on; NULL: the context's own buffer again.  whole != 0: the buffer already holds both
 * complete maps of the current frame (the caller gathered the stripes into it). */
int psm_set_map_buffer(psm_ctx *ctx, void *dev_maps, int whole);
/* One process, several contexts (one per GPU or logical stripes on one GPU): copies the stripe rows of every context's
 * maps into root's maps (root may be one of them); checks that the stripes tile [0, H) and that every context has run
 * psm_disp_select for the frame.  lmap/rmap (optional) receive the whole maps. */
int psm_gather_rows_ctx(psm_ctx *root, psm_ctx *const *stripes, int nstripes, uint8_t *lmap, uint8_t *rmap, size_t stride);
/* How many legs of psm_gather_rows_ctx / psm_disp_merge_ctx with this root went through host memory so far (devices without
 * peer access, or PSM_OPT_GATHER_STAGED) instead of a device / peer copy. */
int psm_gather_staged_legs(const psm_ctx *root);

/* ---- several pairs per launch: the reference's use on Middlebury-size data is a loop over pairs / datasets
 * (src/main.cpp:64-73, src/StereoMatch.cpp:556-607) - one 450 x 375 x 64 pair is 1.7 rounds of the chip's resident workgroups
 * behind four launches at their latency floor ----
 * psm_compute_batch runs DispEst::CostConst_GPU + CostFilter_GPU + DispSelect_GPU (src/DispEst.cpp:272-276,299-308,323-328) for
 * the n contexts ctxs[0..n) - same width, height, max_disp, slice range, dtype, device and options, each holding its own pair
 * (psm_upload_pair / psm_upload_pair_async) - in SHARED launches: one guidance kernel (which also prepares the images; 8-bit mode: a preparation launch before it), one fused
 * CVC + CVF + WTA grid over all pairs (two in the two-phase form), one reduction.  Afterwards every context is exactly where
 * psm_cost_construct + psm_cost_filter + psm_disp_select(ctx, NULL, NULL, 0) would have left it - same maps bit for bit
 * (psm_download_maps, psm_download_maps_async), same packed minima on a disparity shard, post-processing and volume readers
 * as usual.  The launches run on ctxs[0]'s stream, ordered after everything already queued on the other contexts' streams
 * and before anything queued on them later; synchronous on return unless ctxs[0] has PSM_OPT_ASYNC.  Default select path
 * only: contexts with a row stripe, the storing flags or the direct kernel variant are refused.  Stage timers of every context
 * receive the batch's wall time. */
int psm_compute_batch(psm_ctx *const *ctxs, int n);
/* The contexts of a batch (one device) run on ONE compute stream and one copy stream each way from now on, instead of three
 * streams per context - what a frame loop over batches wants: the runtime multiplexes streams onto a few hardware queues, and
 * with 8 contexts' 24 streams every asynchronous copy cost 0.2 ms of HOST time (measured).  Call once, before the first frame;
 * the streams live until the last of the contexts is destroyed.  psm_set_stream is refused afterwards. */
int psm_share_streams(psm_ctx *const *ctxs, int n);

/* ---- score: the display maps and the error metric of StereoMatch::compute on the device (src/StereoMatch.cpp:181-185,
 * 248-249, 275-309).  The definition is tests/score_model.py; the device equals it in every element and counter.
 * An independent stage: it reads the context's current result and writes its own planes - maps, masks, volumes and the SGM
 * stage's buffers are untouched. ----
 * Sources.  PSM_SCORE_GIF: the current 8-bit maps, as psm_download_maps would return them (after whichever of psm_disp_select,
 * psm_lr_check, psm_fill_invalid, psm_wgt_median, psm_joint_wmf, psm_upload_maps ran last); display of both sides =
 * min(v * scale_factor, 255) (convertTo(CV_8U, scale_factor)); the left one is scored.  The right display is the right map (the
 * reference's rightDispMap = lDispMap, :252, is not mirrored).
 * PSM_SCORE_SGM: the int16 map of the last psm_sgm_compute*; minVal / maxVal over the whole map, the invalid value included
 * (minMaxLoc); alpha = (float)(255.0 / ((double)maxVal - (double)minVal)); m = sat_u8(rne((float)v * alpha)) - one fp32 multiply,
 * negative products saturate to 0; m = sat_u8(rne((float)m * 0.25f)); display = min(m * scale_factor, 255); the metric runs on
 * the display with scale 1.  maxVal == minVal (the reference divides by zero): alpha = 0, an all-zero display, PSM_SCORE_FLAT.
 * PSM_SCORE_SGM_INT: min(max(d16, 0) >> 4, 255) of that map, then as a PSM_SCORE_GIF left map (the figure comparable with the
 * GIF path's).
 * Metric on the 8-bit display p, ground truth g, mask k: e = |p - g|; e = 0 for columns x <= max_disp; unit = 127 / max_disp
 * (integer; 0 from max_disp 128 up); e = 0 where e <= error_threshold * unit (THRESH_TOZERO); with a mask, after k = (k > 254 ?
 * k : 0) under PSM_MASK_DISC, e = sat_u8(rne((double)(e * k) * (double)(1 / 255.f))); bad = #(e != 0), err_sum = sum of e.
 * %BP = 100.0 * bad / pixels; Avg Err = unit ? ((double)err_sum / pixels) / unit : 0.0 - both exact on the host in double. */
enum { PSM_SCORE_GIF = 0, PSM_SCORE_SGM = 1, PSM_SCORE_SGM_INT = 2 };
enum { PSM_MASK_NONE = 0, PSM_MASK_NONOCC = 1, PSM_MASK_DISC = 2 };      /* include/StereoMatch.h */
enum { PSM_SCORE_FLAT = 1 };                                             /* psm_score.flags */
struct psm_score {
    int32_t min_val, max_val;   /* PSM_SCORE_SGM: minMaxLoc of the int16 map; the other sources: 0 */
    uint32_t pixels, bad;       /* W * H; pixels whose error survived (0 without a truth) */
    uint64_t err_sum;           /* the sum of the surviving errors */
    int32_t unit;               /* 127 / max_disp */
    uint32_t flags;             /* PSM_SCORE_FLAT */
};
/* The ground truth and (mask != NULL) the error mask of this context's dataset, H rows of W bytes, pitch stride_bytes (0: W),
 * copied to the device once; they stay until replaced or cleared and survive psm_release_scratch.  mask NULL: no mask. */
int psm_score_set_truth(psm_ctx *ctx, const uint8_t *gt, const uint8_t *mask, size_t stride_bytes);
int psm_score_clear_truth(psm_ctx *ctx);
/* scale_factor in 1..255, error_threshold in 0..255, mask_mode PSM_MASK_NONE (an uploaded mask is ignored) | PSM_MASK_NONOCC (the
 * mask as it is) | PSM_MASK_DISC.  A new context has (4, 4, PSM_MASK_NONOCC), the reference's settings for Cones and Teddy. */
int psm_score_set_params(psm_ctx *ctx, int scale_factor, int error_threshold, int mask_mode);
/* Display map(s), error plane and record of `source`, in one launch (two for PSM_SCORE_SGM), the counters zeroed on the stream
 * ahead of them.  Synchronous, the record in *out, unless PSM_OPT_ASYNC: then the record travels to a page-locked slot and
 * psm_score_wait collects it (one record in flight; out is not written).  Without a truth the display maps and min_val / max_val
 * are written all the same, bad = err_sum = 0 and the error plane is zero.  Refused with nothing enqueued: a GIF source without
 * current maps or with maps that cover a row stripe only, an SGM source without a compute, an unknown source. */
int psm_score(psm_ctx *ctx, int source, struct psm_score *out);
int psm_score_wait(psm_ctx *ctx, struct psm_score *out);
/* The planes of the last psm_score / psm_score_batch: left display, right display (PSM_SCORE_GIF only), error plane; any pointer
 * may be NULL; H rows of W bytes, pitch stride (0: W).  Synchronises. */
int psm_score_download(psm_ctx *ctx, uint8_t *ldisp, uint8_t *rdisp, uint8_t *emap, size_t stride);
/* psm_score of the n contexts ctxs[0..n) in one set of launches, the context on a grid axis of its own; each context scores its
 * own result against its own truth.  Same width, height, max_disp, device and score parameters on all; a truth (and a mask) on
 * all or on none - anything else is refused naming the context, with nothing enqueued.  The launches run on ctxs[0]'s stream,
 * ordered as psm_sgm_compute_batch's; synchronous with the records in outs[0..n) unless ctxs[0] has PSM_OPT_ASYNC (then every
 * context's psm_score_wait collects its own).  Afterwards every context is exactly where its own psm_score would have left it. */
int psm_score_batch(psm_ctx *const *ctxs, int n, int source, struct psm_score *outs);
/* Device ms of the launches of the last psm_score (a batch: on ctxs[0], for all pairs); needs PSM_OPT_PROFILE. */
int psm_score_time(psm_ctx *ctx, double *ms);

/* ---- reproject: from disparity to depth on the device - cv::reprojectImageTo3D of the current result with the Q of
 * cv::stereoRectify (the reference computes it at src/StereoMatch.cpp:456-458 and drops it), and the ordered, compacted,
 * coloured point cloud.  The definition is tests/depth_model.py; the device equals it in every bit.  An
 * independent stage like psm_score: it reads the context's current result and writes planes of its own. ----
 * For pixel (x, y) of the W x H map: xf = (double)(x + crop_x), yf = (double)(y + crop_y) - the maps are those of the cropped
 * image, Q speaks of the uncropped rectified one (the cropBox of src/StereoMatch.cpp:474-481).
 * Disparity d (double) and "missing".  PSM_DEPTH_GIF: d = the byte of the current LEFT 8-bit map, as psm_download_maps would
 * return it; missing only under PSM_DEPTH_USE_MASK: the left validity byte of the current L-R mask is 0.  PSM_DEPTH_SGM:
 * d = (double)v * 0.0625 of the int16 map the SGM sources of psm_score read (the plane of psm_score_upload_sgm_map while it is on,
 * else the last psm_sgm_compute*'s); missing: v == (min_disparity - 1) * 16, the invalid value of the range that map was
 * computed with (the hook plane: of the current psm_sgm_set_range setting).  While psm_wls_publish is on (and the hook plane
 * off) both stages read the map of the last psm_wls_filter with the invalid value it was made with.
 * Arithmetic: fp64, every product and sum rounded on its own (no FMA), the terms added left to right, for i = 0..3:
 *   s_i = ((Q[i][0]*xf + Q[i][1]*yf) + Q[i][2]*d) + Q[i][3];   r = 1.0 / s_3;   p_i = s_i * r (i = 0..2)
 * - the reciprocal-then-multiply reading of OpenCV's Vec3d /= double.  Agreement with a live OpenCV is unpinned.
 * A point is void if it is missing or any p_i is not finite (s_3 == 0: with a CALIB_ZERO_DISPARITY Q every pixel of disparity
 * 0).  Void pixels hold the bit pattern 0x7FC00000 in every component of the dense planes - stored, never computed; every other
 * pixel holds (float)p_i, round to nearest even, +-inf and subnormal floats kept.
 * Kept for the cloud: not void and z_min < zf <= z_max on the stored float zf.  The cloud is the 16-byte records
 *   struct { float x, y, z; uint8_t b, g, r, a; }     a = 255
 * of the kept pixels in raster order, without gaps.  The colour is the left image of the current pair at (x, y), float pairs
 * quantised as the SGM stage reads them (saturate(rint(f * 255.0f))); under PSM_DEPTH_SGM with a result of psm_sgm_compute_gray
 * it is that call's left plane, the byte three times. */
enum { PSM_DEPTH_GIF = 0, PSM_DEPTH_SGM = 1 };                            /* sources */
enum { PSM_DEPTH_XYZ = 1, PSM_DEPTH_Z = 2, PSM_DEPTH_CLOUD = 4 };         /* outputs */
enum { PSM_DEPTH_USE_MASK = 1 };                                          /* flags */
/* Q: 16 finite doubles, row-major; crop_x, crop_y in [-32768, 32767].  No Q is set in a new context; it survives
 * psm_release_scratch. */
int psm_reproject_set_q(psm_ctx *ctx, const double Q[16], int crop_x, int crop_y);
/* z_min < z_max, neither NaN (infinities are allowed).  A new context has (0, FLT_MAX). */
int psm_reproject_set_range(psm_ctx *ctx, float z_min, float z_max);
/* The outputs asked for (a non-empty set of PSM_DEPTH_*: the [H][W][3] float plane, the [H][W] float plane of z alone, the
 * cloud) of `source`, in three launches whatever the data (two without the cloud): the points, the dense planes and one count
 * of kept pixels per tile; the tiles' offsets; the records.  *count: the number of kept pixels (with or without the cloud).
 * Synchronous unless PSM_OPT_ASYNC: then the count travels to a page-locked slot and psm_reproject_wait collects it (count may
 * be NULL).  Buffers are allocated on first use, for the outputs asked for only (12, 4 and 16 bytes per pixel), and given back
 * by psm_release_scratch.  Refused with nothing enqueued and the previous result intact: no Q set, an unknown source, output
 * or flag bit, outputs == 0, a GIF source without current maps or with maps that cover a row stripe only, PSM_DEPTH_USE_MASK
 * without a current mask or with an SGM source, an SGM source with neither a compute nor the hook plane, PSM_DEPTH_CLOUD
 * without a current pair. */
int psm_reproject(psm_ctx *ctx, int source, int outputs, int flags, uint32_t *count);
int psm_reproject_wait(psm_ctx *ctx, uint32_t *count);
/* The dense planes of the last psm_reproject / psm_reproject_batch (either pointer may be NULL; one that is not must have been
 * among its outputs): z as H rows of W floats stride_bytes apart, xyz as H rows of 3 W floats 3 * stride_bytes apart;
 * stride_bytes 0: packed, else a multiple of 4 that is >= 4 W.  Synchronises. */
int psm_reproject_download(psm_ctx *ctx, float *xyz, float *z, size_t stride_bytes);
/* The records of the last run (which had PSM_DEPTH_CLOUD), *written of them; max_records below the count is refused. */
int psm_reproject_download_cloud(psm_ctx *ctx, void *records, uint32_t max_records, uint32_t *written);
/* psm_reproject of the n contexts ctxs[0..n) in one set of launches, the context on a grid axis of its own.  Same width,
 * height and device on all; each context uses its own Q, crop, range and result.  The launches run on ctxs[0]'s stream,
 * ordered as psm_score_batch's; synchronous with the counts in counts[0..n) unless ctxs[0] has PSM_OPT_ASYNC.  Afterwards
 * every context is exactly where its own psm_reproject would have left it. */
int psm_reproject_batch(psm_ctx *const *ctxs, int n, int source, int outputs, int flags, uint32_t *counts);
/* Device ms of the launches of the last psm_reproject (a batch: on ctxs[0], for all pairs); needs PSM_OPT_PROFILE. */
int psm_reproject_time(psm_ctx *ctx, double *ms);

/* ---- WLS smoothing: the confidence-weighted, edge-aware global smoothing of a sub-pixel disparity map that users of
 * cv::StereoSGBM apply at this point (cv::ximgproc::DisparityWLSFilter), by Min et al.'s Fast Global Smoother - separable
 * tridiagonal solves along rows and columns, guided by the left image.  It fills the holes of the int16 map from
 * their surroundings, keeps depth edges on image edges and keeps the sixteenths.  It follows no library's convention: the
 * definition is tests/wls_model.py; the device equals it in every bit.  Agreement with a live OpenCV is unpinned.  An
 * independent stage like psm_score: it reads the context's current result and writes planes of its own - it never writes the
 * SGM map, the 8-bit maps or the masks. ----
 * Inputs: an int16 map v[H][W] in 16ths with its invalid value inv, and a guide g[H][W][ch] of bytes - the left image exactly
 * as psm_reproject takes the cloud's colours from it: the current pair's, float pairs quantised as the SGM stage reads them
 * (saturate(rint(f * 255.0f))), or under PSM_WLS_SGM with a result of psm_sgm_compute_gray that call's left plane as one channel.
 * Sources.  PSM_WLS_SGM: the int16 map of the last psm_sgm_compute* (the plane of psm_score_upload_sgm_map while it is on) with
 * inv = (min_disparity - 1) * 16 of the range it belongs to - never the stage's own published result.  PSM_WLS_GIF: the current
 * LEFT 8-bit map, v = byte * 16, inv = -16; nothing is missing, except under PSM_WLS_USE_MASK the pixels whose left validity
 * byte is 0.
 * Link indices: kh[y][x] = max over channels |g[y][x] - g[y][x+1]| (x < W-1), kv[y][x] the same between rows y and y+1; 0..255.
 * Weight table: tab[k] = (float)exp(-(double)k / (double)sigma), k = 0..255, formed on the host with the C library's exp.
 * Per-iteration lambda: lam_t = (float)((1.5 * (double)lambda * (double)4^(T-1-t)) / (double)(4^T - 1)), t = 0..T-1.
 * Start: den = valid ? 1.0f : 0.0f, num = valid ? (float)v : 0.0f.
 * Iterations: for t = 0..T-1, first every row, then every column, as one line of N pixels with link indices k[0..N-2].  All
 * fp32, every operation rounded on its own (no FMA), 1.0f / m a correctly rounded division, subnormals kept; N = 1 is the identity:
 *   lw[n] = lam_t * tab[k[n]]                 a[n] = n > 0   ? -lw[n-1] : 0
 *                                             c[n] = n < N-1 ? -lw[n]   : 0
 *   b[n] = (1 - a[n]) - c[n]
 *   m = n ? b[n] - cp[n-1]*a[n] : b[0];       r = 1.0f / m;      cp[n] = c[n] * r
 *   np[n] = (num[n] - np[n-1]*a[n]) * r       (n = 0: num[0] * r)        dp likewise from den
 *   back:  u[N-1] = np[N-1];  u[n] = np[n] - cp[n]*u[n+1]                 likewise for den
 * num and den are replaced by their u.  (m lies in [1, 1 + 2 lam_t]: r is always normal; the subnormals arise in np, dp and u.
 * In fp32 that holds while 1.5 * lambda stays below 2^24; beyond it m can round to 0 next to a cut link, and the pixels the NaNs
 * reach are void in the result.)
 * End: q = num / den, one correctly rounded division.  A pixel is good if den >= 0x1p-64f and q is finite (below that mass it is
 * connected to no valid pixel).  A good pixel gets min(max(rintf(q), inv + 1), 32767), every other pixel inv: the result has the
 * conventions of the map it came from.  The float plane holds q for good pixels and the stored pattern 0x7FC00000 elsewhere. */
enum { PSM_WLS_GIF = 0, PSM_WLS_SGM = 1 };                                /* sources (numbered as PSM_DEPTH_*) */
enum { PSM_WLS_USE_MASK = 1, PSM_WLS_CONFIDENCE = 2 };                    /* flags */
enum { PSM_WLS_CONF_LR = 1, PSM_WLS_CONF_VAR = 2 };                       /* terms of the graded confidence */
/* PSM_WLS_CONFIDENCE (the SGM source only): the start is graded - den = (float)conf, num = (float)conf * (float)v, one exact
 * multiply - with a confidence byte per pixel from the left-right consistency of the SGM stage's summed costs S and from the
 * variance of the map around the pixel; everything behind the start is unchanged.  The definition is tests/wls_conf_model.py,
 * all integer; the device equals it in every bit.  (A confidence of 255 everywhere is not the unflagged start bit for bit: a
 * call without the flag is the stage as it ever was.)
 *   right16[y][xr]  the right view's map in 16ths from the S [H][W][D] of the last psm_sgm_compute* with its range (dmin, D): the
 *                   smallest (S[y][xr + dmin + k][k], k) over the k in [0, D) with 0 <= xr + dmin + k < W, the lowest k on ties;
 *                   xl = xr + dmin + k, S0 that minimum; inner = 0 < k < D-1 and xl-1 >= 0 and xl+1 < W; Sm = S[y][xl-1][k-1],
 *                   Sp = S[y][xl+1][k+1]; den = max(Sm + Sp - 2 S0, 1), sub = floor(((Sm - Sp) 16 + den) / (2 den)); the value is
 *                   (dmin + k) 16 + (inner ? sub : 0); a column without a candidate gets rinv = (dmin - 1) 16.
 *   L-R term        0 where v == inv; else xq = x - ((v + 8) >> 4), arithmetic; 0 if xq is outside [0, W) or right16[y][xq] ==
 *                   rinv; else 255 - min((|v - right16[y][xq]| 255) / lr_thresh, 255), the quotient floored.
 *   variance term   over the (2 radius + 1)^2 window, pixels outside the image and invalid ones contributing nothing: n the
 *                   count, s the sum of v, ss the sum of v^2, t = floor((255 (n ss - s^2)) / (n^2 << var_shift)); 255 - min(t, 255)
 *                   where the centre is valid, 0 elsewhere (var_shift 8: one step per square pixel of disparity variance).
 *   conf            floor((c_var c_lr + 127) / 255), a term that is switched off counting as 255, an invalid pixel 0.
 * Out of scope: a confidence for the GIF source, a speckle or uniqueness pass on the right map, a confidence supplied by the
 * host; agreement with a live OpenCV stays unpinned, like the rest of the stage.
 * psm_wls_set_confidence: terms in {1, 2, 3}, lr_thresh in [1, 32767], radius in [1, 4], var_shift in [0, 16].  A new context has
 * (PSM_WLS_CONF_LR | PSM_WLS_CONF_VAR, 24, 2, 8); the parameters survive psm_release_scratch.
 * Under the flag psm_wls_filter and psm_wls_filter_batch launch k_sgm_right16 (if a member has the L-R term; members without it
 * take no part) and k_wls_conf ahead of their 1 + 2 T launches; a batch uses every member's own terms and parameters.  The two
 * planes - 3 more bytes per pixel - are allocated on first use and given back by psm_release_scratch.  Refused ahead of the first
 * launch, the previous result intact (a batch: naming the member): the flag with PSM_WLS_GIF; the L-R term while the plane of
 * psm_score_upload_sgm_map is on (S does not belong to it) or without the S of a psm_sgm_compute* of this context (never
 * computed, or released), or with a range or width k_sgm_right16 cannot serve.  The variance term alone needs only the map. */
int psm_wls_set_confidence(psm_ctx *ctx, int terms, int lr_thresh, int radius, int var_shift);
/* The confidence bytes and the right map of the last psm_wls_filter; either pointer may be NULL.  conf as H rows of W bytes
 * conf_stride apart, right16 as H rows of W int16 right_stride_bytes apart (0: packed; right_stride_bytes even).  Refused after
 * a call without PSM_WLS_CONFIDENCE, and right16 after one without the L-R term.  Synchronises. */
int psm_wls_download_confidence(psm_ctx *ctx, uint8_t *conf, size_t conf_stride, int16_t *right16, size_t right_stride_bytes);
/* Device ms of the two launches PSM_WLS_CONFIDENCE adds (they lie inside psm_wls_time's bracket too); needs PSM_OPT_PROFILE. */
int psm_wls_conf_time(psm_ctx *ctx, double *ms);
/* lambda > 0, sigma > 0, both finite; iterations in [1, 4].  A new context has (8000, 1.5, 3); the parameters survive
 * psm_release_scratch. */
int psm_wls_set_params(psm_ctx *ctx, float lambda, float sigma, int iterations);
/* The filter of `source` on the context's stream, in 1 + 2 T launches whatever the data: num, den and the link indices; per
 * iteration one pass over the rows and one over the columns, the last of which forms the quotient.  Synchronous unless
 * PSM_OPT_ASYNC: then psm_wls_wait waits for it (the downloads do so too).  The planes - 35 bytes per pixel - are allocated on
 * first use and given back by psm_release_scratch.  Refused with nothing enqueued and the previous result intact: an unknown
 * source or flag bit, a GIF source without current maps or with maps that cover a row stripe only, PSM_WLS_USE_MASK without a
 * current mask or with the SGM source, the SGM source with neither a compute nor the hook plane, no current image pair (except
 * under PSM_WLS_SGM after psm_sgm_compute_gray, whose left plane guides). */
int psm_wls_filter(psm_ctx *ctx, int source, int flags);
/* psm_wls_filter of the n <= 4096 contexts ctxs[0..n) in one set of 1 + 2 T launches, the context on a grid axis of its own:
 * the chains of different pairs are independent, so they run side by side.  source and flags apply to every context.  Same
 * width, height, device and iterations on all (T is the batch's); each context uses its own lambda, sigma, map, guide and
 * planes, and uploads its weight table only when its sigma changed.  The launches run on ctxs[0]'s stream, ordered as
 * psm_score_batch's: behind every context's earlier work, ahead of its later work.  Synchronous unless ctxs[0] has
 * PSM_OPT_ASYNC: then every context's psm_wls_wait collects.  Under PSM_OPT_PROFILE psm_wls_time of ctxs[0] is the batch's;
 * the other contexts count as not timed.  Afterwards every context is exactly where its own psm_wls_filter would have left it
 * (its planes, map, table and publishing switch).  Refused with nothing enqueued and every context's previous result intact,
 * the message - on ctxs[0] - naming the context: what psm_wls_filter refuses, a NULL or repeated context, another width, height,
 * device or iterations than context 0.  The table of the contexts' records belongs to ctxs[0] (psm_release_scratch frees it). */
int psm_wls_filter_batch(psm_ctx *const *ctxs, int n, int source, int flags);
int psm_wls_wait(psm_ctx *ctx);
/* The planes of the last psm_wls_filter; any pointer may be NULL.  disp: the filtered int16 map; q: the float plane; num, den:
 * the working planes as the last pass left them (a debug view).  The float planes as H rows of W floats stride_bytes apart,
 * disp as H rows of W int16 stride_bytes / 2 apart; stride_bytes 0: packed, else a multiple of 4 that is >= 4 W.  Synchronises. */
int psm_wls_download(psm_ctx *ctx, int16_t *disp, float *q, float *num, float *den, size_t stride_bytes);
/* The weight table the last psm_wls_filter read on the device. */
int psm_wls_download_table(psm_ctx *ctx, float tab[256]);
/* Device ms of the launches of the last psm_wls_filter; needs PSM_OPT_PROFILE. */
int psm_wls_time(psm_ctx *ctx, double *ms);
/* on != 0: from now on the SGM sources of psm_score, psm_score_batch, psm_reproject and psm_reproject_batch read the map and
 * the invalid value of the last psm_wls_filter (whichever source it had) instead of the SGM stage's - the way to a dense cloud
 * that keeps the sixteenths.  The hook plane of psm_score_upload_sgm_map wins while it is on.  Refused without a result.
 * on == 0, or psm_release_scratch (which frees the planes): every call is again bit for bit what it is without this stage. */
int psm_wls_publish(psm_ctx *ctx, int on);

/* ---- the guided-filter path over a one-channel pair ----
 * Cost build, guided-filter aggregation and winner-takes-all of a monochrome pair in one call: what FastGuidedFilter's dispatch on
 * I.channels() intends (src/fastguidedfilter.cpp:38-49,89-119) - the one-channel reading of GuidedFilter_cv (src/CVF.cpp:72-165) over
 * costs that are myCostGrd (src/CVC.cpp:18-39) with the colour sum over one channel and the x-gradient of the plane itself.  Four box
 * filters per voxel instead of eight, no 3 x 3 solve.  The definition, which the device equals in every bit, is
 * tests/gray_model.py: per side, with I the side's own plane, mI = box(I), inv = 1 / (box(I I) - mI mI + 1e-4f);
 * per slice p: a = inv (box(I p) - mI box(p)), b = box(p) - a mI, q = box(b) + box(a) I; fp32 operations rounded one by one, box =
 * cv::boxFilter(Size(8,8)) in this library's order; selection d = 1 .. max_disp - 1, strict <, default 0.
 * l, r: host planes, H rows of W one-channel pixels stride_bytes apart (0: packed) - bytes (depth PSM_IMG_U8, scaled by 1/255.0f
 * as psm_upload_pair scales) or floats (PSM_IMG_F32, used as they are).  The staged colour pair and its slots are untouched.  The
 * maps go to the context's map buffer and - lmap / rmap, either may be NULL - to H rows of W bytes map_stride apart (0: packed).
 * Afterwards the context is exactly where psm_sgm_select_maps leaves it: whole-image maps are current, there is no mask; volumes,
 * minima and anything pending of the colour path are untouched, so psm_lr_check, psm_fill_invalid, psm_score(PSM_SCORE_GIF),
 * psm_download_maps* and psm_reproject work behind it as they do there.  On the context's stream; synchronous on return unless
 * PSM_OPT_ASYNC is set (the upload of the planes always completes before the call returns).  The PSM_FLAG_* values of the float
 * path are ignored: there is one arithmetic.  No volume is ever held: the stage's buffers - 8 bytes per pixel for the pair, 16 per
 * pixel and side of guidance, 16 per pixel of minima and a scratch of at most 32 slices' {a, b} of both sides (at most 1 GiB,
 * whatever max_disp is) - are allocated on first use and given back by psm_release_scratch and psm_destroy.
 * Refused - psm_last_error names the call, nothing has been enqueued, the previous maps are still current - for a NULL context
 * (psm_last_error(NULL)), NULL planes, an unknown depth, a stride below a row, a map_stride below W, a PSM_U8 context, a disparity
 * shard, a row stripe in force (psm_set_rows).
 * Out of scope: FrameRing, 8-bit mode, rectified upload, and the tail stages that read
 * the image - psm_wgt_median, psm_joint_wmf, the guide of psm_wls_filter and the colours of psm_reproject's cloud keep reading
 * the staged colour pair.  psm_upload_pair* keep refusing 1 channel. */
int psm_gray_compute(psm_ctx *ctx, const void *l, const void *r, size_t stride_bytes, int depth, uint8_t *lmap, uint8_t *rmap,
                     size_t map_stride);
/* psm_gray_compute of the pairs of n contexts (1 <= n <= 4096) in one set of launches, the pair on a grid axis: 2 + 2 per chunk of
 * 32 slices whatever n is (the reference's use on small data is a loop over pairs, src/main.cpp:64-73).  The contexts share width,
 * height, max_disp, device and options, as psm_compute_batch requires; member i takes its own planes ls[i], rs[i]; depth and
 * stride_bytes are the call's.  lmaps / rmaps may be NULL, and so may any entry; else entry i receives member i's map, H rows of W
 * bytes map_stride apart.  The launches run on ctxs[0]'s stream, ordered after everything queued on the members' streams and before
 * anything queued on them later; synchronous on return unless ctxs[0] has PSM_OPT_ASYNC; every host plane has been read before the
 * call returns.  Afterwards every member is exactly where its own psm_gray_compute would have left it - maps, state and the bits
 * of both; the test hooks work on each.  Buffers stay per member; ctxs[0] owns a device table of the members' pointers.
 * psm_gray_time on ctxs[0] gives the batch's device ms; the other members count as not timed.
 * Refused before anything is enqueued on any member - every member's earlier maps stay current, psm_last_error(ctxs[0]) names the
 * call and the member's index (psm_last_error(NULL) for NULL ctxs, n < 1 and a NULL ctxs[0]) - for n out of range, a NULL member,
 * the same context twice, a member whose geometry, device or options differ from ctxs[0]'s, and per member or for the call what
 * psm_gray_compute refuses. */
int psm_gray_compute_batch(psm_ctx *const *ctxs, int n, const void *const *ls, const void *const *rs, size_t stride_bytes, int depth,
                           uint8_t *const *lmaps, uint8_t *const *rmaps, size_t map_stride);
/* psm_gray_compute with the Fast Guided Filter in place of the full-resolution one: FastGuidedFilterMono
 * (src/fastguidedfilter.cpp:89-119), the one-channel half of the reference's FastGuidedFilter(I, 8, 1e-4, subsample_rate)
 * (src/DispEst.cpp:281-296), as psm_cost_filter_fgf is its colour half.  The definition, which the device equals in every bit, is
 * tests/gray_fgf_model.py: with s = subsample_rate in {2, 4, 8}, k = 2 (8 / s) + 1, nn = cv::resize(INTER_NN) to
 * H / s x W / s, blur = cv::blur(Size(k, k)), up = cv::resize(INTER_LINEAR) back to H x W as psm_cost_filter_fgf has them: per side
 * Is = nn(I), mI = blur(Is), den = (blur(Is Is) - mI mI) + 1e-4f; per slice ps = nn(cost), a = (blur(Is ps) - mI blur(ps)) / den (the
 * reference's per-voxel quotient), b = blur(ps) - a mI, q = up(blur(a)) I + up(blur(b)); costs and selection are psm_gray_compute's.
 * The cost is formed at the sampled pixels only; the stage's scratch is two chunks of at most 32 slices' {a, b} of both sides at the
 * subsampled size, whatever max_disp is.  Arguments, state afterwards, stream and timer (psm_gray_time) are psm_gray_compute's;
 * so are the refusals, plus a subsample_rate outside {2, 4, 8} and a W / s or H / s not above 8 / s (psm_cost_filter_fgf's bound).
 * psm_gray_compute_fgf_batch is to it what psm_gray_compute_batch is to psm_gray_compute: 2 + 3 launches per chunk whatever n is.
 * The hooks of one form are refused after a call of the other form: the planes belong to the last call of the stage.
 * psm_gray_fgf_guidance: planes receives [3][H / s][W / s] floats of `side`: Is, mI, den.
 * psm_gray_fgf_volume: the slices [d0, d1) of `side` through the storing instantiation of the same kernels: q receives
 * [d1-d0][H][W] floats, model - may be NULL - [d1-d0][4][H / s][W / s]: a, b, blur(a), blur(b) of every slice.  The chunks of the
 * walk begin at d0.  Keys and maps are not touched.  Both synchronise. */
int psm_gray_compute_fgf(psm_ctx *ctx, const void *l, const void *r, size_t stride_bytes, int depth, int subsample_rate, uint8_t *lmap,
                         uint8_t *rmap, size_t map_stride);
int psm_gray_compute_fgf_batch(psm_ctx *const *ctxs, int n, const void *const *ls, const void *const *rs, size_t stride_bytes, int depth,
                               int subsample_rate, uint8_t *const *lmaps, uint8_t *const *rmaps, size_t map_stride);
int psm_gray_fgf_guidance(psm_ctx *ctx, int side, float *planes);
int psm_gray_fgf_volume(psm_ctx *ctx, int side, int d0, int d1, float *q, float *model);
/* Device ms of the launches of the last psm_gray_compute or psm_gray_compute_fgf (guidance, every chunk, the maps); needs
 * PSM_OPT_PROFILE. */
int psm_gray_time(psm_ctx *ctx, double *ms);
/* Test hooks on the pair of the last psm_gray_compute (refused before any, and after psm_release_scratch).
 * psm_gray_guidance: planes receives [4][H][W] floats of `side`: I, G, mI, inv.
 * psm_gray_volume: the slices [d0, d1) of `side` through the storing instantiation of the same kernels (slice 0 included, which
 * the selection never computes): q receives [d1-d0][H][W] floats, ab - may be NULL - [d1-d0][2][H][W]: the planes a and b of
 * every slice.  The chunks of the walk begin at d0.  Keys and maps are not touched.  Both synchronise. */
int psm_gray_guidance(psm_ctx *ctx, int side, float *planes);
int psm_gray_volume(psm_ctx *ctx, int side, int d0, int d1, float *q, float *ab);

/* ---- debug / bench entry points (no counterpart in the reference) ---- */
/* Test hook of the score stage: an int16 map (H rows of W values, pitch stride_bytes; 0: packed) that the SGM sources of
 * psm_score read from now on instead of the map of the last psm_sgm_compute - maps no compute would produce.  Kept in a plane
 * of its own: the SGM stage and its readers never see it.  disp NULL: the hook map is dropped again. */
int psm_score_upload_sgm_map(psm_ctx *ctx, const int16_t *disp, size_t stride_bytes);
/* Replace the device maps and validity masks (any may be NULL = keep) - lets the post-processing stages run on maps
 * that did not come from this context's WTA.  H rows of W bytes, pitch `stride`; map values must be < max_disp. */
int psm_upload_maps(psm_ctx *ctx, const uint8_t *lmap, const uint8_t *rmap, const uint8_t *lvalid, const uint8_t *rvalid,
                    size_t stride);

/* Copy slices [d0,d1) (global disparity numbers) of a volume to/from dense host memory
 * [d1-d0][H][W]; element type = the context's dtype. */
int psm_download_volume(psm_ctx *ctx, int side, int d0, int d1, void *host);
/* Uploaded float costs may have any scale: slices whose non-zero magnitudes leave 2^-60 .. 2^60 (measured on the device) make
 * the following psm_cost_filter run its storing form (see PSM_IMG_F32 above) - same results as the reference arithmetic at any
 * scale, never a silent difference between the two forms. */
int psm_upload_volume(psm_ctx *ctx, int side, int d0, int d1, const void *host);
/* After psm_cost_filter: the a0,a1,a2,b intermediates of the LAST filtered side (right) are
 * still in the scratch buffer; psm_filter_stage_a(side) runs only the first half of the
 * guided filter for `side` and leaves them there.  host: [d1-d0][H][W][4] floats. */
int psm_filter_stage_a(psm_ctx *ctx, int side);
int psm_download_ab(psm_ctx *ctx, int d0, int d1, float *host);
/* guidance planes of `side` after psm_cost_filter/psm_filter_stage_a: host receives
 * [14][H][W] floats: I0,I1,I2,grad, mI0,mI1,mI2,invDET, A00,A01,A02,A11,A12,A22.  (PSM_U8 contexts: `grad` is the 8-bit
 * gradient of assets/cvc.cl's preprocessing as a float - the float x-gradient is not kept in that mode.) */
int psm_download_guidance(psm_ctx *ctx, int side, float *host);
/* The north-star kernel in isolation: cv::boxFilter(Size(8,8)) semantics applied to every
 * slice of volume `side`, result left in the scratch buffer; host (optional) receives
 * [Dlocal][H][W] floats. */
int psm_box8_volume(psm_ctx *ctx, int side, float *host);

/* Wall time of the last call of each stage in microseconds (the reference's
 * cvc_time/cvf_time/dispsel_time, src/StereoMatch.cpp:227-241). */
int psm_stage_time_us(psm_ctx *ctx, int stage, double *us);
/* With PSM_OPT_PROFILE=1: accumulated device time (hipEvent pairs on the launch stream)
 * and launch count of a kernel class since the last psm_reset_kernel_times(). */
int psm_kernel_time_ms(psm_ctx *ctx, int kernel, double *total_ms, int *launches);
int psm_reset_kernel_times(psm_ctx *ctx);
/* With PSM_OPT_PROFILE=2: duration in ms (first workgroup start to last workgroup end, device constant-rate clock) and form
 * (1 = minima planes, 2 = key plane, 0 = storing) of every launch of the fused filter kernel since the last call, in launch
 * order; at most max_launches (the library keeps 4096).  A phase without a live work item (the minima planes of a forced
 * two-phase selection whose only seed slice is d = 0) starts no kernel and leaves no record.  Costs two 64-bit atomics per workgroup and no events or
 * synchronisation between kernels, so it can stay on inside a timed region.  Resets the record. */
int psm_filter_launch_times(psm_ctx *ctx, double *ms, int *form, int max_launches, int *n_launches);

/* geometry queries */
int psm_get_info(const psm_ctx *ctx, int *width, int *height, int *max_disp, int *d_begin,
                 int *d_end, int *dtype, int *device);

#ifdef __cplusplus
}
#endif
#endif
