/*
 * ms_stitch.h -- C-ABI of libmsstitch.so: the MI355X-native (gfx950, hand-written HIP) per-frame
 * 360-degree stitching compositor.  Drop-in boundary for the hot path of ultravideo/video-stitcher
 * (360_stitcher/timed.cpp stitch_online/stitch_one -> OpenCV-3.4-fork MultiBandBlender
 * feed_online/blend and the cv::cuda:: image ops underneath).
 *
 * The reference has no FFI layer; its seam is (1) the host<->.cu launcher boundary -- free functions
 * taking POD PtrStepSz<T> {data, step, cols, rows} + cudaStream_t -- and (2) the C++ API of
 * cv::cuda::* / detail::MultiBandBlender / detail::*WarperGpu.  This header restates both as plain C:
 * every entry point cites the reference interface it replaces (paths relative to the reference
 * repo; OCV = sources/modules, APP = 360_stitcher).  INTEGRATION.md shows the C++ shim a
 * maintainer adds so that timed.cpp-style callers compile unchanged.
 *
 * Conventions
 *   - ms_image has the fields of cv::cuda::PtrStepSz<T> in the reference's own order -- {data, step} (PtrStep, cuda_types.hpp:95-107) then
 *     {cols, rows} (PtrStepSz, :109-120) -- followed by the OpenCV type code: it is filled from a cv::cuda::GpuMat without copying,
 *     {m.data, m.step, m.cols, m.rows, m.type()}, and the kernels' by-value PtrStepSz arguments map onto its first four fields.
 *     All ms_image pointers are DEVICE pointers unless a parameter says "host".
 *   - ms_stream is a hipStream_t (NULL = the default stream).  Calls only enqueue work.
 *   - Every function returns MS_OK (0) or a negative ms_status; ms_last_error() returns the
 *     message of the calling thread's most recent failure (cf. sts_net_get_last_error, APP/netlib.h:74).
 *     Nothing throws across this boundary (the reference throws cv::Exception: OCV/core/include/
 *     opencv2/core/cuda/common.hpp:66-75).
 *   - There is NO CPU fallback: without a HIP device every compute entry point fails with
 *     MS_ERR_NO_DEVICE (the reference's no-CUDA build does throw_no_cuda(), OCV/cudawarping/src/remap.cpp:47).
 */
#ifndef MS_STITCH_H
#define MS_STITCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MS_API __attribute__((visibility("default")))

typedef enum ms_status {
    MS_OK = 0,
    MS_ERR_INVALID = -1,      /* bad argument (CV_Assert in the reference)          */
    MS_ERR_UNSUPPORTED = -2,  /* type/flag combination the hot path never uses      */
    MS_ERR_HIP = -3,          /* HIP runtime error (cudaSafeCall in the reference)  */
    MS_ERR_NO_DEVICE = -4,    /* no gfx950 device visible                           */
    MS_ERR_STATE = -5,        /* call order violated (e.g. stitch before calibrate) */
    MS_ERR_NOMEM = -6,
    MS_ERR_COMM = -7          /* multi-GPU transport (RCCL / host mailbox) failure or timeout: ms_dist.h */
} ms_status;
#define MS_ERR_COMM MS_ERR_COMM

/* OpenCV type codes CV_MAKETYPE(depth, cn) = depth + ((cn-1) << 3)  (OCV/core/include/opencv2/core/hal/interface.h) */
enum { MS_8UC1 = 0, MS_8UC3 = 16, MS_16SC1 = 3, MS_16SC3 = 19, MS_32FC1 = 5 };
/* cv::BorderTypes / cv::InterpolationFlags values used on the path */
enum { MS_BORDER_CONSTANT = 0, MS_BORDER_REFLECT = 2 };
enum { MS_INTER_NEAREST = 0, MS_INTER_LINEAR = 1,
       MS_INTER_LINEAR_FIXPT = 0x101 };   /* cv::remap's CPU arithmetic (1/32-px coordinates, 15-bit weight table; imgwarp.cpp:211-284, :643-850, :1203-1270) */
/* warper kinds: detail::{Plane,Cylindrical,Spherical}WarperGpu (OCV/stitching/include/opencv2/stitching/detail/warpers.hpp:435-550) */
enum { MS_PROJ_PLANE = 0, MS_PROJ_CYLINDRICAL = 1, MS_PROJ_SPHERICAL = 2 };

typedef struct ms_image {   /* PtrStepSz<T> field for field (OCV/core/include/opencv2/core/cuda_types.hpp:95-120), then the type code */
    void *data;
    size_t step;            /* row pitch in bytes: any value >= the row's bytes (cols * element size) -- pitched allocations and ROIs of larger images as they are;
                             * the images of ms_stitch* / ms_feed additionally need step < 2^24 (16 MiB) and rows * step < 2^32 (see ms_stitch) */
    int cols, rows;         /* PtrStepSz order: cols first */
    int type;
} ms_image;

typedef struct ms_rect { int x, y, width, height; } ms_rect;   /* cv::Rect */
typedef void *ms_stream;                                        /* hipStream_t */

MS_API const char *ms_last_error(void);
MS_API const char *ms_version(void);
MS_API int ms_device_count(void);       /* cuda::getCudaEnabledDeviceCount (blenders.cpp:226) */

/* =============================================================================================
 * 1. Image-op entry points: one per cv::cuda:: call / device launcher on the hot path
 * ============================================================================================= */

/* cuda::remap(src, dst, xmap, ymap, INTER_LINEAR|INTER_NEAREST, borderMode, Scalar(0), stream)
 * OCV/cudawarping/src/remap.cpp:61-102 -> device::imgproc::remap_gpu<uchar3|uchar> (cuda/remap.cu:56-86).
 * BORDER_CONSTANT(0): 8UC3 linear, 8UC1 linear/nearest (the per-frame warps, timed.cpp:84-101; mask warps);
 * BORDER_REFLECT: 8UC3 linear (the seam-scale image warp, calibration.cpp:118).  dst.size == xmap.size == ymap.size.
 * MS_INTER_LINEAR_FIXPT (8UC1 / 8UC3, BORDER_CONSTANT) is the CPU cv::remap(..., INTER_LINEAR) flavour instead: what MeshWarper::createMesh
 * warps its images with (meshwarper.cpp:72) and what the reference's CPU pipeline (BASELINE configs[0]) produces, bit for bit. */
MS_API int ms_remap(const ms_image *src, const ms_image *xmap, const ms_image *ymap, ms_image *dst,
                    int interpolation, int border_type, ms_stream stream);

/* cuda::resize(src, dst, Size(), fx, fy, INTER_LINEAR, stream)  OCV/cudawarping/src/resize.cpp:57-106
 * -> device::resize<uchar3|uchar> (cuda/resize.cu:71-106).  Two call forms, as resize.cpp:72-81:
 *   fx > 0 && fy > 0  (the app's form, Size() + compose_scale, APP/timed.cpp:77): dst must be
 *                     saturate_cast<int>(cols*fx) x saturate_cast<int>(rows*fy); the kernel gets 1/fx, 1/fy;
 *   fx == 0 && fy == 0: dsize = dst size; fx = dsize.width / src.cols, fy likewise. */
MS_API int ms_resize_linear(const ms_image *src, ms_image *dst, double fx, double fy, ms_stream stream);
/* The same for n 8UC3 images of one geometry in ONE launch: stitch_online's cuda::resize of every view by compose_scale (APP/timed.cpp:75-85 -- on the
 * per-frame path with the shipped COMPOSE_MEGAPIX, defs.h:53) for all views of a frame (or of a batch of frames).  Bit-identical to n ms_resize_linear calls. */
MS_API int ms_resize_linear_batch(const ms_image *src, ms_image *dst, int n, double fx, double fy, ms_stream stream);
/* cvtColor(YUV2BGR_NV12) (APP/networking.cpp:45-47) and that cuda::resize (APP/timed.cpp:75-85) in ONE pass: what a rig with NV12 cameras (defs.h:10-17) and the
 * shipped COMPOSE_MEGAPIX (defs.h:53) does to every frame before the warp, without the full-size BGR image in between.  src_nv12: n DEVICE 8UC1 images of
 * (rows * 3 / 2) x cols -- Y plane, then interleaved UV -- with even rows and cols, one geometry and one step; dst_bgr: n 8UC3 images of one size.  The two call
 * forms are those of ms_resize_linear (fx, fy > 0 with the saturate_cast<int>(cols * fx) size check against the FRAME size rows x cols, or both 0 = dst's size).
 * Each of the four taps is converted from the planes with cvtColor's integer formula first; coordinates, clamps, weights, fma order and saturation are those of
 * ms_resize_linear: bit-identical to ms_nv12_to_bgr_batch followed by ms_resize_linear_batch.  Equal sizes are refused as there (ms_nv12_to_bgr_batch is the whole job). */
MS_API int ms_nv12_resize_linear_batch(const ms_image *src_nv12, ms_image *dst_bgr, int n, double fx, double fy, ms_stream stream);

/* GpuMat::convertTo(dst, same type, alpha)  OCV/core/src/cuda/gpu_mat.cu:488-512 (exposure gain,
 * APP/timed.cpp:94 / GainCompensator::apply_gpu exposure_compensate.cpp:155-160).  8U any channels, in place ok. */
MS_API int ms_convert_scale_8u(const ms_image *src, ms_image *dst, double alpha, ms_stream stream);

/* GpuMat::convertTo(dst, rtype[, alpha], stream) for the depth changes the path uses:
 * 8U->16S (blenders.cpp:713), 16S->8U (APP/timed.cpp:251), 8U->32F with alpha (blenders.cpp:412). */
MS_API int ms_convert(const ms_image *src, ms_image *dst, double alpha, ms_stream stream);

/* cuda::copyMakeBorder(src, dst, top, bottom, left, right, borderType, Scalar(), stream)
 * OCV/cudaarithm/src/cuda/copy_make_border.cu:126-157.  BORDER_REFLECT for 8UC3/8UC1 (blenders.cpp:711),
 * BORDER_CONSTANT(0) for 32FC1 (blenders.cpp:420). */
MS_API int ms_copy_make_border(const ms_image *src, ms_image *dst, int top, int bottom, int left, int right,
                               int border_type, ms_stream stream);

/* cuda::pyrDown(src, dst, stream)  OCV/cudawarping/src/pyramids.cpp:66-92 -> pyrDown_gpu<short3|float>
 * (cuda/pyr_down.cu:55-188).  16SC3, 16SC1, 32FC1; dst must be ((rows+1)/2, (cols+1)/2). */
MS_API int ms_pyr_down(const ms_image *src, ms_image *dst, ms_stream stream);

/* cuda::pyrUp(src, dst, stream)  OCV/cudawarping/src/pyramids.cpp:106-132 -> pyrUp_gpu<short3>
 * (cuda/pyr_up.cu:55-157).  16SC3 / 16SC1; dst must be (2*rows, 2*cols). */
MS_API int ms_pyr_up(const ms_image *src, ms_image *dst, ms_stream stream);

/* cuda::subtract / cuda::add on CV_16S, no mask  OCV/cudaarithm/src/element_operations.cpp:182,170
 * -> SubOp1/AddOp1<short> (cuda/sub_mat.cu:59-65, cuda/add_mat.cu:59-65).  dst may alias a or b. */
MS_API int ms_subtract_16s(const ms_image *a, const ms_image *b, ms_image *dst, ms_stream stream);
MS_API int ms_add_16s(const ms_image *a, const ms_image *b, ms_image *dst, ms_stream stream);

/* device::blend::addSrcWeightGpu32F(src, src_weight, dst, dst_weight, rc)
 * OCV/stitching/src/blenders.cpp:54-55 -> cuda/multiband_blend.cu:36-60.  dst/dst_weight are the
 * already-offset ROI views (dst(rc)), rc_width x rc_height is the rect size. */
MS_API int ms_add_src_weight_32f(const ms_image *src, const ms_image *src_weight, ms_image *dst,
                                 ms_image *dst_weight, int rc_width, int rc_height, ms_stream stream);

/* device::blend::normalizeUsingWeightMapGpu32F(weight, src, width, height)
 * blenders.cpp:58-59 -> cuda/multiband_blend.cu:85-108. */
MS_API int ms_normalize_using_weight_32f(const ms_image *weight, ms_image *src, int width, int height,
                                         ms_stream stream);

/* The fixed-point flavour of the same two launchers -- MultiBandBlender(weight_type = CV_16S): weights 0..256 (8 fractional bits, blenders.cpp:414-418).
 * device::blend::addSrcWeightGpu16S / normalizeUsingWeightMapGpu16S  blenders.cpp:52-53,56-57 -> cuda/multiband_blend.cu:10-34, 62-83:
 * dst += short((src * w) >> 8), dst_weight += w;  src = short((src << 8) / w).  The app never selects this flavour (weight_type_ stays CV_32F,
 * blenders.hpp:129); provided per-op for completeness of the blender's launcher surface.  A zero weight in the normalise step is an integer division
 * by zero in the reference (undefined); here the result is 0. */
MS_API int ms_add_src_weight_16s(const ms_image *src, const ms_image *src_weight, ms_image *dst,
                                 ms_image *dst_weight, int rc_width, int rc_height, ms_stream stream);
MS_API int ms_normalize_using_weight_16s(const ms_image *weight, ms_image *src, int width, int height,
                                         ms_stream stream);

/* cuda::compare(src32F, eps, dst8U, CMP_GT) / cuda::compare(src8U, 0, dst8U, CMP_EQ)
 * OCV/cudaarithm/src/element_operations.cpp:292 -> cuda/cmp_scalar.cu:59-82 (blenders.cpp:803,808). */
MS_API int ms_compare_gt_32f(const ms_image *src, float thr, ms_image *dst, ms_stream stream);
MS_API int ms_compare_eq_8u(const ms_image *src, int val, ms_image *dst, ms_stream stream);

/* GpuMat::setTo(Scalar::all(0), mask, stream) on 16SC3  gpu_mat.cu:369-374,431 (blenders.cpp:810) */
MS_API int ms_set_zero_masked_16sc3(ms_image *img, const ms_image *mask, ms_stream stream);

/* cuda::bitwise_and 8UC1 (APP/calibration.cpp:237) and the 3x3 dilation of APP/calibration.cpp:209,232 */
MS_API int ms_bitwise_and_8u(const ms_image *a, const ms_image *b, ms_image *dst, ms_stream stream);
MS_API int ms_dilate3x3_8u(const ms_image *src, ms_image *dst, ms_stream stream);

/* seam_finder->find(images_warped, corners, masks_warped) with the VoronoiSeamFinder (APP/calibration.cpp:134-135 -> VoronoiSeamFinder::find / findInPair,
 * OCV/stitching/src/seam_finders.cpp:85-160): for every pair i < j whose ROIs overlap, in the reference's order, the overlap's pixels nearer (L1, strictly) to
 * view i's own pixels are cleared from mask j, all others from mask i.  masks: n DEVICE 8UC1 images, masks[i] exactly rois[i].width x rois[i].height with
 * contiguous rows (step == width), edited IN PLACE as the reference edits masks_warped: pair (0, 1)'s result is pair (0, 2)'s input.  Any non-zero value counts
 * as set.  rois: HOST, corner + size of every view.  SYNCHRONOUS: allocates its distance planes and returns after `stream` has drained.
 * MS_ERR_INVALID (checked before the device is touched): n outside [1, MS_MAX_VIEWS], a null pointer, an empty ROI, a mask of another type or size than its
 * ROI, or rows that are not contiguous (nothing is staged: pass a packed copy). */
MS_API int ms_voronoi_seams(int n, const ms_rect *rois, ms_image *masks, ms_stream stream);
/* compensator->feed(corners, images_warped, masks_warped) with the GainCompensator (APP/calibration.cpp:122-132 -> GainCompensator::feed,
 * OCV/stitching/src/exposure_compensate.cpp:71-145): per pair i <= j with overlapping ROIs, N = max(1, #pixels where both masks are 255) and the mean of
 * sqrt(b^2 + g^2 + r^2) of either view over those pixels (double sums in raster order), the normal equations (alpha 0.01, beta 100) and cv::solve(DECOMP_LU).
 * images: n DEVICE 8UC3 (step == 3 * width), masks: n DEVICE 8UC1 (step == width), each exactly its ROI's size; rois and gains_host (n doubles): HOST.
 * N_host / I_host (HOST, n x n row-major, either may be NULL): the overlap counts and mean intensities the solve consumed, 0 where two ROIs do not meet.
 * SYNCHRONOUS: allocates, and returns after `stream` has drained.  MS_ERR_INVALID as for ms_voronoi_seams (checked before the device is touched), and for a
 * singular system (not reachable while every N[i][i] >= 1). */
MS_API int ms_estimate_gains(int n, const ms_rect *rois, const ms_image *images, const ms_image *masks,
                             double *gains_host, int *N_host, double *I_host, ms_stream stream);
/* Content-aware seams: seam_finder->find(images_warped, corners, masks_warped) (APP/calibration.cpp:134-135) with a minimum-cost path through every overlap instead
 * of the VoronoiSeamFinder, which never looks at a pixel (the reference's own comment, calibration.cpp:207: "Better solution might be needed").  In the spirit of
 * detail::DpSeamFinder (OCV/stitching/src/seam_finders.cpp) but NOT a restatement of it: the contract is the one below, all of it integer arithmetic, so results
 * are bit-exact and two calls return the same bytes (tests/dp_seam_ref.py is its numpy statement).
 * Arguments as for ms_estimate_gains / ms_voronoi_seams: images n DEVICE 8UC3 (step == 3 * width), masks n DEVICE 8UC1 (step == width), each exactly its ROI's
 * size; rois HOST; a set mask pixel is != 0; masks are edited IN PLACE, pairs i < j with overlapping ROIs in the reference's order (PairwiseSeamFinder::run), so
 * pair (0, 1)'s result is pair (0, 2)'s input.  SYNCHRONOUS: allocates its scratch and returns after `stream` has drained.
 * One pair, with the overlap rectangle O of w x h pixels:
 *   Orientation and sides.  Per view: its set pixels inside O grown by 10 on every side (ms_voronoi_seams' gap) and clipped to the view's ROI, coordinates
 *     relative to (O.x - 10, O.y - 10); n, Sx, Sy their count and coordinate sums (int64).  dx = Sx_j n_i - Sx_i n_j, dy likewise: the sign of the difference of
 *     the two centroids.  The seam is VERTICAL (one column per row) if |dx| >= |dy|, else HORIZONTAL (one row per column): the same algorithm on the transpose.
 *     The first side -- the columns <= the seam's -- belongs to view i if the chosen d >= 0, else to view j.  Pixels decide, not ROI centres: the view that
 *     straddles +-pi has a full-width ROI.
 *   Cost.  B = the pixels of O set in both masks.  c = |db| + |dg| + |dr| (0 .. 765) on B, 1024 elsewhere in O.
 *   DP.  M(0, x) = c(0, x); M(y, x) = c(y, x) + min M(y - 1, x') over x' in {x - 1, x, x + 1} within [0, w), ties preferring x, then x - 1, then x + 1.  The
 *     seam ends at the argmin of the last row, ties preferring the smallest |2 x - (w - 1)|, then the smaller x, and is traced back from there.  M < 2^23.
 *   Edit.  Only pixels of B change: on the first side the other view's mask is cleared, beyond the seam the first side's owner's.  Behind a pair no pixel of its
 *     overlap is set in both masks.
 * MS_ERR_INVALID, all checked on the host before the device is touched: as for ms_estimate_gains (n outside [1, MS_MAX_VIEWS], a null pointer, an empty ROI, an
 * image or mask of another type or size than its ROI, rows that are not contiguous), and an overlap with a side above MS_DP_MAX_SIDE, naming the pair. */
enum { MS_DP_MAX_SIDE = 4096 };
MS_API int ms_dp_seams(int n, const ms_rect *rois, const ms_image *images, ms_image *masks, ms_stream stream);

/* device::imgproc::buildWarp{Plane,Spherical,Cylindrical}Maps(tl_u, tl_v, map_x, map_y, k_rinv, r_kinv[, t], scale, stream)
 * OCV/stitching/src/warpers_cuda.cpp:51-67 -> cuda/build_warp_maps.cu:155-216.  k_rinv, r_kinv: 9 floats
 * (HOST), t: 3 floats (HOST, plane only, may be NULL). */
MS_API int ms_build_warp_maps(int projection, int tl_u, int tl_v, ms_image *map_x, ms_image *map_y,
                              const float *k_rinv, const float *r_kinv, const float *t, float scale,
                              ms_stream stream);

/* Lens distortion.  The warpers above assume an ideal pinhole (K * R^-1 alone); ms_lens puts a distortion model between R^-1 and K, so that a rig with calibrated
 * Brown-Conrady coefficients or fisheye lenses gets its maps, ROIs and seam-scale calibration from the library (ms_set_lens + ms_build_maps) instead of bringing
 * maps of its own (ms_set_maps).  For a ray (X, Y, Z) in camera coordinates (R^-1 times the warper's direction, R^-1 = R^T in double): rho = hypot(X, Y),
 * theta = atan2(rho, Z); the view does not see the ray when theta > max_theta -- its map entry is (-1, -1), the reference's own "behind the camera" marker
 * (stitching/src/cuda/build_warp_maps.cu:137-152).  Otherwise the distorted normalised coordinates (xd, yd) are
 *   MS_LENS_BROWN (cvProjectPoints2, calib3d/src/calibration.cpp:760-790): x = X / Z, y = Y / Z, r2 = x^2 + y^2,
 *       cdist = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3), xd = x cdist + 2 p1 x y + p2 (r2 + 2 x^2), yd = y cdist + p1 (r2 + 2 y^2) + 2 p2 x y;
 *   MS_LENS_FISHEYE (cv::fisheye::projectPoints, calib3d/src/fisheye.cpp:130-150): theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
 *       (xd, yd) = (X, Y) theta_d / rho, (0, 0) at rho = 0.  The atan2 form equals OpenCV's atan(r) for Z > 0 and goes on past 90 degrees;
 *   MS_LENS_NONE: xd = X / Z, yd = Y / Z, seen iff Z > 0;
 * and the pixel is (K[0] xd + K[1] yd + K[2], K[4] yd + K[5]).  Everything is evaluated in double -- from (double)u / (double)(float)scale with double sin / cos -- and
 * rounded to float once, at the store: calibration-time work, no fp32 evaluation order is part of the contract.  The inverse, pixel to ray, is ms_lens_unproject below. */
enum { MS_LENS_NONE = 0, MS_LENS_BROWN = 1, MS_LENS_FISHEYE = 2 };
typedef struct ms_lens {
    unsigned struct_size;   /* as ms_config: mismatch = MS_ERR_INVALID */
    int model;              /* MS_LENS_* */
    double k[8];            /* BROWN: OpenCV distCoeffs order k1 k2 p1 p2 k3 k4 k5 k6; FISHEYE: k1..k4, k[4..7] must be 0 */
    double max_theta_deg;   /* rays further than this from the optical axis are not seen.  BROWN: (0, 89]; FISHEYE: (0, 180]; 0 = default (BROWN 89, FISHEYE 180) */
} ms_lens;
/* Host only, no device needed.  MS_ERR_INVALID for: a null pointer, a struct_size mismatch, an unknown model, a non-finite coefficient, FISHEYE with non-zero k[4..7],
 * max_theta_deg outside its range, and a radial profile that is not strictly increasing on [0, max_theta] -- r cdist(r) over r in [0, tan max_theta] for BROWN,
 * theta_d(theta) for FISHEYE, sampled at 4096 uniform steps in double: a fold-back would put rays far outside the field of view back into the image (lower
 * max_theta_deg to the range the calibration holds on).  BROWN's tangential terms p1, p2 are NOT part of the check.  MS_LENS_NONE passes whatever k holds. */
MS_API int ms_lens_check(const ms_lens *lens);
/* The model above on the host, for callers and tests: K 9 floats, ray = (X, Y, Z) in camera coordinates, px = the pixel, or (-1, -1) with *seen = 0.
 * lens == NULL is MS_LENS_NONE; a lens ms_lens_check refuses is refused here. */
MS_API int ms_lens_project(const float *K, const ms_lens *lens, const double ray[3], double px[2], int *seen);
/* The inverse of the model: the source pixel -> the UNIT camera ray (cv::undistortPoints / cv::fisheye::undistortPoints, normalised), in double, one copy of the
 * arithmetic for this host call, ms_lens_unproject_points and the lens form of the rig refinement.  yd = (py - K[5]) / K[4], xd = (px - K[2] - K[1] yd) / K[0]; then
 *   MS_LENS_NONE: the ray is (xd, yd, 1) normalised; every finite pixel is seen;
 *   MS_LENS_FISHEYE: theta_d = hypot(xd, yd); not seen when theta_d > theta_d(max_theta).  theta solves theta_d(theta) = theta_d on [0, max_theta], where
 *       ms_lens_check found the profile increasing: a Newton iteration with the analytic slope from min(theta_d, max_theta), kept inside a bracket [lo, hi] (the
 *       bracket's midpoint where a step leaves it or the slope is not positive), until theta no longer changes, 60 rounds at most.  The ray is
 *       (sin theta xd / theta_d, sin theta yd / theta_d, cos theta), (0, 0, 1) at theta_d = 0; past 90 degrees it has Z < 0;
 *   MS_LENS_BROWN: (x, y) solves the full forward model, tangential terms included: a 2-D Newton iteration from (xd, yd) with the analytic 2 x 2 Jacobian, settled
 *       when max |step| <= 2^-50 max(1, |x|, |y|), 50 rounds at most (OpenCV's five fixed-point rounds are not accurate enough for a
 *       bundle adjustment; a zero step is not asked for, the last bit may alternate).  Not seen: the iteration does not settle, a Jacobian is singular, anything is
 *       not finite, hypot(x, y) > tan(max_theta).  The ray is (x, y, 1) normalised.
 * A pixel that is not finite is not seen.  Not seen: *seen = 0 and ray = (0, 0, 0).  The round trips ray -> ms_lens_project -> ms_lens_unproject and pixel ->
 * unproject -> project return to 1e-11 rad and 1e-9 pixels (tests/test_rig_lens_abi.py).  Host only, no device needed.  lens == NULL is MS_LENS_NONE.
 * MS_ERR_INVALID: a null pointer, a lens ms_lens_check refuses, a K entry that is not finite, K[0] or K[4] zero. */
MS_API int ms_lens_unproject(const float *K, const ms_lens *lens, const double px[2], double ray[3], int *seen);
/* ms_lens_unproject for n pixels on the device, one lane a point: a rig's keypoints (float pixel pairs, ORB's keypoint rows) become the unit rays
 * ms_refine_rig_rotations takes.  px_host: n x 2 floats, rays_host: n x 3 doubles, seen_host: n bytes, all HOST; a point the lens does not see gets the ray
 * (0, 0, 0) and the flag 0.  One upload, one launch, one copy back, one synchronise.  Host and device run the same code: rays differ by libm's sin / cos / hypot
 * and the last Newton round only (1e-12).  MS_ERR_INVALID as above, and for n outside [1, 2^20]. */
MS_API int ms_lens_unproject_points(const float *K, const ms_lens *lens, int n, const float *px_host, double *rays_host, unsigned char *seen_host, ms_stream stream);
/* ms_build_warp_maps for a camera with a lens (buildWarp{Spherical,Cylindrical}Maps, stitching/src/cuda/build_warp_maps.cu:155-216, with the distortion between
 * R^-1 and K, which is why K and R -- 9 floats each, HOST -- are passed separately).  map_x / map_y: 32FC1 of one size, any row step (pitched images, ROIs of
 * larger ones).  lens == NULL is MS_LENS_NONE.  MS_PROJ_PLANE is MS_ERR_UNSUPPORTED. */
MS_API int ms_build_warp_maps_lens(int projection, int tl_u, int tl_v, ms_image *map_x, ms_image *map_y, const float *K, const float *R, const ms_lens *lens,
                                   float scale, ms_stream stream);
/* RotationWarper::warpRoi (warpers_inl.hpp:136-146) for a camera with a lens, by forward evaluation on the device.  With s = (float)scale and U = llrint(pi s), the
 * candidates are the integer warper coordinates u in [-U, U) and v in [0, U) (spherical) or v in [-V, V], V = ceil(s tan MS_LENS_CYL_MAX_ELEVATION_DEG) (cylindrical:
 * the warper's v = tan(elevation) has no end, so views are cut at +-80 degrees).  A candidate is seen when its truncated float map coordinates lie in
 * [0, src_w) x [0, src_h) -- the rule of the warp masks (remap of a white image, NEAREST, BORDER_CONSTANT: calibration.cpp:224-227) -- and the ROI is the bounding box
 * of the seen candidates: every border row and column holds a seen pixel, a view that straddles +-pi or contains a pole comes out 2U wide (never wider than a canvas of
 * out_width = 2 pi scale; the window is half-open for that reason).  SYNCHRONOUS.  MS_ERR_INVALID: a null pointer, an empty source, scale outside (0, 8192], a lens
 * ms_lens_check refuses, no seen candidate ("sees nothing").  MS_PROJ_PLANE is MS_ERR_UNSUPPORTED. */
enum { MS_LENS_CYL_MAX_ELEVATION_DEG = 80 };
MS_API int ms_warp_roi_lens(int projection, const float *K, const float *R, const ms_lens *lens, float scale, int src_w, int src_h, ms_rect *roi, ms_stream stream);

/* cvtColor(src, dst, CV_YUV2BGR_NV12): the capture-side conversion the reference runs on the CPU per camera frame
 * (APP/networking.cpp:45-47, 1920x1620 NV12 -> 1920x1080 BGR, defs.h:10-17) -> YUV420sp2RGB888Invoker<0,0>
 * (OCV/imgproc/src/color.cpp).  src 8UC1 of (rows*3/2) x cols (Y plane, then interleaved UV); dst 8UC3, even size. */
MS_API int ms_nv12_to_bgr(const ms_image *src, ms_image *dst, ms_stream stream);
/* The same for n cameras of one geometry in ONE launch (the capture threads convert per camera, networking.cpp:45-47).  Bit-identical to n single calls. */
MS_API int ms_nv12_to_bgr_batch(const ms_image *src, ms_image *dst, int n, ms_stream stream);

/* cvtColor(src, dst, COLOR_BGR2YUV_I420): the encoder input of consume() (APP/timed.cpp:308-316) ->
 * RGB888toYUV420pInvoker (OCV/imgproc/src/color.cpp:9082-9160).  src 8UC3 with even width/height; dst contiguous
 * 8UC1 of (rows*3/2) x cols = planar I420.  Also what bench.py gathers across GPUs (half the bytes of BGR). */
MS_API int ms_bgr_to_i420(const ms_image *src, ms_image *dst, ms_stream stream);
/* consume()'s pixel work on the device, in ONE pass (APP/timed.cpp:251-316): the 8U panorama resized (INTER_LINEAR) to out_width x image_height --
 * image_height = (int)(out_width / cols * rows + 0.5) capped at out_height when keep_aspect_ratio (timed.cpp:256-271), else out_height --, placed in the middle of a
 * black out_width x out_height frame (from row out_height / 2 - image_height / 2, timed.cpp:283-289) and converted to the encoder's planar I420
 * (timed.cpp:308-316; the two BGR2RGB swaps before it cancel).  The reference resizes on the CPU (cv::resize's fixed-point arithmetic); this is
 * cuda::resize's (the arithmetic of ms_resize_linear), i.e. what moving the step to the GPU with the reference's own library gives: <= 1 LSB apart.
 * Equal, bit for bit, to ms_resize_linear + copy into a black frame + ms_bgr_to_i420.  dst: DEVICE 8UC1 contiguous (out_height * 3 / 2) x out_width;
 * image_height (may be NULL) receives the height used. */
MS_API int ms_consume_i420(const ms_image *pano8u, ms_image *dst, int out_width, int out_height, int keep_aspect_ratio, int *image_height, ms_stream stream);
/* cuda::cvtColor(gpu_img, gpu_img, CV_BGR2GRAY) of featurefinder::findFeatures (APP/featurefinder.cpp:34) -> RGB2GrayConvert
 * (OCV/core/include/opencv2/core/cuda/detail/color_detail.hpp:97-101, :444-447): (b * 1868 + g * 9617 + r * 4899 + 2^13) >> 14. */
MS_API int ms_bgr_to_gray(const ms_image *src, ms_image *dst, ms_stream stream);
/* The same conversion for n frames of one geometry (same size and step) in one launch: the egress of a batch of panoramas. */
MS_API int ms_bgr_to_i420_batch(const ms_image *src, ms_image *dst, int n, ms_stream stream);

/* custom_resize(GpuMat &in, GpuMat &out, Size t_size)  APP/resize.cu:30-45, APP/calibration.h:15.
 * out->rows/cols give t_size.  32FC1. */
MS_API int ms_custom_resize_32f(const ms_image *in, ms_image *out, ms_stream stream);

/* =============================================================================================
 * 2. Host geometry (integer/fp32 host code in the reference too)
 * ============================================================================================= */

/* RotationWarper::warpRoi(src_size, K, R)  OCV/stitching/include/opencv2/stitching/detail/warpers_inl.hpp:136-146
 * incl. the per-warper detectResultRoi (warpers.cpp:277-318, warpers.hpp:287-290).  K, R: 9 floats row-major. */
MS_API int ms_warp_roi(int projection, const float *K, const float *R, float scale, int src_w, int src_h,
                       ms_rect *roi);
/* detail::resultRoi(corners, sizes)  OCV/stitching/src/util.cpp:125-138 */
MS_API int ms_result_roi(int n, const ms_rect *view_rois, ms_rect *roi);

/* calibrateCameras + the scale bookkeeping of stitch_calib / warpImages (APP/calibration.cpp:28-68, :101-116, :147-181, :269-288; defs.h:51-53):
 * the fixed rig model -- view i rotated by 2 pi i / N about +y, principal point at the image centre, focal = ppx / tan(hfov / 2), aspect 1 --
 * and every scale the calibration derives from the three megapixel budgets.  Host arithmetic in the reference's types (double scales,
 * float rotation angle, K().convertTo(CV_32F)). */
#define MS_MAX_VIEWS 16
typedef struct ms_rig_params {
    int num_views;                 /* NUM_IMAGES (defs.h:37) */
    int src_width, src_height;     /* full_img_size */
    double hfov_deg;               /* 90 in the reference (calibration.cpp:31) */
    double work_megapix;           /* WORK_MEGAPIX 0.6; negative = original size (defs.h:51, calibration.cpp:269-277) */
    double seam_megapix;           /* SEAM_MEAGPIX 0.01 (defs.h:52, calibration.cpp:280) */
    double compose_megapix;        /* COMPOSE_MEGAPIX 1.4; not positive = compose at the original resolution (defs.h:53, calibration.cpp:147-150) */
} ms_rig_params;
typedef struct ms_rig {
    double work_scale, seam_scale, seam_work_aspect, compose_scale, compose_work_aspect;
    float warped_image_scale;      /* static_cast<float>(cameras[0].focal) at work scale (calibration.cpp:288) */
    float seam_warp_scale;         /* static_cast<float>(warped_image_scale * seam_work_aspect): the seam-scale warper (:101) */
    float compose_warp_scale;      /* warped_image_scale * static_cast<float>(compose_work_aspect): the compose warper (:156) = ms_config.warp_scale */
    int resize_input;              /* |compose_scale - 1| > 0.1: every frame goes through cuda::resize before the remap (timed.cpp:75, calibration.cpp:161) */
    int compose_width, compose_height;   /* cvRound(full * compose_scale) if resize_input, else the full size (:163-164) = ms_config.src_width / height */
    float K_compose[MS_MAX_VIEWS][9];    /* cameras[i].K() after *= compose_work_aspect, as CV_32F (:171-176) -> ms_set_camera */
    float K_seam[MS_MAX_VIEWS][9];       /* K at work scale as CV_32F, four entries times (float)seam_work_aspect (:108-116) -> ms_calibrate_seam */
    float R[MS_MAX_VIEWS][9];            /* Rz * Ry * Rx with only Ry non-trivial (:36-55) */
} ms_rig;
MS_API int ms_calibrate_cameras(const ms_rig_params *params, ms_rig *rig);
/* blend_width = sqrt(area(resultRoi)) * BLEND_STRENGTH / 100 and mb->setNumBands(ceil(log2(blend_width)) - 1) (calibration.cpp:183-194, defs.h:55);
 * num_bands = 0 where the reference falls back to Blender::NO (blend_width < 1). */
MS_API int ms_num_bands_rule(int pano_width, int pano_height, float blend_strength, float *blend_width, int *num_bands);

/* =============================================================================================
 * 3. The compositor context: calibration tables once, then one fused launch sequence per frame
 * ============================================================================================= */

typedef struct ms_ctx ms_ctx;

typedef struct ms_config {
    unsigned struct_size;   /* sizeof(ms_config) of the caller's header: ms_create rejects a mismatch (ABI guard)  */
    int num_views;          /* NUM_IMAGES (APP/defs.h:37)                                             */
    int src_width, src_height;   /* camera frame size (after the optional compose_scale resize)       */
    int projection;         /* MS_PROJ_*: the app ships cylindrical (APP/calibration.cpp:100,156)     */
    float warp_scale;       /* warper scale = warped_image_scale * compose_work_aspect (calibration.cpp:156) */
    int num_bands;          /* MultiBandBlender num_bands (blenders.hpp:129 default 5; calibration.cpp:193) */
    int enable_cpw;         /* enable_local (APP/defs.h:27): second remap through the mesh maps       */
    int out_width, out_height;   /* equirect canvas (0,0 = emit the pano ROI only)                     */
    int max_frames;         /* frames batched per ms_stitch call (1 = live; >1 amortises launches; <= 64) */
    int view_shards;        /* 0 / 1 = this context composites whole frames; S = 2..4: it owns one shard of the views (ms_stitch_partial) */
    int view_shard_index;   /* which shard, 0 .. S-1                                                   */
    int cpu_flavour_remap;  /* != 0: the projection warp uses cv::remap's CPU arithmetic (1/32-px coordinates, 15-bit weights): the
                             * reference's CPU pipeline of BASELINE configs[0]; needs debug_simple_kernels and no CPW; changes results BY DESIGN */
    /* developer knobs: none of them changes a result */
    int debug_simple_kernels;    /* != 0: the one-pixel-per-lane reference kernels instead of the tiled ones      */
    int warp_lds_stage;          /* 0: direct tap gathers (default); 1: source tiles staged in LDS by LDS-DMA (k_warp_a, measured slower on config 2); 2: never stage */
    int raster_tile_order;       /* != 0: work lists in raster order instead of the XCD-aware order               */
    /* Pano-column sharding (the alternative to view sharding): S = 2..16 contexts -- one per GPU -- each composite the columns
     * [ms_get_col_window) of the panorama ROI, bit-identical there to an unsharded context.  The work lists are cut down to what those columns depend on
     * (their own pixels plus <= 3 * 2^num_bands columns of halo on either side, recomputed); views that do not reach the window are never read
     * (their ms_image may be all-zero).  Output pixels outside the window are unspecified.  0 / 1 = the whole panorama. */
    int col_shards;
    int col_shard_index;         /* which shard, 0 .. S-1 */
    /* > 0 (with enable_cpw): ms_update_mask only ENQUEUES work -- the blend tables are double-buffered and the work lists are planned for masks
     * whose edges move by up to this many pixels, so a re-warped mask needs no new plan.  An update whose mesh displaces further than the margin
     * (ms_get_mesh_displacement) leaves the tables as they are.  0: ms_update_mask rebuilds tables and work lists synchronously (calibration-time call). */
    int update_mask_margin;
    int self_check;              /* 1: ms_init_blender verifies the shared-reciprocal division of the band kernels against IEEE division over every
                                  * denominator of this context's tables (a few ms; the test suite sets it); 0: no check (was reserved[0], must be 0 or 1) */
} ms_config;

MS_API int ms_create(const ms_config *cfg, ms_ctx **out);
MS_API void ms_destroy(ms_ctx *ctx);

/* cameras[i].K() / cameras[i].R as fp32 row-major 3x3 (APP/calibration.cpp:28-68,217-221) */
MS_API int ms_set_camera(ms_ctx *ctx, int view, const float *K, const float *R);
/* The view's lens (ms_lens above; cvProjectPoints2's distCoeffs / cv::fisheye::projectPoints' D beside cameras[i].K()): copied.  NULL or MS_LENS_NONE clears it.
 * Like ms_set_camera it invalidates maps, masks and blender.  A context on which no view has a lens is bit for bit what it is without this call.  With a lens on
 * at least one view, ms_build_maps sends EVERY view down the dense route (views without a lens as MS_LENS_NONE, in the same double arithmetic): ROIs from
 * ms_warp_roi_lens' rule, maps from ms_build_warp_maps_lens' kernel into the storage ms_set_maps fills, no 1-D projection tables, the per-frame kernels of
 * ms_set_maps, and its limits -- a view of at least MS_MAPS_MIN_WIDTH x MS_MAPS_MIN_HEIGHT with no side above MS_MAPS_MAX_SIDE, a padded panorama of at most 32767
 * a side: MS_ERR_INVALID naming the view.  ms_get_map_source reports MS_MAPS_LENS.  Everything that reads maps, ROIs and masks works unchanged (every ms_stitch* form,
 * CPW, ms_update_mask, ms_set_active_views, exposure tracking, column and view shards -- every shard is given the same cameras and lenses --, the developer knobs),
 * and so does ms_calibrate_seam: distortion acts on normalised coordinates, so the same ms_lens serves at seam scale with K_seam.  Stated limits: MS_PROJ_PLANE
 * contexts refuse a lens and ms_save_tables refuses a lens context (the blob format has no lens record), both MS_ERR_UNSUPPORTED.
 * MS_ERR_INVALID: a bad view index, a lens ms_lens_check refuses (ms_get_lens: a null pointer). */
MS_API int ms_set_lens(ms_ctx *ctx, int view, const ms_lens *lens);
MS_API int ms_get_lens(const ms_ctx *ctx, int view, ms_lens *lens);
/* GainCompensator::gains()[view]  (exposure_compensate.cpp:164-170, APP/timed.cpp:94) */
MS_API int ms_set_gain(ms_ctx *ctx, int view, double gain);

/* warper->warpRoi + gpu_warper->buildMaps per view (APP/calibration.cpp:168-181,221) and
 * blender->prepare(corners, sizes) (calibration.cpp:196 -> blenders.cpp:82-85,237-295). */
MS_API int ms_build_maps(ms_ctx *ctx, ms_stream stream);
/* stitch_online's x_maps[i] / y_maps[i] as the caller's own (APP/timed.cpp:56, :84-90, :123-129) instead of gpu_warper->buildMaps' (calibration.cpp:221):
 * the per-frame path of the reference remaps through whatever maps it is handed, so a rig with calibrated lens distortion, a fisheye model or any third-party
 * calibration brings its own.  Replaces ms_build_maps and needs no ms_set_camera.
 *   rois:  HOST, num_views rectangles: corner and size of each warped view in warper coordinates (what ms_view_geom.roi reports and blender->prepare(corners,
 *          sizes) receives).
 *   xmaps[i] / ymaps[i]: DEVICE 32FC1, exactly rois[i].width x rois[i].height; row step >= 4 * width and a multiple of 4, data 4-byte aligned.  The values are
 *          cuda::remap's backward map -- source pixel coordinates -- and may be anything: outside the source, negative, NaN, +-inf (such pixels sample
 *          BORDER_CONSTANT 0 like the reference's remap).
 * The maps are COPIED into context storage (the caller may free or overwrite them when the call returns); resultRoi / prepare / the per-view padding and the
 * canvas placement are those of ms_build_maps.  SYNCHRONOUS, calibration-time: drains `stream`, marks the maps built and invalidates masks and blender, so
 * ms_build_masks or ms_set_mask, ms_set_gain and ms_init_blender / ms_init_feather follow as usual; not callable while another thread stitches.  Everything that
 * depends on maps, ROIs and masks only works unchanged (every ms_stitch* form, CPW, ms_set_active_views, exposure tracking, column and view shards -- every shard
 * is given the same maps --, the developer knobs; warp_lds_stage = 1 never stages).  What needs cameras is refused with MS_ERR_UNSUPPORTED: ms_calibrate_seam
 * (it re-warps at seam scale) and ms_save_tables (the blob replays cameras).  A later ms_build_maps returns the context to the analytic maps (with ms_set_lens: the lens maps).
 * ms_get_maps returns the stored copies, ms_get_view_geom / ms_get_pano_geom the geometry derived from `rois`.
 * MS_ERR_INVALID, before the device is touched: a null pointer; an image of another type or size than its ROI; a bad step or alignment; a ROI narrower than
 * MS_MAPS_MIN_WIDTH, lower than MS_MAPS_MIN_HEIGHT or with a side above MS_MAPS_MAX_SIDE; a padded panorama (the ROIs' union) with a side above 32767.
 *   MS_MAPS_MIN_WIDTH / _HEIGHT: the tiled kernels fetch a bilinear tap row as 8 bytes = 3 pixels clamped into the image and two rows at once; with CPW the
 *          image sampled is the warped view itself, so a view has at least 3 columns and 2 rows (narrower contexts would fall back to the reference kernels).
 *   MS_MAPS_MAX_SIDE: a work-list tile keeps its origin inside the PADDED view in 16 bits (<= 32767); the padding adds less than 8 * 2^num_bands <= 1024
 *          columns / rows (num_bands <= 7: a gap of 3 * 2^num_bands either side, rounded out to multiples of 2^num_bands), hence 32768 - 1024. */
enum { MS_MAPS_MIN_WIDTH = 3, MS_MAPS_MIN_HEIGHT = 2, MS_MAPS_MAX_SIDE = 31744 };
MS_API int ms_set_maps(ms_ctx *ctx, const ms_rect *rois, const ms_image *xmaps, const ms_image *ymaps, ms_stream stream);
/* where the context's maps come from: ms_build_maps (ANALYTIC, also before any maps are built; LENS when a view had a lens, ms_set_lens) or ms_set_maps (CUSTOM) */
enum { MS_MAPS_ANALYTIC = 0, MS_MAPS_CUSTOM = 1, MS_MAPS_LENS = MS_MAPS_CUSTOM + 1 /* 2 */ };
MS_API int ms_get_map_source(const ms_ctx *ctx, int *source);

/* Compose-size blend masks (APP/calibration.cpp:224-237).  mode 0: warp(255, NEAREST) only;
 * mode 1: AND with Voronoi seams (VoronoiSeamFinder, seam_finders.cpp:85-160) computed at compose size
 * (the app computes them at seam scale and resizes up: stated simplification).
 * The call has no images: mode 1 is Voronoi whatever ms_set_seam_finder says. */
MS_API int ms_build_masks(ms_ctx *ctx, int mode, ms_stream stream);
/* Which seam finder ms_calibrate_seam cuts with (seam_finder->find, calibration.cpp:134-135): MS_SEAM_VORONOI, ms_voronoi_seams' (the default: a context that
 * never calls the setter behaves bit for bit as before), or MS_SEAM_DP, ms_dp_seams' on the warped seam-scale images.  Calibration state like the masks it
 * shapes: ms_save_tables does not store it, ms_create and ms_load_tables contexts start at Voronoi.  MS_ERR_INVALID: a null pointer, another value. */
enum { MS_SEAM_VORONOI = 0, MS_SEAM_DP = 1 };
MS_API int ms_set_seam_finder(ms_ctx *ctx, int finder);
MS_API int ms_get_seam_finder(const ms_ctx *ctx, int *finder);
/* The reference's own calibration at seam scale (APP/calibration.cpp:92-135, 224-237): resize the N full frames (DEVICE 8UC3) by
 * seam_scale, warp image (LINEAR/REFLECT) and a 255-mask (NEAREST/CONSTANT) with the per-view seam intrinsics K_seam (HOST, N x 9,
 * = K at work scale times seam_work_aspect, calibration.cpp:110-116) and seam_warp_scale, estimate the exposure gains
 * (GainCompensator::feed, exposure_compensate.cpp:71-145), cut Voronoi seams (or ms_dp_seams': ms_set_seam_finder), optionally dilate, resize the seam masks to the compose
 * mask size and AND them with warp(255) at compose scale.  Leaves the masks ready for ms_init_blender; gains_out (HOST, N) may be NULL.
 * The full frames may be larger than the context's source size (compose_scale < 1: the context composites the resized frames, the seam
 * images are still cut from the full ones, calibration.cpp:95); all N must have one size. */
typedef struct ms_seam_params {
    double seam_scale;        /* min(1, sqrt(SEAM_MEGAPIX*1e6 / area))  (calibration.cpp:280)            */
    float seam_warp_scale;    /* warped_image_scale * seam_work_aspect  (calibration.cpp:101)             */
    int dilate;               /* enable_local: 3x3 dilation of the seam masks (calibration.cpp:209,231)   */
    int estimate_gains;       /* also ms_set_gain() the estimated gains                                   */
} ms_seam_params;
MS_API int ms_calibrate_seam(ms_ctx *ctx, const ms_image *full_imgs, const float *K_seam, const ms_seam_params *params,
                             double *gains_out, ms_stream stream);
/* Or hand a mask over, as init_gpu(img, mask, tl) receives it (blenders.cpp:344): HOST 8UC1, view-ROI sized. */
MS_API int ms_set_mask(ms_ctx *ctx, int view, const uint8_t *mask_host, size_t step);
/* mb->init_gpu(_, mask, corner) for every view, in view order (calibration.cpp:240 -> blenders.cpp:344-461),
 * plus the frame-invariant weight sums the reference re-accumulates every frame (blenders.cpp:736, :775). */
MS_API int ms_init_blender(ms_ctx *ctx, ms_stream stream);
/* FeatherBlender (detail::FeatherBlender, blenders.cpp:139-186; the CPU blender of the reference's 2-view example): same call order as
 * ms_init_blender on a context created with num_bands = 0.  Weight maps are createWeightMap(mask, sharpness) (blenders.cpp:944-951:
 * L1 distance transform * sharpness, truncated at 1; OpenCV's default sharpness is 0.02) instead of mask/255; ms_stitch then runs
 * feed x N + blend as one single-band pass. */
MS_API int ms_init_feather(ms_ctx *ctx, float sharpness, ms_stream stream);
/* MeshWarper::interpolateMesh (meshwarper.cpp:337-354) followed by convertMeshesToMap: mesh = start + (end - start) * progress (fp32), the
 * RECALIB_INTERP branch of the recalibration thread (timed.cpp:449-457).  HOST vertex meshes, same conventions as ms_set_mesh. */
MS_API int ms_set_mesh_interp(ms_ctx *ctx, int view, const float *start_x, const float *start_y, const float *end_x, const float *end_y,
                              int N, int M, float progress, ms_stream stream);
/* Largest |x_mesh - x| / |y_mesh - y| (pixels) of the active CPW mesh of `view`, measured on the device by ms_set_mesh / ms_set_mesh_maps.
 * While it stays <= 32 the first CPW remap (timed.cpp:90-94) skips the tiles the mesh remap cannot reach; larger meshes warp whole views. */
MS_API int ms_get_mesh_displacement(ms_ctx *ctx, int view, float *out_px);
/* MultiBandBlender::update_mask (blenders.cpp:297-315; its call is commented out in the reference's main loop, timed.cpp:598-605):
 * the mask init_gpu received for `view`, remapped through the view's active CPW mesh (INTER_LINEAR, BORDER_CONSTANT 0), replaces the view's
 * blend-weight pyramid.  Needs enable_cpw, ms_init_blender and a mesh for the view.  The reference re-accumulates the weight sums each frame;
 * here they are frame-invariant tables, so the call rebuilds them (and the work lists) as ms_init_blender does, keeping meshes and gains.
 * With ms_config.update_mask_margin > 0 the call is asynchronous like ms_set_mesh: it enqueues the re-warp, the view's weight pyramid, the weight
 * sums, the result mask and the owner maps into the inactive copy of the tables on `stream` and swaps; the next ms_stitch waits for it on the GPU.
 * Safe from the recalibration thread while another thread stitches (timed.cpp:598-605 calls it right after the mesh swap).
 * ms_get_mask keeps returning the original mask; ms_set_mask / ms_build_masks / ms_calibrate_seam drop the re-warped one.
 * MS_ERR_STATE while views are left out (ms_set_active_views): make every view active first. */
MS_API int ms_update_mask(ms_ctx *ctx, int view, ms_stream stream);

/* Camera dropout.  Bit v set = view v is composited.  The views left out are treated exactly as MultiBandBlender treats a view whose feed_online
 * was not called for the frame (blenders.cpp:700-749, 758-832): they add nothing to the band sums or the weight sums; pixels covered only by them
 * come out 0 with result mask 0.  Panorama ROI, canvas placement and output sizes do not change.
 *   - Takes effect at the next ms_stitch / ms_stitch_nv12 / ms_stitch_i420 / ms_stitch_nv12_i420 / ms_blend issued after the call returns, for every frame of that call.
 *     The set is per call, not per frame: a caller that sees a camera drop out in the middle of a batch splits the batch there.
 *   - Enqueue-only: the table rebuild runs on `stream`, and the next stitch waits for it on the GPU.  The call never waits for GPU work; it waits
 *     only for a stitch being enqueued on another thread, or a table rebuild (ms_init_blender, synchronous ms_update_mask), to finish.  Safe from
 *     another thread while one thread stitches (same contract as ms_set_mesh).
 *   - The views left out are never read: their ms_image may be all-zero.  ms_blend needs only the active views fed (feeds of the others are ignored),
 *     ms_get_needed_views returns needed & active, ms_get_result_mask the active set's mask.
 *   - All views = the original tables again (bit-identical, no rebuild).  The full-set tables are never overwritten.  ms_init_blender, ms_load_tables
 *     and everything else that rebuilds the tables start with all views active; ms_save_tables saves the full-set tables (the set is run-time state).
 *     ms_set_mesh* and ms_set_gain stay allowed for every view: a mesh set on an inactive view is used once it is active again, and a gain applies to
 *     the full set and to every cached subset.
 *   - A subset's tables (made on the device: weight sums, result mask and owner maps of the active views, work lists without the others) are cached
 *     for the last num_views + 1 subsets, so a camera that goes away and comes back costs a pointer swap after the first time.  Memory per cached set:
 *     4 bytes per pixel of every pano level (the weight sums: about 5.3 bytes per pano-ROI pixel), 1 byte per pano-ROI pixel
 *     (the result mask), 1 byte per 64 x 16 cell per band (owner maps), the work lists (24 bytes per warp tile, 8 per pyramid / band tile), plus once per
 *     context zeros as large as the largest view's level-0 weights.
 * MS_ERR_INVALID: mask 0 or a bit >= num_views.  MS_ERR_STATE: before ms_init_blender.  MS_ERR_UNSUPPORTED: view-sharded contexts and FeatherBlender
 * contexts (ms_init_feather).  Column-sharded contexts are supported. */
MS_API int ms_set_active_views(ms_ctx *ctx, unsigned mask, ms_stream stream);
MS_API int ms_get_active_views(const ms_ctx *ctx, unsigned *mask);

/* Exposure tracking.  The reference estimates the gains once, at calibration, from seam-scale images (GainCompensator::feed,
 * stitching/src/exposure_compensate.cpp:71-145, called from APP/calibration.cpp:131-132) and keeps them; its once-a-second recalibration touches the
 * meshes only.  Cameras with auto-exposure drift apart within seconds.  ms_track_gains re-estimates the gains from one set of LIVE source frames at compose
 * scale, on the caller's stream: overlap statistics -> normal equations -> solve -> smoothing -> the device view tables, with no host wait, so that the next
 * ms_stitch* on that stream uses the new gains.
 *   views: num_views DEVICE 8UC3 images of the context's source size, ONE frame (of a batched call normally the last time step).  Views outside the active
 *     set (ms_set_active_views) are never read.
 *   The statistic.  T = dst_roi_final (ms_get_pano_geom), roi_v = the warped ROI of view v, (mx_v, my_v) the maps of ms_get_maps.  A pano pixel (u, v) in
 *     warper coordinates is a sample iff (u - T.x) % stride == 0 && (v - T.y) % stride == 0.  View a sees a sample iff it lies in roi_a and the truncated map
 *     coordinate hits the source -- the warp mask BEFORE seam cutting, as GainCompensator gets it (calibration.cpp:118-132); the blend masks (ms_get_mask) are
 *     not used.  Its value there is q_a = llrint(sqrt((double)(b*b + g*g + r*r)) * 2^20) of the source pixel at the truncated coordinate: nearest sampling, and
 *     the CPW mesh is ignored (exposure does not depend on a few pixels of displacement).  For every ordered pair of ACTIVE views whose ROIs intersect as plain
 *     rectangles (i == j included, exposure_compensate.cpp:90; no wrap across +-pi, as in the reference): cnt = #samples both see, N[i][j] = N[j][i] =
 *     max(1, cnt), S[i][j] = sum of q_i, S[j][i] = sum of q_j over them; every other entry 0.  I[i][j] = S[i][j] / 2^20 / N[i][j].  The sums are integers:
 *     independent of the order of the reduction, hence bit-reproducible, and within 2^-21 per pixel of the reference's double sum (:103-117).
 *   Solve / smooth / publish.  The normal equations and cv::solve of exposure_compensate.cpp:123-139 (alpha 0.01, beta 100) over the active views; an inactive
 *     view keeps its gain.  g <- g + smoothing * (g_estimated - g) in double; the state starts from ms_set_gain's values, and ms_set_gain after tracking
 *     overrides it for its view.  A singular system changes nothing and is counted.  The float gain is written into every view table a later stitch may read
 *     (the full set, its enqueue-only-mask-update copy, every cached subset); ms_init_blender, ms_update_mask, ms_set_active_views and ms_save_tables all
 *     see the tracked values: no path brings an older gain back.
 *   ms_track_gains is enqueue-only (no allocation, no copy to the host, no wait for the GPU) and callable while another thread stitches (contract of
 *     ms_set_active_views).  ms_gain_stats is the statistics alone, blocking, for tests and diagnostics: N and S (num_views x num_views long long each) to the
 *     HOST.  ms_get_gains waits for `stream` and returns the gains the next stitch on it will use (num_views doubles) and the solve counters (may be NULL).
 *     Ordering against stitches on ANOTHER stream: the kernel that publishes the gains runs behind the last ms_stitch* enqueued on the context, and the next
 *     ms_stitch* waits for it, so every frame is composited with the gains before or after an update, never a mix of the two; the statistics kernel still overlaps
 *     the stitch, the publication does not.  On one stream nothing is added.
 *   ms_gain_track_default_params: stride 4, smoothing 0.25 -- starting values, not tuned on a rig.
 *   NV12 sources (the cameras' format, defs.h:10-17; ms_stitch_nv12 callers).  ms_gain_stats_nv12 / ms_track_gains_nv12 are the same statistic, solve, smoothing
 *     and publication with the pixel read from the planes: views_nv12 = num_views DEVICE 8UC1 images of (src_height * 3 / 2) x src_width, ONE frame.  For the
 *     truncated source coordinate (xx, yy): Y = plane[yy][xx], (U, V) = plane[src_height + yy / 2][xx & ~1, (xx & ~1) + 1], converted to b, g, r with cvtColor's
 *     integer formula (the capture threads' cvtColor(COLOR_YUV2BGR_NV12), networking.cpp:45-47), then q as above.  N and S equal, integer for integer,
 *     ms_gain_stats on the ms_nv12_to_bgr_batch copies of the same frames, so every guarantee above holds (enqueue-only, no allocation, callable while another
 *     thread stitches, inactive views never read, no path brings an older gain back); both forms share the context's accumulators and gain state and may alternate.
 *     They read the maps only: they also work where ms_stitch_nv12 is refused (debug_simple_kernels).  MS_ERR_INVALID also for an odd source size.
 * MS_ERR_INVALID: null context / params / views, struct_size mismatch, stride < 1, smoothing outside (0, 1], an image of the wrong size or type.
 * MS_ERR_STATE: before ms_init_blender.  MS_ERR_UNSUPPORTED: view-sharded and column-sharded contexts (a shard does not hold every overlap: column shards
 * track with ms_gain_stats_partial / ms_track_gains_from_partials below, view shards with ms_gain_samples / ms_track_gains_from_samples further below, ranks
 * with ms_dist_track_gains / ms_dist_track_gains_views) and FeatherBlender contexts (ms_init_feather). */
typedef struct ms_gain_track_params {
    unsigned struct_size;   /* sizeof of the caller's struct; mismatch = MS_ERR_INVALID (as ms_config)                   */
    int stride;             /* >= 1: every stride-th pano column and row is sampled                                      */
    double smoothing;       /* lambda in (0, 1]: g <- g + lambda * (g_estimated - g); 1 = take the estimate              */
} ms_gain_track_params;
MS_API int ms_gain_track_default_params(ms_gain_track_params *prm);
MS_API int ms_gain_stats(ms_ctx *ctx, const ms_image *views, int stride, long long *N_host, long long *S_host, ms_stream stream);
MS_API int ms_track_gains(ms_ctx *ctx, const ms_image *views, const ms_gain_track_params *prm, ms_stream stream);
MS_API int ms_gain_stats_nv12(ms_ctx *ctx, const ms_image *views_nv12, int stride, long long *N_host, long long *S_host, ms_stream stream);
MS_API int ms_track_gains_nv12(ms_ctx *ctx, const ms_image *views_nv12, const ms_gain_track_params *prm, ms_stream stream);
MS_API int ms_get_gains(ms_ctx *ctx, double *gains_host, int *solves_ok, int *solves_singular, ms_stream stream);

/* Exposure tracking on column shards (extends ms_track_gains / ms_gain_stats above to ms_config.col_shards > 1; allowed on unsharded contexts too).  The statistic
 * is a set of integer sums, and the column windows (ms_get_col_window) partition the ROI columns: a pano pixel (u, v) is a sample of shard k iff it is a sample as
 * defined above and col_begin <= u - T.x < col_end.  Every sample belongs to exactly one shard, so the shards' raw sums add up, integer for integer, to the
 * unsharded cnt and S; every shard then runs the same deterministic solve on the same integers and reaches bit-identical gains, with no host in the loop and no
 * gain ever exchanged.  On a context without column shards the window is the whole ROI.
 *   A partial: ms_gain_partial_bytes(ctx) bytes of caller-owned DEVICE memory, 8-byte aligned (valid after ms_create: it depends on num_views only; 0 for a null
 *     context).  Eight 32-bit words -- magic, num_views, the active-view mask, stride, T.x, T.y, T.width, T.height -- then cnt[i][j] (symmetric) and S[i][j],
 *     num_views x num_views unsigned 64-bit each: the raw accumulators, BEFORE the max(1, cnt) rule.  The size is the caller's responsibility: only the header
 *     is checked, a shorter buffer is read or written past its end.
 *   ms_gain_stats_partial / ms_gain_stats_partial_nv12 write this context's partial from one frame set on `stream` (the kernel of ms_track_gains over the window's
 *     lattice columns, then one small launch that stores header and sums).  ms_track_gains_from_partials takes n_partials (1 .. 16) DEVICE pointers in a HOST array
 *     -- normally one per shard of the group, in the same order on every shard -- and on `stream`: checks that every header equals what this context and this call
 *     expect (magic, num_views, active set, prm->stride, T), adds the integers partial by partial, then does exactly what ms_track_gains does behind its
 *     statistics: N = max(1, cnt) on the pairs whose ROIs meet, I, the solve over the active views, smoothing in double, publication into every view table a
 *     stitch may read.  On a header mismatch nothing changes and one rejected update is counted (ms_get_gain_track_counters); no error surfaces later.
 *     ms_gain_stats_partial + ms_track_gains_from_partials of that one partial on an unsharded context == ms_track_gains, bit for bit.
 *   Both are enqueue-only (no allocation, no copy to the host, no wait for the GPU) and callable while another thread stitches: the contract of ms_track_gains.
 *     They share the context's accumulators and gain state with ms_track_gains / ms_gain_stats, and every "no older gain comes back" guarantee above holds.
 *     The caller orders the partials' producers before ms_track_gains_from_partials (same stream, or an event); partials that arrive from other GPUs are moved
 *     by the caller (ms_dist_track_gains does it for a column group).
 *   ms_get_gain_views: the views the caller uploads for a time step it tracks on.  Bit v set = view v is active and either its warped ROI meets the window's
 *     columns (these, and no others, are read by ms_gain_stats_partial) or ms_stitch reads it (ms_get_needed_views).  The first set is defined on the warp ROI
 *     BEFORE seam cutting, so it holds views ms_get_needed_views lacks; the second holds views whose ROI ends just outside the window but whose blend weights
 *     reach into the pyramid halo of the window.  The union is what a step that is both stitched and tracked needs.  Views outside the mask are never read by
 *     ms_gain_stats_partial: their ms_image may be all-zero.
 *   ms_get_gain_track_counters waits for `stream` (as ms_get_gains): updates solved, singular systems, rejected updates since ms_create.
 * View shards stay out of THESE calls: a pair statistic needs both views' pixels at the same sample, and a view shard holds only its own views' pixels.  They
 * track through per-view sample vectors: "Exposure tracking on view shards" below.
 * MS_ERR_INVALID: null context / params / views / partial(s), a partial not 8-byte aligned, n_partials outside [1, 16], struct_size mismatch, stride < 1,
 * smoothing outside (0, 1], an image of the wrong size or type (views the statistic reads only).  MS_ERR_STATE: before ms_init_blender.  MS_ERR_UNSUPPORTED:
 * view-sharded contexts (they have ms_gain_samples / ms_track_gains_from_samples) and FeatherBlender contexts. */
typedef struct ms_gain_track_counters {
    unsigned struct_size;   /* sizeof of the caller's struct, set by the caller; mismatch = MS_ERR_INVALID                */
    int solves_ok;          /* updates that solved and published (ms_track_gains* and ms_track_gains_from_partials)      */
    int solves_singular;    /* singular systems: nothing changed                                                         */
    int updates_rejected;   /* ms_track_gains_from_partials / _from_samples calls whose buffers did not agree: nothing changed */
} ms_gain_track_counters;
MS_API size_t ms_gain_partial_bytes(const ms_ctx *ctx);
MS_API int ms_get_gain_views(const ms_ctx *ctx, unsigned *mask);
MS_API int ms_gain_stats_partial(ms_ctx *ctx, const ms_image *views, int stride, void *partial_dev, ms_stream stream);
MS_API int ms_gain_stats_partial_nv12(ms_ctx *ctx, const ms_image *views_nv12, int stride, void *partial_dev, ms_stream stream);
MS_API int ms_track_gains_from_partials(ms_ctx *ctx, const void *const *partials_dev, int n_partials, const ms_gain_track_params *prm, ms_stream stream);
MS_API int ms_get_gain_track_counters(ms_ctx *ctx, ms_gain_track_counters *out, ms_stream stream);

/* Exposure tracking on view shards (extends ms_track_gains / ms_gain_stats above to ms_config.view_shards > 1 with ms_stitch_partial / ms_stitch_finish; allowed
 * on unsharded contexts too, which own every view).  A pair statistic needs both views' pixels at one sample, and a view shard holds only its own views' -- but
 * what a pair needs of view a at a lattice sample is ONE integer: q_a as defined above, or "not seen".  The owner of a view computes it alone, from its own
 * pixels and the static maps, which every context of the group holds (the shards are created from the same cameras).  So each shard stores the q of its own
 * views on the lattice (a "sample vector" per view), the buffers are exchanged, and every shard forms cnt and S of every pair from all of them: the integers
 * k_gain_stats produces on an unsharded context, then the one solve of ms_track_gains.  Gains are bit-identical on every shard and on a single GPU; no host in
 * the loop, no gain on the wire.
 *   A sample buffer: ms_gain_samples_bytes(ctx, stride, view_shard_index) bytes of caller-owned DEVICE memory, 4-byte aligned; -1 = this context's own shard, and
 *     any rank can size any peer's buffer: the size depends on the geometry (cameras, stride, the shard's block of views, the active set) only.  Valid after
 *     ms_build_maps; 0 for a null context, stride < 1, an index outside [-1, view_shards), a buffer beyond 4 GiB, and the contexts every call below refuses
 *     (column shards, FeatherBlender).  ms_get_view_shard: the context's (view_shards, view_shard_index); (1, 0) without view sharding.  32-bit words:
 *       [0] magic 0x56474d53  [1] num_views  [2] active-view mask  [3] stride  [4..7] T.x, T.y, T.width, T.height (dst_roi_final)
 *       [8] the mask of the views held = owned & active  [9] total bytes  [10..15] 0
 *       [16 + v], v < num_views: the word offset of view v's data from the start of the buffer; 0 = not held
 *       then, per held view v in view order, row-major, one word per lattice sample of the rectangle R_v: R_v = the lattice indices (sx, sy), 0 <= sx <
 *       ceil(T.width / stride), 0 <= sy < ceil(T.height / stride), whose pano pixel (T.x + sx * stride, T.y + sy * stride) lies in roi_v; it may be empty.
 *       A word is 0 when the view does not see the sample (the truncated map coordinate is outside the source: the rule above), q + 1 otherwise (q < 2^29).
 *     The size is the caller's responsibility, and every buffer handed to a consumer holds at least 64 + 4 * num_views readable bytes: behind a header that
 *     passes the checks below, only words inside the stated size are read; behind one that does not, none.
 *   ms_get_gain_sample_views: the views ms_gain_samples reads = owned & active.  The other entries of `views` are never dereferenced: their ms_image may be
 *     all-zero.  ms_gain_samples / ms_gain_samples_nv12 (views as for ms_gain_stats_nv12) write this context's buffer from one frame set on `stream`: one launch.
 *   ms_track_gains_from_samples takes n (1 .. 4 = the largest view_shards) DEVICE pointers in a HOST array, in any order, and on `stream`: checks the headers on
 *     the device, forms cnt / S over the whole lattice, then does exactly what ms_track_gains does behind its statistics: N = max(1, cnt) on the pairs whose ROIs
 *     meet, I, the solve over the active views, smoothing in double, publication into every view table a stitch may read.  Rejected -- nothing changes, one
 *     rejected update is counted (ms_get_gain_track_counters), no error surfaces later -- when a header differs from what this context and this call expect
 *     (magic, num_views, active set, prm->stride, T, offsets, size), two buffers hold the same view, or an active view is held by none.
 *     ms_gain_samples + ms_track_gains_from_samples of that one buffer on an unsharded context == ms_track_gains, bit for bit; with views left out
 *     (ms_set_active_views) those are neither written nor paired.
 *   ms_gain_stats_from_samples: the statistics alone, blocking, N and S to the HOST as ms_gain_stats; a rejected set reports zeros and is counted.
 *   All but ms_gain_stats_from_samples are enqueue-only (no allocation, no copy to the host, no wait for the GPU) and callable while another thread stitches.
 *     They share the context's accumulators, gain state and counters with the routes above and keep their ordering guarantees: no older gain comes back, and a
 *     frame is composited with the gains before or after an update, never a mix.  The caller orders the buffers' producers before the consumer (same stream,
 *     or an event); buffers from other GPUs are moved by the caller (ms_dist_track_gains_views does it for a view-shard group).
 * MS_ERR_INVALID: null context / params / views / buffer(s), a buffer not 4-byte aligned, n outside [1, 4], struct_size mismatch, stride < 1, smoothing outside
 * (0, 1], an image of the wrong size or type among the views read.  MS_ERR_STATE: before ms_init_blender.  MS_ERR_UNSUPPORTED: FeatherBlender contexts and
 * contexts with col_shards > 1 (they have the partial route; a combination of the two shardings does not exist). */
MS_API size_t ms_gain_samples_bytes(const ms_ctx *ctx, int stride, int view_shard_index);
MS_API int ms_get_view_shard(const ms_ctx *ctx, int *view_shards, int *view_shard_index);
MS_API int ms_get_gain_sample_views(const ms_ctx *ctx, unsigned *mask);
MS_API int ms_gain_samples(ms_ctx *ctx, const ms_image *views, int stride, void *samples_dev, ms_stream stream);
MS_API int ms_gain_samples_nv12(ms_ctx *ctx, const ms_image *views_nv12, int stride, void *samples_dev, ms_stream stream);
MS_API int ms_gain_stats_from_samples(ms_ctx *ctx, const void *const *samples_dev, int n, int stride, long long *N_host, long long *S_host, ms_stream stream);
MS_API int ms_track_gains_from_samples(ms_ctx *ctx, const void *const *samples_dev, int n, const ms_gain_track_params *prm, ms_stream stream);

/* MeshWarper::convertMeshesToMap for one view (APP/meshwarper.cpp:823-886): N x M vertex mesh (HOST fp32,
 * forward positions in view-ROI pixels) -> dense backward maps x_mesh/y_mesh, double-buffered; takes
 * effect at the next ms_stitch.  Thread-safe against ms_stitch (recalibration thread, APP/timed.cpp:414-463). */
MS_API int ms_set_mesh(ms_ctx *ctx, int view, const float *mesh_x, const float *mesh_y, int N, int M,
                       ms_stream stream);
/* The same for ALL views of the context in one call -- convertMeshesToMap as the reference calls it (it loops over the images, meshwarper.cpp:823-886):
 * mesh_x / mesh_y = num_views meshes of N x M back to back (HOST).  Two launches and ONE completion event per recalibration instead of two of each per view; bit-identical maps.
 * The caller's arrays are copied into pinned staging before the call returns (a ring of eight generations: the call blocks only if the caller is eight updates ahead of the GPU). */
MS_API int ms_set_meshes(ms_ctx *ctx, const float *mesh_x, const float *mesh_y, int N, int M, ms_stream stream);
/* Or supply the dense maps directly (x_mesh[i], y_mesh[i] GpuMats, APP/timed.cpp:100). DEVICE 32FC1. */
MS_API int ms_set_mesh_maps(ms_ctx *ctx, int view, const ms_image *x_mesh, const ms_image *y_mesh, ms_stream stream);

/* stitch_one (APP/timed.cpp:123-152): for each of n_frames frames, views[f*num_views + i] is the 8UC3
 * camera frame (DEVICE; full_imgs[i] after upload, timed.cpp:68).  Writes per frame:
 *   out8u[f]  8UC3 out_width x out_height equirect canvas (pano ROI placed at its spherical position;
 *             = consume()'s convertTo(CV_8U), timed.cpp:251) -- may be NULL;
 *   out16s[f] 16SC3 pano ROI (dst_roi_final sized) = blend()'s gpuOut (blenders.cpp:811) -- may be NULL.
 * Layout of views, out8u and out16s (every frame its own; a GpuMat's data / step pass through unchanged): any row step from the row's bytes up to, not including,
 * 2^24 bytes (16 MiB), with rows * step < 2^32 -- the kernels form row * step with a 24-bit multiply or in 32 bits; any base address for the 8U images; 2-byte
 * alignment of base address and step for out16s.  Bytes between the end of a row and the next row, and canvas pixels outside the panorama ROI, are never written.
 * Anything else is refused with MS_ERR_INVALID before a kernel is enqueued, in every entry point that takes these images (ms_stitch_nv12, ms_blend for the
 * images ms_feed recorded, ms_stitch_partial / ms_stitch_finish, ms_stitch_timed).
 * No allocation, no host sync. */
MS_API int ms_stitch(ms_ctx *ctx, int n_frames, const ms_image *views, ms_image *out8u, ms_image *out16s,
                     ms_stream stream);
/* The reference's own call shape (timed.cpp:127-137): stitch_online(view) for every view, then MultiBandBlender::blend.  ms_feed records the
 * view's device image (8UC3, source size; borrowed until ms_blend), ms_blend composites the frame exactly like ms_stitch(ctx, 1, views, ...)
 * and fails with MS_ERR_STATE if a view was not fed since the previous blend.  (feed_online's per-view work is batched across views here, so
 * it runs inside ms_blend; the stream argument of ms_feed is accepted for signature parity and ignored.) */
MS_API int ms_feed(ms_ctx *ctx, int view, const ms_image *img, ms_stream stream);
MS_API int ms_blend(ms_ctx *ctx, ms_image *out8u, ms_image *out16s, ms_stream stream);

/* View sharding (BASELINE configs[4]): create every rank's context with the SAME cameras/masks and
 * ms_config.view_shards = number of shards S (<= 4), view_shard_index = this rank's shard index; shard k owns the contiguous block
 * of views [k*N/S, (k+1)*N/S).  The weighted accumulation into the dst Laplacian pyramid is a sum of int16 terms
 * (multiband_blend.cu:46-49), so each rank writes the partial sums of its views (ms_stitch_partial; entries of `views` for
 * views it does not own are ignored), the caller moves the partial buffers to the sink rank (RCCL send/recv: int16 has no
 * reduce op), and the sink adds them (wrap-around, order independent => bit-identical to one GPU), normalises, collapses and
 * writes the outputs (ms_stitch_finish).  ms_partial_bytes = size of one frame's partial buffer. */
MS_API size_t ms_partial_bytes(const ms_ctx *ctx);
MS_API int ms_stitch_partial(ms_ctx *ctx, int n_frames, const ms_image *views, void *partial_out, ms_stream stream);
MS_API int ms_stitch_finish(ms_ctx *ctx, int n_frames, const void *const *partials, int n_partials,
                            ms_image *out8u, ms_image *out16s, ms_stream stream);

/* gpu_dst_mask_ (blenders.cpp:803): frame-invariant; 8UC1 pano-ROI sized DEVICE image owned by ctx.  While views are left out (ms_set_active_views) it is
 * the active set's mask, held by that set's cached tables: valid until the next ms_set_active_views or table rebuild (ms_init_blender, ms_update_mask). */
MS_API int ms_get_result_mask(ms_ctx *ctx, ms_image *mask);

/* Calibration tables as a blob (the reference re-runs stitch_calib at every start, APP/timed.cpp:553).  ms_save_tables writes what the static
 * tables of a ready context derive from -- configuration, per view K, R, gain and blend mask, blender kind -- into `buf` (buf == NULL: only *bytes_out, the size
 * needed).  ms_load_tables creates a context from such a blob and rebuilds every table (same library build => bit-identical tables, e.g. on every rank of a
 * multi-GPU run); CPW meshes are run-time state and are set afterwards (ms_set_meshes).  Corrupt / foreign blobs are MS_ERR_INVALID before the device is touched: the FNV-1a
 * checksum covers the whole blob, the embedded configuration included.  A blob replays its context's configuration verbatim, so a column / view SHARD does not save
 * (MS_ERR_UNSUPPORTED): "one blob for every rank" is the blob of the unsharded context; shards are created from the same cameras / gains / masks. */
MS_API int ms_save_tables(ms_ctx *ctx, void *buf, size_t cap, size_t *bytes_out);
MS_API int ms_load_tables(const void *buf, size_t bytes, ms_ctx **out, ms_stream stream);
/* Diagnostics of the band kernels' work classification (no reference counterpart: the reference runs the general arithmetic everywhere).  The 64 x 16 pixel cells
 * of band `level` by class -- owned: one view with weight exactly 1 everywhere (no multiply, no division); exclusive (level 0 only): several views meet but every
 * pixel has one contributing view with weight exactly 1 (binary seam masks) -- the same integer arithmetic, selected by the mask bytes; general: the reference's
 * float multiply + divide.  Results are identical in every class (tests/test_compositor_gpu.py); bands without a map report every cell as general. */
MS_API int ms_get_band_cells(ms_ctx *ctx, int level, unsigned *owned, unsigned *exclusive, unsigned *general);

/* Diagnostics of the work lists (no reference counterpart: the reference launches full grids over every padded view).  build_plan keeps only the tiles some consumer
 * reads; the counts say what a launch touches, e.g. n_warp_tiles x warp_tile_w x warp_tile_h = the level-0 pixels the projection warp writes per frame (bench.py's
 * compulsory-byte figure `frac_useful` is computed from them).  struct_size as in ms_config. */
typedef struct ms_plan_stats {
    unsigned struct_size;
    int warp_tile_w, warp_tile_h, n_warp_tiles;          /* level-0 tiles of the projection warp (CPW: of the mesh remap)        */
    int n_stage1_tiles, n_stage1_reachable;              /* CPW: tiles of the first remap; those within reach of the mesh remap  */
    int down_tile_w, down_tile_h, n_down_tiles[8];       /* output tiles of the reduce from level l to l + 1 (tile kernel)       */
    int blend_tile_w, blend_tile_h, n_blend_tiles[8];    /* panorama tiles of band l (tile kernel)                               */
} ms_plan_stats;
MS_API int ms_get_plan_stats(ms_ctx *ctx, ms_plan_stats *out);

/* Which form of the remap kernels (a5: cuda::remap, cudawarping/src/cuda/remap.cu:56-86) the LAST ms_stitch* call of the context launched -- every form computes the
 * same pixels; which one runs is a function of the context and of the frames handed over.  SHARED_*: the frames of a view have one row step (and, for ALIGNED, one
 * address modulo 4), so a pixel's tap offset is built once for all frames of a call; PER_FRAME_*: they differ (e.g. per-frame ROI views of buffers of different
 * pitch, an odd byte offset) and every frame builds its own; ALIGNED / UNALIGNED: 12-byte aligned tap windows or 8-byte unaligned ones (chosen from the rig's
 * minification).  *stage1_kernel is MS_WARP_KERNEL_NONE without CPW.  A call of more frames than one source table holds (192 / views) sends these launches out in
 * chunks; the form reported is that of the first, full chunk.  Diagnostics for tests and profiles; no reference counterpart. */
enum { MS_WARP_KERNEL_NONE = 0, MS_WARP_KERNEL_SIMPLE = 1, MS_WARP_KERNEL_SHARED_ALIGNED = 2, MS_WARP_KERNEL_SHARED_UNALIGNED = 3, MS_WARP_KERNEL_PER_FRAME_ALIGNED = 4,
       MS_WARP_KERNEL_PER_FRAME_UNALIGNED = 5, MS_WARP_KERNEL_NV12 = 6, MS_WARP_KERNEL_LDS_STAGED = 7 };
MS_API int ms_get_stitch_kernels(ms_ctx *ctx, int *warp_kernel, int *stage1_kernel);

/* geometry read-back (top_/left_/bottom_/right_, x_tl_.., dst_roi_: blenders.hpp:143-175) */
typedef struct ms_view_geom {
    ms_rect roi;                        /* corner + size of the warped view (warpRoi)        */
    int top, left, bottom, right;       /* reflect border (blenders.cpp:378-381)             */
    int x_tl, y_tl, x_br, y_br;         /* padded rect inside the padded pano (blenders.cpp:425-428) */
} ms_view_geom;
typedef struct ms_pano_geom {
    int num_bands;
    ms_rect dst_roi_final, dst_roi;     /* unpadded / padded pano ROI                         */
    int canvas_x, canvas_y;             /* where pano (0,0) lands in the out8u canvas         */
} ms_pano_geom;
MS_API int ms_get_view_geom(const ms_ctx *ctx, int view, ms_view_geom *g);
MS_API int ms_get_pano_geom(const ms_ctx *ctx, ms_pano_geom *g);
/* ---- CPW mesh optimiser: MeshWarper::createMesh after feature matching (360_stitcher/meshwarper.cpp:279-301) ------------------------
 * The feature front-end (ORB, matching, RANSAC: featurefinder.cpp) stays with the caller; what crosses the boundary is what
 * createMesh hands to calcLocalTerm / calcGlobalTerm: per view, the selected matches (filterMatches, meshwarper.cpp:888-946, capped at
 * MAX_FEATURES_PER_IMAGE) as keypoint positions in WARPED-VIEW pixels. */
typedef struct ms_mesh_match {
    float x1, y1;       /* features[src].keypoints[queryIdx].pt, src = the view the list belongs to */
    float x2, y2;       /* features[dst].keypoints[trainIdx].pt (temporal lists: the same view in the previous calibration) */
    int dst;            /* matchWithDst_t::dst (ignored in temporal lists) */
} ms_mesh_match;

typedef struct ms_mesh_params {
    int mesh_cols, mesh_rows;       /* M, N: MESH_WIDTH, MESH_HEIGHT (defs.h:65-66) */
    float alphas[4];                /* ALPHAS (defs.h:69): local, global, smoothness, temporal term weights; temporal is used iff != 0 (defs.h:70) */
    int global_dist;                /* GLOBAL_DIST (defs.h:71) */
    float focal_length;             /* MeshWarper::focal_length */
    double compose_scale, work_scale;
    int wrap_around;                /* wrapAround (defs.h:25) */
    int theta_rule;                 /* 0: the reference's hard-coded 6-camera angles (meshwarper.cpp:617-629); 1: (dst - src) * 2 pi / n_views, wrapped */
    int max_iterations;             /* 0 = Eigen's default, 2 * columns */
    double tolerance;               /* 0 = Eigen's default, DBL_EPSILON */
} ms_mesh_params;

typedef struct ms_mesh_info {
    int rows, cols, nnz;            /* the system actually assembled (the reference allocates more, all-zero, rows) */
    int iterations;                 /* solver.iterations() */
    double error;                   /* solver.error() = ||A^T r|| / ||A^T b|| */
} ms_mesh_info;

MS_API int ms_mesh_default_params(ms_mesh_params *prm);      /* defs.h values, 10 x 10 mesh */
/* calcSmoothnessTerm's salience (meshwarper.cpp:497-563) of every (vertex, triangle) of one warped view (device 8UC3):
 * sal_host[(i * mesh_cols + j) * 8 + t], NaN where triangle t of vertex (j, i) leaves the mesh.  The pixel pass (masked sum / sum of squares
 * per cell crop, cv::meanStdDev under a cv::fillConvexPoly mask) runs on the device. */
MS_API int ms_mesh_saliency(const ms_image *warped_view, int mesh_cols, int mesh_rows, float *sal_host, ms_stream stream);
/* The 8 triangle masks of one mesh cell as calcSmoothnessTerm builds them (meshwarper.cpp:527-551: `Mat mask(cell_h, cell_w)` +
 * cv::fillConvexPoly of the triangle's corners), produced by the device kernel ms_mesh_saliency uses.  masks_host: 8 * cell_h * cell_w bytes
 * (0 / 255), triangle-major; counts_host (may be NULL): 8 set-pixel counts.  Inspection / test aid. */
MS_API int ms_mesh_triangle_masks(int cell_w, int cell_h, uint8_t *masks_host, unsigned *counts_host, ms_stream stream);
/* createMesh's loop + solve (meshwarper.cpp:279-301): for every view calcLocalTerm, calcGlobalTerm, calcSmoothnessTerm[, calcTemporalLocalTerm],
 * then x = LeastSquaresConjugateGradient(A).solve(b) in fp64 on the device and convertVectorToMesh.
 * warped_views[n_views]: the remapped frames `images[idx]` (device 8UC3; mesh_size = their sizes).  matches: the per-view lists back to back,
 * match_count[v] entries each (host); temporal / temporal_count likewise or NULL.  mesh_x / mesh_y: host, n_views * mesh_rows * mesh_cols
 * vertex positions in view pixels, ready for ms_set_mesh / ms_set_mesh_interp.  Synchronises `stream`. */
MS_API int ms_create_mesh(int n_views, const ms_image *warped_views, const ms_mesh_match *matches, const int *match_count,
                          const ms_mesh_match *temporal, const int *temporal_count, const ms_mesh_params *prm,
                          float *mesh_x, float *mesh_y, ms_mesh_info *info, ms_stream stream);

/* DescriptorMatcher::create("BruteForce-Hamming")->knnMatch(query, train, matches, 2) of featurefinder::matchFeatures / matchFeaturesTemporal
 * (360_stitcher/featurefinder.cpp:50-61, :117-128; BFMatcher::knnMatchImpl, features2d/src/matchers.cpp:815-880; cv::batchDistance,
 * core/src/stat.cpp:3946-4008).  query / train: DEVICE 8UC1 descriptor rows (ORB: 32 bytes; any multiple of 4 up to 64).  For query row q,
 * train_idx_host[2q], [2q+1] and distance_host[2q], [2q+1] receive the two nearest train rows in (distance, index) order -- exactly the rows
 * and tie-breaks of the reference's insertion loop; index -1 / distance INT_MAX where train has fewer than two rows.  The 0.7 ratio test and
 * findHomography stay with the caller (msshim::knnRatioMatches does the former).  Synchronises `stream`. */
MS_API int ms_knn_match_hamming2(const ms_image *query, const ms_image *train, int *train_idx_host, int *distance_host, ms_stream stream);

/* ---- feature front-end of the recalibration path ----------------------------------------------------------------------------
 * cuda::ORB::create(nfeatures, scaleFactor, nlevels)->detectAndCompute(gray, mask, keypoints, descriptors) of featurefinder::findFeatures
 * (360_stitcher/featurefinder.cpp:13-46 -> cudafeatures2d/src/orb.cpp:430-865, cuda/fast.cu, cuda/orb.cu): image / mask pyramids, FAST 9-16 with
 * score and 3 x 3 non-max suppression, per-level budgets, Harris responses, intensity-centroid angles, rBRIEF descriptors (WTA_K = 2, HARRIS_SCORE,
 * no blur: the creator's defaults).  gray: DEVICE 8UC1 (ms_bgr_to_gray); mask: DEVICE 8UC1 of the same size or NULL.
 * keypoints_host: max_keypoints x 6 floats (x, y, response, angle in degrees, octave, size), the rows of cuda::ORB's keypoint matrix;
 * descriptors: DEVICE 8UC1 max_keypoints x 32 (row i belongs to keypoint i; rows from *n_keypoints on are not written).  Synchronises once.
 * The result, defined here (the reference leaves the order to atomics and an unstable sort); oracle/orb_oracle.py states it in numpy and the tests hold the
 * library to it byte for byte:
 *   order    levels in turn (mergeKeyPoints, orb.cpp:823-865).  Inside a level: raster order after FAST; each cull (to 2n by FAST response, :772, then to n by
 *            Harris response, :778; cull: :719-733) is a stable descending sort of that order where the level holds more than it keeps, and no change otherwise.
 *   budgets  orb.cpp:501-512 (a geometric series rounded per level, the last level takes nfeatures minus the others), which gives some levels 0 at small
 *            nfeatures (nfeatures 1: only the last level has a budget) and the last level a negative number at a few (nfeatures 7 at the defaults: -1), where
 *            the reference is undefined.  Here a level whose budget is <= 0 contributes no keypoints and the call succeeds.  The other levels keep their
 *            budgets, so with a negative last budget up to (nlevels - 1) / 2 more than nfeatures keypoints come back (each rounding adds at most one half):
 *            max_keypoints >= nfeatures + nlevels / 2 holds them at any parameters; a smaller buffer that overflows is MS_ERR_INVALID, and nothing past row
 *            max_keypoints - 1 is written.
 *   over-cap where a level has more raw FAST corners than the detector's buffer (max_npoints = 0.05 * its area, orb.cpp:753), the reference keeps whichever win
 *            its atomic counter (fast.cu:338-341); here the candidates are the first max_npoints raw corners in raster order, each suppressed against the
 *            whole score map.
 *   limits   first_level 0, patch_size 31 (the learned pattern), 1..16 levels, nfeatures >= 1, scale_factor > 1; edge_threshold >= 19 (the reach of the
 *            rotated pattern: the kernels read around a keypoint without bounds checks) and fast_threshold in [1, 254]; an image of at most 32767 x 32767
 *            (keypoint coordinates are 16-bit on the device); a mask, where given, with data, 8UC1 and of the image size; descriptors 8UC1, 32 columns, at
 *            least max_keypoints (>= nfeatures) rows and a step of at least 32 bytes.  Anything else is MS_ERR_INVALID before anything is launched.  The
 *            pyramid ends before the first level narrower or lower than 8 pixels; a level not larger than 2 * edge_threshold in both dimensions has no
 *            keypoints.
 * The call is ms_orb_detect_and_compute_batch with n_views = 1 (see there for the mechanism): it works over the calling thread's grow-only staging blocks -- no
 * allocation once they have grown -- with nlevels + 10 launches at most and ONE synchronisation. */
typedef struct ms_orb_params {
    int nfeatures; float scale_factor; int nlevels;      /* ORB::create(2500, 1.2f, 8)  featurefinder.cpp:15 */
    int edge_threshold, first_level, patch_size, fast_threshold;     /* 31, 0, 31, 20 (cuda::ORB::create defaults) */
} ms_orb_params;
MS_API int ms_orb_default_params(ms_orb_params *prm);
MS_API int ms_orb_detect_and_compute(const ms_image *gray, const ms_image *mask, const ms_orb_params *prm, float *keypoints_host, int max_keypoints,
                                     ms_image *descriptors, int *n_keypoints, ms_stream stream);
/* The same for every view of a rig in one device pass: what featurefinder::findFeatures (360_stitcher/featurefinder.cpp:13-46) asks of
 * cuda::ORB::detectAndCompute (cudafeatures2d/src/orb.cpp:430-865) view after view.  gray: n_views DEVICE 8UC1 images, which may differ in size; masks: NULL, or
 * n_views entries (data == NULL: no mask for that view); keypoints_host: n_views x max_keypoints x 6 floats; descriptors: n_views DEVICE 8UC1 matrices of
 * max_keypoints x 32, none overlapping another.  View v gets the result ms_orb_detect_and_compute defines for (gray + v, its mask or NULL, prm), bit for bit and in
 * that order, at keypoints_host + 6 * max_keypoints * v, descriptors + v and n_keypoints + v: n_keypoints[v] keypoint rows and the first n_keypoints[v]
 * descriptor rows; descriptor rows from n_keypoints[v] on are not written.  The single call is this with n_views = 1.  The output is the input ms_match_pairs takes.
 * A segment is one pyramid level of one view.  Sizes, budgets (orb.cpp:501-512), the detector's buffer (0.05 * area, :753) and every buffer offset follow from
 * the shapes and prm, so they go up once as a table and no count comes back before the end.  On the device, each step one launch over all segments: the pyramid
 * level by level (resize from the level below, :686; masks with it and through THRESH_TOZERO 254, :690-693); FAST scores (fast.cu:224-344); raw corners per row,
 * scan, survivors per row, scan, write -- raster order, with the over-cap rule of the single call's comment applied in every segment (a level within the buffer has
 * every raw corner as a candidate); the cull to 2n by FAST response (:772: a 256-bin histogram, then
 * one ordered pass; no change and raster order where the level holds no more); Harris (orb.cu:93-138); the cull to n (:778) as a stable rank sort, keys through
 * LDS in tiles of 1024; angles (orb.cu:160-211) and the six floats of mergeKeyPoints (:823-865) at the view's row offset; descriptors (orb.cu:222-367) straight
 * into the caller's matrices.  No atomic decides an order: two calls return the same bytes.  Per call, whatever n_views is: nlevels + 10 launches at most,
 * 1 upload, 1 clear, 1 copy back, 1 synchronisation, over the calling thread's grow-only staging blocks (no allocation once they have grown).  Device scratch in
 * bytes, with A_v the sum of w * h over the levels of view v (about 3.3 times its area at 1.2 / 8 levels): 48 KiB of tables + 24 * n_views * max_keypoints
 * + sum over v of [A_v (scores) + (A_v - area_v) (pyramid; twice with a mask) + 0.25 * A_v (candidates: 5 bytes for each of 0.05 * w * h) + 8 rows(A_v)]
 * -- some 4.5 times the views' area without masks, 5.5 with; MS_ERR_NOMEM before anything is launched where it cannot be had.
 * MS_ERR_INVALID, before the device is touched and naming the view: n_views outside [1, MS_MAX_VIEWS]; a null array; the limits of the single call's comment; a view
 * that is not 8UC1, has no data or is larger than 32767 in a dimension; a mask of another type or size; a descriptor matrix of another shape than max_keypoints
 * (>= nfeatures) x 32 with a step of at least 32, or whose byte range (steps included) overlaps another view's.  After the pass: a view with more than max_keypoints keypoints (see the
 * single call: max_keypoints >= nfeatures + nlevels / 2 always holds them); the device clamps, so nothing past row max_keypoints - 1 of any view is written.
 * Limits: one parameter set for the batch (no per-view nfeatures).  Synchronises. */
MS_API int ms_orb_detect_and_compute_batch(int n_views, const ms_image *gray, const ms_image *masks, const ms_orb_params *prm, float *keypoints_host,
                                           int max_keypoints, ms_image *descriptors, int *n_keypoints, ms_stream stream);
/* The feature mask createMesh builds for findFeatures (360_stitcher/meshwarper.cpp:82-115): 255 inside the two column bands where neighbouring
 * views overlap (rect_a / rect_b: x0, width -- cv::rectangle clips them to the image) AND where the warped view is not black (inRange(0, 0) negated:
 * the pixels the projection did not fill).  warped_view: DEVICE 8UC3; mask: DEVICE 8UC1 of the same size. */
MS_API int ms_feature_mask(const ms_image *warped_view, int a_x0, int a_width, int b_x0, int b_width, ms_image *mask, ms_stream stream);
/* The grey images and the feature masks of every view of a round in ONE launch: cuda::cvtColor(BGR2GRAY) of findFeatures (360_stitcher/featurefinder.cpp:34) and
 * createMesh's mask loop (meshwarper.cpp:82-115), which the reference and the two single calls above run view after view.  warped_views: n_views DEVICE 8UC3
 * images, which may differ in size; bands: n_views x {a_x0, a_width, b_x0, b_width} (HOST), needed with masks; gray / masks: n_views DEVICE 8UC1 images of their
 * view's size, either array may be NULL but not both.  gray[v] is byte-equal to ms_bgr_to_gray(warped_views + v) and masks[v] to ms_feature_mask(warped_views + v,
 * the bands of v) -- the bands clipped to the image as there --; bytes past a row's width are not written.  The grid is laid over the views' 256 x 4 pixel tiles,
 * a workgroup finds its (view, tile) from the per-view table that goes up with the launch; a lane takes 4 pixels of a row and reads each BGR pixel once for both
 * outputs.  Enqueue-only, as the single calls.
 * MS_ERR_INVALID before the device is touched, naming the view: n_views outside [1, MS_MAX_VIEWS]; null warped_views; gray and masks both NULL; masks without
 * bands; a view, grey image or mask without data, empty, of another type, with a step below its row; a grey image or mask of another size than its view. */
MS_API int ms_feature_inputs_batch(int n_views, const ms_image *warped_views, const int *bands, ms_image *gray, ms_image *masks, ms_stream stream);
/* cv::findHomography(src, dst, mask, RANSAC) of featurefinder::matchFeatures (featurefinder.cpp:68-90 -> calib3d/src/fundam.cpp:319-402,
 * ptsetreg.cpp:53-290, levmarq.cpp:76-214): src_xy / dst_xy HOST, n points (x, y) each.  reproj_threshold <= 0 -> 3, max_iters <= 0 -> 2000,
 * confidence outside (0, 1) -> 0.995 (the reference's defaults).  Same cv::RNG subset sequence, subset checks, acceptance rule and adaptive
 * iteration count as the reference; all candidate 4-point models are fitted and scored on the device (the batch of one of the call below), the final
 * N-point fit and the 10-iteration Levenberg-Marquardt polish of the winner run on the host.  H: 9 doubles row-major (H[8] = 1); inlier_mask: n bytes
 * (may be NULL).  Returns MS_OK, 1 if no model was found (H zeroed; the reference returns an empty Mat), or a negative status. */
MS_API int ms_find_homography_ransac(const float *src_xy, const float *dst_xy, int n, double reproj_threshold, int max_iters, double confidence,
                                     double *H, uint8_t *inlier_mask, int *n_inliers, ms_stream stream);
/* The same for n_problems independent point sets in one device pass: what BestOf2NearestMatcher::match (OCV/stitching/src/matchers.cpp:699-770) driven over all
 * pairs asks of cv::findHomography (calib3d/src/fundam.cpp:319-402) pair after pair.  Problem p holds the points offsets[p] .. offsets[p + 1] - 1 of src_xy / dst_xy
 * (HOST, (x, y) each; offsets: n_problems + 1 ints, ascending, offsets[0] = 0; empty problems are allowed) and gets exactly what
 * ms_find_homography_ransac(src_xy + 2 * offsets[p], dst_xy + 2 * offsets[p], offsets[p + 1] - offsets[p], ...) returns, bit for bit: H + 9 * p (zeroed without a
 * model), inlier_mask + offsets[p] (may be NULL), n_inliers[p] (may be NULL) and status[p] = 0 (a model) or 1 (none).  A problem's result depends neither on
 * its neighbours nor on its place in the batch.  The three RANSAC parameters are shared and follow the same defaults rule.
 * Per problem on the host, as in the single call: the cv::RNG subset sequence (seeded per problem), the subset checks, the sequential first-strictly-better scan
 * with the adaptive iteration count, the final N-point fit and the polish; problems with fewer than 5 points or no drawable subset never reach the device.  On the
 * device, for all problems at once: one lane per hypothesis fits its 4-point model (k_ransac_fit); one workgroup per (problem, 64 hypotheses) counts inliers, the
 * problem's points staged through LDS in chunks of 512 and split over the workgroup's 4 waves, 128 points of a chunk each (k_ransac_score; the counts are
 * integers, so the split changes nothing); after the host's scans a third launch gathers the winners' models.  Per batch, whatever n_problems is: at most
 * 3 launches, 4 copies (upload; counts back; winners' numbers up; their models back) and 2 synchronisations over the calling thread's grow-only staging
 * blocks, no allocation once they have grown; none of it where no problem needs the device or (the last launch and its two copies) where none has a winner.
 * Returns MS_OK (also when every problem ends without a model) or a negative status.  MS_ERR_INVALID before the device is touched: n_problems < 0; null offsets,
 * H or status; offsets[0] != 0 or a descending pair; null src_xy or dst_xy with offsets[n_problems] > 0; a reproj_threshold or confidence that is not finite.
 * n_problems == 0 is MS_OK and touches nothing.  Synchronises. */
MS_API int ms_find_homography_ransac_batch(int n_problems, const int *offsets, const float *src_xy, const float *dst_xy, double reproj_threshold, int max_iters,
                                           double confidence, double *H, uint8_t *inlier_mask, int *n_inliers, int *status, ms_stream stream);

/* ---- Rig rotation refinement: ray bundle adjustment from feature matches ---------------------------------------------------------------------
 * detail::BundleAdjusterRay (OCV/stitching/src/motion_estimators.cpp:514-700) with the focals held: the stage between the feature front end above and
 * ms_set_camera / ms_build_maps that the reference app leaves out because it hard-codes the ring of ms_calibrate_cameras.  A warped pixel (u, v) of view i shows
 * the source pixel whose camera ray is R_i^-1 d(u, v), d the warper's backward direction -- on the analytic route and on the lens route alike -- so matches in
 * warped-view pixels carry the camera rays and the refinement needs neither K nor an inverse of the distortion.
 * The arithmetic contract, all of it in double:
 *   A match k on the view pair (i, j) holds two unit camera rays of one scene point, a_k seen by view i and b_k by view j.  The unknowns are the rotations R_v
 *   (camera to rig, the R of ms_set_camera) of every view but the anchor, whose rotation is held (the gauge).  Pairs are taken as i < j (a and b swapped where a
 *   match lists (j, i)); a pair with fewer than min_pair_matches matches is ignored and counted; after that every view must be connected to the anchor.
 *   Residual (BundleAdjusterRay::calcError, motion_estimators.cpp:556-627; with the focals held its sqrt(f1 f2) factor drops out): with p = R_i a, q = R_j b
 *   (row r: R[3r] a0 + R[3r+1] a1 + R[3r+2] a2, summed left to right), r = p - q, s = sqrt(r0 r0 + r1 r1 + r2 r2).  Huber threshold h in radians: w = 1 and
 *   rho = s^2 when h = 0 or s <= h, otherwise w = h / s and rho = (2 h) s - h h.  cost = sum rho.
 *   Linearisation about the update R_v <- Exp(delta_v) R_v (Exp = Rodrigues): J_i = -[p]x, J_j = +[q]x,
 *     g_i = sum w J_i^T r = sum w (p x r),            g_j = sum w J_j^T r = sum -(w (q x r)),
 *     H_ii = sum w J_i^T J_i = sum w [p]x^T [p]x       (diagonal w (p1 p1 + p2 p2), ..; off-diagonal -(w (p0 p1)), ..), H_jj likewise with q,
 *     H_ij = sum w J_i^T J_j = sum w (q p^T - (p.q) I) (row r, column c: w (q_r p_c); diagonal -(w (p1 q1 + p2 q2)), ..), H_ji = H_ij^T.
 *   Every product and sum of a term is one IEEE operation in the order written (no fused multiply-add): implementations differ by the order of the sums only.
 *   Levenberg-Marquardt: lambda = 1e-3; solve (H + lambda diag H) delta = -g over the non-anchor views (at most 45 unknowns) by Cholesky -- a pivot that is not
 *   positive counts as a rejected step; form the trial rotations and accept iff cost_trial <= cost.  Accept: lambda <- max(lambda / 10, 1e-12), stop as
 *   CONVERGED when max |delta| < step_tol.  Reject: lambda <- 10 lambda, stop as STALLED when lambda > 1e12.  Every judged trial (and every refused pivot) is one
 *   iteration; stop as ITERATION_LIMIT at max_iters.  All three return MS_OK with the last ACCEPTED rotations: cost_final <= cost_initial always. */
enum { MS_RIG_CONVERGED = 0, MS_RIG_STALLED = 1, MS_RIG_ITERATION_LIMIT = 2 };
typedef struct ms_rig_match {
    int view_a, view_b;
    double a[3], b[3];             /* unit camera rays of one scene point: a in view_a's camera, b in view_b's */
} ms_rig_match;
typedef struct ms_rig_refine_params {
    unsigned struct_size;          /* as ms_config: mismatch = MS_ERR_INVALID */
    int anchor_view;               /* 0: the view whose rotation is held */
    double huber_rad;              /* 0 = plain least squares; otherwise the Huber threshold on |r| in radians */
    int max_iters;                 /* 50; [1, 1000] */
    double step_tol;               /* 1e-10 */
    int min_pair_matches;          /* 4: pairs with fewer matches are ignored */
} ms_rig_refine_params;
typedef struct ms_rig_refine_info {
    int iterations, stop_reason;   /* MS_RIG_* */
    double cost_initial, cost_final;
    int matches_used, pairs_used, pairs_ignored;
    int outliers;                  /* matches with s > huber_rad at the returned rotations (0 without Huber) */
    double max_rotation_rad;       /* the largest angle between a view's input and output rotation */
} ms_rig_refine_info;
/* RotationWarper::warpBackward's direction (Plane / Spherical / CylindricalProjector::mapBackward, stitching/include/opencv2/stitching/detail/warpers_inl.hpp:229-307)
 * as a camera ray.  Host only, needs no device.  uv: n absolute warper coordinates (ROI corner + view pixel); rays: n unit camera rays R^T d(u, v) / |R^T d(u, v)| with,
 * in double from u' = (double)u / (double)scale, v' likewise: spherical d = (sin(pi - v') sin u', cos(pi - v'), sin(pi - v') cos u'), cylindrical d = (sin u', v', cos u'),
 * plane d = (u' - t0, v' - t1, 1 - t2) (t: 3 floats, NULL = zero; ignored by the other two).  R: 9 doubles row-major. */
MS_API int ms_warper_rays(int projection, float scale, const float *t, const double *R, int n, const float *uv, double *rays);
/* BundleAdjusterRay's defaults in this contract's terms (motion_estimators.cpp:514-555): anchor 0, no Huber, 50 iterations, step_tol 1e-10, 4 matches a pair */
MS_API int ms_rig_refine_default_params(ms_rig_refine_params *prm);
/* BundleAdjusterRay::calcError + calcJacobian (motion_estimators.cpp:556-700) as the normal equations, per op: cost, H (3 n_views x 3 n_views row-major, the anchor
 * included -- no view is held here) and g (3 n_views) at the rotations R (n_views x 9 doubles), every pair used whatever its size.  All pointers HOST.  Synchronises. */
MS_API int ms_rig_accumulate(int n_views, const double *R, const ms_rig_match *matches, int n, double huber_rad, double *cost, double *H, double *g, ms_stream stream);
/* BundleAdjusterBase::estimate (motion_estimators.cpp:223-324: CvLevMarq over calcError / calcJacobian) for the contract above, the whole loop on the device: matches
 * are grouped by pair on the host (stably: input order is kept inside a pair) and uploaded once, max_iters + 1 rounds of two kernels are enqueued with no host step
 * in between -- they return at once after the stop flag is set --, the result comes back in one copy and `stream` is synchronised once, at the end.  No
 * floating-point atomics: two calls on the same inputs return the same bits.  R_in is used as given (n_views x 9 doubles, HOST); R_out likewise, the anchor's
 * bit-equal to its R_in; info may be NULL.
 * MS_ERR_INVALID, before the device is touched: a null pointer; n_views outside [2, MS_MAX_VIEWS]; a view index out of range or view_a == view_b; a ray (or
 * rotation) that is not finite or whose length is off 1 by more than 1e-6; n outside [1, 2^20]; a bad anchor; a struct_size mismatch; max_iters outside [1, 1000],
 * a negative huber_rad or step_tol, min_pair_matches < 1; a view not connected to the anchor (the message names the first). */
MS_API int ms_refine_rig_rotations(int n_views, const double *R_in, const ms_rig_match *matches, int n, const ms_rig_refine_params *prm, double *R_out,
                                   ms_rig_refine_info *info, ms_stream stream);
/* The context form (Stitcher::estimateCameraParams' bundle adjustment, stitching/src/stitcher.cpp:573-574, on the matches featurefinder::matchFeatures selects):
 * the per-view lists in ms_create_mesh's layout -- x1, y1 in the list's own view, x2, y2 in view dst, pixels of the projection-warped views before any CPW mesh --
 * are turned into rays with the context's projection, warp_scale, view ROI corners and CURRENT cameras by ms_warper_rays' arithmetic (corner + pixel added in
 * double), then refined as above from the current rotations.  R_out: num_views x 9 floats for ms_set_camera; nothing is applied -- the caller runs the usual
 * chain (ms_set_camera, ms_build_maps, masks, ms_init_blender).  Lens contexts work unchanged.  MS_ERR_STATE before ms_build_maps; MS_ERR_UNSUPPORTED for
 * MS_MAPS_CUSTOM contexts (no cameras); MS_ERR_INVALID as above and for a list that names its own view or a view out of range. */
MS_API int ms_refine_rig(ms_ctx *ctx, const ms_mesh_match *matches, const int *match_count, const ms_rig_refine_params *prm, float *R_out,
                         ms_rig_refine_info *info, ms_stream stream);

/* ---- Self-calibrating rigs: focals and rotations from feature matches ----------------------------------------------------------------------------
 * The three steps of OpenCV's stitching pipeline that produce and correct the one rig parameter the section above holds fixed, the focal length:
 * detail::focalsFromHomography (OCV/stitching/src/autocalib.cpp:63-91), detail::HomographyBasedEstimator (motion_estimators.cpp:127-193: estimateFocal, the maximum
 * spanning tree, CalcRotation) and detail::BundleAdjusterRay over focal AND rotation (motion_estimators.cpp:514-700).  The first two are a few dozen operations on
 * the host; the bundle adjustment runs on the device with the whole Levenberg-Marquardt loop resident there, as the rotation refinement above does.
 * The arithmetic contract of the bundle adjustment, all of it in double:
 *   A match k on the view pair (i, j) holds two CENTRED source pixels of one scene point, (xa, ya) in view i and (xb, yb) in view j: pixels measured from the
 *   principal point, y already divided by the aspect ratio K[4] / K[0].  Pairs are taken as i < j (the two pixels swapped where a match lists (j, i)); a pair with
 *   fewer than min_pair_matches matches is ignored and counted; after that every view must be connected to the anchor.
 *   Unknowns per view v: the rotation R_v (camera to rig), updated R_v <- Exp(delta_v) R_v, the anchor's held; and the log-focal s_v = ln f_v, updated
 *   f_v <- f_v exp(d_v) (a focal never turns non-positive).  The anchor's focal is free.  shared_focal != 0: one s for the whole rig.  At most 3 * 15 + 16 = 61.
 *   Rays: na = sqrt(xa xa + ya ya + f_i f_i), a = (xa / na, ya / na, f_i / na); nb and b likewise with f_j.  p = R_i a, q = R_j b (row r: R[3r] a0 + R[3r+1] a1 +
 *   R[3r+2] a2, summed left to right).
 *   Residual (calcError's `mult`): m = sqrt(f_i f_j), r_k = m (p_k - q_k): pixels.  (Without m, f -> infinity sends every ray to the axis and the cost to 0.)
 *   s = sqrt(r0 r0 + r1 r1 + r2 r2).  Huber threshold h = huber_px: w = 1 and rho = s^2 when h = 0 or s <= h, otherwise w = h / s and rho = (2 h) s - h h.
 *   Jacobian, analytic (OpenCV differentiates numerically), with u_k = m p_k, v_k = m q_k, ma = m a2, mb = m b2:
 *     dr/d delta_i = -[u]x,   dr/d s_i = ci,  ci_k = 0.5 r_k + ma (R_i[3k+2] - a2 p_k)        (d a / d s_i = a2 (e_z - a2 a), d m / d s_i = m / 2)
 *     dr/d delta_j = +[v]x,   dr/d s_j = cj,  cj_k = 0.5 r_k - mb (R_j[3k+2] - b2 q_k)
 *   The 46 sums of a pair, 4 unknowns a view in the order (delta_0, delta_1, delta_2, s); x is the cross product, (x)_k its component k:
 *     cost  sum rho
 *     g_i   sum w (u x r)_k, k = 0 1 2: w (u1 r2 - u2 r1), w (u2 r0 - u0 r2), w (u0 r1 - u1 r0);   then sum w (ci0 r0 + ci1 r1 + ci2 r2)
 *     g_j   sum -(w (v x r)_k);                                                                     then sum w (cj0 r0 + cj1 r1 + cj2 r2)
 *     H_ii  symmetric, stored (00 01 02 03 11 12 13 22 23 33): w (u1 u1 + u2 u2), -(w (u0 u1)), -(w (u0 u2)), w (u x ci)_0, w (u0 u0 + u2 u2), -(w (u1 u2)),
 *           w (u x ci)_1, w (u0 u0 + u1 u1), w (u x ci)_2, w (ci0 ci0 + ci1 ci1 + ci2 ci2)
 *     H_jj  the same with v and cj, its three rotation-focal entries negated: -(w (v x cj)_k)
 *     H_ij  4 x 4 row-major (rows: view i): rotation rows r, rotation columns c: w (v_r u_c) off the diagonal, -(w (u1 v1 + u2 v2)), -(w (u0 v0 + u2 v2)),
 *           -(w (u0 v0 + u1 v1)) on it; column 3: w (u x cj)_r; row 3: -(w (v x ci)_c), then w (ci0 cj0 + ci1 cj1 + ci2 cj2).  H_ji = H_ij^T.
 *     outliers  the number of matches with s > h
 *   Every product, sum, division and sqrt above is one IEEE operation in the order written (no fused multiply-add), sums of three left to right: two
 *   implementations differ by the order of the per-match sums only.  With a shared focal the focal rows and columns of all views are added into one.
 *   Levenberg-Marquardt: exactly the rule of the section above (lambda = 1e-3, Cholesky of H + lambda diag H with a non-positive pivot a rejected step, accept iff
 *   cost_trial <= cost, lambda / 10 floored at 1e-12 or * 10, the MS_RIG_* stop reasons); step_tol is tested on max |.| over the rotation AND log-focal
 *   components of the step.  The call returns the last ACCEPTED state: cost_final <= cost_initial always. */
typedef struct ms_pair_homography {
    int view_a, view_b;
    double H[9];                   /* row-major; maps centred pixels of view_a to centred pixels of view_b */
    int weight;                    /* the pair's inlier count: the edge weight of the spanning tree */
} ms_pair_homography;
typedef struct ms_rig_estimate_info {
    int focal_estimates;           /* pairs whose homography gave both focals */
    int tree_parent[MS_MAX_VIEWS]; /* the view each view's rotation was chained from; -1 for the anchor */
} ms_rig_estimate_info;
typedef struct ms_rig_px_match {
    int view_a, view_b;
    double a[2], b[2];             /* centred source pixels of one scene point: a in view_a, b in view_b */
} ms_rig_px_match;
typedef struct ms_rig_focal_params {
    unsigned struct_size;          /* as ms_config: mismatch = MS_ERR_INVALID */
    int anchor_view;               /* 0: the view whose rotation is held */
    int shared_focal;              /* 1: one focal for the whole rig (identical cameras); 0: one a view */
    int max_iters;                 /* 50; [1, 1000] */
    double huber_px;               /* 0 = plain least squares; otherwise the Huber threshold on |r| in pixels */
    double step_tol;               /* 1e-10 */
    int min_pair_matches;          /* 4: pairs with fewer matches are ignored */
} ms_rig_focal_params;
typedef struct ms_rig_focal_info {
    int iterations, stop_reason;   /* MS_RIG_* */
    double cost_initial, cost_final;
    int matches_used, pairs_used, pairs_ignored;
    int outliers;                  /* matches with s > huber_px at the returned cameras (0 without Huber) */
    double max_rotation_rad;       /* the largest angle between a view's input and output rotation */
    double max_focal_ratio;        /* the largest of f_out / f_in and f_in / f_out over the views (>= 1) */
} ms_rig_focal_info;
/* detail::focalsFromHomography (autocalib.cpp:63-91) on a homography between CENTRED pixel coordinates: *f0 the focal of the source view, *f1 of the destination,
 * each written only where its flag comes back 1 (a rotation about the optical axis alone, the identity among them, determines neither).  Host only, no device. */
MS_API int ms_focals_from_homography(const double H[9], double *f0, double *f1, int *f0_ok, int *f1_ok);
/* detail::HomographyBasedEstimator (motion_estimators.cpp:127-193) on centred pixels, aspect 1.  Host only, no device.  Focal: the median of sqrt(f0 f1) over the pairs
 * whose homography gives both (an even count: the mean of the middle two), for every view; none valid: every focal is width + height and the call returns 1
 * (estimateFocal's fallback, autocalib.cpp:129-137).  Rotations: a maximum spanning tree over `weight` (Kruskal, ties to the earlier pair), walked breadth-first
 * from `anchor`, whose rotation is the identity; along an edge a -> b with H mapping a to b, R_b = R_a K_a^-1 H^-1 K_b (H itself where the pair is listed (b, a)),
 * K = diag(f, f, 1); every product is then projected onto SO(3) as U V^T of its singular value decomposition (a one-sided Jacobi SVD; the column of U of the smallest
 * singular value negated where det U V^T < 0), which also removes H's free scale.  focals: n_views doubles, R: n_views x 9 doubles row-major, info may be NULL.
 * MS_ERR_INVALID: a null pointer, n_views outside [2, MS_MAX_VIEWS], n_pairs outside [1, MS_MAX_VIEWS^2], a bad anchor or view index, a pair of a view with itself, a negative weight, a
 * non-finite or singular H, width or height < 1, a view the pairs do not connect to the anchor (the message names it). */
MS_API int ms_estimate_rig(int n_views, const ms_pair_homography *pairs, int n_pairs, int anchor, int width, int height, double *focals, double *R,
                           ms_rig_estimate_info *info);
/* anchor 0, per-view focals, 50 iterations, no Huber, step_tol 1e-10, 4 matches a pair */
MS_API int ms_rig_focal_default_params(ms_rig_focal_params *prm);
/* The normal equations of the contract above, per op: cost, H (4 n_views x 4 n_views row-major, view v at rows 4v .. 4v + 3, one focal a view, no view held) and g
 * (4 n_views) at the focals f (n_views) and rotations R (n_views x 9), every pair used whatever its size.  All pointers HOST.  Synchronises. */
MS_API int ms_rig_focal_accumulate(int n_views, const double *f, const double *R, const ms_rig_px_match *matches, int n, double huber_px, double *cost, double *H,
                                   double *g, ms_stream stream);
/* BundleAdjusterBase::estimate over focals and rotations, the whole loop on the device exactly as ms_refine_rig_rotations runs it: matches grouped by pair on the host
 * (stably), one pinned upload, max_iters + 1 rounds of two kernels with no host step in between, one copy back, one synchronise.  No floating-point atomics: two calls
 * on the same inputs return the same bits.  f_in / f_out: n_views doubles, R_in / R_out: n_views x 9 doubles, HOST; the anchor's R_out is bit-equal to its R_in; with
 * shared_focal every f_out is the same double; info may be NULL.
 * MS_ERR_INVALID, before the device is touched: a null pointer; n_views outside [2, MS_MAX_VIEWS]; n outside [1, 2^20]; a focal that is not finite or not positive;
 * with shared_focal, f_in that are not all equal; a rotation that is not finite or whose R R^T is off the identity by more than 1e-6 in an entry; a view index out
 * of range or view_a == view_b; a pixel that is not finite; a bad anchor; a struct_size mismatch; max_iters outside [1, 1000]; a negative or non-finite huber_px or
 * step_tol; min_pair_matches < 1; a view not connected to the anchor (the message names the first). */
MS_API int ms_refine_rig_cameras(int n_views, const double *f_in, const double *R_in, const ms_rig_px_match *matches, int n, const ms_rig_focal_params *prm,
                                 double *f_out, double *R_out, ms_rig_focal_info *info, ms_stream stream);
/* The context form, ms_refine_rig's with the focals free: the same per-view lists of projection-warped view pixels become camera rays by ms_warper_rays' arithmetic
 * with the context's CURRENT cameras, and a ray (x, y, z) becomes the centred pixel f_cur (x / z, y / z), f_cur = (double)K[0] of its view.  focal_out: num_views
 * doubles; R_out: num_views x 9 floats.  Nothing is applied: the caller sets K[0] = f and K[4] = f (old K[4] / K[0]) and runs the usual chain (ms_set_camera,
 * ms_build_maps, masks, ms_init_blender).  MS_ERR_STATE before ms_build_maps; MS_ERR_UNSUPPORTED for MS_MAPS_CUSTOM contexts (no cameras) and for lens contexts: a
 * warped pixel of a lens context carries the camera ray but not the source pixel, and the ray's pixel at ANOTHER focal lies at another distorted radius -- refining
 * a focal under a lens needs the inverse distortion, which this pinhole form does not apply: ms_refine_rig_focals_lens below does.  MS_ERR_INVALID as above, for a list that names its own view or a view out of
 * range, and for a ray with z <= 0 (behind the camera: it has no pixel), naming the match. */
MS_API int ms_refine_rig_focals(ms_ctx *ctx, const ms_mesh_match *matches, const int *match_count, const ms_rig_focal_params *prm, double *focal_out, float *R_out,
                                ms_rig_focal_info *info, ms_stream stream);
/* The lens form: the contract above with every view behind a FIXED lens (lenses: n_views ms_lens, HOST; per view, not unknowns; MS_LENS_NONE where a view has none).
 * detail::BundleAdjusterRay again; OpenCV has no counterpart that keeps distortion between the pixel and its ray.  Matches are ms_rig_px_match as above: pixels
 * centred on the principal point, y divided by the aspect ratio, so a view's distorted normalised coordinates are (xa / f, ya / f).  The 46 sums, Huber,
 * m = sqrt(f_i f_j), r = m (p - q), the Levenberg-Marquardt rule and the stop rules stay; two things generalise, with s = ln f:
 *   a      the unit ray of ms_lens_unproject at (xa / f_i, ya / f_i) through view i's lens, b the same for view j; p = R_i a, q = R_j b
 *   ci_k = 0.5 r_k + m (R_i da/ds_i)_k, cj_k = 0.5 r_k - m (R_j db/ds_j)_k, (R d)_k = R[3k] d0 + R[3k+1] d1 + R[3k+2] d2, where da/ds is
 *     NONE     a2 (e_z - a2 a): the view takes the pinhole contract's expressions for a and ci to the letter (ma = m a2, ci_k = 0.5 r_k + ma (R_i[3k+2] - a2 p_k)), so
 *              a call whose lenses are all NONE returns the bits of ms_rig_focal_accumulate / ms_refine_rig_cameras
 *     FISHEYE  e = (xd, yd) / theta_d, theta' = -theta_d / (d theta_d / d theta)(theta): da/ds = (theta' (cos theta e0), theta' (cos theta e1), -(theta' sin theta));
 *              0 at the centre
 *     BROWN    J the forward model's Jacobian at (x, y), (x', y') = -J^-1 (xd, yd) by Cramer's rule, n = sqrt(x^2 + y^2 + 1), t = a0 x' + a1 y':
 *              da/ds = ((x' - a0 t) / n, (y' - a1 t) / n, -(a2 t) / n)
 *   sin, cos, hypot and the last Newton round are not fixed to the bit: two implementations differ by the order of the sums and by those.
 * A match with a pixel its lens does not see at the TRIAL cameras adds +infinity to the cost and nothing to any other sum: the trial is rejected by the accept rule
 * (cost_trial <= cost fails), so every returned camera sees every match.  At the INPUT cameras such a pixel is MS_ERR_INVALID naming the match, found on the host
 * before the device is touched.  Both calls refuse what their pinhole forms refuse, and a lens ms_lens_check refuses; no floating-point atomics, two calls return
 * the same bits.  Stated limits: principal points are held in these two calls (ms_refine_rig_pp below frees them), and so are the lenses (ms_refine_rig_coeffs frees the coefficients of
 * a lens the whole rig shares); ms_estimate_rig stays pinhole, a lens rig starts from a nominal focal. */
MS_API int ms_rig_lens_accumulate(int n_views, const double *f, const double *R, const ms_lens *lenses, const ms_rig_px_match *matches, int n, double huber_px,
                                  double *cost, double *H, double *g, ms_stream stream);
MS_API int ms_refine_rig_cameras_lens(int n_views, const double *f_in, const double *R_in, const ms_lens *lenses, const ms_rig_px_match *matches, int n,
                                      const ms_rig_focal_params *prm, double *f_out, double *R_out, ms_rig_focal_info *info, ms_stream stream);
/* The context form for lens AND analytic contexts, what ms_refine_rig_focals is to pinhole ones: the same per-view lists of projection-warped view pixels become
 * camera rays by ms_warper_rays' arithmetic; a ray becomes its source pixel by the forward model (ms_lens_project's arithmetic, no inverse needed) with the view's
 * current camera and lens, centred: (px - K[2], (py - K[5]) K[0] / K[4]), evaluated as the model's pixel for the camera (K[0], 0, 0; K[0], 0) so that nothing is
 * rounded against the principal point; then ms_refine_rig_cameras_lens runs.  On an analytic context the result is ms_refine_rig_focals' bit for bit.  Nothing is
 * applied.  MS_ERR_STATE before ms_build_maps; MS_ERR_UNSUPPORTED for MS_MAPS_CUSTOM contexts and for a view with K[1] != 0; MS_ERR_INVALID as above and for a ray
 * its view's lens does not see, naming the match. */
MS_API int ms_refine_rig_focals_lens(ms_ctx *ctx, const ms_mesh_match *matches, const int *match_count, const ms_rig_focal_params *prm, double *focal_out, float *R_out,
                                     ms_rig_focal_info *info, ms_stream stream);
/* The coefficient form: the lens form above with ONE lens shared by all views (lens: one ms_lens of model BROWN or FISHEYE, HOST) and G of its k[] entries free,
 * 1 <= G <= 4, named by the bit mask free_coeffs (bit b frees k[b]).  FISHEYE: bits 0..3 (k1..k4).  BROWN: bits 0, 1, 4 (k1, k2, k3) and 2, 3 (p1, p2); bits 5..7, the
 * rational denominator, stay fixed (non-zero values are fine): a free one is MS_ERR_UNSUPPORTED.  It generalises ms_rig_lens_accumulate / ms_refine_rig_cameras_lens:
 * the residual, m = sqrt(f_i f_j), Huber, the 46 sums, the Levenberg-Marquardt rule and the stop rules are theirs, and the 46 sums of a pair are their bits.
 * Per match there are G more columns of the residual's Jacobian, one per free coefficient in ascending bit order, from the implicit-function theorem on the forward
 * model with the pixel and the focal held; with theta, e, (x, y), J, n, a as in the lens form and the trial lens's coefficients:
 *   FISHEYE  q_0 = theta (theta theta), q_n = q_(n-1) (theta theta) (= theta^(2n+3)), theta'_n = -q_n / (d theta_d / d theta)(theta):
 *            da/dk_n = (theta'_n (cos theta e0), theta'_n (cos theta e1), -(theta'_n sin theta)); 0 at the centre
 *   BROWN    r2 = x x + y y, D = 1 + ((k6 r2 + k5) r2 + k4) r2 (the fixed denominator), s = r2 / D for k1, (r2 r2) / D for k2, ((r2 r2) r2) / D for k3:
 *            dF = (x s, y s);  p1: dF = ((2 x) y, r2 + (2 y) y);  p2: dF = (r2 + (2 x) x, (2 x) y);
 *            (x', y') = -J^-1 dF by Cramer's rule: x' = -((J3 dF0 - J1 dF1) / det), y' = -((J0 dF1 - J2 dF0) / det), t = a0 x' + a1 y':
 *            da/dk_n = ((x' - a0 t) / n, (y' - a1 t) / n, -(a2 t) / n), the projection onto the sphere da/ds uses
 *   e_n,k = m (R_i da/dk_n)_k - m (R_j db/dk_n)_k, (R d)_k as above.
 * The border sums of a pair follow its 46, G + G (G + 1) / 2 + 8 G of them (46 for G = 4), in this order:
 *     g_n      sum w (e_n0 r0 + e_n1 r1 + e_n2 r2), n = 0 .. G - 1
 *     H_nn'    upper triangle row-major (00 01 .. 0(G-1) 11 ..): sum w (e_n0 e_n'0 + e_n1 e_n'1 + e_n2 e_n'2)
 *     then for n = 0 .. G - 1 eight sums: H(rot_i, n) = w (u x e_n)_k, k = 0 1 2;  H(f_i, n) = w (ci0 e_n0 + ci1 e_n1 + ci2 e_n2);
 *                                         H(rot_j, n) = -(w (v x e_n)_k);           H(f_j, n) = w (cj0 e_n0 + cj1 e_n1 + cj2 e_n2)
 * with the cross products written out as in g_i.  The solved system gets G rows after the existing ones (after the one focal where the focal is shared): 65 unknowns at
 * most.  The step is additive, k <- k + d; lambda diag(H) makes the scale of a coefficient irrelevant; step_tol is tested on max |.| over ALL components of the step.
 * A trial lens must stay a lens: ms_lens_check's profile rule (4096 samples on [0, max_theta]) is evaluated on the device for the trial coefficients, and a trial
 * that fails it is treated as a non-positive pivot is: lambda <- 10 lambda, one iteration, solve again.  The fisheye limit theta_d(max_theta) is the TRIAL lens's; a
 * pixel the trial lens no longer sees adds +infinity to the cost as above.  So every returned lens passes ms_lens_check and sees every match.
 * Stated limits: one lens a rig, at most 4 free coefficients, no denominators, no principal points (ms_refine_rig_pp, with the lenses fixed), no prior on the coefficients (a coefficient the matches do not
 * constrain -- rays near the axis only -- is held by the damping alone). */
typedef struct ms_rig_coeff_params {
    unsigned struct_size;          /* as ms_config: mismatch = MS_ERR_INVALID */
    int anchor_view;               /* the fields of ms_rig_focal_params, with its defaults ... */
    int shared_focal;
    int max_iters;
    double huber_px;
    double step_tol;
    int min_pair_matches;
    unsigned free_coeffs;          /* ... and the free entries of lens.k[], bit b for k[b]; default 1 (k1) */
} ms_rig_coeff_params;
typedef struct ms_rig_coeff_info {
    int iterations, stop_reason;   /* the fields of ms_rig_focal_info ... */
    double cost_initial, cost_final;
    int matches_used, pairs_used, pairs_ignored;
    int outliers;
    double max_rotation_rad;
    double max_focal_ratio;
    double max_coeff_change;       /* ... and the largest |k_out - k_in| over the free coefficients */
} ms_rig_coeff_info;
MS_API int ms_rig_coeff_default_params(ms_rig_coeff_params *prm);
/* The normal equations per op, ms_rig_lens_accumulate's with the coefficient rows last: H is (4 n_views + G)^2 row-major, g has 4 n_views + G entries.  The cost,
 * the leading 4 n_views x 4 n_views block and the first 4 n_views entries of g are the bits of ms_rig_lens_accumulate with `lens` on every view; free_coeffs == 0
 * (G = 0) is allowed here and returns exactly those.  Synchronises. */
MS_API int ms_rig_coeff_accumulate(int n_views, const double *f, const double *R, const ms_lens *lens, unsigned free_coeffs, const ms_rig_px_match *matches, int n,
                                   double huber_px, double *cost, double *H, double *g, ms_stream stream);
/* ms_refine_rig_cameras_lens with the shared lens's free coefficients among the unknowns: one pinned upload, max_iters + 1 rounds of two kernels, one copy back, one
 * synchronise; no floating-point atomics, two calls return the same bits.  lens_out is lens_in with the free entries replaced.  Refused before the device is touched:
 * everything ms_refine_rig_cameras_lens refuses (MS_ERR_INVALID), and a null lens, MS_LENS_NONE as the lens, free_coeffs empty or with more than 4 bits, a bit outside
 * the model's set (MS_ERR_INVALID; a BROWN denominator bit: MS_ERR_UNSUPPORTED), a pixel the input lens does not see (naming the match). */
MS_API int ms_refine_rig_coeffs(int n_views, const double *f_in, const double *R_in, const ms_lens *lens_in, const ms_rig_px_match *matches, int n,
                                const ms_rig_coeff_params *prm, double *f_out, double *R_out, ms_lens *lens_out, ms_rig_coeff_info *info, ms_stream stream);
/* The context form, built like ms_refine_rig_focals_lens: the lists become centred source pixels through the context's cameras and lens, then ms_refine_rig_coeffs
 * runs.  It needs a lens context whose views all hold the same model, coefficients and max_theta_deg: otherwise MS_ERR_UNSUPPORTED naming the first view that
 * differs (view 0 where it has no lens).  Nothing is applied: the caller runs ms_set_lens and the usual chain.  State errors and refusals as ms_refine_rig_focals_lens. */
MS_API int ms_refine_rig_coeffs_ctx(ms_ctx *ctx, const ms_mesh_match *matches, const int *match_count, const ms_rig_coeff_params *prm, double *focal_out, float *R_out,
                                    ms_lens *lens_out, ms_rig_coeff_info *info, ms_stream stream);
/* The centre form: the lens form above (every view behind a FIXED lens, one per view, MS_LENS_NONE where it has none) with each view's principal point among the
 * unknowns -- what detail::BundleAdjusterReproj (OCV/stitching/src/motion_estimators.cpp:329-511) estimates beside the focal (its ppx, ppy under the
 * refinement mask).  Matches are ms_rig_px_match as before: pixels centred on the NOMINAL principal point, y divided by the aspect ratio.  pp: n_views x 2 doubles (ox, oy), the
 * offset of the true centre from the point the pixels are centred on, in the same units.  View i's side of a match is the centred pixel (xa - ox_i, ya - oy_i), each
 * one subtraction; from there on the ray a, p = R_i a, m = sqrt(f_i f_j), r = m (p - q), Huber, the Levenberg-Marquardt rule and the stop rules are the lens form's,
 * and a pixel the lens does not see at the trial cameras and offsets adds +infinity to the cost and nothing to any other sum.
 * Six unknowns a view in the order (delta_0, delta_1, delta_2, s, ox, oy); the step of a centre is additive, o <- o + d.  With A = d a / d (xd, yd) at
 * (xd, yd) = pixel / f, da/dox = -(A[:,0]) / f and da/doy = -(A[:,1]) / f:
 *   NONE     n = sqrt(x x + y y + f f) (the pinhole contract's na):
 *            da/dox = (-((1 - a0 a0) / n), (a0 a1) / n, (a0 a2) / n),  da/doy = ((a0 a1) / n, -((1 - a1 a1) / n), (a1 a2) / n)       (= -((e_x - a0 a) / n), -((e_y - a1 a) / n))
 *   FISHEYE  A v = ((v . e) / slope) (cos theta e0, cos theta e1, -sin theta) + ((v . e^) sin theta / theta_d) (-e1, e0, 0), e^ = (-e1, e0), slope = d theta_d / d theta;
 *            with g = sin theta / theta_d, c0 = e0 / slope, c1 = e1 / slope, s0 = e1 g, s1 = e0 g:
 *            A[:,0] = (c0 (cos theta e0) + s0 e1, c0 (cos theta e1) - s0 e0, -(c0 sin theta)),  A[:,1] = (c1 (cos theta e0) - s1 e1, c1 (cos theta e1) + s1 e0, -(c1 sin theta));
 *            at the centre A is the first two columns of the identity.  da/dox = (-(A00 / f), -(A10 / f), -(A20 / f)), da/doy likewise
 *   BROWN    (x', y') is column c of J^-1 by Cramer's rule: (J3 / det, -(J2 / det)) for c = 0, (-(J1 / det), J0 / det) for c = 1; t = a0 x' + a1 y';
 *            A[:,c] = ((x' - a0 t) / n, (y' - a1 t) / n, -(a2 t) / n), the projection onto the sphere da/ds and da/dk use; da/dox, da/doy from A as for FISHEYE
 *   Residual columns: ex_i,k = m (R_i da/dox_i)_k and ey_i likewise, (R d)_k = R[3k] d0 + R[3k+1] d1 + R[3k+2] d2; for view j the columns are -(m (R_j db/dox_j)_k),
 *   -(m (R_j db/doy_j)_k).  With c_i = (ci, ex_i, ey_i) and c_j = (cj, -(m R_j db/dox_j), -(m R_j db/doy_j)) the three non-rotation columns of each view:
 * The 92 sums of a pair (RigSums<6>), x the cross product written out as in g_i, . the dot product x0 y0 + x1 y1 + x2 y2 left to right:
 *     cost  sum rho
 *     g_i   sum w (u x r)_k, k = 0 1 2;  then sum w (c_i[n] . r), n = 0 1 2          g_j   sum -(w (v x r)_k);  then sum w (c_j[n] . r)
 *     H_ii  symmetric, upper triangle row-major (00 01 .. 05 11 .. 15 22 .. 55): the rotation block of the 46 sums; (k, 3 + n): w (u x c_i[n])_k;
 *           (3 + n, 3 + n'), n <= n': w (c_i[n] . c_i[n'])
 *     H_jj  the same with v and c_j, its rotation-column entries negated: -(w (v x c_j[n])_k)
 *     H_ij  6 x 6 row-major (rows: view i): the rotation block of the 46 sums; (r, 3 + n): w (u x c_j[n])_r; (3 + n, c): -(w (v x c_i[n])_c);
 *           (3 + n, 3 + n'): w (c_i[n] . c_j[n'])
 *     outliers
 *   every product, sum, division and sqrt one IEEE operation in the order written.  The 46 sums among the 92 that involve only the rotations and the focals are the
 *   lens form's expressions in the lens form's summation order: they are THE BITS of ms_rig_lens_accumulate on matches whose pixels had the offsets subtracted in
 *   double beforehand.
 * The system: the anchor's rotation is held, its focal and centre are free; with per-view focals at most 6 * 16 - 3 = 93 unknowns; shared_focal folds the focal
 * rows and columns of all views into one (78 at most); the centres are always per view.  step_tol is tested on max |.| over ALL components of the step, the centre
 * components divided by the view's current focal first, so the test is in radians like the rest.
 * Prior: pp_prior is a weight w >= 0, 0 = none.  The refinement's cost is the data cost plus w sum_v ((ox_v - ox_in_v)^2 + (oy_v - oy_in_v)^2); the step kernel adds it
 * after the assembly, view after view: w onto the two diagonal entries, w (o - o_in) onto the two entries of g; accept and reject use the total cost.  w is
 * (match noise / centre tolerance)^2: with 0.5 px of match noise, w = 0.0025 holds a centre to about 10 px where the matches say nothing.  A ring of 4 views
 * constrains its centres weakly (they trade against the rotations); from 6 views on no prior is needed.
 * A warning the siblings share in principle and this form makes practical: r = m (p - q) with m = sqrt(f_i f_j) has a trivial minimum at f -> 0 (|p - q| <= 2).  From
 * a start inside the basin of the true cameras the loop never goes there, but free centres widen the ways out of a poor one: on sparse, partly false matches a
 * shared-focal run without Huber has walked to f ~ 1e-27 at a cost of 0.  The call does not judge its answer: check info.max_focal_ratio and max_pp_shift against
 * what the rig can be, select pairs by confidence before it as BundleAdjusterBase does, and give pp_prior where matches are few.
 * Stated limits: the lenses are fixed in this call (alternate it with ms_refine_rig_coeffs for a joint calibration; a joint form would carry about 154 sums a
 * pair); no aspect ratio or skew among the unknowns; no centre shared between views. */
typedef struct ms_rig_pp_params {
    unsigned struct_size;          /* as ms_config: mismatch = MS_ERR_INVALID */
    int anchor_view;               /* the fields of ms_rig_focal_params, with its defaults ... */
    int shared_focal;
    int max_iters;
    double huber_px;
    double step_tol;
    int min_pair_matches;
    double pp_prior;               /* ... and the weight of the prior on the centres; default 0 (none) */
} ms_rig_pp_params;
typedef struct ms_rig_pp_info {
    int iterations, stop_reason;   /* the fields of ms_rig_focal_info ... */
    double cost_initial, cost_final;   /* (with the prior's share) */
    int matches_used, pairs_used, pairs_ignored;
    int outliers;
    double max_rotation_rad;
    double max_focal_ratio;
    double max_pp_shift;           /* ... and the largest |o_out - o_in| over both components of every view, in pixels */
} ms_rig_pp_info;
/* anchor 0, per-view focals, 50 iterations, no Huber, step_tol 1e-10, 4 matches a pair, no prior */
MS_API int ms_rig_pp_default_params(ms_rig_pp_params *prm);
/* The normal equations of the centre form, per op (no counterpart in OpenCV, which differentiates calcError numerically: calcJacobian, motion_estimators.cpp:448-511):
 * cost, H ((6 n_views)^2 row-major, view v at rows 6v .. 6v + 5, no view held) and g (6 n_views) at the focals f, rotations R and offsets pp, every pair used
 * whatever its size, no prior.  lenses == NULL: every view is MS_LENS_NONE.  H is symmetric bit for bit.  All pointers HOST.  Synchronises. */
MS_API int ms_rig_pp_accumulate(int n_views, const double *f, const double *R, const double *pp, const ms_lens *lenses, const ms_rig_px_match *matches, int n,
                                double huber_px, double *cost, double *H, double *g, ms_stream stream);
/* detail::BundleAdjusterReproj's estimate with the centres free (BundleAdjusterBase::estimate, motion_estimators.cpp:223-326), on the ray residual of the lens form:
 * one pinned upload, max_iters + 1 rounds of two kernels, one copy back, one synchronise; no floating-point atomics, two calls return the same bits; the anchor's
 * R_out is its R_in's bits.  pp_in / pp_out: n_views x 2 doubles; lenses may be NULL (all NONE).  Refused before the device is touched: everything
 * ms_refine_rig_cameras_lens refuses, a non-finite offset, a negative or non-finite pp_prior, and a pixel its lens does not see at the input cameras AND offsets,
 * naming the match (all MS_ERR_INVALID). */
MS_API int ms_refine_rig_pp(int n_views, const double *f_in, const double *R_in, const double *pp_in, const ms_lens *lenses, const ms_rig_px_match *matches, int n,
                            const ms_rig_pp_params *prm, double *f_out, double *R_out, double *pp_out, ms_rig_pp_info *info, ms_stream stream);
/* The context form (BundleAdjusterReproj on a context's cameras): the lists become centred source pixels exactly as in ms_refine_rig_focals_lens, pp_in = 0, then
 * ms_refine_rig_pp runs.  pp_out: num_views x 2 doubles, the new K[2] and K[5] of each view: K[2] + ox and K[5] + oy K[4] / K[0].  focal_out: num_views doubles;
 * R_out: num_views x 9 floats.  Nothing is applied: the caller sets K and runs the usual chain (ms_set_camera, ms_build_maps, masks, ms_init_blender).  State errors
 * and refusals are ms_refine_rig_focals_lens': MS_ERR_STATE before ms_build_maps, MS_ERR_UNSUPPORTED for MS_MAPS_CUSTOM contexts and for a view with K[1] != 0. */
MS_API int ms_refine_rig_pp_ctx(ms_ctx *ctx, const ms_mesh_match *matches, const int *match_count, const ms_rig_pp_params *prm, double *focal_out, double *pp_out,
                                float *R_out, ms_rig_pp_info *info, ms_stream stream);

/* ---- Pairwise matching: every view pair of a rig in one call ---------------------------------------------------------------------------------------
 * detail::BestOf2NearestMatcher / BestOf2NearestRangeMatcher (OCV/stitching/src/matchers.cpp:248-297 the two-direction 2-NN match with ratio test and
 * cross-check, :692-770 the per-pair homography and confidence, :784-808 the candidate pairs), the stage of Stitcher::estimateCameraParams between
 * ms_orb_detect_and_compute and ms_estimate_rig; then leaveBiggestComponent (motion_estimators.cpp:1041-1097) and waveCorrect (:892-970), the two host
 * steps that turn its output into a connected, level rig.
 * Candidate pairs: every (i, j), i < j, with j < i + range_width where range_width > 0 and pair_mask[i * n_views + j] != 0 where pair_mask is given, in
 * lexicographic order; pairs_out lists them all.  A pair with an empty view is listed with count 0, no H and confidence 0 (the reference skips it and
 * leaves the default MatchesInfo).
 * The device stage, integers only but for one float compare, exact: for a pair (a, b) the two nearest rows of b for every row of a and of a for every
 * row of b, by ms_knn_match_hamming2's rule ((distance, index) order); a query whose train side has fewer than two rows yields nothing.  Ratio test:
 * t = 1.f - match_conf (one float subtraction); query q with nearest (j0, d0) and second (j1, d1) passes iff (float)d0 < t * (float)d1 (one float
 * multiply).  The pair's list: every passing row q of a, ascending, as (q, j0, d0) -- n_forward of them --, then every passing row q of b, ascending, as
 * (j0, q, d0) unless (j0, q) is already there, i.e. unless row j0 of a passed and its nearest row is q.  The order is part of the contract (the fixed
 * RANSAC subset sequence indexes into it).  Two launches whatever the number of pairs: the 2-NN of every row of every directed pair (a workgroup stages
 * tiles of train rows in LDS and scores 64 queries against each), then one workgroup a pair for ratio test, cross-check and an ordered prefix-scan
 * compaction (no atomics: two calls return the same bits); one upload, one copy back, one synchronise.
 * The host stage, two batched rounds of ms_find_homography_ransac_batch instead of up to two RANSAC calls a pair; per pair the rule is
 * BestOf2NearestMatcher::match line for line, and every field is what a ms_find_homography_ransac call on that pair alone gives.  Round 1 holds every pair with
 * count >= num_matches_thresh1: the matches' keypoints as centred floats (x - width * 0.5f, y - height * 0.5f) in list order (inlier flags, num_inliers, H;
 * no model: have_H = 0); |det H| < DBL_EPSILON: have_H stays 1, num_inliers = 0, confidence 0; otherwise confidence = num_inliers / (8 + 0.3 * count) in double,
 * a value above 3 becomes 0 (two views of the same image).  Round 2 holds every pair that passed the determinant test with num_inliers >= num_matches_thresh2:
 * a second RANSAC on the inliers alone replaces H (no model: have_H = 0; flags, count and confidence stay).  Below thresh1: have_H = 0, num_inliers = 0,
 * confidence 0, every inlier flag 0.  A round without a pair costs nothing.
 * Descriptors: 8UC1, the same length in every view, a multiple of 4 up to 64 bytes, data and step multiples of 4 (32 bytes is the specialised kernel);
 * these are checked on the views that have keypoints.
 * MS_ERR_INVALID before the device is touched: a null pointer; n_views outside [2, MS_MAX_VIEWS]; a struct_size mismatch; match_conf not finite or outside
 * [0, 1); a negative threshold or range_width; a descriptor type, length, step or alignment off the rule above or lengths that differ; n_keypoints negative,
 * above descriptors.rows or above MS_MATCH_MAX_KEYPOINTS; null keypoints or descriptors where n_keypoints > 0; keypoint_stride < 2; width or height < 1;
 * pairs_cap below the number of candidate pairs.  After the device stage: matches_cap below the total, with the needed total in *n_matches (and the
 * candidate count in *n_pairs), as ms_orb_detect_and_compute treats a short buffer. */
#define MS_MATCH_MAX_KEYPOINTS 32768
typedef struct ms_view_features {
    ms_image descriptors;          /* DEVICE 8UC1, rows >= n_keypoints (ORB hands back `cap` rows), cols = descriptor bytes */
    const float *keypoints;        /* HOST; row k starts at keypoints + k * keypoint_stride, x then y (ms_orb_detect_and_compute rows: stride 6) */
    int keypoint_stride, n_keypoints;
    int width, height;             /* ImageFeatures::img_size */
} ms_view_features;
typedef struct ms_pair_match_params {
    unsigned struct_size;          /* as ms_config: mismatch = MS_ERR_INVALID */
    float match_conf;              /* 0.3f (the ORB value of stitching_detailed) */
    int num_matches_thresh1;       /* 6 */
    int num_matches_thresh2;       /* 6 */
    int range_width;               /* 0: every pair i < j; k > 0: j < i + k (BestOf2NearestRangeMatcher) */
    const unsigned char *pair_mask;/* NULL or n_views x n_views, row-major, entry (i, j), i < j, non-zero = try the pair */
    double ransac_reproj_threshold; int ransac_max_iters; double ransac_confidence;   /* 0 = ms_find_homography_ransac's defaults */
} ms_pair_match_params;
typedef struct ms_feature_match { int query, train, distance, inlier; } ms_feature_match;   /* query in view_a, train in view_b */
typedef struct ms_pair_matches {
    int view_a, view_b;            /* view_a < view_b */
    int first, count;              /* this pair's slice of matches_out */
    int n_forward;                 /* how many of them came from the a -> b direction (they come first) */
    int num_inliers, have_H;
    double H[9];                   /* centred pixels of view_a -> centred pixels of view_b: ms_pair_homography's convention */
    double confidence;
} ms_pair_matches;
/* match_conf 0.3f, thresholds 6 and 6 (BestOf2NearestMatcher's defaults with the ORB match_conf of stitching_detailed), every pair, RANSAC defaults */
MS_API int ms_pair_match_default_params(ms_pair_match_params *prm);
MS_API int ms_match_pairs(int n_views, const ms_view_features *views, const ms_pair_match_params *prm,
                          ms_pair_matches *pairs_out, int pairs_cap, int *n_pairs,
                          ms_feature_match *matches_out, int matches_cap, int *n_matches, ms_stream stream);
/* The application's own matcher over an explicit list of directed problems: featurefinder::matchFeatures and matchFeaturesTemporal
 * (360_stitcher/featurefinder.cpp:48-108, :110-170) -- knnMatch(k = 2) in ONE direction, the 0.7 ratio test (:62-66), no cross-check, findHomography(RANSAC) on
 * every non-empty list (:68-90), confidence 1 (:106) -- where ms_match_pairs above is BestOf2NearestMatcher's rule.  One call serves the ring of lines 55-59, the
 * temporal list of lines 117-121, or both.
 * sets: a table of n_sets feature sets, n_sets in [1, 2 * MS_MAX_VIEWS] (one round's features and the previous round's fit in one table), ms_view_features with
 * ms_match_pairs' descriptor rules.  problems: n_problems in [0, MS_MATCH_MAX_PROBLEMS] pairs (query_set, train_set) of table indices; a problem may name any
 * two sets, the same set twice, and a problem may be repeated.  out: n_problems records -- view_a the query set, view_b the train set, first / count the slice of
 * matches_out in problem order, n_forward = count, confidence 1.0 always.
 * The result of problem p is what the per-pair route (ms_knn_match_hamming2, the ratio test, ms_find_homography_ransac) computes for that pair alone, bit for bit,
 * and depends neither on the problem's neighbours nor on its place in the list.  With fewer than 1 query row or fewer than 2 train rows the list is empty.
 * Otherwise, for every query row q in ascending order, with its two nearest train rows (j0, d0), (j1, d1) in ms_knn_match_hamming2's (distance, index) order: q
 * passes iff (double)d0 < ratio * (double)d1 (one double multiply, one compare; at 0.7 that is 10 d0 < 7 d1 for all distances up to 512: the boundary pairs
 * (7, 10), (14, 20), ... do not pass), and the list is the passing rows as (q, j0, d0).  The order is part of the contract (the fixed RANSAC subset sequence indexes
 * into it).  With find_homography every problem with count >= 1 gets what ms_find_homography_ransac returns on its own for the matches' keypoints as centred
 * floats (x - width * 0.5f, y - height * 0.5f), the mask zeroed first: H, the inlier flags, num_inliers, have_H = (status == 0).  find_homography 0: lists
 * only -- have_H 0, num_inliers 0, every flag 0.
 * Device stage, two launches whatever n_problems is, one upload, one copy back, one synchronise, over the calling thread's grow-only scratch: a problem is a
 * directed segment of ms_match_pairs' 2-NN kernel; then one workgroup a problem takes 256 queries a round through the ratio test and an ordered ballot /
 * prefix-scan compaction (no atomics: two calls return the same bytes).  Host stage: one ms_find_homography_ransac_batch round over the non-empty lists.
 * MS_ERR_INVALID before the device is touched: a null pointer; n_sets or n_problems out of range; a set index out of range; a struct_size mismatch; ratio not
 * finite or outside (0, 1]; the RANSAC parameter rules and the per-set rules of ms_match_pairs; a negative matches_cap.  After the device stage and before
 * RANSAC: matches_cap below the total, with the needed total in *n_matches.  n_problems == 0 is MS_OK with *n_matches = 0 and touches nothing. */
#define MS_MATCH_MAX_PROBLEMS 64
typedef struct ms_match_problem { int query_set, train_set; } ms_match_problem;
typedef struct ms_list_match_params {
    unsigned struct_size;          /* as ms_config: mismatch = MS_ERR_INVALID */
    double ratio;                  /* 0.7 (featurefinder.cpp:65) */
    int find_homography;           /* 1; 0 = lists only */
    double ransac_reproj_threshold; int ransac_max_iters; double ransac_confidence;   /* 0 = ms_find_homography_ransac's defaults */
} ms_list_match_params;
/* ratio 0.7, find_homography 1, RANSAC defaults (featurefinder.cpp:65, :90) */
MS_API int ms_list_match_default_params(ms_list_match_params *prm);
MS_API int ms_match_lists(int n_sets, const ms_view_features *sets, int n_problems, const ms_match_problem *problems,
                          const ms_list_match_params *prm, ms_pair_matches *out, ms_feature_match *matches_out,
                          int matches_cap, int *n_matches, ms_stream stream);
/* leaveBiggestComponent (motion_estimators.cpp:1041-1097).  Host only, no device.  The views are joined over the pairs with confidence >= conf_threshold;
 * keep receives the views of the largest component in ascending order (room for n_views), *n_keep their number.  Among components of equal size the one
 * that holds the lowest view index wins.  n_views in [1, MS_MAX_VIEWS]; pairs may be NULL where n_pairs is 0 (then keep is view 0 alone).
 * MS_ERR_INVALID: a null pointer, a negative n_pairs, a view index out of range, view_a == view_b, a conf_threshold that is not a number. */
MS_API int ms_biggest_component(int n_views, const ms_pair_matches *pairs, int n_pairs, double conf_threshold, int *keep, int *n_keep);
/* waveCorrect (motion_estimators.cpp:892-970) in double (the reference works in float).  Host only, no device.  R_in / R_out: n_views x 9 doubles row-major,
 * camera to rig; they may be the same array.  moment = sum over the views of x x^T, x a rotation's first column; its eigenvectors by cyclic Jacobi rotations,
 * eigenvalues in descending order as cv::eigen gives them; rg1 = the eigenvector of the smallest eigenvalue for MS_WAVE_HORIZ, of the largest for MS_WAVE_VERT;
 * rg0 = rg1 x (sum of the third columns), normalised; rg2 = rg0 x rg1; HORIZ: sum of rg0 . x < 0, VERT: sum of rg1 . x > 0 negates rg0 and rg1 (lines 936-956:
 * the result does not depend on the eigenvector's sign); R_out[v] = [rg0; rg1; rg2] R_in[v].  Returns 1 with R_out = R_in where |rg0| <= DBL_MIN or
 * n_views <= 1 (the reference returns without touching the rotations).  MS_ERR_INVALID: a null pointer, n_views outside [1, MS_MAX_VIEWS], another kind,
 * a rotation entry that is not finite. */
enum { MS_WAVE_HORIZ = 0, MS_WAVE_VERT = 1 };
MS_API int ms_wave_correct(int n_views, const double *R_in, int kind, double *R_out);

/* device-resident static tables, for parity tests: x_maps[i]/y_maps[i] (32FC1), masks (8UC1),
 * weight pyramid level (32FC1). Borrowed pointers owned by ctx. */
MS_API int ms_get_maps(const ms_ctx *ctx, int view, ms_image *xmap, ms_image *ymap);
MS_API int ms_get_mask(const ms_ctx *ctx, int view, ms_image *mask);
MS_API int ms_get_weight_level(const ms_ctx *ctx, int view, int level, ms_image *w);
MS_API int ms_get_mesh_maps(const ms_ctx *ctx, int view, ms_image *xmesh, ms_image *ymesh);

/* ms_stitch on the cameras' NV12 frames (APP/defs.h:10-17: the cameras deliver NV12; the capture threads run cvtColor(COLOR_YUV2BGR_NV12) per camera, networking.cpp:45-47):
 * views_nv12[f * num_views + i] = 8UC1, (src_height * 3 / 2) x src_width -- the Y plane followed by the interleaved UV plane -- every frame of a view with the same step.
 * The projection warp samples the planes itself and converts each bilinear tap with cvtColor's integer formula: bit-identical to ms_nv12_to_bgr_batch followed by
 * ms_stitch, without the BGR image (half the input bytes).  With CPW it is the first remap (stage 1) that samples the planes.  Frames that go through the per-frame
 * compose-scale resize first (timed.cpp:75-85) are converted with ms_nv12_to_bgr_batch, resized and stitched from BGR. */
MS_API int ms_stitch_nv12(ms_ctx *ctx, int n_frames, const ms_image *views_nv12, ms_image *out8u, ms_image *out16s, ms_stream stream);
/* Encoder-ready output: the panorama as planar I420, what consume() produces with cvtColor(BGR2YUV_I420) for the encoder (APP/timed.cpp:308-316),
 * written by the level-0 band kernel itself (no 8UC3 canvas, no conversion pass: 1.5 instead of 3 + 4.5 bytes per pixel of traffic).
 * out_i420[f]: contiguous 8UC1 image of (rows * 3 / 2) x out_width holding the canvas rows [first_row, first_row + rows) given by
 * ms_get_i420_rows (the even-aligned row span of the panorama ROI).  Only panorama pixels are written: initialise each buffer once to black
 * (Y = 16, U = V = 128; equals ms_bgr_to_i420 of a zeroed canvas).  Bit-identical to ms_stitch(out8u) + ms_bgr_to_i420 of those rows.
 * Needs the tiled band path (>= 1 band, panorama width a multiple of 8, no view sharding); MS_ERR_UNSUPPORTED otherwise. */
MS_API int ms_stitch_i420(ms_ctx *ctx, int n_frames, const ms_image *views, ms_image *out_i420, ms_stream stream);
/* Both at once: the cameras' NV12 frames in (APP/defs.h:10-17, networking.cpp:45-47), the encoder's planar I420 out (APP/timed.cpp:308-316) -- neither the BGR frames
 * nor the BGR canvas exist.  Inputs as ms_stitch_nv12, outputs as ms_stitch_i420 (same buffers, same ms_get_i420_rows span, initialise once to black); the same
 * kernels as those two calls (ms_get_stitch_kernels reports MS_WARP_KERNEL_NV12), under ms_set_active_views subsets, with CPW and up to 64 frames per call.
 * Bit-identical to ms_stitch_nv12(out8u) followed by ms_bgr_to_i420 of the I420 rows.  MS_ERR_UNSUPPORTED exactly where ms_stitch_nv12 or ms_stitch_i420 is
 * refused; the message names the condition that failed. */
MS_API int ms_stitch_nv12_i420(ms_ctx *ctx, int n_frames, const ms_image *views_nv12, ms_image *out_i420, ms_stream stream);
MS_API int ms_get_i420_rows(const ms_ctx *ctx, int *first_canvas_row, int *rows);
/* Pano-column sharding: the columns [*begin, *end) of the panorama ROI (= canvas columns [*begin + canvas_x, *end + canvas_x), ms_get_pano_geom) this
 * context composites; the whole ROI for an unsharded context.  Shard boundaries are multiples of 16 columns.  Valid after ms_init_blender. */
MS_API int ms_get_col_window(const ms_ctx *ctx, int *begin, int *end);
/* Bit v set = ms_stitch reads view v (always all views of an unsharded context; a column shard reads only the views that reach its window plus
 * halo; a view shard only the views it owns): the caller need not upload the others and may pass an all-zero ms_image for them. */
MS_API int ms_get_needed_views(const ms_ctx *ctx, unsigned *mask);

/* per-kernel GPU time of the last ms_stitch_timed call (hipEvents on `stream`), for bench.py's roofline.
 * names/ms: arrays of `cap` entries; returns the number of kernels recorded. */
MS_API int ms_stitch_timed(ms_ctx *ctx, int n_frames, const ms_image *views, ms_image *out8u, ms_image *out16s,
                           ms_stream stream, int cap, const char **names, float *ms);

/* Profiling aid: tuned streaming device-to-device copy (16 B per lane, four loads in flight, non-temporal) of a known byte count.
 * Calibrates the rocprofv3 FETCH_SIZE / WRITE_SIZE counters (tools/profile_traffic.sh) and is the measured bandwidth ceiling the
 * per-frame kernels are compared with (bench.py `ceiling`; no reference counterpart). */
MS_API int ms_calib_copy(const void *src, void *dst, size_t bytes, ms_stream stream);
/* ... and its read-only companion (the read side alone sustains more than a copy: the per-frame kernels read 3-5x what they write). */
MS_API int ms_calib_read(const void *src, size_t bytes, ms_stream stream);
/* Counter calibration on the access shapes of the per-frame kernels: every 128-byte line of `buf` is touched exactly once, so a launch moves `bytes` of HBM traffic
 * whatever the shape -- 0: one dword-aligned 12-byte read per lane at a 24-byte stride (k_warp_t's tap read), 1: one 8-byte read per lane (the band kernels' row
 * windows), 2: dword stores in 32-byte runs, four passes per line (k_warp_t's plane stores).  tools/profile_traffic.sh records what FETCH_SIZE / WRITE_SIZE report. */
MS_API int ms_calib_shape(void *buf, size_t bytes, int shape, ms_stream stream);

/* Self-test of the shared-reciprocal division used by the band kernels (normalizeUsingWeightKernel32F,
 * multiband_blend.cu:85-100 divides three channels by the same w + 1e-5): for each of the n HOST denominators,
 * all 65536 int16 numerators are divided both ways on the device; returns the number of results whose bits differ
 * from the compiler's correctly rounded a / d (expected 0), or a negative ms_status. */
MS_API int ms_selftest_divide(const float *denominators_host, int n, ms_stream stream);
/* The same comparison for EVERY float denominator in [d_lo, d_hi] (all bit patterns in between) x all 65536 int16 numerators, enumerated
 * on the device.  [1e-5, 64) -- every value a weight sum + 1e-5 of up to 16 views can take, with margin -- is 1.9e8 denominators = 1.2e13
 * quotients (tests/test_prims_gpu.py runs it: the proof by enumeration behind the bit-exactness of the normalise step). */
MS_API int ms_selftest_divide_range(float d_lo, float d_hi, unsigned long long *mismatches_out, unsigned long long *checked_out, ms_stream stream);

/* Self-test of the single-instruction saturate_cast<uchar>(float) (v_cvt_pk_u8_f32) used by the warp kernels: compares it with
 * the rint / clamp / NaN->0 definition over ALL 2^32 float bit patterns on the device; *mismatches_out must come back 0. */
MS_API int ms_selftest_cvt_u8(unsigned long long *mismatches_out, ms_stream stream);

/* =============================================================================================
 * 5. Virtual cameras: viewports, cube faces and re-levelled panoramas rendered from the panorama
 * =============================================================================================
 * The reference stops at the equirect: consume() ships it to a player that "place[s] the image correctly on the sphere" (APP/timed.cpp:296-300) and the
 * re-projection happens there.  These entry points do the player's step on the device: the direction "virtual camera pixel -> panorama pixel" as dense maps
 * (ms_build_view_maps: detail::{Spherical,Cylindrical}Projector::mapForward, OCV/stitching/include/opencv2/stitching/detail/warpers_inl.hpp:222-236, :258-273, behind
 * the inverse lens model of ms_lens_unproject), and a batched cuda::remap that wraps at the +-pi seam (ms_reproject).
 * Stated limits: 8UC3 panoramas only (no 16S source); INTER_LINEAR only (no nearest, no cubic); coordinates come from maps, except under a ROTATION that changes every
 * frame, which ms_reproject_poses renders without maps (a zoom or a lens that changes per frame still rebuilds them: ms_build_view_maps is one launch); MS_PROJ_PLANE panoramas are MS_ERR_UNSUPPORTED; one GPU.
 * Antialiasing: ms_reproject point-samples, as cuda::remap does -- right for a view as fine as the panorama, moire for a coarser one.  ms_reproject_aa is the
 * player's mip-mapped texture unit: ISOTROPIC trilinear over a per-call mip chain (ms_build_pano_mips), the level chosen per pixel from the view's footprint
 * (ms_build_view_footprint).  No anisotropic filtering, no cubic or Lanczos taps.  What that buys, measured on the numpy statement (tests/reproject_aa_ref.py, stripes
 * of period 3 panorama pixels on a 384 x 192 equirect, RMS error against an 8 x 8 supersample, relative to point sampling): 0.14 for a 24 x 14 viewport of 90
 * degrees (footprint 3.3-5.1 px), and 1.06 -- WORSE than point sampling -- for a 48 x 27 one (footprint 1.6-2.5): isotropic trilinear blurs a signal that lies barely
 * above the view's Nyquist rate, the known price of mip mapping.  footprint_scale is the caller's knob: below 1 it trades that blur for alias. */

/* How a panorama image lies on the warper surface: image pixel (x, y) is the warper coordinate (u0 + x, v0 + y) of a warper of `scale`. */
typedef struct ms_pano_frame {
    unsigned struct_size;   /* as ms_config: mismatch = MS_ERR_INVALID */
    int projection;         /* MS_PROJ_SPHERICAL or MS_PROJ_CYLINDRICAL; MS_PROJ_PLANE is MS_ERR_UNSUPPORTED */
    float scale;            /* the warper scale */
    int u0, v0;             /* warper coordinates of image pixel (0, 0) */
    int wrap_cols;          /* 0, or the image's column count where the image spans the full turn (column wrap_cols is column 0 again) */
    int clamp_rows;         /* 0 or 1: the image's first and last rows are the poles' (samples beyond them repeat the edge row) */
} ms_pano_frame;

/* A virtual camera.  R: view to rig, row-major, the convention of ms_set_camera (a rig direction is R times the view's ray). */
enum { MS_VIEW_CAMERA = 0, MS_VIEW_SURFACE = 1 };
typedef struct ms_view {
    unsigned struct_size;   /* as ms_config: mismatch = MS_ERR_INVALID */
    int kind;               /* MS_VIEW_CAMERA: a camera with K and a lens; MS_VIEW_SURFACE: a piece of a warper surface, e.g. the whole equirect under another rotation */
    int width, height;      /* [1, 32767] each */
    float R[9];
    float K[9];             /* CAMERA: intrinsics, as ms_lens_unproject takes them */
    ms_lens lens;           /* CAMERA: MS_LENS_NONE (also an all-zero struct) = pinhole; BROWN / FISHEYE as ms_lens_unproject: a virtual fisheye */
    int projection;         /* SURFACE: MS_PROJ_SPHERICAL or MS_PROJ_CYLINDRICAL */
    float scale;            /* SURFACE: its warper scale */
    int tl_u, tl_v;         /* SURFACE: warper coordinates of view pixel (0, 0) */
} ms_view;

/* One view of an ms_reproject call: its maps (DEVICE 32FC1 of one size -- that size is the view's --, data 4-byte aligned, step a multiple of 4) and where the view
 * goes in every destination frame. */
typedef struct ms_view_job {
    ms_image map_x, map_y;
    int dst_x, dst_y;
} ms_view_job;

/* A pan / tilt / zoom pinhole (host only, no device).  R = Ry(yaw) Rx(pitch) Rz(roll) with Ry(a) = [c 0 s; 0 1 0; -s 0 c], Rx(a) = [1 0 0; 0 c -s; 0 s c],
 * Rz(a) = [c -s 0; s c 0; 0 0 1]: yaw a degrees puts the optical axis at u = a scale (radians times scale) of the warper, positive pitch looks up, toward v = 0.
 * K: f = (width / 2) / tan(hfov / 2) on both axes, centre ((width - 1) / 2, (height - 1) / 2).  Computed in double, stored as float.  *out is filled completely
 * (struct_size, kind = MS_VIEW_CAMERA, lens MS_LENS_NONE).  MS_ERR_INVALID: a null pointer, an angle that is not finite, hfov_deg outside (0, 179], width or
 * height outside [1, 32767]. */
MS_API int ms_look_at_view(double yaw_deg, double pitch_deg, double roll_deg, double hfov_deg, int width, int height, ms_view *out);
/* Face `face` of a cube map of size x size faces: 0..5 = front, right, back, left, up, down = ms_look_at_view with (yaw, pitch) = (0, 0), (90, 0), (180, 0),
 * (-90, 0), (0, 90), (0, -90), roll 0, hfov 90: f = size / 2, c = (size - 1) / 2, pixel centres at half-integers of the face.  MS_ERR_INVALID: a null
 * pointer, face outside [0, 5], size outside [1, 32767]. */
MS_API int ms_cube_face_view(int face, int size, ms_view *out);

/* Where a context's output images lie on the warper surface (place_panorama's placement, read back).  MS_PANO_CANVAS: the out8u canvas -- u0 = -out_width / 2,
 * v0 = 0 (spherical) or -out_height / 2 (cylindrical), wrap_cols = out_width where 2 llrint(pi (double)scale) == out_width (else 0), clamp_rows = 1 for a
 * spherical canvas with out_height == llrint(pi (double)scale) (else 0).  MS_PANO_ROI: the pano ROI (out16s, out8u without a canvas): u0, v0 = dst_roi_final.x, .y,
 * no wrap, no clamp.  MS_ERR_STATE before ms_build_maps / ms_set_maps; MS_ERR_UNSUPPORTED for MS_PROJ_PLANE contexts and for the canvas of a context with
 * out_width == 0; MS_ERR_INVALID: a null pointer, another `which`. */
enum { MS_PANO_CANVAS = 0, MS_PANO_ROI = 1 };
MS_API int ms_get_pano_frame(const ms_ctx *ctx, int which, ms_pano_frame *out);

/* The backward maps of a view into a panorama image: map (x, y) = the panorama image coordinates view pixel (x, y) samples.  ONE launch, one lane per pixel;
 * everything in double and rounded to float once, at the store (calibration-time arithmetic, as ms_build_warp_maps_lens: no fp32 evaluation order is part of
 * the contract; tests/reproject_ref.py is the numpy statement).
 *   1. the view ray c of the integer pixel (x, y).  CAMERA: ms_lens_unproject's arithmetic on ((double)x, (double)y); not seen = the entry (-1, -1).
 *      SURFACE: the warper's backward direction (detail::*Projector::mapBackward, warpers_inl.hpp:238-255, :275-290) at U' = (double)(tl_u + x) / (double)scale,
 *      V' = (double)(tl_v + y) / (double)scale: spherical (sin V' sin U', -cos V', sin V' cos U'), cylindrical (sin U', V', cos U');
 *   2. the rig direction d_k = R[3k] c0 + R[3k+1] c1 + R[3k+2] c2 with (double)R, summed left to right;
 *   3. panorama coordinates (mapForward): h = hypot(d0, d2), S = (double)src->scale, U = S atan2(d0, d2); spherical V = S atan2(h, -d1) -- equal to
 *      SphericalProjector::mapForward's S (pi - acos(d1 / |d|)) and accurate at the poles, where acos is not; cylindrical V = S d1 / h, h == 0 = not seen;
 *   4. image coordinates X = U - u0, Y = V - v0; with wrap_cols > 0, X -= wrap_cols floor(X / wrap_cols), and a float result equal to wrap_cols is stored as 0.
 *      Without wrap X is stored as it is: ms_reproject turns what lies outside into black.
 * map_x / map_y: DEVICE 32FC1 of the view's size, any row step (pitched images, ROIs of larger ones).
 * Refused before the device is touched -- MS_ERR_INVALID: a null pointer, a struct_size mismatch, an unknown kind, maps that are not 32FC1 or not of the view's
 * size, a non-finite K (CAMERA), R or scale, a scale outside (0, 8192], a lens ms_lens_check refuses, K[0] or K[4] zero, wrap_cols < 0, clamp_rows other than 0 / 1,
 * width or height outside [1, 32767]; MS_ERR_UNSUPPORTED: MS_PROJ_PLANE as either projection. */
MS_API int ms_build_view_maps(const ms_pano_frame *src, const ms_view *view, ms_image *map_x, ms_image *map_y, ms_stream stream);

/* cuda::remap(src, dst, xmap, ymap, INTER_LINEAR, BORDER_CONSTANT, Scalar(0), stream) (OCV/cudawarping/src/remap.cpp:61-102) for n_frames panoramas and n_jobs
 * views in ONE launch, sampling a panorama that wraps: the job table travels in the kernel argument, nothing is allocated, the host never waits.
 *   src:  n_frames DEVICE 8UC3 panoramas of one size and one step (step < 2^24, rows * step < 2^32), any base address.
 *   dst:  n_frames DEVICE images of one geometry.  MS_VIEW_BGR: 8UC3, any step -- a job may write a rectangle of a larger atlas.  MS_VIEW_I420: contiguous 8UC1
 *         of (rows * 3 / 2) x cols, exactly as ms_bgr_to_i420's.
 *   jobs: HOST.  Job j writes the rectangle (dst_x, dst_y, map cols, map rows) of every frame; no byte outside the jobs' rectangles (I420: outside the three
 *         planes' sub-rectangles) is written.
 * Arithmetic.  The result equals, bit for bit, ms_remap(INTER_LINEAR, BORDER_CONSTANT) on the source extended by one column on either side and one row above and
 * below, with the maps shifted by (+1, +1) -- one fp32 addition per coordinate, which the kernel performs.  The extra columns hold columns cols - 1 and 0 of the
 * source when wrap_cols == cols, zeros otherwise; the extra rows then repeat rows 0 and rows - 1 (of the column-extended image) when clamp_rows is set, zeros
 * otherwise.  In words: taps, weights, the fma chain and the saturation are ms_remap's; a tap at column -1 or cols wraps, a tap at row -1 or rows repeats the
 * edge row, every other tap outside reads 0.  The maps may hold ANY float -- NaN, +-inf, +-1e30, the (-1, -1) marker (which, by the rule above, samples the
 * extension's corner pixel) --: the kernel writes what ms_remap writes and never forms an address outside the source.
 * MS_VIEW_I420 equals ms_bgr_to_i420 of the BGR atlas the call would have written: Y from every pixel, U and V from the top-left pixel of each 2 x 2 block.
 * Kernel shape (csrc/reproject.hip): a lane owns four pixels -- 4 x 1 of a row for BGR (12-byte stores), one 2 x 2 block for I420 --, builds their tap state
 * once from the maps and walks MS_VIEW_FRAME_GROUP frames with it; workgroups are tiles of MS_VIEW_TILE_W x MS_VIEW_TILE_H (BGR) / 32 x 32 (I420) pixels.
 * MS_ERR_INVALID, before a kernel is enqueued: a null pointer; n_frames outside [1, MS_VIEW_MAX_FRAMES] or n_jobs outside [1, MS_VIEW_MAX_JOBS]; an unknown
 * format; src frames that are not 8UC3, differ in geometry, have step >= 2^24 or rows * step >= 2^32; wrap_cols other than 0 or cols; clamp_rows other than
 * 0 / 1; a job whose maps differ in size, are not 32FC1 or are misaligned; dst frames of another type or differing in geometry; a rectangle that leaves dst;
 * two jobs whose rectangles overlap; for I420 an odd dst_x, dst_y, width, height or frame size, or a non-contiguous dst; a dst frame whose byte range
 * overlaps a src frame's. */
enum { MS_VIEW_BGR = 0, MS_VIEW_I420 = 1 };
enum { MS_VIEW_MAX_FRAMES = 64, MS_VIEW_MAX_JOBS = 16, MS_VIEW_FRAME_GROUP = 8, MS_VIEW_TILE_W = 64, MS_VIEW_TILE_H = 16 };
MS_API int ms_reproject(const ms_image *src, ms_image *dst, int n_frames, const ms_view_job *jobs, int n_jobs, int wrap_cols, int clamp_rows, int format,
                        ms_stream stream);

/* The packing of a panorama's mip chain (host only, no device) -- replaces the mip chain the player's GPU builds for the equirect texture it is handed
 * (APP/timed.cpp:296-300).  out[l - 1] describes level l = 1..levels of a cols x rows 8UC3 image: cols_l = (cols_{l-1} + 1) / 2, rows_l = (rows_{l-1} + 1) / 2,
 * pixel (x, y) at byte offset + y step + 3 x of the frame's buffer; *bytes is that buffer's size.  The levels do not overlap; every offset is a multiple of 256,
 * every step a multiple of 16 (>= 3 cols_l), and the buffer itself must be 16-byte aligned: the builder stores whole words, and level 3 is read back with aligned
 * wide loads when levels 4 and up are made.  Read the levels through this function only.  MS_ERR_INVALID: a null pointer, levels outside
 * [1, MS_VIEW_MAX_LEVELS], cols or rows outside [1, 32767]. */
enum { MS_VIEW_MAX_LEVELS = 6 };
typedef struct ms_mip_level { size_t offset, step; int cols, rows; } ms_mip_level;
MS_API int ms_pano_mips_layout(int cols, int rows, int levels, ms_mip_level *out, size_t *bytes);

/* The mip chains of n_frames panoramas -- replaces glGenerateMipmap's box filter in the player (APP/timed.cpp:296-300 hands the equirect to it).
 *   src:  n_frames DEVICE 8UC3 images of one geometry, as ms_reproject's src (any base address, step < 2^24, rows * step < 2^32), sides in [1, 32767].
 *   mips: HOST array of n_frames DEVICE buffers of ms_pano_mips_layout's *bytes bytes each, 16-byte aligned.
 * Arithmetic (integers, exact).  Level 0 is the source and is never copied.  Level l is made from the STORED bytes of level l - 1, per channel
 *   p_l(x, y) = (p(2x, 2y) + p(2x+1, 2y) + p(2x, 2y+1) + p(2x+1, 2y+1) + 2) >> 2,
 * an index past the last column or row of level l - 1 reading the last one.  No byte outside a level's cols_l x rows_l x 3 pixels is written (row padding and
 * the bytes between levels keep what they held).
 * Launches: ceil(levels / 3), whatever n_frames is -- a lane holds an 8 x 8 block of the source and finishes its level-1, -2 and -3 pixels in registers; levels
 * 4 to 6 are the same kernel on level 3 (csrc/reproject_aa.hip).  Nothing is allocated, the host never waits.
 * MS_ERR_INVALID, before the device is touched: a null pointer; n_frames outside [1, MS_VIEW_MAX_FRAMES]; levels outside [1, MS_VIEW_MAX_LEVELS]; src frames
 * that are not 8UC3, differ in geometry or break the limits above; a null or misaligned mips[f]; a mips buffer whose byte range overlaps a src frame's or
 * another mips buffer's.  No CPU fallback: MS_ERR_NO_DEVICE as elsewhere. */
MS_API int ms_build_pano_mips(const ms_image *src, void *const *mips, int n_frames, int levels, ms_stream stream);

/* The footprint of a view's pixels in the panorama -- replaces the derivative the player's texture unit takes per fragment to choose a mip level.  rho(x, y) is
 * the side, in level-0 panorama pixels, of the patch view pixel (x, y) covers.  Calibration-time work like ms_build_view_maps: ONE launch, one lane per pixel,
 * everything in double and rounded to float once, at the store; tests/reproject_aa_ref.py is the numpy statement.
 *   An entry is UNSEEN when both maps hold exactly -1 or either value is not finite; rho of an unseen pixel is 0, an unseen neighbour counts as absent.
 *   a = E(x+1, y) - E(x, y) with E = ((double)map_x, (double)map_y); E(x, y) - E(x-1, y) where the forward neighbour is absent (outside the maps, or unseen);
 *   (0, 0) where both are.  b likewise along y.
 *   Wrap: with W = src->wrap_cols > 0 the x component d of each difference becomes d - W floor(d / W + 0.5).
 *   Spherical weight: for a spherical src the x components are then multiplied by s = sin(min(max((Y + v0) / S, 0), pi)), Y = map_y(x, y), S = (double)src->scale;
 *   a cylindrical src has s = 1.  An equirect row at polar angle theta holds 1 / sin(theta) columns per unit of angle: a step of many columns near a pole is a
 *   small step on the sphere, and the panorama there is band-limited in angle, not in columns.  Without the weight every "up" or "down" view would be blurred to
 *   the coarsest level.
 *   rho = footprint_scale max(hypot(a), hypot(b)).  footprint_scale in (0, 16]; 1 is neutral, below 1 trades blur for alias (section 5's head).
 * map_x / map_y / rho: DEVICE 32FC1 of one size, any row step, data and step 4-byte aligned.
 * MS_ERR_INVALID, before the device is touched: a null pointer; ms_build_view_maps' checks on src (struct_size, projection, scale, wrap_cols, clamp_rows); maps
 * or rho that are not 32FC1, not of one size or misaligned; a footprint_scale that is not finite or lies outside (0, 16].  MS_ERR_UNSUPPORTED: MS_PROJ_PLANE. */
MS_API int ms_build_view_footprint(const ms_pano_frame *src, const ms_image *map_x, const ms_image *map_y, double footprint_scale, ms_image *rho, ms_stream stream);

/* ms_reproject with the player's trilinear, mip-mapped texture lookup (APP/timed.cpp:296-300: the equirect goes to a player whose GPU samples it so) in place of
 * the point sample: n_frames panoramas and n_jobs views in ONE launch, the job table in the kernel argument, exactly like ms_reproject.
 *   src, dst, wrap_cols, clamp_rows, format: as ms_reproject's.  mips: HOST array of n_frames DEVICE buffers, ms_build_pano_mips' of the same src and levels.
 *   jobs: HOST; job, as ms_reproject's, and rho: DEVICE 32FC1 of the maps' size (ms_build_view_footprint's, or any float -- see below).
 * Arithmetic per pixel, all fp32.  (X, Y) the map entry, r = rho, L = levels.
 *   Level: !(r > 1) (NaN, zero and negatives included): l = 0, t = 0.  Else r >= 2^L: l = L, t = 0.  Else l = floor(log2 r), read from the float's exponent
 *   field, and t = fmaf(r, 2^-l, -1.0f) -- exact, 0 <= t < 1.
 *   Coordinates at level k: X_k = fmaf(X, 2^-k, 2^-(k+1) - 0.5f), Y_k likewise (the constants are exact: one rounding each; level 0 keeps X, Y).
 *   C_k[c] is the UNSATURATED fp32 fma chain of ms_reproject run on image level k (level 0 = src) at (X_k, Y_k): the +1 shift and the extended-source rule with
 *   that level's cols_k, rows_k; the level wraps iff wrap_cols != 0 and clamps iff clamp_rows is set.
 *   o[c] = fmaf(t, C_{l+1}[c] - C_l[c], C_l[c]), stored through ms_remap's saturation; where t == 0 level l + 1 is not read and o[c] = C_l[c].
 * Consequences: a job whose rho is at most 1 everywhere is ms_reproject's output, bit for bit; MS_VIEW_I420 equals ms_bgr_to_i420 of the BGR atlas the call would
 * have written; the maps and rho may hold ANY float and no address outside the source or a level is ever formed.
 * Kernel shape (csrc/reproject_aa.hip): ms_reproject's -- a lane owns four pixels, builds their two tap states once and walks MS_VIEW_FRAME_GROUP frames with them;
 * a wave whose pixels all stay on level 0 takes ms_reproject's one-level loop.
 * MS_ERR_INVALID, before a kernel is enqueued: everything ms_reproject refuses; a null mips; levels outside [1, MS_VIEW_MAX_LEVELS]; a null or misaligned mips[f];
 * src sides outside [1, 32767]; wrap_cols != 0 with cols no multiple of 2^levels (the coarse level would not close the turn); a rho that is not 32FC1 of the
 * maps' size or is misaligned; a dst frame whose byte range overlaps a mips buffer's. */
typedef struct ms_view_job_aa { ms_view_job job; ms_image rho; } ms_view_job_aa;
MS_API int ms_reproject_aa(const ms_image *src, void *const *mips, int levels, ms_image *dst, int n_frames, const ms_view_job_aa *jobs, int n_jobs, int wrap_cols,
                           int clamp_rows, int format, ms_stream stream);

/* ms_reproject for a camera that MOVES: n_frames panoramas and n_jobs views in ONE launch, every frame under a rotation of its own, the coordinates computed in
 * the kernel -- no maps are built, stored or read, and the host stays out of the loop.
 *   frame:     how the src images lie on the warper surface, as ms_build_view_maps takes it; frame->wrap_cols must be 0 or the source's column count.
 *   src, dst, format: as ms_reproject's.
 *   jobs:      HOST, n_jobs in [1, MS_VIEW_POSE_MAX_JOBS].  view: as ms_build_view_maps takes it (kind, size, K, lens / projection, scale, tl_u, tl_v) -- view.R is
 *              read by ms_view_pose_table only; job j writes the rectangle (dst_x, dst_y, view.width, view.height) of every frame.
 *   poses_dev: DEVICE, 4-byte aligned, n_jobs * n_frames * 9 floats: the rotation (view to rig, row-major, ms_set_camera's convention) of job j in frame f starts
 *              at poses_dev[(j * n_frames + f) * 9].  On the device because 8 x 64 x 36 bytes do not fit a kernel argument, and because a stabiliser or a
 *              pose filter may well produce the table there: nothing is allocated or copied by the call, the host never waits.
 * Contract, bit for bit.  Frame f, job j gets exactly the bytes that ms_build_view_maps(frame, view_j with R = that frame's nine floats) followed by
 * ms_reproject(&src[f], &dst[f], 1, {those maps, dst_x, dst_y}, 1, frame->wrap_cols, frame->clamp_rows, format) writes: steps 1 to 4 of ms_build_view_maps in
 * double, rounded to float once, then ms_reproject's taps, weights, fma chain and saturation -- the wrap rule and the == wrap_cols -> 0 rule, the (-1, -1) entry
 * of an unseen pixel (which samples the extension's corner), I420 as ms_bgr_to_i420 of the BGR atlas.  No byte outside the jobs' rectangles is written.
 * The host cannot inspect the rotations: ANY nine floats -- NaN, +-inf, zeros, a matrix scaled by 1e30 -- give what the formulas above give for them (the
 * two-call route where ms_build_view_maps accepts the matrix), and no address outside the source is ever formed: the taps are made from the two floats alone.
 * Kernel shape (csrc/reproject_poses.hip): ms_reproject's tiles and lanes.  A lane builds the view rays of its four pixels once -- ms_lens_unproject's Newton
 * solves, the dear part of a lens view -- and walks MS_VIEW_POSE_FRAME_GROUP frames with them; per frame and pixel it rotates the ray and evaluates one hypot
 * and two atan2 in double.
 * Stated limits: rotations only (a zoom or a lens that changes per frame still rebuilds maps); point sampling only -- there is no _aa form, the footprint depends
 * on the pose; MS_VIEW_POSE_MAX_JOBS jobs; 8UC3 sources; one GPU.
 * Refused before the device is touched -- MS_ERR_INVALID: a null pointer; a struct_size mismatch; everything ms_build_view_maps refuses about frame and about
 * each view except a non-finite view.R; frame->wrap_cols other than 0 or the source's columns; everything ms_reproject refuses about src, dst, n_frames, format,
 * rectangles that leave dst or overlap, I420 parity and dst overlapping src; n_jobs outside [1, MS_VIEW_POSE_MAX_JOBS]; a misaligned poses_dev.
 * MS_ERR_UNSUPPORTED: MS_PROJ_PLANE as either projection. */
enum { MS_VIEW_POSE_MAX_JOBS = 8, MS_VIEW_POSE_FRAME_GROUP = 8 };   /* a cube map is 6 jobs */
typedef struct ms_view_pose_job {
    ms_view view;
    int dst_x, dst_y;       /* as ms_view_job's */
} ms_view_pose_job;
MS_API int ms_reproject_poses(const ms_pano_frame *frame, const ms_image *src, ms_image *dst, int n_frames, const ms_view_pose_job *jobs, int n_jobs,
                              const float *poses_dev, int format, ms_stream stream);

/* The pose table of "these views, under the rig rotation P_f in frame f" (host only, no device): poses_host[(j * n_frames + f) * 9 + i] =
 * (float)(P_f (double)jobs[j].view.R)[i], row-major 3 x 3 products, each summed left to right in double.  rig_poses: n_frames x 9 doubles, row-major, or NULL
 * for the identity: every frame then gets view.R itself.  Upload the result and hand it to ms_reproject_poses.
 * MS_ERR_INVALID: a null jobs or poses_host; n_jobs outside [1, MS_VIEW_POSE_MAX_JOBS]; n_frames outside [1, MS_VIEW_MAX_FRAMES]; a view's struct_size
 * mismatch; a view.R or rig_poses entry that is not finite. */
MS_API int ms_view_pose_table(const ms_view_pose_job *jobs, int n_jobs, const double *rig_poses, int n_frames, float *poses_host);

#ifdef __cplusplus
}
#endif
#endif /* MS_STITCH_H */
