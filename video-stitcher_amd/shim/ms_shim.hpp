// ms_shim.hpp -- thin C++ shim over the C-ABI (include/ms_stitch.h) that re-exposes the reference's call
// surface: cv::cuda::-style free functions on any GpuMat-like type and a MultiBandBlender-style compositor
// object, so that 360_stitcher/timed.cpp / calibration.cpp style callers change an include and a namespace.
//
// "GpuMat-like" = anything with  data, step, rows, cols, type()  (cv::cuda::GpuMat qualifies unchanged:
// sources/modules/core/include/opencv2/core/cuda.hpp:283-303).  Header-only, no OpenCV dependency.
// Errors become exceptions here (the reference throws cv::Exception), never across the C boundary.
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../include/ms_stitch.h"

namespace msshim {

struct Error : std::runtime_error { int code; Error(int c, const char *m) : std::runtime_error(m), code(c) {} };
inline void check(int rc) { if (rc < 0) throw Error(rc, ms_last_error()); }

template <class Mat> inline ms_image wrap(const Mat &m)
{
    return ms_image{(void *)m.data, (size_t)m.step, m.cols, m.rows, m.type()};
}

// ---- cv::cuda:: free functions (dst must be pre-created, as GpuMat::create would) ------------------------
namespace cuda {
template <class Mat> void remap(const Mat &src, Mat &dst, const Mat &xmap, const Mat &ymap, int interpolation, int borderMode = MS_BORDER_CONSTANT, ms_stream s = nullptr)
{ ms_image a = wrap(src), x = wrap(xmap), y = wrap(ymap), d = wrap(dst); check(ms_remap(&a, &x, &y, &d, interpolation, borderMode, s)); }
template <class Mat> void resize(const Mat &src, Mat &dst, double fx, double fy, ms_stream s = nullptr)
{ ms_image a = wrap(src), d = wrap(dst); check(ms_resize_linear(&a, &d, fx, fy, s)); }
// every view of a frame in one launch (the loop of cuda::resize calls of stitch_online, timed.cpp:75-85)
template <class Mat> void resize(const std::vector<Mat> &src, std::vector<Mat> &dst, double fx, double fy, ms_stream s = nullptr)
{
    std::vector<ms_image> a(src.size()), d(dst.size());
    for (size_t i = 0; i < src.size(); ++i) { a[i] = wrap(src[i]); d[i] = wrap(dst[i]); }
    check(ms_resize_linear_batch(a.data(), d.data(), (int)src.size(), fx, fy, s));
}
// the same for cameras that deliver NV12 (defs.h:10-17): cvtColor(YUV2BGR_NV12) (networking.cpp:45-47) + that resize in one pass from the planes; src[i] = 8UC1 (rows * 3 / 2) x cols
template <class Mat> void resize_nv12(const std::vector<Mat> &src_nv12, std::vector<Mat> &dst, double fx, double fy, ms_stream s = nullptr)
{
    std::vector<ms_image> a(src_nv12.size()), d(dst.size());
    for (size_t i = 0; i < src_nv12.size(); ++i) { a[i] = wrap(src_nv12[i]); d[i] = wrap(dst[i]); }
    check(ms_nv12_resize_linear_batch(a.data(), d.data(), (int)src_nv12.size(), fx, fy, s));
}
template <class Mat> void copyMakeBorder(const Mat &src, Mat &dst, int top, int bottom, int left, int right, int borderType, ms_stream s = nullptr)
{ ms_image a = wrap(src), d = wrap(dst); check(ms_copy_make_border(&a, &d, top, bottom, left, right, borderType, s)); }
template <class Mat> void pyrDown(const Mat &src, Mat &dst, ms_stream s = nullptr)
{ ms_image a = wrap(src), d = wrap(dst); check(ms_pyr_down(&a, &d, s)); }
template <class Mat> void pyrUp(const Mat &src, Mat &dst, ms_stream s = nullptr)
{ ms_image a = wrap(src), d = wrap(dst); check(ms_pyr_up(&a, &d, s)); }
template <class Mat> void subtract(const Mat &a, const Mat &b, Mat &dst, ms_stream s = nullptr)
{ ms_image x = wrap(a), y = wrap(b), d = wrap(dst); check(ms_subtract_16s(&x, &y, &d, s)); }
template <class Mat> void add(const Mat &a, const Mat &b, Mat &dst, ms_stream s = nullptr)
{ ms_image x = wrap(a), y = wrap(b), d = wrap(dst); check(ms_add_16s(&x, &y, &d, s)); }
template <class Mat> void convertTo(const Mat &src, Mat &dst, double alpha = 1.0, ms_stream s = nullptr)
{
    ms_image a = wrap(src), d = wrap(dst);
    check(a.type == d.type ? ms_convert_scale_8u(&a, &d, alpha, s) : ms_convert(&a, &d, alpha, s));
}
}  // namespace cuda

// device::blend launchers (blenders.cpp:48-61)
template <class Mat> void addSrcWeightGpu32F(const Mat &src, const Mat &w, Mat &dst, Mat &dst_w, int rc_w, int rc_h, ms_stream s = nullptr)
{ ms_image a = wrap(src), b = wrap(w), d = wrap(dst), e = wrap(dst_w); check(ms_add_src_weight_32f(&a, &b, &d, &e, rc_w, rc_h, s)); }
template <class Mat> void normalizeUsingWeightMapGpu32F(const Mat &w, Mat &src, int width, int height, ms_stream s = nullptr)
{ ms_image a = wrap(w), d = wrap(src); check(ms_normalize_using_weight_32f(&a, &d, width, height, s)); }
// consume()'s resize + black bars + cvtColor(BGR2YUV_I420) (timed.cpp:251-316) in one pass; i420: contiguous 8UC1 (out_h * 3 / 2) x out_w.  Returns image_height.
template <class Mat> int consume_i420(const Mat &pano8u, Mat &i420, int out_w, int out_h, bool keep_aspect_ratio = true, ms_stream s = nullptr)
{
    ms_image a = wrap(pano8u), b = wrap(i420);
    int ih = 0;
    check(ms_consume_i420(&a, &b, out_w, out_h, keep_aspect_ratio ? 1 : 0, &ih, s));
    return ih;
}

// custom_resize (APP/calibration.h:15)
template <class Mat> void custom_resize(const Mat &in, Mat &out, ms_stream s = nullptr)
{ ms_image a = wrap(in), d = wrap(out); check(ms_custom_resize_32f(&a, &d, s)); }

// ---- the compositor: stitch_calib tables + stitch_one ----------------------------------------------------------
class Compositor {
public:
    // num_bands as MultiBandBlender(try_gpu, num_bands); projection MS_PROJ_CYLINDRICAL is what calibration.cpp:100 ships
    Compositor(int num_views, int src_w, int src_h, int projection, float warp_scale, int num_bands, bool enable_local,
               int out_w, int out_h, int frames_in_flight = 1, int update_mask_margin = 0)
    {
        ms_config c{};
        c.update_mask_margin = update_mask_margin;      // > 0: update_mask() only enqueues (timed.cpp:598-605 could call it after every mesh swap)
        c.struct_size = (unsigned)sizeof(ms_config);
        c.num_views = num_views; c.src_width = src_w; c.src_height = src_h; c.projection = projection; c.warp_scale = warp_scale;
        c.num_bands = num_bands; c.enable_cpw = enable_local; c.out_width = out_w; c.out_height = out_h; c.max_frames = frames_in_flight;
        check(ms_create(&c, &ctx_));
        n_ = num_views;
    }
    ~Compositor() { ms_destroy(ctx_); }
    Compositor(const Compositor &) = delete;
    Compositor &operator=(const Compositor &) = delete;

    // calibrateCameras + warpImages (calibration.cpp:28-248): K, R are the 3x3 CV_32F matrices of cameras[i]
    void setCamera(int i, const float *K, const float *R) { check(ms_set_camera(ctx_, i, K, R)); }
    void setGain(int i, double g) { check(ms_set_gain(ctx_, i, g)); }                 // gc->gains()[i]
    // cameras[i]'s distortion (cvProjectPoints2's distCoeffs / cv::fisheye::projectPoints' D): with a lens on any view buildMaps / calibrateSeam go through the lens model
    void setLens(int i, const ms_lens *lens) { check(ms_set_lens(ctx_, i, lens)); }   // nullptr clears it
    void buildMaps(ms_stream s = nullptr) { check(ms_build_maps(ctx_, s)); }          // gpu_warper->buildMaps + blender->prepare
    // ... or the caller's own x_maps / y_maps (what stitch_online receives, timed.cpp:56, :84-90) with the corners / sizes prepare() gets: any lens model or third-party
    // calibration; no setCamera needed.  The maps are copied.  calibrate_seam / save_tables are refused on such a context (they need cameras).
    template <class Mat> void setMaps(const std::vector<ms_rect> &rois, const std::vector<Mat> &x_maps, const std::vector<Mat> &y_maps, ms_stream s = nullptr)
    {
        if ((int)rois.size() != n_ || (int)x_maps.size() != n_ || (int)y_maps.size() != n_) throw Error(MS_ERR_INVALID, "setMaps: one ROI and one pair of maps per view");
        std::vector<ms_image> x, y;
        for (int i = 0; i < n_; ++i) { x.push_back(wrap(x_maps[i])); y.push_back(wrap(y_maps[i])); }
        check(ms_set_maps(ctx_, rois.data(), x.data(), y.data(), s));
    }
    bool customMaps() const { int src = MS_MAPS_ANALYTIC; check(ms_get_map_source(ctx_, &src)); return src == MS_MAPS_CUSTOM; }
    int mapSource() const { int src = MS_MAPS_ANALYTIC; check(ms_get_map_source(ctx_, &src)); return src; }      // MS_MAPS_ANALYTIC / _CUSTOM / _LENS
    void buildMasks(bool voronoi_seams = true, ms_stream s = nullptr) { check(ms_build_masks(ctx_, voronoi_seams ? 1 : 0, s)); }
    // what calibrateSeam cuts with (seam_finder->find, calibration.cpp:134-135): MS_SEAM_VORONOI as the reference, or MS_SEAM_DP, a minimum-cost seam through the warped images
    void setSeamFinder(int finder) { check(ms_set_seam_finder(ctx_, finder)); }
    int seamFinder() const { int f = MS_SEAM_VORONOI; check(ms_get_seam_finder(ctx_, &f)); return f; }
    void setMask(int i, const uint8_t *host_mask, size_t step) { check(ms_set_mask(ctx_, i, host_mask, step)); }
    void init_gpu(ms_stream s = nullptr) { check(ms_init_blender(ctx_, s)); }         // mb->init_gpu for every view
    void update_mask(int img_num, ms_stream s = nullptr) { check(ms_update_mask(ctx_, img_num, s)); }   // mb->update_mask(idx, x_mesh, y_mesh): uses the view's active mesh
    // camera dropout (no reference counterpart: timed.cpp exits when a camera fails): composite only the views whose bit is set, from the next stitch on
    void setActiveViews(unsigned mask, ms_stream s = nullptr) { check(ms_set_active_views(ctx_, mask, s)); }
    // exposure tracking (no reference counterpart: GainCompensator::feed runs once, calibration.cpp:131-132): re-estimate the gains from one live frame set on `s`;
    // enqueue-only, the next stitch_one on `s` uses them.  stride / smoothing <= 0: the library's starting values
    template <class Mat> void trackGains(const std::vector<Mat> &full_imgs, int stride = 0, double smoothing = 0, ms_stream s = nullptr)
    {
        ms_gain_track_params prm;
        check(ms_gain_track_default_params(&prm));
        if (stride > 0) prm.stride = stride;
        if (smoothing > 0) prm.smoothing = smoothing;
        std::vector<ms_image> v;
        for (const Mat &m : full_imgs) v.push_back(wrap(m));
        if ((int)v.size() != n_) throw Error(MS_ERR_INVALID, "trackGains: one image per view");
        check(ms_track_gains(ctx_, v.data(), &prm, s));
    }
    // ... from the cameras' NV12 frames (8UC1, (rows * 3 / 2) x cols): the same statistic and gain state, no BGR copy
    template <class Mat> void trackGainsNv12(const std::vector<Mat> &nv12_imgs, int stride = 0, double smoothing = 0, ms_stream s = nullptr)
    {
        ms_gain_track_params prm;
        check(ms_gain_track_default_params(&prm));
        if (stride > 0) prm.stride = stride;
        if (smoothing > 0) prm.smoothing = smoothing;
        std::vector<ms_image> v;
        for (const Mat &m : nv12_imgs) v.push_back(wrap(m));
        if ((int)v.size() != n_) throw Error(MS_ERR_INVALID, "trackGainsNv12: one image per view");
        check(ms_track_gains_nv12(ctx_, v.data(), &prm, s));
    }
    std::vector<double> gains(ms_stream s = nullptr)       // gc->gains() as the next stitch on `s` uses them (waits for `s`)
    {
        std::vector<double> g((size_t)n_);
        check(ms_get_gains(ctx_, g.data(), nullptr, nullptr, s));
        return g;
    }
    // MeshWarper::convertMeshesToMap (meshwarper.cpp:823): callable from the recalibration thread
    void convertMeshToMap(int i, const float *mesh_x, const float *mesh_y, int N, int M, ms_stream s = nullptr)
    { check(ms_set_mesh(ctx_, i, mesh_x, mesh_y, N, M, s)); }
    // ... and for all views at once, as MeshWarper::convertMeshesToMap itself loops over the images: num_views meshes of N x M back to back, two launches in all
    void convertMeshesToMap(const float *mesh_x, const float *mesh_y, int N, int M, ms_stream s = nullptr) { check(ms_set_meshes(ctx_, mesh_x, mesh_y, N, M, s)); }

    // stitch_one (timed.cpp:123-152): full_imgs = the NUM_IMAGES uploaded frames; out = caller-owned ring slot
    template <class Mat> void stitch_one(const std::vector<Mat> &full_imgs, Mat *out8u, Mat *out16s, ms_stream s = nullptr)
    {
        std::vector<ms_image> v;
        for (const Mat &m : full_imgs) v.push_back(wrap(m));
        ms_image o8{}, o16{};
        if (out8u) o8 = wrap(*out8u);
        if (out16s) o16 = wrap(*out16s);
        check(ms_stitch(ctx_, (int)(v.size() / n_), v.data(), out8u ? &o8 : nullptr, out16s ? &o16 : nullptr, s));
    }
    // stitch_one on the cameras' NV12 frames (defs.h:10-17; the capture threads' cvtColor(YUV2BGR_NV12), networking.cpp:45-47, folded into the warp): nv12_imgs[i] = 8UC1 (rows * 3 / 2) x cols
    template <class Mat> void stitch_one_nv12(const std::vector<Mat> &nv12_imgs, Mat *out8u, Mat *out16s, ms_stream s = nullptr)
    {
        std::vector<ms_image> v;
        for (const Mat &m : nv12_imgs) v.push_back(wrap(m));
        ms_image o8{}, o16{};
        if (out8u) o8 = wrap(*out8u);
        if (out16s) o16 = wrap(*out16s);
        check(ms_stitch_nv12(ctx_, (int)(v.size() / n_), v.data(), out8u ? &o8 : nullptr, out16s ? &o16 : nullptr, s));
    }
    // stitch_one + consume()'s cvtColor(BGR2YUV_I420) (timed.cpp:308-316) in one: i420[f] = contiguous 8UC1 (rows * 3 / 2) x out_w, rows from i420Rows()
    template <class Mat> void stitch_one_i420(const std::vector<Mat> &full_imgs, std::vector<Mat> &i420, ms_stream s = nullptr)
    {
        std::vector<ms_image> v, o;
        for (const Mat &m : full_imgs) v.push_back(wrap(m));
        for (const Mat &m : i420) o.push_back(wrap(m));
        check(ms_stitch_i420(ctx_, (int)(v.size() / n_), v.data(), o.data(), s));
    }
    // ... with the cameras' NV12 frames as input: neither BGR frames nor a BGR canvas
    template <class Mat> void stitch_one_nv12_i420(const std::vector<Mat> &nv12_imgs, std::vector<Mat> &i420, ms_stream s = nullptr)
    {
        std::vector<ms_image> v, o;
        for (const Mat &m : nv12_imgs) v.push_back(wrap(m));
        for (const Mat &m : i420) o.push_back(wrap(m));
        check(ms_stitch_nv12_i420(ctx_, (int)(v.size() / n_), v.data(), o.data(), s));
    }
    void i420Rows(int &first_canvas_row, int &rows) const { check(ms_get_i420_rows(ctx_, &first_canvas_row, &rows)); }
    // MultiBandBlender::feed_online(img, idx, stream) / blend(dst, dst_mask, gpuOut, true) call shape (timed.cpp:110,137)
    template <class Mat> void feed_online(const Mat &img, int idx, ms_stream s = nullptr) { ms_image v = wrap(img); check(ms_feed(ctx_, idx, &v, s)); }
    template <class Mat> void blend(Mat *out8u, Mat *out16s, ms_stream s = nullptr)
    {
        ms_image o8{}, o16{};
        if (out8u) o8 = wrap(*out8u);
        if (out16s) o16 = wrap(*out16s);
        check(ms_blend(ctx_, out8u ? &o8 : nullptr, out16s ? &o16 : nullptr, s));
    }
    ms_pano_geom panoGeom() const { ms_pano_geom g; check(ms_get_pano_geom(ctx_, &g)); return g; }
    ms_view_geom viewGeom(int i) const { ms_view_geom g; check(ms_get_view_geom(ctx_, i, &g)); return g; }
    ms_ctx *raw() { return ctx_; }
    // warpImages' seam-scale half (calibration.cpp:92-135, 224-237): resize, seam warps, gains, Voronoi seams, dilate, resize up, AND
    template <class Mat> void calibrateSeam(const std::vector<Mat> &full_imgs, const float *K_seam, const ms_seam_params &prm, double *gains_out = nullptr, ms_stream s = nullptr)
    {
        std::vector<ms_image> v;
        for (const Mat &m : full_imgs) v.push_back(wrap(m));
        check(ms_calibrate_seam(ctx_, v.data(), K_seam, &prm, gains_out, s));
    }

private:
    ms_ctx *ctx_ = nullptr;
    int n_ = 0;
};


// ---- calibrateCameras / stitch_calib (360_stitcher/calibration.cpp:28-68, 252-311) ---------------------------------------------------
// The rig model and every scale of the calibration, in product code: cameras[i].{focal, ppx, ppy, R} at compose and seam scale plus
// work / seam / compose scales and warper scales (ms_calibrate_cameras restates calibration.cpp:28-68, 101-116, 147-181, 269-288).
inline ms_rig calibrateCameras(int num_views, int full_w, int full_h, double hfov_deg = 90.0,
                               double work_megapix = 0.6, double seam_megapix = 0.01, double compose_megapix = 1.4)      // defs.h:51-53
{
    ms_rig_params q{num_views, full_w, full_h, hfov_deg, work_megapix, seam_megapix, compose_megapix};
    ms_rig rig;
    check(ms_calibrate_cameras(&q, &rig));
    return rig;
}

struct Calibration {
    ms_rig rig;
    int num_bands = 0;             // mb->setNumBands(...) of calibration.cpp:193
    float blend_width = 0.f;
    ms_rect pano_roi{};            // resultRoi(corners, sizes)
    std::vector<double> gains;     // GainCompensator::gains()
};

// stitch_calib (calibration.cpp:252-311) up to the blender being ready for stitch_one: rig + scales (calibrateCameras), compose-scale ROIs and the
// num_bands rule (:163-194), warp maps + blender->prepare (:196-221), the seam-scale pipeline with exposure gains (:92-135, 224-237),
// init_gpu for every view (:240).  full_imgs: the first frame of every camera, device 8UC3 at full size.  With compose_scale more than 10 %
// from 1 the returned compositor expects frames already resized to rig.compose_width x compose_height (msshim::cuda::resize, timed.cpp:75-85).
// projection: the app ships MS_PROJ_CYLINDRICAL (calibration.cpp:100,156); out_w / out_h: canvas for the 8U output, 0 = none.
// update_mask_margin > 0 (CPW only): update_mask() on the returned compositor only enqueues, so the recalibration thread may call it after every
// mesh swap while frames flow; with 0 it is the synchronous rebuild, which makes a concurrent stitch_one wait (never race) for its ~50 ms.
// lenses: nullptr, or one ms_lens per view (model MS_LENS_NONE = that view has none): handed to ms_set_lens, so that the ROIs, the maps and the seam-scale
// pipeline go through the lens model (spherical and cylindrical projections).
// seam_finder: MS_SEAM_VORONOI (calibration.cpp:134) or MS_SEAM_DP (Compositor::setSeamFinder).
template <class Mat>
std::unique_ptr<Compositor> stitch_calib(const std::vector<Mat> &full_imgs, int projection, bool enable_local, Calibration &cal,
                                         double hfov_deg = 90.0, double work_megapix = 0.6, double seam_megapix = 0.01, double compose_megapix = 1.4,
                                         float blend_strength = 5.f, int out_w = 0, int out_h = 0, int frames_in_flight = 1,
                                         int num_bands_override = -1, ms_stream s = nullptr, int update_mask_margin = 0, const ms_lens *lenses = nullptr,
                                         int seam_finder = MS_SEAM_VORONOI)
{
    const int n = (int)full_imgs.size();
    if (n < 1) throw Error(MS_ERR_INVALID, "stitch_calib: no images");
    cal.rig = calibrateCameras(n, full_imgs[0].cols, full_imgs[0].rows, hfov_deg, work_megapix, seam_megapix, compose_megapix);
    const ms_rig &rig = cal.rig;
    std::vector<ms_rect> rois(n);
    for (int i = 0; i < n; ++i)            // warper->warpRoi(sz, K, R) at compose scale :163-181
        check(lenses ? ms_warp_roi_lens(projection, rig.K_compose[i], rig.R[i], &lenses[i], rig.compose_warp_scale, rig.compose_width, rig.compose_height, &rois[i], s)
                     : ms_warp_roi(projection, rig.K_compose[i], rig.R[i], rig.compose_warp_scale, rig.compose_width, rig.compose_height, &rois[i]));
    check(ms_result_roi(n, rois.data(), &cal.pano_roi));
    check(ms_num_bands_rule(cal.pano_roi.width, cal.pano_roi.height, blend_strength, &cal.blend_width, &cal.num_bands));       // :183-194
    if (num_bands_override >= 0) cal.num_bands = num_bands_override;
    if (out_w < 0 || out_h < 0) {          // fit the 8U canvas to the panorama ROI (the compositor places pano x = 0 at canvas column out_w / 2)
        const ms_rect &r = cal.pano_roi;
        out_w = (2 * std::max(std::abs(r.x), std::abs(r.x + r.width)) + 1) & ~1;
        out_h = projection == MS_PROJ_SPHERICAL ? ((r.y + r.height + 1) & ~1) : ((2 * std::max(std::abs(r.y), std::abs(r.y + r.height)) + 1) & ~1);
    }
    std::unique_ptr<Compositor> comp(new Compositor(n, rig.compose_width, rig.compose_height, projection, rig.compose_warp_scale, cal.num_bands,
                                                    enable_local, out_w, out_h, frames_in_flight, enable_local ? update_mask_margin : 0));
    for (int i = 0; i < n; ++i) comp->setCamera(i, rig.K_compose[i], rig.R[i]);
    if (lenses) for (int i = 0; i < n; ++i) comp->setLens(i, &lenses[i]);
    comp->buildMaps(s);                                                                                          // :196, :221
    if (seam_finder != MS_SEAM_VORONOI) comp->setSeamFinder(seam_finder);
    ms_seam_params sp{rig.seam_scale, rig.seam_warp_scale, enable_local ? 1 : 0, 1};
    cal.gains.assign(n, 1.0);
    comp->calibrateSeam(full_imgs, &rig.K_seam[0][0], sp, cal.gains.data(), s);                                  // :92-135, :224-237
    comp->init_gpu(s);                                                                                           // :240
    return comp;
}

// ---- matchFeatures' descriptor matching (featurefinder.cpp:50-66): dm->knnMatch(f1.descriptors, f2.descriptors, matches, 2) on the device,
// then the 0.7 ratio test.  query / train: GpuMat-like 8UC1 descriptor matrices (upload of ImageFeatures::descriptors).
// Calls emit(queryIdx, trainIdx, distance) for every kept pair, in query order -- push_back(DMatch(...)) in the caller.
template <class Mat, class Emit> void knnRatioMatches(const Mat &query, const Mat &train, Emit emit, ms_stream s = nullptr)
{
    ms_image q = wrap(query), t = wrap(train);
    std::vector<int> idx((size_t)2 * q.rows), dist((size_t)2 * q.rows);
    check(ms_knn_match_hamming2(&q, &t, idx.data(), dist.data(), s));
    for (int i = 0; i < q.rows; ++i)
        if (idx[2 * i + 1] >= 0 && (float)dist[2 * i] < 0.7 * (float)dist[2 * i + 1]) emit(i, idx[2 * i], (float)dist[2 * i]);
}

// ---- featurefinder (360_stitcher/featurefinder.cpp, featurefinder.h:7-13) over the device front-end ----------------------------------------
// Mat = a GpuMat-like device image type with create(rows, cols, type) (cv::cuda::GpuMat qualifies).  ImageFeatures / MatchesInfo have the fields
// of cv::detail::ImageFeatures / MatchesInfo that the application reads; descriptors stay on the device (the reference downloads them and matches
// on the CPU; here matching runs on the device too).
namespace featurefinder {
struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; float size, angle, response; int octave; };
struct Size { int width, height; };
struct DMatch { int queryIdx, trainIdx; float distance; };
template <class Mat> struct ImageFeatures { int img_idx = 0; Size img_size{0, 0}; std::vector<KeyPoint> keypoints; Mat descriptors; };
struct MatchesInfo {
    int src_img_idx = -1, dst_img_idx = -1;
    std::vector<DMatch> matches;
    std::vector<unsigned char> inliers_mask;
    int num_inliers = 0;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // empty Mat in the reference when no model was found: have_H = false
    bool have_H = false;
    double confidence = 0;
};

// createMesh's feature masks (meshwarper.cpp:82-115): overlap bands of 400 px on both sides (the hard-coded split of view 3 when the rig has 6 views), minus black pixels
template <class Mat> void featureMasks(const std::vector<Mat> &images, std::vector<Mat> &masks, int overlap = 400, ms_stream s = nullptr)
{
    masks.resize(images.size());
    // every view's mask in ONE ms_feature_inputs_batch launch, MS_MAX_VIEWS views at a time
    for (size_t i0 = 0; i0 < images.size(); i0 += MS_MAX_VIEWS) {
        const size_t m = std::min(images.size() - i0, (size_t)MS_MAX_VIEWS);
        std::vector<ms_image> im(m), mk(m);
        std::vector<int> bands(4 * m);
        for (size_t j = 0; j < m; ++j) {
            const size_t idx = i0 + j;
            const int cols = images[idx].cols, rows = images[idx].rows;
            masks[idx].create(rows, cols, MS_8UC1);
            int ax0 = 0, bx0 = cols - overlap;
            if (idx == 3 && images.size() == 6) {        // "Opencv splits the third video (idx == 3) in the middle"
                const float split_l = images[0].cols * 0.25f * 2.0f, split_r = -images[0].cols * 0.25f * 2.0f;
                ax0 = (int)split_l - overlap; bx0 = cols + (int)split_r;
            }
            im[j] = wrap(images[idx]); mk[j] = wrap(masks[idx]);
            bands[4 * j] = ax0; bands[4 * j + 1] = overlap; bands[4 * j + 2] = bx0; bands[4 * j + 3] = overlap;
        }
        check(ms_feature_inputs_batch((int)m, im.data(), bands.data(), nullptr, mk.data(), s));
    }
}

// findFeatures (featurefinder.cpp:13-46) with work_scale < 0 (what createMesh passes): BGR2GRAY, cuda::ORB::create(2500, 1.2f, 8)->detectAndCompute
template <class Mat> void findFeatures(const std::vector<Mat> &images, const std::vector<Mat> &masks, std::vector<ImageFeatures<Mat>> &features, ms_stream s = nullptr,
                                       int nfeatures = 2500, float scale_factor = 1.2f, int nlevels = 8)
{
    features.resize(images.size());
    ms_orb_params prm;
    check(ms_orb_default_params(&prm));
    prm.nfeatures = nfeatures; prm.scale_factor = scale_factor; prm.nlevels = nlevels;
    const int cap = nfeatures + nlevels / 2;        // the rounded per-level budgets can add up to (nlevels - 1) / 2 more than nfeatures (ms_stitch.h)
    // grey as the reference converts it, every view in ONE ms_feature_inputs_batch launch, then every view's detectAndCompute in ONE ms_orb_detect_and_compute_batch
    // call, MS_MAX_VIEWS views at a time
    for (size_t i0 = 0; i0 < images.size(); i0 += MS_MAX_VIEWS) {
        const size_t m = std::min(images.size() - i0, (size_t)MS_MAX_VIEWS);
        std::vector<Mat> gray(m);
        std::vector<ms_image> im(m), g(m), mk(m), d(m);
        std::vector<float> kp((size_t)6 * cap * m);
        std::vector<int> n(m, 0);
        for (size_t j = 0; j < m; ++j) {
            const size_t i = i0 + j;
            gray[j].create(images[i].rows, images[i].cols, MS_8UC1);
            im[j] = wrap(images[i]);
            g[j] = wrap(gray[j]);
            features[i].descriptors.create(cap, 32, MS_8UC1);
            d[j] = wrap(features[i].descriptors);
            mk[j] = (i < masks.size() && masks[i].data) ? wrap(masks[i]) : ms_image{};
        }
        check(ms_feature_inputs_batch((int)m, im.data(), nullptr, g.data(), nullptr, s));       // cuda::cvtColor(gpu_img, gpu_img, CV_BGR2GRAY)
        check(ms_orb_detect_and_compute_batch((int)m, g.data(), mk.data(), &prm, kp.data(), cap, d.data(), n.data(), s));
        for (size_t j = 0; j < m; ++j) {
            const size_t i = i0 + j;
            features[i].img_idx = (int)i;
            features[i].img_size = Size{images[i].cols, images[i].rows};
            features[i].keypoints.resize(n[j]);
            for (int k = 0; k < n[j]; ++k) {
                const float *r = &kp[6 * ((size_t)cap * j + k)];
                features[i].keypoints[k] = KeyPoint{{r[0], r[1]}, r[5], r[3], r[2], (int)r[4]};
            }
        }
    }
}

// the body shared by matchFeatures (featurefinder.cpp:48-108) and matchFeaturesTemporal (:110-170): knnMatch(k = 2) + 0.7 ratio, centred points,
// findHomography(RANSAC), inlier count; confidence ends as 1 in both.  matchLists runs it for a list of (query features, train features) pairs in ONE ms_match_lists
// call -- MS_MATCH_MAX_PROBLEMS / 4 pairs at a time, so that the sets a call names always fit its table --; info[p] receives pair p's result.
template <class Mat> void matchLists(const std::vector<std::pair<const ImageFeatures<Mat> *, const ImageFeatures<Mat> *>> &pairs, const std::vector<MatchesInfo *> &info,
                                     ms_stream s = nullptr)
{
    static_assert(sizeof(KeyPoint) == 6 * sizeof(float), "KeyPoint rows are read as 6 floats, x and y first");
    const size_t chunk = MS_MATCH_MAX_PROBLEMS / 4;          // 16 problems name 32 sets at most: 2 * MS_MAX_VIEWS
    ms_list_match_params prm;
    check(ms_list_match_default_params(&prm));
    for (size_t p0 = 0; p0 < pairs.size(); p0 += chunk) {
        const size_t m = std::min(pairs.size() - p0, chunk);
        std::vector<const ImageFeatures<Mat> *> table;
        std::vector<ms_match_problem> problems(m);
        size_t cap = 0;
        for (size_t j = 0; j < m; ++j) {
            const ImageFeatures<Mat> *f[2] = {pairs[p0 + j].first, pairs[p0 + j].second};
            int at[2];
            for (int k = 0; k < 2; ++k) {
                const size_t i = (size_t)(std::find(table.begin(), table.end(), f[k]) - table.begin());
                if (i == table.size()) table.push_back(f[k]);
                at[k] = (int)i;
            }
            problems[j] = ms_match_problem{at[0], at[1]};
            cap += f[0]->keypoints.size();                   // a list holds at most one match per query row
        }
        std::vector<ms_view_features> sets(table.size());
        for (size_t i = 0; i < table.size(); ++i) {          // (a set without keypoints takes no part: its image size may be unset)
            const ImageFeatures<Mat> &f = *table[i];
            const bool none = f.keypoints.empty();
            sets[i] = ms_view_features{wrap(f.descriptors), none ? nullptr : &f.keypoints[0].pt.x, 6, (int)f.keypoints.size(), none ? 1 : f.img_size.width, none ? 1 : f.img_size.height};
        }
        std::vector<ms_pair_matches> out(m);
        std::vector<ms_feature_match> matches(cap + 1);
        int n_matches = 0;
        check(ms_match_lists((int)sets.size(), sets.data(), (int)m, problems.data(), &prm, out.data(), matches.data(), (int)cap, &n_matches, s));
        for (size_t j = 0; j < m; ++j) {
            MatchesInfo &pm = *info[p0 + j];
            const ms_pair_matches &r = out[j];
            pm.matches.clear(); pm.inliers_mask.clear(); pm.num_inliers = 0; pm.have_H = false;
            for (int i = 0; i < r.count; ++i) {
                const ms_feature_match &fm = matches[r.first + i];
                pm.matches.push_back(DMatch{fm.query, fm.train, (float)fm.distance});
                pm.inliers_mask.push_back((unsigned char)fm.inlier);
            }
            if (r.count > 0) {                               // findHomography ran: H (zeros without a model), the inlier count
                for (int e = 0; e < 9; ++e) pm.H[e] = r.H[e];
                pm.num_inliers = r.num_inliers; pm.have_H = r.have_H != 0;
            }
            pm.confidence = r.confidence;
        }
    }
}
template <class Mat> void matchPair(const ImageFeatures<Mat> &f1, const ImageFeatures<Mat> &f2, MatchesInfo &pm, ms_stream s = nullptr)
{
    matchLists<Mat>({{&f1, &f2}}, {&pm}, s);                 // the batch of one
}
// the ring of featurefinder.cpp:55-59: view i against its left neighbour
template <class Mat> void ringPairs(const std::vector<ImageFeatures<Mat>> &features, std::vector<MatchesInfo> &pairwise_matches,
                                    std::vector<std::pair<const ImageFeatures<Mat> *, const ImageFeatures<Mat> *>> &pairs, std::vector<MatchesInfo *> &info)
{
    const int n = (int)features.size();
    for (size_t i = 0; i < pairwise_matches.size(); ++i) {
        const int idx1 = (int)i, idx2 = i == 0 ? n - 1 : (int)i - 1;
        pairwise_matches[i].src_img_idx = idx1; pairwise_matches[i].dst_img_idx = idx2;
        pairs.push_back({&features[idx1], &features[idx2]});
        info.push_back(&pairwise_matches[i]);
    }
}
// featurefinder.cpp:117-121: view i now against view i of the previous round
template <class Mat> void temporalPairs(const std::vector<ImageFeatures<Mat>> &features, const std::vector<ImageFeatures<Mat>> &prev_features, std::vector<MatchesInfo> &temporal_matches,
                                        std::vector<std::pair<const ImageFeatures<Mat> *, const ImageFeatures<Mat> *>> &pairs, std::vector<MatchesInfo *> &info)
{
    for (size_t i = 0; i < temporal_matches.size(); ++i) {
        temporal_matches[i].src_img_idx = temporal_matches[i].dst_img_idx = (int)i;
        pairs.push_back({&features[i], &prev_features[i]});
        info.push_back(&temporal_matches[i]);
    }
}
template <class Mat> void matchFeatures(const std::vector<ImageFeatures<Mat>> &features, std::vector<MatchesInfo> &pairwise_matches, ms_stream s = nullptr)
{
    std::vector<std::pair<const ImageFeatures<Mat> *, const ImageFeatures<Mat> *>> pairs;
    std::vector<MatchesInfo *> info;
    ringPairs(features, pairwise_matches, pairs, info);
    matchLists<Mat>(pairs, info, s);
}
template <class Mat> void matchFeaturesTemporal(const std::vector<ImageFeatures<Mat>> &features, const std::vector<ImageFeatures<Mat>> &prev_features,
                                                std::vector<MatchesInfo> &pairwise_matches, ms_stream s = nullptr)
{
    std::vector<std::pair<const ImageFeatures<Mat> *, const ImageFeatures<Mat> *>> pairs;
    std::vector<MatchesInfo *> info;
    temporalPairs(features, prev_features, pairwise_matches, pairs, info);
    matchLists<Mat>(pairs, info, s);
}
// both of the above in one call (createMesh with USE_TEMPORAL, meshwarper.cpp:119-125): with N views, 2N problems over a table of 2N sets
template <class Mat> void matchFeaturesBoth(const std::vector<ImageFeatures<Mat>> &features, const std::vector<ImageFeatures<Mat>> &prev_features,
                                            std::vector<MatchesInfo> &pairwise_matches, std::vector<MatchesInfo> &temporal_matches, ms_stream s = nullptr)
{
    std::vector<std::pair<const ImageFeatures<Mat> *, const ImageFeatures<Mat> *>> pairs;
    std::vector<MatchesInfo *> info;
    ringPairs(features, pairwise_matches, pairs, info);
    temporalPairs(features, prev_features, temporal_matches, pairs, info);
    matchLists<Mat>(pairs, info, s);
}

// detail::BestOf2NearestMatcher / BestOf2NearestRangeMatcher::operator() (OCV/stitching/src/matchers.cpp:784-808 -> MatchPairsBody, :65-111) over ms_match_pairs:
// every candidate pair in one call, pairwise_matches the reference's n x n table -- entry (i, j), i < j, as ms_match_pairs returns it, entry (j, i) its dual with
// queryIdx / trainIdx swapped and H inverted (:88-99).  params: ms_pair_match_default_params with the caller's edits, or nullptr for the defaults.
template <class Mat> void matchPairs(const std::vector<ImageFeatures<Mat>> &features, std::vector<MatchesInfo> &pairwise_matches, const ms_pair_match_params *params = nullptr,
                                     ms_stream s = nullptr)
{
    static_assert(sizeof(KeyPoint) == 6 * sizeof(float), "KeyPoint rows are read as 6 floats, x and y first");
    const int n = (int)features.size();
    ms_pair_match_params prm;
    check(ms_pair_match_default_params(&prm));
    if (params) prm = *params;
    std::vector<ms_view_features> views(n);
    size_t cap = 0;
    for (int i = 0; i < n; ++i) {
        const ImageFeatures<Mat> &f = features[i];
        views[i] = ms_view_features{wrap(f.descriptors), f.keypoints.empty() ? nullptr : &f.keypoints[0].pt.x, 6, (int)f.keypoints.size(), f.img_size.width, f.img_size.height};
        cap += f.keypoints.size() * (size_t)(n - 1);         // a pair's list holds at most one match per row of either view
    }
    std::vector<ms_pair_matches> pairs((size_t)n * n);
    std::vector<ms_feature_match> matches(cap + 1);
    int n_pairs = 0, n_matches = 0;
    check(ms_match_pairs(n, views.data(), &prm, pairs.data(), n * n, &n_pairs, matches.data(), (int)cap, &n_matches, s));
    pairwise_matches.assign((size_t)n * n, MatchesInfo());
    for (int k = 0; k < n_pairs; ++k) {
        const ms_pair_matches &p = pairs[k];
        MatchesInfo &m = pairwise_matches[(size_t)p.view_a * n + p.view_b], &dual = pairwise_matches[(size_t)p.view_b * n + p.view_a];
        m.src_img_idx = p.view_a; m.dst_img_idx = p.view_b;
        for (int i = 0; i < p.count; ++i) {
            const ms_feature_match &fm = matches[p.first + i];
            m.matches.push_back(DMatch{fm.query, fm.train, (float)fm.distance});
            m.inliers_mask.push_back((unsigned char)fm.inlier);
        }
        m.num_inliers = p.num_inliers; m.have_H = p.have_H != 0; m.confidence = p.confidence;
        for (int e = 0; e < 9; ++e) m.H[e] = p.H[e];
        dual = m;
        dual.src_img_idx = p.view_b; dual.dst_img_idx = p.view_a;
        for (DMatch &d : dual.matches) { const int q = d.queryIdx; d.queryIdx = d.trainIdx; d.trainIdx = q; }
        if (m.have_H) {                                      // H.inv(): the adjugate over the determinant; a singular H inverts to zeros as cv::Mat::inv(DECOMP_LU) does
            const double *h = m.H;
            const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
            const double adj[9] = {h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4], h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6],
                                   h[2] * h[3] - h[0] * h[5], h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]};
            for (int e = 0; e < 9; ++e) dual.H[e] = det != 0.0 ? adj[e] / det : 0.0;
        }
    }
}
}  // namespace featurefinder

// ---- MeshWarper: createMesh's host logic around ms_create_mesh (360_stitcher/meshwarper.cpp:158-335) --------------------------
// Works on anything shaped like cv::detail::ImageFeatures (.img_size, .keypoints[i].pt) and cv::detail::MatchesInfo (.src_img_idx,
// .dst_img_idx, .matches[i].queryIdx/.trainIdx, .inliers_mask, .num_inliers): msshim::featurefinder's types above, or the caller's own.
// Differences from the reference, all stated: NUM_IMAGES is the run-time view count (the literal 5 of filterMatches is num_images - 1);
// prev_avg starts at 0 (an uninitialised member in the reference); old matches are kept as resolved positions instead of indices into a
// copy of the old ImageFeatures.
class MeshWarper {
public:
    static const int RECALIB_THRESH = 15;            // defs.h:49
    static const int MAX_FEATURES_PER_IMAGE = 100;   // defs.h:60
    static const int MAX_TEMPORAL_FEATURES_PER_IMAGE = 100;   // defs.h:61

    MeshWarper(int num_images, int mesh_width, int mesh_height, float focal_length, double compose_scale, double work_scale)
        : n_(num_images), old_(num_images), prev_(num_images), prev_avg_(2 * num_images, 0.f), have_old_(num_images, 0)
    {
        check(ms_mesh_default_params(&prm_));
        prm_.mesh_cols = mesh_width; prm_.mesh_rows = mesh_height; prm_.focal_length = focal_length;
        prm_.compose_scale = compose_scale; prm_.work_scale = work_scale;
    }
    ms_mesh_params &params() { return prm_; }

    // theta of a camera pair in camera steps, meshwarper.cpp:617-629 / :914-925 (before the * 2 pi / 6, which filterMatches never applies);
    // params().theta_rule = 1 (evenly spaced ring): the wrapped index difference, in radians
    float theta(int src, int dst) const
    {
        if (prm_.theta_rule == 1) {
            int d = dst - src;
            if (d > n_ / 2.0) d -= n_;
            if (d < -n_ / 2.0) d += n_;
            return (float)(d * 2 * 3.1415926535897932384626 / n_);
        }
        float t = (float)(dst - src);
        if (src == 0 && dst == n_ - 1 && prm_.wrap_around) t = -1;
        if (src == 3) t = 4.25f;
        if (src == 4) t = -0.25f;
        return t;
    }

    // filterMatches, meshwarper.cpp:888-946: inliers of the kept camera pairs whose offset is plausible for the rig
    template <class Features, class Matches>
    void filterMatches(const std::vector<Matches> &pairwise_matches, const std::vector<Features> &features, std::vector<std::vector<ms_mesh_match>> &filt) const
    {
        filt.assign(n_, {});
        for (const Matches &pw : pairwise_matches) {
            const int src = pw.src_img_idx, dst = pw.dst_img_idx;
            if (!pw.matches.size() || !pw.num_inliers) continue;
            if (dst != n_ - 1 || (src != 0 && dst == n_ - 1))
                if (src - dst - 1 != 0) continue;
            for (size_t i = 0; i < pw.inliers_mask.size(); ++i) {
                if (!pw.inliers_mask[i]) continue;
                const auto &p1 = features[src].keypoints[pw.matches[i].queryIdx].pt;
                const auto &p2 = features[dst].keypoints[pw.matches[i].trainIdx].pt;
                const float scale = (float)(prm_.compose_scale / prm_.work_scale);
                const float max_x_dist = theta(src, dst) * prm_.focal_length * scale;
                if (std::fabs(p1.y - p2.y) > 40) continue;
                if (std::fabs(max_x_dist - (p1.x - p2.x)) > 300) continue;
                filt[src].push_back(ms_mesh_match{p1.x, p1.y, p2.x, p2.y, dst});
            }
        }
    }

    // the match lists createMesh hands to calcLocalTerm / calcGlobalTerm (meshwarper.cpp:158-292), and the state update (:313-334)
    template <class Features, class Matches>
    std::vector<std::vector<ms_mesh_match>> select(const std::vector<Features> &features, const std::vector<Matches> &pairwise_matches)
    {
        std::vector<std::vector<ms_mesh_match>> all, sel(n_), use(n_);
        filterMatches(pairwise_matches, features, all);
        for (int v = 0; v < n_; ++v)
            sel[v].assign(all[v].begin(), all[v].begin() + std::min<size_t>(MAX_FEATURES_PER_IMAGE, all[v].size()));
        // average x of the matched points per image half: [2 idx] = as source (left partner), [2 idx + 1] = as destination
        std::vector<float> sum(2 * n_, 0.f), cnt(2 * n_, 0.f), avg(2 * n_, 0.f);
        for (int v = 0; v < n_; ++v)
            for (const ms_mesh_match &m : sel[v]) { sum[v * 2] += m.x1; sum[m.dst * 2 + 1] += m.x2; cnt[v * 2]++; cnt[m.dst * 2 + 1]++; }
        for (int k = 0; k < 2 * n_; ++k) if (cnt[k] != 0) avg[k] = sum[k] / cnt[k];
        std::vector<char> use_old(n_, 0);
        for (int v = 0; v < n_; ++v) {
            const int v2 = v == 0 ? n_ - 1 : v - 1;
            const float d = std::fabs(avg[v * 2] - avg[v2 * 2 + 1]), dp = std::fabs(prev_avg_[v * 2] - prev_avg_[v2 * 2 + 1]);
            const bool found = avg[v * 2] != 0 && avg[v2 * 2 + 1] != 0, found_prev = prev_avg_[v * 2] != 0 && prev_avg_[v2 * 2 + 1] != 0;
            use_old[v] = std::fabs(d - dp) < RECALIB_THRESH || (!found && found_prev);
            use[v] = use_old[v] ? old_[v] : sel[v];
        }
        for (int v = 0; v < n_; ++v) {
            prev_[v] = sel[v];
            const int v2 = v == 0 ? n_ - 1 : v - 1;
            if (use_old[v] && !prev_[v].empty() && have_old_[v]) continue;
            old_[v] = sel[v];   have_old_[v] = 1;  prev_avg_[v * 2] = avg[v * 2];   prev_avg_[v * 2 + 1] = avg[v * 2 + 1];
            old_[v2] = sel[v2]; have_old_[v2] = 1; prev_avg_[v2 * 2] = avg[v2 * 2]; prev_avg_[v2 * 2 + 1] = avg[v2 * 2 + 1];
        }
        return use;
    }

    // filterTemporalMatches, meshwarper.cpp:948-982: inliers of a view's match against itself one round earlier that moved no more than 30 px along either axis;
    // (x1, y1) is the point now, (x2, y2) the point in the previous round's keypoints
    template <class Features, class Matches>
    void filterTemporalMatches(const std::vector<Matches> &temporal_matches, const std::vector<Features> &features, const std::vector<Features> &prev_features,
                               std::vector<std::vector<ms_mesh_match>> &filt) const
    {
        filt.assign(n_, {});
        for (const Matches &pw : temporal_matches) {
            const int src = pw.src_img_idx, dst = pw.dst_img_idx;
            if (!pw.matches.size() || !pw.num_inliers) continue;
            for (size_t i = 0; i < pw.inliers_mask.size(); ++i) {
                if (!pw.inliers_mask[i]) continue;
                const auto &p1 = features[src].keypoints[pw.matches[i].queryIdx].pt;
                const auto &p2 = prev_features[dst].keypoints[pw.matches[i].trainIdx].pt;
                if (std::fabs(p1.y - p2.y) > 30) continue;
                if (std::fabs(p1.x - p2.x) > 30) continue;
                filt[src].push_back(ms_mesh_match{p1.x, p1.y, p2.x, p2.y, dst});
            }
        }
    }
    // the lists createMesh hands to calcTemporalLocalTerm (meshwarper.cpp:139-150): the first MAX_TEMPORAL_FEATURES_PER_IMAGE of every view's filtered matches
    template <class Features, class Matches>
    std::vector<std::vector<ms_mesh_match>> selectTemporal(const std::vector<Matches> &temporal_matches, const std::vector<Features> &features,
                                                           const std::vector<Features> &prev_features) const
    {
        std::vector<std::vector<ms_mesh_match>> all;
        filterTemporalMatches(temporal_matches, features, prev_features, all);
        for (auto &l : all) l.resize(std::min<size_t>(MAX_TEMPORAL_FEATURES_PER_IMAGE, l.size()));
        return all;
    }

    // createMesh from the matching step on: warped = images[idx] (the remapped frames, device 8UC3); meshes come back as n x N x M host floats
    template <class Mat, class Features, class Matches>
    ms_mesh_info createMesh(const std::vector<Mat> &warped, const std::vector<Features> &features, const std::vector<Matches> &pairwise_matches,
                            std::vector<float> &mesh_x, std::vector<float> &mesh_y, ms_stream s = nullptr)
    {
        return solve(warped, select(features, pairwise_matches), nullptr, mesh_x, mesh_y, s);
    }
    // ... with USE_TEMPORAL (meshwarper.cpp:121-151, :289-291): temporal_matches from matchFeaturesTemporal / matchFeaturesBoth against prev_features, the features of
    // the round before.  Without previous features (the first round) or with params().alphas[3] == 0 there is no temporal term, as in the overload above.
    // temporalSelected() tells how many temporal matches the last call handed to the solver.
    template <class Mat, class Features, class Matches>
    ms_mesh_info createMesh(const std::vector<Mat> &warped, const std::vector<Features> &features, const std::vector<Matches> &pairwise_matches,
                            const std::vector<Matches> &temporal_matches, const std::vector<Features> &prev_features, std::vector<float> &mesh_x, std::vector<float> &mesh_y,
                            ms_stream s = nullptr)
    {
        const std::vector<std::vector<ms_mesh_match>> use = select(features, pairwise_matches);
        if (prev_features.empty() || prm_.alphas[3] == 0) return solve(warped, use, nullptr, mesh_x, mesh_y, s);
        const std::vector<std::vector<ms_mesh_match>> temporal = selectTemporal(temporal_matches, features, prev_features);
        return solve(warped, use, &temporal, mesh_x, mesh_y, s);
    }
    size_t temporalSelected() const { return temporal_selected_; }

    // calibrateMeshWarp (meshwarper.cpp:356-376): createMesh + convertMeshesToMap into the compositor
    template <class Mat, class Features, class Matches>
    ms_mesh_info calibrateMeshWarp(Compositor &comp, const std::vector<Mat> &warped, const std::vector<Features> &features,
                                   const std::vector<Matches> &pairwise_matches, ms_stream s = nullptr)
    {
        std::vector<float> mx, my;
        const ms_mesh_info info = createMesh(warped, features, pairwise_matches, mx, my, s);
        const size_t per = (size_t)prm_.mesh_rows * prm_.mesh_cols;
        for (int v = 0; v < n_; ++v) comp.convertMeshToMap(v, mx.data() + v * per, my.data() + v * per, prm_.mesh_rows, prm_.mesh_cols, s);
        return info;
    }
    // ... with the temporal term: createMesh's second overload
    template <class Mat, class Features, class Matches>
    ms_mesh_info calibrateMeshWarp(Compositor &comp, const std::vector<Mat> &warped, const std::vector<Features> &features, const std::vector<Matches> &pairwise_matches,
                                   const std::vector<Matches> &temporal_matches, const std::vector<Features> &prev_features, ms_stream s = nullptr)
    {
        std::vector<float> mx, my;
        const ms_mesh_info info = createMesh(warped, features, pairwise_matches, temporal_matches, prev_features, mx, my, s);
        const size_t per = (size_t)prm_.mesh_rows * prm_.mesh_cols;
        for (int v = 0; v < n_; ++v) comp.convertMeshToMap(v, mx.data() + v * per, my.data() + v * per, prm_.mesh_rows, prm_.mesh_cols, s);
        return info;
    }

private:
    // createMesh's loop + solve over the selected lists; temporal: nullptr, or one list per view
    template <class Mat>
    ms_mesh_info solve(const std::vector<Mat> &warped, const std::vector<std::vector<ms_mesh_match>> &use, const std::vector<std::vector<ms_mesh_match>> *temporal,
                       std::vector<float> &mesh_x, std::vector<float> &mesh_y, ms_stream s)
    {
        std::vector<ms_image> views;
        std::vector<ms_mesh_match> flat, tflat;
        std::vector<int> count, tcount;
        for (const Mat &m : warped) views.push_back(wrap(m));
        for (const auto &l : use) { flat.insert(flat.end(), l.begin(), l.end()); count.push_back((int)l.size()); }
        if (temporal) for (const auto &l : *temporal) { tflat.insert(tflat.end(), l.begin(), l.end()); tcount.push_back((int)l.size()); }
        temporal_selected_ = tflat.size();
        mesh_x.assign((size_t)n_ * prm_.mesh_rows * prm_.mesh_cols, 0.f);
        mesh_y.assign(mesh_x.size(), 0.f);
        ms_mesh_info info{};
        check(ms_create_mesh(n_, views.data(), flat.data(), count.data(), temporal ? tflat.data() : nullptr, temporal ? tcount.data() : nullptr, &prm_, mesh_x.data(), mesh_y.data(),
                             &info, s));
        return info;
    }

    size_t temporal_selected_ = 0;
    int n_;
    ms_mesh_params prm_{};
    std::vector<std::vector<ms_mesh_match>> old_, prev_;    // old_matches / prev_matches, resolved to positions
    std::vector<float> prev_avg_;
    std::vector<char> have_old_;                             // !old_features.at(idx).empty()
};

// ---- rig rotations from the same matches: detail::BundleAdjusterRay (stitching/src/motion_estimators.cpp:514-700) with the focals held ---------
// Every RANSAC inlier of every pair, as the per-view lists ms_refine_rig takes (ms_create_mesh's layout: x1, y1 in view src, x2, y2 in view dst).
template <class Features, class Matches>
std::vector<std::vector<ms_mesh_match>> inlierLists(const std::vector<Features> &features, const std::vector<Matches> &pairwise_matches)
{
    std::vector<std::vector<ms_mesh_match>> lists(features.size());
    for (const Matches &pw : pairwise_matches)
        for (size_t i = 0; i < pw.inliers_mask.size(); ++i) {
            if (!pw.inliers_mask[i]) continue;
            const auto &p1 = features[pw.src_img_idx].keypoints[pw.matches[i].queryIdx].pt;
            const auto &p2 = features[pw.dst_img_idx].keypoints[pw.matches[i].trainIdx].pt;
            lists[pw.src_img_idx].push_back(ms_mesh_match{p1.x, p1.y, p2.x, p2.y, pw.dst_img_idx});
        }
    return lists;
}
// (*bundle_adjuster_)(features_, pairwise_matches_, cameras_) (stitching/src/stitcher.cpp:573-574) for the rotations of a calibrated compositor: R_out receives
// num_views x 9 floats for setCamera; nothing is applied -- setCamera, buildMaps, the masks and init_gpu follow as in the first calibration.  prm == nullptr: the defaults
inline ms_rig_refine_info refineRig(Compositor &comp, const std::vector<std::vector<ms_mesh_match>> &lists, std::vector<float> &R_out, const ms_rig_refine_params *prm = nullptr,
                                    ms_stream s = nullptr)
{
    ms_rig_refine_params dflt;
    check(ms_rig_refine_default_params(&dflt));
    std::vector<ms_mesh_match> flat;
    std::vector<int> count;
    for (const auto &l : lists) { flat.insert(flat.end(), l.begin(), l.end()); count.push_back((int)l.size()); }
    R_out.assign(9 * lists.size(), 0.f);
    ms_rig_refine_info info{};
    check(ms_refine_rig(comp.raw(), flat.data(), count.data(), prm ? prm : &dflt, R_out.data(), &info, s));
    return info;
}

}  // namespace msshim
