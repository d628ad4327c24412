// launchers.hpp -- internal host-side launchers shared by the C-ABI wrappers (api.cpp) and the
// compositor (compositor.hip).  The analogue of the reference's host<->.cu seam
// (device::imgproc::*_gpu / device::blend::* free functions taking PtrStepSz by value).
#pragma once
#include "common.hpp"

namespace ms {

int launch_remap(const ms_image &src, const ms_image &xm, const ms_image &ym, ms_image &dst, int interp, int border, hipStream_t st);
int launch_resize_linear(const ms_image &src, ms_image &dst, double fx, double fy, hipStream_t st);
int launch_resize_linear_batch(const ms_image *src, ms_image *dst, int n, double fx, double fy, hipStream_t st);
int launch_nv12_resize_linear_batch(const ms_image *src, ms_image *dst, int n, double fx, double fy, hipStream_t st);
int launch_convert_scale_8u(const ms_image &src, ms_image &dst, double alpha, hipStream_t st);
int launch_convert(const ms_image &src, ms_image &dst, double alpha, hipStream_t st);
int launch_sub_16s(const ms_image &a, const ms_image &b, ms_image &dst, hipStream_t st);
int launch_add_16s(const ms_image &a, const ms_image &b, ms_image &dst, hipStream_t st);
int launch_and_8u(const ms_image &a, const ms_image &b, ms_image &dst, hipStream_t st);
int launch_compare_gt_32f(const ms_image &src, float thr, ms_image &dst, hipStream_t st);
int launch_compare_eq_8u(const ms_image &src, int val, ms_image &dst, hipStream_t st);
int launch_copy_make_border(const ms_image &src, ms_image &dst, int top, int left, int border_type, hipStream_t st);
int launch_pyr_down(const ms_image &src, ms_image &dst, hipStream_t st);
int launch_pyr_up(const ms_image &src, ms_image &dst, hipStream_t st);
int launch_add_src_weight(const ms_image &src, const ms_image &w, ms_image &dst, ms_image &dstw, int rcw, int rch, hipStream_t st);
int launch_add_src_weight_16s(const ms_image &src, const ms_image &w, ms_image &dst, ms_image &dstw, int rcw, int rch, hipStream_t st);
int launch_normalize_16s(const ms_image &w, ms_image &src, int width, int height, hipStream_t st);
int launch_normalize(const ms_image &w, ms_image &src, int width, int height, hipStream_t st);
int launch_zero_masked(ms_image &img, const ms_image &mask, hipStream_t st);
int launch_dilate3(const ms_image &src, ms_image &dst, hipStream_t st);
int launch_build_warp_maps(int proj, int tl_u, int tl_v, ms_image &mx, ms_image &my, const float *k_rinv, const float *t, float scale, hipStream_t st);
int launch_nv12_to_bgr(const ms_image &src, ms_image &dst, hipStream_t st);
int launch_nv12_to_bgr_batch(const ms_image *src, ms_image *dst, int n, hipStream_t st);
int launch_bgr_to_i420(const ms_image &src, ms_image &dst, hipStream_t st);
int launch_consume_i420(const ms_image &src, ms_image &dst, int out_w, int out_h, int ih, int y_off, hipStream_t st);
int launch_bgr_to_gray(const ms_image &src, ms_image &dst, hipStream_t st);
int launch_bgr_to_i420_batch(const ms_image *src, ms_image *dst, int n, hipStream_t st);
int launch_custom_resize(const ms_image &in, ms_image &out, hipStream_t st);

// host geometry (geometry.cpp)
struct Projector { float k[9], rinv[9], r_kinv[9], k_rinv[9], t[3], scale; };
void set_camera_params(Projector &p, const float *K, const float *R, const float *T, float scale);
void k_rinv_gemm(const float *K, const float *R, float *k_rinv);   // warpers_cuda.cpp: K * R.t()
void r_kinv_gemm(const float *K, const float *R, float *r_kinv);
ms_rect warp_roi(int proj, const Projector &p, int src_w, int src_h);
int calibrate_cameras(const ms_rig_params &q, ms_rig &r);
void num_bands_rule(int pano_w, int pano_h, float blend_strength, float *blend_width, int *num_bands);
ms_rect result_roi(int n, const ms_rect *rois);

struct BlendGeom { int num_bands; ms_rect dst_roi_final, dst_roi; };
struct ViewPad { int top, left, bottom, right, x_tl, y_tl, x_br, y_br; };
BlendGeom blender_prepare(ms_rect dst_roi, int actual_num_bands);
ViewPad blender_view_pad(const BlendGeom &g, int tl_x, int tl_y, int mask_cols, int mask_rows);
// VoronoiSeamFinder over device masks (contiguous, roi-sized), in place
int voronoi_seams_device(int n, const ms_rect *rois, uint8_t *const *masks_dev, hipStream_t st);                 // calib.hip
// N_host / I_host (n x n each, may be null): the overlap counts and mean intensities the solve consumed (ms_estimate_gains hands them out)
int estimate_gains_device(int n, const ms_rect *rois, const uint8_t *const *images_dev, const uint8_t *const *masks_dev, double *gains_host, hipStream_t st,
                          int *N_host = nullptr, double *I_host = nullptr);
// exposure tracking (ms_gain_stats / ms_track_gains; kernels in calib.hip).  The sample lattice, the views' static maps and this call's frames, by value:
struct ViewDesc;
struct GainTrackViews {
    const float *xmap[MS_MAX_VIEWS]; int pitch[MS_MAX_VIEWS];      // projection maps (ymap follows xmap: roi.height rows further), pitch in elements
    ms_rect roi[MS_MAX_VIEWS];
    const uint8_t *src[MS_MAX_VIEWS]; unsigned step[MS_MAX_VIEWS]; // this call's 8UC3 frames, or their NV12 planes (active views only)
    ms_rect T; int stride, nsx, nsy;                               // pano ROI, lattice step, samples per row / column
    int n, src_w, src_h; unsigned active;
};
constexpr int GAIN_TRACK_MAX_TABLES = MS_MAX_VIEWS + 4;            // full set, its alternate copy, num_views + 1 cached subsets
struct GainTrackTables { ViewDesc *tab[GAIN_TRACK_MAX_TABLES]; int n; };
// the tracker's per-context device block: accumulators, the exported statistics, the gains (double) and the solve counters
struct GainTrackBuf {
    unsigned long long acc[2 * MS_MAX_VIEWS * MS_MAX_VIEWS];
    long long outN[MS_MAX_VIEWS * MS_MAX_VIEWS], outS[MS_MAX_VIEWS * MS_MAX_VIEWS];
    double state[MS_MAX_VIEWS];
    int solves_ok, solves_singular, rejected, pad_;
};
int launch_gain_stats(const GainTrackViews &V, GainTrackBuf *buf, bool nv12, hipStream_t st);
int launch_gain_export(const GainTrackViews &V, GainTrackBuf *buf, hipStream_t st);
int launch_gain_update(const GainTrackViews &V, const GainTrackTables &W, GainTrackBuf *buf, double lambda, hipStream_t st);
// Partial statistics (ms_gain_stats_partial / ms_track_gains_from_partials): the raw accumulators of one column window in a caller-owned device buffer, so that
// the windows' integers add up on the device to the unsharded statistic.  Layout of a partial of an n-view context (ms_gain_partial_bytes):
//   GainPartialHeader, cnt[n * n] (symmetric), S[n * n]  -- unsigned 64-bit each, before the max(1, cnt) rule
constexpr unsigned GAIN_PARTIAL_MAGIC = 0x50474d53u;               // "SMGP"
constexpr int GAIN_MAX_PARTIALS = 16;                              // = the largest ms_config.col_shards
struct GainPartialHeader { unsigned magic, n, active, stride; int tx, ty, tw, th; };      // T = the pano ROI the lattice starts from (the same on every shard)
struct GainPartials { const unsigned long long *p[GAIN_MAX_PARTIALS]; int n; };
inline size_t gain_partial_bytes(int n) { return sizeof(GainPartialHeader) + 2 * (size_t)n * n * sizeof(unsigned long long); }
int launch_gain_partial_export(const GainTrackViews &V, const GainPartialHeader &H, GainTrackBuf *buf, void *partial, hipStream_t st);
int launch_gain_update_partials(const GainTrackViews &V, const GainTrackTables &W, const GainPartialHeader &H, const GainPartials &P, GainTrackBuf *buf, double lambda, hipStream_t st);
// Sample vectors (ms_gain_samples / ms_track_gains_from_samples): view shards.  What a pair needs of view a at a lattice sample is one integer, q_a or "not
// seen"; the owner of a view stores it for every sample of the view's lattice rectangle R_v, the buffers travel, and every shard forms the pair sums from all of
// them.  Layout of a buffer (ms_gain_samples_bytes; 32-bit words):
//   [0] magic  [1] num_views  [2] active mask  [3] stride  [4..7] T.x, T.y, T.width, T.height  [8] mask of the views held  [9] total bytes  [10..15] 0
//   [16 + v]   word offset of view v's data from the start of the buffer; 0 = not held
//   data       per held view in view order, R_v row-major: 0 = not seen, else q + 1
constexpr unsigned GAIN_SAMPLES_MAGIC = 0x56474d53u;               // "SMGV"
constexpr int GAIN_SAMPLES_HEADER_WORDS = 16;
constexpr int GAIN_MAX_SAMPLE_BUFS = 4;
// R_v in lattice indices: the (sx, sy) with T.x + sx * stride in [roi.x, roi.x + roi.width) and the same in y; w or h may be 0.  off = the word offset of the
// view in the buffer of a shard that holds `held`; computed on the host by gain_sample_rects alone, handed to producer and consumer by value.
struct GainSampleRects { int x0[MS_MAX_VIEWS], y0[MS_MAX_VIEWS], w[MS_MAX_VIEWS], h[MS_MAX_VIEWS]; };
struct GainSampleBufs { const unsigned *p[GAIN_MAX_SAMPLE_BUFS]; int n; };
inline void gain_sample_rects(const GainTrackViews &V, GainSampleRects &R)
{
    auto first = [](int lo, int s) { return lo <= 0 ? 0 : (lo + s - 1) / s; };      // the smallest k >= 0 with k * s >= lo
    for (int v = 0; v < V.n; ++v) {
        const ms_rect r = V.roi[v];
        const int x0 = first(r.x - V.T.x, V.stride), x1 = std::min(V.nsx, first(r.x + r.width - V.T.x, V.stride));
        const int y0 = first(r.y - V.T.y, V.stride), y1 = std::min(V.nsy, first(r.y + r.height - V.T.y, V.stride));
        R.x0[v] = x0; R.y0[v] = y0; R.w[v] = std::max(0, x1 - x0); R.h[v] = std::max(0, y1 - y0);
    }
}
// word offsets of the views `held` in their buffer (0 elsewhere); returns the buffer's size in words
inline size_t gain_sample_offsets(const GainTrackViews &V, const GainSampleRects &R, unsigned held, unsigned *off)
{
    size_t at = GAIN_SAMPLES_HEADER_WORDS + (size_t)V.n;
    for (int v = 0; v < V.n; ++v) {
        off[v] = 0;
        if (!((held >> v) & 1u)) continue;
        off[v] = (unsigned)at;
        at += (size_t)R.w[v] * R.h[v];
    }
    return at;
}
int launch_gain_samples(const GainTrackViews &V, const GainSampleRects &R, unsigned held, bool nv12, void *samples, hipStream_t st);
int launch_gain_stats_from_samples(const GainTrackViews &V, const GainSampleRects &R, const GainSampleBufs &P, GainTrackBuf *buf, hipStream_t st);
int launch_gain_update_samples(const GainTrackViews &V, const GainTrackTables &W, const GainSampleRects &R, const GainSampleBufs &P, GainTrackBuf *buf, double lambda, hipStream_t st);
int launch_gain_export_samples(const GainTrackViews &V, const GainSampleRects &R, const GainSampleBufs &P, GainTrackBuf *buf, hipStream_t st);
void feather_weight_map(const uint8_t *mask, int rows, int cols, float sharpness, float *w);

}  // namespace ms
