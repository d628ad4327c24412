// reproject.hip -- virtual cameras rendered from the panorama (include/ms_stitch.h section 5): the host helpers (ms_look_at_view, ms_cube_face_view,
// ms_get_pano_frame), the calibration-time map kernel behind ms_build_view_maps, and the per-frame sampler behind ms_reproject.
//   The maps are detail::{Spherical,Cylindrical}Projector::mapForward (OCV/stitching/include/opencv2/stitching/detail/warpers_inl.hpp:222-236, :258-273) of the
// view's ray -- lens_unproject (lens.hpp) for a camera, the warper's backward direction for a piece of a surface -- in double, rounded once at the store.
//   The sampler is cuda::remap(INTER_LINEAR, BORDER_CONSTANT) (k_remap_linear, prims.hip: same taps, weights, fma chain, saturation) on a source that wraps at
// the +-pi seam and repeats its pole rows, for every frame and every view of a call in ONE launch: the job table travels in the kernel argument
// (as k_feature_inputs, features.hip), a lane builds the tap state of its four pixels once and walks its frames with it (as k_warp_s, tile_kernels.hpp).
#include <algorithm>
#include <cmath>
#include "ctx.hpp"
#include "lens.hpp"
#include "reproject.hpp"

namespace ms {

// ------------------------------------------------------------------------------------------------
// ms_build_view_maps

struct ViewMapArgs {
    LensCam cam;          // CAMERA: K's five entries and the lens; r = R (view to rig) for both kinds
    LensDist dist;
    double view_scale;    // SURFACE
    double src_scale;
    int kind, view_proj, tl_u, tl_v;
    int src_proj, u0, v0, wrap;
};

// one lane per map pixel, 64 x 4 workgroups (k_lens_maps' shape)
__global__ void __launch_bounds__(256) k_view_maps(const ViewMapArgs A, int cols, int rows, float *__restrict__ mapx, size_t mxstep, float *__restrict__ mapy, size_t mystep)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    double c[3];
    bool seen = true;
    if (A.kind == MS_VIEW_CAMERA) {
        seen = lens_unproject(A.cam, A.dist, (double)x, (double)y, c);
    } else {
        const double u = (double)(A.tl_u + x) / A.view_scale, v = (double)(A.tl_v + y) / A.view_scale;
        if (A.view_proj == MS_PROJ_SPHERICAL) { const double sv = sin(v); c[0] = sv * sin(u); c[1] = -cos(v); c[2] = sv * cos(u); }
        else { c[0] = sin(u); c[1] = v; c[2] = cos(u); }
    }
    float ox, oy;
    rp_pano_coords(seen, A.cam.r, c, A.src_scale, A.src_proj, A.u0, A.v0, A.wrap, ox, oy);
    row_ptr<float>(mapx, mxstep, y)[x] = ox;
    row_ptr<float>(mapy, mystep, y)[x] = oy;
}

// ------------------------------------------------------------------------------------------------
// ms_reproject

struct ReprojArgs {
    const uint8_t *src[MS_VIEW_MAX_FRAMES];
    uint8_t *dst[MS_VIEW_MAX_FRAMES];
    ReprojJob job[MS_VIEW_MAX_JOBS];
    size_t dstep;                 // BGR: the destination's row step
    int n_jobs, n_frames;
    unsigned sstep;
    int scols, srows;
    int dcols, drows;             // I420: the frame's size W x H (the planes' geometry)
    int wrap, clamp;
};

// (the tap state, the row reads, the fma chain and the store: reproject.hpp, shared with ms_reproject_aa)
// A workgroup = one tile of one job for one group of RP_G frames: 16 x 16 lanes, a lane = 4 x 1 pixels (BGR: tiles of 64 x 16) or 2 x 2 (I420: 32 x 32).
// blockIdx.x = the tile (jobs one behind the other, ReprojJob::tile0), blockIdx.y = the frame group.
template <int FMT>
__global__ void __launch_bounds__(256) k_reproject(const ReprojArgs A)
{
    int ji = 0;
    while (ji + 1 < A.n_jobs && (int)blockIdx.x >= A.job[ji + 1].tile0) ++ji;
    const ReprojJob &J = A.job[ji];
    const int local = (int)blockIdx.x - J.tile0, ty = local / J.tiles_x, tx = local - ty * J.tiles_x;
    const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
    const int x0 = FMT == MS_VIEW_BGR ? tx * MS_VIEW_TILE_W + 4 * lx : tx * 32 + 2 * lx;
    const int y0 = FMT == MS_VIEW_BGR ? ty * MS_VIEW_TILE_H + ly : ty * 32 + 2 * ly;
    if (x0 >= J.cols || y0 >= J.rows) return;

    RpTaps T[RP_PX];
    int n_px = 0;      // BGR: the pixels of this lane inside the view (I420 views are even: always the whole block)
#pragma unroll
    for (int k = 0; k < RP_PX; ++k) {
        const int x = FMT == MS_VIEW_BGR ? x0 + k : x0 + (k & 1), y = FMT == MS_VIEW_BGR ? y0 : y0 + (k >> 1);
        if (x < J.cols && y < J.rows) {
            T[k] = rp_make_taps(row_ptr<float>(J.mx, J.mxstep, y)[x], row_ptr<float>(J.my, J.mystep, y)[x], A);
            ++n_px;
        } else {
            T[k] = RpTaps{0u, 0u, 0, 0, 0.f, 0.f, 0.f, 0.f, 0u};
        }
    }

    const int f0 = (int)blockIdx.y * RP_G, f1 = min(A.n_frames, f0 + RP_G);
    const int dx = J.dst_x + x0, dy = J.dst_y + y0;
    for (int f = f0; f < f1; ++f) {
        const uint8_t *S = A.src[f];
        RpRow r1[RP_PX], r2[RP_PX];
#pragma unroll
        for (int k = 0; k < RP_PX; ++k) {
            r1[k] = rp_row(S, T[k].o1, T[k], (T[k].flags & RP_Y1) != 0);
            r2[k] = rp_row(S, T[k].o2, T[k], (T[k].flags & RP_Y2) != 0);
        }
        if (FMT == MS_VIEW_BGR) {
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < RP_PX; ++k) {
                float o[3];
                rp_blend(T[k], r1[k], r2[k], o);
                rp_pack_bgr(o, k, w);
            }
            // rp_store_bgr's body, kept here: called as a function, the byte-store tail comes out in another block order and with other registers
            uint8_t *d = A.dst[f] + (size_t)dy * A.dstep + 3 * (size_t)dx;
            if (n_px == RP_PX && ((uintptr_t)d & 3) == 0) {
                rp_u32x3_a4 v; v.x = w[0]; v.y = w[1]; v.z = w[2];
                *(RP_GLOBAL rp_u32x3_a4 *)(uintptr_t)d = v;
            } else {
                RP_GLOBAL uint8_t *g = (RP_GLOBAL uint8_t *)(uintptr_t)d;
#pragma unroll
                for (int i = 0; i < 3 * RP_PX; ++i)
                    if (i < 3 * n_px) g[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            unsigned yq[2] = {0u, 0u}, uq = 0u, vq = 0u;
#pragma unroll
            for (int k = 0; k < RP_PX; ++k) {
                float o[3];
                rp_blend(T[k], r1[k], r2[k], o);
                rp_pack_i420(o, k, yq, uq, vq);
            }
            rp_store_i420(A, f, dx, dy, yq, uq, vq);
        }
    }
}

}  // namespace ms

// ------------------------------------------------------------------------------------------------
// host side

using namespace ms;

extern "C" {

int ms_look_at_view(double yaw_deg, double pitch_deg, double roll_deg, double hfov_deg, int width, int height, ms_view *out)
{
    const char *fn = "ms_look_at_view";
    MS_CHECK(out, "%s: null out", fn);
    MS_CHECK(std::isfinite(yaw_deg) && std::isfinite(pitch_deg) && std::isfinite(roll_deg), "%s: yaw, pitch and roll must be finite", fn);
    MS_CHECK(hfov_deg > 0.0 && hfov_deg <= 179.0, "%s: hfov_deg %g outside (0, 179]", fn, hfov_deg);
    if (int e = rp_check_side(fn, "width x height", width, height)) return e;
    const double D = LENS_PI / 180.0, ya = yaw_deg * D, pa = pitch_deg * D, ra = roll_deg * D;
    const double Ry[9] = {cos(ya), 0, sin(ya), 0, 1, 0, -sin(ya), 0, cos(ya)};
    const double Rx[9] = {1, 0, 0, 0, cos(pa), -sin(pa), 0, sin(pa), cos(pa)};
    const double Rz[9] = {cos(ra), -sin(ra), 0, sin(ra), cos(ra), 0, 0, 0, 1};
    double Ryx[9], R[9];
    rp_rot_mul(Ry, Rx, Ryx);
    rp_rot_mul(Ryx, Rz, R);
    ms_view v{};
    v.struct_size = sizeof(ms_view);
    v.kind = MS_VIEW_CAMERA;
    v.width = width; v.height = height;
    for (int i = 0; i < 9; ++i) v.R[i] = (float)R[i];
    const double f = ((double)width / 2.0) / tan(hfov_deg * D / 2.0);
    v.K[0] = (float)f; v.K[2] = (float)(((double)width - 1.0) / 2.0);
    v.K[4] = (float)f; v.K[5] = (float)(((double)height - 1.0) / 2.0);
    v.K[8] = 1.f;
    v.lens.struct_size = sizeof(ms_lens);
    v.lens.model = MS_LENS_NONE;
    v.projection = MS_PROJ_SPHERICAL;
    *out = v;
    return MS_OK;
}

int ms_cube_face_view(int face, int size, ms_view *out)
{
    const char *fn = "ms_cube_face_view";
    MS_CHECK(out, "%s: null out", fn);
    MS_CHECK(face >= 0 && face <= 5, "%s: face %d outside [0, 5] (front, right, back, left, up, down)", fn, face);
    MS_CHECK(size >= 1 && size <= 32767, "%s: size %d outside [1, 32767]", fn, size);
    static const double yaw[6] = {0, 90, 180, -90, 0, 0}, pitch[6] = {0, 0, 0, 0, 90, -90};
    return ms_look_at_view(yaw[face], pitch[face], 0.0, 90.0, size, size, out);
}

int ms_get_pano_frame(const ms_ctx *c, int which, ms_pano_frame *out)
{
    const char *fn = "ms_get_pano_frame";
    MS_CHECK(c && out, "%s: null argument (ctx / out)", fn);
    MS_CHECK(which == MS_PANO_CANVAS || which == MS_PANO_ROI, "%s: which = %d is neither MS_PANO_CANVAS nor MS_PANO_ROI", fn, which);
    if (c->cfg.projection == MS_PROJ_PLANE) return fail(MS_ERR_UNSUPPORTED, "%s: a MS_PROJ_PLANE context has no sphere to look at", fn);
    if (which == MS_PANO_CANVAS && c->cfg.out_width == 0) return fail(MS_ERR_UNSUPPORTED, "%s: MS_PANO_CANVAS of a context without a canvas (out_width == 0)", fn);
    if (!c->maps_built) return fail(MS_ERR_STATE, "%s: before ms_build_maps", fn);
    ms_pano_frame p{};
    p.struct_size = sizeof(ms_pano_frame);
    p.projection = c->cfg.projection;
    p.scale = c->cfg.warp_scale;
    if (which == MS_PANO_ROI) {
        p.u0 = c->bg.dst_roi_final.x; p.v0 = c->bg.dst_roi_final.y;
    } else {
        const long long half_turn = llrint(LENS_PI * (double)c->cfg.warp_scale);
        const bool sph = c->cfg.projection == MS_PROJ_SPHERICAL;
        p.u0 = -(c->cfg.out_width / 2);
        p.v0 = sph ? 0 : -(c->cfg.out_height / 2);
        p.wrap_cols = 2 * half_turn == (long long)c->cfg.out_width ? c->cfg.out_width : 0;
        p.clamp_rows = sph && (long long)c->cfg.out_height == half_turn ? 1 : 0;
    }
    *out = p;
    return MS_OK;
}

int ms_build_view_maps(const ms_pano_frame *src, const ms_view *view, ms_image *map_x, ms_image *map_y, ms_stream stream)
{
    const char *fn = "ms_build_view_maps";
    MS_CHECK(src && view && map_x && map_y, "%s: null argument (src / view / map_x / map_y)", fn);
    MS_CHECK(src->struct_size == sizeof(ms_pano_frame), "%s: ms_pano_frame.struct_size %u, this library's is %zu", fn, src->struct_size, sizeof(ms_pano_frame));
    if (int e = rp_check_pano_frame(fn, src)) return e;
    const ms_lens *lens = nullptr;
    if (int e = rp_check_view(fn, "view", view, true, &lens)) return e;
    if (int e = rp_check_view_map(fn, "map_x", *map_x)) return e;
    if (int e = rp_check_view_map(fn, "map_y", *map_y)) return e;
    MS_CHECK(map_x->cols == view->width && map_x->rows == view->height && map_y->cols == view->width && map_y->rows == view->height,
             "%s: map_x %d x %d / map_y %d x %d are not of the view's size %d x %d", fn, map_x->cols, map_x->rows, map_y->cols, map_y->rows, view->width, view->height);
    if (int e = require_device()) return e;
    ViewMapArgs A{};
    static const float I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    A.cam = lens_cam(view->kind == MS_VIEW_CAMERA ? view->K : I3, view->R, lens);
    A.dist = lens_dist(lens);
    A.view_scale = view->kind == MS_VIEW_SURFACE ? (double)view->scale : 1.0;
    A.src_scale = (double)src->scale;
    A.kind = view->kind; A.view_proj = view->projection; A.tl_u = view->tl_u; A.tl_v = view->tl_v;
    A.src_proj = src->projection; A.u0 = src->u0; A.v0 = src->v0; A.wrap = src->wrap_cols;
    k_view_maps<<<dim3(div_up(view->width, 64), div_up(view->height, 4)), dim3(64, 4), 0, as_stream(stream)>>>(A, view->width, view->height, (float *)map_x->data, map_x->step,
                                                                                                             (float *)map_y->data, map_y->step);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

int ms_reproject(const ms_image *src, ms_image *dst, int n_frames, const ms_view_job *jobs, int n_jobs, int wrap_cols, int clamp_rows, int format, ms_stream stream)
{
    const char *fn = "ms_reproject";
    RpPlan P;
    if (int e = rp_plan(fn, src, dst, n_frames, jobs, sizeof(ms_view_job), n_jobs, wrap_cols, clamp_rows, format, P)) return e;
    const bool i420 = format == MS_VIEW_I420;
    const ms_image &s0 = src[0], &d0 = dst[0];
    if (int e = require_device()) return e;
    ReprojArgs A{};
    for (int j = 0; j < n_jobs; ++j) A.job[j] = P.job[j];
    for (int f = 0; f < n_frames; ++f) { A.src[f] = (const uint8_t *)src[f].data; A.dst[f] = (uint8_t *)dst[f].data; }
    A.dstep = d0.step;
    A.n_jobs = n_jobs; A.n_frames = n_frames;
    A.sstep = (unsigned)s0.step; A.scols = s0.cols; A.srows = s0.rows;
    A.dcols = P.fw; A.drows = P.fh;
    A.wrap = wrap_cols != 0; A.clamp = clamp_rows;
    const dim3 grid(P.tiles, div_up(n_frames, RP_G));
    if (i420) k_reproject<MS_VIEW_I420><<<grid, 256, 0, as_stream(stream)>>>(A);
    else k_reproject<MS_VIEW_BGR><<<grid, 256, 0, as_stream(stream)>>>(A);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

}  // extern "C"
