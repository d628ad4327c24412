// reproject_poses.hip -- virtual cameras that move (include/ms_stitch.h section 5): ms_reproject_poses renders every frame and view of a call in ONE launch, each
// frame under a rotation of its own, without maps; ms_view_pose_table builds the table of those rotations on the host.
//   The contract is the two-call route's, bit for bit: k_view_maps' coordinates (reproject.hip) followed by k_reproject's sample.  Both halves are shared source:
// the view ray is lens_unproject (lens.hpp) or the warper's backward direction as k_view_maps writes it, the coordinates are rp_pano_coords, the taps, row reads,
// fma chain and stores are reproject.hpp's.  The library is built with -ffp-contract=off, so the same source gives the same bits here and there.
//   What does not depend on the frame -- the view ray of each of a lane's four pixels, whose Newton solves are the dear part of a lens view -- is built once
// per lane; the frame loop rotates it, evaluates one hypot and two atan2 in double, and samples.
#include <cmath>
#include "ctx.hpp"
#include "lens.hpp"
#include "reproject.hpp"

namespace ms {

constexpr int RPP_G = MS_VIEW_POSE_FRAME_GROUP;      // frames a lane walks with one set of rays

// A view as the kernel takes it: what lens_unproject reads of LensCam and LensDist (no rotation, one copy of the coefficients), the surface form, the rectangle
struct PoseJob {
    double k00, k01, k02, k11, k12;       // CAMERA: K[0], K[1], K[2], K[4], K[5]
    double k[8], max_theta, limit;        // CAMERA: LensDist's
    double view_scale;                    // SURFACE
    int model, kind, view_proj, tl_u, tl_v;
    int cols, rows, dst_x, dst_y, tile0, tiles_x;
};

struct PoseArgs {
    const uint8_t *src[MS_VIEW_MAX_FRAMES];
    uint8_t *dst[MS_VIEW_MAX_FRAMES];
    PoseJob job[MS_VIEW_POSE_MAX_JOBS];
    const float *poses;           // DEVICE: [job][frame][9]
    size_t dstep;                 // BGR: the destination's row step
    double src_scale;
    int n_jobs, n_frames;
    unsigned sstep;
    int scols, srows;
    int dcols, drows;             // I420: the frame's size W x H (the planes' geometry)
    int wrap, clamp;              // the sampler's flags (rp_make_taps)
    int src_proj, u0, v0, wrap_cols;      // the panorama frame (rp_pano_coords)
};
static_assert(sizeof(PoseArgs) <= 4096, "the kernel argument of k_reproject_poses must fit the 4 KiB a launch carries");

// k_reproject's shape (reproject.hip): a workgroup = one tile of one job for one group of RPP_G frames, 16 x 16 lanes, a lane = 4 x 1 pixels (BGR: tiles of
// 64 x 16) or 2 x 2 (I420: 32 x 32); blockIdx.x = the tile (jobs one behind the other), blockIdx.y = the frame group.
template <int FMT>
__global__ void __launch_bounds__(256) k_reproject_poses(const PoseArgs A)
{
    int ji = 0;
    while (ji + 1 < A.n_jobs && (int)blockIdx.x >= A.job[ji + 1].tile0) ++ji;
    const PoseJob &J = A.job[ji];
    const int local = (int)blockIdx.x - J.tile0, ty = local / J.tiles_x, tx = local - ty * J.tiles_x;
    const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
    const int x0 = FMT == MS_VIEW_BGR ? tx * MS_VIEW_TILE_W + 4 * lx : tx * 32 + 2 * lx;
    const int y0 = FMT == MS_VIEW_BGR ? ty * MS_VIEW_TILE_H + ly : ty * 32 + 2 * ly;
    if (x0 >= J.cols || y0 >= J.rows) return;

    // step 1 of ms_build_view_maps, k_view_maps' lines: the view rays, once for all frames
    double c[RP_PX][3];
    bool seen[RP_PX];
    int n_px = 0;      // BGR: the pixels of this lane inside the view (I420 views are even: always the whole block)
    {
        LensCam cam{};
        cam.k00 = J.k00; cam.k01 = J.k01; cam.k02 = J.k02; cam.k11 = J.k11; cam.k12 = J.k12;
        LensDist dist{};
        for (int i = 0; i < 8; ++i) dist.k[i] = J.k[i];
        dist.max_theta = J.max_theta; dist.limit = J.limit; dist.model = J.model;
#pragma unroll
        for (int k = 0; k < RP_PX; ++k) {
            const int x = FMT == MS_VIEW_BGR ? x0 + k : x0 + (k & 1), y = FMT == MS_VIEW_BGR ? y0 : y0 + (k >> 1);
            seen[k] = false;
            c[k][0] = c[k][1] = c[k][2] = 0.0;
            if (x < J.cols && y < J.rows) {
                ++n_px;
                if (J.kind == MS_VIEW_CAMERA) {
                    seen[k] = lens_unproject(cam, dist, (double)x, (double)y, c[k]);
                } else {
                    const double u = (double)(J.tl_u + x) / J.view_scale, v = (double)(J.tl_v + y) / J.view_scale;
                    if (J.view_proj == MS_PROJ_SPHERICAL) { const double sv = sin(v); c[k][0] = sv * sin(u); c[k][1] = -cos(v); c[k][2] = sv * cos(u); }
                    else { c[k][0] = sin(u); c[k][1] = v; c[k][2] = cos(u); }
                    seen[k] = true;
                }
            }
        }
    }

    const int f0 = (int)blockIdx.y * RPP_G, f1 = min(A.n_frames, f0 + RPP_G);
    const int dx = J.dst_x + x0, dy = J.dst_y + y0;
    const float *pose = A.poses + ((size_t)ji * (size_t)A.n_frames + (size_t)f0) * 9;
    for (int f = f0; f < f1; ++f, pose += 9) {
        double r[9];      // the frame's rotation: the same nine words for the whole workgroup
#pragma unroll
        for (int i = 0; i < 9; ++i) r[i] = (double)pose[i];
        RpTaps T[RP_PX];
#pragma unroll
        for (int k = 0; k < RP_PX; ++k) {
            if (k < n_px) {       // (a lane's pixels inside the view are its first n_px: 4 x 1 clipped at the right edge, or all four)
                float ox, oy;
                rp_pano_coords(seen[k], r, c[k], A.src_scale, A.src_proj, A.u0, A.v0, A.wrap_cols, ox, oy);
                T[k] = rp_make_taps(ox, oy, A);
            } else {
                T[k] = RpTaps{0u, 0u, 0, 0, 0.f, 0.f, 0.f, 0.f, 0u};
            }
        }
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
            rp_store_bgr(A, f, dx, dy, n_px, w);
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

int ms_view_pose_table(const ms_view_pose_job *jobs, int n_jobs, const double *rig_poses, int n_frames, float *poses_host)
{
    const char *fn = "ms_view_pose_table";
    MS_CHECK(jobs && poses_host, "%s: null argument (jobs / poses_host)", fn);
    MS_CHECK(n_jobs >= 1 && n_jobs <= MS_VIEW_POSE_MAX_JOBS, "%s: n_jobs = %d outside [1, %d]", fn, n_jobs, MS_VIEW_POSE_MAX_JOBS);
    MS_CHECK(n_frames >= 1 && n_frames <= MS_VIEW_MAX_FRAMES, "%s: n_frames = %d outside [1, %d]", fn, n_frames, MS_VIEW_MAX_FRAMES);
    for (int j = 0; j < n_jobs; ++j) {
        const ms_view &v = jobs[j].view;
        MS_CHECK(v.struct_size == sizeof(ms_view), "%s: jobs[%d].view: ms_view.struct_size %u, this library's is %zu", fn, j, v.struct_size, sizeof(ms_view));
        for (int i = 0; i < 9; ++i) MS_CHECK(std::isfinite(v.R[i]), "%s: jobs[%d].view R is not finite", fn, j);
    }
    if (rig_poses)
        for (int i = 0; i < 9 * n_frames; ++i) MS_CHECK(std::isfinite(rig_poses[i]), "%s: rig_poses of frame %d is not finite", fn, i / 9);
    for (int j = 0; j < n_jobs; ++j) {
        double R[9];
        for (int i = 0; i < 9; ++i) R[i] = (double)jobs[j].view.R[i];
        for (int f = 0; f < n_frames; ++f) {
            float *o = poses_host + ((size_t)j * n_frames + f) * 9;
            if (!rig_poses) { for (int i = 0; i < 9; ++i) o[i] = jobs[j].view.R[i]; continue; }
            double PR[9];
            rp_rot_mul(rig_poses + 9 * (size_t)f, R, PR);
            for (int i = 0; i < 9; ++i) o[i] = (float)PR[i];
        }
    }
    return MS_OK;
}

int ms_reproject_poses(const ms_pano_frame *frame, const ms_image *src, ms_image *dst, int n_frames, const ms_view_pose_job *jobs, int n_jobs, const float *poses_dev,
                       int format, ms_stream stream)
{
    const char *fn = "ms_reproject_poses";
    MS_CHECK(frame && src && dst && jobs && poses_dev, "%s: null argument (frame / src / dst / jobs / poses_dev)", fn);
    if (int e = rp_check_pano_frame(fn, frame)) return e;
    MS_CHECK(((uintptr_t)poses_dev & 3) == 0, "%s: poses_dev must be 4-byte aligned", fn);
    RpLayout L;
    const ms_lens *lens[MS_VIEW_POSE_MAX_JOBS];
    const int e = rp_layout(fn, src, dst, n_frames, n_jobs, MS_VIEW_POSE_MAX_JOBS, frame->wrap_cols, frame->clamp_rows, format, [&](int j, RpRect &r) -> int {
        char name[32];
        snprintf(name, sizeof(name), "jobs[%d].view", j);
        if (int e = rp_check_view(fn, name, &jobs[j].view, false, &lens[j])) return e;
        r = RpRect{jobs[j].view.width, jobs[j].view.height, jobs[j].dst_x, jobs[j].dst_y};
        return MS_OK;
    }, L);
    if (e) return e;
    if (int e = require_device()) return e;
    const bool i420 = format == MS_VIEW_I420;
    const ms_image &s0 = src[0], &d0 = dst[0];
    PoseArgs A{};
    for (int j = 0; j < n_jobs; ++j) {
        const ms_view &v = jobs[j].view;
        PoseJob &P = A.job[j];
        if (v.kind == MS_VIEW_CAMERA) {
            const LensCam cam = lens_cam(v.K, nullptr, lens[j]);
            const LensDist dist = lens_dist(lens[j]);
            P.k00 = cam.k00; P.k01 = cam.k01; P.k02 = cam.k02; P.k11 = cam.k11; P.k12 = cam.k12;
            for (int i = 0; i < 8; ++i) P.k[i] = dist.k[i];
            P.max_theta = dist.max_theta; P.limit = dist.limit; P.model = dist.model;
        }
        P.view_scale = v.kind == MS_VIEW_SURFACE ? (double)v.scale : 1.0;
        P.kind = v.kind; P.view_proj = v.projection; P.tl_u = v.tl_u; P.tl_v = v.tl_v;
        P.cols = L.rect[j].w; P.rows = L.rect[j].h; P.dst_x = L.rect[j].dst_x; P.dst_y = L.rect[j].dst_y;
        P.tile0 = L.tile0[j]; P.tiles_x = L.tiles_x[j];
    }
    for (int f = 0; f < n_frames; ++f) { A.src[f] = (const uint8_t *)src[f].data; A.dst[f] = (uint8_t *)dst[f].data; }
    A.poses = poses_dev;
    A.dstep = d0.step;
    A.src_scale = (double)frame->scale;
    A.n_jobs = n_jobs; A.n_frames = n_frames;
    A.sstep = (unsigned)s0.step; A.scols = s0.cols; A.srows = s0.rows;
    A.dcols = L.fw; A.drows = L.fh;
    A.wrap = frame->wrap_cols != 0; A.clamp = frame->clamp_rows;
    A.src_proj = frame->projection; A.u0 = frame->u0; A.v0 = frame->v0; A.wrap_cols = frame->wrap_cols;
    const dim3 grid(L.tiles, div_up(n_frames, RPP_G));
    if (i420) k_reproject_poses<MS_VIEW_I420><<<grid, 256, 0, as_stream(stream)>>>(A);
    else k_reproject_poses<MS_VIEW_BGR><<<grid, 256, 0, as_stream(stream)>>>(A);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

}  // extern "C"
