// lens.hip -- warp maps and view ROIs of a camera with lens distortion (ms_lens, lens.hpp): calibration-time kernels behind ms_build_warp_maps_lens,
// ms_warp_roi_lens, and through them ms_build_maps / ms_calibrate_seam of a context with a lens.  The per-frame path never runs anything of this unit: it reads
// the dense maps these kernels store (PROJ_MAPS, tile_kernels.hpp).
//   The maps are the backward maps of detail::{Spherical,Cylindrical}WarperGpu::buildMaps (stitching/src/cuda/build_warp_maps.cu:67-152) with the distortion
// between R^-1 and K.  The ROI is found by forward evaluation only: every integer warper coordinate of a fixed candidate window is mapped, and the ROI is the
// bounding box of those whose truncated map coordinates hit the source (k_valid_mask's rule).
//   k_lens_unproject, behind ms_lens_unproject_points, is the inverse (lens.hpp, lens_unproject): source pixels, a rig's keypoints, to unit camera rays.
#include <algorithm>
#include <climits>
#include <type_traits>
#include "launchers.hpp"
#include "lens.hpp"

namespace ms {

// the map entry of warper coordinate (u, v): rounded to float ONCE, here; (-1, -1) where the lens does not see the ray
template <int PROJ, int MODEL>
__device__ __forceinline__ float2 lens_map_entry(const LensCam &c, double su, double cu, double v)
{
    double X, Y, Z, px, py;
    lens_ray(PROJ, c, su, cu, v, X, Y, Z);
    if (!lens_project(MODEL, c, X, Y, Z, px, py)) return make_float2(-1.f, -1.f);
    return make_float2((float)px, (float)py);
}

// one lane per map pixel, 64 x 4 workgroups
template <int PROJ, int MODEL>
__global__ void __launch_bounds__(256) k_lens_maps(int tl_u, int tl_v, int cols, int rows, float *__restrict__ mapx, size_t mxstep, float *__restrict__ mapy, size_t mystep,
                                                   LensCam cam, double scale)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const double u = (double)(tl_u + x) / scale;
    const float2 m = lens_map_entry<PROJ, MODEL>(cam, sin(u), cos(u), (double)(tl_v + y) / scale);
    row_ptr<float>(mapx, mxstep, y)[x] = m.x;
    row_ptr<float>(mapy, mystep, y)[x] = m.y;
}

__device__ __forceinline__ int wave_min_i32(int v) { for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64)); return v; }
__device__ __forceinline__ int wave_max_i32(int v) { for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64)); return v; }

__global__ void k_lens_box_init(int *box) { if (threadIdx.x == 0) { box[0] = box[1] = INT_MAX; box[2] = box[3] = INT_MIN; } }

// One lane per candidate of the window [u0, u0 + cols) x [v0, v0 + rows): a lane keeps its column (sin / cos of u once) and strides over the rows with the grid, so a
// window of millions of candidates is a few thousand workgroups.  box = {min u, min v, max u, max v} of the seen candidates (k_lens_box_init resets it).
template <int PROJ, int MODEL>
__global__ void __launch_bounds__(256) k_lens_bbox(int u0, int v0, int cols, int rows, int src_w, int src_h, LensCam cam, double scale, int *__restrict__ box)
{
    __shared__ int s_box[4][4];
    const int x = blockIdx.x * 256 + threadIdx.x;
    int lo_u = INT_MAX, lo_v = INT_MAX, hi_u = INT_MIN, hi_v = INT_MIN;
    if (x < cols) {
        const double u = (double)(u0 + x) / scale, su = sin(u), cu = cos(u);
        for (int y = blockIdx.y; y < rows; y += gridDim.y) {
            const float2 m = lens_map_entry<PROJ, MODEL>(cam, su, cu, (double)(v0 + y) / scale);
            const int xx = f2i_rz(m.x), yy = f2i_rz(m.y);
            if (xx >= 0 && xx < src_w && yy >= 0 && yy < src_h) {
                lo_v = min(lo_v, v0 + y); hi_v = max(hi_v, v0 + y);
                lo_u = hi_u = u0 + x;
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool any = __ballot(lo_u != INT_MAX) != 0ull;      // (most waves of a scan see nothing: no butterflies for them)
    if (any) { lo_u = wave_min_i32(lo_u); lo_v = wave_min_i32(lo_v); hi_u = wave_max_i32(hi_u); hi_v = wave_max_i32(hi_v); }
    if (lane == 0) { s_box[wave][0] = lo_u; s_box[wave][1] = lo_v; s_box[wave][2] = hi_u; s_box[wave][3] = hi_v; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lo_u = min(lo_u, s_box[w][0]); lo_v = min(lo_v, s_box[w][1]);
            hi_u = max(hi_u, s_box[w][2]); hi_v = max(hi_v, s_box[w][3]);
        }
        if (lo_u != INT_MAX) { atomicMin(&box[0], lo_u); atomicMin(&box[1], lo_v); atomicMax(&box[2], hi_u); atomicMax(&box[3], hi_v); }
    }
}

// f(<PROJ, MODEL> as integral constants) for the two projections and three models the lens path takes
template <typename Fn>
static int with_proj_model(const char *who, int proj, int model, Fn &&f)
{
#define MS_LENS_CASE(P, M) if (proj == P && model == M) { f(std::integral_constant<int, P>{}, std::integral_constant<int, M>{}); return MS_OK; }
    MS_LENS_CASE(MS_PROJ_SPHERICAL, MS_LENS_NONE) MS_LENS_CASE(MS_PROJ_SPHERICAL, MS_LENS_BROWN) MS_LENS_CASE(MS_PROJ_SPHERICAL, MS_LENS_FISHEYE)
    MS_LENS_CASE(MS_PROJ_CYLINDRICAL, MS_LENS_NONE) MS_LENS_CASE(MS_PROJ_CYLINDRICAL, MS_LENS_BROWN) MS_LENS_CASE(MS_PROJ_CYLINDRICAL, MS_LENS_FISHEYE)
#undef MS_LENS_CASE
    if (proj == MS_PROJ_PLANE) return fail(MS_ERR_UNSUPPORTED, "%s: the lens model is built for the spherical and cylindrical warpers, not MS_PROJ_PLANE", who);
    return fail(MS_ERR_INVALID, "%s: unknown projection %d or lens model %d", who, proj, model);
}

int launch_lens_maps(int proj, int tl_u, int tl_v, ms_image &mx, ms_image &my, const float *K, const float *R, const ms_lens *lens, float scale, hipStream_t st)
{
    const LensCam cam = lens_cam(K, R, lens);
    const dim3 g(div_up(mx.cols, 64), div_up(mx.rows, 4)), b(64, 4);
    if (int e = with_proj_model("ms_build_warp_maps_lens", proj, cam.model, [&](auto P, auto M) {
            k_lens_maps<decltype(P)::value, decltype(M)::value><<<g, b, 0, st>>>(tl_u, tl_v, mx.cols, mx.rows, (float *)mx.data, mx.step, (float *)my.data, my.step, cam, (double)scale);
        })) return e;
    MS_LAUNCH_CHECK();
    return MS_OK;
}

static void lens_roi_window(int proj, float scale, int &u0, int &v0, int &cols, int &rows)
{
    const double s = (double)scale;
    const long long U = llrint(LENS_PI * s);
    u0 = (int)-U; cols = (int)(2 * U);
    if (proj == MS_PROJ_SPHERICAL) { v0 = 0; rows = (int)U; }
    else { const long long V = (long long)ceil(s * tan(MS_LENS_CYL_MAX_ELEVATION_DEG * (LENS_PI / 180.0))); v0 = (int)-V; rows = (int)(2 * V + 1); }
}

int lens_roi_device(int proj, const float *K, const float *R, const ms_lens *lens, float scale, int src_w, int src_h, ms_rect *roi, bool *seen_any, hipStream_t st)
{
    // (the scan is 2 * llrint(pi * scale) columns wide; a context's panorama side is at most 32767, which no scale above 5215 fits)
    MS_CHECK(scale > 0.f && scale <= 8192.f, "ms_warp_roi_lens: warper scale %g outside (0, 8192]", (double)scale);
    const LensCam cam = lens_cam(K, R, lens);
    int u0, v0, cols, rows;
    lens_roi_window(proj, scale, u0, v0, cols, rows);
    MS_CHECK(cols >= 1 && rows >= 1, "ms_warp_roi_lens: warper scale %g leaves no candidate window", (double)scale);
    int *box = (int *)device_scratch().get(4 * sizeof(int));
    if (!box) return fail(MS_ERR_NOMEM, "ms_warp_roi_lens: no device memory for the bounding box");
    k_lens_box_init<<<1, 64, 0, st>>>(box);
    MS_LAUNCH_CHECK();
    const dim3 g(div_up(cols, 256), std::min(rows, 256));
    if (int e = with_proj_model("ms_warp_roi_lens", proj, cam.model, [&](auto P, auto M) {
            k_lens_bbox<decltype(P)::value, decltype(M)::value><<<g, 256, 0, st>>>(u0, v0, cols, rows, src_w, src_h, cam, (double)scale, box);
        })) return e;
    MS_LAUNCH_CHECK();
    int h[4];
    MS_HIP(hipMemcpyAsync(h, box, sizeof(h), hipMemcpyDeviceToHost, st));
    MS_HIP(hipStreamSynchronize(st));
    *seen_any = h[0] != INT_MAX;
    if (*seen_any) *roi = ms_rect{h[0], h[1], h[2] - h[0] + 1, h[3] - h[1] + 1};
    return MS_OK;
}

// one lane per point: the float pixel widened to double, lens_unproject, the ray and the flag stored; a point the lens does not see gets the ray (0, 0, 0)
__global__ void __launch_bounds__(256) k_lens_unproject(int n, const float2 *__restrict__ px, LensCam cam, LensDist lens, double *__restrict__ rays, unsigned char *__restrict__ seen)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float2 p = px[k];
    double ray[3] = {0.0, 0.0, 0.0};
    const bool ok = lens_unproject(cam, lens, (double)p.x, (double)p.y, ray);
    rays[3 * (size_t)k] = ok ? ray[0] : 0.0; rays[3 * (size_t)k + 1] = ok ? ray[1] : 0.0; rays[3 * (size_t)k + 2] = ok ? ray[2] : 0.0;
    seen[k] = ok ? 1 : 0;
}

// One device block, pixels | rays | flags: the pixels go up in one copy, rays and flags (adjacent) come back in one.
int lens_unproject_device(const float *K, const ms_lens *lens, int n, const float *px_host, double *rays_host, unsigned char *seen_host, hipStream_t st)
{
    const size_t o_rays = (size_t)n * sizeof(float2), o_seen = o_rays + (size_t)n * 3 * sizeof(double), total = o_seen + (size_t)n;
    char *base = (char *)device_scratch().get(total), *host = (char *)pinned_scratch().get(total);
    if (!base || !host) return fail(MS_ERR_NOMEM, "ms_lens_unproject_points: no memory for %zu bytes", total);
    memcpy(host, px_host, o_rays);
    MS_HIP(hipMemcpyAsync(base, host, o_rays, hipMemcpyHostToDevice, st));
    k_lens_unproject<<<div_up(n, 256), 256, 0, st>>>(n, (const float2 *)base, lens_cam(K, nullptr, lens), lens_dist(lens), (double *)(base + o_rays), (unsigned char *)(base + o_seen));
    MS_LAUNCH_CHECK();
    MS_HIP(hipMemcpyAsync(host + o_rays, base + o_rays, total - o_rays, hipMemcpyDeviceToHost, st));
    MS_HIP(hipStreamSynchronize(st));
    memcpy(rays_host, host + o_rays, (size_t)n * 3 * sizeof(double));
    memcpy(seen_host, host + o_seen, (size_t)n);
    return MS_OK;
}

}  // namespace ms
