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
    float ox = -1.f, oy = -1.f;
    if (seen) {
        const double *r = A.cam.r;
        const double d0 = r[0] * c[0] + r[1] * c[1] + r[2] * c[2], d1 = r[3] * c[0] + r[4] * c[1] + r[5] * c[2], d2 = r[6] * c[0] + r[7] * c[1] + r[8] * c[2];
        const double h = hypot(d0, d2), S = A.src_scale;
        const double U = S * atan2(d0, d2);
        double V = 0.0;
        if (A.src_proj == MS_PROJ_SPHERICAL) V = S * atan2(h, -d1);
        else if (h == 0.0) seen = false;
        else V = S * d1 / h;
        if (seen) {
            double X = U - (double)A.u0;
            const double Y = V - (double)A.v0;
            if (A.wrap > 0) X -= (double)A.wrap * floor(X / (double)A.wrap);
            ox = (float)X; oy = (float)Y;
            if (A.wrap > 0 && ox == (float)A.wrap) ox = 0.f;
        }
    }
    row_ptr<float>(mapx, mxstep, y)[x] = ox;
    row_ptr<float>(mapy, mystep, y)[x] = oy;
}

// ------------------------------------------------------------------------------------------------
// ms_reproject

constexpr int RP_G = MS_VIEW_FRAME_GROUP;      // frames a lane walks with one tap state
constexpr int RP_PX = 4;                       // pixels a lane owns: 4 x 1 (BGR), 2 x 2 (I420)

struct ReprojJob { const float *mx, *my; size_t mxstep, mystep; int cols, rows, dst_x, dst_y, tile0, tiles_x; };
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

#define RP_GLOBAL __attribute__((address_space(1)))
typedef unsigned rp_u32x2_a1 __attribute__((ext_vector_type(2), aligned(1)));
typedef unsigned rp_u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));

// the two BGR pixels of a tap row: lo = B1 G1 R1 B2, hi = G2 R2 x x (the unaligned 8-byte tap window of tile_kernels.hpp)
struct RpRow { unsigned lo, hi; };
__device__ __forceinline__ RpRow rp_load8(const uint8_t *p)
{
    const rp_u32x2_a1 v = *(const RP_GLOBAL rp_u32x2_a1 *)(uintptr_t)p;
    return RpRow{v.x, v.y};
}
__device__ __forceinline__ unsigned rp_load_px(const uint8_t *p)      // one pixel, three byte reads: the seam / edge form
{
    const RP_GLOBAL uint8_t *g = (const RP_GLOBAL uint8_t *)(uintptr_t)p;
    return (unsigned)g[0] | ((unsigned)g[1] << 8) | ((unsigned)g[2] << 16);
}
__device__ __forceinline__ float rp_ch(const RpRow &r, int tap, int c)
{
    const int b = 3 * tap + c;
    const unsigned w = b < 4 ? r.lo : r.hi;
    return (float)((w >> (8 * (b & 3))) & 0xffu);          // v_cvt_f32_ubyteN
}

// A pixel's tap state, built once from its map entry.  Coordinates are those of the EXTENDED source (one column either side, one row above and below), i.e. the
// map entry plus 1 in fp32; an extended column e is source column e - 1, column cols - 1 / 0 at e = 0 / cols + 1 when the source wraps, nothing otherwise; rows
// likewise with clamp (edge row repeated).
enum { RP_FAST = 1, RP_X1 = 2, RP_X2 = 4, RP_Y1 = 8, RP_Y2 = 16, RP_ACTIVE = 32 };
struct RpTaps {
    unsigned o1, o2;       // byte offsets of the two tap rows (0 where the row reads nothing)
    int cb1, cb2;          // byte offsets of the two tap columns inside a row (0 where the column reads nothing)
    float w11, w12, w21, w22;
    unsigned flags;
};
__device__ __forceinline__ bool rp_axis(int e, int n, bool edge_ok, int lo_src, int hi_src, int &s)
{
    if ((unsigned)e - 1u < (unsigned)n) { s = e - 1; return true; }
    if (edge_ok && e == 0) { s = lo_src; return true; }
    if (edge_ok && e == n + 1) { s = hi_src; return true; }
    s = 0;
    return false;
}
__device__ __forceinline__ RpTaps rp_make_taps(float xc, float yc, const ReprojArgs &A)
{
    RpTaps t;
    const float xe = xc + 1.f, ye = yc + 1.f;
    // k_remap_linear's arithmetic (prims.hip bilinear_taps) from here on
    const int x1 = f2i_rd(xe), y1 = f2i_rd(ye);
    const int x2 = (int)((unsigned)x1 + 1u), y2 = (int)((unsigned)y1 + 1u);
    const float wx2 = (float)x2 - xe, wx1 = xe - (float)x1;
    const float wy2 = (float)y2 - ye, wy1 = ye - (float)y1;
    t.w11 = wx2 * wy2; t.w12 = wx1 * wy2; t.w21 = wx2 * wy1; t.w22 = wx1 * wy1;
    int c1, c2, r1, r2;
    const bool vx1 = rp_axis(x1, A.scols, A.wrap != 0, A.scols - 1, 0, c1), vx2 = rp_axis(x2, A.scols, A.wrap != 0, A.scols - 1, 0, c2);
    const bool vy1 = rp_axis(y1, A.srows, A.clamp != 0, 0, A.srows - 1, r1), vy2 = rp_axis(y2, A.srows, A.clamp != 0, 0, A.srows - 1, r2);
    t.o1 = (unsigned)r1 * A.sstep; t.o2 = (unsigned)r2 * A.sstep;
    t.cb1 = 3 * c1; t.cb2 = 3 * c2;
    // the common case: both taps of a row adjacent and inside, the 8-byte window inside the row (c1 + 2 < cols), both rows readable
    const bool fast = vx1 && vx2 && vy1 && vy2 && c2 == c1 + 1 && c1 + 2 < A.scols;
    t.flags = (fast ? RP_FAST : 0u) | (vx1 ? RP_X1 : 0u) | (vx2 ? RP_X2 : 0u) | (vy1 ? RP_Y1 : 0u) | (vy2 ? RP_Y2 : 0u) | RP_ACTIVE;
    return t;
}
// the six tap bytes of one row; a tap that reads nothing is 0 (BORDER_CONSTANT), and still goes through the fma chain with its weight, as in k_remap_linear
__device__ __forceinline__ RpRow rp_row(const uint8_t *S, unsigned o, const RpTaps &t, bool row_ok)
{
    if (t.flags & RP_FAST) return rp_load8(S + o + (unsigned)t.cb1);
    const unsigned p1 = (row_ok && (t.flags & RP_X1)) ? rp_load_px(S + o + (unsigned)t.cb1) : 0u;
    const unsigned p2 = (row_ok && (t.flags & RP_X2)) ? rp_load_px(S + o + (unsigned)t.cb2) : 0u;
    return RpRow{p1 | (p2 << 24), p2 >> 8};
}
__device__ __forceinline__ void rp_blend(const RpTaps &t, const RpRow &r1, const RpRow &r2, float out[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float o = __builtin_fmaf(rp_ch(r1, 0, c), t.w11, 0.f);
        o = __builtin_fmaf(rp_ch(r1, 1, c), t.w12, o);
        o = __builtin_fmaf(rp_ch(r2, 0, c), t.w21, o);
        o = __builtin_fmaf(rp_ch(r2, 1, c), t.w22, o);
        out[c] = o;
    }
}
// clamp((a >> 20), 0, 255) behind an empty asm: neighbouring results packed into one word must not fuse into gfx950's miscompiled pack instruction (prims.hip, clamp_u8_opaque)
__device__ __forceinline__ unsigned rp_clamp_u8(int v) { int r = min(max(v, 0), 255); asm("" : "+v"(r)); return (unsigned)r; }

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
#pragma unroll
                for (int c = 0; c < 3; ++c) w[(3 * k + c) >> 2] = sat_u8_into(o[c], (unsigned)((3 * k + c) & 3), w[(3 * k + c) >> 2]);
            }
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
            // ms_bgr_to_i420's formula (prims.hip bgr_to_i420_cell) on the pixels ms_reproject(MS_VIEW_BGR) would have stored
            constexpr int SH = 20, HALF = 1 << (SH - 1);
            constexpr int CRY = 269484, CGY = 528482, CBY = 102760, CRU = -155188, CGU = -305135, CBU = 460324, CGV = -385875, CBV = -74448;
            unsigned yq[2] = {0u, 0u}, uq = 0u, vq = 0u;
#pragma unroll
            for (int k = 0; k < RP_PX; ++k) {
                float o[3];
                rp_blend(T[k], r1[k], r2[k], o);
                const int b = (int)sat_u8(o[0]), g = (int)sat_u8(o[1]), rr = (int)sat_u8(o[2]);
                yq[k >> 1] |= rp_clamp_u8((CRY * rr + CGY * g + CBY * b + HALF + (16 << SH)) >> SH) << (8 * (k & 1));
                if (k == 0) {
                    uq = rp_clamp_u8((CRU * rr + CGU * g + CBU * b + HALF + (128 << SH)) >> SH);
                    vq = rp_clamp_u8((CBU * rr + CGV * g + CBV * b + HALF + (128 << SH)) >> SH);
                }
            }
            const size_t W = (size_t)A.dcols, H = (size_t)A.drows;
            RP_GLOBAL uint8_t *Y = (RP_GLOBAL uint8_t *)(uintptr_t)A.dst[f], *U = Y + W * H, *V = U + (W / 2) * (H / 2);
            // dx, dy and W are even: the two luma bytes of a row are one aligned 16-bit store
            *(RP_GLOBAL unsigned short *)(Y + (size_t)dy * W + dx) = (unsigned short)yq[0];
            *(RP_GLOBAL unsigned short *)(Y + (size_t)(dy + 1) * W + dx) = (unsigned short)yq[1];
            U[(size_t)(dy / 2) * (W / 2) + dx / 2] = (uint8_t)uq;
            V[(size_t)(dy / 2) * (W / 2) + dx / 2] = (uint8_t)vq;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side

static bool finite9(const float *m) { for (int i = 0; i < 9; ++i) if (!std::isfinite(m[i])) return false; return true; }
static int check_proj(const char *fn, const char *what, int proj)
{
    if (proj == MS_PROJ_PLANE) return fail(MS_ERR_UNSUPPORTED, "%s: %s is MS_PROJ_PLANE: virtual cameras are built for spherical and cylindrical panoramas", fn, what);
    MS_CHECK(proj == MS_PROJ_SPHERICAL || proj == MS_PROJ_CYLINDRICAL, "%s: %s: unknown projection %d", fn, what, proj);
    return MS_OK;
}
static int check_scale(const char *fn, const char *what, float s)
{
    MS_CHECK(std::isfinite(s) && s > 0.f && s <= 8192.f, "%s: %s %g outside (0, 8192]", fn, what, (double)s);
    return MS_OK;
}
static int check_side(const char *fn, const char *what, int w, int h)
{
    MS_CHECK(w >= 1 && w <= 32767 && h >= 1 && h <= 32767, "%s: %s %d x %d outside [1, 32767]", fn, what, w, h);
    return MS_OK;
}
static int check_view_map(const char *fn, const char *what, const ms_image &m)
{
    MS_CHECK(m.data, "%s: %s has no data", fn, what);
    MS_CHECK(m.type == MS_32FC1, "%s: %s must be 32FC1 (type code %d, got %d)", fn, what, MS_32FC1, m.type);
    MS_CHECK(m.cols >= 1 && m.rows >= 1 && m.step >= (size_t)m.cols * 4, "%s: %s: empty image or step %zu below a row of %d floats", fn, what, m.step, m.cols);
    MS_CHECK(((uintptr_t)m.data & 3) == 0 && (m.step & 3) == 0, "%s: %s: data and step must be 4-byte aligned", fn, what);
    return MS_OK;
}

static void rot_mul(const double *a, const double *b, double *o)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_look_at_view(double yaw_deg, double pitch_deg, double roll_deg, double hfov_deg, int width, int height, ms_view *out)
{
    const char *fn = "ms_look_at_view";
    MS_CHECK(out, "%s: null out", fn);
    MS_CHECK(std::isfinite(yaw_deg) && std::isfinite(pitch_deg) && std::isfinite(roll_deg), "%s: yaw, pitch and roll must be finite", fn);
    MS_CHECK(hfov_deg > 0.0 && hfov_deg <= 179.0, "%s: hfov_deg %g outside (0, 179]", fn, hfov_deg);
    if (int e = check_side(fn, "width x height", width, height)) return e;
    const double D = LENS_PI / 180.0, ya = yaw_deg * D, pa = pitch_deg * D, ra = roll_deg * D;
    const double Ry[9] = {cos(ya), 0, sin(ya), 0, 1, 0, -sin(ya), 0, cos(ya)};
    const double Rx[9] = {1, 0, 0, 0, cos(pa), -sin(pa), 0, sin(pa), cos(pa)};
    const double Rz[9] = {cos(ra), -sin(ra), 0, sin(ra), cos(ra), 0, 0, 0, 1};
    double Ryx[9], R[9];
    rot_mul(Ry, Rx, Ryx);
    rot_mul(Ryx, Rz, R);
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
    MS_CHECK(view->struct_size == sizeof(ms_view), "%s: ms_view.struct_size %u, this library's is %zu", fn, view->struct_size, sizeof(ms_view));
    MS_CHECK(view->kind == MS_VIEW_CAMERA || view->kind == MS_VIEW_SURFACE, "%s: view kind %d is neither MS_VIEW_CAMERA nor MS_VIEW_SURFACE", fn, view->kind);
    if (int e = check_proj(fn, "src projection", src->projection)) return e;
    if (int e = check_scale(fn, "src scale", src->scale)) return e;
    MS_CHECK(src->wrap_cols >= 0, "%s: src wrap_cols %d is negative", fn, src->wrap_cols);
    MS_CHECK(src->clamp_rows == 0 || src->clamp_rows == 1, "%s: src clamp_rows %d is neither 0 nor 1", fn, src->clamp_rows);
    if (int e = check_side(fn, "view width x height", view->width, view->height)) return e;
    MS_CHECK(finite9(view->R), "%s: view R is not finite", fn);
    const ms_lens *lens = nullptr;
    if (view->kind == MS_VIEW_CAMERA) {
        MS_CHECK(finite9(view->K), "%s: view K is not finite", fn);
        MS_CHECK(view->K[0] != 0.f && view->K[4] != 0.f, "%s: view K[0] = %g and K[4] = %g must not be zero", fn, (double)view->K[0], (double)view->K[4]);
        if (view->lens.model != MS_LENS_NONE) {
            if (int e = lens_check("ms_build_view_maps: view lens", &view->lens)) return e;
            lens = &view->lens;
        }
    } else {
        if (int e = check_proj(fn, "view projection", view->projection)) return e;
        if (int e = check_scale(fn, "view scale", view->scale)) return e;
    }
    if (int e = check_view_map(fn, "map_x", *map_x)) return e;
    if (int e = check_view_map(fn, "map_y", *map_y)) return e;
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
    MS_CHECK(src && dst && jobs, "%s: null argument (src / dst / jobs)", fn);
    MS_CHECK(n_frames >= 1 && n_frames <= MS_VIEW_MAX_FRAMES, "%s: n_frames = %d outside [1, %d]", fn, n_frames, MS_VIEW_MAX_FRAMES);
    MS_CHECK(n_jobs >= 1 && n_jobs <= MS_VIEW_MAX_JOBS, "%s: n_jobs = %d outside [1, %d]", fn, n_jobs, MS_VIEW_MAX_JOBS);
    MS_CHECK(format == MS_VIEW_BGR || format == MS_VIEW_I420, "%s: format %d is neither MS_VIEW_BGR nor MS_VIEW_I420", fn, format);
    const bool i420 = format == MS_VIEW_I420;
    const ms_image &s0 = src[0], &d0 = dst[0];
    for (int f = 0; f < n_frames; ++f) {
        const ms_image &s = src[f];
        MS_CHECK(s.data && s.type == MS_8UC3 && s.cols >= 1 && s.rows >= 1 && s.step >= (size_t)s.cols * 3, "%s: src frame %d must be a non-empty 8UC3 image", fn, f);
        MS_CHECK(s.cols == s0.cols && s.rows == s0.rows && s.step == s0.step, "%s: src frame %d differs in geometry from frame 0", fn, f);
    }
    MS_CHECK(s0.step < ((size_t)1 << 24) && (unsigned long long)s0.rows * s0.step < (1ull << 32), "%s: src step %zu must be below 2^24 and rows * step below 2^32", fn, s0.step);
    MS_CHECK(wrap_cols == 0 || wrap_cols == s0.cols, "%s: wrap_cols %d is neither 0 nor the source's %d columns", fn, wrap_cols, s0.cols);
    MS_CHECK(clamp_rows == 0 || clamp_rows == 1, "%s: clamp_rows %d is neither 0 nor 1", fn, clamp_rows);
    for (int f = 0; f < n_frames; ++f) {
        const ms_image &d = dst[f];
        MS_CHECK(d.data && d.cols >= 1 && d.rows >= 1 && d.type == (i420 ? MS_8UC1 : MS_8UC3) && d.step >= (size_t)d.cols * (i420 ? 1 : 3),
                 "%s: dst frame %d must be a non-empty %s image", fn, f, i420 ? "8UC1 (planar I420)" : "8UC3");
        MS_CHECK(d.cols == d0.cols && d.rows == d0.rows && d.step == d0.step, "%s: dst frame %d differs in geometry from frame 0", fn, f);
    }
    int fw = d0.cols, fh = d0.rows;      // the frame the rectangles lie in
    if (i420) {
        MS_CHECK(d0.step == (size_t)d0.cols, "%s: an I420 dst must be contiguous (step %zu, %d columns)", fn, d0.step, d0.cols);
        MS_CHECK(d0.rows % 3 == 0 && d0.cols % 2 == 0 && (d0.rows / 3 * 2) % 2 == 0, "%s: an I420 dst is (rows * 3 / 2) x cols of an even-sized frame, not %d x %d", fn, d0.rows, d0.cols);
        fh = d0.rows / 3 * 2;
    }
    int tiles = 0;
    ReprojArgs A{};
    for (int j = 0; j < n_jobs; ++j) {
        const ms_view_job &J = jobs[j];
        char name[48];
        snprintf(name, sizeof(name), "jobs[%d].map_x", j);
        if (int e = check_view_map(fn, name, J.map_x)) return e;
        snprintf(name, sizeof(name), "jobs[%d].map_y", j);
        if (int e = check_view_map(fn, name, J.map_y)) return e;
        MS_CHECK(J.map_x.cols == J.map_y.cols && J.map_x.rows == J.map_y.rows, "%s: jobs[%d]: map_x is %d x %d, map_y %d x %d", fn, j, J.map_x.cols, J.map_x.rows, J.map_y.cols, J.map_y.rows);
        if (int e = check_side(fn, "a job's maps", J.map_x.cols, J.map_x.rows)) return e;
        const int w = J.map_x.cols, h = J.map_x.rows;
        MS_CHECK(J.dst_x >= 0 && J.dst_y >= 0 && (long long)J.dst_x + w <= fw && (long long)J.dst_y + h <= fh,
                 "%s: jobs[%d]: the rectangle (%d, %d, %d x %d) leaves the %d x %d dst", fn, j, J.dst_x, J.dst_y, w, h, fw, fh);
        if (i420) MS_CHECK(J.dst_x % 2 == 0 && J.dst_y % 2 == 0 && w % 2 == 0 && h % 2 == 0, "%s: jobs[%d]: an I420 rectangle (%d, %d, %d x %d) must be even", fn, j, J.dst_x, J.dst_y, w, h);
        for (int k = 0; k < j; ++k) {
            const ms_view_job &P = jobs[k];
            MS_CHECK(J.dst_x >= P.dst_x + P.map_x.cols || P.dst_x >= J.dst_x + w || J.dst_y >= P.dst_y + P.map_x.rows || P.dst_y >= J.dst_y + h,
                     "%s: the rectangles of jobs[%d] and jobs[%d] overlap", fn, k, j);
        }
        ReprojJob &R = A.job[j];
        R.mx = (const float *)J.map_x.data; R.my = (const float *)J.map_y.data; R.mxstep = J.map_x.step; R.mystep = J.map_y.step;
        R.cols = w; R.rows = h; R.dst_x = J.dst_x; R.dst_y = J.dst_y;
        R.tile0 = tiles;
        R.tiles_x = i420 ? div_up(w, 32) : div_up(w, MS_VIEW_TILE_W);
        tiles += R.tiles_x * (i420 ? div_up(h, 32) : div_up(h, MS_VIEW_TILE_H));
    }
    const size_t s_bytes = (size_t)(s0.rows - 1) * s0.step + (size_t)s0.cols * 3;
    const size_t d_bytes = (size_t)(d0.rows - 1) * d0.step + (size_t)d0.cols * (i420 ? 1 : 3);
    for (int f = 0; f < n_frames; ++f)
        for (int g = 0; g < n_frames; ++g) {
            const uintptr_t a = (uintptr_t)dst[f].data, b = (uintptr_t)src[g].data;
            MS_CHECK(a + d_bytes <= b || b + s_bytes <= a, "%s: dst frame %d overlaps src frame %d in memory", fn, f, g);
        }
    if (int e = require_device()) return e;
    for (int f = 0; f < n_frames; ++f) { A.src[f] = (const uint8_t *)src[f].data; A.dst[f] = (uint8_t *)dst[f].data; }
    A.dstep = d0.step;
    A.n_jobs = n_jobs; A.n_frames = n_frames;
    A.sstep = (unsigned)s0.step; A.scols = s0.cols; A.srows = s0.rows;
    A.dcols = fw; A.drows = fh;
    A.wrap = wrap_cols != 0; A.clamp = clamp_rows;
    const dim3 grid(tiles, div_up(n_frames, RP_G));
    if (i420) k_reproject<MS_VIEW_I420><<<grid, 256, 0, as_stream(stream)>>>(A);
    else k_reproject<MS_VIEW_BGR><<<grid, 256, 0, as_stream(stream)>>>(A);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

}  // extern "C"
