// reproject.hpp -- what the three samplers of the virtual cameras share (include/ms_stitch.h section 5): ms_reproject (reproject.hip), ms_reproject_aa
// (reproject_aa.hip) and ms_reproject_poses (reproject_poses.hip).  The tap state of cuda::remap(INTER_LINEAR, BORDER_CONSTANT) on a source that wraps at the +-pi
// seam and repeats its pole rows, its row reads and fma chain, the BGR / I420 store of a lane's four pixels, the coordinates of a view ray in the panorama image
// (ms_build_view_maps' and ms_reproject_poses'), and the host-side argument checks and job table of a call.
#pragma once
#include <cmath>
#include <cstdio>
#include "ctx.hpp"

namespace ms {

constexpr int RP_G = MS_VIEW_FRAME_GROUP;      // frames a lane walks with one tap state
constexpr int RP_PX = 4;                       // pixels a lane owns: 4 x 1 (BGR), 2 x 2 (I420)

struct ReprojJob { const float *mx, *my; size_t mxstep, mystep; int cols, rows, dst_x, dst_y, tile0, tiles_x; };

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
// A: the sampled image's geometry -- scols, srows, sstep, wrap, clamp (the kernel argument of ms_reproject; one level of ms_reproject_aa)
template <class Geom>
__device__ __forceinline__ RpTaps rp_make_taps(float xc, float yc, const Geom &A)
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

// A lane's four BGR pixels, saturated as ms_remap saturates: 12 bytes in three words, then into row dy of frame f at column dx -- n_px of the four pixels lie
// inside the view.  A: the kernel argument (dst, dstep).
__device__ __forceinline__ void rp_pack_bgr(const float (&o)[3], int k, unsigned (&w)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) w[(3 * k + c) >> 2] = sat_u8_into(o[c], (unsigned)((3 * k + c) & 3), w[(3 * k + c) >> 2]);
}
template <class Args>
__device__ __forceinline__ void rp_store_bgr(const Args &A, int f, int dx, int dy, int n_px, const unsigned (&w)[3])
{
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
}
// A lane's 2 x 2 block as I420: ms_bgr_to_i420's formula (prims.hip bgr_to_i420_cell) on the pixels the BGR form would have stored -- Y from every pixel,
// U and V from the top-left one.  A: the kernel argument (dst, dcols, drows: the frame's size W x H, the planes' geometry).
__device__ __forceinline__ void rp_pack_i420(const float o[3], int k, unsigned yq[2], unsigned &uq, unsigned &vq)
{
    constexpr int SH = 20, HALF = 1 << (SH - 1);
    constexpr int CRY = 269484, CGY = 528482, CBY = 102760, CRU = -155188, CGU = -305135, CBU = 460324, CGV = -385875, CBV = -74448;
    const int b = (int)sat_u8(o[0]), g = (int)sat_u8(o[1]), rr = (int)sat_u8(o[2]);
    yq[k >> 1] |= rp_clamp_u8((CRY * rr + CGY * g + CBY * b + HALF + (16 << SH)) >> SH) << (8 * (k & 1));
    if (k == 0) {
        uq = rp_clamp_u8((CRU * rr + CGU * g + CBU * b + HALF + (128 << SH)) >> SH);
        vq = rp_clamp_u8((CBU * rr + CGV * g + CBV * b + HALF + (128 << SH)) >> SH);
    }
}
template <class Args>
__device__ __forceinline__ void rp_store_i420(const Args &A, int f, int dx, int dy, const unsigned yq[2], unsigned uq, unsigned vq)
{
    const size_t W = (size_t)A.dcols, H = (size_t)A.drows;
    RP_GLOBAL uint8_t *Y = (RP_GLOBAL uint8_t *)(uintptr_t)A.dst[f], *U = Y + W * H, *V = U + (W / 2) * (H / 2);
    // dx, dy and W are even: the two luma bytes of a row are one aligned 16-bit store
    *(RP_GLOBAL unsigned short *)(Y + (size_t)dy * W + dx) = (unsigned short)yq[0];
    *(RP_GLOBAL unsigned short *)(Y + (size_t)(dy + 1) * W + dx) = (unsigned short)yq[1];
    U[(size_t)(dy / 2) * (W / 2) + dx / 2] = (uint8_t)uq;
    V[(size_t)(dy / 2) * (W / 2) + dx / 2] = (uint8_t)vq;
}

// Steps 2 to 4 of ms_build_view_maps (include/ms_stitch.h): the view ray c under the rotation r (view to rig, row-major) -> the rig direction -> panorama
// coordinates (mapForward) -> image coordinates with the wrap rule, in double, rounded to float once.  ONE copy: k_view_maps (reproject.hip) stores the two floats,
// k_reproject_poses (reproject_poses.hip) samples at them; the library is built with -ffp-contract=off, so the same source gives the same bits in both.
// seen: the view sees the pixel (step 1); an unseen pixel, and a direction a cylindrical panorama does not see (h == 0), is the entry (-1, -1).
__device__ __forceinline__ void rp_pano_coords(bool seen, const double *r, const double *c, double S, int src_proj, int u0, int v0, int wrap, float &out_x, float &out_y)
{
    float ox = -1.f, oy = -1.f;
    if (seen) {
        const double d0 = r[0] * c[0] + r[1] * c[1] + r[2] * c[2], d1 = r[3] * c[0] + r[4] * c[1] + r[5] * c[2], d2 = r[6] * c[0] + r[7] * c[1] + r[8] * c[2];
        const double h = hypot(d0, d2);
        const double U = S * atan2(d0, d2);
        double V = 0.0;
        if (src_proj == MS_PROJ_SPHERICAL) V = S * atan2(h, -d1);
        else if (h == 0.0) seen = false;
        else V = S * d1 / h;
        if (seen) {
            double X = U - (double)u0;
            const double Y = V - (double)v0;
            if (wrap > 0) X -= (double)wrap * floor(X / (double)wrap);
            ox = (float)X; oy = (float)Y;
            if (wrap > 0 && ox == (float)wrap) ox = 0.f;
        }
    }
    out_x = ox; out_y = oy;
}

// ------------------------------------------------------------------------------------------------
// host side: the checks the entry points of section 5 share

// o = a b for row-major 3 x 3 matrices, each product summed left to right (ms_look_at_view's Ry Rx Rz, ms_view_pose_table's P R)
static inline void rp_rot_mul(const double *a, const double *b, double *o)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

static inline int rp_check_proj(const char *fn, const char *what, int proj)
{
    if (proj == MS_PROJ_PLANE) return fail(MS_ERR_UNSUPPORTED, "%s: %s is MS_PROJ_PLANE: virtual cameras are built for spherical and cylindrical panoramas", fn, what);
    MS_CHECK(proj == MS_PROJ_SPHERICAL || proj == MS_PROJ_CYLINDRICAL, "%s: %s: unknown projection %d", fn, what, proj);
    return MS_OK;
}
static inline int rp_check_scale(const char *fn, const char *what, float s)
{
    MS_CHECK(std::isfinite(s) && s > 0.f && s <= 8192.f, "%s: %s %g outside (0, 8192]", fn, what, (double)s);
    return MS_OK;
}
static inline int rp_check_side(const char *fn, const char *what, int w, int h)
{
    MS_CHECK(w >= 1 && w <= 32767 && h >= 1 && h <= 32767, "%s: %s %d x %d outside [1, 32767]", fn, what, w, h);
    return MS_OK;
}
static inline int rp_check_view_map(const char *fn, const char *what, const ms_image &m)
{
    MS_CHECK(m.data, "%s: %s has no data", fn, what);
    MS_CHECK(m.type == MS_32FC1, "%s: %s must be 32FC1 (type code %d, got %d)", fn, what, MS_32FC1, m.type);
    MS_CHECK(m.cols >= 1 && m.rows >= 1 && m.step >= (size_t)m.cols * 4, "%s: %s: empty image or step %zu below a row of %d floats", fn, what, m.step, m.cols);
    MS_CHECK(((uintptr_t)m.data & 3) == 0 && (m.step & 3) == 0, "%s: %s: data and step must be 4-byte aligned", fn, what);
    return MS_OK;
}
// ms_build_view_maps' checks on the panorama frame
static inline int rp_check_pano_frame(const char *fn, const ms_pano_frame *src)
{
    MS_CHECK(src->struct_size == sizeof(ms_pano_frame), "%s: ms_pano_frame.struct_size %u, this library's is %zu", fn, src->struct_size, sizeof(ms_pano_frame));
    if (int e = rp_check_proj(fn, "src projection", src->projection)) return e;
    if (int e = rp_check_scale(fn, "src scale", src->scale)) return e;
    MS_CHECK(src->wrap_cols >= 0, "%s: src wrap_cols %d is negative", fn, src->wrap_cols);
    MS_CHECK(src->clamp_rows == 0 || src->clamp_rows == 1, "%s: src clamp_rows %d is neither 0 nor 1", fn, src->clamp_rows);
    return MS_OK;
}

// ms_build_view_maps' checks on a view (`what` names it: "view", "jobs[2].view"); *lens is the view's lens, or null for a pinhole / a surface.  check_R: R must be
// finite (ms_reproject_poses takes its rotations from the pose table and never reads view.R).
static inline int rp_check_view(const char *fn, const char *what, const ms_view *view, bool check_R, const ms_lens **lens)
{
    char name[96];
    MS_CHECK(view->struct_size == sizeof(ms_view), "%s: %s: ms_view.struct_size %u, this library's is %zu", fn, what, view->struct_size, sizeof(ms_view));
    MS_CHECK(view->kind == MS_VIEW_CAMERA || view->kind == MS_VIEW_SURFACE, "%s: %s kind %d is neither MS_VIEW_CAMERA nor MS_VIEW_SURFACE", fn, what, view->kind);
    snprintf(name, sizeof(name), "%s width x height", what);
    if (int e = rp_check_side(fn, name, view->width, view->height)) return e;
    auto finite9 = [](const float *m) { for (int i = 0; i < 9; ++i) if (!std::isfinite(m[i])) return false; return true; };
    if (check_R) MS_CHECK(finite9(view->R), "%s: %s R is not finite", fn, what);
    *lens = nullptr;
    if (view->kind == MS_VIEW_CAMERA) {
        MS_CHECK(finite9(view->K), "%s: %s K is not finite", fn, what);
        MS_CHECK(view->K[0] != 0.f && view->K[4] != 0.f, "%s: %s K[0] = %g and K[4] = %g must not be zero", fn, what, (double)view->K[0], (double)view->K[4]);
        if (view->lens.model != MS_LENS_NONE) {
            snprintf(name, sizeof(name), "%s: %s lens", fn, what);
            if (int e = lens_check(name, &view->lens)) return e;
            *lens = &view->lens;
        }
    } else {
        snprintf(name, sizeof(name), "%s projection", what);
        if (int e = rp_check_proj(fn, name, view->projection)) return e;
        snprintf(name, sizeof(name), "%s scale", what);
        if (int e = rp_check_scale(fn, name, view->scale)) return e;
    }
    return MS_OK;
}

// What every sampler of section 5 refuses about its frames and rectangles, and the tile layout of its launch: the counts, the format, the source and destination
// frames, each job's rectangle (inside dst, even for I420, disjoint from the earlier ones) and dst against src in memory.  job_rect(j, rect) checks what is the
// caller's own about job j -- its maps (ms_reproject, ms_reproject_aa) or its view (ms_reproject_poses) -- and names the rectangle.
struct RpRect { int w, h, dst_x, dst_y; };
struct RpLayout { RpRect rect[MS_VIEW_MAX_JOBS]; int tile0[MS_VIEW_MAX_JOBS], tiles_x[MS_VIEW_MAX_JOBS]; int tiles, fw, fh; };
template <class JobRect>
static inline int rp_layout(const char *fn, const ms_image *src, ms_image *dst, int n_frames, int n_jobs, int max_jobs, int wrap_cols, int clamp_rows, int format,
                            JobRect job_rect, RpLayout &L)
{
    MS_CHECK(n_frames >= 1 && n_frames <= MS_VIEW_MAX_FRAMES, "%s: n_frames = %d outside [1, %d]", fn, n_frames, MS_VIEW_MAX_FRAMES);
    MS_CHECK(n_jobs >= 1 && n_jobs <= max_jobs, "%s: n_jobs = %d outside [1, %d]", fn, n_jobs, max_jobs);
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
    for (int j = 0; j < n_jobs; ++j) {
        RpRect &J = L.rect[j];
        if (int e = job_rect(j, J)) return e;
        MS_CHECK(J.dst_x >= 0 && J.dst_y >= 0 && (long long)J.dst_x + J.w <= fw && (long long)J.dst_y + J.h <= fh,
                 "%s: jobs[%d]: the rectangle (%d, %d, %d x %d) leaves the %d x %d dst", fn, j, J.dst_x, J.dst_y, J.w, J.h, fw, fh);
        if (i420) MS_CHECK(J.dst_x % 2 == 0 && J.dst_y % 2 == 0 && J.w % 2 == 0 && J.h % 2 == 0, "%s: jobs[%d]: an I420 rectangle (%d, %d, %d x %d) must be even", fn, j, J.dst_x, J.dst_y, J.w, J.h);
        for (int k = 0; k < j; ++k) {
            const RpRect &Q = L.rect[k];
            MS_CHECK(J.dst_x >= Q.dst_x + Q.w || Q.dst_x >= J.dst_x + J.w || J.dst_y >= Q.dst_y + Q.h || Q.dst_y >= J.dst_y + J.h,
                     "%s: the rectangles of jobs[%d] and jobs[%d] overlap", fn, k, j);
        }
        L.tile0[j] = tiles;
        L.tiles_x[j] = i420 ? div_up(J.w, 32) : div_up(J.w, MS_VIEW_TILE_W);
        tiles += L.tiles_x[j] * (i420 ? div_up(J.h, 32) : div_up(J.h, MS_VIEW_TILE_H));
    }
    const size_t s_bytes = (size_t)(s0.rows - 1) * s0.step + (size_t)s0.cols * 3;
    const size_t d_bytes = (size_t)(d0.rows - 1) * d0.step + (size_t)d0.cols * (i420 ? 1 : 3);
    for (int f = 0; f < n_frames; ++f)
        for (int g = 0; g < n_frames; ++g) {
            const uintptr_t a = (uintptr_t)dst[f].data, b = (uintptr_t)src[g].data;
            MS_CHECK(a + d_bytes <= b || b + s_bytes <= a, "%s: dst frame %d overlaps src frame %d in memory", fn, f, g);
        }
    L.tiles = tiles; L.fw = fw; L.fh = fh;
    return MS_OK;
}

// Everything ms_reproject refuses, and what its launch needs: the job table, the tile count and the frame the rectangles lie in.  `jobs` is walked with
// job_stride bytes between entries (ms_view_job, or the ms_view_job at the head of an ms_view_job_aa).
struct RpPlan { ReprojJob job[MS_VIEW_MAX_JOBS]; int tiles, fw, fh; };
static inline int rp_plan(const char *fn, const ms_image *src, ms_image *dst, int n_frames, const void *jobs, size_t job_stride, int n_jobs, int wrap_cols, int clamp_rows,
                          int format, RpPlan &P)
{
    MS_CHECK(src && dst && jobs, "%s: null argument (src / dst / jobs)", fn);
    auto job_at = [&](int j) -> const ms_view_job & { return *(const ms_view_job *)((const char *)jobs + (size_t)j * job_stride); };
    RpLayout L;
    const int e = rp_layout(fn, src, dst, n_frames, n_jobs, MS_VIEW_MAX_JOBS, wrap_cols, clamp_rows, format, [&](int j, RpRect &r) -> int {
        const ms_view_job &J = job_at(j);
        char name[48];
        snprintf(name, sizeof(name), "jobs[%d].map_x", j);
        if (int e = rp_check_view_map(fn, name, J.map_x)) return e;
        snprintf(name, sizeof(name), "jobs[%d].map_y", j);
        if (int e = rp_check_view_map(fn, name, J.map_y)) return e;
        MS_CHECK(J.map_x.cols == J.map_y.cols && J.map_x.rows == J.map_y.rows, "%s: jobs[%d]: map_x is %d x %d, map_y %d x %d", fn, j, J.map_x.cols, J.map_x.rows, J.map_y.cols, J.map_y.rows);
        if (int e = rp_check_side(fn, "a job's maps", J.map_x.cols, J.map_x.rows)) return e;
        r = RpRect{J.map_x.cols, J.map_x.rows, J.dst_x, J.dst_y};
        return MS_OK;
    }, L);
    if (e) return e;
    for (int j = 0; j < n_jobs; ++j) {
        const ms_view_job &J = job_at(j);
        ReprojJob &R = P.job[j];
        R.mx = (const float *)J.map_x.data; R.my = (const float *)J.map_y.data; R.mxstep = J.map_x.step; R.mystep = J.map_y.step;
        R.cols = L.rect[j].w; R.rows = L.rect[j].h; R.dst_x = J.dst_x; R.dst_y = J.dst_y;
        R.tile0 = L.tile0[j]; R.tiles_x = L.tiles_x[j];
    }
    P.tiles = L.tiles; P.fw = L.fw; P.fh = L.fh;
    return MS_OK;
}

}  // namespace ms
