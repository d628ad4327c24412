// reproject_aa.hip -- antialiased virtual cameras (include/ms_stitch.h section 5): the panorama's mip chain (ms_pano_mips_layout, ms_build_pano_mips), the
// per-pixel footprint of a view (ms_build_view_footprint) and the trilinear sampler (ms_reproject_aa).
//   The chain is a cascaded 2 x 2 box with round-half-up, in integers: one launch takes a source to its next three levels -- a lane holds an 8 x 8 block,
// finishes its 4 x 4, 2 x 2 and 1 x 1 pixels in registers -- for every frame of the call (blockIdx.z); levels 4 and up are the same launch again on level 3.
//   The sampler is ms_reproject's kernel (reproject.hpp: same taps, weights, fma chain, saturation, stores) with two tap states per pixel, one per level of the
// pair its footprint falls between, and one fma between the two unsaturated results.  A wave whose pixels all stay on level 0 runs ms_reproject's loop.
#include <algorithm>
#include <cmath>
#include "ctx.hpp"
#include "lens.hpp"
#include "reproject.hpp"

namespace ms {

// ------------------------------------------------------------------------------------------------
// the chain's packing: every level's first byte on a 256-byte boundary of the buffer, its rows 16 bytes apart at least
constexpr size_t MIP_LEVEL_ALIGN = 256, MIP_STEP_ALIGN = 16, MIP_BASE_ALIGN = 16;

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static void mip_layout(int cols, int rows, int levels, ms_mip_level *out, size_t *bytes)
{
    size_t off = 0;
    for (int l = 0; l < levels; ++l) {
        cols = (cols + 1) / 2; rows = (rows + 1) / 2;
        out[l].offset = off; out[l].step = align_up((size_t)cols * 3, MIP_STEP_ALIGN); out[l].cols = cols; out[l].rows = rows;
        off += align_up(out[l].step * (size_t)rows, MIP_LEVEL_ALIGN);
    }
    *bytes = off;
}

// ------------------------------------------------------------------------------------------------
// ms_build_pano_mips

constexpr int MIP_PASS = 3;      // levels one launch makes
struct MipOut { size_t off; unsigned step; int cols, rows; };
struct MipArgs {
    const uint8_t *src[MS_VIEW_MAX_FRAMES];      // the pass's source: the panorama, or level 3 inside the mips buffer
    uint8_t *dst[MS_VIEW_MAX_FRAMES];            // the mips buffers
    size_t sstep;
    int scols, srows, nout;
    MipOut out[MIP_PASS];
};

typedef unsigned mip_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned mip_u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// byte j of a block row's 24 (8 BGR pixels in six words)
__device__ __forceinline__ unsigned mip_byte(const unsigned (&w)[6], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// The 24 bytes of columns 8 bx .. 8 bx + 7 of one source row.  Whole blocks: seven aligned words around the (arbitrarily aligned) 24 bytes, shifted into place;
// the seventh is read only when the 24 bytes reach into it, so every word read holds a byte of the row.  The block at the right edge: byte reads, a column past
// the last one reads the last one.
__device__ __forceinline__ void mip_load_row(const uint8_t *row, int bx, int scols, unsigned (&w)[6])
{
    if (8 * bx + 8 <= scols) {
        const uintptr_t p = (uintptr_t)row + 24u * (unsigned)bx;
        const unsigned a = (unsigned)p & 3u;
        const RP_GLOBAL uint8_t *q = (const RP_GLOBAL uint8_t *)(p - a);
        const mip_u32x4_a4 v0 = *(const RP_GLOBAL mip_u32x4_a4 *)q;
        const mip_u32x2_a4 v1 = *(const RP_GLOBAL mip_u32x2_a4 *)(q + 16);
        const unsigned v2 = a ? *(const RP_GLOBAL unsigned *)(q + 24) : 0u;
        const unsigned d[7] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v2};
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], a);
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const RP_GLOBAL uint8_t *g = (const RP_GLOBAL uint8_t *)((uintptr_t)row + 3u * (unsigned)min(8 * bx + k, scols - 1));
#pragma unroll
            for (int c = 0; c < 3; ++c) w[(3 * k + c) >> 2] |= (unsigned)g[c] << (8 * ((3 * k + c) & 3));
        }
    }
}

// the pixels (x, y) of an n x n block of a level, from the 2n x 2n block below it of which vc x vr lie inside that level: an index past the last column or row
// reads the last one (which, for an odd extent, is the pixel's own even partner -- always in this block)
template <int N>
__device__ __forceinline__ void mip_reduce(const unsigned (&a)[2 * N][2 * N][3], int vc, int vr, unsigned (&o)[N][N][3])
{
#pragma unroll
    for (int y = 0; y < N; ++y)
#pragma unroll
        for (int x = 0; x < N; ++x)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const bool xin = 2 * x + 1 < vc, yin = 2 * y + 1 < vr;
                const unsigned p00 = a[2 * y][2 * x][c], p01 = xin ? a[2 * y][2 * x + 1][c] : p00;
                const unsigned q10 = a[2 * y + 1][2 * x][c], q11 = a[2 * y + 1][2 * x + 1][c];
                const unsigned p10 = yin ? q10 : p00, p11 = yin ? (xin ? q11 : q10) : p01;
                o[y][x][c] = (p00 + p01 + p10 + p11 + 2u) >> 2;
            }
}
template <int N>
__device__ __forceinline__ void mip_store_bytes(uint8_t *base, const MipOut &L, int px0, int py0, const unsigned (&o)[N][N][3])
{
#pragma unroll
    for (int y = 0; y < N; ++y)
#pragma unroll
        for (int x = 0; x < N; ++x)
            if (px0 + x < L.cols && py0 + y < L.rows) {
                RP_GLOBAL uint8_t *g = (RP_GLOBAL uint8_t *)((uintptr_t)base + L.off + (size_t)(py0 + y) * L.step + 3u * (unsigned)(px0 + x));
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] = (uint8_t)o[y][x][c];
            }
}

// A workgroup = 32 x 8 lanes = 256 x 64 source pixels of one frame; a lane = one 8 x 8 block.  Adjacent lanes read adjacent 24 bytes of a row and write
// adjacent 12 bytes of a level-1 row.
__global__ void __launch_bounds__(256) k_pano_mips(const MipArgs A)
{
    const int bx = (int)blockIdx.x * 32 + ((int)threadIdx.x & 31), by = (int)blockIdx.y * 8 + ((int)threadIdx.x >> 5);
    if (8 * bx >= A.scols || 8 * by >= A.srows) return;
    const uint8_t *S = A.src[blockIdx.z];
    uint8_t *D = A.dst[blockIdx.z];

    unsigned l1[4][4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // two source rows (a row past the last one reads the last one) make one level-1 row; the loads clamp, so every index is "inside"
        unsigned w0[6], w1[6];
        mip_load_row(S + (size_t)min(8 * by + 2 * i, A.srows - 1) * A.sstep, bx, A.scols, w0);
        mip_load_row(S + (size_t)min(8 * by + 2 * i + 1, A.srows - 1) * A.sstep, bx, A.scols, w1);
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                l1[i][x][c] = (mip_byte(w0, 6 * x + c) + mip_byte(w0, 6 * x + 3 + c) + mip_byte(w1, 6 * x + c) + mip_byte(w1, 6 * x + 3 + c) + 2u) >> 2;
    }
    const MipOut &L1 = A.out[0];
    const int vc1 = L1.cols - 4 * bx, vr1 = L1.rows - 4 * by;      // level-1 pixels of this block inside the level: both >= 1
    if (vc1 >= 4) {
        // offset, step and the 12 bytes per lane keep every row's store word-aligned
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < vr1) {
                unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int c = 0; c < 3; ++c) w[(3 * x + c) >> 2] |= l1[i][x][c] << (8 * ((3 * x + c) & 3));
                rp_u32x3_a4 v; v.x = w[0]; v.y = w[1]; v.z = w[2];
                *(RP_GLOBAL rp_u32x3_a4 *)((uintptr_t)D + L1.off + (size_t)(4 * by + i) * L1.step + 12u * (unsigned)bx) = v;
            }
    } else {
        mip_store_bytes<4>(D, L1, 4 * bx, 4 * by, l1);
    }
    if (A.nout < 2) return;
    unsigned l2[2][2][3];
    mip_reduce<2>(l1, vc1, vr1, l2);
    const MipOut &L2 = A.out[1];
    mip_store_bytes<2>(D, L2, 2 * bx, 2 * by, l2);
    if (A.nout < 3) return;
    unsigned l3[1][1][3];
    mip_reduce<1>(l2, L2.cols - 2 * bx, L2.rows - 2 * by, l3);
    mip_store_bytes<1>(D, A.out[2], bx, by, l3);
}

// ------------------------------------------------------------------------------------------------
// ms_build_view_footprint

struct FootArgs {
    const float *mx, *my;
    float *rho;
    size_t mxstep, mystep, rstep;
    int cols, rows;
    double S, v0, W, fscale;      // W: wrap_cols (0 = none)
    int sph;
};

__device__ __forceinline__ bool foot_entry(const FootArgs &A, int x, int y, double &X, double &Y)
{
    if ((unsigned)x >= (unsigned)A.cols || (unsigned)y >= (unsigned)A.rows) return false;
    const float fx = row_ptr<float>(A.mx, A.mxstep, y)[x], fy = row_ptr<float>(A.my, A.mystep, y)[x];
    if ((fx == -1.f && fy == -1.f) || !__builtin_isfinite(fx) || !__builtin_isfinite(fy)) return false;
    X = (double)fx; Y = (double)fy;
    return true;
}
// |forward difference| (backward where the forward neighbour is absent, 0 where both are) of the map entry along (sx, sy), x component unwrapped and weighted
__device__ __forceinline__ double foot_step(const FootArgs &A, int x, int y, int sx, int sy, double X, double Y, double s)
{
    double Xn, Yn, dx = 0.0, dy = 0.0;
    if (foot_entry(A, x + sx, y + sy, Xn, Yn)) { dx = Xn - X; dy = Yn - Y; }
    else if (foot_entry(A, x - sx, y - sy, Xn, Yn)) { dx = X - Xn; dy = Y - Yn; }
    if (A.W > 0.0) dx = dx - A.W * floor(dx / A.W + 0.5);
    dx = dx * s;
    return hypot(dx, dy);
}
// one lane per pixel, 64 x 4 workgroups (k_view_maps' shape)
__global__ void __launch_bounds__(256) k_view_footprint(const FootArgs A)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.cols || y >= A.rows) return;
    double X, Y;
    float out = 0.f;
    if (foot_entry(A, x, y, X, Y)) {
        const double s = A.sph ? sin(fmin(fmax((Y + A.v0) / A.S, 0.0), LENS_PI)) : 1.0;
        const double a = foot_step(A, x, y, 1, 0, X, Y, s), b = foot_step(A, x, y, 0, 1, X, Y, s);
        out = (float)(A.fscale * fmax(a, b));
    }
    row_ptr<float>(A.rho, A.rstep, y)[x] = out;
}

// ------------------------------------------------------------------------------------------------
// ms_reproject_aa

struct AaLevel { unsigned off, sstep; int scols, srows; };      // level 0: the source itself (off 0); level k: inside the mips buffer
struct ReprojAaArgs {
    const uint8_t *src[MS_VIEW_MAX_FRAMES];
    const uint8_t *mips[MS_VIEW_MAX_FRAMES];
    uint8_t *dst[MS_VIEW_MAX_FRAMES];
    ReprojJob job[MS_VIEW_MAX_JOBS];
    const float *rho[MS_VIEW_MAX_JOBS];
    size_t rstep[MS_VIEW_MAX_JOBS];
    AaLevel lev[MS_VIEW_MAX_LEVELS + 1];
    size_t dstep;
    int n_jobs, n_frames, levels;
    int dcols, drows;
    int wrap, clamp;
};

enum { RP_MIP = 64 };      // beside reproject.hpp's flags: the tap rows lie in the mips buffer, not in the source
struct AaGeom { unsigned off, sstep; int scols, srows, wrap, clamp; };
// a pixel's state: the tap states on level l (a) and l + 1 (b: no flags where t == 0, it then reads nothing), and the weight of b
struct AaPx { RpTaps a, b; float t; };

// level k's geometry; k differs from lane to lane, the table lies in the kernel argument: a chain of selects, not an indexed read
__device__ __forceinline__ AaGeom aa_geom(const ReprojAaArgs &A, int k)
{
    AaGeom g{A.lev[0].off, A.lev[0].sstep, A.lev[0].scols, A.lev[0].srows, A.wrap, A.clamp};
#pragma unroll
    for (int i = 1; i <= MS_VIEW_MAX_LEVELS; ++i)
        if (k == i) { g.off = A.lev[i].off; g.sstep = A.lev[i].sstep; g.scols = A.lev[i].scols; g.srows = A.lev[i].srows; }
    return g;
}
__device__ __forceinline__ RpTaps aa_taps(const ReprojAaArgs &A, float X, float Y, int k)
{
    const float s = __builtin_bit_cast(float, (unsigned)(127 - k) << 23);      // 2^-k
    const float h = 0.5f * s - 0.5f;                                           // 2^-(k+1) - 0.5: exact
    const AaGeom g = aa_geom(A, k);
    RpTaps t = rp_make_taps(__builtin_fmaf(X, s, h), __builtin_fmaf(Y, s, h), g);
    t.o1 += g.off; t.o2 += g.off;
    if (k > 0) t.flags |= RP_MIP;
    return t;
}
__device__ __forceinline__ AaPx aa_make_px(const ReprojAaArgs &A, float X, float Y, float r, bool &two)
{
    int l = 0;
    float t = 0.f;
    if (r > 1.f) {
        l = (int)((__builtin_bit_cast(unsigned, r) >> 23) & 0xffu) - 127;      // floor(log2 r): r is positive and normal here
        if (l >= A.levels) l = A.levels;                                        // r >= 2^levels, +inf included
        else t = __builtin_fmaf(r, __builtin_bit_cast(float, (unsigned)(127 - l) << 23), -1.f);
    }
    AaPx p;
    p.t = t;
    p.a = aa_taps(A, X, Y, l);
    if (t != 0.f) p.b = aa_taps(A, X, Y, l + 1);
    else p.b = RpTaps{0u, 0u, 0, 0, 0.f, 0.f, 0.f, 0.f, 0u};
    two = two || l != 0 || t != 0.f;
    return p;
}

// the frames f0 .. f1 - 1 of a lane's four pixels.  TWO = false: every pixel of the wave stays on level 0 -- k_reproject's loop.
template <int FMT, bool TWO>
__device__ __forceinline__ void aa_frames(const ReprojAaArgs &A, const AaPx (&P)[RP_PX], int n_px, int dx, int dy, int f0, int f1)
{
    for (int f = f0; f < f1; ++f) {
        const uint8_t *S = A.src[f], *M = TWO ? A.mips[f] : nullptr;
        RpRow a1[RP_PX], a2[RP_PX], b1[RP_PX], b2[RP_PX];
#pragma unroll
        for (int k = 0; k < RP_PX; ++k) {
            const uint8_t *Sa = TWO && (P[k].a.flags & RP_MIP) ? M : S;
            a1[k] = rp_row(Sa, P[k].a.o1, P[k].a, (P[k].a.flags & RP_Y1) != 0);
            a2[k] = rp_row(Sa, P[k].a.o2, P[k].a, (P[k].a.flags & RP_Y2) != 0);
            if (TWO) {
                b1[k] = rp_row(M, P[k].b.o1, P[k].b, (P[k].b.flags & RP_Y1) != 0);
                b2[k] = rp_row(M, P[k].b.o2, P[k].b, (P[k].b.flags & RP_Y2) != 0);
            }
        }
        auto pixel = [&](int k, float (&o)[3]) {
            rp_blend(P[k].a, a1[k], a2[k], o);
            if (TWO) {
                float ob[3];
                rp_blend(P[k].b, b1[k], b2[k], ob);
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = P[k].t != 0.f ? __builtin_fmaf(P[k].t, ob[c] - o[c], o[c]) : o[c];
            }
        };
        if (FMT == MS_VIEW_BGR) {
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < RP_PX; ++k) {
                float o[3];
                pixel(k, o);
                rp_pack_bgr(o, k, w);
            }
            rp_store_bgr(A, f, dx, dy, n_px, w);
        } else {
            unsigned yq[2] = {0u, 0u}, uq = 0u, vq = 0u;
#pragma unroll
            for (int k = 0; k < RP_PX; ++k) {
                float o[3];
                pixel(k, o);
                rp_pack_i420(o, k, yq, uq, vq);
            }
            rp_store_i420(A, f, dx, dy, yq, uq, vq);
        }
    }
}

// k_reproject's grid and lane layout (reproject.hip)
template <int FMT>
__global__ void __launch_bounds__(256) k_reproject_aa(const ReprojAaArgs A)
{
    int ji = 0;
    while (ji + 1 < A.n_jobs && (int)blockIdx.x >= A.job[ji + 1].tile0) ++ji;
    const ReprojJob &J = A.job[ji];
    const int local = (int)blockIdx.x - J.tile0, ty = local / J.tiles_x, tx = local - ty * J.tiles_x;
    const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
    const int x0 = FMT == MS_VIEW_BGR ? tx * MS_VIEW_TILE_W + 4 * lx : tx * 32 + 2 * lx;
    const int y0 = FMT == MS_VIEW_BGR ? ty * MS_VIEW_TILE_H + ly : ty * 32 + 2 * ly;
    if (x0 >= J.cols || y0 >= J.rows) return;

    AaPx P[RP_PX];
    int n_px = 0;
    bool two = false;
#pragma unroll
    for (int k = 0; k < RP_PX; ++k) {
        const int x = FMT == MS_VIEW_BGR ? x0 + k : x0 + (k & 1), y = FMT == MS_VIEW_BGR ? y0 : y0 + (k >> 1);
        if (x < J.cols && y < J.rows) {
            P[k] = aa_make_px(A, row_ptr<float>(J.mx, J.mxstep, y)[x], row_ptr<float>(J.my, J.mystep, y)[x], row_ptr<float>(A.rho[ji], A.rstep[ji], y)[x], two);
            ++n_px;
        } else {
            P[k].a = RpTaps{0u, 0u, 0, 0, 0.f, 0.f, 0.f, 0.f, 0u}; P[k].b = P[k].a; P[k].t = 0.f;
        }
    }
    const int f0 = (int)blockIdx.y * RP_G, f1 = min(A.n_frames, f0 + RP_G);
    const int dx = J.dst_x + x0, dy = J.dst_y + y0;
    if (__any(two)) aa_frames<FMT, true>(A, P, n_px, dx, dy, f0, f1);
    else aa_frames<FMT, false>(A, P, n_px, dx, dy, f0, f1);
}

// ------------------------------------------------------------------------------------------------
// host side

static int check_levels(const char *fn, int levels)
{
    MS_CHECK(levels >= 1 && levels <= MS_VIEW_MAX_LEVELS, "%s: levels = %d outside [1, %d]", fn, levels, MS_VIEW_MAX_LEVELS);
    return MS_OK;
}
static int check_mips_ptr(const char *fn, void *const *mips, int f)
{
    MS_CHECK(mips[f], "%s: mips[%d] is null", fn, f);
    MS_CHECK(((uintptr_t)mips[f] & (MIP_BASE_ALIGN - 1)) == 0, "%s: mips[%d] must be %zu-byte aligned", fn, f, MIP_BASE_ALIGN);
    return MS_OK;
}
static bool ranges_overlap(uintptr_t a, size_t an, uintptr_t b, size_t bn) { return !(a + an <= b || b + bn <= a); }

}  // namespace ms

using namespace ms;

extern "C" {

int ms_pano_mips_layout(int cols, int rows, int levels, ms_mip_level *out, size_t *bytes)
{
    const char *fn = "ms_pano_mips_layout";
    MS_CHECK(out && bytes, "%s: null argument (out / bytes)", fn);
    if (int e = check_levels(fn, levels)) return e;
    if (int e = rp_check_side(fn, "cols x rows", cols, rows)) return e;
    mip_layout(cols, rows, levels, out, bytes);
    return MS_OK;
}

int ms_build_pano_mips(const ms_image *src, void *const *mips, int n_frames, int levels, ms_stream stream)
{
    const char *fn = "ms_build_pano_mips";
    MS_CHECK(src && mips, "%s: null argument (src / mips)", fn);
    MS_CHECK(n_frames >= 1 && n_frames <= MS_VIEW_MAX_FRAMES, "%s: n_frames = %d outside [1, %d]", fn, n_frames, MS_VIEW_MAX_FRAMES);
    if (int e = check_levels(fn, levels)) return e;
    const ms_image &s0 = src[0];
    for (int f = 0; f < n_frames; ++f) {
        const ms_image &s = src[f];
        MS_CHECK(s.data && s.type == MS_8UC3 && s.cols >= 1 && s.rows >= 1 && s.step >= (size_t)s.cols * 3, "%s: src frame %d must be a non-empty 8UC3 image", fn, f);
        MS_CHECK(s.cols == s0.cols && s.rows == s0.rows && s.step == s0.step, "%s: src frame %d differs in geometry from frame 0", fn, f);
    }
    MS_CHECK(s0.step < ((size_t)1 << 24) && (unsigned long long)s0.rows * s0.step < (1ull << 32), "%s: src step %zu must be below 2^24 and rows * step below 2^32", fn, s0.step);
    if (int e = rp_check_side(fn, "src cols x rows", s0.cols, s0.rows)) return e;
    ms_mip_level lv[MS_VIEW_MAX_LEVELS];
    size_t bytes = 0;
    mip_layout(s0.cols, s0.rows, levels, lv, &bytes);
    const size_t s_bytes = (size_t)(s0.rows - 1) * s0.step + (size_t)s0.cols * 3;
    for (int f = 0; f < n_frames; ++f) {
        if (int e = check_mips_ptr(fn, mips, f)) return e;
        for (int g = 0; g < n_frames; ++g)
            MS_CHECK(!ranges_overlap((uintptr_t)mips[f], bytes, (uintptr_t)src[g].data, s_bytes), "%s: mips[%d] overlaps src frame %d in memory", fn, f, g);
        for (int g = 0; g < f; ++g)
            MS_CHECK(!ranges_overlap((uintptr_t)mips[f], bytes, (uintptr_t)mips[g], bytes), "%s: mips[%d] overlaps mips[%d] in memory", fn, f, g);
    }
    if (int e = require_device()) return e;
    for (int first = 0; first < levels; first += MIP_PASS) {
        MipArgs A{};
        for (int f = 0; f < n_frames; ++f) {
            A.src[f] = first ? (const uint8_t *)mips[f] + lv[first - 1].offset : (const uint8_t *)src[f].data;
            A.dst[f] = (uint8_t *)mips[f];
        }
        A.sstep = first ? lv[first - 1].step : s0.step;
        A.scols = first ? lv[first - 1].cols : s0.cols;
        A.srows = first ? lv[first - 1].rows : s0.rows;
        A.nout = std::min(MIP_PASS, levels - first);
        for (int i = 0; i < A.nout; ++i) A.out[i] = MipOut{lv[first + i].offset, (unsigned)lv[first + i].step, lv[first + i].cols, lv[first + i].rows};
        k_pano_mips<<<dim3(div_up(A.scols, 256), div_up(A.srows, 64), n_frames), 256, 0, as_stream(stream)>>>(A);
        MS_LAUNCH_CHECK();
    }
    return MS_OK;
}

int ms_build_view_footprint(const ms_pano_frame *src, const ms_image *map_x, const ms_image *map_y, double footprint_scale, ms_image *rho, ms_stream stream)
{
    const char *fn = "ms_build_view_footprint";
    MS_CHECK(src && map_x && map_y && rho, "%s: null argument (src / map_x / map_y / rho)", fn);
    if (int e = rp_check_pano_frame(fn, src)) return e;
    if (int e = rp_check_view_map(fn, "map_x", *map_x)) return e;
    if (int e = rp_check_view_map(fn, "map_y", *map_y)) return e;
    if (int e = rp_check_view_map(fn, "rho", *rho)) return e;
    MS_CHECK(map_x->cols == map_y->cols && map_x->rows == map_y->rows && map_x->cols == rho->cols && map_x->rows == rho->rows,
             "%s: map_x %d x %d, map_y %d x %d and rho %d x %d are not of one size", fn, map_x->cols, map_x->rows, map_y->cols, map_y->rows, rho->cols, rho->rows);
    if (int e = rp_check_side(fn, "the maps", map_x->cols, map_x->rows)) return e;
    MS_CHECK(std::isfinite(footprint_scale) && footprint_scale > 0.0 && footprint_scale <= 16.0, "%s: footprint_scale %g outside (0, 16]", fn, footprint_scale);
    if (int e = require_device()) return e;
    FootArgs A{};
    A.mx = (const float *)map_x->data; A.my = (const float *)map_y->data; A.rho = (float *)rho->data;
    A.mxstep = map_x->step; A.mystep = map_y->step; A.rstep = rho->step;
    A.cols = map_x->cols; A.rows = map_x->rows;
    A.S = (double)src->scale; A.v0 = (double)src->v0; A.W = (double)src->wrap_cols; A.fscale = footprint_scale;
    A.sph = src->projection == MS_PROJ_SPHERICAL;
    k_view_footprint<<<dim3(div_up(A.cols, 64), div_up(A.rows, 4)), dim3(64, 4), 0, as_stream(stream)>>>(A);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

int ms_reproject_aa(const ms_image *src, void *const *mips, int levels, ms_image *dst, int n_frames, const ms_view_job_aa *jobs, int n_jobs, int wrap_cols, int clamp_rows,
                    int format, ms_stream stream)
{
    const char *fn = "ms_reproject_aa";
    MS_CHECK(mips, "%s: null argument (mips)", fn);
    if (int e = check_levels(fn, levels)) return e;
    RpPlan P;
    if (int e = rp_plan(fn, src, dst, n_frames, jobs, sizeof(ms_view_job_aa), n_jobs, wrap_cols, clamp_rows, format, P)) return e;
    const bool i420 = format == MS_VIEW_I420;
    const ms_image &s0 = src[0], &d0 = dst[0];
    if (int e = rp_check_side(fn, "src cols x rows", s0.cols, s0.rows)) return e;
    MS_CHECK(wrap_cols == 0 || s0.cols % (1 << levels) == 0, "%s: a wrapping source of %d columns is no multiple of 2^levels = %d: the coarse levels would not close the turn", fn,
             s0.cols, 1 << levels);
    for (int j = 0; j < n_jobs; ++j) {
        char name[48];
        snprintf(name, sizeof(name), "jobs[%d].rho", j);
        if (int e = rp_check_view_map(fn, name, jobs[j].rho)) return e;
        MS_CHECK(jobs[j].rho.cols == P.job[j].cols && jobs[j].rho.rows == P.job[j].rows, "%s: jobs[%d]: rho is %d x %d, the maps %d x %d", fn, j, jobs[j].rho.cols, jobs[j].rho.rows,
                 P.job[j].cols, P.job[j].rows);
    }
    ms_mip_level lv[MS_VIEW_MAX_LEVELS];
    size_t bytes = 0;
    mip_layout(s0.cols, s0.rows, levels, lv, &bytes);
    MS_CHECK(bytes < ((size_t)1 << 32), "%s: the mip chain of a %d x %d source takes %zu bytes, 2^32 or more", fn, s0.cols, s0.rows, bytes);
    const size_t d_bytes = (size_t)(d0.rows - 1) * d0.step + (size_t)d0.cols * (i420 ? 1 : 3);
    for (int f = 0; f < n_frames; ++f) {
        if (int e = check_mips_ptr(fn, mips, f)) return e;
        for (int g = 0; g < n_frames; ++g)
            MS_CHECK(!ranges_overlap((uintptr_t)dst[g].data, d_bytes, (uintptr_t)mips[f], bytes), "%s: dst frame %d overlaps mips[%d] in memory", fn, g, f);
    }
    if (int e = require_device()) return e;
    ReprojAaArgs A{};
    for (int j = 0; j < n_jobs; ++j) { A.job[j] = P.job[j]; A.rho[j] = (const float *)jobs[j].rho.data; A.rstep[j] = jobs[j].rho.step; }
    for (int f = 0; f < n_frames; ++f) { A.src[f] = (const uint8_t *)src[f].data; A.mips[f] = (const uint8_t *)mips[f]; A.dst[f] = (uint8_t *)dst[f].data; }
    A.lev[0] = AaLevel{0u, (unsigned)s0.step, s0.cols, s0.rows};
    for (int l = 1; l <= MS_VIEW_MAX_LEVELS; ++l) {
        const ms_mip_level &m = lv[std::min(l, levels) - 1];      // (entries past `levels` are never selected)
        A.lev[l] = AaLevel{(unsigned)m.offset, (unsigned)m.step, m.cols, m.rows};
    }
    A.dstep = d0.step;
    A.n_jobs = n_jobs; A.n_frames = n_frames; A.levels = levels;
    A.dcols = P.fw; A.drows = P.fh;
    A.wrap = wrap_cols != 0; A.clamp = clamp_rows;
    const dim3 grid(P.tiles, div_up(n_frames, RP_G));
    if (i420) k_reproject_aa<MS_VIEW_I420><<<grid, 256, 0, as_stream(stream)>>>(A);
    else k_reproject_aa<MS_VIEW_BGR><<<grid, 256, 0, as_stream(stream)>>>(A);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

}  // extern "C"
