// mesh_maps.hip -- the CPW mesh maps of a context: MeshWarper::convertMeshesToMap (APP/meshwarper.cpp:823-886) on the device.  A vertex mesh becomes a
// view's dense backward maps in two launches: ms_set_meshes runs every view of the rig in one pair (a list of jobs, one per view), ms_set_mesh one
// view's job through the single-view form of the same device functions.  Both build their jobs on one scratch block.  The maps are double buffered: an
// update only enqueues work into the buffer ms_stitch does not read and publishes it under mesh_mu; the per-frame path (compositor.hip) picks the
// active buffers up through the members of ms_ctx it shares with this unit (ctx.hpp).
#include <algorithm>
#include <mutex>
#include <vector>
#include "common.hpp"
#include "launchers.hpp"
#include "descs.hpp"
#include "ctx.hpp"

namespace ms {

// custom_resize (APP/resize.cu:9-27) of one output element, the taps fetched through `at(row, col)`: the same expression tree as
// k_custom_resize (prims.hip), so a fused consumer sees the bits the materialised map would hold
// one axis of custom_resize: cell index i = x * (n - 1) / t (integer division) and fraction ((float)x * (float)(n - 1) / (float)t) - (float)i.
// While t * (n - 1) < 2^23 the float quotient q is the correctly rounded value of an exact ratio whose distance to the next integer is at
// least 1/t > ulp(q)/2, so (int)q IS the integer quotient and the ~40-instruction integer division disappears (`exact` says which case).
__device__ __forceinline__ void resize_axis(int x, int n, int t, bool exact, int &i, float &frac)
{
    const float q = ((float)x) * (float)(n - 1) / (float)t;
    i = exact ? (int)q : x * (n - 1) / t;
    frac = q - (float)i;
}
__device__ __forceinline__ bool resize_axis_exact(int n, int t) { return (long long)t * (n - 1) < (1ll << 23); }
template <class At>
__device__ __forceinline__ float custom_resize_at(int tx, int ty, int cols, int rows, int x, int y, At at)
{
    int left, top;
    float uu, vv;
    resize_axis(x, cols, tx, resize_axis_exact(cols, tx), left, uu);
    resize_axis(y, rows, ty, resize_axis_exact(rows, ty), top, vv);
    float r = ((1.f - uu) * (1.f - vv)) * at(top, left);
    r = __builtin_fmaf(uu * (1.f - vv), at(top, left + 1), r);
    r = __builtin_fmaf((1.f - uu) * vv, at(top + 1, left), r);
    r = __builtin_fmaf(uu * vv, at(top + 1, left + 1), r);
    return r;
}
// convertMeshesToMap, first half in one launch (meshwarper.cpp:838-869): vertex mesh -> per-pixel forward position (custom_resize, not
// materialised) -> scatter into the half-resolution sums.  Also clears what the previous update dirtied in the other accumulator
// (ping-pong: no memset call between updates) and the displacement word of this update.
constexpr int MESH_SR = 4;                         // rows per lane: a workgroup scatters a 64 x 16 pixel block
constexpr int MESH_WW = 48, MESH_WH = 20, MESH_WMX = 6, MESH_WMY = 4;   // LDS window (half-resolution cells) around where the block's first pixel lands
// one view's update: what both launches of convertMeshesToMap need (ms_set_meshes runs all views of a context in ONE pair of launches, blockIdx.z = view)
struct MeshJob {
    const float *smx, *smy;                    // N x M vertex mesh (device)
    unsigned long long *ax, *ay;               // half-resolution accumulators of this update
    unsigned long long *clear; size_t n_clear; // what the previous update dirtied in the other accumulator
    unsigned *disp_word;
    float *dx, *dy;                            // dense maps being written (the view's inactive buffer)
    int aw, ah, hw, hh, pitch, tiles_x, n_tiles;
};
struct MeshJobs { MeshJob j[MAX_VIEWS]; };
__device__ __forceinline__ void mesh_expand_scatter_block(const MeshJob &J, int N, int M, int bx, int by, int gx, int gy)
{
    const float *__restrict__ smx = J.smx, *__restrict__ smy = J.smy;
    const int aw = J.aw, ah = J.ah, hw = J.hw, hh = J.hh;
    unsigned long long *ax = J.ax, *ay = J.ay, *__restrict__ clear = J.clear;
    const size_t n_clear = J.n_clear;
    unsigned *disp_word = J.disp_word;
    // The pixels of a block land in a compact patch of the half-resolution grid (the mesh is a smooth deformation), and four of them share a
    // cell: accumulate the patch in LDS and send one pair of global atomics per touched cell instead of one per pixel (device-scope atomics
    // were 60 % of the update's GPU time); pixels landing outside the window go to memory directly.
    __shared__ unsigned long long wx[MESH_WH * MESH_WW], wy[MESH_WH * MESH_WW];
    const int lt = threadIdx.y * 64 + threadIdx.x;
    const size_t tid = ((size_t)by * gx + bx) * 256 + lt, nthreads = (size_t)gx * gy * 256;
    for (size_t k = tid; k < n_clear; k += nthreads) clear[k] = 0ull;
    if (tid == 0) *disp_word = 0u;
    for (int k = lt; k < MESH_WH * MESH_WW; k += 256) { wx[k] = 0ull; wy[k] = 0ull; }
    const bool ex = resize_axis_exact(M, aw), ey = resize_axis_exact(N, ah);
    auto forward = [&](int x, int y, float &fx, float &fy) {          // custom_resize of both vertex maps at (x, y): the expression tree of custom_resize_at
        int left, top;
        float uu, vv;
        resize_axis(x, M, aw, ex, left, uu);
        resize_axis(y, N, ah, ey, top, vv);
        const float w00 = (1.f - uu) * (1.f - vv), w01 = uu * (1.f - vv), w10 = (1.f - uu) * vv, w11 = uu * vv;
        const int i0 = top * M + left, i1 = i0 + M;
        fx = w00 * smx[i0]; fy = w00 * smy[i0];
        fx = __builtin_fmaf(w01, smx[i0 + 1], fx); fy = __builtin_fmaf(w01, smy[i0 + 1], fy);
        fx = __builtin_fmaf(w10, smx[i1], fx);     fy = __builtin_fmaf(w10, smy[i1], fy);
        fx = __builtin_fmaf(w11, smx[i1 + 1], fx); fy = __builtin_fmaf(w11, smy[i1 + 1], fy);
    };
    auto finite_i32 = [](float v) { return v > -2147483648.f && v < 2147483648.f; };
    float ox, oy;
    forward(bx * 64, by * (4 * MESH_SR), ox, oy);          // the same for every lane: the window's anchor
    const int wx0 = (finite_i32(ox) ? (int)ox / 2 : 0) - MESH_WMX, wy0 = (finite_i32(oy) ? (int)oy / 2 : 0) - MESH_WMY;
    __syncthreads();
    const int x = bx * 64 + threadIdx.x;
#pragma unroll
    for (int r = 0; r < MESH_SR; ++r) {
        const int y = by * (4 * MESH_SR) + r * 4 + threadIdx.y;
        if (x >= aw || y >= ah) continue;
        float fx, fy;
        forward(x, y, fx, fy);
        if (!(finite_i32(fx) && finite_i32(fy))) continue;
        const int x_ = (int)fx / 2, y_ = (int)fy / 2;
        if (x_ >= 0 && y_ >= 0 && x_ < hw && y_ < hh) {
            // sum_x += x, sum_y += y, set_values++ as two 64-bit integer adds: [count : 24 | sum : 40].  The reference's float sums are integers,
            // exact (and therefore order-independent) below 2^24, where (float)sum is the very same value
            const unsigned long long vx = (1ull << 40) | (unsigned long long)x, vy = (unsigned long long)y;
            const int cx = x_ - wx0, cy = y_ - wy0;
            if ((unsigned)cx < (unsigned)MESH_WW && (unsigned)cy < (unsigned)MESH_WH) {
                atomicAdd(&wx[cy * MESH_WW + cx], vx);
                atomicAdd(&wy[cy * MESH_WW + cx], vy);
            } else {
                atomicAdd(&ax[(size_t)y_ * hw + x_], vx);
                atomicAdd(&ay[(size_t)y_ * hw + x_], vy);
            }
        }
    }
    __syncthreads();
    for (int k = lt; k < MESH_WH * MESH_WW; k += 256) {
        const unsigned long long vx = wx[k];
        if (vx == 0ull) continue;
        const int cy = k / MESH_WW, cx = k - cy * MESH_WW;
        const size_t g = (size_t)(wy0 + cy) * hw + (wx0 + cx);
        atomicAdd(&ax[g], vx);
        atomicAdd(&ay[g], wy[k]);
    }
}
__global__ void __launch_bounds__(256) k_mesh_expand_scatter(const float *__restrict__ smx, const float *__restrict__ smy, int N, int M, int aw, int ah,
                                                             unsigned long long *ax, unsigned long long *ay, int hw, int hh,
                                                             unsigned long long *__restrict__ clear, size_t n_clear, unsigned *disp_word)
{
    MeshJob J{smx, smy, ax, ay, clear, n_clear, disp_word, nullptr, nullptr, aw, ah, hw, hh, 0, 0, 0};
    mesh_expand_scatter_block(J, N, M, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, (int)gridDim.y);
}
__global__ void __launch_bounds__(256) k_mesh_expand_scatter_all(MeshJobs T, int N, int M)
{
    const MeshJob &J = T.j[blockIdx.z];
    const int gx = (J.aw + 63) / 64, gy = (J.ah + 4 * MESH_SR - 1) / (4 * MESH_SR);
    if ((int)blockIdx.x >= gx || (int)blockIdx.y >= gy) return;          // (the grid is sized for the largest view)
    mesh_expand_scatter_block(J, N, M, (int)blockIdx.x, (int)blockIdx.y, gx, gy);
}
// second half (meshwarper.cpp:870-883): mean (0/0 -> NaN hole) + custom_resize back to the view size for both maps, and the largest
// displacement of the new maps (see k_mesh_disp)
constexpr int MESH_TR = 4;                      // output rows per lane: a workgroup step is a 64 x 16 pixel tile (64 x 4 until round 5: the straddling view's 9 420 tiles were 18 serial
                                                // steps -- each a chain of cell loads, two barriers, stores -- for each of its 512 workgroups: 54 us; four times fewer, fatter steps)
constexpr int MESH_FW = 72, MESH_FH = 4 * MESH_TR / 2 + 4;       // LDS footprint (cells) of a 64 x 16 output block: <= 64 * (hw - 1) / aw + 2 columns, likewise rows
__device__ __forceinline__ void mesh_mean_resize_blocks(const MeshJob &J, int first_tile, int tile_stride)
{
    const unsigned long long *__restrict__ ax = J.ax, *__restrict__ ay = J.ay;
    const int hw = J.hw, hh = J.hh, pitch = J.pitch, aw = J.aw, ah = J.ah, tiles_x = J.tiles_x, n_tiles = J.n_tiles;
    float *__restrict__ dx = J.dx, *__restrict__ dy = J.dy;
    unsigned *disp_word = J.disp_word;
    __shared__ float mxs[MESH_FH][MESH_FW], mys[MESH_FH][MESH_FW];
    __shared__ float wmax[4];
    const bool ex = resize_axis_exact(hw, aw), ey = resize_axis_exact(hh, ah);
    constexpr unsigned long long SUM = (1ull << 40) - 1;
    float d = 0.f;
    // a workgroup walks 64 x 16 output tiles grid-stride: one atomic on the displacement word per workgroup, not per tile (thousands of
    // same-address atomics serialise: they were most of this kernel's time)
    for (int tile = first_tile; tile < n_tiles; tile += tile_stride) {
        const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
        const int x = txi * 64 + threadIdx.x;
        // footprint of the tile in the half-resolution maps
        const int bx0 = txi * 64, by0 = tyi * (4 * MESH_TR), bx1 = min(bx0 + 63, aw - 1), by1 = min(by0 + 4 * MESH_TR - 1, ah - 1);
        int c0, c1, r0, r1;
        float t;
        resize_axis(bx0, hw, aw, ex, c0, t); resize_axis(bx1, hw, aw, ex, c1, t);
        resize_axis(by0, hh, ah, ey, r0, t); resize_axis(by1, hh, ah, ey, r1, t);
        const int fw = c1 - c0 + 2, fh = r1 - r0 + 2;
        const bool staged = fw <= MESH_FW && fh <= MESH_FH;             // (always for hw = aw / 2; the direct path keeps odd geometries correct)
        if (staged) {
            for (int k = threadIdx.y * 64 + threadIdx.x; k < fw * fh; k += 256) {
                const int rr = k / fw, cc = k - rr * fw, r = r0 + rr, c = c0 + cc;
                float vx = 0.f, vy = 0.f;
                if (r < hh && c < hw) {            // mean = sum / count; 0 / 0 -> NaN hole, as the reference (remap then yields 0)
                    const unsigned long long a = ax[(size_t)r * hw + c];
                    const float n = (float)(a >> 40);
                    vx = (float)(a & SUM) / n;
                    vy = (float)(ay[(size_t)r * hw + c] & SUM) / n;
                }
                mxs[rr][cc] = vx; mys[rr][cc] = vy;
            }
            __syncthreads();
        }
#pragma unroll
        for (int tr = 0; tr < MESH_TR; ++tr) {
        const int y = by0 + 4 * tr + (int)threadIdx.y;
        if (x < aw && y < ah) {
            int left, top;
            float uu, vv;
            resize_axis(x, hw, aw, ex, left, uu);
            resize_axis(y, hh, ah, ey, top, vv);
            const float w00 = (1.f - uu) * (1.f - vv), w01 = uu * (1.f - vv), w10 = (1.f - uu) * vv, w11 = uu * vv;
            float mx, my;
            if (staged) {
                const int cc = left - c0, rr = top - r0;
                mx = w00 * mxs[rr][cc];                            my = w00 * mys[rr][cc];
                mx = __builtin_fmaf(w01, mxs[rr][cc + 1], mx);     my = __builtin_fmaf(w01, mys[rr][cc + 1], my);
                mx = __builtin_fmaf(w10, mxs[rr + 1][cc], mx);     my = __builtin_fmaf(w10, mys[rr + 1][cc], my);
                mx = __builtin_fmaf(w11, mxs[rr + 1][cc + 1], mx); my = __builtin_fmaf(w11, mys[rr + 1][cc + 1], my);
            } else {
                mx = custom_resize_at(aw, ah, hw, hh, x, y, [&](int r, int c) { const unsigned long long v = ax[(size_t)r * hw + c]; return (float)(v & SUM) / (float)(v >> 40); });
                my = custom_resize_at(aw, ah, hw, hh, x, y, [&](int r, int c) { return (float)(ay[(size_t)r * hw + c] & SUM) / (float)(ax[(size_t)r * hw + c] >> 40); });
            }
            dx[(size_t)y * pitch + x] = mx;
            dy[(size_t)y * pitch + x] = my;
            const float a = fabsf(mx - (float)x), b = fabsf(my - (float)y);
            d = fmaxf(d, fmaxf(a == a ? a : 0.f, b == b ? b : 0.f));
        }
        }
        __syncthreads();                                                 // the staging arrays are rewritten by the next tile
    }
    for (int o = 32; o > 0; o >>= 1) d = fmaxf(d, __shfl_xor(d, o));
    if (threadIdx.x == 0) wmax[threadIdx.y] = d;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        d = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        if (d > 0.f) atomicMax(disp_word, __float_as_uint(d));
    }
}
__global__ void __launch_bounds__(256) k_mesh_mean_resize(const unsigned long long *__restrict__ ax, const unsigned long long *__restrict__ ay, int hw, int hh,
                                                          float *__restrict__ dx, float *__restrict__ dy, int pitch, int aw, int ah, int tiles_x, int n_tiles, unsigned *disp_word)
{
    MeshJob J{nullptr, nullptr, const_cast<unsigned long long *>(ax), const_cast<unsigned long long *>(ay), nullptr, 0, disp_word, dx, dy, aw, ah, hw, hh, pitch, tiles_x, n_tiles};
    mesh_mean_resize_blocks(J, (int)blockIdx.x, (int)gridDim.x);
}
__global__ void __launch_bounds__(256) k_mesh_mean_resize_all(MeshJobs T)
{
    mesh_mean_resize_blocks(T.j[blockIdx.y], (int)blockIdx.x, (int)gridDim.x);
}

}  // namespace ms

using namespace ms;

extern "C" {

// max over the view of |x_mesh - x|, |y_mesh - y| (NaN = hole of convertMeshesToMap: samples nothing, ignored); non-negative floats
// order like their bit patterns, so one atomicMax on the bits reduces the launch
__global__ void __launch_bounds__(256) k_mesh_disp(const float *__restrict__ mx, const float *__restrict__ my, int pitch, int ah, int aw, unsigned *out)
{
    float d = 0.f;
    for (int y = blockIdx.x; y < ah; y += gridDim.x)            // a block walks rows, grid-stride: few atomics on the one result word
        for (int x = threadIdx.x; x < aw; x += 256) {
            const float a = fabsf(mx[(size_t)y * pitch + x] - (float)x), b = fabsf(my[(size_t)y * pitch + x] - (float)y);
            d = fmaxf(d, fmaxf(a == a ? a : 0.f, b == b ? b : 0.f));
        }
    for (int o = 32; o > 0; o >>= 1) d = fmaxf(d, __shfl_xor(d, o));
    if ((threadIdx.x & 63) == 0 && d > 0.f) atomicMax(out, __float_as_uint(d));
}
static int measure_mesh_disp(ms_ctx *c, int view, int tgt, hipStream_t st)
{
    const int aw = c->roi[view].width, ah = c->roi[view].height;
    const float *base = (const float *)c->mesh[tgt].p + c->mesh_off[view];
    unsigned *word = (unsigned *)c->disp_dev.p + 2 * view + tgt;
    MS_HIP(hipMemsetAsync(word, 0, sizeof(unsigned), st));
    k_mesh_disp<<<std::min(ah, 128), 256, 0, st>>>(base, base + (size_t)ah * c->map_pitch[view], c->map_pitch[view], ah, aw, word);
    MS_LAUNCH_CHECK();
    return MS_OK;          // (no host synchronisation: the stage-1 kernel reads the word on the device, ms_get_mesh_displacement waits on mesh_ready)
}

// ---- CPW mesh maps ------------------------------------------------------------------------------
// What an update needs beside the map buffers, made or grown on demand; every setter calls it first.  The displacement words; and for a vertex mesh
// of n_small floats per map (0: dense maps, nothing to expand) the device scratch and the pinned staging ring.  The scratch is reallocated when the
// vertex count exceeds its capacity (first call or a larger mesh; a smaller mesh reuses it) or the views' accumulators changed size (a rebuilt rig):
// earlier updates are drained first, the new block is cleared on the update's own stream and every view starts over with clean accumulators.
static size_t mesh_vertex_bytes(int n_views, size_t cap) { return (2 * cap * n_views * sizeof(float) + 15) & ~(size_t)15; }      // the vertex slots in front of the accumulators
static int mesh_reserve(ms_ctx *c, size_t n_small, hipStream_t st)
{
    ms_ctx::MeshUpdater &U = c->mesh_upd;
    if (!c->disp_dev.p) {
        if (int e = c->disp_dev.alloc(2 * MAX_VIEWS * sizeof(unsigned))) return e;
        MS_HIP(hipMemsetAsync(c->disp_dev.p, 0xff, 2 * MAX_VIEWS * sizeof(unsigned), st));      // "unbounded" until measured
    }
    if (n_small == 0) return MS_OK;
    size_t acc_words = 0;                                    // per view [ax | ay] x two parities
    for (int v = 0; v < c->N; ++v) acc_words += 4 * (size_t)(c->roi[v].width / 2) * (c->roi[v].height / 2);
    if (U.scratch.p && n_small <= U.cap && acc_words == U.acc_off[c->N]) return MS_OK;
    if (c->mesh_chain_set) MS_HIP(hipEventSynchronize(c->mesh_chain));
    const size_t cap = std::max(U.cap, n_small);
    U.cap = 0;
    const size_t bytes = mesh_vertex_bytes(c->N, cap) + acc_words * sizeof(unsigned long long);
    if (int e = U.scratch.alloc(bytes)) return e;
    MS_HIP(hipMemsetAsync(U.scratch.p, 0, bytes, st));      // on the update's own stream: a plain hipMemset runs on the NULL stream, asynchronously to the host, and non-blocking streams do not wait for it
    U.cap = cap;
    for (int v = 0; v < c->N; ++v) {
        U.acc_off[v + 1] = U.acc_off[v] + 4 * (size_t)(c->roi[v].width / 2) * (c->roi[v].height / 2);
        U.parity[v] = 0; U.dirty[v] = false;
    }
    if (U.stage_floats < 2 * cap) {
        if (U.stage) (void)hipHostFree(U.stage);
        U.stage = nullptr; U.stage_floats = 0;
        MS_HIP(hipHostMalloc((void **)&U.stage, (ms_ctx::MESH_STAGE_GENS + 1) * (2 * cap * sizeof(float) * MAX_VIEWS), hipHostMallocDefault));      // (the ring + ms_set_mesh's own generation behind it)
        for (bool &b_ : U.stage_ev_set) b_ = false;
        U.stage_gen = 0;
        U.stage_floats = 2 * cap;
    }
    return MS_OK;
}
// One view's job.  Its vertex mesh (n_small floats per map) goes to the view's place among the vertex slots; it adds into the accumulator pair of
// the view's parity and clears the other pair if the view's previous update left its sums there.  INVARIANT: the accumulators a launch adds into are
// zero on entry -- cleared by the allocation's stream-ordered memset, or by this view's previous launch (updates run one behind the other on the
// device: mesh_chain).  The caller flips the parity once the launches are out (mesh_job_enqueued).
static MeshJob mesh_job(const ms_ctx *c, int v, int tgt, size_t n_small)
{
    const ms_ctx::MeshUpdater &U = c->mesh_upd;
    const int aw = c->roi[v].width, ah = c->roi[v].height, hw = aw / 2, hh = ah / 2, p = U.parity[v];
    const size_t n_half = (size_t)hw * hh;
    unsigned long long *acc = (unsigned long long *)((char *)U.scratch.p + mesh_vertex_bytes(c->N, U.cap)) + U.acc_off[v];
    unsigned long long *mine = acc + (size_t)p * 2 * n_half, *other = acc + (size_t)(1 - p) * 2 * n_half;
    ms_image dx = mesh_image(c, tgt, v, 0), dy = mesh_image(c, tgt, v, 1);
    MeshJob J;
    J.smx = (float *)U.scratch.p + (size_t)v * 2 * n_small; J.smy = J.smx + n_small;
    J.ax = mine; J.ay = mine + n_half;
    J.clear = other; J.n_clear = U.dirty[v] ? 2 * n_half : 0;
    J.disp_word = (unsigned *)c->disp_dev.p + 2 * v + tgt;
    J.dx = (float *)dx.data; J.dy = (float *)dy.data;
    J.aw = aw; J.ah = ah; J.hw = hw; J.hh = hh; J.pitch = c->map_pitch[v];
    J.tiles_x = div_up(aw, 64); J.n_tiles = J.tiles_x * div_up(ah, 4 * MESH_TR);
    return J;
}
static void mesh_job_enqueued(ms_ctx *c, int v) { c->mesh_upd.dirty[v] = true; c->mesh_upd.parity[v] ^= 1; }
// Callers hold mesh_update_mu (one update at a time).  mesh_mu is taken here only around the bookkeeping ms_stitch shares: ms_stitch holds it from
// picking the active buffers up to recording last_stitch, so `last_stitch` seen here covers every stitch that may still read the inactive buffer.
static int mesh_begin_update(ms_ctx *c, int view, int *target, hipStream_t st, bool enqueue_waits = true)
{
    if (!c->blender_ready || !c->cfg.enable_cpw) return fail(MS_ERR_STATE, "mesh update needs enable_cpw and ms_init_blender");
    std::lock_guard<std::mutex> lk(c->mesh_mu);
    *target = c->mesh_set[view] ? 1 - c->mesh_active[view] : c->mesh_active[view];
    if (!c->mesh_ready[view]) MS_HIP(hipEventCreateWithFlags(&c->mesh_ready[view], hipEventDisableTiming));
    if (!c->mesh_chain) MS_HIP(hipEventCreateWithFlags(&c->mesh_chain, hipEventDisableTiming));
    // the inactive buffer may still be read by a stitch enqueued before the previous swap: the update waits for it ON THE GPU
    // (the reference releases its mutex before the async remap finishes, timed.cpp:98-103); no host synchronisation anywhere
    if (enqueue_waits) {      // (ms_set_meshes: once for all views of the call)
        if (c->stitch_pending) MS_HIP(hipStreamWaitEvent(st, c->last_stitch, 0));
        if (c->mesh_chain_set) MS_HIP(hipStreamWaitEvent(st, c->mesh_chain, 0));
    }
    return MS_OK;
}
// one view's update: its own event + the chain, both recorded BEFORE the view is published (ms_set_meshes publishes all its views itself, behind one record of the chain)
static int mesh_end_update(ms_ctx *c, int view, int tgt, hipStream_t st, bool measure = true)
{
    if (measure) if (int e = measure_mesh_disp(c, view, tgt, st)) return e;
    std::lock_guard<std::mutex> lk(c->mesh_mu);
    MS_HIP(hipEventRecord(c->mesh_ready[view], st));
    MS_HIP(hipEventRecord(c->mesh_chain, st));
    c->mesh_ready_via_chain[view] = false;
    c->mesh_chain_set = true;
    c->mesh_wait[view] = true;
    c->mesh_active[view] = tgt;
    c->mesh_set[view] = true;
    return MS_OK;
}

int ms_set_mesh_maps(ms_ctx *c, int view, const ms_image *xm, const ms_image *ym, ms_stream stream)
{
    if (int e = ctx_check_view(c, view)) return e;
    MS_CHECK(xm && ym && xm->data && ym->data, "ms_set_mesh_maps: null image");
    std::lock_guard<std::mutex> lk(c->mesh_update_mu);
    int tgt;
    hipStream_t st = as_stream(stream);
    const int aw = c->roi[view].width, ah = c->roi[view].height;
    MS_CHECK(xm->rows == ah && xm->cols == aw && ym->rows == ah && ym->cols == aw && xm->type == MS_32FC1 && ym->type == MS_32FC1,
             "ms_set_mesh_maps: maps must be 32FC1 %dx%d", aw, ah);
    if (int e = mesh_begin_update(c, view, &tgt, st)) return e;
    if (int e = mesh_reserve(c, 0, st)) return e;
    ms_image dx = mesh_image(c, tgt, view, 0), dy = mesh_image(c, tgt, view, 1);
    MS_HIP(hipMemcpy2DAsync(dx.data, dx.step, xm->data, xm->step, (size_t)aw * 4, ah, hipMemcpyDeviceToDevice, st));
    MS_HIP(hipMemcpy2DAsync(dy.data, dy.step, ym->data, ym->step, (size_t)aw * 4, ah, hipMemcpyDeviceToDevice, st));
    return mesh_end_update(c, view, tgt, st);
}

int ms_set_mesh(ms_ctx *c, int view, const float *mesh_x, const float *mesh_y, int N, int M, ms_stream stream)
{
    if (int e = ctx_check_view(c, view)) return e;
    MS_CHECK(mesh_x && mesh_y && N >= 2 && M >= 2, "ms_set_mesh: need an N x M (>= 2x2) vertex mesh");
    std::lock_guard<std::mutex> lk(c->mesh_update_mu);       // (ms_stitch never takes this one: the waits and allocations below cannot stall it)
    int tgt;
    hipStream_t st = as_stream(stream);
    const int aw = c->roi[view].width, ah = c->roi[view].height, hw = aw / 2, hh = ah / 2;
    MS_CHECK(hw >= 2 && hh >= 2, "ms_set_mesh: view too small");
    MS_CHECK((long long)aw * ah < (1ll << 24) && aw < 65536 && ah < 65536, "ms_set_mesh: view %dx%d exceeds the scatter accumulators ([count:24 | sum:40])", aw, ah);
    const size_t n_small = (size_t)N * M;
    if (int e = mesh_reserve(c, n_small, st)) return e;
    if (int e = mesh_begin_update(c, view, &tgt, st)) return e;
    // the caller's arrays may be freed right after return: stage them in pinned memory (one slot per view; a slot is reused only by
    // the next update of the same view, whose copy of the previous one finished long before -- checked on its event)
    bool slot_busy;
    hipEvent_t busy_ev = nullptr;
    { std::lock_guard<std::mutex> mk(c->mesh_mu); slot_busy = c->mesh_ready[view] && (c->mesh_wait[view] || c->mesh_set[view]); if (slot_busy) busy_ev = mesh_ready_event(c, view); }
    if (slot_busy && busy_ev) MS_HIP(hipEventSynchronize(busy_ev));
    // (generation MESH_STAGE_GENS, outside the ring ms_set_meshes walks: a batched call can never overwrite a slot whose single-view copy has not run yet -- ADVICE r05)
    float *stg = c->mesh_upd.stage + ((size_t)ms_ctx::MESH_STAGE_GENS * MAX_VIEWS + view) * c->mesh_upd.stage_floats;
    memcpy(stg, mesh_x, n_small * 4);
    memcpy(stg + n_small, mesh_y, n_small * 4);
    // The view's job through the single-view kernels: the same device functions as the batched pair, the job's fields as plain arguments.  (As a job list of one through
    // the batched kernels six views back to back took 3.8 % more GPU time and 16 % more host time, the kernels themselves none: what grows is the launch, whose 1.4 KB
    // by-value list goes into the kernel-argument buffer twice per call -- profiles/set_mesh.jsonl.)
    const MeshJob J = mesh_job(c, view, tgt, n_small);
    MS_HIP(hipMemcpyAsync(const_cast<float *>(J.smx), stg, 2 * n_small * 4, hipMemcpyHostToDevice, st));
    const dim3 blk(64, 4);
    k_mesh_expand_scatter<<<dim3(div_up(aw, 64), div_up(ah, 4 * MESH_SR)), blk, 0, st>>>(J.smx, J.smy, N, M, aw, ah, J.ax, J.ay, hw, hh, J.clear, J.n_clear, J.disp_word);        // meshwarper.cpp:838-869
    MS_LAUNCH_CHECK();
    k_mesh_mean_resize<<<std::min(J.n_tiles, 1024), blk, 0, st>>>(J.ax, J.ay, hw, hh, J.dx, J.dy, J.pitch, aw, ah, J.tiles_x, J.n_tiles, J.disp_word);   // :870-883
    MS_LAUNCH_CHECK();
    mesh_job_enqueued(c, view);
    return mesh_end_update(c, view, tgt, st, false);
}

// MeshWarper::convertMeshesToMap as the reference calls it -- for ALL views at once (meshwarper.cpp:823-886 loops over the images): the same two kernels
// with blockIdx.z / .y = view, i.e. two launches per recalibration instead of two per view.  The per-view launches are latency-bound (47 us each for a
// 960 x 627 view): six views cost 0.3 ms of GPU time one after the other, about a third of that together.  Same arithmetic, bit-identical maps.
// mesh_x / mesh_y: HOST, num_views meshes of N x M back to back.
int ms_set_meshes(ms_ctx *c, const float *mesh_x, const float *mesh_y, int N, int M, ms_stream stream)
{
    if (!c) return fail(MS_ERR_INVALID, "null context");
    MS_CHECK(mesh_x && mesh_y && N >= 2 && M >= 2, "ms_set_meshes: need N x M (>= 2x2) vertex meshes");
    if (!c->blender_ready || !c->cfg.enable_cpw) return fail(MS_ERR_STATE, "ms_set_meshes needs enable_cpw and ms_init_blender");
    std::lock_guard<std::mutex> lk(c->mesh_update_mu);
    hipStream_t st = as_stream(stream);
    const int NV = c->N;
    const size_t n_small = (size_t)N * M;
    int max_aw = 0, max_ah = 0, max_tiles = 0;
    for (int v = 0; v < NV; ++v) {
        const int aw = c->roi[v].width, ah = c->roi[v].height, hw = aw / 2, hh = ah / 2;
        MS_CHECK(hw >= 2 && hh >= 2, "ms_set_meshes: view %d too small", v);
        MS_CHECK((long long)aw * ah < (1ll << 24) && aw < 65536 && ah < 65536, "ms_set_meshes: view %dx%d exceeds the scatter accumulators ([count:24 | sum:40])", aw, ah);
        max_aw = std::max(max_aw, aw); max_ah = std::max(max_ah, ah);
        max_tiles = std::max(max_tiles, div_up(aw, 64) * div_up(ah, 4 * MESH_TR));
    }
    if (int e = mesh_reserve(c, n_small, st)) return e;
    ms_ctx::MeshUpdater &U = c->mesh_upd;
    int tgt[MAX_VIEWS];
    for (int v = 0; v < NV; ++v) if (int e = mesh_begin_update(c, v, &tgt[v], st, v == 0)) return e;
    // the staging generation this call fills: free once the copy of the call a ring ago has run (its own event, recorded right behind that copy).  Until round 5 the host waited
    // here for the PREVIOUS update, twelve events were recorded and as many waits enqueued per call: a recalibration every 60 frames cost config 3 10.5 % of its frame rate with
    // 4 % of GPU work in it; now 4.5 % (same-box A/B 22.8 k -> 24.3 k frames/s, profiles/r05_experiments.txt)
    const int gen = U.stage_gen;
    if (U.stage_ev_set[gen]) MS_HIP(hipEventSynchronize(U.stage_ev[gen]));      // (blocks only when the caller is a whole ring of updates ahead of the GPU)
    // stage the caller's arrays in pinned memory, laid out like the vertex slots on the device (view after view, x | y): one copy for all views
    float *stage_gen = U.stage + (size_t)gen * MAX_VIEWS * U.stage_floats;
    MeshJobs T{};
    for (int v = 0; v < NV; ++v) {
        float *stg = stage_gen + (size_t)v * 2 * n_small;
        memcpy(stg, mesh_x + (size_t)v * n_small, n_small * 4);
        memcpy(stg + n_small, mesh_y + (size_t)v * n_small, n_small * 4);
        T.j[v] = mesh_job(c, v, tgt[v], n_small);
    }
    MS_HIP(hipMemcpyAsync(U.scratch.p, stage_gen, 2 * n_small * NV * sizeof(float), hipMemcpyHostToDevice, st));
    if (!U.stage_ev[gen]) MS_HIP(hipEventCreateWithFlags(&U.stage_ev[gen], hipEventDisableTiming));
    MS_HIP(hipEventRecord(U.stage_ev[gen], st));
    U.stage_ev_set[gen] = true;
    U.stage_gen = (gen + 1) % ms_ctx::MESH_STAGE_GENS;
    const dim3 blk(64, 4);
    k_mesh_expand_scatter_all<<<dim3(div_up(max_aw, 64), div_up(max_ah, 4 * MESH_SR), NV), blk, 0, st>>>(T, N, M);         // meshwarper.cpp:838-869, every view
    MS_LAUNCH_CHECK();
    k_mesh_mean_resize_all<<<dim3(std::min(max_tiles, 512), NV), blk, 0, st>>>(T);                                           // :870-883
    MS_LAUNCH_CHECK();
    for (int v = 0; v < NV; ++v) mesh_job_enqueued(c, v);
    // Publish every view in ONE mesh_mu critical section, the chain's record FIRST: a stitch on another thread that takes mesh_mu between two views of a
    // per-view publication saw mesh_wait[v] set while mesh_chain still held the PREVIOUS update's record (or none), waited for that, cleared the flag and read the
    // buffer k_mesh_mean_resize_all was still writing.  A stitch now sees either none of this call's views or all of them, behind this call's record.
    {
        std::lock_guard<std::mutex> mk(c->mesh_mu);
        MS_HIP(hipEventRecord(c->mesh_chain, st));
        c->mesh_chain_set = true;
        for (int v = 0; v < NV; ++v) {
            c->mesh_ready_via_chain[v] = true;
            c->mesh_wait[v] = true;
            c->mesh_active[v] = tgt[v];
            c->mesh_set[v] = true;
        }
    }
    return MS_OK;
}

// MeshWarper::interpolateMesh (meshwarper.cpp:337-354) + convertMeshesToMap: the RECALIB_INTERP branch of the recalibration thread
// (timed.cpp:449-457) re-expands start + (end - start) * progress every 30 ms
int ms_set_mesh_interp(ms_ctx *c, int view, const float *x0, const float *y0, const float *x1, const float *y1, int N, int M, float progress, ms_stream stream)
{
    MS_CHECK(x0 && y0 && x1 && y1 && N >= 2 && M >= 2, "ms_set_mesh_interp: need two N x M (>= 2x2) vertex meshes");
    std::vector<float> mx((size_t)N * M), my((size_t)N * M);
    for (size_t i = 0; i < mx.size(); ++i) {
        mx[i] = x0[i] + (x1[i] - x0[i]) * progress;        // fp32, in this order (-ffp-contract=off)
        my[i] = y0[i] + (y1[i] - y0[i]) * progress;
    }
    return ms_set_mesh(c, view, mx.data(), my.data(), N, M, stream);
}

int ms_get_mesh_displacement(ms_ctx *c, int view, float *out_px)
{
    if (int e = ctx_check_view(c, view)) return e;
    MS_CHECK(out_px != nullptr, "ms_get_mesh_displacement: null output");
    std::lock_guard<std::mutex> lk(c->mesh_update_mu);       // no update in flight while we look; ms_stitch is not blocked by this lock
    if (!c->blender_ready || !c->cfg.enable_cpw || !c->mesh_set[view] || !c->disp_dev.p) return fail(MS_ERR_STATE, "ms_get_mesh_displacement: no mesh set for view %d", view);
    if (c->mesh_ready[view]) { hipEvent_t rdy_; { std::lock_guard<std::mutex> mk_(c->mesh_mu); rdy_ = mesh_ready_event(c, view); } if (rdy_) MS_HIP(hipEventSynchronize(rdy_)); }
    float *h = (float *)pinned_scratch().get(sizeof(float));          // pinned landing zone: see PinnedScratch (common.hpp)
    if (!h) return fail(MS_ERR_NOMEM, "ms_get_mesh_displacement: no pinned staging memory");
    MS_HIP(hipMemcpy(h, (const unsigned *)c->disp_dev.p + 2 * view + c->mesh_active[view], sizeof(float), hipMemcpyDeviceToHost));
    *out_px = *h;
    return MS_OK;
}

int ms_get_mesh_maps(const ms_ctx *c, int view, ms_image *xm, ms_image *ym)
{
    if (int e = ctx_check_view(c, view)) return e;
    if (!c->blender_ready || !c->cfg.enable_cpw || !c->mesh_set[view]) return fail(MS_ERR_STATE, "ms_get_mesh_maps: no mesh set for view %d", view);
    if (c->mesh_ready[view]) { ms_ctx *mc_ = const_cast<ms_ctx *>(c); hipEvent_t rdy_; { std::lock_guard<std::mutex> mk_(mc_->mesh_mu); rdy_ = mesh_ready_event(mc_, view); } if (rdy_) MS_HIP(hipEventSynchronize(rdy_)); }       // updates are asynchronous: the maps are final after this
    if (xm) *xm = mesh_image(c, c->mesh_active[view], view, 0);
    if (ym) *ym = mesh_image(c, c->mesh_active[view], view, 1);
    return MS_OK;
}

}  // extern "C"
