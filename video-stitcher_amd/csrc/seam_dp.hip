// seam_dp.hip -- content-aware seams (ms_dp_seams; ms_calibrate_seam with MS_SEAM_DP): a minimum-cost dynamic-programming seam through the overlap of every
// view pair, in the spirit of detail::DpSeamFinder (sources/modules/stitching/src/seam_finders.cpp) but the project's own contract, stated in ms_stitch.h:
// integers only, so two calls return the same bytes and tests/dp_seam_ref.py is compared bit for bit.
//
// One pair = five launches on the caller's stream, every later one reading what the earlier ones left in the call's scratch block:
//   k_dp_sums    wide   count, sum x, sum y of either view's set pixels in the overlap grown by the gap: one partial per band of window rows
//   k_dp_decide  1 wg   partials -> orientation and owner of the first side (DpDecision), in 64-bit integers
//   k_dp_cost    wide   the cost plane in DP order: row t = DP step, column p = seam position (the transpose of the overlap for a horizontal seam)
//   k_dp_seam    1 wg   the recurrence, the end column and the backtrack
//   k_dp_edit    wide   the mask edit
// No atomics anywhere: partials are summed in a fixed order (and are integers).
//
// k_dp_seam.  Positions go across the 256 lanes, lane l takes p = l, l + 256, ...  The two live rows of M are in LDS (2 x 4096 x 4 bytes); a lane reads
// M(t-1, p-1 .. p+1), writes M(t, p) into the other row, and one barrier per row separates the rows.  The plane is walked in slabs of S = DP_SLAB_CELLS / P
// rows (>= 8): a slab's costs come into LDS with one wide load (the row loop then never waits for global memory), and the lane that consumes a cell's cost
// puts the cell's direction in its place.  A plane of one slab never leaves LDS.  A larger one writes each finished slab over its own costs in the global
// plane; the backtrack then brings the slabs back one at a time, last first, again with wide loads, and one lane walks S rows in LDS per slab: no chain of
// dependent global loads.
#include "common.hpp"
#include "launchers.hpp"

namespace ms {
namespace {

constexpr int DP_GAP = 10;                      // the orientation window: the overlap grown by findInPair's gap
constexpr unsigned DP_OUTSIDE = 1024;           // cost of an overlap pixel that is not set in both masks (> 765, the largest difference)
constexpr int DP_WG = 256;
constexpr int DP_SLAB_CELLS = 32768;            // 64 KiB of 16-bit cells: 8 rows of the widest plane
constexpr int DP_BAND = 8;                      // window rows per partial of k_dp_sums
static_assert(DP_SLAB_CELLS >= MS_DP_MAX_SIDE, "a slab holds at least one row");

struct DpPair { int rx, ry, rw, rh; int x1, y1, w1, h1; int x2, y2, w2, h2; };        // overlap roi, the two views' rois
struct DpDecision { int horizontal, first; };   // first = 0: view i owns the positions <= seam, 1: view j

__device__ __forceinline__ uint8_t dp_mask(const uint8_t *m, int w, int h, int y, int x) { return (y >= 0 && x >= 0 && y < h && x < w) ? m[(size_t)y * w + x] : 0; }

// the sum of six 64-bit values per lane over the workgroup, in s[0..6) (valid for every thread behind the call)
__device__ __forceinline__ void dp_block_sum6(unsigned long long v[6], unsigned long long (*s_w)[6], unsigned long long *s)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
        if (lane == 0) s_w[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned long long a = 0;
        for (int w = 0; w < DP_WG / 64; ++w) a += s_w[w][threadIdx.x];
        s[threadIdx.x] = a;
    }
    __syncthreads();
}

// partial[blockIdx.x] = {n1, sx1, sy1, n2, sx2, sy2} over the window rows [blockIdx.x * DP_BAND, + DP_BAND), coordinates relative to the window's corner
__global__ void __launch_bounds__(DP_WG) k_dp_sums(const uint8_t *__restrict__ m1, const uint8_t *__restrict__ m2, DpPair g, unsigned long long *__restrict__ partial)
{
    __shared__ unsigned long long s_w[DP_WG / 64][6], s[6];
    const int C = g.rw + 2 * DP_GAP, R = g.rh + 2 * DP_GAP;
    const int y0 = blockIdx.x * DP_BAND, rows = min(DP_BAND, R - y0);
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < rows * C; i += DP_WG) {
        const int y = y0 + i / C, x = i % C;
        if (dp_mask(m1, g.w1, g.h1, g.ry - g.y1 + y - DP_GAP, g.rx - g.x1 + x - DP_GAP)) { v[0] += 1; v[1] += (unsigned)x; v[2] += (unsigned)y; }
        if (dp_mask(m2, g.w2, g.h2, g.ry - g.y2 + y - DP_GAP, g.rx - g.x2 + x - DP_GAP)) { v[3] += 1; v[4] += (unsigned)x; v[5] += (unsigned)y; }
    }
    dp_block_sum6(v, s_w, s);
    if (threadIdx.x < 6) partial[(size_t)blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x];
}

// d = (sum_j n_i - sum_i n_j) per axis: the sign of the difference of the two centroids without a division.  n <= 4116^2 and sum <= 4116^3, so the products stay below 2^61.
__global__ void __launch_bounds__(DP_WG) k_dp_decide(const unsigned long long *__restrict__ partial, int n_partial, DpDecision *__restrict__ out)
{
    __shared__ unsigned long long s_w[DP_WG / 64][6], s[6];
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < n_partial; b += DP_WG)
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] += partial[(size_t)b * 6 + k];
    dp_block_sum6(v, s_w, s);
    if (threadIdx.x == 0) {
        const long long n1 = (long long)s[0], sx1 = (long long)s[1], sy1 = (long long)s[2], n2 = (long long)s[3], sx2 = (long long)s[4], sy2 = (long long)s[5];
        const long long dx = sx2 * n1 - sx1 * n2, dy = sy2 * n1 - sy1 * n2;
        const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
        DpDecision d;
        d.horizontal = ax >= ay ? 0 : 1;
        d.first = (d.horizontal ? dy : dx) >= 0 ? 0 : 1;
        *out = d;
    }
}

// overlap pixel (y, x) -> cell of the DP plane
__device__ __forceinline__ size_t dp_cell(const DpPair &g, int horizontal, int y, int x) { return horizontal ? (size_t)x * g.rh + y : (size_t)y * g.rw + x; }

// lanes along x: the two images and masks are read in their own row order; a horizontal seam's plane is written transposed (calibration-time: no LDS transpose)
__global__ void __launch_bounds__(DP_WG) k_dp_cost(const uint8_t *__restrict__ i1, const uint8_t *__restrict__ m1, const uint8_t *__restrict__ i2,
                                                   const uint8_t *__restrict__ m2, DpPair g, const DpDecision *__restrict__ dec, uint16_t *__restrict__ plane)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= g.rw || y >= g.rh) return;
    const size_t p1 = (size_t)(g.ry - g.y1 + y) * g.w1 + (g.rx - g.x1 + x), p2 = (size_t)(g.ry - g.y2 + y) * g.w2 + (g.rx - g.x2 + x);
    unsigned c = DP_OUTSIDE;
    if (m1[p1] && m2[p2]) {
        const uint8_t *a = i1 + 3 * p1, *b = i2 + 3 * p2;
        c = (unsigned)(abs((int)a[0] - (int)b[0]) + abs((int)a[1] - (int)b[1]) + abs((int)a[2] - (int)b[2]));
    }
    plane[dp_cell(g, dec->horizontal, y, x)] = (uint16_t)c;
}

// directions a cell holds once its cost is consumed: where the path came from
enum : uint16_t { DP_SAME = 0, DP_LEFT = 1, DP_RIGHT = 2 };

// `plane` is read and (for a plane of more than one slab) written by this workgroup alone; no __restrict__: the backtrack reads what the forward pass stored
__global__ void __launch_bounds__(DP_WG) k_dp_seam(DpPair g, const DpDecision *__restrict__ dec, uint16_t *plane, int *__restrict__ seam)
{
    __shared__ unsigned s_M[2][MS_DP_MAX_SIDE];
    __shared__ uint16_t s_slab[DP_SLAB_CELLS];
    __shared__ unsigned long long s_key[DP_WG / 64];
    __shared__ int s_x;
    const int tid = threadIdx.x;
    const int horizontal = dec->horizontal;
    const int P = horizontal ? g.rh : g.rw, T = horizontal ? g.rw : g.rh;        // positions per row, rows
    const int S = DP_SLAB_CELLS / P, n_slabs = (T + S - 1) / S;
    int cur = 0;                                                                // the row of s_M that holds M(t - 1, .)
    for (int sl = 0; sl < n_slabs; ++sl) {
        const int t0 = sl * S, rows = min(S, T - t0), cells = rows * P;
        uint16_t *gslab = plane + (size_t)t0 * P;
        for (int i = tid; i < cells; i += DP_WG) s_slab[i] = gslab[i];
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            uint16_t *row = s_slab + r * P;
            const unsigned *prev = s_M[cur];
            unsigned *next = s_M[cur ^ 1];
            if (t0 + r == 0) {
                for (int p = tid; p < P; p += DP_WG) { next[p] = row[p]; row[p] = DP_SAME; }
            } else {
                for (int p = tid; p < P; p += DP_WG) {
                    unsigned best = prev[p];
                    uint16_t d = DP_SAME;                                        // ties prefer p, then p - 1, then p + 1
                    if (p > 0 && prev[p - 1] < best) { best = prev[p - 1]; d = DP_LEFT; }
                    if (p + 1 < P && prev[p + 1] < best) { best = prev[p + 1]; d = DP_RIGHT; }
                    next[p] = best + row[p];
                    row[p] = d;
                }
            }
            cur ^= 1;
            __syncthreads();                                                    // the one barrier per row: M(t, .) complete, M(t - 1, .) free
        }
        if (n_slabs > 1) {                                                      // (uniform) the slab's directions over its costs
            for (int i = tid; i < cells; i += DP_WG) gslab[i] = s_slab[i];
            __syncthreads();
        }
    }
    // the end column: least M(T - 1, p), then least |2 p - (P - 1)|, then least p -- one 64-bit key (M < 2^23, the distance < 2^13, p < 2^13)
    unsigned long long key = ~0ull;
    for (int p = tid; p < P; p += DP_WG) {
        const int off = 2 * p - (P - 1);
        const unsigned long long k = ((unsigned long long)s_M[cur][p] << 32) | ((unsigned long long)(unsigned)(off < 0 ? -off : off) << 16) | (unsigned)p;
        key = k < key ? k : key;
    }
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(key, d, 64); key = o < key ? o : key; }
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DP_WG / 64; ++w) key = s_key[w] < key ? s_key[w] : key;
        s_x = (int)(key & 0xffffu);
    }
    __syncthreads();
    // backtrack: the last slab is still in LDS
    for (int sl = n_slabs - 1; sl >= 0; --sl) {
        const int t0 = sl * S, rows = min(S, T - t0);
        if (sl != n_slabs - 1) {
            const uint16_t *gslab = plane + (size_t)t0 * P;
            for (int i = tid; i < rows * P; i += DP_WG) s_slab[i] = gslab[i];
            __syncthreads();
        }
        if (tid == 0) {
            int x = s_x;
            for (int r = rows - 1; r >= 0; --r) {
                seam[t0 + r] = x;
                const uint16_t d = s_slab[r * P + x];
                x += d == DP_LEFT ? -1 : d == DP_RIGHT ? 1 : 0;
            }
            s_x = x;
        }
        __syncthreads();
    }
}

// only pixels both masks hold change: at or before the seam the second view's is cleared, beyond it the first view's
__global__ void __launch_bounds__(DP_WG) k_dp_edit(uint8_t *__restrict__ m1, uint8_t *__restrict__ m2, DpPair g, const DpDecision *__restrict__ dec, const int *__restrict__ seam)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= g.rw || y >= g.rh) return;
    const size_t p1 = (size_t)(g.ry - g.y1 + y) * g.w1 + (g.rx - g.x1 + x), p2 = (size_t)(g.ry - g.y2 + y) * g.w2 + (g.rx - g.x2 + x);
    if (!(m1[p1] && m2[p2])) return;
    const DpDecision d = *dec;
    const bool near = d.horizontal ? y <= seam[x] : x <= seam[y];
    if (near == (d.first == 0)) m2[p2] = 0;
    else m1[p1] = 0;
}

}  // namespace

// DP seams over DEVICE images (8UC3) and masks (8UC1), contiguous and roi-sized, masks in place, pairs in PairwiseSeamFinder::run's order.  The caller has checked
// that no overlap side exceeds MS_DP_MAX_SIDE.  Synchronous: one scratch block for the call, freed behind the stream.
int dp_seams_device(int n, const ms_rect *rois, const uint8_t *const *images, uint8_t *const *masks, hipStream_t st)
{
    size_t cells = 0;
    int side = 0, rows = 0;
    auto meet = [&](int i, int j, DpPair &g) {
        const int x0 = std::max(rois[i].x, rois[j].x), y0 = std::max(rois[i].y, rois[j].y);
        const int x1 = std::min(rois[i].x + rois[i].width, rois[j].x + rois[j].width), y1 = std::min(rois[i].y + rois[i].height, rois[j].y + rois[j].height);
        if (!(x0 < x1 && y0 < y1)) return false;
        g = DpPair{x0, y0, x1 - x0, y1 - y0, rois[i].x, rois[i].y, rois[i].width, rois[i].height, rois[j].x, rois[j].y, rois[j].width, rois[j].height};
        return true;
    };
    DpPair g;
    for (int i = 0; i + 1 < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (meet(i, j, g)) {
                if (g.rw > MS_DP_MAX_SIDE || g.rh > MS_DP_MAX_SIDE) return fail(MS_ERR_INVALID, "dp_seams_device: overlap of views %d and %d is %dx%d, a side above %d", i, j, g.rw, g.rh, MS_DP_MAX_SIDE);
                cells = std::max(cells, (size_t)g.rw * g.rh);
                side = std::max(side, std::max(g.rw, g.rh));
                rows = std::max(rows, g.rh + 2 * DP_GAP);
            }
    if (!cells) return MS_OK;
    // scratch: partials | decision | seam | plane
    const size_t n_part = (size_t)div_up(rows, DP_BAND);
    const size_t off_dec = n_part * 6 * sizeof(unsigned long long), off_seam = off_dec + 16, off_plane = (off_seam + (size_t)side * sizeof(int) + 15) & ~(size_t)15;
    char *buf = nullptr;
    MS_HIP(hipMalloc((void **)&buf, off_plane + cells * sizeof(uint16_t)));
    unsigned long long *partial = (unsigned long long *)buf;
    DpDecision *dec = (DpDecision *)(buf + off_dec);
    int *seam = (int *)(buf + off_seam);
    uint16_t *plane = (uint16_t *)(buf + off_plane);
    int rc = MS_OK;
    for (int i = 0; i + 1 < n && rc == MS_OK; ++i)
        for (int j = i + 1; j < n && rc == MS_OK; ++j) {
            if (!meet(i, j, g)) continue;
            const int np = div_up(g.rh + 2 * DP_GAP, DP_BAND);
            const dim3 grid(div_up(g.rw, 64), div_up(g.rh, 4)), block(64, 4);
            k_dp_sums<<<np, DP_WG, 0, st>>>(masks[i], masks[j], g, partial);
            k_dp_decide<<<1, DP_WG, 0, st>>>(partial, np, dec);
            k_dp_cost<<<grid, block, 0, st>>>(images[i], masks[i], images[j], masks[j], g, dec, plane);
            k_dp_seam<<<1, DP_WG, 0, st>>>(g, dec, plane, seam);
            k_dp_edit<<<grid, block, 0, st>>>(masks[i], masks[j], g, dec, seam);
            if (hipGetLastError() != hipSuccess) rc = fail(MS_ERR_HIP, "dp_seams_device: launch failed");
        }
    if (hipStreamSynchronize(st) != hipSuccess && rc == MS_OK) rc = fail(MS_ERR_HIP, "dp_seams_device: sync failed");
    (void)hipFree(buf);
    return rc;
}

}  // namespace ms
