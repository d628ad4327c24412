// calib.hip -- calibration-time pixel work that the reference runs on the CPU, on the device:
//   VoronoiSeamFinder::findInPair       sources/modules/stitching/src/seam_finders.cpp:111-160
//       distanceTransform(DIST_L1, 3)   sources/modules/imgproc/src/distransform.cpp:70-137
//   GainCompensator::feed               sources/modules/stitching/src/exposure_compensate.cpp:71-145 (overlap sums, normal equations, cv::solve)
// so that ms_build_masks / ms_calibrate_seam move no pixels to the host: the only thing that comes back is the N gains.
// Below them, exposure tracking from live frames (ms_gain_stats / ms_track_gains and their NV12, column-shard and view-shard forms): GainCompensator::feed's
// statistics at compose scale on the caller's stream -- the kernels, and behind them the entry points that launch them (the context type comes from ctx.hpp).
//
// Exactness.  The reference's two-pass 3 x 3 chamfer with costs (1, 2) IS the city-block distance to the nearest zero pixel of the window
// (a diagonal step costs two axis steps), in 16.16 fixed point; here the same integers come from two separable 1-D passes (columns, then
// rows), which parallelise.  Where a window has no zero pixel at all the chamfer leaves INIT + 1 everywhere; the separable form leaves a
// large constant too, and the only use of the distances is `dist1 < dist2`, so the seam is the same.
// The gain sums are DOUBLE sums of square roots in raster order (exposure_compensate.cpp:103-117): order matters for the last bit, so one
// thread per image pair walks its overlap in that order (the overlaps are seam-scale images: a few thousand pixels); the n x n solve follows
// cv::solve's closed forms / LU (as the host version did) in a single thread.
#include "common.hpp"
#include "launchers.hpp"
#include "descs.hpp"
#include "ctx.hpp"

namespace ms {
// ---- exposure tracking: what its kernels take by value (the entry points below fill it).  The sample lattice, the views' static maps and this call's frames: -------
struct GainTrackViews {
    const float *xmap[MS_MAX_VIEWS]; int pitch[MS_MAX_VIEWS];      // projection maps (ymap follows xmap: roi.height rows further), pitch in elements
    ms_rect roi[MS_MAX_VIEWS];
    const uint8_t *src[MS_MAX_VIEWS]; unsigned step[MS_MAX_VIEWS]; // this call's 8UC3 frames, or their NV12 planes (active views only)
    ms_rect T; int stride, nsx, nsy;                               // pano ROI, lattice step, samples per row / column
    int n, src_w, src_h; unsigned active;
};
constexpr int GAIN_TRACK_MAX_TABLES = MS_MAX_VIEWS + 4;            // full set, its alternate copy, num_views + 1 cached subsets
struct GainTrackTables { ViewDesc *tab[GAIN_TRACK_MAX_TABLES]; int n; };
// Partial statistics (ms_gain_stats_partial / ms_track_gains_from_partials): the raw accumulators of one column window in a caller-owned device buffer, so that
// the windows' integers add up on the device to the unsharded statistic.  Layout of a partial of an n-view context (ms_gain_partial_bytes):
//   GainPartialHeader, cnt[n * n] (symmetric), S[n * n]  -- unsigned 64-bit each, before the max(1, cnt) rule
constexpr unsigned GAIN_PARTIAL_MAGIC = 0x50474d53u;               // "SMGP"
constexpr int GAIN_MAX_PARTIALS = 16;                              // = the largest ms_config.col_shards
struct GainPartialHeader { unsigned magic, n, active, stride; int tx, ty, tw, th; };      // T = the pano ROI the lattice starts from (the same on every shard)
struct GainPartials { const unsigned long long *p[GAIN_MAX_PARTIALS]; int n; };
inline size_t gain_partial_bytes(int n) { return sizeof(GainPartialHeader) + 2 * (size_t)n * n * sizeof(unsigned long long); }
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
inline GainSampleRects gain_sample_rects(const GainTrackViews &V)
{
    GainSampleRects R;
    auto first = [](int lo, int s) { return lo <= 0 ? 0 : (lo + s - 1) / s; };      // the smallest k >= 0 with k * s >= lo
    for (int v = 0; v < V.n; ++v) {
        const ms_rect r = V.roi[v];
        const int x0 = first(r.x - V.T.x, V.stride), x1 = std::min(V.nsx, first(r.x + r.width - V.T.x, V.stride));
        const int y0 = first(r.y - V.T.y, V.stride), y1 = std::min(V.nsy, first(r.y + r.height - V.T.y, V.stride));
        R.x0[v] = x0; R.y0[v] = y0; R.w[v] = std::max(0, x1 - x0); R.h[v] = std::max(0, y1 - y0);
    }
    return R;
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

namespace {

constexpr int VGAP = 10;                 // findInPair's `gap`
constexpr int DINF = 1 << 28;

struct PairGeom { int rx, ry, rw, rh; int x1, y1, w1, h1; int x2, y2, w2, h2; };        // overlap roi, the two views' rois

__device__ __forceinline__ uint8_t at_mask(const uint8_t *m, int w, int h, int y, int x) { return (y >= 0 && x >= 0 && y < h && x < w) ? m[(size_t)y * w + x] : 0; }

// columns of the (rh + 2 gap) x (rw + 2 gap) window: distance, along the column, to the nearest pixel that is set in exactly one of the two masks
__global__ void __launch_bounds__(64) k_vor_cols(const uint8_t *__restrict__ m1, const uint8_t *__restrict__ m2, PairGeom g, int *__restrict__ d1, int *__restrict__ d2)
{
    const int C = g.rw + 2 * VGAP, R = g.rh + 2 * VGAP;
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= C) return;
    int a1 = DINF, a2 = DINF;
    for (int y = 0; y < R; ++y) {
        const uint8_t a = at_mask(m1, g.w1, g.h1, g.ry - g.y1 + y - VGAP, g.rx - g.x1 + x - VGAP);
        const uint8_t b = at_mask(m2, g.w2, g.h2, g.ry - g.y2 + y - VGAP, g.rx - g.x2 + x - VGAP);
        const bool both = a && b;
        a1 = (!both && a) ? 0 : min(a1 + 1, DINF);
        a2 = (!both && b) ? 0 : min(a2 + 1, DINF);
        d1[(size_t)y * C + x] = a1; d2[(size_t)y * C + x] = a2;
    }
    a1 = a2 = DINF;
    for (int y = R - 1; y >= 0; --y) {
        const size_t i = (size_t)y * C + x;
        a1 = min(min(a1 + 1, DINF), d1[i]); a2 = min(min(a2 + 1, DINF), d2[i]);
        d1[i] = a1; d2[i] = a2;
    }
}
// rows: the second 1-D pass, then the seam decision of findInPair (:148-159) on the overlap itself
__global__ void __launch_bounds__(64) k_vor_rows(uint8_t *__restrict__ m1, uint8_t *__restrict__ m2, PairGeom g, int *__restrict__ d1, int *__restrict__ d2)
{
    const int C = g.rw + 2 * VGAP, R = g.rh + 2 * VGAP;
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (y >= R) return;
    int *r1 = d1 + (size_t)y * C, *r2 = d2 + (size_t)y * C;
    int a1 = DINF, a2 = DINF;
    for (int x = 0; x < C; ++x) { a1 = min(min(a1 + 1, DINF), r1[x]); a2 = min(min(a2 + 1, DINF), r2[x]); r1[x] = a1; r2[x] = a2; }
    a1 = a2 = DINF;
    const bool inner_row = y >= VGAP && y < VGAP + g.rh;
    for (int x = C - 1; x >= 0; --x) {
        a1 = min(min(a1 + 1, DINF), r1[x]); a2 = min(min(a2 + 1, DINF), r2[x]);
        if (inner_row && x >= VGAP && x < VGAP + g.rw) {
            const int yy = y - VGAP, xx = x - VGAP;
            if (a1 < a2) m2[(size_t)(g.ry - g.y2 + yy) * g.w2 + (g.rx - g.x2 + xx)] = 0;
            else m1[(size_t)(g.ry - g.y1 + yy) * g.w1 + (g.rx - g.x1 + xx)] = 0;
        }
    }
}

// GainCompensator::feed's overlap statistics (exposure_compensate.cpp:90-121), one thread per pair i <= j
struct GainViews { const uint8_t *img[MS_MAX_VIEWS]; const uint8_t *mask[MS_MAX_VIEWS]; ms_rect roi[MS_MAX_VIEWS]; int n; };
__global__ void __launch_bounds__(64) k_gain_pairs(GainViews V, int *__restrict__ Nm, double *__restrict__ Im)
{
    const int p = blockIdx.x * 64 + threadIdx.x, n = V.n;
    if (p >= n * n) return;
    const int i = p / n, j = p % n;
    if (j < i) return;
    const ms_rect a = V.roi[i], b = V.roi[j];
    const int x0 = max(a.x, b.x), y0 = max(a.y, b.y), x1 = min(a.x + a.width, b.x + b.width), y1 = min(a.y + a.height, b.y + b.height);
    if (!(x0 < x1 && y0 < y1)) return;                                    // (the matrices are zero-initialised)
    int cnt = 0;
    double s1 = 0, s2 = 0;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const size_t p1 = (size_t)(y - a.y) * a.width + (x - a.x), p2 = (size_t)(y - b.y) * b.width + (x - b.x);
            if (V.mask[i][p1] != 255 || V.mask[j][p2] != 255) continue;
            ++cnt;
            const uint8_t *u = V.img[i] + 3 * p1, *w = V.img[j] + 3 * p2;
            s1 += sqrt(static_cast<double>(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]));
            s2 += sqrt(static_cast<double>(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]));
        }
    const int N = max(1, cnt);
    Nm[i * n + j] = Nm[j * n + i] = N;
    Im[i * n + j] = s1 / N;
    Im[j * n + i] = s2 / N;
}
// the normal equations (:123-139) and cv::solve(A, b, gains) with DECOMP_LU semantics (closed forms up to 3 x 3: lapack.cpp:1107-1237; LU with partial
// pivoting otherwise: matrix_decomp.cpp:52-112) in one thread; ok = 0 if the system is singular
__device__ void gain_solve(int n, const int *__restrict__ Nm, const double *__restrict__ Im, double *__restrict__ gains, int *__restrict__ ok)
{
    double A[MS_MAX_VIEWS * MS_MAX_VIEWS], b[MS_MAX_VIEWS];
    const double alpha = 0.01, beta = 100;
    for (int i = 0; i < n; ++i) { b[i] = 0; for (int j = 0; j < n; ++j) A[i * n + j] = 0; }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            b[i] += beta * Nm[i * n + j];
            A[i * n + i] += beta * Nm[i * n + j];
            if (j == i) continue;
            A[i * n + i] += 2 * alpha * Im[i * n + j] * Im[i * n + j] * Nm[i * n + j];
            A[i * n + j] -= 2 * alpha * Im[i * n + j] * Im[j * n + i] * Nm[i * n + j];
        }
#define AT(i, j) A[(i) * n + (j)]
    *ok = 1;
    if (n == 1) { if (AT(0, 0) == 0.) *ok = 0; else b[0] = b[0] / AT(0, 0); }
    else if (n == 2) {
        double d = AT(0, 0) * AT(1, 1) - AT(0, 1) * AT(1, 0);
        if (d == 0.) *ok = 0;
        else { d = 1. / d; const double t = (b[0] * AT(1, 1) - b[1] * AT(0, 1)) * d; b[1] = (b[1] * AT(0, 0) - b[0] * AT(1, 0)) * d; b[0] = t; }
    } else if (n == 3) {
        double d = AT(0, 0) * (AT(1, 1) * AT(2, 2) - AT(1, 2) * AT(2, 1)) - AT(0, 1) * (AT(1, 0) * AT(2, 2) - AT(1, 2) * AT(2, 0)) +
                   AT(0, 2) * (AT(1, 0) * AT(2, 1) - AT(1, 1) * AT(2, 0));
        if (d == 0.) *ok = 0;
        else {
            d = 1. / d;
            const double t0 = ((AT(1, 1) * AT(2, 2) - AT(1, 2) * AT(2, 1)) * b[0] + (AT(0, 2) * AT(2, 1) - AT(0, 1) * AT(2, 2)) * b[1] + (AT(0, 1) * AT(1, 2) - AT(0, 2) * AT(1, 1)) * b[2]) * d;
            const double t1 = ((AT(1, 2) * AT(2, 0) - AT(1, 0) * AT(2, 2)) * b[0] + (AT(0, 0) * AT(2, 2) - AT(0, 2) * AT(2, 0)) * b[1] + (AT(0, 2) * AT(1, 0) - AT(0, 0) * AT(1, 2)) * b[2]) * d;
            const double t2 = ((AT(1, 0) * AT(2, 1) - AT(1, 1) * AT(2, 0)) * b[0] + (AT(0, 1) * AT(2, 0) - AT(0, 0) * AT(2, 1)) * b[1] + (AT(0, 0) * AT(1, 1) - AT(0, 1) * AT(1, 0)) * b[2]) * d;
            b[0] = t0; b[1] = t1; b[2] = t2;
        }
    } else {
        const double eps = 2.220446049250313e-16 * 100;
        for (int i = 0; i < n && *ok; ++i) {
            int k = i;
            for (int j = i + 1; j < n; ++j) if (fabs(AT(j, i)) > fabs(AT(k, i))) k = j;
            if (fabs(AT(k, i)) < eps) { *ok = 0; break; }
            if (k != i) { for (int j = i; j < n; ++j) { const double t = AT(i, j); AT(i, j) = AT(k, j); AT(k, j) = t; } const double t = b[i]; b[i] = b[k]; b[k] = t; }
            const double d = -1 / AT(i, i);
            for (int j = i + 1; j < n; ++j) {
                const double al = AT(j, i) * d;
                for (int q = i + 1; q < n; ++q) AT(j, q) += al * AT(i, q);
                b[j] += al * b[i];
            }
        }
        for (int i = n - 1; i >= 0 && *ok; --i) {
            double sv = b[i];
            for (int q = i + 1; q < n; ++q) sv -= AT(i, q) * b[q];
            b[i] = sv / AT(i, i);
        }
    }
#undef AT
    for (int i = 0; i < n; ++i) gains[i] = *ok ? b[i] : 1.0;
}
__global__ void k_gain_solve(int n, const int *__restrict__ Nm, const double *__restrict__ Im, double *__restrict__ gains, int *__restrict__ ok)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    gain_solve(n, Nm, Im, gains, ok);
}

// ---- exposure tracking (ms_track_gains): GainCompensator::feed's statistics at compose scale from live frames, on the caller's stream ---------
// A lane owns one sample of the pano lattice.  It finds the views that see the sample (k_valid_mask's rule on the static maps), keeps their
// q = llrint(sqrt(b^2 + g^2 + r^2) * 2^20) (< 2^29, so 32 bits) in its own LDS column, and the wave then walks the pairs some lane of it saw:
// ballot + popcount for the count, a 64-bit butterfly for the sums, one LDS atomic per pair and wave, one global atomic per non-zero cell and
// workgroup.  Everything is an integer, so the result does not depend on the order in which workgroups arrive.
//   acc[0 .. n*n)       cnt of the pair (i, j), stored at i <= j only
//   acc[n*n .. 2 n*n)   S[i][j] = sum of q_i over the samples i and j both see
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ bool rects_meet(const ms_rect &a, const ms_rect &b)
{
    return max(a.x, b.x) < min(a.x + a.width, b.x + b.width) && max(a.y, b.y) < min(a.y + a.height, b.y + b.height);
}
// NV12: the frames are the cameras' planes (ms_gain_stats_nv12 / ms_track_gains_nv12) -- Y at the truncated coordinate, the UV pair of its 2 x 2 block, through
// cvtColor's integer formula (nv12_bgr, common.hpp) to the b, g, r the 8UC3 form reads from memory: 1 + 2 bytes per view and sample instead of 3, the same integers.
// q of view a at the pixel (lx, ly) of its warped ROI, or "not seen": the one copy of map -> source pixel -> q (k_gain_stats and k_gain_samples)
template <bool NV12>
__device__ __forceinline__ bool gain_sample_q(const GainTrackViews &V, int a, int lx, int ly, unsigned &q)
{
    const ms_rect r = V.roi[a];
    const size_t at = (size_t)ly * V.pitch[a] + lx;
    const int xx = f2i_rz(V.xmap[a][at]), yy = f2i_rz(V.xmap[a][at + (size_t)r.height * V.pitch[a]]);      // (ymap follows xmap)
    if (!(xx >= 0 && xx < V.src_w && yy >= 0 && yy < V.src_h)) return false;
    int b0, b1, b2;
    if constexpr (NV12) {
        const uint8_t *uv = V.src[a] + (size_t)(V.src_h + (yy >> 1)) * V.step[a] + (xx & ~1);
        const NvRGB c = nv12_bgr(V.src[a][(size_t)yy * V.step[a] + xx], (unsigned)uv[0] | ((unsigned)uv[1] << 8));
        b0 = (int)c.b; b1 = (int)c.g; b2 = (int)c.r;
    } else {
        const uint8_t *p = V.src[a] + (size_t)yy * V.step[a] + 3 * xx;
        b0 = p[0]; b1 = p[1]; b2 = p[2];
    }
    q = (unsigned)llrint(sqrt(static_cast<double>(b0 * b0 + b1 * b1 + b2 * b2)) * 1048576.0);
    return true;
}
// the pair walk behind the lanes' s_q columns: the one copy of it (k_gain_stats and k_gain_stats_from_samples).  s_acc is zeroed by the caller before.
__device__ __forceinline__ void gain_pair_sums(int n, unsigned seen, unsigned wave_seen, const unsigned (*s_q)[256], unsigned long long *s_acc,
                                               unsigned long long *__restrict__ acc, int tid, int lane)
{
    const int nn = n * n;
    __syncthreads();
    for (unsigned mi = wave_seen; mi; mi &= mi - 1u) {
        const int i = __ffs(mi) - 1;
        for (unsigned mj = mi; mj; mj &= mj - 1u) {           // j >= i, i itself included (exposure_compensate.cpp:90)
            const int j = __ffs(mj) - 1;
            const bool both = ((seen >> i) & (seen >> j) & 1u) != 0u;
            const unsigned long long bal = __ballot(both);
            if (!bal) continue;
            const unsigned long long si = wave_sum_u64(both ? s_q[i][tid] : 0u);
            const unsigned long long sj = j != i ? wave_sum_u64(both ? s_q[j][tid] : 0u) : 0ull;
            if (lane == 0) {
                atomicAdd(&s_acc[i * n + j], (unsigned long long)__popcll(bal));
                atomicAdd(&s_acc[nn + i * n + j], si);
                if (j != i) atomicAdd(&s_acc[nn + j * n + i], sj);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * nn; i += 256)
        if (s_acc[i]) atomicAdd(&acc[i], s_acc[i]);
}
template <bool NV12>
__global__ void __launch_bounds__(256) k_gain_stats(GainTrackViews V, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned s_q[MS_MAX_VIEWS][256];
    __shared__ unsigned long long s_acc[2 * MS_MAX_VIEWS * MS_MAX_VIEWS];
    const int n = V.n, nn = n * n, tid = threadIdx.y * 64 + threadIdx.x, lane = threadIdx.x;
    for (int i = tid; i < 2 * nn; i += 256) s_acc[i] = 0ull;
    const int sx = blockIdx.x * 64 + threadIdx.x, sy = blockIdx.y * 4 + threadIdx.y;
    const bool inside = sx < V.nsx && sy < V.nsy;
    const int u = V.T.x + sx * V.stride, v = V.T.y + sy * V.stride;
    unsigned seen = 0u, wave_seen = 0u;
    for (int a = 0; a < n; ++a) {
        if (!((V.active >> a) & 1u)) continue;
        const ms_rect r = V.roi[a];
        const int lx = u - r.x, ly = v - r.y;
        bool s = false;
        unsigned q = 0u;
        if (inside && lx >= 0 && ly >= 0 && lx < r.width && ly < r.height) s = gain_sample_q<NV12>(V, a, lx, ly, q);
        s_q[a][tid] = q;                                      // (read back by this lane only)
        if (s) seen |= 1u << a;
        if (__ballot(s)) wave_seen |= 1u << a;                // (wave-uniform)
    }
    gain_pair_sums(n, seen, wave_seen, s_q, s_acc, acc, tid, lane);
}
// N and S as the header states them, from the accumulators; which are cleared for the next call
__device__ __forceinline__ void gain_cell(const GainTrackViews &V, const unsigned long long *acc, int i, int j, long long &N, long long &S)
{
    N = 0; S = 0;
    if (!((V.active >> i) & (V.active >> j) & 1u) || !rects_meet(V.roi[i], V.roi[j])) return;
    const long long cnt = (long long)acc[min(i, j) * V.n + max(i, j)];
    N = cnt > 1 ? cnt : 1;
    S = (long long)acc[V.n * V.n + i * V.n + j];
}
__global__ void __launch_bounds__(256) k_gain_export(GainTrackViews V, unsigned long long *__restrict__ acc, long long *__restrict__ outN, long long *__restrict__ outS)
{
    const int n = V.n, nn = n * n, p = threadIdx.x;
    if (p < nn) gain_cell(V, acc, p / n, p % n, outN[p], outS[p]);
    __syncthreads();
    for (int i = p; i < 2 * nn; i += 256) acc[i] = 0ull;
}
// statistics -> I -> solve over the active views -> smooth -> state and every listed view table; one workgroup of 256.  `acc` = the accumulators of this
// context (k_gain_update) or the sum of the shards' partials in LDS (k_gain_update_partials): one body, so both routes run the same arithmetic in the same order.
__device__ __forceinline__ void gain_update_body(const GainTrackViews &V, const GainTrackTables &W, const unsigned long long *acc, double *__restrict__ state,
                                                 int *__restrict__ counters, double lambda)
{
    __shared__ int s_N[MS_MAX_VIEWS * MS_MAX_VIEWS];
    __shared__ double s_I[MS_MAX_VIEWS * MS_MAX_VIEWS], s_g[MS_MAX_VIEWS];
    __shared__ int s_ok;
    const int n = V.n, nn = n * n, p = threadIdx.x, m = __popc(V.active);
    if (p < nn) {
        const int i = p / n, j = p % n;
        if ((V.active >> i) & (V.active >> j) & 1u) {         // the system holds the active views only, in view order
            const int ci = __popc(V.active & ((1u << i) - 1u)), cj = __popc(V.active & ((1u << j) - 1u));
            long long N, S;
            gain_cell(V, acc, i, j, N, S);
            s_N[ci * m + cj] = (int)N;
            s_I[ci * m + cj] = N ? (double)S / 1048576.0 / (double)N : 0.0;
        }
    }
    __syncthreads();
    if (p == 0) {
        gain_solve(m, s_N, s_I, s_g, &s_ok);
        counters[s_ok ? 0 : 1] += 1;
    }
    __syncthreads();
    if (p < n && ((V.active >> p) & 1u) && s_ok) {            // singular: nothing changes; an inactive view keeps its gain
        double g = state[p];
        g = g + lambda * (s_g[__popc(V.active & ((1u << p) - 1u))] - g);
        state[p] = g;
        for (int t = 0; t < W.n; ++t) W.tab[t][p].gain = (float)g;
    }
}
__global__ void __launch_bounds__(256) k_gain_update(GainTrackViews V, GainTrackTables W, unsigned long long *__restrict__ acc, double *__restrict__ state,
                                                     int *__restrict__ counters, double lambda)
{
    gain_update_body(V, W, acc, state, counters, lambda);
    for (int i = threadIdx.x; i < 2 * V.n * V.n; i += 256) acc[i] = 0ull;      // (behind the body's barriers: every read of a cell is done)
}

// ---- partial statistics: column shards (ms_gain_stats_partial / ms_track_gains_from_partials) ------------------------------------------------------
// k_gain_stats over the lattice columns of this context's window IS the partial statistic: ms_gain_stats_partial hands it a lattice whose origin is the window's first
// sample column (V.T.x, V.nsx), so the kernel that reads the pixels is the one ms_track_gains runs.  k_gain_partial_export moves the raw accumulators into the
// caller's buffer behind a header and clears them for the next call; plain vector stores.
__global__ void __launch_bounds__(256) k_gain_partial_export(int n, GainPartialHeader H, unsigned long long *__restrict__ acc, unsigned *__restrict__ out)
{
    const int nn = n * n, p = threadIdx.x;
    unsigned long long *body = reinterpret_cast<unsigned long long *>(out + sizeof(GainPartialHeader) / sizeof(unsigned));
    if (p == 0) { out[0] = H.magic; out[1] = H.n; out[2] = H.active; out[3] = H.stride; out[4] = (unsigned)H.tx; out[5] = (unsigned)H.ty; out[6] = (unsigned)H.tw; out[7] = (unsigned)H.th; }
    if (p < nn) {
        const int i = p / n, j = p % n;
        body[p] = acc[min(i, j) * n + max(i, j)];             // (k_gain_stats keeps cnt at i <= j only)
        body[nn + p] = acc[nn + p];
    }
    __syncthreads();
    for (int i = p; i < 2 * nn; i += 256) acc[i] = 0ull;
}
// P partials -> header check -> integer sums in LDS, partial by partial in the order given -> gain_update_body.  One workgroup of 256.  A header that differs from
// what this context and this call expect (another rig, active set, stride or lattice origin; or not a partial at all): nothing changes, one rejected update counted.
__global__ void __launch_bounds__(256) k_gain_update_partials(GainTrackViews V, GainTrackTables W, GainPartialHeader H, GainPartials P, double *__restrict__ state,
                                                              int *__restrict__ counters, double lambda)
{
    __shared__ unsigned long long s_sum[2 * MS_MAX_VIEWS * MS_MAX_VIEWS];
    const int nn = V.n * V.n, p = threadIdx.x;
    constexpr int HW = sizeof(GainPartialHeader) / sizeof(unsigned);
    const unsigned want[HW] = {H.magic, H.n, H.active, H.stride, (unsigned)H.tx, (unsigned)H.ty, (unsigned)H.tw, (unsigned)H.th};
    int bad = 0;
    for (int k = p; k < P.n * HW; k += 256)
        bad |= reinterpret_cast<const unsigned *>(P.p[k / HW])[k % HW] != want[k % HW];
    if (__syncthreads_or(bad)) {                              // (uniform: every thread leaves)
        if (p == 0) counters[2] += 1;
        return;
    }
    for (int i = p; i < 2 * nn; i += 256) {
        unsigned long long s = 0ull;
        for (int k = 0; k < P.n; ++k) s += P.p[k][HW / 2 + i];
        s_sum[i] = s;
    }
    __syncthreads();
    gain_update_body(V, W, s_sum, state, counters, lambda);
}


// ---- sample vectors: view shards (ms_gain_samples / ms_track_gains_from_samples) -------------------------------------------------------------------------
// A view shard holds the pixels of its own views only, so it cannot form a pair sum; it can store what a pair needs of each of its views, q or "not seen" at
// every lattice sample of the view's rectangle R_v (GainSampleRects, above).  k_gain_samples: a lane owns one sample of one held view, lanes along sx, so a wave stores
// one contiguous run of 4-byte words and reads the maps as k_gain_stats does.  The grid is the held views' own 64 x 4 tiles one after the other (first[i] = the
// first workgroup of the i-th held view): no workgroup for a view of another shard, none beyond a small rectangle because another view's is large.  Workgroup 0
// also stores header and offset table.
struct GainSampleOut { unsigned off[MS_MAX_VIEWS]; unsigned held, words; int nheld; unsigned char view[MS_MAX_VIEWS]; unsigned first[MS_MAX_VIEWS + 1]; };
template <bool NV12>
__global__ void __launch_bounds__(256) k_gain_samples(GainTrackViews V, GainSampleRects R, GainSampleOut O, unsigned *__restrict__ out)
{
    const int tid = threadIdx.y * 64 + threadIdx.x;
    if (blockIdx.x == 0) {
        const unsigned hdr[GAIN_SAMPLES_HEADER_WORDS] = {GAIN_SAMPLES_MAGIC, (unsigned)V.n, V.active, (unsigned)V.stride, (unsigned)V.T.x, (unsigned)V.T.y,
                                                         (unsigned)V.T.width, (unsigned)V.T.height, O.held, O.words * 4u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (tid < GAIN_SAMPLES_HEADER_WORDS) out[tid] = hdr[tid];
        else if (tid < GAIN_SAMPLES_HEADER_WORDS + V.n) out[tid] = O.off[tid - GAIN_SAMPLES_HEADER_WORDS];
    }
    int i = 0;
    while (i < O.nheld && blockIdx.x >= O.first[i + 1]) ++i;      // (uniform; <= 16 steps)
    if (i >= O.nheld) return;                                     // (the lone workgroup of a buffer without samples)
    const int a = O.view[i], tile = blockIdx.x - O.first[i], tiles_x = (R.w[a] + 63) / 64;
    const int rx = (tile % tiles_x) * 64 + threadIdx.x, ry = (tile / tiles_x) * 4 + threadIdx.y;
    if (rx >= R.w[a] || ry >= R.h[a]) return;
    const ms_rect r = V.roi[a];
    const int lx = V.T.x + (R.x0[a] + rx) * V.stride - r.x, ly = V.T.y + (R.y0[a] + ry) * V.stride - r.y;
    unsigned q = 0u;
    bool s = false;
    if (lx >= 0 && ly >= 0 && lx < r.width && ly < r.height) s = gain_sample_q<NV12>(V, a, lx, ly, q);      // (holds by the definition of R_v)
    out[O.off[a] + (size_t)ry * R.w[a] + rx] = s ? q + 1u : 0u;
}
// The headers of the buffers against what this context and this call expect, and which buffer holds which view: s_src[v] = the data of view v.  Every thread of
// the workgroup (<= 256, at least 128) calls it; the answer is uniform.  Refused: a header word that differs (magic, views, active set, stride, T, padding), a
// view held twice or held but not active, an active view nobody holds, an offset table or a size other than what gain_sample_offsets gives for the views held
// -- so behind a header that passes, every word this call reads lies inside the size the producer was given.
__device__ __forceinline__ bool gain_samples_resolve(const GainTrackViews &V, const GainSampleRects &R, const GainSampleBufs &P, const unsigned **s_src)
{
    constexpr int HW = GAIN_SAMPLES_HEADER_WORDS, TW = HW + MS_MAX_VIEWS;
    __shared__ unsigned s_h[GAIN_MAX_SAMPLE_BUFS][TW];
    __shared__ int s_good;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    if (tid < P.n * TW && tid % TW < HW + V.n) s_h[tid / TW][tid % TW] = P.p[tid / TW][tid % TW];
    __syncthreads();
    if (tid == 0) {
        const unsigned want[8] = {GAIN_SAMPLES_MAGIC, (unsigned)V.n, V.active, (unsigned)V.stride, (unsigned)V.T.x, (unsigned)V.T.y, (unsigned)V.T.width, (unsigned)V.T.height};
        bool good = true;
        unsigned have = 0u;
        for (int k = 0; k < P.n; ++k) {
            const unsigned *h = s_h[k], held = h[8];
            for (int w = 0; w < 8; ++w) good = good && h[w] == want[w];
            for (int w = 10; w < HW; ++w) good = good && h[w] == 0u;
            good = good && !(held & ~V.active) && !(held & have);
            unsigned at = HW + V.n;
            for (int v = 0; v < V.n; ++v) {
                if ((held >> v) & 1u) {
                    good = good && h[HW + v] == at;
                    s_src[v] = P.p[k] + at;
                    at += (unsigned)R.w[v] * (unsigned)R.h[v];
                } else
                    good = good && h[HW + v] == 0u;
            }
            good = good && h[9] == at * 4u;
            have |= held;
        }
        s_good = good && have == V.active;
    }
    __syncthreads();
    return s_good != 0;
}
// k_gain_stats' lattice walk with s_q filled from the buffers.  Every workgroup checks the headers itself (a few hundred bytes out of L2) before it reads a data
// word: a set that the update below will reject adds nothing to the accumulators, and no launch has to run between "checked" and "summed".
__global__ void __launch_bounds__(256) k_gain_stats_from_samples(GainTrackViews V, GainSampleRects R, GainSampleBufs P, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned s_q[MS_MAX_VIEWS][256];
    __shared__ unsigned long long s_acc[2 * MS_MAX_VIEWS * MS_MAX_VIEWS];
    __shared__ const unsigned *s_src[MS_MAX_VIEWS];
    const int n = V.n, nn = n * n, tid = threadIdx.y * 64 + threadIdx.x, lane = threadIdx.x;
    for (int i = tid; i < 2 * nn; i += 256) s_acc[i] = 0ull;
    if (!gain_samples_resolve(V, R, P, s_src)) return;        // (uniform)
    const int sx = blockIdx.x * 64 + threadIdx.x, sy = blockIdx.y * 4 + threadIdx.y;
    const bool inside = sx < V.nsx && sy < V.nsy;
    unsigned seen = 0u, wave_seen = 0u;
    for (int a = 0; a < n; ++a) {
        if (!((V.active >> a) & 1u)) continue;
        const int rx = sx - R.x0[a], ry = sy - R.y0[a];
        unsigned word = 0u;
        if (inside && rx >= 0 && ry >= 0 && rx < R.w[a] && ry < R.h[a]) word = s_src[a][(size_t)ry * R.w[a] + rx];
        const bool s = word != 0u;
        s_q[a][tid] = s ? word - 1u : 0u;
        if (s) seen |= 1u << a;
        if (__ballot(s)) wave_seen |= 1u << a;                // (wave-uniform)
    }
    gain_pair_sums(n, seen, wave_seen, s_q, s_acc, acc, tid, lane);
}
// the update behind k_gain_stats_from_samples; one workgroup of 256.  The same check decides: rejected = the accumulators are cleared (nothing was added), one
// rejected update is counted, gains and tables stay; otherwise k_gain_update.
__global__ void __launch_bounds__(256) k_gain_update_samples(GainTrackViews V, GainTrackTables W, GainSampleRects R, GainSampleBufs P, unsigned long long *__restrict__ acc,
                                                             double *__restrict__ state, int *__restrict__ counters, double lambda)
{
    __shared__ const unsigned *s_src[MS_MAX_VIEWS];
    if (gain_samples_resolve(V, R, P, s_src)) gain_update_body(V, W, acc, state, counters, lambda);
    else if (threadIdx.x == 0) counters[2] += 1;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * V.n * V.n; i += 256) acc[i] = 0ull;
}
// ms_gain_stats_from_samples: k_gain_export behind the same check; a rejected set reports zeros and is counted
__global__ void __launch_bounds__(256) k_gain_export_samples(GainTrackViews V, GainSampleRects R, GainSampleBufs P, unsigned long long *__restrict__ acc,
                                                             long long *__restrict__ outN, long long *__restrict__ outS, int *__restrict__ counters)
{
    __shared__ const unsigned *s_src[MS_MAX_VIEWS];
    const int n = V.n, nn = n * n, p = threadIdx.x;
    const bool good = gain_samples_resolve(V, R, P, s_src);
    if (p < nn) {
        if (good) gain_cell(V, acc, p / n, p % n, outN[p], outS[p]);
        else outN[p] = outS[p] = 0;
    }
    if (!good && p == 0) counters[2] += 1;
    __syncthreads();
    for (int i = p; i < 2 * nn; i += 256) acc[i] = 0ull;
}
}  // namespace

// VoronoiSeamFinder over DEVICE masks (contiguous, roi-sized), in place, pairs in the reference's order (PairwiseSeamFinder::run: i < j, overlapping rois)
int voronoi_seams_device(int n, const ms_rect *rois, uint8_t *const *masks, hipStream_t st)
{
    size_t cells = 0;
    for (int i = 0; i + 1 < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const int x0 = std::max(rois[i].x, rois[j].x), y0 = std::max(rois[i].y, rois[j].y);
            const int x1 = std::min(rois[i].x + rois[i].width, rois[j].x + rois[j].width), y1 = std::min(rois[i].y + rois[i].height, rois[j].y + rois[j].height);
            if (x0 < x1 && y0 < y1) cells = std::max(cells, (size_t)(x1 - x0 + 2 * VGAP) * (y1 - y0 + 2 * VGAP));
        }
    if (!cells) return MS_OK;
    int *d = nullptr;
    MS_HIP(hipMalloc((void **)&d, 2 * cells * sizeof(int)));
    int rc = MS_OK;
    for (int i = 0; i + 1 < n && rc == MS_OK; ++i)
        for (int j = i + 1; j < n && rc == MS_OK; ++j) {
            const int x0 = std::max(rois[i].x, rois[j].x), y0 = std::max(rois[i].y, rois[j].y);
            const int x1 = std::min(rois[i].x + rois[i].width, rois[j].x + rois[j].width), y1 = std::min(rois[i].y + rois[i].height, rois[j].y + rois[j].height);
            if (!(x0 < x1 && y0 < y1)) continue;
            const PairGeom g{x0, y0, x1 - x0, y1 - y0, rois[i].x, rois[i].y, rois[i].width, rois[i].height, rois[j].x, rois[j].y, rois[j].width, rois[j].height};
            const int C = g.rw + 2 * VGAP, R = g.rh + 2 * VGAP;
            k_vor_cols<<<div_up(C, 64), 64, 0, st>>>(masks[i], masks[j], g, d, d + cells);
            k_vor_rows<<<div_up(R, 64), 64, 0, st>>>(masks[i], masks[j], g, d, d + cells);
            if (hipGetLastError() != hipSuccess) rc = fail(MS_ERR_HIP, "voronoi_seams_device: launch failed");
        }
    if (hipStreamSynchronize(st) != hipSuccess && rc == MS_OK) rc = fail(MS_ERR_HIP, "voronoi_seams_device: sync failed");
    (void)hipFree(d);
    return rc;
}

// GainCompensator::feed over DEVICE images (8UC3, contiguous) and masks (8UC1, contiguous); gains come back to the host (n doubles)
int estimate_gains_device(int n, const ms_rect *rois, const uint8_t *const *images, const uint8_t *const *masks, double *gains_host, hipStream_t st, int *N_host, double *I_host)
{
    if (n > MS_MAX_VIEWS) return fail(MS_ERR_INVALID, "estimate_gains_device: too many views");
    GainViews V{};
    V.n = n;
    for (int i = 0; i < n; ++i) { V.img[i] = images[i]; V.mask[i] = masks[i]; V.roi[i] = rois[i]; }
    char *buf = nullptr;
    const size_t nn = (size_t)n * n, bytes = nn * sizeof(double) + nn * sizeof(int) + n * sizeof(double) + 16;
    MS_HIP(hipMalloc((void **)&buf, bytes));
    double *Im = (double *)buf, *g = Im + nn;
    int *Nm = (int *)(g + n), *ok = Nm + nn;
    int rc = MS_OK;
    if (hipMemsetAsync(buf, 0, bytes, st) != hipSuccess) rc = fail(MS_ERR_HIP, "estimate_gains_device: memset failed");
    if (rc == MS_OK) {
        k_gain_pairs<<<div_up((int)nn, 64), 64, 0, st>>>(V, Nm, Im);
        k_gain_solve<<<1, 1, 0, st>>>(n, Nm, Im, g, ok);
        int hok = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(gains_host, g, n * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(&hok, ok, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
            (N_host && hipMemcpyAsync(N_host, Nm, nn * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) ||
            (I_host && hipMemcpyAsync(I_host, Im, nn * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) || hipStreamSynchronize(st) != hipSuccess)
            rc = fail(MS_ERR_HIP, "estimate_gains_device: launch / copy failed");
        else if (!hok) rc = fail(MS_ERR_INVALID, "singular gain system");
    }
    (void)hipFree(buf);
    return rc;
}
}  // namespace ms

using namespace ms;

// ---- exposure tracking: ms_gain_stats / ms_track_gains / ms_get_gains and their sharded forms, beside the kernels they launch ---------------------------------------
static unsigned gain_window_reads(const ms_ctx *c, unsigned active)      // the active views whose warped ROI meets the window's columns
{
    const ms_rect T = c->bg.dst_roi_final;
    const bool windowed = c->col_end > c->col_begin;
    const int x0 = T.x + (windowed ? c->col_begin : 0), x1 = T.x + (windowed ? c->col_end : T.width);
    unsigned m = 0;
    for (int v = 0; v < c->N; ++v)
        if (((active >> v) & 1u) && c->roi[v].x < x1 && c->roi[v].x + c->roi[v].width > x0) m |= 1u << v;
    return m;
}
// the whole lattice of a stride, the views' ROIs and static maps, the active set -- without a call's checks (maps built, tables_mu held): what the sizes depend on
static void gain_geometry_fill(const ms_ctx *c, int stride, GainTrackViews &V)
{
    V = GainTrackViews{};
    V.n = c->N; V.src_w = c->cfg.src_width; V.src_h = c->cfg.src_height;
    V.active = c->act ? c->act->views : all_views(c->N);
    V.T = c->bg.dst_roi_final; V.stride = stride;
    V.nsx = div_up(V.T.width, stride); V.nsy = div_up(V.T.height, stride);
    for (int v = 0; v < c->N; ++v) {
        V.xmap[v] = (const float *)c->maps.p + c->map_off[v]; V.pitch[v] = c->map_pitch[v];
        V.roi[v] = c->roi[v];
    }
}
// What every entry point checks on its context, and the by-value kernel argument without frames (taken under tables_mu: the active set and the geometry cannot
// change meanwhile).  The caller states its sharding rule: view_shards / col_shards = a context sharded that way is served.  ms_gain_stats / ms_track_gains serve
// neither (a shard does not hold every overlap); the partial calls serve column shards, the sample calls view shards.  frames: the call reads `views`, refused here
// if null (gain_frames checks them one by one).  nv12: the views are the cameras' planes (8UC1, (src_height * 3 / 2) x src_width); the maps are all the statistic
// needs, so the tiled warp is not required.
static int gain_geometry(ms_ctx *c, const char *who, bool view_shards, bool col_shards, bool frames, const ms_image *views, int stride, bool nv12, GainTrackViews &V)
{
    if (!c->blender_ready) return fail(MS_ERR_STATE, "%s: call ms_init_blender first", who);
    const bool by_view = sharded_ctx(c) || c->cfg.view_shards > 1, by_col = c->cfg.col_shards > 1;
    if (!view_shards && !col_shards && (by_view || by_col))
        return fail(MS_ERR_UNSUPPORTED, "%s: not for a view- or column-sharded context (a shard does not hold every overlap); column shards track with ms_gain_stats_partial / ms_track_gains_from_partials", who);
    if (!col_shards && by_col) return fail(MS_ERR_UNSUPPORTED, "%s: not for a column-sharded context (column shards track with ms_gain_stats_partial / ms_track_gains_from_partials)", who);
    if (!view_shards && by_view) return fail(MS_ERR_UNSUPPORTED, "%s: not for a view-sharded context (a pair statistic needs both views' pixels at one sample; a view shard holds only its own)", who);
    if (c->feather_sharpness >= 0.f) return fail(MS_ERR_UNSUPPORTED, "%s: not for FeatherBlender contexts (ms_init_feather)", who);
    if (frames) MS_CHECK(views, "%s: null views", who);
    MS_CHECK(stride >= 1, "%s: stride %d < 1", who, stride);
    if (nv12) MS_CHECK((c->cfg.src_width & 1) == 0 && (c->cfg.src_height & 1) == 0, "%s: NV12 frames have an even size, the context's source size is %dx%d", who, c->cfg.src_width, c->cfg.src_height);
    gain_geometry_fill(c, stride, V);
    return MS_OK;
}
// this call's frames of the views in `reads`: a view left out, one no sample of the window lies in, or another shard's, is never read and not looked at
static int gain_frames(const char *who, const ms_image *views, unsigned reads, bool nv12, GainTrackViews &V)
{
    for (int v = 0; v < V.n; ++v) {
        if (!((reads >> v) & 1u)) continue;
        if (nv12)
            MS_CHECK(views[v].data && views[v].type == MS_8UC1 && views[v].rows == V.src_h * 3 / 2 && views[v].cols == V.src_w && views[v].step >= (size_t)V.src_w,
                     "%s: view %d must be the NV12 planes of a %dx%d frame (DEVICE 8UC1, %d rows)", who, v, V.src_w, V.src_h, V.src_h * 3 / 2);
        else
            MS_CHECK(views[v].data && views[v].type == MS_8UC3 && views[v].rows == V.src_h && views[v].cols == V.src_w && views[v].step >= (size_t)V.src_w * 3,
                     "%s: view %d must be a DEVICE 8UC3 image of %dx%d", who, v, V.src_w, V.src_h);
        V.src[v] = (const uint8_t *)views[v].data; V.step[v] = (unsigned)views[v].step;
    }
    return MS_OK;
}
// the header of a partial of V's rig, active set, stride and whole-ROI lattice (the same on every shard: before ms_gain_stats_partial narrows V to its window)
static GainPartialHeader gain_partial_header(const GainTrackViews &V)
{
    return GainPartialHeader{GAIN_PARTIAL_MAGIC, (unsigned)V.n, V.active, (unsigned)V.stride, V.T.x, V.T.y, V.T.width, V.T.height};
}
// the one check of ms_gain_track_params (dist.cpp has its own: it refuses before anything moves between ranks)
static int gain_params_check(const char *who, const ms_gain_track_params *prm)
{
    if (!prm) return fail(MS_ERR_INVALID, "%s: null params", who);
    MS_CHECK(prm->struct_size == sizeof(ms_gain_track_params), "%s: ms_gain_track_params.struct_size is %u, this library expects %zu", who, prm->struct_size, sizeof(ms_gain_track_params));
    MS_CHECK(prm->smoothing > 0.0 && prm->smoothing <= 1.0, "%s: smoothing %g outside (0, 1]", who, prm->smoothing);
    return MS_OK;
}
// every view table a later stitch may read (tables_mu held): the full set, its enqueue-only-mask-update copy, the cached subsets
static GainTrackTables gain_track_tables(ms_ctx *c)
{
    GainTrackTables W{};
    W.tab[W.n++] = (ViewDesc *)c->view_tab.p;
    if (c->alt.view_tab.p && (int)c->alt.h_views.size() == c->N) W.tab[W.n++] = (ViewDesc *)c->alt.view_tab.p;
    for (auto &T : c->subsets)
        if (T->view_tab.p && W.n < GAIN_TRACK_MAX_TABLES) W.tab[W.n++] = (ViewDesc *)T->view_tab.p;
    return W;
}
// The one enqueue of every call that uses the accumulators (B).  The caller holds tables_mu (lock order: tables_mu, gain_mu, mesh_mu), so the geometry and the table
// list it made stay valid until the kernels are in the stream; both locks are held for the enqueue only, never for a GPU wait.  `accumulate` adds this call's
// statistics (or nothing: the partials are summed by the update itself), `finish` exports or solves and leaves the accumulators cleared.  A call that publishes
// gains waits for the last stitch of another stream BETWEEN the two: the statistics overlap that stitch, only the update that rewrites its view tables runs behind it.
// N_host, S_host: the tail of both statistics calls, the exported block to the host.  It cannot be overwritten before it is read back: the next call waits for
// gain_ev, recorded behind the copies.  The caller synchronises once its locks are released.
template <typename Accumulate, typename Finish>
static int gain_enqueue(ms_ctx *c, hipStream_t st, bool publishes, Accumulate accumulate, Finish finish, long long *N_host = nullptr, long long *S_host = nullptr)
{
    GainTrackBuf *B = (GainTrackBuf *)c->gain_buf.p;
    std::lock_guard<std::mutex> gk(c->gain_mu);
    // the accumulators are shared by every call of the context: behind the last one, and behind whatever may still rewrite a view table
    if (c->gain_ev_set) MS_HIP(hipStreamWaitEvent(st, c->gain_ev, 0));
    if (c->subset_built_set) MS_HIP(hipStreamWaitEvent(st, c->subset_built, 0));
    { std::lock_guard<std::mutex> mk(c->mesh_mu); if (c->tab_wait) MS_HIP(hipStreamWaitEvent(st, c->tab_ready, 0)); }
    if (int e = accumulate(B)) return e;
    // a call that publishes gains: behind every stitch that may still read the view tables, when that stitch runs on another stream
    if (publishes && c->stitch_pending && c->last_stream_set && c->last_stream != st) MS_HIP(hipStreamWaitEvent(st, c->last_stitch, 0));
    if (int e = finish(B)) return e;
    if (N_host) {
        const size_t nn = (size_t)c->N * c->N;
        MS_HIP(hipMemcpyAsync(N_host, B->outN, nn * sizeof(long long), hipMemcpyDeviceToHost, st));
        MS_HIP(hipMemcpyAsync(S_host, B->outS, nn * sizeof(long long), hipMemcpyDeviceToHost, st));
    }
    MS_HIP(hipEventRecord(c->gain_ev, st));
    c->gain_ev_set = true;
    if (publishes) {      // ... and now that gain_ev is recorded behind it, the next stitch on another stream waits for that event
        c->gain_tracked = true;
        c->gain_pub_stream = st; c->gain_pub_pending = true;
    }
    return MS_OK;
}
static int launch_checked() { MS_LAUNCH_CHECK(); return MS_OK; }
// k_gain_stats over V's lattice, from 8UC3 frames or NV12 planes: what ms_gain_stats, ms_track_gains and ms_gain_stats_partial accumulate
static int gain_accumulate(const GainTrackViews &V, GainTrackBuf *B, bool nv12, hipStream_t st)
{
    if (V.nsx <= 0 || V.nsy <= 0) return MS_OK;
    const dim3 g(div_up(V.nsx, 64), div_up(V.nsy, 4)), b(64, 4);
    if (nv12) k_gain_stats<true><<<g, b, 0, st>>>(V, B->acc);
    else k_gain_stats<false><<<g, b, 0, st>>>(V, B->acc);
    return launch_checked();
}
// k_gain_stats' lattice walk from the shards' sample buffers: what ms_gain_stats_from_samples and ms_track_gains_from_samples accumulate
static int gain_accumulate_samples(const GainTrackViews &V, const GainSampleRects &R, const GainSampleBufs &P, GainTrackBuf *B, hipStream_t st)
{
    k_gain_stats_from_samples<<<dim3(div_up(V.nsx, 64), div_up(V.nsy, 4)), dim3(64, 4), 0, st>>>(V, R, P, B->acc);
    return launch_checked();
}

extern "C" {

int ms_gain_track_default_params(ms_gain_track_params *prm)
{
    if (!prm) return fail(MS_ERR_INVALID, "ms_gain_track_default_params: null argument");
    prm->struct_size = (unsigned)sizeof(ms_gain_track_params);
    prm->stride = 4;
    prm->smoothing = 0.25;
    return MS_OK;
}

// ms_gain_stats / ms_gain_stats_nv12: only the kernel that reads the pixels differs
static int gain_stats_impl(ms_ctx *c, const char *who, const ms_image *views, int stride, bool nv12, long long *N_host, long long *S_host, hipStream_t st)
{
    if (!c) return fail(MS_ERR_INVALID, "%s: null context", who);
    if (!N_host || !S_host) return fail(MS_ERR_INVALID, "%s: null output", who);
    {
        std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);
        GainTrackViews V;
        if (int e = gain_geometry(c, who, false, false, true, views, stride, nv12, V)) return e;
        if (int e = gain_frames(who, views, V.active, nv12, V)) return e;
        auto accumulate = [&](GainTrackBuf *B) { return gain_accumulate(V, B, nv12, st); };
        auto finish = [&](GainTrackBuf *B) {
            k_gain_export<<<1, 256, 0, st>>>(V, B->acc, B->outN, B->outS);
            return launch_checked();
        };
        if (int e = gain_enqueue(c, st, false, accumulate, finish, N_host, S_host)) return e;
    }
    MS_HIP(hipStreamSynchronize(st));
    return MS_OK;
}

// ms_track_gains / ms_track_gains_nv12: the same accumulators, solve, smoothing and publication; calls of either form may alternate on one context
static int track_gains_impl(ms_ctx *c, const char *who, const ms_image *views, const ms_gain_track_params *prm, bool nv12, hipStream_t st)
{
    if (!c) return fail(MS_ERR_INVALID, "%s: null context", who);
    if (int e = gain_params_check(who, prm)) return e;
    std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);
    GainTrackViews V;
    if (int e = gain_geometry(c, who, false, false, true, views, prm->stride, nv12, V)) return e;
    if (int e = gain_frames(who, views, V.active, nv12, V)) return e;
    const GainTrackTables W = gain_track_tables(c);
    auto accumulate = [&](GainTrackBuf *B) { return gain_accumulate(V, B, nv12, st); };
    auto finish = [&](GainTrackBuf *B) {
        k_gain_update<<<1, 256, 0, st>>>(V, W, B->acc, B->state, &B->solves_ok, prm->smoothing);
        return launch_checked();
    };
    return gain_enqueue(c, st, true, accumulate, finish);
}

int ms_gain_stats(ms_ctx *c, const ms_image *views, int stride, long long *N_host, long long *S_host, ms_stream stream)
{
    return gain_stats_impl(c, "ms_gain_stats", views, stride, false, N_host, S_host, as_stream(stream));
}
int ms_gain_stats_nv12(ms_ctx *c, const ms_image *views_nv12, int stride, long long *N_host, long long *S_host, ms_stream stream)
{
    return gain_stats_impl(c, "ms_gain_stats_nv12", views_nv12, stride, true, N_host, S_host, as_stream(stream));
}
int ms_track_gains(ms_ctx *c, const ms_image *views, const ms_gain_track_params *prm, ms_stream stream)
{
    return track_gains_impl(c, "ms_track_gains", views, prm, false, as_stream(stream));
}
int ms_track_gains_nv12(ms_ctx *c, const ms_image *views_nv12, const ms_gain_track_params *prm, ms_stream stream)
{
    return track_gains_impl(c, "ms_track_gains_nv12", views_nv12, prm, true, as_stream(stream));
}

int ms_get_gains(ms_ctx *c, double *gains_host, int *solves_ok, int *solves_singular, ms_stream stream)
{
    if (!c) return fail(MS_ERR_INVALID, "null context");
    if (!gains_host) return fail(MS_ERR_INVALID, "ms_get_gains: null output");
    if (!c->blender_ready || !c->gain_buf.p) return fail(MS_ERR_STATE, "ms_get_gains: call ms_init_blender first");
    hipStream_t st = as_stream(stream);
    bool wait;
    { std::lock_guard<std::mutex> gk(c->gain_mu); wait = c->gain_ev_set; }
    if (wait) MS_HIP(hipStreamWaitEvent(st, c->gain_ev, 0));      // (a track call on another stream)
    GainTrackBuf *B = (GainTrackBuf *)c->gain_buf.p;
    double g[MAX_VIEWS];
    int cnt[2];
    MS_HIP(hipMemcpyAsync(g, B->state, sizeof(g), hipMemcpyDeviceToHost, st));
    MS_HIP(hipMemcpyAsync(cnt, &B->solves_ok, sizeof(cnt), hipMemcpyDeviceToHost, st));
    MS_HIP(hipStreamSynchronize(st));
    std::lock_guard<std::mutex> gk(c->gain_mu);
    for (int v = 0; v < c->N; ++v) gains_host[v] = c->gain[v] = g[v];
    if (solves_ok) *solves_ok = cnt[0];
    if (solves_singular) *solves_singular = cnt[1];
    return MS_OK;
}

// ---- exposure tracking on column shards: partial statistics in caller-owned device memory, summed and solved on the device ---------------------------------------
size_t ms_gain_partial_bytes(const ms_ctx *c)
{
    if (!c) { (void)fail(MS_ERR_INVALID, "ms_gain_partial_bytes: null context"); return 0; }
    return gain_partial_bytes(c->N);
}

int ms_get_gain_views(const ms_ctx *cc, unsigned *mask)
{
    if (!mask) return fail(MS_ERR_INVALID, "ms_get_gain_views: null output");
    if (!cc) return fail(MS_ERR_INVALID, "ms_get_gain_views: null context");
    ms_ctx *c = const_cast<ms_ctx *>(cc);
    std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);
    GainTrackViews V;
    if (int e = gain_geometry(c, "ms_get_gain_views", false, true, false, nullptr, 1, false, V)) return e;
    *mask = gain_window_reads(c, V.active) | (c->own_mask & c->needed_mask & V.active);
    return MS_OK;
}

// ms_gain_stats_partial: the lattice columns of this context's column window (the whole ROI without column shards); only the views whose ROI meets those columns are checked and read
static int gain_partial_impl(ms_ctx *c, const char *who, const ms_image *views, int stride, bool nv12, void *partial, hipStream_t st)
{
    // (what does not depend on the context first: these checks run, and are tested, without a device)
    MS_CHECK(partial && ((uintptr_t)partial & 7u) == 0, "%s: the partial must be a DEVICE buffer of ms_gain_partial_bytes, 8-byte aligned", who);
    MS_CHECK(views, "%s: null views", who);
    MS_CHECK(stride >= 1, "%s: stride %d < 1", who, stride);
    if (!c) return fail(MS_ERR_INVALID, "%s: null context", who);
    std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);
    GainTrackViews V;
    if (int e = gain_geometry(c, who, false, true, true, views, stride, nv12, V)) return e;
    if (int e = gain_frames(who, views, gain_window_reads(c, V.active), nv12, V)) return e;
    const GainPartialHeader H = gain_partial_header(V);
    if (c->col_end > c->col_begin) {      // the samples with col_begin <= u - T.x < col_end: the lattice starts at the window's first sample column
        const int s0 = div_up(c->col_begin, stride), s1 = div_up(c->col_end, stride);
        V.T.x += s0 * stride; V.nsx = s1 - s0;
    }
    auto accumulate = [&](GainTrackBuf *B) { return gain_accumulate(V, B, nv12, st); };
    auto finish = [&](GainTrackBuf *B) {
        k_gain_partial_export<<<1, 256, 0, st>>>(V.n, H, B->acc, (unsigned *)partial);
        return launch_checked();
    };
    return gain_enqueue(c, st, false, accumulate, finish);
}
int ms_gain_stats_partial(ms_ctx *c, const ms_image *views, int stride, void *partial_dev, ms_stream stream)
{
    return gain_partial_impl(c, "ms_gain_stats_partial", views, stride, false, partial_dev, as_stream(stream));
}
int ms_gain_stats_partial_nv12(ms_ctx *c, const ms_image *views_nv12, int stride, void *partial_dev, ms_stream stream)
{
    return gain_partial_impl(c, "ms_gain_stats_partial_nv12", views_nv12, stride, true, partial_dev, as_stream(stream));
}

int ms_track_gains_from_partials(ms_ctx *c, const void *const *partials, int n_partials, const ms_gain_track_params *prm, ms_stream stream)
{
    const char *who = "ms_track_gains_from_partials";
    if (int e = gain_params_check(who, prm)) return e;
    MS_CHECK(partials, "%s: null partials", who);
    MS_CHECK(n_partials >= 1 && n_partials <= GAIN_MAX_PARTIALS, "%s: %d partials, not in [1, %d]", who, n_partials, GAIN_MAX_PARTIALS);
    GainPartials P{};
    P.n = n_partials;
    for (int k = 0; k < n_partials; ++k) {
        MS_CHECK(partials[k] && ((uintptr_t)partials[k] & 7u) == 0, "%s: partial %d is null or not 8-byte aligned", who, k);
        P.p[k] = (const unsigned long long *)partials[k];
    }
    MS_CHECK(prm->stride >= 1, "%s: stride %d < 1", who, prm->stride);
    if (!c) return fail(MS_ERR_INVALID, "%s: null context", who);
    hipStream_t st = as_stream(stream);
    std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);
    GainTrackViews V;
    if (int e = gain_geometry(c, who, false, true, false, nullptr, prm->stride, false, V)) return e;
    const GainPartialHeader H = gain_partial_header(V);
    const GainTrackTables W = gain_track_tables(c);
    // (the partials are the caller's: whatever wrote them is ordered before this call by the caller's stream)
    auto accumulate = [](GainTrackBuf *) { return MS_OK; };      // (the update sums the partials itself)
    auto finish = [&](GainTrackBuf *B) {
        k_gain_update_partials<<<1, 256, 0, st>>>(V, W, H, P, B->state, &B->solves_ok, prm->smoothing);
        return launch_checked();
    };
    return gain_enqueue(c, st, true, accumulate, finish);
}

// ---- exposure tracking on view shards: per-view sample vectors in caller-owned device memory, paired, summed and solved on the device -------------------------------
static unsigned view_shard_mask(int N, int S, int k)      // the block of views of shard k of S (ms_create)
{
    unsigned m = 0;
    for (int v = k * N / S; v < (k + 1) * N / S; ++v) m |= 1u << v;
    return m;
}
size_t ms_gain_samples_bytes(const ms_ctx *c, int stride, int view_shard_index)
{
    const char *who = "ms_gain_samples_bytes";
    if (!c) { (void)fail(MS_ERR_INVALID, "%s: null context", who); return 0; }
    if (stride < 1) { (void)fail(MS_ERR_INVALID, "%s: stride %d < 1", who, stride); return 0; }
    const int S = c->cfg.view_shards > 1 ? c->cfg.view_shards : 1;
    if (view_shard_index < -1 || view_shard_index >= S) { (void)fail(MS_ERR_INVALID, "%s: view shard %d of %d", who, view_shard_index, S); return 0; }
    if (!c->maps_built) { (void)fail(MS_ERR_STATE, "%s: call ms_build_maps first", who); return 0; }
    if (c->cfg.col_shards > 1 || c->feather_sharpness >= 0.f) { (void)fail(MS_ERR_UNSUPPORTED, "%s: not for column-sharded or FeatherBlender contexts", who); return 0; }
    std::lock_guard<std::recursive_mutex> tables_lk(const_cast<ms_ctx *>(c)->tables_mu);
    const unsigned own = view_shard_index < 0 ? c->own_mask & all_views(c->N) : view_shard_mask(c->N, S, view_shard_index);
    GainTrackViews V;
    gain_geometry_fill(c, stride, V);
    unsigned off[MS_MAX_VIEWS];
    const size_t words = gain_sample_offsets(V, gain_sample_rects(V), own & V.active, off);
    if (words > 0xffffffffu / 4u) { (void)fail(MS_ERR_INVALID, "%s: the buffer would exceed 4 GiB at stride %d; use a larger stride", who, stride); return 0; }
    return words * 4;
}

int ms_get_view_shard(const ms_ctx *c, int *view_shards, int *view_shard_index)
{
    if (!view_shards || !view_shard_index) return fail(MS_ERR_INVALID, "ms_get_view_shard: null output");
    if (!c) return fail(MS_ERR_INVALID, "ms_get_view_shard: null context");
    const bool sharded = c->cfg.view_shards > 1;
    *view_shards = sharded ? c->cfg.view_shards : 1;
    *view_shard_index = sharded ? c->cfg.view_shard_index : 0;
    return MS_OK;
}

int ms_get_gain_sample_views(const ms_ctx *cc, unsigned *mask)
{
    const char *who = "ms_get_gain_sample_views";
    if (!mask) return fail(MS_ERR_INVALID, "%s: null output", who);
    if (!cc) return fail(MS_ERR_INVALID, "%s: null context", who);
    ms_ctx *c = const_cast<ms_ctx *>(cc);
    std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);
    GainTrackViews V;
    if (int e = gain_geometry(c, who, true, false, false, nullptr, 1, false, V)) return e;
    *mask = V.active & c->own_mask;
    return MS_OK;
}

// ms_gain_samples: the whole lattice, the views this context owns.  The accumulators are not used: outside gain_enqueue, no gain_mu
static int gain_samples_impl(ms_ctx *c, const char *who, const ms_image *views, int stride, bool nv12, void *samples, hipStream_t st)
{
    // (what does not depend on the context first: these checks run, and are tested, without a device)
    MS_CHECK(samples && ((uintptr_t)samples & 3u) == 0, "%s: the samples must be a DEVICE buffer of ms_gain_samples_bytes, 4-byte aligned", who);
    MS_CHECK(views, "%s: null views", who);
    MS_CHECK(stride >= 1, "%s: stride %d < 1", who, stride);
    if (!c) return fail(MS_ERR_INVALID, "%s: null context", who);
    std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);      // for the enqueue only (as ms_track_gains)
    GainTrackViews V;
    if (int e = gain_geometry(c, who, true, false, true, views, stride, nv12, V)) return e;
    const unsigned held = V.active & c->own_mask;
    if (int e = gain_frames(who, views, held, nv12, V)) return e;
    const GainSampleRects R = gain_sample_rects(V);
    GainSampleOut O{};
    O.held = held;
    const size_t words = gain_sample_offsets(V, R, held, O.off);
    MS_CHECK(words <= 0xffffffffu / 4u, "%s: the buffer would exceed 4 GiB at stride %d; use a larger stride", who, stride);
    O.words = (unsigned)words;
    for (int v = 0; v < V.n; ++v) {
        if (!((held >> v) & 1u) || R.w[v] == 0 || R.h[v] == 0) continue;
        O.view[O.nheld] = (unsigned char)v;
        O.first[O.nheld + 1] = O.first[O.nheld] + (unsigned)div_up(R.w[v], 64) * (unsigned)div_up(R.h[v], 4);
        ++O.nheld;
    }
    const dim3 b(64, 4), g(std::max(1u, O.first[O.nheld]));
    if (nv12) k_gain_samples<true><<<g, b, 0, st>>>(V, R, O, (unsigned *)samples);
    else k_gain_samples<false><<<g, b, 0, st>>>(V, R, O, (unsigned *)samples);
    return launch_checked();
}
int ms_gain_samples(ms_ctx *c, const ms_image *views, int stride, void *samples_dev, ms_stream stream)
{
    return gain_samples_impl(c, "ms_gain_samples", views, stride, false, samples_dev, as_stream(stream));
}
int ms_gain_samples_nv12(ms_ctx *c, const ms_image *views_nv12, int stride, void *samples_dev, ms_stream stream)
{
    return gain_samples_impl(c, "ms_gain_samples_nv12", views_nv12, stride, true, samples_dev, as_stream(stream));
}

// the checks both consumers share; everything that needs no context first
static int gain_sample_bufs(const char *who, const void *const *samples, int n, int stride, GainSampleBufs &P)
{
    MS_CHECK(samples, "%s: null samples", who);
    MS_CHECK(n >= 1 && n <= GAIN_MAX_SAMPLE_BUFS, "%s: %d sample buffers, not in [1, %d]", who, n, GAIN_MAX_SAMPLE_BUFS);
    P = GainSampleBufs{};
    P.n = n;
    for (int k = 0; k < n; ++k) {
        MS_CHECK(samples[k] && ((uintptr_t)samples[k] & 3u) == 0, "%s: sample buffer %d is null or not 4-byte aligned", who, k);
        P.p[k] = (const unsigned *)samples[k];
    }
    MS_CHECK(stride >= 1, "%s: stride %d < 1", who, stride);
    return MS_OK;
}

int ms_gain_stats_from_samples(ms_ctx *c, const void *const *samples, int n, int stride, long long *N_host, long long *S_host, ms_stream stream)
{
    const char *who = "ms_gain_stats_from_samples";
    if (!N_host || !S_host) return fail(MS_ERR_INVALID, "%s: null output", who);
    GainSampleBufs P;
    if (int e = gain_sample_bufs(who, samples, n, stride, P)) return e;
    if (!c) return fail(MS_ERR_INVALID, "%s: null context", who);
    hipStream_t st = as_stream(stream);
    {   // (as ms_gain_stats)
        std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);
        GainTrackViews V;
        if (int e = gain_geometry(c, who, true, false, false, nullptr, stride, false, V)) return e;
        const GainSampleRects R = gain_sample_rects(V);
        auto accumulate = [&](GainTrackBuf *B) { return gain_accumulate_samples(V, R, P, B, st); };
        auto finish = [&](GainTrackBuf *B) {
            k_gain_export_samples<<<1, 256, 0, st>>>(V, R, P, B->acc, B->outN, B->outS, &B->solves_ok);
            return launch_checked();
        };
        if (int e = gain_enqueue(c, st, false, accumulate, finish, N_host, S_host)) return e;
    }
    MS_HIP(hipStreamSynchronize(st));
    return MS_OK;
}

int ms_track_gains_from_samples(ms_ctx *c, const void *const *samples, int n, const ms_gain_track_params *prm, ms_stream stream)
{
    const char *who = "ms_track_gains_from_samples";
    if (int e = gain_params_check(who, prm)) return e;
    GainSampleBufs P;
    if (int e = gain_sample_bufs(who, samples, n, prm->stride, P)) return e;
    if (!c) return fail(MS_ERR_INVALID, "%s: null context", who);
    hipStream_t st = as_stream(stream);
    std::lock_guard<std::recursive_mutex> tables_lk(c->tables_mu);
    GainTrackViews V;
    if (int e = gain_geometry(c, who, true, false, false, nullptr, prm->stride, false, V)) return e;
    const GainSampleRects R = gain_sample_rects(V);
    const GainTrackTables W = gain_track_tables(c);
    // (the buffers are the caller's: whatever wrote them is ordered before this call by the caller's stream)
    auto accumulate = [&](GainTrackBuf *B) { return gain_accumulate_samples(V, R, P, B, st); };
    auto finish = [&](GainTrackBuf *B) {
        k_gain_update_samples<<<1, 256, 0, st>>>(V, W, R, P, B->acc, B->state, &B->solves_ok, prm->smoothing);
        return launch_checked();
    };
    return gain_enqueue(c, st, true, accumulate, finish);
}

int ms_get_gain_track_counters(ms_ctx *c, ms_gain_track_counters *out, ms_stream stream)
{
    if (!out) return fail(MS_ERR_INVALID, "ms_get_gain_track_counters: null output");
    MS_CHECK(out->struct_size == sizeof(ms_gain_track_counters), "ms_get_gain_track_counters: ms_gain_track_counters.struct_size is %u, this library expects %zu", out->struct_size, sizeof(ms_gain_track_counters));
    if (!c) return fail(MS_ERR_INVALID, "ms_get_gain_track_counters: null context");
    if (!c->blender_ready || !c->gain_buf.p) return fail(MS_ERR_STATE, "ms_get_gain_track_counters: call ms_init_blender first");
    hipStream_t st = as_stream(stream);
    bool wait;
    { std::lock_guard<std::mutex> gk(c->gain_mu); wait = c->gain_ev_set; }
    if (wait) MS_HIP(hipStreamWaitEvent(st, c->gain_ev, 0));      // (a track call on another stream)
    int cnt[3];
    MS_HIP(hipMemcpyAsync(cnt, &((GainTrackBuf *)c->gain_buf.p)->solves_ok, sizeof(cnt), hipMemcpyDeviceToHost, st));
    MS_HIP(hipStreamSynchronize(st));
    out->solves_ok = cnt[0]; out->solves_singular = cnt[1]; out->updates_rejected = cnt[2];
    return MS_OK;
}

}  // extern "C"
