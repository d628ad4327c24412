// calib.hip -- calibration-time pixel work that the reference runs on the CPU, on the device:
//   VoronoiSeamFinder::findInPair       sources/modules/stitching/src/seam_finders.cpp:111-160
//       distanceTransform(DIST_L1, 3)   sources/modules/imgproc/src/distransform.cpp:70-137
//   GainCompensator::feed               sources/modules/stitching/src/exposure_compensate.cpp:71-145 (overlap sums, normal equations, cv::solve)
// so that ms_build_masks / ms_calibrate_seam move no pixels to the host: the only thing that comes back is the N gains.
//
// Exactness.  The reference's two-pass 3 x 3 chamfer with costs (1, 2) IS the city-block distance to the nearest zero pixel of the window
// (a diagonal step costs two axis steps), in 16.16 fixed point; here the same integers come from two separable 1-D passes (columns, then
// rows), which parallelise.  Where a window has no zero pixel at all the chamfer leaves INIT + 1 everywhere; the separable form leaves a
// large constant too, and the only use of the distances is `dist1 < dist2`, so the seam is the same.
// The gain sums are DOUBLE sums of square roots in raster order (exposure_compensate.cpp:103-117): order matters for the last bit, so one
// thread per image pair walks its overlap in that order (the overlaps are seam-scale images: a few thousand pixels); the n x n solve follows
// cv::solve's closed forms / LU (as the host version did) in a single thread.
#include <vector>
#include "common.hpp"
#include "launchers.hpp"
#include "descs.hpp"

namespace ms {
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
// k_gain_stats over the lattice columns of this context's window IS the partial statistic: the launcher hands it a lattice whose origin is the window's first
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
// every lattice sample of the view's rectangle R_v (launchers.hpp).  k_gain_samples: a lane owns one sample of one held view, lanes along sx, so a wave stores
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

// ---- exposure tracking: the launches ms_gain_stats / ms_track_gains enqueue (compositor.hip owns the buffers and the ordering) --------------------
int launch_gain_stats(const GainTrackViews &V, GainTrackBuf *buf, bool nv12, hipStream_t st)
{
    if (V.nsx <= 0 || V.nsy <= 0) return MS_OK;
    const dim3 g(div_up(V.nsx, 64), div_up(V.nsy, 4)), b(64, 4);
    if (nv12) k_gain_stats<true><<<g, b, 0, st>>>(V, buf->acc);
    else k_gain_stats<false><<<g, b, 0, st>>>(V, buf->acc);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
int launch_gain_export(const GainTrackViews &V, GainTrackBuf *buf, hipStream_t st)
{
    k_gain_export<<<1, 256, 0, st>>>(V, buf->acc, buf->outN, buf->outS);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
int launch_gain_update(const GainTrackViews &V, const GainTrackTables &W, GainTrackBuf *buf, double lambda, hipStream_t st)
{
    k_gain_update<<<1, 256, 0, st>>>(V, W, buf->acc, buf->state, &buf->solves_ok, lambda);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
int launch_gain_partial_export(const GainTrackViews &V, const GainPartialHeader &H, GainTrackBuf *buf, void *partial, hipStream_t st)
{
    k_gain_partial_export<<<1, 256, 0, st>>>(V.n, H, buf->acc, (unsigned *)partial);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
int launch_gain_update_partials(const GainTrackViews &V, const GainTrackTables &W, const GainPartialHeader &H, const GainPartials &P, GainTrackBuf *buf, double lambda, hipStream_t st)
{
    k_gain_update_partials<<<1, 256, 0, st>>>(V, W, H, P, buf->state, &buf->solves_ok, lambda);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

int launch_gain_samples(const GainTrackViews &V, const GainSampleRects &R, unsigned held, bool nv12, void *samples, hipStream_t st)
{
    GainSampleOut O{};
    O.held = held;
    O.words = (unsigned)gain_sample_offsets(V, R, held, O.off);
    for (int v = 0; v < V.n; ++v) {
        if (!((held >> v) & 1u) || R.w[v] == 0 || R.h[v] == 0) continue;
        O.view[O.nheld] = (unsigned char)v;
        O.first[O.nheld + 1] = O.first[O.nheld] + (unsigned)div_up(R.w[v], 64) * (unsigned)div_up(R.h[v], 4);
        ++O.nheld;
    }
    dim3 b(64, 4), g(std::max(1u, O.first[O.nheld]));
    if (nv12) k_gain_samples<true><<<g, b, 0, st>>>(V, R, O, (unsigned *)samples);
    else k_gain_samples<false><<<g, b, 0, st>>>(V, R, O, (unsigned *)samples);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
int launch_gain_stats_from_samples(const GainTrackViews &V, const GainSampleRects &R, const GainSampleBufs &P, GainTrackBuf *buf, hipStream_t st)
{
    dim3 b(64, 4), g(div_up(V.nsx, 64), div_up(V.nsy, 4));
    k_gain_stats_from_samples<<<g, b, 0, st>>>(V, R, P, buf->acc);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
int launch_gain_update_samples(const GainTrackViews &V, const GainTrackTables &W, const GainSampleRects &R, const GainSampleBufs &P, GainTrackBuf *buf, double lambda, hipStream_t st)
{
    k_gain_update_samples<<<1, 256, 0, st>>>(V, W, R, P, buf->acc, buf->state, &buf->solves_ok, lambda);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
int launch_gain_export_samples(const GainTrackViews &V, const GainSampleRects &R, const GainSampleBufs &P, GainTrackBuf *buf, hipStream_t st)
{
    k_gain_export_samples<<<1, 256, 0, st>>>(V, R, P, buf->acc, buf->outN, buf->outS, &buf->solves_ok);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
}  // namespace ms
