// rig.hip -- rig rotations from feature matches: the ray bundle adjustment of include/ms_stitch.h ("Rig rotation refinement"), kernels and entry points in one unit.
// Replaces detail::BundleAdjusterRay (OCV/stitching/src/motion_estimators.cpp:514-700) with the focals held.  Calibration-time work: the per-frame path never runs
// anything of this unit.  Everything is double; -ffp-contract=off keeps every product and sum of the per-match terms a separate IEEE operation, in the order the
// header states, so two implementations of the contract differ by the ORDER of their sums only.
//   k_rig_accum   one workgroup per view pair: the 28 sums of the pair (cost, g_i, g_j, H_ii, H_jj, H_ij) plus its outlier count
//   k_rig_step    one workgroup: assembles the system in pair order, accepts or rejects the trial, moves lambda, Cholesky in LDS, writes the next trial rotations
// A refinement is max_iters + 1 rounds of the two, enqueued at once; both return at their first instruction once the stop flag is set (the mesh solver's max_it
// launches work the same way).  No floating-point atomics: every sum has one fixed order, so a call's result does not depend on scheduling.
#include <algorithm>
#include <cmath>
#include <vector>
#include "ctx.hpp"
#include "lens.hpp"

namespace ms {

constexpr int RIG_DIM = 3 * MS_MAX_VIEWS;     // rows of the normal matrix over all views
constexpr int RIG_SUMS = 29;                  // cost | g_i | g_j | H_ii (xx xy xz yy yz zz) | H_jj | H_ij (row-major) | outliers
constexpr int RIG_PART = 32;                  // doubles per pair in the partials array
constexpr int RIG_MAX_MATCHES = 1 << 20;
constexpr int RIG_STEP_THREADS = 256;         // k_rig_step's one workgroup

struct RigPair { int i, j, off, cnt; };       // views i < j, the pair's matches are rays[off .. off + cnt)
struct RigRay { double a[3], b[3]; };         // a seen by view i, b by view j

// device-resident state of one refinement: nothing of it is read by the host before the last round has run
struct RigState {
    double R_cur[MS_MAX_VIEWS * 9];           // the last accepted rotations
    double R_trial[MS_MAX_VIEWS * 9];         // what k_rig_accum evaluates
    double H[RIG_DIM * RIG_DIM], g[RIG_DIM];  // the system at R_cur
    double lam, cost, cost0, dmax, outliers;
    int round, iters, stop, reason;
};

struct RigStepPrm { int n_views, anchor, max_iters, assemble_only; double step_tol; };

// ---- k_rig_accum --------------------------------------------------------------------------------------------------------------------------------
// The terms of one match, added into acc in the header's order.  h == 0: plain least squares.
__device__ __forceinline__ void rig_terms(const double *Ri, const double *Rj, const RigRay &m, double h, double acc[RIG_SUMS])
{
    const double p0 = Ri[0] * m.a[0] + Ri[1] * m.a[1] + Ri[2] * m.a[2], p1 = Ri[3] * m.a[0] + Ri[4] * m.a[1] + Ri[5] * m.a[2], p2 = Ri[6] * m.a[0] + Ri[7] * m.a[1] + Ri[8] * m.a[2];
    const double q0 = Rj[0] * m.b[0] + Rj[1] * m.b[1] + Rj[2] * m.b[2], q1 = Rj[3] * m.b[0] + Rj[4] * m.b[1] + Rj[5] * m.b[2], q2 = Rj[6] * m.b[0] + Rj[7] * m.b[1] + Rj[8] * m.b[2];
    const double r0 = p0 - q0, r1 = p1 - q1, r2 = p2 - q2;
    const double s2 = r0 * r0 + r1 * r1 + r2 * r2;
    double w = 1.0, rho = s2, out = 0.0;
    if (h > 0.0) {
        const double s = sqrt(s2);
        if (s > h) { w = h / s; rho = (2.0 * h) * s - h * h; out = 1.0; }
    }
    acc[0] += rho;
    acc[1] += w * (p1 * r2 - p2 * r1); acc[2] += w * (p2 * r0 - p0 * r2); acc[3] += w * (p0 * r1 - p1 * r0);               // g_i = w p x r
    acc[4] += -(w * (q1 * r2 - q2 * r1)); acc[5] += -(w * (q2 * r0 - q0 * r2)); acc[6] += -(w * (q0 * r1 - q1 * r0));      // g_j = -w q x r
    acc[7] += w * (p1 * p1 + p2 * p2); acc[8] += -(w * (p0 * p1)); acc[9] += -(w * (p0 * p2));                              // H_ii = w [p]x^T [p]x
    acc[10] += w * (p0 * p0 + p2 * p2); acc[11] += -(w * (p1 * p2)); acc[12] += w * (p0 * p0 + p1 * p1);
    acc[13] += w * (q1 * q1 + q2 * q2); acc[14] += -(w * (q0 * q1)); acc[15] += -(w * (q0 * q2));                           // H_jj = w [q]x^T [q]x
    acc[16] += w * (q0 * q0 + q2 * q2); acc[17] += -(w * (q1 * q2)); acc[18] += w * (q0 * q0 + q1 * q1);
    acc[19] += -(w * (p1 * q1 + p2 * q2)); acc[20] += w * (q0 * p1); acc[21] += w * (q0 * p2);                              // H_ij = w [p]x [q]x = w (q p^T - (p.q) I)
    acc[22] += w * (q1 * p0); acc[23] += -(w * (p0 * q0 + p2 * q2)); acc[24] += w * (q1 * p2);
    acc[25] += w * (q2 * p0); acc[26] += w * (q2 * p1); acc[27] += -(w * (p0 * q0 + p1 * q1));
    acc[28] += out;
}

// One 256-thread workgroup per used pair.  A thread sums the matches t, t + 256, ... in index order into registers; the 64 lanes of a wave are folded by a
// butterfly of fixed shape (lane ^ 32, ^ 16, ... ^ 1: every lane ends with the same bits), the four waves through LDS in wave order; RIG_SUMS lanes store.
__global__ void __launch_bounds__(256) k_rig_accum(const RigState *__restrict__ st, const RigPair *__restrict__ pairs, const RigRay *__restrict__ rays, double h,
                                                   double *__restrict__ part)
{
    __shared__ double s_sum[4][RIG_PART];
    if (st->stop) return;
    const RigPair pr = pairs[blockIdx.x];
    double Ri[9], Rj[9], acc[RIG_SUMS];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ri[k] = st->R_trial[pr.i * 9 + k]; Rj[k] = st->R_trial[pr.j * 9 + k]; }
#pragma unroll
    for (int e = 0; e < RIG_SUMS; ++e) acc[e] = 0.0;
    for (int k = threadIdx.x; k < pr.cnt; k += 256) rig_terms(Ri, Rj, rays[pr.off + k], h, acc);
#pragma unroll
    for (int e = 0; e < RIG_SUMS; ++e)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[e] += __shfl_xor(acc[e], d, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < RIG_SUMS; ++e) s_sum[wave][e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < RIG_SUMS) {
        const int e = threadIdx.x;
        part[(size_t)blockIdx.x * RIG_PART + e] = ((s_sum[0][e] + s_sum[1][e]) + s_sum[2][e]) + s_sum[3][e];
    }
}

// ---- k_rig_step ---------------------------------------------------------------------------------------------------------------------------------
// R <- Exp(d) R, Exp by the Rodrigues formula with 1 - cos t = 2 sin^2(t / 2)
__device__ void rig_rotate(const double *d, const double *R, double *out)
{
    const double t = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(t > 0.0)) { for (int k = 0; k < 9; ++k) out[k] = R[k]; return; }
    const double kx = d[0] / t, ky = d[1] / t, kz = d[2] / t, s = sin(t), sh = sin(0.5 * t), c1 = 2.0 * sh * sh;
    const double E[9] = {1.0 - c1 * (ky * ky + kz * kz), -s * kz + c1 * kx * ky, s * ky + c1 * kx * kz,
                         s * kz + c1 * kx * ky, 1.0 - c1 * (kx * kx + kz * kz), -s * kx + c1 * ky * kz,
                         -s * ky + c1 * kx * kz, s * kx + c1 * ky * kz, 1.0 - c1 * (kx * kx + ky * ky)};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[r * 3 + c] = E[r * 3] * R[c] + E[r * 3 + 1] * R[3 + c] + E[r * 3 + 2] * R[6 + c];
}

// where the 6 stored entries of a symmetric 3 x 3 block go
__device__ __constant__ int c_rig_sym_r[6] = {0, 0, 0, 1, 1, 2}, c_rig_sym_c[6] = {0, 1, 2, 1, 2, 2};

// One workgroup of RIG_STEP_THREADS lanes.  Rounds: round 0 takes the system at R_in and proposes the first trial; every later round judges the trial k_rig_accum has just
// evaluated.  prm.assemble_only: store the assembled cost / H / g and return (ms_rig_accumulate).
__global__ void __launch_bounds__(RIG_STEP_THREADS) k_rig_step(RigState *__restrict__ st, const RigPair *__restrict__ pairs, int n_pairs, const double *__restrict__ part, RigStepPrm prm)
{
    __shared__ double Hs[RIG_DIM * RIG_DIM], A[RIG_DIM * RIG_DIM], gs[RIG_DIM], xs[RIG_DIM];
    __shared__ double s_cost, s_outl, s_lam;
    __shared__ int s_accept, s_stop, s_reason, s_iters, s_ok;
    if (st->stop) return;
    const int tid = threadIdx.x, nv = prm.n_views;
    for (int k = tid; k < RIG_DIM * RIG_DIM; k += RIG_STEP_THREADS) Hs[k] = 0.0;
    if (tid < RIG_DIM) gs[tid] = 0.0;
    __syncthreads();
    // the system, pair after pair: inside a pair every sum goes to a place of its own
    for (int p = 0; p < n_pairs; ++p) {
        if (tid >= 1 && tid < 28) {
            const double v = part[(size_t)p * RIG_PART + tid];
            const int i3 = 3 * pairs[p].i, j3 = 3 * pairs[p].j;
            if (tid < 4) gs[i3 + tid - 1] += v;
            else if (tid < 7) gs[j3 + tid - 4] += v;
            else if (tid < 19) {
                const int b3 = tid < 13 ? i3 : j3, k = tid < 13 ? tid - 7 : tid - 13, r = c_rig_sym_r[k], c = c_rig_sym_c[k];
                Hs[(b3 + r) * RIG_DIM + b3 + c] += v;
                if (r != c) Hs[(b3 + c) * RIG_DIM + b3 + r] += v;
            } else {
                const int k = tid - 19, r = k / 3, c = k % 3;
                Hs[(i3 + r) * RIG_DIM + j3 + c] += v;
                Hs[(j3 + c) * RIG_DIM + i3 + r] += v;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double cost = 0.0, outl = 0.0;
        for (int p = 0; p < n_pairs; ++p) { cost += part[(size_t)p * RIG_PART]; outl += part[(size_t)p * RIG_PART + 28]; }
        s_cost = cost; s_outl = outl;
    }
    __syncthreads();
    if (prm.assemble_only) {
        for (int k = tid; k < RIG_DIM * RIG_DIM; k += RIG_STEP_THREADS) st->H[k] = Hs[k];
        if (tid < RIG_DIM) st->g[tid] = gs[tid];
        if (tid == 0) st->cost = s_cost;
        return;
    }
    // accept or reject, lambda, the stop rules
    if (tid == 0) {
        double lam = st->lam;
        int iters = st->iters, accept = 1, stop = 0, reason = 0;
        if (st->round == 0) st->cost0 = s_cost;
        else {
            accept = s_cost <= st->cost ? 1 : 0;      // (a NaN cost is a rejected step)
            ++iters;
            if (accept) { lam = fmax(lam / 10.0, 1e-12); if (st->dmax < prm.step_tol) { stop = 1; reason = MS_RIG_CONVERGED; } }
            else { lam = 10.0 * lam; if (lam > 1e12) { stop = 1; reason = MS_RIG_STALLED; } }
            if (!stop && iters >= prm.max_iters) { stop = 1; reason = MS_RIG_ITERATION_LIMIT; }
        }
        if (accept) { st->cost = s_cost; st->outliers = s_outl; }
        s_accept = accept; s_stop = stop; s_reason = reason; s_lam = lam; s_iters = iters;
    }
    __syncthreads();
    if (s_accept) {
        for (int k = tid; k < nv * 9; k += RIG_STEP_THREADS) st->R_cur[k] = st->R_trial[k];
        for (int k = tid; k < RIG_DIM * RIG_DIM; k += RIG_STEP_THREADS) st->H[k] = Hs[k];
        if (tid < RIG_DIM) st->g[tid] = gs[tid];
    } else {
        for (int k = tid; k < RIG_DIM * RIG_DIM; k += RIG_STEP_THREADS) Hs[k] = st->H[k];
        if (tid < RIG_DIM) gs[tid] = st->g[tid];
    }
    __syncthreads();
    // (H + lambda diag H) d = -g over the views but the anchor; a pivot that is not positive is a rejected step
    const int m = 3 * (nv - 1), a3 = 3 * prm.anchor;
    while (!s_stop) {
        const double lam = s_lam;
        for (int k = tid; k < m * m; k += RIG_STEP_THREADS) {
            const int r = k / m, c = k % m, fr = r + (r >= a3 ? 3 : 0), fc = c + (c >= a3 ? 3 : 0);
            const double hv = Hs[fr * RIG_DIM + fc];
            A[r * RIG_DIM + c] = r == c ? hv + lam * hv : hv;
        }
        if (tid == 0) s_ok = 1;
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            if (tid == 0) { const double d = A[k * RIG_DIM + k]; if (d > 0.0 && d < HUGE_VAL) A[k * RIG_DIM + k] = sqrt(d); else s_ok = 0; }
            __syncthreads();
            if (!s_ok) break;
            const double piv = A[k * RIG_DIM + k];
            for (int i = k + 1 + tid; i < m; i += RIG_STEP_THREADS) A[i * RIG_DIM + k] /= piv;
            __syncthreads();
            const int t = m - k - 1;                // the trailing t x t block, one element a lane and pass (lower triangle only)
            for (int e = tid; e < t * t; e += RIG_STEP_THREADS) {
                const int i = k + 1 + e / t, j = k + 1 + e % t;
                if (j <= i) A[i * RIG_DIM + j] -= A[i * RIG_DIM + k] * A[j * RIG_DIM + k];
            }
            __syncthreads();
        }
        if (s_ok) {
            // L y = -g, then L^T d = y: column by column, the pivot lane divides and every row still open subtracts the column's share
            if (tid < m) xs[tid] = -gs[tid + (tid >= a3 ? 3 : 0)];
            __syncthreads();
            for (int c = 0; c < m; ++c) {
                if (tid == 0) xs[c] /= A[c * RIG_DIM + c];
                __syncthreads();
                if (tid > c && tid < m) xs[tid] -= A[tid * RIG_DIM + c] * xs[c];
                __syncthreads();
            }
            for (int c = m - 1; c >= 0; --c) {
                if (tid == 0) xs[c] /= A[c * RIG_DIM + c];
                __syncthreads();
                if (tid < c) xs[tid] -= A[c * RIG_DIM + tid] * xs[c];
                __syncthreads();
            }
            if (tid == 0) {
                double dmax = 0.0;
                for (int r = 0; r < m; ++r) { dmax = fmax(dmax, fabs(xs[r])); if (!(fabs(xs[r]) < HUGE_VAL)) s_ok = 0; }
                st->dmax = dmax;
            }
        }
        __syncthreads();
        if (s_ok) break;
        if (tid == 0) {
            s_lam = 10.0 * s_lam; ++s_iters;
            if (s_lam > 1e12) { s_stop = 1; s_reason = MS_RIG_STALLED; }
            else if (s_iters >= prm.max_iters) { s_stop = 1; s_reason = MS_RIG_ITERATION_LIMIT; }
        }
        __syncthreads();
    }
    if (!s_stop && tid < nv) {
        if (tid == prm.anchor) { for (int k = 0; k < 9; ++k) st->R_trial[tid * 9 + k] = st->R_cur[tid * 9 + k]; }
        else rig_rotate(&xs[3 * (tid - (tid > prm.anchor ? 1 : 0))], &st->R_cur[tid * 9], &st->R_trial[tid * 9]);
    }
    if (tid == 0) { st->lam = s_lam; st->iters = s_iters; st->reason = s_reason; st->stop = s_stop; st->round = st->round + 1; }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
// the warper's backward direction of absolute warper coordinates, turned into the camera by R^T (R^-1 = R^T) and normalised
static void warper_ray(int proj, double scale, const float *t, const double *R, double u, double v, double *out)
{
    const double up = u / scale, vp = v / scale;
    double dx, dy, dz;
    if (proj == MS_PROJ_SPHERICAL) { const double sv = sin(LENS_PI - vp); dx = sv * sin(up); dy = cos(LENS_PI - vp); dz = sv * cos(up); }
    else if (proj == MS_PROJ_CYLINDRICAL) { dx = sin(up); dy = vp; dz = cos(up); }
    else { dx = up - (t ? (double)t[0] : 0.0); dy = vp - (t ? (double)t[1] : 0.0); dz = 1.0 - (t ? (double)t[2] : 0.0); }
    const double X = R[0] * dx + R[3] * dy + R[6] * dz, Y = R[1] * dx + R[4] * dy + R[7] * dz, Z = R[2] * dx + R[5] * dy + R[8] * dz;
    const double n = sqrt(X * X + Y * Y + Z * Z);
    out[0] = X / n; out[1] = Y / n; out[2] = Z / n;
}

static bool rig_unit(const double *r)
{
    const double n = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    return std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]) && std::fabs(n - 1.0) <= 1e-6;
}

static int rig_check_matches(const char *fn, int n_views, const double *R, const ms_rig_match *matches, int n)
{
    MS_CHECK(n_views >= 2 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d outside [2, %d]", fn, n_views, MS_MAX_VIEWS);
    MS_CHECK(R && matches, "%s: null argument", fn);
    MS_CHECK(n >= 1 && n <= RIG_MAX_MATCHES, "%s: %d matches outside [1, %d]", fn, n, RIG_MAX_MATCHES);
    for (int k = 0; k < n_views * 9; ++k) MS_CHECK(std::isfinite(R[k]), "%s: rotation of view %d is not finite", fn, k / 9);
    for (int k = 0; k < n; ++k) {
        const ms_rig_match &m = matches[k];
        MS_CHECK(m.view_a >= 0 && m.view_a < n_views && m.view_b >= 0 && m.view_b < n_views, "%s: match %d names views %d, %d outside [0, %d)", fn, k, m.view_a, m.view_b, n_views);
        MS_CHECK(m.view_a != m.view_b, "%s: match %d pairs view %d with itself", fn, k, m.view_a);
        MS_CHECK(rig_unit(m.a) && rig_unit(m.b), "%s: match %d: a ray is not finite or its length is off 1 by more than 1e-6", fn, k);
    }
    return MS_OK;
}

// Matches grouped by canonical pair (i < j, a and b swapped where the caller listed (j, i)), pairs in (i, j) order, input order kept inside a pair.  A pair with fewer
// than min_pair matches is left out and counted.
struct RigGroups { std::vector<RigPair> pairs; std::vector<RigRay> rays; int ignored = 0; };
static RigGroups rig_group(int n_views, const ms_rig_match *matches, int n, int min_pair)
{
    std::vector<int> cnt(n_views * n_views, 0), slot(n_views * n_views, -1);
    auto key = [&](const ms_rig_match &m) { return std::min(m.view_a, m.view_b) * n_views + std::max(m.view_a, m.view_b); };
    for (int k = 0; k < n; ++k) ++cnt[key(matches[k])];
    RigGroups G;
    int off = 0;
    for (int q = 0; q < n_views * n_views; ++q) {
        if (!cnt[q]) continue;
        if (cnt[q] < min_pair) { ++G.ignored; continue; }
        slot[q] = (int)G.pairs.size();
        G.pairs.push_back(RigPair{q / n_views, q % n_views, off, 0});
        off += cnt[q];
    }
    G.rays.resize(off);
    for (int k = 0; k < n; ++k) {
        const ms_rig_match &m = matches[k];
        const int s = slot[key(m)];
        if (s < 0) continue;
        RigPair &p = G.pairs[s];
        RigRay &r = G.rays[p.off + p.cnt++];
        const bool swap = m.view_a > m.view_b;
        for (int c = 0; c < 3; ++c) { r.a[c] = swap ? m.b[c] : m.a[c]; r.b[c] = swap ? m.a[c] : m.b[c]; }
    }
    return G;
}

// One device block, state | pairs | rays | partials (all 8-byte aligned): the first three are laid out in pinned memory and go up in ONE copy.
struct RigDevice { RigState *st; RigPair *pairs; RigRay *rays; double *part; };
static int rig_upload(const char *fn, const RigGroups &G, int n_views, const double *R, RigDevice &D, hipStream_t s)
{
    const size_t np = G.pairs.size(), o_pairs = sizeof(RigState), o_rays = o_pairs + np * sizeof(RigPair), o_part = o_rays + G.rays.size() * sizeof(RigRay),
                 total = o_part + np * RIG_PART * sizeof(double);
    char *base = (char *)device_scratch().get(total), *host = (char *)pinned_scratch().get(o_part);
    if (!base || !host) return fail(MS_ERR_NOMEM, "%s: no memory for %zu bytes", fn, total);
    D.st = (RigState *)base; D.pairs = (RigPair *)(base + o_pairs); D.rays = (RigRay *)(base + o_rays); D.part = (double *)(base + o_part);
    RigState *st = (RigState *)host;
    memset(st, 0, sizeof(RigState));
    memcpy(st->R_cur, R, sizeof(double) * 9 * n_views);
    memcpy(st->R_trial, R, sizeof(double) * 9 * n_views);
    st->lam = 1e-3;
    memcpy(host + o_pairs, G.pairs.data(), np * sizeof(RigPair));
    memcpy(host + o_rays, G.rays.data(), G.rays.size() * sizeof(RigRay));
    MS_HIP(hipMemcpyAsync(base, host, o_part, hipMemcpyHostToDevice, s));
    return MS_OK;
}

static double rig_angle(const double *A, const double *B)      // the angle of A B^T
{
    double M[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[r * 3 + c] = A[r * 3] * B[c * 3] + A[r * 3 + 1] * B[c * 3 + 1] + A[r * 3 + 2] * B[c * 3 + 2];
    const double x = M[7] - M[5], y = M[2] - M[6], z = M[3] - M[1];
    return atan2(0.5 * sqrt(x * x + y * y + z * z), 0.5 * (M[0] + M[4] + M[8] - 1.0));
}

static int rig_check_params(const char *fn, int n_views, const ms_rig_refine_params *prm)
{
    MS_CHECK(prm, "%s: null params", fn);
    MS_CHECK(prm->struct_size == sizeof(ms_rig_refine_params), "%s: params.struct_size %u, this library's ms_rig_refine_params has %zu bytes", fn, prm->struct_size,
             sizeof(ms_rig_refine_params));
    MS_CHECK(prm->anchor_view >= 0 && prm->anchor_view < n_views, "%s: anchor_view %d outside [0, %d)", fn, prm->anchor_view, n_views);
    MS_CHECK(prm->huber_rad >= 0.0 && std::isfinite(prm->huber_rad), "%s: huber_rad %g must be finite and not negative", fn, prm->huber_rad);
    MS_CHECK(prm->max_iters >= 1 && prm->max_iters <= 1000, "%s: max_iters %d outside [1, 1000]", fn, prm->max_iters);
    MS_CHECK(prm->step_tol >= 0.0 && std::isfinite(prm->step_tol), "%s: step_tol %g must be finite and not negative", fn, prm->step_tol);
    MS_CHECK(prm->min_pair_matches >= 1, "%s: min_pair_matches %d must be at least 1", fn, prm->min_pair_matches);
    return MS_OK;
}

// everything ms_refine_rig_rotations does; fn names the entry point in messages
static int rig_refine(const char *fn, int n_views, const double *R_in, const ms_rig_match *matches, int n, const ms_rig_refine_params *prm, double *R_out,
                      ms_rig_refine_info *info, hipStream_t s)
{
    if (int e = rig_check_matches(fn, n_views, R_in, matches, n)) return e;
    MS_CHECK(R_out, "%s: null R_out", fn);
    if (int e = rig_check_params(fn, n_views, prm)) return e;
    const RigGroups G = rig_group(n_views, matches, n, prm->min_pair_matches);
    // every view must hang on the anchor through used pairs
    std::vector<char> seen(n_views, 0);
    std::vector<int> todo{prm->anchor_view};
    seen[prm->anchor_view] = 1;
    while (!todo.empty()) {
        const int v = todo.back(); todo.pop_back();
        for (const RigPair &p : G.pairs) {
            const int o = p.i == v ? p.j : p.j == v ? p.i : -1;
            if (o >= 0 && !seen[o]) { seen[o] = 1; todo.push_back(o); }
        }
    }
    for (int v = 0; v < n_views; ++v)
        MS_CHECK(seen[v], "%s: view %d is not connected to the anchor view %d by pairs of at least %d matches (%d pairs ignored)", fn, v, prm->anchor_view,
                 prm->min_pair_matches, G.ignored);
    if (int e = require_device()) return e;

    RigDevice D;
    if (int e = rig_upload(fn, G, n_views, R_in, D, s)) return e;
    const RigStepPrm sp{n_views, prm->anchor_view, prm->max_iters, 0, prm->step_tol};
    const int np = (int)G.pairs.size();
    for (int round = 0; round <= prm->max_iters; ++round) {
        k_rig_accum<<<np, 256, 0, s>>>(D.st, D.pairs, D.rays, prm->huber_rad, D.part);
        k_rig_step<<<1, RIG_STEP_THREADS, 0, s>>>(D.st, D.pairs, np, D.part, sp);
    }
    MS_LAUNCH_CHECK();
    struct Tail { double lam, cost, cost0, dmax, outliers; int round, iters, stop, reason; } tail;      // RigState from lam on
    static_assert(sizeof(Tail) == sizeof(RigState) - offsetof(RigState, lam), "Tail mirrors the end of RigState");
    std::vector<double> R(9 * n_views);
    MS_HIP(hipMemcpyAsync(R.data(), D.st->R_cur, sizeof(double) * 9 * n_views, hipMemcpyDeviceToHost, s));
    MS_HIP(hipMemcpyAsync(&tail, &D.st->lam, sizeof(tail), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    if (!tail.stop) return fail(MS_ERR_HIP, "%s: the device loop ended without a stop reason (round %d, %d iterations)", fn, tail.round, tail.iters);
    memcpy(R_out, R.data(), sizeof(double) * 9 * n_views);
    if (info) {
        info->iterations = tail.iters; info->stop_reason = tail.reason;
        info->cost_initial = tail.cost0; info->cost_final = tail.cost;
        info->matches_used = (int)G.rays.size(); info->pairs_used = np; info->pairs_ignored = G.ignored;
        info->outliers = (int)tail.outliers;
        info->max_rotation_rad = 0.0;
        for (int v = 0; v < n_views; ++v) info->max_rotation_rad = std::max(info->max_rotation_rad, rig_angle(R_out + 9 * v, R_in + 9 * v));
    }
    return MS_OK;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_warper_rays(int projection, float scale, const float *t, const double *R, int n, const float *uv, double *rays)
{
    MS_CHECK(projection == MS_PROJ_PLANE || projection == MS_PROJ_CYLINDRICAL || projection == MS_PROJ_SPHERICAL, "ms_warper_rays: unknown projection %d", projection);
    MS_CHECK(R && uv && rays, "ms_warper_rays: null argument");
    MS_CHECK(scale > 0.f && std::isfinite(scale), "ms_warper_rays: warper scale %g must be positive", (double)scale);
    MS_CHECK(n >= 1, "ms_warper_rays: n = %d", n);
    for (int k = 0; k < n; ++k) warper_ray(projection, (double)scale, t, R, (double)uv[2 * k], (double)uv[2 * k + 1], rays + 3 * k);
    return MS_OK;
}

int ms_rig_refine_default_params(ms_rig_refine_params *prm)
{
    MS_CHECK(prm, "ms_rig_refine_default_params: null params");
    *prm = ms_rig_refine_params{};
    prm->struct_size = (unsigned)sizeof(ms_rig_refine_params);
    prm->anchor_view = 0; prm->huber_rad = 0.0; prm->max_iters = 50; prm->step_tol = 1e-10; prm->min_pair_matches = 4;
    return MS_OK;
}

int ms_rig_accumulate(int n_views, const double *R, const ms_rig_match *matches, int n, double huber_rad, double *cost, double *H, double *g, ms_stream stream)
{
    if (int e = rig_check_matches("ms_rig_accumulate", n_views, R, matches, n)) return e;
    MS_CHECK(cost && H && g, "ms_rig_accumulate: null output");
    MS_CHECK(huber_rad >= 0.0 && std::isfinite(huber_rad), "ms_rig_accumulate: huber_rad %g must be finite and not negative", huber_rad);
    if (int e = require_device()) return e;
    hipStream_t s = as_stream(stream);
    const RigGroups G = rig_group(n_views, matches, n, 1);
    RigDevice D;
    if (int e = rig_upload("ms_rig_accumulate", G, n_views, R, D, s)) return e;
    std::vector<RigState> host(1);
    RigState &h = host[0];
    const int np = (int)G.pairs.size();
    k_rig_accum<<<np, 256, 0, s>>>(D.st, D.pairs, D.rays, huber_rad, D.part);
    k_rig_step<<<1, RIG_STEP_THREADS, 0, s>>>(D.st, D.pairs, np, D.part, RigStepPrm{n_views, 0, 1, 1, 0.0});
    MS_LAUNCH_CHECK();
    MS_HIP(hipMemcpyAsync(&h, D.st, sizeof(RigState), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    const int d = 3 * n_views;
    *cost = h.cost;
    for (int r = 0; r < d; ++r) {
        g[r] = h.g[r];
        for (int c = 0; c < d; ++c) H[r * d + c] = h.H[r * RIG_DIM + c];
    }
    return MS_OK;
}

int ms_refine_rig_rotations(int n_views, const double *R_in, const ms_rig_match *matches, int n, const ms_rig_refine_params *prm, double *R_out, ms_rig_refine_info *info,
                            ms_stream stream)
{
    return rig_refine("ms_refine_rig_rotations", n_views, R_in, matches, n, prm, R_out, info, as_stream(stream));
}

int ms_refine_rig(ms_ctx *c, const ms_mesh_match *matches, const int *match_count, const ms_rig_refine_params *prm, float *R_out, ms_rig_refine_info *info, ms_stream stream)
{
    MS_CHECK(c && matches && match_count && prm && R_out, "ms_refine_rig: null argument");
    if (!c->maps_built) return fail(MS_ERR_STATE, "ms_refine_rig: call ms_build_maps first (the matches are pixels of the views it lays out)");
    if (c->custom_maps && !c->lens_maps)
        return fail(MS_ERR_UNSUPPORTED, "ms_refine_rig: the context's maps are the caller's own (ms_set_maps): it has no cameras to refine");
    const int N = c->N;
    long long total = 0;
    for (int v = 0; v < N; ++v) { MS_CHECK(match_count[v] >= 0, "ms_refine_rig: match_count[%d] = %d", v, match_count[v]); total += match_count[v]; }
    MS_CHECK(total >= 1 && total <= RIG_MAX_MATCHES, "ms_refine_rig: %lld matches outside [1, %d]", total, RIG_MAX_MATCHES);
    std::vector<double> R(9 * N), Rr(9 * N);
    for (int v = 0; v < N; ++v)
        for (int k = 0; k < 9; ++k) R[9 * v + k] = (double)c->R[v][k];
    // view pixel + ROI corner = the absolute warper coordinate, in double; the plane warper's t is zero in a context
    std::vector<ms_rig_match> rm((size_t)total);
    const double scale = (double)c->cfg.warp_scale;
    size_t k = 0;
    for (int v = 0; v < N; ++v)
        for (int q = 0; q < match_count[v]; ++q, ++k) {
            const ms_mesh_match &m = matches[k];
            MS_CHECK(m.dst >= 0 && m.dst < N && m.dst != v, "ms_refine_rig: match %d of view %d names view %d", q, v, m.dst);
            MS_CHECK(std::isfinite(m.x1) && std::isfinite(m.y1) && std::isfinite(m.x2) && std::isfinite(m.y2), "ms_refine_rig: match %d of view %d is not finite", q, v);
            rm[k].view_a = v; rm[k].view_b = m.dst;
            warper_ray(c->cfg.projection, scale, nullptr, &R[9 * v], (double)c->roi[v].x + (double)m.x1, (double)c->roi[v].y + (double)m.y1, rm[k].a);
            warper_ray(c->cfg.projection, scale, nullptr, &R[9 * m.dst], (double)c->roi[m.dst].x + (double)m.x2, (double)c->roi[m.dst].y + (double)m.y2, rm[k].b);
        }
    if (int e = rig_refine("ms_refine_rig", N, R.data(), rm.data(), (int)total, prm, Rr.data(), info, as_stream(stream))) return e;
    for (int q = 0; q < 9 * N; ++q) R_out[q] = (float)Rr[q];
    return MS_OK;
}

}  // extern "C"
