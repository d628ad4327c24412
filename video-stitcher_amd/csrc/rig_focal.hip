// rig_focal.hip -- self-calibrating rigs: focals and rotations from feature matches (include/ms_stitch.h, "Self-calibrating rigs"), kernels and entry points in one unit.
// detail::focalsFromHomography and detail::HomographyBasedEstimator on the host (a few dozen operations), detail::BundleAdjusterRay over focal and rotation
// (OCV/stitching/src/motion_estimators.cpp:514-700) on the device.  Calibration-time work: the per-frame path never runs anything of this unit, and rig.hip, whose
// structure this unit follows, is untouched (the helpers the two share are a few lines and are restated here).  Everything is double; -ffp-contract=off keeps every
// product, sum, division and sqrt of the per-match terms a separate IEEE operation, in the order the header states.
//   k_rigf_accum  one workgroup per view pair: the 46 sums of the pair (cost, g_i, g_j, H_ii, H_jj, H_ij, outliers), 4 unknowns a view
//   k_rigf_step   one workgroup: assembles the system in pair order, accepts or rejects the trial, moves lambda, folds the focal columns where the focal is shared,
//                 Cholesky in LDS, writes the next trial rotations and focals
// A refinement is max_iters + 1 rounds of the two, enqueued at once; both return at their first instruction once the stop flag is set.  No floating-point atomics.
#include <algorithm>
#include <cmath>
#include <vector>
#include "ctx.hpp"

namespace ms {

constexpr int RIGF_DIM = 4 * MS_MAX_VIEWS;        // rows of the normal matrix over all views, one focal a view
constexpr int RIGF_RED = 3 * (MS_MAX_VIEWS - 1) + MS_MAX_VIEWS;      // the largest system solved: 61
constexpr int RIGF_SUMS = 46;                     // cost | g_i (4) | g_j (4) | H_ii (00 01 02 03 11 12 13 22 23 33) | H_jj | H_ij (4 x 4 row-major) | outliers
constexpr int RIGF_PART = 48;                     // doubles per pair in the partials array
constexpr int RIGF_MAX_MATCHES = 1 << 20;
constexpr int RIGF_STEP_THREADS = 256;            // k_rigf_step's one workgroup

struct RigfPair { int i, j, off, cnt; };          // views i < j, the pair's matches are px[off .. off + cnt)
struct RigfPx { double a[2], b[2]; };             // centred pixels: a in view i, b in view j

// device-resident state of one refinement: nothing of it is read by the host before the last round has run
struct RigfState {
    double R_cur[MS_MAX_VIEWS * 9], f_cur[MS_MAX_VIEWS];          // the last accepted cameras
    double R_trial[MS_MAX_VIEWS * 9], f_trial[MS_MAX_VIEWS];      // what k_rigf_accum evaluates
    double H[RIGF_DIM * RIGF_DIM], g[RIGF_DIM];                   // the system at the accepted cameras, one focal a view
    double lam, cost, cost0, dmax, outliers;
    int round, iters, stop, reason;
};

struct RigfStepPrm { int n_views, anchor, shared, max_iters, assemble_only; double step_tol; };

// ---- k_rigf_accum -------------------------------------------------------------------------------------------------------------------------------
// The terms of one match, added into acc in the header's order.  h == 0: plain least squares.
__device__ __forceinline__ void rigf_terms(const double *Ri, const double *Rj, double fi, double fj, double m, const RigfPx &px, double h, double acc[RIGF_SUMS])
{
    const double na = sqrt(px.a[0] * px.a[0] + px.a[1] * px.a[1] + fi * fi), nb = sqrt(px.b[0] * px.b[0] + px.b[1] * px.b[1] + fj * fj);
    const double a0 = px.a[0] / na, a1 = px.a[1] / na, a2 = fi / na, b0 = px.b[0] / nb, b1 = px.b[1] / nb, b2 = fj / nb;
    const double p0 = Ri[0] * a0 + Ri[1] * a1 + Ri[2] * a2, p1 = Ri[3] * a0 + Ri[4] * a1 + Ri[5] * a2, p2 = Ri[6] * a0 + Ri[7] * a1 + Ri[8] * a2;
    const double q0 = Rj[0] * b0 + Rj[1] * b1 + Rj[2] * b2, q1 = Rj[3] * b0 + Rj[4] * b1 + Rj[5] * b2, q2 = Rj[6] * b0 + Rj[7] * b1 + Rj[8] * b2;
    const double u0 = m * p0, u1 = m * p1, u2 = m * p2, v0 = m * q0, v1 = m * q1, v2 = m * q2;
    const double r0 = m * (p0 - q0), r1 = m * (p1 - q1), r2 = m * (p2 - q2);
    const double s2 = r0 * r0 + r1 * r1 + r2 * r2;
    double w = 1.0, rho = s2, out = 0.0;
    if (h > 0.0) {
        const double s = sqrt(s2);
        if (s > h) { w = h / s; rho = (2.0 * h) * s - h * h; out = 1.0; }
    }
    const double ma = m * a2, mb = m * b2;
    const double ci0 = 0.5 * r0 + ma * (Ri[2] - a2 * p0), ci1 = 0.5 * r1 + ma * (Ri[5] - a2 * p1), ci2 = 0.5 * r2 + ma * (Ri[8] - a2 * p2);
    const double cj0 = 0.5 * r0 - mb * (Rj[2] - b2 * q0), cj1 = 0.5 * r1 - mb * (Rj[5] - b2 * q1), cj2 = 0.5 * r2 - mb * (Rj[8] - b2 * q2);
    acc[0] += rho;
    acc[1] += w * (u1 * r2 - u2 * r1); acc[2] += w * (u2 * r0 - u0 * r2); acc[3] += w * (u0 * r1 - u1 * r0);                // g_i: w u x r, then w ci . r
    acc[4] += w * (ci0 * r0 + ci1 * r1 + ci2 * r2);
    acc[5] += -(w * (v1 * r2 - v2 * r1)); acc[6] += -(w * (v2 * r0 - v0 * r2)); acc[7] += -(w * (v0 * r1 - v1 * r0));       // g_j: -w v x r, then w cj . r
    acc[8] += w * (cj0 * r0 + cj1 * r1 + cj2 * r2);
    acc[9] += w * (u1 * u1 + u2 * u2); acc[10] += -(w * (u0 * u1)); acc[11] += -(w * (u0 * u2)); acc[12] += w * (u1 * ci2 - u2 * ci1);      // H_ii
    acc[13] += w * (u0 * u0 + u2 * u2); acc[14] += -(w * (u1 * u2)); acc[15] += w * (u2 * ci0 - u0 * ci2);
    acc[16] += w * (u0 * u0 + u1 * u1); acc[17] += w * (u0 * ci1 - u1 * ci0);
    acc[18] += w * (ci0 * ci0 + ci1 * ci1 + ci2 * ci2);
    acc[19] += w * (v1 * v1 + v2 * v2); acc[20] += -(w * (v0 * v1)); acc[21] += -(w * (v0 * v2)); acc[22] += -(w * (v1 * cj2 - v2 * cj1));  // H_jj
    acc[23] += w * (v0 * v0 + v2 * v2); acc[24] += -(w * (v1 * v2)); acc[25] += -(w * (v2 * cj0 - v0 * cj2));
    acc[26] += w * (v0 * v0 + v1 * v1); acc[27] += -(w * (v0 * cj1 - v1 * cj0));
    acc[28] += w * (cj0 * cj0 + cj1 * cj1 + cj2 * cj2);
    acc[29] += -(w * (u1 * v1 + u2 * v2)); acc[30] += w * (v0 * u1); acc[31] += w * (v0 * u2); acc[32] += w * (u1 * cj2 - u2 * cj1);        // H_ij, row by row
    acc[33] += w * (v1 * u0); acc[34] += -(w * (u0 * v0 + u2 * v2)); acc[35] += w * (v1 * u2); acc[36] += w * (u2 * cj0 - u0 * cj2);
    acc[37] += w * (v2 * u0); acc[38] += w * (v2 * u1); acc[39] += -(w * (u0 * v0 + u1 * v1)); acc[40] += w * (u0 * cj1 - u1 * cj0);
    acc[41] += -(w * (v1 * ci2 - v2 * ci1)); acc[42] += -(w * (v2 * ci0 - v0 * ci2)); acc[43] += -(w * (v0 * ci1 - v1 * ci0));
    acc[44] += w * (ci0 * cj0 + ci1 * cj1 + ci2 * cj2);
    acc[45] += out;
}

// One 256-thread workgroup per used pair.  A thread sums the matches t, t + 256, ... in index order into registers; the 64 lanes of a wave are folded by a
// butterfly of fixed shape (lane ^ 32, ^ 16, ... ^ 1: every lane ends with the same bits), the four waves through LDS in wave order; RIGF_SUMS lanes store.
__global__ void __launch_bounds__(256) k_rigf_accum(const RigfState *__restrict__ st, const RigfPair *__restrict__ pairs, const RigfPx *__restrict__ px, double h,
                                                    double *__restrict__ part)
{
    __shared__ double s_sum[4][RIGF_PART];
    if (st->stop) return;
    const RigfPair pr = pairs[blockIdx.x];
    double Ri[9], Rj[9], acc[RIGF_SUMS];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ri[k] = st->R_trial[pr.i * 9 + k]; Rj[k] = st->R_trial[pr.j * 9 + k]; }
    const double fi = st->f_trial[pr.i], fj = st->f_trial[pr.j], m = sqrt(fi * fj);
#pragma unroll
    for (int e = 0; e < RIGF_SUMS; ++e) acc[e] = 0.0;
    for (int k = threadIdx.x; k < pr.cnt; k += 256) rigf_terms(Ri, Rj, fi, fj, m, px[pr.off + k], h, acc);
#pragma unroll
    for (int e = 0; e < RIGF_SUMS; ++e)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[e] += __shfl_xor(acc[e], d, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < RIGF_SUMS; ++e) s_sum[wave][e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < RIGF_SUMS) {
        const int e = threadIdx.x;
        part[(size_t)blockIdx.x * RIGF_PART + e] = ((s_sum[0][e] + s_sum[1][e]) + s_sum[2][e]) + s_sum[3][e];
    }
}

// ---- k_rigf_step --------------------------------------------------------------------------------------------------------------------------------
// R <- Exp(d) R, Exp by the Rodrigues formula with 1 - cos t = 2 sin^2(t / 2)
__device__ void rigf_rotate(const double *d, const double *R, double *out)
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

// where the 10 stored entries of a symmetric 4 x 4 block go
__device__ __constant__ int c_rigf_sym_r[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3}, c_rigf_sym_c[10] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};

// The solved system's row r as a row of the full one (4 a view): per-view focals drop the anchor's three rotation rows; a shared focal keeps the rotation rows of the
// views but the anchor, view after view, and returns -1 for the last row, the one focal (the sum of every view's focal row).
__device__ __forceinline__ int rigf_full_row(int r, int m, int anchor, int shared)
{
    if (!shared) return r + (r >= 4 * anchor ? 3 : 0);
    if (r == m - 1) return -1;
    const int v = r / 3;
    return 4 * (v + (v >= anchor ? 1 : 0)) + r % 3;
}

// entry (r, c) of the solved system from the full one in LDS; the focal sums of a shared focal run over the views in order
__device__ double rigf_entry(const double *Hs, int nv, int r, int c, int m, int anchor, int shared)
{
    const int fr = rigf_full_row(r, m, anchor, shared), fc = rigf_full_row(c, m, anchor, shared);
    if (fr >= 0 && fc >= 0) return Hs[fr * RIGF_DIM + fc];
    double t = 0.0;
    if (fr < 0 && fc < 0) {
        for (int v = 0; v < nv; ++v)
            for (int w = 0; w < nv; ++w) t += Hs[(4 * v + 3) * RIGF_DIM + 4 * w + 3];
    } else {
        const int o = fr < 0 ? fc : fr;       // (the full matrix is symmetric bit for bit)
        for (int v = 0; v < nv; ++v) t += Hs[o * RIGF_DIM + 4 * v + 3];
    }
    return t;
}

// One workgroup of RIGF_STEP_THREADS lanes.  Round 0 takes the system at the input cameras and proposes the first trial; every later round judges the trial k_rigf_accum
// has just evaluated.  prm.assemble_only: store the assembled cost / H / g and return (ms_rig_focal_accumulate).
// LDS: the full system Hs (64 x 64) and the solved one A (61 x 61, row stride 61) are 32768 + 29768 bytes; with the two vectors and the scalars 63.6 KB of the 64 KB a
// workgroup may declare.
__global__ void __launch_bounds__(RIGF_STEP_THREADS) k_rigf_step(RigfState *__restrict__ st, const RigfPair *__restrict__ pairs, int n_pairs, const double *__restrict__ part,
                                                                 RigfStepPrm prm)
{
    __shared__ double Hs[RIGF_DIM * RIGF_DIM], A[RIGF_RED * RIGF_RED], gs[RIGF_DIM], xs[RIGF_DIM];
    __shared__ double s_cost, s_outl, s_lam;
    __shared__ int s_accept, s_stop, s_reason, s_iters, s_ok;
    if (st->stop) return;
    const int tid = threadIdx.x, nv = prm.n_views;
    for (int k = tid; k < RIGF_DIM * RIGF_DIM; k += RIGF_STEP_THREADS) Hs[k] = 0.0;
    if (tid < RIGF_DIM) gs[tid] = 0.0;
    __syncthreads();
    // the system, pair after pair: inside a pair every sum goes to a place of its own
    for (int p = 0; p < n_pairs; ++p) {
        if (tid >= 1 && tid < 45) {
            const double v = part[(size_t)p * RIGF_PART + tid];
            const int i4 = 4 * pairs[p].i, j4 = 4 * pairs[p].j;
            if (tid < 5) gs[i4 + tid - 1] += v;
            else if (tid < 9) gs[j4 + tid - 5] += v;
            else if (tid < 29) {
                const int b4 = tid < 19 ? i4 : j4, k = tid < 19 ? tid - 9 : tid - 19, r = c_rigf_sym_r[k], c = c_rigf_sym_c[k];
                Hs[(b4 + r) * RIGF_DIM + b4 + c] += v;
                if (r != c) Hs[(b4 + c) * RIGF_DIM + b4 + r] += v;
            } else {
                const int k = tid - 29, r = k / 4, c = k % 4;
                Hs[(i4 + r) * RIGF_DIM + j4 + c] += v;
                Hs[(j4 + c) * RIGF_DIM + i4 + r] += v;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double cost = 0.0, outl = 0.0;
        for (int p = 0; p < n_pairs; ++p) { cost += part[(size_t)p * RIGF_PART]; outl += part[(size_t)p * RIGF_PART + 45]; }
        s_cost = cost; s_outl = outl;
    }
    __syncthreads();
    if (prm.assemble_only) {
        for (int k = tid; k < RIGF_DIM * RIGF_DIM; k += RIGF_STEP_THREADS) st->H[k] = Hs[k];
        if (tid < RIGF_DIM) st->g[tid] = gs[tid];
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
        for (int k = tid; k < nv * 9; k += RIGF_STEP_THREADS) st->R_cur[k] = st->R_trial[k];
        if (tid < nv) st->f_cur[tid] = st->f_trial[tid];
        for (int k = tid; k < RIGF_DIM * RIGF_DIM; k += RIGF_STEP_THREADS) st->H[k] = Hs[k];
        if (tid < RIGF_DIM) st->g[tid] = gs[tid];
    } else {
        for (int k = tid; k < RIGF_DIM * RIGF_DIM; k += RIGF_STEP_THREADS) Hs[k] = st->H[k];
        if (tid < RIGF_DIM) gs[tid] = st->g[tid];
    }
    __syncthreads();
    // (H + lambda diag H) d = -g over the rotations of the views but the anchor and the focals; a pivot that is not positive is a rejected step
    const int shared = prm.shared, anchor = prm.anchor, m = shared ? 3 * (nv - 1) + 1 : 4 * nv - 3;
    while (!s_stop) {
        const double lam = s_lam;
        for (int k = tid; k < m * m; k += RIGF_STEP_THREADS) {
            const int r = k / m, c = k % m;
            if (c > r) continue;                    // the factorisation reads the lower triangle only
            const double hv = rigf_entry(Hs, nv, r, c, m, anchor, shared);
            A[r * RIGF_RED + c] = r == c ? hv + lam * hv : hv;
        }
        if (tid == 0) s_ok = 1;
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            if (tid == 0) { const double d = A[k * RIGF_RED + k]; if (d > 0.0 && d < HUGE_VAL) A[k * RIGF_RED + k] = sqrt(d); else s_ok = 0; }
            __syncthreads();
            if (!s_ok) break;
            const double piv = A[k * RIGF_RED + k];
            for (int i = k + 1 + tid; i < m; i += RIGF_STEP_THREADS) A[i * RIGF_RED + k] /= piv;
            __syncthreads();
            const int t = m - k - 1;                // the trailing t x t block, one element a lane and pass (lower triangle only)
            for (int e = tid; e < t * t; e += RIGF_STEP_THREADS) {
                const int i = k + 1 + e / t, j = k + 1 + e % t;
                if (j <= i) A[i * RIGF_RED + j] -= A[i * RIGF_RED + k] * A[j * RIGF_RED + k];
            }
            __syncthreads();
        }
        if (s_ok) {
            // L y = -g, then L^T d = y: column by column, the pivot lane divides and every row still open subtracts the column's share
            if (tid < m) {
                const int fr = rigf_full_row(tid, m, anchor, shared);
                double gv = 0.0;
                if (fr >= 0) gv = gs[fr];
                else for (int v = 0; v < nv; ++v) gv += gs[4 * v + 3];
                xs[tid] = -gv;
            }
            __syncthreads();
            for (int c = 0; c < m; ++c) {
                if (tid == 0) xs[c] /= A[c * RIGF_RED + c];
                __syncthreads();
                if (tid > c && tid < m) xs[tid] -= A[tid * RIGF_RED + c] * xs[c];
                __syncthreads();
            }
            for (int c = m - 1; c >= 0; --c) {
                if (tid == 0) xs[c] /= A[c * RIGF_RED + c];
                __syncthreads();
                if (tid < c) xs[tid] -= A[c * RIGF_RED + tid] * xs[c];
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
        // where view tid's step sits in xs: per-view focals (rotation, focal) view after view with the anchor's rotation left out; shared: the focal is the last entry
        const int rot = shared ? 3 * (tid - (tid > anchor ? 1 : 0)) : 4 * tid - (tid > anchor ? 3 : 0);
        const int foc = shared ? m - 1 : (tid == anchor ? rot : rot + 3);
        if (tid == anchor) { for (int k = 0; k < 9; ++k) st->R_trial[tid * 9 + k] = st->R_cur[tid * 9 + k]; }
        else rigf_rotate(&xs[rot], &st->R_cur[tid * 9], &st->R_trial[tid * 9]);
        st->f_trial[tid] = st->f_cur[tid] * exp(xs[foc]);
    }
    if (tid == 0) { st->lam = s_lam; st->iters = s_iters; st->reason = s_reason; st->stop = s_stop; st->round = st->round + 1; }
}

// ---- host side: the homography estimator --------------------------------------------------------------------------------------------------------
static void rigf_focals_from_h(const double *h, double *f0, double *f1, int *ok0, int *ok1)
{
    // the two candidate squares of a focal and their denominators; the candidate with the larger denominator wins where both are positive
    auto pick = [](double v1, double d1, double v2, double d2, double *f) {
        if (v1 < v2) { std::swap(v1, v2); }
        if (v1 > 0.0 && v2 > 0.0) { *f = std::sqrt(std::fabs(d1) > std::fabs(d2) ? v1 : v2); return 1; }
        if (v1 > 0.0) { *f = std::sqrt(v1); return 1; }
        return 0;
    };
    double d1 = h[6] * h[7], d2 = (h[7] - h[6]) * (h[7] + h[6]);
    *ok1 = pick(-(h[0] * h[1] + h[3] * h[4]) / d1, d1, (h[0] * h[0] + h[3] * h[3] - h[1] * h[1] - h[4] * h[4]) / d2, d2, f1);
    d1 = h[0] * h[3] + h[1] * h[4]; d2 = h[0] * h[0] + h[1] * h[1] - h[3] * h[3] - h[4] * h[4];
    *ok0 = pick(-h[2] * h[5] / d1, d1, (h[5] * h[5] - h[2] * h[2]) / d2, d2, f0);
}

static void rigf_mul3(const double *A, const double *B, double *C)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
}

static double rigf_det3(const double *M)
{
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

static bool rigf_inv3(const double *M, double *out)
{
    const double d = rigf_det3(M);
    if (!(std::fabs(d) > 0.0) || !std::isfinite(d)) return false;
    const double adj[9] = {M[4] * M[8] - M[5] * M[7], M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4],
                           M[5] * M[6] - M[3] * M[8], M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5],
                           M[3] * M[7] - M[4] * M[6], M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3]};
    for (int k = 0; k < 9; ++k) { out[k] = adj[k] / d; if (!std::isfinite(out[k])) return false; }
    return true;
}

// The rotation nearest to M: U V^T of M = U S V^T by a one-sided Jacobi SVD (column pairs of M V are turned until they are orthogonal; V collects the turns), the
// column of U of the smallest singular value negated where det U V^T < 0.  false: a singular value is zero.
static bool rigf_nearest_rotation(const double *M, double *R)
{
    double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) A[k] = M[k];
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool turned = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int k = 0; k < 3; ++k) { al += A[k * 3 + p] * A[k * 3 + p]; be += A[k * 3 + q] * A[k * 3 + q]; ga += A[k * 3 + p] * A[k * 3 + q]; }
                if (!(std::fabs(ga) > 1e-17 * std::sqrt(al * be))) continue;
                turned = true;
                const double zeta = (be - al) / (2.0 * ga), t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta)), c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < 3; ++k) {
                    const double ap = A[k * 3 + p], aq = A[k * 3 + q], vp = V[k * 3 + p], vq = V[k * 3 + q];
                    A[k * 3 + p] = c * ap - s * aq; A[k * 3 + q] = s * ap + c * aq;
                    V[k * 3 + p] = c * vp - s * vq; V[k * 3 + q] = s * vp + c * vq;
                }
            }
        if (!turned) break;
    }
    double U[9], sv[3];
    for (int c = 0; c < 3; ++c) {
        sv[c] = std::sqrt(A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c]);
        if (!(sv[c] > 0.0) || !std::isfinite(sv[c])) return false;
        for (int k = 0; k < 3; ++k) U[k * 3 + c] = A[k * 3 + c] / sv[c];
    }
    auto uvt = [&]() { for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = U[r * 3] * V[c * 3] + U[r * 3 + 1] * V[c * 3 + 1] + U[r * 3 + 2] * V[c * 3 + 2]; };
    uvt();
    if (rigf_det3(R) < 0.0) {
        const int lo = sv[0] <= sv[1] && sv[0] <= sv[2] ? 0 : (sv[1] <= sv[2] ? 1 : 2);
        for (int k = 0; k < 3; ++k) U[k * 3 + lo] = -U[k * 3 + lo];
        uvt();
    }
    return true;
}

// ---- host side: the bundle adjustment -----------------------------------------------------------------------------------------------------------
// the warper's backward direction of absolute warper coordinates, turned into the camera by R^T and normalised (ms_warper_rays' arithmetic)
static void rigf_warper_ray(int proj, double scale, const double *R, double u, double v, double *out)
{
    const double pi = 3.14159265358979323846, up = u / scale, vp = v / scale;
    double dx, dy, dz;
    if (proj == MS_PROJ_SPHERICAL) { const double sv = sin(pi - vp); dx = sv * sin(up); dy = cos(pi - vp); dz = sv * cos(up); }
    else if (proj == MS_PROJ_CYLINDRICAL) { dx = sin(up); dy = vp; dz = cos(up); }
    else { dx = up; dy = vp; dz = 1.0; }
    const double X = R[0] * dx + R[3] * dy + R[6] * dz, Y = R[1] * dx + R[4] * dy + R[7] * dz, Z = R[2] * dx + R[5] * dy + R[8] * dz;
    const double n = sqrt(X * X + Y * Y + Z * Z);
    out[0] = X / n; out[1] = Y / n; out[2] = Z / n;
}

static int rigf_check_cameras(const char *fn, int n_views, const double *f, const double *R)
{
    MS_CHECK(n_views >= 2 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d outside [2, %d]", fn, n_views, MS_MAX_VIEWS);
    MS_CHECK(f && R, "%s: null argument", fn);
    for (int v = 0; v < n_views; ++v) {
        MS_CHECK(std::isfinite(f[v]) && f[v] > 0.0, "%s: focal of view %d (%g) is not finite and positive", fn, v, f[v]);
        const double *Rv = R + 9 * v;
        for (int k = 0; k < 9; ++k) MS_CHECK(std::isfinite(Rv[k]), "%s: rotation of view %d is not finite", fn, v);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double e = Rv[r * 3] * Rv[c * 3] + Rv[r * 3 + 1] * Rv[c * 3 + 1] + Rv[r * 3 + 2] * Rv[c * 3 + 2] - (r == c ? 1.0 : 0.0);
                MS_CHECK(std::fabs(e) <= 1e-6, "%s: rotation of view %d is not orthonormal: R R^T is off the identity by %g", fn, v, std::fabs(e));
            }
    }
    return MS_OK;
}

static int rigf_check_matches(const char *fn, int n_views, const ms_rig_px_match *matches, int n)
{
    MS_CHECK(matches, "%s: null argument", fn);
    MS_CHECK(n >= 1 && n <= RIGF_MAX_MATCHES, "%s: %d matches outside [1, %d]", fn, n, RIGF_MAX_MATCHES);
    for (int k = 0; k < n; ++k) {
        const ms_rig_px_match &m = matches[k];
        MS_CHECK(m.view_a >= 0 && m.view_a < n_views && m.view_b >= 0 && m.view_b < n_views, "%s: match %d names views %d, %d outside [0, %d)", fn, k, m.view_a, m.view_b, n_views);
        MS_CHECK(m.view_a != m.view_b, "%s: match %d pairs view %d with itself", fn, k, m.view_a);
        MS_CHECK(std::isfinite(m.a[0]) && std::isfinite(m.a[1]) && std::isfinite(m.b[0]) && std::isfinite(m.b[1]), "%s: match %d: a pixel is not finite", fn, k);
    }
    return MS_OK;
}

// Matches grouped by canonical pair (i < j, a and b swapped where the caller listed (j, i)), pairs in (i, j) order, input order kept inside a pair.  A pair with fewer
// than min_pair matches is left out and counted.
struct RigfGroups { std::vector<RigfPair> pairs; std::vector<RigfPx> px; int ignored = 0; };
static RigfGroups rigf_group(int n_views, const ms_rig_px_match *matches, int n, int min_pair)
{
    std::vector<int> cnt(n_views * n_views, 0), slot(n_views * n_views, -1);
    auto key = [&](const ms_rig_px_match &m) { return std::min(m.view_a, m.view_b) * n_views + std::max(m.view_a, m.view_b); };
    for (int k = 0; k < n; ++k) ++cnt[key(matches[k])];
    RigfGroups G;
    int off = 0;
    for (int q = 0; q < n_views * n_views; ++q) {
        if (!cnt[q]) continue;
        if (cnt[q] < min_pair) { ++G.ignored; continue; }
        slot[q] = (int)G.pairs.size();
        G.pairs.push_back(RigfPair{q / n_views, q % n_views, off, 0});
        off += cnt[q];
    }
    G.px.resize(off);
    for (int k = 0; k < n; ++k) {
        const ms_rig_px_match &m = matches[k];
        const int s = slot[key(m)];
        if (s < 0) continue;
        RigfPair &p = G.pairs[s];
        RigfPx &r = G.px[p.off + p.cnt++];
        const bool swap = m.view_a > m.view_b;
        for (int c = 0; c < 2; ++c) { r.a[c] = swap ? m.b[c] : m.a[c]; r.b[c] = swap ? m.a[c] : m.b[c]; }
    }
    return G;
}

// One device block, state | pairs | pixels | partials (all 8-byte aligned): the first three are laid out in pinned memory and go up in ONE copy.
struct RigfDevice { RigfState *st; RigfPair *pairs; RigfPx *px; double *part; };
static int rigf_upload(const char *fn, const RigfGroups &G, int n_views, const double *f, const double *R, RigfDevice &D, hipStream_t s)
{
    const size_t np = G.pairs.size(), o_pairs = sizeof(RigfState), o_px = o_pairs + np * sizeof(RigfPair), o_part = o_px + G.px.size() * sizeof(RigfPx),
                 total = o_part + np * RIGF_PART * sizeof(double);
    char *base = (char *)device_scratch().get(total), *host = (char *)pinned_scratch().get(o_part);
    if (!base || !host) return fail(MS_ERR_NOMEM, "%s: no memory for %zu bytes", fn, total);
    D.st = (RigfState *)base; D.pairs = (RigfPair *)(base + o_pairs); D.px = (RigfPx *)(base + o_px); D.part = (double *)(base + o_part);
    RigfState *st = (RigfState *)host;
    memset(st, 0, sizeof(RigfState));
    memcpy(st->R_cur, R, sizeof(double) * 9 * n_views); memcpy(st->R_trial, R, sizeof(double) * 9 * n_views);
    memcpy(st->f_cur, f, sizeof(double) * n_views); memcpy(st->f_trial, f, sizeof(double) * n_views);
    st->lam = 1e-3;
    memcpy(host + o_pairs, G.pairs.data(), np * sizeof(RigfPair));
    memcpy(host + o_px, G.px.data(), G.px.size() * sizeof(RigfPx));
    MS_HIP(hipMemcpyAsync(base, host, o_part, hipMemcpyHostToDevice, s));
    return MS_OK;
}

static double rigf_angle(const double *A, const double *B)      // the angle of A B^T
{
    double M[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[r * 3 + c] = A[r * 3] * B[c * 3] + A[r * 3 + 1] * B[c * 3 + 1] + A[r * 3 + 2] * B[c * 3 + 2];
    const double x = M[7] - M[5], y = M[2] - M[6], z = M[3] - M[1];
    return atan2(0.5 * sqrt(x * x + y * y + z * z), 0.5 * (M[0] + M[4] + M[8] - 1.0));
}

static int rigf_check_params(const char *fn, int n_views, const ms_rig_focal_params *prm)
{
    MS_CHECK(prm, "%s: null params", fn);
    MS_CHECK(prm->struct_size == sizeof(ms_rig_focal_params), "%s: params.struct_size %u, this library's ms_rig_focal_params has %zu bytes", fn, prm->struct_size,
             sizeof(ms_rig_focal_params));
    MS_CHECK(prm->anchor_view >= 0 && prm->anchor_view < n_views, "%s: anchor_view %d outside [0, %d)", fn, prm->anchor_view, n_views);
    MS_CHECK(prm->huber_px >= 0.0 && std::isfinite(prm->huber_px), "%s: huber_px %g must be finite and not negative", fn, prm->huber_px);
    MS_CHECK(prm->max_iters >= 1 && prm->max_iters <= 1000, "%s: max_iters %d outside [1, 1000]", fn, prm->max_iters);
    MS_CHECK(prm->step_tol >= 0.0 && std::isfinite(prm->step_tol), "%s: step_tol %g must be finite and not negative", fn, prm->step_tol);
    MS_CHECK(prm->min_pair_matches >= 1, "%s: min_pair_matches %d must be at least 1", fn, prm->min_pair_matches);
    return MS_OK;
}

// everything ms_refine_rig_cameras does; fn names the entry point in messages
static int rigf_refine(const char *fn, int n_views, const double *f_in, const double *R_in, const ms_rig_px_match *matches, int n, const ms_rig_focal_params *prm,
                       double *f_out, double *R_out, ms_rig_focal_info *info, hipStream_t s)
{
    if (int e = rigf_check_cameras(fn, n_views, f_in, R_in)) return e;
    if (int e = rigf_check_matches(fn, n_views, matches, n)) return e;
    MS_CHECK(f_out && R_out, "%s: null output", fn);
    if (int e = rigf_check_params(fn, n_views, prm)) return e;
    if (prm->shared_focal)
        for (int v = 1; v < n_views; ++v)
            MS_CHECK(f_in[v] == f_in[0], "%s: shared_focal asks for equal input focals; view %d has %.17g, view 0 has %.17g", fn, v, f_in[v], f_in[0]);
    const RigfGroups G = rigf_group(n_views, matches, n, prm->min_pair_matches);
    // every view must hang on the anchor through used pairs
    std::vector<char> seen(n_views, 0);
    std::vector<int> todo{prm->anchor_view};
    seen[prm->anchor_view] = 1;
    while (!todo.empty()) {
        const int v = todo.back(); todo.pop_back();
        for (const RigfPair &p : G.pairs) {
            const int o = p.i == v ? p.j : p.j == v ? p.i : -1;
            if (o >= 0 && !seen[o]) { seen[o] = 1; todo.push_back(o); }
        }
    }
    for (int v = 0; v < n_views; ++v)
        MS_CHECK(seen[v], "%s: view %d is not connected to the anchor view %d by pairs of at least %d matches (%d pairs ignored)", fn, v, prm->anchor_view,
                 prm->min_pair_matches, G.ignored);
    if (int e = require_device()) return e;

    RigfDevice D;
    if (int e = rigf_upload(fn, G, n_views, f_in, R_in, D, s)) return e;
    const RigfStepPrm sp{n_views, prm->anchor_view, prm->shared_focal ? 1 : 0, prm->max_iters, 0, prm->step_tol};
    const int np = (int)G.pairs.size();
    for (int round = 0; round <= prm->max_iters; ++round) {
        k_rigf_accum<<<np, 256, 0, s>>>(D.st, D.pairs, D.px, prm->huber_px, D.part);
        k_rigf_step<<<1, RIGF_STEP_THREADS, 0, s>>>(D.st, D.pairs, np, D.part, sp);
    }
    MS_LAUNCH_CHECK();
    struct Tail { double lam, cost, cost0, dmax, outliers; int round, iters, stop, reason; } tail;      // RigfState from lam on
    static_assert(sizeof(Tail) == sizeof(RigfState) - offsetof(RigfState, lam), "Tail mirrors the end of RigfState");
    static_assert(offsetof(RigfState, f_cur) == sizeof(double) * 9 * MS_MAX_VIEWS, "f_cur follows R_cur: the two come back in one copy");
    std::vector<double> cam(10 * MS_MAX_VIEWS);
    MS_HIP(hipMemcpyAsync(cam.data(), D.st->R_cur, sizeof(double) * 10 * MS_MAX_VIEWS, hipMemcpyDeviceToHost, s));
    MS_HIP(hipMemcpyAsync(&tail, &D.st->lam, sizeof(tail), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    if (!tail.stop) return fail(MS_ERR_HIP, "%s: the device loop ended without a stop reason (round %d, %d iterations)", fn, tail.round, tail.iters);
    memcpy(R_out, cam.data(), sizeof(double) * 9 * n_views);
    memcpy(f_out, cam.data() + 9 * MS_MAX_VIEWS, sizeof(double) * n_views);
    if (info) {
        info->iterations = tail.iters; info->stop_reason = tail.reason;
        info->cost_initial = tail.cost0; info->cost_final = tail.cost;
        info->matches_used = (int)G.px.size(); info->pairs_used = np; info->pairs_ignored = G.ignored;
        info->outliers = (int)tail.outliers;
        info->max_rotation_rad = 0.0; info->max_focal_ratio = 1.0;
        for (int v = 0; v < n_views; ++v) {
            info->max_rotation_rad = std::max(info->max_rotation_rad, rigf_angle(R_out + 9 * v, R_in + 9 * v));
            info->max_focal_ratio = std::max(info->max_focal_ratio, std::max(f_out[v] / f_in[v], f_in[v] / f_out[v]));
        }
    }
    return MS_OK;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_focals_from_homography(const double H[9], double *f0, double *f1, int *f0_ok, int *f1_ok)
{
    MS_CHECK(H && f0 && f1 && f0_ok && f1_ok, "ms_focals_from_homography: null argument");
    for (int k = 0; k < 9; ++k) MS_CHECK(std::isfinite(H[k]), "ms_focals_from_homography: H[%d] is not finite", k);
    double a = 0.0, b = 0.0;
    rigf_focals_from_h(H, &a, &b, f0_ok, f1_ok);
    if (*f0_ok) *f0 = a;
    if (*f1_ok) *f1 = b;
    return MS_OK;
}

int ms_estimate_rig(int n_views, const ms_pair_homography *pairs, int n_pairs, int anchor, int width, int height, double *focals, double *R, ms_rig_estimate_info *info)
{
    const char *fn = "ms_estimate_rig";
    MS_CHECK(n_views >= 2 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d outside [2, %d]", fn, n_views, MS_MAX_VIEWS);
    MS_CHECK(pairs && focals && R, "%s: null argument", fn);
    MS_CHECK(n_pairs >= 1 && n_pairs <= MS_MAX_VIEWS * MS_MAX_VIEWS, "%s: n_pairs = %d outside [1, %d]", fn, n_pairs, MS_MAX_VIEWS * MS_MAX_VIEWS);
    MS_CHECK(anchor >= 0 && anchor < n_views, "%s: anchor %d outside [0, %d)", fn, anchor, n_views);
    MS_CHECK(width >= 1 && height >= 1, "%s: image size %d x %d", fn, width, height);
    std::vector<double> Hinv(9 * (size_t)n_pairs);
    for (int k = 0; k < n_pairs; ++k) {
        const ms_pair_homography &p = pairs[k];
        MS_CHECK(p.view_a >= 0 && p.view_a < n_views && p.view_b >= 0 && p.view_b < n_views, "%s: pair %d names views %d, %d outside [0, %d)", fn, k, p.view_a, p.view_b, n_views);
        MS_CHECK(p.view_a != p.view_b, "%s: pair %d pairs view %d with itself", fn, k, p.view_a);
        MS_CHECK(p.weight >= 0, "%s: pair %d has weight %d", fn, k, p.weight);
        for (int e = 0; e < 9; ++e) MS_CHECK(std::isfinite(p.H[e]), "%s: pair %d: H[%d] is not finite", fn, k, e);
        MS_CHECK(rigf_inv3(p.H, &Hinv[9 * (size_t)k]), "%s: pair %d: H is singular", fn, k);
    }
    // the maximum spanning tree: pairs by falling weight, the earlier first among equals, taken where they join two components
    std::vector<int> order(n_pairs), comp(n_views), parent(n_views, -2), via(n_views, -1);
    for (int k = 0; k < n_pairs; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return pairs[x].weight > pairs[y].weight; });
    for (int v = 0; v < n_views; ++v) comp[v] = v;
    std::vector<int> tree;
    for (int k : order) {
        const int ca = comp[pairs[k].view_a], cb = comp[pairs[k].view_b];
        if (ca == cb) continue;
        for (int v = 0; v < n_views; ++v) if (comp[v] == cb) comp[v] = ca;
        tree.push_back(k);
    }
    // breadth-first from the anchor
    std::vector<int> queue{anchor};
    parent[anchor] = -1;
    for (size_t head = 0; head < queue.size(); ++head) {
        const int v = queue[head];
        for (int k : tree) {
            const int o = pairs[k].view_a == v ? pairs[k].view_b : pairs[k].view_b == v ? pairs[k].view_a : -1;
            if (o >= 0 && parent[o] == -2) { parent[o] = v; via[o] = k; queue.push_back(o); }
        }
    }
    for (int v = 0; v < n_views; ++v) MS_CHECK(parent[v] != -2, "%s: view %d is not connected to the anchor view %d by the %d pairs", fn, v, anchor, n_pairs);
    // the focal every view gets
    std::vector<double> est;
    for (int k = 0; k < n_pairs; ++k) {
        double f0 = 0.0, f1 = 0.0; int ok0 = 0, ok1 = 0;
        rigf_focals_from_h(pairs[k].H, &f0, &f1, &ok0, &ok1);
        if (ok0 && ok1) est.push_back(std::sqrt(f0 * f1));
    }
    std::sort(est.begin(), est.end());
    const size_t ne = est.size();
    const double focal = ne == 0 ? (double)width + (double)height : (ne % 2 ? est[ne / 2] : (est[ne / 2 - 1] + est[ne / 2]) * 0.5);
    for (int v = 0; v < n_views; ++v) focals[v] = focal;
    // the rotations along the tree
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, K[9] = {focal, 0, 0, 0, focal, 0, 0, 0, 1}, Kinv[9] = {1.0 / focal, 0, 0, 0, 1.0 / focal, 0, 0, 0, 1};
    for (int v : queue) {
        if (v == anchor) { memcpy(R + 9 * v, I3, sizeof(I3)); continue; }
        const ms_pair_homography &p = pairs[via[v]];
        const double *back = p.view_b == v ? &Hinv[9 * (size_t)via[v]] : p.H;      // the map from v's pixels to its parent's
        double T1[9], T2[9], M[9];
        rigf_mul3(Kinv, back, T1); rigf_mul3(T1, K, T2); rigf_mul3(R + 9 * parent[v], T2, M);
        MS_CHECK(rigf_nearest_rotation(M, R + 9 * v), "%s: pair %d: the chained rotation of view %d is singular", fn, via[v], v);
    }
    if (info) {
        info->focal_estimates = (int)ne;
        for (int v = 0; v < MS_MAX_VIEWS; ++v) info->tree_parent[v] = v < n_views ? parent[v] : -1;
    }
    return ne == 0 ? 1 : MS_OK;
}

int ms_rig_focal_default_params(ms_rig_focal_params *prm)
{
    MS_CHECK(prm, "ms_rig_focal_default_params: null params");
    *prm = ms_rig_focal_params{};
    prm->struct_size = (unsigned)sizeof(ms_rig_focal_params);
    prm->anchor_view = 0; prm->shared_focal = 0; prm->huber_px = 0.0; prm->max_iters = 50; prm->step_tol = 1e-10; prm->min_pair_matches = 4;
    return MS_OK;
}

int ms_rig_focal_accumulate(int n_views, const double *f, const double *R, const ms_rig_px_match *matches, int n, double huber_px, double *cost, double *H, double *g,
                            ms_stream stream)
{
    const char *fn = "ms_rig_focal_accumulate";
    if (int e = rigf_check_cameras(fn, n_views, f, R)) return e;
    if (int e = rigf_check_matches(fn, n_views, matches, n)) return e;
    MS_CHECK(cost && H && g, "%s: null output", fn);
    MS_CHECK(huber_px >= 0.0 && std::isfinite(huber_px), "%s: huber_px %g must be finite and not negative", fn, huber_px);
    if (int e = require_device()) return e;
    hipStream_t s = as_stream(stream);
    const RigfGroups G = rigf_group(n_views, matches, n, 1);
    RigfDevice D;
    if (int e = rigf_upload(fn, G, n_views, f, R, D, s)) return e;
    std::vector<RigfState> host(1);
    RigfState &h = host[0];
    const int np = (int)G.pairs.size();
    k_rigf_accum<<<np, 256, 0, s>>>(D.st, D.pairs, D.px, huber_px, D.part);
    k_rigf_step<<<1, RIGF_STEP_THREADS, 0, s>>>(D.st, D.pairs, np, D.part, RigfStepPrm{n_views, 0, 0, 1, 1, 0.0});
    MS_LAUNCH_CHECK();
    MS_HIP(hipMemcpyAsync(&h, D.st, sizeof(RigfState), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    const int d = 4 * n_views;
    *cost = h.cost;
    for (int r = 0; r < d; ++r) {
        g[r] = h.g[r];
        for (int c = 0; c < d; ++c) H[r * d + c] = h.H[r * RIGF_DIM + c];
    }
    return MS_OK;
}

int ms_refine_rig_cameras(int n_views, const double *f_in, const double *R_in, const ms_rig_px_match *matches, int n, const ms_rig_focal_params *prm, double *f_out,
                          double *R_out, ms_rig_focal_info *info, ms_stream stream)
{
    return rigf_refine("ms_refine_rig_cameras", n_views, f_in, R_in, matches, n, prm, f_out, R_out, info, as_stream(stream));
}

int ms_refine_rig_focals(ms_ctx *c, const ms_mesh_match *matches, const int *match_count, const ms_rig_focal_params *prm, double *focal_out, float *R_out,
                         ms_rig_focal_info *info, ms_stream stream)
{
    const char *fn = "ms_refine_rig_focals";
    MS_CHECK(c && matches && match_count && prm && focal_out && R_out, "%s: null argument", fn);
    if (!c->maps_built) return fail(MS_ERR_STATE, "%s: call ms_build_maps first (the matches are pixels of the views it lays out)", fn);
    if (c->custom_maps && !c->lens_maps)
        return fail(MS_ERR_UNSUPPORTED, "%s: the context's maps are the caller's own (ms_set_maps): it has no cameras to refine", fn);
    if (c->lens_maps)
        return fail(MS_ERR_UNSUPPORTED, "%s: the context has a lens (ms_set_lens): a focal under a lens needs the inverse distortion, which the library does not have", fn);
    const int N = c->N;
    long long total = 0;
    for (int v = 0; v < N; ++v) { MS_CHECK(match_count[v] >= 0, "%s: match_count[%d] = %d", fn, v, match_count[v]); total += match_count[v]; }
    MS_CHECK(total >= 1 && total <= RIGF_MAX_MATCHES, "%s: %lld matches outside [1, %d]", fn, total, RIGF_MAX_MATCHES);
    std::vector<double> R(9 * N), Rr(9 * N), f(N);
    for (int v = 0; v < N; ++v) {
        for (int k = 0; k < 9; ++k) R[9 * v + k] = (double)c->R[v][k];
        f[v] = (double)c->K[v][0];
    }
    // view pixel + ROI corner = the absolute warper coordinate, in double; the plane warper's t is zero in a context
    std::vector<ms_rig_px_match> pm((size_t)total);
    const double scale = (double)c->cfg.warp_scale;
    size_t k = 0;
    for (int v = 0; v < N; ++v)
        for (int q = 0; q < match_count[v]; ++q, ++k) {
            const ms_mesh_match &m = matches[k];
            MS_CHECK(m.dst >= 0 && m.dst < N && m.dst != v, "%s: match %d of view %d names view %d", fn, q, v, m.dst);
            MS_CHECK(std::isfinite(m.x1) && std::isfinite(m.y1) && std::isfinite(m.x2) && std::isfinite(m.y2), "%s: match %d of view %d is not finite", fn, q, v);
            double ra[3], rb[3];
            rigf_warper_ray(c->cfg.projection, scale, &R[9 * v], (double)c->roi[v].x + (double)m.x1, (double)c->roi[v].y + (double)m.y1, ra);
            rigf_warper_ray(c->cfg.projection, scale, &R[9 * m.dst], (double)c->roi[m.dst].x + (double)m.x2, (double)c->roi[m.dst].y + (double)m.y2, rb);
            MS_CHECK(ra[2] > 0.0 && rb[2] > 0.0, "%s: match %d of view %d: a ray lies behind its camera (z = %g, %g): it has no source pixel", fn, q, v, ra[2], rb[2]);
            pm[k].view_a = v; pm[k].view_b = m.dst;
            pm[k].a[0] = f[v] * (ra[0] / ra[2]); pm[k].a[1] = f[v] * (ra[1] / ra[2]);
            pm[k].b[0] = f[m.dst] * (rb[0] / rb[2]); pm[k].b[1] = f[m.dst] * (rb[1] / rb[2]);
        }
    // single-precision rotations are orthonormal to about 1e-7 only: what the context holds is used as it is, as ms_refine_rig does
    if (int e = rigf_refine(fn, N, f.data(), R.data(), pm.data(), (int)total, prm, focal_out, Rr.data(), info, as_stream(stream))) return e;
    for (int q = 0; q < 9 * N; ++q) R_out[q] = (float)Rr[q];
    return MS_OK;
}

}  // extern "C"
