// rig_lm.hpp -- the Levenberg-Marquardt core the rig refinements share: rig.hip (rotations from unit rays, B = 3 unknowns a view), rig_focal.hip (rotations and
// focals from centred pixels, B = 4) and rig_lens.hip (the same through fixed lenses, B = 4).  Internal; those three units include it and nothing else does.  A unit
// supplies a policy -- its match record, B, what a workgroup loads per pair beside the two rotations (from the state, and from an array Aux of fixed per-view data
// that goes up next to the state: the lenses; char and empty where a policy has none), and the per-match terms of include/ms_stitch.h -- and gets from here, each once:
//   k_rig_accum<P>   one workgroup per view pair: the sums of the pair (RigSums<B>) in one fixed order
//   k_rig_step<B>    one workgroup: assembles the system in pair order, accepts or rejects the trial, moves lambda, folds the focal columns where the focal is shared
//                    (B = 4), Cholesky in LDS, writes the next trial
// and the host side around them: the grouping by pair, the one pinned upload, the connectivity check, the max_iters + 1 rounds, the copy back, the parameter checks and
// the walk over a context's match lists.  Everything is double; no floating-point atomics: every sum has one fixed order, so a call's result does not depend on scheduling.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>
#include "ctx.hpp"
#include "lens.hpp"

namespace ms {

constexpr int RIG_MAX_MATCHES = 1 << 20;
constexpr int RIG_STEP_THREADS = 256;         // k_rig_step's one workgroup

// The sums of one pair: cost | g_i (B) | g_j (B) | H_ii upper triangle row-major (B (B + 1) / 2) | H_jj (same) | H_ij (B x B row-major) | outliers
template <int B> struct RigSums {
    static constexpr int TRI = B * (B + 1) / 2;
    static constexpr int G_I = 1, G_J = G_I + B, H_II = G_J + B, H_JJ = H_II + TRI, H_IJ = H_JJ + TRI, OUTL = H_IJ + B * B;
    static constexpr int SUMS = OUTL + 1;                     // 29, 46
    static constexpr int PART = (SUMS + 15) / 16 * 16;        // doubles per pair in the partials array: 32, 48
    static constexpr int DIM = B * MS_MAX_VIEWS;              // rows of the normal matrix over all views
    static constexpr int RED = 3 * (MS_MAX_VIEWS - 1) + (B == 4 ? MS_MAX_VIEWS : 0);      // the largest system solved: 45, 61
};

// where the stored entries of a symmetric B x B block go
template <int B> struct RigSym { int r[RigSums<B>::TRI], c[RigSums<B>::TRI]; };
template <int B> constexpr RigSym<B> rig_sym()
{
    RigSym<B> t{};
    for (int r = 0, k = 0; r < B; ++r)
        for (int c = r; c < B; ++c, ++k) { t.r[k] = r; t.c[k] = c; }
    return t;
}

struct RigPair { int i, j, off, cnt; };     // views i < j, the pair's matches are items[off .. off + cnt)

// device-resident state of one refinement: nothing of it is read by the host before the last round has run (B = 3 leaves the focals unused)
struct RigTail { double lam, cost, cost0, dmax, outliers; int round, iters, stop, reason; };
template <int B> struct RigState {
    double R_cur[MS_MAX_VIEWS * 9], f_cur[MS_MAX_VIEWS];          // the last accepted cameras: they come back in one copy
    double R_trial[MS_MAX_VIEWS * 9], f_trial[MS_MAX_VIEWS];      // what k_rig_accum evaluates
    double H[RigSums<B>::DIM * RigSums<B>::DIM], g[RigSums<B>::DIM];      // the system at the accepted cameras
    RigTail t;                                                    // comes back in one copy
};

struct RigStepPrm { int n_views, anchor, shared, max_iters, assemble_only; double step_tol; };

// ---- k_rig_accum --------------------------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per used pair.  A thread sums the matches t, t + 256, ... in index order into registers; the 64 lanes of a wave are folded by a
// butterfly of fixed shape (lane ^ 32, ^ 16, ... ^ 1: every lane ends with the same bits), the four waves through LDS in wave order; SUMS lanes store.
template <class P> __global__ void __launch_bounds__(256) k_rig_accum(const RigState<P::B> *__restrict__ st, const RigPair *__restrict__ pairs,
                                                                      const typename P::Match *__restrict__ items, const typename P::Aux *__restrict__ aux, double h,
                                                                      double *__restrict__ part)
{
    using S = RigSums<P::B>;
    __shared__ double s_sum[4][S::PART];
    if (st->t.stop) return;
    const RigPair pr = pairs[blockIdx.x];
    double Ri[9], Rj[9], acc[S::SUMS];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ri[k] = st->R_trial[pr.i * 9 + k]; Rj[k] = st->R_trial[pr.j * 9 + k]; }
    const typename P::Cams cams = P::load(st, pr, aux);
#pragma unroll
    for (int e = 0; e < S::SUMS; ++e) acc[e] = 0.0;
    for (int k = threadIdx.x; k < pr.cnt; k += 256) P::terms(Ri, Rj, cams, items[pr.off + k], h, acc);
#pragma unroll
    for (int e = 0; e < S::SUMS; ++e)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[e] += __shfl_xor(acc[e], d, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < S::SUMS; ++e) s_sum[wave][e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < S::SUMS) {
        const int e = threadIdx.x;
        part[(size_t)blockIdx.x * S::PART + e] = ((s_sum[0][e] + s_sum[1][e]) + s_sum[2][e]) + s_sum[3][e];
    }
}

// ---- k_rig_step ---------------------------------------------------------------------------------------------------------------------------------
// R <- Exp(d) R, Exp by the Rodrigues formula with 1 - cos t = 2 sin^2(t / 2)
static __device__ void rig_rotate(const double *d, const double *R, double *out)
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

// The solved system's row r as a row of the full one (B a view): the anchor's three rotation rows are dropped.  A shared focal (B = 4) keeps the rotation rows of the
// views but the anchor, view after view, and returns -1 for the last row, the one focal (the sum of every view's focal row).
template <int B> __device__ __forceinline__ int rig_full_row(int r, int m, int anchor, int shared)
{
    if (B != 4 || !shared) return r + (r >= B * anchor ? 3 : 0);      // (B is a constant: the B = 3 instance ends here)
    if (r == m - 1) return -1;
    const int v = r / 3;
    return 4 * (v + (v >= anchor ? 1 : 0)) + r % 3;
}

// entry (r, c) of the solved system from the full one in LDS; the focal sums of a shared focal run over the views in order
template <int B> __device__ double rig_entry(const double *Hs, int nv, int r, int c, int m, int anchor, int shared)
{
    constexpr int DIM = RigSums<B>::DIM;
    const int fr = rig_full_row<B>(r, m, anchor, shared), fc = rig_full_row<B>(c, m, anchor, shared);
    if (fr >= 0 && fc >= 0) return Hs[fr * DIM + fc];
    double t = 0.0;
    if constexpr (B == 4) {
        if (fr < 0 && fc < 0) {
            for (int v = 0; v < nv; ++v)
                for (int w = 0; w < nv; ++w) t += Hs[(4 * v + 3) * DIM + 4 * w + 3];
        } else {
            const int o = fr < 0 ? fc : fr;       // (the full matrix is symmetric bit for bit)
            for (int v = 0; v < nv; ++v) t += Hs[o * DIM + 4 * v + 3];
        }
    }
    return t;
}

// One workgroup of RIG_STEP_THREADS lanes.  Round 0 takes the system at the input cameras and proposes the first trial; every later round judges the trial k_rig_accum
// has just evaluated.  prm.assemble_only: store the assembled cost / H / g and return (ms_rig_accumulate, ms_rig_focal_accumulate).
// LDS, B = 4: the full system Hs (64 x 64) and the solved one A (61 x 61, row stride 61) are 32768 + 29768 bytes; with the two vectors and the scalars 63.6 KB of the
// 64 KB a workgroup may declare.
template <int B> __global__ void __launch_bounds__(RIG_STEP_THREADS) k_rig_step(RigState<B> *__restrict__ st, const RigPair *__restrict__ pairs, int n_pairs,
                                                                                const double *__restrict__ part, RigStepPrm prm)
{
    using S = RigSums<B>;
    constexpr int DIM = S::DIM, RED = S::RED, PART = S::PART;
    constexpr RigSym<B> sym = rig_sym<B>();
    __shared__ double Hs[DIM * DIM], A[RED * RED], gs[DIM], xs[DIM];
    __shared__ double s_cost, s_outl, s_lam;
    __shared__ int s_accept, s_stop, s_reason, s_iters, s_ok;
    if (st->t.stop) return;
    const int tid = threadIdx.x, nv = prm.n_views;
    for (int k = tid; k < DIM * DIM; k += RIG_STEP_THREADS) Hs[k] = 0.0;
    if (tid < DIM) gs[tid] = 0.0;
    __syncthreads();
    // the system, pair after pair: inside a pair every sum goes to a place of its own
    for (int p = 0; p < n_pairs; ++p) {
        if (tid >= S::G_I && tid < S::OUTL) {
            const double v = part[(size_t)p * PART + tid];
            const int iB = B * pairs[p].i, jB = B * pairs[p].j;
            if (tid < S::G_J) gs[iB + tid - S::G_I] += v;
            else if (tid < S::H_II) gs[jB + tid - S::G_J] += v;
            else if (tid < S::H_IJ) {
                const int bB = tid < S::H_JJ ? iB : jB, k = tid < S::H_JJ ? tid - S::H_II : tid - S::H_JJ, r = sym.r[k], c = sym.c[k];
                Hs[(bB + r) * DIM + bB + c] += v;
                if (r != c) Hs[(bB + c) * DIM + bB + r] += v;
            } else {
                const int k = tid - S::H_IJ, r = k / B, c = k % B;
                Hs[(iB + r) * DIM + jB + c] += v;
                Hs[(jB + c) * DIM + iB + r] += v;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double cost = 0.0, outl = 0.0;
        for (int p = 0; p < n_pairs; ++p) { cost += part[(size_t)p * PART]; outl += part[(size_t)p * PART + S::OUTL]; }
        s_cost = cost; s_outl = outl;
    }
    __syncthreads();
    if (prm.assemble_only) {
        for (int k = tid; k < DIM * DIM; k += RIG_STEP_THREADS) st->H[k] = Hs[k];
        if (tid < DIM) st->g[tid] = gs[tid];
        if (tid == 0) st->t.cost = s_cost;
        return;
    }
    // accept or reject, lambda, the stop rules
    if (tid == 0) {
        double lam = st->t.lam;
        int iters = st->t.iters, accept = 1, stop = 0, reason = 0;
        if (st->t.round == 0) st->t.cost0 = s_cost;
        else {
            accept = s_cost <= st->t.cost ? 1 : 0;      // (a NaN cost is a rejected step)
            ++iters;
            if (accept) { lam = fmax(lam / 10.0, 1e-12); if (st->t.dmax < prm.step_tol) { stop = 1; reason = MS_RIG_CONVERGED; } }
            else { lam = 10.0 * lam; if (lam > 1e12) { stop = 1; reason = MS_RIG_STALLED; } }
            if (!stop && iters >= prm.max_iters) { stop = 1; reason = MS_RIG_ITERATION_LIMIT; }
        }
        if (accept) { st->t.cost = s_cost; st->t.outliers = s_outl; }
        s_accept = accept; s_stop = stop; s_reason = reason; s_lam = lam; s_iters = iters;
    }
    __syncthreads();
    if (s_accept) {
        for (int k = tid; k < nv * 9; k += RIG_STEP_THREADS) st->R_cur[k] = st->R_trial[k];
        if constexpr (B == 4) { if (tid < nv) st->f_cur[tid] = st->f_trial[tid]; }
        for (int k = tid; k < DIM * DIM; k += RIG_STEP_THREADS) st->H[k] = Hs[k];
        if (tid < DIM) st->g[tid] = gs[tid];
    } else {
        for (int k = tid; k < DIM * DIM; k += RIG_STEP_THREADS) Hs[k] = st->H[k];
        if (tid < DIM) gs[tid] = st->g[tid];
    }
    __syncthreads();
    // (H + lambda diag H) d = -g over the rotations of the views but the anchor (and the focals); a pivot that is not positive is a rejected step
    const int shared = B == 4 ? prm.shared : 0, anchor = prm.anchor, m = shared ? 3 * (nv - 1) + 1 : B * nv - 3;
    while (!s_stop) {
        const double lam = s_lam;
        for (int k = tid; k < m * m; k += RIG_STEP_THREADS) {
            const int r = k / m, c = k % m;
            if (c > r) continue;                    // the factorisation reads the lower triangle only
            const double hv = rig_entry<B>(Hs, nv, r, c, m, anchor, shared);
            A[r * RED + c] = r == c ? hv + lam * hv : hv;
        }
        if (tid == 0) s_ok = 1;
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            if (tid == 0) { const double d = A[k * RED + k]; if (d > 0.0 && d < HUGE_VAL) A[k * RED + k] = sqrt(d); else s_ok = 0; }
            __syncthreads();
            if (!s_ok) break;
            const double piv = A[k * RED + k];
            for (int i = k + 1 + tid; i < m; i += RIG_STEP_THREADS) A[i * RED + k] /= piv;
            __syncthreads();
            const int t = m - k - 1;                // the trailing t x t block, one element a lane and pass (lower triangle only)
            for (int e = tid; e < t * t; e += RIG_STEP_THREADS) {
                const int i = k + 1 + e / t, j = k + 1 + e % t;
                if (j <= i) A[i * RED + j] -= A[i * RED + k] * A[j * RED + k];
            }
            __syncthreads();
        }
        if (s_ok) {
            // L y = -g, then L^T d = y: column by column, the pivot lane divides and every row still open subtracts the column's share
            if (tid < m) {
                const int fr = rig_full_row<B>(tid, m, anchor, shared);
                double gv = 0.0;
                if (fr >= 0) gv = gs[fr];
                else for (int v = 0; v < nv; ++v) gv += gs[B * v + 3];
                xs[tid] = -gv;
            }
            __syncthreads();
            for (int c = 0; c < m; ++c) {
                if (tid == 0) xs[c] /= A[c * RED + c];
                __syncthreads();
                if (tid > c && tid < m) xs[tid] -= A[tid * RED + c] * xs[c];
                __syncthreads();
            }
            for (int c = m - 1; c >= 0; --c) {
                if (tid == 0) xs[c] /= A[c * RED + c];
                __syncthreads();
                if (tid < c) xs[tid] -= A[c * RED + tid] * xs[c];
                __syncthreads();
            }
            if (tid == 0) {
                double dmax = 0.0;
                for (int r = 0; r < m; ++r) { dmax = fmax(dmax, fabs(xs[r])); if (!(fabs(xs[r]) < HUGE_VAL)) s_ok = 0; }
                st->t.dmax = dmax;
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
        // where view tid's step sits in xs: its B unknowns view after view with the anchor's rotation left out; a shared focal is the last entry
        const int rot = shared ? 3 * (tid - (tid > anchor ? 1 : 0)) : B * tid - (tid > anchor ? 3 : 0);
        if (tid == anchor) { for (int k = 0; k < 9; ++k) st->R_trial[tid * 9 + k] = st->R_cur[tid * 9 + k]; }
        else rig_rotate(&xs[rot], &st->R_cur[tid * 9], &st->R_trial[tid * 9]);
        if constexpr (B == 4) {
            const int foc = shared ? m - 1 : (tid == anchor ? rot : rot + 3);
            st->f_trial[tid] = st->f_cur[tid] * exp(xs[foc]);
        }
    }
    if (tid == 0) { st->t.lam = s_lam; st->t.iters = s_iters; st->t.reason = s_reason; st->t.stop = s_stop; st->t.round = st->t.round + 1; }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
// the warper's backward direction of absolute warper coordinates, turned into the camera by R^T (R^-1 = R^T) and normalised; t: the plane warper's, may be null
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

static double rig_angle(const double *A, const double *B)      // the angle of A B^T
{
    double M[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[r * 3 + c] = A[r * 3] * B[c * 3] + A[r * 3 + 1] * B[c * 3 + 1] + A[r * 3 + 2] * B[c * 3 + 2];
    const double x = M[7] - M[5], y = M[2] - M[6], z = M[3] - M[1];
    return atan2(0.5 * sqrt(x * x + y * y + z * z), 0.5 * (M[0] + M[4] + M[8] - 1.0));
}

// Matches grouped by canonical pair (i < j, a and b swapped where the caller listed (j, i)), pairs in (i, j) order, input order kept inside a pair.  A pair with fewer
// than min_pair matches is left out and counted.  Item: the device's match record, In: the caller's (both carry a[], b[] of the same length).
template <class Item> struct RigGroups { std::vector<RigPair> pairs; std::vector<Item> items; int ignored = 0; };
template <class Item, class In> static RigGroups<Item> rig_group(int n_views, const In *matches, int n, int min_pair)
{
    constexpr int C = sizeof(Item::a) / sizeof(double);
    static_assert(sizeof(In::a) == sizeof(Item::a), "the caller's match and the device's carry the same coordinates");
    std::vector<int> cnt(n_views * n_views, 0), slot(n_views * n_views, -1);
    auto key = [&](const In &m) { return std::min(m.view_a, m.view_b) * n_views + std::max(m.view_a, m.view_b); };
    for (int k = 0; k < n; ++k) ++cnt[key(matches[k])];
    RigGroups<Item> G;
    int off = 0;
    for (int q = 0; q < n_views * n_views; ++q) {
        if (!cnt[q]) continue;
        if (cnt[q] < min_pair) { ++G.ignored; continue; }
        slot[q] = (int)G.pairs.size();
        G.pairs.push_back(RigPair{q / n_views, q % n_views, off, 0});
        off += cnt[q];
    }
    G.items.resize(off);
    for (int k = 0; k < n; ++k) {
        const In &m = matches[k];
        const int s = slot[key(m)];
        if (s < 0) continue;
        RigPair &p = G.pairs[s];
        Item &r = G.items[p.off + p.cnt++];
        const bool swap = m.view_a > m.view_b;
        for (int c = 0; c < C; ++c) { r.a[c] = swap ? m.b[c] : m.a[c]; r.b[c] = swap ? m.a[c] : m.b[c]; }
    }
    return G;
}

// One device block, state | pairs | items | aux | partials (all 8-byte aligned): the first four are laid out in pinned memory and go up in ONE copy.  f: null for
// B = 3; aux: n_aux records of the policy's per-view data, null and 0 where it has none.
template <class P> struct RigDevice { RigState<P::B> *st; RigPair *pairs; typename P::Match *items; typename P::Aux *aux; double *part; };
template <class P> static int rig_upload(const char *fn, const RigGroups<typename P::Match> &G, int n_views, const double *f, const double *R, const typename P::Aux *aux,
                                         int n_aux, RigDevice<P> &D, hipStream_t s)
{
    using State = RigState<P::B>;
    using Item = typename P::Match;
    static_assert(sizeof(Item) % 8 == 0 && (sizeof(typename P::Aux) % 8 == 0 || sizeof(typename P::Aux) == 1), "the block's parts stay 8-byte aligned");
    const size_t np = G.pairs.size(), o_pairs = sizeof(State), o_items = o_pairs + np * sizeof(RigPair), o_aux = o_items + G.items.size() * sizeof(Item),
                 o_part = o_aux + (size_t)n_aux * sizeof(typename P::Aux), total = o_part + np * RigSums<P::B>::PART * sizeof(double);
    char *base = (char *)device_scratch().get(total), *host = (char *)pinned_scratch().get(o_part);
    if (!base || !host) return fail(MS_ERR_NOMEM, "%s: no memory for %zu bytes", fn, total);
    D.st = (State *)base; D.pairs = (RigPair *)(base + o_pairs); D.items = (Item *)(base + o_items); D.aux = (typename P::Aux *)(base + o_aux); D.part = (double *)(base + o_part);
    State *st = (State *)host;
    memset(st, 0, sizeof(State));
    memcpy(st->R_cur, R, sizeof(double) * 9 * n_views); memcpy(st->R_trial, R, sizeof(double) * 9 * n_views);
    if (f) { memcpy(st->f_cur, f, sizeof(double) * n_views); memcpy(st->f_trial, f, sizeof(double) * n_views); }
    st->t.lam = 1e-3;
    memcpy(host + o_pairs, G.pairs.data(), np * sizeof(RigPair));
    memcpy(host + o_items, G.items.data(), G.items.size() * sizeof(Item));
    if (n_aux) memcpy(host + o_aux, aux, (size_t)n_aux * sizeof(typename P::Aux));
    MS_HIP(hipMemcpyAsync(base, host, o_part, hipMemcpyHostToDevice, s));
    return MS_OK;
}

// The parameters of either refinement (the two public structs differ in layout and in the name of the Huber field: each unit checks its struct_size and converts)
struct RigLmParams { int anchor, shared, max_iters, min_pair; double huber, step_tol; };
static int rig_check_params(const char *fn, int n_views, const RigLmParams &p, const char *huber_name)
{
    MS_CHECK(p.anchor >= 0 && p.anchor < n_views, "%s: anchor_view %d outside [0, %d)", fn, p.anchor, n_views);
    MS_CHECK(p.huber >= 0.0 && std::isfinite(p.huber), "%s: %s %g must be finite and not negative", fn, huber_name, p.huber);
    MS_CHECK(p.max_iters >= 1 && p.max_iters <= 1000, "%s: max_iters %d outside [1, 1000]", fn, p.max_iters);
    MS_CHECK(p.step_tol >= 0.0 && std::isfinite(p.step_tol), "%s: step_tol %g must be finite and not negative", fn, p.step_tol);
    MS_CHECK(p.min_pair >= 1, "%s: min_pair_matches %d must be at least 1", fn, p.min_pair);
    return MS_OK;
}

// The normal equations at the given cameras, every pair used: one round with assemble_only, the whole state copied back.  The caller has checked its arguments.
template <class P, class In> static int rig_lm_accumulate(const char *fn, int n_views, const double *f, const double *R, const In *matches, int n, double huber, double *cost,
                                                          double *H, double *g, hipStream_t s, const typename P::Aux *aux = nullptr, int n_aux = 0)
{
    constexpr int B = P::B;
    if (int e = require_device()) return e;
    const RigGroups<typename P::Match> G = rig_group<typename P::Match>(n_views, matches, n, 1);
    RigDevice<P> D;
    if (int e = rig_upload(fn, G, n_views, f, R, aux, n_aux, D, s)) return e;
    std::vector<RigState<B>> host(1);
    RigState<B> &h = host[0];
    const int np = (int)G.pairs.size();
    k_rig_accum<P><<<np, 256, 0, s>>>(D.st, D.pairs, D.items, D.aux, huber, D.part);
    k_rig_step<B><<<1, RIG_STEP_THREADS, 0, s>>>(D.st, D.pairs, np, D.part, RigStepPrm{n_views, 0, 0, 1, 1, 0.0});
    MS_LAUNCH_CHECK();
    MS_HIP(hipMemcpyAsync(&h, D.st, sizeof(RigState<B>), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    const int d = B * n_views;
    *cost = h.t.cost;
    for (int r = 0; r < d; ++r) {
        g[r] = h.g[r];
        for (int c = 0; c < d; ++c) H[r * d + c] = h.H[r * RigSums<B>::DIM + c];
    }
    return MS_OK;
}

// The refinement from the grouping on, the caller having checked its arguments: the connectivity check, the upload, max_iters + 1 rounds of the two kernels enqueued
// at once (both return at their first instruction once the stop flag is set), one copy back of the cameras and one of the tail, and what the two public info structs
// share.  f_in / f_out: null for B = 3.
template <class P, class In, class Info> static int rig_lm_refine(const char *fn, int n_views, const double *f_in, const double *R_in, const In *matches, int n,
                                                                  const RigLmParams &p, double *f_out, double *R_out, Info *info, hipStream_t s,
                                                                  const typename P::Aux *aux = nullptr, int n_aux = 0)
{
    constexpr int B = P::B;
    const RigGroups<typename P::Match> G = rig_group<typename P::Match>(n_views, matches, n, p.min_pair);
    // every view must hang on the anchor through used pairs
    std::vector<char> seen(n_views, 0);
    std::vector<int> todo{p.anchor};
    seen[p.anchor] = 1;
    while (!todo.empty()) {
        const int v = todo.back(); todo.pop_back();
        for (const RigPair &pr : G.pairs) {
            const int o = pr.i == v ? pr.j : pr.j == v ? pr.i : -1;
            if (o >= 0 && !seen[o]) { seen[o] = 1; todo.push_back(o); }
        }
    }
    for (int v = 0; v < n_views; ++v)
        MS_CHECK(seen[v], "%s: view %d is not connected to the anchor view %d by pairs of at least %d matches (%d pairs ignored)", fn, v, p.anchor, p.min_pair, G.ignored);
    if (int e = require_device()) return e;

    RigDevice<P> D;
    if (int e = rig_upload(fn, G, n_views, f_in, R_in, aux, n_aux, D, s)) return e;
    const RigStepPrm sp{n_views, p.anchor, p.shared, p.max_iters, 0, p.step_tol};
    const int np = (int)G.pairs.size();
    for (int round = 0; round <= p.max_iters; ++round) {
        k_rig_accum<P><<<np, 256, 0, s>>>(D.st, D.pairs, D.items, D.aux, p.huber, D.part);
        k_rig_step<B><<<1, RIG_STEP_THREADS, 0, s>>>(D.st, D.pairs, np, D.part, sp);
    }
    MS_LAUNCH_CHECK();
    static_assert(offsetof(RigState<B>, f_cur) == sizeof(double) * 9 * MS_MAX_VIEWS, "f_cur follows R_cur: the two come back in one copy");
    RigTail tail;
    std::vector<double> cam(10 * MS_MAX_VIEWS);
    MS_HIP(hipMemcpyAsync(cam.data(), D.st->R_cur, sizeof(double) * (B == 4 ? 10 * MS_MAX_VIEWS : 9 * n_views), hipMemcpyDeviceToHost, s));
    MS_HIP(hipMemcpyAsync(&tail, &D.st->t, sizeof(tail), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    if (!tail.stop) return fail(MS_ERR_HIP, "%s: the device loop ended without a stop reason (round %d, %d iterations)", fn, tail.round, tail.iters);
    memcpy(R_out, cam.data(), sizeof(double) * 9 * n_views);
    if (f_out) memcpy(f_out, cam.data() + 9 * MS_MAX_VIEWS, sizeof(double) * n_views);
    if (info) {
        info->iterations = tail.iters; info->stop_reason = tail.reason;
        info->cost_initial = tail.cost0; info->cost_final = tail.cost;
        info->matches_used = (int)G.items.size(); info->pairs_used = np; info->pairs_ignored = G.ignored;
        info->outliers = (int)tail.outliers;
        info->max_rotation_rad = 0.0;
        for (int v = 0; v < n_views; ++v) info->max_rotation_rad = std::max(info->max_rotation_rad, rig_angle(R_out + 9 * v, R_in + 9 * v));
    }
    return MS_OK;
}

// What ms_refine_rig and ms_refine_rig_focals share: the context must have cameras of its own ...
static int rig_ctx_check(const char *fn, const ms_ctx *c)
{
    if (!c->maps_built) return fail(MS_ERR_STATE, "%s: call ms_build_maps first (the matches are pixels of the views it lays out)", fn);
    if (c->custom_maps && !c->lens_maps)
        return fail(MS_ERR_UNSUPPORTED, "%s: the context's maps are the caller's own (ms_set_maps): it has no cameras to refine", fn);
    return MS_OK;
}

// ... and the walk over its match lists: R (9 N doubles) gets the context's rotations and out one match of the unit's public type for each of the lists', its views
// set; fill(out[k], q, ra, rb) turns the two camera rays of the match, the q-th of view out[k].view_a, into its coordinates or refuses it.
// View pixel + ROI corner = the absolute warper coordinate, in double; the plane warper's t is zero in a context.
template <class Out, class Fill> static int rig_ctx_matches(const char *fn, const ms_ctx *c, const ms_mesh_match *matches, const int *match_count, std::vector<double> &R,
                                                            std::vector<Out> &out, Fill fill)
{
    const int N = c->N;
    long long total = 0;
    for (int v = 0; v < N; ++v) { MS_CHECK(match_count[v] >= 0, "%s: match_count[%d] = %d", fn, v, match_count[v]); total += match_count[v]; }
    MS_CHECK(total >= 1 && total <= RIG_MAX_MATCHES, "%s: %lld matches outside [1, %d]", fn, total, RIG_MAX_MATCHES);
    R.resize(9 * N);
    for (int v = 0; v < N; ++v)
        for (int k = 0; k < 9; ++k) R[9 * v + k] = (double)c->R[v][k];
    out.resize((size_t)total);
    const double scale = (double)c->cfg.warp_scale;
    size_t k = 0;
    for (int v = 0; v < N; ++v)
        for (int q = 0; q < match_count[v]; ++q, ++k) {
            const ms_mesh_match &m = matches[k];
            MS_CHECK(m.dst >= 0 && m.dst < N && m.dst != v, "%s: match %d of view %d names view %d", fn, q, v, m.dst);
            MS_CHECK(std::isfinite(m.x1) && std::isfinite(m.y1) && std::isfinite(m.x2) && std::isfinite(m.y2), "%s: match %d of view %d is not finite", fn, q, v);
            double ra[3], rb[3];
            warper_ray(c->cfg.projection, scale, nullptr, &R[9 * v], (double)c->roi[v].x + (double)m.x1, (double)c->roi[v].y + (double)m.y1, ra);
            warper_ray(c->cfg.projection, scale, nullptr, &R[9 * m.dst], (double)c->roi[m.dst].x + (double)m.x2, (double)c->roi[m.dst].y + (double)m.y2, rb);
            out[k].view_a = v; out[k].view_b = m.dst;
            if (int e = fill(out[k], q, ra, rb)) return e;
        }
    return MS_OK;
}

}  // namespace ms
