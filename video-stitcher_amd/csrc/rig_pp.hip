// rig_pp.hip -- self-calibrating lens rigs, the principal points included: rotations, focals and the offset (ox, oy) of every view's principal point from the point its
// pixels are centred on, from feature matches on source pixels behind fixed lenses (include/ms_stitch.h, "Self-calibrating rigs", the centre form).  What
// detail::BundleAdjusterReproj (OCV/stitching/src/motion_estimators.cpp) estimates beside the focal.  Calibration-time work: the per-frame path never runs anything of
// this unit.  Everything is double; -ffp-contract=off as in rig_focal.hip.
// This unit holds the policy RigPpPixels (6 unknowns a view: RigLensPixels' ray code from rig_px.hpp on the pixel with the trial offset subtracted, then two more
// columns a view and the 92 sums of RigSums<6>), the state of that form (RigState<6>, which carries the offsets and a packed system), a step kernel of its own (the
// 96 x 96 system does not fit k_rig_step's LDS layout, and the prior is added here) and the entry points.  k_rig_accum<RigPpPixels> is rig_lm.hpp's kernel as it
// stands, so the per-lane order, the butterfly and the wave fold are the siblings'; grouping, parameter checks and the walk over a context's lists are rig_lm.hpp's
// and rig_px.hpp's.  Nothing here is seen by rig.o, rig_focal.o, rig_lens.o or rig_coeffs.o.
#include <type_traits>
#include "rig_px.hpp"

namespace ms {

constexpr int RIGP_B = 6;
constexpr int RIGP_DIM = RigSums<RIGP_B>::DIM;                 // 96 rows of the full system: view v at 6v .. 6v + 5, (delta0, delta1, delta2, s, ox, oy)
constexpr int RIGP_TRI = RIGP_DIM * (RIGP_DIM + 1) / 2;        // its lower triangle, packed: row r at r (r + 1) / 2
constexpr int RIGP_RED = RIGP_DIM - 3;                         // the largest system solved: 93

// The device-resident state of the centre form: RigState's members (k_rig_accum reads R_trial and the tail), the offsets beside the focals, and the system at the
// accepted cameras as a packed lower triangle.
template <> struct RigState<RIGP_B> {
    double R_cur[MS_MAX_VIEWS * 9], f_cur[MS_MAX_VIEWS], pp_cur[MS_MAX_VIEWS * 2];          // the last accepted cameras: they come back in one copy
    double R_trial[MS_MAX_VIEWS * 9], f_trial[MS_MAX_VIEWS], pp_trial[MS_MAX_VIEWS * 2];    // what k_rig_accum evaluates
    double pp_in[MS_MAX_VIEWS * 2];                                                         // what the prior pulls towards
    double H[RIGP_TRI], g[RIGP_DIM];
    RigTail t;
};
using RigPpState = RigState<RIGP_B>;
// What rig_lm.hpp's k_rig_accum and RigDevice take from a state: the trial rotations and the tail.  A change of the primary template that makes the kernel read
// anything else has to be followed here.  (RigSums<6>::RED counts a focal row for B == 4 only and is not used by this unit: RIGP_RED is.)
static_assert(std::is_same<decltype(RigPpState::R_trial), double[MS_MAX_VIEWS * 9]>::value && std::is_same<decltype(RigPpState::t), RigTail>::value &&
              std::is_same<decltype(RigState<4>::R_trial), decltype(RigPpState::R_trial)>::value && std::is_same<decltype(RigState<4>::t), decltype(RigPpState::t)>::value,
              "RigState<6> keeps the members k_rig_accum reads as the primary template declares them");

struct RigPpStepPrm { int n_views, anchor, shared, max_iters, assemble_only; double step_tol, prior; };

// m (R d)_k, (R d)_k = R[3k] d0 + R[3k+1] d1 + R[3k+2] d2
static __device__ __forceinline__ void rigpp_column(double m, const double *R, double d0, double d1, double d2, double *c)
{
    c[0] = m * (R[0] * d0 + R[1] * d1 + R[2] * d2); c[1] = m * (R[3] * d0 + R[4] * d1 + R[5] * d2); c[2] = m * (R[6] * d0 + R[7] * d1 + R[8] * d2);
}

struct RigPpPixels {
    using Match = RigfPx;
    using Aux = LensDist;                         // one a view
    static constexpr int B = RIGP_B;
    struct Cams { LensDist li, lj; double fi, fj, m, oi[2], oj[2]; };
    static __device__ __forceinline__ Cams load(const RigPpState *st, const RigPair &pr, const LensDist *lenses)
    {
        const double fi = st->f_trial[pr.i], fj = st->f_trial[pr.j], m = sqrt(fi * fj);
        return Cams{lenses[pr.i], lenses[pr.j], fi, fj, m, {st->pp_trial[2 * pr.i], st->pp_trial[2 * pr.i + 1]}, {st->pp_trial[2 * pr.j], st->pp_trial[2 * pr.j + 1]}};
    }
    // One view's side of a match at the centred pixel px (the offset already subtracted): p = R a and t = m R da/ds by RigLensPixels::view's expressions to the letter,
    // and ex = m R da/dox, ey = m R da/doy (include/ms_stitch.h).  false: the lens does not see the pixel at this focal.
    static __device__ __forceinline__ bool view(const LensDist &l, double f, double m, const double *R, const double *px, double *p, double *t, double *ex, double *ey)
    {
        if (l.model == MS_LENS_NONE) {
            const double na = sqrt(px[0] * px[0] + px[1] * px[1] + f * f);
            const double a0 = px[0] / na, a1 = px[1] / na, a2 = f / na;
            p[0] = R[0] * a0 + R[1] * a1 + R[2] * a2; p[1] = R[3] * a0 + R[4] * a1 + R[5] * a2; p[2] = R[6] * a0 + R[7] * a1 + R[8] * a2;
            const double ma = m * a2;
            t[0] = ma * (R[2] - a2 * p[0]); t[1] = ma * (R[5] - a2 * p[1]); t[2] = ma * (R[8] - a2 * p[2]);
            const double xy = (a0 * a1) / na;
            rigpp_column(m, R, -((1.0 - a0 * a0) / na), xy, (a0 * a2) / na, ex);
            rigpp_column(m, R, xy, -((1.0 - a1 * a1) / na), (a1 * a2) / na, ey);
            return true;
        }
        RigLensRay o;
        if (!rig_lens_ray(l, f, px, o)) return false;
        rig_lens_rotate(m, R, o, p, t);
        double A0[3], A1[3];                          // the columns of d a / d (xd, yd)
        if (l.model == MS_LENS_FISHEYE) {
            if (o.centre) { A0[0] = 1.0; A0[1] = 0.0; A0[2] = 0.0; A1[0] = 0.0; A1[1] = 1.0; A1[2] = 0.0; }
            else {
                const double td = hypot(px[0] / f, px[1] / f), g = o.st / td, c0 = o.e0 / o.slope, c1 = o.e1 / o.slope, s0 = o.e1 * g, s1 = o.e0 * g;
                A0[0] = c0 * (o.ct * o.e0) + s0 * o.e1; A0[1] = c0 * (o.ct * o.e1) - s0 * o.e0; A0[2] = -(c0 * o.st);
                A1[0] = c1 * (o.ct * o.e0) - s1 * o.e1; A1[1] = c1 * (o.ct * o.e1) + s1 * o.e0; A1[2] = -(c1 * o.st);
            }
        } else {
            const double x0 = o.J[3] / o.det, y0 = -(o.J[2] / o.det), x1 = -(o.J[1] / o.det), y1 = o.J[0] / o.det;      // the columns of J^-1
            const double t0 = o.a0 * x0 + o.a1 * y0, t1 = o.a0 * x1 + o.a1 * y1;
            A0[0] = (x0 - o.a0 * t0) / o.n; A0[1] = (y0 - o.a1 * t0) / o.n; A0[2] = -(o.a2 * t0) / o.n;
            A1[0] = (x1 - o.a0 * t1) / o.n; A1[1] = (y1 - o.a1 * t1) / o.n; A1[2] = -(o.a2 * t1) / o.n;
        }
        rigpp_column(m, R, -(A0[0] / f), -(A0[1] / f), -(A0[2] / f), ex);
        rigpp_column(m, R, -(A1[0] / f), -(A1[1] / f), -(A1[2] / f), ey);
        return true;
    }
    // (x x y)_k and x . y as rig_px_sums writes them
    static __device__ __forceinline__ double cross(const double *x, const double *y, int k)
    {
        return k == 0 ? x[1] * y[2] - x[2] * y[1] : k == 1 ? x[2] * y[0] - x[0] * y[2] : x[0] * y[1] - x[1] * y[0];
    }
    static __device__ __forceinline__ double dot(const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }
    static constexpr int tri(int r, int c) { return r * B - r * (r - 1) / 2 + (c - r); }      // (r, c), c >= r, in a stored upper triangle
    // The 92 terms of one match in the header's order.  ci[n], cj[n]: the residual's columns by (s, ox, oy) of view i and of view j.  The 46 among them that involve
    // the rotations and the focals only are rig_px_sums' expressions.
    static __device__ __forceinline__ void sums(const RigPxResidual &e, const double (&ci)[3][3], const double (&cj)[3][3], double *acc)
    {
        using S = RigSums<B>;
        const double u[3] = {e.u0, e.u1, e.u2}, v[3] = {e.v0, e.v1, e.v2}, r[3] = {e.r0, e.r1, e.r2}, w = e.w;
        acc[0] += e.rho;
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[S::G_I + k] += w * cross(u, r, k); acc[S::G_J + k] += -(w * cross(v, r, k)); }
#pragma unroll
        for (int n = 0; n < 3; ++n) { acc[S::G_I + 3 + n] += w * dot(ci[n], r); acc[S::G_J + 3 + n] += w * dot(cj[n], r); }
        // H_ii and H_jj: rotation by rotation, rotation by column (H_jj's negated), column by column
        acc[S::H_II + tri(0, 0)] += w * (u[1] * u[1] + u[2] * u[2]); acc[S::H_II + tri(0, 1)] += -(w * (u[0] * u[1])); acc[S::H_II + tri(0, 2)] += -(w * (u[0] * u[2]));
        acc[S::H_II + tri(1, 1)] += w * (u[0] * u[0] + u[2] * u[2]); acc[S::H_II + tri(1, 2)] += -(w * (u[1] * u[2]));
        acc[S::H_II + tri(2, 2)] += w * (u[0] * u[0] + u[1] * u[1]);
        acc[S::H_JJ + tri(0, 0)] += w * (v[1] * v[1] + v[2] * v[2]); acc[S::H_JJ + tri(0, 1)] += -(w * (v[0] * v[1])); acc[S::H_JJ + tri(0, 2)] += -(w * (v[0] * v[2]));
        acc[S::H_JJ + tri(1, 1)] += w * (v[0] * v[0] + v[2] * v[2]); acc[S::H_JJ + tri(1, 2)] += -(w * (v[1] * v[2]));
        acc[S::H_JJ + tri(2, 2)] += w * (v[0] * v[0] + v[1] * v[1]);
#pragma unroll
        for (int n = 0; n < 3; ++n) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { acc[S::H_II + tri(k, 3 + n)] += w * cross(u, ci[n], k); acc[S::H_JJ + tri(k, 3 + n)] += -(w * cross(v, cj[n], k)); }
#pragma unroll
            for (int c = n; c < 3; ++c) { acc[S::H_II + tri(3 + n, 3 + c)] += w * dot(ci[n], ci[c]); acc[S::H_JJ + tri(3 + n, 3 + c)] += w * dot(cj[n], cj[c]); }
        }
        // H_ij, rows of view i
        acc[S::H_IJ + 0 * B + 0] += -(w * (u[1] * v[1] + u[2] * v[2])); acc[S::H_IJ + 0 * B + 1] += w * (v[0] * u[1]); acc[S::H_IJ + 0 * B + 2] += w * (v[0] * u[2]);
        acc[S::H_IJ + 1 * B + 0] += w * (v[1] * u[0]); acc[S::H_IJ + 1 * B + 1] += -(w * (u[0] * v[0] + u[2] * v[2])); acc[S::H_IJ + 1 * B + 2] += w * (v[1] * u[2]);
        acc[S::H_IJ + 2 * B + 0] += w * (v[2] * u[0]); acc[S::H_IJ + 2 * B + 1] += w * (v[2] * u[1]); acc[S::H_IJ + 2 * B + 2] += -(w * (u[0] * v[0] + u[1] * v[1]));
#pragma unroll
        for (int n = 0; n < 3; ++n) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { acc[S::H_IJ + k * B + 3 + n] += w * cross(u, cj[n], k); acc[S::H_IJ + (3 + n) * B + k] += -(w * cross(v, ci[n], k)); }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[S::H_IJ + (3 + n) * B + 3 + c] += w * dot(ci[n], cj[c]);
        }
        acc[S::OUTL] += e.out;
    }
    // The terms of one match.  A pixel its lens does not see at the trial cameras and offsets: +infinity to the cost and nothing to any other sum.
    static __device__ __forceinline__ void terms(const double *Ri, const double *Rj, const Cams &cams, const RigfPx &px, double h, double *acc)
    {
        const double pa[2] = {px.a[0] - cams.oi[0], px.a[1] - cams.oi[1]}, pb[2] = {px.b[0] - cams.oj[0], px.b[1] - cams.oj[1]};
        double p[3], q[3], ti[3], tj[3], ci[3][3], cj[3][3];
        const bool seen_i = view(cams.li, cams.fi, cams.m, Ri, pa, p, ti, ci[1], ci[2]), seen_j = view(cams.lj, cams.fj, cams.m, Rj, pb, q, tj, cj[1], cj[2]);
        if (!seen_i || !seen_j) { acc[0] += HUGE_VAL; return; }
        const RigPxResidual e = rig_px_residual(cams.m, p[0], p[1], p[2], q[0], q[1], q[2], h);
        ci[0][0] = 0.5 * e.r0 + ti[0]; ci[0][1] = 0.5 * e.r1 + ti[1]; ci[0][2] = 0.5 * e.r2 + ti[2];
        cj[0][0] = 0.5 * e.r0 - tj[0]; cj[0][1] = 0.5 * e.r1 - tj[1]; cj[0][2] = 0.5 * e.r2 - tj[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) { cj[1][k] = -cj[1][k]; cj[2][k] = -cj[2][k]; }      // r = m (p - q): view j's columns carry the sign
        sums(e, ci, cj, acc);
    }
};

// ---- k_rigpp_step -------------------------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ int rigpp_at(int r, int c) { return r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r; }

// Row r of the solved system (m rows) as a row of the full one.  Per-view focals: the anchor's three rotation rows are dropped.  A shared focal: (delta, ox, oy) view
// after view with the anchor's rotation left out, and -1 for the last row, the one focal (the sum of every view's focal row).
static __device__ __forceinline__ int rigpp_full_row(int r, int m, int anchor, int shared)
{
    if (!shared) return r + (r >= RIGP_B * anchor ? 3 : 0);
    if (r == m - 1) return -1;
    const int a5 = 5 * anchor;
    if (r >= a5 && r < a5 + 2) return RIGP_B * anchor + 4 + (r - a5);
    const int q = r < a5 ? r : r - a5 - 2, v = q / 5 + (r < a5 ? 0 : anchor + 1), k = q % 5;
    return RIGP_B * v + (k < 3 ? k : k + 1);
}

// entry (fr, fc) of the solved system from the packed full one; fold[o]: row o of the full system summed over the focal columns of the views in order, ff: the
// focal rows of fold summed in view order (both made once a round, shared focal only)
static __device__ __forceinline__ double rigpp_entry(const double *H, const double *fold, double ff, int fr, int fc)
{
    if (fr >= 0 && fc >= 0) return H[rigpp_at(fr, fc)];
    return fr < 0 && fc < 0 ? ff : fold[fr < 0 ? fc : fr];
}

// k_rig_step's rule for 6 unknowns a view, one workgroup of RIG_STEP_THREADS lanes: the same assembly in pair order, accept rule, lambda rule, stop rules and
// Cholesky.  What is its own: the full system is assembled as ONE packed triangle in LDS (96 * 97 / 2 doubles, 37.2 KB), gets the prior, and goes to the state in
// global memory where the trial is accepted; after a barrier the damped, reduced and focal-folded system is built from the state's triangle into the same LDS and
// factored packed in place; with a shared focal the focal rows are folded once a round into LDS (fold, s_ff), not at every lambda retry.  39.6 KB of LDS with the vectors, inside the 64 KB a workgroup may declare.  step_tol sees the centre steps divided by the focal.
__global__ void __launch_bounds__(RIG_STEP_THREADS) k_rigpp_step(RigPpState *st, const RigPair *__restrict__ pairs, int n_pairs, const double *__restrict__ part,
                                                                 RigPpStepPrm prm)
{
    using S = RigSums<RIGP_B>;
    constexpr int B = RIGP_B, DIM = RIGP_DIM, PART = S::PART;
    constexpr RigSym<B> sym = rig_sym<B>();
    static_assert(RIGP_RED * (RIGP_RED + 1) / 2 <= RIGP_TRI, "the packed factor fits where the packed full system was");
    __shared__ double A[RIGP_TRI], gs[DIM], xs[DIM], fold[DIM];
    __shared__ double s_cost, s_outl, s_lam, s_ff;
    __shared__ int s_accept, s_stop, s_reason, s_iters, s_ok;
    if (st->t.stop) return;
    const int tid = threadIdx.x, nv = prm.n_views;
    for (int k = tid; k < RIGP_TRI; k += RIG_STEP_THREADS) A[k] = 0.0;
    if (tid < DIM) gs[tid] = 0.0;
    __syncthreads();
    // the system, pair after pair: inside a pair every sum goes to a place of its own (i < j: H_ij lies below the diagonal as H_ji)
    for (int p = 0; p < n_pairs; ++p) {
        if (tid >= S::G_I && tid < S::OUTL) {
            const double v = part[(size_t)p * PART + tid];
            const int iB = B * pairs[p].i, jB = B * pairs[p].j;
            if (tid < S::G_J) gs[iB + tid - S::G_I] += v;
            else if (tid < S::H_II) gs[jB + tid - S::G_J] += v;
            else if (tid < S::H_IJ) {
                const int bB = tid < S::H_JJ ? iB : jB, k = tid < S::H_JJ ? tid - S::H_II : tid - S::H_JJ;
                A[rigpp_at(bB + sym.c[k], bB + sym.r[k])] += v;
            } else {
                const int k = tid - S::H_IJ;
                A[rigpp_at(jB + k % B, iB + k / B)] += v;
            }
        }
        __syncthreads();
    }
    const bool prior = !prm.assemble_only && prm.prior > 0.0;
    if (tid == 0) {
        double cost = 0.0, outl = 0.0;
        for (int p = 0; p < n_pairs; ++p) { cost += part[(size_t)p * PART]; outl += part[(size_t)p * PART + S::OUTL]; }
        if (prior) {
            double q = 0.0;
            for (int v = 0; v < nv; ++v) {
                const double dx = st->pp_trial[2 * v] - st->pp_in[2 * v], dy = st->pp_trial[2 * v + 1] - st->pp_in[2 * v + 1];
                q += dx * dx + dy * dy;
            }
            cost += prm.prior * q;
        }
        s_cost = cost; s_outl = outl;
    }
    if (prior && tid < 2 * nv) {
        const int row = B * (tid >> 1) + 4 + (tid & 1);
        A[rigpp_at(row, row)] += prm.prior;
        gs[row] += prm.prior * (st->pp_trial[tid] - st->pp_in[tid]);
    }
    __syncthreads();
    if (prm.assemble_only) {
        for (int k = tid; k < RIGP_TRI; k += RIG_STEP_THREADS) st->H[k] = A[k];
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
        if (tid < nv) st->f_cur[tid] = st->f_trial[tid];
        if (tid < 2 * nv) st->pp_cur[tid] = st->pp_trial[tid];
        for (int k = tid; k < RIGP_TRI; k += RIG_STEP_THREADS) st->H[k] = A[k];
        if (tid < DIM) st->g[tid] = gs[tid];
    } else if (tid < DIM) gs[tid] = st->g[tid];
    __threadfence_block();
    __syncthreads();                                // from here on A is the solved system; the full one is the state's
    // (H + lambda diag H) d = -g over the rotations of the views but the anchor, the focals and the centres; a pivot that is not positive is a rejected step
    const int shared = prm.shared, anchor = prm.anchor, m = shared ? 5 * nv - 2 : B * nv - 3;
    auto at = [](int r, int c) { return r * (r + 1) / 2 + c; };      // c <= r
    if (shared) {
        // the focal fold of the accepted system, once a round: every lambda retry below reads it from LDS
        if (tid < B * nv) {
            double t = 0.0;
            for (int v = 0; v < nv; ++v) t += st->H[rigpp_at(tid, B * v + 3)];
            fold[tid] = t;
        }
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int v = 0; v < nv; ++v) t += fold[B * v + 3];
            s_ff = t;
        }
        __syncthreads();
    }
    while (!s_stop) {
        const double lam = s_lam;
        for (int k = tid; k < m * m; k += RIG_STEP_THREADS) {
            const int r = k / m, c = k % m;
            if (c > r) continue;
            const double hv = rigpp_entry(st->H, fold, s_ff, rigpp_full_row(r, m, anchor, shared), rigpp_full_row(c, m, anchor, shared));
            A[at(r, c)] = r == c ? hv + lam * hv : hv;
        }
        if (tid == 0) s_ok = 1;
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            if (tid == 0) { const double d = A[at(k, k)]; if (d > 0.0 && d < HUGE_VAL) A[at(k, k)] = sqrt(d); else s_ok = 0; }
            __syncthreads();
            if (!s_ok) break;
            const double piv = A[at(k, k)];
            for (int i = k + 1 + tid; i < m; i += RIG_STEP_THREADS) A[at(i, k)] /= piv;
            __syncthreads();
            const int t = m - k - 1;                // the trailing t x t block, one element a lane and pass (lower triangle only)
            for (int e = tid; e < t * t; e += RIG_STEP_THREADS) {
                const int i = k + 1 + e / t, j = k + 1 + e % t;
                if (j <= i) A[at(i, j)] -= A[at(i, k)] * A[at(j, k)];
            }
            __syncthreads();
        }
        if (s_ok) {
            // L y = -g, then L^T d = y: column by column, the pivot lane divides and every row still open subtracts the column's share
            if (tid < m) {
                const int fr = rigpp_full_row(tid, m, anchor, shared);
                double gv = 0.0;
                if (fr >= 0) gv = gs[fr];
                else for (int v = 0; v < nv; ++v) gv += gs[B * v + 3];
                xs[tid] = -gv;
            }
            __syncthreads();
            for (int c = 0; c < m; ++c) {
                if (tid == 0) xs[c] /= A[at(c, c)];
                __syncthreads();
                if (tid > c && tid < m) xs[tid] -= A[at(tid, c)] * xs[c];
                __syncthreads();
            }
            for (int c = m - 1; c >= 0; --c) {
                if (tid == 0) xs[c] /= A[at(c, c)];
                __syncthreads();
                if (tid < c) xs[tid] -= A[at(c, tid)] * xs[c];
                __syncthreads();
            }
            if (tid == 0) {
                double dmax = 0.0;
                for (int r = 0; r < m; ++r) {
                    if (!(fabs(xs[r]) < HUGE_VAL)) s_ok = 0;
                    const int fr = rigpp_full_row(r, m, anchor, shared);
                    dmax = fmax(dmax, fr >= 0 && fr % B >= 4 ? fabs(xs[r]) / st->f_cur[fr / B] : fabs(xs[r]));      // a centre step in radians
                }
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
        // where view tid's step sits in xs: its unknowns view after view with the anchor's rotation left out; a shared focal is the last entry
        const int per = shared ? 5 : B, base = per * tid - (tid > anchor ? 3 : 0), rot = tid == anchor ? 0 : 3;
        if (tid == anchor) { for (int k = 0; k < 9; ++k) st->R_trial[tid * 9 + k] = st->R_cur[tid * 9 + k]; }
        else rig_rotate(&xs[base], &st->R_cur[tid * 9], &st->R_trial[tid * 9]);
        const int foc = shared ? m - 1 : base + rot, cen = shared ? base + rot : base + rot + 1;
        st->f_trial[tid] = st->f_cur[tid] * exp(xs[foc]);
        st->pp_trial[2 * tid] = st->pp_cur[2 * tid] + xs[cen]; st->pp_trial[2 * tid + 1] = st->pp_cur[2 * tid + 1] + xs[cen + 1];
    }
    if (tid == 0) { st->t.lam = s_lam; st->t.iters = s_iters; st->t.reason = s_reason; st->t.stop = s_stop; st->t.round = st->t.round + 1; }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
// the caller's lenses, each through ms_lens_check, as the device takes them; null: every view is MS_LENS_NONE
static int rigpp_lenses(const char *fn, int n_views, const ms_lens *lenses, std::vector<LensDist> &L)
{
    L.resize(n_views);
    for (int v = 0; v < n_views; ++v) {
        if (lenses) { if (int e = lens_check(fn, &lenses[v])) return e; }
        L[v] = lens_dist(lenses ? &lenses[v] : nullptr);
    }
    return MS_OK;
}

static int rigpp_check_offsets(const char *fn, int n_views, const double *pp)
{
    MS_CHECK(pp, "%s: null offsets", fn);
    for (int v = 0; v < n_views; ++v)
        MS_CHECK(std::isfinite(pp[2 * v]) && std::isfinite(pp[2 * v + 1]), "%s: principal point offset of view %d (%g, %g) is not finite", fn, v, pp[2 * v], pp[2 * v + 1]);
    return MS_OK;
}

// every pixel must be seen through its lens at the input focals and offsets (cameras, offsets and matches have been checked)
static int rigpp_check_seen(const char *fn, const double *f, const double *pp, const LensDist *L, const ms_rig_px_match *matches, int n)
{
    for (int k = 0; k < n; ++k) {
        const ms_rig_px_match &m = matches[k];
        for (int side = 0; side < 2; ++side) {
            const int v = side ? m.view_b : m.view_a;
            const double *px = side ? m.b : m.a, x = px[0] - pp[2 * v], y = px[1] - pp[2 * v + 1];
            LensCam cam{};
            cam.k00 = f[v]; cam.k11 = f[v];
            double ray[3];
            MS_CHECK(lens_unproject(cam, L[v], x, y, ray), "%s: match %d: the lens of view %d does not see the centred pixel (%g, %g) at the focal %g and the offset (%g, %g)", fn,
                     k, v, px[0], px[1], f[v], pp[2 * v], pp[2 * v + 1]);
        }
    }
    return MS_OK;
}

// One device block, state | pairs | items | lenses | partials: the first four are laid out in pinned memory and go up in ONE copy.
static int rigpp_upload(const char *fn, const RigGroups<RigfPx> &G, int n_views, const double *f, const double *R, const double *pp, const LensDist *L,
                        RigDevice<RigPpPixels> &D, hipStream_t s)
{
    static_assert(sizeof(RigPpState) % 8 == 0 && sizeof(RigPair) % 8 == 0 && sizeof(RigfPx) % 8 == 0 && sizeof(LensDist) % 8 == 0, "the block's parts stay 8-byte aligned");
    const size_t np = G.pairs.size(), o_pairs = sizeof(RigPpState), o_items = o_pairs + np * sizeof(RigPair), o_aux = o_items + G.items.size() * sizeof(RigfPx),
                 o_part = o_aux + (size_t)n_views * sizeof(LensDist), total = o_part + np * RigSums<RIGP_B>::PART * sizeof(double);
    char *base = (char *)device_scratch().get(total), *host = (char *)pinned_scratch().get(o_part);
    if (!base || !host) return fail(MS_ERR_NOMEM, "%s: no memory for %zu bytes", fn, total);
    D.st = (RigPpState *)base; D.pairs = (RigPair *)(base + o_pairs); D.items = (RigfPx *)(base + o_items); D.aux = (LensDist *)(base + o_aux); D.part = (double *)(base + o_part);
    RigPpState *st = (RigPpState *)host;
    memset(st, 0, sizeof(RigPpState));
    memcpy(st->R_cur, R, sizeof(double) * 9 * n_views); memcpy(st->R_trial, R, sizeof(double) * 9 * n_views);
    memcpy(st->f_cur, f, sizeof(double) * n_views); memcpy(st->f_trial, f, sizeof(double) * n_views);
    memcpy(st->pp_cur, pp, sizeof(double) * 2 * n_views); memcpy(st->pp_trial, pp, sizeof(double) * 2 * n_views); memcpy(st->pp_in, pp, sizeof(double) * 2 * n_views);
    st->t.lam = 1e-3;
    memcpy(host + o_pairs, G.pairs.data(), np * sizeof(RigPair));
    memcpy(host + o_items, G.items.data(), G.items.size() * sizeof(RigfPx));
    memcpy(host + o_aux, L, (size_t)n_views * sizeof(LensDist));
    MS_HIP(hipMemcpyAsync(base, host, o_part, hipMemcpyHostToDevice, s));
    return MS_OK;
}

static void rigpp_round(const RigDevice<RigPpPixels> &D, int np, double huber, const RigPpStepPrm &sp, hipStream_t s)
{
    k_rig_accum<RigPpPixels><<<np, 256, 0, s>>>(D.st, D.pairs, D.items, D.aux, huber, D.part);
    k_rigpp_step<<<1, RIG_STEP_THREADS, 0, s>>>(D.st, D.pairs, np, D.part, sp);
}

// every check of ms_refine_rig_pp, then rig_lm_refine's frame around this unit's two kernels
static int rigpp_refine(const char *fn, int n_views, const double *f_in, const double *R_in, const double *pp_in, const ms_lens *lenses, const ms_rig_px_match *matches,
                        int n, const ms_rig_pp_params *prm, double *f_out, double *R_out, double *pp_out, ms_rig_pp_info *info, hipStream_t s)
{
    std::vector<LensDist> L;
    if (int e = rigf_check_cameras(fn, n_views, f_in, R_in)) return e;
    if (int e = rigpp_lenses(fn, n_views, lenses, L)) return e;
    if (int e = rigpp_check_offsets(fn, n_views, pp_in)) return e;
    if (int e = rigf_check_matches(fn, n_views, matches, n)) return e;
    MS_CHECK(f_out && R_out && pp_out, "%s: null output", fn);
    MS_CHECK(prm, "%s: null params", fn);
    MS_CHECK(prm->struct_size == sizeof(ms_rig_pp_params), "%s: params.struct_size %u, this library's ms_rig_pp_params has %zu bytes", fn, prm->struct_size,
             sizeof(ms_rig_pp_params));
    const RigLmParams p{prm->anchor_view, prm->shared_focal ? 1 : 0, prm->max_iters, prm->min_pair_matches, prm->huber_px, prm->step_tol};
    if (int e = rig_check_params(fn, n_views, p, "huber_px")) return e;
    MS_CHECK(prm->pp_prior >= 0.0 && std::isfinite(prm->pp_prior), "%s: pp_prior %g must be finite and not negative", fn, prm->pp_prior);
    if (prm->shared_focal)
        for (int v = 1; v < n_views; ++v)
            MS_CHECK(f_in[v] == f_in[0], "%s: shared_focal asks for equal input focals; view %d has %.17g, view 0 has %.17g", fn, v, f_in[v], f_in[0]);
    if (int e = rigpp_check_seen(fn, f_in, pp_in, L.data(), matches, n)) return e;

    const RigGroups<RigfPx> G = rig_group<RigfPx>(n_views, matches, n, p.min_pair);
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

    RigDevice<RigPpPixels> D;
    if (int e = rigpp_upload(fn, G, n_views, f_in, R_in, pp_in, L.data(), D, s)) return e;
    const RigPpStepPrm sp{n_views, p.anchor, p.shared, p.max_iters, 0, p.step_tol, prm->pp_prior};
    const int np = (int)G.pairs.size();
    for (int round = 0; round <= p.max_iters; ++round) {
        rigpp_round(D, np, p.huber, sp, s);
        MS_LAUNCH_CHECK();
    }
    static_assert(offsetof(RigPpState, f_cur) == sizeof(double) * 9 * MS_MAX_VIEWS && offsetof(RigPpState, pp_cur) == sizeof(double) * 10 * MS_MAX_VIEWS,
                  "f_cur and pp_cur follow R_cur: the three come back in one copy");
    RigTail tail;
    std::vector<double> cam(12 * MS_MAX_VIEWS);
    MS_HIP(hipMemcpyAsync(cam.data(), D.st->R_cur, sizeof(double) * cam.size(), hipMemcpyDeviceToHost, s));
    MS_HIP(hipMemcpyAsync(&tail, &D.st->t, sizeof(tail), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    if (!tail.stop) return fail(MS_ERR_HIP, "%s: the device loop ended without a stop reason (round %d, %d iterations)", fn, tail.round, tail.iters);
    memcpy(R_out, cam.data(), sizeof(double) * 9 * n_views);
    memcpy(f_out, cam.data() + 9 * MS_MAX_VIEWS, sizeof(double) * n_views);
    memcpy(pp_out, cam.data() + 10 * MS_MAX_VIEWS, sizeof(double) * 2 * n_views);
    if (info) {
        info->iterations = tail.iters; info->stop_reason = tail.reason;
        info->cost_initial = tail.cost0; info->cost_final = tail.cost;
        info->matches_used = (int)G.items.size(); info->pairs_used = np; info->pairs_ignored = G.ignored;
        info->outliers = (int)tail.outliers;
        info->max_rotation_rad = 0.0; info->max_focal_ratio = 1.0; info->max_pp_shift = 0.0;
        for (int v = 0; v < n_views; ++v) {
            info->max_rotation_rad = std::max(info->max_rotation_rad, rig_angle(R_out + 9 * v, R_in + 9 * v));
            info->max_focal_ratio = std::max(info->max_focal_ratio, std::max(f_out[v] / f_in[v], f_in[v] / f_out[v]));
            info->max_pp_shift = std::max(info->max_pp_shift, std::max(std::fabs(pp_out[2 * v] - pp_in[2 * v]), std::fabs(pp_out[2 * v + 1] - pp_in[2 * v + 1])));
        }
    }
    return MS_OK;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_rig_pp_default_params(ms_rig_pp_params *prm)
{
    MS_CHECK(prm, "ms_rig_pp_default_params: null argument");
    *prm = ms_rig_pp_params{};
    prm->struct_size = sizeof(ms_rig_pp_params);
    prm->max_iters = 50; prm->step_tol = 1e-10; prm->min_pair_matches = 4;
    return MS_OK;
}

int ms_rig_pp_accumulate(int n_views, const double *f, const double *R, const double *pp, const ms_lens *lenses, const ms_rig_px_match *matches, int n, double huber_px,
                         double *cost, double *H, double *g, ms_stream stream)
{
    const char *fn = "ms_rig_pp_accumulate";
    hipStream_t s = as_stream(stream);
    std::vector<LensDist> L;
    if (int e = rigf_check_cameras(fn, n_views, f, R)) return e;
    if (int e = rigpp_lenses(fn, n_views, lenses, L)) return e;
    if (int e = rigpp_check_offsets(fn, n_views, pp)) return e;
    if (int e = rigf_check_matches(fn, n_views, matches, n)) return e;
    MS_CHECK(cost && H && g, "%s: null output", fn);
    MS_CHECK(huber_px >= 0.0 && std::isfinite(huber_px), "%s: huber_px %g must be finite and not negative", fn, huber_px);
    if (int e = rigpp_check_seen(fn, f, pp, L.data(), matches, n)) return e;
    if (int e = require_device()) return e;
    const RigGroups<RigfPx> G = rig_group<RigfPx>(n_views, matches, n, 1);
    RigDevice<RigPpPixels> D;
    if (int e = rigpp_upload(fn, G, n_views, f, R, pp, L.data(), D, s)) return e;
    std::vector<RigPpState> host(1);
    RigPpState &h = host[0];
    rigpp_round(D, (int)G.pairs.size(), huber_px, RigPpStepPrm{n_views, 0, 0, 1, 1, 0.0, 0.0}, s);
    MS_LAUNCH_CHECK();
    MS_HIP(hipMemcpyAsync(&h, D.st, sizeof(RigPpState), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    const int d = RIGP_B * n_views;
    *cost = h.t.cost;
    for (int r = 0; r < d; ++r) {
        g[r] = h.g[r];
        for (int c = 0; c < d; ++c) H[r * d + c] = h.H[r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r];
    }
    return MS_OK;
}

int ms_refine_rig_pp(int n_views, const double *f_in, const double *R_in, const double *pp_in, const ms_lens *lenses, const ms_rig_px_match *matches, int n,
                     const ms_rig_pp_params *prm, double *f_out, double *R_out, double *pp_out, ms_rig_pp_info *info, ms_stream stream)
{
    return rigpp_refine("ms_refine_rig_pp", n_views, f_in, R_in, pp_in, lenses, matches, n, prm, f_out, R_out, pp_out, info, as_stream(stream));
}

int ms_refine_rig_pp_ctx(ms_ctx *c, const ms_mesh_match *matches, const int *match_count, const ms_rig_pp_params *prm, double *focal_out, double *pp_out, float *R_out,
                         ms_rig_pp_info *info, ms_stream stream)
{
    const char *fn = "ms_refine_rig_pp_ctx";
    MS_CHECK(c && matches && match_count && prm && focal_out && pp_out && R_out, "%s: null argument", fn);
    if (int e = rig_ctx_check(fn, c)) return e;
    const int N = c->N;
    std::vector<double> R, Rr(9 * N), f(N), pp(2 * N, 0.0), po(2 * N);
    std::vector<ms_lens> lenses(N);
    std::vector<LensCam> cam(N);
    for (int v = 0; v < N; ++v) {
        if (c->K[v][1] != 0.f)
            return fail(MS_ERR_UNSUPPORTED, "%s: view %d has a skew (K[1] = %g): centred pixels do not carry it", fn, v, (double)c->K[v][1]);
        f[v] = (double)c->K[v][0];
        lenses[v] = c->lens[v];
        if (lenses[v].model == MS_LENS_NONE) { lenses[v] = ms_lens{}; lenses[v].struct_size = sizeof(ms_lens); }      // (a view ms_set_lens never saw holds zeros)
        const float Kc[9] = {c->K[v][0], 0.f, 0.f, 0.f, c->K[v][0], 0.f, 0.f, 0.f, 1.f};      // as ms_refine_rig_focals_lens centres its pixels
        cam[v] = lens_cam(Kc, nullptr, c->lens[v].model != MS_LENS_NONE ? &c->lens[v] : nullptr);
    }
    std::vector<ms_rig_px_match> pm;
    auto pixels = [&](ms_rig_px_match &o, int q, const double *ra, const double *rb) {
        const int v = o.view_a, dst = o.view_b;
        const bool sa = lens_project(cam[v].model, cam[v], ra[0], ra[1], ra[2], o.a[0], o.a[1]), sb = lens_project(cam[dst].model, cam[dst], rb[0], rb[1], rb[2], o.b[0], o.b[1]);
        MS_CHECK(sa && sb, "%s: match %d of view %d: the lens of view %d does not see the ray (%g, %g, %g): it has no source pixel", fn, q, v, sa ? dst : v, sa ? rb[0] : ra[0],
                 sa ? rb[1] : ra[1], sa ? rb[2] : ra[2]);
        return (int)MS_OK;
    };
    if (int e = rig_ctx_matches(fn, c, matches, match_count, R, pm, pixels)) return e;
    if (int e = rigpp_refine(fn, N, f.data(), R.data(), pp.data(), lenses.data(), pm.data(), (int)pm.size(), prm, focal_out, Rr.data(), po.data(), info, as_stream(stream)))
        return e;
    for (int v = 0; v < N; ++v) {
        pp_out[2 * v] = (double)c->K[v][2] + po[2 * v];
        pp_out[2 * v + 1] = (double)c->K[v][5] + po[2 * v + 1] * (double)c->K[v][4] / (double)c->K[v][0];
    }
    for (int q = 0; q < 9 * N; ++q) R_out[q] = (float)Rr[q];
    return MS_OK;
}

}  // extern "C"
