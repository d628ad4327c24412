// rig_coeffs.hip -- self-calibrating lens rigs, the lens included: focals, rotations and up to four distortion coefficients of ONE lens all views share, from feature
// matches on source pixels (include/ms_stitch.h, "Self-calibrating rigs", the coefficient form).  What rig_lens.hip refines with the lenses fixed, plus G columns a
// match: the derivative of the residual by each free coefficient, from the implicit-function theorem on the forward model (lens.hpp's slope and Jacobian).
// Calibration-time work: the per-frame path never runs anything of this unit.  Everything is double; -ffp-contract=off as in rig_focal.hip.
// This unit holds the policy RigCoeffPixels<G> (the 46 sums of RigLensPixels by the code of rig_px.hpp, then the border sums), an accumulate kernel and a step kernel
// of its own (the system has G rows more than k_rig_step<4>'s and the trial lens is judged on the device, so rig.o, rig_focal.o and rig_lens.o keep their kernels as
// they are), and the entry points.  Grouping, parameter checks and the walk over a context's lists are rig_lm.hpp's and rig_px.hpp's.
#include "rig_px.hpp"

namespace ms {

constexpr int RIGC_MAX_G = 4;
constexpr int RIGC_VIEWS = 4 * MS_MAX_VIEWS;                   // the coefficient rows of the full system follow the views': 64 .. 67
constexpr int RIGC_DIM = RIGC_VIEWS + RIGC_MAX_G;              // 68
constexpr int RIGC_RED = RigSums<4>::RED + RIGC_MAX_G;         // the largest system solved: 65
constexpr int RIGC_PROFILE_STEPS = 4096;                       // ms_lens_check's

// The sums of one pair: the 46 of RigSums<4> | g_k (G) | H_kk upper triangle row-major (G (G + 1) / 2) | per coefficient n: H(rot_i, n) (3), H(f_i, n), H(rot_j, n) (3), H(f_j, n)
template <int G> struct RigcSums {
    static constexpr int TRI = G * (G + 1) / 2;
    static constexpr int G_K = RigSums<4>::SUMS, H_KK = G_K + G, H_VK = H_KK + TRI, SUMS = H_VK + 8 * G;      // 46, 56, 67, 79, 92
    static constexpr int PART = (SUMS + 15) / 16 * 16;
};

// the shared lens but its coefficients, which are state: by value to both kernels
struct RigcLens { int model, G, idx[RIGC_MAX_G]; double max_theta, end; };      // idx: the free entries of k[], ascending; end: where ms_lens_check's profile ends

struct RigcState {
    double R_cur[MS_MAX_VIEWS * 9], f_cur[MS_MAX_VIEWS], k_cur[8];              // the last accepted cameras and lens: they come back in one copy
    double R_trial[MS_MAX_VIEWS * 9], f_trial[MS_MAX_VIEWS], k_trial[8], limit_trial;
    double H[RIGC_DIM * RIGC_DIM], g[RIGC_DIM];
    RigTail t;
};

// d a / d k[idx] of a view's ray, the pixel and the focal held (include/ms_stitch.h)
static __device__ __forceinline__ void rigc_dray(const LensDist &l, int idx, const RigLensRay &o, double *d)
{
    if (l.model == MS_LENS_FISHEYE) {
        if (o.centre) { d[0] = 0.0; d[1] = 0.0; d[2] = 0.0; return; }
        const double t2 = o.theta * o.theta;
        double q = o.theta * t2;                                // theta^(2 idx + 3)
        for (int i = 0; i < idx; ++i) q = q * t2;
        const double tp = -q / o.slope;
        d[0] = tp * (o.ct * o.e0); d[1] = tp * (o.ct * o.e1); d[2] = -(tp * o.st);
        return;
    }
    const double x = o.x, y = o.y, r2 = x * x + y * y;
    double F0, F1;
    if (idx == 2) { F0 = (2.0 * x) * y; F1 = r2 + (2.0 * y) * y; }
    else if (idx == 3) { F0 = r2 + (2.0 * x) * x; F1 = (2.0 * x) * y; }
    else {
        const double D = 1.0 + ((l.k[7] * r2 + l.k[6]) * r2 + l.k[5]) * r2;
        const double s = idx == 0 ? r2 / D : idx == 1 ? (r2 * r2) / D : ((r2 * r2) * r2) / D;
        F0 = x * s; F1 = y * s;
    }
    const double xs = -((o.J[3] * F0 - o.J[1] * F1) / o.det), ys = -((o.J[0] * F1 - o.J[2] * F0) / o.det);
    const double t = o.a0 * xs + o.a1 * ys;
    d[0] = (xs - o.a0 * t) / o.n; d[1] = (ys - o.a1 * t) / o.n; d[2] = -(o.a2 * t) / o.n;
}

template <int G> struct RigCoeffPixels {
    using S = RigcSums<G>;
    struct Cams { LensDist l; double fi, fj, m; };
    // The terms of one match: RigLensPixels' to the letter for the 46, then the border sums in the header's order.
    static __device__ __forceinline__ void terms(const double *Ri, const double *Rj, const Cams &cams, const RigcLens &cf, const RigfPx &px, double h, double *acc)
    {
        RigLensRay ra, rb;
        double p[3], q[3], ti[3], tj[3];
        const bool seen_i = rig_lens_ray(cams.l, cams.fi, px.a, ra), seen_j = rig_lens_ray(cams.l, cams.fj, px.b, rb);
        if (!seen_i || !seen_j) { acc[0] += HUGE_VAL; return; }
        rig_lens_rotate(cams.m, Ri, ra, p, ti); rig_lens_rotate(cams.m, Rj, rb, q, tj);
        const RigPxResidual e = rig_px_residual(cams.m, p[0], p[1], p[2], q[0], q[1], q[2], h);
        const double ci0 = 0.5 * e.r0 + ti[0], ci1 = 0.5 * e.r1 + ti[1], ci2 = 0.5 * e.r2 + ti[2], cj0 = 0.5 * e.r0 - tj[0], cj1 = 0.5 * e.r1 - tj[1], cj2 = 0.5 * e.r2 - tj[2];
        rig_px_sums(e, ci0, ci1, ci2, cj0, cj1, cj2, acc);
        if constexpr (G > 0) {
            const double m = cams.m, w = e.w, u0 = e.u0, u1 = e.u1, u2 = e.u2, v0 = e.v0, v1 = e.v1, v2 = e.v2;
            double E[G][3];
#pragma unroll
            for (int n = 0; n < G; ++n) {
                double da[3], db[3];
                rigc_dray(cams.l, cf.idx[n], ra, da); rigc_dray(cams.l, cf.idx[n], rb, db);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    E[n][k] = m * (Ri[3 * k] * da[0] + Ri[3 * k + 1] * da[1] + Ri[3 * k + 2] * da[2]) - m * (Rj[3 * k] * db[0] + Rj[3 * k + 1] * db[1] + Rj[3 * k + 2] * db[2]);
            }
#pragma unroll
            for (int n = 0, t = 0; n < G; ++n) {
                const double e0 = E[n][0], e1 = E[n][1], e2 = E[n][2];
                acc[S::G_K + n] += w * (e0 * e.r0 + e1 * e.r1 + e2 * e.r2);
#pragma unroll
                for (int c = n; c < G; ++c, ++t) acc[S::H_KK + t] += w * (e0 * E[c][0] + e1 * E[c][1] + e2 * E[c][2]);
                double *b = acc + S::H_VK + 8 * n;
                b[0] += w * (u1 * e2 - u2 * e1); b[1] += w * (u2 * e0 - u0 * e2); b[2] += w * (u0 * e1 - u1 * e0);
                b[3] += w * (ci0 * e0 + ci1 * e1 + ci2 * e2);
                b[4] += -(w * (v1 * e2 - v2 * e1)); b[5] += -(w * (v2 * e0 - v0 * e2)); b[6] += -(w * (v0 * e1 - v1 * e0));
                b[7] += w * (cj0 * e0 + cj1 * e1 + cj2 * e2);
            }
        }
    }
};

// ---- k_rigc_accum: k_rig_accum's schedule (one 256-thread workgroup a pair, the same per-lane order, butterfly and wave fold), with the lens taken from the state ----
template <int G> __global__ void __launch_bounds__(256) k_rigc_accum(const RigcState *__restrict__ st, const RigPair *__restrict__ pairs, const RigfPx *__restrict__ items,
                                                                     RigcLens cf, double h, double *__restrict__ part)
{
    using P = RigCoeffPixels<G>;
    using S = RigcSums<G>;
    __shared__ double s_sum[4][S::PART];
    if (st->t.stop) return;
    const RigPair pr = pairs[blockIdx.x];
    double Ri[9], Rj[9], acc[S::SUMS];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ri[k] = st->R_trial[pr.i * 9 + k]; Rj[k] = st->R_trial[pr.j * 9 + k]; }
    typename P::Cams cams;
#pragma unroll
    for (int k = 0; k < 8; ++k) cams.l.k[k] = st->k_trial[k];
    cams.l.max_theta = cf.max_theta; cams.l.limit = st->limit_trial; cams.l.model = cf.model;
    cams.fi = st->f_trial[pr.i]; cams.fj = st->f_trial[pr.j]; cams.m = sqrt(cams.fi * cams.fj);
#pragma unroll
    for (int e = 0; e < S::SUMS; ++e) acc[e] = 0.0;
    for (int k = threadIdx.x; k < pr.cnt; k += 256) P::terms(Ri, Rj, cams, cf, items[pr.off + k], h, acc);
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

// ---- k_rigc_step --------------------------------------------------------------------------------------------------------------------------------------
// row r of the solved system as a row of the full one: k_rig_step<4>'s rows (m0 of them; -1: the shared focal), then the coefficients
static __device__ __forceinline__ int rigc_full_row(int r, int m0, int anchor, int shared)
{
    return r < m0 ? rig_full_row<4>(r, m0, anchor, shared) : RIGC_VIEWS + (r - m0);
}

static __device__ double rigc_entry(const double *Hs, int nv, int r, int c, int m0, int anchor, int shared)
{
    const int fr = rigc_full_row(r, m0, anchor, shared), fc = rigc_full_row(c, m0, anchor, shared);
    if (fr >= 0 && fc >= 0) return Hs[fr * RIGC_DIM + fc];
    double t = 0.0;
    if (fr < 0 && fc < 0) {
        for (int v = 0; v < nv; ++v)
            for (int w = 0; w < nv; ++w) t += Hs[(4 * v + 3) * RIGC_DIM + 4 * w + 3];
    } else {
        const int o = fr < 0 ? fc : fr;           // (the full matrix is symmetric bit for bit)
        for (int v = 0; v < nv; ++v) t += Hs[o * RIGC_DIM + 4 * v + 3];
    }
    return t;
}

// k_rig_step<4> with G coefficient rows after the views': the same assembly in pair order, accept rule, lambda rule, stop rules and Cholesky.  Two things are its own:
// the factor is stored packed (row r at r (r + 1) / 2), so that the 68 x 68 full system and the 65 x 65 factor take 36992 + 17160 bytes of LDS, 55.3 KB with the
// vectors, inside the 64 KB a workgroup may declare; and a solved step is followed by ms_lens_check's profile rule on the trial coefficients, 16 of the 4096 samples
// a lane: a trial that fails it is a failed solve (lambda <- 10 lambda, one iteration, solve again).
template <int G> __global__ void __launch_bounds__(RIG_STEP_THREADS) k_rigc_step(RigcState *__restrict__ st, const RigPair *__restrict__ pairs, int n_pairs,
                                                                                 const double *__restrict__ part, RigcLens cf, RigStepPrm prm)
{
    using S4 = RigSums<4>;
    using S = RigcSums<G>;
    constexpr int DIM = RIGC_DIM, PART = S::PART, KV = RIGC_VIEWS;
    constexpr RigSym<4> sym = rig_sym<4>();
    __shared__ double Hs[DIM * DIM], A[RIGC_RED * (RIGC_RED + 1) / 2], gs[DIM], xs[DIM], s_k[8];
    __shared__ double s_cost, s_outl, s_lam;
    __shared__ int s_accept, s_stop, s_reason, s_iters, s_ok;
    if (st->t.stop) return;
    const int tid = threadIdx.x, nv = prm.n_views;
    for (int k = tid; k < DIM * DIM; k += RIG_STEP_THREADS) Hs[k] = 0.0;
    if (tid < DIM) gs[tid] = 0.0;
    __syncthreads();
    // the system, pair after pair: inside a pair every sum goes to a place of its own
    for (int p = 0; p < n_pairs; ++p) {
        if (tid >= S4::G_I && tid < S::SUMS && tid != S4::OUTL) {
            const double v = part[(size_t)p * PART + tid];
            const int iB = 4 * pairs[p].i, jB = 4 * pairs[p].j;
            if (tid < S4::G_J) gs[iB + tid - S4::G_I] += v;
            else if (tid < S4::H_II) gs[jB + tid - S4::G_J] += v;
            else if (tid < S4::H_IJ) {
                const int bB = tid < S4::H_JJ ? iB : jB, k = tid < S4::H_JJ ? tid - S4::H_II : tid - S4::H_JJ, r = sym.r[k], c = sym.c[k];
                Hs[(bB + r) * DIM + bB + c] += v;
                if (r != c) Hs[(bB + c) * DIM + bB + r] += v;
            } else if (tid < S4::OUTL) {
                const int k = tid - S4::H_IJ, r = k / 4, c = k % 4;
                Hs[(iB + r) * DIM + jB + c] += v;
                Hs[(jB + c) * DIM + iB + r] += v;
            } else if (tid < S::H_KK) gs[KV + tid - S::G_K] += v;
            else if (tid < S::H_VK) {
                int k = tid - S::H_KK, r = 0;
                while (k >= G - r) { k -= G - r; ++r; }       // row r of the upper triangle holds G - r entries
                const int c = r + k;
                Hs[(KV + r) * DIM + KV + c] += v;
                if (r != c) Hs[(KV + c) * DIM + KV + r] += v;
            } else {
                const int k = tid - S::H_VK, n = k / 8, e = k % 8, row = e < 4 ? iB + e : jB + e - 4;
                Hs[row * DIM + KV + n] += v;
                Hs[(KV + n) * DIM + row] += v;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double cost = 0.0, outl = 0.0;
        for (int p = 0; p < n_pairs; ++p) { cost += part[(size_t)p * PART]; outl += part[(size_t)p * PART + S4::OUTL]; }
        s_cost = cost; s_outl = outl;
    }
    __syncthreads();
    if (prm.assemble_only) {
        for (int k = tid; k < DIM * DIM; k += RIG_STEP_THREADS) st->H[k] = Hs[k];
        if (tid < DIM) st->g[tid] = gs[tid];
        if (tid == 0) st->t.cost = s_cost;
        return;
    }
    if constexpr (G > 0) {
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
            if (tid < 8) st->k_cur[tid] = st->k_trial[tid];
            for (int k = tid; k < DIM * DIM; k += RIG_STEP_THREADS) st->H[k] = Hs[k];
            if (tid < DIM) st->g[tid] = gs[tid];
        } else {
            for (int k = tid; k < DIM * DIM; k += RIG_STEP_THREADS) Hs[k] = st->H[k];
            if (tid < DIM) gs[tid] = st->g[tid];
        }
        __syncthreads();
        // (H + lambda diag H) d = -g over the rotations of the views but the anchor, the focals and the coefficients
        const int shared = prm.shared, anchor = prm.anchor, m0 = shared ? 3 * (nv - 1) + 1 : 4 * nv - 3, m = m0 + G;
        auto at = [](int r, int c) { return r * (r + 1) / 2 + c; };      // c <= r
        while (!s_stop) {
            const double lam = s_lam;
            for (int k = tid; k < m * m; k += RIG_STEP_THREADS) {
                const int r = k / m, c = k % m;
                if (c > r) continue;
                const double hv = rigc_entry(Hs, nv, r, c, m0, anchor, shared);
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
                const int t = m - k - 1;
                for (int e = tid; e < t * t; e += RIG_STEP_THREADS) {
                    const int i = k + 1 + e / t, j = k + 1 + e % t;
                    if (j <= i) A[at(i, j)] -= A[at(i, k)] * A[at(j, k)];
                }
                __syncthreads();
            }
            if (s_ok) {
                if (tid < m) {
                    const int fr = rigc_full_row(tid, m0, anchor, shared);
                    double gv = 0.0;
                    if (fr >= 0) gv = gs[fr];
                    else for (int v = 0; v < nv; ++v) gv += gs[4 * v + 3];
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
                    for (int r = 0; r < m; ++r) { dmax = fmax(dmax, fabs(xs[r])); if (!(fabs(xs[r]) < HUGE_VAL)) s_ok = 0; }
                    st->t.dmax = dmax;
                    // the trial lens: k <- k + d on the free entries
                    for (int k = 0; k < 8; ++k) s_k[k] = st->k_cur[k];
                    for (int n = 0; n < G; ++n) { s_k[cf.idx[n]] = st->k_cur[cf.idx[n]] + xs[m0 + n]; if (!(fabs(s_k[cf.idx[n]]) < HUGE_VAL)) s_ok = 0; }
                }
                __syncthreads();
                if (s_ok) {
                    // ms_lens_check's rule: the profile rises from sample to sample; lane tid holds samples 16 tid + 1 .. 16 tid + 16
                    constexpr int PER = RIGC_PROFILE_STEPS / RIG_STEP_THREADS;
                    static_assert(PER * RIG_STEP_THREADS == RIGC_PROFILE_STEPS, "every lane takes the same number of samples");
                    const bool fish = cf.model == MS_LENS_FISHEYE;
                    auto profile = [&](int i) { const double a = cf.end * i / RIGC_PROFILE_STEPS; return fish ? lens_fisheye_theta_d(s_k, a) : a * lens_brown_cdist(s_k, a * a); };
                    double prev = tid == 0 ? 0.0 : profile(PER * tid);
                    bool rises = true;
                    for (int i = PER * tid + 1; i <= PER * tid + PER; ++i) {
                        const double f = profile(i);
                        if (!(f > prev) || !(fabs(f) < HUGE_VAL)) rises = false;
                        prev = f;
                    }
                    __syncthreads();                         // (every lane has read s_ok)
                    if (!rises) s_ok = 0;
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
            const int rot = shared ? 3 * (tid - (tid > anchor ? 1 : 0)) : 4 * tid - (tid > anchor ? 3 : 0);
            if (tid == anchor) { for (int k = 0; k < 9; ++k) st->R_trial[tid * 9 + k] = st->R_cur[tid * 9 + k]; }
            else rig_rotate(&xs[rot], &st->R_cur[tid * 9], &st->R_trial[tid * 9]);
            const int foc = shared ? m0 - 1 : (tid == anchor ? rot : rot + 3);
            st->f_trial[tid] = st->f_cur[tid] * exp(xs[foc]);
        }
        if (!s_stop && tid < 8) st->k_trial[tid] = s_k[tid];
        if (tid == 0) {
            if (!s_stop) st->limit_trial = cf.model == MS_LENS_FISHEYE ? lens_fisheye_theta_d(s_k, cf.max_theta) : cf.end;
            st->t.lam = s_lam; st->t.iters = s_iters; st->t.reason = s_reason; st->t.stop = s_stop; st->t.round = st->t.round + 1;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
// the shared lens and the free set, as the device takes them
static int rigc_lens(const char *fn, const ms_lens *lens, unsigned free_coeffs, bool refine, LensDist &L, RigcLens &cf)
{
    MS_CHECK(lens, "%s: null lens", fn);
    if (int e = lens_check(fn, lens)) return e;
    MS_CHECK(lens->model != MS_LENS_NONE, "%s: lens is MS_LENS_NONE: it has no coefficients to refine (ms_refine_rig_cameras refines a pinhole rig)", fn);
    const bool fish = lens->model == MS_LENS_FISHEYE;
    MS_CHECK(!(free_coeffs >> 8), "%s: free_coeffs 0x%x names a bit outside k[0..7]", fn, free_coeffs);
    if (fish) MS_CHECK(!(free_coeffs & 0xf0u), "%s: free_coeffs 0x%x names a bit outside MS_LENS_FISHEYE's k1..k4 (bits 0..3)", fn, free_coeffs);
    else if (free_coeffs & 0xe0u)
        return fail(MS_ERR_UNSUPPORTED, "%s: free_coeffs 0x%x frees a coefficient of MS_LENS_BROWN's denominator (bits 5..7): those stay fixed", fn, free_coeffs);
    cf = RigcLens{};
    for (int b = 0; b < 8; ++b)
        if (free_coeffs >> b & 1u) {
            MS_CHECK(cf.G < RIGC_MAX_G, "%s: free_coeffs 0x%x frees more than %d coefficients", fn, free_coeffs, RIGC_MAX_G);
            cf.idx[cf.G++] = b;
        }
    MS_CHECK(!refine || cf.G >= 1, "%s: free_coeffs is empty: nothing of the lens to refine (ms_refine_rig_cameras_lens refines behind fixed lenses)", fn);
    L = lens_dist(lens);
    cf.model = lens->model; cf.max_theta = L.max_theta; cf.end = fish ? L.max_theta : L.limit;
    return MS_OK;
}

// every pixel must be seen through the lens at the input focals (cameras and matches have been checked)
static int rigc_check_seen(const char *fn, const double *f, const LensDist &L, const ms_rig_px_match *matches, int n)
{
    for (int k = 0; k < n; ++k) {
        const ms_rig_px_match &m = matches[k];
        for (int side = 0; side < 2; ++side) {
            const int v = side ? m.view_b : m.view_a;
            const double *px = side ? m.b : m.a;
            LensCam cam{};
            cam.k00 = f[v]; cam.k11 = f[v];
            double ray[3];
            MS_CHECK(lens_unproject(cam, L, px[0], px[1], ray), "%s: match %d: the lens does not see the centred pixel (%g, %g) of view %d at the focal %g", fn, k, px[0], px[1],
                     v, f[v]);
        }
    }
    return MS_OK;
}

// One device block, state | pairs | items | partials: the first three are laid out in pinned memory and go up in ONE copy.
struct RigcDevice { RigcState *st; RigPair *pairs; RigfPx *items; double *part; };
static int rigc_upload(const char *fn, const RigGroups<RigfPx> &G, int n_views, const double *f, const double *R, const LensDist &L, RigcDevice &D, hipStream_t s)
{
    const size_t np = G.pairs.size(), o_pairs = sizeof(RigcState), o_items = o_pairs + np * sizeof(RigPair), o_part = o_items + G.items.size() * sizeof(RigfPx),
                 total = o_part + np * RigcSums<RIGC_MAX_G>::PART * sizeof(double);
    static_assert(sizeof(RigcState) % 8 == 0 && sizeof(RigPair) % 8 == 0, "the block's parts stay 8-byte aligned");
    char *base = (char *)device_scratch().get(total), *host = (char *)pinned_scratch().get(o_part);
    if (!base || !host) return fail(MS_ERR_NOMEM, "%s: no memory for %zu bytes", fn, total);
    D.st = (RigcState *)base; D.pairs = (RigPair *)(base + o_pairs); D.items = (RigfPx *)(base + o_items); D.part = (double *)(base + o_part);
    RigcState *st = (RigcState *)host;
    memset(st, 0, sizeof(RigcState));
    memcpy(st->R_cur, R, sizeof(double) * 9 * n_views); memcpy(st->R_trial, R, sizeof(double) * 9 * n_views);
    memcpy(st->f_cur, f, sizeof(double) * n_views); memcpy(st->f_trial, f, sizeof(double) * n_views);
    memcpy(st->k_cur, L.k, sizeof(L.k)); memcpy(st->k_trial, L.k, sizeof(L.k));
    st->limit_trial = L.limit;
    st->t.lam = 1e-3;
    memcpy(host + o_pairs, G.pairs.data(), np * sizeof(RigPair));
    memcpy(host + o_items, G.items.data(), G.items.size() * sizeof(RigfPx));
    MS_HIP(hipMemcpyAsync(base, host, o_part, hipMemcpyHostToDevice, s));
    return MS_OK;
}

template <int G> static void rigc_round(const RigcDevice &D, int np, const RigcLens &cf, double huber, const RigStepPrm &sp, hipStream_t s)
{
    k_rigc_accum<G><<<np, 256, 0, s>>>(D.st, D.pairs, D.items, cf, huber, D.part);
    k_rigc_step<G><<<1, RIG_STEP_THREADS, 0, s>>>(D.st, D.pairs, np, D.part, cf, sp);
}
static void rigc_round(const RigcDevice &D, int np, const RigcLens &cf, double huber, const RigStepPrm &sp, hipStream_t s)
{
    switch (cf.G) {
    case 0: rigc_round<0>(D, np, cf, huber, sp, s); break;
    case 1: rigc_round<1>(D, np, cf, huber, sp, s); break;
    case 2: rigc_round<2>(D, np, cf, huber, sp, s); break;
    case 3: rigc_round<3>(D, np, cf, huber, sp, s); break;
    default: rigc_round<4>(D, np, cf, huber, sp, s); break;
    }
}

// The refinement from the checked arguments on: rig_lm_refine's frame around this unit's two kernels.
static int rigc_refine(const char *fn, int n_views, const double *f_in, const double *R_in, const ms_lens *lens_in, const LensDist &L, const RigcLens &cf,
                       const ms_rig_px_match *matches, int n, const RigLmParams &p, double *f_out, double *R_out, ms_lens *lens_out, ms_rig_coeff_info *info, hipStream_t s)
{
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

    RigcDevice D;
    if (int e = rigc_upload(fn, G, n_views, f_in, R_in, L, D, s)) return e;
    const RigStepPrm sp{n_views, p.anchor, p.shared, p.max_iters, 0, p.step_tol};
    const int np = (int)G.pairs.size();
    for (int round = 0; round <= p.max_iters; ++round) rigc_round(D, np, cf, p.huber, sp, s);
    MS_LAUNCH_CHECK();
    static_assert(offsetof(RigcState, f_cur) == sizeof(double) * 9 * MS_MAX_VIEWS && offsetof(RigcState, k_cur) == sizeof(double) * 10 * MS_MAX_VIEWS,
                  "f_cur and k_cur follow R_cur: the three come back in one copy");
    RigTail tail;
    std::vector<double> cam(10 * MS_MAX_VIEWS + 8);
    MS_HIP(hipMemcpyAsync(cam.data(), D.st->R_cur, sizeof(double) * cam.size(), hipMemcpyDeviceToHost, s));
    MS_HIP(hipMemcpyAsync(&tail, &D.st->t, sizeof(tail), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    if (!tail.stop) return fail(MS_ERR_HIP, "%s: the device loop ended without a stop reason (round %d, %d iterations)", fn, tail.round, tail.iters);
    memcpy(R_out, cam.data(), sizeof(double) * 9 * n_views);
    memcpy(f_out, cam.data() + 9 * MS_MAX_VIEWS, sizeof(double) * n_views);
    ms_lens out = *lens_in;
    double kmax = 0.0;
    for (int q = 0; q < cf.G; ++q) {
        out.k[cf.idx[q]] = cam[10 * MS_MAX_VIEWS + cf.idx[q]];
        kmax = std::max(kmax, std::fabs(out.k[cf.idx[q]] - lens_in->k[cf.idx[q]]));
    }
    *lens_out = out;
    if (info) {
        info->iterations = tail.iters; info->stop_reason = tail.reason;
        info->cost_initial = tail.cost0; info->cost_final = tail.cost;
        info->matches_used = (int)G.items.size(); info->pairs_used = np; info->pairs_ignored = G.ignored;
        info->outliers = (int)tail.outliers;
        info->max_rotation_rad = 0.0; info->max_focal_ratio = 1.0;
        for (int v = 0; v < n_views; ++v) {
            info->max_rotation_rad = std::max(info->max_rotation_rad, rig_angle(R_out + 9 * v, R_in + 9 * v));
            info->max_focal_ratio = std::max(info->max_focal_ratio, std::max(f_out[v] / f_in[v], f_in[v] / f_out[v]));
        }
        info->max_coeff_change = kmax;
    }
    return MS_OK;
}

// every check of ms_refine_rig_coeffs, then the refinement
static int rigc_checked_refine(const char *fn, int n_views, const double *f_in, const double *R_in, const ms_lens *lens_in, const ms_rig_px_match *matches, int n,
                               const ms_rig_coeff_params *prm, double *f_out, double *R_out, ms_lens *lens_out, ms_rig_coeff_info *info, hipStream_t s)
{
    if (int e = rigf_check_cameras(fn, n_views, f_in, R_in)) return e;
    if (int e = rigf_check_matches(fn, n_views, matches, n)) return e;
    MS_CHECK(f_out && R_out && lens_out, "%s: null output", fn);
    MS_CHECK(prm, "%s: null params", fn);
    MS_CHECK(prm->struct_size == sizeof(ms_rig_coeff_params), "%s: params.struct_size %u, this library's ms_rig_coeff_params has %zu bytes", fn, prm->struct_size,
             sizeof(ms_rig_coeff_params));
    const RigLmParams p{prm->anchor_view, prm->shared_focal ? 1 : 0, prm->max_iters, prm->min_pair_matches, prm->huber_px, prm->step_tol};
    if (int e = rig_check_params(fn, n_views, p, "huber_px")) return e;
    if (prm->shared_focal)
        for (int v = 1; v < n_views; ++v)
            MS_CHECK(f_in[v] == f_in[0], "%s: shared_focal asks for equal input focals; view %d has %.17g, view 0 has %.17g", fn, v, f_in[v], f_in[0]);
    LensDist L;
    RigcLens cf;
    if (int e = rigc_lens(fn, lens_in, prm->free_coeffs, true, L, cf)) return e;
    if (int e = rigc_check_seen(fn, f_in, L, matches, n)) return e;
    return rigc_refine(fn, n_views, f_in, R_in, lens_in, L, cf, matches, n, p, f_out, R_out, lens_out, info, s);
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_rig_coeff_default_params(ms_rig_coeff_params *prm)
{
    MS_CHECK(prm, "ms_rig_coeff_default_params: null argument");
    *prm = ms_rig_coeff_params{};
    prm->struct_size = sizeof(ms_rig_coeff_params);
    prm->max_iters = 50; prm->step_tol = 1e-10; prm->min_pair_matches = 4;
    prm->free_coeffs = 1u;
    return MS_OK;
}

int ms_rig_coeff_accumulate(int n_views, const double *f, const double *R, const ms_lens *lens, unsigned free_coeffs, const ms_rig_px_match *matches, int n,
                            double huber_px, double *cost, double *H, double *g, ms_stream stream)
{
    const char *fn = "ms_rig_coeff_accumulate";
    hipStream_t s = as_stream(stream);
    LensDist L;
    RigcLens cf;
    if (int e = rigf_check_cameras(fn, n_views, f, R)) return e;
    if (int e = rigc_lens(fn, lens, free_coeffs, false, L, cf)) return e;
    if (int e = rigf_check_matches(fn, n_views, matches, n)) return e;
    MS_CHECK(cost && H && g, "%s: null output", fn);
    MS_CHECK(huber_px >= 0.0 && std::isfinite(huber_px), "%s: huber_px %g must be finite and not negative", fn, huber_px);
    if (int e = rigc_check_seen(fn, f, L, matches, n)) return e;
    if (int e = require_device()) return e;
    const RigGroups<RigfPx> G = rig_group<RigfPx>(n_views, matches, n, 1);
    RigcDevice D;
    if (int e = rigc_upload(fn, G, n_views, f, R, L, D, s)) return e;
    std::vector<RigcState> host(1);
    RigcState &h = host[0];
    rigc_round(D, (int)G.pairs.size(), cf, huber_px, RigStepPrm{n_views, 0, 0, 1, 1, 0.0}, s);
    MS_LAUNCH_CHECK();
    MS_HIP(hipMemcpyAsync(&h, D.st, sizeof(RigcState), hipMemcpyDeviceToHost, s));
    MS_HIP(hipStreamSynchronize(s));
    // the coefficient rows follow the views' in the caller's system as they do in the device's, which always has room for MS_MAX_VIEWS
    const int nv4 = 4 * n_views, d = nv4 + cf.G;
    auto full = [&](int r) { return r < nv4 ? r : RIGC_VIEWS + (r - nv4); };
    *cost = h.t.cost;
    for (int r = 0; r < d; ++r) {
        g[r] = h.g[full(r)];
        for (int c = 0; c < d; ++c) H[r * d + c] = h.H[full(r) * RIGC_DIM + full(c)];
    }
    return MS_OK;
}

int ms_refine_rig_coeffs(int n_views, const double *f_in, const double *R_in, const ms_lens *lens_in, const ms_rig_px_match *matches, int n,
                         const ms_rig_coeff_params *prm, double *f_out, double *R_out, ms_lens *lens_out, ms_rig_coeff_info *info, ms_stream stream)
{
    return rigc_checked_refine("ms_refine_rig_coeffs", n_views, f_in, R_in, lens_in, matches, n, prm, f_out, R_out, lens_out, info, as_stream(stream));
}

int ms_refine_rig_coeffs_ctx(ms_ctx *c, const ms_mesh_match *matches, const int *match_count, const ms_rig_coeff_params *prm, double *focal_out, float *R_out,
                             ms_lens *lens_out, ms_rig_coeff_info *info, ms_stream stream)
{
    const char *fn = "ms_refine_rig_coeffs_ctx";
    MS_CHECK(c && matches && match_count && prm && focal_out && R_out && lens_out, "%s: null argument", fn);
    if (int e = rig_ctx_check(fn, c)) return e;
    const int N = c->N;
    if (c->lens[0].model == MS_LENS_NONE) return fail(MS_ERR_UNSUPPORTED, "%s: view 0 has no lens: the context's views must share one BROWN or FISHEYE lens", fn);
    for (int v = 1; v < N; ++v) {
        bool same = c->lens[v].model == c->lens[0].model && c->lens[v].max_theta_deg == c->lens[0].max_theta_deg;
        for (int k = 0; k < 8 && same; ++k) same = c->lens[v].k[k] == c->lens[0].k[k];
        if (!same) return fail(MS_ERR_UNSUPPORTED, "%s: the lens of view %d differs from view 0's: one lens is refined for the whole rig", fn, v);
    }
    std::vector<double> R, Rr(9 * N), f(N);
    std::vector<LensCam> cam(N);
    for (int v = 0; v < N; ++v) {
        if (c->K[v][1] != 0.f)
            return fail(MS_ERR_UNSUPPORTED, "%s: view %d has a skew (K[1] = %g): centred pixels do not carry it", fn, v, (double)c->K[v][1]);
        f[v] = (double)c->K[v][0];
        const float Kc[9] = {c->K[v][0], 0.f, 0.f, 0.f, c->K[v][0], 0.f, 0.f, 0.f, 1.f};      // as ms_refine_rig_focals_lens centres its pixels
        cam[v] = lens_cam(Kc, nullptr, &c->lens[v]);
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
    const ms_lens lens = c->lens[0];
    if (int e = rigc_checked_refine(fn, N, f.data(), R.data(), &lens, pm.data(), (int)pm.size(), prm, focal_out, Rr.data(), lens_out, info, as_stream(stream))) return e;
    for (int q = 0; q < 9 * N; ++q) R_out[q] = (float)Rr[q];
    return MS_OK;
}

}  // extern "C"
