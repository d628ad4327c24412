// rig_focal.hip -- self-calibrating rigs: focals and rotations from feature matches (include/ms_stitch.h, "Self-calibrating rigs").
// detail::focalsFromHomography and detail::HomographyBasedEstimator on the host (a few dozen operations), detail::BundleAdjusterRay over focal and rotation
// (OCV/stitching/src/motion_estimators.cpp:514-700) on the device.  Calibration-time work: the per-frame path never runs anything of this unit.  Everything is double;
// -ffp-contract=off keeps every product, sum, division and sqrt of the per-match terms a separate IEEE operation, in the order the header states.
// This unit holds what is the focal problem's own: the per-match terms (the policy RigPixels, 4 unknowns a view), the homography estimator, the checks of cameras and
// pixel matches and the entry points.  The kernels k_rig_accum<RigPixels> and k_rig_step<4>, the Levenberg-Marquardt rule and the host side around them are
// rig_lm.hpp's, shared with rig.hip; what a pixel match shares with the lens form (rig_lens.hip) -- the residual, the 46 sums, the checks -- is rig_px.hpp's.
#include "rig_px.hpp"

namespace ms {

struct RigPixels {
    using Match = RigfPx;
    using Aux = char;                             // no per-view data beside the state
    static constexpr int B = 4;
    struct Cams { double fi, fj, m; };            // the pair's two focals and their geometric mean
    static __device__ __forceinline__ Cams load(const RigState<4> *st, const RigPair &pr, const Aux *)
    {
        const double fi = st->f_trial[pr.i], fj = st->f_trial[pr.j], m = sqrt(fi * fj);
        return Cams{fi, fj, m};
    }
    // The terms of one match: the rays, the focal columns; the residual and the sums are rig_px.hpp's.
    static __device__ __forceinline__ void terms(const double *Ri, const double *Rj, const Cams &cams, const RigfPx &px, double h, double acc[RigSums<4>::SUMS])
    {
        const double fi = cams.fi, fj = cams.fj, m = cams.m;
        const double na = sqrt(px.a[0] * px.a[0] + px.a[1] * px.a[1] + fi * fi), nb = sqrt(px.b[0] * px.b[0] + px.b[1] * px.b[1] + fj * fj);
        const double a0 = px.a[0] / na, a1 = px.a[1] / na, a2 = fi / na, b0 = px.b[0] / nb, b1 = px.b[1] / nb, b2 = fj / nb;
        const double p0 = Ri[0] * a0 + Ri[1] * a1 + Ri[2] * a2, p1 = Ri[3] * a0 + Ri[4] * a1 + Ri[5] * a2, p2 = Ri[6] * a0 + Ri[7] * a1 + Ri[8] * a2;
        const double q0 = Rj[0] * b0 + Rj[1] * b1 + Rj[2] * b2, q1 = Rj[3] * b0 + Rj[4] * b1 + Rj[5] * b2, q2 = Rj[6] * b0 + Rj[7] * b1 + Rj[8] * b2;
        const RigPxResidual e = rig_px_residual(m, p0, p1, p2, q0, q1, q2, h);
        const double ma = m * a2, mb = m * b2;
        const double ci0 = 0.5 * e.r0 + ma * (Ri[2] - a2 * p0), ci1 = 0.5 * e.r1 + ma * (Ri[5] - a2 * p1), ci2 = 0.5 * e.r2 + ma * (Ri[8] - a2 * p2);
        const double cj0 = 0.5 * e.r0 - mb * (Rj[2] - b2 * q0), cj1 = 0.5 * e.r1 - mb * (Rj[5] - b2 * q1), cj2 = 0.5 * e.r2 - mb * (Rj[8] - b2 * q2);
        rig_px_sums(e, ci0, ci1, ci2, cj0, cj1, cj2, acc);
    }
};

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
    return rig_lm_accumulate<RigPixels>(fn, n_views, f, R, matches, n, huber_px, cost, H, g, as_stream(stream));
}

int ms_refine_rig_cameras(int n_views, const double *f_in, const double *R_in, const ms_rig_px_match *matches, int n, const ms_rig_focal_params *prm, double *f_out,
                          double *R_out, ms_rig_focal_info *info, ms_stream stream)
{
    return rigf_refine<RigPixels>("ms_refine_rig_cameras", n_views, f_in, R_in, matches, n, prm, f_out, R_out, info, as_stream(stream), [] { return (int)MS_OK; });
}

int ms_refine_rig_focals(ms_ctx *c, const ms_mesh_match *matches, const int *match_count, const ms_rig_focal_params *prm, double *focal_out, float *R_out,
                         ms_rig_focal_info *info, ms_stream stream)
{
    const char *fn = "ms_refine_rig_focals";
    MS_CHECK(c && matches && match_count && prm && focal_out && R_out, "%s: null argument", fn);
    if (int e = rig_ctx_check(fn, c)) return e;
    if (c->lens_maps)
        return fail(MS_ERR_UNSUPPORTED, "%s: the context has a lens (ms_set_lens): a focal under a lens needs the inverse distortion: ms_refine_rig_focals_lens has it", fn);
    const int N = c->N;
    std::vector<double> R, Rr(9 * N), f(N);
    for (int v = 0; v < N; ++v) f[v] = (double)c->K[v][0];
    // a ray in front of its camera is the centred pixel f (x / z, y / z)
    std::vector<ms_rig_px_match> pm;
    auto pixels = [&](ms_rig_px_match &o, int q, const double *ra, const double *rb) {
        const int v = o.view_a, dst = o.view_b;
        MS_CHECK(ra[2] > 0.0 && rb[2] > 0.0, "%s: match %d of view %d: a ray lies behind its camera (z = %g, %g): it has no source pixel", fn, q, v, ra[2], rb[2]);
        o.a[0] = f[v] * (ra[0] / ra[2]); o.a[1] = f[v] * (ra[1] / ra[2]);
        o.b[0] = f[dst] * (rb[0] / rb[2]); o.b[1] = f[dst] * (rb[1] / rb[2]);
        return (int)MS_OK;
    };
    if (int e = rig_ctx_matches(fn, c, matches, match_count, R, pm, pixels)) return e;
    // single-precision rotations are orthonormal to about 1e-7 only: what the context holds is used as it is, as ms_refine_rig does
    if (int e = rigf_refine<RigPixels>(fn, N, f.data(), R.data(), pm.data(), (int)pm.size(), prm, focal_out, Rr.data(), info, as_stream(stream), [] { return (int)MS_OK; })) return e;
    for (int q = 0; q < 9 * N; ++q) R_out[q] = (float)Rr[q];
    return MS_OK;
}

}  // extern "C"
