// rig_lens.hip -- self-calibrating rigs behind lenses: focals and rotations from feature matches on source pixels of Brown-Conrady and fisheye cameras
// (include/ms_stitch.h, "Self-calibrating rigs", the lens form).  detail::BundleAdjusterRay over focal and rotation (OCV/stitching/src/motion_estimators.cpp:514-700)
// with the inverse of the lens model (lens.hpp: cv::undistortPoints, cv::fisheye::undistortPoints) between a pixel and its ray.  Calibration-time work: the per-frame
// path never runs anything of this unit.  Everything is double; -ffp-contract=off as in rig_focal.hip.
// This unit holds the policy RigLensPixels (4 unknowns a view; the lenses are fixed per view, uploaded once next to the state, and not unknowns) and the entry
// points.  The residual, the 46 sums and the checks of cameras and matches are rig_px.hpp's, shared with rig_focal.hip; the kernels k_rig_accum<RigLensPixels> and
// k_rig_step<4> (as rig_focal.hip launches it), the Levenberg-Marquardt rule and the host side around them are rig_lm.hpp's.
#include "rig_px.hpp"

namespace ms {

struct RigLensPixels {
    using Match = RigfPx;
    using Aux = LensDist;                         // one a view
    static constexpr int B = 4;
    struct Cams { LensDist li, lj; double fi, fj, m; };
    static __device__ __forceinline__ Cams load(const RigState<4> *st, const RigPair &pr, const LensDist *lenses)
    {
        const double fi = st->f_trial[pr.i], fj = st->f_trial[pr.j], m = sqrt(fi * fj);
        return Cams{lenses[pr.i], lenses[pr.j], fi, fj, m};
    }
    // One view's side of a match: p = R a, a the unit ray of the centred pixel px at the focal f, and t = m R da/ds, s = ln f (ci = 0.5 r + t_i, cj = 0.5 r - t_j).
    // A view without a lens takes RigPixels' expressions to the letter.  false: the lens does not see the pixel at this focal.
    static __device__ __forceinline__ bool view(const LensDist &l, double f, double m, const double *R, const double *px, double *p, double *t)
    {
        if (l.model == MS_LENS_NONE) {
            const double na = sqrt(px[0] * px[0] + px[1] * px[1] + f * f);
            const double a0 = px[0] / na, a1 = px[1] / na, a2 = f / na;
            p[0] = R[0] * a0 + R[1] * a1 + R[2] * a2; p[1] = R[3] * a0 + R[4] * a1 + R[5] * a2; p[2] = R[6] * a0 + R[7] * a1 + R[8] * a2;
            const double ma = m * a2;
            t[0] = ma * (R[2] - a2 * p[0]); t[1] = ma * (R[5] - a2 * p[1]); t[2] = ma * (R[8] - a2 * p[2]);
            return true;
        }
        RigLensRay ray;                               // (rig_px.hpp: the coefficient refinement runs the same code)
        if (!rig_lens_ray(l, f, px, ray)) return false;
        rig_lens_rotate(m, R, ray, p, t);
        return true;
    }
    // The terms of one match.  A pixel its lens does not see at the trial cameras: +infinity to the cost and nothing to any other sum, so k_rig_step refuses the trial.
    static __device__ __forceinline__ void terms(const double *Ri, const double *Rj, const Cams &cams, const RigfPx &px, double h, double acc[RigSums<4>::SUMS])
    {
        double p[3], q[3], ti[3], tj[3];
        const bool seen_i = view(cams.li, cams.fi, cams.m, Ri, px.a, p, ti), seen_j = view(cams.lj, cams.fj, cams.m, Rj, px.b, q, tj);
        if (!seen_i || !seen_j) { acc[0] += HUGE_VAL; return; }
        const RigPxResidual e = rig_px_residual(cams.m, p[0], p[1], p[2], q[0], q[1], q[2], h);
        rig_px_sums(e, 0.5 * e.r0 + ti[0], 0.5 * e.r1 + ti[1], 0.5 * e.r2 + ti[2], 0.5 * e.r0 - tj[0], 0.5 * e.r1 - tj[1], 0.5 * e.r2 - tj[2], acc);
    }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
// the caller's lenses, each through ms_lens_check, as the device takes them
static int rigl_lenses(const char *fn, int n_views, const ms_lens *lenses, std::vector<LensDist> &L)
{
    MS_CHECK(lenses, "%s: null lenses", fn);
    MS_CHECK(n_views >= 2 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d outside [2, %d]", fn, n_views, MS_MAX_VIEWS);
    L.resize(n_views);
    for (int v = 0; v < n_views; ++v) {
        if (int e = lens_check(fn, &lenses[v])) return e;
        L[v] = lens_dist(&lenses[v]);
    }
    return MS_OK;
}

// every pixel must be seen through its lens at the input focals (cameras and matches have been checked)
static int rigl_check_seen(const char *fn, const double *f, const LensDist *L, const ms_rig_px_match *matches, int n)
{
    for (int k = 0; k < n; ++k) {
        const ms_rig_px_match &m = matches[k];
        for (int side = 0; side < 2; ++side) {
            const int v = side ? m.view_b : m.view_a;
            const double *px = side ? m.b : m.a;
            LensCam cam{};
            cam.k00 = f[v]; cam.k11 = f[v];
            double ray[3];
            MS_CHECK(lens_unproject(cam, L[v], px[0], px[1], ray), "%s: match %d: the lens of view %d does not see the centred pixel (%g, %g) at the focal %g", fn, k, v,
                     px[0], px[1], f[v]);
        }
    }
    return MS_OK;
}

static int rigl_refine(const char *fn, int n_views, const double *f_in, const double *R_in, const LensDist *L, const ms_rig_px_match *matches, int n,
                       const ms_rig_focal_params *prm, double *f_out, double *R_out, ms_rig_focal_info *info, hipStream_t s)
{
    return rigf_refine<RigLensPixels>(fn, n_views, f_in, R_in, matches, n, prm, f_out, R_out, info, s, [&] { return rigl_check_seen(fn, f_in, L, matches, n); }, L, n_views);
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_rig_lens_accumulate(int n_views, const double *f, const double *R, const ms_lens *lenses, const ms_rig_px_match *matches, int n, double huber_px, double *cost,
                           double *H, double *g, ms_stream stream)
{
    const char *fn = "ms_rig_lens_accumulate";
    std::vector<LensDist> L;
    if (int e = rigf_check_cameras(fn, n_views, f, R)) return e;
    if (int e = rigl_lenses(fn, n_views, lenses, L)) return e;
    if (int e = rigf_check_matches(fn, n_views, matches, n)) return e;
    MS_CHECK(cost && H && g, "%s: null output", fn);
    MS_CHECK(huber_px >= 0.0 && std::isfinite(huber_px), "%s: huber_px %g must be finite and not negative", fn, huber_px);
    if (int e = rigl_check_seen(fn, f, L.data(), matches, n)) return e;
    return rig_lm_accumulate<RigLensPixels>(fn, n_views, f, R, matches, n, huber_px, cost, H, g, as_stream(stream), L.data(), n_views);
}

int ms_refine_rig_cameras_lens(int n_views, const double *f_in, const double *R_in, const ms_lens *lenses, const ms_rig_px_match *matches, int n,
                               const ms_rig_focal_params *prm, double *f_out, double *R_out, ms_rig_focal_info *info, ms_stream stream)
{
    const char *fn = "ms_refine_rig_cameras_lens";
    std::vector<LensDist> L;
    if (int e = rigl_lenses(fn, n_views, lenses, L)) return e;
    return rigl_refine(fn, n_views, f_in, R_in, L.data(), matches, n, prm, f_out, R_out, info, as_stream(stream));
}

int ms_refine_rig_focals_lens(ms_ctx *c, const ms_mesh_match *matches, const int *match_count, const ms_rig_focal_params *prm, double *focal_out, float *R_out,
                              ms_rig_focal_info *info, ms_stream stream)
{
    const char *fn = "ms_refine_rig_focals_lens";
    MS_CHECK(c && matches && match_count && prm && focal_out && R_out, "%s: null argument", fn);
    if (int e = rig_ctx_check(fn, c)) return e;
    const int N = c->N;
    std::vector<double> R, Rr(9 * N), f(N);
    std::vector<LensDist> L(N);
    std::vector<LensCam> cam(N);
    for (int v = 0; v < N; ++v) {
        if (c->K[v][1] != 0.f)
            return fail(MS_ERR_UNSUPPORTED, "%s: view %d has a skew (K[1] = %g): centred pixels do not carry it", fn, v, (double)c->K[v][1]);
        f[v] = (double)c->K[v][0];
        const ms_lens *lens = c->lens[v].model != MS_LENS_NONE ? &c->lens[v] : nullptr;
        L[v] = lens_dist(lens);
        // the centred pixel (px - K[2], (py - K[5]) K[0] / K[4]) of lens_project's pixel is lens_project's with the camera (f, 0, 0; f, 0): no rounding of a sum with the
        // principal point and of its difference
        const float Kc[9] = {c->K[v][0], 0.f, 0.f, 0.f, c->K[v][0], 0.f, 0.f, 0.f, 1.f};
        cam[v] = lens_cam(Kc, nullptr, lens);
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
    // single-precision rotations are orthonormal to about 1e-7 only: what the context holds is used as it is, as ms_refine_rig does
    if (int e = rigl_refine(fn, N, f.data(), R.data(), L.data(), pm.data(), (int)pm.size(), prm, focal_out, Rr.data(), info, as_stream(stream))) return e;
    for (int q = 0; q < 9 * N; ++q) R_out[q] = (float)Rr[q];
    return MS_OK;
}

}  // extern "C"
