// rig.hip -- rig rotations from feature matches: the ray bundle adjustment of include/ms_stitch.h ("Rig rotation refinement").
// Replaces detail::BundleAdjusterRay (OCV/stitching/src/motion_estimators.cpp:514-700) with the focals held.  Calibration-time work: the per-frame path never runs
// anything of this unit.  Everything is double; -ffp-contract=off keeps every product and sum of the per-match terms a separate IEEE operation, in the order the
// header states, so two implementations of the contract differ by the ORDER of their sums only.
// This unit holds what is the ray problem's own: the per-match terms (the policy RigRays, 3 unknowns a view), the checks of a ray match and the entry points.  The
// kernels k_rig_accum<RigRays> and k_rig_step<3>, the Levenberg-Marquardt rule and the host side around them are rig_lm.hpp's, shared with rig_focal.hip.
#include "rig_lm.hpp"

namespace ms {

struct RigRay { double a[3], b[3]; };         // a seen by view i, b by view j

struct RigRays {
    using Match = RigRay;
    static constexpr int B = 3;
    using Aux = char;                         // no per-view data beside the state
    struct Cams {};                           // a pair needs nothing beside its two rotations
    static __device__ __forceinline__ Cams load(const RigState<3> *, const RigPair &, const Aux *) { return Cams{}; }
    // The terms of one match, added into acc in the header's order.  h == 0: plain least squares.
    static __device__ __forceinline__ void terms(const double *Ri, const double *Rj, const Cams &, const RigRay &m, double h, double acc[RigSums<3>::SUMS])
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
};

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
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

// everything ms_refine_rig_rotations does; fn names the entry point in messages
static int rig_refine(const char *fn, int n_views, const double *R_in, const ms_rig_match *matches, int n, const ms_rig_refine_params *prm, double *R_out,
                      ms_rig_refine_info *info, hipStream_t s)
{
    if (int e = rig_check_matches(fn, n_views, R_in, matches, n)) return e;
    MS_CHECK(R_out, "%s: null R_out", fn);
    MS_CHECK(prm, "%s: null params", fn);
    MS_CHECK(prm->struct_size == sizeof(ms_rig_refine_params), "%s: params.struct_size %u, this library's ms_rig_refine_params has %zu bytes", fn, prm->struct_size,
             sizeof(ms_rig_refine_params));
    const RigLmParams p{prm->anchor_view, 0, prm->max_iters, prm->min_pair_matches, prm->huber_rad, prm->step_tol};
    if (int e = rig_check_params(fn, n_views, p, "huber_rad")) return e;
    return rig_lm_refine<RigRays>(fn, n_views, nullptr, R_in, matches, n, p, nullptr, R_out, info, s);
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
    return rig_lm_accumulate<RigRays>("ms_rig_accumulate", n_views, nullptr, R, matches, n, huber_rad, cost, H, g, as_stream(stream));
}

int ms_refine_rig_rotations(int n_views, const double *R_in, const ms_rig_match *matches, int n, const ms_rig_refine_params *prm, double *R_out, ms_rig_refine_info *info,
                            ms_stream stream)
{
    return rig_refine("ms_refine_rig_rotations", n_views, R_in, matches, n, prm, R_out, info, as_stream(stream));
}

int ms_refine_rig(ms_ctx *c, const ms_mesh_match *matches, const int *match_count, const ms_rig_refine_params *prm, float *R_out, ms_rig_refine_info *info, ms_stream stream)
{
    const char *fn = "ms_refine_rig";
    MS_CHECK(c && matches && match_count && prm && R_out, "%s: null argument", fn);
    if (int e = rig_ctx_check(fn, c)) return e;
    std::vector<double> R;
    std::vector<ms_rig_match> rm;
    auto rays = [](ms_rig_match &o, int, const double *ra, const double *rb) {
        for (int e = 0; e < 3; ++e) { o.a[e] = ra[e]; o.b[e] = rb[e]; }
        return MS_OK;
    };
    if (int e = rig_ctx_matches(fn, c, matches, match_count, R, rm, rays)) return e;
    const int N = c->N;
    std::vector<double> Rr(9 * N);
    if (int e = rig_refine(fn, N, R.data(), rm.data(), (int)rm.size(), prm, Rr.data(), info, as_stream(stream))) return e;
    for (int q = 0; q < 9 * N; ++q) R_out[q] = (float)Rr[q];
    return MS_OK;
}

}  // extern "C"
