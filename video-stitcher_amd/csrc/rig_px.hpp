// rig_px.hpp -- what the two pixel policies of the rig refinement share (include/ms_stitch.h, "Self-calibrating rigs"): RigPixels (rig_focal.hip, pinhole views) and
// RigLensPixels (rig_lens.hip, views behind fixed lenses); rig_coeffs.hip (one shared lens with free coefficients) builds on both.  Internal; those three units include it.  Both have 4 unknowns a view and the match record of centred pixels;
// they differ in how a pixel becomes its unit ray a and the ray's derivative by the log focal, i.e. in the focal columns ci, cj.  From the rotated rays on, the
// residual, the Huber weight and the 46 sums are one copy, here, and so are the checks of cameras and pixel matches and the frame of the refinement's entry points.
#pragma once
#include "rig_lm.hpp"

namespace ms {

struct RigfPx { double a[2], b[2]; };             // centred pixels: a in view i, b in view j

// u = m p, v = m q, r = m (p - q) and the Huber terms of s = |r|.  h == 0: plain least squares.
struct RigPxResidual { double u0, u1, u2, v0, v1, v2, r0, r1, r2, w, rho, out; };
static __device__ __forceinline__ RigPxResidual rig_px_residual(double m, double p0, double p1, double p2, double q0, double q1, double q2, double h)
{
    RigPxResidual e;
    e.u0 = m * p0; e.u1 = m * p1; e.u2 = m * p2; e.v0 = m * q0; e.v1 = m * q1; e.v2 = m * q2;
    e.r0 = m * (p0 - q0); e.r1 = m * (p1 - q1); e.r2 = m * (p2 - q2);
    const double s2 = e.r0 * e.r0 + e.r1 * e.r1 + e.r2 * e.r2;
    e.w = 1.0; e.rho = s2; e.out = 0.0;
    if (h > 0.0) {
        const double s = sqrt(s2);
        if (s > h) { e.w = h / s; e.rho = (2.0 * h) * s - h * h; e.out = 1.0; }
    }
    return e;
}

// The terms of one match, added into acc in the header's order, from the residual and the two focal columns.
static __device__ __forceinline__ void rig_px_sums(const RigPxResidual &e, double ci0, double ci1, double ci2, double cj0, double cj1, double cj2, double acc[RigSums<4>::SUMS])
{
    const double u0 = e.u0, u1 = e.u1, u2 = e.u2, v0 = e.v0, v1 = e.v1, v2 = e.v2, r0 = e.r0, r1 = e.r1, r2 = e.r2, w = e.w;
    acc[0] += e.rho;
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
    acc[45] += e.out;
}

// One view's side of a match behind a BROWN or FISHEYE lens, shared by RigLensPixels (rig_lens.hip) and the coefficient refinement (rig_coeffs.hip): the unit ray a of
// the centred pixel px at the focal f, da/ds (s = ln f), and the quantities both are made of, which the coefficient columns need again.  false: the lens does not see
// the pixel at this focal.
struct RigLensRay {
    double a0, a1, a2, d0, d1, d2;
    double theta, st, ct, e0, e1, slope;          // FISHEYE (td > 0; at the centre a = e_z, d = 0 and centre is set)
    double x, y, J[4], det, n;                    // BROWN
    bool centre;
};
static __device__ __forceinline__ bool rig_lens_ray(const LensDist &l, double f, const double *px, RigLensRay &o)
{
    const double xd = px[0] / f, yd = px[1] / f;
    o.centre = false;
    if (l.model == MS_LENS_FISHEYE) {
        const double td = hypot(xd, yd);
        if (!lens_fisheye_solve(l, td, o.theta)) return false;
        if (td > 0.0) {
            o.st = sin(o.theta); o.ct = cos(o.theta); o.slope = lens_fisheye_slope(l.k, o.theta); o.e0 = xd / td; o.e1 = yd / td;
            const double st = o.st, ct = o.ct, tp = -td / o.slope, e0 = o.e0, e1 = o.e1;
            o.a0 = st * xd / td; o.a1 = st * yd / td; o.a2 = ct;
            o.d0 = tp * (ct * e0); o.d1 = tp * (ct * e1); o.d2 = -(tp * st);
        } else { o.centre = true; o.a0 = 0.0; o.a1 = 0.0; o.a2 = 1.0; o.d0 = 0.0; o.d1 = 0.0; o.d2 = 0.0; }
    } else {
        double fx, fy;
        if (!lens_brown_solve(l, xd, yd, o.x, o.y)) return false;
        lens_brown_forward(l.k, o.x, o.y, fx, fy, o.J);
        const double x = o.x, y = o.y, *J = o.J;
        o.det = J[0] * J[3] - J[1] * J[2];
        const double det = o.det;
        if (!(fabs(det) > 0.0)) return false;
        const double xs = -((J[3] * xd - J[1] * yd) / det), ys = -((J[0] * yd - J[2] * xd) / det);      // (x', y') = -J^-1 (xd, yd)
        o.n = sqrt(x * x + y * y + 1.0);
        const double n = o.n;
        o.a0 = x / n; o.a1 = y / n; o.a2 = 1.0 / n;
        const double dot = o.a0 * xs + o.a1 * ys;
        o.d0 = (xs - o.a0 * dot) / n; o.d1 = (ys - o.a1 * dot) / n; o.d2 = -(o.a2 * dot) / n;
    }
    return true;
}
// p = R a and t = m R da/ds of that ray
static __device__ __forceinline__ void rig_lens_rotate(double m, const double *R, const RigLensRay &o, double *p, double *t)
{
    p[0] = R[0] * o.a0 + R[1] * o.a1 + R[2] * o.a2; p[1] = R[3] * o.a0 + R[4] * o.a1 + R[5] * o.a2; p[2] = R[6] * o.a0 + R[7] * o.a1 + R[8] * o.a2;
    t[0] = m * (R[0] * o.d0 + R[1] * o.d1 + R[2] * o.d2); t[1] = m * (R[3] * o.d0 + R[4] * o.d1 + R[5] * o.d2); t[2] = m * (R[6] * o.d0 + R[7] * o.d1 + R[8] * o.d2);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
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
    MS_CHECK(n >= 1 && n <= RIG_MAX_MATCHES, "%s: %d matches outside [1, %d]", fn, n, RIG_MAX_MATCHES);
    for (int k = 0; k < n; ++k) {
        const ms_rig_px_match &m = matches[k];
        MS_CHECK(m.view_a >= 0 && m.view_a < n_views && m.view_b >= 0 && m.view_b < n_views, "%s: match %d names views %d, %d outside [0, %d)", fn, k, m.view_a, m.view_b, n_views);
        MS_CHECK(m.view_a != m.view_b, "%s: match %d pairs view %d with itself", fn, k, m.view_a);
        MS_CHECK(std::isfinite(m.a[0]) && std::isfinite(m.a[1]) && std::isfinite(m.b[0]) && std::isfinite(m.b[1]), "%s: match %d: a pixel is not finite", fn, k);
    }
    return MS_OK;
}

// Everything ms_refine_rig_cameras does, for the policy P; fn names the entry point in messages.  extra(): the policy's own checks of its inputs (the lenses), run after
// those of cameras and matches and before the device is touched.
template <class P, class Extra> static int rigf_refine(const char *fn, int n_views, const double *f_in, const double *R_in, const ms_rig_px_match *matches, int n,
                                                       const ms_rig_focal_params *prm, double *f_out, double *R_out, ms_rig_focal_info *info, hipStream_t s, Extra extra,
                                                       const typename P::Aux *aux = nullptr, int n_aux = 0)
{
    if (int e = rigf_check_cameras(fn, n_views, f_in, R_in)) return e;
    if (int e = rigf_check_matches(fn, n_views, matches, n)) return e;
    MS_CHECK(f_out && R_out, "%s: null output", fn);
    MS_CHECK(prm, "%s: null params", fn);
    MS_CHECK(prm->struct_size == sizeof(ms_rig_focal_params), "%s: params.struct_size %u, this library's ms_rig_focal_params has %zu bytes", fn, prm->struct_size,
             sizeof(ms_rig_focal_params));
    const RigLmParams p{prm->anchor_view, prm->shared_focal ? 1 : 0, prm->max_iters, prm->min_pair_matches, prm->huber_px, prm->step_tol};
    if (int e = rig_check_params(fn, n_views, p, "huber_px")) return e;
    if (prm->shared_focal)
        for (int v = 1; v < n_views; ++v)
            MS_CHECK(f_in[v] == f_in[0], "%s: shared_focal asks for equal input focals; view %d has %.17g, view 0 has %.17g", fn, v, f_in[v], f_in[0]);
    if (int e = extra()) return e;
    if (int e = rig_lm_refine<P>(fn, n_views, f_in, R_in, matches, n, p, f_out, R_out, info, s, aux, n_aux)) return e;
    if (info) {
        info->max_focal_ratio = 1.0;
        for (int v = 0; v < n_views; ++v) info->max_focal_ratio = std::max(info->max_focal_ratio, std::max(f_out[v] / f_in[v], f_in[v] / f_out[v]));
    }
    return MS_OK;
}

}  // namespace ms
