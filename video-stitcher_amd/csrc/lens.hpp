// lens.hpp -- the lens model of include/ms_stitch.h (ms_lens): ONE copy of the arithmetic, host and device.  ms_lens_project (api.cpp) calls it on the
// host, k_lens_maps / k_lens_bbox (lens.hip) on the device.  Everything is double: this is calibration-time work, evaluated once per map pixel and rounded
// to float once at the store; no fp32 evaluation order is part of the contract (unlike warp_combine, common.hpp, which the per-frame kernels share).
//   BROWN    cvProjectPoints2           OCV/calib3d/src/calibration.cpp:760-790
//   FISHEYE  cv::fisheye::projectPoints OCV/calib3d/src/fisheye.cpp:130-150, with theta = atan2(rho, Z) instead of atan(rho / Z): equal for Z > 0, and it goes on past 90 degrees
#pragma once
#include <cmath>
#include "common.hpp"

namespace ms {

// a view's camera as the lens kernels take it (by value): the five entries of K the pixel needs, R as doubles, the coefficients, max_theta in radians
struct LensCam {
    double k00, k01, k02, k11, k12;   // K[0], K[1], K[2], K[4], K[5]
    double r[9];                      // R, row-major: the camera ray of a warper direction d is R^T d (R^-1 = R^T)
    double k[8];
    double max_theta;
    int model;
};

constexpr double LENS_PI = 3.1415926535897932384626433832795;

static inline double lens_max_theta_deg(const ms_lens &l)
{
    return l.max_theta_deg != 0.0 ? l.max_theta_deg : (l.model == MS_LENS_FISHEYE ? 180.0 : 89.0);
}

// lens == nullptr: MS_LENS_NONE
static inline LensCam lens_cam(const float *K, const float *R, const ms_lens *lens)
{
    LensCam c{};
    c.k00 = K[0]; c.k01 = K[1]; c.k02 = K[2]; c.k11 = K[4]; c.k12 = K[5];
    for (int i = 0; i < 9; ++i) c.r[i] = R ? (double)R[i] : (i % 4 == 0 ? 1.0 : 0.0);
    c.model = lens ? lens->model : (int)MS_LENS_NONE;
    if (c.model != MS_LENS_NONE) {
        for (int i = 0; i < 8; ++i) c.k[i] = lens->k[i];
        c.max_theta = lens_max_theta_deg(*lens) * (LENS_PI / 180.0);
    }
    return c;
}

// the radial profiles ms_lens_check samples (the tangential terms of BROWN are not part of them)
__host__ __device__ inline double lens_brown_cdist(const double *k, double r2)
{
    return (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2);
}
__host__ __device__ inline double lens_fisheye_theta_d(const double *k, double theta)
{
    const double t2 = theta * theta;
    return theta * (1.0 + (((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2);
}

// The camera ray (X, Y, Z) -> the source pixel.  false: the view does not see the ray (the map entry is then (-1, -1), the reference's own "behind the camera"
// marker, stitching/src/cuda/build_warp_maps.cu:137-152); px / py are not written.
__host__ __device__ inline bool lens_project(int model, const LensCam &c, double X, double Y, double Z, double &px, double &py)
{
    double xd, yd;
    if (model == MS_LENS_NONE) {
        if (!(Z > 0.0)) return false;
        xd = X / Z; yd = Y / Z;
    } else {
        const double rho = hypot(X, Y), theta = atan2(rho, Z);
        if (!(theta <= c.max_theta)) return false;
        if (model == MS_LENS_BROWN) {
            const double x = X / Z, y = Y / Z, r2 = x * x + y * y, cd = lens_brown_cdist(c.k, r2);
            xd = x * cd + 2.0 * c.k[2] * x * y + c.k[3] * (r2 + 2.0 * x * x);
            yd = y * cd + c.k[2] * (r2 + 2.0 * y * y) + 2.0 * c.k[3] * x * y;
        } else {
            const double s = rho > 0.0 ? lens_fisheye_theta_d(c.k, theta) / rho : 0.0;
            xd = X * s; yd = Y * s;
        }
    }
    px = c.k00 * xd + c.k01 * yd + c.k02;
    py = c.k11 * yd + c.k12;
    return true;
}

// ---- the inverse: distorted normalised coordinates -> the camera ray ------------------------------------------------------------------------------
// What ms_lens_unproject (api.cpp), k_lens_unproject (lens.hip) and the lens policy of the rig refinement (rig_lens.hip) share.  `limit` is where the view's field
// ends in the solver's own variable: theta_d(max_theta) for FISHEYE, tan(max_theta) for BROWN.
struct LensDist { double k[8], max_theta, limit; int model; };

static inline LensDist lens_dist(const ms_lens *lens)
{
    LensDist d{};
    d.model = lens ? lens->model : (int)MS_LENS_NONE;
    if (d.model != MS_LENS_NONE) {
        for (int i = 0; i < 8; ++i) d.k[i] = lens->k[i];
        d.max_theta = lens_max_theta_deg(*lens) * (LENS_PI / 180.0);
        d.limit = d.model == MS_LENS_FISHEYE ? lens_fisheye_theta_d(d.k, d.max_theta) : std::tan(d.max_theta);
    }
    return d;
}

// d theta_d / d theta
__host__ __device__ inline double lens_fisheye_slope(const double *k, double theta)
{
    const double t2 = theta * theta;
    return 1.0 + ((((9.0 * k[3]) * t2 + 7.0 * k[2]) * t2 + 5.0 * k[1]) * t2 + 3.0 * k[0]) * t2;
}

// theta of theta_d on [0, max_theta], where ms_lens_check found the profile increasing: Newton steps kept inside a bracket (the midpoint where a step leaves it or
// the slope is not positive), until theta stands still, 60 rounds at most.  false: theta_d lies past the profile's value at max_theta (or is not a number).
__host__ __device__ inline bool lens_fisheye_solve(const LensDist &l, double td, double &theta)
{
    if (!(td <= l.limit)) return false;
    double lo = 0.0, hi = l.max_theta, t = fmin(td, l.max_theta);
    for (int it = 0; it < 60; ++it) {
        const double g = lens_fisheye_theta_d(l.k, t) - td, d = lens_fisheye_slope(l.k, t);
        if (g > 0.0) hi = t; else lo = t;
        double tn = d > 0.0 ? t - g / d : 0.5 * (lo + hi);
        if (!(tn >= lo && tn <= hi)) tn = 0.5 * (lo + hi);
        if (tn == t) break;
        t = tn;
    }
    theta = t;
    return true;
}

// BROWN forward on normalised coordinates, tangential terms included, and its Jacobian J = {dxd/dx, dxd/dy, dyd/dx, dyd/dy}
__host__ __device__ inline void lens_brown_forward(const double *k, double x, double y, double &xd, double &yd, double *J)
{
    const double r2 = x * x + y * y;
    const double N = 1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2, D = 1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2;
    const double dN = (3.0 * k[4] * r2 + 2.0 * k[1]) * r2 + k[0], dD = (3.0 * k[7] * r2 + 2.0 * k[6]) * r2 + k[5];
    const double cd = N / D, dc = (dN * D - N * dD) / (D * D);      // cdist and d cdist / d r2
    xd = x * cd + 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x);
    yd = y * cd + k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y;
    J[0] = cd + 2.0 * x * x * dc + 2.0 * k[2] * y + 6.0 * k[3] * x;
    J[1] = J[2] = 2.0 * x * y * dc + 2.0 * k[2] * x + 2.0 * k[3] * y;
    J[3] = cd + 2.0 * y * y * dc + 6.0 * k[2] * y + 2.0 * k[3] * x;
}

// (x, y) of (xd, yd) by Newton on the full forward model from (xd, yd); settled when max |step| <= 2^-50 max(1, |x|, |y|) (a zero step is not asked for: the last
// bit may alternate for ever), 50 rounds at most.  false: not settled, a singular Jacobian, anything not finite, or hypot(x, y) > tan(max_theta).
__host__ __device__ inline bool lens_brown_solve(const LensDist &l, double xd, double yd, double &x, double &y)
{
    double px = xd, py = yd, J[4];
    bool settled = false;
    for (int it = 0; it < 50 && !settled; ++it) {
        double fx, fy;
        lens_brown_forward(l.k, px, py, fx, fy, J);
        const double det = J[0] * J[3] - J[1] * J[2], ex = fx - xd, ey = fy - yd;
        if (!(fabs(det) > 0.0) || !(fabs(det) < HUGE_VAL)) return false;
        const double dx = (J[3] * ex - J[1] * ey) / det, dy = (J[0] * ey - J[2] * ex) / det;
        px -= dx; py -= dy;
        if (!(fabs(px) < HUGE_VAL) || !(fabs(py) < HUGE_VAL)) return false;
        settled = fmax(fabs(dx), fabs(dy)) <= 0x1p-50 * fmax(1.0, fmax(fabs(px), fabs(py)));
    }
    if (!settled || !(hypot(px, py) <= l.limit)) return false;
    x = px; y = py;
    return true;
}

// The source pixel -> the unit camera ray (cv::undistortPoints / cv::fisheye::undistortPoints, with a solver that ends at the rounding floor instead of after a
// fixed number of fixed-point rounds).  c: the five entries of K.  false: the lens does not see the pixel; ray is not written.
__host__ __device__ inline bool lens_unproject(const LensCam &c, const LensDist &l, double px, double py, double *ray)
{
    const double yd = (py - c.k12) / c.k11, xd = (px - c.k02 - c.k01 * yd) / c.k00;
    if (l.model == MS_LENS_FISHEYE) {
        const double td = hypot(xd, yd);
        double theta;
        if (!lens_fisheye_solve(l, td, theta)) return false;
        if (!(td > 0.0)) { ray[0] = 0.0; ray[1] = 0.0; ray[2] = 1.0; return true; }
        const double st = sin(theta);
        ray[0] = st * xd / td; ray[1] = st * yd / td; ray[2] = cos(theta);
        return true;
    }
    double x = xd, y = yd;
    if (l.model == MS_LENS_BROWN && !lens_brown_solve(l, xd, yd, x, y)) return false;
    const double n = sqrt(x * x + y * y + 1.0);
    if (!(n < HUGE_VAL)) return false;
    ray[0] = x / n; ray[1] = y / n; ray[2] = 1.0 / n;
    return true;
}

// The warper direction of the integer warper coordinate (u, v) -- detail::SphericalProjector / CylindricalProjector::mapBackward
// (OCV/stitching/include/opencv2/stitching/detail/warpers_inl.hpp:238-255, :275-290) in double, from (double)u / (double)(float)scale -- turned into the camera by R^T.
// cu / su: cos and sin of u / scale (a lane of k_lens_bbox keeps its column over all rows).
__host__ __device__ inline void lens_ray(int proj, const LensCam &c, double su, double cu, double v, double &X, double &Y, double &Z)
{
    double dx, dy, dz;
    if (proj == MS_PROJ_SPHERICAL) { const double sv = sin(v); dx = sv * su; dy = -cos(v); dz = sv * cu; }
    else { dx = su; dy = v; dz = cu; }
    X = c.r[0] * dx + c.r[3] * dy + c.r[6] * dz;
    Y = c.r[1] * dx + c.r[4] * dy + c.r[7] * dz;
    Z = c.r[2] * dx + c.r[5] * dy + c.r[8] * dz;
}

}  // namespace ms
