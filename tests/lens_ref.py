"""float64 numpy restatement of the lens model and of the ROI rule of include/ms_stitch.h (ms_lens, ms_build_warp_maps_lens, ms_warp_roi_lens): the reference
of tests/test_lens_abi.py and tests/test_lens_gpu.py.  Written from the header's text, vectorised; nothing here calls the library.

Lens values are plain tuples (model, k, max_theta_deg) with model "none" / "brown" / "fisheye"; `to_ms` turns one into the binding's Lens."""
import math

import numpy as np

NONE = ("none", (), 0.0)
BROWN = ("brown", (-0.18, 0.03, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0), 75.0)
BROWN_ZERO = ("brown", (0.0,) * 8, 0.0)
FISH = ("fisheye", (-0.02, 0.003, 0.0, 0.0), 100.0)
CYL_MAX_ELEVATION_DEG = 80.0


def to_ms(ms, lens):
    model, k, mt = lens
    if model == "none":
        return None
    return (ms.Lens.brown if model == "brown" else ms.Lens.fisheye)(*k, max_theta_deg=mt)


def max_theta(lens):
    model, _, mt = lens
    if model == "none":
        return None
    return math.radians(mt if mt else (180.0 if model == "fisheye" else 89.0))


def theta_d(k, theta):
    k = list(k) + [0.0] * (4 - len(k))
    return theta * (1 + k[0] * theta ** 2 + k[1] * theta ** 4 + k[2] * theta ** 6 + k[3] * theta ** 8)


def project(K, lens, X, Y, Z):
    """camera rays (arrays) -> (px, py, seen) in float64; px = py = -1 where not seen"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    X, Y, Z = [np.asarray(a, np.float64) for a in (X, Y, Z)]
    model, k, _ = lens
    k = list(k) + [0.0] * (8 - len(k))
    rho = np.hypot(X, Y)
    theta = np.arctan2(rho, Z)
    with np.errstate(all="ignore"):
        if model == "none":
            seen = Z > 0
            xd, yd = X / Z, Y / Z
        elif model == "brown":
            seen = theta <= max_theta(lens)
            x, y = X / Z, Y / Z
            r2 = x * x + y * y
            num = 1 + k[0] * r2 + k[1] * r2 ** 2 + k[4] * r2 ** 3
            den = 1 + k[5] * r2 + k[6] * r2 ** 2 + k[7] * r2 ** 3
            cdist = num / den
            xd = x * cdist + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
            yd = y * cdist + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        else:
            seen = theta <= max_theta(lens)
            ratio = np.divide(theta_d(k, theta), rho, out=np.zeros_like(rho), where=rho > 0)
            xd, yd = X * ratio, Y * ratio
        px = K[0, 0] * xd + K[0, 1] * yd + K[0, 2]
        py = K[1, 1] * yd + K[1, 2]
    return np.where(seen, px, -1.0), np.where(seen, py, -1.0), seen


def rays(proj, R, scale, u0, v0, w, h):
    """camera rays (X, Y, Z, each h x w) of the integer warper coordinates [u0, u0 + w) x [v0, v0 + h); proj "sph" / "cyl" """
    R = np.asarray(R, np.float64).reshape(3, 3)
    s = float(np.float32(scale))
    u = np.arange(u0, u0 + w, dtype=np.float64)[None, :] / s
    v = np.arange(v0, v0 + h, dtype=np.float64)[:, None] / s
    one_u, one_v = np.ones_like(u), np.ones_like(v)
    if proj == "sph":
        d = (np.sin(v) * np.sin(u), -np.cos(v) * one_u, np.sin(v) * np.cos(u))
    else:
        d = (np.sin(u) * one_v, v * one_u, np.cos(u) * one_v)
    Rt = R.T        # R^-1
    return tuple(Rt[j, 0] * d[0] + Rt[j, 1] * d[1] + Rt[j, 2] * d[2] for j in range(3))


def maps(proj, K, R, lens, scale, u0, v0, w, h):
    """the float64 backward maps of the window, and the rays' theta (for the comparison's exclusion rule)"""
    X, Y, Z = rays(proj, R, scale, u0, v0, w, h)
    mx, my, _ = project(K, lens, X, Y, Z)
    return mx, my, np.arctan2(np.hypot(X, Y), Z)


def seen_mask(mx, my, src_w, src_h):
    """k_valid_mask's rule on the float32-rounded coordinates: the truncated coordinates lie in [0, src_w) x [0, src_h)"""
    xx, yy = np.trunc(np.float32(mx).astype(np.float64)), np.trunc(np.float32(my).astype(np.float64))
    return (xx >= 0) & (xx < src_w) & (yy >= 0) & (yy < src_h)


def window(proj, scale):
    """the candidate window (u0, v0, w, h): u in [-U, U), v in [0, U) spherical, [-V, V] cylindrical"""
    s = float(np.float32(scale))
    U = int(np.rint(math.pi * s))
    if proj == "sph":
        return -U, 0, 2 * U, U
    V = int(math.ceil(s * math.tan(math.radians(CYL_MAX_ELEVATION_DEG))))
    return -U, -V, 2 * U, 2 * V + 1


def bbox(mask, u0, v0):
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return None
    return (int(xs.min()) + u0, int(ys.min()) + v0, int(xs.max() - xs.min()) + 1, int(ys.max() - ys.min()) + 1)


def roi(proj, K, R, lens, scale, src_w, src_h, margin=1e-6):
    """(ROI, robust): the bounding box of the seen candidates, and whether moving every candidate whose float64 coordinate lies within `margin` px of a validity
    threshold (-1, src_w, src_h) in or out of the seen set leaves it unchanged"""
    u0, v0, w, h = window(proj, scale)
    mx, my, _ = maps(proj, K, R, lens, scale, u0, v0, w, h)
    m = seen_mask(mx, my, src_w, src_h)
    marker = (mx == -1.0) & (my == -1.0)
    near = (np.minimum(np.minimum(np.abs(mx + 1), np.abs(mx - src_w)), np.minimum(np.abs(my + 1), np.abs(my - src_h))) <= margin) & ~marker
    box = bbox(m, u0, v0)
    return box, box == bbox(m & ~near, u0, v0) == bbox(m | near, u0, v0)
