"""float64 numpy statement of the virtual-camera contract of include/ms_stitch.h section 5 (ms_look_at_view, ms_cube_face_view, ms_build_view_maps) and the
extended-source route ms_reproject is defined by: the reference of tests/test_reproject_abi.py and tests/test_reproject_gpu.py.  Written from the header's text,
vectorised; nothing here calls the library.

A panorama frame is a dict(proj="sph" | "cyl", scale, u0, v0, wrap, clamp); a view a dict(kind="camera", w, h, K, R, lens) with a lens_ref lens tuple, or
dict(kind="surface", w, h, R, proj, scale, tl_u, tl_v).  `to_ms_frame` / `to_ms_view` turn them into the binding's structs."""
import math

import numpy as np

import lens_ref as L
import np_ref

FACES = [(0.0, 0.0), (90.0, 0.0), (180.0, 0.0), (-90.0, 0.0), (0.0, 90.0), (0.0, -90.0)]      # front, right, back, left, up, down: (yaw, pitch)


def look_at_R(yaw_deg, pitch_deg, roll_deg):
    """Ry(yaw) Rx(pitch) Rz(roll) in double (libm's sin / cos of degrees * (pi / 180))"""
    a, p, r = [math.radians(v) for v in (yaw_deg, pitch_deg, roll_deg)]
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float64)
    Rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]], np.float64)
    Rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]], np.float64)
    mul = lambda A, B: np.array([[A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j] for j in range(3)] for i in range(3)], np.float64)      # sums left to right
    return mul(mul(Ry, Rx), Rz)


def look_at_K(hfov_deg, w, h):
    f = (w / 2.0) / math.tan(math.radians(hfov_deg) / 2.0)
    return np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float64)


def look_at(yaw, pitch, roll, hfov, w, h, lens=L.NONE):
    return dict(kind="camera", w=w, h=h, K=np.float32(look_at_K(hfov, w, h)), R=np.float32(look_at_R(yaw, pitch, roll)), lens=lens)


def cube_face(face, size):
    return look_at(FACES[face][0], FACES[face][1], 0.0, 90.0, size, size)


def to_ms_frame(ms, fr):
    return ms.PanoFrame.make(ms.PROJ_SPHERICAL if fr["proj"] == "sph" else ms.PROJ_CYLINDRICAL, fr["scale"], fr["u0"], fr["v0"], fr["wrap"], fr["clamp"])


def to_ms_view(ms, v):
    if v["kind"] == "camera":
        return ms.View.camera(v["w"], v["h"], np.float32(v["K"]).reshape(-1), np.float32(v["R"]).reshape(-1), L.to_ms(ms, v["lens"]))
    return ms.View.surface(v["w"], v["h"], np.float32(v["R"]).reshape(-1), ms.PROJ_SPHERICAL if v["proj"] == "sph" else ms.PROJ_CYLINDRICAL, v["scale"],
                           v["tl_u"], v["tl_v"])


# ---- ms_lens_unproject's arithmetic, vectorised ---------------------------------------------------------------------------------------------------
def _fisheye_theta(k, td, mt):
    """theta of theta_d on [0, max_theta]: bracketed Newton until theta stands still (60 rounds at most); (theta, seen)"""
    k = list(k) + [0.0] * (4 - len(k))
    seen = td <= L.theta_d(k, mt)
    lo, hi = np.zeros_like(td), np.full_like(td, mt)
    t = np.minimum(td, mt)
    for _ in range(60):
        t2 = t * t
        g = L.theta_d(k, t) - td
        d = 1 + (((9 * k[3] * t2 + 7 * k[2]) * t2 + 5 * k[1]) * t2 + 3 * k[0]) * t2
        hi = np.where(g > 0, t, hi); lo = np.where(g > 0, lo, t)
        with np.errstate(all="ignore"):
            tn = np.where(d > 0, t - g / d, 0.5 * (lo + hi))
        tn = np.where((tn >= lo) & (tn <= hi), tn, 0.5 * (lo + hi))
        if np.array_equal(tn, t):
            break
        t = tn
    return t, seen


def _brown_forward(k, x, y):
    r2 = x * x + y * y
    N = 1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
    D = 1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2
    dN = (3 * k[4] * r2 + 2 * k[1]) * r2 + k[0]
    dD = (3 * k[7] * r2 + 2 * k[6]) * r2 + k[5]
    cd, dc = N / D, (dN * D - N * dD) / (D * D)
    xd = x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    J = (cd + 2 * x * x * dc + 2 * k[2] * y + 6 * k[3] * x, 2 * x * y * dc + 2 * k[2] * x + 2 * k[3] * y, cd + 2 * y * y * dc + 6 * k[2] * y + 2 * k[3] * x)
    return xd, yd, J


def _brown_solve(k, xd, yd, mt):
    """2-D Newton on the full forward model from (xd, yd), settled at max |step| <= 2^-50 max(1, |x|, |y|), 50 rounds at most; (x, y, seen)"""
    k = list(k) + [0.0] * (8 - len(k))
    x, y = xd.copy(), yd.copy()
    settled = np.zeros(xd.shape, bool)
    bad = np.zeros(xd.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(50):
            fx, fy, (j0, j1, j3) = _brown_forward(k, x, y)
            det = j0 * j3 - j1 * j1
            ex, ey = fx - xd, fy - yd
            bad |= ~settled & ~((np.abs(det) > 0) & np.isfinite(det))
            dx, dy = (j3 * ex - j1 * ey) / det, (j0 * ey - j1 * ex) / det
            act = ~settled & ~bad
            x = np.where(act, x - dx, x); y = np.where(act, y - dy, y)
            bad |= act & ~(np.isfinite(x) & np.isfinite(y))
            settled |= act & ~bad & (np.maximum(np.abs(dx), np.abs(dy)) <= 2.0 ** -50 * np.maximum(1.0, np.maximum(np.abs(x), np.abs(y))))
            if (settled | bad).all():
                break
        seen = settled & ~bad & (np.hypot(x, y) <= math.tan(mt))
    return x, y, seen


def unproject(K, lens, px, py):
    """pixels (arrays, float64) -> (unit camera rays c0, c1, c2, seen)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    model, k, _ = lens
    yd = (py - K[1, 2]) / K[1, 1]
    xd = (px - K[0, 2] - K[0, 1] * yd) / K[0, 0]
    if model == "fisheye":
        td = np.hypot(xd, yd)
        theta, seen = _fisheye_theta(k, td, L.max_theta(lens))
        with np.errstate(all="ignore"):
            s = np.where(td > 0, np.sin(theta) / td, 0.0)
        return np.where(td > 0, s * xd, 0.0), np.where(td > 0, s * yd, 0.0), np.where(td > 0, np.cos(theta), 1.0), seen
    if model == "brown":
        x, y, seen = _brown_solve(k, xd, yd, L.max_theta(lens))
    else:
        x, y, seen = xd, yd, np.ones(xd.shape, bool)
    n = np.sqrt(x * x + y * y + 1.0)
    return x / n, y / n, 1.0 / n, seen


# ---- contract 4: the maps ---------------------------------------------------------------------------------------------------------------------------
def view_rays(view):
    """step 1: the view rays of the integer pixels, each h x w, and the seen flags"""
    w, h = view["w"], view["h"]
    x = np.arange(w, dtype=np.float64)[None, :] * np.ones((h, 1))
    y = np.arange(h, dtype=np.float64)[:, None] * np.ones((1, w))
    if view["kind"] == "camera":
        return unproject(np.float32(view["K"]), view["lens"], x, y)
    s = float(np.float32(view["scale"]))
    U, V = (view["tl_u"] + x) / s, (view["tl_v"] + y) / s
    if view["proj"] == "sph":
        return np.sin(V) * np.sin(U), -np.cos(V), np.sin(V) * np.cos(U), np.ones((h, w), bool)
    return np.sin(U), V, np.cos(U), np.ones((h, w), bool)


def view_maps(frame, view):
    """(X, Y, seen): the float64 maps of `view` into the panorama image `frame`; X = Y = -1 where not seen.  X is NOT yet rounded: see rounded_x."""
    c0, c1, c2, seen = view_rays(view)
    R = np.float32(view["R"]).astype(np.float64).reshape(3, 3)
    d = [R[k, 0] * c0 + R[k, 1] * c1 + R[k, 2] * c2 for k in range(3)]      # step 2, summed left to right
    S = float(np.float32(frame["scale"]))
    hh = np.hypot(d[0], d[2])
    U = S * np.arctan2(d[0], d[2])
    if frame["proj"] == "sph":
        V = S * np.arctan2(hh, -d[1])
    else:
        seen = seen & (hh != 0)
        with np.errstate(all="ignore"):
            V = S * d[1] / hh
    X, Y = U - frame["u0"], V - frame["v0"]
    if frame["wrap"] > 0:
        X = X - frame["wrap"] * np.floor(X / frame["wrap"])
    return np.where(seen, X, -1.0), np.where(seen, Y, -1.0), seen


def ulp_bound(ref64):
    """1 float32 ulp of max(|ref|, 1)"""
    return np.spacing(np.maximum(np.abs(np.float32(ref64)), np.float32(1))).astype(np.float64)


def within_one_ulp(got, ref64, wrap=0):
    """|got - float32(ref)| <= 1 ulp of max(|ref|, 1); with wrap > 0 the difference is taken modulo wrap (a coordinate within an ulp of the seam may come out at
    either end)"""
    d = np.abs(got.astype(np.float64) - np.float32(ref64).astype(np.float64))
    if wrap > 0:
        d = np.minimum(d, wrap - d)
    return d <= ulp_bound(ref64)


# ---- contract 5: the sampler, by the route the header defines it with ---------------------------------------------------------------------------------
def extend(src, wrap, clamp):
    """the source with one column either side (columns cols - 1 and 0 when it wraps, zeros otherwise), then one row above and below (the edge rows of the
    column-extended image when clamped, zeros otherwise)"""
    h, w = src.shape[:2]
    e = np.zeros((h, w + 2, 3), np.uint8)
    e[:, 1:-1] = src
    if wrap:
        e[:, 0] = src[:, w - 1]; e[:, -1] = src[:, 0]
    out = np.zeros((h + 2, w + 2, 3), np.uint8)
    out[1:-1] = e
    if clamp:
        out[0] = e[0]; out[-1] = e[h - 1]
    return out


def shifted(m):
    """a map shifted by +1: one fp32 addition"""
    with np.errstate(all="ignore"):
        return (np.float32(m) + np.float32(1)).astype(np.float32)


def reproject_view(src, mx, my, wrap, clamp):
    """ms_remap's arithmetic (np_ref.remap_linear) on the extended source with the maps shifted by (+1, +1)"""
    with np.errstate(all="ignore"):
        return np_ref.remap_linear(extend(src, wrap, clamp), shifted(mx), shifted(my))


def fnv1a0(data):
    """the host applications' checksum: FNV-1a's step from 0"""
    h = 0
    for b in np.asarray(data, np.uint8).reshape(-1).tolist():
        h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
    return h
