"""numpy reference of the inverse lens model and of the focal-and-rotation bundle adjustment under fixed lenses (include/ms_stitch.h: ms_lens_unproject and the lens
form of "Self-calibrating rigs"), built on tests/lens_ref.py (the forward model, the lens tuples) and tests/rig_focal_ref.py (the layout of the 46 terms, the selection
matrix, the step).  Written from the header's text, vectorised over the points; nothing here calls the library.

Every function takes a dtype: float64 is the reference, numpy.longdouble the yardstick for how far float64 terms lie from the exact ones (term_deviation).
A lens is lens_ref's tuple (model, k, max_theta_deg); a match is rig_focal_ref's (view_a, view_b, a, b) with a, b centred pixels."""
import math

import numpy as np

import lens_ref as L
import rig_focal_ref as fr

N_TERMS = fr.N_TERMS


def _k(lens, n, dtype):
    k = list(lens[1]) + [0.0] * (n - len(lens[1]))
    return [dtype(v) for v in k]


def limit(lens, dtype=np.float64):
    """where the field ends in the solver's variable: theta_d(max_theta) for a fisheye, tan(max_theta) for Brown"""
    mt = dtype(L.max_theta(lens))
    return fisheye_profile(_k(lens, 4, dtype), mt) if lens[0] == "fisheye" else np.tan(mt)


def fisheye_profile(k, t):
    t2 = t * t
    return t * (1.0 + (((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2)


def fisheye_slope(k, t):
    t2 = t * t
    return 1.0 + ((((9.0 * k[3]) * t2 + 7.0 * k[2]) * t2 + 5.0 * k[1]) * t2 + 3.0 * k[0]) * t2


def fisheye_solve(lens, td, dtype=np.float64):
    """theta of theta_d (array) on [0, max_theta] -> (theta, seen, rounds): the safeguarded Newton iteration of the header"""
    k = _k(lens, 4, dtype)
    mt = dtype(L.max_theta(lens))
    td = np.asarray(td, dtype)
    with np.errstate(all="ignore"):
        seen = td <= limit(lens, dtype)
        lo = np.zeros_like(td); hi = np.full_like(td, mt); t = np.minimum(td, mt)
        live = seen.copy()
        rounds = 0
        for _ in range(60):
            if not live.any():
                break
            rounds += 1
            g = fisheye_profile(k, t) - td; d = fisheye_slope(k, t)
            hi = np.where(live & (g > 0), t, hi); lo = np.where(live & ~(g > 0), t, lo)
            mid = 0.5 * (lo + hi)
            tn = np.where(d > 0, t - g / d, mid)
            tn = np.where((tn >= lo) & (tn <= hi), tn, mid)
            live = live & (tn != t)
            t = np.where(live, tn, t)
    return t, seen, rounds


def brown_forward(k, x, y):
    """-> xd, yd, J (4 arrays: dxd/dx, dxd/dy, dyd/dx, dyd/dy)"""
    r2 = x * x + y * y
    N = 1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2; D = 1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2
    dN = (3.0 * k[4] * r2 + 2.0 * k[1]) * r2 + k[0]; dD = (3.0 * k[7] * r2 + 2.0 * k[6]) * r2 + k[5]
    cd = N / D; dc = (dN * D - N * dD) / (D * D)
    xd = x * cd + 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x)
    yd = y * cd + k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y
    off = 2.0 * x * y * dc + 2.0 * k[2] * x + 2.0 * k[3] * y
    return xd, yd, (cd + 2.0 * x * x * dc + 2.0 * k[2] * y + 6.0 * k[3] * x, off, off, cd + 2.0 * y * y * dc + 6.0 * k[2] * y + 2.0 * k[3] * x)


def brown_solve(lens, xd, yd, dtype=np.float64, stop=2.0 ** -50):
    """(x, y) of (xd, yd) (arrays) -> (x, y, seen, settled, rounds): the 2-D Newton iteration of the header; stop: the relative step at which it counts as settled"""
    k = _k(lens, 8, dtype)
    xd = np.asarray(xd, dtype); yd = np.asarray(yd, dtype)
    x = xd.copy(); y = yd.copy()
    settled = np.zeros(x.shape, bool); failed = np.zeros(x.shape, bool)
    rounds = 0
    with np.errstate(all="ignore"):
        for _ in range(50):
            live = ~settled & ~failed
            if not live.any():
                break
            rounds += 1
            fx, fy, J = brown_forward(k, x, y)
            det = J[0] * J[3] - J[1] * J[2]; ex = fx - xd; ey = fy - yd
            failed |= live & ~((np.abs(det) > 0) & np.isfinite(det))
            dx = (J[3] * ex - J[1] * ey) / det; dy = (J[0] * ey - J[2] * ex) / det
            xn = x - dx; yn = y - dy
            live &= ~failed
            failed |= live & ~(np.isfinite(xn) & np.isfinite(yn))
            live &= ~failed
            x = np.where(live, xn, x); y = np.where(live, yn, y)
            settled |= live & (np.maximum(np.abs(dx), np.abs(dy)) <= stop * np.maximum(1.0, np.maximum(np.abs(x), np.abs(y))))
        seen = settled & ~failed & (np.hypot(x, y) <= limit(lens, dtype))
    return x, y, seen, settled & ~failed, rounds


def view_ray(lens, xd, yd, dtype=np.float64):
    """distorted normalised coordinates (arrays) -> (a (3 arrays), da/ds (3 arrays), seen), s = ln f with the pixel held: the unit ray and how it moves with the focal.
    Rows that are not seen hold anything."""
    xd = np.asarray(xd, dtype); yd = np.asarray(yd, dtype)
    with np.errstate(all="ignore"):
        if lens[0] == "none":
            n = np.sqrt(xd * xd + yd * yd + 1.0)
            a = [xd / n, yd / n, 1.0 / n]
            return a, [a[2] * (0.0 - a[2] * a[0]), a[2] * (0.0 - a[2] * a[1]), a[2] * (1.0 - a[2] * a[2])], np.isfinite(n)
        if lens[0] == "fisheye":
            k = _k(lens, 4, dtype)
            td = np.hypot(xd, yd)
            th, seen, _ = fisheye_solve(lens, td, dtype)
            c = td > 0
            tds = np.where(c, td, 1.0)
            st, ct = np.sin(th), np.cos(th)
            tp = -td / fisheye_slope(k, th); e0 = xd / tds; e1 = yd / tds
            a = [np.where(c, st * xd / tds, 0.0), np.where(c, st * yd / tds, 0.0), np.where(c, ct, 1.0)]
            d = [np.where(c, tp * (ct * e0), 0.0), np.where(c, tp * (ct * e1), 0.0), np.where(c, -(tp * st), 0.0)]
            return a, d, seen
        k = _k(lens, 8, dtype)
        x, y, seen, _, _ = brown_solve(lens, xd, yd, dtype)
        _, _, J = brown_forward(k, x, y)
        det = J[0] * J[3] - J[1] * J[2]
        seen = seen & (np.abs(det) > 0)
        xs = -((J[3] * xd - J[1] * yd) / det); ys = -((J[0] * yd - J[2] * xd) / det)
        n = np.sqrt(x * x + y * y + 1.0)
        a = [x / n, y / n, 1.0 / n]
        dot = a[0] * xs + a[1] * ys
        return a, [(xs - a[0] * dot) / n, (ys - a[1] * dot) / n, -(a[2] * dot) / n], seen


def unproject(K, lens, px, py, dtype=np.float64):
    """source pixels (arrays) -> (rays (n, 3), seen (n,)); unseen rows are (0, 0, 0)"""
    K = np.asarray(K, np.float64).reshape(3, 3).astype(dtype)
    px = np.atleast_1d(np.asarray(px, dtype)); py = np.atleast_1d(np.asarray(py, dtype))
    with np.errstate(all="ignore"):
        yd = (py - K[1, 2]) / K[1, 1]; xd = (px - K[0, 2] - K[0, 1] * yd) / K[0, 0]
        a, _, seen = view_ray(lens, xd, yd, dtype)
        seen = seen & np.isfinite(px) & np.isfinite(py)
        rays = np.stack([np.where(seen, c, 0.0) for c in a], axis=-1)
    return rays, seen


def _side(f, R, lenses, view, px, m, dtype):
    """one side of every match: p = R a (3 arrays), t = m R da/ds (3 arrays), seen.  A view without a lens takes the pinhole contract's expressions."""
    n = len(view)
    p = [np.zeros(n, dtype) for _ in range(3)]; t = [np.zeros(n, dtype) for _ in range(3)]; seen = np.ones(n, bool)
    for v in sorted(set(view.tolist())):
        s = view == v
        fv = f[v]; Rv = R[v]; x = px[s, 0]; y = px[s, 1]; ms_ = m[s]
        with np.errstate(all="ignore"):
            if lenses[v][0] == "none":
                na = np.sqrt(x * x + y * y + fv * fv)
                a = [x / na, y / na, fv / na]
                pv = [Rv[r, 0] * a[0] + Rv[r, 1] * a[1] + Rv[r, 2] * a[2] for r in range(3)]
                ma = ms_ * a[2]
                tv = [ma * (Rv[r, 2] - a[2] * pv[r]) for r in range(3)]
                ok = np.ones(len(x), bool)
            else:
                a, d, ok = view_ray(lenses[v], x / fv, y / fv, dtype)
                pv = [Rv[r, 0] * a[0] + Rv[r, 1] * a[1] + Rv[r, 2] * a[2] for r in range(3)]
                tv = [ms_ * (Rv[r, 0] * d[0] + Rv[r, 1] * d[1] + Rv[r, 2] * d[2]) for r in range(3)]
        for r in range(3):
            p[r][s] = pv[r]; t[r][s] = tv[r]
        seen[s] = ok
    return p, t, seen


def terms(f, R, lenses, i, j, a, b, h, dtype=np.float64, branch=None):
    """the 46 terms of every match (n, 46) in the header's layout, s (n,) and seen (n,).  A match that is not seen: cost +infinity, every other term 0.
    branch: the matches to put on Huber's linear branch instead of those with s > h (term_deviation: both precisions on one branch)"""
    f = np.asarray(f, np.float64).astype(dtype); R = np.asarray(R, np.float64).astype(dtype)
    a = np.asarray(a, np.float64).astype(dtype); b = np.asarray(b, np.float64).astype(dtype)
    h = dtype(h)
    m = np.sqrt(f[i] * f[j])
    p, ti, si = _side(f, R, lenses, i, a, m, dtype)
    q, tj, sj = _side(f, R, lenses, j, b, m, dtype)
    seen = si & sj
    with np.errstate(all="ignore"):
        u = [m * p[k] for k in range(3)]; v = [m * q[k] for k in range(3)]
        r = [m * (p[k] - q[k]) for k in range(3)]
        s2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
        s = np.sqrt(s2)
        w = np.ones_like(s2); rho = s2.copy(); out = np.zeros_like(s2)
        if h > 0:
            o = (s > h) if branch is None else branch
            w[o] = h / s[o]
            rho[o] = (2.0 * h) * s[o] - h * h
            out[o] = 1.0
        ci = [0.5 * r[k] + ti[k] for k in range(3)]
        cj = [0.5 * r[k] - tj[k] for k in range(3)]
        T = np.empty((len(s2), N_TERMS), dtype)
        T[:, 0] = rho
        ur = fr._cross(u, r); vr = fr._cross(v, r)
        for k in range(3):
            T[:, 1 + k] = w * ur[k]; T[:, 5 + k] = -(w * vr[k])
        T[:, 4] = w * fr._dot(ci, r); T[:, 8] = w * fr._dot(cj, r)
        for o, x, c, sign in ((9, u, ci, 1), (19, v, cj, -1)):
            xc = fr._cross(x, c)
            T[:, o] = w * (x[1] * x[1] + x[2] * x[2]); T[:, o + 1] = -(w * (x[0] * x[1])); T[:, o + 2] = -(w * (x[0] * x[2]))
            T[:, o + 4] = w * (x[0] * x[0] + x[2] * x[2]); T[:, o + 5] = -(w * (x[1] * x[2])); T[:, o + 7] = w * (x[0] * x[0] + x[1] * x[1])
            for k, e in enumerate((3, 6, 8)):
                T[:, o + e] = w * xc[k] if sign > 0 else -(w * xc[k])
            T[:, o + 9] = w * fr._dot(c, c)
        ucj = fr._cross(u, cj); vci = fr._cross(v, ci)
        diag = [u[1] * v[1] + u[2] * v[2], u[0] * v[0] + u[2] * v[2], u[0] * v[0] + u[1] * v[1]]
        for rr_ in range(3):
            for c in range(3):
                T[:, 29 + 4 * rr_ + c] = -(w * diag[rr_]) if rr_ == c else w * (v[rr_] * u[c])
            T[:, 29 + 4 * rr_ + 3] = w * ucj[rr_]
            T[:, 41 + rr_] = -(w * vci[rr_])
        T[:, 44] = w * fr._dot(ci, cj)
        T[:, 45] = out
    T[~seen] = 0.0
    T[~seen, 0] = np.inf
    return T, s, seen


def _sum_terms(X, i, j, n):
    """cost, H (4n x 4n), g (4n) of the terms X, summed match by match in the given order"""
    gi, gj, Hii, Hjj, Hij = fr._blocks(X)
    cost = X.dtype.type(0.0); H = np.zeros((4 * n, 4 * n), X.dtype); g = np.zeros(4 * n, X.dtype)
    for k in range(len(X)):
        I = slice(4 * i[k], 4 * i[k] + 4); J = slice(4 * j[k], 4 * j[k] + 4)
        cost += X[k, 0]
        g[I] += gi[k]; g[J] += gj[k]
        H[I, I] += Hii[k]; H[J, J] += Hjj[k]; H[I, J] += Hij[k]; H[J, I] += Hij[k].T
    return cost, H, g


def accumulate(f, R, lenses, matches, h=0.0, with_abs=False, dtype=np.float64):
    """cost, H (4n x 4n), g (4n) at the cameras over ALL matches, summed match by match in the given order; with_abs: also the sums of the terms' absolute values"""
    i, j, a, b = fr.unpack(matches)
    T, _, _ = terms(f, R, lenses, i, j, a, b, h, dtype)
    res = list(_sum_terms(T, i, j, len(R)))
    if with_abs:
        res += list(_sum_terms(np.abs(T), i, j, len(R)))
    res[0] = float(res[0]) if dtype is np.float64 else res[0]
    return tuple(res)


def term_deviation(f, R, lenses, matches, h=0.0):
    """How far the float64 terms lie from the exact ones, entry by entry of cost, H and g: sum |T64 - Tlong| over the matches, in units of 2^-52 S, S the sum of the
    float64 terms' absolute values (0 where S is 0) -> the largest over all entries.  Huber's branch is taken from the float64 residuals on both sides (a threshold
    that IS a residual, the median, would otherwise flip with the last bit; the two branches meet there with equal value and slope)."""
    i, j, a, b = fr.unpack(matches)
    T64, _, _ = terms(f, R, lenses, i, j, a, b, h)
    TL, _, _ = terms(f, R, lenses, i, j, a, b, h, np.longdouble, branch=T64[:, 45] > 0)
    D = np.abs(T64.astype(np.longdouble) - TL).astype(np.float64)
    n = len(R)
    dc, dH, dg = _sum_terms(D, i, j, n)
    sc, sH, sg = _sum_terms(np.abs(T64), i, j, n)
    worst = 0.0
    for d, s in ((np.array([dc]), np.array([sc])), (dH, sH), (dg, sg)):
        nz = s > 0
        if nz.any():
            worst = max(worst, float(np.max(d[nz] / (2.0 ** -52 * s[nz]))))
    return worst


def cost_only(f, R, lenses, matches, h=0.0):
    i, j, a, b = fr.unpack(matches)
    return float(terms(f, R, lenses, i, j, a, b, h)[0][:, 0].sum())


def all_seen(f, R, lenses, matches):
    i, j, a, b = fr.unpack(matches)
    return bool(terms(f, R, lenses, i, j, a, b, 0.0)[2].all())


def refine(f_in, R_in, lenses, matches, anchor=0, shared_focal=False, huber_px=0.0, max_iters=50, step_tol=1e-10, min_pair_matches=4):
    """the Levenberg-Marquardt loop of the contract (rig_focal_ref.refine's, with the terms above: a trial that loses a pixel has an infinite cost and is rejected)
    -> (f, R, info dict)"""
    import rig_ref as rr
    f = np.array(f_in, np.float64); R = np.array(R_in, np.float64)
    n = len(R)
    i, j, _, _ = fr.unpack(matches)
    counts = {}
    for k in range(len(matches)):
        counts[(i[k], j[k])] = counts.get((i[k], j[k]), 0) + 1
    used = [m for k, m in enumerate(matches) if counts[(i[k], j[k])] >= min_pair_matches]
    if not all_seen(f, R, lenses, used):
        raise ValueError("a pixel is not seen at the input cameras")
    P = fr.selection(n, anchor, shared_focal)
    lam, iters = 1e-3, 0
    cost, H, g = accumulate(f, R, lenses, used, huber_px)
    cost0 = cost

    def done(reason):
        ui, uj, ua, ub = fr.unpack(used)
        _, s, _ = terms(f, R, lenses, ui, uj, ua, ub, huber_px)
        return f, R, dict(iterations=iters, stop_reason=reason, cost_initial=cost0, cost_final=cost, matches_used=len(used),
                          pairs_used=sum(1 for c in counts.values() if c >= min_pair_matches), pairs_ignored=sum(1 for c in counts.values() if c < min_pair_matches),
                          outliers=int((s > huber_px).sum()) if huber_px > 0 else 0, max_rotation_rad=max(rr.angle(R[v], R_in[v]) for v in range(n)),
                          max_focal_ratio=max(max(f[v] / f_in[v], f_in[v] / f[v]) for v in range(n)))

    while True:
        while True:
            Hr = P.T @ H @ P
            A = Hr + lam * np.diag(np.diag(Hr))
            try:
                np.linalg.cholesky(A)
                delta = np.linalg.solve(A, -(P.T @ g))
                ok = bool(np.all(np.isfinite(delta)))
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                break
            lam *= 10.0; iters += 1
            if lam > 1e12:
                return done(fr.STALLED)
            if iters >= max_iters:
                return done(fr.ITERATION_LIMIT)
        ft, Rt = fr.apply_step(f, R, P @ delta)
        ct, Ht, gt = accumulate(ft, Rt, lenses, used, huber_px)
        iters += 1
        if ct <= cost:
            f, R, cost, H, g = ft, Rt, ct, Ht, gt
            lam = max(lam / 10.0, 1e-12)
            if np.max(np.abs(delta)) < step_tol:
                return done(fr.CONVERGED)
        else:
            lam *= 10.0
            if lam > 1e12:
                return done(fr.STALLED)
        if iters >= max_iters:
            return done(fr.ITERATION_LIMIT)


# ---- synthetic lens rigs ----------------------------------------------------------------------------------------------------------------------------
def centred_pixels(f, lens, rays):
    """camera rays (n, 3) -> (centred pixels (n, 2), seen) through the FORWARD model (lens_ref.project) at the focal f, principal point 0"""
    K = [[f, 0.0, 0.0], [0.0, f, 0.0], [0.0, 0.0, 1.0]]
    px, py, seen = L.project(K, lens, rays[:, 0], rays[:, 1], rays[:, 2])
    return np.stack([px, py], axis=-1), seen


def make_lens_matches(ft, Rt, lenses, pairs, per_pair, rng, noise_px=0.0, outlier_frac=0.0, spread_deg=20.0, outlier_px=(0.5, 1.5), margin_deg=2.0):
    """per_pair matches (a number, or one per pair) of every pair: world rays around the bisector of the two optical axes, seen through the TRUE cameras and lenses by
    the forward model; rays either lens does not see, or sees within margin_deg of its limit (of 88 degrees for a view without a lens), are drawn again"""
    import rig_ref as rr
    out = []
    for k, (i, j) in enumerate(pairs):
        want = per_pair[k] if isinstance(per_pair, (list, tuple)) else per_pair
        mid = Rt[i][:, 2] + Rt[j][:, 2]
        mid /= np.linalg.norm(mid)
        got = 0
        while got < want:
            d = rr.exp_so3(np.radians(rng.uniform(-spread_deg, spread_deg, 3))) @ mid
            px = []
            for v in (i, j):
                c = Rt[v].T @ d
                th = math.degrees(math.atan2(math.hypot(c[0], c[1]), c[2]))
                lim = math.degrees(L.max_theta(lenses[v])) if lenses[v][0] != "none" else 88.0
                if th > lim - margin_deg:
                    break
                p, seen = centred_pixels(ft[v], lenses[v], c[None, :])
                assert seen[0]
                px.append(p[0])
            if len(px) < 2:
                continue
            a, b = px
            if noise_px > 0:
                a = a + rng.normal(0, noise_px, 2); b = b + rng.normal(0, noise_px, 2)
            if outlier_frac > 0 and rng.uniform() < outlier_frac:
                t = rng.uniform(0.0, 2.0 * math.pi)
                b = b + rng.uniform(*outlier_px) * np.array([math.cos(t), math.sin(t)])
            out.append((i, j, a, b))
            got += 1
    return out
