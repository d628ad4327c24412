"""numpy reference of the rig refinement with every view's principal point free (include/ms_stitch.h, the centre form of "Self-calibrating rigs"), built on
tests/rig_lens_ref.py: the rays, the solvers, the forward model and the synthetic rigs are its; here are the two centre columns of a view, the 92 terms of a match,
their accumulation with 6 rows a view, the prior and the Levenberg-Marquardt loop.  Written from the header's text; nothing here calls the library.

A lens is lens_ref's tuple (model, k, max_theta_deg), one a view; pp is (n, 2), the offsets (ox, oy); a match is (view_a, view_b, a, b) with a, b pixels centred on
the NOMINAL principal point.  Every function takes a dtype as rig_lens_ref's do."""
import math

import numpy as np

import rig_focal_ref as fr
import rig_lens_ref as lr

B = 6
TRI = B * (B + 1) // 2
G_I, G_J, H_II, H_JJ, H_IJ, OUTL = 1, 1 + B, 1 + 2 * B, 1 + 2 * B + TRI, 1 + 2 * B + 2 * TRI, 1 + 2 * B + 2 * TRI + B * B
N_TERMS = OUTL + 1                                                # 92
SYM = [(r, c) for r in range(B) for c in range(r, B)]


def tri(r, c):
    return SYM.index((r, c))


def lens_subset():
    """the places of rig_lens_ref's 46 terms among the 92, in its order"""
    idx = [0] + [G_I + k for k in range(4)] + [G_J + k for k in range(4)]
    for o in (H_II, H_JJ):
        idx += [o + tri(r, c) for r in range(4) for c in range(r, 4)]
    idx += [H_IJ + r * B + c for r in range(4) for c in range(4)]
    return idx + [OUTL]


def view_rows(n):
    """the rows of the 4n x 4n lens system inside the 6n x 6n one"""
    return np.array([B * v + k for v in range(n) for k in range(4)])


def centre_columns(lens, f, x, y, dtype=np.float64):
    """da/dox, da/doy (two lists of 3 arrays) of the unit ray of the centred pixels (x, y) (arrays, the offset already subtracted) at the focal f"""
    x = np.asarray(x, dtype); y = np.asarray(y, dtype)
    with np.errstate(all="ignore"):
        if lens[0] == "none":
            na = np.sqrt(x * x + y * y + f * f)
            a = [x / na, y / na, f / na]
            xy = (a[0] * a[1]) / na
            return [-((1.0 - a[0] * a[0]) / na), xy, (a[0] * a[2]) / na], [xy, -((1.0 - a[1] * a[1]) / na), (a[1] * a[2]) / na]
        xd = x / f; yd = y / f
        if lens[0] == "fisheye":
            k = lr._k(lens, 4, dtype)
            td = np.hypot(xd, yd)
            th, _, _ = lr.fisheye_solve(lens, td, dtype)
            c = td > 0
            tds = np.where(c, td, 1.0)
            st, ct = np.sin(th), np.cos(th)
            e0 = xd / tds; e1 = yd / tds
            slope = lr.fisheye_slope(k, th)
            g = st / tds; c0 = e0 / slope; c1 = e1 / slope; s0 = e1 * g; s1 = e0 * g
            one = np.ones_like(td); zero = np.zeros_like(td)
            A0 = [np.where(c, c0 * (ct * e0) + s0 * e1, one), np.where(c, c0 * (ct * e1) - s0 * e0, zero), np.where(c, -(c0 * st), zero)]
            A1 = [np.where(c, c1 * (ct * e0) - s1 * e1, zero), np.where(c, c1 * (ct * e1) + s1 * e0, one), np.where(c, -(c1 * st), zero)]
        else:
            k = lr._k(lens, 8, dtype)
            xu, yu, _, _, _ = lr.brown_solve(lens, xd, yd, dtype)
            _, _, J = lr.brown_forward(k, xu, yu)
            det = J[0] * J[3] - J[1] * J[2]
            n = np.sqrt(xu * xu + yu * yu + 1.0)
            a = [xu / n, yu / n, 1.0 / n]
            A = []
            for xs, ys in ((J[3] / det, -(J[2] / det)), (-(J[1] / det), J[0] / det)):
                t = a[0] * xs + a[1] * ys
                A.append([(xs - a[0] * t) / n, (ys - a[1] * t) / n, -(a[2] * t) / n])
            A0, A1 = A
        return [-(A0[q] / f) for q in range(3)], [-(A1[q] / f) for q in range(3)]


def _centre_side(f, R, lenses, view, px, m, dtype):
    """one side of every match: m (R da/dox), m (R da/doy), two lists of 3 arrays"""
    n = len(view)
    ex = [np.zeros(n, dtype) for _ in range(3)]; ey = [np.zeros(n, dtype) for _ in range(3)]
    for v in sorted(set(view.tolist())):
        s = view == v
        Rv = R[v]; ms_ = m[s]
        dx, dy = centre_columns(lenses[v], f[v], px[s, 0], px[s, 1], dtype)
        with np.errstate(all="ignore"):
            for r in range(3):
                ex[r][s] = ms_ * (Rv[r, 0] * dx[0] + Rv[r, 1] * dx[1] + Rv[r, 2] * dx[2])
                ey[r][s] = ms_ * (Rv[r, 0] * dy[0] + Rv[r, 1] * dy[1] + Rv[r, 2] * dy[2])
    return ex, ey


def _cast(f, R, pp, a, b, dtype):
    return tuple(np.asarray(x, np.float64).astype(dtype) for x in (f, R, pp, a, b))


def residual(f, R, pp, lenses, i, j, a, b, dtype=np.float64):
    """r = m (p - q) of every match at the offsets pp -> (3 arrays, seen)"""
    f, R, pp, a, b = _cast(f, R, pp, a, b, dtype)
    m = np.sqrt(f[i] * f[j])
    p, _, si = lr._side(f, R, lenses, i, a - pp[i], m, dtype)
    q, _, sj = lr._side(f, R, lenses, j, b - pp[j], m, dtype)
    return [m * (p[k] - q[k]) for k in range(3)], si & sj


def columns(f, R, pp, lenses, i, j, a, b, dtype=np.float64):
    """the four analytic centre columns of every match: dr/dox_i, dr/doy_i, dr/dox_j, dr/doy_j (each 3 arrays)"""
    f, R, pp, a, b = _cast(f, R, pp, a, b, dtype)
    m = np.sqrt(f[i] * f[j])
    ex, ey = _centre_side(f, R, lenses, i, a - pp[i], m, dtype)
    fx, fy = _centre_side(f, R, lenses, j, b - pp[j], m, dtype)
    return ex, ey, [-c for c in fx], [-c for c in fy]


def terms(f, R, pp, lenses, i, j, a, b, h, dtype=np.float64, branch=None):
    """the 92 terms of every match (n, 92) in the header's layout, s (n,) and seen (n,).  A match that is not seen: cost +infinity, every other term 0.
    branch: as rig_lens_ref.terms'"""
    f, R, pp, a, b = _cast(f, R, pp, a, b, dtype)
    h = dtype(h)
    m = np.sqrt(f[i] * f[j])
    pa = a - pp[i]; pb = b - pp[j]
    p, ti, si = lr._side(f, R, lenses, i, pa, m, dtype)
    q, tj, sj = lr._side(f, R, lenses, j, pb, m, dtype)
    ex, ey = _centre_side(f, R, lenses, i, pa, m, dtype)
    fx, fy = _centre_side(f, R, lenses, j, pb, m, dtype)
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
        ci = [[0.5 * r[k] + ti[k] for k in range(3)], ex, ey]
        cj = [[0.5 * r[k] - tj[k] for k in range(3)], [-c for c in fx], [-c for c in fy]]
        T = np.zeros((len(s2), N_TERMS), dtype)
        T[:, 0] = rho
        ur = fr._cross(u, r); vr = fr._cross(v, r)
        for k in range(3):
            T[:, G_I + k] = w * ur[k]; T[:, G_J + k] = -(w * vr[k])
        for n in range(3):
            T[:, G_I + 3 + n] = w * fr._dot(ci[n], r); T[:, G_J + 3 + n] = w * fr._dot(cj[n], r)
        for o, x, c, sign in ((H_II, u, ci, 1), (H_JJ, v, cj, -1)):
            T[:, o + tri(0, 0)] = w * (x[1] * x[1] + x[2] * x[2]); T[:, o + tri(0, 1)] = -(w * (x[0] * x[1])); T[:, o + tri(0, 2)] = -(w * (x[0] * x[2]))
            T[:, o + tri(1, 1)] = w * (x[0] * x[0] + x[2] * x[2]); T[:, o + tri(1, 2)] = -(w * (x[1] * x[2])); T[:, o + tri(2, 2)] = w * (x[0] * x[0] + x[1] * x[1])
            for n in range(3):
                xc = fr._cross(x, c[n])
                for k in range(3):
                    T[:, o + tri(k, 3 + n)] = w * xc[k] if sign > 0 else -(w * xc[k])
                for n2 in range(n, 3):
                    T[:, o + tri(3 + n, 3 + n2)] = w * fr._dot(c[n], c[n2])
        diag = [u[1] * v[1] + u[2] * v[2], u[0] * v[0] + u[2] * v[2], u[0] * v[0] + u[1] * v[1]]
        for rr_ in range(3):
            for c in range(3):
                T[:, H_IJ + B * rr_ + c] = -(w * diag[rr_]) if rr_ == c else w * (v[rr_] * u[c])
        for n in range(3):
            ucj = fr._cross(u, cj[n]); vci = fr._cross(v, ci[n])
            for k in range(3):
                T[:, H_IJ + B * k + 3 + n] = w * ucj[k]
                T[:, H_IJ + B * (3 + n) + k] = -(w * vci[k])
            for n2 in range(3):
                T[:, H_IJ + B * (3 + n) + 3 + n2] = w * fr._dot(ci[n], cj[n2])
        T[:, OUTL] = out
    T[~seen] = 0.0
    T[~seen, 0] = np.inf
    return T, s, seen


def _blocks(T):
    def sym(o):
        M = np.empty((len(T), B, B), T.dtype)
        for k, (r, c) in enumerate(SYM):
            M[:, r, c] = T[:, o + k]; M[:, c, r] = T[:, o + k]
        return M
    return T[:, G_I:G_J], T[:, G_J:H_II], sym(H_II), sym(H_JJ), T[:, H_IJ:OUTL].reshape(-1, B, B)


def _sum_terms(X, i, j, n, order=None):
    """cost, H (6n x 6n), g (6n) of the terms X, summed match by match in the given order (order: a permutation of the matches)"""
    gi, gj, Hii, Hjj, Hij = _blocks(X)
    cost = X.dtype.type(0.0); H = np.zeros((B * n, B * n), X.dtype); g = np.zeros(B * n, X.dtype)
    for k in (range(len(X)) if order is None else order):
        I = slice(B * i[k], B * i[k] + B); J = slice(B * j[k], B * j[k] + B)
        cost += X[k, 0]
        g[I] += gi[k]; g[J] += gj[k]
        H[I, I] += Hii[k]; H[J, J] += Hjj[k]; H[I, J] += Hij[k]; H[J, I] += Hij[k].T
    return cost, H, g


def accumulate(f, R, pp, lenses, matches, h=0.0, with_abs=False, dtype=np.float64, order=None):
    """cost, H (6n x 6n), g (6n) at the cameras over ALL matches, no prior; with_abs: also the sums of the terms' absolute values"""
    i, j, a, b = fr.unpack(matches)
    T, _, _ = terms(f, R, pp, lenses, i, j, a, b, h, dtype)
    res = list(_sum_terms(T, i, j, len(R), order))
    if with_abs:
        res += list(_sum_terms(np.abs(T), i, j, len(R), order))
    res[0] = float(res[0]) if dtype is np.float64 else res[0]
    return tuple(res)


def term_deviation(f, R, pp, lenses, matches, h=0.0):
    """rig_lens_ref.term_deviation over the 92 terms: sum |T64 - Tlong| over the matches per entry of cost, H and g, in units of 2^-52 S -> the largest"""
    i, j, a, b = fr.unpack(matches)
    T64, _, _ = terms(f, R, pp, lenses, i, j, a, b, h)
    TL, _, _ = terms(f, R, pp, lenses, i, j, a, b, h, np.longdouble, branch=T64[:, OUTL] > 0)
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


def all_seen(f, R, pp, lenses, matches):
    i, j, a, b = fr.unpack(matches)
    return bool(residual(f, R, pp, lenses, i, j, a, b)[1].all())


def shift(matches, pp):
    """the matches with the offsets subtracted in double: what ms_rig_lens_accumulate takes for the 46-sum pin"""
    pp = np.asarray(pp, np.float64)
    return [(va, vb, np.asarray(a, np.float64) - pp[va], np.asarray(b, np.float64) - pp[vb]) for va, vb, a, b in matches]


def selection(n, anchor, shared):
    """P (6n x m): the solved unknowns as combinations of the full ones -- the anchor's rotation left out; one focal column of ones where the focal is shared"""
    cols = []
    for v in range(n):
        for k in range(B):
            if (k < 3 and v == anchor) or (k == 3 and shared):
                continue
            e = np.zeros(B * n); e[B * v + k] = 1.0; cols.append(e)
    if shared:
        e = np.zeros(B * n); e[3::B] = 1.0; cols.append(e)
    return np.array(cols).T


def apply_step(f, R, pp, full):
    """the cameras after the step `full` (6n): R_v <- Exp(delta_v) R_v, f_v <- f_v exp(d_v), o_v <- o_v + d"""
    import rig_ref as rr
    n = len(R)
    Rn = np.array([R[v] if not full[B * v:B * v + 3].any() else rr.exp_so3(full[B * v:B * v + 3]) @ R[v] for v in range(n)])
    return np.array([f[v] * math.exp(full[B * v + 3]) for v in range(n)]), Rn, np.array([[pp[v][0] + full[B * v + 4], pp[v][1] + full[B * v + 5]] for v in range(n)])


def refine(f_in, R_in, pp_in, lenses, matches, anchor=0, shared_focal=False, huber_px=0.0, max_iters=50, step_tol=1e-10, min_pair_matches=4, pp_prior=0.0, order=None):
    """the Levenberg-Marquardt loop of the contract with the prior w = pp_prior on the centres -> (f, R, pp, info dict).  order: a permutation of the USED matches
    in which the sums are taken (a second summation order of the same reference)"""
    import rig_ref as rr
    f = np.array(f_in, np.float64); R = np.array(R_in, np.float64); pp = np.array(pp_in, np.float64); p0 = pp.copy()
    n = len(R)
    i, j, _, _ = fr.unpack(matches)
    counts = {}
    for k in range(len(matches)):
        counts[(i[k], j[k])] = counts.get((i[k], j[k]), 0) + 1
    used = [m for k, m in enumerate(matches) if counts[(i[k], j[k])] >= min_pair_matches]
    if not all_seen(f, R, pp, lenses, used):
        raise ValueError("a pixel is not seen at the input cameras")
    P = selection(n, anchor, shared_focal)
    w = float(pp_prior)
    centre = np.array([B * v + k for v in range(n) for k in (4, 5)])

    def system(f, R, pp):
        cost, H, g = accumulate(f, R, pp, lenses, used, huber_px, order=order)
        if w > 0:
            d = (pp - p0).reshape(-1)
            cost = cost + w * float(np.sum(d * d))
            H[centre, centre] += w
            g[centre] += w * d
        return cost, H, g

    lam, iters = 1e-3, 0
    cost, H, g = system(f, R, pp)
    cost0 = cost

    def done(reason):
        ui, uj, ua, ub = fr.unpack(used)
        _, s, _ = terms(f, R, pp, lenses, ui, uj, ua, ub, huber_px)
        return f, R, pp, dict(iterations=iters, stop_reason=reason, cost_initial=cost0, cost_final=cost, matches_used=len(used),
                              pairs_used=sum(1 for c in counts.values() if c >= min_pair_matches), pairs_ignored=sum(1 for c in counts.values() if c < min_pair_matches),
                              outliers=int((s > huber_px).sum()) if huber_px > 0 else 0, max_rotation_rad=max(rr.angle(R[v], R_in[v]) for v in range(n)),
                              max_focal_ratio=max(max(f[v] / f_in[v], f_in[v] / f[v]) for v in range(n)), max_pp_shift=float(np.max(np.abs(pp - p0))))

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
        full = P @ delta
        ft, Rt, pt = apply_step(f, R, pp, full)
        scaled = np.abs(full)
        scaled[centre] /= np.repeat(f, 2)                     # the centre steps in radians
        ct, Ht, gt = system(ft, Rt, pt)
        iters += 1
        if ct <= cost:
            f, R, pp, cost, H, g = ft, Rt, pt, ct, Ht, gt
            lam = max(lam / 10.0, 1e-12)
            if np.max(scaled) < step_tol:
                return done(fr.CONVERGED)
        else:
            lam *= 10.0
            if lam > 1e12:
                return done(fr.STALLED)
        if iters >= max_iters:
            return done(fr.ITERATION_LIMIT)


def make_pp_matches(ft, Rt, ppt, lenses, pairs, per_pair, rng, **kw):
    """rig_lens_ref.make_lens_matches through the true cameras, then moved onto the nominal centre: a pixel measured from the nominal principal point is the true
    centred pixel plus the true offset"""
    ppt = np.asarray(ppt, np.float64)
    return [(i, j, a + ppt[i], b + ppt[j]) for i, j, a, b in lr.make_lens_matches(ft, Rt, lenses, pairs, per_pair, rng, **kw)]
