"""numpy reference of the rig refinement with the shared lens's coefficients free (include/ms_stitch.h, the coefficient form of "Self-calibrating rigs"), built on
tests/rig_lens_ref.py: the 46 terms, the solvers, the forward model and the synthetic rigs are its; here are the G coefficient columns of a match, the border terms,
the accumulation with the coefficient rows last, the profile rule of ms_lens_check and the Levenberg-Marquardt loop with the trial-lens rule.  Written from the
header's text; nothing here calls the library.

A lens is lens_ref's tuple (model, k, max_theta_deg), ONE for the whole rig; `free` is the bit mask free_coeffs.  Every function takes a dtype as rig_lens_ref's do."""
import math

import numpy as np

import lens_ref as L
import rig_focal_ref as fr
import rig_lens_ref as lr

ALLOWED = {"fisheye": (0, 1, 2, 3), "brown": (0, 1, 2, 3, 4)}
PROFILE_STEPS = 4096


def free_list(free):
    return [b for b in range(32) if free >> b & 1]


def n_border(G):
    return G + G * (G + 1) // 2 + 8 * G


def with_k(lens, k):
    return (lens[0], tuple(float(v) for v in k), lens[2])


def k8(lens):
    return list(lens[1]) + [0.0] * (8 - len(lens[1]))


def lens_ok(lens):
    """ms_lens_check's profile rule: strictly increasing and finite over 4096 uniform samples of [0, max_theta] (fisheye: theta_d(theta)) or [0, tan max_theta]
    (Brown: r cdist(r))"""
    k = k8(lens)
    if not all(math.isfinite(v) for v in k):
        return False
    mt = L.max_theta(lens)
    end = mt if lens[0] == "fisheye" else math.tan(mt)
    a = end * np.arange(1, PROFILE_STEPS + 1, dtype=np.float64) / PROFILE_STEPS
    with np.errstate(all="ignore"):
        if lens[0] == "fisheye":
            p = lr.fisheye_profile(k, a)
        else:
            r2 = a * a
            p = a * ((1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2))
    return bool(np.all(np.isfinite(p)) and np.all(np.diff(np.concatenate([[0.0], p])) > 0))


def dray(lens, idx, xd, yd, dtype=np.float64):
    """d a / d k[idx] of the unit ray of the distorted normalised coordinates (arrays), the pixel and the focal held -> 3 arrays (anything where not seen)"""
    xd = np.asarray(xd, dtype); yd = np.asarray(yd, dtype)
    with np.errstate(all="ignore"):
        if lens[0] == "fisheye":
            k = lr._k(lens, 4, dtype)
            td = np.hypot(xd, yd)
            th, _, _ = lr.fisheye_solve(lens, td, dtype)
            c = td > 0
            tds = np.where(c, td, 1.0)
            st, ct = np.sin(th), np.cos(th)
            e0 = xd / tds; e1 = yd / tds
            t2 = th * th
            q = th * t2
            for _ in range(idx):
                q = q * t2
            tp = -q / lr.fisheye_slope(k, th)
            return [np.where(c, tp * (ct * e0), 0.0), np.where(c, tp * (ct * e1), 0.0), np.where(c, -(tp * st), 0.0)]
        k = lr._k(lens, 8, dtype)
        x, y, _, _, _ = lr.brown_solve(lens, xd, yd, dtype)
        _, _, J = lr.brown_forward(k, x, y)
        det = J[0] * J[3] - J[1] * J[2]
        r2 = x * x + y * y
        if idx == 2:
            F0 = (2.0 * x) * y; F1 = r2 + (2.0 * y) * y
        elif idx == 3:
            F0 = r2 + (2.0 * x) * x; F1 = (2.0 * x) * y
        else:
            D = 1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2
            s = r2 / D if idx == 0 else (r2 * r2) / D if idx == 1 else ((r2 * r2) * r2) / D
            F0 = x * s; F1 = y * s
        xs = -((J[3] * F0 - J[1] * F1) / det); ys = -((J[0] * F1 - J[2] * F0) / det)
        n = np.sqrt(x * x + y * y + 1.0)
        a = [x / n, y / n, 1.0 / n]
        t = a[0] * xs + a[1] * ys
        return [(xs - a[0] * t) / n, (ys - a[1] * t) / n, -(a[2] * t) / n]


def _cast(f, R, a, b, dtype):
    return (np.asarray(f, np.float64).astype(dtype), np.asarray(R, np.float64).astype(dtype), np.asarray(a, np.float64).astype(dtype),
            np.asarray(b, np.float64).astype(dtype))


def residual(f, R, lens, i, j, a, b, dtype=np.float64):
    """r = m (p - q) of every match -> (3 arrays, seen)"""
    f, R, a, b = _cast(f, R, a, b, dtype)
    lenses = [lens] * len(R)
    m = np.sqrt(f[i] * f[j])
    p, _, si = lr._side(f, R, lenses, i, a, m, dtype)
    q, _, sj = lr._side(f, R, lenses, j, b, m, dtype)
    return [m * (p[k] - q[k]) for k in range(3)], si & sj


def columns(f, R, lens, free, i, j, a, b, dtype=np.float64):
    """the G analytic columns e_n = m (R_i da/dk_n) - m (R_j db/dk_n) of every match -> a list of G lists of 3 arrays"""
    f, R, a, b = _cast(f, R, a, b, dtype)
    m = np.sqrt(f[i] * f[j])
    Ri, Rj = R[i], R[j]
    E = []
    for idx in free_list(free):
        da = dray(lens, idx, a[:, 0] / f[i], a[:, 1] / f[i], dtype); db = dray(lens, idx, b[:, 0] / f[j], b[:, 1] / f[j], dtype)
        E.append([m * (Ri[:, k, 0] * da[0] + Ri[:, k, 1] * da[1] + Ri[:, k, 2] * da[2]) - m * (Rj[:, k, 0] * db[0] + Rj[:, k, 1] * db[1] + Rj[:, k, 2] * db[2])
                  for k in range(3)])
    return E


def terms(f, R, lens, free, i, j, a, b, h, dtype=np.float64, branch=None):
    """-> (T (n, 46) rig_lens_ref's terms, Bd (n, n_border(G)) the border terms in the header's order, s, seen).  Not seen: cost +infinity, everything else 0."""
    lenses = [lens] * len(R)
    T, s, seen = lr.terms(f, R, lenses, i, j, a, b, h, dtype, branch)
    G = len(free_list(free))
    Bd = np.zeros((len(s), n_border(G)), dtype)
    if G == 0:
        return T, Bd, s, seen
    f_, R_, a_, b_ = _cast(f, R, a, b, dtype)
    hd = dtype(h)
    m = np.sqrt(f_[i] * f_[j])
    p, ti, _ = lr._side(f_, R_, lenses, i, a_, m, dtype)
    q, tj, _ = lr._side(f_, R_, lenses, j, b_, m, dtype)
    E = columns(f, R, lens, free, i, j, a, b, dtype)
    with np.errstate(all="ignore"):
        u = [m * p[k] for k in range(3)]; v = [m * q[k] for k in range(3)]
        r = [m * (p[k] - q[k]) for k in range(3)]
        w = np.ones_like(m)
        if hd > 0:
            o = T[:, 45] > 0
            sd = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
            w[o] = hd / sd[o]
        ci = [0.5 * r[k] + ti[k] for k in range(3)]; cj = [0.5 * r[k] - tj[k] for k in range(3)]
        t = G
        for n in range(G):
            Bd[:, n] = w * fr._dot(E[n], r)
            for c in range(n, G):
                Bd[:, t] = w * fr._dot(E[n], E[c]); t += 1
            o = G + G * (G + 1) // 2 + 8 * n
            ue = fr._cross(u, E[n]); ve = fr._cross(v, E[n])
            for k in range(3):
                Bd[:, o + k] = w * ue[k]; Bd[:, o + 4 + k] = -(w * ve[k])
            Bd[:, o + 3] = w * fr._dot(ci, E[n]); Bd[:, o + 7] = w * fr._dot(cj, E[n])
    Bd[~seen] = 0.0
    return T, Bd, s, seen


def _sum_terms(T, Bd, i, j, n, G):
    """cost, H ((4n + G)^2), g (4n + G) of the terms, summed match by match in the given order"""
    c, H4, g4 = lr._sum_terms(T, i, j, n)
    d = 4 * n + G
    H = np.zeros((d, d), T.dtype); g = np.zeros(d, T.dtype)
    H[:4 * n, :4 * n] = H4; g[:4 * n] = g4
    tri = [(r, cc) for r in range(G) for cc in range(r, G)]
    for k in range(len(T)):
        for q in range(G):
            g[4 * n + q] += Bd[k, q]
        for t, (r, cc) in enumerate(tri):
            H[4 * n + r, 4 * n + cc] += Bd[k, G + t]
            if r != cc:
                H[4 * n + cc, 4 * n + r] += Bd[k, G + t]
        for q in range(G):
            o = G + len(tri) + 8 * q
            for e in range(8):
                row = 4 * i[k] + e if e < 4 else 4 * j[k] + e - 4
                H[row, 4 * n + q] += Bd[k, o + e]; H[4 * n + q, row] += Bd[k, o + e]
    return c, H, g


def accumulate(f, R, lens, free, matches, h=0.0, with_abs=False, dtype=np.float64):
    """cost, H, g with the coefficient rows last, over ALL matches in the given order; with_abs: also the sums of the terms' absolute values"""
    i, j, a, b = fr.unpack(matches)
    G = len(free_list(free))
    T, Bd, _, _ = terms(f, R, lens, free, i, j, a, b, h, dtype)
    res = list(_sum_terms(T, Bd, i, j, len(R), G))
    if with_abs:
        res += list(_sum_terms(np.abs(T), np.abs(Bd), i, j, len(R), G))
    res[0] = float(res[0]) if dtype is np.float64 else res[0]
    return tuple(res)


def term_deviation(f, R, lens, free, matches, h=0.0):
    """rig_lens_ref.term_deviation extended to the border entries: sum |T64 - Tlong| over the matches per entry of cost, H and g, in units of 2^-52 S -> the largest"""
    i, j, a, b = fr.unpack(matches)
    G = len(free_list(free))
    T64, B64, _, _ = terms(f, R, lens, free, i, j, a, b, h)
    TL, BL, _, _ = terms(f, R, lens, free, i, j, a, b, h, np.longdouble, branch=T64[:, 45] > 0)
    D = np.abs(T64.astype(np.longdouble) - TL).astype(np.float64); DB = np.abs(B64.astype(np.longdouble) - BL).astype(np.float64)
    n = len(R)
    dc, dH, dg = _sum_terms(D, DB, i, j, n, G)
    sc, sH, sg = _sum_terms(np.abs(T64), np.abs(B64), i, j, n, G)
    worst = 0.0
    for d, s in ((np.array([dc]), np.array([sc])), (dH, sH), (dg, sg)):
        nz = s > 0
        if nz.any():
            worst = max(worst, float(np.max(d[nz] / (2.0 ** -52 * s[nz]))))
    return worst


def all_seen(f, R, lens, matches):
    return lr.all_seen(f, R, [lens] * len(R), matches)


def selection(n, anchor, shared, G):
    """rig_focal_ref.selection with G coefficient columns after it"""
    P4 = fr.selection(n, anchor, shared)
    P = np.zeros((4 * n + G, P4.shape[1] + G))
    P[:4 * n, :P4.shape[1]] = P4
    for q in range(G):
        P[4 * n + q, P4.shape[1] + q] = 1.0
    return P


def apply_step(f, R, lens, free, full):
    """the cameras and the lens after the step `full` (4n + G): rig_focal_ref.apply_step, and k <- k + d on the free entries"""
    n = len(R)
    ft, Rt = fr.apply_step(f, R, full[:4 * n])
    k = k8(lens)
    for q, idx in enumerate(free_list(free)):
        k[idx] = k[idx] + float(full[4 * n + q])
    return ft, Rt, with_k(lens, k)


def propose(f, R, lens, free, matches, anchor, shared_focal, lam, huber_px=0.0):
    """one proposal at (f, R, lens) over ALL matches -> (ft, Rt, trial lens): what refine()'s first solve at this lambda gives, whatever the trial-lens rule says of it"""
    G = len(free_list(free))
    P = selection(len(R), anchor, shared_focal, G)
    _, H, g = accumulate(f, R, lens, free, matches, huber_px)
    Hr = P.T @ H @ P
    delta = np.linalg.solve(Hr + lam * np.diag(np.diag(Hr)), -(P.T @ g))
    return apply_step(f, R, lens, free, P @ delta)


def refine(f_in, R_in, lens_in, free, matches, anchor=0, shared_focal=False, huber_px=0.0, max_iters=50, step_tol=1e-10, min_pair_matches=4, trace=None):
    """rig_lens_ref.refine's loop with the coefficient columns: a solved step whose trial lens fails lens_ok is a failed solve (lambda * 10, one iteration, solve
    again) -> (f, R, lens, info dict; lens_rejections: the solves the trial-lens rule rejected); trace: a list that gets
    (iteration, accepted, max |step|, trial cost, lambda) of every evaluated trial"""
    import rig_ref as rr
    f = np.array(f_in, np.float64); R = np.array(R_in, np.float64); lens = lens_in
    n = len(R)
    G = len(free_list(free))
    i, j, _, _ = fr.unpack(matches)
    counts = {}
    for k in range(len(matches)):
        counts[(i[k], j[k])] = counts.get((i[k], j[k]), 0) + 1
    used = [m for k, m in enumerate(matches) if counts[(i[k], j[k])] >= min_pair_matches]
    if not all_seen(f, R, lens, used):
        raise ValueError("a pixel is not seen at the input cameras")
    P = selection(n, anchor, shared_focal, G)
    lam, iters, lens_rejections = 1e-3, 0, 0
    cost, H, g = accumulate(f, R, lens, free, used, huber_px)
    cost0 = cost

    def done(reason):
        ui, uj, ua, ub = fr.unpack(used)
        _, s, _ = lr.terms(f, R, [lens] * n, ui, uj, ua, ub, huber_px)
        return f, R, lens, dict(iterations=iters, stop_reason=reason, cost_initial=cost0, cost_final=cost, matches_used=len(used),
                                pairs_used=sum(1 for c in counts.values() if c >= min_pair_matches), pairs_ignored=sum(1 for c in counts.values() if c < min_pair_matches),
                                outliers=int((s > huber_px).sum()) if huber_px > 0 else 0, max_rotation_rad=max(rr.angle(R[v], R_in[v]) for v in range(n)),
                                max_focal_ratio=max(max(f[v] / f_in[v], f_in[v] / f[v]) for v in range(n)),
                                max_coeff_change=max(abs(k8(lens)[b] - k8(lens_in)[b]) for b in free_list(free)), lens_rejections=lens_rejections)

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
                ft, Rt, lt = apply_step(f, R, lens, free, P @ delta)
                ok = lens_ok(lt)
                lens_rejections += 0 if ok else 1
            if ok:
                break
            lam *= 10.0; iters += 1
            if lam > 1e12:
                return done(fr.STALLED)
            if iters >= max_iters:
                return done(fr.ITERATION_LIMIT)
        ct, Ht, gt = accumulate(ft, Rt, lt, free, used, huber_px)
        iters += 1
        if trace is not None:
            trace.append((iters, bool(ct <= cost), float(np.max(np.abs(delta))), float(ct), lam))
        if ct <= cost:
            f, R, lens, cost, H, g = ft, Rt, lt, ct, Ht, gt
            lam = max(lam / 10.0, 1e-12)
            if np.max(np.abs(delta)) < step_tol:
                return done(fr.CONVERGED)
        else:
            lam *= 10.0
            if lam > 1e12:
                return done(fr.STALLED)
        if iters >= max_iters:
            return done(fr.ITERATION_LIMIT)
