"""numpy reference of the rig rotation refinement contract (include/ms_stitch.h, "Rig rotation refinement"), and the synthetic rigs the tests share.

The per-match terms are the contract's formulas, one IEEE operation per product and sum in the order the header writes them (numpy's elementwise float64
ufuncs do not fuse).  Everything around them is built differently from the device code: one plain accumulation loop over the matches in the order they are
given (no pair grouping, no tree), numpy.linalg.solve for the step, the textbook Rodrigues formula.  A match is (view_a, view_b, a, b)."""
import math

import numpy as np

CONVERGED, STALLED, ITERATION_LIMIT = 0, 1, 2
_SYM = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def unpack(matches):
    """-> i, j (canonical i < j), a, b arrays"""
    va = np.array([m[0] for m in matches]); vb = np.array([m[1] for m in matches])
    a = np.array([m[2] for m in matches], np.float64).reshape(-1, 3); b = np.array([m[3] for m in matches], np.float64).reshape(-1, 3)
    sw = va > vb
    return np.where(sw, vb, va), np.where(sw, va, vb), np.where(sw[:, None], b, a), np.where(sw[:, None], a, b)


def terms(R, i, j, a, b, h):
    """the 28 terms of every match (n, 28): cost | g_i | g_j | H_ii (xx xy xz yy yz zz) | H_jj | H_ij row-major; and s (n,)"""
    Ri, Rj = R[i], R[j]
    p = [Ri[:, r, 0] * a[:, 0] + Ri[:, r, 1] * a[:, 1] + Ri[:, r, 2] * a[:, 2] for r in range(3)]
    q = [Rj[:, r, 0] * b[:, 0] + Rj[:, r, 1] * b[:, 1] + Rj[:, r, 2] * b[:, 2] for r in range(3)]
    r = [p[k] - q[k] for k in range(3)]
    s2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    s = np.sqrt(s2)
    w = np.ones_like(s2); rho = s2.copy()
    if h > 0:
        out = s > h
        w[out] = h / s[out]
        rho[out] = (2.0 * h) * s[out] - h * h
    T = np.empty((len(s2), 28))
    T[:, 0] = rho
    T[:, 1] = w * (p[1] * r[2] - p[2] * r[1]); T[:, 2] = w * (p[2] * r[0] - p[0] * r[2]); T[:, 3] = w * (p[0] * r[1] - p[1] * r[0])
    T[:, 4] = -(w * (q[1] * r[2] - q[2] * r[1])); T[:, 5] = -(w * (q[2] * r[0] - q[0] * r[2])); T[:, 6] = -(w * (q[0] * r[1] - q[1] * r[0]))
    for o, x in ((7, p), (13, q)):
        T[:, o] = w * (x[1] * x[1] + x[2] * x[2]); T[:, o + 1] = -(w * (x[0] * x[1])); T[:, o + 2] = -(w * (x[0] * x[2]))
        T[:, o + 3] = w * (x[0] * x[0] + x[2] * x[2]); T[:, o + 4] = -(w * (x[1] * x[2])); T[:, o + 5] = w * (x[0] * x[0] + x[1] * x[1])
    T[:, 19] = -(w * (p[1] * q[1] + p[2] * q[2])); T[:, 20] = w * (q[0] * p[1]); T[:, 21] = w * (q[0] * p[2])
    T[:, 22] = w * (q[1] * p[0]); T[:, 23] = -(w * (p[0] * q[0] + p[2] * q[2])); T[:, 24] = w * (q[1] * p[2])
    T[:, 25] = w * (q[2] * p[0]); T[:, 26] = w * (q[2] * p[1]); T[:, 27] = -(w * (p[0] * q[0] + p[1] * q[1]))
    return T, s


def _blocks(T):
    """(n, 28) terms -> g_i (n, 3), g_j, H_ii (n, 3, 3), H_jj, H_ij"""
    def sym(o):
        B = np.empty((len(T), 3, 3))
        for k, (r, c) in enumerate(_SYM):
            B[:, r, c] = T[:, o + k]; B[:, c, r] = T[:, o + k]
        return B
    return T[:, 1:4], T[:, 4:7], sym(7), sym(13), T[:, 19:28].reshape(-1, 3, 3)


def accumulate(R, matches, h=0.0, with_abs=False):
    """cost, H (3n x 3n), g (3n) at R over ALL matches, summed match by match in the given order; with_abs: also the sums of the terms' absolute values"""
    R = np.asarray(R, np.float64)
    n = len(R)
    i, j, a, b = unpack(matches)
    T, _ = terms(R, i, j, a, b, h)
    res = []
    for X in ((T, np.abs(T)) if with_abs else (T,)):
        gi, gj, Hii, Hjj, Hij = _blocks(X)
        cost = 0.0; H = np.zeros((3 * n, 3 * n)); g = np.zeros(3 * n)
        for k in range(len(X)):
            I = slice(3 * i[k], 3 * i[k] + 3); J = slice(3 * j[k], 3 * j[k] + 3)
            cost += X[k, 0]
            g[I] += gi[k]; g[J] += gj[k]
            H[I, I] += Hii[k]; H[J, J] += Hjj[k]; H[I, J] += Hij[k]; H[J, I] += Hij[k].T
        res += [cost, H, g]
    return tuple(res)


def exp_so3(d):
    t = math.sqrt(float(d @ d))
    if t == 0.0:
        return np.eye(3)
    k = d / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def angle(A, B):
    """the angle of A B^T, accurate near 0"""
    M = np.asarray(A, np.float64) @ np.asarray(B, np.float64).T
    v = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return math.atan2(0.5 * math.sqrt(float(v @ v)), 0.5 * (np.trace(M) - 1.0))


def step(R, matches, anchor, lam, huber_rad=0.0):
    """one proposal of refine() at the cameras R over ALL matches -> (A, delta): the solved matrix H + lam diag H without the anchor's rows, and the step
    numpy.linalg.solve returns for it (view after view, the anchor left out); the same operations as refine()'s, so the same bits"""
    R = np.asarray(R, np.float64)
    keep = np.array([v for v in range(3 * len(R)) if v // 3 != anchor])
    _, H, g = accumulate(R, matches, huber_rad)
    Hr = H[np.ix_(keep, keep)]
    A = Hr + lam * np.diag(np.diag(Hr))
    return A, np.linalg.solve(A, -g[keep])


def refine(R_in, matches, anchor=0, huber_rad=0.0, max_iters=50, step_tol=1e-10, min_pair_matches=4):
    """the Levenberg-Marquardt loop of the contract -> (R, info dict)"""
    R = np.array(R_in, np.float64)
    n = len(R)
    i, j, _, _ = unpack(matches)
    counts = {}
    for k in range(len(matches)):
        counts[(i[k], j[k])] = counts.get((i[k], j[k]), 0) + 1
    used = [m for k, m in enumerate(matches) if counts[(i[k], j[k])] >= min_pair_matches]
    keep = np.array([v for v in range(3 * n) if v // 3 != anchor])
    lam, iters = 1e-3, 0
    cost, H, g = accumulate(R, used, huber_rad)
    cost0 = cost

    def done(reason):
        ui, uj, ua, ub = unpack(used)
        _, s = terms(R, ui, uj, ua, ub, huber_rad)
        return R, dict(iterations=iters, stop_reason=reason, cost_initial=cost0, cost_final=cost, matches_used=len(used),
                       pairs_used=sum(1 for c in counts.values() if c >= min_pair_matches), pairs_ignored=sum(1 for c in counts.values() if c < min_pair_matches),
                       outliers=int((s > huber_rad).sum()) if huber_rad > 0 else 0, max_rotation_rad=max(angle(R[v], R_in[v]) for v in range(n)))

    while True:
        while True:
            Hr = H[np.ix_(keep, keep)]
            A = Hr + lam * np.diag(np.diag(Hr))
            try:
                np.linalg.cholesky(A)
                delta = np.linalg.solve(A, -g[keep])
                ok = bool(np.all(np.isfinite(delta)))
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                break
            lam *= 10.0; iters += 1
            if lam > 1e12:
                return done(STALLED)
            if iters >= max_iters:
                return done(ITERATION_LIMIT)
        full = np.zeros(3 * n); full[keep] = delta
        Rt = np.array([R[v] if v == anchor else exp_so3(full[3 * v:3 * v + 3]) @ R[v] for v in range(n)])
        ct, Ht, gt = accumulate(Rt, used, huber_rad)
        iters += 1
        if ct <= cost:
            R, cost, H, g = Rt, ct, Ht, gt
            lam = max(lam / 10.0, 1e-12)
            if np.max(np.abs(delta)) < step_tol:
                return done(CONVERGED)
        else:
            lam *= 10.0
            if lam > 1e12:
                return done(STALLED)
        if iters >= max_iters:
            return done(ITERATION_LIMIT)


# ---- warper directions in float64 (warpers_inl.hpp mapBackward / mapForward), for the tests ---------------------------------------------------------
PLANE, CYLINDRICAL, SPHERICAL = 0, 1, 2


def warper_dir(proj, scale, u, v, t=(0.0, 0.0, 0.0)):
    up = float(u) / float(scale); vp = float(v) / float(scale)
    if proj == SPHERICAL:
        sv = math.sin(math.pi - vp)
        return np.array([sv * math.sin(up), math.cos(math.pi - vp), sv * math.cos(up)])
    if proj == CYLINDRICAL:
        return np.array([math.sin(up), vp, math.cos(up)])
    return np.array([up - float(t[0]), vp - float(t[1]), 1.0 - float(t[2])])


def warper_ray(proj, scale, R, u, v, t=(0.0, 0.0, 0.0)):
    """the unit camera ray R^T d / |R^T d|, in the operation order of the header"""
    d = warper_dir(proj, scale, u, v, t)
    R = np.asarray(R, np.float64)
    X = [float(R[0, c]) * d[0] + float(R[1, c]) * d[1] + float(R[2, c]) * d[2] for c in range(3)]
    n = math.sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2])
    return np.array([X[0] / n, X[1] / n, X[2] / n])


def warper_forward(proj, scale, d):
    """warper coordinates (u, v) of the direction d (spherical / cylindrical)"""
    x, y, z = d
    u = scale * math.atan2(x, z)
    if proj == SPHERICAL:
        return u, scale * (math.pi - math.acos(y / math.sqrt(x * x + y * y + z * z)))
    return u, scale * y / math.sqrt(x * x + z * z)


# ---- synthetic rigs -----------------------------------------------------------------------------------------------------------------------------
def rot_y(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def ring(n):
    """the ideal ring of ms_calibrate_cameras in float64"""
    return np.array([rot_y(2.0 * math.pi * v / n) for v in range(n)])


def perturbed(R, rng, max_deg):
    """every rotation turned by up to max_deg about each axis"""
    return np.array([exp_so3(np.radians(rng.uniform(-max_deg, max_deg, 3))) @ Rv for Rv in R])


def ring_pairs(n):
    return [(0, 1)] if n == 2 else [(v, (v + 1) % n) for v in range(n)]


def make_matches(Rt, pairs, per_pair, rng, noise=0.0, outlier_frac=0.0, spread_deg=20.0):
    """per_pair matches (a number, or one per pair) of every pair: world rays around the bisector of the two optical axes, seen through the TRUE rotations Rt;
    Gaussian noise on the rays (renormalised); outliers are replaced by random directions"""
    out = []
    for k, (i, j) in enumerate(pairs):
        m = per_pair[k] if isinstance(per_pair, (list, tuple)) else per_pair
        mid = Rt[i][:, 2] + Rt[j][:, 2]
        mid /= np.linalg.norm(mid)
        for _ in range(m):
            d = exp_so3(np.radians(rng.uniform(-spread_deg, spread_deg, 3))) @ mid
            a = Rt[i].T @ d; b = Rt[j].T @ d
            if noise > 0:
                a = a + rng.normal(0, noise, 3); b = b + rng.normal(0, noise, 3)
            if outlier_frac > 0 and rng.uniform() < outlier_frac:
                b = rng.normal(0, 1, 3)
            out.append((i, j, a / np.linalg.norm(a), b / np.linalg.norm(b)))
    return out


def expected(R_in, Rt, anchor):
    """the truth in the gauge of the held anchor: R_in[anchor] Rt[anchor]^T Rt[v]"""
    G = R_in[anchor] @ Rt[anchor].T
    return np.array([G @ Rv for Rv in Rt])
