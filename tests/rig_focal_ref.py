"""numpy reference of the focal-and-rotation bundle adjustment and of the homography estimator (include/ms_stitch.h, "Self-calibrating rigs"), and the synthetic
rigs the tests share.

The per-match terms are the contract's formulas, one IEEE operation per product, sum, division and sqrt in the order the header writes them (numpy's elementwise
float64 ufuncs do not fuse).  Everything around them is built differently from the device code: one plain accumulation loop over the matches in the order they are
given (no pair grouping, no tree), a selection matrix P with H_solved = P^T H P for the held anchor and the shared focal, numpy.linalg.solve for the step, the textbook
Rodrigues formula of tests/rig_ref.py, numpy.linalg.svd and numpy.linalg.inv in the estimator.  A match is (view_a, view_b, a, b) with a, b centred pixels."""
import math

import numpy as np

import rig_ref as rr

CONVERGED, STALLED, ITERATION_LIMIT = rr.CONVERGED, rr.STALLED, rr.ITERATION_LIMIT
N_TERMS = 46
_SYM4 = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]


def unpack(matches):
    """-> i, j (canonical i < j), a, b (n, 2) arrays"""
    va = np.array([m[0] for m in matches]); vb = np.array([m[1] for m in matches])
    a = np.array([m[2] for m in matches], np.float64).reshape(-1, 2); b = np.array([m[3] for m in matches], np.float64).reshape(-1, 2)
    sw = va > vb
    return np.where(sw, vb, va), np.where(sw, va, vb), np.where(sw[:, None], b, a), np.where(sw[:, None], a, b)


def _cross(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def _dot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def terms(f, R, i, j, a, b, h):
    """the 46 terms of every match (n, 46) in the header's layout, and s (n,)"""
    f = np.asarray(f, np.float64); R = np.asarray(R, np.float64)
    fi, fj, Ri, Rj = f[i], f[j], R[i], R[j]
    na = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + fi * fi); nb = np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + fj * fj)
    ra = [a[:, 0] / na, a[:, 1] / na, fi / na]; rb = [b[:, 0] / nb, b[:, 1] / nb, fj / nb]
    p = [Ri[:, r, 0] * ra[0] + Ri[:, r, 1] * ra[1] + Ri[:, r, 2] * ra[2] for r in range(3)]
    q = [Rj[:, r, 0] * rb[0] + Rj[:, r, 1] * rb[1] + Rj[:, r, 2] * rb[2] for r in range(3)]
    m = np.sqrt(fi * fj)
    u = [m * p[k] for k in range(3)]; v = [m * q[k] for k in range(3)]
    r = [m * (p[k] - q[k]) for k in range(3)]
    s2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    s = np.sqrt(s2)
    w = np.ones_like(s2); rho = s2.copy(); out = np.zeros_like(s2)
    if h > 0:
        o = s > h
        w[o] = h / s[o]
        rho[o] = (2.0 * h) * s[o] - h * h
        out[o] = 1.0
    ma = m * ra[2]; mb = m * rb[2]
    ci = [0.5 * r[k] + ma * (Ri[:, k, 2] - ra[2] * p[k]) for k in range(3)]
    cj = [0.5 * r[k] - mb * (Rj[:, k, 2] - rb[2] * q[k]) for k in range(3)]
    T = np.empty((len(s2), N_TERMS))
    T[:, 0] = rho
    ur = _cross(u, r); vr = _cross(v, r)
    for k in range(3):
        T[:, 1 + k] = w * ur[k]; T[:, 5 + k] = -(w * vr[k])
    T[:, 4] = w * _dot(ci, r); T[:, 8] = w * _dot(cj, r)
    for o, x, c, sign in ((9, u, ci, 1), (19, v, cj, -1)):
        xc = _cross(x, c)
        T[:, o] = w * (x[1] * x[1] + x[2] * x[2]); T[:, o + 1] = -(w * (x[0] * x[1])); T[:, o + 2] = -(w * (x[0] * x[2]))
        T[:, o + 4] = w * (x[0] * x[0] + x[2] * x[2]); T[:, o + 5] = -(w * (x[1] * x[2])); T[:, o + 7] = w * (x[0] * x[0] + x[1] * x[1])
        for k, e in enumerate((3, 6, 8)):
            T[:, o + e] = w * xc[k] if sign > 0 else -(w * xc[k])
        T[:, o + 9] = w * _dot(c, c)
    ucj = _cross(u, cj); vci = _cross(v, ci)
    diag = [u[1] * v[1] + u[2] * v[2], u[0] * v[0] + u[2] * v[2], u[0] * v[0] + u[1] * v[1]]
    for rr_ in range(3):
        for c in range(3):
            T[:, 29 + 4 * rr_ + c] = -(w * diag[rr_]) if rr_ == c else w * (v[rr_] * u[c])
        T[:, 29 + 4 * rr_ + 3] = w * ucj[rr_]
        T[:, 41 + rr_] = -(w * vci[rr_])
    T[:, 44] = w * _dot(ci, cj)
    T[:, 45] = out
    return T, s


def _blocks(T):
    """(n, 46) terms -> g_i (n, 4), g_j, H_ii (n, 4, 4), H_jj, H_ij"""
    def sym(o):
        B = np.empty((len(T), 4, 4))
        for k, (r, c) in enumerate(_SYM4):
            B[:, r, c] = T[:, o + k]; B[:, c, r] = T[:, o + k]
        return B
    return T[:, 1:5], T[:, 5:9], sym(9), sym(19), T[:, 29:45].reshape(-1, 4, 4)


def accumulate(f, R, matches, h=0.0, with_abs=False):
    """cost, H (4n x 4n), g (4n) at the cameras over ALL matches, summed match by match in the given order; with_abs: also the sums of the terms' absolute values"""
    n = len(R)
    i, j, a, b = unpack(matches)
    T, _ = terms(f, R, i, j, a, b, h)
    res = []
    for X in ((T, np.abs(T)) if with_abs else (T,)):
        gi, gj, Hii, Hjj, Hij = _blocks(X)
        cost = 0.0; H = np.zeros((4 * n, 4 * n)); g = np.zeros(4 * n)
        for k in range(len(X)):
            I = slice(4 * i[k], 4 * i[k] + 4); J = slice(4 * j[k], 4 * j[k] + 4)
            cost += X[k, 0]
            g[I] += gi[k]; g[J] += gj[k]
            H[I, I] += Hii[k]; H[J, J] += Hjj[k]; H[I, J] += Hij[k]; H[J, I] += Hij[k].T
        res += [cost, H, g]
    return tuple(res)


def cost_only(f, R, matches, h=0.0):
    i, j, a, b = unpack(matches)
    return float(terms(f, R, i, j, a, b, h)[0][:, 0].sum())


def selection(n, anchor, shared):
    """P (4n x m): the solved unknowns as combinations of the full ones -- the anchor's rotation left out; one focal column of ones where the focal is shared"""
    cols = []
    for v in range(n):
        for k in range(3):
            if v != anchor:
                e = np.zeros(4 * n); e[4 * v + k] = 1.0; cols.append(e)
        if not shared:
            e = np.zeros(4 * n); e[4 * v + 3] = 1.0; cols.append(e)
    if shared:
        e = np.zeros(4 * n); e[3::4] = 1.0; cols.append(e)
    return np.array(cols).T


def apply_step(f, R, full):
    """the cameras after the step `full` (4n): R_v <- Exp(delta_v) R_v, f_v <- f_v exp(d_v)"""
    n = len(R)
    Rn = np.array([R[v] if not full[4 * v:4 * v + 3].any() else rr.exp_so3(full[4 * v:4 * v + 3]) @ R[v] for v in range(n)])
    return np.array([f[v] * math.exp(full[4 * v + 3]) for v in range(n)]), Rn


def step(f, R, matches, anchor, shared_focal, lam, huber_px=0.0):
    """one proposal of refine() at the cameras (f, R) over ALL matches -> (A, delta): the solved matrix P^T H P + lam diag of it, and the step numpy.linalg.solve
    returns for it (the columns of selection()); the same operations as refine()'s, so the same bits"""
    P = selection(len(R), anchor, shared_focal)
    _, H, g = accumulate(f, R, matches, huber_px)
    Hr = P.T @ H @ P
    A = Hr + lam * np.diag(np.diag(Hr))
    return A, np.linalg.solve(A, -(P.T @ g))


def refine(f_in, R_in, matches, anchor=0, shared_focal=False, huber_px=0.0, max_iters=50, step_tol=1e-10, min_pair_matches=4):
    """the Levenberg-Marquardt loop of the contract -> (f, R, info dict)"""
    f = np.array(f_in, np.float64); R = np.array(R_in, np.float64)
    n = len(R)
    i, j, _, _ = unpack(matches)
    counts = {}
    for k in range(len(matches)):
        counts[(i[k], j[k])] = counts.get((i[k], j[k]), 0) + 1
    used = [m for k, m in enumerate(matches) if counts[(i[k], j[k])] >= min_pair_matches]
    P = selection(n, anchor, shared_focal)
    lam, iters = 1e-3, 0
    cost, H, g = accumulate(f, R, used, huber_px)
    cost0 = cost

    def done(reason):
        ui, uj, ua, ub = unpack(used)
        _, s = terms(f, R, ui, uj, ua, ub, huber_px)
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
                return done(STALLED)
            if iters >= max_iters:
                return done(ITERATION_LIMIT)
        ft, Rt = apply_step(f, R, P @ delta)
        ct, Ht, gt = accumulate(ft, Rt, used, huber_px)
        iters += 1
        if ct <= cost:
            f, R, cost, H, g = ft, Rt, ct, Ht, gt
            lam = max(lam / 10.0, 1e-12)
            if np.max(np.abs(delta)) < step_tol:
                return done(CONVERGED)
        else:
            lam *= 10.0
            if lam > 1e12:
                return done(STALLED)
        if iters >= max_iters:
            return done(ITERATION_LIMIT)


# ---- the homography estimator ---------------------------------------------------------------------------------------------------------------------
def focals_from_homography(H):
    """-> (f0 or None, f1 or None): the focal of the source and of the destination view of a homography between centred pixels"""
    h = np.asarray(H, np.float64).reshape(9)
    with np.errstate(divide="ignore", invalid="ignore"):
        d1 = h[6] * h[7]; d2 = (h[7] - h[6]) * (h[7] + h[6])
        f1 = _pick_cv(float(-(h[0] * h[1] + h[3] * h[4]) / d1), float(d1), float((h[0] * h[0] + h[3] * h[3] - h[1] * h[1] - h[4] * h[4]) / d2), float(d2))
        d1 = h[0] * h[3] + h[1] * h[4]; d2 = h[0] * h[0] + h[1] * h[1] - h[3] * h[3] - h[4] * h[4]
        f0 = _pick_cv(float(-h[2] * h[5] / d1), float(d1), float((h[5] * h[5] - h[2] * h[2]) / d2), float(d2))
    return f0, f1


def _pick_cv(v1, d1, v2, d2):
    """the two candidate squares: the larger first (only the values are swapped, as the reference does); both positive: the first if |d1| > |d2|, else the second"""
    if v1 < v2:
        v1, v2 = v2, v1
    if v1 > 0 and v2 > 0:
        return math.sqrt(v1 if abs(d1) > abs(d2) else v2)
    return math.sqrt(v1) if v1 > 0 else None


def estimate_rig(n, pairs, size, anchor=0):
    """pairs: [(view_a, view_b, H, weight)] -> (focals (n,), R (n, 3, 3), status); raises ValueError naming a view the pairs do not connect to the anchor"""
    est = []
    for _, _, H, _ in pairs:
        f0, f1 = focals_from_homography(H)
        if f0 is not None and f1 is not None:
            est.append(math.sqrt(f0 * f1))
    focal = float(np.median(est)) if est else float(size[0] + size[1])
    # maximum spanning tree: take the heaviest (earliest among equals) pair that joins two components, until none does
    comp = list(range(n)); tree = []
    for k in sorted(range(len(pairs)), key=lambda k: (-pairs[k][3], k)):
        a, b = pairs[k][0], pairs[k][1]
        if comp[a] != comp[b]:
            old = comp[b]
            comp = [comp[a] if c == old else c for c in comp]
            tree.append(k)
    K = np.diag([focal, focal, 1.0])
    R = [None] * n
    R[anchor] = np.eye(3)
    queue = [anchor]
    while queue:
        v = queue.pop(0)
        for k in tree:
            a, b, H, _ = pairs[k]
            H = np.asarray(H, np.float64).reshape(3, 3)
            if a == v and R[b] is None:
                M = R[a] @ np.linalg.inv(K) @ np.linalg.inv(H) @ K; o = b
            elif b == v and R[a] is None:
                M = R[b] @ np.linalg.inv(K) @ H @ K; o = a
            else:
                continue
            U, _, Vt = np.linalg.svd(M)
            if np.linalg.det(U @ Vt) < 0:
                U[:, 2] = -U[:, 2]
            R[o] = U @ Vt
            queue.append(o)
    for v in range(n):
        if R[v] is None:
            raise ValueError("view %d is not connected" % v)
    return np.full(n, focal), np.array(R), 0 if est else 1


def homography(fa, Ra, fb, Rb):
    """the exact homography from centred pixels of camera a to those of camera b (rotations camera to rig): K_b R_b^T R_a K_a^-1"""
    return np.diag([fb, fb, 1.0]) @ Rb.T @ Ra @ np.diag([1.0 / fa, 1.0 / fa, 1.0])


# ---- synthetic rigs -----------------------------------------------------------------------------------------------------------------------------
def make_px_matches(ft, Rt, pairs, per_pair, rng, noise_px=0.0, outlier_frac=0.0, spread_deg=20.0, outlier_px=None):
    """per_pair matches (a number, or one per pair) of every pair: world rays around the bisector of the two optical axes, seen through the TRUE cameras (ft, Rt) as
    centred pixels; Gaussian pixel noise; an outlier's second pixel is moved by a distance drawn from outlier_px = (lo, hi) in a random direction (a match to the
    feature next door), or, with outlier_px None, replaced by a random pixel within 0.8 f of the principal point"""
    out = []
    for k, (i, j) in enumerate(pairs):
        m = per_pair[k] if isinstance(per_pair, (list, tuple)) else per_pair
        mid = Rt[i][:, 2] + Rt[j][:, 2]
        mid /= np.linalg.norm(mid)
        for _ in range(m):
            d = rr.exp_so3(np.radians(rng.uniform(-spread_deg, spread_deg, 3))) @ mid
            ca = Rt[i].T @ d; cb = Rt[j].T @ d
            a = ft[i] * ca[:2] / ca[2]; b = ft[j] * cb[:2] / cb[2]
            if noise_px > 0:
                a = a + rng.normal(0, noise_px, 2); b = b + rng.normal(0, noise_px, 2)
            if outlier_frac > 0 and rng.uniform() < outlier_frac:
                if outlier_px is None:
                    b = rng.uniform(-0.8, 0.8, 2) * ft[j]
                else:
                    t = rng.uniform(0.0, 2.0 * math.pi)
                    b = b + rng.uniform(*outlier_px) * np.array([math.cos(t), math.sin(t)])
            out.append((i, j, a, b))
    return out
