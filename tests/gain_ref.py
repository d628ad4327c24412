"""Numpy restatement of the exposure tracker (ms_gain_stats / ms_track_gains), written from the statement in include/ms_stitch.h and from
GainCompensator::feed (stitching/src/exposure_compensate.cpp:71-145), independent of the device code: integer overlap statistics on the sample lattice
of the pano ROI, the normal equations, their solution (LAPACK), the energy they minimise, and the smoothing step."""
import numpy as np

ALPHA, BETA = 0.01, 100.0          # exposure_compensate.cpp:123-124
QBITS = 20                         # q = llrint(sqrt(b^2 + g^2 + r^2) * 2^20)


def q_of(px):
    """uint8 (..., 3) -> int64 fixed-point norm of each pixel (round half to even, like llrint in the default rounding mode)."""
    p = px.astype(np.int64)
    s = p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1] + p[..., 2] * p[..., 2]
    return np.rint(np.sqrt(s.astype(np.float64)) * float(1 << QBITS)).astype(np.int64)


def sample_view(xm, ym, frame):
    """The warp mask before seam cutting and the nearest-sampled q of one view over its whole warped ROI: (seen bool, q int64), both roi-sized.
    A pixel is seen iff the map coordinate truncated toward zero hits the source (k_valid_mask's rule)."""
    h, w = frame.shape[:2]
    tx, ty = np.trunc(np.nan_to_num(xm.astype(np.float64))), np.trunc(np.nan_to_num(ym.astype(np.float64)))
    seen = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    ix, iy = np.where(seen, tx, 0).astype(np.int64), np.where(seen, ty, 0).astype(np.int64)
    return seen, np.where(seen, q_of(frame[iy, ix]), 0)


def rects_meet(a, b):
    return max(a[0], b[0]) < min(a[0] + a[2], b[0] + b[2]) and max(a[1], b[1]) < min(a[1] + a[3], b[1] + b[3])


def stats(rois, seen, q, T, stride, active=None):
    """N, S (n x n int64) and the raw counts.  rois / T = (x, y, w, h) in warper coordinates; seen[v], q[v] roi-sized; active = bit mask (None: all)."""
    n = len(rois)
    active = (1 << n) - 1 if active is None else active
    us, vs = np.arange(T[0], T[0] + T[2], stride), np.arange(T[1], T[1] + T[3], stride)
    see, val = [], []
    for v in range(n):                                   # each view on the lattice
        x, y, w, h = rois[v]
        cx, cy = (us >= x) & (us < x + w), (vs >= y) & (vs < y + h)
        m = np.zeros((len(vs), len(us)), bool)
        qq = np.zeros((len(vs), len(us)), np.int64)
        if cx.any() and cy.any():
            sub = np.ix_(vs[cy] - y, us[cx] - x)
            m[np.ix_(cy, cx)] = seen[v][sub]
            qq[np.ix_(cy, cx)] = q[v][sub]
        see.append(m); val.append(qq)
    N, S, cnt = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i, n):
            if not ((active >> i) & (active >> j) & 1) or not rects_meet(rois[i], rois[j]):
                continue
            both = see[i] & see[j]
            cnt[i, j] = cnt[j, i] = int(both.sum())
            N[i, j] = N[j, i] = max(1, cnt[i, j])
            S[i, j] = int(val[i][both].sum())
            S[j, i] = int(val[j][both].sum())
    return N, S, cnt


def intensities(N, S):
    I = np.zeros(N.shape, np.float64)
    nz = N > 0
    I[nz] = S[nz].astype(np.float64) / float(1 << QBITS) / N[nz].astype(np.float64)
    return I


def normal_equations(N, I):
    """exposure_compensate.cpp:123-139."""
    n = N.shape[0]
    A, b = np.zeros((n, n)), np.zeros(n)
    for i in range(n):
        for j in range(n):
            b[i] += BETA * N[i, j]
            A[i, i] += BETA * N[i, j]
            if j == i:
                continue
            A[i, i] += 2 * ALPHA * I[i, j] * I[i, j] * N[i, j]
            A[i, j] -= 2 * ALPHA * I[i, j] * I[j, i] * N[i, j]
    return A, b


def solve(N, S, active=None):
    """Gains of the active views (in view order) from the integer statistics; returns (indices, gains)."""
    n = N.shape[0]
    idx = [v for v in range(n) if active is None or (active >> v) & 1]
    Na, Ia = N[np.ix_(idx, idx)], intensities(N, S)[np.ix_(idx, idx)]
    A, b = normal_equations(Na, Ia)
    return idx, np.linalg.solve(A, b)


def energy(N, I, g):
    """E(g) = sum_ij N_ij (alpha (g_i I_ij - g_j I_ji)^2 + beta (1 - g_i)^2): what GainCompensator minimises (Brown & Lowe 2007, eq. 29 with sigma folded in)."""
    g = np.asarray(g, np.float64)
    d = g[:, None] * I - g[None, :] * I.T
    return float((N * (ALPHA * d * d + BETA * (1.0 - g[:, None]) ** 2)).sum())


def smooth(g, g_est, lam):
    """The tracker's update, as the kernel writes it (no contraction: the library is built with -ffp-contract=off)."""
    return g + lam * (g_est - g)
