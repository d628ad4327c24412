"""Numpy restatement of the partial statistics of column shards (ms_gain_stats_partial), written from the statement in include/ms_stitch.h: the column
windows as ms_get_col_window cuts them, the raw cnt / S of the samples of one window, and their sum.  Imports tests/gain_ref.py for the per-view sampling."""
import numpy as np

import gain_ref as G


def col_windows(fw, S):
    """[(begin, end)] of the S column shards of an fw-column pano ROI: boundaries at floor(k * fw / S) rounded down to a multiple of 16, 0 and fw at the ends."""
    b = [0 if k <= 0 else (fw if k >= S else (k * fw // S) // 16 * 16) for k in range(S + 1)]
    return [(b[k], b[k + 1]) for k in range(S)]


def window_views(rois, T, window, active=None):
    """Bit mask of the active views whose ROI meets the window's columns: the views the partial statistic reads."""
    n = len(rois)
    active = (1 << n) - 1 if active is None else active
    x0, x1 = T[0] + window[0], T[0] + window[1]
    return sum(1 << v for v in range(n) if (active >> v) & 1 and rois[v][0] < x1 and rois[v][0] + rois[v][2] > x0)


def window_stats(rois, seen, q, T, stride, window, active=None):
    """Raw (cnt, S), n x n int64, over the samples (u, v) of the lattice of T with window[0] <= u - T.x < window[1]; no max(1, .) rule.
    rois / T = (x, y, w, h) in warper coordinates; seen[v], q[v] roi-sized (gain_ref.sample_view)."""
    n = len(rois)
    active = (1 << n) - 1 if active is None else active
    us, vs = np.arange(T[0], T[0] + T[2], stride), np.arange(T[1], T[1] + T[3], stride)
    us = us[(us - T[0] >= window[0]) & (us - T[0] < window[1])]
    cnt, S = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    see, val = [], []
    for v in range(n):
        x, y, w, h = rois[v]
        cx, cy = (us >= x) & (us < x + w), (vs >= y) & (vs < y + h)
        m = np.zeros((len(vs), len(us)), bool)
        qq = np.zeros((len(vs), len(us)), np.int64)
        if (active >> v) & 1 and cx.any() and cy.any():
            sub = np.ix_(vs[cy] - y, us[cx] - x)
            m[np.ix_(cy, cx)] = seen[v][sub]
            qq[np.ix_(cy, cx)] = q[v][sub]
        see.append(m); val.append(qq)
    for i in range(n):
        for j in range(i, n):
            both = see[i] & see[j]
            cnt[i, j] = cnt[j, i] = int(both.sum())
            S[i, j] = int(val[i][both].sum())
            S[j, i] = int(val[j][both].sum())
    return cnt, S


def finish(rois, cnt, S, active=None):
    """N, S as ms_gain_stats reports them, from summed raw partials: N = max(1, cnt) on the pairs of active views whose ROIs meet, everything else 0."""
    n = len(rois)
    active = (1 << n) - 1 if active is None else active
    N, So = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(n):
            if (active >> i) & (active >> j) & 1 and G.rects_meet(rois[i], rois[j]):
                N[i, j] = max(1, int(cnt[i, j]))
                So[i, j] = S[i, j]
    return N, So


def has_cross_pair(cnt):
    """The partition test's condition: some pair i != j of the partial has samples."""
    c = np.array(cnt, copy=True)
    np.fill_diagonal(c, 0)
    return bool(c.any())
