"""numpy restatement of ms_match_lists' device-stage contract (include/ms_stitch.h), on top of pair_match_ref's hamming / knn2: per directed problem the rows
(query, nearest train row, distance) that pass the double ratio rule, in ascending query order."""
import numpy as np

import pair_match_ref as PR


def ratio_pass(d0, d1, ratio=0.7):
    """(double)d0 < ratio * (double)d1: one float64 multiply, one compare"""
    return np.asarray(d0).astype(np.float64) < np.float64(ratio) * np.asarray(d1).astype(np.float64)


def problem_list(Q, T, ratio=0.7):
    """The list of the directed problem (Q against T): (count, 3) int32 rows of (query, train, distance); empty with no query row or fewer than two train rows"""
    if len(Q) < 1 or len(T) < 2:
        return np.zeros((0, 3), np.int32)
    idx, dist = PR.knn2(Q, T)
    keep = dist[:, 0].astype(np.float64) < np.float64(ratio) * dist[:, 1].astype(np.float64)
    q = np.nonzero(keep)[0]
    return np.stack([q, idx[q, 0], dist[q, 0]], axis=1).astype(np.int32).reshape(-1, 3)


def match_lists(descs, problems, ratio=0.7):
    """Every problem's record (query_set, train_set, first, count) and its rows, as ms_match_lists lists them"""
    recs, rows, first = [], [], 0
    for q, t in problems:
        r = problem_list(descs[q], descs[t], ratio)
        recs.append((q, t, first, len(r))); rows.append(r)
        first += len(r)
    return recs, rows
