"""numpy restatement of the pairwise-matching contract of include/ms_stitch.h (ms_match_pairs, ms_biggest_component, ms_wave_correct), written from the contract:
brute-force Hamming 2-NN in (distance, index) order, the float32 ratio rule, list order and cross-check; the confidence formula; the biggest component; wave
correction through numpy.linalg.eigh."""
import numpy as np

_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


def hamming(A, B):
    """(na, nb) int32 Hamming distances between the uint8 rows of A and B"""
    A = np.asarray(A, np.uint8); B = np.asarray(B, np.uint8)
    return _POP[A[:, None, :] ^ B[None, :, :]].sum(axis=2, dtype=np.int32)


def knn2(Q, T):
    """For every row of Q the two nearest rows of T in (distance, index) order -> (idx (nq, 2), dist (nq, 2)) int32; T needs two rows or more.
    The order is one integer key, distance * nt + index: the two smallest keys of a row are its two nearest rows."""
    D = hamming(Q, T)
    nq, nt = D.shape
    assert nt >= 2
    key = D.astype(np.int64) * nt + np.arange(nt, dtype=np.int64)[None, :]
    two = np.sort(key, axis=1)[:, :2]
    return (two % nt).astype(np.int32), (two // nt).astype(np.int32)


def ratio_pass(d0, d1, match_conf):
    """(float)d0 < t * (float)d1 with t = 1.f - match_conf: one float32 subtraction, one float32 multiply"""
    t = np.float32(1.0) - np.float32(match_conf)
    return np.float32(d0) < np.float32(t * np.float32(d1))


def pair_list_from_knn(idx_ab, dist_ab, idx_ba, dist_ba, match_conf):
    """The pair's match list from the two 2-NN tables (None where that direction's train side has fewer than two rows): (rows (count, 3) int32 of
    (query in a, train in b, distance), n_forward)"""
    out = []
    fwd = set()
    if idx_ab is not None:
        for q in range(len(idx_ab)):
            if ratio_pass(dist_ab[q, 0], dist_ab[q, 1], match_conf):
                out.append((q, int(idx_ab[q, 0]), int(dist_ab[q, 0])))
                fwd.add((q, int(idx_ab[q, 0])))
    n_forward = len(out)
    if idx_ba is not None:
        for q in range(len(idx_ba)):
            if ratio_pass(dist_ba[q, 0], dist_ba[q, 1], match_conf) and (int(idx_ba[q, 0]), q) not in fwd:
                out.append((int(idx_ba[q, 0]), q, int(dist_ba[q, 0])))
    return np.array(out, np.int32).reshape(-1, 3), n_forward


def pair_list(A, B, match_conf):
    """The match list of the pair (a, b) from the descriptor rows A of a and B of b"""
    ab = knn2(A, B) if len(A) and len(B) >= 2 else (None, None)
    ba = knn2(B, A) if len(B) and len(A) >= 2 else (None, None)
    return pair_list_from_knn(ab[0], ab[1], ba[0], ba[1], match_conf)


def candidate_pairs(n, range_width=0, pair_mask=None):
    return [(i, j) for i in range(n - 1) for j in range(i + 1, n)
            if (range_width == 0 or j < i + range_width) and (pair_mask is None or pair_mask[i][j])]


def match_lists(descs, match_conf=0.3, range_width=0, pair_mask=None):
    """Every candidate pair's record (view_a, view_b, first, count, n_forward) and its rows, as ms_match_pairs lists them"""
    recs, rows, first = [], [], 0
    for a, b in candidate_pairs(len(descs), range_width, pair_mask):
        if len(descs[a]) == 0 or len(descs[b]) == 0:
            r, nf = np.zeros((0, 3), np.int32), 0
        else:
            r, nf = pair_list(descs[a], descs[b], match_conf)
        recs.append((a, b, first, len(r), nf)); rows.append(r)
        first += len(r)
    return recs, rows


def centred_points(kp, size, index):
    """keypoints (n, >= 2) float32, size (width, height), index: the list's keypoint indices -> (m, 2) float32 of (x - width * 0.5f, y - height * 0.5f)"""
    kp = np.asarray(kp, np.float32)
    out = np.empty((len(index), 2), np.float32)
    out[:, 0] = kp[index, 0] - np.float32(size[0]) * np.float32(0.5)
    out[:, 1] = kp[index, 1] - np.float32(size[1]) * np.float32(0.5)
    return out


def confidence(num_inliers, count):
    c = num_inliers / (8 + 0.3 * count)
    return 0.0 if c > 3.0 else c


def biggest_component(n_views, pairs, conf_threshold):
    """pairs: (view_a, view_b, confidence) -> the ascending views of the largest component; ties to the component that holds the lowest view"""
    comp = list(range(n_views))
    for a, b, c in pairs:
        if c >= conf_threshold and comp[a] != comp[b]:
            lo, hi = min(comp[a], comp[b]), max(comp[a], comp[b])
            comp = [lo if x == hi else x for x in comp]
    groups = {}
    for v, c in enumerate(comp):
        groups.setdefault(c, []).append(v)
    return max(groups.values(), key=lambda g: (len(g), -g[0]))


def wave_correct(R, kind=0):
    """R (n, 3, 3) float64 camera to rig, kind 0 = HORIZ, 1 = VERT -> (corrected rotations, status 1 where the input is returned)"""
    R = np.asarray(R, np.float64)
    if len(R) <= 1:
        return R.copy(), 1
    X = R[:, :, 0]
    moment = X.T @ X
    w, V = np.linalg.eigh(moment)           # ascending
    rg1 = V[:, 0] if kind == 0 else V[:, 2]
    rg0 = np.cross(rg1, R[:, :, 2].sum(axis=0))
    nrm = np.linalg.norm(rg0)
    if nrm <= np.finfo(np.float64).tiny:
        return R.copy(), 1
    rg0 = rg0 / nrm
    rg2 = np.cross(rg0, rg1)
    conf = (X @ rg0).sum() if kind == 0 else -(X @ rg1).sum()
    if conf < 0:
        rg0, rg1 = -rg0, -rg1
    G = np.stack([rg0, rg1, rg2])
    return np.einsum("ij,vjk->vik", G, R), 0
