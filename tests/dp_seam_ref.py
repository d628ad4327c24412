"""The contract of ms_dp_seams (include/ms_stitch.h) in numpy: per-pair loops and a row loop, nothing shared with the product.  Integer arithmetic only, so
the product is compared with np.array_equal.

rois = [(x, y, w, h)], images uint8 (h, w, 3), masks uint8 (h, w); dp_seams returns the edited copies of the masks and leaves its inputs alone."""
import numpy as np

GAP = 10                 # the window of the orientation rule: the overlap grown by Voronoi's gap
OUTSIDE = 1024           # cost of an overlap pixel that is not set in both masks
MAX_SIDE = 4096          # MS_DP_MAX_SIDE


def overlap(a, b):
    x0, y0 = max(a[0], b[0]), max(a[1], b[1])
    x1, y1 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    return (x0, y0, x1 - x0, y1 - y0) if x0 < x1 and y0 < y1 else None


def _sums(roi, mask, o):
    """n, sum x, sum y (python ints) of the view's set pixels inside the overlap grown by GAP and clipped to the view, relative to (o.x - GAP, o.y - GAP)"""
    wx0, wy0 = o[0] - GAP, o[1] - GAP
    x0, y0 = max(wx0, roi[0]), max(wy0, roi[1])
    x1, y1 = min(o[0] + o[2] + GAP, roi[0] + roi[2]), min(o[1] + o[3] + GAP, roi[1] + roi[3])
    ys, xs = np.nonzero(mask[y0 - roi[1]:y1 - roi[1], x0 - roi[0]:x1 - roi[0]])
    return int(len(xs)), int(xs.astype(np.int64).sum()) + len(xs) * (x0 - wx0), int(ys.astype(np.int64).sum()) + len(ys) * (y0 - wy0)


def orientation(roi_i, mask_i, roi_j, mask_j, o):
    """(horizontal, first): horizontal = the seam is one row per column; first = 0 if view i owns the side at or before the seam, else 1"""
    ni, sxi, syi = _sums(roi_i, mask_i, o)
    nj, sxj, syj = _sums(roi_j, mask_j, o)
    dx, dy = sxj * ni - sxi * nj, syj * ni - syi * nj
    horizontal = not abs(dx) >= abs(dy)
    d = dy if horizontal else dx
    return horizontal, 0 if d >= 0 else 1


def cost_plane(img_i, mask_i, img_j, mask_j):
    """the overlap's cost (int64) and B from the two views' overlap windows"""
    both = (mask_i != 0) & (mask_j != 0)
    c = np.abs(img_i.astype(np.int64) - img_j.astype(np.int64)).sum(axis=2)
    return np.where(both, c, OUTSIDE), both


def dp_path(c):
    """the seam column of every row of the cost plane c (h, w), and the path's cost M(h - 1, end)"""
    h, w = c.shape
    M = np.zeros((h, w), np.int64)
    step = np.zeros((h, w), np.int64)          # the column offset to the predecessor
    M[0] = c[0]
    never = np.array([np.iinfo(np.int64).max], np.int64)
    for y in range(1, h):
        up = M[y - 1]
        left, right = np.concatenate([never, up[:-1]]), np.concatenate([up[1:], never])        # M(y - 1, x - 1), M(y - 1, x + 1); nothing outside [0, w)
        best, dxy = up.copy(), np.zeros(w, np.int64)                        # ties prefer x, then x - 1, then x + 1
        take = left < best
        best[take], dxy[take] = left[take], -1
        take = right < best
        best[take], dxy[take] = right[take], 1
        M[y], step[y] = c[y] + best, dxy
    end = min(range(w), key=lambda x: (int(M[h - 1, x]), abs(2 * x - (w - 1)), x))
    seam = np.zeros(h, np.int64)
    x = end
    for y in range(h - 1, -1, -1):
        seam[y] = x
        x += step[y, x]
    return seam, int(M[h - 1, end])


def pair_seam(roi_i, img_i, mask_i, roi_j, img_j, mask_j):
    """None if the ROIs do not meet, else dict(o, horizontal, first, seam, cost, c, both): seam[t] is the column of row t (vertical) or the row of column t"""
    o = overlap(roi_i, roi_j)
    if o is None:
        return None
    assert o[2] <= MAX_SIDE and o[3] <= MAX_SIDE
    si = (slice(o[1] - roi_i[1], o[1] - roi_i[1] + o[3]), slice(o[0] - roi_i[0], o[0] - roi_i[0] + o[2]))
    sj = (slice(o[1] - roi_j[1], o[1] - roi_j[1] + o[3]), slice(o[0] - roi_j[0], o[0] - roi_j[0] + o[2]))
    horizontal, first = orientation(roi_i, mask_i, roi_j, mask_j, o)
    c, both = cost_plane(img_i[si], mask_i[si], img_j[sj], mask_j[sj])
    seam, cost = dp_path(c.T if horizontal else c)
    return dict(o=o, horizontal=horizontal, first=first, seam=seam, cost=cost, c=c, both=both, si=si, sj=sj)


def first_side(p):
    """bool (h, w) over the overlap: the pixels at or before the seam"""
    _, _, w, h = p["o"]
    if p["horizontal"]:
        return np.arange(h)[:, None] <= p["seam"][None, :]
    return np.arange(w)[None, :] <= p["seam"][:, None]


def dp_seams(rois, images, masks, trace=None):
    """every pair i < j with overlapping ROIs, in order, each on the masks the pairs before it left.  trace (a list) receives (i, j, pair_seam's dict)."""
    masks = [m.copy() for m in masks]
    n = len(rois)
    for i in range(n - 1):
        for j in range(i + 1, n):
            p = pair_seam(rois[i], images[i], masks[i], rois[j], images[j], masks[j])
            if p is None:
                continue
            near = first_side(p)
            own_first, own_second = (masks[i], masks[j]) if p["first"] == 0 else (masks[j], masks[i])
            s_first, s_second = (p["si"], p["sj"]) if p["first"] == 0 else (p["sj"], p["si"])
            own_second[s_second][p["both"] & near] = 0                      # on the first side the second view goes
            own_first[s_first][p["both"] & ~near] = 0                       # beyond the seam the first view goes
            if trace is not None:
                trace.append((i, j, p))
    return masks
