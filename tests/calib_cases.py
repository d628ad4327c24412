"""Inputs of the per-op calibration tests: ms_voronoi_seams / ms_estimate_gains (tests/test_calib_kernels_gpu.py) and the CPU cross-check of the two references
on the very same inputs (tests/test_np_ref_crosscheck.py).  numpy only; every case is a pure function of its name (fixed seeds), so both files see the same bytes.

A Voronoi case is (rois, masks); a gain case is (rois, images, masks): rois = [(x, y, w, h)], masks uint8 (h, w), images uint8 (h, w, 3)."""
import zlib

import numpy as np

GAP = 10                                       # findInPair's gap (seam_finders.cpp:113): the kernels' window is the overlap grown by it
EDGE = (1, 43, 44, 45, 108, 109)               # overlap widths / heights rw for which rw + 2 * GAP is 21, 63, 64, 65, 128, 129: either side of the 64-lane blocks


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _holes(rng, m, rects=3, pixels=6, value=0):
    """random rectangular and single-pixel holes, in place"""
    h, w = m.shape
    for _ in range(int(rng.integers(0, rects + 1))):
        hh, ww = int(rng.integers(1, max(2, h // 3))), int(rng.integers(1, max(2, w // 3)))
        y, x = int(rng.integers(0, h - hh + 1)), int(rng.integers(0, w - ww + 1))
        m[y:y + hh, x:x + ww] = value
    for _ in range(int(rng.integers(1, pixels + 1))):
        m[int(rng.integers(0, h)), int(rng.integers(0, w))] = value
    return m


def _full(r):
    return np.full((r[3], r[2]), 255, np.uint8)


def overlap(a, b):
    x0, y0 = max(a[0], b[0]), max(a[1], b[1])
    x1, y1 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    return (x0, y0, x1 - x0, y1 - y0) if x0 < x1 and y0 < y1 else None


def _axis(rng, o, ov):
    """One axis of a two-view layout with an overlap of exactly `ov`: (start0, len0, start1, len1).  View 1 hangs over view 0's far end, over its near end,
    or lies inside it."""
    mode = int(rng.integers(0, 3))
    e0, e1 = int(rng.integers(3, 25)), int(rng.integers(3, 25))
    if mode == 0:
        return o, ov + e0, o + e0, ov + e1
    if mode == 1:
        return o, ov + e0, o - e1, ov + e1
    return o, ov + e0 + e1, o + e0, ov


def _two_views(name, rw, rh):
    rng = _rng(name)
    x0, w0, x1, w1 = _axis(rng, int(rng.integers(-70, 20)), rw)
    y0, h0, y1, h1 = _axis(rng, int(rng.integers(-70, 20)), rh)
    rois = [(x0, y0, w0, h0), (x1, y1, w1, h1)]
    if rng.integers(0, 2):
        rois.reverse()
    ox, oy, ow, oh = overlap(*rois)
    assert (ow, oh) == (rw, rh)
    masks = [_holes(rng, _full(r)) for r in rois]
    for m, r in zip(masks, rois):                      # at least one pixel both views claim, so that the seam has something to decide
        m[oy - r[1], ox - r[0]] = 255
    return rois, masks


def _mutual(name, n):
    """n views that all overlap one another: every pair's in-place edit is a later pair's input"""
    rng = _rng(name)
    rois = [(int(rng.integers(-18, 19)), int(rng.integers(-14, 15)), int(rng.integers(44, 60)), int(rng.integers(36, 50))) for _ in range(n)]
    assert all(overlap(rois[i], rois[j]) for i in range(n) for j in range(i + 1, n))
    return rois, [_holes(rng, _full(r)) for r in rois]


def _ring16(name):
    rng = _rng(name)
    rois = []
    for i in range(16):
        a = 2 * np.pi * i / 16
        rois.append((int(round(52 * np.cos(a))) - 12 + int(rng.integers(-2, 3)), int(round(40 * np.sin(a))) - 10 + int(rng.integers(-2, 3)),
                     int(rng.integers(24, 31)), int(rng.integers(20, 27))))
    assert all(overlap(rois[i], rois[(i + 1) % 16]) for i in range(16)) and not overlap(rois[0], rois[8])
    return rois, [_holes(rng, _full(r), rects=1, pixels=3) for r in rois]


def _grey(name):
    """mask values other than 0 and 255: findInPair tests `!= 0` (seam_finders.cpp:142-148), so 1, 128 and 254 are set pixels"""
    rng = _rng(name)
    rois = [(-9, 4, 47, 39), (14, -6, 52, 41), (3, 17, 40, 33)]
    masks = []
    for r in rois:
        m = rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), size=(r[3], r[2]), p=[0.1, 0.15, 0.15, 0.15, 0.45])
        masks.append(np.ascontiguousarray(m))
    return rois, masks


def _voronoi_builders():
    b = {}
    # two views: random corners (negative ones included), rectangular and single-pixel holes; every EDGE value as a width and as a height, crossed sparingly
    for rw, rh in ((1, 45), (43, 1), (44, 108), (45, 43), (108, 44), (109, 109), (45, 44), (1, 1)):
        b["pair_%dx%d" % (rw, rh)] = lambda n, rw=rw, rh=rh: _two_views(n, rw, rh)
    # no unique pixel in the gap-grown window: the first view has none (it lies inside the second one's set pixels), the second has none, neither has one
    b["nounique_first"] = lambda n: ([(0, 0, 30, 22), (-14, -12, 60, 50)], [_holes(_rng(n), _full((0, 0, 30, 22))), _full((0, 0, 60, 50))])
    b["nounique_second"] = lambda n: ([(-14, -12, 60, 50), (0, 0, 30, 22)], [_full((0, 0, 60, 50)), _holes(_rng(n), _full((0, 0, 30, 22)))])
    b["nounique_both"] = lambda n: ([(-7, 5, 47, 33), (-7, 5, 47, 33)], [_full((0, 0, 47, 33)), _full((0, 0, 47, 33))])
    # exact ties: mirror-symmetric full masks put dist1 == dist2 on the overlap's middle column / row (odd overlap) -- `<` sends them to the second view
    b["ties_columns"] = lambda n: ([(0, 0, 40, 30), (25, 0, 40, 30)], [_full((0, 0, 40, 30)), _full((0, 0, 40, 30))])
    b["ties_rows"] = lambda n: ([(3, -20, 31, 36), (3, 5, 31, 36)], [_full((0, 0, 31, 36)), _full((0, 0, 31, 36))])
    b["ties_none_even"] = lambda n: ([(0, 0, 40, 30), (24, 0, 40, 30)], [_full((0, 0, 40, 30)), _full((0, 0, 40, 30))])

    def nested(n):
        rng = _rng(n)
        rois = [(-20, -15, 70, 58), (-12, -9, 33, 27)]         # inside by 8 and 6 pixels on the near sides: less than the gap
        return rois, [_holes(rng, _full(r)) for r in rois]
    b["nested"] = nested
    b["touching"] = lambda n: ([(-5, 0, 30, 20), (25, 3, 22, 20)], [_holes(_rng(n), _full((0, 0, 30, 20))), _holes(_rng(n + "b"), _full((0, 0, 22, 20)))])
    b["disjoint"] = lambda n: ([(-5, 0, 30, 20), (40, -30, 22, 20)], [_holes(_rng(n), _full((0, 0, 30, 20))), _holes(_rng(n + "b"), _full((0, 0, 22, 20)))])
    b["single"] = lambda n: ([(-3, -4, 37, 29)], [_holes(_rng(n), _full((0, 0, 37, 29)))])
    for k in (3, 4, 5):
        b["mutual_%d" % k] = lambda n, k=k: _mutual(n, k)
    b["ring_16"] = _ring16
    b["grey_values"] = _grey
    return b


_VORONOI = _voronoi_builders()
VORONOI_CASES = list(_VORONOI)
VORONOI_UNTOUCHED = ("touching", "disjoint", "single")


def voronoi_case(name):
    rois, masks = _VORONOI[name](name)
    return [tuple(int(v) for v in r) for r in rois], [np.ascontiguousarray(m, np.uint8) for m in masks]


# ---- gains ----------------------------------------------------------------------------------------------------------------------------------------
def _image(rng, r, ratio):
    """a smooth random scene times the view's exposure ratio, with an all-0 and an all-255 patch: sqrt(0) and sqrt(3 * 255^2) are the ends of the range"""
    h, w = r[3], r[2]
    yy, xx = np.mgrid[0:h, 0:w]
    base = 120 + 60 * np.sin((xx + r[0]) * 0.21)[..., None] * np.cos((yy + r[1]) * 0.17)[..., None] + rng.integers(-25, 26, size=(h, w, 3))
    im = np.clip(base * ratio, 0, 255).astype(np.uint8)
    im[: h // 4, : w // 5] = 0
    im[h - h // 4:, w - w // 5:] = 255
    return im


def _gain_mask(rng, r):
    m = _holes(rng, _full(r))
    _holes(rng, m, rects=1, pixels=3, value=254)                  # 254 and 128 are not feed's level value 255: such pixels must not count
    _holes(rng, m, rects=1, pixels=3, value=128)
    return m


def _gain_rig(name, n):
    """n views along a row, each over its next two, corners below zero; from 4 views on one view nested in another and far pairs that do not meet"""
    rng = _rng(name)
    rois = []
    for i in range(n):
        rois.append((-45 + 17 * i + int(rng.integers(-3, 4)), -12 + int(rng.integers(-6, 7)), int(rng.integers(38, 48)), int(rng.integers(30, 40))))
    if n >= 4:
        a = rois[1]
        rois[n - 1] = (a[0] + 5, a[1] + 4, a[2] - 11, a[3] - 9)   # the last view lies inside view 1
    if n >= 5:
        assert any(overlap(rois[i], rois[j]) is None for i in range(n) for j in range(i + 1, n))
    ratios = [0.55 + 0.9 * ((i * 7) % n) / max(1, n - 1) for i in range(n)]
    return rois, [_image(rng, r, q) for r, q in zip(rois, ratios)], [_gain_mask(rng, r) for r in rois]


def _gain_no_common(name):
    """views 0 and 1 overlap as rectangles but share no 255 pixel there (N = 1, I = 0); both share plenty with view 2"""
    rng = _rng(name)
    rois = [(-30, -8, 40, 34), (-2, -4, 42, 30), (-20, 10, 56, 30)]
    masks = [_gain_mask(rng, r) for r in rois]
    ox, oy, ow, oh = overlap(rois[0], rois[1])
    m0 = masks[0][oy - rois[0][1]:oy - rois[0][1] + oh, ox - rois[0][0]:ox - rois[0][0] + ow]
    m0[m0 == 255] = 254
    return rois, [_image(rng, r, q) for r, q in zip(rois, (0.7, 1.0, 1.3))], masks


def _gain_row_swap(name):
    """A system on which LUImpl exchanges rows (matrix_decomp.cpp:60-77).  Views 0 and 1 are 255 only inside their common overlap, so N00 = N01 = N11 = N; view 0
    is near intensity 30 there, view 1 near 441.  Then |A10| = 0.02 * 30 * 441 * N = 264.6 N exceeds A00 = (200 + 0.02 * 30^2) N + 100 (pairs with N = 1) = 218 N + ...:
    column 0's pivot is row 1.  Views 2 and 3 are an ordinary pair further along."""
    rng = _rng(name)
    rois = [(-20, -10, 40, 30), (0, -6, 44, 32), (30, -2, 40, 30), (52, 4, 38, 28)]
    masks = [np.zeros((r[3], r[2]), np.uint8) for r in rois[:2]] + [_gain_mask(rng, r) for r in rois[2:]]
    ox, oy, ow, oh = overlap(rois[0], rois[1])
    for k in (0, 1):
        masks[k][oy - rois[k][1]:oy - rois[k][1] + oh, ox - rois[k][0]:ox - rois[k][0] + ow] = 255
    imgs = [rng.integers(15, 20, size=(rois[0][3], rois[0][2], 3)).astype(np.uint8), rng.integers(250, 256, size=(rois[1][3], rois[1][2], 3)).astype(np.uint8),
            _image(rng, rois[2], 0.8), _image(rng, rois[3], 1.2)]
    return rois, imgs, masks


def counted_extremes(rois, imgs, masks):
    """(black, white): how many all-0 and all-255 image pixels enter a pair sum, i.e. lie in the overlap of two different views under 255 in both masks"""
    black = white = 0
    for i in range(len(rois)):
        for j in range(i + 1, len(rois)):
            o = overlap(rois[i], rois[j])
            if o is None:
                continue
            ox, oy, ow, oh = o
            win = [(slice(oy - r[1], oy - r[1] + oh), slice(ox - r[0], ox - r[0] + ow)) for r in (rois[i], rois[j])]
            both = (masks[i][win[0]] == 255) & (masks[j][win[1]] == 255)
            for k, s in zip((i, j), win):
                black += int(((imgs[k][s] == 0).all(axis=2) & both).sum())
                white += int(((imgs[k][s] == 255).all(axis=2) & both).sum())
    return black, white


def _gain_builders():
    b = {}
    for n in (1, 2, 3, 4, 5, 8, 9, 16):            # 1-3: the closed forms; 8, 9: n^2 on either side of k_gain_pairs' 64-thread block; 16 = MS_MAX_VIEWS
        b["views_%d" % n] = lambda name, n=n: _gain_rig(name, n)
    b["no_common_255"] = _gain_no_common
    b["lu_row_exchange"] = _gain_row_swap
    return b


_GAINS = _gain_builders()
GAIN_CASES = list(_GAINS)
GAIN_ROW_SWAP_CASES = ("lu_row_exchange",)


def gain_case(name):
    rois, imgs, masks = _GAINS[name](name)
    return ([tuple(int(v) for v in r) for r in rois], [np.ascontiguousarray(i, np.uint8) for i in imgs], [np.ascontiguousarray(m, np.uint8) for m in masks])
