"""ms_dp_seams / ms_set_seam_finder / ms_get_seam_finder at the C-ABI, without a device: declared, exported and bound; every argument check of ms_dp_seams runs
before the first HIP call (MS_ERR_INVALID with a message on a machine without a GPU, where a well-formed call gets as far as MS_ERR_NO_DEVICE); and the numpy
statement of the contract (tests/dp_seam_ref.py), which the GPU tests compare the kernels with bit for bit, checked against itself: brute-force path enumeration,
the invariants of the edit, and what the seam is for -- on the parallax scene it goes round the object the Voronoi seam cuts through."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import dp_seam_cases as cases
import dp_seam_ref as ref
import np_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_dp_seams", "ms_set_seam_finder", "ms_get_seam_finder")
MS_MAX_VIEWS = 16


def test_declared_exported_and_listed(ms):
    raw = open(os.path.join(ROOT, "include", "ms_stitch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in ms_stitch.h" % n
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
        assert n in ms.EXPORTS
    assert int(re.search(r"MS_DP_MAX_SIDE\s*=\s*(\d+)", text).group(1)) == ref.MAX_SIDE == ms.DP_MAX_SIDE
    assert re.search(r"MS_SEAM_VORONOI\s*=\s*0\s*,\s*MS_SEAM_DP\s*=\s*1", text) and (ms.SEAM_VORONOI, ms.SEAM_DP) == (0, 1)
    comment = raw[:raw.index("MS_API int ms_dp_seams(")].rsplit("/*", 1)[1]
    for word in ("SYNCHRONOUS", "IN PLACE", "calibration.cpp:134-135", "1024", "|2 x - (w - 1)|", "MS_DP_MAX_SIDE"):      # the contract is stated where the call is declared
        assert word in comment, word
    assert hasattr(ms, "dp_seams") and hasattr(ms.Compositor, "set_seam_finder")


class Args:
    """two well-formed views in host memory standing in for device memory: no check may dereference them"""

    def __init__(self, ms, n=2, w=12, h=9, dx=5):
        self.ms, self.n = ms, n
        self.buf = (C.c_uint8 * (12 * 9 * 3))()
        p = C.cast(self.buf, C.c_void_p)
        self.rois = (ms.Rect * n)(*[ms.Rect(-3 + dx * i, -2, w, h) for i in range(n)])
        self.masks = (ms.Image * n)(*[ms.Image(p, w, w, h, ms.MS_8UC1) for _ in range(n)])
        self.imgs = (ms.Image * n)(*[ms.Image(p, 3 * w, w, h, ms.MS_8UC3) for _ in range(n)])

    def dp(self, n=None, rois=0, imgs=0, masks=0):
        return self.ms.load().ms_dp_seams(self.n if n is None else n, self.rois if rois == 0 else rois, self.imgs if imgs == 0 else imgs,
                                          self.masks if masks == 0 else masks, None)


def _invalid(ms, rc, *words):
    msg = ms.load().ms_last_error().decode()
    assert rc == -1, (rc, msg)          # MS_ERR_INVALID
    assert all(w in msg for w in words), msg


def test_well_formed_call_reaches_the_device_check(ms):
    if ms.device_count() > 0:
        return                      # (host memory must not reach a kernel; on a GPU box tests/test_dp_seams_gpu.py runs these view counts)
    assert Args(ms).dp() == -4 and Args(ms, n=1).dp() == -4 and Args(ms, n=MS_MAX_VIEWS).dp() == -4          # MS_ERR_NO_DEVICE
    assert Args(ms, w=ref.MAX_SIDE + 30, h=2, dx=30).dp() == -4                                                  # an overlap of exactly MS_DP_MAX_SIDE is served


@pytest.mark.parametrize("n", [0, -1, MS_MAX_VIEWS + 1])
def test_view_count_outside_the_range(ms, n):
    _invalid(ms, Args(ms, n=MS_MAX_VIEWS + 1).dp(n=n), "ms_dp_seams", "outside [1, 16]")


def test_null_pointers(ms):
    a = Args(ms)
    _invalid(ms, a.dp(rois=None), "ms_dp_seams", "null rois")
    _invalid(ms, a.dp(masks=None), "ms_dp_seams", "null")
    _invalid(ms, a.dp(imgs=None), "ms_dp_seams", "null")
    a.masks[1].data = None
    _invalid(ms, a.dp(), "mask 1", "null image")
    a = Args(ms)
    a.imgs[0].data = None
    _invalid(ms, a.dp(), "image 0", "null image")


def test_type_codes(ms):
    a = Args(ms)
    a.masks[1].type = ms.MS_8UC3
    _invalid(ms, a.dp(), "mask 1", "8UC1")
    a = Args(ms)
    for t in (ms.MS_8UC1, ms.MS_16SC3, ms.MS_32FC1):
        a.imgs[1].type = t
        _invalid(ms, a.dp(), "image 1", "8UC3")


@pytest.mark.parametrize("field,delta", [("cols", 1), ("cols", -1), ("rows", 1), ("rows", -1)])
def test_sizes_must_equal_the_roi(ms, field, delta):
    a = Args(ms)
    setattr(a.masks[0], field, getattr(a.masks[0], field) + delta)
    _invalid(ms, a.dp(), "mask 0", "its ROI 12x9")
    a = Args(ms)
    setattr(a.imgs[1], field, getattr(a.imgs[1], field) + delta)
    _invalid(ms, a.dp(), "image 1", "its ROI 12x9")


@pytest.mark.parametrize("w,h", [(0, 9), (12, 0), (-12, 9), (12, -1)])
def test_empty_roi(ms, w, h):
    a = Args(ms)
    a.rois[1].width, a.rois[1].height = w, h
    a.masks[1].cols, a.masks[1].rows, a.imgs[1].cols, a.imgs[1].rows = w, h, w, h
    _invalid(ms, a.dp(), "roi 1", "empty")


def test_roi_that_leaves_the_int_range(ms):
    a = Args(ms)
    a.rois[0].x = 2 ** 31 - 5            # x + width > INT_MAX: the overlap arithmetic would wrap
    _invalid(ms, a.dp(), "roi 0")
    a.rois[0].x, a.rois[0].y = 0, 2 ** 31 - 5
    _invalid(ms, a.dp(), "roi 0")


@pytest.mark.parametrize("pad", [1, 4, 64])
def test_rows_must_be_contiguous(ms, pad):
    a = Args(ms)
    a.masks[1].step = 12 + pad
    _invalid(ms, a.dp(), "mask 1", "contiguous")
    a = Args(ms)
    a.imgs[0].step = 36 + pad
    _invalid(ms, a.dp(), "image 0", "contiguous")
    a.imgs[0].step = 12                  # (a step shorter than a row is no better)
    _invalid(ms, a.dp(), "image 0", "contiguous")


def test_overlap_side_above_the_limit_names_the_pair(ms):
    """M stays below 2^23 and a row of it in LDS because no overlap side exceeds MS_DP_MAX_SIDE; 4097 is refused on the host, width or height, and the message says which pair"""
    side = ref.MAX_SIDE + 1
    a = Args(ms, n=3, w=side + 30, h=2, dx=30)          # views 0 and 1 overlap by 4097 columns (so do 1 and 2; 0 and 2 by 4067)
    _invalid(ms, a.dp(), "views 0 and 1", "%dx2" % side, "MS_DP_MAX_SIDE")
    a = Args(ms, n=3, w=3, h=side, dx=700)
    a.rois[2].x, a.rois[2].y = a.rois[1].x + 1, a.rois[1].y          # only views 1 and 2 meet: 2 columns, 4097 rows
    _invalid(ms, a.dp(), "views 1 and 2", "2x%d" % side)


def test_finder_value_and_null_context(ms):
    lib = ms.load()
    for bad in (-1, 2, 77):
        _invalid(ms, lib.ms_set_seam_finder(None, bad), "ms_set_seam_finder", "finder %d" % bad)
    _invalid(ms, lib.ms_set_seam_finder(None, ms.SEAM_DP), "null context")
    v = C.c_int(5)
    _invalid(ms, lib.ms_get_seam_finder(None, C.byref(v)), "ms_get_seam_finder", "null")


# ---- the reference against itself -----------------------------------------------------------------------------------------------------------------------
def _brute(c):
    """the least path cost over every path of the contract's shape, and -- among the least ones -- nothing else: (cost)"""
    h, w = c.shape
    best = None
    for x0 in range(w):
        for steps in itertools.product((-1, 0, 1), repeat=h - 1):
            x, s, ok = x0, int(c[0, x0]), True
            for y, d in enumerate(steps, 1):
                x += d
                if not 0 <= x < w:
                    ok = False
                    break
                s += int(c[y, x])
            if ok and (best is None or s < best):
                best = s
    return best


def test_dp_value_equals_brute_force_enumeration():
    rng = np.random.default_rng(20261019)
    for k in range(300):
        h, w = int(rng.integers(1, 5)), int(rng.integers(1, 6))          # at most 5 x 4
        c = rng.choice(np.array([0, 0, 3, 7, 40, ref.OUTSIDE]), size=(h, w)) if k % 2 else rng.integers(0, 766, size=(h, w))
        seam, cost = ref.dp_path(c.astype(np.int64))
        assert cost == _brute(c), (k, c)
        assert cost == sum(int(c[y, seam[y]]) for y in range(h)) and all(abs(int(seam[y]) - int(seam[y - 1])) <= 1 for y in range(1, h))


def test_all_costs_equal_on_full_masks_gives_the_straight_middle_line():
    """every cost ties: each step prefers x itself, and the end column is the one nearest the middle, the smaller of two"""
    for w in (1, 2, 7, 8):
        seam, cost = ref.dp_path(np.zeros((6, w), np.int64))
        assert cost == 0 and (seam == (w - 1) // 2).all(), (w, seam)


@pytest.mark.parametrize("name", cases.CASES)
def test_reference_invariants(name):
    rois, imgs, masks = cases.case(name)
    trace = []
    out = ref.dp_seams(rois, imgs, masks, trace)
    assert all(np.array_equal(a, b) for a, b in zip(masks, cases.case(name)[2])), "the reference edited its input"
    for v, (a, b) in enumerate(zip(masks, out)):
        assert ((b == a) | (b == 0)).all(), "view %d: a seam only clears" % v
    n = len(rois)
    for i in range(n - 1):
        for j in range(i + 1, n):
            o = ref.overlap(rois[i], rois[j])
            if o is None:
                continue
            si = (slice(o[1] - rois[i][1], o[1] - rois[i][1] + o[3]), slice(o[0] - rois[i][0], o[0] - rois[i][0] + o[2]))
            sj = (slice(o[1] - rois[j][1], o[1] - rois[j][1] + o[3]), slice(o[0] - rois[j][0], o[0] - rois[j][0] + o[2]))
            assert not ((out[i][si] != 0) & (out[j][sj] != 0)).any(), "views %d and %d both still claim a pixel of their overlap" % (i, j)
    # a pixel only one view held at the start is nobody's to clear
    cx, cy, cw, ch = cases._canvas(rois)
    count = np.zeros((ch, cw), np.int64)
    for r, m in zip(rois, masks):
        count[r[1] - cy:r[1] - cy + r[3], r[0] - cx:r[0] - cx + r[2]] += m != 0
    for v, (r, a, b) in enumerate(zip(rois, masks, out)):
        alone = (count[r[1] - cy:r[1] - cy + r[3], r[0] - cx:r[0] - cx + r[2]] == 1) & (a != 0)
        assert np.array_equal(a[alone], b[alone]), "view %d lost pixels only it held" % v
    if name in cases.PAIR_ORIENTATION:
        assert len(trace) == 1 and (trace[0][2]["horizontal"], trace[0][2]["first"]) == cases.PAIR_ORIENTATION[name], "the case no longer has the orientation its name says"
    if name in cases.MULTI_SLAB_CASES:
        assert trace[0][2]["c"].size > cases.SLAB_CELLS
    if name.endswith("/same"):
        assert all(p["cost"] == ref.OUTSIDE * int((~p["both"].T if p["horizontal"] else ~p["both"])[np.arange(len(p["seam"])), p["seam"]].sum()) for _, _, p in trace)


def test_the_case_list_covers_what_the_kernel_branches_on():
    import calib_cases
    assert {c.split("/")[0] for c in cases.LAYOUT_CASES} == set(calib_cases.VORONOI_CASES) and len(cases.LAYOUT_CASES) == 3 * len(calib_cases.VORONOI_CASES)
    for w in (1, 2, 63, 64, 65, 255, 256, 257):
        assert "v_w%d" % w in cases.CASES and "h_w%d" % w in cases.CASES
    assert {"v_65x1", "v_65x2", "h_65x1", "h_65x2", "v_1100x7", "v_i_second", "h_i_second"} <= set(cases.CASES)


def test_parallax_scene_the_dp_seam_goes_round_the_object_voronoi_cuts_it():
    rois, imgs, masks = cases.parallax_scene()
    p = ref.pair_seam(rois[0], imgs[0], masks[0], rois[1], imgs[1], masks[1])
    assert p["o"] == (52, 0, 48, 64) and not p["horizontal"] and p["first"] == 0 and p["both"].all()
    c = p["c"]
    rows = np.arange(64)
    dp_on_object = int((c[rows, p["seam"]] > 300).sum())
    vor = np_ref.voronoi_seams([r[:2] for r in rois], [m.copy() for m in masks])
    kept = vor[0][:, 52:100] != 0                                   # view 0's side of the Voronoi cut, over the overlap
    assert kept[:, 0].all() and not kept[:, -1].all() and (np.diff(kept.astype(np.int8), axis=1) <= 0).all()
    vor_seam = kept.sum(axis=1) - 1                                 # its last column in every row: the Voronoi seam in the DP seam's terms
    vor_on_object = int((c[rows, vor_seam] > 300).sum())
    vor_cost = int(c[rows, vor_seam].sum())
    print("seam pixels with c > 300: dp %d, voronoi %d of 64; seam cost: dp %d, voronoi %d" % (dp_on_object, vor_on_object, p["cost"], vor_cost))
    assert dp_on_object == 0
    assert vor_on_object > 0
    assert p["cost"] <= vor_cost
    out = ref.dp_seams(rois, imgs, masks)
    assert not ((out[0][:, 52:100] != 0) & (out[1][:, 0:48] != 0)).any() and ((out[0][:, 52:100] != 0) | (out[1][:, 0:48] != 0)).all()
