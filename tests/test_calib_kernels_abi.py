"""ms_voronoi_seams / ms_estimate_gains at the C-ABI, without a device: declared, exported and bound, and every argument check runs before the first HIP call --
a bad argument is MS_ERR_INVALID (-1) with a message on a machine without a GPU too, where a well-formed call gets as far as MS_ERR_NO_DEVICE (-4)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_voronoi_seams", "ms_estimate_gains")
MS_MAX_VIEWS = 16


def test_declared_exported_and_listed(ms):
    raw = open(os.path.join(ROOT, "include", "ms_stitch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in ms_stitch.h" % n
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
        assert n in ms.EXPORTS
    assert int(re.search(r"#define\s+MS_MAX_VIEWS\s+(\d+)", text).group(1)) == MS_MAX_VIEWS
    # each cites the reference call it replaces, and says that it blocks
    for n, cites in (("ms_voronoi_seams", ("seam_finders.cpp:85-160", "calibration.cpp:134-135")), ("ms_estimate_gains", ("exposure_compensate.cpp:71-145", "calibration.cpp:122-132"))):
        comment = raw[:raw.index("MS_API int %s(" % n)].rsplit("/*", 1)[1]
        assert all(c in comment for c in cites) and "SYNCHRONOUS" in comment, n


class Args:
    """two well-formed views in host memory standing in for device memory: no check may dereference them"""

    def __init__(self, ms, n=2, w=12, h=9):
        self.ms, self.n = ms, n
        self.buf = (C.c_uint8 * (w * h * 3))()
        p = C.cast(self.buf, C.c_void_p)
        self.rois = (ms.Rect * n)(*[ms.Rect(-3 + 5 * i, -2, w, h) for i in range(n)])
        self.masks = (ms.Image * n)(*[ms.Image(p, w, w, h, ms.MS_8UC1) for _ in range(n)])
        self.imgs = (ms.Image * n)(*[ms.Image(p, 3 * w, w, h, ms.MS_8UC3) for _ in range(n)])
        self.g, self.N, self.I = (C.c_double * n)(), (C.c_int * (n * n))(), (C.c_double * (n * n))()

    def voronoi(self, n=None, rois=0, masks=0):
        return self.ms.load().ms_voronoi_seams(self.n if n is None else n, self.rois if rois == 0 else rois, self.masks if masks == 0 else masks, None)

    def gains(self, n=None, rois=0, imgs=0, masks=0, g=0, N=0, I=0):
        return self.ms.load().ms_estimate_gains(self.n if n is None else n, self.rois if rois == 0 else rois, self.imgs if imgs == 0 else imgs,
                                                self.masks if masks == 0 else masks, self.g if g == 0 else g, self.N if N == 0 else N, self.I if I == 0 else I, None)


def _invalid(ms, rc, *words):
    msg = ms.load().ms_last_error().decode()
    assert rc == -1, (rc, msg)          # MS_ERR_INVALID
    assert all(w in msg for w in words), msg


def test_well_formed_call_reaches_the_device_check(ms):
    if ms.device_count() > 0:
        return                      # (host memory must not reach a kernel; on a GPU box tests/test_calib_kernels_gpu.py runs these view counts)
    a = Args(ms)
    assert a.voronoi() == -4 and a.gains() == -4 and a.gains(N=None, I=None) == -4          # MS_ERR_NO_DEVICE; N / I are optional
    one = Args(ms, n=1)
    assert one.voronoi() == -4 and one.gains() == -4
    full = Args(ms, n=MS_MAX_VIEWS)
    assert full.voronoi() == -4 and full.gains() == -4


@pytest.mark.parametrize("n", [0, -1, MS_MAX_VIEWS + 1])
def test_view_count_outside_the_range(ms, n):
    a = Args(ms, n=MS_MAX_VIEWS + 1)
    _invalid(ms, a.voronoi(n=n), "ms_voronoi_seams", "outside [1, 16]")
    _invalid(ms, a.gains(n=n), "ms_estimate_gains", "outside [1, 16]")


def test_null_pointers(ms):
    a = Args(ms)
    _invalid(ms, a.voronoi(rois=None), "ms_voronoi_seams", "null rois")
    _invalid(ms, a.voronoi(masks=None), "ms_voronoi_seams", "null masks")
    _invalid(ms, a.gains(rois=None), "ms_estimate_gains", "null rois")
    for kw in ("imgs", "masks", "g"):
        _invalid(ms, a.gains(**{kw: None}), "ms_estimate_gains", "null")
    a.masks[1].data = None
    _invalid(ms, a.voronoi(), "mask 1", "null image")
    _invalid(ms, a.gains(), "mask 1", "null image")
    a = Args(ms)
    a.imgs[0].data = None
    _invalid(ms, a.gains(), "image 0", "null image")


def test_type_codes(ms):
    a = Args(ms)
    a.masks[1].type = ms.MS_8UC3
    _invalid(ms, a.voronoi(), "mask 1", "8UC1")
    _invalid(ms, a.gains(), "mask 1", "8UC1")
    a = Args(ms)
    for t in (ms.MS_8UC1, ms.MS_16SC3, ms.MS_32FC1):
        a.imgs[1].type = t
        _invalid(ms, a.gains(), "image 1", "8UC3")


@pytest.mark.parametrize("field,delta", [("cols", 1), ("cols", -1), ("rows", 1), ("rows", -1)])
def test_sizes_must_equal_the_roi(ms, field, delta):
    a = Args(ms)
    setattr(a.masks[0], field, getattr(a.masks[0], field) + delta)
    _invalid(ms, a.voronoi(), "mask 0", "its ROI 12x9")
    _invalid(ms, a.gains(), "mask 0", "its ROI 12x9")
    a = Args(ms)
    setattr(a.imgs[1], field, getattr(a.imgs[1], field) + delta)
    _invalid(ms, a.gains(), "image 1", "its ROI 12x9")


@pytest.mark.parametrize("w,h", [(0, 9), (12, 0), (-12, 9), (12, -1)])
def test_empty_roi(ms, w, h):
    a = Args(ms)
    a.rois[1].width, a.rois[1].height = w, h
    a.masks[1].cols, a.masks[1].rows, a.imgs[1].cols, a.imgs[1].rows = w, h, w, h
    _invalid(ms, a.voronoi(), "roi 1", "empty")
    _invalid(ms, a.gains(), "roi 1", "empty")


def test_roi_that_leaves_the_int_range(ms):
    a = Args(ms)
    a.rois[0].x = 2 ** 31 - 5            # x + width > INT_MAX: the overlap arithmetic would wrap
    _invalid(ms, a.voronoi(), "roi 0")
    a.rois[0].x, a.rois[0].y = 0, 2 ** 31 - 5
    _invalid(ms, a.gains(), "roi 0")


@pytest.mark.parametrize("pad", [1, 4, 64])
def test_rows_must_be_contiguous(ms, pad):
    """the kernels index step == width and step == 3 * width: a padded image is refused with a message, not staged and not misread"""
    a = Args(ms)
    a.masks[1].step = 12 + pad
    _invalid(ms, a.voronoi(), "mask 1", "contiguous")
    _invalid(ms, a.gains(), "mask 1", "contiguous")
    a = Args(ms)
    a.imgs[0].step = 36 + pad
    _invalid(ms, a.gains(), "image 0", "contiguous")
    a.imgs[0].step = 12                  # (a step shorter than a row is no better)
    _invalid(ms, a.gains(), "image 0", "contiguous")
