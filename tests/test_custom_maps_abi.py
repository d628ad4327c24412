"""ms_set_maps / ms_get_map_source: what is refused before the device is touched, and the binding's view of the header (no GPU needed).
A context cannot exist without a device (ms_create), so the argument checks that need one are in tests/test_custom_maps_gpu.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_arguments_are_invalid(ms):
    lib = ms.load()
    r = (ms.Rect * 1)(ms.Rect(0, 0, 8, 8))
    m = (ms.Image * 1)(ms.Image())
    assert lib.ms_set_maps(None, r, m, m, None) == -1      # MS_ERR_INVALID
    assert b"ms_set_maps" in lib.ms_last_error()
    src = C.c_int(7)
    assert lib.ms_get_map_source(None, C.byref(src)) == -1 and src.value == 7
    assert b"ms_get_map_source" in lib.ms_last_error()


def test_binding_constants_are_the_headers(ms):
    text = open(os.path.join(ROOT, "include", "ms_stitch.h")).read()
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(MS_MAPS_\w+)\s*=\s*(\d+)", text))
    assert enums == {"MS_MAPS_MIN_WIDTH": ms.MAPS_MIN_WIDTH, "MS_MAPS_MIN_HEIGHT": ms.MAPS_MIN_HEIGHT, "MS_MAPS_MAX_SIDE": ms.MAPS_MAX_SIDE,
                     "MS_MAPS_ANALYTIC": ms.MAPS_ANALYTIC, "MS_MAPS_CUSTOM": ms.MAPS_CUSTOM}
    assert "ms_set_maps" in ms.EXPORTS and "ms_get_map_source" in ms.EXPORTS
    assert callable(ms.Compositor.set_maps) and callable(ms.Compositor.map_source)


def test_the_max_side_leaves_room_for_the_padding():
    """MS_MAPS_MAX_SIDE is derived from the 16-bit tile origins: padded view = view + less than 8 * 2^num_bands, num_bands <= 7 (blender_view_pad: a gap of
    3 * 2^nb either side, the start rounded down and the size rounded up to multiples of 2^nb), and must stay at or below 32767"""
    text = open(os.path.join(ROOT, "include", "ms_stitch.h")).read()
    side = int(re.search(r"MS_MAPS_MAX_SIDE\s*=\s*(\d+)", text).group(1))
    descs = open(os.path.join(ROOT, "video-stitcher_amd", "csrc", "descs.hpp")).read()
    max_levels = int(re.search(r"MAX_LEVELS\s*=\s*(\d+)", descs).group(1))
    m = 1 << (max_levels - 1)
    worst = 0
    for off in range(m):                       # the view's corner at every offset inside the padded pano, far from its edges
        tl = 10 * m + off
        ax = (tl - 3 * m) // m * m
        wdt = -(-(tl + side + 3 * m - ax) // m) * m
        worst = max(worst, wdt)
    assert worst <= 32767 and worst < side + 8 * m
    assert side + 8 * m == 32768
