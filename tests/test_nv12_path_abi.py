"""The NV12 path at the C-ABI: ms_stitch_nv12_i420, ms_gain_stats_nv12, ms_track_gains_nv12 and ms_nv12_resize_linear_batch are declared, exported and listed;
they refuse a null context / null image with a message, and the per-op call reports the missing device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_stitch_nv12_i420", "ms_gain_stats_nv12", "ms_track_gains_nv12", "ms_nv12_resize_linear_batch")
MS_ERR_INVALID, MS_ERR_NO_DEVICE = -1, -4


def test_declared_exported_and_listed(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in ms_stitch.h" % n
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
        assert n in ms.EXPORTS
    assert "out of scope: convert one frame set" not in open(os.path.join(ROOT, "include", "ms_stitch.h")).read()


def test_null_context_is_invalid(ms):
    lib = ms.load()
    prm = ms.gain_track_default_params()
    n, s = (C.c_longlong * 4)(), (C.c_longlong * 4)()
    views, out = (ms.Image * 2)(), (ms.Image * 1)()
    for rc in (lib.ms_stitch_nv12_i420(None, 1, views, out, None), lib.ms_gain_stats_nv12(None, views, 1, n, s, None),
               lib.ms_track_gains_nv12(None, views, C.byref(prm), None)):
        assert rc == MS_ERR_INVALID
        assert b"null context" in lib.ms_last_error()


def test_null_image_is_invalid(ms):
    lib = ms.load()
    one = (ms.Image * 1)()          # data == NULL
    dst = (ms.Image * 1)(ms.Image(1, 48, 16, 8, ms.MS_8UC3))
    for rc in (lib.ms_nv12_resize_linear_batch(None, dst, 1, C.c_double(0), C.c_double(0), None),
               lib.ms_nv12_resize_linear_batch(one, None, 1, C.c_double(0), C.c_double(0), None),
               lib.ms_nv12_resize_linear_batch(one, dst, 1, C.c_double(0), C.c_double(0), None),
               lib.ms_nv12_resize_linear_batch(one, dst, 0, C.c_double(0), C.c_double(0), None)):
        assert rc == MS_ERR_INVALID
        assert b"ms_nv12_resize_linear_batch" in lib.ms_last_error()
    assert lib.ms_stitch_nv12_i420(None, 1, one, None, None) == MS_ERR_INVALID
    assert b"null" in lib.ms_last_error()


def test_without_a_device_the_per_op_call_says_so(ms):
    if ms.device_count() > 0:
        return                      # (on a GPU box tests/test_nv12_path_gpu.py runs the call)
    lib = ms.load()
    src = (ms.Image * 1)(ms.Image(4096, 32, 32, 24, ms.MS_8UC1))        # never dereferenced: the device check comes first
    dst = (ms.Image * 1)(ms.Image(8192, 72, 24, 12, ms.MS_8UC3))
    assert lib.ms_nv12_resize_linear_batch(src, dst, 1, C.c_double(0), C.c_double(0), None) == MS_ERR_NO_DEVICE
    assert b"no HIP device" in lib.ms_last_error()
