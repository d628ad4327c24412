"""Camera dropout at the C-ABI: ms_set_active_views / ms_get_active_views are declared, exported and listed, and refuse a null context without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_set_active_views", "ms_get_active_views")


def test_declared_exported_and_listed(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in ms_stitch.h" % n
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
        assert n in ms.EXPORTS


def test_null_context_is_invalid(ms):
    lib = ms.load()
    assert lib.ms_set_active_views(None, C.c_uint(1), None) == -1       # MS_ERR_INVALID
    assert b"null context" in lib.ms_last_error()
    m = C.c_uint(0)
    assert lib.ms_get_active_views(None, C.byref(m)) == -1
