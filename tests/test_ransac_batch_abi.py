"""ms_find_homography_ransac_batch without a device: the name is declared, exported and listed; every argument error is MS_ERR_INVALID with a message that names
the argument, BEFORE the library looks for a device; an empty batch is MS_OK and touches nothing."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ms_find_homography_ransac_batch"
OK, INVALID, NO_DEVICE = 0, -1, -4


def test_name_is_declared_exported_and_listed(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    assert re.search(r"MS_API\s+int\s+%s\s*\(" % NAME, text), "%s is not declared" % NAME
    assert hasattr(ms.load(), NAME), "%s is not exported" % NAME
    assert NAME in ms.EXPORTS and callable(ms.find_homography_ransac_batch)


class _Call:
    """A valid call over two problems of 5 and 3 points; edit, then run"""

    def __init__(self):
        self.off = np.array([0, 5, 8], np.int32)
        self.src = np.arange(16, dtype=np.float32)
        self.dst = np.arange(16, dtype=np.float32) * 2
        self.H = np.full(18, 7.0)
        self.mask = np.full(8, 9, np.uint8)
        self.cnt = np.full(2, -3, np.int32)
        self.status = np.full(2, -3, np.int32)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        self.args = dict(n=2, off=self.off.ctypes.data_as(ip), src=self.src.ctypes.data_as(fp), dst=self.dst.ctypes.data_as(fp), thr=3.0, iters=2000, conf=0.995,
                         H=self.H.ctypes.data_as(C.POINTER(C.c_double)), mask=self.mask.ctypes.data_as(C.POINTER(C.c_uint8)), cnt=self.cnt.ctypes.data_as(ip),
                         status=self.status.ctypes.data_as(ip))

    def run(self, ms):
        a = self.args
        lib = ms.load()
        rc = getattr(lib, NAME)(a["n"], a["off"], a["src"], a["dst"], C.c_double(a["thr"]), a["iters"], C.c_double(a["conf"]), a["H"], a["mask"], a["cnt"], a["status"], None)
        return rc, lib.ms_last_error().decode()

    def untouched(self):
        return (self.H == 7.0).all() and (self.mask == 9).all() and (self.cnt == -3).all() and (self.status == -3).all()


def _refusals():
    """(name, edit(call), the word the message must hold)"""
    def arg(k, v):
        return lambda c: c.args.__setitem__(k, v)

    def offsets(*v):
        return lambda c: c.off.__setitem__(slice(None), v)

    return [
        ("null offsets", arg("off", None), "offsets"), ("null H", arg("H", None), "H"), ("null status", arg("status", None), "status"),
        ("null src_xy", arg("src", None), "src_xy"), ("null dst_xy", arg("dst", None), "dst_xy"),
        ("n_problems negative", arg("n", -1), "n_problems"),
        ("offsets[0] not 0", offsets(1, 5, 8), "offsets[0]"), ("offsets descend", offsets(0, 5, 4), "offsets"), ("offsets descend at once", offsets(0, -1, 8), "offsets"),
        ("threshold nan", arg("thr", float("nan")), "reproj_threshold"), ("threshold inf", arg("thr", float("inf")), "reproj_threshold"),
        ("confidence nan", arg("conf", float("nan")), "confidence"), ("confidence -inf", arg("conf", float("-inf")), "confidence"),
    ]


def test_every_refusal_comes_before_the_device(ms):
    seen = 0
    for name, edit, word in _refusals():
        c = _Call()
        edit(c)
        rc, msg = c.run(ms)
        assert rc == INVALID, "%s: status %d (%s)" % (name, rc, msg)
        assert NAME in msg and word in msg, "%s: message %r lacks %r" % (name, msg, word)
        assert c.untouched(), "%s: an output was written" % name
        seen += 1
    assert seen == 13


def test_an_empty_batch_is_ok_and_touches_nothing(ms):
    c = _Call()
    c.args["n"] = 0
    rc, _ = c.run(ms)
    assert rc == OK and c.untouched()
    for k in ("off", "src", "dst", "H", "mask", "cnt", "status"):      # nothing is read either
        c.args[k] = None
    assert c.run(ms)[0] == OK
    assert ms.find_homography_ransac_batch([]) == []


def test_valid_arguments_need_a_device(ms):
    c = _Call()
    rc, msg = c.run(ms)
    if ms.load().ms_device_count() > 0:
        assert rc == OK and c.status.tolist() == [1, 1], msg      # 5 collinear points, then 3 points: neither has a model
        assert not c.H.any() and not c.mask.any() and not c.cnt.any()
        return
    assert rc == NO_DEVICE, (rc, msg)
    c = _Call()          # null points are fine where the batch holds none: still no device
    c.off[:] = 0
    c.args["src"] = c.args["dst"] = None
    assert c.run(ms)[0] == NO_DEVICE
