"""ms_orb_detect_and_compute_batch without a device: the name is declared, exported and bound; every argument error is MS_ERR_INVALID with a message that
names the call and, where a view is at fault, the view -- BEFORE the library looks for a device; valid arguments then need one."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ms_orb_detect_and_compute_batch"
INVALID, NO_DEVICE = -1, -4
N, CAP = 3, 40


def test_name_is_declared_exported_and_bound(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    assert re.search(r"MS_API\s+int\s+%s\s*\(" % NAME, text), "%s is not declared" % NAME
    assert hasattr(ms.load(), NAME), "%s is not exported" % NAME
    assert NAME in ms.EXPORTS and callable(ms.orb_detect_and_compute_batch)


class _Call:
    """A valid call over three views of different sizes, the middle one masked.  The pointers are made-up addresses that nothing may follow: the checks
    come before the device, and without a device the call ends there.  Edit, then run."""

    def __init__(self, ms):
        self.ms = ms
        sizes = [(96, 80), (120, 90), (64, 70)]
        self.gray = (ms.Image * N)(*[ms.Image(0x10000000 + 0x100000 * v, w, w, h, ms.MS_8UC1) for v, (w, h) in enumerate(sizes)])
        self.masks = (ms.Image * N)(ms.Image(), ms.Image(0x20000000, 120, 120, 90, ms.MS_8UC1), ms.Image())
        self.desc = (ms.Image * N)(*[ms.Image(0x30000000 + 0x10000 * v, 32, 32, CAP, ms.MS_8UC1) for v in range(N)])
        self.prm = ms.orb_params(nfeatures=CAP - 4)
        self.kp = np.full((N, CAP, 6), 7, np.float32)
        self.cnt = np.full(N, -3, np.int32)
        self.args = dict(n=N, gray=self.gray, masks=self.masks, prm=C.byref(self.prm), kp=self.kp.ctypes.data_as(C.POINTER(C.c_float)), cap=CAP, desc=self.desc,
                         cnt=self.cnt.ctypes.data_as(C.POINTER(C.c_int)))

    def run(self):
        a = self.args
        lib = self.ms.load()
        rc = getattr(lib, NAME)(a["n"], a["gray"], a["masks"], a["prm"], a["kp"], a["cap"], a["desc"], a["cnt"], None)
        return rc, lib.ms_last_error().decode()

    def untouched(self):
        return (self.kp == 7).all() and (self.cnt == -3).all()


def _refusals(ms):
    """(name, edit(call), the words the message must hold)"""
    def arg(k, v):
        return lambda c: c.args.__setitem__(k, v)

    def field(arr, v, name, value):
        return lambda c: setattr(getattr(c, arr)[v], name, value)

    def prm(name, value):
        return lambda c: setattr(c.prm, name, value)

    def overlap(c):
        c.desc[2].data = c.desc[0].data + 32 * (CAP - 1)          # the first row of view 2 is the last row of view 0

    def overlap_by_step(c):
        c.desc[0].step = 0x10000 // (CAP - 1) + 64                # a pitch that carries view 0's last row into view 1's matrix

    return [
        ("n_views 0", arg("n", 0), ["n_views"]), ("n_views 17", arg("n", 17), ["n_views"]),
        ("n_views negative", arg("n", -2), ["n_views"]),
        ("null gray", arg("gray", None), ["gray"]), ("null prm", arg("prm", None), ["prm"]), ("null keypoints", arg("kp", None), ["keypoints_host"]),
        ("null descriptors", arg("desc", None), ["descriptors"]), ("null counts", arg("cnt", None), ["n_keypoints"]),
        ("first_level", prm("first_level", 1), ["first_level"]), ("patch_size", prm("patch_size", 15), ["patch_size"]), ("nlevels 0", prm("nlevels", 0), ["levels"]),
        ("nlevels 17", prm("nlevels", 17), ["levels"]), ("nfeatures 0", prm("nfeatures", 0), ["levels"]), ("scale_factor 1", prm("scale_factor", 1.0), ["levels"]),
        ("edge_threshold 18", prm("edge_threshold", 18), ["edge_threshold"]), ("fast_threshold 0", prm("fast_threshold", 0), ["fast_threshold"]),
        ("fast_threshold 255", prm("fast_threshold", 255), ["fast_threshold"]),
        ("max_keypoints below nfeatures", arg("cap", CAP - 5), ["max_keypoints"]),
        ("view 1 has no data", field("gray", 1, "data", None), ["view 1", "gray"]), ("view 2 is 8UC3", field("gray", 2, "type", ms.MS_8UC3), ["view 2", "gray"]),
        ("view 0 too wide", field("gray", 0, "cols", 40000), ["view 0"]), ("view 2 negative rows", field("gray", 2, "rows", -1), ["view 2"]),
        ("mask 1 of another width", field("masks", 1, "cols", 119), ["view 1", "mask"]), ("mask 1 of another height", field("masks", 1, "rows", 91), ["view 1", "mask"]),
        ("mask 1 of another type", field("masks", 1, "type", ms.MS_8UC3), ["view 1", "mask"]),
        ("descriptors 2 have no data", field("desc", 2, "data", None), ["view 2", "descriptors"]), ("descriptors 0 are 31 wide", field("desc", 0, "cols", 31), ["view 0", "descriptors"]),
        ("descriptors 1 are short", field("desc", 1, "rows", CAP - 1), ["view 1", "descriptors"]), ("descriptors 1 are 16S", field("desc", 1, "type", ms.MS_16SC1), ["view 1", "descriptors"]),
        ("descriptors 2 have a step below a row", field("desc", 2, "step", 16), ["view 2", "descriptors"]),
        ("descriptors 2 overlap 0", overlap, ["view 2", "overlap", "view 0"]), ("descriptors 0 reach into 1 by their step", overlap_by_step, ["view 1", "overlap", "view 0"]),
    ]


def test_every_refusal_comes_before_the_device(ms):
    seen = 0
    for name, edit, words in _refusals(ms):
        c = _Call(ms)
        edit(c)
        rc, msg = c.run()
        assert rc == INVALID, "%s: status %d (%s)" % (name, rc, msg)
        assert NAME in msg and all(w in msg for w in words), "%s: message %r lacks one of %r" % (name, msg, words)
        assert c.untouched(), "%s: an output was written" % name
        seen += 1
    assert seen == 32


def test_valid_arguments_need_a_device(ms):
    """(with a device the made-up pointers must not be followed: the call is made only where there is none; tests/test_orb_batch_gpu.py runs it for real)"""
    if ms.load().ms_device_count() > 0:
        return
    c = _Call(ms)
    rc, msg = c.run()
    assert rc == NO_DEVICE, (rc, msg)
    assert c.untouched()
    c = _Call(ms)          # no masks at all, one view: still no device
    c.args["masks"] = None
    c.args["n"] = 1
    assert c.run()[0] == NO_DEVICE
