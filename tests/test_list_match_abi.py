"""ms_match_lists / ms_feature_inputs_batch without a device: names and layouts, the default parameters, every refusal (all of them come before the device is
touched), the empty problem list, the numpy reference's own ratio edges, and the host-only check of MeshWarper::filterTemporalMatches (tests/shim_temporal_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import list_match_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ms_list_match_default_params", "ms_match_lists", "ms_feature_inputs_batch"]
INVALID, NO_DEVICE = -1, -4


# ---------------------------------------------------------------------------------------------------------------- names and layout

def test_names_are_declared_exported_and_listed(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared" % n
        assert hasattr(lib, n), "%s is not exported" % n
        assert n in ms.EXPORTS
    for n in ("match_lists", "list_match_default_params", "feature_inputs_batch"):
        assert callable(getattr(ms, n))


def test_struct_layouts_equal_the_headers(ms, tmp_path):
    fields = {"ms_match_problem": ["query_set", "train_set"],
              "ms_list_match_params": ["struct_size", "ratio", "find_homography", "ransac_reproj_threshold", "ransac_max_iters", "ransac_confidence"]}
    classes = {"ms_match_problem": ms.MatchProblem, "ms_list_match_params": ms.ListMatchParams}
    exprs = ["MS_MATCH_MAX_PROBLEMS", "MS_MAX_VIEWS"]
    for s, fs in fields.items():
        exprs.append("sizeof(%s)" % s)
        exprs += ["offsetof(%s, %s)" % (s, f) for f in fs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ms_stitch.h"\nint main(void) { printf("' + " ".join(["%zu"] * len(exprs)) + '\\n", '
                   + ", ".join("(size_t)(%s)" % e for e in exprs) + "); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
    want = [ms.MATCH_MAX_PROBLEMS, 16]
    for s, fs in fields.items():
        cls = classes[s]
        assert [f for f, _ in cls._fields_] == fs
        want.append(C.sizeof(cls))
        want += [getattr(cls, f).offset for f in fs]
    assert got == want
    assert got[0] == 64 and C.sizeof(ms.MatchProblem) == 8 and C.sizeof(ms.ListMatchParams) == 48


def test_default_params(ms):
    p = ms.list_match_default_params()
    assert p.struct_size == C.sizeof(ms.ListMatchParams)
    assert p.ratio == 0.7 and p.find_homography == 1
    assert p.ransac_reproj_threshold == 0.0 and p.ransac_max_iters == 0 and p.ransac_confidence == 0.0
    assert ms.load().ms_list_match_default_params(None) == INVALID and b"ms_list_match_default_params" in ms.load().ms_last_error()


# ---------------------------------------------------------------------------------------------------------------- ms_match_lists refusals

class _Call:
    """A valid ms_match_lists call over host memory only (the descriptor pointers are never followed before the device check); edit, then run"""

    def __init__(self, ms, n=3, nkp=5, with_rows=True):
        self.ms, self.n = ms, n
        self.kp = [np.zeros((max(nkp, 1), 6), np.float32) for _ in range(n)]
        self.sets = (ms.ViewFeatures * 40)()
        for v in range(n):
            im = ms.Image(0x1000 if with_rows else None, 32, 32, 8 if with_rows else 0, ms.MS_8UC1)
            self.sets[v] = ms.ViewFeatures(im, self.kp[v].ctypes.data_as(C.POINTER(C.c_float)), 6, nkp if with_rows else 0, 640, 480)
        self.problems = (ms.MatchProblem * 80)()
        for p, (q, t) in enumerate(((0, 1), (1, 2), (2, 0), (1, 1))):
            self.problems[p] = ms.MatchProblem(q, t)
        self.prm = ms.list_match_default_params()
        self.out = (ms.PairMatches * 80)()
        self.matches = (ms.FeatureMatch * 64)()
        self.n_matches = C.c_int(-7)
        self.args = dict(n_sets=n, sets=self.sets, n_problems=4, problems=self.problems, prm=C.byref(self.prm), out=self.out, matches=self.matches, matches_cap=64,
                         n_matches=C.byref(self.n_matches))

    def run(self):
        a = self.args
        lib = self.ms.load()
        rc = lib.ms_match_lists(a["n_sets"], a["sets"], a["n_problems"], a["problems"], a["prm"], a["out"], a["matches"], a["matches_cap"], a["n_matches"], None)
        return rc, lib.ms_last_error().decode()


def _refusals(ms):
    """(name, edit(call), a word the message must hold)"""
    def arg(k, v):
        return lambda c: c.args.__setitem__(k, v)

    def prm(k, v):
        return lambda c: setattr(c.prm, k, v)

    def sset(v, k, val):
        return lambda c: setattr(c.sets[v], k, val)

    def desc(v, k, val):
        return lambda c: setattr(c.sets[v].descriptors, k, val)

    def prob(p, k, val):
        return lambda c: setattr(c.problems[p], k, val)

    def mixed_lengths(c):
        c.sets[2].descriptors.cols = 64; c.sets[2].descriptors.step = 64

    return [
        ("null sets", arg("sets", None), "null"), ("null problems", arg("problems", None), "null"), ("null params", arg("prm", None), "null"),
        ("null out", arg("out", None), "null"), ("null matches_out", arg("matches", None), "null"), ("null n_matches", arg("n_matches", None), "null"),
        ("no set", arg("n_sets", 0), "n_sets"), ("too many sets", arg("n_sets", 33), "n_sets"),
        ("negative n_problems", arg("n_problems", -1), "n_problems"), ("too many problems", arg("n_problems", 65), "n_problems"),
        ("query_set negative", prob(1, "query_set", -1), "query_set"), ("query_set out of range", prob(3, "query_set", 3), "query_set"),
        ("train_set negative", prob(0, "train_set", -1), "train_set"), ("train_set out of range", prob(2, "train_set", 3), "train_set"),
        ("struct_size", prm("struct_size", C.sizeof(ms.ListMatchParams) - 8), "struct_size"),
        ("ratio 0", prm("ratio", 0.0), "ratio"), ("ratio negative", prm("ratio", -0.5), "ratio"), ("ratio above 1", prm("ratio", 1.0000001), "ratio"),
        ("ratio nan", prm("ratio", float("nan")), "ratio"), ("ratio inf", prm("ratio", float("inf")), "ratio"),
        ("ransac threshold negative", prm("ransac_reproj_threshold", -1.0), "ransac_reproj_threshold"), ("ransac threshold nan", prm("ransac_reproj_threshold", float("nan")), "ransac_reproj_threshold"),
        ("ransac iterations negative", prm("ransac_max_iters", -1), "ransac_max_iters"), ("ransac confidence 1", prm("ransac_confidence", 1.0), "ransac_confidence"),
        ("ransac confidence negative", prm("ransac_confidence", -0.1), "ransac_confidence"),
        ("descriptor type", desc(1, "type", ms.MS_8UC3), "type"), ("descriptor length 0", desc(1, "cols", 0), "length"),
        ("descriptor length 30", desc(1, "cols", 30), "length"), ("descriptor length 68", desc(1, "cols", 68), "length"),
        ("descriptor step", desc(1, "step", 34), "step"), ("descriptor lengths differ", mixed_lengths, "differs"),
        ("n_keypoints negative", sset(1, "n_keypoints", -1), "n_keypoints"), ("n_keypoints above rows", sset(1, "n_keypoints", 9), "n_keypoints"),
        ("n_keypoints above the limit", lambda c: (setattr(c.sets[1], "n_keypoints", ms.MATCH_MAX_KEYPOINTS + 1), setattr(c.sets[1].descriptors, "rows", 1 << 20)), "n_keypoints"),
        ("null keypoints", sset(1, "keypoints", C.POINTER(C.c_float)()), "keypoints"), ("null descriptors", desc(1, "data", None), "descriptors"),
        ("keypoint_stride", sset(0, "keypoint_stride", 1), "keypoint_stride"), ("width", sset(2, "width", 0), "width"), ("height", sset(2, "height", 0), "height"),
        ("matches_cap negative", arg("matches_cap", -1), "matches_cap"),
    ]


def test_every_match_lists_refusal_comes_before_the_device(ms):
    seen = []
    for name, edit, word in _refusals(ms):
        c = _Call(ms)
        edit(c)
        rc, msg = c.run()
        assert rc == INVALID, "%s: status %d (%s)" % (name, rc, msg)
        assert "ms_match_lists" in msg and word in msg, "%s: message %r lacks %r" % (name, msg, word)
        seen.append(name)
    assert len(seen) == 40
    c = _Call(ms)       # the per-set rules name the set
    c.sets[2].keypoint_stride = 1
    assert "set 2" in c.run()[1]


def test_the_limits_themselves_are_accepted(ms):
    """32 sets and 64 problems pass the argument checks: the call gets as far as the device check (or, with a device and no rows anywhere, through)"""
    lib = ms.load()
    c = _Call(ms, n=32, with_rows=False)
    for p in range(64):
        c.problems[p] = ms.MatchProblem(p % 32, 31 - p % 32)
    c.args["n_problems"] = 64
    rc, msg = c.run()
    if lib.ms_device_count() > 0:
        assert rc == 0 and c.n_matches.value == 0, msg
        assert all(c.out[p].view_a == p % 32 and c.out[p].view_b == 31 - p % 32 and c.out[p].count == 0 and c.out[p].confidence == 1.0 for p in range(64))
    else:
        assert rc == NO_DEVICE, (rc, msg)


def test_no_problems_is_ok_and_touches_nothing(ms):
    c = _Call(ms)
    c.args["n_problems"] = 0
    rc, msg = c.run()
    assert rc == 0 and c.n_matches.value == 0, (rc, msg)         # also on a machine without a device: not even the device check runs
    assert ms.match_lists([(np.zeros((0, 2), np.float32), None, (4, 4))], []) == []
    c = _Call(ms)       # ... but its arguments are still checked
    c.args["n_problems"] = 0
    c.prm.ratio = 2.0
    assert c.run()[0] == INVALID


def test_valid_arguments_need_a_device(ms):
    lib = ms.load()
    if lib.ms_device_count() > 0:       # with a device the host pointers of _Call must not be followed: sets without keypoints run through with every list empty
        c = _Call(ms, with_rows=False)
        rc, msg = c.run()
        assert rc == 0 and c.n_matches.value == 0, msg
        return
    rc, msg = _Call(ms).run()
    assert rc == NO_DEVICE, (rc, msg)


# ---------------------------------------------------------------------------------------------------------------- the reference checks itself

def test_reference_ratio_rule_is_the_integer_rule_at_0_7():
    d0, d1 = np.meshgrid(np.arange(513), np.arange(513), indexing="ij")
    assert np.array_equal(LR.ratio_pass(d0, d1, 0.7), 10 * d0 < 7 * d1)
    for a, b in ((7, 10), (14, 20), (21, 30), (0, 0), (5, 5)):
        assert not LR.ratio_pass(a, b)
    assert LR.ratio_pass(6, 10) and LR.ratio_pass(0, 1)
    assert LR.ratio_pass(9, 10, 1.0) and not LR.ratio_pass(10, 10, 1.0) and not LR.ratio_pass(5, 10, 0.5) and LR.ratio_pass(4, 10, 0.5)


def test_reference_lists():
    rng = np.random.default_rng(2)
    A = rng.integers(0, 256, (9, 4), dtype=np.uint8)
    B = np.concatenate([A[[3, 0]], rng.integers(0, 256, (5, 4), dtype=np.uint8)])
    rows = LR.problem_list(A, B)
    assert [0, 1, 0] in rows.tolist() and [3, 0, 0] in rows.tolist() and np.all(np.diff(rows[:, 0]) > 0)
    assert len(LR.problem_list(A[:0], B)) == 0 and len(LR.problem_list(A, B[:1])) == 0
    recs, lists = LR.match_lists([A, B], [(0, 1), (1, 1), (0, 1)])
    assert recs[0][3] == recs[2][3] and recs[2][2] == recs[0][3] + recs[1][3] and np.array_equal(lists[0], lists[2])
    assert lists[1][:, 0].tolist() == lists[1][:, 1].tolist() and np.all(lists[1][:, 2] == 0)      # a set against itself: every row finds itself, unless a duplicate ties


# ---------------------------------------------------------------------------------------------------------------- ms_feature_inputs_batch refusals

class _Inputs:
    """A valid ms_feature_inputs_batch call over made-up device addresses (never followed before the device check)"""

    def __init__(self, ms, n=3):
        self.ms = ms
        sizes = [(40, 30), (67, 5), (16, 16)][:n]
        self.views = (ms.Image * 17)(); self.gray = (ms.Image * 17)(); self.masks = (ms.Image * 17)()
        for v, (w, h) in enumerate(sizes):
            self.views[v] = ms.Image(0x10000, w * 3 + 4, w, h, ms.MS_8UC3)
            self.gray[v] = ms.Image(0x20000, w + 3, w, h, ms.MS_8UC1)
            self.masks[v] = ms.Image(0x30000, w, w, h, ms.MS_8UC1)
        self.bands = (C.c_int * (4 * 17))(*([0, 8, 20, 8] * 17))
        self.args = dict(n=n, views=self.views, bands=self.bands, gray=self.gray, masks=self.masks)

    def run(self):
        a = self.args
        lib = self.ms.load()
        rc = lib.ms_feature_inputs_batch(a["n"], a["views"], a["bands"], a["gray"], a["masks"], None)
        return rc, lib.ms_last_error().decode()


def test_every_feature_inputs_refusal_comes_before_the_device(ms):
    def arg(k, v):
        return lambda c: c.args.__setitem__(k, v)

    def f(arr, v, k, val):
        return lambda c: setattr(getattr(c, arr)[v], k, val)

    def both_null(c):
        c.args["gray"] = None; c.args["masks"] = None

    cases = [
        ("no view", arg("n", 0), "n_views"), ("too many views", arg("n", 17), "n_views"), ("null views", arg("views", None), "warped_views"),
        ("no output", both_null, "both null"), ("masks without bands", arg("bands", None), "bands"),
        ("view without data", f("views", 1, "data", None), "view 1"), ("view without rows", f("views", 2, "rows", 0), "view 2"), ("view without columns", f("views", 0, "cols", 0), "view 0"),
        ("view type", f("views", 1, "type", ms.MS_8UC1), "view 1"), ("view step", f("views", 1, "step", 67 * 3 - 1), "view 1"),
        ("gray without data", f("gray", 2, "data", None), "gray"), ("gray type", f("gray", 0, "type", ms.MS_8UC3), "gray"), ("gray width", f("gray", 1, "cols", 66), "gray"),
        ("gray height", f("gray", 1, "rows", 6), "gray"), ("gray step", f("gray", 1, "step", 66), "gray"),
        ("mask without data", f("masks", 0, "data", None), "mask"), ("mask type", f("masks", 2, "type", ms.MS_8UC3), "mask"), ("mask width", f("masks", 1, "cols", 68), "mask"),
        ("mask height", f("masks", 2, "rows", 15), "mask"), ("mask step", f("masks", 0, "step", 39), "mask"),
    ]
    for name, edit, word in cases:
        c = _Inputs(ms)
        edit(c)
        rc, msg = c.run()
        assert rc == INVALID, "%s: status %d (%s)" % (name, rc, msg)
        assert "ms_feature_inputs_batch" in msg and word in msg, "%s: message %r lacks %r" % (name, msg, word)
    c = _Inputs(ms)
    c.gray[1].step = 66
    assert "view 1" in c.run()[1]
    if ms.load().ms_device_count() == 0:        # valid forms get as far as the device check: both outputs, grey alone (bands not needed), masks alone
        for edit in (lambda c: None, lambda c: (arg("masks", None)(c), arg("bands", None)(c)), arg("gray", None)):
            c = _Inputs(ms)
            edit(c)
            assert c.run()[0] == NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------- MeshWarper::filterTemporalMatches

def test_shim_filter_temporal_matches(tmp_path):
    exe = str(tmp_path / "shim_temporal")
    pkg = os.path.join(ROOT, "video-stitcher_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_temporal_check.cpp"),
                           "-L" + pkg, "-lmsstitch", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
