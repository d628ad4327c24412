"""ms_match_pairs / ms_biggest_component / ms_wave_correct without a device: names and layouts, every refusal of ms_match_pairs (all of them come before the device is
touched), the numpy reference's own checks (tests/pair_match_ref.py), and the two host-only steps against it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pair_match_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ms_pair_match_default_params", "ms_match_pairs", "ms_biggest_component", "ms_wave_correct"]
INVALID, NO_DEVICE = -1, -4


# ---------------------------------------------------------------------------------------------------------------- names and layout

def test_names_are_declared_exported_and_listed(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared" % n
        assert hasattr(lib, n), "%s is not exported" % n
        assert n in ms.EXPORTS
    for n in ("match_pairs", "biggest_component", "wave_correct", "pairs_for_estimate_rig", "pair_match_default_params"):
        assert callable(getattr(ms, n))


def test_struct_layouts_equal_the_headers(ms, tmp_path):
    fields = {"ms_view_features": ["descriptors", "keypoints", "keypoint_stride", "n_keypoints", "width", "height"],
              "ms_pair_match_params": ["struct_size", "match_conf", "num_matches_thresh1", "num_matches_thresh2", "range_width", "pair_mask", "ransac_reproj_threshold",
                                       "ransac_max_iters", "ransac_confidence"],
              "ms_feature_match": ["query", "train", "distance", "inlier"],
              "ms_pair_matches": ["view_a", "view_b", "first", "count", "n_forward", "num_inliers", "have_H", "H", "confidence"]}
    classes = {"ms_view_features": ms.ViewFeatures, "ms_pair_match_params": ms.PairMatchParams, "ms_feature_match": ms.FeatureMatch, "ms_pair_matches": ms.PairMatches}
    exprs = ["MS_MATCH_MAX_KEYPOINTS", "MS_WAVE_HORIZ", "MS_WAVE_VERT", "MS_MAX_VIEWS"]
    for s, fs in fields.items():
        exprs.append("sizeof(%s)" % s)
        exprs += ["offsetof(%s, %s)" % (s, f) for f in fs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ms_stitch.h"\nint main(void) { printf("' + " ".join(["%zu"] * len(exprs)) + '\\n", '
                   + ", ".join("(size_t)(%s)" % e for e in exprs) + "); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
    want = [ms.MATCH_MAX_KEYPOINTS, ms.WAVE_HORIZ, ms.WAVE_VERT, 16]
    for s, fs in fields.items():
        cls = classes[s]
        assert [f for f, _ in cls._fields_] == fs
        want.append(C.sizeof(cls))
        want += [getattr(cls, f).offset for f in fs]
    assert got == want
    assert got[0] == 32768 and C.sizeof(ms.FeatureMatch) == 16 and C.sizeof(ms.PairMatches) == 28 + 4 + 72 + 8


def test_default_params(ms):
    p = ms.pair_match_default_params()
    assert p.struct_size == C.sizeof(ms.PairMatchParams)
    assert p.match_conf == np.float32(0.3) and p.num_matches_thresh1 == 6 and p.num_matches_thresh2 == 6 and p.range_width == 0
    assert not p.pair_mask and p.ransac_reproj_threshold == 0.0 and p.ransac_max_iters == 0 and p.ransac_confidence == 0.0
    assert ms.load().ms_pair_match_default_params(None) == INVALID and b"ms_pair_match_default_params" in ms.load().ms_last_error()


# ---------------------------------------------------------------------------------------------------------------- refusals

class _Call:
    """A valid ms_match_pairs call over host memory only (the descriptor pointers are never followed before the device check); edit, then run"""

    def __init__(self, ms, n=3, nkp=5, with_rows=True):
        self.ms, self.n = ms, n
        self.kp = [np.zeros((max(nkp, 1), 6), np.float32) for _ in range(n)]
        self.views = (ms.ViewFeatures * n)()
        for v in range(n):
            im = ms.Image(0x1000 if with_rows else None, 32, 32, 8 if with_rows else 0, ms.MS_8UC1)
            self.views[v] = ms.ViewFeatures(im, self.kp[v].ctypes.data_as(C.POINTER(C.c_float)), 6, nkp if with_rows else 0, 640, 480)
        self.prm = ms.pair_match_default_params()
        self.pairs = (ms.PairMatches * 16)()
        self.matches = (ms.FeatureMatch * 64)()
        self.n_pairs, self.n_matches = C.c_int(-7), C.c_int(-7)
        self.args = dict(n_views=n, views=self.views, prm=C.byref(self.prm), pairs=self.pairs, pairs_cap=16, n_pairs=C.byref(self.n_pairs), matches=self.matches,
                         matches_cap=64, n_matches=C.byref(self.n_matches))

    def run(self):
        a = self.args
        lib = self.ms.load()
        rc = lib.ms_match_pairs(a["n_views"], a["views"], a["prm"], a["pairs"], a["pairs_cap"], a["n_pairs"], a["matches"], a["matches_cap"], a["n_matches"], None)
        return rc, lib.ms_last_error().decode()


def _refusals(ms):
    """(name, edit(call), a word the message must hold)"""
    def arg(k, v):
        return lambda c: c.args.__setitem__(k, v)

    def prm(k, v):
        return lambda c: setattr(c.prm, k, v)

    def view(v, k, val):
        return lambda c: setattr(c.views[v], k, val)

    def desc(v, k, val):
        return lambda c: setattr(c.views[v].descriptors, k, val)

    def mixed_lengths(c):
        c.views[2].descriptors.cols = 64; c.views[2].descriptors.step = 64

    return [
        ("null views", arg("views", None), "null"), ("null params", arg("prm", None), "null"), ("null pairs_out", arg("pairs", None), "null"),
        ("null n_pairs", arg("n_pairs", None), "null"), ("null matches_out", arg("matches", None), "null"), ("null n_matches", arg("n_matches", None), "null"),
        ("one view", arg("n_views", 1), "n_views"), ("too many views", arg("n_views", 17), "n_views"),
        ("struct_size", prm("struct_size", C.sizeof(ms.PairMatchParams) - 8), "struct_size"),
        ("match_conf 1", prm("match_conf", 1.0), "match_conf"), ("match_conf negative", prm("match_conf", -0.01), "match_conf"),
        ("match_conf nan", prm("match_conf", float("nan")), "match_conf"), ("match_conf inf", prm("match_conf", float("inf")), "match_conf"),
        ("thresh1 negative", prm("num_matches_thresh1", -1), "num_matches_thresh1"), ("thresh2 negative", prm("num_matches_thresh2", -1), "num_matches_thresh2"),
        ("range_width negative", prm("range_width", -1), "range_width"),
        ("descriptor type", desc(1, "type", ms.MS_8UC3), "type"), ("descriptor length 0", desc(1, "cols", 0), "length"),
        ("descriptor length 30", desc(1, "cols", 30), "length"), ("descriptor length 68", desc(1, "cols", 68), "length"),
        ("descriptor step", desc(1, "step", 34), "step"), ("descriptor lengths differ", mixed_lengths, "differs"),
        ("n_keypoints negative", view(1, "n_keypoints", -1), "n_keypoints"), ("n_keypoints above rows", view(1, "n_keypoints", 9), "n_keypoints"),
        ("n_keypoints above the limit", lambda c: (setattr(c.views[1], "n_keypoints", ms.MATCH_MAX_KEYPOINTS + 1), setattr(c.views[1].descriptors, "rows", 1 << 20)), "n_keypoints"),
        ("null keypoints", view(1, "keypoints", C.POINTER(C.c_float)()), "keypoints"), ("null descriptors", desc(1, "data", None), "descriptors"),
        ("keypoint_stride", view(0, "keypoint_stride", 1), "keypoint_stride"), ("width", view(2, "width", 0), "width"), ("height", view(2, "height", 0), "height"),
        ("pairs_cap", arg("pairs_cap", 2), "pairs_cap"),
    ]


def test_every_refusal_comes_before_the_device(ms):
    seen = []
    for name, edit, word in _refusals(ms):
        c = _Call(ms)
        edit(c)
        rc, msg = c.run()
        assert rc == INVALID, "%s: status %d (%s)" % (name, rc, msg)
        assert "ms_match_pairs" in msg and word in msg, "%s: message %r lacks %r" % (name, msg, word)
        seen.append(name)
    assert len(seen) == 31


def test_valid_arguments_need_a_device(ms):
    lib = ms.load()
    if lib.ms_device_count() > 0:       # with a device the host pointers of _Call must not be followed: views without keypoints run through and list every pair empty
        c = _Call(ms, with_rows=False)
        rc, msg = c.run()
        assert rc == 0 and c.n_pairs.value == 3 and c.n_matches.value == 0, msg
        return
    c = _Call(ms)
    rc, msg = c.run()
    assert rc == NO_DEVICE, (rc, msg)
    c = _Call(ms)
    c.prm.range_width = 2       # 2 candidate pairs: a pairs_cap of 2 is enough
    c.args["pairs_cap"] = 2
    assert c.run()[0] == NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------- the reference checks itself

def test_reference_knn_against_unpackbits_and_a_stable_sort():
    rng = np.random.default_rng(5)
    for nq, nt, nb in ((40, 57, 32), (9, 2, 4), (33, 70, 64)):
        Q = rng.integers(0, 256, (nq, nb), dtype=np.uint8); T = rng.integers(0, 256, (nt, nb), dtype=np.uint8)
        T[nt // 2] = T[0]; Q[1] = T[0]; Q[2] = T[1]         # ties in the distance, an exact duplicate
        idx, dist = PR.knn2(Q, T)
        D = np.unpackbits(Q[:, None, :] ^ T[None, :, :], axis=2).sum(axis=2)
        order = np.argsort(D, axis=1, kind="stable")[:, :2]
        assert np.array_equal(idx, order) and np.array_equal(dist, np.take_along_axis(D, order, axis=1))
        assert idx[1, 0] == 0 and idx[1, 1] == nt // 2 and dist[1, 0] == 0 and dist[1, 1] == 0      # equal distances: the lower index first


def test_reference_ratio_edges():
    mc = np.float32(0.3)
    assert np.float32(np.float32(1.0) - mc) * np.float32(10.0) == np.float32(7.0)       # 0.69999999f * 10.f rounds to 7.f
    for d0, d1 in ((7, 10), (14, 20), (21, 30)):
        assert not PR.ratio_pass(d0, d1, mc), (d0, d1)
    assert PR.ratio_pass(6, 10, mc)
    assert not PR.ratio_pass(0, 0, mc)
    assert PR.ratio_pass(0, 1, mc)


def test_reference_list_order_and_cross_check():
    """a's rows 0, 1 match b's rows 1, 0 both ways (the backward copies are dropped); b's row 2 matches a's row 2 in the backward direction only"""
    z = np.zeros(4, np.uint8)
    def row(*bits):
        r = z.copy()
        for b in bits:
            r[b // 8] |= 1 << (b % 8)
        return r
    A = np.stack([row(0), row(8, 9), row(16, 17, 18, 19, 20, 21), row(*range(24, 32))])
    B = np.stack([row(8, 9), row(0), row(16, 17, 18, 19, 20, 21, 22)])
    rows, nf = PR.pair_list(A, B, 0.3)
    # forward: a0 -> b1 (d 0, second 3), a1 -> b0 (0, 3), a2 -> b2 (1, 7), a3: 9 / 10 fails; backward: b0 -> a1 and b1 -> a0 duplicates, b2 -> a2 duplicate as well
    assert nf == 3 and rows.tolist() == [[0, 1, 0], [1, 0, 0], [2, 2, 1]]
    # make a2 fail forward (its two nearest equally far) while b2 -> a2 still passes backward
    B2 = np.stack([row(8, 9), row(0), row(16, 17, 18, 19, 20, 21, 22), row(16, 17, 18, 19, 20, 21, 23)])
    rows, nf = PR.pair_list(A, B2, 0.3)
    assert nf == 2 and rows.tolist() == [[0, 1, 0], [1, 0, 0], [2, 2, 1], [2, 3, 1]]
    assert PR.confidence(30, 40) == 30 / (8 + 0.3 * 40) and PR.confidence(100, 5) == 0.0


# ---------------------------------------------------------------------------------------------------------------- ms_wave_correct

def _rot(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _random_rig(rng, n):
    return np.stack([_rot(rng.normal(size=3), rng.uniform(0, np.pi)) for _ in range(n)])


def _ring(n, jitter=None, rng=None, span=2 * np.pi):
    R = np.stack([_rot([0, 1, 0], span * v / n) for v in range(n)])
    if jitter:
        R = np.stack([_rot(rng.normal(size=3), jitter * rng.normal()) @ r for r in R])
    return R


def _check_rotations(out, R):
    for v in range(len(R)):
        assert np.abs(out[v] @ out[v].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(out[v]) - 1) <= 1e-12
    G = out[0] @ R[0].T
    for v in range(1, len(R)):
        assert np.abs(out[v] @ R[v].T - G).max() <= 1e-12


def test_wave_correct_matches_the_reference_on_random_rigs(ms):
    rng = np.random.default_rng(11)
    n_cases = 0
    for n in (2, 3, 4, 6, 8, 16):
        for kind in (ms.WAVE_HORIZ, ms.WAVE_VERT):
            for make in (lambda: _random_rig(rng, n), lambda: _ring(n, 0.2, rng) if kind == ms.WAVE_HORIZ else np.stack([_rot([1, 0, 0], 0.3 * v) @ _rot(rng.normal(size=3), 0.1) for v in range(n)])):
                R = make()
                w = np.linalg.eigvalsh(R[:, :, 0].T @ R[:, :, 0])
                if (w[1] - w[0] if kind == ms.WAVE_HORIZ else w[2] - w[1]) < 0.05:       # the wanted eigenvector is ill-determined: not a case for a 1e-12 comparison
                    continue
                want, st_want = PR.wave_correct(R, kind)
                got, st = ms.wave_correct(R, kind)
                assert st == st_want == 0
                assert np.abs(got - want).max() <= 1e-12, (n, kind, np.abs(got - want).max())
                _check_rotations(got, R)
                n_cases += 1
    assert n_cases >= 16


def test_wave_correct_levels_a_tilted_ring(ms):
    rng = np.random.default_rng(3)
    for n in (3, 5, 8):
        T = _rot(rng.normal(size=3), 0.4)
        R = np.einsum("ij,vjk->vik", T, _ring(n, span=1.5 * np.pi))       # three quarters of a ring: the optical axes do not cancel, rg0 is well determined
        assert np.abs(R[:, 1, 0]).max() > 1e-3          # the tilt shows in the first columns' Y
        out, st = ms.wave_correct(R, ms.WAVE_HORIZ)
        assert st == 0 and np.abs(out[:, 1, 0]).max() <= 1e-12
        _check_rotations(out, R)


def test_wave_correct_degenerate_inputs_come_back_unchanged(ms):
    one = _rot([1, 2, 3], 0.7)[None]
    out, st = ms.wave_correct(one, ms.WAVE_HORIZ)
    assert st == 1 and np.array_equal(out, one)
    rolls = np.stack([_rot([0, 0, 1], a) for a in (0.1, 0.9, 2.0)])      # first columns in the XY plane, every third column e_z: rg1 = e_z is parallel to their sum
    out, st = ms.wave_correct(rolls, ms.WAVE_HORIZ)
    assert st == 1 and np.array_equal(out, rolls)
    assert PR.wave_correct(rolls, 0)[1] == 1


def test_wave_correct_refusals(ms):
    lib = ms.load()
    R = _ring(4)
    dp = C.POINTER(C.c_double)
    out = np.zeros_like(R)
    for kind in (-1, 2):
        assert lib.ms_wave_correct(4, R.ctypes.data_as(dp), kind, out.ctypes.data_as(dp)) == INVALID and b"kind" in lib.ms_last_error()
    assert lib.ms_wave_correct(4, None, 0, out.ctypes.data_as(dp)) == INVALID and b"null" in lib.ms_last_error()
    assert lib.ms_wave_correct(4, R.ctypes.data_as(dp), 0, None) == INVALID
    assert lib.ms_wave_correct(0, R.ctypes.data_as(dp), 0, out.ctypes.data_as(dp)) == INVALID and b"n_views" in lib.ms_last_error()
    assert lib.ms_wave_correct(17, R.ctypes.data_as(dp), 0, out.ctypes.data_as(dp)) == INVALID
    bad = R.copy(); bad[2, 1, 1] = np.nan
    assert lib.ms_wave_correct(4, bad.ctypes.data_as(dp), 0, out.ctypes.data_as(dp)) == INVALID and b"finite" in lib.ms_last_error()


# ---------------------------------------------------------------------------------------------------------------- ms_biggest_component

def _pairs(ms, recs):
    return [{"view_a": a, "view_b": b, "confidence": c} for a, b, c in recs]


@pytest.mark.parametrize("name, n, recs, thr, want", [
    ("two components of unequal size", 6, [(0, 1, 2.0), (2, 3, 1.5), (3, 5, 1.2), (0, 2, 0.4), (1, 4, 0.9)], 1.0, [2, 3, 5]),
    ("a tie goes to the component with the lowest view", 6, [(1, 5, 2.0), (0, 4, 2.0), (2, 3, 2.0)], 1.0, [0, 4]),
    ("a tie, the larger indices listed first", 4, [(2, 3, 1.0), (0, 1, 1.0)], 1.0, [0, 1]),
    ("confidence equal to the threshold joins", 3, [(0, 1, 1.0), (1, 2, 0.9999999999999999)], 1.0, [0, 1]),
    ("all views isolated", 4, [(0, 1, 0.2), (1, 2, 0.0), (2, 3, 0.99)], 1.0, [0]),
    ("no pairs at all", 3, [], 1.0, [0]),
    ("everything connected", 5, [(0, 1, 1.1), (1, 2, 1.1), (2, 3, 1.1), (3, 4, 1.1), (0, 4, 0.1)], 1.0, [0, 1, 2, 3, 4]),
])
def test_biggest_component(ms, name, n, recs, thr, want):
    assert PR.biggest_component(n, recs, thr) == want
    assert ms.biggest_component(n, _pairs(ms, recs), thr) == want


def test_biggest_component_refusals(ms):
    lib = ms.load()
    keep, nk = (C.c_int * 16)(), C.c_int(0)
    for recs, word in (([(0, 4, 1.0)], "views"), ([(-1, 2, 1.0)], "views"), ([(2, 2, 1.0)], "itself")):
        arr = ms.pair_matches(_pairs(ms, recs))
        assert lib.ms_biggest_component(4, arr, 1, C.c_double(1.0), keep, C.byref(nk)) == INVALID and word.encode() in lib.ms_last_error()
    arr = ms.pair_matches(_pairs(ms, [(0, 1, 1.0)]))
    assert lib.ms_biggest_component(4, None, 1, C.c_double(1.0), keep, C.byref(nk)) == INVALID
    assert lib.ms_biggest_component(4, arr, 1, C.c_double(1.0), None, C.byref(nk)) == INVALID
    assert lib.ms_biggest_component(4, arr, 1, C.c_double(1.0), keep, None) == INVALID
    assert lib.ms_biggest_component(0, arr, 1, C.c_double(1.0), keep, C.byref(nk)) == INVALID
    assert lib.ms_biggest_component(17, arr, 1, C.c_double(1.0), keep, C.byref(nk)) == INVALID
    assert lib.ms_biggest_component(4, arr, -1, C.c_double(1.0), keep, C.byref(nk)) == INVALID
