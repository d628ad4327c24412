"""Self-calibrating rigs (ms_focals_from_homography, ms_estimate_rig, ms_rig_focal_default_params, ms_rig_focal_accumulate, ms_refine_rig_cameras,
ms_refine_rig_focals): what holds without a device -- the six names, the struct layouts and defaults, every validation case of the device entry points (refused before
the device is touched), the two host-only entry points in full, and the numpy reference's own terms, gradient and convergence."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import rig_focal_ref as fr
import rig_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ms_focals_from_homography", "ms_estimate_rig", "ms_rig_focal_default_params", "ms_rig_focal_accumulate", "ms_refine_rig_cameras", "ms_refine_rig_focals"]


def _err(ms):
    return ms.load().ms_last_error().decode()


def test_the_six_names_are_declared_exported_and_bound(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in include/ms_stitch.h" % n
        assert n in ms.EXPORTS and hasattr(lib, n), n
    for f in ("focals_from_homography", "estimate_rig", "rig_focal_default_params", "rig_focal_accumulate", "refine_rig_cameras"):
        assert callable(getattr(ms, f))
    assert callable(ms.Compositor.refine_rig_focals)


def test_defaults_and_struct_sizes(ms):
    p = ms.rig_focal_default_params()
    assert (p.struct_size, p.anchor_view, p.shared_focal, p.max_iters, p.huber_px, p.step_tol, p.min_pair_matches) == (C.sizeof(ms.RigFocalParams), 0, 0, 50, 0.0, 1e-10, 4)
    # the layouts include/ms_stitch.h declares
    assert C.sizeof(ms.RigPxMatch) == 40 and C.sizeof(ms.RigFocalParams) == 40 and C.sizeof(ms.RigFocalInfo) == 56 and C.sizeof(ms.PairHomography) == 88
    assert C.sizeof(ms.RigEstimateInfo) == 4 * 17
    assert ms.load().ms_rig_focal_default_params(None) == -1 and "ms_rig_focal_default_params" in _err(ms)


# ---- validation of the device entry points ----------------------------------------------------------------------------------------------------------
def _call(ms, n_views, f, R, matches, n, prm, accumulate=False, null=None):
    """the raw entry point with everything valid but what the case breaks; returns (status, message)"""
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    nv = max(n_views, 1)
    fo = np.zeros(nv); out = np.zeros((nv, 3, 3)); H = np.zeros((4 * nv) ** 2); g = np.zeros(4 * nv); cost = C.c_double()
    info = ms.RigFocalInfo()
    arr = ms.rig_px_matches(matches)
    ptr = lambda name, a: None if null == name else a.ctypes.data_as(dp)
    if accumulate:
        rc = lib.ms_rig_focal_accumulate(n_views, ptr("f", fa), ptr("R", Ra), None if null == "matches" else arr, n, C.c_double(prm), None if null == "cost" else C.byref(cost),
                                         ptr("H", H), ptr("g", g), None)
    else:
        rc = lib.ms_refine_rig_cameras(n_views, ptr("f", fa), ptr("R", Ra), None if null == "matches" else arr, n, None if null == "prm" else C.byref(prm), ptr("f_out", fo),
                                       ptr("R_out", out), C.byref(info), None)
    return rc, _err(ms)


def _valid(n=3):
    rng = np.random.default_rng(9)
    R = rr.ring(6)[:n].copy()
    f = np.full(n, 400.0)
    return f, R, fr.make_px_matches(f * 1.03, rr.perturbed(R, rng, 2.0), [(v, v + 1) for v in range(n - 1)], 5, rng)


def _with(m, **kw):
    va, vb, a, b = m
    return (kw.get("va", va), kw.get("vb", vb), kw.get("a", a), kw.get("b", b))


BAD_MATCH = {
    "view index out of range": lambda m: _with(m, vb=3),
    "negative view index": lambda m: _with(m, va=-1),
    "view_a == view_b": lambda m: _with(m, vb=m[0]),
    "NaN pixel": lambda m: _with(m, a=np.array([np.nan, 0.0])),
    "infinite pixel": lambda m: _with(m, b=np.array([0.0, -np.inf])),
}


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", sorted(BAD_MATCH))
def test_bad_matches_are_invalid_before_the_device_is_touched(ms, case, accumulate):
    f, R, M = _valid()
    M[3] = BAD_MATCH[case](M[3])
    rc, msg = _call(ms, 3, f, R, M, len(M), 0.0 if accumulate else ms.rig_focal_default_params(), accumulate)
    assert rc == -1 and "match 3" in msg, (rc, msg)


@pytest.mark.parametrize("accumulate", [False, True])
def test_bad_cameras_counts_and_null_pointers_are_invalid(ms, accumulate):
    f, R, M = _valid()
    prm = (lambda: 0.0) if accumulate else ms.rig_focal_default_params
    name = "ms_rig_focal_accumulate" if accumulate else "ms_refine_rig_cameras"
    for nv in (1, 0, -3, 17):
        rc, msg = _call(ms, nv, np.full(17, 400.0), np.array([np.eye(3)] * 17), M, len(M), prm(), accumulate)
        assert rc == -1 and name in msg and "n_views" in msg, (nv, rc, msg)
    for n in (0, -1, (1 << 20) + 1):
        rc, msg = _call(ms, 3, f, R, M, n, prm(), accumulate)
        assert rc == -1 and name in msg and "matches" in msg, (n, rc, msg)
    for null in (("f", "R", "matches", "cost", "H", "g") if accumulate else ("f", "R", "matches", "prm", "f_out", "R_out")):
        rc, msg = _call(ms, 3, f, R, M, len(M), prm(), accumulate, null=null)
        assert rc == -1 and "null" in msg, (null, rc, msg)
    for bad in (0.0, -400.0, float("nan"), float("inf")):
        fb = f.copy(); fb[1] = bad
        rc, msg = _call(ms, 3, fb, R, M, len(M), prm(), accumulate)
        assert rc == -1 and "focal of view 1" in msg, (bad, rc, msg)
    Rb = R.copy(); Rb[2, 1, 1] = np.nan
    rc, msg = _call(ms, 3, f, Rb, M, len(M), prm(), accumulate)
    assert rc == -1 and "rotation of view 2 is not finite" in msg, (rc, msg)
    Rb = R.copy(); Rb[1] = Rb[1] * (1.0 + 2e-6)            # R R^T off the identity by 4e-6
    rc, msg = _call(ms, 3, f, Rb, M, len(M), prm(), accumulate)
    assert rc == -1 and "rotation of view 1 is not orthonormal" in msg, (rc, msg)
    Rb = R.copy(); Rb[1] = Rb[1] * (1.0 + 2e-7)            # ... by 4e-7: inside the band, the next refusal is the missing device (or none with a GPU)
    rc, msg = _call(ms, 3, f, Rb, M, len(M), prm(), accumulate)
    assert rc in (0, -4), (rc, msg)


def test_bad_params_are_invalid(ms):
    f, R, M = _valid()
    for field, value, word in (("anchor_view", 3, "anchor"), ("anchor_view", -1, "anchor"), ("struct_size", 44, "struct_size"), ("struct_size", 0, "struct_size"),
                               ("max_iters", 0, "max_iters"), ("max_iters", 1001, "max_iters"), ("huber_px", -1e-3, "huber_px"), ("huber_px", float("nan"), "huber_px"),
                               ("step_tol", -1.0, "step_tol"), ("step_tol", float("inf"), "step_tol"), ("min_pair_matches", 0, "min_pair_matches")):
        prm = ms.rig_focal_default_params(**{field: value})
        rc, msg = _call(ms, 3, f, R, M, len(M), prm)
        assert rc == -1 and "ms_refine_rig_cameras" in msg and word in msg, (field, value, rc, msg)
    for bad in (-1.0, float("nan"), float("inf")):
        rc, msg = _call(ms, 3, f, R, M, len(M), bad, accumulate=True)
        assert rc == -1 and "huber_px" in msg, (bad, rc, msg)
    fb = f.copy(); fb[2] = np.nextafter(fb[2], 1e9)
    rc, msg = _call(ms, 3, fb, R, M, len(M), ms.rig_focal_default_params(shared_focal=1))
    assert rc == -1 and "shared_focal" in msg and "view 2" in msg, (rc, msg)


def test_a_view_cut_off_from_the_anchor_is_invalid_and_named(ms):
    """host-side, before the device: views 0-1-2-3 chained, the pair (1, 2) has 3 matches < min_pair_matches"""
    rng = np.random.default_rng(3)
    R = rr.ring(6)[:4]; f = np.full(4, 400.0)
    M = fr.make_px_matches(f, R, [(0, 1), (1, 2), (2, 3)], [5, 3, 5], rng)
    rc, msg = _call(ms, 4, f, R, M, len(M), ms.rig_focal_default_params())
    assert rc == -1 and "view 2 is not connected" in msg and "1 pairs ignored" in msg, (rc, msg)
    rc, msg = _call(ms, 4, f, R, M, len(M), ms.rig_focal_default_params(anchor_view=3))
    assert rc == -1 and "view 0 is not connected" in msg, (rc, msg)


def test_well_formed_calls_reach_the_device(ms):
    """valid arguments pass every host check: without a device the refusal is MS_ERR_NO_DEVICE, with one the call succeeds"""
    import torch
    f, R, M = _valid()
    want = 0 if torch.cuda.is_available() else -4
    for accumulate in (False, True):
        for prm in ((0.0, 2.5) if accumulate else (ms.rig_focal_default_params(), ms.rig_focal_default_params(shared_focal=1, huber_px=2.0, anchor_view=2))):
            rc, msg = _call(ms, 3, f, R, M, len(M), prm, accumulate)
            assert rc == want and (want == 0 or "no CPU fallback" in msg), (rc, msg)


def test_context_form_refuses_null_arguments(ms):
    lib = ms.load()
    prm = ms.rig_focal_default_params()
    out = (C.c_float * 18)(); fo = (C.c_double * 2)(); cnt = (C.c_int * 2)(1, 0); m = (ms.MeshMatch * 1)()
    assert lib.ms_refine_rig_focals(None, m, cnt, C.byref(prm), fo, out, None, None) == -1 and "ms_refine_rig_focals" in _err(ms) and "null" in _err(ms)


# ---- the host-only entry points ---------------------------------------------------------------------------------------------------------------------
def off_ring(n, seed, deg=2.0):
    """a ring of n views with every view but view 0 up to `deg` degrees off it about each axis"""
    rng = np.random.default_rng(seed)
    R = rr.perturbed(rr.ring(n), rng, deg)
    R[0] = np.eye(3)
    return R


def test_focals_from_homography_recovers_both_focals(ms):
    """H = K_b R_b^T R_a K_a^-1 exactly, f_a != f_b: f0 = f_a and f1 = f_b.  The squares are quotients of differences of O(1) squares of H's entries, condition below
    100 for these 60 degree steps, and H carries the rounding of its own two products: 1e-12 relative leaves two orders."""
    R = off_ring(6, 4)
    for v, (fa, fb) in enumerate([(400.0, 520.0), (731.5, 388.25), (1000.0, 1000.0), (350.0, 351.0), (600.0, 420.0), (480.0, 611.0)]):
        H = fr.homography(fa, R[v], fb, R[(v + 1) % 6]) * (1.0 + 0.5 * v)      # the scale of H is free
        f0, f1 = ms.focals_from_homography(H)
        r0, r1 = fr.focals_from_homography(H)
        assert f0 is not None and f1 is not None
        assert abs(f0 / fa - 1.0) <= 1e-12 and abs(f1 / fb - 1.0) <= 1e-12, (v, f0, f1)
        assert abs(f0 / r0 - 1.0) <= 8 * 2.0 ** -52 and abs(f1 / r1 - 1.0) <= 8 * 2.0 ** -52      # the same dozen operations in both


def test_focals_from_homography_reports_what_it_cannot_determine(ms):
    assert ms.focals_from_homography(np.eye(3)) == (None, None)
    assert ms.focals_from_homography(np.diag([1.0, 1.0, 1.0]) @ rr.exp_so3(np.array([0.0, 0.0, 0.3]))) == (None, None)      # a roll alone
    lib = ms.load()
    H = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1); d = C.c_double(); k = C.c_int()
    assert lib.ms_focals_from_homography(None, C.byref(d), C.byref(d), C.byref(k), C.byref(k)) == -1 and "ms_focals_from_homography" in _err(ms)
    assert lib.ms_focals_from_homography(H, C.byref(d), C.byref(d), C.byref(k), None) == -1
    H[4] = float("nan")
    assert lib.ms_focals_from_homography(H, C.byref(d), C.byref(d), C.byref(k), C.byref(k)) == -1 and "H[4]" in _err(ms)


def ring_homographies(n, f, R, flip=()):
    """the exact homographies of the ring's neighbouring pairs, weights 10 + pair index; pairs in `flip` listed (j, i) with the inverse map at another scale"""
    out = []
    for v, (i, j) in enumerate(rr.ring_pairs(n)):
        H = fr.homography(f, R[i], f, R[j])
        out.append((j, i, np.linalg.inv(H) * 2.5, 10 + v) if v in flip else (i, j, H, 10 + v))
    return out


@pytest.mark.parametrize("anchor, flip", [(0, ()), (3, (1, 4)), (5, (0, 1, 2, 3, 4, 5))])
def test_estimate_rig_on_exact_ring_homographies(ms, anchor, flip):
    """6 views off the ring, one true focal, exact homographies: the true focal and the true rotations in the anchor's gauge.  Against the numpy reference
    (numpy.linalg.inv / svd): along an edge both implementations spend a few dozen double operations (three 3 x 3 products, an inverse, the decomposition) on a matrix
    that is a rotation up to scale once K is taken out (condition 1), at most 32 roundings of 2^-53 relative each, 32 * 2^-52 between the two; the tree chains at
    most n - 1 = 5 edges: 160 * 2^-52 = 3.6e-14 rad.  The focal is the same dozen operations in both: 8 * 2^-52 relative."""
    n, f_true = 6, 431.5
    Rt = off_ring(n, 12)
    pairs = ring_homographies(n, f_true, Rt, flip)
    f, R, info = ms.estimate_rig(n, pairs, (640, 480), anchor=anchor)
    rf, rR, rstatus = fr.estimate_rig(n, pairs, (640, 480), anchor=anchor)
    want = rr.expected(np.array([np.eye(3)] * n), Rt, anchor)
    to_ref = max(rr.angle(R[v], rR[v]) for v in range(n)); to_truth = max(rr.angle(R[v], want[v]) for v in range(n))
    print("anchor %d: %.3e rad to the reference, %.3e rad to the truth, focal %.17g (reference %.17g), tree %s" % (anchor, to_ref, to_truth, f[0], rf[0], info["tree_parent"]))
    assert info["status"] == 0 == rstatus and info["focal_estimates"] == 6
    assert np.all(f == f[0]) and abs(f[0] / rf[0] - 1.0) <= 8 * 2.0 ** -52 and abs(f[0] / f_true - 1.0) <= 1e-12
    assert to_ref <= (n - 1) * 32 * 2.0 ** -52
    assert to_truth <= 1e-12
    assert R[anchor].tobytes() == np.eye(3).tobytes() and info["tree_parent"][anchor] == -1
    assert all(abs(np.linalg.det(R[v]) - 1.0) < 1e-14 and np.allclose(R[v] @ R[v].T, np.eye(3), atol=1e-14) for v in range(n))
    # the maximum spanning tree drops the lightest pair of the ring, (0, 1) with weight 10: view 1 hangs on view 2, not on view 0
    assert info["tree_parent"][1] == 2 or anchor == 1


def test_estimate_rig_tree_median_and_fallback(ms):
    """weights decide the tree (ties to the earlier pair); the focal is the median of the valid estimates; no valid estimate: width + height and status 1"""
    n = 4
    Rt = off_ring(6, 5)[:n]
    H = lambda i, j, f=500.0: fr.homography(f, Rt[i], f, Rt[j])
    # 0-1 (9), 1-2 (9), 0-2 (9, later: closes a cycle, left out), 2-3 (1), 1-3 (1, later, left out)
    pairs = [(0, 1, H(0, 1), 9), (1, 2, H(1, 2), 9), (0, 2, H(0, 2), 9), (2, 3, H(2, 3), 1), (1, 3, H(1, 3), 1)]
    f, R, info = ms.estimate_rig(n, pairs, (640, 480))
    assert info["tree_parent"] == [-1, 0, 1, 2]
    # an even number of estimates: the mean of the middle two.  Pairs at 400, 500, 600, 700 -> 550
    pairs = [(0, 1, H(0, 1, 400.0), 5), (1, 2, H(1, 2, 700.0), 5), (2, 3, H(2, 3, 600.0), 5), (0, 2, H(0, 2, 500.0), 1)]
    f, R, info = ms.estimate_rig(n, pairs, (640, 480))
    rf, _, _ = fr.estimate_rig(n, pairs, (640, 480))
    assert info["focal_estimates"] == 4 and abs(f[0] - 550.0) <= 1e-9 and abs(f[0] / rf[0] - 1.0) <= 8 * 2.0 ** -52
    # rolls determine no focal
    roll = lambda t: rr.exp_so3(np.array([0.0, 0.0, t]))
    f, R, info = ms.estimate_rig(3, [(0, 1, roll(0.2), 5), (1, 2, roll(0.3), 5)], (640, 480))
    assert info["status"] == 1 and info["focal_estimates"] == 0 and np.all(f == 1120.0)
    assert max(rr.angle(R[v], roll(-t)) for v, t in ((1, 0.2), (2, 0.5))) <= 1e-14      # K commutes with a roll: the chain is still exact


def test_estimate_rig_validation(ms):
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    Rt = off_ring(6, 5)
    good = [(v, v + 1, fr.homography(500.0, Rt[v], 500.0, Rt[v + 1]), 7) for v in range(3)]
    f = np.zeros(16); R = np.zeros(16 * 9)

    def call(n_views, pairs, n_pairs=None, anchor=0, size=(640, 480), null=None):
        arr = ms.pair_homographies(pairs)
        rc = lib.ms_estimate_rig(n_views, None if null == "pairs" else arr, len(pairs) if n_pairs is None else n_pairs, anchor, size[0], size[1],
                                 None if null == "focals" else f.ctypes.data_as(dp), None if null == "R" else R.ctypes.data_as(dp), None)
        return rc, _err(ms)

    assert call(4, good)[0] == 0
    for kw, word in ((dict(n_views=1), "n_views"), (dict(n_views=17), "n_views"), (dict(n_pairs=0), "n_pairs"), (dict(n_pairs=257), "n_pairs"), (dict(anchor=4), "anchor"), (dict(anchor=-1), "anchor"),
                     (dict(size=(0, 480)), "image size"), (dict(null="pairs"), "null"), (dict(null="focals"), "null"), (dict(null="R"), "null")):
        rc, msg = call(**{"n_views": 4, "pairs": good, **kw})
        assert rc == -1 and "ms_estimate_rig" in msg and word in msg, (kw, rc, msg)
    for bad, word in (((0, 4, good[0][2], 7), "pair 1 names views"), ((2, 2, good[0][2], 7), "pair 1 pairs view 2 with itself"), ((1, 2, good[1][2], -1), "weight"),
                      ((1, 2, good[1][2] * np.nan, 7), "not finite"), ((1, 2, np.ones((3, 3)), 7), "singular")):
        rc, msg = call(4, [good[0], bad, good[2]])
        assert rc == -1 and word in msg, (word, rc, msg)
    rc, msg = call(4, [good[0], good[2]])              # 0-1 and 2-3: views 2 and 3 hang on nothing
    assert rc == -1 and "view 2 is not connected to the anchor view 0" in msg, (rc, msg)
    rc, msg = call(4, [good[0], good[2]], anchor=3)
    assert rc == -1 and "view 0 is not connected to the anchor view 3" in msg, (rc, msg)
    with pytest.raises(ValueError, match="view 2"):
        fr.estimate_rig(4, [good[0], good[2]], (640, 480))


# ---- the reference against itself ---------------------------------------------------------------------------------------------------------------------
def _case(seed=1):
    rng = np.random.default_rng(seed)
    n = 4
    R = rr.perturbed(rr.ring(6)[:n], rng, 3.0)
    f = np.array([500.0, 520.0, 480.0, 510.0])
    M = fr.make_px_matches(f * (1 + rng.uniform(-0.05, 0.05, n)), rr.perturbed(R, rng, 2.0), [(0, 1), (1, 2), (2, 3), (0, 2)], 12, rng, noise_px=0.5)
    M[3] = (M[3][1], M[3][0], M[3][3], M[3][2])       # one match listed (j, i)
    return n, f, R, M


def test_reference_terms_are_the_matrix_form():
    """tests/rig_focal_ref.py's explicit per-match terms against J^T r and J^T J with J_i = [-[u]x | ci], J_j = [[v]x | cj] built as matrices"""
    n, f, R, M = _case()
    i, j, a, b = fr.unpack(M)
    assert np.all(i < j)
    sk = lambda x: np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
    for h in (0.0, 15.0):
        T, s = fr.terms(f, R, i, j, a, b, h)
        assert h == 0.0 or (0 < (s > h).sum() < len(s))
        for k in range(len(M)):
            fi, fj = f[i[k]], f[j[k]]
            ra = np.array([a[k, 0], a[k, 1], fi]); ra /= np.linalg.norm(ra)
            rb = np.array([b[k, 0], b[k, 1], fj]); rb /= np.linalg.norm(rb)
            m = math.sqrt(fi * fj)
            p = R[i[k]] @ ra; q = R[j[k]] @ rb; r = m * (p - q)
            Ji = np.column_stack([-m * sk(p), r / 2 + m * ra[2] * (R[i[k]][:, 2] - ra[2] * p)])
            Jj = np.column_stack([m * sk(q), r / 2 - m * rb[2] * (R[j[k]][:, 2] - rb[2] * q)])
            w = 1.0 if h == 0.0 or np.linalg.norm(r) <= h else h / np.linalg.norm(r)
            rho = r @ r if w == 1.0 else 2 * h * np.linalg.norm(r) - h * h
            gi, gj, Hii, Hjj, Hij = [x[0] for x in fr._blocks(T[k:k + 1])]
            for got, want in ((T[k, 0], rho), (gi, w * Ji.T @ r), (gj, w * Jj.T @ r), (Hii, w * Ji.T @ Ji), (Hjj, w * Jj.T @ Jj), (Hij, w * Ji.T @ Jj)):
                # entries up to m^2 = 2.7e5; every factor (u, v, ci, cj, r) is a dozen roundings of 2^-53 from its matrix-form twin, a product of two doubles
                # that, a sum of three adds a few: 64
                assert np.allclose(got, want, rtol=0, atol=64 * 2.0 ** -53 * 2.7e5), (k, np.max(np.abs(got - want)))
            assert T[k, 45] == (1.0 if w < 1.0 else 0.0)


def test_reference_gradient_is_the_central_difference_of_the_cost():
    """d cost / d unknown = 2 g for every rotation and log-focal component, both Huber branches.  A cost of len(M) + 8 rounded terms is known to (len(M) + 8) 2^-52 cost,
    so a central difference over 2 eps is known to that over 2 eps (1.3e-4 here); the truncation, eps^2 / 6 times a third derivative of the order of |g|, is far below."""
    n, f, R, M = _case()
    eps = 1e-6
    for h in (0.0, 15.0):
        cost, H, g = fr.accumulate(f, R, M, h)
        num = np.zeros(4 * n)
        for e in range(4 * n):
            d = np.zeros(4 * n); d[e] = eps
            num[e] = (fr.cost_only(*fr.apply_step(f, R, d), M, h) - fr.cost_only(*fr.apply_step(f, R, -d), M, h)) / (2 * eps)
        bound = (len(M) + 8) * 2.0 ** -52 * cost / (2 * eps) + eps * eps * np.max(np.abs(g))
        print("h = %g: max |central difference - 2 g| = %.3e (bound %.3e) on entries up to %.3e" % (h, np.max(np.abs(num - 2 * g)), bound, np.max(np.abs(g))))
        assert np.max(np.abs(num - 2 * g)) <= bound and np.max(np.abs(g)) > 1e4
        assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() > 0


RECOVERY = {}


def recovery_case(shared):
    """6 views x 60 exact matches a ring pair; the true rig's non-anchor rotations up to 2 degrees off the ring; per view: true focals up to 5 % off 400, the start 15 % low
    and 20 % high in turn; shared: true focal 400, the start 30 % low.  The start rotations are the ideal ring."""
    if shared not in RECOVERY:
        n = 6
        rng = np.random.default_rng(2)
        R0 = rr.ring(n)
        Rt = rr.perturbed(R0, rng, 2.0); Rt[0] = R0[0]
        ft = np.full(n, 400.0) if shared else 400.0 * (1 + rng.uniform(-0.05, 0.05, n))
        f0 = np.full(n, 280.0) if shared else 400.0 * np.where(np.arange(n) % 2, 0.85, 1.2)
        M = fr.make_px_matches(ft, Rt, rr.ring_pairs(n), 60, rng)
        RECOVERY[shared] = (f0, R0, ft, Rt, M, fr.refine(f0, R0, M, shared_focal=shared, step_tol=1e-13))
    return RECOVERY[shared]


@pytest.mark.parametrize("shared", [False, True])
def test_reference_recovers_exactly_from_wrong_focals(shared):
    """exact matches have the true cameras as a zero of the cost: the loop must end there, at the rounding floor (measured 2e-16 relative and 1e-16 rad; the bound
    leaves the conditioning of a 360-match system three orders)"""
    f0, R0, ft, Rt, M, (f, R, info) = recovery_case(shared)
    err_f = np.max(np.abs(f / ft - 1.0)); err_R = max(rr.angle(R[v], Rt[v]) for v in range(6))
    print("shared %s: focal ratio off 1 by %.3e, rotations %.3e rad, %s" % (shared, err_f, err_R, info))
    assert info["stop_reason"] == fr.CONVERGED and info["iterations"] <= 25
    assert err_f <= 1e-13 and err_R <= 1e-13
    assert info["cost_final"] <= 1e-18 * info["cost_initial"] and info["max_focal_ratio"] > 1.15
    assert not shared or np.all(f == f[0])
