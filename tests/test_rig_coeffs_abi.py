"""The coefficient form of the rig refinement (ms_rig_coeff_default_params, ms_rig_coeff_accumulate, ms_refine_rig_coeffs, ms_refine_rig_coeffs_ctx): what holds
without a device -- the names, the defaults, struct_size, and every refusal, each with its code and naming its argument, before the device is touched.

A context cannot exist without a device (ms_create): of the context form only the null-argument refusal is decided here, the rest in tests/test_rig_coeffs_gpu.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import lens_ref as L
import rig_lens_ref as lr
import rig_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ms_rig_coeff_default_params", "ms_rig_coeff_accumulate", "ms_refine_rig_coeffs", "ms_refine_rig_coeffs_ctx"]


def _err(ms):
    return ms.load().ms_last_error().decode()


def _valid(lens=L.FISH):
    rng = np.random.default_rng(9)
    R = rr.ring(6)[:3].copy()
    f = np.full(3, 400.0)
    return f, R, lr.make_lens_matches(f * 1.03, rr.perturbed(R, rng, 2.0), [lens] * 3, [(0, 1), (1, 2)], 5, rng)


def _call(ms, n_views, f, R, lens, matches, n, prm, accumulate=False, null=None):
    """the raw calls; prm: a RigCoeffParams, or for accumulate (free_coeffs, huber_px)"""
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    nv = max(n_views, 1)
    fo = np.zeros(nv); out = np.zeros((nv, 3, 3)); H = np.zeros((4 * nv + 8) ** 2); g = np.zeros(4 * nv + 8); cost = C.c_double()
    info = ms.RigCoeffInfo(); lens_out = ms.Lens()
    arr = ms.rig_px_matches(matches)
    lp = None if null == "lens" else C.byref(lens if isinstance(lens, ms.Lens) else L.to_ms(ms, lens))
    ptr = lambda name, a: None if null == name else a.ctypes.data_as(dp)
    if accumulate:
        rc = lib.ms_rig_coeff_accumulate(n_views, ptr("f", fa), ptr("R", Ra), lp, C.c_uint(prm[0]), None if null == "matches" else arr, n, C.c_double(prm[1]),
                                         None if null == "cost" else C.byref(cost), ptr("H", H), ptr("g", g), None)
    else:
        rc = lib.ms_refine_rig_coeffs(n_views, ptr("f", fa), ptr("R", Ra), lp, None if null == "matches" else arr, n, None if null == "prm" else C.byref(prm),
                                      ptr("f_out", fo), ptr("R_out", out), None if null == "lens_out" else C.byref(lens_out), C.byref(info), None)
    return rc, _err(ms)


def test_the_names_are_declared_exported_and_bound(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in include/ms_stitch.h" % n
        assert n in ms.EXPORTS and hasattr(lib, n), n
    for f in ("rig_coeff_default_params", "rig_coeff_accumulate", "refine_rig_coeffs"):
        assert callable(getattr(ms, f))
    assert callable(ms.Compositor.refine_rig_coeffs)
    assert "ms_rig_coeff_params" in text and "ms_rig_coeff_info" in text and "max_coeff_change" in text


def test_defaults_and_struct_size(ms):
    p = ms.rig_coeff_default_params(); q = ms.rig_focal_default_params()
    assert p.struct_size == C.sizeof(ms.RigCoeffParams) and p.free_coeffs == 1
    for name, _ in ms.RigFocalParams._fields_[1:]:
        assert getattr(p, name) == getattr(q, name), name
    assert (p.anchor_view, p.shared_focal, p.max_iters, p.huber_px, p.step_tol, p.min_pair_matches) == (0, 0, 50, 0.0, 1e-10, 4)
    assert [n for n, _ in ms.RigCoeffInfo._fields_] == [n for n, _ in ms.RigFocalInfo._fields_] + ["max_coeff_change"]
    assert ms.load().ms_rig_coeff_default_params(None) == -1 and "ms_rig_coeff_default_params: null" in _err(ms)
    f, R, M = _valid()
    p.struct_size += 8
    rc, msg = _call(ms, 3, f, R, L.FISH, M, len(M), p)
    assert rc == -1 and "struct_size" in msg and "ms_rig_coeff_params" in msg


@pytest.mark.parametrize("accumulate", [False, True])
def test_refusals_of_the_lens_and_the_free_set(ms, accumulate):
    f, R, M = _valid()
    fb, Rb, Mb = _valid(L.BROWN)
    prm = (lambda free: (free, 0.0)) if accumulate else (lambda free: ms.rig_coeff_default_params(free_coeffs=free))
    name = "ms_rig_coeff_accumulate" if accumulate else "ms_refine_rig_coeffs"
    rc, msg = _call(ms, 3, f, R, L.FISH, M, len(M), prm(1), accumulate, null="lens")
    assert rc == -1 and name in msg and "null lens" in msg
    rc, msg = _call(ms, 3, f, R, ms.Lens.make(ms.LENS_NONE), M, len(M), prm(1), accumulate)
    assert rc == -1 and name in msg and "MS_LENS_NONE" in msg
    # a lens ms_lens_check refuses
    rc, msg = _call(ms, 3, f, R, ("fisheye", (-0.2, 0.0, 0.0, 0.0), 100.0), M, len(M), prm(1), accumulate)
    assert rc == -1 and "radial profile" in msg
    # bits outside the model's set
    for lens, free, code, word in ((L.FISH, 0x10, -1, "bits 0..3"), (L.FISH, 0x80, -1, "bits 0..3"), (L.FISH, 0x100, -1, "k[0..7]"), (L.BROWN, 0x100, -1, "k[0..7]"),
                                   (L.BROWN, 0x20, -2, "denominator"), (L.BROWN, 0x80 | 1, -2, "denominator")):
        args = (fb, Rb, lens, Mb) if lens is L.BROWN else (f, R, lens, M)
        rc, msg = _call(ms, 3, args[0], args[1], args[2], args[3], len(args[3]), prm(free), accumulate)
        assert rc == code and name in msg and word in msg and "0x%x" % free in msg, (free, rc, msg)
    # more than 4 bits
    rc, msg = _call(ms, 3, fb, Rb, L.BROWN, Mb, len(Mb), prm(0x1f), accumulate)
    assert rc == -1 and "more than 4" in msg
    # the empty set: refused by the refinement only
    rc, msg = _call(ms, 3, f, R, L.FISH, M, len(M), prm(0), accumulate)
    if accumulate:
        assert "free_coeffs" not in msg, msg                     # (with no device the call ends later, at the device)
    else:
        assert rc == -1 and "free_coeffs is empty" in msg
    # fixed non-zero denominator entries are fine: nothing about the lens is refused
    rat = ("brown", (-0.1, 0.01, 0.0, 0.0, 0.0, 0.02, 0.0, 0.0), 60.0)
    fr_, Rr_, Mr_ = _valid(rat)
    rc, msg = _call(ms, 3, fr_, Rr_, rat, Mr_, len(Mr_), prm(0b10011), accumulate)
    assert "free_coeffs" not in msg and "lens" not in msg, msg


@pytest.mark.parametrize("accumulate", [False, True])
def test_refusals_of_the_lens_form_stay(ms, accumulate):
    """everything ms_refine_rig_cameras_lens refuses: null pointers, n_views, focals, rotations, matches, the parameters"""
    f, R, M = _valid()
    prm = (lambda **kw: (1, 0.0)) if accumulate else ms.rig_coeff_default_params
    for null in ("f", "R", "matches") + (("cost", "H", "g") if accumulate else ("prm", "f_out", "R_out", "lens_out")):
        rc, msg = _call(ms, 3, f, R, L.FISH, M, len(M), prm(), accumulate, null=null)
        assert rc == -1 and "null" in msg, (null, rc, msg)
    for nv in (1, 17):
        rc, msg = _call(ms, nv, np.full(17, 400.0), np.array([np.eye(3)] * 17), L.FISH, M, len(M), prm(), accumulate)
        assert rc == -1 and "n_views" in msg
    for n in (0, (1 << 20) + 1):
        rc, msg = _call(ms, 3, f, R, L.FISH, M, n, prm(), accumulate)
        assert rc == -1 and "matches outside" in msg
    fb = f.copy(); fb[1] = -400.0
    rc, msg = _call(ms, 3, fb, R, L.FISH, M, len(M), prm(), accumulate)
    assert rc == -1 and "focal of view 1" in msg
    Rb = R.copy(); Rb[2] = Rb[2] * 1.001
    rc, msg = _call(ms, 3, f, Rb, L.FISH, M, len(M), prm(), accumulate)
    assert rc == -1 and "rotation of view 2 is not orthonormal" in msg
    Mb = list(M); Mb[3] = (Mb[3][0], Mb[3][0], Mb[3][2], Mb[3][3])
    rc, msg = _call(ms, 3, f, R, L.FISH, Mb, len(Mb), prm(), accumulate)
    assert rc == -1 and "match 3" in msg
    Mb = list(M); Mb[4] = (Mb[4][0], Mb[4][1], np.array([float("nan"), 0.0]), Mb[4][3])
    rc, msg = _call(ms, 3, f, R, L.FISH, Mb, len(Mb), prm(), accumulate)
    assert rc == -1 and "match 4" in msg and "not finite" in msg
    if accumulate:
        rc, msg = _call(ms, 3, f, R, L.FISH, M, len(M), (1, float("nan")), True)
        assert rc == -1 and "huber_px" in msg
        return
    for kw, word in ((dict(anchor_view=3), "anchor_view"), (dict(max_iters=0), "max_iters"), (dict(max_iters=1001), "max_iters"), (dict(huber_px=-1.0), "huber_px"),
                     (dict(step_tol=float("inf")), "step_tol"), (dict(min_pair_matches=0), "min_pair_matches")):
        rc, msg = _call(ms, 3, f, R, L.FISH, M, len(M), ms.rig_coeff_default_params(**kw))
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = _call(ms, 3, np.array([400.0, 401.0, 400.0]), R, L.FISH, M, len(M), ms.rig_coeff_default_params(shared_focal=1))
    assert rc == -1 and "shared_focal" in msg and "view 1" in msg
    rc, msg = _call(ms, 3, f, R, L.FISH, [m for m in M if m[0] == 0], 5, ms.rig_coeff_default_params())
    assert rc == -1 and "view 2 is not connected" in msg


@pytest.mark.parametrize("accumulate", [False, True])
def test_an_unseen_pixel_at_the_input_lens_names_its_match(ms, accumulate):
    """the pixel of a ray at 99.9 degrees of the fisheye (limit 100) at the focal 600 lies outside the field at the input focal 400"""
    f, R, M = _valid()
    th = math.radians(99.9)
    px, seen = lr.centred_pixels(600.0, L.FISH, np.array([[math.sin(th), 0.0, math.cos(th)]]))
    assert seen[0] and not lr.unproject(np.diag([400.0, 400.0, 1.0]), L.FISH, px[0, 0], px[0, 1])[1][0]
    Mb = list(M)
    va, vb, a, b = Mb[7]
    Mb[7] = (va, vb, a, px[0])
    rc, msg = _call(ms, 3, f, R, L.FISH, Mb, len(Mb), (1, 0.0) if accumulate else ms.rig_coeff_default_params(), accumulate)
    assert rc == -1 and "match 7" in msg and "view %d" % vb in msg and "does not see" in msg, (rc, msg)


def test_the_context_form_refuses_null_arguments(ms):
    lib = ms.load()
    assert lib.ms_refine_rig_coeffs_ctx(None, None, None, None, None, None, None, None, None) == -1 and "ms_refine_rig_coeffs_ctx: null" in _err(ms)
