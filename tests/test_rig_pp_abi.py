"""The centre form of the rig refinement (ms_rig_pp_default_params, ms_rig_pp_accumulate, ms_refine_rig_pp, ms_refine_rig_pp_ctx): what holds without a device --
the names, the defaults, struct_size, and every refusal, each with its code and naming its argument, before the device is touched.

A context cannot exist without a device (ms_create): of the context form only the null-argument refusal is decided here, the rest in tests/test_rig_pp_gpu.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import lens_ref as L
import rig_lens_ref as lr
import rig_pp_ref as pr
import rig_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ms_rig_pp_default_params", "ms_rig_pp_accumulate", "ms_refine_rig_pp", "ms_refine_rig_pp_ctx"]
PP = np.array([[3.0, -2.0], [0.5, 4.0], [-6.0, 1.0]])


def _err(ms):
    return ms.load().ms_last_error().decode()


def _valid(lens=L.FISH):
    rng = np.random.default_rng(9)
    R = rr.ring(6)[:3].copy()
    f = np.full(3, 400.0)
    return f, R, pr.make_pp_matches(f * 1.03, rr.perturbed(R, rng, 2.0), PP, [lens] * 3, [(0, 1), (1, 2)], 5, rng)


def _call(ms, n_views, f, R, pp, lenses, matches, n, prm, accumulate=False, null=None):
    """the raw calls; prm: a RigPpParams, or for accumulate huber_px; lenses: lens_ref tuples, or None for the null pointer"""
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64); pa = np.ascontiguousarray(pp, np.float64)
    nv = max(n_views, 1)
    fo = np.zeros(nv); out = np.zeros((nv, 3, 3)); po = np.zeros((nv, 2)); H = np.zeros((6 * nv) ** 2); g = np.zeros(6 * nv); cost = C.c_double()
    info = ms.RigPpInfo()
    arr = ms.rig_px_matches(matches)
    la = ms.lens_array([L.to_ms(ms, l) if l[0] != "none" else None for l in lenses]) if lenses is not None else None
    ptr = lambda name, a: None if null == name else a.ctypes.data_as(dp)
    if accumulate:
        rc = lib.ms_rig_pp_accumulate(n_views, ptr("f", fa), ptr("R", Ra), ptr("pp", pa), la, None if null == "matches" else arr, n, C.c_double(prm),
                                      None if null == "cost" else C.byref(cost), ptr("H", H), ptr("g", g), None)
    else:
        rc = lib.ms_refine_rig_pp(n_views, ptr("f", fa), ptr("R", Ra), ptr("pp", pa), la, None if null == "matches" else arr, n, None if null == "prm" else C.byref(prm),
                                  ptr("f_out", fo), ptr("R_out", out), ptr("pp_out", po), C.byref(info), None)
    return rc, _err(ms)


def test_the_names_are_declared_exported_and_bound(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in include/ms_stitch.h" % n
        assert n in ms.EXPORTS and hasattr(lib, n), n
    for f in ("rig_pp_default_params", "rig_pp_accumulate", "refine_rig_pp"):
        assert callable(getattr(ms, f))
    assert callable(ms.Compositor.refine_rig_pp)
    assert "ms_rig_pp_params" in text and "ms_rig_pp_info" in text and "max_pp_shift" in text and "pp_prior" in text
    # every new entry point cites the reference call it replaces
    full = open(os.path.join(ROOT, "include", "ms_stitch.h")).read()
    assert full.count("BundleAdjusterReproj") >= 3 and "motion_estimators.cpp:329-511" in full


def test_defaults_and_struct_size(ms):
    p = ms.rig_pp_default_params(); q = ms.rig_focal_default_params()
    assert p.struct_size == C.sizeof(ms.RigPpParams) == 48 and p.pp_prior == 0.0
    for name, _ in ms.RigFocalParams._fields_[1:]:
        assert getattr(p, name) == getattr(q, name), name
    assert (p.anchor_view, p.shared_focal, p.max_iters, p.huber_px, p.step_tol, p.min_pair_matches) == (0, 0, 50, 0.0, 1e-10, 4)
    assert [n for n, _ in ms.RigPpInfo._fields_] == [n for n, _ in ms.RigFocalInfo._fields_] + ["max_pp_shift"]
    assert ms.load().ms_rig_pp_default_params(None) == -1 and "ms_rig_pp_default_params: null" in _err(ms)
    f, R, M = _valid()
    p.struct_size += 8
    rc, msg = _call(ms, 3, f, R, PP, [L.FISH] * 3, M, len(M), p)
    assert rc == -1 and "struct_size" in msg and "ms_rig_pp_params" in msg


@pytest.mark.parametrize("accumulate", [False, True])
def test_refusals_of_the_offsets_the_prior_and_the_lenses(ms, accumulate):
    f, R, M = _valid()
    name = "ms_rig_pp_accumulate" if accumulate else "ms_refine_rig_pp"
    prm = (lambda **kw: 0.0) if accumulate else ms.rig_pp_default_params
    rc, msg = _call(ms, 3, f, R, PP, [L.FISH] * 3, M, len(M), prm(), accumulate, null="pp")
    assert rc == -1 and name in msg and "null offsets" in msg
    for bad in (float("nan"), float("inf")):
        pb = PP.copy(); pb[1, 1] = bad
        rc, msg = _call(ms, 3, f, R, pb, [L.FISH] * 3, M, len(M), prm(), accumulate)
        assert rc == -1 and name in msg and "offset of view 1" in msg and "not finite" in msg
    # a lens ms_lens_check refuses, in any view
    rc, msg = _call(ms, 3, f, R, PP, [L.FISH, L.FISH, ("fisheye", (-0.2, 0.0, 0.0, 0.0), 100.0)], M, len(M), prm(), accumulate)
    assert rc == -1 and "radial profile" in msg
    if not accumulate:
        for w in (-1e-3, float("nan"), float("inf")):
            rc, msg = _call(ms, 3, f, R, PP, [L.FISH] * 3, M, len(M), ms.rig_pp_default_params(pp_prior=w))
            assert rc == -1 and name in msg and "pp_prior" in msg, (w, rc, msg)
    # lenses == NULL is every view without a lens: nothing about the lenses is refused (with no device the call ends later, at the device)
    fn, Rn, Mn = _valid(("none", (), 0.0))
    rc, msg = _call(ms, 3, fn, Rn, PP, None, Mn, len(Mn), prm(), accumulate)
    assert rc == 0 or ("lens" not in msg and "null" not in msg), msg


@pytest.mark.parametrize("accumulate", [False, True])
def test_refusals_of_the_lens_form_stay(ms, accumulate):
    """everything ms_refine_rig_cameras_lens refuses: null pointers, n_views, focals, rotations, matches, the parameters"""
    f, R, M = _valid()
    lenses = [L.FISH] * 3
    prm = (lambda **kw: 0.0) if accumulate else ms.rig_pp_default_params
    for null in ("f", "R", "matches") + (("cost", "H", "g") if accumulate else ("prm", "f_out", "R_out", "pp_out")):
        rc, msg = _call(ms, 3, f, R, PP, lenses, M, len(M), prm(), accumulate, null=null)
        assert rc == -1 and "null" in msg, (null, rc, msg)
    for nv in (1, 17):
        rc, msg = _call(ms, nv, np.full(17, 400.0), np.array([np.eye(3)] * 17), np.zeros((17, 2)), [L.FISH] * 17, M, len(M), prm(), accumulate)
        assert rc == -1 and "n_views" in msg
    for n in (0, (1 << 20) + 1):
        rc, msg = _call(ms, 3, f, R, PP, lenses, M, n, prm(), accumulate)
        assert rc == -1 and "matches outside" in msg
    fb = f.copy(); fb[1] = -400.0
    rc, msg = _call(ms, 3, fb, R, PP, lenses, M, len(M), prm(), accumulate)
    assert rc == -1 and "focal of view 1" in msg
    Rb = R.copy(); Rb[2] = Rb[2] * 1.001
    rc, msg = _call(ms, 3, f, Rb, PP, lenses, M, len(M), prm(), accumulate)
    assert rc == -1 and "rotation of view 2 is not orthonormal" in msg
    Mb = list(M); Mb[3] = (Mb[3][0], Mb[3][0], Mb[3][2], Mb[3][3])
    rc, msg = _call(ms, 3, f, R, PP, lenses, Mb, len(Mb), prm(), accumulate)
    assert rc == -1 and "match 3" in msg
    Mb = list(M); Mb[4] = (Mb[4][0], Mb[4][1], np.array([float("nan"), 0.0]), Mb[4][3])
    rc, msg = _call(ms, 3, f, R, PP, lenses, Mb, len(Mb), prm(), accumulate)
    assert rc == -1 and "match 4" in msg and "not finite" in msg
    if accumulate:
        rc, msg = _call(ms, 3, f, R, PP, lenses, M, len(M), float("nan"), True)
        assert rc == -1 and "huber_px" in msg
        return
    for kw, word in ((dict(anchor_view=3), "anchor_view"), (dict(max_iters=0), "max_iters"), (dict(max_iters=1001), "max_iters"), (dict(huber_px=-1.0), "huber_px"),
                     (dict(step_tol=float("inf")), "step_tol"), (dict(min_pair_matches=0), "min_pair_matches")):
        rc, msg = _call(ms, 3, f, R, PP, lenses, M, len(M), ms.rig_pp_default_params(**kw))
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = _call(ms, 3, np.array([400.0, 401.0, 400.0]), R, PP, lenses, M, len(M), ms.rig_pp_default_params(shared_focal=1))
    assert rc == -1 and "shared_focal" in msg and "view 1" in msg
    rc, msg = _call(ms, 3, f, R, PP, lenses, [m for m in M if m[0] == 0], 5, ms.rig_pp_default_params())
    assert rc == -1 and "view 2 is not connected" in msg


@pytest.mark.parametrize("accumulate", [False, True])
def test_an_unseen_pixel_at_the_input_cameras_and_offsets_names_its_match(ms, accumulate):
    """a pixel 0.5 px inside the rim of the fisheye's field at the focal 400 is seen with the offset 0 and not with an offset that moves it 2 px outwards: the check
    runs at the input cameras AND offsets"""
    f, R, M = _valid()
    th = math.radians(100.0)
    rim, seen = lr.centred_pixels(400.0, L.FISH, np.array([[math.sin(th), 0.0, math.cos(th)]]))
    assert seen[0]
    px = np.array([rim[0, 0] - 0.5, 0.0])
    unproj = lambda x: lr.unproject(np.diag([400.0, 400.0, 1.0]), L.FISH, x, 0.0)[1][0]
    assert unproj(px[0]) and not unproj(px[0] + 2.0)
    prm = 0.0 if accumulate else ms.rig_pp_default_params()
    Mb = list(M)
    va, vb, a, b = Mb[7]
    pp = PP.copy(); pp[vb] = (0.0, 0.0)
    Mb[7] = (va, vb, a, px)
    rc, msg = _call(ms, 3, f, R, pp, [L.FISH] * 3, Mb, len(Mb), prm, accumulate)
    assert rc == 0 or "does not see" not in msg, msg           # (with no device the call ends later, at the device)
    pp[vb] = (-2.0, 0.0)
    rc, msg = _call(ms, 3, f, R, pp, [L.FISH] * 3, Mb, len(Mb), prm, accumulate)
    assert rc == -1 and "match 7" in msg and "view %d" % vb in msg and "does not see" in msg and "offset" in msg, (rc, msg)


def test_the_context_form_refuses_null_arguments(ms):
    lib = ms.load()
    assert lib.ms_refine_rig_pp_ctx(None, None, None, None, None, None, None, None, None) == -1 and "ms_refine_rig_pp_ctx: null" in _err(ms)
