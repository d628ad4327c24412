"""Rig rotation refinement (ms_warper_rays, ms_rig_accumulate, ms_refine_rig_rotations, ms_refine_rig): what holds without a device -- the host-only ray
arithmetic, every validation case (refused before the device is touched), the defaults and struct sizes, and the numpy reference's own terms."""
import ctypes as C
import math

import numpy as np
import pytest

import rig_ref as rr


def _err(ms):
    return ms.load().ms_last_error().decode()


@pytest.mark.parametrize("proj", [rr.PLANE, rr.CYLINDRICAL, rr.SPHERICAL])
def test_warper_rays_against_the_float64_formulas(ms, proj):
    """R^T d(u, v) / |R^T d(u, v)| with d the mapBackward direction in float64: relative 1e-15 per component"""
    rng = np.random.default_rng(40 + proj)
    scale = float(np.float32(611.15))
    R = rr.exp_so3(np.array([0.3, -1.1, 0.2]))
    uv = np.stack([rng.uniform(-math.pi * scale, math.pi * scale, 200), rng.uniform(0.05 * scale, 3.0 * scale, 200)], 1).astype(np.float32)
    if proj != rr.SPHERICAL:
        uv[:, 1] -= np.float32(1.5 * scale)
    for t in ((None,) if proj != rr.PLANE else (None, (0.25, -0.5, 0.125))):
        got = ms.warper_rays(proj, scale, R, uv, t=t)
        for k in range(len(uv)):
            want = rr.warper_ray(proj, scale, R, uv[k, 0], uv[k, 1], t or (0.0, 0.0, 0.0))
            assert np.all(np.abs(got[k] - want) <= 1e-15 * np.abs(want)), (k, got[k], want)
            assert abs(np.linalg.norm(got[k]) - 1.0) < 4e-16


def test_warper_rays_validation(ms):
    lib = ms.load()
    R = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1); uv = (C.c_float * 2)(1, 2); out = (C.c_double * 3)()
    assert lib.ms_warper_rays(7, C.c_float(100), None, R, 1, uv, out) == -1 and "ms_warper_rays" in _err(ms)
    assert lib.ms_warper_rays(2, C.c_float(0), None, R, 1, uv, out) == -1
    assert lib.ms_warper_rays(2, C.c_float(100), None, None, 1, uv, out) == -1
    assert lib.ms_warper_rays(2, C.c_float(100), None, R, 0, uv, out) == -1
    assert lib.ms_warper_rays(2, C.c_float(100), None, R, 1, uv, out) == 0


def test_defaults_and_struct_sizes(ms):
    p = ms.rig_refine_default_params()
    assert (p.struct_size, p.anchor_view, p.huber_rad, p.max_iters, p.step_tol, p.min_pair_matches) == (C.sizeof(ms.RigRefineParams), 0, 0.0, 50, 1e-10, 4)
    assert C.sizeof(ms.RigMatch) == 56 and C.sizeof(ms.RigRefineParams) == 40 and C.sizeof(ms.RigRefineInfo) == 48      # the layouts include/ms_stitch.h declares
    assert ms.load().ms_rig_refine_default_params(None) == -1
    assert (ms.RIG_CONVERGED, ms.RIG_STALLED, ms.RIG_ITERATION_LIMIT) == (rr.CONVERGED, rr.STALLED, rr.ITERATION_LIMIT)


def _call(ms, n_views, R, matches, n, prm, accumulate=False, null=None):
    """the raw entry point with everything valid but what the case breaks; returns (status, message)"""
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    Ra = np.ascontiguousarray(R, np.float64)
    out = np.zeros((max(n_views, 1), 3, 3)); H = np.zeros((3 * max(n_views, 1)) ** 2); g = np.zeros(3 * max(n_views, 1)); cost = C.c_double()
    info = ms.RigRefineInfo()
    arr = ms.rig_matches(matches)
    if accumulate:
        rc = lib.ms_rig_accumulate(n_views, None if null == "R" else Ra.ctypes.data_as(dp), None if null == "matches" else arr, n, C.c_double(prm), None if null == "cost" else C.byref(cost),
                                   None if null == "H" else H.ctypes.data_as(dp), None if null == "g" else g.ctypes.data_as(dp), None)
    else:
        rc = lib.ms_refine_rig_rotations(n_views, None if null == "R" else Ra.ctypes.data_as(dp), None if null == "matches" else arr, n, None if null == "prm" else C.byref(prm),
                                         None if null == "out" else out.ctypes.data_as(dp), C.byref(info), None)
    return rc, _err(ms)


def _valid(n=3):
    rng = np.random.default_rng(9)
    R = rr.ring(n)
    return R, rr.make_matches(rr.perturbed(R, rng, 2.0), rr.ring_pairs(n) if n != 3 else [(0, 1), (1, 2)], 5, rng)


def _with(m, **kw):
    va, vb, a, b = m
    return (kw.get("va", va), kw.get("vb", vb), kw.get("a", a), kw.get("b", b))


BAD_MATCH = {
    "view index out of range": lambda m: _with(m, vb=3),
    "negative view index": lambda m: _with(m, va=-1),
    "view_a == view_b": lambda m: _with(m, vb=m[0]),
    "NaN ray": lambda m: _with(m, a=np.array([np.nan, 0.0, 1.0])),
    "infinite ray": lambda m: _with(m, b=np.array([np.inf, 0.0, 0.0])),
    "ray too long": lambda m: _with(m, a=m[2] * (1.0 + 2e-6)),
    "ray too short": lambda m: _with(m, b=m[3] * (1.0 - 2e-6)),
}


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", sorted(BAD_MATCH))
def test_bad_matches_are_invalid_before_the_device_is_touched(ms, case, accumulate):
    R, M = _valid()
    M[3] = BAD_MATCH[case](M[3])
    rc, msg = _call(ms, 3, R, M, len(M), 0.0 if accumulate else ms.rig_refine_default_params(), accumulate)
    assert rc == -1 and "match 3" in msg, (rc, msg)


@pytest.mark.parametrize("accumulate", [False, True])
def test_bad_counts_and_null_pointers_are_invalid(ms, accumulate):
    R, M = _valid()
    prm = (lambda: 0.0) if accumulate else ms.rig_refine_default_params
    name = "ms_rig_accumulate" if accumulate else "ms_refine_rig_rotations"
    for nv in (1, 0, -3, 17):
        rc, msg = _call(ms, nv, rr.ring(16), M, len(M), prm(), accumulate)
        assert rc == -1 and name in msg and "n_views" in msg, (nv, rc, msg)
    for n in (0, -1, (1 << 20) + 1):
        rc, msg = _call(ms, 3, R, M, n, prm(), accumulate)
        assert rc == -1 and name in msg and "matches" in msg, (n, rc, msg)
    for null in (("R", "matches", "cost", "H", "g") if accumulate else ("R", "matches", "prm", "out")):
        rc, msg = _call(ms, 3, R, M, len(M), prm(), accumulate, null=null)
        assert rc == -1 and "null" in msg, (null, rc, msg)
    # a ray just inside the 1e-6 band passes validation: the next refusal is the missing device (or none with a GPU)
    M[0] = _with(M[0], a=M[0][2] * (1.0 + 5e-7))
    rc, msg = _call(ms, 3, R, M, len(M), prm(), accumulate)
    assert rc in (0, -4), (rc, msg)


def test_bad_params_are_invalid(ms):
    R, M = _valid()
    for field, value, word in (("anchor_view", 3, "anchor"), ("anchor_view", -1, "anchor"), ("struct_size", 44, "struct_size"), ("struct_size", 0, "struct_size"),
                               ("max_iters", 0, "max_iters"), ("huber_rad", -1e-3, "huber_rad"), ("huber_rad", float("nan"), "huber_rad"), ("step_tol", -1.0, "step_tol"),
                               ("min_pair_matches", 0, "min_pair_matches")):
        prm = ms.rig_refine_default_params(**{field: value})
        rc, msg = _call(ms, 3, R, M, len(M), prm)
        assert rc == -1 and word in msg, (field, value, rc, msg)
    rc, msg = _call(ms, 3, R, M, len(M), -1.0, accumulate=True)
    assert rc == -1 and "huber_rad" in msg


def test_a_view_cut_off_from_the_anchor_is_invalid_and_named(ms):
    """host-side, before the device: views 0-1-2 chained, the pair (1, 2) has 3 matches < min_pair_matches"""
    rng = np.random.default_rng(3)
    R = rr.ring(4)
    M = rr.make_matches(R, [(0, 1), (1, 2), (2, 3)], [5, 3, 5], rng)
    rc, msg = _call(ms, 4, R, M, len(M), ms.rig_refine_default_params())
    assert rc == -1 and "view 2 is not connected" in msg and "1 pairs ignored" in msg, (rc, msg)
    rc, msg = _call(ms, 4, R, M, len(M), ms.rig_refine_default_params(anchor_view=3))
    assert rc == -1 and "view 0 is not connected" in msg, (rc, msg)


def test_valid_arguments_without_a_device_fail_loudly(ms):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path is exercised on the CPU-only container")
    R, M = _valid()
    for accumulate in (False, True):
        rc, msg = _call(ms, 3, R, M, len(M), 0.0 if accumulate else ms.rig_refine_default_params(), accumulate)
        assert rc == -4 and "no CPU fallback" in msg, (rc, msg)


def test_refine_rig_context_form_refuses_null_arguments(ms):
    lib = ms.load()
    prm = ms.rig_refine_default_params()
    out = (C.c_float * 18)(); cnt = (C.c_int * 2)(1, 0); m = (ms.MeshMatch * 1)()
    assert lib.ms_refine_rig(None, m, cnt, C.byref(prm), out, None, None) == -1 and "ms_refine_rig" in _err(ms)


def test_reference_terms_are_the_matrix_form():
    """tests/rig_ref.py's explicit per-match terms against J^T r and J^T J with J_i = -[p]x, J_j = +[q]x built as matrices (the two differ by rounding only)"""
    rng = np.random.default_rng(11)
    R = rr.perturbed(rr.ring(3), rng, 5.0)
    M = rr.make_matches(rr.perturbed(rr.ring(3), rng, 5.0), [(0, 1), (2, 1)], 6, rng, noise=1e-3)
    i, j, a, b = rr.unpack(M)
    assert np.all(i < j)
    for h in (0.0, 0.05):
        T, s = rr.terms(R, i, j, a, b, h)
        assert h == 0.0 or (0 < (s > h).sum() < len(s))
        for k in range(len(M)):
            p = R[i[k]] @ a[k]; q = R[j[k]] @ b[k]; r = p - q
            sk = lambda x: np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
            Ji, Jj = -sk(p), sk(q)
            w = 1.0 if h == 0.0 or np.linalg.norm(r) <= h else h / np.linalg.norm(r)
            rho = r @ r if w == 1.0 else 2 * h * np.linalg.norm(r) - h * h
            gi, gj, Hii, Hjj, Hij = [x[0] for x in rr._blocks(T[k:k + 1])]
            for got, want in ((T[k, 0], rho), (gi, w * Ji.T @ r), (gj, w * Jj.T @ r), (Hii, w * Ji.T @ Ji), (Hjj, w * Jj.T @ Jj), (Hij, w * Ji.T @ Jj)):
                assert np.allclose(got, want, rtol=0, atol=1e-14)      # values below 2, a dozen roundings of 2^-53 each between the two forms
