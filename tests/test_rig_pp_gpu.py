"""The rig refinement with every view's principal point free on the GPU (csrc/rig_pp.hip) against the numpy reference of tests/rig_pp_ref.py.

1. ms_rig_pp_accumulate per op: every entry within the bound for two summation orders plus the measured share of libm and the Newton stop
2. bit pins: the 46 sums of rotations and focals are ms_rig_lens_accumulate's bits on pre-shifted pixels; H symmetric; (j, i) is the swapped (i, j); determinism
3. the refinement against the reference: 3 and 6 views, exact and noisy, each lens model, per-view and shared focal, anchors, Huber
4. the largest systems: 16 views, 93 and 78 unknowns
5. the prior
6. stop rules and rejected trials
7. the context form against the array form, and its refusals"""
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded, as in every GPU module of the suite)

import lens_ref as L
import rig_focal_ref as fr
import rig_lens_ref as lr
import rig_pp_ref as pr
import rig_ref as rr
import synth

pytestmark = pytest.mark.gpu

NONE = ("none", (), 0.0)
MODELS = {"none": NONE, "fisheye": L.FISH, "brown": L.BROWN}


def to_lenses(ms, lenses):
    return [L.to_ms(ms, l) if l[0] != "none" else None for l in lenses]


def device_refine(ms, f_in, R_in, pp_in, lenses, M, **kw):
    kw = {{"anchor": "anchor_view"}.get(k, k): (int(v) if k == "shared_focal" else v) for k, v in kw.items()}
    return ms.refine_rig_pp(f_in, R_in, pp_in, to_lenses(ms, lenses), M, ms.rig_pp_default_params(**kw))


_REF = {}


def ref_refine(key, f_in, R_in, pp_in, lenses, M, **kw):
    """the reference's answer for a named case, computed once"""
    if key not in _REF:
        _REF[key] = pr.refine(f_in, R_in, pp_in, lenses, M, **kw)
    return _REF[key]


def gaps(f, R, pp, rf, rR, rpp):
    """rotation entries, relative focals, centre offsets divided by the focal"""
    return float(np.max(np.abs(R - rR))), float(np.max(np.abs(f / rf - 1.0))), float(np.max(np.abs(pp - rpp) / np.asarray(rf)[:, None]))


# ---- 1. accumulate, per op --------------------------------------------------------------------------------------------------------------------------
def accumulate_case(m, lens):
    """2 views behind `lens`, one pair with m matches, offsets of several pixels, a third of the matches listed as (1, 0); the Huber threshold is the median residual"""
    rng = np.random.default_rng(700 + m)
    R = rr.perturbed(rr.ring(6)[:2], rng, 5.0)
    f = np.array([400.0, 431.5])
    pp = np.array([[9.5, -6.25], [-4.0, 12.75]])
    M = pr.make_pp_matches(f * (1 + rng.uniform(-0.03, 0.03, 2)), rr.perturbed(rr.ring(6)[:2], rng, 5.0), pp + rng.uniform(-2, 2, (2, 2)), [lens] * 2, [(0, 1)], m, rng,
                           noise_px=0.7)
    M = [(vb, va, b, a) if rng.uniform() < 1 / 3 else (va, vb, a, b) for va, vb, a, b in M]
    i, j, a, b = fr.unpack(M)
    s = pr.terms(f, R, pp, [lens] * 2, i, j, a, b, 0.0)[1]
    return f, R, pp, M, float(np.sort(s)[(len(s) - 1) // 2])


@pytest.mark.parametrize("m", [1, 64, 65, 257])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_accumulate_per_op(ms, cuda, model, m):
    """2 views, m = 1, 64, 65, 257 matches (the wave and workgroup edges of k_rig_accum), each lens model, Huber off and at the median residual, non-zero offsets.
    Bound per entry of cost, H and g: ((m + 8) + T) 2^-52 S, S the reference's sum of the terms' absolute values: the siblings' bound and reason ((m + 8) for two
    summation orders of the same rounded terms; T = 8 times the deviation rig_pp_ref.term_deviation measures between float64 and longdouble terms, for libm, hypot and
    the Newton stop; measured against the reference, never the device).  Measured on the CPU (profiles/rig_pp.jsonl, "term_deviation"), smallest to largest deviation
    over the four m and both Huber settings: none 3.1 to 46.6; brown 8.2 to 828.2 (m = 1: one match, entries that
    nearly cancel); fisheye 5.6 to 65.2."""
    lens = MODELS[model]
    lenses = [lens] * 2
    f, R, pp, M, h_mid = accumulate_case(m, lens)
    assert any(va > vb for va, vb, _, _ in M) or m == 1
    assert pr.all_seen(f, R, pp, lenses, M)
    for h in (0.0, h_mid):
        dev = pr.term_deviation(f, R, pp, lenses, M, h)
        T = 8.0 * dev
        cost, H, g = ms.rig_pp_accumulate(f, R, pp, to_lenses(ms, lenses), M, h)
        rc, rH, rg, sc, sH, sg = pr.accumulate(f, R, pp, lenses, M, h, with_abs=True)
        tol = ((m + 8) + T) * 2.0 ** -52
        print("%s m=%d h=%g: term deviation %.1f, T %.1f; cost %.3e of %.3e, H %.3e, g %.3e (max |diff| / S)" % (model, m, h, dev, T, abs(cost - rc) / sc, tol,
              np.max(np.abs(H - rH) / np.maximum(sH, 1e-300)), np.max(np.abs(g - rg) / np.maximum(sg, 1e-300))))
        assert H.shape == (12, 12) and g.shape == (12,)
        assert abs(cost - rc) <= tol * sc
        assert np.all(np.abs(H - rH) <= tol * sH) and np.all(np.abs(g - rg) <= tol * sg)
        assert H.all() and g.all()


# ---- 2. bit pins ------------------------------------------------------------------------------------------------------------------------------------
def pin_case(lenses, zero):
    n = len(lenses)
    rng = np.random.default_rng(41 + n)
    R = rr.perturbed(rr.ring(6)[:n], rng, 4.0)
    f = 400.0 * (1 + rng.uniform(-0.05, 0.05, n))
    pp = np.zeros((n, 2)) if zero else rng.uniform(-14, 14, (n, 2))
    pairs = [(v, v + 1) for v in range(n - 1)]
    M = pr.make_pp_matches(f * (1 + rng.uniform(-0.02, 0.02, n)), rr.perturbed(rr.ring(6)[:n], rng, 4.0), pp, lenses, pairs, [130, 7, 64][:n - 1], rng, noise_px=0.5)
    M = [M[k] for k in rng.permutation(len(M))]
    return f, R, pp, M


@pytest.mark.parametrize("zero", [True, False], ids=["zero-offsets", "offsets"])
@pytest.mark.parametrize("name", ["mixed", "all-none", "null-lenses"])
def test_the_46_sums_are_the_lens_forms_bits(ms, cuda, name, zero):
    """the cost and the sums over rotations and focals (rows 6v .. 6v + 3 of every view) are ms_rig_lens_accumulate's bits on matches whose pixels had the offsets
    subtracted in double beforehand; H is symmetric bit for bit; a match listed as (j, i) gives the bits of the swapped (i, j); two calls return the same bits"""
    lenses = {"mixed": [L.FISH, NONE, L.BROWN, L.FISH], "all-none": [NONE] * 3, "null-lenses": [NONE] * 3}[name]
    n = len(lenses)
    f, R, pp, M = pin_case(lenses, zero)
    ml = to_lenses(ms, lenses)
    rows = pr.view_rows(n)
    for h in (0.0, 0.6):
        cost, H, g = ms.rig_pp_accumulate(f, R, pp, None if name == "null-lenses" else ml, M, h)
        lc, lH, lg = ms.rig_lens_accumulate(f, R, ml, pr.shift(M, pp), h)
        assert cost == lc and H[np.ix_(rows, rows)].tobytes() == lH.tobytes() and g[rows].tobytes() == lg.tobytes()
        assert np.array_equal(H, H.T) and H[4:6, :12].all() and g[4:6].all()
        sw = [(vb, va, b, a) if k % 3 == 0 else (va, vb, a, b) for k, (va, vb, a, b) in enumerate(M)]
        c2, H2, g2 = ms.rig_pp_accumulate(f, R, pp, None if name == "null-lenses" else ml, sw, h)
        assert c2 == cost and H2.tobytes() == H.tobytes() and g2.tobytes() == g.tobytes()
        c3, H3, g3 = ms.rig_pp_accumulate(f, R, pp, None if name == "null-lenses" else ml, M, h)
        assert c3 == cost and H3.tobytes() == H.tobytes() and g3.tobytes() == g.tobytes()


# ---- 3. the refinement against the reference --------------------------------------------------------------------------------------------------------
# name: views, lens model(s), noise in pixels, outlier fraction, Huber threshold, shared focal, anchor
CASES = {
    "3-exact-none": dict(n=3, lens="none", noise=0.0, out=0.0, huber=0.0, shared=False, anchor=0),
    "3-exact-fisheye-shared": dict(n=3, lens="fisheye", noise=0.0, out=0.0, huber=0.0, shared=True, anchor=2),
    "3-noisy-brown": dict(n=3, lens="brown", noise=0.02, out=0.0, huber=0.0, shared=False, anchor=1),
    "6-exact-brown": dict(n=6, lens="brown", noise=0.0, out=0.0, huber=0.0, shared=False, anchor=0),
    "6-exact-mixed-shared": dict(n=6, lens="mixed", noise=0.0, out=0.0, huber=0.0, shared=True, anchor=3),
    "6-noisy-none-huber": dict(n=6, lens="none", noise=0.02, out=0.15, huber=0.1, shared=False, anchor=4),
    "6-noisy-fisheye-huber-shared": dict(n=6, lens="fisheye", noise=0.02, out=0.15, huber=0.1, shared=True, anchor=0),
    "6-noisy-mixed": dict(n=6, lens="mixed", noise=0.02, out=0.0, huber=0.0, shared=False, anchor=2),
}
MIXED = [L.FISH, L.FISH, L.BROWN, NONE, L.BROWN, L.FISH]


def refine_case(name):
    """n views of the 6-ring (3: the chain 0-1-2; 6: the closed ring), 64 matches a pair through true cameras whose centres are up to 12 px off, focals 2 % (shared:
    3 %) and rotations 1 degree off; the start: the ideal ring, the nominal focal, offsets 0"""
    c = CASES[name]
    n = c["n"]
    rng = np.random.default_rng(sorted(CASES).index(name) + 900)
    lenses = MIXED[:n] if c["lens"] == "mixed" else [MODELS[c["lens"]]] * n
    R0 = rr.ring(6)[:n].copy(); Rt = rr.perturbed(R0, rng, 1.0)
    ft = np.full(n, 412.0) if c["shared"] else 400.0 * (1 + rng.uniform(-0.02, 0.02, n))
    ppt = rng.uniform(-12, 12, (n, 2))
    pairs = rr.ring_pairs(6) if n == 6 else [(0, 1), (1, 2)]
    M = pr.make_pp_matches(ft, Rt, ppt, lenses, pairs, 64, rng, noise_px=c["noise"], outlier_frac=c["out"], spread_deg=25.0)
    kw = dict(huber_px=c["huber"], shared_focal=c["shared"], anchor=c["anchor"], step_tol=1e-13 if c["noise"] == 0 else 1e-12, max_iters=100)
    return np.full(n, 400.0), R0, np.zeros((n, 2)), lenses, M, kw, ft, Rt, ppt


@pytest.mark.parametrize("name", sorted(CASES))
def test_refinement_against_the_reference(ms, cuda, name):
    """Device and reference within 1e-10 in rotation entries, relative focals and centre offsets divided by the focal (the project's bound for the sibling
    refinements); on exact matches no further from the truth than 4 times the reference's own error plus 1e-12; the anchor's R is its input's bits; with a shared focal
    every focal is one double; cost_final <= cost_initial; every returned camera sees every match.
    The cases were chosen on the CPU so that the reference under two summation orders (the matches as given, and reversed) stays inside 1e-10: the largest gap of
    the three figures over these eight cases is 2.9e-12 (3-noisy-brown; the 3-view chain constrains its centres least); profiles/rig_pp.jsonl, "two_orders"."""
    f0, R0, p0, lenses, M, kw, ft, Rt, ppt = refine_case(name)
    exact = CASES[name]["noise"] == 0
    rf, rR, rpp, ri = ref_refine(name, f0, R0, p0, lenses, M, **kw)
    f, R, pp, info = device_refine(ms, f0, R0, p0, lenses, M, **kw)
    d = gaps(f, R, pp, rf, rR, rpp)
    print("%s: device to reference %.3e rotation, %.3e focal, %.3e centre / f; cost %.6e -> %.6e (reference %.6e); iterations %d (%d), stop %d (%d), outliers %d (%d), "
          "centres moved %.3f px" % ((name,) + d + (info["cost_initial"], info["cost_final"], ri["cost_final"], info["iterations"], ri["iterations"], info["stop_reason"],
                                                    ri["stop_reason"], info["outliers"], ri["outliers"], info["max_pp_shift"])))
    assert max(d) <= 1e-10
    a = kw["anchor"]
    if exact:
        assert ri["stop_reason"] == fr.CONVERGED and ri["iterations"] < 100, ri
        want = rr.expected(R0, Rt, a)
        err = gaps(f, R, pp, ft, want, ppt); ref_err = gaps(rf, rR, rpp, ft, want, ppt)
        print("    to the truth %.3e, %.3e, %.3e (reference %.3e, %.3e, %.3e)" % (err + ref_err))
        assert all(e <= 4.0 * r + 1e-12 for e, r in zip(err, ref_err))
    assert info["cost_final"] <= info["cost_initial"]
    assert abs(info["outliers"] - ri["outliers"]) <= 2 and (CASES[name]["huber"] == 0 or info["outliers"] > 0)
    assert info["matches_used"] == ri["matches_used"] == len(M) and info["pairs_used"] == ri["pairs_used"]
    assert R[a].tobytes() == np.asarray(R0)[a].tobytes() and (not kw["shared_focal"] or np.all(f == f[0]))
    assert pr.all_seen(f, R, pp, lenses, M) and info["max_pp_shift"] == float(np.max(np.abs(pp - p0))) and info["max_pp_shift"] > 1.0


# ---- 4. the largest systems -------------------------------------------------------------------------------------------------------------------------
def sixteen_case(shared):
    """16 views on the ring with the 16 neighbour pairs, 40 matches a pair, lenses of all three models in turn; noise 0.001 px
    (at 0.01 px the reference's two summation orders end 2e-10 apart: the accept rule is then decided by the cost's rounding).  Per-view focals: 6 * 16 - 3 = 93
    unknowns; shared: 5 * 16 - 2 = 78, anchor 5"""
    rng = np.random.default_rng(160 + shared)
    lenses = [(L.FISH, NONE, L.BROWN)[v % 3] for v in range(16)]
    R0 = rr.ring(16).copy(); Rt = rr.perturbed(R0, rng, 0.5)
    ft = np.full(16, 409.0) if shared else 400.0 * (1 + rng.uniform(-0.02, 0.02, 16))
    ppt = rng.uniform(-10, 10, (16, 2))
    M = pr.make_pp_matches(ft, Rt, ppt, lenses, rr.ring_pairs(16), 40, rng, noise_px=0.001, spread_deg=20.0)
    return np.full(16, 400.0), R0, np.zeros((16, 2)), lenses, M, dict(shared_focal=bool(shared), anchor=5 if shared else 0, step_tol=1e-12, max_iters=100)


@pytest.mark.parametrize("shared", [False, True], ids=["per-view-93", "shared-78"])
def test_sixteen_views_the_largest_systems(ms, cuda, shared):
    """the step kernel at full size: its launch, the packed triangle of the 96 x 96 system, the fold of 16 focal rows.  Within 1e-10 of the reference, whose two
    summation orders agree to 3.7e-12 here (measured on the CPU; profiles/rig_pp.jsonl, "two_orders")"""
    f0, R0, p0, lenses, M, kw = sixteen_case(shared)
    rf, rR, rpp, ri = ref_refine(("sixteen", shared), f0, R0, p0, lenses, M, **kw)
    f, R, pp, info = device_refine(ms, f0, R0, p0, lenses, M, **kw)
    d = gaps(f, R, pp, rf, rR, rpp)
    print("16 views shared=%s: device to reference %.3e, %.3e, %.3e; cost %.6e -> %.6e (reference %.6e), iterations %d (%d), stop %d (%d)" % ((shared,) + d + (
        info["cost_initial"], info["cost_final"], ri["cost_final"], info["iterations"], ri["iterations"], info["stop_reason"], ri["stop_reason"])))
    assert max(d) <= 1e-10
    assert info["pairs_used"] == 16 and info["matches_used"] == 640 and info["cost_final"] <= 1e-3 * info["cost_initial"]
    assert R[kw["anchor"]].tobytes() == R0[kw["anchor"]].tobytes() and (not shared or np.all(f == f[0])) and info["max_pp_shift"] > 5.0


# ---- 5. the prior -----------------------------------------------------------------------------------------------------------------------------------
def four_ring_case():
    """the weakly constrained rig: 4 fisheye views 90 degrees apart with the four neighbour pairs (the fields overlap widely); noise 0.01 px, true centres up to
    12 px off, input offsets of up to 2 px"""
    rng = np.random.default_rng(12)
    lenses = [L.FISH] * 4
    R0 = rr.ring(4).copy(); Rt = rr.perturbed(R0, rng, 1.0)
    ft = 400.0 * (1 + rng.uniform(-0.02, 0.02, 4))
    ppt = rng.uniform(-12, 12, (4, 2))
    M = pr.make_pp_matches(ft, Rt, ppt, lenses, rr.ring_pairs(4), 48, rng, noise_px=0.01, spread_deg=25.0)
    return np.full(4, 400.0), R0, rng.uniform(-2, 2, (4, 2)), lenses, M


def test_a_heavy_prior_holds_the_centres(ms, cuda):
    """pp_prior = 1e12: pp_out is pp_in to 1e-9 px while the focals and rotations still move"""
    f0, R0, p0, lenses, M = four_ring_case()
    f, R, pp, info = device_refine(ms, f0, R0, p0, lenses, M, pp_prior=1e12, step_tol=1e-12, max_iters=100)
    print("w = 1e12: centres moved %.3e px, focal ratio %.6f, rotation %.3e rad, cost %.4e -> %.4e, %d iterations" % (info["max_pp_shift"], info["max_focal_ratio"],
          info["max_rotation_rad"], info["cost_initial"], info["cost_final"], info["iterations"]))
    assert float(np.max(np.abs(pp - p0))) <= 1e-9 and info["max_pp_shift"] <= 1e-9
    assert info["max_focal_ratio"] > 1.001 and info["max_rotation_rad"] > 1e-3 and info["cost_final"] < info["cost_initial"]


@pytest.mark.parametrize("w", [1e-2, 1.0])
def test_a_prior_on_a_four_view_ring_against_the_reference(ms, cuda, w):
    """the device's prior is the reference's: the total cost, the two diagonal entries and the two entries of g a view.  The reference moves the centres 10.8 px at w = 0.01 and 8.1 px at
    w = 1 (11.0 px without a prior); its two summation orders end 2.8e-13 and 4.7e-12 apart (profiles/rig_pp.jsonl, "two_orders")"""
    f0, R0, p0, lenses, M = four_ring_case()
    kw = dict(pp_prior=w, step_tol=1e-12, max_iters=100)
    rf, rR, rpp, ri = ref_refine(("prior", w), f0, R0, p0, lenses, M, **kw)
    f, R, pp, info = device_refine(ms, f0, R0, p0, lenses, M, **kw)
    d = gaps(f, R, pp, rf, rR, rpp)
    print("w = %g: device to reference %.3e, %.3e, %.3e; cost %.6e -> %.6e (reference %.6e); centres moved %.3f px (%.3f); iterations %d (%d)" % ((w,) + d + (
        info["cost_initial"], info["cost_final"], ri["cost_final"], info["max_pp_shift"], ri["max_pp_shift"], info["iterations"], ri["iterations"])))
    assert max(d) <= 1e-10
    assert abs(info["cost_final"] - ri["cost_final"]) <= 1e-9 * ri["cost_final"] and info["cost_final"] <= info["cost_initial"]
    assert info["cost_initial"] == pytest.approx(ri["cost_initial"], rel=1e-12)


# ---- 6. stop rules and rejected trials --------------------------------------------------------------------------------------------------------------
def test_one_iteration_ends_at_the_iteration_limit(ms, cuda):
    f0, R0, p0, lenses, M, kw, _, _, _ = refine_case("6-noisy-mixed")
    kw = dict(kw, max_iters=1)
    f, R, pp, info = device_refine(ms, f0, R0, p0, lenses, M, **kw)
    rf, rR, rpp, ri = ref_refine("one-iteration", f0, R0, p0, lenses, M, **kw)
    assert info["iterations"] == 1 and info["stop_reason"] == fr.ITERATION_LIMIT == ri["stop_reason"]
    assert info["cost_final"] <= info["cost_initial"] and max(gaps(f, R, pp, rf, rR, rpp)) <= 1e-10
    assert info["cost_final"] < info["cost_initial"] and info["max_pp_shift"] > 0.0          # the one trial was accepted and is what comes back


def edge_case():
    """tests/test_rig_lens_gpu.py's edge_case with the centres free: 3 fisheye views, exact matches of cameras whose shared focal is 400, the start at 420; one more
    match has its pixel in view 0 at 1 - 1e-4 of the field's end AT the focal 420 and the offset 0: the first proposal, which lowers the focal, loses it"""
    rng = np.random.default_rng(77)
    lenses = [L.FISH] * 3
    R0 = rr.ring(6)[:3].copy(); Rt = rr.perturbed(R0, rng, 1.0)
    M = lr.make_lens_matches(np.full(3, 400.0), Rt, lenses, [(0, 1), (1, 2)], 30, rng, spread_deg=15.0)
    a = 420.0 * float(lr.limit(L.FISH)) * (1.0 - 1e-4) * np.array([math.cos(0.3), math.sin(0.3)])
    ray, seen = lr.unproject(np.diag([420.0, 420.0, 1.0]), L.FISH, a[0], a[1])
    assert seen[0]
    b, seen = lr.centred_pixels(420.0, L.FISH, (R0[1].T @ R0[0] @ ray[0])[None, :])
    assert seen[0]
    return np.full(3, 420.0), R0, np.zeros((3, 2)), lenses, M + [(0, 1, a, b[0])]


def test_a_trial_that_loses_a_rim_pixel_is_rejected(ms, cuda):
    f0, R0, p0, lenses, M = edge_case()
    assert pr.all_seen(f0, R0, p0, lenses, M)
    # the precondition, on the CPU: the reference's first proposal does move the pixel out
    P = pr.selection(3, 0, True)
    _, H, g = pr.accumulate(f0, R0, p0, lenses, M)
    Hr = P.T @ H @ P
    delta = np.linalg.solve(Hr + 1e-3 * np.diag(np.diag(Hr)), -(P.T @ g))
    ft, Rt, pt = pr.apply_step(f0, R0, p0, P @ delta)
    assert not pr.all_seen(ft, Rt, pt, lenses, M)
    f, R, pp, info = device_refine(ms, f0, R0, p0, lenses, M, shared_focal=True)
    print("focal %.6f, offsets of view 0 (%.4f, %.4f), cost %.6e -> %.6e, %d iterations, stop %d" % (f[0], pp[0, 0], pp[0, 1], info["cost_initial"], info["cost_final"],
          info["iterations"], info["stop_reason"]))
    assert info["cost_final"] <= info["cost_initial"] and math.isfinite(info["cost_final"])
    assert pr.all_seen(f, R, pp, lenses, M)


def test_two_calls_return_the_same_bits(ms, cuda):
    f0, R0, p0, lenses, M, kw, _, _, _ = refine_case("6-noisy-fisheye-huber-shared")
    a = device_refine(ms, f0, R0, p0, lenses, M, **kw)
    b = device_refine(ms, f0, R0, p0, lenses, M, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]


# ---- 7. the context form ----------------------------------------------------------------------------------------------------------------------------
CTX_N, CTX_W, CTX_H = 4, 64, 48
CTX_LENS = ("brown", (-0.1, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), 0.0)
CTX_ASPECT = 1.125


def ctx_camera(v, skew=False):
    """view v of the 6-ring at 64 x 48, the principal point off the middle of the image, K[4] = 1.125 K[0]"""
    K, R0 = synth.camera(6, CTX_W, CTX_H, 90.0, v)
    K[0][2] += 1.5 + 0.25 * v; K[1][2] -= 1.0 + 0.5 * v; K[1][1] = K[0][0] * CTX_ASPECT
    if skew:
        K[0][1] = 0.5
    return K, R0


def small_rig(ms, lens, build=True, skew=None):
    comp = ms.Compositor(CTX_N, (CTX_W, CTX_H), ms.PROJ_SPHERICAL, synth.warp_scale(128), num_bands=2, out_size=(128, 64))
    for v in range(CTX_N):
        K, R0 = ctx_camera(v, skew == v)
        if lens is not None:
            comp.set_lens(v, L.to_ms(ms, lens))
        comp.set_camera(v, K, R0)
    if build:
        comp.build_maps()
    return comp


def fabricate_lists(comp, lens, rng, per_pair=14):
    """tests/test_rig_lens_gpu.py's fabricate_lists for a scene whose cameras differ from the context's in rotation (1 degree), focal (4 %) AND centre (up to 2.5 px):
    a world ray's centred source pixel through the TRUE camera, moved by the true offset, shows up in the warped view where the CONTEXT's camera puts that pixel.
    Returns the lists and the same matches as centred source pixels at the context's cameras in float64 (numpy formulas on the float positions the lists hold)."""
    lens_t = lens if lens is not None else NONE
    scale = float(np.float32(comp.cfg.warp_scale))
    R0 = np.array([ctx_camera(v)[1] for v in range(CTX_N)], np.float64)
    f_ctx = float(ctx_camera(0)[0][0][0])
    Rt = rr.perturbed(R0, rng, 1.0)
    ppt = rng.uniform(-2.5, 2.5, (CTX_N, 2))
    corner = [comp.view_geom(v).roi.tuple()[:2] for v in range(CTX_N)]
    Kc = np.diag([f_ctx, f_ctx, 1.0])
    lists = [[] for _ in range(CTX_N)]
    px = []

    def back(v, x, y):
        ray = rr.warper_ray(rr.SPHERICAL, scale, R0[v], corner[v][0] + float(x), corner[v][1] + float(y))
        p, seen = lr.centred_pixels(f_ctx, lens_t, np.asarray(ray, np.float64)[None, :])
        assert seen[0]
        return p[0]

    for i, j in [(v, v + 1) for v in range(CTX_N - 1)]:
        mid = Rt[i][:, 2] + Rt[j][:, 2]
        mid /= np.linalg.norm(mid)
        for _ in range(per_pair):
            d = rr.exp_so3(np.radians(rng.uniform(-12, 12, 3))) @ mid
            pos = []
            for v in (i, j):
                src, seen = lr.centred_pixels(f_ctx / 1.04, lens_t, (Rt[v].T @ d)[None, :])
                ray, seen2 = lr.unproject(Kc, lens_t, src[0, 0] + ppt[v, 0], src[0, 1] + ppt[v, 1])
                assert seen[0] and seen2[0]
                u, w = rr.warper_forward(rr.SPHERICAL, scale, R0[v] @ ray[0])
                pos += [np.float32(u - corner[v][0]), np.float32(w - corner[v][1])]
            lists[i].append((pos[0], pos[1], pos[2], pos[3], j))
            px.append((i, j, back(i, pos[0], pos[1]), back(j, pos[2], pos[3])))
    return lists, [m for v in range(CTX_N) for m in px if m[0] == v], R0, f_ctx


@pytest.mark.parametrize("kind", ["analytic", "lens"])
def test_context_form_is_the_array_form_on_its_pixels(ms, cuda, kind):
    """4 views of 64 x 48 with K[2], K[5] off the middle and K[4] = 1.125 K[0], analytic and behind one BROWN lens: focal_out, pp_out and R_out are the array form's on
    the centred pixels the test forms itself (equal to the context's to 1e-9 px), pp_in = 0, with pp_out = (K[2] + ox, K[5] + oy K[4] / K[0]); a prior of 0.01 holds
    the chain's centres.  Agreement to 1e-9 (relative focal, pixels; rotations after the rounding to float both undergo).  Nothing is applied to the context."""
    lens = CTX_LENS if kind == "lens" else None
    rng = np.random.default_rng(23)
    comp = small_rig(ms, lens)
    assert comp.map_source() == (ms.MAPS_LENS if lens else ms.MAPS_ANALYTIC)
    lists, px, R0, f_ctx = fabricate_lists(comp, lens, rng)
    prm = ms.rig_pp_default_params(pp_prior=1e-2, max_iters=100)
    f, pp, R, info = comp.refine_rig_pp(lists, prm)
    assert f.dtype == np.float64 and pp.dtype == np.float64 and pp.shape == (CTX_N, 2) and R.dtype == np.float32
    assert info["matches_used"] == 42 and info["pairs_used"] == 3
    lenses = [lens if lens else NONE] * CTX_N
    fa, Ra, pa, ia = ms.refine_rig_pp(np.full(CTX_N, f_ctx), R0, np.zeros((CTX_N, 2)), to_lenses(ms, lenses), px, prm)
    K = [np.asarray(ctx_camera(v)[0], np.float64) for v in range(CTX_N)]
    want = np.array([[K[v][0, 2] + pa[v, 0], K[v][1, 2] + pa[v, 1] * K[v][1, 1] / K[v][0, 0]] for v in range(CTX_N)])
    d = float(np.max(np.abs(R.astype(np.float64) - Ra.astype(np.float32).astype(np.float64)))); df = float(np.max(np.abs(f / fa - 1.0))); dp = float(np.max(np.abs(pp - want)))
    print("%s context against array form: %.3e rotation, %.3e relative focal, %.3e px; centres %s; focals %s; cost %.3e -> %.3e, %d iterations" % (kind, d, df, dp,
          np.round(pp, 3).tolist(), np.round(f, 3).tolist(), info["cost_initial"], info["cost_final"], info["iterations"]))
    assert d <= 1e-9 and df <= 1e-9 and dp <= 1e-9
    assert info["cost_final"] <= info["cost_initial"] and info["iterations"] >= 2 and ia["max_pp_shift"] > 0.1
    assert abs(info["max_pp_shift"] - ia["max_pp_shift"]) <= 1e-9
    again = comp.refine_rig_pp(lists, prm)                    # nothing was applied: the same call returns the same bits
    assert again[0].tobytes() == f.tobytes() and again[1].tobytes() == pp.tobytes() and again[2].tobytes() == R.tobytes() and again[3] == info
    comp.close()


def test_context_form_state_and_refusals(ms, cuda):
    lists = [[(8.0 + 3 * q, 10.0 + 5 * q, 12.0 + 2 * q, 14.0 + q, (v + 1) % CTX_N) for q in range(4)] for v in range(CTX_N)]
    comp = small_rig(ms, CTX_LENS, build=False)
    with pytest.raises(ms.MsError, match="-5.*ms_build_maps first"):         # MS_ERR_STATE
        comp.refine_rig_pp(lists)
    comp.build_maps()
    f, pp, R, info = comp.refine_rig_pp(lists, ms.rig_pp_default_params(pp_prior=1.0))
    assert info["cost_final"] <= info["cost_initial"]
    with pytest.raises(ms.MsError, match="-1.*names view"):
        comp.refine_rig_pp([[(10.0, 20.0, 30.0, 40.0, v)] * 4 for v in range(CTX_N)])
    with pytest.raises(ms.MsError, match="-1.*pp_prior"):
        comp.refine_rig_pp(lists, ms.rig_pp_default_params(pp_prior=-1.0))
    # a pixel half a turn along the warper's u axis shows what lies behind the camera: past the lens's 89 degrees
    behind = [list(l) for l in lists]
    behind[2][1] = (10.0 + math.pi * comp.cfg.warp_scale, 20.0, 30.0, 40.0, 3)
    with pytest.raises(ms.MsError, match="-1.*match 1 of view 2.*does not see"):
        comp.refine_rig_pp(behind)
    # a context on the caller's own maps has no cameras
    rois = [comp.view_geom(v).roi.tuple() for v in range(CTX_N)]
    maps = [comp.maps(v) for v in range(CTX_N)]
    twin = ms.Compositor(CTX_N, (CTX_W, CTX_H), ms.PROJ_SPHERICAL, synth.warp_scale(128), num_bands=2, out_size=(128, 64))
    twin.set_maps(rois, [m[0].clone() for m in maps], [m[1].clone() for m in maps])
    assert twin.map_source() == ms.MAPS_CUSTOM
    with pytest.raises(ms.MsError, match="-2.*ms_set_maps"):                 # MS_ERR_UNSUPPORTED
        twin.refine_rig_pp(lists)
    # centred pixels carry no skew
    skew = small_rig(ms, CTX_LENS, skew=3)
    with pytest.raises(ms.MsError, match=r"-2.*view 3.*K\[1\]"):
        skew.refine_rig_pp(lists)
    skew.close(); twin.close(); comp.close()
