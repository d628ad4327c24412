"""The rig refinement with the shared lens's coefficients free on the GPU (csrc/rig_coeffs.hip) against the numpy reference of tests/rig_coeff_ref.py.

1. ms_rig_coeff_accumulate per op: every entry within the bound for two summation orders plus the measured share of libm and the Newton stop; the cost and the
   views' block are the bits of ms_rig_lens_accumulate
2. exact recovery of two coefficients, focals and rotations from coefficients at zero, fisheye (rays to the rim) and Brown, per-view and shared focal
3. noise and outliers with Huber against the reference
4. a trial lens whose profile folds back is rejected on the device
5. size edges: 2 views; 16 views on the complete graph with four free coefficients (65 unknowns), per-view and shared focal
6. determinism
7. the context form against the array form, and its refusals"""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded, as in every GPU module of the suite)

import lens_ref as L
import rig_coeff_ref as cr
import rig_focal_ref as fr
import rig_lens_ref as lr
import rig_ref as rr
import synth

pytestmark = pytest.mark.gpu

K1, K2, P1, P2, K3 = 1, 2, 4, 8, 16         # free_coeffs bits (OpenCV's order k1 k2 p1 p2 k3; the fisheye's k3, k4 are bits 2, 3)


def lens_tuple(ml):
    return ("brown" if ml.model == 1 else "fisheye", tuple(ml.k[q] for q in range(8 if ml.model == 1 else 4)), ml.max_theta_deg)


def device_refine(ms, f_in, R_in, lens, free, M, **kw):
    kw = {{"anchor": "anchor_view"}.get(k, k): (int(v) if k == "shared_focal" else v) for k, v in kw.items()}
    f, R, ml, info = ms.refine_rig_coeffs(f_in, R_in, L.to_ms(ms, lens), M, ms.rig_coeff_default_params(free_coeffs=free, **kw))
    assert ms.load().ms_lens_check(C.byref(ml)) == 0, "the returned lens does not pass ms_lens_check"
    return f, R, lens_tuple(ml), info


def max_angle(A, B):
    return max(rr.angle(a, b) for a, b in zip(A, B))


def coeff_gap(la, lb, free):
    """the largest difference of a free coefficient, coefficient n scaled by max_theta^(2n+2), its effect at the rim (Brown: tan max_theta, powers 2, 4, 2, 2, 6 of
    k1 k2 p1 p2 k3)"""
    fish = la[0] == "fisheye"
    rim = L.max_theta(la) if fish else math.tan(L.max_theta(la))
    power = (lambda b: 2 * b + 2) if fish else (lambda b: {0: 2, 1: 4, 2: 2, 3: 2, 4: 6}[b])
    return max(abs(cr.k8(la)[b] - cr.k8(lb)[b]) * rim ** power(b) for b in cr.free_list(free))


_REF = {}


def ref_refine(key, f_in, R_in, lens, free, M, **kw):
    """the reference's answer for a named case, computed once"""
    if key not in _REF:
        _REF[key] = cr.refine(f_in, R_in, lens, free, M, **kw)
    return _REF[key]


def against_the_reference(ms, key, f0, R0, lens, free, M, kw, huber=True):
    """what tests 3 and 5 ask: within 1e-10 of the reference in rotations, relative focals and scaled coefficients, outliers within 2, cost_final <= cost_initial"""
    rf, rR, rl, ri = ref_refine(key, f0, R0, lens, free, M, **kw)
    f, R, lo, info = device_refine(ms, f0, R0, lens, free, M, **kw)
    d = max_angle(R, rR); df = float(np.max(np.abs(f / rf - 1.0))); dk = coeff_gap(lo, rl, free)
    print("%s: %.3e rad, %.3e relative focal, %.3e scaled coefficient between device and reference; cost %.6e -> %.6e (reference %.6e); outliers %d (%d); iterations "
          "%d (%d), stop %d (%d); k %s" % (key, d, df, dk, info["cost_initial"], info["cost_final"], ri["cost_final"], info["outliers"], ri["outliers"], info["iterations"],
                                            ri["iterations"], info["stop_reason"], ri["stop_reason"], [cr.k8(lo)[b] for b in cr.free_list(free)]))
    assert d <= 1e-10 and df <= 1e-10 and dk <= 1e-10
    assert info["cost_final"] <= info["cost_initial"]
    assert abs(info["outliers"] - ri["outliers"]) <= 2 and (not huber or info["outliers"] > 0)
    assert info["matches_used"] == ri["matches_used"] and info["pairs_used"] == ri["pairs_used"]
    a = kw.get("anchor", 0)
    assert R[a].tobytes() == np.asarray(R0)[a].tobytes()
    assert cr.all_seen(f, R, lo, M)
    assert abs(info["max_coeff_change"] - max(abs(cr.k8(lo)[b] - cr.k8(lens)[b]) for b in cr.free_list(free))) <= 1e-300
    return f, R, lo, info, ri


# ---- 1. accumulate, per op --------------------------------------------------------------------------------------------------------------------------
ACC = {"fish-k1": (L.FISH, K1), "fish-k1234": (L.FISH, 0b1111), "brown-k1": (L.BROWN, K1), "brown-k1k2p1p2": (L.BROWN, K1 | K2 | P1 | P2), "brown-k1k2k3": (L.BROWN, K1 | K2 | K3)}


def accumulate_case(m, lens):
    """tests/test_rig_lens_gpu.py's accumulate_case with the one lens on the three views"""
    rng = np.random.default_rng(600 + m)
    R = rr.perturbed(rr.ring(6)[:3], rng, 5.0)
    f = np.array([400.0, 431.5, 388.25])
    M = lr.make_lens_matches(f * (1 + rng.uniform(-0.03, 0.03, 3)), rr.perturbed(rr.ring(6)[:3], rng, 5.0), [lens] * 3, [(0, 1), (1, 2)], [m, 5], rng, noise_px=0.7)
    M = [M[k] for k in rng.permutation(len(M))]
    M = [(vb, va, b, a) if rng.uniform() < 1 / 3 else (va, vb, a, b) for va, vb, a, b in M]
    i, j, a, b = fr.unpack(M)
    s = lr.terms(f, R, [lens] * 3, i, j, a, b, 0.0)[1]
    return f, R, M, float(np.sort(s)[len(s) // 2 - 1])


@pytest.mark.parametrize("m", [1, 64, 65, 257])
@pytest.mark.parametrize("name", sorted(ACC))
def test_accumulate_per_op(ms, cuda, name, m):
    """3 views behind one lens; pair (0, 1) with m matches, pair (1, 2) with 5, pair (0, 2) with none; shuffled, a third listed as (j, i); Huber off, then at the
    median residual.  Bound per entry: ((m + 8) + T) 2^-52 S, S the sum of the terms' absolute values: tests/test_rig_lens_gpu.py::test_accumulate_per_op's bound, margin
    and reason ((m + 8) for two summation orders of the same rounded terms; T = 8 times the deviation rig_coeff_ref.term_deviation measures between float64 and
    longdouble terms, border entries included, for libm and the Newton stop).  Measured on the CPU (profiles/rig_coeffs.jsonl, "term_deviation"), smallest to
    largest deviation over m = 1, 64, 65, 257 and both Huber settings (T is 8 times it): brown-k1 6.9 to 46.1; brown-k1k2k3 7.3 to 46.1; brown-k1k2p1p2 6.9 to 46.1; fish-k1 5.7 to 99.6; fish-k1234 6.0 to 99.6.
    In every case the cost, the leading 12 x 12 block of H and the first 12 entries of g are the bits of ms_rig_lens_accumulate with the lens on every view, and with
    free_coeffs == 0 they are the whole output."""
    lens, free = ACC[name]
    G = len(cr.free_list(free))
    f, R, M, h_mid = accumulate_case(m, lens)
    assert any(va > vb for va, vb, _, _ in M) or m == 1
    assert cr.all_seen(f, R, lens, M)
    ml = L.to_ms(ms, lens)
    for h in (0.0, h_mid):
        dev = cr.term_deviation(f, R, lens, free, M, h)
        T = 8.0 * dev
        cost, H, g = ms.rig_coeff_accumulate(f, R, ml, free, M, h)
        rc, rH, rg, sc, sH, sg = cr.accumulate(f, R, lens, free, M, h, with_abs=True)
        tol = ((m + 8) + T) * 2.0 ** -52
        print("%s m=%d h=%g: term deviation %.1f, T %.1f; cost %.3e of %.3e, H %.3e, g %.3e (max |diff| / S)" % (name, m, h, dev, T, abs(cost - rc) / sc, tol,
              np.max(np.abs(H - rH) / np.maximum(sH, 1e-300)), np.max(np.abs(g - rg) / np.maximum(sg, 1e-300))))
        assert H.shape == (12 + G, 12 + G) and g.shape == (12 + G,)
        assert abs(cost - rc) <= tol * sc
        assert np.all(np.abs(H - rH) <= tol * sH) and np.all(np.abs(g - rg) <= tol * sg)
        assert np.array_equal(H, H.T) and not H[0:4, 8:12].any() and H[12:, :].all() and g[12:].all()
        lc, lH, lg = ms.rig_lens_accumulate(f, R, [ml] * 3, M, h)
        assert cost == lc and H[:12, :12].tobytes() == lH.tobytes() and g[:12].tobytes() == lg.tobytes()
        zc, zH, zg = ms.rig_coeff_accumulate(f, R, ml, 0, M, h)
        assert zc == lc and zH.tobytes() == lH.tobytes() and zg.tobytes() == lg.tobytes()


# ---- 2. exact recovery ------------------------------------------------------------------------------------------------------------------------------
REC = {"fisheye": (L.FISH, 60.0), "brown": (L.BROWN, 30.0)}       # the true lens; the spread of the world rays about a pair's bisector, in degrees


def recovery_case(model, shared):
    """6 views on the ring behind ONE lens, exact matches by the forward model, fisheye rays out to the rim (tests/test_rig_lens_gpu.py's recovery_case spread).  The
    start: the ideal ring, k1 = k2 = 0, the focals 20 and 15 % high in turn (shared: 30 % high) -- high, because at a focal below the truth the rim's pixels lie
    outside the field."""
    lens, spread = REC[model]
    rng = np.random.default_rng(50 + shared)
    R0 = rr.ring(6); Rt = rr.perturbed(R0, rng, 2.0)
    ft = np.full(6, 400.0) if shared else 400.0 * (1 + rng.uniform(-0.05, 0.05, 6))
    f0 = np.full(6, 520.0) if shared else ft * np.where(np.arange(6) % 2, 1.15, 1.2)
    pairs = rr.ring_pairs(6)
    M = lr.make_lens_matches(ft, Rt, [lens] * 6, pairs, 40, rng, spread_deg=spread)
    k0 = list(cr.k8(lens)); k0[0] = 0.0; k0[1] = 0.0
    return f0, R0, cr.with_k(lens, k0), ft, Rt, lens, pairs, M


@pytest.mark.parametrize("shared", [False, True], ids=["per-view", "shared"])
@pytest.mark.parametrize("model", sorted(REC))
def test_exact_recovery(ms, cuda, model, shared):
    """exact matches have the true cameras and lens as a zero of the cost.  Precondition, on the CPU: the reference stops CONVERGED inside max_iters.  The device ends
    within 1e-10 of the reference (the project's bound for the sibling refinements; coefficient n scaled by its effect at the rim) and no further from the truth than
    4 times the reference's own error plus 1e-12; the anchor's R is its input's bits; lens_out passes ms_lens_check (device_refine)."""
    f0, R0, lens0, ft, Rt, lt, pairs, M = recovery_case(model, shared)
    free = K1 | K2
    if model == "fisheye":
        i, j, a, b = fr.unpack(M)
        ray, _, seen = lr.view_ray(lt, a[:, 0] / ft[i], a[:, 1] / ft[i])
        th = np.degrees(np.arctan2(np.hypot(ray[0], ray[1]), ray[2]))
        assert seen.all() and ((th > 90.0) & (th < 100.0)).sum() >= 5, "no fisheye match past 90 degrees"
    kw = dict(anchor=0, shared_focal=shared, step_tol=1e-13, max_iters=100)
    rf, rR, rl, ri = ref_refine(("rec", model, shared), f0, R0, lens0, free, M, **kw)
    assert ri["stop_reason"] == fr.CONVERGED and ri["iterations"] < 100, ri
    want = rr.expected(R0, Rt, 0)
    ref_err = (max_angle(rR, want), float(np.max(np.abs(rf / ft - 1.0))), coeff_gap(rl, lt, free))
    f, R, lo, info = device_refine(ms, f0, R0, lens0, free, M, **kw)
    err = (max_angle(R, want), float(np.max(np.abs(f / ft - 1.0))), coeff_gap(lo, lt, free))
    d = (max_angle(R, rR), float(np.max(np.abs(f / rf - 1.0))), coeff_gap(lo, rl, free))
    print("%s shared=%s: device to the truth %.3e rad, %.3e focal, %.3e coefficient (reference %.3e, %.3e, %.3e); device to reference %.3e, %.3e, %.3e; %d iterations "
          "(reference %d), stop %d, cost %.3e -> %.3e, k1 k2 %s" % ((model, shared) + err + ref_err + d + (info["iterations"], ri["iterations"], info["stop_reason"],
                                                                                                       info["cost_initial"], info["cost_final"], cr.k8(lo)[:2])))
    assert max(d) <= 1e-10
    assert all(e <= 4.0 * r + 1e-12 for e, r in zip(err, ref_err))
    assert R[0].tobytes() == R0[0].tobytes() and (not shared or np.all(f == f[0]))
    assert info["matches_used"] == len(M) and info["pairs_used"] == len(pairs) and info["outliers"] == 0 and info["cost_final"] <= info["cost_initial"]
    assert cr.all_seen(f, R, lo, M) and cr.k8(lo)[2:] == cr.k8(lens0)[2:]


# ---- 3. noise and outliers --------------------------------------------------------------------------------------------------------------------------
# tests/test_rig_lens_gpu.py's Huber cases behind the shared lens
NOISY = {
    "huber": dict(noise_px=0.02, outlier_frac=0.15, huber_px=0.1, shared=False, anchor=4),
    "huber-shared": dict(noise_px=0.02, outlier_frac=0.15, huber_px=0.1, shared=True, anchor=2),
}


def noisy_case(name):
    c = NOISY[name]
    rng = np.random.default_rng(sorted(NOISY).index(name) + 270)
    R0 = rr.ring(6).copy()
    ft = np.full(6, 412.0) if c["shared"] else 400.0 * (1 + rng.uniform(-0.04, 0.04, 6))
    M = lr.make_lens_matches(ft, rr.perturbed(R0, rng, 2.0), [L.FISH] * 6, rr.ring_pairs(6), 64, rng, noise_px=c["noise_px"], outlier_frac=c["outlier_frac"], spread_deg=40.0)
    return np.full(6, 400.0), R0, M, dict(huber_px=c["huber_px"], shared_focal=c["shared"], anchor=c["anchor"], step_tol=1e-12, max_iters=100)


@pytest.mark.parametrize("name", sorted(NOISY))
def test_noisy_matches_against_the_reference(ms, cuda, name):
    f0, R0, M, kw = noisy_case(name)
    against_the_reference(ms, name, f0, R0, L.FISH, K1 | K2, M, kw)


# ---- 4. a trial lens that folds back ----------------------------------------------------------------------------------------------------------------
FOLD_START = ("fisheye", (-0.06, 0.0, 0.0, 0.0), 100.0)           # theta_d' = 1 + 3 k1 theta^2 stays positive up to 100 degrees for k1 > -0.1094


def fold_case():
    """3 fisheye views whose true lens has k1 = -0.10, inside the monotone range at max_theta = 100 degrees; the start has k1 = -0.06 and the focal 6 % high, which
    the first, nearly undamped proposal answers with k1 = -0.122, past -0.1094: its profile folds back before 100 degrees.  Exact matches: the reference still ends at
    the truth, CONVERGED, after three rejected solves"""
    rng = np.random.default_rng(91)
    true = ("fisheye", (-0.10, 0.0, 0.0, 0.0), 100.0)
    R0 = rr.ring(6)[:3].copy(); Rt = rr.perturbed(R0, rng, 1.0)
    M = lr.make_lens_matches(np.full(3, 400.0), Rt, [true] * 3, [(0, 1), (1, 2)], 40, rng, spread_deg=30.0, margin_deg=15.0)
    return np.full(3, 424.0), R0, M


def test_a_trial_lens_that_folds_back_is_rejected(ms, cuda):
    f0, R0, M = fold_case()
    assert cr.lens_ok(FOLD_START) and cr.all_seen(f0, R0, FOLD_START, M)
    # the precondition, on the CPU: the reference's first proposal is not a lens
    _, _, trial = cr.propose(f0, R0, FOLD_START, K1, M, 0, True, 1e-3)
    assert not cr.lens_ok(trial), trial
    kw = dict(shared_focal=True, step_tol=1e-12, max_iters=100)
    rf, rR, rl, ri = ref_refine("fold", f0, R0, FOLD_START, K1, M, **kw)
    f, R, lo, info = device_refine(ms, f0, R0, FOLD_START, K1, M, **kw)
    d = max_angle(R, rR); df = float(np.max(np.abs(f / rf - 1.0))); dk = coeff_gap(lo, rl, K1)
    print("first trial k1 %.6f; device k1 %.9f focal %.6f, %d iterations (reference %d), stop %d (%d); to the reference %.3e rad, %.3e focal, %.3e coefficient"
          % (cr.k8(trial)[0], cr.k8(lo)[0], f[0], info["iterations"], ri["iterations"], info["stop_reason"], ri["stop_reason"], d, df, dk))
    assert d <= 1e-10 and df <= 1e-10 and dk <= 1e-10
    # the extra round: a solve rejected by the trial-lens rule counts as an iteration, the reference counted at least one, and the device's count is the reference's
    assert ri["lens_rejections"] >= 1 and info["iterations"] == ri["iterations"] and info["stop_reason"] == ri["stop_reason"]
    assert cr.lens_ok(lo) and info["cost_final"] <= info["cost_initial"]


# ---- 5. size edges ----------------------------------------------------------------------------------------------------------------------------------
def two_view_case():
    rng = np.random.default_rng(31)
    R0 = rr.ring(6)[:2].copy()
    M = lr.make_lens_matches(np.full(2, 408.0), rr.perturbed(R0, rng, 2.0), [L.FISH] * 2, [(0, 1)], 96, rng, noise_px=0.02, outlier_frac=0.15, spread_deg=50.0)
    return np.full(2, 400.0), R0, M, dict(huber_px=0.1, shared_focal=True, anchor=1, step_tol=1e-12, max_iters=100)


def test_two_views_one_pair(ms, cuda):
    f0, R0, M, kw = two_view_case()
    against_the_reference(ms, "two", f0, R0, L.FISH, K1, M, kw)


def complete_case(shared):
    """16 fisheye views on the ring, all 120 pairs (views up to 180 degrees apart share rays near 90 degrees off both axes), 8 matches a pair: with k1..k4 free the
    largest system, 3 * 15 + 16 + 4 = 65 unknowns (shared focal: 50).  The start focal lies above every true one (below, the rim's pixels leave the field).
    Noise 0.004 pixels, outliers 0.1 to 0.3 pixels off, Huber at 0.02: the accept rule cost_trial <= cost is decided by rounding once a step changes the cost by less
    than 2^-52 of it, and the two implementations may then end one such step apart; a cost 25 times below the noisy cases' keeps that step, times the 262 that
    scales k4, below 1e-10 (measured on the CPU between summation orders of the reference: up to 4e-11)"""
    rng = np.random.default_rng(160 + shared)
    R0 = rr.ring(16).copy()
    ft = np.full(16, 405.0) if shared else 400.0 * (1 + rng.uniform(-0.03, 0.03, 16))
    pairs = [(i, j) for i in range(16) for j in range(i + 1, 16)]
    M = lr.make_lens_matches(ft, rr.perturbed(R0, rng, 1.0), [L.FISH] * 16, pairs, 8, rng, noise_px=0.004, outlier_frac=0.1, spread_deg=8.0, outlier_px=(0.1, 0.3),
                             margin_deg=1.0)
    return np.full(16, 415.0), R0, M, dict(huber_px=0.02, shared_focal=bool(shared), anchor=5, step_tol=1e-10, max_iters=100)


@pytest.mark.parametrize("shared", [False, True], ids=["per-view", "shared"])
def test_sixteen_views_complete_graph_four_coefficients(ms, cuda, shared):
    f0, R0, M, kw = complete_case(shared)
    _, _, _, info, _ = against_the_reference(ms, ("complete", shared), f0, R0, L.FISH, 0b1111, M, kw)
    assert info["pairs_used"] == 120 and info["matches_used"] == 960


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits(ms, cuda):
    f0, R0, M, kw = noisy_case("huber")
    a = device_refine(ms, f0, R0, L.FISH, K1 | K2, M, **kw)
    b = device_refine(ms, f0, R0, L.FISH, K1 | K2, M, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3] == b[3]
    ml = L.to_ms(ms, L.FISH)
    ca = ms.rig_coeff_accumulate(f0, R0, ml, 0b1111, M, 1.5); cb = ms.rig_coeff_accumulate(f0, R0, ml, 0b1111, M, 1.5)
    assert ca[0] == cb[0] and ca[1].tobytes() == cb[1].tobytes() and ca[2].tobytes() == cb[2].tobytes()


# ---- 7. the context form ----------------------------------------------------------------------------------------------------------------------------
def test_context_form_is_the_array_form_on_its_pixels(ms, cuda):
    """tests/test_rig_lens_gpu.py's small lens context (6 views of 160 x 120 behind one BROWN lens) and fabricated lists: the context form derives the centred pixels
    ms_refine_rig_focals_lens derives (`px`, the same numpy formulas on the float positions, equal to 1e-9 pixels) and then is the array form: the results agree to
    1e-9 (the float rounding of R aside), and nothing is applied to the context."""
    import test_rig_lens_gpu as G
    rng = np.random.default_rng(17)
    comp = G.small_rig(ms, G.CTX_LENS)
    Rt = rr.perturbed(rr.ring(6), rng, 1.5)
    lists, px, R0 = G.fabricate_lists(comp, G.CTX_LENS, Rt, 12, rng)
    prm = ms.rig_coeff_default_params(free_coeffs=K1, shared_focal=1)
    before = [tuple(comp.get_lens(v).k) for v in range(6)]
    f, R, ml, info = comp.refine_rig_coeffs(lists, prm)
    assert f.dtype == np.float64 and R.dtype == np.float32 and info["matches_used"] == 72 and info["pairs_used"] == 6
    assert ms.load().ms_lens_check(C.byref(ml)) == 0 and [tuple(comp.get_lens(v).k) for v in range(6)] == before
    fa, Ra, la, ia = ms.refine_rig_coeffs(np.full(6, G.F_CTX), R0, L.to_ms(ms, G.CTX_LENS), px, prm)
    d = max_angle(R.astype(np.float64), Ra.astype(np.float32).astype(np.float64)); df = float(np.max(np.abs(f / fa - 1.0))); dk = abs(ml.k[0] - la.k[0])
    print("context against array form: %.3e rad, %.3e relative focal, %.3e in k1; k1 %.6f -> %.6f, focal %.4f, cost %.3e -> %.3e" % (d, df, dk, G.CTX_LENS[1][0], ml.k[0], f[0],
          info["cost_initial"], info["cost_final"]))
    assert d <= 1e-9 and df <= 1e-9 and dk <= 1e-9
    assert info["cost_final"] <= info["cost_initial"] and info["iterations"] >= 2 and tuple(ml.k)[1:] == tuple(G.CTX_LENS[1])[1:]
    comp.close()


def test_context_form_state_and_refusals(ms, cuda):
    import test_rig_lens_gpu as G
    lists = [[(10.0 + 3 * q, 20.0 + 5 * q, 30.0 + 2 * q, 40.0 + q, (v + 1) % 6) for q in range(4)] for v in range(6)]
    comp = G.small_rig(ms, G.CTX_LENS, build=False)
    with pytest.raises(ms.MsError, match="-5.*ms_build_maps first"):         # MS_ERR_STATE
        comp.refine_rig_coeffs(lists)
    comp.build_maps()
    f, R, ml, info = comp.refine_rig_coeffs(lists)
    assert info["cost_final"] <= info["cost_initial"]
    with pytest.raises(ms.MsError, match="-2.*denominator"):
        comp.refine_rig_coeffs(lists, ms.rig_coeff_default_params(free_coeffs=0x20))
    with pytest.raises(ms.MsError, match="-1.*free_coeffs is empty"):
        comp.refine_rig_coeffs(lists, ms.rig_coeff_default_params(free_coeffs=0))
    with pytest.raises(ms.MsError, match="-1.*names view"):
        comp.refine_rig_coeffs([[(10.0, 20.0, 30.0, 40.0, v)] * 4 for v in range(6)])
    # one lens a rig: a view with other coefficients, another field, another model, no lens
    other = ("brown", (-0.1, 0.011, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), 0.0)
    for v, lens, word in ((3, other, "view 3"), (2, (G.CTX_LENS[0], G.CTX_LENS[1], 80.0), "view 2"), (4, ("fisheye", (0.0,) * 4, 89.0), "view 4"), (5, None, "view 5"),
                          (0, None, "view 0")):
        twin = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
        for q in range(6):
            Kq, Rq = synth.camera(6, 160, 120, 90.0, q)
            l = lens if q == v else G.CTX_LENS
            if l is not None:
                twin.set_lens(q, L.to_ms(ms, l))
            twin.set_camera(q, Kq, Rq)
        twin.build_maps()
        with pytest.raises(ms.MsError, match="-2.*%s" % word):               # MS_ERR_UNSUPPORTED
            twin.refine_rig_coeffs(lists)
        twin.close()
    skew = G.small_rig(ms, G.CTX_LENS, skew=3)
    with pytest.raises(ms.MsError, match=r"-2.*view 3.*K\[1\]"):
        skew.refine_rig_coeffs(lists)
    skew.close(); comp.close()
