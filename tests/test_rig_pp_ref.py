"""tests/rig_pp_ref.py against itself, no GPU: the analytic centre columns dr/dox, dr/doy of both views against central differences of the reference's own residual
in numpy.longdouble, the 46-term subset against tests/rig_lens_ref.py on pre-shifted pixels, and the Levenberg-Marquardt loop with and without the prior."""
import math

import numpy as np
import pytest

import lens_ref as L
import rig_focal_ref as fr
import rig_lens_ref as lr
import rig_pp_ref as pr
import rig_ref as rr

LD = np.longdouble
NONE = ("none", (), 0.0)
LENSES = {"none": NONE, "fisheye": L.FISH, "brown": L.BROWN}


def column_case(lens):
    """2 views of the ring behind `lens` with offsets of a few pixels, noisy matches out to the rim (fisheye: past 90 degrees), and one match whose pixel in view 0
    lies exactly on the true centre (the centred pixel (0, 0) after the offset is subtracted)"""
    rng = np.random.default_rng(5)
    R = rr.perturbed(rr.ring(6)[:2], rng, 3.0)
    f = np.array([400.0, 431.5])
    pp = np.array([[7.25, -4.5], [-3.0, 9.75]])
    spread = {"fisheye": 60.0, "brown": 25.0, "none": 25.0}[lens[0]]
    M = pr.make_pp_matches(f, rr.perturbed(rr.ring(6)[:2], rng, 3.0), pp, [lens] * 2, [(0, 1)], 40, rng, noise_px=0.5, spread_deg=spread)
    b, seen = lr.centred_pixels(f[1], lens, (R[1].T @ R[0] @ np.array([0.0, 0.0, 1.0]))[None, :])
    assert seen[0]
    return f, R, pp, M + [(0, 1, pp[0].copy(), b[0] + pp[1])]


@pytest.mark.parametrize("model", sorted(LENSES))
def test_every_centre_column_against_central_differences(model):
    """For each of (ox_0, oy_0, ox_1, oy_1): D(h) = (r(o + h) - r(o - h)) / 2h in longdouble at h and h / 2.  The central difference's error falls by 4 when h halves,
    so |e - D(h/2)| is a third of |D(h) - D(h/2)|; the bound is 2 |D(h) - D(h/2)| plus the rounding floor of D(h/2), 64 eps m / (h/2) (tests/test_rig_coeff_ref.py's
    bound and reason: r = m (p - q) carries a few dozen longdouble roundings of size eps m).  The last match's pixel in view 0 is the centre itself: the fisheye takes its
    identity branch there, and the column is (to rounding) -m R e_x / f."""
    lens = LENSES[model]
    f, R, pp, M = column_case(lens)
    lenses = [lens] * 2
    i, j, a, b = fr.unpack(M)
    assert pr.all_seen(f, R, pp, lenses, M)
    assert a[-1, 0] - pp[0, 0] == 0.0 and a[-1, 1] - pp[0, 1] == 0.0
    eps = float(np.finfo(LD).eps)
    m = math.sqrt(f[0] * f[1])
    h = 1e-2                                                  # pixels
    E = pr.columns(f, R, pp, lenses, i, j, a, b, LD)
    E64 = pr.columns(f, R, pp, lenses, i, j, a, b)
    for q, (view, comp) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        def D(step):
            out = []
            for sgn in (1, -1):
                p2 = pp.astype(LD)
                p2[view, comp] = p2[view, comp] + LD(sgn) * LD(step)
                f_, R_, _, a_, b_ = pr._cast(f, R, pp, a, b, LD)
                mm = np.sqrt(f_[i] * f_[j])
                p, _, si = lr._side(f_, R_, lenses, i, a_ - p2[i], mm, LD)
                qq, _, sj = lr._side(f_, R_, lenses, j, b_ - p2[j], mm, LD)
                assert si.all() and sj.all()
                out.append([mm * (p[c] - qq[c]) for c in range(3)])
            return [(out[0][c] - out[1][c]) / (LD(2) * LD(step)) for c in range(3)]

        D1, D2 = D(h), D(h / 2)
        worst = 0.0
        for c in range(3):
            bound = 2.0 * np.abs(D1[c] - D2[c]) + 64.0 * eps * m / (h / 2)
            err = np.abs(E[q][c] - D2[c])
            assert np.all(err <= bound), (model, q, c, float(np.max(err - bound)))
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(np.abs(E64[q][c].astype(LD) - E[q][c]) <= 1e-9 * max(1.0, float(np.max(np.abs(E[q][c])))))
        print("%s column %d: worst |e - D(h/2)| / bound %.3f; largest |e| %.3e" % (model, q, worst, max(float(np.max(np.abs(E[q][c]))) for c in range(3))))
    # the centre pixel: dr/dox_0 = -m R_0 e_x / f_0 for every model (A is the identity's first two columns there, the pinhole's included)
    for c in range(3):
        assert abs(float(E64[0][c][-1]) + m * R[0][c, 0] / f[0]) <= 1e-12 and abs(float(E64[1][c][-1]) + m * R[0][c, 1] / f[0]) <= 1e-12


def mixed_case(m=40):
    rng = np.random.default_rng(77)
    lenses = [L.FISH, NONE, L.BROWN]
    R = rr.perturbed(rr.ring(6)[:3], rng, 4.0)
    f = np.array([400.0, 431.5, 388.25])
    pp = np.array([[6.5, -3.25], [0.0, 0.0], [-8.0, 11.5]])
    M = pr.make_pp_matches(f * (1 + rng.uniform(-0.02, 0.02, 3)), rr.perturbed(rr.ring(6)[:3], rng, 4.0), pp + rng.uniform(-1, 1, (3, 2)), lenses, [(0, 1), (1, 2)],
                           [m, 7], rng, noise_px=0.6)
    M = [(vb, va, b, a) if rng.uniform() < 1 / 3 else (va, vb, a, b) for va, vb, a, b in M]
    return f, R, pp, lenses, M


@pytest.mark.parametrize("h", [0.0, 0.8])
def test_the_46_term_subset_is_the_lens_reference_on_shifted_pixels(h):
    """the terms that involve only rotations and focals are rig_lens_ref's expressions: bit-equal term by term and sum by sum on pixels shifted in double beforehand"""
    f, R, pp, lenses, M = mixed_case()
    i, j, a, b = fr.unpack(M)
    T, s, seen = pr.terms(f, R, pp, lenses, i, j, a, b, h)
    Ms = pr.shift(M, pp)
    si, sj, sa, sb = fr.unpack(Ms)
    T4, s4, seen4 = lr.terms(f, R, lenses, si, sj, sa, sb, h)
    assert seen.all() and seen4.all() and T.shape == (len(M), 92) and len(pr.lens_subset()) == 46
    assert T[:, pr.lens_subset()].tobytes() == T4.tobytes() and s.tobytes() == s4.tobytes()
    c, H, g = pr.accumulate(f, R, pp, lenses, M, h)
    c4, H4, g4 = lr.accumulate(f, R, lenses, Ms, h)
    rows = pr.view_rows(3)
    assert c == c4 and H[np.ix_(rows, rows)].tobytes() == H4.tobytes() and g[rows].tobytes() == g4.tobytes()
    assert np.array_equal(H, H.T) and H[4:6, :6].all() and g[4:6].all() and not H[0:6, 12:18].any()
    # the centre columns of H are J^T W J's: against the columns themselves
    ex, ey, fx, fy = pr.columns(f, R, pp, lenses, i, j, a, b)
    if h == 0.0:
        k0 = (i == 0) & (j == 1)
        want = sum(float(ex[c][k] * fx[c][k]) for k in np.flatnonzero(k0) for c in range(3))
        assert abs(H[4, 10] - want) <= 1e-9 * abs(want)


def ring_case(n, lens, rng, per_pair=30, noise=0.0, off=12.0):
    R0 = rr.ring(n).copy(); Rt = rr.perturbed(R0, rng, 1.0)
    ft = 400.0 * (1 + rng.uniform(-0.02, 0.02, n))
    ppt = rng.uniform(-off, off, (n, 2))
    lenses = [lens] * n
    M = pr.make_pp_matches(ft, Rt, ppt, lenses, rr.ring_pairs(n), per_pair, rng, noise_px=noise, spread_deg=25.0)
    return np.full(n, 400.0), R0, np.zeros((n, 2)), lenses, M, ft, Rt, ppt


@pytest.mark.parametrize("model", sorted(LENSES))
def test_refine_on_exact_matches_returns_the_truth(model):
    rng = np.random.default_rng(11)
    f0, R0, p0, lenses, M, ft, Rt, ppt = ring_case(6, LENSES[model], rng)
    f, R, pp, info = pr.refine(f0, R0, p0, lenses, M, step_tol=1e-13, max_iters=100)
    want = rr.expected(R0, Rt, 0)
    err = (max(rr.angle(a, b) for a, b in zip(R, want)), float(np.max(np.abs(f / ft - 1.0))), float(np.max(np.abs(pp - ppt))))
    print("%s: %.3e rad, %.3e focal, %.3e px; %d iterations, stop %d, cost %.3e -> %.3e" % ((model,) + err + (info["iterations"], info["stop_reason"], info["cost_initial"],
                                                                                                        info["cost_final"])))
    assert info["stop_reason"] == fr.CONVERGED and err[0] <= 1e-9 and err[1] <= 1e-9 and err[2] <= 1e-6
    assert info["cost_final"] <= info["cost_initial"] and info["cost_final"] <= 1e-15 and info["max_pp_shift"] > 1.0
    assert R[0].tobytes() == R0[0].tobytes()


def test_prior_holds_the_centres_and_its_absence_frees_them():
    rng = np.random.default_rng(12)
    f0, R0, p0, lenses, M, ft, Rt, ppt = ring_case(4, NONE, rng, noise=0.3)
    p_in = rng.uniform(-2, 2, (4, 2))
    costs = []
    for w in (0.0, 1e-2, 1e12):
        f, R, pp, info = pr.refine(f0, R0, p_in, lenses, M, step_tol=1e-12, max_iters=100, pp_prior=w)
        assert info["cost_final"] <= info["cost_initial"]
        costs.append(info["cost_final"])
        print("w = %g: centres moved %.3e px, focal ratio %.6f, cost %.4e -> %.4e, %d iterations, stop %d" % (w, info["max_pp_shift"], info["max_focal_ratio"], info["cost_initial"],
              info["cost_final"], info["iterations"], info["stop_reason"]))
        if w == 1e12:
            assert info["max_pp_shift"] <= 1e-9 and info["max_focal_ratio"] > 1.001 and info["max_rotation_rad"] > 1e-3
        else:
            assert info["max_pp_shift"] > 0.5
    assert costs[0] <= costs[1] <= costs[2]                  # a heavier prior never lowers the total cost at the optimum


def test_selection_and_step():
    P = pr.selection(3, 1, False)
    assert P.shape == (18, 15) and not P[6:9].any() and P[9:12].sum() == 3
    P = pr.selection(3, 1, True)
    assert P.shape == (18, 3 * 2 + 1 + 6) and np.array_equal(P[3::6, -1], np.ones(3)) and P[:, -1].sum() == 3
    full = np.zeros(18); full[4] = 0.5; full[17] = -0.25; full[9] = math.log(2.0)
    f, R, pp = pr.apply_step(np.ones(3), np.array([np.eye(3)] * 3), np.zeros((3, 2)), full)
    assert pp[0, 0] == 0.5 and pp[2, 1] == -0.25 and not pp[1].any() and abs(f[1] - 2.0) < 1e-15 and np.array_equal(R[0], np.eye(3))
