"""tests/rig_coeff_ref.py against itself, no GPU: every analytic coefficient column e_n = dr/dk_n against central differences of the reference's own residual in
numpy.longdouble, and the pieces of its Levenberg-Marquardt loop the GPU tests rely on (the profile rule, the selection matrix, G = 0)."""
import math

import numpy as np
import pytest

import lens_ref as L
import rig_coeff_ref as cr
import rig_focal_ref as fr
import rig_lens_ref as lr
import rig_ref as rr

LD = np.longdouble
FISH4 = ("fisheye", (-0.02, 0.003, -2e-4, 1e-5), 100.0)
BROWN5 = ("brown", (-0.18, 0.03, 1e-3, -5e-4, 0.002, 0.01, 0.001, 0.0), 60.0)      # k3 and a fixed denominator (k4, k5) beside lens_ref.BROWN's entries


def column_case(lens):
    """2 views of the ring behind `lens`, noisy matches out to the rim (fisheye: past 90 degrees), and one match whose pixel in view 0 is the centre"""
    rng = np.random.default_rng(5)
    R = rr.perturbed(rr.ring(6)[:2], rng, 3.0)
    f = np.array([400.0, 431.5])
    M = lr.make_lens_matches(f, rr.perturbed(rr.ring(6)[:2], rng, 3.0), [lens] * 2, [(0, 1)], 40, rng, noise_px=0.5, spread_deg=60.0 if lens[0] == "fisheye" else 25.0)
    b, seen = lr.centred_pixels(f[1], lens, (R[1].T @ R[0] @ np.array([0.0, 0.0, 1.0]))[None, :])
    assert seen[0]
    return f, R, M + [(0, 1, np.zeros(2), b[0])]


@pytest.mark.parametrize("lens", [FISH4, BROWN5, L.FISH, L.BROWN], ids=["fisheye4", "brown5", "fisheye", "brown"])
def test_every_column_against_central_differences(lens):
    """For every allowed bit: D(h) = (r(k + h) - r(k - h)) / 2h in longdouble at h and h / 2.  The central difference's error falls by 4 when h halves, so
    |e - D(h/2)| is a third of |D(h) - D(h/2)|; the bound is 2 |D(h) - D(h/2)| plus the rounding floor of D(h/2), 64 eps m / (h/2) (r = m (p - q) carries a few dozen
    longdouble roundings of size eps m from the solver, sin / cos and the rotation; 64 covers them).  The bound comes from the data: no step size is tuned to pass."""
    assert cr.lens_ok(lens)
    f, R, M = column_case(lens)
    i, j, a, b = fr.unpack(M)
    if lens[0] == "fisheye":
        th = []
        for v, px in ((0, a), (1, b)):
            ray, seen = lr.unproject(np.diag([f[v], f[v], 1.0]), lens, px[:, 0], px[:, 1])
            assert seen.all()
            th += np.degrees(np.arctan2(np.hypot(ray[:, 0], ray[:, 1]), ray[:, 2])).tolist()
        assert max(th) > 90.0, "no fisheye ray past 90 degrees"
    eps = float(np.finfo(LD).eps)
    m = math.sqrt(f[0] * f[1])
    h = 1e-4
    for bit in cr.ALLOWED[lens[0]]:
        E = cr.columns(f, R, lens, 1 << bit, i, j, a, b, LD)[0]
        E64 = cr.columns(f, R, lens, 1 << bit, i, j, a, b)[0]

        def D(step):
            out = []
            for sgn in (1, -1):
                k = [LD(v) for v in cr.k8(lens)]
                k[bit] = k[bit] + LD(sgn) * LD(step)
                r, seen = cr.residual(f, R, (lens[0], tuple(k), lens[2]), i, j, a, b, LD)
                assert seen.all()
                out.append(r)
            return [(out[0][c] - out[1][c]) / (LD(2) * LD(step)) for c in range(3)]

        D1, D2 = D(h), D(h / 2)
        worst = 0.0
        for c in range(3):
            bound = 2.0 * np.abs(D1[c] - D2[c]) + 64.0 * eps * m / (h / 2)
            err = np.abs(E[c] - D2[c])
            assert np.all(err <= bound), (lens[0], bit, c, float(np.max(err - bound)))
            worst = max(worst, float(np.max(err / bound)))
            # the float64 column is the longdouble one up to float64 rounding of a quantity of size m: 1e-9 relative to the column's largest entry and m leaves room
            assert np.all(np.abs(E64[c].astype(LD) - E[c]) <= 1e-9 * max(m, float(np.max(np.abs(E[c])))))
        # the centre pixel (the last match, view 0's side) contributes nothing for a fisheye; the other side does
        assert float(np.max(np.abs(np.array([float(E[c][-1]) for c in range(3)])))) > 0.0 or lens[0] == "fisheye"
        print("%s bit %d: worst |e - D(h/2)| / bound %.3f; largest |e| %.3e" % (lens[0], bit, worst, max(float(np.max(np.abs(E[c]))) for c in range(3))))


def test_fisheye_centre_column_is_zero():
    z = np.zeros(1)
    for bit in range(4):
        assert all(float(c[0]) == 0.0 for c in cr.dray(FISH4, bit, z, z))


def test_profile_rule():
    assert cr.lens_ok(L.FISH) and cr.lens_ok(L.BROWN) and cr.lens_ok(FISH4) and cr.lens_ok(BROWN5)
    assert not cr.lens_ok(("fisheye", (-0.2, 0.0, 0.0, 0.0), 100.0))          # 1 - 0.6 theta^2 < 0 from 74 degrees on
    assert not cr.lens_ok(("brown", (-0.5,) + (0.0,) * 7, 60.0))               # 1 - 1.5 r^2 < 0 from r = 0.82 on, tan 60 = 1.73
    assert not cr.lens_ok(("fisheye", (float("nan"), 0.0, 0.0, 0.0), 100.0))


def test_no_free_coefficient_is_the_lens_reference():
    f, R, M = column_case(L.FISH)
    a = cr.accumulate(f, R, L.FISH, 0, M, 0.4); b = lr.accumulate(f, R, [L.FISH] * 2, M, 0.4)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    c = cr.accumulate(f, R, L.FISH, 0b11, M, 0.4)
    assert c[0] == b[0] and c[1][:8, :8].tobytes() == b[1].tobytes() and c[2][:8].tobytes() == b[2].tobytes() and c[1].shape == (10, 10)
    assert np.array_equal(c[1], c[1].T) and c[1][8:, :].all()


def test_selection_and_step():
    P = cr.selection(3, 1, True, 2)
    assert P.shape == (14, 3 * 2 + 1 + 2) and P[12, 7] == 1.0 and P[13, 8] == 1.0 and not P[12:, :7].any()
    full = np.zeros(14); full[12] = 0.5; full[13] = -0.25
    f, R, lens = cr.apply_step(np.ones(3), np.array([np.eye(3)] * 3), L.BROWN, 0b10010, full)
    assert cr.k8(lens)[1] == 0.03 + 0.5 and cr.k8(lens)[4] == -0.25 and cr.k8(lens)[0] == -0.18
