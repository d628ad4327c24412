"""The inputs of tests/test_rig_lm_gpu.py do what its tests assume, shown on the numpy references alone (no GPU, no library): tests/rig_lm_cases.py.

1. the case tables cover every solved size and the anchors at either end and in the middle
2. one step: the reference ends after one accepted iteration at the iteration limit with a lower cost; its output is Exp(delta) R0 and f0 exp(d) of the step helper,
   laid out by rules written apart from the references'; the derived bound stays orders below what a wrong row costs
3. two and three steps: every step of the reference is accepted, away from the rounding floor
4. the degenerate inputs have a diagonal entry of exactly zero, and the references count 16 refusals (STALLED), stop at the iteration limit, or converge once the
   degenerate view is held
5. the 16-view accumulate cases: both Huber branches, pairs listed (j, i), the blocks that must be zero"""
import numpy as np
import pytest

import rig_focal_ref as fr
import rig_lm_cases as cases
import rig_ref as rr


# ---- 1. the tables --------------------------------------------------------------------------------------------------------------------------------------
def test_the_case_tables_cover_every_size_and_anchor_position():
    ring = [(n, a) for g, n, a in cases.STEP_CASES if g == "ring"]
    assert sorted({n for n, _ in ring}) == list(range(2, 17))
    for n in range(2, 17):
        assert {a for m, a in ring if m == n} == {0, n // 2, n - 1}
    assert sum(1 for n, a in ring if 0 < a < n - 1) == 14                  # a middle anchor at every n from 3
    assert {cases.solved_size("rot", n) for n, _ in ring} == set(range(3, 46, 3))
    assert {cases.solved_size("focal", n) for n, _ in ring} == set(range(5, 62, 4))
    assert {cases.solved_size("shared", n) for n, _ in ring} == set(range(4, 47, 3))
    # the trailing-block loop of the factorisation, e < t * t over 256 lanes, t = m - 1 at the first column: one pass, several, and ragged last passes
    t2 = sorted({(cases.solved_size(f, n) - 1) ** 2 for f in cases.FLAVOURS for n, _ in ring})
    many = [t for t in t2 if t > 256]
    assert any(t < 256 for t in t2) and 256 in t2 and len(many) >= 20 and sum(1 for t in many if t % 256) >= 20 and any(t % 256 == 0 for t in many)
    assert [c for c in cases.STEP_CASES if c[0] == "complete"] == [("complete", 4, 2), ("complete", 16, 8)]
    assert len(cases.pairs_of("complete", 16)) == 120 and len(cases.pairs_of("ring", 16)) == 16 and cases.pairs_of("ring", 2) == [(0, 1)]
    assert cases.MULTI_CASES == [(3, 2), (3, 3), (6, 2), (6, 3), (16, 2), (16, 3)]


# ---- 2. one step ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", cases.FLAVOURS)
def test_one_step_premises(flavour):
    """Measured: cond_2(A) at lambda = 1e-3 up to 685 (rot), 1650 (focal), 1013 (shared); the bound up to 2.5e-11, 8.1e-11, 6.9e-11; |delta|_2 up to 0.51."""
    worst_cond = worst_bound = 0.0
    for graph, n, anchor in cases.STEP_CASES:
        f0, R0, M, kw = cases.inputs(flavour, graph, n, anchor)
        t = cases.one_step(flavour, graph, n, anchor)
        info = t["info"]
        where = (flavour, graph, n, anchor)
        assert info["iterations"] == 1 and info["stop_reason"] == rr.ITERATION_LIMIT and info["cost_final"] < info["cost_initial"], where
        assert info["matches_used"] == len(M) == len(cases.pairs_of(graph, n)) * (6 if graph == "ring" else 3) and info["pairs_ignored"] == 0, where
        assert t["lam"] == 1e-3 and t["A"].shape == (cases.solved_size(flavour, n),) * 2 and np.allclose(t["A"], t["A"].T, rtol=1e-13, atol=0.0), where
        # the reference's output is the helper's step, applied view by view
        fn, Rn = cases.apply_delta(flavour, f0, R0, t["delta"], anchor)
        assert Rn.tobytes() == t["R"].tobytes() and t["R"][anchor].tobytes() == R0[anchor].tobytes(), where
        if flavour != "rot":
            assert fn.tobytes() == t["f"].tobytes() and (flavour == "focal" or np.all(t["f"] == t["f"][0])), where
            assert np.all(t["f"] != f0), where                                 # every focal moves, the anchor's too
        assert all(rr.angle(t["R"][v], R0[v]) > 1e-3 for v in range(n) if v != anchor), where      # every other view turns by far more than the bound
        # the bound is a statement about rounding: orders below the 1e-4 and more of a wrong row, sign or lambda
        assert 2.0 ** -50 < t["bound"] < 1e-9, where
        worst_cond = max(worst_cond, float(np.linalg.cond(t["A"], 2))); worst_bound = max(worst_bound, t["bound"])
    print("%s: cond_2(A) up to %.0f, the bound up to %.2e" % (flavour, worst_cond, worst_bound))
    assert worst_cond < 5e3


def test_a_wrong_lambda_or_a_dropped_row_is_orders_above_the_bound():
    """what the bound must tell apart: the step with lambda ten times off, and the step of a system whose anchor is one view off"""
    for flavour in cases.FLAVOURS:
        f0, R0, M, kw = cases.inputs(flavour, "ring", 6, 3)
        t = cases.one_step(flavour, "ring", 6, 3)
        _, d10 = cases.ref_step(flavour, f0, R0, M, kw, 1e-2)
        _, Rw = cases.apply_delta(flavour, f0, R0, d10, 3)
        assert max(rr.angle(a, b) for a, b in zip(Rw, t["R"])) > 1e4 * t["bound"]
        _, da = cases.ref_step(flavour, f0, R0, M, dict(kw, anchor=2), 1e-3)
        _, Rw = cases.apply_delta(flavour, f0, R0, da, 2)
        assert max(rr.angle(a, b) for a, b in zip(Rw, t["R"])) > 1e4 * t["bound"]


# ---- 3. two and three steps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", cases.FLAVOURS)
@pytest.mark.parametrize("n, iters", cases.MULTI_CASES)
def test_every_step_of_the_multi_step_runs_is_accepted(flavour, n, iters):
    anchor = n // 2
    traj = cases.trajectory(flavour, "ring", n, anchor, iters)
    f0, R0, M, kw = cases.inputs(flavour, "ring", n, anchor)
    f, R, cost = f0, R0, traj[0]["info"]["cost_initial"]
    for k, t in enumerate(traj):
        assert t["info"]["iterations"] == k + 1 and t["info"]["stop_reason"] == rr.ITERATION_LIMIT
        assert t["lam"] == [1e-3, 1e-3 / 10.0, 1e-3 / 10.0 / 10.0][k]
        # accepted: the cost fell, and the cameras are the ones before with this step applied (a refused step would leave them)
        assert t["info"]["cost_final"] < cost
        fn, Rn = cases.apply_delta(flavour, f, R, t["delta"], anchor)
        assert Rn.tobytes() == t["R"].tobytes() and (f is None or fn.tobytes() == t["f"].tobytes())
        # away from the rounding floor: the step is far above step_tol and the cost moves by far more than its own rounding
        assert np.max(np.abs(t["delta"])) > 1e4 * 1e-10 and cost - t["info"]["cost_final"] > 1e6 * 2.0 ** -52 * cost
        f, R, cost = t["f"], t["R"], t["info"]["cost_final"]
    assert cases.multi_bound(traj) < 1e-9 and traj[0]["bound"] >= max(t["bound"] for t in traj[1:]) / 2


# ---- 4. refused pivots ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", cases.FLAVOURS)
def test_the_degenerate_pair_has_an_exact_zero_on_the_diagonal(flavour):
    f0, R0, M, kw = cases.degenerate_pair(flavour)
    H = rr.accumulate(R0, M)[1] if flavour == "rot" else fr.accumulate(f0, R0, M)[1]
    B = 3 if flavour == "rot" else 4
    z = B + 2                                             # view 1's rotation about z
    assert H[z, z] == 0.0 and not H[z].any() and not H[:, z].any()
    assert all(H[k, k] > 0 for k in range(2 * B) if k != z)
    for lam in (1e-3, 1e3, 1e12):
        assert H[z, z] + lam * H[z, z] == 0.0              # no damping lifts it
        with pytest.raises(np.linalg.LinAlgError):
            A, _ = cases.ref_step(flavour, f0, R0, M, kw, lam)
            np.linalg.cholesky(A)


@pytest.mark.parametrize("flavour", cases.FLAVOURS)
def test_the_references_on_the_degenerate_inputs(flavour):
    lam, count = 1e-3, 0
    while lam <= 1e12:
        lam *= 10.0; count += 1
    assert count == 16                                     # 1e-3 times ten until it exceeds 1e12: the same IEEE sequence wherever it runs
    for which, anchor, max_iters, want in (("pair", 0, 50, (16, rr.STALLED)), ("pair", 0, 10, (10, rr.ITERATION_LIMIT)), ("pair", 0, 1, (1, rr.ITERATION_LIMIT)),
                                           ("three", 0, 50, (16, rr.STALLED))):
        f0, R0, M, kw, (f, R, info) = cases.degenerate_ref(flavour, which, max_iters, anchor)
        assert (info["iterations"], info["stop_reason"]) == want, (which, max_iters, info)
        assert R.tobytes() == R0.tobytes() and (f is None or f.tobytes() == f0.tobytes())
        assert info["cost_final"] == info["cost_initial"] > 0 and info["outliers"] == 0
        assert info["matches_used"] == len(M) and info["pairs_ignored"] == 0


def test_with_the_degenerate_view_held_the_same_matches_converge():
    """B = 3, anchor 2: CONVERGED in 4 iterations.  The count is no accident of rounding: the first three steps are four orders and more above step_tol, the fourth is
    below it by a factor 1.6 where two correct implementations differ in the twelfth digit, and every cost falls by orders of magnitude."""
    f0, R0, M, kw, (f, R, info) = cases.degenerate_ref("rot", "three", 50, 2)
    assert (info["iterations"], info["stop_reason"]) == (4, rr.CONVERGED) and info["cost_final"] < 1e-20 * info["cost_initial"]
    assert R[2].tobytes() == R0[2].tobytes() and rr.angle(R[0], R0[0]) > 0.01 and rr.angle(R[1], R0[1]) > 0.01
    Rk, lam, cost = R0, 1e-3, info["cost_initial"]
    for k in range(4):
        _, delta = rr.step(Rk, M, 2, lam)
        Rk, ik = rr.refine(R0, M, **dict(kw, max_iters=k + 1))
        dmax = float(np.max(np.abs(delta)))
        assert (dmax > 1e-6) if k < 3 else (dmax < 1e-10 / 1.5), (k, dmax)
        assert ik["cost_final"] < 1e-2 * cost
        lam, cost = lam / 10.0, ik["cost_final"]
    assert Rk.tobytes() == R.tobytes()
    # and it is the same input that stalls with view 0 held
    assert [m[0:2] for m in cases.degenerate_ref("rot", "three", 50, 0)[2]] == [m[0:2] for m in M]
    assert all(np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) for a, b in zip(cases.degenerate_ref("rot", "three", 50, 0)[2], M))


# ---- 5. accumulate beyond three views ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["rot", "focal"])
@pytest.mark.parametrize("graph", ["complete", "ring"])
def test_accumulate_cases(flavour, graph):
    f, R, M, pairs = cases.accumulate_case(flavour, graph)
    B = 3 if flavour == "rot" else 4
    assert len(R) == 16 and len(M) == (360 if graph == "complete" else 96) and len(pairs) == (120 if graph == "complete" else 16)
    listed = {(min(m[0], m[1]), max(m[0], m[1])) for m in M}
    assert listed == {(min(p), max(p)) for p in pairs} and 0.2 < sum(1 for m in M if m[0] > m[1]) / len(M) < 0.45
    assert [m[:2] for m in M] != sorted(m[:2] for m in M)                 # shuffled
    h = cases.accumulate_huber(flavour, f, R, M)
    i, j, a, b = rr.unpack(M) if flavour == "rot" else fr.unpack(M)
    s = rr.terms(R, i, j, a, b, 0.0)[1] if flavour == "rot" else fr.terms(f, R, i, j, a, b, 0.0)[1]
    assert 0 < (s > h).sum() < len(s)                                      # matches on both Huber branches
    H = rr.accumulate(R, M, h)[1] if flavour == "rot" else fr.accumulate(f, R, M, h)[1]
    zero = sum(1 for p in range(15) for q in range(p + 1, 16) if not H[B * p:B * p + B, B * q:B * q + B].any())
    assert zero == (0 if graph == "complete" else 104)
    assert cases.accumulate_terms(M) == (360, 45) if graph == "complete" else cases.accumulate_terms(M) == (96, 12)
