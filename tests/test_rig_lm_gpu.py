"""The Levenberg-Marquardt step the two rig refinements share (csrc/rig_lm.hpp, k_rig_step<3> through csrc/rig.hip and k_rig_step<4> through csrc/rig_focal.hip) against
numpy, step by step: the inputs and the reference side are tests/rig_lm_cases.py, and tests/test_rig_lm_cases.py shows on the references alone that the inputs do what
these tests assume.

1. max_iters = 1 is exactly one step -- the assembly, the map from the full system to the solved one, the Cholesky in LDS, both triangular solves and the write-back of
   the trial cameras: every view count from 2 to 16, the anchor at either end and in the middle, rotations alone, a focal a view and one shared focal; the complete
   pair graph at 4 and 16 views
2. two and three steps: the lambda update, the solve from the stored system of the accepted state, the round counter
3. refused pivots: MS_RIG_STALLED after 16 refusals, MS_RIG_ITERATION_LIMIT from inside the refusal loop, and the same matches converging once the degenerate view is held

The closeness bound is derived (rig_lm_cases.step_bound), not tuned: K 2^-52 cond_2(A) |delta|_2 + 2^-50 with the reference's own A and delta of each case.  A wrong
row, sign or lambda is off by 1e-4 rad and more; the bound is 1e-10 and less."""
import math

import numpy as np
import pytest
import torch  # noqa: F401      (before the library is loaded, as in every GPU test file: the process binds to the one HIP runtime PyTorch brings)

import rig_lm_cases as cases
import rig_ref as rr

pytestmark = pytest.mark.gpu

STEP_IDS = ["%s-n%d-a%d" % c for c in cases.STEP_CASES]
_WORST = {}


def device_refine(ms, flavour, f0, R0, M, **kw):
    """-> (f or None, R, info) of the flavour's entry point"""
    kw = {{"anchor": "anchor_view"}.get(k, k): (int(v) if k == "shared_focal" else v) for k, v in kw.items()}
    if flavour == "rot":
        R, info = ms.refine_rig_rotations(R0, M, ms.rig_refine_default_params(**kw))
        return None, R, info
    return ms.refine_rig_cameras(f0, R0, M, ms.rig_focal_default_params(**kw))


def distance(f, R, rf, rR):
    """the largest angle between a device rotation and the reference's, and the largest |log| of a focal ratio"""
    d = max(rr.angle(a, b) for a, b in zip(R, rR))
    return d if f is None else max(d, float(np.max(np.abs(np.log(f / rf)))))


def all_finite(f, R, info):
    return bool(np.all(np.isfinite(R))) and (f is None or bool(np.all(np.isfinite(f)))) and all(math.isfinite(float(v)) for v in info.values())


def record(table, flavour, ratio):
    _WORST.setdefault(table, {})[flavour] = max(_WORST.get(table, {}).get(flavour, 0.0), ratio)
    return _WORST[table][flavour]


# ---- 1. one step ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", cases.FLAVOURS)
@pytest.mark.parametrize("graph, n, anchor", cases.STEP_CASES, ids=STEP_IDS)
def test_one_step_against_numpy(ms, cuda, flavour, graph, n, anchor):
    """Round 0 proposes, round 1 accepts: iterations == 1 at the iteration limit, and the output is Exp(delta) R0 (and f0 exp(d)) of the reference's step within the
    derived bound.  Measured on MI355X, the worst error / bound over the 46 cases of a flavour: rot 3.7e-3 (3.9e-17 rad of 1.05e-14), focal 3.5e-3 (7.1e-15 of 2.06e-12), shared
    2.7e-3 (2.4e-15 of 9.1e-13), all three at two views; the errors are a few 1e-16 to 1e-14 everywhere, the worst-case bound is never approached."""
    f0, R0, M, kw = cases.inputs(flavour, graph, n, anchor)
    t = cases.one_step(flavour, graph, n, anchor)
    f, R, info = device_refine(ms, flavour, f0, R0, M, max_iters=1, **kw)
    err = distance(f, R, t["f"], t["R"])
    print("%s %s n=%d anchor=%d m=%d: %.3e to the reference, bound %.3e: ratio %.2e (the flavour's worst so far %.2e); cond %.0f, |delta| %.3f, cost %.4e -> %.4e"
          % (flavour, graph, n, anchor, len(t["delta"]), err, t["bound"], err / t["bound"], record("step", flavour, err / t["bound"]), np.linalg.cond(t["A"], 2),
             np.linalg.norm(t["delta"]), info["cost_initial"], info["cost_final"]))
    assert all_finite(f, R, info)
    assert info["iterations"] == t["info"]["iterations"] == 1 and info["stop_reason"] == t["info"]["stop_reason"] == ms.RIG_ITERATION_LIMIT
    assert R[anchor].tobytes() == R0[anchor].tobytes()
    if flavour == "shared":
        assert np.all(f == f[0]) and f[0] != f0[0]             # they start equal and receive one exp(d)
    assert info["matches_used"] == len(M) and info["pairs_used"] == len(cases.pairs_of(graph, n)) and info["pairs_ignored"] == 0 and info["outliers"] == 0
    assert abs(info["cost_initial"] - t["info"]["cost_initial"]) <= (len(M) + 8) * 2.0 ** -52 * t["info"]["cost_initial"]      # two orders of one sum of squares
    assert info["cost_final"] < info["cost_initial"]
    assert err <= t["bound"]


# ---- 2. two and three steps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", cases.FLAVOURS)
@pytest.mark.parametrize("n, iters", cases.MULTI_CASES)
def test_two_and_three_steps_against_numpy(ms, cuda, flavour, n, iters):
    """The reference takes `iters` accepted steps and ends at the iteration limit; the device must as well, within the sum of the steps' bounds along the reference's
    path, doubled for what an earlier difference does to the later steps.  These runs end far from the rounding floor (the last step is 1e-6 and more against a
    step_tol of 1e-10, and each cost falls by far more than its rounding), so what the other rig test files say about iteration counts -- that the stop step at the
    rounding floor depends on the order of the sums -- does not apply here: the counts are compared for equality.
    Measured on MI355X, the worst error / bound: rot 3.7e-4 (1.1e-16 rad of 2.9e-13), focal 1.3e-4 (6.7e-16 of 5.2e-12), shared 8.7e-5 (2.2e-16 of 2.6e-12), all at
    three views and three steps."""
    anchor = n // 2
    f0, R0, M, kw = cases.inputs(flavour, "ring", n, anchor)
    traj = cases.trajectory(flavour, "ring", n, anchor, iters)
    bound = cases.multi_bound(traj)
    f, R, info = device_refine(ms, flavour, f0, R0, M, max_iters=iters, **kw)
    err = distance(f, R, traj[-1]["f"], traj[-1]["R"])
    print("%s n=%d %d steps: %.3e to the reference, bound %.3e: ratio %.2e (the flavour's worst so far %.2e); cost %.4e -> %.4e (reference %.4e)"
          % (flavour, n, iters, err, bound, err / bound, record("multi", flavour, err / bound), info["cost_initial"], info["cost_final"], traj[-1]["info"]["cost_final"]))
    assert all_finite(f, R, info)
    assert info["iterations"] == traj[-1]["info"]["iterations"] == iters and info["stop_reason"] == traj[-1]["info"]["stop_reason"] == ms.RIG_ITERATION_LIMIT
    assert R[anchor].tobytes() == R0[anchor].tobytes()
    if flavour == "shared":
        assert np.all(f == f[0])
    assert info["cost_final"] < info["cost_initial"] and info["outliers"] == 0
    assert err <= bound


# ---- 3. refused pivots ------------------------------------------------------------------------------------------------------------------------------------
def refused(ms, flavour, which, max_iters, anchor=0):
    """run a degenerate input on the device and assert everything a run that never leaves its start has in common -> the device's info, the reference's"""
    f0, R0, M, kw, (rf, rR, ri) = cases.degenerate_ref(flavour, which, max_iters, anchor)
    f, R, info = device_refine(ms, flavour, f0, R0, M, **kw)
    print("%s %s anchor=%d max_iters=%d: stop %d after %d iterations (reference %d after %d), cost %r -> %r" % (flavour, which, anchor, max_iters, info["stop_reason"],
                                                                                                          info["iterations"], ri["stop_reason"], ri["iterations"],
                                                                                                          info["cost_initial"], info["cost_final"]))
    assert all_finite(f, R, info)
    assert info["stop_reason"] == ri["stop_reason"] and info["iterations"] == ri["iterations"]
    assert R.tobytes() == R0.tobytes() and (f is None or f.tobytes() == f0.tobytes())
    assert info["cost_final"] == info["cost_initial"] > 0 and info["outliers"] == 0
    assert info["matches_used"] == len(M) and info["pairs_ignored"] == 0 and info["max_rotation_rad"] == 0.0
    return info, ri


@pytest.mark.parametrize("flavour", cases.FLAVOURS)
def test_a_zero_pivot_stalls_after_16_refusals(ms, cuda, flavour):
    """one diagonal entry of H is exactly zero and hv + lam hv leaves it zero: every attempt is refused, lambda is multiplied by ten and an iteration counted until
    lambda exceeds 1e12 -- 16 times, the same IEEE sequence on either side"""
    info, _ = refused(ms, flavour, "pair", 50)
    assert (info["stop_reason"], info["iterations"]) == (ms.RIG_STALLED, 16)


@pytest.mark.parametrize("flavour", cases.FLAVOURS)
@pytest.mark.parametrize("max_iters", [10, 1])
def test_the_iteration_limit_inside_the_refusal_loop(ms, cuda, flavour, max_iters):
    info, _ = refused(ms, flavour, "pair", max_iters)
    assert (info["stop_reason"], info["iterations"]) == (ms.RIG_ITERATION_LIMIT, max_iters)


@pytest.mark.parametrize("flavour", cases.FLAVOURS)
def test_a_zero_pivot_behind_good_columns_refuses_the_whole_step(ms, cuda, flavour):
    """three views, anchor 0: view 1's columns factor, view 2's rotation about z is the zero pivot behind them, and no part of the step is applied"""
    info, _ = refused(ms, flavour, "three", 50, anchor=0)
    assert (info["stop_reason"], info["iterations"]) == (ms.RIG_STALLED, 16)


def test_the_same_matches_converge_with_the_degenerate_view_held(ms, cuda):
    """B = 3, anchor 2: the refusal came from the pivot, not from the input as a whole.  The reference ends CONVERGED in 4 iterations, its steps 0.17, 5.6e-3, 1.8e-6
    and 5.9e-11 against a step_tol of 1e-10 (tests/test_rig_lm_cases.py): no step is near the threshold, so the count is compared for equality."""
    f0, R0, M, kw, (rf, rR, ri) = cases.degenerate_ref("rot", "three", 50, 2)
    f, R, info = device_refine(ms, "rot", f0, R0, M, **kw)
    err = distance(None, R, None, rR)
    print("anchor 2: stop %d after %d iterations (reference %d after %d), %.3e rad to the reference, cost %.3e -> %.3e" % (info["stop_reason"], info["iterations"],
                                                                                                                     ri["stop_reason"], ri["iterations"], err,
                                                                                                                     info["cost_initial"], info["cost_final"]))
    assert (info["stop_reason"], info["iterations"]) == (ri["stop_reason"], ri["iterations"]) == (ms.RIG_CONVERGED, 4)
    assert R[2].tobytes() == R0[2].tobytes() and err <= 1e-12 and info["cost_final"] < 1e-20 * info["cost_initial"]
