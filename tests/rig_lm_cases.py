"""Inputs and the reference side of the tests of the rig Levenberg-Marquardt step (csrc/rig_lm.hpp: tests/test_rig_lm_cases.py without a GPU, tests/test_rig_lm_gpu.py
with one).  numpy only; every case is a pure function of its key (fixed seeds), and every reference answer is computed once and shared.

Three flavours of the one step kernel: "rot" (B = 3, rig_ref), "focal" (B = 4, a focal a view) and "shared" (B = 4, one focal), both rig_focal_ref.

STEP_CASES   (graph, n, anchor): the ring pairs with 6 matches a pair for every n of 2 .. 16 and the anchors 0, n // 2 and n - 1 -- every size 3 (n - 1), 4 n - 3 and
             3 (n - 1) + 1 of the solved system, 3 .. 61 -- and the complete pair graph with 3 matches a pair at n = 4 and n = 16 (120 pairs)
MULTI_CASES  (n, iters): two and three steps at n = 3, 6, 16 with the middle anchor
degenerate inputs: one diagonal entry of H is exactly zero, which the damping hv + lam hv cannot lift, so every pivot attempt is refused

Layouts: two views 40 degrees apart; three and four views, and the views of a complete graph, on a cone of 25 degrees about the z axis (every pair of views shares
a field of view, which centred pixels need); from five views the ideal ring of rig_ref.  The start is the layout, the truth up to 5 degrees off about each axis."""
import math

import numpy as np

import rig_focal_ref as fr
import rig_ref as rr

FLAVOURS = ("rot", "focal", "shared")
LAM0 = 1e-3                                 # the lambda of the first proposal
RING_MATCHES, COMPLETE_MATCHES = 6, 3
STEP_CASES = [("ring", n, a) for n in range(2, 17) for a in sorted({0, n // 2, n - 1})] + [("complete", 4, 2), ("complete", 16, 8)]
MULTI_CASES = [(n, k) for n in (3, 6, 16) for k in (2, 3)]


def solved_size(flavour, n):
    return {"rot": 3 * (n - 1), "focal": 4 * n - 3, "shared": 3 * (n - 1) + 1}[flavour]


def cone(n, tilt_deg=25.0):
    t = math.radians(tilt_deg)
    return np.array([rr.exp_so3(np.array([0.0, 0.0, 2.0 * math.pi * v / n])) @ rr.exp_so3(np.array([t, 0.0, 0.0])) for v in range(n)])


def layout(graph, n):
    if n == 2:
        return np.array([np.eye(3), rr.rot_y(math.radians(40.0))])
    return cone(n) if graph == "complete" or n < 5 else rr.ring(n)


def pairs_of(graph, n):
    return rr.ring_pairs(n) if graph == "ring" else [(i, j) for i in range(n - 1) for j in range(i + 1, n)]


_INPUTS = {}


def inputs(flavour, graph, n, anchor):
    """-> (f0 or None, R0, matches, keyword arguments of the refinement but max_iters), the same objects at every call: read only"""
    key = (flavour, graph, n, anchor)
    if key not in _INPUTS:
        rng = np.random.default_rng([n, anchor, graph == "complete"])
        R0 = layout(graph, n)
        Rt = rr.perturbed(R0, rng, 5.0)
        pairs = pairs_of(graph, n)
        per_pair, min_pair = (RING_MATCHES, 4) if graph == "ring" else (COMPLETE_MATCHES, 1)
        if flavour == "rot":
            _INPUTS[key] = (None, R0, rr.make_matches(Rt, pairs, per_pair, rng, noise=5e-4), dict(anchor=anchor, min_pair_matches=min_pair))
        else:
            ft = rng.uniform(380.0, 420.0, n)
            M = fr.make_px_matches(ft, Rt, pairs, per_pair, rng, noise_px=0.05, spread_deg=15.0)
            _INPUTS[key] = (np.full(n, 400.0), R0, M, dict(anchor=anchor, shared_focal=flavour == "shared", min_pair_matches=min_pair))
    return _INPUTS[key]


# ---- the reference side ---------------------------------------------------------------------------------------------------------------------------------
def ref_refine(flavour, f0, R0, M, **kw):
    """-> (f or None, R, info) of the flavour's reference"""
    if flavour == "rot":
        R, info = rr.refine(R0, M, **kw)
        return None, R, info
    return fr.refine(f0, R0, M, **kw)


def ref_step(flavour, f, R, M, kw, lam):
    """-> (A, delta) of one proposal at the cameras (f, R)"""
    if flavour == "rot":
        return rr.step(R, M, kw["anchor"], lam)
    return fr.step(f, R, M, kw["anchor"], kw["shared_focal"], lam)


def step_bound(A, delta, matches_used):
    """How far two correct solutions of one proposal may lie apart, in radians and in log focal.  Both sides solve (H + lam diag H) d = -g; their H and g differ by the
    order of the sums alone, relatively (matches + 8) 2^-52 (the bound of the accumulate tests); Cholesky with two triangular solves, and LAPACK's LU behind
    numpy.linalg.solve, each have a backward error of the order (3 m + 1) 2^-52 |A|.  A relative perturbation e of the system moves its solution by cond_2(A) e |d|, so
    K = 2 (3 m + 1) + 2 (matches + 8) of them by K 2^-52 cond_2(A) |d|_2; 2^-50 covers Exp, exp and the measurement of the angle."""
    m = len(delta)
    K = 2 * (3 * m + 1) + 2 * (matches_used + 8)
    return K * 2.0 ** -52 * float(np.linalg.cond(A, 2)) * float(np.linalg.norm(delta)) + 2.0 ** -50


_TRAJ = {}


def trajectory(flavour, graph, n, anchor, iters, **over):
    """The reference run with max_iters = 1 .. iters, each from the start: entry k - 1 is dict(f, R, info, A, delta, lam, bound) of the run of k iterations, with the
    proposal (A, delta, lam) that led from the run before to it and that proposal's step_bound.  lam follows the accept rule (a tenth after every accepted step): the
    entries describe the reference's path only while every step was accepted, which tests/test_rig_lm_cases.py asserts.  over: keyword arguments that replace the case's."""
    key = (flavour, graph, n, anchor, tuple(sorted(over.items())))
    out = _TRAJ.setdefault(key, [])
    f0, R0, M, kw = inputs(flavour, graph, n, anchor)
    kw = dict(kw, **over)
    while len(out) < iters:
        k = len(out)
        f, R, lam = (f0, R0, LAM0) if k == 0 else (out[-1]["f"], out[-1]["R"], max(out[-1]["lam"] / 10.0, 1e-12))
        A, delta = ref_step(flavour, f, R, M, kw, lam)
        fk, Rk, info = ref_refine(flavour, f0, R0, M, max_iters=k + 1, **kw)
        out.append(dict(f=fk, R=Rk, info=info, A=A, delta=delta, lam=lam, bound=step_bound(A, delta, info["matches_used"])))
    return out[:iters]


def one_step(flavour, graph, n, anchor):
    return trajectory(flavour, graph, n, anchor, 1)[0]


def multi_bound(traj):
    """the sum of the steps' bounds along the reference's path, doubled: a difference an earlier step left is carried through the later ones, which near the
    minimum do not enlarge it (the Gauss-Newton map contracts there), so it counts at most once more"""
    return 2.0 * sum(t["bound"] for t in traj)


def apply_delta(flavour, f, R, delta, anchor):
    """the cameras Exp(delta) R and f exp(d) from a solved step, by rules written apart from the references' own (rig_ref's keep, rig_focal_ref's selection)"""
    n = len(R)
    shared = flavour == "shared"
    Rn = np.array(R, np.float64); fn = None if f is None else np.array(f, np.float64)
    pos = 0
    for v in range(n):
        if v != anchor:
            Rn[v] = rr.exp_so3(delta[pos:pos + 3]) @ R[v]
            pos += 3
        if flavour == "focal":
            fn[v] = f[v] * math.exp(delta[pos])
            pos += 1
    if shared:
        fn = np.array([fv * math.exp(delta[pos]) for fv in f])
        pos += 1
    assert pos == len(delta)
    return fn, Rn


# ---- refused pivots -------------------------------------------------------------------------------------------------------------------------------------
def degenerate_pair(flavour):
    """two views at the identity, four copies of one match whose second ray is e_z exactly: H_jj[zz] = w (0 0 + 0 0) = 0.  -> f0, R0, matches, keywords (anchor 0)"""
    R0 = np.array([np.eye(3), np.eye(3)])
    if flavour == "rot":
        return None, R0, [(0, 1, np.array([0.0, math.sin(0.1), math.cos(0.1)]), np.array([0.0, 0.0, 1.0]))] * 4, dict(anchor=0)
    return np.full(2, 400.0), R0, [(0, 1, np.array([30.0, 40.0]), np.array([0.0, 0.0]))] * 4, dict(anchor=0, shared_focal=flavour == "shared")


def degenerate_behind_good_columns(flavour, anchor):
    """three views at the identity: a healthy pair (0, 1) of 6 exact matches of a rig 5 degrees off, and the pair (1, 2) of degenerate_pair's matches.  Anchor 0: the
    zero pivot, view 2's z, sits behind view 1's good columns.  Anchor 2: the degenerate view is held and the same matches determine the other two."""
    rng = np.random.default_rng(31)
    R0 = np.array([np.eye(3)] * 3)
    Rt = rr.perturbed(R0, rng, 5.0)
    _, _, D, kw = degenerate_pair(flavour)
    D = [(1, 2, a, b) for _, _, a, b in D]
    if flavour == "rot":
        return None, R0, rr.make_matches(Rt, [(0, 1)], 6, rng) + D, dict(kw, anchor=anchor)
    return np.full(3, 400.0), R0, fr.make_px_matches(np.full(3, 400.0), Rt, [(0, 1)], 6, rng, spread_deg=15.0) + D, dict(kw, anchor=anchor)


_DEGEN = {}


def degenerate_ref(flavour, which, max_iters, anchor=0):
    """-> (f0, R0, matches, keywords with max_iters, the reference's (f, R, info)), computed once"""
    key = (flavour, which, max_iters, anchor)
    if key not in _DEGEN:
        f0, R0, M, kw = degenerate_pair(flavour) if which == "pair" else degenerate_behind_good_columns(flavour, anchor)
        kw = dict(kw, max_iters=max_iters)
        _DEGEN[key] = (f0, R0, M, kw, ref_refine(flavour, f0, R0, M, **kw))
    return _DEGEN[key]


# ---- accumulate beyond three views ----------------------------------------------------------------------------------------------------------------------
def accumulate_case(flavour, graph):
    """16 views, the complete graph (120 pairs of 3 matches) or the ring (16 pairs of 6), the matches shuffled and a third of them listed as (j, i); the cameras are
    the layout up to 5 degrees off, the matches those of another rig as far off with noise.  -> f or None, R, matches, pairs"""
    n = 16
    rng = np.random.default_rng([16, graph == "complete", flavour == "rot"])
    R = rr.perturbed(layout(graph, n), rng, 5.0)
    Rt = rr.perturbed(layout(graph, n), rng, 5.0)
    pairs = pairs_of(graph, n)
    per_pair = COMPLETE_MATCHES if graph == "complete" else RING_MATCHES
    if flavour == "rot":
        f, M = None, rr.make_matches(Rt, pairs, per_pair, rng, noise=2e-3)
    else:
        f = 400.0 * (1 + rng.uniform(-0.05, 0.05, n))
        M = fr.make_px_matches(f * (1 + rng.uniform(-0.03, 0.03, n)), Rt, pairs, per_pair, rng, noise_px=0.7, spread_deg=15.0)
    M = [M[k] for k in rng.permutation(len(M))]
    M = [(vb, va, b, a) if rng.uniform() < 1 / 3 else (va, vb, a, b) for va, vb, a, b in M]
    return f, R, M, pairs


def accumulate_huber(flavour, f, R, M):
    """the median residual at the cameras: a Huber threshold with matches on both of its branches"""
    i, j, a, b = rr.unpack(M) if flavour == "rot" else fr.unpack(M)
    s = rr.terms(R, i, j, a, b, 0.0)[1] if flavour == "rot" else fr.terms(f, R, i, j, a, b, 0.0)[1]
    return float(np.sort(s)[len(s) // 2 - 1])


def accumulate_terms(M):
    """how many terms the cost sums, and the most any entry of H or g does: the matches of the view with the most"""
    per_view = {}
    for va, vb, _, _ in M:
        per_view[va] = per_view.get(va, 0) + 1; per_view[vb] = per_view.get(vb, 0) + 1
    return len(M), max(per_view.values())
