"""The inverse lens model and the focal-and-rotation refinement under fixed lenses on the GPU (csrc/lens.hip: k_lens_unproject; csrc/rig_lens.hip) against the host
call and the numpy reference of tests/rig_lens_ref.py.

1. ms_lens_unproject_points against ms_lens_unproject, point counts around the wave and the workgroup
2. ms_rig_lens_accumulate per op, three views behind NONE, BROWN and FISH: every entry of cost, H and g within the bound for two summation orders plus the measured
   share of sin / cos / hypot and the Newton stop
3. all-NONE lenses: the bits of ms_rig_focal_accumulate and ms_refine_rig_cameras, on the "focal" cases of tests/rig_lm_cases.py
4. exact recovery from wrong focals and rotations, per-view and shared focal, fisheye matches past 90 degrees
5. noise and outliers with Huber against the reference, an anchor other than view 0
6. a trial that pushes a pixel out of its lens's field is rejected
7. determinism
8. the context form, ms_refine_rig_focals_lens: lens contexts, analytic contexts (the bits of ms_refine_rig_focals), state and refusals
9. from pixels: 8 views rendered through fisheye lenses, ORB on the source images, ratio test, RANSAC on undistorted pixels, ms_refine_rig_cameras_lens"""
import math

import numpy as np
import pytest

import lens_ref as L
import rig_focal_ref as fr
import rig_lens_ref as lr
import rig_lm_cases as lm_cases
import rig_ref as rr
import synth
from helpers import to_dev

pytestmark = pytest.mark.gpu

K_PTS = [[205.5, 0.0, 321.25], [0.0, 201.75, 238.5], [0.0, 0.0, 1.0]]


def to_lenses(ms, lenses):
    return [L.to_ms(ms, l) for l in lenses]


def device_refine(ms, f_in, R_in, lenses, M, **kw):
    kw = {{"anchor": "anchor_view"}.get(k, k): (int(v) if k == "shared_focal" else v) for k, v in kw.items()}
    return ms.refine_rig_cameras_lens(f_in, R_in, to_lenses(ms, lenses), M, ms.rig_focal_default_params(**kw))


def max_angle(A, B):
    return max(rr.angle(a, b) for a, b in zip(A, B))


_REF = {}


def ref_refine(key, f_in, R_in, lenses, M, **kw):
    """the reference's answer for a named case, computed once"""
    if key not in _REF:
        _REF[key] = lr.refine(f_in, R_in, lenses, M, **kw)
    return _REF[key]


# ---- 1. ms_lens_unproject_points --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["none", "brown", "fish"])
def test_unproject_points_against_the_host_call(ms, cuda, name, n):
    """float pixels inside the field and, scaled away from the principal point, outside it, never within 1e-3 of the limit.  Host and device run the same code: rays
    within 1e-12 (libm and the last Newton round), flags equal, unseen points zero."""
    lens = {"none": L.NONE, "brown": L.BROWN, "fish": L.FISH}[name]; ml = L.to_ms(ms, lens)
    rng = np.random.default_rng(400 + n)
    mt = L.max_theta(lens) or math.radians(80.0)
    th = rng.uniform(0.0, 0.999 * mt, n); ph = rng.uniform(0, 2 * math.pi, n)
    px, py, seen = L.project(K_PTS, lens, np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th))
    assert seen.all()
    if name != "none":
        # every third point: the rim's pixel of its azimuth pushed outwards by 1 to 50 % (both test profiles rise for ever, so it lies past the limit)
        rx, ry, _ = L.project(K_PTS, lens, math.sin(0.999 * mt) * np.cos(ph), math.sin(0.999 * mt) * np.sin(ph), np.full(n, math.cos(0.999 * mt)))
        s = rng.uniform(1.01, 1.5, n)
        out = np.arange(n) % 3 == 1
        px = np.where(out, K_PTS[0][2] + s * (rx - K_PTS[0][2]), px); py = np.where(out, K_PTS[1][2] + s * (ry - K_PTS[1][2]), py)
    if n >= 63:
        px[0], py[0] = K_PTS[0][2], K_PTS[1][2]                   # the image centre
    P = np.stack([px, py], -1).astype(np.float32)
    rays, flags = ms.lens_unproject_points(K_PTS, ml, P)
    assert rays.shape == (n, 3) and flags.shape == (n,)
    worst = 0.0
    for k in range(n):
        h, s = ms.lens_unproject(K_PTS, ml, (float(P[k, 0]), float(P[k, 1])))
        assert bool(flags[k]) == s, (k, P[k])
        assert s or rays[k].tolist() == [0.0, 0.0, 0.0]
        worst = max(worst, float(np.max(np.abs(rays[k] - h))))
    print("%s n=%d: %d seen, %d not; worst |device - host| %.3e" % (name, n, int(flags.sum()), int((~flags).sum()), worst))
    assert worst <= 1e-12
    assert name == "none" or n < 3 or (0 < flags.sum() < n)
    assert n < 63 or rays[0].tolist() == [0.0, 0.0, 1.0]


# ---- 2. accumulate, per op --------------------------------------------------------------------------------------------------------------------------
ACC_LENSES = [L.NONE, L.BROWN, L.FISH]


def accumulate_case(m):
    rng = np.random.default_rng(600 + m)
    R = rr.perturbed(rr.ring(6)[:3], rng, 5.0)
    f = np.array([400.0, 431.5, 388.25])
    M = lr.make_lens_matches(f * (1 + rng.uniform(-0.03, 0.03, 3)), rr.perturbed(rr.ring(6)[:3], rng, 5.0), ACC_LENSES, [(0, 1), (1, 2)], [m, 5], rng, noise_px=0.7)
    M = [M[k] for k in rng.permutation(len(M))]
    M = [(vb, va, b, a) if rng.uniform() < 1 / 3 else (va, vb, a, b) for va, vb, a, b in M]
    i, j, a, b = fr.unpack(M)
    s = lr.terms(f, R, ACC_LENSES, i, j, a, b, 0.0)[1]
    return f, R, M, float(np.sort(s)[len(s) // 2 - 1])


@pytest.mark.parametrize("m", [1, 64, 65, 257])
def test_accumulate_per_op(ms, cuda, m):
    """3 views with three focals behind NONE, BROWN and FISH; pair (0, 1) with m matches, pair (1, 2) with 5, pair (0, 2) with none; shuffled, a third listed as (j, i);
    Huber off, then at the median residual.  Bound per entry: ((m + 8) + T) 2^-52 S, S the sum of the terms' absolute values.  (m + 8): two summation orders of the
    same rounded terms (tests/test_rig_focal_gpu.py).  T: what sin / cos / hypot and the Newton stop may add, which the contract does not fix to the bit.  It is
    measured, not guessed: rig_lens_ref.term_deviation evaluates the reference's terms in float64 and in numpy.longdouble on the same inputs; the largest per-entry
    deviation, in units of 2^-52 S, is how far a correctly rounded float64 evaluation lies from the exact terms, and T is 8 times it (device libm is documented as a
    couple of ulp where glibc is under one, and the stop rule allows one more).  The residual r = m (p - q) cancels two to three digits of p, which is why the figure is in
    tens and not near 1.  Measured on the CPU (profiles/rig_lens.jsonl, "term_deviation"), deviation -> T for m = 1, 64, 65, 257:
    Huber off 36.0 -> 288, 12.8 -> 102, 7.6 -> 61, 4.7 -> 38; Huber at the median 31.5 -> 252, 11.4 -> 91, 8.3 -> 66, 4.4 -> 35."""
    f, R, M, h_mid = accumulate_case(m)
    assert any(va > vb for va, vb, _, _ in M) or m == 1
    assert lr.all_seen(f, R, ACC_LENSES, M)
    i, j, a, b = fr.unpack(M)
    s = lr.terms(f, R, ACC_LENSES, i, j, a, b, 0.0)[1]
    assert 0 < (s > h_mid).sum() < len(s)                     # matches on both Huber branches
    for h in (0.0, h_mid):
        dev = lr.term_deviation(f, R, ACC_LENSES, M, h)
        T = 8.0 * dev
        cost, H, g = ms.rig_lens_accumulate(f, R, to_lenses(ms, ACC_LENSES), M, h)
        rc, rH, rg, sc, sH, sg = lr.accumulate(f, R, ACC_LENSES, M, h, with_abs=True)
        tol = ((m + 8) + T) * 2.0 ** -52
        print("m=%d h=%g: term deviation %.1f, T %.1f; cost %.3e of %.3e, H %.3e, g %.3e (max |diff| / S)" % (m, h, dev, T, abs(cost - rc) / sc, tol,
              np.max(np.abs(H - rH) / np.maximum(sH, 1e-300)), np.max(np.abs(g - rg) / np.maximum(sg, 1e-300))))
        assert abs(cost - rc) <= tol * sc
        assert np.all(np.abs(H - rH) <= tol * sH) and np.all(np.abs(g - rg) <= tol * sg)
        assert np.array_equal(H, H.T) and not H[0:4, 8:12].any() and H[4:8, 4:8].all() and H[0:4, 4:8].all()


# ---- 3. all-NONE lenses: the pinhole path bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["complete", "ring"])
def test_all_none_accumulate_is_the_pinhole_call_bit_for_bit(ms, cuda, graph):
    f, R, M, _ = lm_cases.accumulate_case("focal", graph)
    none = [None] * len(f)
    for h in (0.0, lm_cases.accumulate_huber("focal", f, R, M)):
        a = ms.rig_lens_accumulate(f, R, none, M, h); b = ms.rig_focal_accumulate(f, R, M, h)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("flavour", ["focal", "shared"])
@pytest.mark.parametrize("case", [("ring", 2, 0), ("ring", 3, 1), ("ring", 6, 3), ("ring", 16, 15), ("complete", 4, 2), ("complete", 16, 8)], ids=lambda c: "%s%d-%d" % c)
def test_all_none_refinement_is_the_pinhole_call_bit_for_bit(ms, cuda, flavour, case):
    f0, R0, M, kw = lm_cases.inputs(flavour, *case)
    prm = ms.rig_focal_default_params(anchor_view=kw["anchor"], shared_focal=int(kw["shared_focal"]), min_pair_matches=kw["min_pair_matches"], huber_px=0.05)
    a = ms.refine_rig_cameras_lens(f0, R0, [None] * len(f0), M, prm); b = ms.refine_rig_cameras(f0, R0, M, prm)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert a[2]["iterations"] >= 2


# ---- 4. exact recovery ------------------------------------------------------------------------------------------------------------------------------
REC_LENSES = [L.FISH, L.FISH, L.BROWN, L.NONE, L.BROWN, L.FISH]


def recovery_case(shared):
    """6 views on the ring behind FISH, FISH, BROWN, NONE, BROWN, FISH.  The two all-fisheye pairs get rays up to 98 degrees off an axis.  The start: the ideal ring,
    the focals 20 and 15 % high in turn (shared: 30 % high) -- high, because at a focal below the truth the rim's pixels lie outside the lens's field."""
    rng = np.random.default_rng(50 + shared)
    R0 = rr.ring(6); Rt = rr.perturbed(R0, rng, 2.0)
    ft = np.full(6, 400.0) if shared else 400.0 * (1 + rng.uniform(-0.05, 0.05, 6))
    f0 = np.full(6, 520.0) if shared else ft * np.where(np.arange(6) % 2, 1.15, 1.2)
    pairs = rr.ring_pairs(6)
    M = []
    for p in pairs:
        wide = all(REC_LENSES[v][0] == "fisheye" for v in p)
        M += lr.make_lens_matches(ft, Rt, REC_LENSES, [p], 40, rng, spread_deg=60.0 if wide else 15.0)
    return f0, R0, ft, Rt, pairs, M


def theta_deg(ft, lenses, M):
    """the angle of every fisheye pixel's ray to its axis at the focals ft, in degrees"""
    out = []
    for va, vb, a, b in M:
        for v, p in ((va, a), (vb, b)):
            if lenses[v][0] == "fisheye":
                ray, seen = lr.unproject(np.diag([ft[v], ft[v], 1.0]), lenses[v], p[0], p[1])
                out.append(math.degrees(math.atan2(math.hypot(ray[0, 0], ray[0, 1]), ray[0, 2])))
    return np.array(out)


@pytest.mark.parametrize("shared", [False, True], ids=["per-view", "shared"])
def test_exact_recovery(ms, cuda, shared):
    """exact matches made with the FORWARD model have the true cameras as a zero of the cost.  The device ends within 1e-10 of the reference (the project's bound for
    the sibling refinements) and no further from the truth than 4 times the reference's own error plus 1e-12."""
    f0, R0, ft, Rt, pairs, M = recovery_case(shared)
    th = theta_deg(ft, REC_LENSES, M)
    assert ((th > 90.0) & (th < 100.0)).sum() >= 5, "no fisheye match past 90 degrees"
    kw = dict(anchor=0, shared_focal=shared, step_tol=1e-13)
    rf, rR, ri = ref_refine(("rec", shared), f0, R0, REC_LENSES, M, **kw)
    want = rr.expected(R0, Rt, 0)
    ref_err_R = max_angle(rR, want); ref_err_f = float(np.max(np.abs(rf / ft - 1.0)))
    f, R, info = device_refine(ms, f0, R0, REC_LENSES, M, **kw)
    err_R = max_angle(R, want); err_f = float(np.max(np.abs(f / ft - 1.0)))
    d = max_angle(R, rR); df = float(np.max(np.abs(f / rf - 1.0)))
    print("shared=%s: %d fisheye rays past 90 degrees (max %.2f); device to the truth %.3e focal, %.3e rad (reference %.3e, %.3e); device to reference %.3e, %.3e rad; %d "
          "iterations, stop %d, cost %.3e -> %.3e" % (shared, int((th > 90).sum()), th.max(), err_f, err_R, ref_err_f, ref_err_R, df, d, info["iterations"], info["stop_reason"],
                                                   info["cost_initial"], info["cost_final"]))
    assert d <= 1e-10 and df <= 1e-10
    assert err_f <= 4.0 * ref_err_f + 1e-12 and err_R <= 4.0 * ref_err_R + 1e-12
    assert R[0].tobytes() == R0[0].tobytes() and (not shared or np.all(f == f[0]))
    assert info["matches_used"] == len(M) and info["pairs_used"] == len(pairs) and info["outliers"] == 0 and info["cost_final"] <= info["cost_initial"]
    assert lr.all_seen(f, R, REC_LENSES, M)


# ---- 5. noise and outliers --------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_rig_focal_gpu.py (see there for what 1e-10 between two correct implementations asks of the noise level), behind lenses
NOISY = {
    "huber": dict(noise_px=0.02, outlier_frac=0.15, huber_px=0.1, shared=False, anchor=4),
    "huber-shared": dict(noise_px=0.02, outlier_frac=0.15, huber_px=0.1, shared=True, anchor=2),
}


def noisy_case(name):
    c = NOISY[name]
    rng = np.random.default_rng(sorted(NOISY).index(name) + 270)
    R0 = rr.ring(6).copy()
    ft = np.full(6, 412.0) if c["shared"] else 400.0 * (1 + rng.uniform(-0.04, 0.04, 6))
    M = lr.make_lens_matches(ft, rr.perturbed(R0, rng, 2.0), REC_LENSES, rr.ring_pairs(6), 64, rng, noise_px=c["noise_px"], outlier_frac=c["outlier_frac"], spread_deg=15.0)
    return np.full(6, 400.0), R0, M, dict(huber_px=c["huber_px"], shared_focal=c["shared"], anchor=c["anchor"], step_tol=1e-12, max_iters=100)


@pytest.mark.parametrize("name", sorted(NOISY))
def test_noisy_matches_against_the_reference(ms, cuda, name):
    f0, R0, M, kw = noisy_case(name)
    rf, rR, ri = ref_refine(name, f0, R0, REC_LENSES, M, **kw)
    f, R, info = device_refine(ms, f0, R0, REC_LENSES, M, **kw)
    d = max_angle(R, rR); df = float(np.max(np.abs(f / rf - 1.0)))
    print("%s: %.3e rad and %.3e relative focal between device and reference; cost %.6e -> %.6e (reference %.6e); outliers %d (reference %d); iterations %d (reference %d); "
          "focals %s" % (name, d, df, info["cost_initial"], info["cost_final"], ri["cost_final"], info["outliers"], ri["outliers"], info["iterations"], ri["iterations"], f))
    assert d <= 1e-10 and df <= 1e-10
    assert info["cost_final"] <= info["cost_initial"]
    assert abs(info["outliers"] - ri["outliers"]) <= 2 and info["outliers"] > 0
    assert info["matches_used"] == ri["matches_used"] and info["pairs_used"] == ri["pairs_used"]
    assert R[kw["anchor"]].tobytes() == R0[kw["anchor"]].tobytes()


# ---- 6. a trial that leaves the lens's field ----------------------------------------------------------------------------------------------------------
def edge_case():
    """3 fisheye views, exact matches of cameras whose shared focal is 400, the start at 420: the first step lowers the focal towards 400.  One more match has its
    pixel in view 0 at 1 - 1e-4 of the field's end AT the focal 420: any focal below 419.96 loses it."""
    rng = np.random.default_rng(77)
    lenses = [L.FISH] * 3
    R0 = rr.ring(6)[:3].copy(); Rt = rr.perturbed(R0, rng, 1.0)
    ft = np.full(3, 400.0); f0 = np.full(3, 420.0)
    M = lr.make_lens_matches(ft, Rt, lenses, [(0, 1), (1, 2)], 30, rng, spread_deg=15.0)
    a = 420.0 * float(lr.limit(L.FISH)) * (1.0 - 1e-4) * np.array([math.cos(0.3), math.sin(0.3)])
    ray, seen = lr.unproject(np.diag([420.0, 420.0, 1.0]), L.FISH, a[0], a[1])
    assert seen[0]
    b, seen = lr.centred_pixels(420.0, L.FISH, (R0[1].T @ R0[0] @ ray[0])[None, :])
    assert seen[0]
    return f0, R0, lenses, M + [(0, 1, a, b[0])]


def test_a_trial_that_loses_a_pixel_is_rejected(ms, cuda):
    f0, R0, lenses, M = edge_case()
    assert lr.all_seen(f0, R0, lenses, M)
    # the precondition, on the CPU: the reference's first proposal does move the pixel out
    P = fr.selection(3, 0, True)
    _, H, g = lr.accumulate(f0, R0, lenses, M)
    Hr = P.T @ H @ P
    delta = np.linalg.solve(Hr + 1e-3 * np.diag(np.diag(Hr)), -(P.T @ g))
    ft, Rt = fr.apply_step(f0, R0, P @ delta)
    assert ft[0] < 419.9 and not lr.all_seen(ft, Rt, lenses, M)
    f, R, info = device_refine(ms, f0, R0, lenses, M, shared_focal=True)
    print("focal %.6f, cost %.6e -> %.6e, %d iterations, stop %d" % (f[0], info["cost_initial"], info["cost_final"], info["iterations"], info["stop_reason"]))
    assert info["cost_final"] <= info["cost_initial"] and math.isfinite(info["cost_final"])
    assert lr.all_seen(f, R, lenses, M) and f[0] >= 420.0 * (1.0 - 1.01e-4)


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits(ms, cuda):
    f0, R0, M, kw = noisy_case("huber")
    a = device_refine(ms, f0, R0, REC_LENSES, M, **kw)
    b = device_refine(ms, f0, R0, REC_LENSES, M, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    ls = to_lenses(ms, REC_LENSES)
    ca = ms.rig_lens_accumulate(f0, R0, ls, M, 1.5); cb = ms.rig_lens_accumulate(f0, R0, ls, M, 1.5)
    assert ca[0] == cb[0] and ca[1].tobytes() == cb[1].tobytes() and ca[2].tobytes() == cb[2].tobytes()


# ---- 8. the context form ----------------------------------------------------------------------------------------------------------------------------
F_CTX, F_SCENE = 80.0, 80.0 / 1.05          # the context's focal (synth.camera at 160 x 120, 90 degrees) is 5 % off the scene's
CTX_LENS = ("brown", (-0.1, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), 0.0)      # the lens of test_context_form_state_and_refusals' rig


def small_rig(ms, lens=None, build=True, skew=None):
    """6 views of 160 x 120 on the ideal ring, every view behind `lens`, calibrated up to the maps"""
    comp = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    for v in range(6):
        K, R0 = synth.camera(6, 160, 120, 90.0, v)
        assert K[0][0] == F_CTX and K[1][1] == F_CTX
        if skew is not None and v == skew:
            K[0][1] = 0.5
        if lens is not None:
            comp.set_lens(v, L.to_ms(ms, lens))
        comp.set_camera(v, K, R0)
    if build:
        comp.build_maps()
    return comp


def fabricate_lists(comp, lens, Rt, per_pair, rng):
    """tests/test_rig_focal_gpu.py's fabricate_lists behind a lens: a world ray is seen at a source pixel through the TRUE camera (Rt, F_SCENE) and the lens, and that
    source pixel shows up in the warped view where the CONTEXT's camera (the ring, F_CTX) and the same lens put it.  Returns the lists and the same matches as centred
    source pixels at the context's cameras in float64 (numpy formulas on the float positions)."""
    scale = float(np.float32(comp.cfg.warp_scale))
    R0 = np.array([synth.camera(6, 160, 120, 90.0, v)[1] for v in range(6)], np.float64)
    corner = [comp.view_geom(v).roi.tuple()[:2] for v in range(6)]
    Kc = np.diag([F_CTX, F_CTX, 1.0])
    lists = [[] for _ in range(6)]
    px = []

    def back(v, x, y):
        ray = rr.warper_ray(rr.SPHERICAL, scale, R0[v], corner[v][0] + float(x), corner[v][1] + float(y))
        p, seen = lr.centred_pixels(F_CTX, lens, np.asarray(ray, np.float64)[None, :])
        assert seen[0]
        return p[0]

    for i, j in rr.ring_pairs(6):
        mid = Rt[i][:, 2] + Rt[j][:, 2]
        mid /= np.linalg.norm(mid)
        for _ in range(per_pair):
            d = rr.exp_so3(np.radians(rng.uniform(-12, 12, 3))) @ mid
            pos = []
            for v in (i, j):
                src, seen = lr.centred_pixels(F_SCENE, lens, (Rt[v].T @ d)[None, :])
                ray, seen2 = lr.unproject(Kc, lens, src[0, 0], src[0, 1])
                assert seen[0] and seen2[0]
                u, w = rr.warper_forward(rr.SPHERICAL, scale, R0[v] @ ray[0])
                pos += [np.float32(u - corner[v][0]), np.float32(w - corner[v][1])]
            lists[i].append((pos[0], pos[1], pos[2], pos[3], j))
            px.append((i, j, back(i, pos[0], pos[1]), back(j, pos[2], pos[3])))
    order = [m for v in range(6) for m in px if m[0] == v]       # the order the context form builds: list after list
    return lists, order, R0


@pytest.mark.parametrize("shared", [False, True])
def test_context_form_on_a_lens_context(ms, cuda, shared):
    """BROWN on every view: ms_refine_rig_focals refuses, ms_refine_rig_focals_lens refines.  Device against the reference 1e-10 (rotations after the rounding to
    float both undergo); to the truth 1e-5 in the focal and in radians, tests/test_rig_focal_gpu.py's derivation (float positions known to 3e-5 pixels, lever arms of
    tens of pixels; the lens's Jacobian stays between 0.6 and 1 over these views)."""
    rng = np.random.default_rng(17)
    comp = small_rig(ms, CTX_LENS)
    assert comp.map_source() == ms.MAPS_LENS
    Rt = rr.perturbed(rr.ring(6), rng, 1.5)
    lists, px, R0 = fabricate_lists(comp, CTX_LENS, Rt, 12, rng)
    prm = ms.rig_focal_default_params(shared_focal=int(shared))
    with pytest.raises(ms.MsError, match="-2.*inverse distortion"):
        comp.refine_rig_focals(lists, prm)
    f, R, info = comp.refine_rig_focals_lens(lists, prm)
    assert f.dtype == np.float64 and R.dtype == np.float32 and info["matches_used"] == 72 and info["pairs_used"] == 6
    rf, rR, ri = lr.refine(np.full(6, F_CTX), R0, [CTX_LENS] * 6, px, shared_focal=shared)
    d = max_angle(R.astype(np.float64), rR.astype(np.float32).astype(np.float64)); df = float(np.max(np.abs(f / rf - 1.0)))
    truth = max_angle(R.astype(np.float64), rr.expected(R0, Rt, 0)); truth_f = float(np.max(np.abs(f / F_SCENE - 1.0)))
    print("shared=%s: %.3e rad and %.3e relative focal to the reference; %.3e rad and %.3e relative focal to the truth; cost %.3e -> %.3e; focals %s"
          % (shared, d, df, truth, truth_f, info["cost_initial"], info["cost_final"], f))
    assert d <= 1e-10 and df <= 1e-10
    assert truth <= 1e-5 and truth_f <= 1e-5
    assert info["cost_final"] <= info["cost_initial"] and abs(info["max_focal_ratio"] - 1.05) < 1e-4
    comp.close()


@pytest.mark.parametrize("shared", [False, True])
def test_context_form_on_an_analytic_context_is_the_pinhole_call_bit_for_bit(ms, cuda, shared):
    import test_rig_focal_gpu as G
    rng = np.random.default_rng(17)
    comp = small_rig(ms)
    assert comp.map_source() == ms.MAPS_ANALYTIC
    lists, _, _ = G.fabricate_lists(comp, rr.perturbed(rr.ring(6), rng, 1.5), 12, rng)
    prm = ms.rig_focal_default_params(shared_focal=int(shared))
    a = comp.refine_rig_focals_lens(lists, prm); b = comp.refine_rig_focals(lists, prm)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[2]["iterations"] >= 2
    comp.close()


def test_context_form_state_and_refusals(ms, cuda):
    lists = [[(10.0 + 3 * q, 20.0 + 5 * q, 30.0 + 2 * q, 40.0 + q, (v + 1) % 6) for q in range(4)] for v in range(6)]
    comp = small_rig(ms, CTX_LENS, build=False)
    with pytest.raises(ms.MsError, match="-5.*ms_build_maps first"):         # MS_ERR_STATE
        comp.refine_rig_focals_lens(lists)
    comp.build_maps()
    f, R, info = comp.refine_rig_focals_lens(lists)
    assert info["cost_final"] <= info["cost_initial"]
    with pytest.raises(ms.MsError, match="-1.*names view"):
        comp.refine_rig_focals_lens([[(10.0, 20.0, 30.0, 40.0, v)] * 4 for v in range(6)])
    # a pixel half a turn along the warper's u axis shows what lies behind the camera: past the lens's 89 degrees
    behind = [list(l) for l in lists]
    behind[2][1] = (10.0 + math.pi * comp.cfg.warp_scale, 20.0, 30.0, 40.0, 3)
    with pytest.raises(ms.MsError, match="-1.*match 1 of view 2.*does not see"):
        comp.refine_rig_focals_lens(behind)
    # a context on the caller's own maps has no cameras
    rois = [comp.view_geom(v).roi.tuple() for v in range(6)]
    maps = [comp.maps(v) for v in range(6)]
    twin = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    twin.set_maps(rois, [m[0].clone() for m in maps], [m[1].clone() for m in maps])
    assert twin.map_source() == ms.MAPS_CUSTOM
    with pytest.raises(ms.MsError, match="-2.*ms_set_maps"):                 # MS_ERR_UNSUPPORTED
        twin.refine_rig_focals_lens(lists)
    # centred pixels carry no skew
    skew = small_rig(ms, CTX_LENS, skew=3)
    with pytest.raises(ms.MsError, match=r"-2.*view 3.*K\[1\]"):
        skew.refine_rig_focals_lens(lists)
    skew.close(); twin.close(); comp.close()


# ---- 9. from pixels ---------------------------------------------------------------------------------------------------------------------------------
PX_N = 8
FOCAL_OFF = 1.10            # the focal the pipeline is given, over the true one


def render_lens(R, scale, f, lens, w, h):
    """tests/test_rig_pixels_gpu.py's texture (random grey blocks fixed on the sphere, a smooth ripple inside each) sampled along rig_lens_ref.unproject's rays of a
    w x h view with the focal f behind `lens`, principal point at the image centre; black where the lens does not see"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    rays, seen = lr.unproject([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]], lens, x.ravel(), y.ravel())
    d = (rays @ R.T).reshape(h, w, 3)
    u = np.arctan2(d[..., 0], d[..., 2]) + math.pi
    v = math.pi - np.arccos(np.clip(d[..., 1], -1.0, 1.0))
    cell = 32.0 / scale
    cu, cv = np.floor(u / cell).astype(np.int64), np.floor(v / cell).astype(np.int64)
    fu, fv = u / cell - cu, v / cell - cv
    out = np.empty((h, w, 3), np.uint8)
    for ch in range(3):
        hh = ((cu * 73856093) ^ (cv * 19349663) ^ (ch * 83492791)).astype(np.uint64) & 0xffffffff
        hh ^= hh >> 13; hh = (hh * 0x5bd1e995) & 0xffffffff; hh ^= hh >> 15
        val = 40.0 + ((hh >> 8) & 0xff).astype(np.float64) * 175.0 / 255.0 + 18.0 * np.sin(2 * math.pi * (fu + 0.3 * ch)) * np.sin(2 * math.pi * fv)
        out[..., ch] = np.clip(np.rint(val), 1, 255)
    out[~seen.reshape(h, w)] = 0
    return out


def lens_pixels_case(ms):
    """the whole pipeline on 8 rendered 640 x 480 fisheye views (true focal 320; the pipeline is given 352); returns the figures the test asserts on"""
    import test_rig_focal_gpu as G
    import test_rig_pixels_gpu as T
    assert (T.W, T.H, T.HFOV) == (640, 480, 90.0) and G.PX_N == PX_N
    f_true = (T.W / 2.0) / math.tan(math.radians(T.HFOV) / 2.0)
    f_given = f_true * FOCAL_OFF
    Rt = G.true_rig8()
    R0 = rr.ring(PX_N)                                  # the nominal rig: ms_estimate_rig stays pinhole
    scale = synth.warp_scale(T.OUT_W)
    lens = L.FISH; ml = L.to_ms(ms, lens)
    Kg = [[f_given, 0.0, T.W / 2.0], [0.0, f_given, T.H / 2.0], [0.0, 0.0, 1.0]]
    feats = []
    for v in range(PX_N):
        k, d = ms.orb_detect_and_compute(ms.bgr_to_gray(to_dev(render_lens(Rt[v], scale, f_true, lens, T.W, T.H))), None, nfeatures=2500)
        rays, seen = ms.lens_unproject_points(Kg, ml, np.ascontiguousarray(k[:, :2], np.float32)) if len(k) else (np.zeros((0, 3)), np.zeros(0, bool))
        feats.append((k, d, rays, seen))
    M, inliers = [], []
    centre = np.array([T.W * 0.5, T.H * 0.5], np.float64)
    for i, j in rr.ring_pairs(PX_N):
        (k1, d1, r1, s1), (k2, d2, r2, s2) = feats[i], feats[j]
        idx, dist = ms.knn_match_hamming2(d1, d2)
        good = [q for q in range(len(k1)) if idx[q, 1] >= 0 and dist[q, 0] < 0.7 * dist[q, 1] and s1[q] and s2[idx[q, 0]] and r1[q, 2] > 0.1 and r2[idx[q, 0], 2] > 0.1]
        # RANSAC, for inlier selection only, on the pixels undistorted at the given focal: f x / z
        src = np.array([f_given * r1[q, :2] / r1[q, 2] for q in good], np.float32).reshape(-1, 2)
        dst = np.array([f_given * r2[idx[q, 0], :2] / r2[idx[q, 0], 2] for q in good], np.float32).reshape(-1, 2)
        Hm, inl = (None, np.zeros(0, np.uint8)) if len(good) < 4 else ms.find_homography_ransac(src, dst)
        inliers.append(int(inl.sum()) if Hm is not None else 0)
        if Hm is not None:
            M += [(i, j, k1[q, :2].astype(np.float64) - centre, k2[idx[q, 0], :2].astype(np.float64) - centre) for n_, q in enumerate(good) if inl[n_]]
    prm = ms.rig_focal_default_params(shared_focal=1, huber_px=2.0)
    out = dict(f_true=f_true, f_given=f_given, inliers=inliers, min_pair_matches=prm.min_pair_matches)
    if min(inliers) >= prm.min_pair_matches:
        f0 = np.full(PX_N, f_given)
        f, R, info = ms.refine_rig_cameras_lens(f0, R0, [ml] * PX_N, M, prm)
        rf, rR, ri = lr.refine(f0, R0, [lens] * PX_N, M, shared_focal=True, huber_px=2.0)
        want = rr.expected(R0, Rt, 0)
        out.update(info=info, ref_info=ri, f_refined=float(f[0]), f_reference=float(rf[0]), to_reference_rad=max_angle(R, rR), to_reference_focal=float(np.max(np.abs(f / rf - 1.0))),
                   before_px=[rr.angle(R0[v], want[v]) * f_true for v in range(PX_N)], after_px=[rr.angle(R[v], want[v]) * f_true for v in range(PX_N)],
                   ref_after_px=[rr.angle(rR[v], want[v]) * f_true for v in range(PX_N)], focal_err_before_pct=abs(f_given / f_true - 1.0) * 100.0,
                   focal_err_after_pct=abs(float(f[0]) / f_true - 1.0) * 100.0, ref_focal_err_after_pct=abs(float(rf[0]) / f_true - 1.0) * 100.0)
    return out


def test_lens_rig_from_pixels(ms, cuda):
    """No absolute bound from the code under test: the device is held to the numpy reference on the same matches, and to not ending worse than it started.  Measured
    on MI355X (profiles/rig_lens.jsonl, "rig_lens_pixels"): 101 to 172 RANSAC inliers a neighbouring pair (1102 in all); the start, the nominal ring with the focal
    352 against the true 320, has the views 7.6 to 12.6 pixels from the truth; refined, the focal is 319.823 (0.055 % off) and the views end 0.32 to 0.78 pixels from
    the truth, 88 matches beyond the Huber threshold, 9 iterations; device and reference 2.9e-16 rad apart, the focals the same double."""
    r = lens_pixels_case(ms)
    print("inliers per neighbouring pair: %s" % r["inliers"])
    assert min(r["inliers"]) >= r["min_pair_matches"], "a neighbouring pair delivered %d inliers, fewer than min_pair_matches: %s" % (min(r["inliers"]), r["inliers"])
    print("focal: true %.3f, given %.3f (%.3f %% off), refined %.3f (%.3f %% off), reference %.3f (%.3f %% off)" % (r["f_true"], r["f_given"], r["focal_err_before_pct"],
          r["f_refined"], r["focal_err_after_pct"], r["f_reference"], r["ref_focal_err_after_pct"]))
    print("angle to the truth in pixels at the true focal, start:     %s" % ["%.3f" % x for x in r["before_px"]])
    print("angle to the truth in pixels at the true focal, refined:   %s" % ["%.3f" % x for x in r["after_px"]])
    print("angle to the truth in pixels at the true focal, reference: %s" % ["%.3f" % x for x in r["ref_after_px"]])
    print("device against the reference: %.3e rad, %.3e relative focal; info %s; reference %s" % (r["to_reference_rad"], r["to_reference_focal"], r["info"], r["ref_info"]))
    assert r["to_reference_rad"] <= 1e-10 and r["to_reference_focal"] <= 1e-10
    assert r["info"]["cost_final"] <= r["info"]["cost_initial"]
    assert r["focal_err_after_pct"] <= r["focal_err_before_pct"]
    assert all(a <= b for a, b in zip(r["after_px"], r["before_px"])), "a view ends further from the truth than it started"
    f_true = r["f_true"]
    assert r["focal_err_after_pct"] / 100.0 <= r["ref_focal_err_after_pct"] / 100.0 + 1e-9
    assert all(a / f_true <= b / f_true + 1e-9 for a, b in zip(r["after_px"], r["ref_after_px"]))
