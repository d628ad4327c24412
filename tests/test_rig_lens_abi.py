"""The inverse lens model and the lens form of the rig refinement (ms_lens_unproject, ms_lens_unproject_points, ms_rig_lens_accumulate, ms_refine_rig_cameras_lens,
ms_refine_rig_focals_lens): what holds without a device -- the five names, ms_lens_unproject in full against the forward model and the numpy reference of
tests/rig_lens_ref.py, every refusal of the device entry points (before the device is touched), and the reference's own Jacobian and convergence.

A context cannot exist without a device (ms_create), so the context form's refusals that need one -- K[1] != 0 among them -- are in tests/test_rig_lens_gpu.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import lens_ref as L
import rig_focal_ref as fr
import rig_lens_ref as lr
import rig_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ms_lens_unproject", "ms_lens_unproject_points", "ms_rig_lens_accumulate", "ms_refine_rig_cameras_lens", "ms_refine_rig_focals_lens"]
K = [[205.5, 0.0, 321.25], [0.0, 201.75, 238.5], [0.0, 0.0, 1.0]]           # two focals, an off-centre principal point; BROWN at 75 degrees stays below 2^12 pixels
K_SKEW = [[205.5, 1.75, 321.25], [0.0, 201.75, 238.5], [0.0, 0.0, 1.0]]
LENSES = {"none": L.NONE, "brown": L.BROWN, "fish": L.FISH}
# a rational profile x / (1 + r2) rises up to r = 1 (tan 40 degrees = 0.84 passes ms_lens_check) and never exceeds 0.5: xd = 2 has no preimage at all
NO_PREIMAGE = ("brown", (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0), 40.0)


def _err(ms):
    return ms.load().ms_last_error().decode()


def _angle(a, b):
    return math.atan2(np.linalg.norm(np.cross(a, b)), float(np.dot(a, b)))


def _rays(lens, rng, n, lo=1e-6, hi=1.0 - 1e-6):
    """unit rays with theta in [lo, hi] of the lens's limit (80 degrees without a lens), all azimuths"""
    mt = L.max_theta(lens) or math.radians(80.0)
    th = rng.uniform(lo * mt, hi * mt, n); ph = rng.uniform(0, 2 * math.pi, n)
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=-1)


def test_the_five_names_are_declared_exported_and_bound(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in include/ms_stitch.h" % n
        assert n in ms.EXPORTS and hasattr(lib, n), n
    for f in ("lens_unproject", "lens_unproject_points", "rig_lens_accumulate", "refine_rig_cameras_lens"):
        assert callable(getattr(ms, f))
    assert callable(ms.Compositor.refine_rig_focals_lens)


# ---- ms_lens_unproject ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kc", [K, K_SKEW], ids=["plain", "skew"])
@pytest.mark.parametrize("name", sorted(LENSES))
def test_ray_to_pixel_and_back(ms, name, Kc):
    """ray -> ms_lens_project -> ms_lens_unproject returns the ray within 1e-11 rad: pixel values are below 2^12 at 2^-52 relative precision, 1e-12, and a factor of
    1000 covers the Newton stop and libm (both test lenses have a profile slope of at least 0.5).  FISH reaches 100 degrees: some rays have Z < 0."""
    lens = LENSES[name]; ml = L.to_ms(ms, lens)
    R = _rays(lens, np.random.default_rng(5), 400)
    assert name != "fish" or (R[:, 2] < 0).sum() > 10
    worst = 0.0
    for r in R:
        px, seen = ms.lens_project(Kc, ml, r)
        assert seen and max(abs(px[0]), abs(px[1])) < 4096.0
        back, seen2 = ms.lens_unproject(Kc, ml, px)
        assert seen2 and abs(np.linalg.norm(back) - 1.0) <= 4e-16
        worst = max(worst, _angle(back, r))
    print("%s: ray round trip, worst %.3e rad" % (name, worst))
    assert worst <= 1e-11


@pytest.mark.parametrize("name", sorted(LENSES))
def test_pixel_to_ray_and_back(ms, name):
    """pixel -> ms_lens_unproject -> ms_lens_project returns the pixel within 1e-9 px (the same derivation), and the ray is the numpy reference's within 1e-12"""
    lens = LENSES[name]; ml = L.to_ms(ms, lens)
    rng = np.random.default_rng(6)
    px, py, seen = L.project(K, lens, *_rays(lens, rng, 400, hi=0.98).T)
    assert seen.all()
    px = px + rng.uniform(-0.3, 0.3, len(px)); py = py + rng.uniform(-0.3, 0.3, len(py))      # pixels that are no image of a float64 ray
    ref, ref_seen = lr.unproject(K, lens, px, py)
    assert ref_seen.all()
    worst = worst_ref = 0.0
    for k in range(len(px)):
        ray, s = ms.lens_unproject(K, ml, (px[k], py[k]))
        assert s
        (qx, qy), s2 = ms.lens_project(K, ml, ray)
        assert s2
        worst = max(worst, abs(qx - px[k]), abs(qy - py[k])); worst_ref = max(worst_ref, float(np.max(np.abs(ray - ref[k]))))
    print("%s: pixel round trip, worst %.3e px; %.3e to the numpy reference" % (name, worst, worst_ref))
    assert worst <= 1e-9 and worst_ref <= 1e-12


def test_the_image_centre_is_the_optical_axis(ms):
    for name, lens in LENSES.items():
        ray, seen = ms.lens_unproject(K, L.to_ms(ms, lens), (K[0][2], K[1][2]))
        assert seen and ray.tolist() == [0.0, 0.0, 1.0], name


@pytest.mark.parametrize("name", ["brown", "fish"])
def test_seen_flags_on_both_sides_of_max_theta(ms, name):
    """rays 1e-6 relative inside the limit come back seen from their pixel, pixels of rays 1e-6 outside (made with a lens of a wider limit) do not, and carry the ray (0, 0, 0)"""
    lens = LENSES[name]; ml = L.to_ms(ms, lens)
    wide = (lens[0], lens[1], lens[2] + 1.0)                   # the same coefficients, one degree more: its forward model makes the pixels just outside
    L_wide = L.to_ms(ms, wide)
    ms.lens_check(L_wide)
    mt = L.max_theta(lens)
    for ph in np.linspace(0.0, 2 * math.pi, 24, endpoint=False):
        for rel, want in ((1.0 - 1e-6, True), (1.0 + 1e-6, False), (0.5, True), (1.004, False)):
            th = mt * rel
            r = np.array([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)])
            px, seen = ms.lens_project(K, L_wide, r)
            assert seen
            ray, s = ms.lens_unproject(K, ml, px)
            assert s == want, (name, ph, rel)
            assert s or ray.tolist() == [0.0, 0.0, 0.0]
            assert lr.unproject(K, lens, px[0], px[1])[1][0] == want


def test_a_brown_pixel_that_does_not_settle_is_not_seen(ms):
    ml = L.to_ms(ms, NO_PREIMAGE)
    ms.lens_check(ml)
    px = (K[0][2] + 2.0 * K[0][0], K[1][2])                    # xd = 2, yd = 0
    _, _, ref_seen, ref_settled, rounds = lr.brown_solve(NO_PREIMAGE, np.array([2.0]), np.array([0.0]))
    assert not ref_settled[0] and not ref_seen[0]              # the reference runs out of rounds (or meets a singular Jacobian) too
    ray, seen = ms.lens_unproject(K, ml, px)
    assert not seen and ray.tolist() == [0.0, 0.0, 0.0]
    ray, seen = ms.lens_unproject(K, ml, (K[0][2] + 0.3 * K[0][0], K[1][2]))       # inside the field the same lens inverts
    assert seen and abs(ray[0] / ray[2] / (1.0 + (ray[0] / ray[2]) ** 2) - 0.3) < 1e-15
    for bad in (float("nan"), float("inf")):
        for lens in LENSES.values():
            assert not ms.lens_unproject(K, L.to_ms(ms, lens), (bad, 10.0))[1]


def test_the_stop_rule_settles_in_a_handful_of_rounds():
    """the header's rule, max |step| <= 2^-50 max(1, |x|, |y|), ends far below its cap of 50 rounds over the whole field (a zero-step rule would run into the cap where
    the last bit alternates); fisheye, capped at 60, needs a few"""
    rng = np.random.default_rng(8)
    R = _rays(L.BROWN, rng, 2000)
    x, y = R[:, 0] / R[:, 2], R[:, 1] / R[:, 2]
    xd, yd, _ = lr.brown_forward([np.float64(v) for v in L.BROWN[1]], x, y)
    bx, by, seen, settled, rounds = lr.brown_solve(L.BROWN, xd, yd)
    print("brown: %d rounds, worst |x - x_true| %.3e" % (rounds, float(np.max(np.abs(bx - x)))))
    assert seen.all() and rounds <= 25 and np.max(np.abs(bx - x)) <= 1e-13 and np.max(np.abs(by - y)) <= 1e-13
    th = rng.uniform(0.0, L.max_theta(L.FISH) * (1 - 1e-6), 2000)
    t, seen, rounds = lr.fisheye_solve(L.FISH, lr.fisheye_profile([np.float64(v) for v in L.FISH[1]], th))
    print("fisheye: %d rounds, worst |theta - theta_true| %.3e" % (rounds, float(np.max(np.abs(t - th)))))
    assert seen.all() and rounds <= 8 and np.max(np.abs(t - th)) <= 1e-14


def test_unproject_refusals(ms):
    lib = ms.load()
    kp = (C.c_float * 9)(*[v for row in K for v in row])
    px = (C.c_double * 2)(100.0, 100.0); ray = (C.c_double * 3)(); seen = C.c_int()
    good = L.to_ms(ms, L.FISH)
    assert lib.ms_lens_unproject(kp, C.byref(good), px, ray, C.byref(seen)) == 0 and seen.value == 1
    for args in ((None, C.byref(good), px, ray, C.byref(seen)), (kp, C.byref(good), None, ray, C.byref(seen)), (kp, C.byref(good), px, None, C.byref(seen)),
                 (kp, C.byref(good), px, ray, None)):
        assert lib.ms_lens_unproject(*args) == -1 and "ms_lens_unproject: null" in _err(ms)
    fold = ms.Lens.brown(-0.4, max_theta_deg=60.0)            # folds back before 60 degrees
    bad_size = L.to_ms(ms, L.FISH); bad_size.struct_size -= 4
    for bad, word in ((fold, "not strictly increasing"), (bad_size, "struct_size")):
        assert lib.ms_lens_unproject(kp, C.byref(bad), px, ray, C.byref(seen)) == -1 and "ms_lens_unproject" in _err(ms) and word in _err(ms)
    k0 = (C.c_float * 9)(*[0.0 if i == 0 else v for i, v in enumerate(v for row in K for v in row)])
    assert lib.ms_lens_unproject(k0, None, px, ray, C.byref(seen)) == -1 and "K[0]" in _err(ms)
    # the device form refuses the same, and a count out of range, before it looks for a device
    pts = (C.c_float * 8)(); rays = (C.c_double * 12)(); flags = (C.c_ubyte * 4)()
    for n in (0, -1, (1 << 20) + 1):
        assert lib.ms_lens_unproject_points(kp, C.byref(good), n, pts, rays, flags, None) == -1 and "points outside" in _err(ms)
    for args in ((None, None, 4, pts, rays, flags, None), (kp, None, 4, None, rays, flags, None), (kp, None, 4, pts, None, flags, None), (kp, None, 4, pts, rays, None, None)):
        assert lib.ms_lens_unproject_points(*args) == -1 and "ms_lens_unproject_points: null" in _err(ms)
    for bad, word in ((fold, "not strictly increasing"), (bad_size, "struct_size")):
        assert lib.ms_lens_unproject_points(kp, C.byref(bad), 4, pts, rays, flags, None) == -1 and word in _err(ms)


# ---- refusals of the refinement's entry points --------------------------------------------------------------------------------------------------------
RIG_LENSES = [L.NONE, L.BROWN, L.FISH]


def _valid():
    rng = np.random.default_rng(9)
    R = rr.ring(6)[:3].copy()
    f = np.full(3, 400.0)
    return f, R, lr.make_lens_matches(f * 1.03, rr.perturbed(R, rng, 2.0), RIG_LENSES, [(0, 1), (1, 2)], 5, rng)


def _call(ms, n_views, f, R, lenses, matches, n, prm, accumulate=False, null=None):
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    nv = max(n_views, 1)
    fo = np.zeros(nv); out = np.zeros((nv, 3, 3)); H = np.zeros((4 * nv) ** 2); g = np.zeros(4 * nv); cost = C.c_double()
    info = ms.RigFocalInfo()
    arr = ms.rig_px_matches(matches)
    la = None if null == "lenses" else (lenses if isinstance(lenses, C.Array) else ms.lens_array([L.to_ms(ms, l) for l in lenses]))
    ptr = lambda name, a: None if null == name else a.ctypes.data_as(dp)
    if accumulate:
        rc = lib.ms_rig_lens_accumulate(n_views, ptr("f", fa), ptr("R", Ra), la, None if null == "matches" else arr, n, C.c_double(prm),
                                        None if null == "cost" else C.byref(cost), ptr("H", H), ptr("g", g), None)
    else:
        rc = lib.ms_refine_rig_cameras_lens(n_views, ptr("f", fa), ptr("R", Ra), la, None if null == "matches" else arr, n, None if null == "prm" else C.byref(prm),
                                            ptr("f_out", fo), ptr("R_out", out), C.byref(info), None)
    return rc, _err(ms)


@pytest.mark.parametrize("accumulate", [False, True])
def test_refinement_refusals_before_the_device_is_touched(ms, accumulate):
    f, R, M = _valid()
    prm = (lambda **kw: 0.0) if accumulate else ms.rig_focal_default_params
    name = "ms_rig_lens_accumulate" if accumulate else "ms_refine_rig_cameras_lens"
    for null in (("f", "R", "lenses", "matches", "cost", "H", "g") if accumulate else ("f", "R", "lenses", "matches", "prm", "f_out", "R_out")):
        rc, msg = _call(ms, 3, f, R, RIG_LENSES, M, len(M), prm(), accumulate, null=null)
        assert rc == -1 and name in msg and "null" in msg, (null, rc, msg)
    for nv in (1, 0, 17):
        rc, msg = _call(ms, nv, np.full(17, 400.0), np.array([np.eye(3)] * 17), [L.NONE] * 17, M, len(M), prm(), accumulate)
        assert rc == -1 and name in msg and "n_views" in msg, (nv, rc, msg)
    for n in (0, -1, (1 << 20) + 1):
        rc, msg = _call(ms, 3, f, R, RIG_LENSES, M, n, prm(), accumulate)
        assert rc == -1 and name in msg and "matches" in msg, (n, rc, msg)
    # a lens ms_lens_check refuses: a fold-back, a struct_size mismatch, an unknown model
    for v, make, word in ((1, lambda l: ms.Lens.brown(-0.4, max_theta_deg=60.0), "not strictly increasing"), (2, lambda l: _resized(l), "struct_size"),
                          (0, lambda l: ms.Lens.make(7), "unknown lens model")):
        arr = ms.lens_array([L.to_ms(ms, l) for l in RIG_LENSES])
        arr[v] = make(arr[v])
        rc, msg = _call(ms, 3, f, R, arr, M, len(M), prm(), accumulate)
        assert rc == -1 and name in msg and word in msg, (v, rc, msg)
    # what the pinhole forms refuse: a focal, a rotation, a match
    fb = f.copy(); fb[1] = -400.0
    rc, msg = _call(ms, 3, fb, R, RIG_LENSES, M, len(M), prm(), accumulate)
    assert rc == -1 and "focal of view 1" in msg
    Rb = R.copy(); Rb[2] = Rb[2] * 1.001
    rc, msg = _call(ms, 3, f, Rb, RIG_LENSES, M, len(M), prm(), accumulate)
    assert rc == -1 and "rotation of view 2 is not orthonormal" in msg
    Mb = list(M); Mb[3] = (Mb[3][0], Mb[3][0], Mb[3][2], Mb[3][3])
    rc, msg = _call(ms, 3, f, R, RIG_LENSES, Mb, len(Mb), prm(), accumulate)
    assert rc == -1 and "match 3" in msg
    if not accumulate:
        p = ms.rig_focal_default_params(); p.struct_size += 8
        rc, msg = _call(ms, 3, f, R, RIG_LENSES, M, len(M), p)
        assert rc == -1 and "struct_size" in msg
        for kw, word in ((dict(anchor_view=3), "anchor_view"), (dict(max_iters=0), "max_iters"), (dict(huber_px=-1.0), "huber_px"), (dict(min_pair_matches=0), "min_pair_matches")):
            rc, msg = _call(ms, 3, f, R, RIG_LENSES, M, len(M), ms.rig_focal_default_params(**kw))
            assert rc == -1 and word in msg, (kw, rc, msg)
        rc, msg = _call(ms, 3, np.array([400.0, 401.0, 400.0]), R, RIG_LENSES, M, len(M), ms.rig_focal_default_params(shared_focal=1))
        assert rc == -1 and "shared_focal" in msg and "view 1" in msg
        rc, msg = _call(ms, 3, f, R, RIG_LENSES, [m for m in M if m[0] == 0], 5, ms.rig_focal_default_params())
        assert rc == -1 and "view 2 is not connected" in msg
    else:
        rc, msg = _call(ms, 3, f, R, RIG_LENSES, M, len(M), float("nan"), True)
        assert rc == -1 and "huber_px" in msg


def _resized(lens):
    lens.struct_size += 4
    return lens


@pytest.mark.parametrize("accumulate", [False, True])
def test_an_unseen_pixel_at_the_input_cameras_names_its_match(ms, accumulate):
    """the pixel of a ray at 74.9 degrees of the Brown view (limit 75) at the focal 600 lies outside the field at the input focal 400, and so does the fisheye's at 99.9"""
    f, R, M = _valid()
    prm = 0.0 if accumulate else ms.rig_focal_default_params()
    for k, view, lens, deg in ((2, 1, L.BROWN, 74.9), (7, 2, L.FISH, 99.9)):
        th = math.radians(deg)
        px, seen = lr.centred_pixels(600.0, lens, np.array([[math.sin(th), 0.0, math.cos(th)]]))
        assert seen[0] and not lr.unproject(np.diag([400.0, 400.0, 1.0]), lens, px[0, 0], px[0, 1])[1][0]
        Mb = list(M)
        va, vb, a, b = Mb[k]
        assert view in (va, vb)
        Mb[k] = (va, vb, px[0], b) if va == view else (va, vb, a, px[0])
        rc, msg = _call(ms, 3, f, R, RIG_LENSES, Mb, len(Mb), prm, accumulate)
        assert rc == -1 and "match %d" % k in msg and "view %d" % view in msg and "does not see" in msg, (rc, msg)
    lib = ms.load()
    assert lib.ms_refine_rig_focals_lens(None, None, None, None, None, None, None, None) == -1 and "ms_refine_rig_focals_lens: null" in _err(ms)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LENSES))
def test_reference_ray_derivative_against_central_differences(name):
    """da/ds of rig_lens_ref.view_ray against central differences of its own unproject in s = ln f, step 1e-6: the truncation error is (1e-6)^2 / 6 times a third
    derivative of order 1 to 100 at the rim, the rounding error 2^-53 / 1e-6 = 1e-10; 1e-8 covers both"""
    lens = LENSES[name]
    rng = np.random.default_rng(11)
    f = 400.0
    rays = _rays(lens, rng, 500, lo=0.01, hi=0.97)
    px, seen = lr.centred_pixels(f, lens, rays)
    assert seen.all()
    a, d, ok = lr.view_ray(lens, px[:, 0] / f, px[:, 1] / f)
    assert ok.all() and np.max(np.abs(np.stack(a, -1) - rays)) <= 1e-12
    e = 1e-6
    Kp = np.diag([f * math.exp(e), f * math.exp(e), 1.0]); Km = np.diag([f * math.exp(-e), f * math.exp(-e), 1.0])
    ap, sp = lr.unproject(Kp, lens, px[:, 0], px[:, 1]); am, sm = lr.unproject(Km, lens, px[:, 0], px[:, 1])
    both = sp & sm
    assert both.sum() >= 450
    worst = float(np.max(np.abs((ap - am)[both] / (2 * e) - np.stack(d, -1)[both])))
    print("%s: max |central difference - analytic da/ds| %.3e" % (name, worst))
    assert worst <= 1e-8


def test_reference_gradient_against_central_differences_of_its_cost():
    """g of rig_lens_ref.accumulate is the derivative of half the cost by the rotation and log-focal of every view"""
    rng = np.random.default_rng(12)
    R = rr.perturbed(rr.ring(6)[:3], rng, 3.0); f = np.array([400.0, 431.5, 388.25])
    M = lr.make_lens_matches(f * 1.02, rr.perturbed(rr.ring(6)[:3], rng, 3.0), RIG_LENSES, [(0, 1), (1, 2)], 20, rng, noise_px=0.5)
    _, _, g = lr.accumulate(f, R, RIG_LENSES, M)
    e = 1e-6
    for k in range(12):
        d = np.zeros(12); d[k] = e
        fp, Rp = fr.apply_step(f, R, d); fm, Rm = fr.apply_step(f, R, -d)
        fd = (lr.cost_only(fp, Rp, RIG_LENSES, M) - lr.cost_only(fm, Rm, RIG_LENSES, M)) / (2 * e) / 2.0
        assert abs(fd - g[k]) <= 1e-6 * max(1.0, abs(g[k])), (k, fd, g[k])


def test_reference_all_none_is_rig_focal_ref_bit_for_bit():
    rng = np.random.default_rng(13)
    R = rr.perturbed(rr.ring(6)[:3], rng, 3.0); f = np.array([400.0, 431.5, 388.25])
    M = fr.make_px_matches(f * 1.02, rr.perturbed(rr.ring(6)[:3], rng, 3.0), [(0, 1), (1, 2)], 20, rng, noise_px=0.5)
    for h in (0.0, 1.0):
        a = lr.accumulate(f, R, [L.NONE] * 3, M, h); b = fr.accumulate(f, R, M, h)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_reference_recovers_the_truth():
    """exact matches through NONE, BROWN and FISH views, the start 15 to 20 % off in focal and 2 degrees in rotation: the reference alone ends at the truth"""
    rng = np.random.default_rng(14)
    lenses = [L.NONE, L.BROWN, L.FISH, L.FISH]
    R0 = rr.ring(6)[:4].copy(); Rt = rr.perturbed(R0, rng, 2.0)
    ft = 400.0 * (1 + rng.uniform(-0.05, 0.05, 4)); f0 = 400.0 * np.array([0.85, 1.2, 0.85, 1.2])
    M = lr.make_lens_matches(ft, Rt, lenses, [(0, 1), (1, 2), (2, 3)], 40, rng, spread_deg=15.0)
    M = [m for m in M if lr.all_seen(f0, R0, lenses, [m])]
    f, R, info = lr.refine(f0, R0, lenses, M, step_tol=1e-13)
    err_f = float(np.max(np.abs(f / ft - 1.0))); err_R = max(rr.angle(a, b) for a, b in zip(R, rr.expected(R0, Rt, 0)))
    print("focal ratio off 1 by %.3e, %.3e rad to the truth, %d iterations, stop %d" % (err_f, err_R, info["iterations"], info["stop_reason"]))
    assert err_f <= 1e-11 and err_R <= 1e-11 and info["cost_final"] <= 1e-18 * info["cost_initial"]
