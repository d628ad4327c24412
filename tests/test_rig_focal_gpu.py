"""Focals and rotations from feature matches on the GPU (csrc/rig_focal.hip) against the numpy reference of tests/rig_focal_ref.py.

1. ms_rig_focal_accumulate per op: every entry of cost, H and g within the worst-case bound for two summation orders of the same rounded terms
2. ms_refine_rig_cameras: exact recovery from wrong focals and rotations, per-view and shared focal, up to the 61-unknown system
3. noisy matches and outliers (Huber) against the reference on the same inputs, an anchor other than view 0
4. determinism: two calls return the same bits
5. pairs below min_pair_matches
6. the context form, ms_refine_rig_focals, and its refusals
7. from pixels with an unknown rig: ORB on the source images, ratio test, RANSAC homographies, ms_estimate_rig, ms_refine_rig_cameras

The stop step at the rounding floor depends on the order of the sums, so no test compares iteration counts."""
import math

import numpy as np
import pytest
import torch

import lens_ref as L
import rig_focal_ref as fr
import rig_lm_cases as lm_cases
import rig_ref as rr
import synth
from helpers import to_dev

pytestmark = pytest.mark.gpu

_REF = {}


def ref_refine(key, f_in, R_in, M, **kw):
    """the reference's answer for a named case, computed once"""
    if key not in _REF:
        _REF[key] = fr.refine(f_in, R_in, M, **kw)
    return _REF[key]


def device_refine(ms, f_in, R_in, M, **kw):
    kw = {{"anchor": "anchor_view"}.get(k, k): (int(v) if k == "shared_focal" else v) for k, v in kw.items()}
    return ms.refine_rig_cameras(f_in, R_in, M, ms.rig_focal_default_params(**kw))


def max_angle(A, B):
    return max(rr.angle(a, b) for a, b in zip(A, B))


# ---- 1. accumulate, per op --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4, 63, 64, 65, 255, 256, 257, 1000])
def test_accumulate_per_op(ms, cuda, m):
    """3 views with three focals, pair (0, 1) with m matches, pair (1, 2) with 5, pair (0, 2) with none, listed in shuffled order with a third of them as (j, i).  The
    terms of the two implementations are the same bits (the contract fixes their arithmetic); only the order of the sums differs, and for two orders of n rounded
    terms the results differ by at most (n - 1) 2^-52 S, S the sum of the terms' absolute values: the bound, (m + 8) 2^-52 S, covers the m + 5 terms of any entry.
    m = 1, 4: a lane holds at most one match; 63, 64, 65: one wave's butterfly; 255, 256, 257: the lane stride; 1000: four matches a lane."""
    rng = np.random.default_rng(200 + m)
    R = rr.perturbed(rr.ring(6)[:3], rng, 5.0)
    f = np.array([400.0, 431.5, 388.25])
    M = fr.make_px_matches(f * (1 + rng.uniform(-0.03, 0.03, 3)), rr.perturbed(rr.ring(6)[:3], rng, 5.0), [(0, 1), (1, 2)], [m, 5], rng, noise_px=0.7)
    M = [M[k] for k in rng.permutation(len(M))]
    M = [(vb, va, b, a) if rng.uniform() < 1 / 3 else (va, vb, a, b) for va, vb, a, b in M]
    assert any(va > vb for va, vb, _, _ in M)                 # a pair listed (j, i)
    i, j, a, b = fr.unpack(M)
    s = fr.terms(f, R, i, j, a, b, 0.0)[1]
    h_mid = float(np.sort(s)[len(s) // 2 - 1])
    assert 0 < (s > h_mid).sum() < len(s)                     # matches on both Huber branches
    for h in (0.0, h_mid):
        cost, H, g = ms.rig_focal_accumulate(f, R, M, h)
        rc, rH, rg, sc, sH, sg = fr.accumulate(f, R, M, h, with_abs=True)
        tol = (m + 8) * 2.0 ** -52
        print("m=%d h=%g: cost %.3e of %.3e, H %.3e, g %.3e (max |diff| / S)" % (m, h, abs(cost - rc) / sc, tol, np.max(np.abs(H - rH) / np.maximum(sH, 1e-300)),
                                                                                   np.max(np.abs(g - rg) / np.maximum(sg, 1e-300))))
        assert abs(cost - rc) <= tol * sc
        assert np.all(np.abs(H - rH) <= tol * sH) and np.all(np.abs(g - rg) <= tol * sg)
        assert np.array_equal(H, H.T) and not H[0:4, 8:12].any() and H[4:8, 4:8].all() and H[0:4, 4:8].all()


@pytest.mark.parametrize("graph", ["complete", "ring"])
def test_accumulate_per_op_16_views(ms, cuda, graph):
    """16 views with 16 focals (rows up to 64 of the full matrix): the complete graph, 120 pairs of 3 matches, and the ring, 16 pairs of 6, shuffled with a third listed
    as (j, i) (tests/rig_lm_cases.py).  The bound of test_accumulate_per_op per entry: the cost sums every match, an entry of H or g at most the matches of one view.
    H is symmetric bit for bit, and a block is zero exactly where its pair has no match: none of the complete graph's, 104 of the ring's 120."""
    f, R, M, pairs = lm_cases.accumulate_case("focal", graph)
    n_cost, n_entry = lm_cases.accumulate_terms(M)
    for h in (0.0, lm_cases.accumulate_huber("focal", f, R, M)):
        cost, H, g = ms.rig_focal_accumulate(f, R, M, h)
        rc, rH, rg, sc, sH, sg = fr.accumulate(f, R, M, h, with_abs=True)
        tol_c, tol = (n_cost + 8) * 2.0 ** -52, (n_entry + 8) * 2.0 ** -52
        print("%s h=%g: cost %.3e of %.3e, H %.3e, g %.3e of %.3e (max |diff| / S)" % (graph, h, abs(cost - rc) / sc, tol_c, np.max(np.abs(H - rH) / np.maximum(sH, 1e-300)),
                                                                                     np.max(np.abs(g - rg) / np.maximum(sg, 1e-300)), tol))
        assert abs(cost - rc) <= tol_c * sc
        assert np.all(np.abs(H - rH) <= tol * sH) and np.all(np.abs(g - rg) <= tol * sg)
        assert np.array_equal(H, H.T)
        used = {(min(p), max(p)) for p in pairs}
        zero = 0
        for i in range(15):
            for j in range(i + 1, 16):
                blk = H[4 * i:4 * i + 4, 4 * j:4 * j + 4]
                assert blk.any() == ((i, j) in used), (i, j)
                zero += not blk.any()
        assert zero == (0 if graph == "complete" else 104) and all(H[4 * v:4 * v + 4, 4 * v:4 * v + 4].all() for v in range(16))


# ---- 2. exact recovery ------------------------------------------------------------------------------------------
def recovery_case(name):
    """-> f0, R0 (the start), ft, Rt (the truth), pairs, matches.  The start: the ideal layout, focals 15 % low and 20 % high in turn (shared: 30 % low)."""
    n, shared = {"pair2": (2, False), "ring6": (6, False), "ring6-shared": (6, True), "chords16": (16, False), "chords16-shared": (16, True)}[name]
    rng = np.random.default_rng(30 + n + shared)
    R0 = np.array([np.eye(3), rr.rot_y(math.radians(40.0))]) if n == 2 else rr.ring(n)
    pairs = rr.ring_pairs(n) + ([(v, (v + 2) % 16) for v in range(0, 16, 2)] if n == 16 else [])
    Rt = rr.perturbed(R0, rng, 2.0)
    ft = np.full(n, 400.0) if shared else 400.0 * (1 + rng.uniform(-0.05, 0.05, n))
    f0 = np.full(n, 280.0) if shared else 400.0 * np.where(np.arange(n) % 2, 0.85, 1.2)
    return f0, R0, ft, Rt, pairs, fr.make_px_matches(ft, Rt, pairs, 30 if n == 16 else 60, rng, spread_deg=15.0)


@pytest.mark.parametrize("name", ["pair2", "ring6", "ring6-shared", "chords16", "chords16-shared"])
def test_exact_recovery(ms, cuda, name):
    """exact matches have the true cameras as a zero of the cost; chords16 is the 61-unknown system, k_rig_step<4>'s LDS limit.  Bounds: the reference ends within
    6e-16 of the true focal ratio and 3e-16 rad; 1e-12 leaves the conditioning of the largest system three orders."""
    f0, R0, ft, Rt, pairs, M = recovery_case(name)
    n, shared = len(f0), name.endswith("shared")
    for anchor in sorted({0, n // 2, n - 1}) if n >= 3 else (0, n - 1):
        f, R, info = device_refine(ms, f0, R0, M, anchor=anchor, shared_focal=shared, step_tol=1e-13)
        err_R = max_angle(R, rr.expected(R0, Rt, anchor)); err_f = float(np.max(np.abs(f / ft - 1.0)))
        print("%s anchor=%d: focal ratio off 1 by %.3e, %.3e rad to the truth, %d iterations, stop %d, cost %.3e -> %.3e" % (name, anchor, err_f, err_R, info["iterations"],
                                                                                                                       info["stop_reason"], info["cost_initial"], info["cost_final"]))
        assert err_f <= 1e-12 and err_R <= 1e-12
        assert R[anchor].tobytes() == R0[anchor].tobytes()
        assert not shared or np.all(f == f[0])
        assert info["matches_used"] == len(M) and info["pairs_used"] == len(pairs) and info["pairs_ignored"] == 0 and info["outliers"] == 0
        assert info["cost_final"] <= info["cost_initial"] and 0.005 < info["max_rotation_rad"] < 0.2 and 1.15 < info["max_focal_ratio"] < 1.5


# ---- 3. noise and outliers against the reference ------------------------------------------------------------------
# What 1e-10 between two correct implementations asks of a case.  The accept rule compares two costs, each a sum of n rounded terms in an order of its own, known to
# about sqrt(n) 2^-53 cost.  A step d near the minimum moves the cost by d^T H d, so once d^T H d falls below that the rule's verdicts are rounding noise: steps are
# refused, lambda climbs until the damped step is under step_tol, and the loop stops wherever it stood.  With residuals left at the minimum (noise, and more so Huber,
# whose weights move with the cameras) Gauss-Newton converges linearly and the loop does reach that floor.  The floor scales with sqrt(cost / H): in pixel units H is
# about n f^2, 0.3 px of noise on 384 matches leaves a cost of 84 and a gross outlier adds 2 h s ~ 10^3 to it, which puts the floor at 3e-10 and 2e-9 rad (the
# reference against itself with the matches in another order differs by that much).  So the cases keep the cost at the minimum below 10: 0.05 px of noise; with Huber
# 0.02 px, the threshold at 0.1 px and outliers 0.5 - 1.5 px off (a match to the feature next door).  Then the reference run on four reorderings of the matches agrees
# with itself to 3e-12 rad and 2e-12 relative in the focals in the worst case.
NOISY = {
    "ring6": dict(n=6, per_pair=64, noise_px=0.05, outlier_frac=0.0, huber_px=0.0, shared=False, anchor=0),
    "ring6-huber": dict(n=6, per_pair=64, noise_px=0.02, outlier_frac=0.15, huber_px=0.1, shared=False, anchor=0),
    "ring6-huber-shared": dict(n=6, per_pair=64, noise_px=0.02, outlier_frac=0.15, huber_px=0.1, shared=True, anchor=4),
    "tri3": dict(n=3, per_pair=9, noise_px=0.5, outlier_frac=0.0, huber_px=0.0, shared=False, anchor=2),
}


def noisy_case(name):
    c = NOISY[name]
    n = c["n"]
    rng = np.random.default_rng(sorted(NOISY).index(name) + 170)
    R0 = rr.ring(6)[:n].copy()
    pairs = [(0, 1), (1, 2), (0, 2)] if n == 3 else rr.ring_pairs(n)
    ft = np.full(n, 412.0) if c["shared"] else 400.0 * (1 + rng.uniform(-0.04, 0.04, n))
    M = fr.make_px_matches(ft, rr.perturbed(R0, rng, 2.0), pairs, c["per_pair"], rng, noise_px=c["noise_px"], outlier_frac=c["outlier_frac"], spread_deg=15.0,
                           outlier_px=(0.5, 1.5))
    return np.full(n, 400.0), R0, M, dict(huber_px=c["huber_px"], shared_focal=c["shared"], anchor=c["anchor"], step_tol=1e-12, max_iters=100)


@pytest.mark.parametrize("name", sorted(NOISY))
def test_noisy_matches_against_the_reference(ms, cuda, name):
    f0, R0, M, kw = noisy_case(name)
    rf, rR, ri = ref_refine(name, f0, R0, M, **kw)
    f, R, info = device_refine(ms, f0, R0, M, **kw)
    d = max_angle(R, rR); df = float(np.max(np.abs(f / rf - 1.0)))
    print("%s: %.3e rad and %.3e relative focal between device and reference; cost %.6e -> %.6e (reference %.6e); outliers %d (reference %d); iterations %d (reference %d); "
          "focals %s" % (name, d, df, info["cost_initial"], info["cost_final"], ri["cost_final"], info["outliers"], ri["outliers"], info["iterations"], ri["iterations"], f))
    assert d <= 1e-10 and df <= 1e-10
    assert info["cost_final"] <= info["cost_initial"]
    assert abs(info["outliers"] - ri["outliers"]) <= 2 and (kw["huber_px"] > 0) == (info["outliers"] > 0)
    assert info["matches_used"] == ri["matches_used"] and info["pairs_used"] == ri["pairs_used"]
    assert abs(info["max_rotation_rad"] - ri["max_rotation_rad"]) <= 1e-10 and abs(info["max_focal_ratio"] - ri["max_focal_ratio"]) <= 1e-9
    assert R[kw["anchor"]].tobytes() == R0[kw["anchor"]].tobytes()


# ---- 4. determinism ---------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits(ms, cuda):
    f0, R0, M, kw = noisy_case("ring6-huber")
    a = device_refine(ms, f0, R0, M, **kw)
    b = device_refine(ms, f0, R0, M, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    ca = ms.rig_focal_accumulate(f0, R0, M, 1.5); cb = ms.rig_focal_accumulate(f0, R0, M, 1.5)
    assert ca[0] == cb[0] and ca[1].tobytes() == cb[1].tobytes() and ca[2].tobytes() == cb[2].tobytes()


# ---- 5. pairs below min_pair_matches ------------------------------------------------------------------------------
def test_small_pairs_are_counted_and_a_view_they_cut_off_is_named(ms, cuda):
    rng = np.random.default_rng(3)
    R = rr.ring(6)[:4]; f = np.full(4, 400.0)
    M = fr.make_px_matches(f * 1.02, rr.perturbed(R, rng, 1.0), [(0, 1), (1, 2), (2, 3), (0, 2)], [8, 3, 8, 8], rng)
    fo, Ro, info = device_refine(ms, f, R, M)                      # (1, 2) is ignored; view 2 still hangs on view 0
    assert info["pairs_ignored"] == 1 and info["pairs_used"] == 3 and info["matches_used"] == 24 and info["cost_final"] <= info["cost_initial"]
    M = [m for m in M if (m[0], m[1]) != (0, 2)]
    with pytest.raises(ms.MsError, match="view 2 is not connected"):
        device_refine(ms, f, R, M)
    fo, Ro, info = device_refine(ms, f, R, M, min_pair_matches=3)       # the same matches with the pair let in
    assert info["pairs_ignored"] == 0 and info["pairs_used"] == 3 and info["cost_final"] <= info["cost_initial"]


# ---- 6. the context form ----------------------------------------------------------------------------------------
F_CTX, F_SCENE = 80.0, 80.0 / 1.05          # the context's focal (synth.camera at 160 x 120, 90 degrees) is 5 % off the scene's


def small_rig(ms):
    """6 views of 160 x 120 on the ideal ring, calibrated up to the maps"""
    comp = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    for v in range(6):
        K, R0 = synth.camera(6, 160, 120, 90.0, v)
        assert K[0][0] == F_CTX and K[1][1] == F_CTX
        comp.set_camera(v, K, R0)
    comp.build_maps()
    return comp


def fabricate_lists(comp, Rt, per_pair, rng):
    """float match lists of a context whose maps were built with the ring R0 and the focal F_CTX while the cameras are really at Rt with the focal F_SCENE: a world ray
    is seen at a source pixel through the TRUE camera, and that source pixel shows up in the warped view where the CONTEXT's camera puts it.  Returns the lists and the
    same matches as centred pixels in float64 (numpy formulas on the float positions)."""
    scale = float(np.float32(comp.cfg.warp_scale))
    R0 = np.array([synth.camera(6, 160, 120, 90.0, v)[1] for v in range(6)], np.float64)
    corner = [comp.view_geom(v).roi.tuple()[:2] for v in range(6)]
    lists = [[] for _ in range(6)]
    px = []

    def back(v, x, y):
        ray = rr.warper_ray(rr.SPHERICAL, scale, R0[v], corner[v][0] + float(x), corner[v][1] + float(y))
        return np.array([F_CTX * (ray[0] / ray[2]), F_CTX * (ray[1] / ray[2])])

    for i, j in rr.ring_pairs(6):
        mid = Rt[i][:, 2] + Rt[j][:, 2]
        mid /= np.linalg.norm(mid)
        for _ in range(per_pair):
            d = rr.exp_so3(np.radians(rng.uniform(-12, 12, 3))) @ mid
            pos = []
            for v in (i, j):
                c = Rt[v].T @ d
                src = F_SCENE * c[:2] / c[2]                                   # the centred source pixel
                u, w = rr.warper_forward(rr.SPHERICAL, scale, R0[v] @ np.array([src[0] / F_CTX, src[1] / F_CTX, 1.0]))
                pos += [np.float32(u - corner[v][0]), np.float32(w - corner[v][1])]
            lists[i].append((pos[0], pos[1], pos[2], pos[3], j))
            px.append((i, j, back(i, pos[0], pos[1]), back(j, pos[2], pos[3])))
    order = [m for v in range(6) for m in px if m[0] == v]       # the order the context form builds: list after list
    return lists, order, R0


@pytest.mark.parametrize("shared", [False, True])
def test_context_form(ms, cuda, shared):
    rng = np.random.default_rng(17)
    comp = small_rig(ms)
    Rt = rr.perturbed(rr.ring(6), rng, 1.5)
    lists, px, R0 = fabricate_lists(comp, Rt, 12, rng)
    prm = ms.rig_focal_default_params(shared_focal=int(shared))
    f, R, info = comp.refine_rig_focals(lists, prm)
    assert f.dtype == np.float64 and R.dtype == np.float32 and info["matches_used"] == 72 and info["pairs_used"] == 6
    rf, rR, ri = fr.refine(np.full(6, F_CTX), R0, px, shared_focal=shared)
    d = max_angle(R.astype(np.float64), rR.astype(np.float32).astype(np.float64)); df = float(np.max(np.abs(f / rf - 1.0)))
    truth = max_angle(R.astype(np.float64), rr.expected(R0, Rt, 0)); truth_f = float(np.max(np.abs(f / F_SCENE - 1.0)))
    print("shared=%s: %.3e rad and %.3e relative focal to the reference; %.3e rad and %.3e relative focal to the truth; cost %.3e -> %.3e; focals %s"
          % (shared, d, df, truth, truth_f, info["cost_initial"], info["cost_final"], f))
    assert d <= 1e-10 and df <= 1e-10
    # the float positions are known to 2^-24 of up to 512 pixels, 3e-5 pixels, against lever arms of tens of pixels at a focal of 76: 1e-5 in the focal and in radians
    assert truth <= 1e-5 and truth_f <= 1e-5
    assert info["cost_final"] <= info["cost_initial"] and abs(info["max_focal_ratio"] - 1.05) < 1e-4
    assert R[0].tobytes() == np.asarray(synth.camera(6, 160, 120, 90.0, 0)[1], np.float32).tobytes()
    # nothing was applied; the usual chain after ms_set_camera with the refined focal and rotation stitches
    for v in range(6):
        K = np.array([[f[v], 0, 80], [0, f[v], 60], [0, 0, 1]], np.float32)      # K[4] = f (old K[4] / K[0]), the aspect ratio 1
        comp.set_camera(v, K, R[v])
    comp.build_maps(); comp.build_masks(1); comp.init_blender()
    pg = comp.pano_geom()
    out16 = torch.zeros((pg.dst_roi_final.height, pg.dst_roi_final.width, 3), dtype=torch.int16, device=cuda)
    comp.stitch([[to_dev(synth.frame(160, 120, v, 0)) for v in range(6)]], out16s=[out16])
    torch.cuda.synchronize()
    assert int(out16.abs().max()) > 0
    comp.close()


def test_context_form_state_and_refusals(ms, cuda):
    comp = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    for v in range(6):
        comp.set_camera(v, *synth.camera(6, 160, 120, 90.0, v))
    lists = [[(10.0 + 3 * q, 20.0 + 5 * q, 30.0 + 2 * q, 40.0 + q, (v + 1) % 6) for q in range(4)] for v in range(6)]
    with pytest.raises(ms.MsError, match="-5.*ms_build_maps first"):         # MS_ERR_STATE
        comp.refine_rig_focals(lists)
    comp.build_maps()
    comp.refine_rig_focals(lists)
    with pytest.raises(ms.MsError, match="-1.*names view"):
        comp.refine_rig_focals([[(10.0, 20.0, 30.0, 40.0, v)] * 4 for v in range(6)])
    # a pixel half a turn along the warper's u axis shows what lies behind the camera
    behind = [list(l) for l in lists]
    behind[2][1] = (10.0 + math.pi * comp.cfg.warp_scale, 20.0, 30.0, 40.0, 3)
    with pytest.raises(ms.MsError, match="-1.*match 1 of view 2.*behind"):
        comp.refine_rig_focals(behind)
    # a context with two focals cannot share one
    two = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    for v in range(6):
        K, R0 = synth.camera(6, 160, 120, 90.0, v)
        if v == 3:
            K[0][0] = K[1][1] = 81.0
        two.set_camera(v, K, R0)
    two.build_maps()
    two.refine_rig_focals(lists)
    with pytest.raises(ms.MsError, match="-1.*shared_focal.*view 3"):
        two.refine_rig_focals(lists, ms.rig_focal_default_params(shared_focal=1))
    two.close()
    # a context on the caller's own maps has no cameras
    rois = [comp.view_geom(v).roi.tuple() for v in range(6)]
    maps = [comp.maps(v) for v in range(6)]
    twin = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    twin.set_maps(rois, [m[0].clone() for m in maps], [m[1].clone() for m in maps])
    assert twin.map_source() == ms.MAPS_CUSTOM
    with pytest.raises(ms.MsError, match="-2.*ms_set_maps"):                 # MS_ERR_UNSUPPORTED
        twin.refine_rig_focals(lists)
    # a lens context: the focal cannot be moved without the inverse distortion
    lens = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    for v in range(6):
        lens.set_lens(v, L.to_ms(ms, ("brown", (-0.1, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), 0.0)))
        lens.set_camera(v, *synth.camera(6, 160, 120, 90.0, v))
    lens.build_maps()
    assert lens.map_source() == ms.MAPS_LENS
    with pytest.raises(ms.MsError, match="-2.*inverse distortion"):
        lens.refine_rig_focals(lists)
    lens.refine_rig(lists)                                                   # (the rotation refinement takes it)
    lens.close(); twin.close(); comp.close()


# ---- 7. from pixels, with an unknown rig --------------------------------------------------------------------------
PX_N = 8


def true_rig8():
    """8 views, every view but view 0 up to 1.5 degrees off the ring about each axis"""
    R = rr.perturbed(rr.ring(PX_N), np.random.default_rng(88), 1.5)
    R[0] = np.eye(3)
    return R


def unknown_rig_case(ms):
    """the whole pipeline on 8 rendered 640 x 480 views of 90 degrees (true focal 320, which nothing below is told); returns the figures the test asserts on"""
    import test_rig_pixels_gpu as T
    assert (T.W, T.H, T.HFOV) == (640, 480, 90.0)
    f_true = (T.W / 2.0) / math.tan(math.radians(T.HFOV) / 2.0)
    Rt = true_rig8()
    scale = synth.warp_scale(T.OUT_W)                 # the texture's cell size only: nothing is warped here
    feats = []
    for v in range(PX_N):
        k, d = ms.orb_detect_and_compute(ms.bgr_to_gray(to_dev(T.render(Rt[v], scale))), None, nfeatures=2500)
        feats.append((k, d))
    pairs, M, inliers = [], [], []
    centre = np.array([T.W * 0.5, T.H * 0.5], np.float32)
    for i, j in rr.ring_pairs(PX_N):
        (k1, d1), (k2, d2) = feats[i], feats[j]
        idx, dist = ms.knn_match_hamming2(d1, d2)
        good = [q for q in range(len(k1)) if idx[q, 1] >= 0 and dist[q, 0] < 0.7 * dist[q, 1]]
        src = np.array([k1[q, :2] - centre for q in good], np.float32).reshape(-1, 2)
        dst = np.array([k2[idx[q, 0], :2] - centre for q in good], np.float32).reshape(-1, 2)
        Hm, inl = (None, np.zeros(0, np.uint8)) if len(good) < 4 else ms.find_homography_ransac(src, dst)
        inliers.append(int(inl.sum()) if Hm is not None else 0)
        if Hm is not None:
            pairs.append((i, j, Hm, inliers[-1]))
            M += [(i, j, src[q].astype(np.float64), dst[q].astype(np.float64)) for q in range(len(good)) if inl[q]]
    prm = ms.rig_focal_default_params(shared_focal=1, huber_px=2.0)
    out = dict(f_true=f_true, inliers=inliers, min_pair_matches=prm.min_pair_matches)
    if min(inliers) >= prm.min_pair_matches:
        f0, R0, est = ms.estimate_rig(PX_N, pairs, (T.W, T.H))
        f, R, info = ms.refine_rig_cameras(f0, R0, M, prm)
        rf, rR, ri = fr.refine(f0, R0, M, shared_focal=True, huber_px=2.0)
        want = rr.expected(R0, Rt, 0)
        out.update(estimate=est, info=info, ref_info=ri, f_start=float(f0[0]), f_refined=float(f[0]), to_reference_rad=max_angle(R, rR),
                   to_reference_focal=float(np.max(np.abs(f / rf - 1.0))), before_px=[rr.angle(R0[v], want[v]) * f_true for v in range(PX_N)],
                   after_px=[rr.angle(R[v], want[v]) * f_true for v in range(PX_N)], focal_err_before_pct=abs(float(f0[0]) / f_true - 1.0) * 100.0,
                   focal_err_after_pct=abs(float(f[0]) / f_true - 1.0) * 100.0)
    return out


def test_unknown_rig_from_pixels(ms, cuda):
    """Measured on MI355X (profiles/rig_focals.jsonl, "rig_focals_pixels"): 23 to 45 RANSAC inliers a neighbouring pair (268 in all); the homography estimate starts
    at a focal of 280.06 against the true 320 (12.5 % off) with the views 3.6 to 14.3 pixels from the truth; refined, the focal is 319.967 (0.0104 % off) and the
    views end 0.37 to 1.41 pixels from the truth, 13 matches beyond the Huber threshold; device and reference 2.2e-11 rad and 1.8e-13 in the focal apart.  The two
    absolute bounds are twice the measured values, rounded up."""
    r = unknown_rig_case(ms)
    print("inliers per neighbouring pair: %s" % r["inliers"])
    assert min(r["inliers"]) >= r["min_pair_matches"], "a neighbouring pair delivered %d inliers, fewer than min_pair_matches: %s" % (min(r["inliers"]), r["inliers"])
    print("focal: true %.3f, homography start %.3f (%.3f %% off), refined %.3f (%.3f %% off)" % (r["f_true"], r["f_start"], r["focal_err_before_pct"], r["f_refined"],
                                                                                             r["focal_err_after_pct"]))
    print("angle to the truth in pixels at the true focal, start:   %s" % ["%.3f" % x for x in r["before_px"]])
    print("angle to the truth in pixels at the true focal, refined: %s" % ["%.3f" % x for x in r["after_px"]])
    print("device against the reference: %.3e rad, %.3e relative focal; estimate %s; info %s; reference %s" % (r["to_reference_rad"], r["to_reference_focal"], r["estimate"],
                                                                                                             r["info"], r["ref_info"]))
    assert r["estimate"]["status"] == 0
    assert r["to_reference_rad"] <= 1e-10 and r["to_reference_focal"] <= 1e-10
    assert r["info"]["cost_final"] <= r["info"]["cost_initial"]
    assert r["focal_err_after_pct"] <= r["focal_err_before_pct"]
    assert all(a <= b for a, b in zip(r["after_px"], r["before_px"])), "a view ends further from the truth than the homography start put it"
    assert r["focal_err_after_pct"] <= FOCAL_BOUND_PCT and max(r["after_px"]) <= ROTATION_BOUND_PX


FOCAL_BOUND_PCT = 0.021        # measured 0.0104 %
ROTATION_BOUND_PX = 2.9        # measured 1.411 pixels at the true focal (view 2)
