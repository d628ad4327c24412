"""Rig rotation refinement on the GPU (csrc/rig.hip) against the numpy reference of tests/rig_ref.py.

1. ms_rig_accumulate per op: every entry of cost, H and g within the worst-case bound for two summation orders of the same rounded terms
2. exact recovery from noise-free matches, either end of the rig and its middle as the anchor
3. noisy matches and outliers (Huber) against the reference on the same inputs
4. determinism: two calls return the same bits
5. degenerate but legal inputs
6. ms_warper_rays against the lens map kernels
7. the context form, ms_refine_rig: analytic and fisheye contexts, refusals, the calibration chain after it

The stop step at the rounding floor depends on the order of the sums, so no test compares iteration counts."""
import math

import numpy as np
import pytest
import torch

import lens_ref as L
import rig_lm_cases as lm_cases
import rig_ref as rr
import synth
from helpers import to_dev

pytestmark = pytest.mark.gpu

_REF = {}


def ref_refine(key, R_in, M, **kw):
    """the reference's answer for a named case, computed once"""
    if key not in _REF:
        _REF[key] = rr.refine(R_in, M, **kw)
    return _REF[key]


def device_refine(ms, R_in, M, **kw):
    return ms.refine_rig_rotations(R_in, M, ms.rig_refine_default_params(**{{"anchor": "anchor_view"}.get(k, k): v for k, v in kw.items()}))


def max_angle(A, B):
    return max(rr.angle(a, b) for a, b in zip(A, B))


# ---- 1. accumulate, per op --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4, 63, 64, 65, 255, 256, 257, 1000, 1025])
def test_accumulate_per_op(ms, cuda, m):
    """3 views, pair (0, 1) with m matches, pair (1, 2) with 5, pair (0, 2) with none, listed in shuffled order with a third of them as (j, i).  The terms of the
    two implementations are the same bits (the contract fixes their arithmetic); only the order of the sums differs, and for two orders of n rounded terms the
    results differ by at most (n - 1) 2^-52 S, S the sum of the terms' absolute values: the bound below, (m + 8) 2^-52 S, covers the m + 5 terms of any entry.
    The sizes are those of tests/test_rig_focal_gpu.py and 1025: the two tests run one reduction body (csrc/rig_lm.hpp) through its two instances."""
    rng = np.random.default_rng(100 + m)
    R = rr.perturbed(rr.ring(3), rng, 5.0)
    M = rr.make_matches(rr.perturbed(rr.ring(3), rng, 5.0), [(0, 1), (1, 2)], [m, 5], rng, noise=2e-3)
    M = [M[k] for k in rng.permutation(len(M))]
    M = [(vb, va, b, a) if rng.uniform() < 1 / 3 else (va, vb, a, b) for va, vb, a, b in M]
    i, j, a, b = rr.unpack(M)
    s = rr.terms(R, i, j, a, b, 0.0)[1]
    h_mid = float(np.sort(s)[len(s) // 2 - 1] if len(s) > 1 else 0.5 * s[0])
    assert 0 < (s > h_mid).sum() < len(s)                    # matches on both Huber branches
    for h in (0.0, h_mid):
        cost, H, g = ms.rig_accumulate(R, M, h)
        rc, rH, rg, sc, sH, sg = rr.accumulate(R, M, h, with_abs=True)
        tol = (m + 8) * 2.0 ** -52
        print("m=%d h=%g: cost %.3e of %.3e, H %.3e, g %.3e (max |diff| / S)" % (m, h, abs(cost - rc) / sc, tol, np.max(np.abs(H - rH) / np.maximum(sH, 1e-300)),
                                                                                   np.max(np.abs(g - rg) / np.maximum(sg, 1e-300))))
        assert abs(cost - rc) <= tol * sc
        assert np.all(np.abs(H - rH) <= tol * sH) and np.all(np.abs(g - rg) <= tol * sg)
        assert np.array_equal(H, H.T) and not H[0:3, 6:9].any() and H[3:6, 3:6].any()


@pytest.mark.parametrize("graph", ["complete", "ring"])
def test_accumulate_per_op_16_views(ms, cuda, graph):
    """16 views (rows up to 48 of the full matrix): the complete graph, 120 pairs of 3 matches, and the ring, 16 pairs of 6, shuffled with a third listed as (j, i)
    (tests/rig_lm_cases.py).  The bound of test_accumulate_per_op per entry: the cost sums every match, an entry of H or g at most the matches of one view.  H is
    symmetric bit for bit, and a block is zero exactly where its pair has no match: none of the complete graph's, 104 of the ring's 120."""
    _, R, M, pairs = lm_cases.accumulate_case("rot", graph)
    n_cost, n_entry = lm_cases.accumulate_terms(M)
    for h in (0.0, lm_cases.accumulate_huber("rot", None, R, M)):
        cost, H, g = ms.rig_accumulate(R, M, h)
        rc, rH, rg, sc, sH, sg = rr.accumulate(R, M, h, with_abs=True)
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
                blk = H[3 * i:3 * i + 3, 3 * j:3 * j + 3]
                assert blk.any() == ((i, j) in used), (i, j)
                zero += not blk.any()
        assert zero == (0 if graph == "complete" else 104) and all(H[3 * v:3 * v + 3, 3 * v:3 * v + 3].any() for v in range(16))


# ---- 2. exact recovery ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, per_pair", [(2, 3), (3, 8), (6, 24), (16, 16)])
def test_exact_recovery(ms, cuda, n, per_pair):
    rng = np.random.default_rng(5 + n)
    R0 = rr.ring(n)
    Rt = rr.perturbed(R0, rng, 5.0)
    pairs = [(0, 1), (1, 2), (0, 2)] if n == 3 else rr.ring_pairs(n)
    M = rr.make_matches(Rt, pairs, per_pair, rng)
    for anchor in sorted({0, n // 2, n - 1}) if n >= 3 else (0, n - 1):
        R, info = device_refine(ms, R0, M, anchor=anchor, step_tol=1e-13, min_pair_matches=min(4, per_pair))
        err = max_angle(R, rr.expected(R0, Rt, anchor))
        print("n=%d anchor=%d: %.3e rad to the truth, %d iterations, stop %d, cost %.3e -> %.3e" % (n, anchor, err, info["iterations"], info["stop_reason"],
                                                                                               info["cost_initial"], info["cost_final"]))
        assert err <= 1e-12
        assert R[anchor].tobytes() == R0[anchor].tobytes()
        assert info["matches_used"] == len(M) and info["pairs_used"] == len(pairs) and info["pairs_ignored"] == 0 and info["outliers"] == 0
        assert info["cost_final"] <= info["cost_initial"] and 0.01 < info["max_rotation_rad"] < 0.4


# ---- 3. noise and outliers against the reference ------------------------------------------------------------------
NOISY = {
    "ring6": dict(n=6, per_pair=64, noise=5e-4, outlier_frac=0.0, huber_rad=0.0),
    "ring6-huber": dict(n=6, per_pair=64, noise=5e-4, outlier_frac=0.2, huber_rad=3e-3),
    "tri3": dict(n=3, per_pair=5, noise=2e-3, outlier_frac=0.0, huber_rad=0.0),
    "pair2": dict(n=2, per_pair=3, noise=1e-3, outlier_frac=0.0, huber_rad=0.0),
}


def noisy_case(name):
    c = NOISY[name]
    rng = np.random.default_rng(sorted(NOISY).index(name) + 70)
    R0 = rr.ring(c["n"])
    pairs = [(0, 1), (1, 2), (0, 2)] if c["n"] == 3 else rr.ring_pairs(c["n"])
    M = rr.make_matches(rr.perturbed(R0, rng, 5.0), pairs, c["per_pair"], rng, noise=c["noise"], outlier_frac=c["outlier_frac"])
    return R0, M, dict(huber_rad=c["huber_rad"], min_pair_matches=min(4, c["per_pair"]))


@pytest.mark.parametrize("name", sorted(NOISY))
def test_noisy_matches_against_the_reference(ms, cuda, name):
    R0, M, kw = noisy_case(name)
    Rr, ri = ref_refine(name, R0, M, **kw)
    R, info = device_refine(ms, R0, M, **kw)
    d = max_angle(R, Rr)
    print("%s: %.3e rad between device and reference; cost %.6e -> %.6e (reference %.6e); outliers %d (reference %d); iterations %d (reference %d)"
          % (name, d, info["cost_initial"], info["cost_final"], ri["cost_final"], info["outliers"], ri["outliers"], info["iterations"], ri["iterations"]))
    assert d <= 1e-10
    assert info["cost_final"] <= info["cost_initial"]
    assert abs(info["outliers"] - ri["outliers"]) <= 2 and (kw["huber_rad"] > 0) == (info["outliers"] > 0)
    assert info["matches_used"] == ri["matches_used"] and info["pairs_used"] == ri["pairs_used"]
    assert abs(info["max_rotation_rad"] - ri["max_rotation_rad"]) <= 1e-10


# ---- 4. determinism ---------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits(ms, cuda):
    R0, M, kw = noisy_case("ring6-huber")
    a = device_refine(ms, R0, M, **kw)
    b = device_refine(ms, R0, M, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    ca = ms.rig_accumulate(R0, M, 3e-3); cb = ms.rig_accumulate(R0, M, 3e-3)
    assert ca[0] == cb[0] and ca[1].tobytes() == cb[1].tobytes() and ca[2].tobytes() == cb[2].tobytes()


# ---- 5. degenerate but legal --------------------------------------------------------------------------------------
def test_a_pair_of_one_repeated_ray_is_legal(ms, cuda):
    """4 matches that are one ray: the rotation about it is free (H is singular before the damping)"""
    rng = np.random.default_rng(8)
    R0 = rr.ring(2)
    Rt = rr.perturbed(R0, rng, 3.0)
    M = rr.make_matches(Rt, [(0, 1)], 1, rng) * 4
    R, info = device_refine(ms, R0, M)
    assert np.all(np.isfinite(R)) and all(math.isfinite(float(v)) for v in info.values())
    assert info["cost_final"] <= info["cost_initial"] and info["matches_used"] == 4
    assert R[0].tobytes() == R0[0].tobytes() and abs(np.linalg.det(R[1]) - 1.0) < 1e-12


def test_a_view_cut_off_by_min_pair_matches_is_named(ms, cuda):
    rng = np.random.default_rng(3)
    R = rr.ring(4)
    M = rr.make_matches(R, [(0, 1), (1, 2), (2, 3)], [5, 3, 5], rng)
    with pytest.raises(ms.MsError, match="view 2 is not connected"):
        device_refine(ms, R, M)
    Rr, info = device_refine(ms, R, M, min_pair_matches=3)       # the same matches with the pair let in
    assert info["pairs_ignored"] == 0 and info["pairs_used"] == 3


# ---- 6. rays against the map kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("p", ["sph", "cyl"])
@pytest.mark.parametrize("lens", [L.NONE, ("brown", (-0.18, 0.03, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0), 0.0)], ids=["none", "brown"])
def test_rays_against_the_lens_map_kernels(ms, cuda, p, lens):
    """for every integer (u, v) of a 37 x 23 window, ms_lens_project(K, lens, ms_warper_rays(u, v)) is the entry ms_build_warp_maps_lens stores, within 1 float ulp
    (the lens maps' own stated bound), or both are the (-1, -1) marker.  A second window, half a turn away, is behind the camera: markers only."""
    proj = ms.PROJ_SPHERICAL if p == "sph" else ms.PROJ_CYLINDRICAL
    cfg = synth.CONFIGS["mini6"]
    scale = synth.warp_scale(cfg["out_w"])
    K, _ = synth.camera(6, cfg["w"], cfg["h"], cfg["hfov_deg"], 0)
    R = (rr.exp_so3(np.array([0.03, 0.4, -0.02]))).astype(np.float32)
    ml = L.to_ms(ms, lens)
    u_c, v_c = rr.warper_forward(rr.SPHERICAL if p == "sph" else rr.CYLINDRICAL, scale, R.astype(np.float64)[:, 2])
    n_seen = 0
    for tl_u, tl_v in ((int(u_c) - 18, int(v_c) - 11), (int(u_c) - 18 + int(round(math.pi * scale)), int(v_c) - 11)):
        mx, my = ms.build_warp_maps_lens(proj, tl_u, tl_v, 23, 37, K, R, ml, scale)
        mx, my = mx.cpu().numpy(), my.cpu().numpy()
        uv = np.array([(tl_u + x, tl_v + y) for y in range(23) for x in range(37)], np.float32)
        rays = ms.warper_rays(proj, scale, R.astype(np.float64), uv)
        for k, ray in enumerate(rays):
            (px, py), seen = ms.lens_project(K, ml, ray)
            gx, gy = mx[k // 37, k % 37], my[k // 37, k % 37]
            if not seen:
                assert (gx, gy) == (-1.0, -1.0), (uv[k], gx, gy)
                continue
            n_seen += 1
            assert abs(np.float32(px) - gx) <= np.spacing(np.abs(gx)) and abs(np.float32(py) - gy) <= np.spacing(np.abs(gy)), (uv[k], px, py, gx, gy)
    assert n_seen == 37 * 23


# ---- 7. the context form ----------------------------------------------------------------------------------------
FISH160 = ("fisheye", (-0.02, 0.003, 0.0, 0.0), 100.0)


def small_rig(ms, p, fisheye, R=None):
    """6 views of 160 x 120 on the ideal ring (or with the rotations R), calibrated up to the maps"""
    proj = ms.PROJ_SPHERICAL if p == "sph" else ms.PROJ_CYLINDRICAL
    comp = ms.Compositor(6, (160, 120), proj, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    for v in range(6):
        K, R0 = synth.camera(6, 160, 120, 90.0, v)
        if fisheye:
            K = np.array([[60.0, 0, 80], [0, 60.0, 60], [0, 0, 1]], np.float32)
            comp.set_lens(v, L.to_ms(ms, FISH160))
        comp.set_camera(v, K, R0 if R is None else R[v])
    comp.build_maps()
    return comp


def fabricate_lists(comp, p, Rt, per_pair, rng):
    """float match lists of a context whose maps were built with the ring R0 while the cameras are really at Rt: a world ray d is seen by view v at the warper
    position of R0_v Rt_v^T d, minus the view's corner.  Returns the lists and the same matches as float64 rays (numpy formulas on the float positions)."""
    proj = rr.SPHERICAL if p == "sph" else rr.CYLINDRICAL
    scale = float(np.float32(comp.cfg.warp_scale))
    R0 = np.array([synth.camera(6, 160, 120, 90.0, v)[1] for v in range(6)], np.float64)
    corner = [comp.view_geom(v).roi.tuple()[:2] for v in range(6)]
    lists = [[] for _ in range(6)]
    rays = []
    for i, j in rr.ring_pairs(6):
        mid = Rt[i][:, 2] + Rt[j][:, 2]
        mid /= np.linalg.norm(mid)
        for _ in range(per_pair):
            d = rr.exp_so3(np.radians(rng.uniform(-12, 12, 3))) @ mid
            pos = []
            for v in (i, j):
                u, w = rr.warper_forward(proj, scale, R0[v] @ Rt[v].T @ d)
                pos += [np.float32(u - corner[v][0]), np.float32(w - corner[v][1])]
            lists[i].append((pos[0], pos[1], pos[2], pos[3], j))
            rays.append((i, j, rr.warper_ray(proj, scale, R0[i], corner[i][0] + float(pos[0]), corner[i][1] + float(pos[1])),
                         rr.warper_ray(proj, scale, R0[j], corner[j][0] + float(pos[2]), corner[j][1] + float(pos[3]))))
    order = [m for v in range(6) for m in rays if m[0] == v]       # the order the context form builds: list after list
    return lists, order, R0


@pytest.mark.parametrize("p, fisheye", [("sph", False), ("cyl", False), ("sph", True)])
def test_context_form(ms, cuda, p, fisheye):
    rng = np.random.default_rng(17)
    comp = small_rig(ms, p, fisheye)
    assert comp.map_source() == (ms.MAPS_LENS if fisheye else ms.MAPS_ANALYTIC)
    R0d = rr.ring(6)
    Rt = rr.perturbed(R0d, rng, 1.5)
    lists, rays, R0 = fabricate_lists(comp, p, Rt, 12, rng)
    R, info = comp.refine_rig(lists)
    assert R.dtype == np.float32 and info["matches_used"] == 72 and info["pairs_used"] == 6
    Rr, ri = rr.refine(R0, rays)
    d = max_angle(R.astype(np.float64), Rr.astype(np.float32).astype(np.float64))
    truth = max_angle(R.astype(np.float64), rr.expected(R0, Rt, 0))
    print("%s fisheye=%s: %.3e rad to the reference, %.3e rad to the truth (bound %.3e), cost %.3e -> %.3e" % (p, fisheye, d, truth, 2.0 ** -21 * math.pi,
                                                                                                          info["cost_initial"], info["cost_final"]))
    assert d <= 1e-10
    assert truth <= 2.0 ** -21 * math.pi
    assert R[0].tobytes() == np.asarray(synth.camera(6, 160, 120, 90.0, 0)[1], np.float32).tobytes()
    # nothing was applied; the usual chain after ms_set_camera(R_out) stitches
    for v in range(6):
        K = np.array([[60.0, 0, 80], [0, 60.0, 60], [0, 0, 1]], np.float32) if fisheye else synth.camera(6, 160, 120, 90.0, v)[0]
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
    lists = [[(10.0, 20.0, 30.0, 40.0, (v + 1) % 6)] * 4 for v in range(6)]
    with pytest.raises(ms.MsError, match="-5.*ms_build_maps first"):         # MS_ERR_STATE
        comp.refine_rig(lists)
    comp.build_maps()
    comp.refine_rig(lists)
    with pytest.raises(ms.MsError, match="-1.*names view"):
        comp.refine_rig([[(10.0, 20.0, 30.0, 40.0, v)] * 4 for v in range(6)])
    # a context on the caller's own maps has no cameras
    rois = [comp.view_geom(v).roi.tuple() for v in range(6)]
    maps = [comp.maps(v) for v in range(6)]
    twin = ms.Compositor(6, (160, 120), ms.PROJ_SPHERICAL, synth.warp_scale(320), num_bands=2, out_size=(320, 160))
    twin.set_maps(rois, [m[0].clone() for m in maps], [m[1].clone() for m in maps])
    assert twin.map_source() == ms.MAPS_CUSTOM
    with pytest.raises(ms.MsError, match="-2.*ms_set_maps"):                 # MS_ERR_UNSUPPORTED
        twin.refine_rig(lists)
    twin.close(); comp.close()
