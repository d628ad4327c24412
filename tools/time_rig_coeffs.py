#!/usr/bin/env python3
"""What refining the shared lens's coefficients (ms_refine_rig_coeffs) costs beside ms_refine_rig_cameras_lens on the same matches, on one box, medians of 5, host
clock around the synchronous C call (the match and lens arrays built beforehand), the two calls of a row ALTERNATING:
  ring6     6 views x 6 neighbouring pairs x 500 matches
  ring16    16 views x 16 pairs x 2000 matches
  each for    fish / brown (every view behind lens_ref.FISH / lens_ref.BROWN) and G = 1, 2, 4 free coefficients (k1; k1 k2; fisheye k1..k4, Brown k1 k2 p1 p2)
  pixels    the rendered fisheye scene of tests/test_rig_lens_gpu.py (8 views, ORB, 2-NN + ratio test, RANSAC) with the pipeline given coefficients of ZERO and a focal
            10 % off: ms_refine_rig_coeffs over k1, k2 against ms_refine_rig_cameras_lens holding the wrong (zero) coefficients
  deviation the float64-against-longdouble term deviation behind the bound of tests/test_rig_coeffs_gpu.py::test_accumulate_per_op (CPU only)
Appends one JSON line per row to profiles/rig_coeffs.jsonl (or --out).

  python tools/time_rig_coeffs.py [--out profiles/rig_coeffs.jsonl] [--only ring6,ring16,pixels,deviation]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import lens_ref as L
import rig_coeff_ref as cr
import rig_lens_ref as lr
import rig_ref as rr

CASES = {"ring6": (6, 500), "ring16": (16, 2000)}
LENSES = {"fish": L.FISH, "brown": L.BROWN}
FREE = {1: 0b1, 2: 0b11, 4: 0b1111}


def ring_rows(name, blocks=5):
    import torch
    import msstitch as ms
    n, per_pair = CASES[name]
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    R0 = rr.ring(n)
    f0 = np.full(n, 420.0)                 # above the truth: at a focal below it the rim's pixels leave the field
    fo = np.empty(n); out = np.empty((n, 3, 3))
    rows = []
    for kind, lens in LENSES.items():
        rng = np.random.default_rng(n)
        ft = 400.0 * (1 + rng.uniform(-0.04, 0.04, n))
        M = lr.make_lens_matches(ft, rr.perturbed(R0, rng, 2.0), [lens] * n, rr.ring_pairs(n), per_pair, rng, noise_px=0.2, spread_deg=15.0)
        arr = ms.rig_px_matches(M)
        ml = L.to_ms(ms, lens)
        larr = ms.lens_array([ml] * n)
        fprm = ms.rig_focal_default_params(); finfo = ms.RigFocalInfo()
        for G, free in FREE.items():
            cprm = ms.rig_coeff_default_params(free_coeffs=free); cinfo = ms.RigCoeffInfo(); lens_out = ms.Lens()

            def coeffs():
                rc = lib.ms_refine_rig_coeffs(n, f0.ctypes.data_as(dp), R0.ctypes.data_as(dp), C.byref(ml), arr, len(M), C.byref(cprm), fo.ctypes.data_as(dp),
                                              out.ctypes.data_as(dp), C.byref(lens_out), C.byref(cinfo), None)
                assert rc == 0, lib.ms_last_error()

            def fixed():
                rc = lib.ms_refine_rig_cameras_lens(n, f0.ctypes.data_as(dp), R0.ctypes.data_as(dp), larr, arr, len(M), C.byref(fprm), fo.ctypes.data_as(dp),
                                                    out.ctypes.data_as(dp), C.byref(finfo), None)
                assert rc == 0, lib.ms_last_error()

            calls = [("coeff_call_ms", coeffs), ("fixed_lens_call_ms", fixed)]
            for _, fn in calls:                # warm-up: code objects, the scratch blocks
                fn()
            runs = {key: [] for key, _ in calls}
            for _ in range(blocks):
                for key, fn in calls:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fn()
                    runs[key].append((time.perf_counter() - t) * 1e3)
            row = {"what": "rig_coeffs", "case": name, "lens": kind, "G": G, "free_coeffs": free, "views": n, "pairs": len(rr.ring_pairs(n)), "matches": len(M),
                   "iterations": cinfo.iterations, "fixed_lens_iterations": finfo.iterations, "stop_reason": cinfo.stop_reason, "launches": 2 * (cprm.max_iters + 1),
                   "cost_initial": cinfo.cost_initial, "cost_final": cinfo.cost_final, "fixed_lens_cost_final": finfo.cost_final, "max_coeff_change": cinfo.max_coeff_change,
                   "k_out": list(lens_out.k)}
            for key, v in runs.items():
                row[key] = statistics.median(v); row[key.replace("_call_ms", "_runs_ms")] = v
            row["ratio_to_fixed_lens"] = row["coeff_call_ms"] / row["fixed_lens_call_ms"]
            rows.append(row)
    return rows


def pixels_row():
    """tests/test_rig_lens_gpu.py::lens_pixels_case's scene and matcher; the pipeline knows neither the coefficients (it starts at zero) nor the focal (10 % high)"""
    import msstitch as ms
    import synth
    import test_rig_focal_gpu as G
    import test_rig_lens_gpu as T
    import test_rig_pixels_gpu as P
    from helpers import to_dev
    n = T.PX_N
    f_true = (P.W / 2.0) / math.tan(math.radians(P.HFOV) / 2.0); f_given = f_true * T.FOCAL_OFF
    Rt = G.true_rig8(); R0 = rr.ring(n)
    lens_true = L.FISH; lens_given = ("fisheye", (0.0, 0.0, 0.0, 0.0), lens_true[2]); mg = L.to_ms(ms, lens_given)
    Kg = [[f_given, 0.0, P.W / 2.0], [0.0, f_given, P.H / 2.0], [0.0, 0.0, 1.0]]
    feats = []
    for v in range(n):
        k, d = ms.orb_detect_and_compute(ms.bgr_to_gray(to_dev(T.render_lens(Rt[v], synth.warp_scale(P.OUT_W), f_true, lens_true, P.W, P.H))), None, nfeatures=2500)
        rays, seen = ms.lens_unproject_points(Kg, mg, np.ascontiguousarray(k[:, :2], np.float32))
        feats.append((k, d, rays, seen))
    M, inliers = [], []
    centre = np.array([P.W * 0.5, P.H * 0.5], np.float64)
    for i, j in rr.ring_pairs(n):
        (k1, d1, r1, s1), (k2, d2, r2, s2) = feats[i], feats[j]
        idx, dist = ms.knn_match_hamming2(d1, d2)
        good = [q for q in range(len(k1)) if idx[q, 1] >= 0 and dist[q, 0] < 0.7 * dist[q, 1] and s1[q] and s2[idx[q, 0]] and r1[q, 2] > 0.1 and r2[idx[q, 0], 2] > 0.1]
        src = np.array([f_given * r1[q, :2] / r1[q, 2] for q in good], np.float32).reshape(-1, 2)
        dst = np.array([f_given * r2[idx[q, 0], :2] / r2[idx[q, 0], 2] for q in good], np.float32).reshape(-1, 2)
        Hm, inl = (None, np.zeros(0, np.uint8)) if len(good) < 4 else ms.find_homography_ransac(src, dst)
        inliers.append(int(inl.sum()) if Hm is not None else 0)
        if Hm is not None:
            M += [(i, j, k1[q, :2].astype(np.float64) - centre, k2[idx[q, 0], :2].astype(np.float64) - centre) for n_, q in enumerate(good) if inl[n_]]
    want = rr.expected(R0, Rt, 0)
    f0 = np.full(n, f_given)
    px = lambda R: [rr.angle(R[v], want[v]) * f_true for v in range(n)]
    f, R, lo, info = ms.refine_rig_coeffs(f0, R0, mg, M, ms.rig_coeff_default_params(shared_focal=1, huber_px=2.0, free_coeffs=0b11))
    ff, Rf, finfo = ms.refine_rig_cameras_lens(f0, R0, [mg] * n, M, ms.rig_focal_default_params(shared_focal=1, huber_px=2.0))
    return {"what": "rig_coeffs_pixels", "views": n, "size": [P.W, P.H], "lens": "fisheye", "k_true": list(lens_true[1]), "k_given": [0.0] * 4, "k_refined": list(lo.k)[:4],
            "f_true": f_true, "f_given": f_given, "f_refined": float(f[0]), "f_fixed_zero_lens": float(ff[0]), "inliers": inliers, "before_px": px(R0), "after_px": px(R),
            "fixed_zero_lens_after_px": px(Rf), "focal_err_before_pct": abs(f_given / f_true - 1) * 100, "focal_err_after_pct": abs(float(f[0]) / f_true - 1) * 100,
            "fixed_zero_lens_focal_err_pct": abs(float(ff[0]) / f_true - 1) * 100, "info": info, "fixed_zero_lens_info": finfo,
            "rim_profile_error": abs(L.theta_d(list(lo.k)[:4], 1.0) - L.theta_d(lens_true[1], 1.0))}


def deviation_rows():
    import test_rig_coeffs_gpu as T
    rows = []
    for name in sorted(T.ACC):
        lens, free = T.ACC[name]
        for m in (1, 64, 65, 257):
            f, R, M, h_mid = T.accumulate_case(m, lens)
            for h in (0.0, h_mid):
                dev = cr.term_deviation(f, R, lens, free, M, h)
                rows.append({"what": "term_deviation", "case": name, "m": m, "huber_px": h, "deviation_in_2^-52_S": dev, "T": 8.0 * dev})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_coeffs.jsonl"))
    ap.add_argument("--only", default="ring6,ring16,pixels,deviation")
    args = ap.parse_args()
    rows = []
    for name in args.only.split(","):
        rows += [pixels_row()] if name == "pixels" else deviation_rows() if name == "deviation" else ring_rows(name)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r, default=float))
            f.write(json.dumps(r, default=float) + "\n")


if __name__ == "__main__":
    main()
