#!/usr/bin/env python3
"""What the focal-and-rotation refinement (ms_refine_rig_cameras) costs, on one box, medians of 5:
  ring6     6 views x 6 neighbouring pairs x 500 matches
  ring16    16 views x 16 pairs x 2000 matches
            each with per-view focals and with a shared focal: wall time of the call (synchronous: grouping on the host, one upload, max_iters + 1 rounds of two
            kernels, one copy back; host clock around the C call, the match array built beforehand) and its iterations, ALTERNATING with ms_refine_rig_rotations on the
            same matches as rays (the focals held at the truth), and the ratio of the two
  pixels    the unknown-rig case of tests/test_rig_focal_gpu.py (8 rendered views, ORB, 2-NN + ratio test, RANSAC, ms_estimate_rig, ms_refine_rig_cameras): the focal
            error in percent and every view's angle to the truth in pixels at the true focal, at the homography start and refined
Appends one JSON line per row to profiles/rig_focals.jsonl (or --out).

  python tools/time_rig_focals.py [--out profiles/rig_focals.jsonl] [--only ring6,ring6-shared,ring16,ring16-shared,pixels]
  python tools/time_rig_focals.py --once ring16      # a warm-up and ONE call, nothing written: the run to put under a kernel trace
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import msstitch as ms
import rig_focal_ref as fr
import rig_ref as rr

CASES = {"ring6": (6, 500, 0), "ring6-shared": (6, 500, 1), "ring16": (16, 2000, 0), "ring16-shared": (16, 2000, 1)}


def ring_case(name):
    """the cameras to start from, the matches as centred pixels and the same matches as unit rays (a pixel (x, y) at the true focal f is the ray (x, y, f) / |.|)"""
    n, per_pair, shared = CASES[name]
    rng = np.random.default_rng(n)
    R0 = rr.ring(n)
    ft = np.full(n, 400.0) if shared else 400.0 * (1 + rng.uniform(-0.04, 0.04, n))
    M = fr.make_px_matches(ft, rr.perturbed(R0, rng, 2.0), rr.ring_pairs(n), per_pair, rng, noise_px=0.2, spread_deg=15.0)
    ray = lambda p, f: np.array([p[0], p[1], f]) / np.linalg.norm([p[0], p[1], f])
    rays = [(i, j, ray(a, ft[i]), ray(b, ft[j])) for i, j, a, b in M]
    return n, shared, np.full(n, 380.0), R0, M, rays


def ring_row(name, blocks=5, once=False):
    n, shared, f0, R0, M, rays = ring_case(name)
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    arr, rarr = ms.rig_px_matches(M), ms.rig_matches(rays)
    prm, rprm = ms.rig_focal_default_params(shared_focal=shared), ms.rig_refine_default_params()
    info, rinfo = ms.RigFocalInfo(), ms.RigRefineInfo()
    fo = np.empty(n); out = np.empty((n, 3, 3)); rout = np.empty((n, 3, 3))

    def focal():
        rc = lib.ms_refine_rig_cameras(n, f0.ctypes.data_as(dp), R0.ctypes.data_as(dp), arr, len(M), C.byref(prm), fo.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(info), None)
        assert rc == 0, lib.ms_last_error()

    def rotations():
        rc = lib.ms_refine_rig_rotations(n, R0.ctypes.data_as(dp), rarr, len(rays), C.byref(rprm), rout.ctypes.data_as(dp), C.byref(rinfo), None)
        assert rc == 0, lib.ms_last_error()

    focal(); rotations()      # warm-up: code objects, the scratch blocks
    if once:
        torch.cuda.synchronize()
        focal()
        return None
    runs, rruns = [], []
    for _ in range(blocks):
        for fn, acc in ((focal, runs), (rotations, rruns)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    rf, rR, ri = fr.refine(f0, R0, M, shared_focal=bool(shared))
    ref_ms = (time.perf_counter() - t) * 1e3
    return {"what": "rig_focals", "case": name, "views": n, "pairs": len(rr.ring_pairs(n)), "matches": len(M), "shared_focal": shared, "unknowns": 3 * (n - 1) + (1 if shared else n),
            "call_ms": statistics.median(runs), "runs_ms": runs, "iterations": info.iterations, "stop_reason": info.stop_reason, "launches": 2 * (prm.max_iters + 1),
            "cost_initial": info.cost_initial, "cost_final": info.cost_final, "max_focal_ratio": info.max_focal_ratio,
            "rotations_only_call_ms": statistics.median(rruns), "rotations_only_runs_ms": rruns, "rotations_only_iterations": rinfo.iterations,
            "ratio_to_rotations_only": statistics.median(runs) / statistics.median(rruns),
            "numpy_reference_ms": ref_ms, "numpy_reference_iterations": ri["iterations"], "device_to_reference_rad": max(rr.angle(out[v], rR[v]) for v in range(n)),
            "device_to_reference_focal": float(np.max(np.abs(fo / rf - 1.0)))}


def pixels_row():
    import test_rig_focal_gpu as T
    r = T.unknown_rig_case(ms)
    return {"what": "rig_focals_pixels", "views": T.PX_N, "size": [640, 480], "true_focal": r["f_true"], "ransac_inliers_per_pair": r["inliers"], "estimate": r.get("estimate"),
            "info": r.get("info"), "focal_start": r.get("f_start"), "focal_refined": r.get("f_refined"), "focal_err_start_pct": r.get("focal_err_before_pct"),
            "focal_err_refined_pct": r.get("focal_err_after_pct"), "start_px": r.get("before_px"), "refined_px": r.get("after_px"),
            "max_refined_px": max(r["after_px"]) if "after_px" in r else None, "device_to_reference_rad": r.get("to_reference_rad"),
            "device_to_reference_focal": r.get("to_reference_focal")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_focals.jsonl"))
    ap.add_argument("--only", default="ring6,ring6-shared,ring16,ring16-shared,pixels")
    ap.add_argument("--once", default=None, help="run a warm-up and one ms_refine_rig_cameras call of this case and exit")
    args = ap.parse_args()
    if args.once:
        ring_row(args.once, once=True)
        return
    rows = [pixels_row() if name == "pixels" else ring_row(name) for name in args.only.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
