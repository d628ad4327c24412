#!/usr/bin/env python3
"""What the focal-and-rotation refinement under lenses (ms_refine_rig_cameras_lens) costs, on one box, medians of 5, host clock around the synchronous C call (the
match and lens arrays built beforehand), the calls of a row ALTERNATING:
  ring6     6 views x 6 neighbouring pairs x 500 matches
  ring16    16 views x 16 pairs x 2000 matches
  each with   none   every lens MS_LENS_NONE, against ms_refine_rig_cameras on the same matches: what the policy costs (the results are the same bits)
              fish   every view behind lens_ref.FISH, brown: behind lens_ref.BROWN, on matches made through those lenses: the Newton solves and sin / cos
  pixels    the fisheye-rig case of tests/test_rig_lens_gpu.py (8 rendered views, ORB, 2-NN + ratio test, ms_lens_unproject_points, RANSAC, ms_refine_rig_cameras_lens)
  deviation the float64-against-longdouble term deviation behind the bound of tests/test_rig_lens_gpu.py::test_accumulate_per_op (CPU only)
Appends one JSON line per row to profiles/rig_lens.jsonl (or --out).

  python tools/time_rig_lens.py [--out profiles/rig_lens.jsonl] [--only ring6,ring16,pixels,deviation]
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

import lens_ref as L
import rig_lens_ref as lr
import rig_ref as rr

CASES = {"ring6": (6, 500), "ring16": (16, 2000)}
LENSES = {"none": L.NONE, "fish": L.FISH, "brown": L.BROWN}


def ring_rows(name, blocks=5):
    import torch
    import msstitch as ms
    n, per_pair = CASES[name]
    lib = ms.load()
    dp = C.POINTER(C.c_double)
    R0 = rr.ring(n)
    f0 = np.full(n, 420.0)                 # above the truth: at a focal below it the rim's pixels leave the field
    prm = ms.rig_focal_default_params()
    info = ms.RigFocalInfo()
    fo = np.empty(n); out = np.empty((n, 3, 3))
    rows = []
    for kind, lens in LENSES.items():
        rng = np.random.default_rng(n)
        ft = 400.0 * (1 + rng.uniform(-0.04, 0.04, n))
        M = lr.make_lens_matches(ft, rr.perturbed(R0, rng, 2.0), [lens] * n, rr.ring_pairs(n), per_pair, rng, noise_px=0.2, spread_deg=15.0)
        arr = ms.rig_px_matches(M)
        larr = ms.lens_array([L.to_ms(ms, lens)] * n)

        def with_lenses():
            rc = lib.ms_refine_rig_cameras_lens(n, f0.ctypes.data_as(dp), R0.ctypes.data_as(dp), larr, arr, len(M), C.byref(prm), fo.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                                C.byref(info), None)
            assert rc == 0, lib.ms_last_error()

        def pinhole():
            rc = lib.ms_refine_rig_cameras(n, f0.ctypes.data_as(dp), R0.ctypes.data_as(dp), arr, len(M), C.byref(prm), fo.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(info), None)
            assert rc == 0, lib.ms_last_error()

        calls = [("lens_call_ms", with_lenses)] + ([("pinhole_call_ms", pinhole)] if kind == "none" else [])
        for _, fn in calls:                # warm-up: code objects, the scratch blocks
            fn()
        runs = {key: [] for key, _ in calls}
        for _ in range(blocks):
            for key, fn in calls:
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                runs[key].append((time.perf_counter() - t) * 1e3)
        with_lenses()
        row = {"what": "rig_lens", "case": name, "lenses": kind, "views": n, "pairs": len(rr.ring_pairs(n)), "matches": len(M), "iterations": info.iterations,
               "stop_reason": info.stop_reason, "launches": 2 * (prm.max_iters + 1), "cost_initial": info.cost_initial, "cost_final": info.cost_final}
        for key, v in runs.items():
            row[key] = statistics.median(v); row[key.replace("_call_ms", "_runs_ms")] = v
        if kind == "none":
            row["ratio_to_pinhole"] = row["lens_call_ms"] / row["pinhole_call_ms"]
        rows.append(row)
    return rows


def pixels_row():
    import msstitch as ms
    import test_rig_lens_gpu as T
    r = T.lens_pixels_case(ms)
    keys = ("f_true", "f_given", "inliers", "info", "f_refined", "f_reference", "focal_err_before_pct", "focal_err_after_pct", "ref_focal_err_after_pct", "before_px", "after_px",
            "ref_after_px", "to_reference_rad", "to_reference_focal")
    return {"what": "rig_lens_pixels", "views": T.PX_N, "size": [640, 480], "lens": "fisheye", **{k: r.get(k) for k in keys}}


def deviation_rows():
    import test_rig_lens_gpu as T
    rows = []
    for m in (1, 64, 65, 257):
        f, R, M, h_mid = T.accumulate_case(m)
        for h in (0.0, h_mid):
            dev = lr.term_deviation(f, R, T.ACC_LENSES, M, h)
            rows.append({"what": "term_deviation", "m": m, "huber_px": h, "deviation_in_2^-52_S": dev, "T": 8.0 * dev})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_lens.jsonl"))
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
