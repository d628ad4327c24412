#!/usr/bin/env python3
"""What the content-aware seam finder (ms_dp_seams) costs beside ms_voronoi_seams, on one box, medians of 5, on the same inputs: config 2's rig (6 x 1080p, hfov 90,
the shipped cylindrical warper), its views warped
  seam001   at seam scale with seam_megapix 0.01 (the default, defs.h:52)
  seam01    at seam scale with seam_megapix 0.1
  compose   at compose scale (compose_megapix 1.4: the size ms_build_masks cuts Voronoi seams at)
            wall time of either call (synchronous: scratch allocation, the launches of every overlapping pair, one stream drain; host clock around the C call, the
            masks restored before every run) and the pairs' overlap sizes
  calibrate ms_calibrate_seam on a config 2 context with either finder (seam_megapix 0.01)
  kernels   with --kernel-stats FILE (the kernel statistics table a profiler run of `--only seam001,seam01,compose` wrote, CSV with Name / TotalDurationNs / Calls
            columns): the share of each k_dp_* launch in the time of all five
Appends one JSON line per row to profiles/dp_seams.jsonl (or --out).

  python tools/time_dp_seams.py [--out profiles/dp_seams.jsonl] [--only seam001,seam01,compose,calibrate] [--kernel-stats FILE --case seam001]
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))

import numpy as np
import torch

import msstitch as ms
import synth

CFG = synth.CONFIGS["cfg2"]
N, W, H = CFG["n"], CFG["w"], CFG["h"]
PROJ = ms.PROJ_CYLINDRICAL
SCALES = {"seam001": 0.01, "seam01": 0.1, "compose": None}


def frames():
    return [torch.from_numpy(synth.frame(W, H, i, 0)).cuda() for i in range(N)]


def warped(full, scale, Ks, R, warp_scale):
    """calibration.cpp:92-122 per view: resize, warpRoi, buildMaps, the image LINEAR / REFLECT, a 255 mask NEAREST / CONSTANT"""
    rois, imgs, masks = [], [], []
    for i in range(N):
        small = ms.resize_linear(full[i], fx=scale, fy=scale) if scale != 1.0 else full[i]
        hs, ws = small.shape[:2]
        roi = ms.warp_roi_lens(PROJ, Ks[i], R[i], None, warp_scale, ws, hs)
        mx, my = ms.build_warp_maps_lens(PROJ, roi[0], roi[1], roi[3], roi[2], Ks[i], R[i], None, warp_scale)
        rois.append(roi)
        imgs.append(ms.remap(small, mx, my, ms.INTER_LINEAR, ms.BORDER_REFLECT))
        masks.append(ms.remap(torch.full((hs, ws), 255, dtype=torch.uint8, device="cuda"), mx, my, ms.INTER_NEAREST, ms.BORDER_CONSTANT))
    return rois, imgs, masks


def overlaps(rois):
    out = []
    for i in range(N - 1):
        for j in range(i + 1, N):
            a, b = rois[i], rois[j]
            w = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
            h = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
            if w > 0 and h > 0:
                out.append([i, j, w, h])
    return out


def median_ms(call, restore, blocks=5):
    restore(); call()      # warm-up: code objects
    runs = []
    for _ in range(blocks):
        restore()
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        runs.append((time.perf_counter() - t) * 1e3)
    return statistics.median(runs), runs


def scale_row(name, full):
    if SCALES[name] is None:
        r = ms.calibrate_cameras(N, W, H, CFG["hfov_deg"], 0.6, 0.01, 1.4)
        rois, imgs, masks = warped(full, r["compose_scale"] if r["resize_input"] else 1.0, r["K_compose"], r["R"], r["compose_warp_scale"])
    else:
        r = ms.calibrate_cameras(N, W, H, CFG["hfov_deg"], 0.6, SCALES[name], 1.4)
        rois, imgs, masks = warped(full, r["seam_scale"], r["K_seam"], r["R"], r["seam_warp_scale"])
    work = [m.clone() for m in masks]

    def restore():
        for a, b in zip(work, masks):
            a.copy_(b)
    dp, dp_runs = median_ms(lambda: ms.dp_seams(rois, imgs, work), restore)
    vor, vor_runs = median_ms(lambda: ms.voronoi_seams(rois, work), restore)
    ov = overlaps(rois)
    return {"what": "dp_seams", "case": name, "views": N, "view_sizes": [[x[2], x[3]] for x in rois], "pairs": len(ov), "overlaps_i_j_w_h": ov,
            "dp_call_ms": dp, "dp_runs_ms": dp_runs, "voronoi_call_ms": vor, "voronoi_runs_ms": vor_runs, "dp_launches": 5 * len(ov), "voronoi_launches": 2 * len(ov)}


def calibrate_row(full):
    r = ms.calibrate_cameras(N, W, H, CFG["hfov_deg"], 0.6, 0.01, 1.4)
    small = ms.resize_linear_batch(full, fx=r["compose_scale"], fy=r["compose_scale"]) if r["resize_input"] else full
    row = {"what": "calibrate_seam", "views": N, "seam_megapix": 0.01, "seam_scale": r["seam_scale"]}
    for name, finder in (("voronoi", ms.SEAM_VORONOI), ("dp", ms.SEAM_DP)):
        comp = ms.Compositor(N, (small[0].shape[1], small[0].shape[0]), PROJ, r["compose_warp_scale"], num_bands=5, out_size=(0, 0))
        for i in range(N):
            comp.set_camera(i, r["K_compose"][i], r["R"][i])
        comp.build_maps()
        comp.set_seam_finder(finder)
        med, runs = median_ms(lambda: comp.calibrate_seam(full, np.stack(r["K_seam"]), r["seam_scale"], r["seam_warp_scale"]), lambda: None)
        row["%s_call_ms" % name], row["%s_runs_ms" % name] = med, runs
        comp.close()
    return row


def kernels_row(path, case):
    tot = {}
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            m = re.search(r"\bk_(dp|vor)_[a-z]+", rec["Name"])
            if m:
                tot[m.group(0)] = {"ns": int(float(rec["TotalDurationNs"])), "calls": int(rec["Calls"])}
    dp = sum(v["ns"] for k, v in tot.items() if k.startswith("k_dp_"))
    for k, v in tot.items():
        if k.startswith("k_dp_"):
            v["share_of_dp"] = v["ns"] / dp
    return {"what": "dp_seams_kernels", "case": case, "kernels": tot}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dp_seams.jsonl"))
    ap.add_argument("--only", default="seam001,seam01,compose,calibrate")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--case", default=None, help="with --kernel-stats: which case the profiled run timed")
    args = ap.parse_args()
    rows = []
    if args.kernel_stats:
        rows.append(kernels_row(args.kernel_stats, args.case))
    else:
        full = frames()
        rows = [calibrate_row(full) if name == "calibrate" else scale_row(name, full) for name in args.only.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
