#!/usr/bin/env python3
"""What the lens model (ms_set_lens) costs, on one box, medians of 5:
  build     wall time of ms_build_maps (a synchronous calibration-time call: host clock around it) with BROWN on every view against the analytic call, on config 2
            and on config 5's geometry (12 x 4K -> 7680 x 3840), alternating; and its two parts through the per-op entry points, summed over the views:
            the bounding-box scan (ms_warp_roi_lens, synchronous: host clock) and the map kernel (ms_build_warp_maps_lens: events on the stream)
  frame     config 2, 32-frame calls: the lens context against the analytic one, alternating (events), and the kernel that reads the maps (`k_warp`, ms_stitch_timed).
            BROWN's barrel distortion widens what a view sees, so its views warp to more pixels than the pinhole's (`level0_pixels`): the call does more work
  frame0    the same with all-zero coefficients: the analytic context's geometry to within a pixel per ROI edge, i.e. the dense route alone against the projection tables
Appends one JSON line per row to profiles/lens_maps.jsonl (or --out).

  python tools/time_lens_maps.py [--reps 10] [--out profiles/lens_maps.jsonl] [--only cfg2,cfg5,frame,frame0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))

import torch

import msstitch as ms
import synth

BROWN = (-0.18, 0.03, 1e-3, -5e-4)
MAX_THETA = 75.0


def context(cfg, lens, nf=1):
    comp = ms.Compositor(cfg["n"], (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"],
                         out_size=(cfg["out_w"], cfg["out_h"]), max_frames=nf)
    for i, g in enumerate(synth.gains(cfg["n"])):
        comp.set_camera(i, *synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i))
        comp.set_gain(i, g)
        if lens is not None:
            comp.set_lens(i, lens)
    return comp


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def build_row(name, blocks=5):
    cfg = synth.CONFIGS[name]
    lens = ms.Lens.brown(*BROWN, max_theta_deg=MAX_THETA)
    a, b = context(cfg, None), context(cfg, lens)
    a.build_maps(); b.build_maps()      # warm-up: code objects, allocations
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(wall_ms(a.build_maps)); tb.append(wall_ms(b.build_maps))
    assert a.map_source() == ms.MAPS_ANALYTIC and b.map_source() == ms.MAPS_LENS
    scale = synth.warp_scale(cfg["out_w"])
    cams = [synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i) for i in range(cfg["n"])]
    rois = [b.view_geom(i).roi.tuple() for i in range(cfg["n"])]
    outs = [(torch.empty((r[3], r[2]), dtype=torch.float32, device="cuda"), torch.empty((r[3], r[2]), dtype=torch.float32, device="cuda")) for r in rois]

    def scan():
        for K, R in cams:
            ms.warp_roi_lens(ms.PROJ_SPHERICAL, K, R, lens, scale, cfg["w"], cfg["h"])

    def maps():
        for (K, R), r, o in zip(cams, rois, outs):
            ms.build_warp_maps_lens(ms.PROJ_SPHERICAL, r[0], r[1], r[3], r[2], K, R, lens, scale, out=o)
    scan(); maps()
    ts = [wall_ms(scan) for _ in range(blocks)]
    tm = [event_ms(maps) for _ in range(blocks)]
    u = int(round(3.141592653589793 * scale))
    row = {"what": "lens_build_maps", "config": name, "views": cfg["n"], "candidates_per_view": 2 * u * u, "map_pixels": sum(r[2] * r[3] for r in rois),
           "analytic_build_maps_ms": statistics.median(ta), "lens_build_maps_ms": statistics.median(tb), "analytic_runs_ms": ta, "lens_runs_ms": tb,
           "bbox_scan_all_views_ms": statistics.median(ts), "bbox_scan_runs_ms": ts, "map_kernel_all_views_ms": statistics.median(tm), "map_kernel_runs_ms": tm}
    a.close(); b.close()
    return row


def frame_row(reps, zero, blocks=5):
    nf = 32
    cfg = synth.CONFIGS["cfg2"]
    lens = ms.Lens.brown() if zero else ms.Lens.brown(*BROWN, max_theta_deg=MAX_THETA)
    a, b = context(cfg, None, nf), context(cfg, lens, nf)
    for c in (a, b):
        c.build_maps(); c.build_masks(1); c.init_blender()
    views = [torch.from_numpy(synth.frame(cfg["w"], cfg["h"], i, 0)).cuda() for i in range(cfg["n"])]
    frames = [views for _ in range(nf)]
    oa = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(nf)]
    ob = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(nf)]
    fa, fb = a.prepared(frames, out8u=oa), b.prepared(frames, out8u=ob)
    for f in (fa, fb):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    assert b.map_source() == ms.MAPS_LENS and "simple" not in b.stitch_kernels()

    def timed(fn):
        return event_ms(lambda: [fn() for _ in range(reps)]) * 1000.0 / reps      # us per call
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(timed(fa)); tb.append(timed(fb))
    ka = [dict(a.stitch_timed(frames, out8u=oa))["k_warp"] * 1000.0 for _ in range(5)]
    kb = [dict(b.stitch_timed(frames, out8u=ob))["k_warp"] * 1000.0 for _ in range(5)]
    ma, mb = statistics.median(ta), statistics.median(tb)
    row = {"what": "lens_per_frame", "config": "cfg2", "lens": "BROWN, all coefficients 0" if zero else "BROWN %s, max_theta %g" % (BROWN, MAX_THETA), "frames_per_call": nf, "kernels": list(b.stitch_kernels()), "analytic_kernels": list(a.stitch_kernels()),
           "analytic_fps": nf / ma * 1e6, "lens_fps": nf / mb * 1e6, "analytic_us": ma, "lens_us": mb, "analytic_blocks_us": ta, "lens_blocks_us": tb,
           "analytic_k_warp_us": statistics.median(ka), "lens_k_warp_us": statistics.median(kb), "lens_over_analytic": mb / ma,
           "level0_pixels": [sum(c.view_geom(i).roi.width * c.view_geom(i).roi.height for i in range(cfg["n"])) for c in (a, b)]}
    a.close(); b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_maps.jsonl"))
    ap.add_argument("--only", default="cfg2,cfg5,frame,frame0")
    args = ap.parse_args()
    rows = [frame_row(args.reps, name == "frame0") if name.startswith("frame") else build_row(name) for name in args.only.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
