#!/usr/bin/env python3
"""What the caller's own maps (ms_set_maps) cost per frame against the analytic maps: an analytic context and a context handed the analytic context's own maps, ROIs and
masks (so both composite the same pixels), same build, same process, alternating A / B, medians of 5 blocks (events on the stream):
  cfg2   config 2 (6 x 1080p -> 3840 x 1920, no CPW): the projection warp reads the dense maps instead of the 1-D projection tables
  cfg3   config 3 (config 2's geometry with CPW): the first CPW remap does
32-frame calls.  Per row: frames/s of both contexts and the time of the kernel that reads the maps (`k_warp`, with CPW `k_remap_gain`) from ms_stitch_timed.
Appends one JSON line per configuration to profiles/custom_maps.jsonl (or --out).

  python tools/time_custom_maps.py [--reps 10] [--out profiles/custom_maps.jsonl] [--only cfg2,cfg3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-stitcher_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch

import msstitch as ms
import synth


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps          # us per call


def ab(fa, fb, reps, blocks=5):
    for f in (fa, fb):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(timed(fa, reps)); tb.append(timed(fb, reps))
    return statistics.median(ta), statistics.median(tb), ta, tb


def contexts(cpw, nf):
    cfg = synth.CONFIGS["cfg2"]
    mk = lambda: ms.Compositor(cfg["n"], (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"], enable_cpw=cpw,
                               out_size=(cfg["out_w"], cfg["out_h"]), max_frames=nf)
    a, b = mk(), mk()
    for i, g in enumerate(synth.gains(cfg["n"])):
        a.set_camera(i, *synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i))
        a.set_gain(i, g); b.set_gain(i, g)
    a.build_maps(); a.build_masks(1); a.init_blender()
    b.set_maps([a.view_geom(i).roi.tuple() for i in range(cfg["n"])], [a.maps(i)[0] for i in range(cfg["n"])], [a.maps(i)[1] for i in range(cfg["n"])])
    for i in range(cfg["n"]):
        b.set_mask(i, a.mask(i).cpu().numpy())
    b.init_blender()
    if cpw:
        meshes = [synth.mesh(a.view_geom(i).roi.width, a.view_geom(i).roi.height, 12, 9, phase=0.3 * i, amp=6.0) for i in range(cfg["n"])]
        a.set_meshes(meshes); b.set_meshes(meshes)
    return a, b, cfg


def kernel_us(comp, frames, outs, name, reps=5):
    ts = []
    for _ in range(reps):
        ts.append(dict(comp.stitch_timed(frames, out8u=outs))[name] * 1000.0)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "custom_maps.jsonl"))
    ap.add_argument("--only", default="cfg2,cfg3")
    args = ap.parse_args()
    nf = 32
    rows = []
    for name in args.only.split(","):
        cpw = name == "cfg3"
        a, b, cfg = contexts(cpw, nf)
        views = [torch.from_numpy(synth.frame(cfg["w"], cfg["h"], i, 0)).cuda() for i in range(cfg["n"])]
        frames = [views for _ in range(nf)]
        oa = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(nf)]
        ob = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(nf)]
        fa, fb = a.prepared(frames, out8u=oa), b.prepared(frames, out8u=ob)
        fa(); fb(); torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(oa, ob)), "the custom-maps context differs from the analytic one"
        assert b.map_source() == ms.MAPS_CUSTOM and a.stitch_kernels() == b.stitch_kernels()
        ta, tb, la, lb = ab(fa, fb, args.reps)
        kname = "k_remap_gain" if cpw else "k_warp"
        ka, kla = kernel_us(a, frames, oa, kname)
        kb, klb = kernel_us(b, frames, ob, kname)
        rows.append({"what": "custom_maps", "config": name, "frames_per_call": nf, "kernels": list(b.stitch_kernels()),
                     "analytic_fps": nf / ta * 1e6, "custom_fps": nf / tb * 1e6, "analytic_us": ta, "custom_us": tb, "analytic_blocks_us": la, "custom_blocks_us": lb,
                     "map_kernel": kname, "analytic_map_kernel_us": ka, "custom_map_kernel_us": kb, "analytic_map_kernel_runs_us": kla, "custom_map_kernel_runs_us": klb,
                     "custom_over_analytic": tb / ta})
        a.close(); b.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r_ in rows:
            print(json.dumps(r_))
            f.write(json.dumps(r_) + "\n")


if __name__ == "__main__":
    main()
