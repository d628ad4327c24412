#!/usr/bin/env python3
"""What the virtual cameras (ms_build_view_maps, ms_reproject) cost, on one box, medians of 5, events on the stream, 32-frame calls, outputs compared equal first,
alternating with the only route the library offered before: the canvas padded by hand (one column either side, one row above and below), one ms_remap per view per
frame into the atlas, and ms_bgr_to_i420_batch for the I420 form.
  cube_bgr / cube_i420   six 960 x 960 faces of the 3840 x 1920 canvas into a 2880 x 1920 atlas
  viewport               one 1920 x 1080 viewport of 90 degrees
  maps                   ms_build_view_maps for both shapes: the cost of moving a viewport
  stitch                 a 32-frame ms_stitch (config 2) followed by the cube-map call, against ms_stitch alone
Each row carries the bytes the algorithm needs, from the shapes: 3 B out per pixel and frame, 8 B of maps per pixel and frame group, and the source footprint of the
views (the distinct source pixels their taps touch) per frame.  Appends one JSON line per row to profiles/reproject.jsonl (or --out).

  python tools/time_reproject.py [--reps 5] [--out profiles/reproject.jsonl] [--only cube_bgr,cube_i420,viewport,maps,stitch]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_reproject.py --once 5      # every batched call 5 times, in a fixed order
  python tools/time_reproject.py --trace-dir DIR                                                             # that trace's kernel times, as a share of 8 TB/s, into a row
"""
import argparse
import csv
import ctypes as C
import glob
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))

import torch

import msstitch as ms
import synth

NF = 32
CW, CH = 3840, 1920
PEAK = 8e12      # bytes / s


def event_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def canvas_frame():
    return ms.PanoFrame.make(ms.PROJ_SPHERICAL, synth.warp_scale(CW), -CW // 2, 0, CW, 1)


def shapes(which):
    """(views, atlas size, rectangles)"""
    if which == "viewport":
        return [ms.look_at_view(30, 10, 0, 90, 1920, 1080)], (1920, 1080), [(0, 0)]
    return [ms.cube_face_view(f, 960) for f in range(6)], (2880, 1920), [((f % 3) * 960, (f // 3) * 960) for f in range(6)]


def footprint_bytes(jobs):
    """3 B per distinct source pixel the four taps of the views touch (wrapping at the seam, repeating the pole rows)"""
    seen = torch.zeros(CW * CH, dtype=torch.bool, device="cuda")
    for mx, my, _, _ in jobs:
        x1, y1 = torch.floor(mx).long(), torch.floor(my).long()
        for dx in (0, 1):
            for dy in (0, 1):
                seen[((y1 + dy).clamp(0, CH - 1) * CW + (x1 + dx) % CW).reshape(-1)] = True
    return 3 * int(seen.sum().item())


def algorithmic_bytes(jobs, nf):
    px = sum(mx.numel() for mx, _, _, _ in jobs)
    return {"out": 3 * px * nf, "maps": 8 * px * math.ceil(nf / ms.VIEW_FRAME_GROUP), "source": footprint_bytes(jobs) * nf}


def loop_route(canvases, atlases, jobs, pad=True):
    """the route without ms_reproject: pad the canvas by hand, one ms_remap per view per frame (descriptors marshalled once, no allocation in the loop)"""
    padded = [torch.zeros((CH + 2, CW + 2, 3), dtype=torch.uint8, device="cuda") for _ in canvases]
    shifted = [(mx + 1.0, my + 1.0) for mx, my, _, _ in jobs]
    calls = []
    for p, a in zip(padded, atlases):
        for (mx, my, x, y), (sx, sy) in zip(jobs, shifted):
            dst = a[y:y + mx.shape[0], x:x + mx.shape[1]]
            calls.append((ms.img(p), ms.img(sx), ms.img(sy), ms.img(dst)))
    fn = ms.load().ms_remap

    def do_pad():
        for c, p in zip(canvases, padded):
            p[1:-1, 1:-1] = c
            p[1:-1, 0] = c[:, -1]; p[1:-1, -1] = c[:, 0]
            p[0] = p[1]; p[-1] = p[-2]

    def run(with_pad=pad):
        if with_pad:
            do_pad()
        st = ms._stream()
        for s, xm, ym, d in calls:
            ms._chk(fn(C.byref(s), C.byref(xm), C.byref(ym), C.byref(d), ms.INTER_LINEAR, ms.BORDER_CONSTANT, st))
    run.keep = (padded, shifted, calls)
    return run


def setup(which, i420):
    views, (aw, ah), rects = shapes(which)
    pf = canvas_frame()
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    canvases = [torch.randint(0, 256, (CH, CW, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(NF)]
    jobs = [ms.build_view_maps(pf, v) + r for v, r in zip(views, rects)]
    atl_a = [torch.zeros((ah, aw, 3), dtype=torch.uint8, device="cuda") for _ in range(NF)]      # the loop's BGR atlases
    if i420:
        out_a = [torch.zeros((ah * 3 // 2, aw), dtype=torch.uint8, device="cuda") for _ in range(NF)]
        out_b = [torch.zeros((ah * 3 // 2, aw), dtype=torch.uint8, device="cuda") for _ in range(NF)]
        batched = ms.reproject_prepared(canvases, out_b, jobs, CW, 1, ms.VIEW_I420)
        remaps, to_i420 = loop_route(canvases, atl_a, jobs), ms.bgr_to_i420_batch_prepared(atl_a, out_a)

        def loop(with_pad=True):
            remaps(with_pad); to_i420()
    else:
        out_a = atl_a
        out_b = [torch.zeros((ah, aw, 3), dtype=torch.uint8, device="cuda") for _ in range(NF)]
        batched = ms.reproject_prepared(canvases, out_b, jobs, CW, 1, ms.VIEW_BGR)
        loop = loop_route(canvases, atl_a, jobs)
    return dict(jobs=jobs, batched=batched, loop=loop, out_a=out_a, out_b=out_b, atlas=(aw, ah), n_views=len(views))


def sampler_row(which, i420, reps, blocks=5):
    s = setup(which, i420)
    s["loop"](); s["batched"]()
    torch.cuda.synchronize()
    for a, b in zip(s["out_a"], s["out_b"]):
        assert torch.equal(a, b), "the batched call and the loop differ"
    tl, tn, tb = [], [], []
    for _ in range(blocks):
        tl.append(event_us(s["loop"], reps)); tb.append(event_us(s["batched"], reps)); tn.append(event_us(lambda: s["loop"](False), reps))
    by = algorithmic_bytes(s["jobs"], NF)
    mb = statistics.median(tb)
    return {"what": "reproject", "shape": which, "format": "i420" if i420 else "bgr", "frames_per_call": NF, "views": s["n_views"], "atlas": "%dx%d" % s["atlas"],
            "outputs_equal": True, "batched_us": mb, "loop_us": statistics.median(tl), "loop_without_padding_us": statistics.median(tn),
            "loop_over_batched": statistics.median(tl) / mb, "batched_blocks_us": tb, "loop_blocks_us": tl, "loop_without_padding_blocks_us": tn,
            "launches_batched": 1, "launches_loop": NF * s["n_views"] + (1 if i420 else 0), "algorithmic_bytes": by,
            "algorithmic_share_of_8TBps_call": sum(by.values()) / (mb * 1e-6) / PEAK}


def maps_row(blocks=5):
    pf = canvas_frame()
    row = {"what": "build_view_maps"}
    for which in ("cube", "viewport"):
        views = shapes(which)[0]
        outs = [(torch.empty((v.height, v.width), dtype=torch.float32, device="cuda"), torch.empty((v.height, v.width), dtype=torch.float32, device="cuda")) for v in views]

        def run():
            for v, o in zip(views, outs):
                ms.build_view_maps(pf, v, out=o)
        run()
        t = [event_us(run, 1) for _ in range(blocks)]
        row[which + "_us"] = statistics.median(t); row[which + "_runs_us"] = t; row[which + "_pixels"] = sum(v.width * v.height for v in views)
    return row


def stitch_row(reps, blocks=5):
    cfg = synth.CONFIGS["cfg2"]
    comp = ms.Compositor(cfg["n"], (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"],
                         out_size=(cfg["out_w"], cfg["out_h"]), max_frames=NF)
    for i, g in enumerate(synth.gains(cfg["n"])):
        comp.set_camera(i, *synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i))
        comp.set_gain(i, g)
    comp.build_maps(); comp.build_masks(1); comp.init_blender()
    views = [torch.from_numpy(synth.frame(cfg["w"], cfg["h"], i, 0)).cuda() for i in range(cfg["n"])]
    frames = [views for _ in range(NF)]
    canvases = [torch.zeros((CH, CW, 3), dtype=torch.uint8, device="cuda") for _ in range(NF)]
    stitch = comp.prepared(frames, out8u=canvases)
    pf = comp.pano_frame()
    vs, (aw, ah), rects = shapes("cube")
    jobs = [ms.build_view_maps(pf, v) + r for v, r in zip(vs, rects)]
    atlases = [torch.zeros((ah, aw, 3), dtype=torch.uint8, device="cuda") for _ in range(NF)]
    cube = ms.reproject_prepared(canvases, atlases, jobs, pf.wrap_cols, pf.clamp_rows)

    def both():
        stitch(); cube()
    for _ in range(3):
        both()
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(event_us(stitch, reps)); tb.append(event_us(both, reps))
    comp.close()
    ma, mb = statistics.median(ta), statistics.median(tb)
    return {"what": "stitch_then_cube", "config": "cfg2", "frames_per_call": NF, "stitch_us": ma, "stitch_then_cube_us": mb, "stitch_fps": NF / ma * 1e6,
            "stitch_then_cube_fps": NF / mb * 1e6, "stitch_blocks_us": ta, "stitch_then_cube_blocks_us": tb}


ONCE_ORDER = [("cube", False), ("cube", True), ("viewport", False)]


def once(n):
    """every batched call n times after a warm-up, in ONCE_ORDER, then the maps of both shapes n times: what --trace-dir expects to find in a kernel trace"""
    plan = {}
    for which, i420 in ONCE_ORDER:
        s = setup(which, i420)
        for _ in range(n + 1):
            s["batched"]()
        torch.cuda.synchronize()
        plan["%s_%s" % (which, "i420" if i420 else "bgr")] = algorithmic_bytes(s["jobs"], NF)
        del s
        torch.cuda.empty_cache()
    pf = canvas_frame()
    for which in ("cube", "viewport"):
        for _ in range(n):
            for v in shapes(which)[0]:
                ms.build_view_maps(pf, v)
    torch.cuda.synchronize()
    print(json.dumps({"what": "once_plan", "n": n, "bytes": plan}))


def trace_row(trace_dir, n):
    """the kernel times of a `--once n` run under rocprofv3 --kernel-trace: per shape the median launch, and the algorithm's bytes over it as a share of 8 TB/s"""
    rp, vm = [], []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            t = (int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
            if "k_reproject" in r["Kernel_Name"]:
                rp.append(t)
            elif "k_view_maps" in r["Kernel_Name"]:
                vm.append(t)
    rp.sort(); vm.sort()
    assert len(rp) == len(ONCE_ORDER) * (n + 1), "expected %d k_reproject launches in the trace, found %d" % (len(ONCE_ORDER) * (n + 1), len(rp))
    row = {"what": "kernel_trace", "source": "rocprofv3 --kernel-trace --stats, a run of its own", "frames_per_call": NF}
    # per shape: setup() builds the maps (6 or 1 k_view_maps), then n + 1 batched calls; the warm-up launch is dropped
    k = 0
    for which, i420 in ONCE_ORDER:
        runs = [us for _, us in rp[k + 1:k + n + 1]]
        k += n + 1
        name = "%s_%s" % (which, "i420" if i420 else "bgr")
        vs, _, rects = shapes(which)
        by = algorithmic_bytes([ms.build_view_maps(canvas_frame(), v) + r for v, r in zip(vs, rects)], NF)
        row[name + "_kernel_us"] = statistics.median(runs)
        row[name + "_algorithmic_bytes"] = by
        row[name + "_share_of_8TBps"] = sum(by.values()) / (statistics.median(runs) * 1e-6) / PEAK
    views = {"cube": 6, "viewport": 1}
    k = sum(views[w] for w, _ in ONCE_ORDER)      # the maps setup() built
    for which in ("cube", "viewport"):
        per_run = [sum(us for _, us in vm[k + i * views[which]:k + (i + 1) * views[which]]) for i in range(n)]
        k += n * views[which]
        row["maps_%s_kernel_us" % which] = statistics.median(per_run)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject.jsonl"))
    ap.add_argument("--only", default="cube_bgr,cube_i420,viewport,maps,stitch")
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--trace-n", type=int, default=5)
    args = ap.parse_args()
    if args.once:
        once(args.once)
        return
    rows = []
    if args.trace_dir:
        rows.append(trace_row(args.trace_dir, args.trace_n))
    else:
        for name in args.only.split(","):
            if name == "cube_bgr": rows.append(sampler_row("cube", False, args.reps))
            elif name == "cube_i420": rows.append(sampler_row("cube", True, args.reps))
            elif name == "viewport": rows.append(sampler_row("viewport", False, args.reps))
            elif name == "maps": rows.append(maps_row())
            elif name == "stitch": rows.append(stitch_row(args.reps))
            else: raise SystemExit("unknown row %s" % name)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
