#!/usr/bin/env python3
"""GPU time of the NV12 path against what it replaces, same build, same process, alternating A / B (events on the stream, medians of 5 blocks):
  resize   ms_nv12_resize_linear_batch            vs  ms_nv12_to_bgr_batch + ms_resize_linear_batch      (6 and 6 x 32 frames, 1080p -> the shipped compose size)
  track    ms_track_gains_nv12                    vs  ms_track_gains on BGR copies                       (config 2, stride 4 and 1)
  i420     ms_stitch_nv12_i420                    vs  ms_stitch_nv12(out8u) + ms_bgr_to_i420_batch       (config 2, 32-frame calls)
Appends one JSON line per comparison to profiles/nv12_path.jsonl (or --out).

  python tools/time_nv12_path.py [--reps 20] [--out profiles/nv12_path.jsonl] [--only resize,track,i420]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-stitcher_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np
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


def rig(name, max_frames):
    cfg = synth.CONFIGS[name]
    comp = ms.Compositor(cfg["n"], (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"],
                         out_size=(cfg["out_w"], cfg["out_h"]), max_frames=max_frames)
    for i, g in enumerate(synth.gains(cfg["n"])):
        comp.set_camera(i, *synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i))
        comp.set_gain(i, g)
    comp.build_maps(); comp.build_masks(1); comp.init_blender()
    return comp, cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nv12_path.jsonl"))
    ap.add_argument("--only", default="resize,track,i420")
    args = ap.parse_args()
    only = set(args.only.split(","))
    rows = []
    w, h = 1920, 1080
    nv6 = [torch.from_numpy(synth.nv12_frame(w, h, i)).cuda() for i in range(6)]
    if "resize" in only:
        r = ms.calibrate_cameras(6, w, h)
        cw, chh, sc = r["compose_width"], r["compose_height"], r["compose_scale"]
        for nf in (1, 32):
            srcs = [nv6[i % 6].clone() for i in range(6 * nf)]
            bgr = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in srcs]
            small_a = [torch.empty((chh, cw, 3), dtype=torch.uint8, device="cuda") for _ in srcs]
            small_b = [torch.empty((chh, cw, 3), dtype=torch.uint8, device="cuda") for _ in srcs]
            fused = ms.nv12_resize_linear_batch_prepared(srcs, small_a, sc, sc)
            cvt, rs = ms.nv12_to_bgr_batch_prepared(srcs, bgr), ms.resize_linear_batch_prepared(bgr, small_b, sc, sc)
            two = lambda: (cvt(), rs())
            fused(); two(); torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(small_a, small_b)), "fused resize differs from the two launches"
            ta, tb, la, lb = ab(fused, two, args.reps)
            n = len(srcs)
            bytes_fused = n * (w * h * 3 // 2 + cw * chh * 3)
            bytes_two = n * (w * h * 3 // 2 + 2 * w * h * 3 + cw * chh * 3)
            rows.append({"what": "resize", "images": n, "src": "%dx%d" % (w, h), "dst": "%dx%d" % (cw, chh), "fused_us": ta, "two_launch_us": tb, "fused_blocks_us": la,
                         "two_launch_blocks_us": lb, "fused_TBps": bytes_fused / ta / 1e6, "two_launch_TBps": bytes_two / tb / 1e6, "ratio_two_over_fused": tb / ta})
    if "track" in only or "i420" in only:
        comp, cfg = rig("cfg2", 32)
        bgr6 = ms.nv12_to_bgr_batch(nv6)
        if "track" in only:
            for stride in (4, 1):
                ta, tb, la, lb = ab(lambda: comp.track_gains_nv12(nv6, stride=stride, smoothing=0.25), lambda: comp.track_gains(bgr6, stride=stride, smoothing=0.25), args.reps)
                rows.append({"what": "track", "config": "cfg2", "stride": stride, "nv12_us": ta, "bgr_us": tb, "nv12_blocks_us": la, "bgr_blocks_us": lb})
        if "i420" in only:
            nf = 32
            frames = [nv6 for _ in range(nf)]
            outs, outs2 = comp.new_i420(nf), comp.new_i420(nf)
            canv = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(nf)]
            y0, rows_ = comp.i420_rows()
            one = comp.prepared_nv12_i420(frames, outs)
            st = comp.prepared_nv12(frames, out8u=canv)
            cv = ms.bgr_to_i420_batch_prepared([c[y0:y0 + rows_] for c in canv], outs2)
            two = lambda: (st(), cv())
            one(); two(); torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(outs, outs2)), "stitch_nv12_i420 differs from stitch_nv12 + bgr_to_i420_batch"
            reps = max(3, args.reps // 4)
            ta, tb, la, lb = ab(one, two, reps)
            rows.append({"what": "i420", "config": "cfg2", "frames_per_call": nf, "nv12_i420_us": ta, "nv12_then_i420_us": tb, "nv12_i420_fps": nf / ta * 1e6,
                         "nv12_then_i420_fps": nf / tb * 1e6, "nv12_i420_blocks_us": la, "nv12_then_i420_blocks_us": lb})
            # frames/s with one track call after every 8th 32-frame stitch_nv12 call
            st16 = comp.prepared_nv12(frames, out8u=canv)

            def eight(track):
                def run():
                    for _ in range(8):
                        st16()
                    if track == "nv12":
                        comp.track_gains_nv12(nv6, stride=4, smoothing=0.25)
                    elif track == "bgr":
                        comp.track_gains(bgr6, stride=4, smoothing=0.25)
                return run
            ta, tb, _, _ = ab(eight("nv12"), eight("bgr"), 2)
            tc, _, _, _ = ab(eight(None), eight(None), 2)
            rows.append({"what": "track_every_8th_call", "config": "cfg2", "frames_per_call": nf, "fps_track_nv12": 8 * nf / ta * 1e6, "fps_track_bgr": 8 * nf / tb * 1e6,
                         "fps_no_tracking": 8 * nf / tc * 1e6})
        comp.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r_ in rows:
            print(json.dumps(r_))
            f.write(json.dumps(r_) + "\n")


if __name__ == "__main__":
    main()
