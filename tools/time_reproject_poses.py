#!/usr/bin/env python3
"""What a moving virtual camera costs (ms_reproject_poses), on one box, medians of 5, events on the stream, 32-frame calls on 3840 x 1920 canvases under an orbit
of poses (the rig rotation Ry(7 f degrees) in frame f), outputs compared equal first, the routes alternating.
  viewport / cube_bgr / cube_i420 / fisheye
              ms_reproject_poses -- ONE launch, no maps -- against the route it replaces in the same build: per frame one ms_build_view_maps per view and one
              one-frame ms_reproject (64 launches for a viewport, 224 for a cube map; one pair of map images per view, reused frame after frame; descriptors
              marshalled once), plus one ms_bgr_to_i420_batch for I420; and against ms_reproject on FIXED maps over the same frames, one launch: what motion
              costs over standing still.  A 1920 x 1080 viewport of 90 degrees, six 960 x 960 cube faces as BGR and as I420, a 1920 x 1080 fisheye viewport
              (which prices the reuse of the view rays across a frame group).
  resources   no device: VGPRs, waves per SIMD, LDS and scratch of the unit's kernels from the compiler's resource report
Appends one JSON line per row to profiles/reproject_poses.jsonl (or --out).  --label tags the rows (the frame-group pricing runs builds of other group sizes
through MSSTITCH_LIB).

  python tools/time_reproject_poses.py [--reps 5] [--out profiles/reproject_poses.jsonl] [--only viewport,cube_bgr,cube_i420,fisheye] [--label G8]
  python tools/time_reproject_poses.py --only resources
"""
import argparse
import ctypes as C
import json
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))

NF = 32
CW, CH = 3840, 1920
ORBIT_DEG = 7.0
SHAPES = {
    "viewport": ("viewport", 1920, 1080, False, None),
    "cube_bgr": ("cube", 960, 960, False, None),
    "cube_i420": ("cube", 960, 960, True, None),
    "fisheye": ("viewport", 1920, 1080, False, (-0.02, 0.003, 0.0, 0.0)),
}


def event_us(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def canvases():
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    return [torch.randint(0, 256, (CH, CW, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(NF)]


def orbit():
    import numpy as np
    out = []
    for f in range(NF):
        a = f * ORBIT_DEG * (math.pi / 180.0)
        out.append([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    return np.array(out, np.float64)


def two_call_route(ms, pf, cv, dsts, views, rects, table, fmt):
    """per frame: ms_build_view_maps of every view under that frame's rotation, then a one-frame ms_reproject of all views; descriptors marshalled once"""
    import torch
    lib = ms.load()
    maps = [(torch.zeros((v.height, v.width), dtype=torch.float32, device="cuda"), torch.zeros((v.height, v.width), dtype=torch.float32, device="cuda")) for v in views]
    mimg = [(ms.img(mx), ms.img(my)) for mx, my in maps]
    jt = (ms.ViewJob * len(views))(*[ms.ViewJob(ix, iy, x, y) for (ix, iy), (x, y) in zip(mimg, rects)])
    per_frame = []
    for f in range(NF):
        vs = []
        for j, v in enumerate(views):
            w = ms.View.from_buffer_copy(v)
            w.R[:] = [float(t) for t in table[j, f]]
            vs.append(w)
        per_frame.append((vs, (ms.Image * 1)(ms.img(cv[f])), (ms.Image * 1)(ms.img(dsts[f]))))
    build, reproject, chk = lib.ms_build_view_maps, lib.ms_reproject, ms._chk
    pfr = C.byref(pf)

    def run():
        s = ms._stream()
        for vs, a, b in per_frame:
            for w, (ix, iy) in zip(vs, mimg):
                chk(build(pfr, C.byref(w), C.byref(ix), C.byref(iy), s))
            chk(reproject(a, b, 1, jt, len(views), pf.wrap_cols, pf.clamp_rows, fmt, s))
    run.keep = (maps, per_frame, jt)
    return run


def shape_row(name, cv, reps, label, blocks=5):
    import torch
    import msstitch as ms
    import synth
    kind, w, h, i420, fish = SHAPES[name]
    pf = ms.PanoFrame.make(ms.PROJ_SPHERICAL, synth.warp_scale(CW), -CW // 2, 0, CW, 1)
    if kind == "cube":
        views, (aw, ah), rects = [ms.cube_face_view(f, w) for f in range(6)], (3 * w, 2 * h), [((f % 3) * w, (f // 3) * h) for f in range(6)]
    else:
        v = ms.look_at_view(30, 10, 0, 90, w, h)
        if fish is not None:
            v.lens = ms.Lens.fisheye(*fish, max_theta_deg=100.0)
        views, (aw, ah), rects = [v], (w, h), [(0, 0)]
    jobs = [(v, x, y) for v, (x, y) in zip(views, rects)]
    table = ms.view_pose_table(jobs, orbit())
    poses = torch.from_numpy(table.reshape(-1)).cuda()
    shape = (ah * 3 // 2, aw) if i420 else (ah, aw, 3)
    new = lambda s: [torch.zeros(s, dtype=torch.uint8, device="cuda") for _ in range(NF)]
    out_p, out_r, out_s = new(shape), new(shape), new(shape)
    fmt = ms.VIEW_I420 if i420 else ms.VIEW_BGR
    moving = ms.reproject_poses_prepared(pf, cv, out_p, jobs, poses, fmt)
    if i420:       # the comparator of the issue: BGR atlases through the two calls, then ms_bgr_to_i420_batch
        bgr = new((ah, aw, 3))
        two, cvt = two_call_route(ms, pf, cv, bgr, views, rects, table, ms.VIEW_BGR), ms.bgr_to_i420_batch_prepared(bgr, out_r)
        route = lambda: (two(), cvt())
    else:
        route = two_call_route(ms, pf, cv, out_r, views, rects, table, fmt)
    fixed_maps = [(*ms.build_view_maps(pf, v), x, y) for v, x, y in jobs]
    still = ms.reproject_prepared(cv, out_s, fixed_maps, CW, 1, fmt)
    moving(); route(); still()
    torch.cuda.synchronize()
    for f in range(NF):
        assert torch.equal(out_p[f], out_r[f]), "ms_reproject_poses differs from the two-call route in frame %d" % f
    tm, tr, ts = [], [], []
    for _ in range(blocks):
        tm.append(event_us(moving, reps)); tr.append(event_us(route, reps)); ts.append(event_us(still, reps))
    mm, mr, mst = statistics.median(tm), statistics.median(tr), statistics.median(ts)
    return {"what": "reproject_poses", "label": label, "shape": name, "format": "i420" if i420 else "bgr", "lens": "fisheye" if fish else "none", "frames_per_call": NF,
            "views": len(views), "atlas": "%dx%d" % (aw, ah), "orbit_deg": ORBIT_DEG, "outputs_equal": True, "route_launches": NF * (len(views) + 1) + (1 if i420 else 0),
            "poses_us": mm, "route_us": mr, "fixed_maps_us": mst, "poses_over_route": mm / mr, "poses_over_fixed_maps": mm / mst,
            "poses_blocks_us": tm, "route_blocks_us": tr, "fixed_maps_blocks_us": ts}


def resources_row():
    """the compiler's resource report of csrc/reproject_poses.hip, with build.sh's flags"""
    flags = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fvisibility=hidden".split()
    src = os.path.join(ROOT, "video-stitcher_amd", "csrc", "reproject_poses.hip")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, check=True)
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s*(\S+)\s*\[-Rpass", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None and key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "TotalSGPRs"):
            cur[key] = int(val)
    return {"what": "kernel_resources", "source": "hipcc -Rpass-analysis=kernel-resource-usage", "kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_poses.jsonl"))
    ap.add_argument("--only", default="viewport,cube_bgr,cube_i420,fisheye")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    names = args.only.split(",")
    rows = []
    if names == ["resources"]:
        rows.append(resources_row())
    else:
        import torch
        cv = canvases()
        for name in names:
            if name not in SHAPES:
                raise SystemExit("unknown row %s" % name)
            rows.append(shape_row(name, cv, args.reps, args.label))
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
