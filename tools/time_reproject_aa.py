#!/usr/bin/env python3
"""What the antialiased virtual cameras (ms_build_pano_mips, ms_reproject_aa) cost, on one box, medians of 5, events on the stream, 32-frame calls on 3840 x 1920
canvases, outputs compared equal to the numpy statement (tests/reproject_aa_ref.py) first, alternating with the comparator.
  mips        ms_build_pano_mips, levels 4, against ms_calib_copy (the tuned device copy) of the same number of bytes read plus written; TB/s of both
  viewport_small / cube_bgr / cube_i420 / viewport_full
              ms_reproject_aa (levels 4, the mips built before) against ms_reproject on the same maps: a 480 x 270 viewport of 90 degrees, six 480 x 480 cube
              faces as BGR and as I420, a 1920 x 1080 viewport of 90 degrees (footprint about 1: the one-level path)
  resources   no device: VGPRs, waves per SIMD, LDS and scratch of the unit's kernels from the compiler's resource report
Appends one JSON line per row to profiles/reproject_aa.jsonl (or --out).

  python tools/time_reproject_aa.py [--reps 5] [--out profiles/reproject_aa.jsonl] [--only mips,viewport_small,cube_bgr,cube_i420,viewport_full]
  python tools/time_reproject_aa.py --only resources
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NF = 32
CW, CH = 3840, 1920
LEVELS = 4
SHAPES = {
    "viewport_small": ("viewport", 480, 270, False),
    "cube_bgr": ("cube", 480, 480, False),
    "cube_i420": ("cube", 480, 480, True),
    "viewport_full": ("viewport", 1920, 1080, False),
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


def mips_row(cv, reps, blocks=5):
    import numpy as np
    import torch
    import msstitch as ms
    import reproject_aa_ref as AA
    lv, nbytes = ms.pano_mips_layout(CW, CH, LEVELS)
    mips = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(NF)]
    ms.build_pano_mips(cv, LEVELS, out=mips)
    torch.cuda.synchronize()
    for f in (0, NF - 1):      # the first and the last frame against the reference, level by level
        chain = AA.mip_chain(cv[f].cpu().numpy(), LEVELS)
        for l, img in zip(lv, chain[1:]):
            assert np.array_equal(ms.mip_level_view(mips[f], l).cpu().numpy(), img), "level differs from the reference"
    read = NF * CW * CH * 3 + (NF * lv[2].cols * lv[2].rows * 3 if LEVELS > 3 else 0)
    written = NF * sum(l.cols * l.rows * 3 for l in lv)
    half = (read + written) // 2 // 256 * 256
    a, b = torch.zeros(half, dtype=torch.uint8, device="cuda"), torch.zeros(half, dtype=torch.uint8, device="cuda")
    build = lambda: ms.build_pano_mips(cv, LEVELS, out=mips)
    copy = lambda: ms.calib_copy(a, b)
    build(); copy()
    tb, tc = [], []
    for _ in range(blocks):
        tb.append(event_us(build, reps)); tc.append(event_us(copy, reps))
    mb, mc = statistics.median(tb), statistics.median(tc)
    return mips, {"what": "build_pano_mips", "frames_per_call": NF, "canvas": "%dx%d" % (CW, CH), "levels": LEVELS, "launches": (LEVELS + 2) // 3, "outputs_equal": True,
                  "bytes_read": read, "bytes_written": written, "mips_us": mb, "mips_TBps": (read + written) / (mb * 1e-6) / 1e12, "copy_bytes_each_way": half,
                  "copy_us": mc, "copy_TBps": 2 * half / (mc * 1e-6) / 1e12, "mips_over_copy": mb / mc, "mips_blocks_us": tb, "copy_blocks_us": tc}


def sampler_row(name, cv, mips, reps, blocks=5, check_stride=7):
    import numpy as np
    import torch
    import msstitch as ms
    import np_ref
    import reproject_aa_ref as AA
    import synth
    kind, w, h, i420 = SHAPES[name]
    pf = ms.PanoFrame.make(ms.PROJ_SPHERICAL, synth.warp_scale(CW), -CW // 2, 0, CW, 1)
    if kind == "cube":
        views, (aw, ah), rects = [ms.cube_face_view(f, w) for f in range(6)], (3 * w, 2 * h), [((f % 3) * w, (f // 3) * h) for f in range(6)]
    else:
        views, (aw, ah), rects = [ms.look_at_view(30, 10, 0, 90, w, h)], (w, h), [(0, 0)]
    jobs, jobs_aa, span = [], [], [float("inf"), 0.0]
    for v, (x, y) in zip(views, rects):
        mx, my = ms.build_view_maps(pf, v)
        rho = ms.build_view_footprint(pf, mx, my)
        span = [min(span[0], float(rho.min())), max(span[1], float(rho.max()))]
        jobs.append((mx, my, x, y)); jobs_aa.append((mx, my, rho, x, y))
    shape = (ah * 3 // 2, aw) if i420 else (ah, aw, 3)
    out_p = [torch.zeros(shape, dtype=torch.uint8, device="cuda") for _ in range(NF)]
    out_a = [torch.zeros(shape, dtype=torch.uint8, device="cuda") for _ in range(NF)]
    fmt = ms.VIEW_I420 if i420 else ms.VIEW_BGR
    plain = ms.reproject_prepared(cv, out_p, jobs, CW, 1, fmt)
    aa = ms.reproject_aa_prepared(cv, mips, LEVELS, out_a, jobs_aa, CW, 1, fmt)
    plain(); aa()
    torch.cuda.synchronize()
    # every check_stride-th pixel of frame 0 (the BGR form: I420 is checked through the BGR call on the same jobs) against the reference
    bgr = out_a[0]
    if i420:
        bgr = torch.zeros((ah, aw, 3), dtype=torch.uint8, device="cuda")
        ms.reproject_aa(cv[:1], mips[:1], LEVELS, [bgr], jobs_aa, CW, 1)
        assert np.array_equal(np_ref.bgr_to_i420(bgr.cpu().numpy()), out_a[0].cpu().numpy()), "I420 differs from ms_bgr_to_i420 of the BGR atlas"
    chain = AA.mip_chain(cv[0].cpu().numpy(), LEVELS)
    got = bgr.cpu().numpy()
    k = check_stride
    for mx, my, rho, x, y in jobs_aa:
        ref = AA.reproject_aa_view(chain, mx.cpu().numpy()[::k, ::k], my.cpu().numpy()[::k, ::k], rho.cpu().numpy()[::k, ::k], True, True)
        assert np.array_equal(got[y:y + mx.shape[0]:k, x:x + mx.shape[1]:k], ref), "ms_reproject_aa differs from the reference"
    ta, tp = [], []
    for _ in range(blocks):
        ta.append(event_us(aa, reps)); tp.append(event_us(plain, reps))
    ma, mp = statistics.median(ta), statistics.median(tp)
    return {"what": "reproject_aa", "shape": name, "format": "i420" if i420 else "bgr", "frames_per_call": NF, "views": len(views), "atlas": "%dx%d" % (aw, ah), "levels": LEVELS,
            "footprint": span, "outputs_equal": True, "aa_us": ma, "point_us": mp, "aa_over_point": ma / mp, "aa_blocks_us": ta, "point_blocks_us": tp}


def resources_row():
    """the compiler's resource report of csrc/reproject_aa.hip, with build.sh's flags"""
    flags = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fvisibility=hidden".split()
    src = os.path.join(ROOT, "video-stitcher_amd", "csrc", "reproject_aa.hip")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_aa.jsonl"))
    ap.add_argument("--only", default="mips,viewport_small,cube_bgr,cube_i420,viewport_full")
    args = ap.parse_args()
    names = args.only.split(",")
    rows = []
    if names == ["resources"]:
        rows.append(resources_row())
    else:
        import torch
        cv = canvases()
        mips, row = mips_row(cv, args.reps)
        if "mips" in names:
            rows.append(row)
        for name in names:
            if name == "mips":
                continue
            if name not in SHAPES:
                raise SystemExit("unknown row %s" % name)
            rows.append(sampler_row(name, cv, mips, args.reps))
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
