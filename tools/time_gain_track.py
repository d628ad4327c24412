"""Run ON THE GPU BOX: cost of exposure tracking (ms_track_gains) for config 2 (6 x 1080p -> 3840 x 1920) and config 3 (the same with CPW 40 x 40 meshes).
Per configuration, 32-frame calls:
  - host time of one ms_track_gains while stitches are in flight (median of several);
  - its GPU time (events around the call on the stitch stream, idle GPU) for stride 1, 4 and 8 (median of several);
  - frames/s with tracking off, after every 8th call and after every call (stride 4), each the median of several repeats, off measured before AND after.
Prints one JSON line per configuration; --out FILE also writes them there."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import msstitch as ms  # noqa: E402
import synth  # noqa: E402
from helpers import make_rig, to_dev  # noqa: E402

F = 32


def fps(run, track, every, calls=16, warmup=3, repeats=5):
    """Median frames/s of `repeats` timed loops of `calls` 32-frame calls; `track` runs after every `every`-th call (0: never)."""
    res = []
    for _ in range(repeats):
        for k in range(warmup):
            run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(calls):
            run()
            if every and (k + 1) % every == 0:
                track()
        torch.cuda.synchronize()
        res.append(calls * F / (time.perf_counter() - t0))
    return statistics.median(res), min(res), max(res)


def gpu_ms(comp, frames, stride, reps=9):
    st = torch.cuda.current_stream()
    t = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(st)
        comp.track_gains(frames, stride=stride, smoothing=0.25)
        b.record(st)
        b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t[2:])


def host_ms_in_flight(comp, run, frames, reps=9):
    t = []
    for _ in range(reps):
        run(); run()                      # two 32-frame calls queued on the GPU
        t0 = time.perf_counter()
        comp.track_gains(frames, stride=4, smoothing=0.25)
        t.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    return statistics.median(t)


def measure(name):
    cpw = name == "cfg3"
    comp, cfg, _ = make_rig(ms, "cfg2", enable_cpw=cpw, max_frames=F)
    n = cfg["n"]
    if cpw:
        for i in range(n):
            r = comp.view_geom(i).roi
            comp.set_mesh(i, *synth.mesh(r.width, r.height, 40, 40, phase=0.1 * i, amp=6.0))
    pool = [[to_dev(synth.frame(cfg["w"], cfg["h"], i, t)) for i in range(n)] for t in range(2)]
    out = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(F)]
    batch = [pool[j % 2] for j in range(F)]
    run = comp.prepared(batch, out8u=out)
    last = batch[-1]

    def track():
        comp.track_gains(last, stride=4, smoothing=0.25)
    r = {"config": name, "frames_per_call": F, "device": torch.cuda.get_device_name(0)}
    r["fps_off"], r["fps_off_min"], r["fps_off_max"] = fps(run, track, 0)
    r["fps_track_every_8th"], r["fps_every_8th_min"], r["fps_every_8th_max"] = fps(run, track, 8)
    r["fps_track_every_call"], r["fps_every_call_min"], r["fps_every_call_max"] = fps(run, track, 1)
    r["fps_off_again"] = fps(run, track, 0)[0]
    r["host_ms_track_in_flight"] = host_ms_in_flight(comp, run, last)
    for stride in (1, 4, 8):
        r["gpu_ms_stride_%d" % stride] = gpu_ms(comp, last, stride)
    g, ok, singular = comp.gains(counters=True)
    r["solves_ok"], r["solves_singular"] = ok, singular
    r["gains"] = [round(float(x), 6) for x in g]
    comp.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="cfg2,cfg3")
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        line = json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in measure(name).items()})
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
