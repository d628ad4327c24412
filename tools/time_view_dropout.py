"""Run ON THE GPU BOX: cost of camera dropout (ms_set_active_views) for config 2 (6 x 1080p -> 3840 x 1920) and config 3 (the same with CPW 40 x 40 meshes).
Per configuration, 32-frame calls:
  - host time of one ms_set_active_views while stitches are in flight: a first-time subset (tables made on the device), a cached one, the full set;
  - GPU time of the table rebuild (events around the call on its own stream), first time and cached;
  - frames/s with every view, without view 0 and without view 3 (the view that wraps around the +-pi seam).
Prints one JSON line per configuration; --out FILE also writes them there."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import msstitch as ms  # noqa: E402
import synth  # noqa: E402
from helpers import make_rig, to_dev  # noqa: E402

F = 32


def fps(run, calls=10, warmup=3):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        run()
    torch.cuda.synchronize()
    return calls * F / (time.perf_counter() - t0)


def gpu_ms(comp, mask, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(st)
    comp.set_active_views(mask, stream=st)
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def host_ms_in_flight(comp, run, mask):
    run(); run()                      # two 32-frame calls queued on the GPU
    t0 = time.perf_counter()
    comp.set_active_views(mask)
    dt = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return dt


def measure(name):
    cpw = name == "cfg3"
    comp, cfg, _ = make_rig(ms, "cfg2", enable_cpw=cpw, max_frames=F)
    n, all_ = cfg["n"], (1 << cfg["n"]) - 1
    if cpw:
        for i in range(n):
            r = comp.view_geom(i).roi
            comp.set_mesh(i, *synth.mesh(r.width, r.height, 40, 40, phase=0.1 * i, amp=6.0))
    pool = [[to_dev(synth.frame(cfg["w"], cfg["h"], i, t)) for i in range(n)] for t in range(2)]
    out = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(F)]
    run = comp.prepared([pool[j % 2] for j in range(F)], out8u=out)
    st = torch.cuda.Stream()
    r = {"config": name, "frames_per_call": F}
    r["fps_all_views"] = fps(run)
    # host time with stitches in flight: first time (tables made), cached (pointer swap), back to the full set
    r["host_ms_first"] = host_ms_in_flight(comp, run, all_ & ~(1 << 1))
    r["host_ms_full"] = host_ms_in_flight(comp, run, all_)
    r["host_ms_cached"] = host_ms_in_flight(comp, run, all_ & ~(1 << 1))
    comp.set_active_views(all_)
    # GPU time of the rebuild: a subset not made yet, then the same subset again (cached: nothing is enqueued)
    r["gpu_ms_first"] = gpu_ms(comp, all_ & ~(1 << 2), st)
    comp.set_active_views(all_)
    r["gpu_ms_cached"] = gpu_ms(comp, all_ & ~(1 << 2), st)
    for v in (0, 3):
        comp.set_active_views(all_ & ~(1 << v))
        r["fps_without_view_%d" % v] = fps(run)
    comp.set_active_views(all_)
    r["fps_all_views_again"] = fps(run)
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
