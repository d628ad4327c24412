"""Run ON THE GPU BOX: cost of exposure tracking through per-view sample vectors (ms_gain_samples + ms_track_gains_from_samples).
  (a) config 2, unsharded context: GPU time of samples + from_samples(1 buffer) against ms_track_gains at strides 1 / 4 / 8, A / B alternating, medians of 5
      rounds of 9 calls each (events around the calls on the stitch stream, idle GPU).
  (b) config 5's geometry (12 x 4K -> 7680 x 3840) as two view shards on one GPU in the form of benchlib/shards.py (both shards' ms_stitch_partial, then
      ms_stitch_finish on the first, one stream, 8-frame calls): frames/s with tracking off, after every 8th call and after every call (stride 4), medians of 5
      loops, off measured before AND after.
--route off measures only what a library without the sample entry points has (MSSTITCH_LIB=<parent build>: the other half of an A / B pair across builds).
Prints one JSON line per part; --out FILE appends them there (profiles/gain_track_views.jsonl)."""
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


def lib_label():
    """Which build is measured, without the path of the box: "in-tree", or the MSSTITCH_LIB file relative to the repository."""
    p = os.environ.get("MSSTITCH_LIB")
    return "in-tree" if not p else os.path.relpath(os.path.realpath(p), ROOT)


def gpu_ms(call, reps=9):
    st = torch.cuda.current_stream()
    t = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(st)
        call()
        b.record(st)
        b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t[2:])


def part_a(route, rounds=5):
    comp, cfg, _ = make_rig(ms, "cfg2", max_frames=1)
    frames = [to_dev(synth.frame(cfg["w"], cfg["h"], i, 0)) for i in range(cfg["n"])]
    r = {"part": "a", "config": "cfg2", "route": route, "device": torch.cuda.get_device_name(0), "lib": lib_label()}
    for stride in (1, 4, 8):
        buf = torch.zeros(comp.gain_samples_bytes(stride) // 4, dtype=torch.int32, device="cuda") if route == "both" else None

        def track():
            comp.track_gains(frames, stride=stride, smoothing=0.25)

        def samples():
            comp.gain_samples(frames, stride, samples=buf)
            comp.track_gains_from_samples([buf], stride=stride, smoothing=0.25)
        a, b = [], []
        for _ in range(rounds):                 # A / B alternating
            a.append(gpu_ms(track))
            if route == "both":
                b.append(gpu_ms(samples))
        r["track_gains_us_stride_%d" % stride] = round(statistics.median(a) * 1e3, 2)
        if b:
            r["sample_route_us_stride_%d" % stride] = round(statistics.median(b) * 1e3, 2)
            r["delta_us_stride_%d" % stride] = round((statistics.median(b) - statistics.median(a)) * 1e3, 2)
            r["buffer_bytes_stride_%d" % stride] = buf.numel() * 4
    comp.close()
    return r


def part_b(route, F=8, calls=16, warmup=2, repeats=5, V=2):
    cfg = synth.CONFIGS["cfg5"]
    n = cfg["n"]
    pool = [[to_dev(synth.frame(cfg["w"], cfg["h"], i, t)) for i in range(n)] for t in range(2)]
    batch = [pool[j % 2] for j in range(F)]
    shards = [make_rig(ms, "cfg5", max_frames=F, shards=V, shard_index=k)[0] for k in range(V)]
    mine = [[[f if (s.needed_views() >> v) & 1 else None for v, f in enumerate(fr)] for fr in batch] for s in shards]
    parts = [torch.zeros(F * s.partial_bytes() // 2, dtype=torch.int16, device="cuda") for s in shards]
    outs = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(F)]
    bufs = [torch.zeros(s.gain_samples_bytes(4) // 4, dtype=torch.int32, device="cuda") for s in shards] if route == "both" else None
    torch.cuda.synchronize()

    def run():
        for k, s in enumerate(shards):
            s.stitch_partial(mine[k], parts[k])
        shards[0].stitch_finish(F, parts, out8u=outs)

    def track():
        for k, s in enumerate(shards):
            s.gain_samples(mine[k][-1], 4, samples=bufs[k])
        for s in shards:
            s.track_gains_from_samples(bufs, stride=4, smoothing=0.25)

    def fps(every):
        res = []
        for _ in range(repeats):
            for _ in range(warmup):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(calls):
                run()
                if every and (k + 1) % every == 0:
                    track()
            torch.cuda.synchronize()
            res.append(calls * F / (time.perf_counter() - t0))
        return round(statistics.median(res), 1)
    r = {"part": "b", "config": "cfg5 as %d view shards on one GPU" % V, "route": route, "frames_per_call": F, "lib": lib_label()}
    r["fps_off"] = fps(0)
    if route == "both":
        r["sample_buffer_bytes"] = [b.numel() * 4 for b in bufs]
        r["fps_track_every_8th"] = fps(8)
        r["fps_track_every_call"] = fps(1)
        r["fps_off_again"] = fps(0)
        r["counters"] = [s.gain_track_counters() for s in shards]
        g = [s.gains() for s in shards]
        r["gains_equal"] = bool((g[0].view("uint64") == g[1].view("uint64")).all())
    for s in shards:
        s.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--route", default="both", choices=["both", "off"])
    a = ap.parse_args()
    for p in a.parts.split(","):
        line = json.dumps({"a": part_a, "b": part_b}[p](a.route))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
