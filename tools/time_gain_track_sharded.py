"""Run ON THE GPU BOX: cost of exposure tracking through partial statistics (ms_gain_stats_partial + ms_track_gains_from_partials).
  (a) config 2, unsharded context: GPU time of partial + from_partials(1) against ms_track_gains at strides 1 / 4 / 8, A / B alternating, medians of 5 rounds
      of 9 calls each (events around the calls on the stitch stream, idle GPU).
  (b) config 5's geometry (12 x 4K -> 7680 x 3840) as two column windows on one GPU, each context on its own stream, 8-frame calls: frames/s with tracking
      off, after every 8th call and after every call (stride 4), medians of 5 loops, off measured before AND after.
  (c) config 2, 32-frame calls: frames/s with ms_track_gains (stride 4) after every call on the stitch stream and on a second stream (the publication is ordered
      behind the last stitch and before the next one), and with tracking off; medians of 5 loops.
--route track|off measures only what a library without the partial entry points has (MSSTITCH_LIB=<parent build>: the other half of an A / B pair across builds).
Prints one JSON line per part; --out FILE appends them there."""
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
    r = {"part": "a", "config": "cfg2", "route": route, "device": torch.cuda.get_device_name(0), "lib": os.environ.get("MSSTITCH_LIB", "in-tree")}
    part = comp.new_gain_partial() if route == "both" else None
    for stride in (1, 4, 8):
        def track():
            comp.track_gains(frames, stride=stride, smoothing=0.25)

        def partial():
            comp.gain_stats_partial(frames, stride, partial=part)
            comp.track_gains_from_partials([part], stride=stride, smoothing=0.25)
        a, b = [], []
        for _ in range(rounds):                 # A / B alternating
            a.append(gpu_ms(track))
            if route == "both":
                b.append(gpu_ms(partial))
        r["track_gains_us_stride_%d" % stride] = round(statistics.median(a) * 1e3, 2)
        if b:
            r["partial_route_us_stride_%d" % stride] = round(statistics.median(b) * 1e3, 2)
            r["delta_us_stride_%d" % stride] = round((statistics.median(b) - statistics.median(a)) * 1e3, 2)
    comp.close()
    return r


def part_b(route, F=8, calls=16, warmup=2, repeats=5):
    shards, streams, runs, lasts = [], [], [], []
    cfg = synth.CONFIGS["cfg5"]
    n = cfg["n"]
    pool = [[to_dev(synth.frame(cfg["w"], cfg["h"], i, t)) for i in range(n)] for t in range(2)]
    for k in range(2):
        comp = make_rig(ms, "cfg5", max_frames=F, col_shards=2, col_shard_index=k)[0]
        up = comp.needed_views() | (comp.gain_views() if route == "both" else 0)
        batch = [[f if (up >> v) & 1 else None for v, f in enumerate(pool[j % 2])] for j in range(F)]
        out = comp.new_i420(F)
        shards.append(comp); streams.append(torch.cuda.Stream()); runs.append(comp.prepared_i420(batch, out))
        lasts.append(batch[-1])
    parts = [s.new_gain_partial() for s in shards] if route == "both" else None
    torch.cuda.synchronize()

    def run():
        for s, st, fn in zip(shards, streams, runs):
            with torch.cuda.stream(st):
                fn()

    def track():
        for k, (s, st) in enumerate(zip(shards, streams)):
            s.gain_stats_partial(lasts[k], 4, partial=parts[k], stream=st)
        for st in streams:                      # every shard's solve reads both partials: behind both producers
            for other in streams:
                if other is not st:
                    st.wait_stream(other)
        for s, st in zip(shards, streams):
            s.track_gains_from_partials(parts, stride=4, smoothing=0.25, stream=st)

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
    r = {"part": "b", "config": "cfg5 as 2 column windows on one GPU", "route": route, "frames_per_call": F, "lib": os.environ.get("MSSTITCH_LIB", "in-tree")}
    r["fps_off"] = fps(0)
    if route == "both":
        r["fps_track_every_8th"] = fps(8)
        r["fps_track_every_call"] = fps(1)
        r["fps_off_again"] = fps(0)
        r["counters"] = [s.gain_track_counters() for s in shards]
        g = [s.gains() for s in shards]
        r["gains_equal"] = bool((g[0].view("uint64") == g[1].view("uint64")).all())
    for s in shards:
        s.close()
    return r


def part_c(route, F=32, calls=16, warmup=3, repeats=5):
    comp, cfg, _ = make_rig(ms, "cfg2", max_frames=F)
    n = cfg["n"]
    pool = [[to_dev(synth.frame(cfg["w"], cfg["h"], i, t)) for i in range(n)] for t in range(2)]
    out = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(F)]
    batch = [pool[j % 2] for j in range(F)]
    run = comp.prepared(batch, out8u=out)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()

    def fps(mode):
        res = []
        for _ in range(repeats):
            for _ in range(warmup):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                run()
                if mode == "same":
                    comp.track_gains(batch[-1], stride=4, smoothing=0.25)
                elif mode == "second":
                    comp.track_gains(batch[-1], stride=4, smoothing=0.25, stream=side)
            torch.cuda.synchronize()
            res.append(calls * F / (time.perf_counter() - t0))
        return round(statistics.median(res), 1)
    r = {"part": "c", "config": "cfg2", "route": route, "frames_per_call": F, "lib": os.environ.get("MSSTITCH_LIB", "in-tree")}
    r["fps_off"] = fps("off")
    if route != "off":
        r["fps_track_every_call_same_stream"] = fps("same")
        r["fps_track_every_call_second_stream"] = fps("second")
        r["fps_off_again"] = fps("off")
    comp.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--route", default="both", choices=["both", "track", "off"])
    a = ap.parse_args()
    for p in a.parts.split(","):
        line = json.dumps({"a": part_a, "b": part_b, "c": part_c}[p](a.route))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
