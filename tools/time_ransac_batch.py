#!/usr/bin/env python3
"""What fitting the homographies of many point sets costs, on one box, medians of 5, the routes ALTERNATING, host clock around the synchronous calls.  Two builds of the
library run in one process: this tree's (msstitch.load(); MSSTITCH_LIB picks another) and a build of the PARENT commit given with --parent-lib, which has no batch call and
fits pair after pair.
  batch     P problems of 400 points (150 of them outliers; P = 1, 12, 24, 120):
              route A: one ms_find_homography_ransac_batch call of this build
              route B: P ms_find_homography_ransac calls of the parent build
              route C: P ms_find_homography_ransac calls of this build (the batch of one)
            every H, mask, inlier count and status of route A is compared with route B's, bit for bit, before anything is timed
  planted   tools/time_pair_match.py's planted-homography case (6 views, 12 of 15 pairs reach RANSAC): the full ms_match_pairs call of both builds and this build's
            call with RANSAC off; both builds' records and match lists are compared byte for byte first
  trace     the rows of a rocprofv3 kernel trace (--output-format csv) of a `--once 24` run, per kernel: see --trace-dir
Appends one JSON line per row to profiles/ransac_batch.jsonl (or --out).

  python tools/time_ransac_batch.py --parent-lib PATH [--out profiles/ransac_batch.jsonl] [--only batch,planted]
  python tools/time_ransac_batch.py [--parent-lib PATH] --once 24      # a warm-up, then ONE batch call of 24 problems (and, with a parent build, its 24 single calls),
                                                                      # nothing written: the run to put under a kernel trace
  python tools/time_ransac_batch.py --trace-dir DIR                    # summarise the *kernel_trace.csv files under DIR into a row
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np

N_POINTS, N_OUTLIERS = 400, 150
BATCHES = (1, 12, 24, 120)
IP, FP, DP, BP = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def scene(seed, n=N_POINTS, outliers=N_OUTLIERS, noise=0.4):
    """n correspondences of one homography in centred pixels, `outliers` of them moved 20 to 200 pixels away (the scenes of tests/test_features_gpu.py)"""
    rng = np.random.default_rng(seed)
    H = np.array([[1.02, 0.03, 14.0], [-0.02, 0.98, -9.0], [2e-5, -1e-5, 1.0]])
    src = rng.uniform(-400, 400, size=(n, 2)).astype(np.float32)
    p = np.c_[src, np.ones(n)] @ H.T
    dst = (p[:, :2] / p[:, 2:3] + rng.normal(0, noise, size=(n, 2))).astype(np.float32)
    bad = rng.choice(n, outliers, replace=False)
    dst[bad] += rng.uniform(20, 200, size=(outliers, 2)).astype(np.float32) * rng.choice([-1, 1], size=(outliers, 2))
    return src, dst


class Problems:
    """P scenes packed for the batch call, and the outputs of both routes"""

    def __init__(self, P):
        self.P = P
        scenes = [scene(1000 + p) for p in range(P)]
        self.src = np.concatenate([s for s, _ in scenes]); self.dst = np.concatenate([d for _, d in scenes])
        self.off = np.arange(P + 1, dtype=np.int32) * N_POINTS
        self.out = {r: (np.zeros((P, 9)), np.zeros(P * N_POINTS, np.uint8), np.zeros(P, np.int32), np.zeros(P, np.int32)) for r in "ABC"}

    def batch(self, lib):
        H, m, cnt, st = self.out["A"]

        def run():
            rc = lib.ms_find_homography_ransac_batch(self.P, self.off.ctypes.data_as(IP), self.src.ctypes.data_as(FP), self.dst.ctypes.data_as(FP), C.c_double(0.0), 0, C.c_double(0.0),
                                                     H.ctypes.data_as(DP), m.ctypes.data_as(BP), cnt.ctypes.data_as(IP), st.ctypes.data_as(IP), None)
            assert rc == 0, lib.ms_last_error()
        return run

    def singles(self, lib, route):
        H, m, cnt, st = self.out[route]
        fn = lib.ms_find_homography_ransac
        calls = []
        for p in range(self.P):
            o = int(self.off[p])
            calls.append((self.src[o:].ctypes.data_as(FP), self.dst[o:].ctypes.data_as(FP), H[p].ctypes.data_as(DP), m[o:].ctypes.data_as(BP), C.byref(C.c_int.from_buffer(cnt, 4 * p)), p))

        def run():
            for s, d, h, mk, c, p in calls:
                rc = fn(s, d, N_POINTS, C.c_double(0.0), 0, C.c_double(0.0), h, mk, c, None)
                assert rc in (0, 1), lib.ms_last_error()
                st[p] = rc
        return run

    def equal(self, r0, r1):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self.out[r0], self.out[r1]))


def timed(fns, blocks=5):
    import torch
    runs = [[] for _ in fns]
    for _ in range(blocks):
        for fn, acc in zip(fns, runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t) * 1e3)
    return runs


def load_parent(path):
    assert path and os.path.isfile(path), "--parent-lib: a libmsstitch.so built from the parent commit is needed (there is no other route to compare with)"
    lib = C.CDLL(path)
    lib.ms_last_error.restype = C.c_char_p
    assert not hasattr(lib, "ms_find_homography_ransac_batch"), "%s already has the batch call: not a build of the parent commit" % path
    return lib


def batch_row(P, lib, parent):
    pr = Problems(P)
    a, b, c = pr.batch(lib), pr.singles(parent, "B"), pr.singles(lib, "C")
    a(); b(); c(); a(); b(); c()      # warm-up: code objects, the scratch blocks
    assert pr.out["A"][3].sum() == 0, "a scene ended without a model"
    assert pr.equal("A", "B"), "the batch call and the parent's single calls differ"
    assert pr.equal("A", "C"), "the batch call and this build's single calls differ"
    ra, rb, rc = timed([a, b, c])
    ma, mb, mc = statistics.median(ra), statistics.median(rb), statistics.median(rc)
    return {"what": "ransac_batch", "problems": P, "points_per_problem": N_POINTS, "outliers_per_problem": N_OUTLIERS, "max_iters": 2000,
            "inliers": [int(pr.out["A"][2].min()), int(pr.out["A"][2].max())], "batch_call_ms": ma, "batch_call_runs_ms": ra, "launches": 3, "copies": 4, "synchronisations": 2,
            "parent_single_calls_ms": mb, "parent_single_calls_runs_ms": rb, "single_calls_ms": mc, "single_calls_runs_ms": rc,
            "speedup_over_parent_single_calls": mb / ma, "single_call_against_parent": mc / mb, "bit_equal_to_parent_single_calls": True}


def planted_row(lib, parent):
    import time_pair_match as TP
    feats = TP.planted_features()
    new, old, off = TP.Caller(feats, lib=lib), TP.Caller(feats, lib=parent), TP.Caller(feats, lib=lib, num_matches_thresh1=TP.NEVER)
    for _ in range(2):
        new(); old(); off()
    k = new.n_pairs.value
    assert k == old.n_pairs.value and new.n_matches.value == old.n_matches.value
    size = C.sizeof(new.pairs[0]) * k
    assert bytes(new.pairs)[:size] == bytes(old.pairs)[:size] and new.out[:new.n_matches.value].tobytes() == old.out[:old.n_matches.value].tobytes(), "the two builds differ"
    rn, ro, rf = timed([new, old, off])
    with_h = [i for i in range(k) if new.pairs[i].have_H]
    return {"what": "pair_match_planted", "views": TP.PLANTED_VIEWS, "pairs": k, "keypoints_per_view": TP.PER_VIEW, "shared_per_neighbouring_pair": TP.PLANTED_SHARED,
            "matches": int(new.n_matches.value), "pairs_with_ransac": sum(1 for i in range(k) if new.pairs[i].count >= 6), "pairs_with_H": len(with_h),
            "inliers": [new.pairs[i].num_inliers for i in with_h], "full_call_ms": statistics.median(rn), "full_call_runs_ms": rn,
            "parent_full_call_ms": statistics.median(ro), "parent_full_call_runs_ms": ro, "ransac_off_ms": statistics.median(rf), "ransac_off_runs_ms": rf,
            "ransac_share": 1.0 - statistics.median(rf) / statistics.median(rn), "speedup_over_parent": statistics.median(ro) / statistics.median(rn), "records_equal_to_parent": True}


def once(P, lib, parent):
    import torch
    pr = Problems(P)
    a = pr.batch(lib)
    b = pr.singles(parent, "B") if parent is not None else None
    a(); a()
    if b:
        b()
    torch.cuda.synchronize()
    a()
    if b:
        b()
    torch.cuda.synchronize()


def trace_row(trace_dir, P=24):
    """per kernel of the RANSAC path: dispatches and their times in the LAST timed part of a `--once` run (one batch call: one dispatch per kernel of this build; then the
    parent's P single calls: P dispatches of its one-lane-per-hypothesis kernel, told apart by the workgroup size of 64)"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("ms::", "").strip()
            if "k_ransac" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 0)) or 0), int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)))
    assert rows, "no k_ransac_* dispatch in the kernel traces under %s" % trace_dir
    rows.sort()
    out = {"what": "ransac_batch_trace", "problems": P, "points_per_problem": N_POINTS, "max_iters": 2000}
    kinds = {"fit": lambda n, wg: n == "k_ransac_fit", "score": lambda n, wg: n == "k_ransac_score" and wg != 64, "gather": lambda n, wg: n == "k_ransac_gather",
             "parent_score": lambda n, wg: n == "k_ransac_score" and wg == 64}
    for kind, match in kinds.items():
        mine = [r for r in rows if match(r[2], r[3])]
        last = mine[-(P if kind == "parent_score" else 1):]
        if last:
            us = [(e - s) / 1e3 for s, e, _, _, _ in last]
            out["k_ransac_%s_us" % kind if kind != "parent_score" else "parent_k_ransac_score_us"] = us[0] if len(us) == 1 else {"dispatches": len(us), "median": statistics.median(us), "min": min(us), "max": max(us), "sum": sum(us)}
            out["%s_grid" % kind] = [last[-1][4], last[-1][3]]
    new = [r for r in rows if r[2] in ("k_ransac_fit", "k_ransac_gather") or r[2] == "k_ransac_score" and r[3] != 64][-3:]
    if len(new) == 3:
        out["batch_first_kernel_start_to_last_kernel_end_us"] = (new[-1][1] - new[0][0]) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_batch.jsonl"))
    ap.add_argument("--only", default="batch,planted")
    ap.add_argument("--parent-lib", default=os.environ.get("MSSTITCH_PARENT_LIB"))
    ap.add_argument("--once", type=int, default=None, help="run a warm-up and one batch call of this many problems and exit")
    ap.add_argument("--trace-dir", default=None, help="summarise the rocprofv3 kernel trace CSVs under this directory into a row and exit")
    args = ap.parse_args()
    rows = []
    if args.trace_dir:
        rows.append(trace_row(args.trace_dir))
    else:
        import torch  # noqa: F401      # first: one HIP runtime per process, PyTorch's
        import msstitch as ms
        lib = ms.load()
        if args.once:
            once(args.once, lib, load_parent(args.parent_lib) if args.parent_lib else None)
            return
        parent = load_parent(args.parent_lib)
        for name in args.only.split(","):
            rows += [batch_row(P, lib, parent) for P in BATCHES] if name == "batch" else [planted_row(lib, parent)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
