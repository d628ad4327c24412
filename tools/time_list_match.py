#!/usr/bin/env python3
"""What the application's matcher costs over a round's problems, on one box, medians of 5, the routes ALTERNATING, host clock around the synchronous calls.
  lists     P directed problems over sets of 2500 rows of 32 bytes with planted homographies -- 6 (the ring of a 6-view rig), 12 (ring + temporal) and 32 (16 views,
            both rings):
              route A: one ms_match_lists call
              route B: the loop it replaces, per problem ms_knn_match_hamming2 + the ratio test in numpy + ms_find_homography_ransac
            once with find_homography on and once off (route B then stops after the ratio test); the outputs of both routes are compared equal before anything is timed
  inputs    ms_feature_inputs_batch (grey images and feature masks of 6 views of 960 x 627 in one launch) against the 12 single launches (6 ms_bgr_to_gray,
            6 ms_feature_mask), each route followed by one synchronisation; outputs compared equal first
Appends one JSON line per row to profiles/list_match.jsonl (or --out).

  python tools/time_list_match.py [--out profiles/list_match.jsonl] [--only lists,inputs]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

PER_SET, SHARED, SHARED_TEMPORAL = 2500, 400, 1500
SIZE = (960, 627)
CASES = ((6, False), (6, True), (16, True))       # (views, with the temporal ring): 6, 12 and 32 problems
IP, FP, DP, BP = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def flip(rng, rows, most):
    """every row with up to `most` of its bits flipped"""
    out = rows.copy()
    for r in range(len(out)):
        for b in rng.choice(8 * out.shape[1], size=int(rng.integers(0, most + 1)), replace=False):
            out[r, b // 8] ^= np.uint8(1 << (b % 8))
    return out


def through(rng, kp, H, noise=0.4):
    p = np.c_[kp.astype(np.float64), np.ones(len(kp))] @ H.T
    return (p[:, :2] / p[:, 2:3] + rng.normal(0, noise, (len(kp), 2))).astype(np.float32)


def planted_sets(views, seed=3):
    """2 x views sets: set v < views is this round's view v, set views + v the same view a round earlier.  View v shares SHARED rows with its left neighbour (its rows
    0 .. SHARED - 1 are the neighbour's rows SHARED .. 2 SHARED - 1, a few bits flipped, the keypoints through a homography plus noise); the earlier round holds
    SHARED_TEMPORAL rows of this one, shuffled, the keypoints a pixel or two away"""
    rng = np.random.default_rng(seed)
    descs = [rng.integers(0, 256, (PER_SET, 32), dtype=np.uint8) for _ in range(views)]
    kps = [np.stack([rng.uniform(0, SIZE[0], PER_SET), rng.uniform(0, SIZE[1], PER_SET)], axis=1).astype(np.float32) for _ in range(views)]
    H_ring = np.array([[1.02, 0.03, -600.0], [-0.02, 0.98, 9.0], [2e-5, -1e-5, 1.0]])
    H_time = np.array([[1.0, 0.001, 1.5], [-0.001, 1.0, -1.0], [0.0, 0.0, 1.0]])
    fresh = [d.copy() for d in descs], [k.copy() for k in kps]
    for v in range(views):
        left = (v - 1) % views
        descs[v][:SHARED] = flip(rng, fresh[0][left][SHARED:2 * SHARED], 12)
        kps[v][:SHARED] = through(rng, fresh[1][left][SHARED:2 * SHARED], np.linalg.inv(H_ring))
    for v in range(views):
        keep = rng.permutation(PER_SET)[:SHARED_TEMPORAL]
        d = np.concatenate([flip(rng, descs[v][keep], 8), rng.integers(0, 256, (PER_SET - SHARED_TEMPORAL, 32), dtype=np.uint8)])
        k = np.concatenate([through(rng, kps[v][keep], H_time, 0.3), np.stack([rng.uniform(0, SIZE[0], PER_SET - SHARED_TEMPORAL), rng.uniform(0, SIZE[1], PER_SET - SHARED_TEMPORAL)], axis=1).astype(np.float32)])
        order = rng.permutation(PER_SET)
        descs.append(d[order]); kps.append(k[order])
    return descs, kps


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


class Round:
    """one round's sets on the device, its problems, and the outputs of both routes"""

    def __init__(self, ms, views, temporal):
        import torch
        self.ms, self.lib = ms, ms.load()
        descs, kps = planted_sets(views)
        self.kps = kps
        self.dev = [torch.from_numpy(d).cuda() for d in descs]
        self.table, self.keep = ms.view_features([(k, d, SIZE) for k, d in zip(kps, self.dev)])
        self.problems = [(v, (v - 1) % views) for v in range(views)] + ([(v, views + v) for v in range(views)] if temporal else [])
        self.P = len(self.problems)
        self.probs = (ms.MatchProblem * self.P)(*[ms.MatchProblem(q, t) for q, t in self.problems])
        self.recs = (ms.PairMatches * self.P)()
        self.cap = PER_SET * self.P
        self.out = np.zeros((self.cap, 4), np.int32)
        self.n_matches = C.c_int(0)
        self.idx = np.zeros((PER_SET, 2), np.int32); self.dist = np.zeros((PER_SET, 2), np.int32)
        self.loop_out = None

    def batch(self, find_homography):
        prm = self.ms.list_match_default_params(find_homography=find_homography)
        n_sets = len(self.dev)

        def run():
            rc = self.lib.ms_match_lists(n_sets, self.table, self.P, self.probs, C.byref(prm), self.recs, self.out.ctypes.data_as(C.POINTER(self.ms.FeatureMatch)), self.cap,
                                         C.byref(self.n_matches), None)
            assert rc == 0, self.lib.ms_last_error()
        return run

    def loop(self, find_homography):
        ms, lib = self.ms, self.lib
        images = [ms.img(d) for d in self.dev]
        half = [np.float32(SIZE[0]) * np.float32(0.5), np.float32(SIZE[1]) * np.float32(0.5)]

        def run():
            res = []
            for q, t in self.problems:
                rc = lib.ms_knn_match_hamming2(C.byref(images[q]), C.byref(images[t]), self.idx.ctypes.data_as(IP), self.dist.ctypes.data_as(IP), None)
                assert rc == 0, lib.ms_last_error()
                rows = np.nonzero(self.dist[:, 0].astype(np.float64) < 0.7 * self.dist[:, 1].astype(np.float64))[0]
                j0, d0 = self.idx[rows, 0].copy(), self.dist[rows, 0].copy()
                H, mask, cnt, st = np.zeros(9), np.zeros(len(rows), np.uint8), C.c_int(0), 1
                if find_homography and len(rows):
                    src = np.ascontiguousarray(self.kps[q][rows] - half); dst = np.ascontiguousarray(self.kps[t][j0] - half)
                    st = lib.ms_find_homography_ransac(src.ctypes.data_as(FP), dst.ctypes.data_as(FP), len(rows), C.c_double(0.0), 0, C.c_double(0.0), H.ctypes.data_as(DP),
                                                       mask.ctypes.data_as(BP), C.byref(cnt), None)
                    assert st in (0, 1), lib.ms_last_error()
                res.append((rows, j0, d0, H, mask, cnt.value, st))
            self.loop_out = res
        return run

    def equal(self, find_homography):
        for p, (rows, j0, d0, H, mask, cnt, st) in zip(self.recs, self.loop_out):
            m = self.out[p.first:p.first + p.count]
            if p.count != len(rows) or not (np.array_equal(m[:, 0], rows) and np.array_equal(m[:, 1], j0) and np.array_equal(m[:, 2], d0)):
                return False
            if find_homography and (np.array(p.H[:]).tobytes() != H.tobytes() or p.num_inliers != cnt or bool(p.have_H) != (st == 0) or not np.array_equal(m[:, 3] != 0, mask != 0)):
                return False
        return True


def lists_rows(ms):
    rows = []
    for views, temporal in CASES:
        rd = Round(ms, views, temporal)
        for fh in (1, 0):
            a, b = rd.batch(fh), rd.loop(fh)
            a(); b(); a(); b()          # warm-up: code objects, the scratch blocks
            assert rd.equal(fh), "ms_match_lists and the per-problem loop differ"
            ra, rb = timed([a, b])
            ma, mb = statistics.median(ra), statistics.median(rb)
            rows.append({"what": "list_match", "views": views, "temporal": temporal, "problems": rd.P, "rows_per_set": PER_SET, "descriptor_bytes": 32, "find_homography": fh,
                         "matches": int(rd.n_matches.value), "with_H": sum(1 for p in rd.recs if p.have_H), "inliers": [p.num_inliers for p in rd.recs],
                         "match_lists_ms": ma, "match_lists_runs_ms": ra, "per_problem_loop_ms": mb, "per_problem_loop_runs_ms": rb,
                         "loop_calls": rd.P * (2 if fh else 1), "speedup": mb / ma, "outputs_equal": True})
    return rows


def inputs_row(ms):
    import torch
    lib = ms.load()
    rng = np.random.default_rng(8)
    n, (w, h) = 6, SIZE
    views = []
    for _ in range(n):
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        px[:, :40] = 0; px[:30] = 0         # the part of a warped view the projection did not fill
        views.append(torch.from_numpy(px).cuda())
    bands = np.array([[0, 96, w - 96, 96]] * n, np.int32)
    new = lambda: [torch.empty((h, w), dtype=torch.uint8, device="cuda") for _ in range(n)]
    g1, m1, g2, m2 = new(), new(), new(), new()
    arr = lambda ts: (ms.Image * n)(*[ms.img(t) for t in ts])
    vi, gi1, mi1, gi2, mi2 = arr(views), arr(g1), arr(m1), arr(g2), arr(m2)
    bp = bands.ctypes.data_as(IP)

    def batch():
        assert lib.ms_feature_inputs_batch(n, vi, bp, gi1, mi1, None) == 0, lib.ms_last_error()
        torch.cuda.synchronize()

    def singles():
        for v in range(n):
            assert lib.ms_bgr_to_gray(C.byref(vi[v]), C.byref(gi2[v]), None) == 0, lib.ms_last_error()
        for v in range(n):
            assert lib.ms_feature_mask(C.byref(vi[v]), int(bands[v, 0]), int(bands[v, 1]), int(bands[v, 2]), int(bands[v, 3]), C.byref(mi2[v]), None) == 0, lib.ms_last_error()
        torch.cuda.synchronize()

    batch(); singles(); batch(); singles()
    assert all(torch.equal(a, b) for a, b in zip(g1 + m1, g2 + m2)), "ms_feature_inputs_batch and the single calls differ"
    ra, rb = timed([batch, singles])
    ma, mb = statistics.median(ra), statistics.median(rb)
    return {"what": "feature_inputs", "views": n, "size": [w, h], "batch_ms": ma, "batch_runs_ms": ra, "launches": 1, "single_calls_ms": mb, "single_calls_runs_ms": rb,
            "single_launches": 2 * n, "speedup": mb / ma, "outputs_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_match.jsonl"))
    ap.add_argument("--only", default="lists,inputs")
    args = ap.parse_args()
    import torch  # noqa: F401      # first: one HIP runtime per process, PyTorch's
    import msstitch as ms
    rows = []
    for name in args.only.split(","):
        rows += lists_rows(ms) if name == "lists" else [inputs_row(ms)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
