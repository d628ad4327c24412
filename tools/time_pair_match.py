#!/usr/bin/env python3
"""What matching every view pair of a rig costs, on one box, medians of 5, the two routes ALTERNATING, host clock around the synchronous calls:
  views6    6 views x 2500 random 32-byte descriptors, all 15 pairs
  views16   16 views x 2500, all 120 pairs
            route A: ms_match_pairs with RANSAC switched off (num_matches_thresh1 no pair reaches): one upload, two launches, one copy back, one synchronise
            route B: what a caller does without it: ms_knn_match_hamming2 for both directions of every pair (2 x pairs synchronous calls, each copying its 2-NN table to
                     the host) and the ratio test and cross-check in numpy
            both routes' lists are compared before anything is timed
  planted   6 views of 2500 keypoints, neighbouring views share 400 of them through a homography: the full call (RANSAC per pair on) against the same call with RANSAC
            off, to show how much of it is the per-pair RANSAC
  pixels    the unknown-overlap case of tests/test_pair_match_gpu.py: every pair's matches, inliers and confidence, the focal error and pixel angles
Appends one JSON line per row to profiles/pair_match.jsonl (or --out).

  python tools/time_pair_match.py [--out profiles/pair_match.jsonl] [--only views6,views16,planted,pixels]
  python tools/time_pair_match.py --once views16      # a warm-up and ONE route-A call, nothing written: the run to put under a kernel trace
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
import torch

import msstitch as ms
import pair_match_ref as PR

NEVER = 10 ** 9
CASES = {"views6": 6, "views16": 16}
PER_VIEW = 2500


def random_views(n, rng):
    """every view: 40 % of a common pool of rows with up to 30 bits flipped, the rest random -- so that the lists are not empty"""
    pool = rng.integers(0, 256, (PER_VIEW, 32), dtype=np.uint8)
    views = []
    for _ in range(n):
        d = rng.integers(0, 256, (PER_VIEW, 32), dtype=np.uint8)
        take = rng.permutation(PER_VIEW)[:PER_VIEW * 4 // 10]
        flips = np.zeros((len(take), 256), np.uint8)
        for r in range(len(take)):
            flips[r, rng.choice(256, size=int(rng.integers(0, 31)), replace=False)] = 1
        d[rng.permutation(PER_VIEW)[:len(take)]] = pool[take] ^ np.packbits(flips, axis=1)
        views.append(d)
    return views


class Caller:
    """ms_match_pairs with its arrays built beforehand"""

    def __init__(self, feats, lib=None, **kw):
        self.lib = lib if lib is not None else ms.load()      # (another build of the same ABI: tools/time_ransac_batch.py)
        self.n = len(feats)
        self.views, self.keep = ms.view_features(feats)
        self.prm = ms.pair_match_default_params(**kw)
        self.cap = self.n * (self.n - 1) * PER_VIEW
        self.pairs = (ms.PairMatches * (self.n * self.n))()
        self.out = np.zeros((self.cap, 4), np.int32)
        self.n_pairs, self.n_matches = C.c_int(0), C.c_int(0)

    def __call__(self):
        rc = self.lib.ms_match_pairs(self.n, self.views, C.byref(self.prm), self.pairs, self.n * self.n, C.byref(self.n_pairs), self.out.ctypes.data_as(C.POINTER(ms.FeatureMatch)),
                                     self.cap, C.byref(self.n_matches), None)
        assert rc == 0, self.lib.ms_last_error()

    def lists(self):
        return [(self.pairs[k].view_a, self.pairs[k].view_b, self.pairs[k].n_forward, self.out[self.pairs[k].first:self.pairs[k].first + self.pairs[k].count, :3].copy())
                for k in range(self.n_pairs.value)]


def route_b(descs_dev, match_conf=0.3):
    """both directions of every pair through ms_knn_match_hamming2, then the host rule, vectorised"""
    n = len(descs_dev)
    t = np.float32(1.0) - np.float32(match_conf)
    out = []
    for a in range(n):
        for b in range(a + 1, n):
            iab, dab = ms.knn_match_hamming2(descs_dev[a], descs_dev[b])
            iba, dba = ms.knn_match_hamming2(descs_dev[b], descs_dev[a])
            pa = dab[:, 0].astype(np.float32) < t * dab[:, 1].astype(np.float32)
            pb = dba[:, 0].astype(np.float32) < t * dba[:, 1].astype(np.float32)
            qa = np.nonzero(pa)[0]
            fwd = np.stack([qa, iab[qa, 0], dab[qa, 0]], axis=1)
            qb = np.nonzero(pb)[0]
            j0 = iba[qb, 0]
            dup = pa[j0] & (iab[j0, 0] == qb)
            qb, j0 = qb[~dup], j0[~dup]
            bwd = np.stack([j0, qb, dba[qb, 0]], axis=1)
            out.append((a, b, len(fwd), np.concatenate([fwd, bwd]).astype(np.int32)))
    return out


def timed(fns, blocks=5):
    runs = [[] for _ in fns]
    for _ in range(blocks):
        for fn, acc in zip(fns, runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t) * 1e3)
    return runs


def views_row(name, once=False):
    n = CASES[name]
    descs = random_views(n, np.random.default_rng(n))
    dev = [torch.from_numpy(d).cuda() for d in descs]
    feats = [(np.zeros((PER_VIEW, 2), np.float32), d, (640, 480)) for d in dev]
    a = Caller(feats, num_matches_thresh1=NEVER)
    a()                       # warm-up: code objects, the scratch blocks
    if once:
        torch.cuda.synchronize()
        a()
        return None
    la, lb = a.lists(), route_b(dev)
    assert len(la) == len(lb) == n * (n - 1) // 2
    for (a0, b0, nf0, r0), (a1, b1, nf1, r1) in zip(la, lb):
        assert (a0, b0, nf0) == (a1, b1, nf1) and np.array_equal(r0, r1), "the two routes differ on pair (%d, %d)" % (a0, b0)
    ra, rb = timed([a, lambda: route_b(dev)])
    return {"what": "pair_match", "case": name, "views": n, "pairs": len(la), "keypoints_per_view": PER_VIEW, "descriptor_bytes": 32, "matches": int(a.n_matches.value),
            "match_pairs_ms": statistics.median(ra), "match_pairs_runs_ms": ra, "launches": 2, "copies": 2, "synchronisations": 1,
            "knn_per_direction_ms": statistics.median(rb), "knn_per_direction_runs_ms": rb, "knn_per_direction_calls": 2 * len(la),
            "speedup": statistics.median(rb) / statistics.median(ra), "lists_equal": True}


PLANTED_VIEWS, PLANTED_SHARED = 6, 400


def planted_features():
    n, shared = PLANTED_VIEWS, PLANTED_SHARED
    rng = np.random.default_rng(7)
    W, H = 640, 480
    c = np.array([W / 2, H / 2])
    kps = [np.zeros((PER_VIEW, 2), np.float32) for _ in range(n)]
    descs = [rng.integers(0, 256, (PER_VIEW, 32), dtype=np.uint8) for _ in range(n)]
    for v in range(n):
        kps[v][:] = rng.uniform([0, 0], [W, H], (PER_VIEW, 2))
    for v in range(n - 1):      # view v + 1 shows `shared` keypoints of view v through a homography
        Hm = np.array([[1.0, 0.02, 40.0], [-0.02, 1.0, 5.0], [3e-5, 0.0, 1.0]])
        src = rng.permutation(PER_VIEW)[:shared]
        dst = rng.permutation(PER_VIEW)[:shared]
        p = np.concatenate([kps[v][src] - c, np.ones((shared, 1))], axis=1) @ Hm.T
        kps[v + 1][dst] = p[:, :2] / p[:, 2:3] + c + rng.normal(0, 0.3, (shared, 2))
        flips = np.zeros((shared, 256), np.uint8)
        for r in range(shared):
            flips[r, rng.choice(256, size=int(rng.integers(0, 31)), replace=False)] = 1
        descs[v + 1][dst] = descs[v][src] ^ np.packbits(flips, axis=1)
    return [(kps[v], torch.from_numpy(descs[v]).cuda(), (W, H)) for v in range(n)]


def planted_row():
    n, shared = PLANTED_VIEWS, PLANTED_SHARED
    feats = planted_features()
    full, off = Caller(feats), Caller(feats, num_matches_thresh1=NEVER)
    full(); off()
    rf, ro = timed([full, off])
    with_h = [k for k in range(full.n_pairs.value) if full.pairs[k].have_H]
    return {"what": "pair_match_planted", "views": n, "pairs": full.n_pairs.value, "keypoints_per_view": PER_VIEW, "shared_per_neighbouring_pair": shared,
            "matches": int(full.n_matches.value), "pairs_with_ransac": sum(1 for k in range(full.n_pairs.value) if full.pairs[k].count >= 6), "pairs_with_H": len(with_h),
            "inliers": [full.pairs[k].num_inliers for k in with_h], "full_call_ms": statistics.median(rf), "full_call_runs_ms": rf,
            "ransac_off_ms": statistics.median(ro), "ransac_off_runs_ms": ro, "ransac_share": 1.0 - statistics.median(ro) / statistics.median(rf)}


def pixels_row():
    import test_pair_match_gpu as T
    r = T.unknown_overlap_case(ms)
    return {"what": "pair_match_pixels", "views": r["n"], "size": [640, 480], "true_focal": r["f_true"],
            "pairs": [[p["view_a"], p["view_b"], p["count"], p["n_forward"], p["num_inliers"], round(p["confidence"], 4), p["have_H"]] for p in r["pairs"]],
            "pairs_columns": ["view_a", "view_b", "matches", "forward", "inliers", "confidence", "have_H"], "tree_parent": r["estimate"]["tree_parent"],
            "conf_thresh": T.PANO_CONF_THRESH, "biggest_component": r["component"], "biggest_component_conf_1": r["component_at_1"], "info": r["info"], "focal_start": r["f_start"], "focal_refined": r["f_refined"],
            "focal_err_start_pct": r["focal_err_before_pct"], "focal_err_refined_pct": r["focal_err_after_pct"], "start_px": r["before_px"], "refined_px": r["after_px"],
            "max_refined_px": max(r["after_px"]), "sum_sq_first_column_y_before_wave_correct": r["y_before"], "sum_sq_first_column_y_after_wave_correct": r["y_after"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_match.jsonl"))
    ap.add_argument("--only", default="views6,views16,planted,pixels")
    ap.add_argument("--once", default=None, help="run a warm-up and one ms_match_pairs call (RANSAC off) of this case and exit")
    args = ap.parse_args()
    if args.once:
        views_row(args.once, once=True)
        return
    rows = [pixels_row() if name == "pixels" else planted_row() if name == "planted" else views_row(name) for name in args.only.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
