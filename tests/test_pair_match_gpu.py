"""ms_match_pairs on the device.

1. the device stage (2-NN of both directions, ratio test, cross-check, list order) against the numpy restatement tests/pair_match_ref.py, exactly
2. the same lists rebuilt from ms_knn_match_hamming2 per direction
3. range_width and pair_mask
4. the host stage (centred points, RANSAC, confidence, the second run) against ms.find_homography_ransac on reference-built points, bit for bit
5. determinism, the short buffer
6. from pixels with an unknown overlap graph: ORB -> match_pairs over all 28 pairs -> estimate_rig -> refine_rig_cameras -> wave_correct"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pair_match_ref as PR
import rig_ref as rr
import synth
from helpers import to_dev

pytestmark = pytest.mark.gpu
NEVER = 10 ** 9         # a num_matches_thresh1 no pair reaches: no RANSAC runs


# ---------------------------------------------------------------------------------------------------------------- synthetic views

def flip_bits(rng, row, k):
    out = row.copy()
    for b in rng.choice(8 * len(row), size=k, replace=False):
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def make_descs(counts, nbytes, seed):
    """View 0: random rows.  Every other view: rows of view 0, permuted, 0 to 40 bits flipped (never more than a third of the bits), plus random distractors; where the
    views are large enough, planted rows: view 0's rows 0, 1, 2 have their two nearest rows of the other view at 7:10, 14:20 and 21:30 bits (descriptors of 32 bytes and
    more), and its row 5 is there twice (d0 = d1 = 0)."""
    rng = np.random.default_rng(seed)
    bits = 8 * nbytes
    A = rng.integers(0, 256, (max(counts[0], 8), nbytes), dtype=np.uint8)
    views = [A[:counts[0]]]
    for n in counts[1:]:
        rows = []
        if n >= 64 and counts[0] >= 64:
            if nbytes >= 32:
                for k in range(3):
                    rows += [flip_bits(rng, A[k], 7 * (k + 1)), flip_bits(rng, A[k], 10 * (k + 1))]
            rows += [A[5].copy(), A[5].copy()]
        src = rng.permutation(np.arange(8, max(counts[0], 8)))[:max(0, (n * 6) // 10 - len(rows))] if counts[0] > 8 else []
        rows += [flip_bits(rng, A[s], int(rng.integers(0, min(40, bits // 3) + 1))) for s in src]
        while len(rows) < max(n, 1):
            rows.append(rng.integers(0, 256, nbytes, dtype=np.uint8))
        B = np.stack(rows)
        if n >= 64:
            B = B[rng.permutation(len(B))]
        views.append(B[:n])
    return views


def on_device(descs, size=(640, 480), kps=None):
    """features for ms.match_pairs: every descriptor matrix with a step 12 bytes over the row and 7 rows more than keypoints, the slack filled with noise"""
    rng = np.random.default_rng(99)
    feats = []
    for v, d in enumerate(descs):
        n, nbytes = d.shape
        buf = rng.integers(0, 256, (n + 7, nbytes + 12), dtype=np.uint8)
        buf[:n, :nbytes] = d
        t = torch.from_numpy(buf).cuda()[:, :nbytes]
        assert t.stride(0) == nbytes + 12 and t.shape[0] == n + 7
        feats.append((np.zeros((n, 2), np.float32) if kps is None else kps[v], t, size))
    return feats


def records(pairs):
    return [(p["view_a"], p["view_b"], p["first"], p["count"], p["n_forward"]) for p in pairs]


def assert_lists_equal(pairs, recs, rows):
    assert records(pairs) == recs
    for p, r in zip(pairs, rows):
        assert np.array_equal(p["matches"][:, :3], r), (p["view_a"], p["view_b"])
        assert not p["matches"][:, 3].any() and not p["have_H"] and p["num_inliers"] == 0 and p["confidence"] == 0.0


DEVICE_CASES = {
    "3 views, 32 bytes": ((257, 300, 130), 32), "5 views, 32 bytes, an empty view and a train side of one row": ((300, 0, 1, 2, 257), 32),
    "5 views, 32 bytes, around a wave": ((64, 3, 63, 65, 130), 32), "3 views, 4 bytes": ((130, 65, 300), 4), "3 views, 64 bytes": ((257, 64, 2), 64),
    "5 views, 64 bytes": ((65, 300, 0, 3, 63), 64),
}
_CASES = {}


def device_case(name):
    """descriptors and the reference's lists, computed once and only read afterwards"""
    if name not in _CASES:
        counts, nbytes = DEVICE_CASES[name]
        descs = make_descs(counts, nbytes, seed=len(name) + nbytes)
        _CASES[name] = (descs,) + PR.match_lists(descs, np.float32(0.3))
    return _CASES[name]


# ---------------------------------------------------------------------------------------------------------------- 1. against the reference

@pytest.mark.parametrize("name", sorted(DEVICE_CASES))
def test_device_stage_against_the_reference(ms, cuda, name):
    descs, recs, rows = device_case(name)
    counts, nbytes = DEVICE_CASES[name]
    n = len(counts)
    assert [r[:2] for r in recs] == [(i, j) for i in range(n) for j in range(i + 1, n)]
    # the inputs hold what they are meant to hold
    for (a, b, first, count, nf), r in zip(recs, rows):
        if counts[a] == 0 or counts[b] == 0:
            assert count == 0
        if a == 0 and counts[0] >= 64 and counts[b] >= 64:
            idx, dist = PR.knn2(descs[0], descs[b])
            assert dist[5].tolist() == [0, 0] and 5 not in r[:nf, 0]                   # the duplicated row: d0 = d1, refused forward ...
            assert sum(1 for m in r[nf:] if m[0] == 5 and m[2] == 0) == 2              # ... and both copies come back from the other direction
            if nbytes >= 32:
                for k in range(3):
                    assert dist[k].tolist() == [7 * (k + 1), 10 * (k + 1)] and k not in r[:nf, 0]
    assert sum(r[3] for r in recs) > 0 and any(r[3] > r[4] > 0 for r in recs)          # forward matches, and backward ones the cross-check let through
    dropped = 0                                                                         # backward matches the cross-check removes
    for (a, b, _, count, nf) in recs:
        if len(descs[b]) and len(descs[a]) >= 2:
            dropped += len(PR.pair_list_from_knn(None, None, *PR.knn2(descs[b], descs[a]), 0.3)[0]) - (count - nf)
    assert dropped > 0
    pairs = ms.match_pairs(on_device(descs), num_matches_thresh1=NEVER)
    assert_lists_equal(pairs, recs, rows)


# ---------------------------------------------------------------------------------------------------------------- 2. against ms_knn_match_hamming2

@pytest.mark.parametrize("name", ["3 views, 32 bytes", "3 views, 4 bytes", "5 views, 64 bytes"])
def test_device_stage_against_knn_match_hamming2(ms, cuda, name):
    descs = device_case(name)[0]
    feats = on_device(descs)
    pairs = ms.match_pairs(feats, num_matches_thresh1=NEVER)
    n = len(descs)
    k = 0
    for a in range(n):
        for b in range(a + 1, n):
            da, db = feats[a][1][:len(descs[a])], feats[b][1][:len(descs[b])]
            ab = ms.knn_match_hamming2(da, db) if len(descs[a]) and len(descs[b]) >= 2 else (None, None)
            ba = ms.knn_match_hamming2(db, da) if len(descs[b]) and len(descs[a]) >= 2 else (None, None)
            r, nf = PR.pair_list_from_knn(ab[0], ab[1], ba[0], ba[1], 0.3) if len(descs[a]) and len(descs[b]) else (np.zeros((0, 3), np.int32), 0)
            assert (pairs[k]["view_a"], pairs[k]["view_b"], pairs[k]["count"], pairs[k]["n_forward"]) == (a, b, len(r), nf)
            assert np.array_equal(pairs[k]["matches"][:, :3], r)
            k += 1
    assert k == len(pairs)


# ---------------------------------------------------------------------------------------------------------------- 3. range_width and pair_mask

def test_range_width_and_pair_mask(ms, cuda):
    descs = make_descs((65, 64, 70, 3, 66), 32, seed=4)
    feats = on_device(descs)
    mask = np.array([[0, 1, 0, 1, 1], [1, 0, 0, 1, 0], [1, 1, 1, 0, 1], [0, 0, 0, 0, 1], [1, 1, 1, 1, 1]], np.uint8)       # the diagonal and the lower half are never read
    for rw, m, want in ((2, None, [(0, 1), (1, 2), (2, 3), (3, 4)]), (3, None, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (2, 4), (3, 4)]), (1, None, []),
                        (0, mask, [(0, 1), (0, 3), (0, 4), (1, 3), (2, 4), (3, 4)]), (3, mask, [(0, 1), (1, 3), (2, 4), (3, 4)]), (0, np.zeros((5, 5), np.uint8), [])):
        assert PR.candidate_pairs(5, rw, m) == want
        recs, rows = PR.match_lists(descs, np.float32(0.3), rw, m)
        pairs = ms.match_pairs(feats, num_matches_thresh1=NEVER, range_width=rw, pair_mask=m)
        assert [(p["view_a"], p["view_b"]) for p in pairs] == want
        assert_lists_equal(pairs, recs, rows)


# ---------------------------------------------------------------------------------------------------------------- 4. the host stage

def apply_h(Hm, xy):
    p = np.concatenate([xy, np.ones((len(xy), 1))], axis=1) @ Hm.T
    return p[:, :2] / p[:, 2:3]


def planted_case(which):
    """Keypoints and descriptors of 3 views of 640 x 480.
    "homographies": view 1 shows rows 0 .. 119 of view 0 through H01 and rows 120 .. 149 at random places (outliers), view 2 shows rows 110 .. 179 through H02: the
                    pair (1, 2) shares rows 110 .. 119 only.
    "identical":    view 1 is view 0 (300 keypoints: 300 / (8 + 90) > 3), view 2 shares 4 rows with it."""
    rng = np.random.default_rng(21)
    W, Hh = 640, 480
    c = np.array([W / 2, Hh / 2])
    d0 = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    k0 = np.zeros((300, 6), np.float32)
    k0[:, :2] = rng.uniform([60, 60], [W - 60, Hh - 60], (300, 2))
    k0[:, 2:] = rng.uniform(0, 1, (300, 4))       # response .. size: never read

    def noisy(rows):
        return np.stack([flip_bits(rng, d0[r], int(rng.integers(0, 30))) for r in rows])

    def extra(n):
        k = np.zeros((n, 2), np.float32)
        k[:] = rng.uniform([0, 0], [W, Hh], (n, 2))
        return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)

    if which == "identical":
        k2, d2 = extra(40)
        d2[:4] = noisy(range(4)); k2[:4] = k0[:4, :2] + 30
        return [k0, k0.copy(), k2], [d0, d0.copy(), d2], (W, Hh)
    H01 = np.array([[0.98, 0.03, 25.0], [-0.02, 1.01, -8.0], [4e-5, -2e-5, 1.0]])
    H02 = np.array([[1.02, -0.04, -30.0], [0.03, 0.97, 12.0], [-3e-5, 5e-5, 1.0]])
    k1, d1 = extra(190)
    d1[:150] = noisy(range(150))
    k1[:120] = apply_h(H01, k0[:120, :2] - c) + c + rng.normal(0, 0.3, (120, 2))
    k2, d2 = extra(100)
    d2[:70] = noisy(range(110, 180))
    k2[:70] = apply_h(H02, k0[110:180, :2] - c) + c + rng.normal(0, 0.3, (70, 2))
    p1, p2 = rng.permutation(190), rng.permutation(100)
    return [k0, k1[p1], k2[p2]], [d0, d1[p1], d2[p2]], (W, Hh)


def check_host_stage(ms, pairs, kps, size, thresh1, thresh2):
    """every record against BestOf2NearestMatcher::match restated over ms.find_homography_ransac; returns the branch each pair took"""
    taken = []
    for p in pairs:
        m = p["matches"]
        if p["count"] < thresh1:
            assert p["H"] is None and p["num_inliers"] == 0 and p["confidence"] == 0.0 and not m[:, 3].any()
            taken.append("below thresh1")
            continue
        src = PR.centred_points(kps[p["view_a"]], size, m[:, 0]); dst = PR.centred_points(kps[p["view_b"]], size, m[:, 1])
        H1, inl = ms.find_homography_ransac(src, dst)
        if H1 is None:
            assert p["H"] is None and p["num_inliers"] == 0 and p["confidence"] == 0.0 and not m[:, 3].any()
            taken.append("no model")
            continue
        assert p["have_H"] == 1 and np.array_equal(m[:, 3], inl) and p["num_inliers"] == int(inl.sum())
        conf = PR.confidence(int(inl.sum()), p["count"])
        assert p["confidence"] == conf
        if p["num_inliers"] < thresh2:
            assert np.array_equal(p["H"], H1)
            taken.append("one run")
        else:
            H2, _ = ms.find_homography_ransac(src[inl != 0], dst[inl != 0])
            assert (p["H"] is None) == (H2 is None) and (H2 is None or np.array_equal(p["H"], H2))
            taken.append("two runs" if conf > 0 else "two runs, confidence above 3")
    return taken


def test_host_stage_planted_homographies(ms, cuda):
    kps, descs, size = planted_case("homographies")
    recs, rows = PR.match_lists(descs, np.float32(0.3))
    pairs = ms.match_pairs(on_device(descs, size, kps), num_matches_thresh1=6, num_matches_thresh2=40)
    assert records(pairs) == recs
    for p, r in zip(pairs, rows):
        assert np.array_equal(p["matches"][:, :3], r)
    for p in pairs:
        print("pair (%d, %d): %d matches, %d inliers, confidence %.4f" % (p["view_a"], p["view_b"], p["count"], p["num_inliers"], p["confidence"]))
    taken = check_host_stage(ms, pairs, kps, size, 6, 40)
    assert taken == ["two runs", "two runs", "one run"]
    assert pairs[0]["num_inliers"] >= 100 and pairs[1]["num_inliers"] >= 50 and 6 <= pairs[2]["count"] and pairs[2]["num_inliers"] < 40
    # the first pair's H is the planted one: the true matches map within the noise
    true = [(q, t) for q, t, _, inl in pairs[0]["matches"] if inl]
    src = PR.centred_points(kps[0], size, [q for q, _ in true]).astype(np.float64); dst = PR.centred_points(kps[1], size, [t for _, t in true]).astype(np.float64)
    assert np.abs(apply_h(pairs[0]["H"], src) - dst).max() < 3.0


def test_host_stage_identical_views_and_a_pair_below_thresh1(ms, cuda):
    kps, descs, size = planted_case("identical")
    pairs = ms.match_pairs(on_device(descs, size, kps))
    taken = check_host_stage(ms, pairs, kps, size, 6, 6)
    assert taken == ["two runs, confidence above 3", "below thresh1", "below thresh1"]
    p = pairs[0]
    assert p["count"] == p["n_forward"] == p["num_inliers"] == 300 and p["confidence"] == 0.0 and p["have_H"] == 1       # every backward match was a duplicate
    assert np.abs(p["H"] - np.eye(3)).max() < 1e-6
    assert 1 <= pairs[1]["count"] < 6 and pairs[1]["have_H"] == 0


# ---------------------------------------------------------------------------------------------------------------- 5. determinism, short buffer

def raw_call(ms, feats, matches_cap, **kw):
    n = len(feats)
    views, keep = ms.view_features(feats)
    prm = ms.pair_match_default_params(**kw)
    pairs = (ms.PairMatches * (n * n))()
    out = np.full((max(matches_cap, 1) + 1, 4), -5, np.int32)
    n_pairs, n_matches = C.c_int(-1), C.c_int(-1)
    rc = ms.load().ms_match_pairs(n, views, C.byref(prm), pairs, n * n, C.byref(n_pairs), out.ctypes.data_as(C.POINTER(ms.FeatureMatch)), matches_cap, C.byref(n_matches),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    del keep
    return rc, n_pairs.value, n_matches.value, bytes(pairs)[:C.sizeof(ms.PairMatches) * max(n_pairs.value, 0)], out


def test_two_calls_return_the_same_bytes(ms, cuda):
    kps, descs, size = planted_case("homographies")
    feats = on_device(descs, size, kps)
    a = raw_call(ms, feats, 2000, num_matches_thresh2=40)
    b = raw_call(ms, feats, 2000, num_matches_thresh2=40)
    assert a[0] == b[0] == 0 and a[1] == b[1] == 3 and a[2] == b[2] > 100
    assert a[3] == b[3] and a[4].tobytes() == b[4].tobytes()
    assert (a[4][a[2]:] == -5).all()            # nothing is written past the total


def test_short_match_buffer(ms, cuda):
    descs = device_case("3 views, 32 bytes")[0]
    feats = on_device(descs)
    rc, n_pairs, total, _, _ = raw_call(ms, feats, 4000, num_matches_thresh1=NEVER)
    assert rc == 0 and n_pairs == 3 and total == sum(r[3] for r in device_case("3 views, 32 bytes")[1])
    rc, n_pairs, needed, _, out = raw_call(ms, feats, total - 1, num_matches_thresh1=NEVER)
    assert rc == -1 and needed == total and n_pairs == 3 and b"matches_cap" in ms.load().ms_last_error()
    assert (out == -5).all()                    # a short buffer is left alone
    rc, _, n, _, _ = raw_call(ms, feats, total, num_matches_thresh1=NEVER)
    assert rc == 0 and n == total


# ---------------------------------------------------------------------------------------------------------------- 6. from pixels, rig unknown

FOCAL_BOUND_PCT = 0.0022       # measured 0.00108 %
ROTATION_BOUND_PX = 2.2        # measured 1.060 pixels at the true focal (view 3)
PANO_CONF_THRESH = 0.5         # leaveBiggestComponent's and the bundle adjuster's conf_thresh (the reference's default is 1: see test_unknown_overlap_from_pixels)


def unknown_overlap_case(ms):
    """ORB on the 8 rendered views of test_rig_focal_gpu.unknown_rig_case, then match_pairs over all 28 pairs (nothing says which views overlap), estimate_rig on the
    pairs with a homography, biggest_component at PANO_CONF_THRESH, refine_rig_cameras (shared focal, Huber 2 pixels) on the inlier matches of the pairs at or above
    that confidence (the pairs BundleAdjusterBase::estimate takes, motion_estimators.cpp:238-248), wave_correct"""
    import test_rig_focal_gpu as F
    import test_rig_pixels_gpu as T
    n = F.PX_N
    f_true = (T.W / 2.0) / math.tan(math.radians(T.HFOV) / 2.0)
    Rt = F.true_rig8()
    scale = synth.warp_scale(T.OUT_W)
    feats = []
    for v in range(n):
        k, d = ms.orb_detect_and_compute(ms.bgr_to_gray(to_dev(T.render(Rt[v], scale))), None, nfeatures=2500)
        feats.append((k, d, (T.W, T.H)))
    pairs = ms.match_pairs(feats)
    M = []
    for p in pairs:
        if p["have_H"] and p["confidence"] >= PANO_CONF_THRESH:
            m = p["matches"][p["matches"][:, 3] != 0]
            src = PR.centred_points(feats[p["view_a"]][0], (T.W, T.H), m[:, 0]).astype(np.float64)
            dst = PR.centred_points(feats[p["view_b"]][0], (T.W, T.H), m[:, 1]).astype(np.float64)
            M += [(p["view_a"], p["view_b"], src[i], dst[i]) for i in range(len(m))]
    prm = ms.rig_focal_default_params(shared_focal=1, huber_px=2.0)
    f0, R0, est = ms.estimate_rig(n, ms.pairs_for_estimate_rig(pairs), (T.W, T.H))
    f, R, info = ms.refine_rig_cameras(f0, R0, M, prm)
    Rw, wave_status = ms.wave_correct(R, ms.WAVE_HORIZ)
    want = rr.expected(R0, Rt, 0)
    return dict(n=n, pairs=pairs, estimate=est, info=info, min_pair_matches=prm.min_pair_matches, f_true=f_true, f_start=float(f0[0]), f_refined=float(f[0]),
                before_px=[rr.angle(R0[v], want[v]) * f_true for v in range(n)], after_px=[rr.angle(R[v], want[v]) * f_true for v in range(n)],
                focal_err_before_pct=abs(float(f0[0]) / f_true - 1.0) * 100.0, focal_err_after_pct=abs(float(f[0]) / f_true - 1.0) * 100.0,
                wave_status=wave_status, y_before=float((R[:, 1, 0] ** 2).sum()), y_after=float((Rw[:, 1, 0] ** 2).sum()), component=ms.biggest_component(n, pairs, PANO_CONF_THRESH), component_at_1=ms.biggest_component(n, pairs, 1.0))


def test_unknown_overlap_from_pixels(ms, cuda):
    """Measured on MI355X (profiles/pair_match.jsonl, "pair_match_pixels"): the 8 neighbouring pairs have 136 to 207 matches, 29 to 72 RANSAC inliers and confidences
    0.59 to 1.16; the 20 pairs of views that share no scene still have 100 to 148 matches each (the texture repeats), 10 to 15 of which RANSAC fits with some homography,
    confidences 0.19 to 0.33.  The maximum spanning tree over the inlier counts chains ring neighbours only.  At the reference's default conf_thresh of 1 the biggest
    component is views 0 to 3 alone (four neighbouring pairs lie below 1), so the pipeline runs at PANO_CONF_THRESH = 0.5, chosen after these figures were seen: there the
    component is the whole rig and the bundle adjustment takes the 8 neighbouring pairs (418 inlier matches).  Fed the inlier matches of ALL 28 pairs instead, the
    refinement collapses (the shared focal runs to 0, where the cost vanishes): the 20 pairs without overlap contradict every rig.  The homography estimate over all 28
    pairs starts at a focal of 266.31 against the true 320 (16.8 % off) with the views 7.0 to 15.2 pixels from the truth; refined, the focal is 320.003 (0.0011 % off)
    and the views end 0.34 to 1.06 pixels from the truth, 26 matches beyond the Huber threshold -- the one-direction, neighbours-only route of
    tests/test_rig_focal_gpu.py ends at 0.0104 % and 1.41 pixels on the same views with 268 inlier matches.  wave_correct takes the summed squared rig-Y component of the
    first columns from 2.01e-3 to 1.71e-3.  The two absolute bounds are twice the measured values, rounded up."""
    r = unknown_overlap_case(ms)
    n = r["n"]
    for p in r["pairs"]:
        print("pair (%d, %d): %4d matches (%4d forward), %3d inliers, confidence %.4f%s" % (p["view_a"], p["view_b"], p["count"], p["n_forward"], p["num_inliers"], p["confidence"],
                                                                                         "" if p["have_H"] else ", no H"))
    print("tree_parent %s; biggest component at confidence %.1f: %s, at confidence 1: %s" % (r["estimate"]["tree_parent"], PANO_CONF_THRESH, r["component"], r["component_at_1"]))
    print("focal: true %.3f, homography start %.3f (%.4f %% off), refined %.3f (%.4f %% off)" % (r["f_true"], r["f_start"], r["focal_err_before_pct"], r["f_refined"],
                                                                                               r["focal_err_after_pct"]))
    print("angle to the truth in pixels at the true focal, start:   %s" % ["%.3f" % x for x in r["before_px"]])
    print("angle to the truth in pixels at the true focal, refined: %s" % ["%.3f" % x for x in r["after_px"]])
    print("refinement %s; sum of squared rig-Y components of the first columns: %.6e before wave_correct, %.6e after" % (r["info"], r["y_before"], r["y_after"]))
    assert len(r["pairs"]) == 28
    for v, parent in enumerate(r["estimate"]["tree_parent"]):
        assert parent == -1 and v == 0 or (v - parent) % n in (1, n - 1), "the spanning tree chains view %d from view %d: not a ring neighbour" % (v, parent)
    neighbours = [p for p in r["pairs"] if (p["view_b"] - p["view_a"]) % n in (1, n - 1)]
    assert len(neighbours) == n
    assert all(p["have_H"] and p["num_inliers"] >= r["min_pair_matches"] for p in neighbours), [(p["view_a"], p["view_b"], p["num_inliers"]) for p in neighbours]
    assert r["component"] == list(range(n))
    assert r["estimate"]["status"] == 0 and r["info"]["cost_final"] <= r["info"]["cost_initial"]
    assert r["focal_err_after_pct"] <= r["focal_err_before_pct"]
    assert all(a <= b for a, b in zip(r["after_px"], r["before_px"])), "a view ends further from the truth than the homography start put it"
    assert r["wave_status"] == 0 and r["y_after"] < r["y_before"]
    assert r["focal_err_after_pct"] <= FOCAL_BOUND_PCT and max(r["after_px"]) <= ROTATION_BOUND_PX
