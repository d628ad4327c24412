"""ms_find_homography_ransac_batch on the device.

1. a mixed batch (the four scenes of test_features_gpu's oracle test, the degenerate problems, one scene twice) against the single call, bit for bit, and the oracle
2. independence: the same problems in reverse order and each alone
3. the score kernel's boundaries: problem sizes around the points one wave takes of a chunk (W) and around the chunk (C), hypothesis counts around the 64-lane block
4. a batch in which every problem fails
5. ms_match_pairs over it: a rig whose pairs take every branch of BestOf2NearestMatcher::match in one call, against the rule restated over single calls"""
import numpy as np
import pytest

import orb_oracle as oo
import pair_match_ref as PR
from test_features_gpu import _scene
from test_pair_match_gpu import apply_h, flip_bits, on_device

pytestmark = pytest.mark.gpu

RS_WAVE_POINTS = 128        # W: csrc/features.hip
RS_CHUNK = 512              # C


# ---------------------------------------------------------------------------------------------------------------- problems and their references

def _square():
    sq = np.array([[0, 0], [100, 0], [100, 100], [0, 100]], np.float32)
    return sq, sq * 2 + 5


def _line(n=20):
    line = np.c_[np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32) * 2]
    return line, line.copy()


def mixed_problems():
    scenes = [_scene(n, o, s)[:2] for n, o, s in ((120, 40, 1), (400, 250, 2), (30, 5, 3), (9, 2, 4))]
    e = np.zeros((0, 2), np.float32)
    three = np.array([[0, 0], [1, 0], [0, 1]], np.float32)
    return scenes + [(e, e), (three, three), _square(), _line(), scenes[0]]


MIXED_STATUS = [0, 0, 0, 0, 1, 1, 0, 1, 0]      # which of them have a model
_REF = {}


def references(ms, key, problems, **kw):
    """(single-call result, oracle result) per problem, computed once and only read afterwards"""
    if key not in _REF:
        thr = kw.get("reproj_threshold", 3.0)
        _REF[key] = ([ms.find_homography_ransac(s, d, **kw) for s, d in problems],
                     [oo.find_homography_ransac(s, d, thr, kw.get("max_iters", 2000), kw.get("confidence", 0.995)) for s, d in problems])
    return _REF[key]


def assert_same_bits(got, want, what):
    assert len(got) == len(want)
    for p, ((H, m), (Hs, msk)) in enumerate(zip(got, want)):
        assert (H is None) == (Hs is None), "%s, problem %d: status differs" % (what, p)
        assert m.dtype == np.uint8 and np.array_equal(m, msk), "%s, problem %d: masks differ" % (what, p)
        assert H is None or H.tobytes() == Hs.tobytes(), "%s, problem %d: H differs by %g" % (what, p, np.abs(H - Hs).max())


def assert_matches_oracle(got, oracle, what, masks_only=False):
    for p, ((H, m), (Hr, mr)) in enumerate(zip(got, oracle)):
        assert (H is None) == (Hr is None), "%s, problem %d: status differs from the oracle's" % (what, p)
        assert np.array_equal(m, mr), "%s, problem %d: mask differs from the oracle's in %d places" % (what, p, int((m != mr).sum()))
        if H is not None and not masks_only:
            rel = np.linalg.norm(H - Hr) / np.linalg.norm(Hr)
            assert rel < 1e-6, "%s, problem %d: H is %g (relative, Frobenius) from the oracle's" % (what, p, rel)


def raw_batch(ms, problems, **kw):
    """the C call itself: H, mask, n_inliers and status as the library wrote them"""
    import ctypes as C
    import torch
    srcs = [np.ascontiguousarray(s, np.float32) for s, _ in problems]; dsts = [np.ascontiguousarray(d, np.float32) for _, d in problems]
    off = np.zeros(len(problems) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in srcs])
    src = np.concatenate(srcs + [np.zeros((1, 2), np.float32)]); dst = np.concatenate(dsts + [np.zeros((1, 2), np.float32)])
    H = np.full((len(problems), 9), 7.0); mask = np.full(int(off[-1]) + 1, 9, np.uint8)
    cnt = np.full(len(problems), -3, np.int32); status = np.full(len(problems), -3, np.int32)
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    rc = ms.load().ms_find_homography_ransac_batch(len(problems), off.ctypes.data_as(ip), src.ctypes.data_as(fp), dst.ctypes.data_as(fp), C.c_double(kw.get("reproj_threshold", 3.0)),
                                                   kw.get("max_iters", 2000), C.c_double(kw.get("confidence", 0.995)), H.ctypes.data_as(C.POINTER(C.c_double)),
                                                   mask.ctypes.data_as(C.POINTER(C.c_uint8)), cnt.ctypes.data_as(ip), status.ctypes.data_as(ip),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, off, H, mask, cnt, status


# ---------------------------------------------------------------------------------------------------------------- 1. the mixed batch

def test_mixed_batch_equals_the_single_call_and_the_oracle(ms, cuda):
    problems = mixed_problems()
    single, oracle = references(ms, "mixed", problems)
    assert [0 if H is not None else 1 for H, _ in single] == MIXED_STATUS
    got = ms.find_homography_ransac_batch(problems)
    assert_same_bits(got, single, "batch against single calls")
    assert_matches_oracle(got, oracle, "batch")
    assert got[8][0].tobytes() == got[0][0].tobytes() and np.array_equal(got[8][1], got[0][1])      # scene 1 a second time: the same bits at another place
    # n_inliers and status as the C call writes them; the byte behind the last mask stays
    rc, off, H, mask, cnt, status = raw_batch(ms, problems)
    assert rc == 0 and status.tolist() == MIXED_STATUS and mask[-1] == 9
    for p, (Hs, msk) in enumerate(single):
        assert cnt[p] == int(msk.sum()) and np.array_equal(mask[off[p]:off[p + 1]], msk)
        assert H[p].tobytes() == (np.zeros(9) if Hs is None else Hs.reshape(-1)).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2. independence

def test_result_depends_neither_on_neighbours_nor_on_place(ms, cuda):
    problems = mixed_problems()
    single, _ = references(ms, "mixed", problems)
    assert_same_bits(ms.find_homography_ransac_batch(problems[::-1])[::-1], single, "reverse order")
    for p, prob in enumerate(problems):
        assert_same_bits(ms.find_homography_ransac_batch([prob]), [single[p]], "problem %d alone" % p)


# ---------------------------------------------------------------------------------------------------------------- 3. boundaries

BOUNDARY_SIZES = [RS_WAVE_POINTS - 1, RS_WAVE_POINTS, RS_WAVE_POINTS + 1, RS_CHUNK - 1, RS_CHUNK, RS_CHUNK + 1, 2 * RS_CHUNK + 3]


def boundary_problems():
    """inlier-rich scenes of the boundary sizes (a tenth of the points are outliers: the adaptive stop ends their scans inside the first block of hypotheses), and one
    outlier-heavy scene whose scan needs a few hundred hypotheses, so that with max_iters 63, 64, 65 the last hypothesis of the budget is looked at"""
    return [_scene(n, n // 10, 100 + n)[:2] for n in BOUNDARY_SIZES] + [_scene(400, 250, 2)[:2]]


@pytest.mark.parametrize("max_iters", [1, 63, 64, 65, 2000])
def test_sizes_around_the_wave_share_and_the_chunk(ms, cuda, max_iters):
    """max_iters 1, 63, 64, 65: the hypothesis count below, at and across the 64-lane block; 2000: the whole budget on the device, the scans end early"""
    problems = boundary_problems()
    single, oracle = references(ms, "boundary %d" % max_iters, problems, max_iters=max_iters)
    got = ms.find_homography_ransac_batch(problems, max_iters=max_iters)
    assert_same_bits(got, single, "max_iters %d" % max_iters)
    assert_matches_oracle(got, oracle, "max_iters %d" % max_iters, masks_only=True)
    if max_iters > 1:       # nine points in ten are inliers: more than one subset in two is clean, so 63 draws find a model that most points follow
        assert all(H is not None and 2 * m.sum() > len(m) for H, m in got[:len(BOUNDARY_SIZES)])


# ---------------------------------------------------------------------------------------------------------------- 4. nothing but failures

def test_a_batch_of_failures_is_ok(ms, cuda):
    e = np.zeros((0, 2), np.float32)
    three = np.array([[0, 0], [1, 0], [0, 1]], np.float32)
    problems = [_line(), (three, three), (e, e), _line(7), (three[:1], three[:1])]
    rc, off, H, mask, cnt, status = raw_batch(ms, problems)
    assert rc == 0 and status.tolist() == [1] * 5 and not H.any() and not mask[:-1].any() and not cnt.any() and mask[-1] == 9
    assert all(H is None and not m.any() for H, m in ms.find_homography_ransac_batch(problems))


# ---------------------------------------------------------------------------------------------------------------- 5. ms_match_pairs

THRESH1, THRESH2 = 6, 40


def branch_rig():
    """6 views of 640 x 480, 32-byte descriptors.  View 1 shows rows 0 .. 119 of view 0 through a homography (and 30 more rows at random places); view 2 shows rows
    200 .. 229 (fewer than THRESH2); view 3 shows rows 250 .. 259, which lie on a line in both views (no subset can be drawn: no model); view 4 shows 3 rows
    (below THRESH1); view 5 has no keypoints.  The views other than view 0 share nothing with one another."""
    rng = np.random.default_rng(33)
    W, Hh = 640, 480
    c = np.array([W / 2, Hh / 2])
    d0 = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    k0 = np.zeros((300, 2), np.float32)
    k0[:] = rng.uniform([60, 60], [W - 60, Hh - 60], (300, 2))
    k0[250:260] = np.stack([100 + 40 * np.arange(10), 80 + 30 * np.arange(10)], axis=1)

    def noisy(rows):
        return np.stack([flip_bits(rng, d0[r], int(rng.integers(0, 30))) for r in rows])

    def extra(n):
        k = np.zeros((n, 2), np.float32)
        k[:] = rng.uniform([0, 0], [W, Hh], (n, 2))
        return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)

    H01 = np.array([[0.98, 0.03, 25.0], [-0.02, 1.01, -8.0], [4e-5, -2e-5, 1.0]])
    H02 = np.array([[1.02, -0.04, -30.0], [0.03, 0.97, 12.0], [-3e-5, 5e-5, 1.0]])
    k1, d1 = extra(190)
    d1[:150] = noisy(range(150))
    k1[:120] = apply_h(H01, k0[:120] - c) + c + rng.normal(0, 0.3, (120, 2))
    k2, d2 = extra(100)
    d2[:30] = noisy(range(200, 230))
    k2[:30] = apply_h(H02, k0[200:230] - c) + c + rng.normal(0, 0.3, (30, 2))
    k3, d3 = extra(80)
    d3[:10] = noisy(range(250, 260))
    k3[:10] = k0[250:260] * np.float32(0.5) + np.float32(20)
    k4, d4 = extra(70)
    d4[:3] = noisy(range(290, 293))
    k4[:3] = k0[290:293] + 10
    p1, p2, p3, p4 = rng.permutation(190), rng.permutation(100), rng.permutation(80), rng.permutation(70)
    kps = [k0, k1[p1], k2[p2], k3[p3], k4[p4], np.zeros((0, 2), np.float32)]
    descs = [d0, d1[p1], d2[p2], d3[p3], d4[p4], np.zeros((0, 32), np.uint8)]
    return kps, descs, (W, Hh)


def check_pairs(ms, pairs, kps, size):
    """every record and flag against BestOf2NearestMatcher::match (matchers.cpp:699-770) restated over single ms.find_homography_ransac calls; the branch of each pair"""
    taken = []
    for p in pairs:
        m = p["matches"]
        nothing = p["H"] is None and p["have_H"] == 0 and p["num_inliers"] == 0 and p["confidence"] == 0.0 and not m[:, 3].any()
        if p["count"] < THRESH1:
            assert nothing
            taken.append("no overlap" if p["count"] == 0 else "below thresh1")
            continue
        src = PR.centred_points(kps[p["view_a"]], size, m[:, 0]); dst = PR.centred_points(kps[p["view_b"]], size, m[:, 1])
        H1, inl = ms.find_homography_ransac(src, dst)
        if H1 is None:
            assert nothing
            taken.append("no model")
            continue
        assert abs(np.linalg.det(H1)) >= np.finfo(np.float64).eps
        assert p["have_H"] == 1 and np.array_equal(m[:, 3], inl) and p["num_inliers"] == int(inl.sum()) and p["confidence"] == PR.confidence(int(inl.sum()), p["count"])
        if p["num_inliers"] < THRESH2:
            assert p["H"].tobytes() == H1.tobytes()
            taken.append("one run")
            continue
        H2, _ = ms.find_homography_ransac(src[inl != 0], dst[inl != 0])
        assert H2 is not None and p["H"].tobytes() == H2.tobytes()
        taken.append("two runs")
    return taken


def test_match_pairs_takes_every_branch_in_one_call(ms, cuda):
    kps, descs, size = branch_rig()
    recs, rows = PR.match_lists(descs, np.float32(0.3))
    pairs = ms.match_pairs(on_device(descs, size, kps), num_matches_thresh1=THRESH1, num_matches_thresh2=THRESH2)
    assert len(pairs) == 15 and [(p["view_a"], p["view_b"], p["first"], p["count"], p["n_forward"]) for p in pairs] == recs
    for p, r in zip(pairs, rows):
        assert np.array_equal(p["matches"][:, :3], r)
    taken = check_pairs(ms, pairs, kps, size)
    by_pair = {(p["view_a"], p["view_b"]): t for p, t in zip(pairs, taken)}
    print(by_pair)
    assert by_pair[(0, 1)] == "two runs" and by_pair[(0, 2)] == "one run" and by_pair[(0, 3)] == "no model" and by_pair[(0, 4)] == "below thresh1"
    assert by_pair[(0, 5)] == "no overlap" and by_pair[(1, 2)] == "no overlap"
    for branch in ("below thresh1", "no model", "one run", "two runs", "no overlap"):
        assert branch in taken, "no pair took the branch %r" % branch
    p01 = pairs[0]
    assert p01["num_inliers"] >= 100 and pairs[1]["count"] >= 25 and pairs[2]["count"] >= THRESH1
    true = p01["matches"][p01["matches"][:, 3] != 0]
    src = PR.centred_points(kps[0], size, true[:, 0]).astype(np.float64); dst = PR.centred_points(kps[1], size, true[:, 1]).astype(np.float64)
    assert np.abs(apply_h(p01["H"], src) - dst).max() < 3.0
