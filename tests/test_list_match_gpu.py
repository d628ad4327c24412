"""ms_match_lists and ms_feature_inputs_batch on the device.

1. the device stage (find_homography = 0) against the numpy restatement tests/list_match_ref.py, exactly: every edge size as query and as train, three descriptor
   lengths, padded steps, a set against itself, repeated problems
2. constructed distances around the ratio boundary at 0.7, 0.5 and 1.0
3. the whole call against the loop it replaces (ms_knn_match_hamming2 + the ratio test + ms_find_homography_ransac per problem), bit for bit; permutation; determinism
4. the short matches_cap
5. ms_feature_inputs_batch against ms_bgr_to_gray / ms_feature_mask, byte for byte, sentinels past the rows intact
6. stitch_app --solve-mesh --temporal"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import list_match_ref as LR
import pair_match_ref as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "video-stitcher_amd", "stitch_app")

# the edges of the 64-query block, the 256-row tile, the 256-query select round and the "fewer than two train rows" rule
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 600)
DEVICE_CASES = {32: SIZES, 4: (0, 1, 2, 64, 65, 257), 64: (0, 1, 2, 63, 256, 257)}


def flip_bits(rng, row, k):
    out = row.copy()
    for b in rng.choice(8 * len(row), size=k, replace=False):
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def make_sets(sizes, nbytes, seed):
    """One set per size: about two thirds of its rows are rows of a common base with 0 to a quarter of the bits flipped (so that lists are neither empty nor full and
    distances tie), the rest random"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (max(sizes), nbytes), dtype=np.uint8)
    sets = []
    for n in sizes:
        rows = [flip_bits(rng, base[s], int(rng.integers(0, 2 * nbytes + 1))) if k % 3 else rng.integers(0, 256, nbytes, dtype=np.uint8)
                for k, s in enumerate(rng.permutation(max(sizes))[:n])]
        sets.append(np.stack(rows) if rows else np.zeros((0, nbytes), np.uint8))
    return sets


def on_device(descs, sizes=None, kps=None, pad=16):
    """sets for ms.match_lists: every descriptor matrix with a step `pad` bytes over the row (48 for 32 bytes) and 5 rows more than keypoints, the slack filled with noise"""
    rng = np.random.default_rng(99)
    out = []
    for v, d in enumerate(descs):
        n, nbytes = d.shape
        buf = rng.integers(0, 256, (n + 5, nbytes + pad), dtype=np.uint8)
        buf[:n, :nbytes] = d
        t = torch.from_numpy(buf).cuda()[:, :nbytes]
        assert t.stride(0) == nbytes + pad
        out.append((np.zeros((n, 2), np.float32) if kps is None else kps[v], t, (640, 480) if sizes is None else sizes[v]))
    return out


_CASES = {}


def device_case(nbytes):
    """the sets, the problems (every size as query against every size as train, a set against itself among them, the first three problems repeated at the end) and the
    reference's lists: computed once and only read afterwards"""
    if nbytes not in _CASES:
        sizes = DEVICE_CASES[nbytes]
        descs = make_sets(sizes, nbytes, seed=nbytes)
        problems = [(q, t) for q in range(len(sizes)) for t in range(len(sizes))]
        problems += [problems[k] for k in (len(problems) - 1, len(sizes) + 1, len(problems) - 1)]
        _CASES[nbytes] = (descs, problems, [LR.problem_list(descs[q], descs[t]) for q, t in problems])
    return _CASES[nbytes]


@pytest.mark.parametrize("nbytes", sorted(DEVICE_CASES))
def test_device_stage_against_the_reference(ms, cuda, nbytes):
    descs, problems, want = device_case(nbytes)
    sizes = DEVICE_CASES[nbytes]
    # the inputs hold what they are meant to hold
    assert sum(len(w) for w in want) > 0
    for (q, t), w in zip(problems, want):
        if sizes[q] < 1 or sizes[t] < 2:
            assert len(w) == 0
        elif sizes[q] >= 63 and sizes[t] >= 63:
            assert 0 < len(w) and (q == t or len(w) < sizes[q]), (q, t)       # (a set against itself: every row finds itself at distance 0)
    assert problems[-1] == problems[-3] == (len(sizes) - 1, len(sizes) - 1) and len(want[-1]) > 0
    feats = on_device(descs)
    assert nbytes != 32 or feats[3][1].stride(0) == 48
    got = []
    for k0 in range(0, len(problems), ms.MATCH_MAX_PROBLEMS):
        chunk = problems[k0:k0 + ms.MATCH_MAX_PROBLEMS]
        res = ms.match_lists(feats, chunk, find_homography=0)
        first = 0
        for (q, t), r in zip(chunk, res):
            assert (r["view_a"], r["view_b"], r["first"], r["n_forward"]) == (q, t, first, r["count"]) and r["confidence"] == 1.0
            assert not r["have_H"] and r["num_inliers"] == 0 and not r["matches"][:, 3].any()
            first += r["count"]
        got += res
    for (q, t), r, w in zip(problems, got, want):
        assert np.array_equal(r["matches"][:, :3], w), (sizes[q], sizes[t], len(r["matches"]), len(w))


def _popcount_rows(counts, nbytes=32):
    rows = np.zeros((len(counts), nbytes), np.uint8)
    for r, c in enumerate(counts):
        bits = np.zeros(8 * nbytes, np.uint8)
        bits[:c] = 1
        rows[r] = np.packbits(bits)
    return rows


def test_constructed_distances(ms, cuda):
    """The query set is one all-zero row, so a train row's distance is its popcount"""
    trains = {"6:10": [10, 6], "7:10": [7, 10], "14:20": [30, 20, 14], "equal": [5, 9, 5], "0:0": [0, 0], "nearest tie": [8, 4, 4, 20], "4:10": [10, 4], "5:10": [5, 10],
              "second tie": [12, 3, 12], "9:10": [9, 10]}
    names = sorted(trains)
    descs = [_popcount_rows([0])] + [_popcount_rows(trains[k]) for k in names]
    feats = on_device(descs)
    problems = [(0, 1 + k) for k in range(len(names))]
    # what the single call reports for the tie: the lower index first, and the same distance second -- which is why no ratio lets it pass
    idx, dist = ms.knn_match_hamming2(feats[0][1][:1], feats[1 + names.index("nearest tie")][1][:4])
    assert idx.tolist() == [[1, 2]] and dist.tolist() == [[4, 4]]
    idx, dist = ms.knn_match_hamming2(feats[0][1][:1], feats[1 + names.index("second tie")][1][:3])
    assert idx.tolist() == [[1, 0]] and dist.tolist() == [[3, 12]]
    passing = {0.7: {"6:10": (1, 6), "4:10": (1, 4), "5:10": (0, 5), "second tie": (1, 3)},
               0.5: {"4:10": (1, 4), "second tie": (1, 3)},
               1.0: {"6:10": (1, 6), "4:10": (1, 4), "5:10": (0, 5), "second tie": (1, 3), "7:10": (0, 7), "14:20": (2, 14), "9:10": (0, 9)}}
    for ratio, ok in passing.items():
        res = ms.match_lists(feats, problems, find_homography=0, ratio=ratio)
        for k, r in zip(names, res):
            want = [[0, ok[k][0], ok[k][1]]] if k in ok else []
            assert r["matches"][:, :3].tolist() == want, (ratio, k, r["matches"].tolist())
            assert r["matches"][:, :3].tolist() == LR.problem_list(descs[0], descs[1 + names.index(k)], ratio).tolist()


# ---------------------------------------------------------------------------------------------------------------- 3. the whole call

_WHOLE = {}


def whole_case():
    """Sets A, B, C of 120 rows -- 80 of B's and of C's are A's rows with a few bits flipped, their keypoints A's through a homography plus noise, the rest random --,
    D of one row, E of none.  B has another image size than A; C has A's (a temporal pair)."""
    if not _WHOLE:
        rng = np.random.default_rng(7)
        sizes = [(640, 480), (600, 400), (640, 480), (640, 480), (320, 240)]
        dA = rng.integers(0, 256, (120, 32), dtype=np.uint8)
        kA = np.stack([rng.uniform(20, 620, 120), rng.uniform(20, 460, 120)], axis=1).astype(np.float32)
        descs, kps = [dA], [kA]
        for H, noise in ((np.array([[0.95, 0.03, -12.0], [-0.02, 0.9, 8.0], [1e-5, -2e-5, 1.0]]), 0.4), (np.array([[1.0, 0.004, 3.0], [-0.003, 1.0, -2.0], [0.0, 1e-6, 1.0]]), 0.3)):
            shared = rng.permutation(120)[:80]
            d = np.stack([flip_bits(rng, dA[s], int(rng.integers(0, 12))) for s in shared] + [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(40)])
            q = np.concatenate([kA[shared], np.ones((80, 1), np.float32)], axis=1).astype(np.float64) @ H.T
            k = np.concatenate([q[:, :2] / q[:, 2:] + rng.normal(0, noise, (80, 2)), np.stack([rng.uniform(20, 580, 40), rng.uniform(20, 380, 40)], axis=1)]).astype(np.float32)
            order = rng.permutation(120)
            descs.append(d[order]); kps.append(k[order])
        descs += [dA[5:6].copy(), np.zeros((0, 32), np.uint8)]
        kps += [kA[5:6].copy(), np.zeros((0, 2), np.float32)]
        _WHOLE["sets"] = (descs, kps, sizes)
        _WHOLE["problems"] = [(0, 1), (1, 0), (0, 2), (0, 3), (4, 0)]       # A -> B, B -> A, temporal A -> C, a train set of one row, a query set of no rows
    return _WHOLE["sets"], _WHOLE["problems"]


def loop_it_replaces(ms, feats, problems):
    """featurefinder::matchPair as it was: per problem one ms_knn_match_hamming2, the ratio test on the host, one ms_find_homography_ransac"""
    out = []
    for q, t in problems:
        (kq, dq, sq), (kt, dt, st) = feats[q], feats[t]
        rows = np.zeros((0, 3), np.int32)
        if len(kq) > 0 and len(kt) > 0:
            idx, dist = ms.knn_match_hamming2(dq[:len(kq)], dt[:len(kt)])
            keep = (idx[:, 1] >= 0) & (dist[:, 0].astype(np.float64) < 0.7 * dist[:, 1].astype(np.float64))
            qq = np.nonzero(keep)[0]
            rows = np.stack([qq, idx[qq, 0], dist[qq, 0]], axis=1).astype(np.int32).reshape(-1, 3)
        H, mask = None, np.zeros(0, np.uint8)
        if len(rows):
            H, mask = ms.find_homography_ransac(PR.centred_points(kq, sq, rows[:, 0]), PR.centred_points(kt, st, rows[:, 1]))
        out.append((rows, H, mask))
    return out


def _bytes_of(res):
    return b"".join(np.array([r["view_a"], r["view_b"], r["first"], r["count"], r["n_forward"], r["num_inliers"], r["have_H"]], np.int32).tobytes() + r["matches"].tobytes()
                    + (r["H"].tobytes() if r["H"] is not None else b"") + np.float64(r["confidence"]).tobytes() for r in res)


def test_whole_call_against_the_loop_it_replaces(ms, cuda):
    (descs, kps, sizes), problems = whole_case()
    feats = on_device(descs, sizes, kps)
    want = loop_it_replaces(ms, feats, problems)
    res = ms.match_lists(feats, problems)
    assert len(want[0][0]) >= 40 and len(want[2][0]) >= 40 and want[0][1] is not None and want[2][1] is not None and want[0][2].sum() >= 30     # the planted models are found
    assert len(want[3][0]) == 0 and len(want[4][0]) == 0
    first = 0
    for (q, t), r, (rows, H, mask) in zip(problems, res, want):
        assert (r["view_a"], r["view_b"], r["first"], r["count"], r["n_forward"]) == (q, t, first, len(rows), len(rows)) and r["confidence"] == 1.0
        assert np.array_equal(r["matches"][:, :3], rows)
        assert np.array_equal(r["matches"][:, 3] != 0, mask != 0) and r["num_inliers"] == int((mask != 0).sum())
        assert bool(r["have_H"]) == (H is not None)
        if H is not None:
            assert r["H"].tobytes() == H.tobytes(), (q, t)
        first += len(rows)
    # a problem's result depends neither on its neighbours nor on its place: permuting the problems permutes the results
    perm = [3, 2, 4, 0, 1]
    res_p = ms.match_lists(feats, [problems[k] for k in perm])
    for k, r in zip(perm, res_p):
        o = res[k]
        assert (r["view_a"], r["view_b"], r["count"], r["num_inliers"], r["have_H"]) == (o["view_a"], o["view_b"], o["count"], o["num_inliers"], o["have_H"])
        assert np.array_equal(r["matches"], o["matches"]) and (r["H"] is None) == (o["H"] is None) and (r["H"] is None or r["H"].tobytes() == o["H"].tobytes())
    # ... a problem alone (the shim's matchPair), and a repeated call
    one = ms.match_lists(feats, [problems[2]])[0]
    assert np.array_equal(one["matches"], res[2]["matches"]) and one["H"].tobytes() == res[2]["H"].tobytes() and one["first"] == 0
    assert _bytes_of(ms.match_lists(feats, problems)) == _bytes_of(res)
    # find_homography = 0: the same lists, nothing else
    bare = ms.match_lists(feats, problems, find_homography=0)
    for r, o in zip(bare, res):
        assert np.array_equal(r["matches"][:, :3], o["matches"][:, :3]) and not r["matches"][:, 3].any() and not r["have_H"] and r["num_inliers"] == 0 and r["confidence"] == 1.0


def test_short_matches_cap(ms, cuda):
    (descs, kps, sizes), problems = whole_case()
    feats = on_device(descs, sizes, kps)
    total = sum(r["count"] for r in ms.match_lists(feats, problems, find_homography=0))
    assert total >= 100
    table, keep = ms.view_features(feats)
    probs = (ms.MatchProblem * len(problems))(*[ms.MatchProblem(q, t) for q, t in problems])
    prm = ms.list_match_default_params()
    recs = (ms.PairMatches * len(problems))()
    out = np.full((total, 4), -3, np.int32)
    lib = ms.load()
    for cap, rc_want in ((total - 1, -1), (0, -1), (total, 0)):
        n = C.c_int(-7)
        rc = lib.ms_match_lists(len(feats), table, len(problems), probs, C.byref(prm), recs, out.ctypes.data_as(C.POINTER(ms.FeatureMatch)), cap, C.byref(n), None)
        assert rc == rc_want and n.value == total, (cap, rc, n.value, lib.ms_last_error())
        if rc:
            assert b"matches_cap" in lib.ms_last_error() and (out == -3).all()      # refused before anything is written
    with pytest.raises(ms.MsError, match="matches_cap"):
        ms.match_lists(feats, problems, matches_cap=total - 1)
    del keep


# ---------------------------------------------------------------------------------------------------------------- 5. ms_feature_inputs_batch

SENTINEL = 0xA5


def _padded(h, w, channels, step, fill=None):
    """(flat device buffer of h * step bytes filled with the sentinel, its (h, w[, channels]) view)"""
    buf = torch.full((h * step,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((h, w, channels), (step, channels, 1)) if channels > 1 else buf.as_strided((h, w), (step, 1))
    if fill is not None:
        view.copy_(torch.from_numpy(fill).cuda())
    return buf, view


def test_feature_inputs_batch_equals_the_single_calls(ms, cuda):
    rng = np.random.default_rng(4)
    lib = ms.load()
    shapes = [(1, 1, 7, 5, 2), (67, 5, 67 * 3 + 2, 67 + 3, 67), (130, 3, 130 * 3 + 5, 130 + 1, 130 + 6), (256, 64, 256 * 3 + 16, 256 + 8, 256 + 4)]     # w, h, steps of view / gray / mask
    bands = [(-5, 9, 0, 5), (-5, 30, 60, 40), (-1000, 1010, 120, 2), (3, 100, 200, 56)]      # clipped at the left edge (a_x0 < 0) and at the right one
    srcs, grays, masks = [], [], []
    for (w, h, ss, gs, msk) in shapes:
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        px[rng.random((h, w)) < 0.3] = 0                    # black pixels: outside the mask
        if w > 4:
            px[0, 2] = (0, 0, 1); px[0, 3] = (1, 0, 0)      # nearly black is not black
        srcs.append(_padded(h, w, 3, ss, px))
        grays.append(_padded(h, w, 1, gs)); masks.append(_padded(h, w, 1, msk))
    n = len(shapes)
    image = lambda pv, typ, step: ms.Image(pv[1].data_ptr(), step, pv[1].shape[1], pv[1].shape[0], typ)
    vi = (ms.Image * n)(*[image(s, ms.MS_8UC3, sh[2]) for s, sh in zip(srcs, shapes)])
    gi = (ms.Image * n)(*[image(g, ms.MS_8UC1, sh[3]) for g, sh in zip(grays, shapes)])
    mi = (ms.Image * n)(*[image(m, ms.MS_8UC1, sh[4]) for m, sh in zip(masks, shapes)])
    b = np.array(bands, np.int32)
    bp = b.ctypes.data_as(C.POINTER(C.c_int))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the single calls
    want_g, want_m = [], []
    for v in range(n):
        want_g.append(ms.bgr_to_gray(srcs[v][1]))
        m = torch.full(tuple(srcs[v][1].shape[:2]), 7, dtype=torch.uint8, device="cuda")
        assert lib.ms_feature_mask(C.byref(vi[v]), *[int(x) for x in bands[v]], C.byref(ms.img(m)), stream) == 0
        want_m.append(m)
    assert any(int(m.max()) == 255 for m in want_m) and all(int((m == 0).sum()) > 0 for m in want_m[1:])

    def check(out, want, shapes_step):
        for v in range(n):
            w, h = shapes[v][0], shapes[v][1]
            flat = out[v][0].cpu().numpy().reshape(h, shapes_step[v])
            assert np.array_equal(flat[:, :w], want[v].cpu().numpy()), v
            assert (flat[:, w:] == SENTINEL).all(), "view %d: bytes past the row were written" % v

    def untouched(out):
        return all(bool((o[0] == SENTINEL).all()) for o in out)

    # both outputs in one launch
    assert lib.ms_feature_inputs_batch(n, vi, bp, gi, mi, stream) == 0, lib.ms_last_error()
    torch.cuda.synchronize()
    check(grays, want_g, [s[3] for s in shapes]); check(masks, want_m, [s[4] for s in shapes])
    # grey only (no bands needed), masks only
    for o in grays + masks:
        o[0].fill_(SENTINEL)
    assert lib.ms_feature_inputs_batch(n, vi, None, gi, None, stream) == 0, lib.ms_last_error()
    torch.cuda.synchronize()
    check(grays, want_g, [s[3] for s in shapes])
    assert untouched(masks)
    for o in grays:
        o[0].fill_(SENTINEL)
    assert lib.ms_feature_inputs_batch(n, vi, bp, None, mi, stream) == 0, lib.ms_last_error()
    torch.cuda.synchronize()
    check(masks, want_m, [s[4] for s in shapes])
    assert untouched(grays)
    # the wrapper, on a subset in another order
    g, m = ms.feature_inputs_batch([srcs[3][1], srcs[1][1]], [bands[3], bands[1]])
    assert torch.equal(g[0], want_g[3]) and torch.equal(g[1], want_g[1]) and torch.equal(m[0], want_m[3]) and torch.equal(m[1], want_m[1])


# ---------------------------------------------------------------------------------------------------------------- 6. the application

def test_stitch_app_temporal(tmp_path):
    """--temporal: from the second round on every view is matched against itself one round earlier in the same ms_match_lists call as the ring, and the filtered
    matches feed the solver's temporal term.  The scene is static, so matches within 30 px exist in every round after the first."""
    out = subprocess.run([APP, "--size", "960x540", "--out", "1920x960", "--frames", "600", "--solve-mesh", "--temporal", "0.01"], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    info = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1])
    print(info)
    assert info["frames"] == 600 and info["recalibrations"] >= 2, info
    assert info["temporal_matches"] > 0 and info["temporal_alpha"] == 0.01, info
    # the option is refused without the solver
    bad = subprocess.run([APP, "--frames", "1", "--temporal", "0.01"], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"--solve-mesh" in bad.stderr
