"""ms_orb_detect_and_compute_batch (csrc/features.hip) against its contract: every view of a batch gets the bytes, in the order, that oracle/orb_oracle.py
gives for that view alone -- keypoint rows, descriptor rows, counts; ms_orb_detect_and_compute is the batch of one and is held to the same view of a batch.
The cases walk the places where the device pipeline decides what the reference's host code decides: levels that hold no more than a cull keeps (order stays
raster), ties in FAST score and Harris response, more raw corners than the detector's buffer, budgets at and below zero, views without an inner rectangle or
with a short pyramid, masks, pitched memory, 1 and 16 views, a reused scratch block, and a view that overflows its buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

import np_ref as R
import orb_oracle as oo
from test_features_edges_gpu import KINDS, blob_mask, noise, oracle_orb, same
from test_features_gpu import textured

pytestmark = pytest.mark.gpu

_ORACLE = {}


def want_of(oracle, g, mask=None, **kw):
    """oracle/orb_oracle.py on one view: (keypoints, descriptors); computed once per (image, mask, parameters) and only read"""
    key = (g.shape, g.tobytes(), None if mask is None else mask.tobytes(), tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = oracle_orb(oracle, g, mask, **kw)
    return _ORACLE[key]


def batch(ms, cuda, grays, masks=None, **kw):
    out = ms.orb_detect_and_compute_batch([torch.from_numpy(g).to(cuda) for g in grays],
                                          None if masks is None else [None if m is None else torch.from_numpy(m).to(cuda) for m in masks], **kw)
    assert [size for _, _, size in out] == [(g.shape[1], g.shape[0]) for g in grays]
    return [(kp, d.cpu().numpy()) for kp, d, _ in out]


def batch_equals_oracle(ms, cuda, oracle, grays, masks=None, **kw):
    got = batch(ms, cuda, grays, masks, **kw)
    for v, g in enumerate(grays):
        same(got[v], want_of(oracle, g, None if masks is None else masks[v], **kw), "view %d" % v)
    return got


def raw_batch(ms, grays, masks, descs, max_keypoints, **kw):
    """the C ABI with caller-made (pitched, prefilled, oversized) tensors: ([keypoints per view], counts)"""
    prm = ms.orb_params(**kw)
    n = len(grays)
    kp = np.zeros((n, max_keypoints, 6), np.float32)
    cnt = (C.c_int * n)()
    gi, di = (ms.Image * n)(*[ms.img(g) for g in grays]), (ms.Image * n)(*[ms.img(d) for d in descs])
    mi = None if masks is None else (ms.Image * n)(*[ms.Image() if m is None else ms.img(m) for m in masks])
    try:
        ms._chk(ms.load().ms_orb_detect_and_compute_batch(n, gi, mi, C.byref(prm), kp.ctypes.data_as(C.POINTER(C.c_float)), max_keypoints, di, cnt, ms._stream()))
    finally:
        torch.cuda.synchronize()
    return [kp[v, :cnt[v]].copy() for v in range(n)], list(cnt)


def level_counts(oracle, g, nfeatures, scale_factor=1.2, nlevels=8):
    """per level of the oracle's pipeline: (candidates after suppression, budget n)"""
    per = oo.n_features_per_level(nfeatures, scale_factor, nlevels)
    out, img = [], g
    for level in range(nlevels):
        lw, lh = R.orb_level_size(g.shape[1], g.shape[0], scale_factor, level)
        if lw < 8 or lh < 8:
            break
        if level:
            img = oracle.resize_linear_8u(img, dsize=(lw, lh))
        if per[level] <= 0:
            continue
        inner = np.zeros(img.shape, np.uint8)
        if lw > 62 and lh > 62:
            inner[31:lh - 31, 31:lw - 31] = 255
        out.append((len(oo.fast_detect(img, inner, 20, int(0.05 * lw * lh))[0]), per[level]))
    return out


def test_mixed_batch(ms, cuda, oracle):
    """views of different sizes and kinds in one call: ties in FAST score and (by symmetry) in Harris response on the checkerboard and the squares; fewer than 256
    rows (one row a lane in the row scan) and more (several rows a lane)"""
    grays = [textured(288, 216, 1), KINDS["checkerboard"](283, 197, 1), KINDS["squares"](288, 216, 2), KINDS["binary"](300, 220, 1), noise(517, 389, 1)]
    got = batch_equals_oracle(ms, cuda, oracle, grays, nfeatures=300)
    assert all(len(kp) > 50 for kp, _ in got)
    ties = got[2][0]
    assert len(set(ties[:, 2])) < len(ties), "the squares must hold equal Harris responses"


def test_degenerate_views_among_good_ones(ms, cuda, oracle):
    """no inner rectangle (62 x 62, 9 x 500), an inner rectangle of 2 x 8 (64 x 70), no level at all (7 x 90), no corner (flat): 0 keypoints or the
    oracle's, the neighbours untouched, and no descriptor row written from n_out[v] on"""
    a, b = textured(288, 216, 3), textured(301, 233, 4)
    grays = [a, noise(62, 62, 41), noise(9, 500, 41), noise(64, 70, 41), noise(7, 90, 41), np.full((300, 200), 128, np.uint8), b]
    cap = 204
    descs = [torch.full((cap, 32), 0xA5, dtype=torch.uint8, device=cuda) for _ in grays]
    kps, cnt = raw_batch(ms, [torch.from_numpy(g).to(cuda) for g in grays], None, descs, cap, nfeatures=200)
    for v, g in enumerate(grays):
        want = want_of(oracle, g, nfeatures=200)
        d = descs[v].cpu().numpy()
        same((kps[v], d[:cnt[v]]), want, "view %d" % v)
        assert (d[cnt[v]:] == 0xA5).all(), "view %d: descriptor rows past its count were written" % v
    assert cnt[1] == cnt[2] == cnt[4] == cnt[5] == 0 and cnt[0] > 100 and cnt[6] > 100


@pytest.mark.parametrize("nfeatures", [1, 2, 3, 4, 5, 7, 10, 21, 50])
def test_budgets_at_and_below_zero(ms, cuda, oracle, nfeatures):
    grays = [textured(288, 216, 5), textured(288, 216, 6)]
    got = batch_equals_oracle(ms, cuda, oracle, grays, nfeatures=nfeatures)
    per = oo.n_features_per_level(nfeatures)
    assert all(len(kp) <= sum(max(p, 0) for p in per) for kp, _ in got)
    if nfeatures >= 10:
        assert all(len(kp) > 0 for kp, _ in got)


def test_culls_with_nothing_to_drop_keep_their_order(ms, cuda, oracle):
    """nfeatures 5000 on small views: levels with count <= n pass both culls in raster order, levels with n < count <= 2n reach the Harris cull in raster order;
    at nfeatures 50 every level has count > 2n.  Both branches of both culls ran, by the oracle's counts."""
    grays = [textured(288, 216, 5), textured(288, 216, 6)]
    got = batch_equals_oracle(ms, cuda, oracle, grays, nfeatures=5000)
    big = [level_counts(oracle, g, 5000) for g in grays]
    small = level_counts(oracle, grays[0], 50)
    assert any(c <= n for lv in big for c, n in lv) and any(c > 2 * n for c, n in small), (big, small)
    batch_equals_oracle(ms, cuda, oracle, grays, nfeatures=50)
    c0, n0 = big[0][0]
    if 0 < c0 <= n0:                                # level 0 of view 0 came through untouched: its keypoints are in raster order
        lvl0 = got[0][0][got[0][0][:, 4] == 0]
        key = lvl0[:, 1] * 1000 + lvl0[:, 0]
        assert len(lvl0) == c0 and (np.diff(key) > 0).all()


def test_more_raw_corners_than_the_detectors_buffer(ms, cuda, oracle):
    """the image of test_features_edges_gpu.py's test of the same name as one view of two: the first max_npoints raw corners in raster order are the candidates"""
    w = h = 640
    rng = np.random.default_rng(5)
    g = np.full((h, w), 10, np.uint8)
    g[::4, ::4] = 250
    g[::4, ::4][rng.random((h // 4, w // 4)) < 0.3] = 200
    raw = oo.fast_scores(g, None) != 0
    assert int(raw[31:h - 31, 31:w - 31].sum()) > int(0.05 * w * h)
    got = batch_equals_oracle(ms, cuda, oracle, [textured(288, 216, 7), g], nfeatures=600)
    kp = got[1][0]
    lvl0 = kp[kp[:, 4] == 0]
    assert len(lvl0) == oo.n_features_per_level(600)[0]
    raw_rows = np.nonzero(raw[31:h - 31].any(axis=1))[0] + 31
    assert lvl0[:, 1].max() < raw_rows[-1] - 40, "corners past the buffer's end must not be reported"


def test_masks(ms, cuda, oracle):
    """grey blob masks (level 0 takes "non-zero", the levels above what is still 255 after the resize) on views 0 and 2, none on view 1; then no masks at all"""
    grays = [noise(330, 250, 31), textured(288, 216, 8), noise(301, 233, 32)]
    masks = [blob_mask(330, 250, 33), None, blob_mask(301, 233, 34)]
    with_masks = batch_equals_oracle(ms, cuda, oracle, grays, masks, nfeatures=600)
    without = batch_equals_oracle(ms, cuda, oracle, grays, None, nfeatures=600)
    assert with_masks[0][0].tobytes() != without[0][0].tobytes() and with_masks[1][0].tobytes() == without[1][0].tobytes()
    lvl0 = with_masks[2][0][with_masks[2][0][:, 4] == 0]
    assert len(lvl0) > 20 and (masks[2][lvl0[:, 1].astype(int), lvl0[:, 0].astype(int)] != 0).all()


def test_pitched_images_masks_and_descriptors_equal_the_contiguous_batch(ms, cuda, oracle):
    sizes, nf = [(301, 233), (288, 216)], 500
    grays = [textured(w, h, 9 + v) for v, (w, h) in enumerate(sizes)]
    masks = [blob_mask(w, h, 35 + v) for v, (w, h) in enumerate(sizes)]
    want = batch_equals_oracle(ms, cuda, oracle, grays, masks, nfeatures=nf)
    gp, mp, dp, wide_d = [], [], [], []
    for v, (w, h) in enumerate(sizes):
        wide = torch.from_numpy(noise(w + 90 + v, h, 36)).to(cuda)             # what surrounds the slice must not be read as image
        wide[:, 37:37 + w] = torch.from_numpy(grays[v]).to(cuda)
        gp.append(wide[:, 37:37 + w])
        wide_m = torch.full((h, w + 13 + v), 255, dtype=torch.uint8, device=cuda)
        wide_m[:, 5:5 + w] = torch.from_numpy(masks[v]).to(cuda)
        mp.append(wide_m[:, 5:5 + w])
        wide_d.append(torch.full((nf + 4, 48 + 16 * v), 0xAB, dtype=torch.uint8, device=cuda))
        dp.append(wide_d[v][:, 8:40])
    assert gp[0].stride(0) == 391 and mp[1].stride(0) == 302 and gp[0].data_ptr() % 4 == 1
    kps, cnt = raw_batch(ms, gp, mp, dp, nf + 4, nfeatures=nf)
    for v in range(2):
        out = wide_d[v].cpu().numpy()
        same((kps[v], out[:cnt[v], 8:40]), want[v], "view %d" % v)
        assert (out[:, :8] == 0xAB).all() and (out[:, 40:] == 0xAB).all() and (out[cnt[v]:] == 0xAB).all(), "bytes outside the descriptor columns / rows were written"


def test_one_view_and_sixteen(ms, cuda, oracle):
    grays = [textured(96 + 4 * v, 80 + (8 * v) // 3, 20 + v) for v in range(16)]
    assert grays[0].shape == (80, 96) and grays[15].shape == (120, 156)
    got = batch_equals_oracle(ms, cuda, oracle, grays, nfeatures=100)
    assert sum(len(kp) for kp, _ in got) > 300
    batch_equals_oracle(ms, cuda, oracle, grays[7:8], nfeatures=100)
    twice = batch(ms, cuda, [grays[15], grays[3], grays[15]], nfeatures=100)
    same(twice[0], twice[2])
    same(twice[0], got[15])


def test_two_calls_give_identical_bytes_over_a_reused_scratch_block(ms, cuda, oracle):
    """large batch, one-view batch, large batch again, on a stream of its own: the scratch block of the first call is reused by the others, every count starts at 0"""
    grays = [textured(640, 360, 17), noise(517, 389, 2), textured(288, 216, 1)]
    masks = [blob_mask(640, 360, 43), None, None]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        first = batch(ms, cuda, grays, masks, nfeatures=2500)
        one = batch(ms, cuda, grays[2:], nfeatures=300)
        third = batch(ms, cuda, grays, masks, nfeatures=2500)
    torch.cuda.synchronize()
    for a, b in zip(first, third):
        assert len(a[0]) > 100
        same(a, b)
    same(one[0], want_of(oracle, grays[2], nfeatures=300))
    same(first[0], want_of(oracle, grays[0], masks[0], nfeatures=2500))


def test_a_view_that_overflows_its_buffer_fails_the_call_by_name(ms, cuda, oracle):
    """nfeatures 7 at the defaults: the budgets are 2, 1, 1, 1, 1, 1, 1 and -1, so a view with corners on every level has 8 keypoints, by the oracle (the single call
    reports "more than max_keypoints" for it: test_features_edges_gpu.py::test_level_budgets_of_zero_and_below).  With max_keypoints == nfeatures the batch fails, names
    view 1 (view 0, flat, has none), and writes nothing past row max_keypoints - 1 of any view."""
    per = oo.n_features_per_level(7)
    assert per[-1] == -1 and sum(max(p, 0) for p in per) == 8
    g = textured(320, 250, 13)
    assert len(want_of(oracle, g, nfeatures=7)[0]) == 8
    grays = [torch.from_numpy(np.full((250, 320), 90, np.uint8)).to(cuda), torch.from_numpy(g).to(cuda)]
    descs = [torch.full((7 + 8, 32), 0xCD, dtype=torch.uint8, device=cuda) for _ in grays]
    with pytest.raises(ms.MsError, match="view 1.*max_keypoints"):
        raw_batch(ms, grays, None, descs, 7, nfeatures=7)
    for d in descs:
        assert (d[7:] == 0xCD).all()
    assert (descs[0] == 0xCD).all()
    kps, cnt = raw_batch(ms, grays, None, descs, 8, nfeatures=7)          # one more row holds it
    assert cnt == [0, 8]
