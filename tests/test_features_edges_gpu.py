"""The feature front end on the device (csrc/features.hip) against oracle/orb_oracle.py at the edges test_features_gpu.py does not reach: image kinds
with score ties and plateaus, more raw corners than the detector's buffer, every 16-bit arc mask, grey and ragged masks, pitched images / masks /
descriptor matrices, tiny and odd pyramids, level budgets of zero and below, determinism -- and ms_feature_mask against a numpy statement.
The oracle itself is held to the definitions by test_orb_oracle.py (CPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import np_ref as R
import orb_oracle as oo
from test_features_gpu import textured

pytestmark = pytest.mark.gpu


def device_orb(ms, cuda, g, mask=None, **kw):
    kp, d = ms.orb_detect_and_compute(torch.from_numpy(g).to(cuda), None if mask is None else torch.from_numpy(mask).to(cuda), **kw)
    return kp, d.cpu().numpy()


def oracle_orb(oracle, g, mask=None, edge_threshold=31, **kw):
    return oo.orb_detect_and_compute(g, mask, edge=edge_threshold, resize=lambda im, sz: oracle.resize_linear_8u(im, dsize=sz), **kw)


def same(got, want, what=""):
    """THE comparison of (keypoints, descriptors) pairs: equal lengths, equal keypoint bytes, equal descriptor bytes -- rows in the same order (the oracle's: raster
    order after FAST, stable descending culls, levels concatenated).  On failure the first differing rows."""
    (kp, d), (kr, dr) = [(np.ascontiguousarray(k, np.float32), np.ascontiguousarray(x, np.uint8)) for k, x in (got, want)]
    assert len(kp) == len(kr) == len(d) == len(dr), (what, len(kp), len(kr), len(d), len(dr))
    if kp.tobytes() != kr.tobytes():
        rows = np.nonzero((kp.view(np.uint32) != kr.view(np.uint32)).any(axis=1))[0]
        raise AssertionError((what, "keypoints", len(rows), "rows differ, the first:", rows[:3].tolist(), kp[rows[:3]].tolist(), kr[rows[:3]].tolist()))
    if d.tobytes() != dr.tobytes():
        rows = np.nonzero((d != dr).any(axis=1))[0]
        raise AssertionError((what, "descriptors", len(rows), "rows differ, the first:", rows[:3].tolist(), d[rows[:3]].tolist(), dr[rows[:3]].tolist()))


def check(ms, cuda, oracle, g, mask=None, **kw):
    want = oracle_orb(oracle, g, mask, **kw)
    same(device_orb(ms, cuda, g, mask, **kw), want)
    return want


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def squares(w, h, seed):
    """8 x 8 squares, one per 16 x 16 cell, most of them 255 on 0 (plateaus of equal score at every corner: suppressed), some at random levels (ties broken)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    level = np.where(rng.random(((h + 15) // 16, (w + 15) // 16)) < 0.5, 255, rng.integers(30, 255, ((h + 15) // 16, (w + 15) // 16)))
    img = np.where((yy % 16 < 8) & (xx % 16 < 8), np.kron(level, np.ones((16, 16), np.int64))[:h, :w], 0)
    img[rng.integers(0, h, 150), rng.integers(0, w, 150)] ^= 64           # single pixels that break some of the ties
    return img.astype(np.uint8)


def checkerboard(w, h, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // 8) + (xx // 8)) & 1) * 255).astype(np.uint8)


def gradient(w, h, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx * 2 + yy * 3) // 8 % 256).astype(np.uint8)


def binary(w, h, seed):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 2, ((h + 4) // 5, (w + 4) // 5))
    img = np.kron(coarse, np.ones((5, 5), np.int64))[:h, :w]
    flip = rng.random((h, w)) < 0.02
    return (np.where(flip, 1 - img, img) * 255).astype(np.uint8)


KINDS = {"noise": noise, "squares": squares, "checkerboard": checkerboard, "gradient": gradient, "binary": binary, "textured": textured}


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_image_kinds(ms, cuda, oracle, kind, seed):
    if kind in ("checkerboard", "gradient") and seed > 1:
        seed = 1                                   # (these two have no seed: the second case runs another size instead)
        g = KINDS[kind](283, 197, seed)
    else:
        g = KINDS[kind](288, 216, seed)
    kp, _ = check(ms, cuda, oracle, g, nfeatures=300)
    if kind == "gradient":
        assert len(kp) == 0                        # none on a ramp
    elif kind == "checkerboard":
        assert not (kp[:, 4] == 0).any()           # no FAST corner at a junction of four squares (arcs of 5); the resampled levels above have some
    else:
        assert len(kp) > 50 and len(set(kp[:, 4])) >= 3, (kind, len(kp))


def test_more_raw_corners_than_the_detectors_buffer(ms, cuda, oracle):
    """single pixels of 250 on 10 on a 4-pixel grid: each is a corner (16 darker circle pixels) and nothing else is, so 1 / 16 of the inner rectangle
    = 0.0625 (W - 62) (H - 62) / (W H) of the image: above the buffer's 5 % for a square image wider than about 590.  Some pixels are raised so that
    the kept corners differ in response and the culls have something to order."""
    w = h = 640
    rng = np.random.default_rng(5)
    g = np.full((h, w), 10, np.uint8)
    g[::4, ::4] = 250
    g[::4, ::4][rng.random((h // 4, w // 4)) < 0.3] = 200
    over = []
    img = g
    for level in range(8):
        lw, lh = R.orb_level_size(w, h, 1.2, level)
        if level:
            img = oracle.resize_linear_8u(img, dsize=(lw, lh))
        inner = np.zeros(img.shape, np.uint8); inner[31:lh - 31, 31:lw - 31] = 255
        over.append(int((oo.fast_scores(img, inner) != 0).sum()) > int(0.05 * lw * lh))
    assert over[0], "level 0 must have more raw corners than 5 % of its area"
    free = np.zeros((200, 200), np.uint8) + 10; free[::4, ::4] = 250
    assert abs((oo.fast_scores(free, None) != 0).mean() - 0.06) < 0.003
    kp, _ = check(ms, cuda, oracle, g, nfeatures=600)
    lvl0 = kp[kp[:, 4] == 0]
    assert len(lvl0) == oo.n_features_per_level(600)[0]
    raw_rows = np.nonzero((oo.fast_scores(g, None) != 0)[31:h - 31].any(axis=1))[0] + 31
    assert lvl0[:, 1].max() < raw_rows[-1] - 40, "corners past the buffer's end must not be reported"


# The detection mask admits the grid centres and a sprinkle of other pixels, not the whole image: every raised circle pixel standing alone is itself a
# corner (16 darker pixels around it), which would bring some 10^5 keypoints per call and, where the circles of neighbouring centres touch, ties that
# suppress a centre.  Suppression reads the score map, which is 0 where the mask is 0, so a centre admitted without its 8 neighbours always survives.
ARC_GRID, ARC_COLS, ARC_ROWS = 7, 128, 64


def arc_image(masks, sign, base=100, threshold=20):
    """centres on a 7-pixel grid inside the 31-pixel border; circle pixel k of centre i = base + sign * (threshold + 1) where bit k of masks[i] is set.
    Returns the image, the detection mask and the centres."""
    img = np.full((62 + ARC_GRID * ARC_ROWS, 62 + ARC_GRID * ARC_COLS), base, np.uint8)
    cy, cx = 34 + ARC_GRID * (np.arange(len(masks)) // ARC_COLS), 34 + ARC_GRID * (np.arange(len(masks)) % ARC_COLS)
    for k, (dy, dx) in enumerate(R.fast_ring()):
        img[cy + dy, cx + dx] = base + sign * (threshold + 1) * ((masks >> k) & 1)
    admit = np.random.default_rng(int(masks[0]) + (sign > 0)).random(img.shape) < 0.004
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            admit[cy + dy, cx + dx] = False
    admit[cy, cx] = True
    return img, np.where(admit, 255, 0).astype(np.uint8), cx, cy


@pytest.mark.parametrize("sign", [1, -1], ids=["brighter", "darker"])
@pytest.mark.parametrize("part", range(65536 // (ARC_COLS * ARC_ROWS)))
def test_every_16_bit_arc_mask(ms, cuda, oracle, part, sign):
    """fast_score_at's rotate-and-AND against the literal rule, over all 65 536 masks (8 192 per call) for brighter and for darker arcs: the grid centres
    reported are exactly the masks that hold a 9-arc, each with score `threshold`.  The admitted pixels off the grid centres (many of them corners:
    raised circle pixels) are compared with the oracle like everything else."""
    masks = np.arange(part * ARC_COLS * ARC_ROWS, (part + 1) * ARC_COLS * ARC_ROWS)
    img, admit, cx, cy = arc_image(masks, sign)
    nfeatures = 6000                                # one level holds the whole budget: no cull (1 025 masks in all have a 9-arc; some 2 000 other pixels are admitted)
    kp, d = device_orb(ms, cuda, img, admit, nfeatures=nfeatures, nlevels=1)
    assert len(kp) < nfeatures // 2 and (kp[:, 4] == 0).all()
    centre_of = {(int(x), int(y)): int(m) for x, y, m in zip(cx, cy, masks)}
    on_grid = np.array([(int(k[0]), int(k[1])) in centre_of for k in kp], bool)
    got = {centre_of[(int(k[0]), int(k[1]))] for k in kp[on_grid]}
    want = set(masks[R.has_arc_by_definition(masks, 9)].tolist())
    assert got == want, (sorted(got - want)[:5], sorted(want - got)[:5])
    assert (~on_grid).sum() > 20
    same((kp, d), oracle_orb(oracle, img, admit, nfeatures=nfeatures, nlevels=1))


def blob_mask(w, h, seed, values=(0, 1, 128, 254, 255)):
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    for _ in range(30):
        y, x, ry, rx = rng.integers(0, h), rng.integers(0, w), rng.integers(4, 40), rng.integers(4, 40)
        yy, xx = np.ogrid[0:h, 0:w]
        m[((yy - y) / ry) ** 2 + ((xx - x) / rx) ** 2 < 1] = values[rng.integers(0, len(values))]
    return m


@pytest.mark.parametrize("kind", ["grey_blobs", "random_pixels", "inside_border", "one_and_254", "all_zero", "all_one"])
def test_masks(ms, cuda, oracle, kind):
    """level 0 takes the mask as "non-zero"; an upper level resizes the level below and keeps only what is still 255"""
    w, h = 330, 250
    g = noise(w, h, 31)
    rng = np.random.default_rng(32)
    if kind == "grey_blobs":
        mask = blob_mask(w, h, 33)
    elif kind == "random_pixels":
        mask = rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), size=(h, w))
    elif kind == "inside_border":                  # boundaries at 20 / 29 / 31 / 32 pixels from the edges: inside, and just at, the 31-pixel border
        mask = np.zeros((h, w), np.uint8); mask[20:h - 29, 31:w - 32] = 255; mask[:, 100:110] = 0
    elif kind == "one_and_254":
        mask = np.where(blob_mask(w, h, 34, values=(0, 255)) != 0, 254, 1).astype(np.uint8)
    else:
        mask = np.full((h, w), 0 if kind == "all_zero" else 1, np.uint8)
    kp, _ = check(ms, cuda, oracle, g, mask, nfeatures=600)
    lvl0 = kp[kp[:, 4] == 0]
    assert (mask[lvl0[:, 1].astype(int), lvl0[:, 0].astype(int)] != 0).all()
    if kind == "all_zero":
        assert len(kp) == 0
    elif kind in ("one_and_254", "all_one"):      # non-zero but never 255: level 0 only
        assert len(lvl0) > 50 and len(lvl0) == len(kp)
    else:
        assert len(lvl0) > 20 and len(kp) > len(lvl0)


def raw_orb(ms, gray, mask, desc, nfeatures, max_keypoints=None, **prm_kw):
    """ms_orb_detect_and_compute through the C ABI with caller-made (possibly pitched) tensors"""
    prm = ms.OrbParams()
    ms._chk(ms.load().ms_orb_default_params(C.byref(prm)))
    prm.nfeatures = nfeatures
    for k, v in prm_kw.items():
        setattr(prm, k, v)
    cap = max_keypoints if max_keypoints is not None else nfeatures
    kp = np.zeros((cap, 6), np.float32)
    n = C.c_int(0)
    di = ms.img(desc)
    ms._chk(ms.load().ms_orb_detect_and_compute(C.byref(ms.img(gray)), None if mask is None else C.byref(ms.img(mask)), C.byref(prm),
                                                kp.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(di), C.byref(n), ms._stream()))
    torch.cuda.synchronize()
    return kp[:n.value].copy(), n.value


def test_pitched_image_mask_and_descriptors_equal_the_contiguous_call(ms, cuda, oracle):
    w, h, nf = 301, 233, 500
    g = textured(w, h, 7)
    mask = blob_mask(w, h, 35)
    kp0, d0 = device_orb(ms, cuda, g, mask, nfeatures=nf)
    assert len(kp0) > 100
    same((kp0, d0), oracle_orb(oracle, g, mask, nfeatures=nf))
    wide = torch.from_numpy(noise(w + 90, h, 36)).to(cuda)                 # what surrounds the slice must not be read as image
    wide[:, 37:37 + w] = torch.from_numpy(g).to(cuda)
    gp = wide[:, 37:37 + w]
    wide_m = torch.full((h, w + 13), 255, dtype=torch.uint8, device=cuda)
    wide_m[:, :w] = torch.from_numpy(mask).to(cuda)
    mp = wide_m[:, :w]
    assert gp.stride(0) == w + 90 and mp.stride(0) == w + 13 and gp.data_ptr() % 4 == 1
    kp1, d1 = ms.orb_detect_and_compute(gp, mp, nfeatures=nf)
    assert kp1.tobytes() == kp0.tobytes() and d1.cpu().numpy().tobytes() == d0.tobytes()
    desc_wide = torch.full((nf, 48), 0xAB, dtype=torch.uint8, device=cuda)
    dp = desc_wide[:, 8:40]
    kp2, n2 = raw_orb(ms, gp, mp, dp, nf)
    assert kp2.tobytes() == kp0.tobytes()
    out = desc_wide.cpu().numpy()
    assert out[:n2, 8:40].tobytes() == d0.tobytes()
    assert (out[:, :8] == 0xAB).all() and (out[:, 40:] == 0xAB).all() and (out[n2:] == 0xAB).all(), "bytes outside the descriptor columns / rows were written"


def test_the_single_call_is_the_batch_of_one(ms, cuda):
    """The marshalling of the batch of one -- the mask pointer, the descriptor step, the n_out slot: ms_orb_detect_and_compute through the raw C ABI returns the bytes
    of the same view inside a two-view batch (view 0 pitched, under a grey blob mask; view 1 contiguous, without a mask) and leaves every descriptor byte outside
    its rows and columns as it was."""
    w, h, nf = 301, 233, 500
    grays, mask = [textured(w, h, 7), textured(w, h, 8)], blob_mask(w, h, 35)
    dev = [torch.from_numpy(g).to(cuda) for g in grays]
    want = [(kp, d.cpu().numpy()) for kp, d, _ in ms.orb_detect_and_compute_batch(dev, [torch.from_numpy(mask).to(cuda), None], nfeatures=nf)]
    assert all(len(kp) > 100 for kp, _ in want)
    assert want[0][0].tobytes() != ms.orb_detect_and_compute_batch(dev[:1], nfeatures=nf)[0][0].tobytes(), "the mask must matter"
    wide = torch.from_numpy(noise(w + 90, h, 36)).to(cuda)
    wide[:, 37:37 + w] = dev[0]
    wide_m = torch.full((h, w + 13), 255, dtype=torch.uint8, device=cuda)
    wide_m[:, 5:5 + w] = torch.from_numpy(mask).to(cuda)
    for v, (g, m) in enumerate([(wide[:, 37:37 + w], wide_m[:, 5:5 + w]), (dev[1], None)]):
        wide_d = torch.full((nf + 4, 48 + 16 * v), 0xAB, dtype=torch.uint8, device=cuda)
        kp, n = raw_orb(ms, g, m, wide_d[:, 8:40], nf, max_keypoints=nf + 4)
        out = wide_d.cpu().numpy()
        same((kp, out[:n, 8:40]), want[v], "view %d" % v)
        assert (out[:, :8] == 0xAB).all() and (out[:, 40:] == 0xAB).all() and (out[n:] == 0xAB).all(), "view %d: bytes outside the descriptor columns / rows were written" % v


@pytest.mark.parametrize("size", [(62, 62), (63, 63), (64, 64), (70, 70), (64, 70), (9, 500), (500, 9), (7, 90), (300, 26), (90, 75)])
def test_small_images(ms, cuda, oracle, size):
    """not wider than 2 * edge_threshold: no keypoints; 63 / 64 / 70: an inner rectangle of 1, 2 and 8 pixels; 9 x 500, 300 x 26 and 90 x 75: a dimension
    falls below 8, or below the border, at some level"""
    w, h = size
    g = noise(w, h, 41)
    kp, _ = check(ms, cuda, oracle, g, nfeatures=500)
    if min(size) <= 62:
        assert len(kp) == 0
    if size in ((70, 70), (90, 75)):
        assert len(kp) > 0
    mask = np.full((h, w), 255, np.uint8); mask[::3] = 0
    check(ms, cuda, oracle, g, mask, nfeatures=500)


@pytest.mark.parametrize("size,scale_factor,nlevels", [((517, 389), 1.2, 16), ((300, 220), 1.05, 8), ((300, 220), 1.05, 16), ((300, 220), 1.5, 8), ((300, 220), 2.0, 8),
                                                       ((301, 223), 2.0, 3), ((300, 220), 1.2, 1)])
def test_pyramid_shapes(ms, cuda, oracle, size, scale_factor, nlevels):
    w, h = size
    g = textured(w, h, 9)
    kp, _ = check(ms, cuda, oracle, g, nfeatures=300, scale_factor=scale_factor, nlevels=nlevels)
    usable = [l for l in range(nlevels) if min(R.orb_level_size(w, h, scale_factor, l)) > 62 + 30]
    assert len(kp) > 100 and set(kp[:, 4].astype(int)) >= set(usable), (sorted(set(kp[:, 4].astype(int))), usable)
    for l in set(kp[:, 4].astype(int)):
        assert (kp[kp[:, 4] == l][:, 5] == np.float32(31) * np.float32(float(np.float32(scale_factor)) ** int(l))).all()
    if size != (517, 389):
        check(ms, cuda, oracle, g, blob_mask(w, h, 42), nfeatures=300, scale_factor=scale_factor, nlevels=nlevels)


@pytest.mark.parametrize("nfeatures,scale_factor,nlevels", [(1, 1.2, 8), (2, 1.2, 8), (3, 1.2, 8), (4, 1.2, 8), (5, 1.2, 8), (10, 1.2, 8), (21, 1.2, 8), (50, 1.2, 8),
                                                           (7, 1.2, 8), (5, 1.05, 8), (3, 2.0, 16)])
def test_level_budgets_of_zero_and_below(ms, cuda, oracle, nfeatures, scale_factor, nlevels):
    """A level whose budget is <= 0 contributes nothing and the call succeeds (nfeatures 7 gives the last level -1, (5, 1.05, 8) gives it -2; the
    reference is undefined there).  The image has more corners on every level than any of these budgets."""
    per = oo.n_features_per_level(nfeatures, scale_factor, nlevels)
    if nfeatures != 50:
        assert min(per) <= 0
    g = textured(320, 250, 13)
    kp, _ = check(ms, cuda, oracle, g, nfeatures=nfeatures, scale_factor=scale_factor, nlevels=nlevels)
    got = [int((kp[:, 4] == l).sum()) for l in range(nlevels)]
    sizes = [R.orb_level_size(320, 250, scale_factor, l) for l in range(nlevels)]
    assert got == [max(p, 0) if min(s) > 62 + 30 else got[l] for l, (p, s) in enumerate(zip(per, sizes))], (got, per)
    assert len(kp) <= sum(max(p, 0) for p in per)
    assert len(kp) <= nfeatures + nlevels // 2
    if min(per) < 0:                               # more keypoints than nfeatures: a buffer of nfeatures rows is an argument error, not an overrun
        assert len(kp) > nfeatures
        desc = torch.full((nfeatures + 8, 32), 0xCD, dtype=torch.uint8, device=cuda)
        with pytest.raises(ms.MsError):
            raw_orb(ms, torch.from_numpy(g).to(cuda), None, desc, nfeatures, scale_factor=scale_factor, nlevels=nlevels)
        assert (desc[nfeatures:] == 0xCD).all()


def test_two_calls_give_identical_bytes_in_identical_order(ms, cuda):
    g = torch.from_numpy(textured(640, 360, 17)).to(cuda)
    m = torch.from_numpy(blob_mask(640, 360, 43)).to(cuda)
    for mask, nf in ((None, 2500), (None, 300), (m, 300)):
        kp0, d0 = ms.orb_detect_and_compute(g, mask, nfeatures=nf)
        d0 = d0.cpu().numpy()
        kp1, d1 = ms.orb_detect_and_compute(g, mask, nfeatures=nf)
        assert len(kp0) > 100 and kp0.tobytes() == kp1.tobytes() and d0.tobytes() == d1.cpu().numpy().tobytes()


# ---- ms_feature_mask ------------------------------------------------------------------------------------------------------------------------------------
def feature_mask(ms, img_t, bands, mask_t):
    ms._chk(ms.load().ms_feature_mask(C.byref(ms.img(img_t)), bands[0], bands[1], bands[2], bands[3], C.byref(ms.img(mask_t)), ms._stream()))
    torch.cuda.synchronize()


def bgr_with_black(w, h, seed):
    rng = np.random.default_rng(seed)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    bgr[rng.random((h, w)) < 0.3] = 0                                     # unfilled pixels
    one = rng.random((h, w)) < 0.1                                        # black in two channels only: still "not black"
    bgr[one] = 0
    bgr[one, rng.integers(0, 3, int(one.sum()))] = 1
    return bgr


@pytest.mark.parametrize("size", [(64, 4), (130, 7), (257, 61), (63, 1), (1, 9), (400, 130)])
@pytest.mark.parametrize("bands", [(10, 20, 40, 15), (10, 30, 25, 30), (0, 12, 50, 1000), (-5, 10, 300, 500), (7, 0, 20, 0), (0, 10 ** 6, 3, 2), (20, 5, 25, 5)],
                         ids=["disjoint", "overlapping", "col0_and_past_cols", "negative_x0_and_outside", "empty", "everything", "touching"])
def test_feature_mask_equals_its_definition(ms, cuda, size, bands):
    w, h = size
    bgr = bgr_with_black(w, h, w * 1000 + h)
    want = R.feature_mask(bgr, *bands)
    mask = torch.full((h, w), 7, dtype=torch.uint8, device=cuda)
    feature_mask(ms, torch.from_numpy(bgr).to(cuda), bands, mask)
    assert np.array_equal(mask.cpu().numpy(), want)
    if bands[1] == 0 and bands[3] == 0:
        assert not want.any()
    # pitched image (a column slice of a wider one) and pitched mask: same bytes, nothing outside the mask's columns written
    wide = torch.from_numpy(bgr_with_black(w + 11, h, 5)).to(cuda)
    wide[:, 3:3 + w] = torch.from_numpy(bgr).to(cuda)
    wide_mask = torch.full((h, w + 29), 9, dtype=torch.uint8, device=cuda)
    feature_mask(ms, wide[:, 3:3 + w], bands, wide_mask[:, 5:5 + w])
    out = wide_mask.cpu().numpy()
    assert np.array_equal(out[:, 5:5 + w], want) and (out[:, :5] == 9).all() and (out[:, 5 + w:] == 9).all()


def test_feature_mask_argument_errors(ms, cuda):
    bgr = torch.zeros((8, 16, 3), dtype=torch.uint8, device=cuda)
    mask = torch.zeros((8, 16), dtype=torch.uint8, device=cuda)
    feature_mask(ms, bgr, (0, 4, 8, 4), mask)
    for bad_img, bad_mask in ((bgr, torch.zeros((8, 15), dtype=torch.uint8, device=cuda)), (bgr, torch.zeros((7, 16), dtype=torch.uint8, device=cuda)),
                              (mask, mask), (bgr, bgr), (bgr, torch.zeros((8, 16), dtype=torch.int16, device=cuda))):
        with pytest.raises(ms.MsError):
            feature_mask(ms, bad_img, (0, 4, 8, 4), bad_mask)
    lib = ms.load()
    assert lib.ms_feature_mask(None, 0, 4, 8, 4, C.byref(ms.img(mask)), ms._stream()) < 0
    assert lib.ms_feature_mask(C.byref(ms.img(bgr)), 0, 4, 8, 4, None, ms._stream()) < 0
