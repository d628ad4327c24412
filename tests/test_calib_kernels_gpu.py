"""The calibration kernels of csrc/calib.hip, per op and bit for bit: k_vor_cols / k_vor_rows through ms_voronoi_seams, k_gain_pairs / k_gain_solve through
ms_estimate_gains, against BOTH references -- the C oracle and tests/np_ref.py -- on the inputs of tests/calib_cases.py, on which
tests/test_np_ref_crosscheck.py shows (without a GPU) that the two references agree.  Library and oracle are built with -ffp-contract=off, so every comparison
is np.array_equal: no tolerance anywhere in this file.

What the pipeline tests (ms_build_masks, ms_calibrate_seam at rtol 2e-3) cannot see and these can: masks with holes, grey values and views without a pixel of
their own; windows on either side of the kernels' 64-lane blocks; distance ties; more than three mutually overlapping views chained through the in-place edit;
every branch of the solve (closed forms for 1, 2, 3 views, LU above, LU with a row exchange); the last bit of the raster-order double sums.

Every mask and image lives inside a larger device buffer with guard bytes on both sides, which must come back untouched.

Out of scope here: the singular exit of the solve.  Every N[i][i] >= 1 puts at least beta = 100 on every diagonal entry and the off-diagonal terms cannot
cancel it, so no input of this entry point reaches it; tests/test_gain_track_sharded_gpu.py covers ok = 0 of the shared gain_solve."""
import numpy as np
import pytest
import torch

import calib_cases
import np_ref

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


class Guarded:
    """arrays packed (contiguous rows: what the entry points require) into device buffers between two guard zones"""

    def __init__(self, arrays):
        self.bufs, self.views = [], []
        for a in arrays:
            buf = torch.full((GUARD + a.size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            buf[GUARD:GUARD + a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
            self.bufs.append(buf)
            self.views.append(buf[GUARD:GUARD + a.size].view(a.shape))

    def host(self):
        return [v.cpu().numpy() for v in self.views]

    def guards_intact(self):
        return all(bool((b[:GUARD] == FILL).all()) and bool((b[-GUARD:] == FILL).all()) for b in self.bufs)


def voronoi_refs(oracle, name):
    """(rois, input masks, oracle's result, np_ref's result)"""
    rois, masks = calib_cases.voronoi_case(name)
    corners = [r[:2] for r in rois]
    return rois, masks, oracle.voronoi_seams(corners, [m.copy() for m in masks]), np_ref.voronoi_seams(corners, [m.copy() for m in masks])


def gain_refs(oracle, name):
    rois, imgs, masks = calib_cases.gain_case(name)
    corners = [r[:2] for r in rois]
    return rois, imgs, masks, np.array(oracle.gain_compensator(corners, imgs, masks), np.float64), np_ref.gain_compensator(corners, imgs, masks)


@pytest.mark.parametrize("name", calib_cases.VORONOI_CASES)
def test_voronoi_seams(ms, cuda, oracle, name):
    rois, masks, want_c, want_np = voronoi_refs(oracle, name)
    dev = Guarded(masks)
    ms.voronoi_seams(rois, dev.views)
    got = dev.host()
    for v, (g, a, b, m) in enumerate(zip(got, want_c, want_np, masks)):
        assert np.array_equal(a, b), "view %d: the references disagree" % v
        assert np.array_equal(g, a), "view %d of %s: %d pixels differ from the references" % (v, name, int((g != a).sum()))
        assert set(np.unique(g)) <= set(np.unique(m)) | {0}                          # a seam only clears
        if name in calib_cases.VORONOI_UNTOUCHED:
            assert np.array_equal(g, m), "view %d: no pair overlaps, the mask must come back as it went in" % v
    assert dev.guards_intact()
    if name == "nounique_both":             # neither view has a pixel of its own in the window: view i loses the whole overlap, view j keeps it
        assert not got[0].any() and got[1].all()


def test_voronoi_seams_twice_is_stable(ms, cuda, oracle):
    """the second run starts from the first one's masks: nothing is contested any more, and whatever the kernels still clear the references clear too"""
    rois, masks, want_c, _ = voronoi_refs(oracle, "mutual_4")
    dev = Guarded(masks)
    ms.voronoi_seams(rois, dev.views)
    ms.voronoi_seams(rois, dev.views)
    again = oracle.voronoi_seams([r[:2] for r in rois], [m.copy() for m in want_c])
    assert all(np.array_equal(g, a) for g, a in zip(dev.host(), again)) and dev.guards_intact()


@pytest.mark.parametrize("name", calib_cases.GAIN_CASES)
def test_estimate_gains(ms, cuda, oracle, name):
    rois, imgs, masks, want_c, (want_np, N_ref, I_ref, swaps) = gain_refs(oracle, name)
    di, dm = Guarded(imgs), Guarded(masks)
    g, N, I = ms.estimate_gains(rois, di.views, dm.views)
    n = len(rois)
    # the statistics first: a last-bit mismatch of the gains is then the solve's
    assert N.shape == (n, n) and np.array_equal(N, N_ref), "overlap counts differ"
    assert np.array_equal(I, I_ref), "mean intensities differ (raster-order double sums)"
    assert np.array_equal(want_c, want_np), "the references disagree"
    assert np.array_equal(g, want_np), "gains differ from np_ref: %r vs %r" % (g.tolist(), want_np.tolist())
    assert np.array_equal(g, want_c), "gains differ from the oracle"
    assert (swaps > 0) == (name in calib_cases.GAIN_ROW_SWAP_CASES), "the case no longer covers the branch its name says"
    assert all(np.array_equal(a, b) for a, b in zip(di.host() + dm.host(), imgs + masks)) and di.guards_intact() and dm.guards_intact()      # inputs are read only


def test_estimate_gains_without_the_statistics(ms, cuda, oracle):
    """N_host and I_host are optional: the gains alone are the same doubles"""
    import ctypes as C
    rois, imgs, masks, want_c, _ = gain_refs(oracle, "views_5")
    di, dm = Guarded(imgs), Guarded(masks)
    n = len(rois)
    g = np.zeros(n)
    a = (ms.Image * n)(*[ms.img(t) for t in di.views]); m = (ms.Image * n)(*[ms.img(t) for t in dm.views])
    r = (ms.Rect * n)(*[ms.Rect(*x) for x in rois])
    ms._chk(ms.load().ms_estimate_gains(n, r, a, m, g.ctypes.data_as(C.POINTER(C.c_double)), None, None, ms._stream()))
    assert np.array_equal(g, want_c)


def test_padded_rows_are_refused_not_misread(ms, cuda):
    """a mask whose rows are not back to back (a slice of a wider buffer) is MS_ERR_INVALID and is left as it is"""
    big = torch.full((20, 40), 255, dtype=torch.uint8, device="cuda")
    other = torch.full((20, 30), 255, dtype=torch.uint8, device="cuda")
    rois = [(0, 0, 30, 20), (10, 0, 30, 20)]
    with pytest.raises(ms.MsError, match="contiguous"):
        ms.voronoi_seams(rois, [big[:, :30], other])
    assert bool((big == 255).all()) and bool((other == 255).all())
    img3 = torch.zeros((20, 30, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ms.MsError, match="contiguous"):
        ms.estimate_gains(rois, [img3, img3], [big[:, :30], other])
