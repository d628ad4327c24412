"""Content-aware seams on the GPU: the kernels of csrc/seam_dp.hip through ms_dp_seams, bit for bit against tests/dp_seam_ref.py (integers only: np.array_equal, no
tolerance anywhere) on every case of tests/dp_seam_cases.py, and the context route -- ms_set_seam_finder, ms_calibrate_seam with MS_SEAM_DP against its replay
through the per-op entry points, a twin context handed the masks, and the host app.

Every mask and image lives inside a larger device buffer with guard bytes on both sides, which must come back untouched; images are read only."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import dp_seam_cases as cases
import dp_seam_ref as ref
import lens_ref as L
import synth
from helpers import to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
FILL = 0xA5


class Guarded:
    """arrays packed (contiguous rows: what the entry point requires) into device buffers between two guard zones"""

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


_WANT = {}


def reference(name):
    """(rois, images, masks, the reference's masks), computed once per case and never edited"""
    if name not in _WANT:
        rois, imgs, masks = cases.parallax_scene() if name == "parallax" else cases.case(name)
        _WANT[name] = (rois, imgs, masks, ref.dp_seams(rois, imgs, masks))
    return _WANT[name]


@pytest.mark.parametrize("name", cases.CASES + ["parallax"])
def test_masks_equal_the_reference(ms, cuda, name):
    rois, imgs, masks, want = reference(name)
    di, dm = Guarded(imgs), Guarded(masks)
    ms.dp_seams(rois, di.views, dm.views)
    got = dm.host()
    for v, (g, a) in enumerate(zip(got, want)):
        assert np.array_equal(g, a), "view %d of %s: %d pixels differ from the reference" % (v, name, int((g != a).sum()))
    assert all(np.array_equal(a, b) for a, b in zip(di.host(), imgs)), "the images are read only"
    assert di.guards_intact() and dm.guards_intact()


@pytest.mark.parametrize("name", ["mutual_5/random", "ring_16/plateau", "grey_values/same", "v_1100x70_slabs", "h_i_second"])
def test_a_second_call_on_its_own_output_changes_nothing(ms, cuda, name):
    """behind the first call no pixel of any overlap is set in both masks: B is empty for every pair, and only pixels of B change"""
    rois, imgs, masks, want = reference(name)
    di, dm = Guarded(imgs), Guarded(masks)
    ms.dp_seams(rois, di.views, dm.views)
    ms.dp_seams(rois, di.views, dm.views)
    assert all(np.array_equal(g, a) for g, a in zip(dm.host(), want)) and dm.guards_intact()


def test_two_calls_return_the_same_bytes(ms, cuda):
    rois, imgs, masks, want = reference("mutual_4/plateau")
    a, b, di = Guarded(masks), Guarded(masks), Guarded(imgs)
    ms.dp_seams(rois, di.views, a.views)
    ms.dp_seams(rois, di.views, b.views)
    assert all(np.array_equal(x, y) for x, y in zip(a.host(), b.host()))


def test_padded_rows_are_refused_not_misread(ms, cuda):
    big = torch.full((20, 40), 255, dtype=torch.uint8, device="cuda")
    other = torch.full((20, 30), 255, dtype=torch.uint8, device="cuda")
    img3 = torch.zeros((20, 30, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ms.MsError, match="contiguous"):
        ms.dp_seams([(0, 0, 30, 20), (10, 0, 30, 20)], [img3, img3], [big[:, :30], other])
    assert bool((big == 255).all()) and bool((other == 255).all())


# ---- the context route ------------------------------------------------------------------------------------------------------------------------------------
def mini6_lens_ctx(ms, finder=None):
    """test_lens_gpu's seam-calibration rig: mini6, spherical, BROWN on every view, composed at the original size; (compositor, rig dict, lens, device frames)"""
    cfg = synth.CONFIGS["mini6"]
    n, w, h = cfg["n"], cfg["w"], cfg["h"]
    r = ms.calibrate_cameras(n, w, h, cfg["hfov_deg"], 0.6, 0.01, -1.0)
    assert not r["resize_input"] and r["seam_scale"] < 1
    lens = L.to_ms(ms, L.BROWN)
    comp = ms.Compositor(n, (w, h), ms.PROJ_SPHERICAL, r["compose_warp_scale"], num_bands=3, out_size=(0, 0))
    for i in range(n):
        comp.set_camera(i, r["K_compose"][i], r["R"][i])
        comp.set_lens(i, lens)
    comp.build_maps()
    if finder is not None:
        comp.set_seam_finder(finder)
    return comp, r, lens


_FRAMES = {}


def mini6_frames():
    if not _FRAMES:
        cfg = synth.CONFIGS["mini6"]
        _FRAMES["f"] = [np.clip(synth.frame(cfg["w"], cfg["h"], i, 0, noise=False).astype(np.float32) * (0.9 + 0.04 * i), 0, 255).astype(np.uint8) for i in range(cfg["n"])]
    return _FRAMES["f"]


def calibrate(comp, r, full, dilate):
    return comp.calibrate_seam(full, np.stack(r["K_seam"]), r["seam_scale"], r["seam_warp_scale"], dilate=dilate, estimate_gains=True)


@pytest.mark.parametrize("dilate", [False, True])
def test_calibrate_seam_with_the_dp_finder_equals_its_per_op_replay(ms, cuda, dilate):
    """test_calibrate_seam_on_a_lens_context_equals_its_per_op_replay with MS_SEAM_DP: the replay ends in ms_dp_seams on the warped seam images.  Gains and every
    view's mask, bit for bit."""
    cfg = synth.CONFIGS["mini6"]
    n, w, h = cfg["n"], cfg["w"], cfg["h"]
    comp, r, lens = mini6_lens_ctx(ms, ms.SEAM_DP)
    assert comp.seam_finder() == ms.SEAM_DP
    full = [to_dev(f) for f in mini6_frames()]
    gains = calibrate(comp, r, full, dilate)
    ss, proj = r["seam_scale"], ms.PROJ_SPHERICAL
    rois, imgs, masks = [], [], []
    for i in range(n):
        seam = ms.resize_linear(full[i], fx=ss, fy=ss)
        hs, ws = seam.shape[:2]
        roi = ms.warp_roi_lens(proj, r["K_seam"][i], r["R"][i], lens, r["seam_warp_scale"], ws, hs)
        mx, my = ms.build_warp_maps_lens(proj, roi[0], roi[1], roi[3], roi[2], r["K_seam"][i], r["R"][i], lens, r["seam_warp_scale"])
        rois.append(roi)
        imgs.append(ms.remap(seam, mx, my, ms.INTER_LINEAR, ms.BORDER_REFLECT))
        masks.append(ms.remap(torch.full((hs, ws), 255, dtype=torch.uint8, device="cuda"), mx, my, ms.INTER_NEAREST, ms.BORDER_CONSTANT))
    want_gains, _, _ = ms.estimate_gains(rois, imgs, masks)
    before = [m.clone() for m in masks]
    ms.dp_seams(rois, imgs, masks)
    assert any(not torch.equal(a, b) for a, b in zip(before, masks)), "the seam cut nothing"
    assert np.array_equal(np.asarray(gains), want_gains), (gains, want_gains)
    white = torch.full((h, w), 255, dtype=torch.uint8, device="cuda")
    for i in range(n):
        g = comp.view_geom(i).roi
        small = ms.dilate3x3(masks[i]) if dilate else masks[i]
        big = ms.resize_linear(small, dsize=(g.width, g.height))
        cx, cy = comp.maps(i)
        want = ms.bitwise_and(big, ms.remap(white, cx, cy, ms.INTER_NEAREST, ms.BORDER_CONSTANT))
        assert torch.equal(comp.mask(i), want), i
    comp.init_blender()      # the blender takes these masks
    comp.close()


def test_setter_round_trip_and_refusals(ms, cuda):
    """default Voronoi; DP and back to Voronoi gives the masks of a context that never called the setter; DP's masks are other masks; a bad value is refused and
    leaves the setting alone; build_masks(1) stays Voronoi whatever the setting"""
    full = [to_dev(f) for f in mini6_frames()]
    plain, r, _ = mini6_lens_ctx(ms)
    assert plain.seam_finder() == ms.SEAM_VORONOI
    g_plain = calibrate(plain, r, full, False)
    want = [plain.mask(i) for i in range(plain.n)]
    comp, r, _ = mini6_lens_ctx(ms)
    comp.set_seam_finder(ms.SEAM_DP)
    with pytest.raises(ms.MsError, match="finder 2"):
        comp.set_seam_finder(2)
    assert comp.seam_finder() == ms.SEAM_DP
    g_dp = calibrate(comp, r, full, False)
    dp = [comp.mask(i) for i in range(comp.n)]
    assert any(not torch.equal(a, b) for a, b in zip(dp, want)), "MS_SEAM_DP cut the Voronoi seams"
    assert g_dp == g_plain                                        # the gains are estimated before the seams are cut
    comp.build_masks(1)                                           # no images: Voronoi at compose size, as on the plain context
    plain.build_masks(1)
    assert all(torch.equal(comp.mask(i), plain.mask(i)) for i in range(comp.n))
    comp.set_seam_finder(ms.SEAM_VORONOI)
    assert comp.seam_finder() == ms.SEAM_VORONOI
    calibrate(comp, r, full, False)
    assert all(torch.equal(comp.mask(i), want[i]) for i in range(comp.n))
    comp.close(); plain.close()


def test_a_twin_context_handed_the_dp_masks_stitches_the_same_panorama(ms, cuda):
    """the finder shapes masks and nothing else: context B never hears of it, gets A's masks (ms_get_mask -> ms_set_mask) and gains, and stitches the same 16S bytes"""
    frames = mini6_frames()
    full = [to_dev(f) for f in frames]
    a, r, _ = mini6_lens_ctx(ms, ms.SEAM_DP)
    gains = calibrate(a, r, full, True)
    a.init_blender()
    b, _, _ = mini6_lens_ctx(ms)
    for i in range(a.n):
        b.set_mask(i, a.mask(i).cpu().numpy())
        b.set_gain(i, gains[i])
    b.init_blender()
    outs = []
    for c in (a, b):
        roi = c.pano_geom().dst_roi_final
        o = torch.full((roi.height, roi.width, 3), 11, dtype=torch.int16, device="cuda")
        c.stitch([full], out16s=[o])
        outs.append(o)
    torch.cuda.synchronize()
    assert outs[0].shape == outs[1].shape and torch.equal(outs[0], outs[1]) and bool((outs[0] != 11).any())
    a.close(); b.close()


def test_stitch_app_reference_calib_with_the_dp_finder(ms, cuda):
    exe = os.path.join(ROOT, "video-stitcher_amd", "stitch_app")
    assert os.path.isfile(exe), "stitch_app not built"
    args = [exe, "--size", "480x270", "--frames", "8", "--reference-calib"]
    out = subprocess.run(args + ["--seam-finder", "dp"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["seam_finder"] == "dp" and line["frames"] == 8 and int(line["checksum"], 16) != 0, line
    bad = subprocess.run([exe, "--size", "480x270", "--frames", "8", "--seam-finder", "dp"], capture_output=True, text=True, timeout=120)      # no images without --reference-calib
    assert bad.returncode == 2 and "--reference-calib" in bad.stderr, bad.stderr
