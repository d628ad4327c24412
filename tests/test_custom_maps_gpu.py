"""ms_set_maps: a context composites through the CALLER's warp maps (stitch_online's x_maps / y_maps as plain images, APP/timed.cpp:56, :84-90) instead of the
analytic warper's.  The tiled warp kernels then read the dense maps (PROJ_MAPS in tile_kernels.hpp) instead of rebuilding coordinates from the 1-D projection tables.

A. oracle parity on maps no analytic context can produce (rotated + radially distorted + cropped, with NaN / inf / far-out / exact-border entries)
B. every per-frame path, by identity: a custom-maps context fed an analytic context's own maps equals it bit for bit
C. the unaligned tap-read forms (3x minification)
D. last-row safety by value (0xFF behind the image)
E. arguments and state

All integer outputs are compared BIT FOR BIT: the coordinates are data here, so there is no float tolerance anywhere."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import synth
from helpers import host, to_dev, to_dev_roi

pytestmark = pytest.mark.gpu


# ---- rigs -----------------------------------------------------------------------------------------------------
def new_comp(ms, name, src=None, **kw):
    cfg = synth.CONFIGS[name]
    w, h = src if src is not None else (cfg["w"], cfg["h"])
    kw.setdefault("num_bands", cfg["num_bands"])
    return ms.Compositor(cfg["n"], (w, h), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), out_size=(cfg["out_w"], cfg["out_h"]), **kw)


def analytic_rig(ms, name, mask_mode=1, feather=False, **kw):
    """(the few lines of helpers.make_rig this file needs)"""
    cfg = synth.CONFIGS[name]
    comp = new_comp(ms, name, **kw)
    g = synth.gains(cfg["n"])
    for i in range(cfg["n"]):
        K, R = synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i)
        comp.set_camera(i, K, R)
        comp.set_gain(i, g[i])
    comp.build_maps()
    comp.build_masks(mask_mode)
    if feather:
        comp.init_feather(0.02)
    else:
        comp.init_blender()
    return comp, cfg, g


def custom_twin(ms, src_comp, name, rng, feather=False, **kw):
    """A second context of the same configuration that is handed src_comp's own maps, ROIs, masks and gains: the maps as ROI views of larger device
    allocations (row step != 4 * width)."""
    cfg = synth.CONFIGS[name]
    comp = new_comp(ms, name, **kw)
    rois = [src_comp.view_geom(i).roi.tuple() for i in range(cfg["n"])]
    xs, ys = [], []
    for i in range(cfg["n"]):
        xm, ym = src_comp.maps(i)
        xs.append(to_dev_roi(host(xm), rng)); ys.append(to_dev_roi(host(ym), rng))
        assert xs[-1].stride(0) != xs[-1].shape[1]
    comp.set_maps(rois, xs, ys)
    g = synth.gains(cfg["n"])
    for i in range(cfg["n"]):
        comp.set_mask(i, host(src_comp.mask(i)))
        comp.set_gain(i, g[i])
    if feather:
        comp.init_feather(0.02)
    else:
        comp.init_blender()
    return comp


_ANALYTIC_MAPS = {}


def analytic_maps(ms, name):
    """ROIs and dense spherical maps (numpy) of a synth rig, read back from an analytic context once per session"""
    if name not in _ANALYTIC_MAPS:
        cfg = synth.CONFIGS[name]
        comp = new_comp(ms, name)
        for i in range(cfg["n"]):
            comp.set_camera(i, *synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i))
        comp.build_maps()
        rois = [comp.view_geom(i).roi.tuple() for i in range(cfg["n"])]
        maps = [tuple(host(m) for m in comp.maps(i)) for i in range(cfg["n"])]
        comp.close()
        _ANALYTIC_MAPS[name] = (rois, maps)
    return _ANALYTIC_MAPS[name]


def distorted_maps(ms, name, specials=False, scale=1.0):
    """The analytic spherical maps with the (-1, -1) entries kept, everything else rotated by 2 degrees about the principal point and scaled by
    1 - 0.18 r^2 + 0.03 r^4 in normalised coordinates (float32 throughout), cropped by 3 / 4 columns and one row top and bottom; `scale` multiplies
    every coordinate (a larger source).  specials: a handful of seeded entries per view overwritten with NaN, +-inf, +-1e9, exactly w - 1 / h - 1,
    -0.5 and w - 0.5 / h - 0.5."""
    cfg = synth.CONFIGS[name]
    rois, maps = analytic_maps(ms, name)
    f32 = np.float32
    w, h = f32(cfg["w"] * scale), f32(cfg["h"] * scale)
    out_rois, out = [], []
    rng = np.random.default_rng(2718)
    for i, ((x, y, rw, rh), (xm, ym)) in enumerate(zip(rois, maps)):
        K, _ = synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i)
        K = np.asarray(K, f32).reshape(3, 3)
        f, cx, cy = K[0, 0], K[0, 2], K[1, 2]
        keep = (xm == f32(-1)) & (ym == f32(-1))
        xn, yn = (xm - cx) / f, (ym - cy) / f
        c, s = f32(math.cos(math.radians(2.0))), f32(math.sin(math.radians(2.0)))
        xr, yr = c * xn - s * yn, s * xn + c * yn
        r2 = xr * xr + yr * yr
        k = f32(1) - f32(0.18) * r2 + f32(0.03) * r2 * r2
        xd = ((xr * k) * f + cx) * f32(scale)
        yd = ((yr * k) * f + cy) * f32(scale)
        xd[keep] = f32(-1); yd[keep] = f32(-1)
        xd = np.ascontiguousarray(xd[1:-1, 3:-4], f32); yd = np.ascontiguousarray(yd[1:-1, 3:-4], f32)
        assert xd.dtype == f32 and yd.dtype == f32
        if specials:
            vals = [(np.nan, None), (None, np.nan), (np.inf, None), (None, -np.inf), (1e9, None), (None, -1e9), (w - 1, h - 1), (-0.5, -0.5), (w - f32(0.5), h - f32(0.5)),
                    (np.nan, np.nan), (np.inf, np.inf), (w - 1, None), (None, h - 1)]
            hh, ww = xd.shape
            spots = [(0, 0), (hh - 1, ww - 1), (0, ww - 1), (hh - 1, 0)] + [(int(rng.integers(0, hh)), int(rng.integers(0, ww))) for _ in range(2 * len(vals))]
            for j, (py, px) in enumerate(spots):
                vx, vy = vals[j % len(vals)]
                if vx is not None:
                    xd[py, px] = f32(vx)
                if vy is not None:
                    yd[py, px] = f32(vy)
        out_rois.append((x + 3, y + 1, rw - 7, rh - 2))
        out.append((xd, yd))
    # the cropped view widths: over the two rigs every residue modulo the 4 pixels of a lane occurs (1, 2, 0 and 1, 2, 3)
    assert sorted({r[2] for r in out_rois}) == {"mini6": [153, 154, 632], "mini4": [149, 150, 503]}[name], [r[2] for r in out_rois]
    return out_rois, out


def custom_rig(ms, name, rois, maps, masks="ones", src=None, meshes=False, **kw):
    """A context on the caller's maps.  masks: "ones" = all-255 through ms_set_mask; 0 / 1 = ms_build_masks(mode)."""
    cfg = synth.CONFIGS[name]
    comp = new_comp(ms, name, src=src, **kw)
    comp.set_maps(rois, [to_dev(m[0]) for m in maps], [to_dev(m[1]) for m in maps])
    g = synth.gains(cfg["n"])
    for i in range(cfg["n"]):
        comp.set_gain(i, g[i])
        if masks == "ones":
            comp.set_mask(i, np.full((rois[i][3], rois[i][2]), 255, np.uint8))
    if masks != "ones":
        comp.build_masks(masks)
    comp.init_blender()
    mesh_maps = None
    if meshes:
        comp.set_meshes([synth.mesh(r[2], r[3], 10, 12, phase=0.3 * i, amp=4.0) for i, r in enumerate(rois)])
        mesh_maps = [tuple(host(m) for m in comp.mesh_maps(i)) for i in range(cfg["n"])]
    return comp, cfg, g, mesh_maps


def run_oracle(O, comp, cfg, gains, frames_np, mesh_maps=None):
    """Blender.stitch_online x N + blend with the context's stored maps (comp.maps) and masks"""
    rois = [comp.view_geom(i).roi.tuple() for i in range(cfg["n"])]
    b = O.Blender([r[:2] for r in rois], [r[2:] for r in rois], cfg["num_bands"])
    for i in range(cfg["n"]):
        b.init_view(i, host(comp.mask(i)))
    O.lib().orc_trunc_s16_range_reset()
    for i in range(cfg["n"]):
        xm, ym = [host(t) for t in comp.maps(i)]
        mx, my = mesh_maps[i] if mesh_maps is not None else (None, None)
        b.stitch_online(i, frames_np[i], xm, ym, gains[i], mx, my)
    out, mask = b.blend()
    b.close()
    assert O.trunc_s16_range_violations() == 0      # (the oracle's out-of-int16 counter: its float -> short convention is pinned inside the range only)
    return out, mask


def canvas_from(out16, pg, out_w, out_h):
    ref = np.zeros((out_h, out_w, 3), np.uint8)
    fh, fw = out16.shape[:2]
    x0, y0 = pg.canvas_x, pg.canvas_y
    xs0, ys0 = max(0, -x0), max(0, -y0)
    xs1, ys1 = min(fw, out_w - x0), min(fh, out_h - y0)
    ref[y0 + ys0:y0 + ys1, x0 + xs0:x0 + xs1] = np.clip(out16[ys0:ys1, xs0:xs1], 0, 255).astype(np.uint8)
    return ref


def new_outs(comp, cfg, nf, fill16=-7):
    pg = comp.pano_geom()
    return ([torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device="cuda") for _ in range(nf)],
            [torch.full((pg.dst_roi_final.height, pg.dst_roi_final.width, 3), fill16, dtype=torch.int16, device="cuda") for _ in range(nf)])


def assert_same(a, b, what=""):
    for t, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s frame %d differs" % (what, t)


def check_against_oracle(O, comp, cfg, gains, frames_np, mesh_maps=None, frames_dev=None):
    o8, o16 = new_outs(comp, cfg, 1)
    comp.stitch([frames_dev if frames_dev is not None else [to_dev(f) for f in frames_np]], out8u=o8, out16s=o16)
    torch.cuda.synchronize()
    ref16, refmask = run_oracle(O, comp, cfg, gains, frames_np, mesh_maps)
    got16 = host(o16[0])
    assert np.array_equal(host(comp.result_mask()), refmask)
    bad = np.argwhere(got16 != ref16)
    assert bad.size == 0, "first mismatches (y,x,c): %s got %s want %s" % (bad[:5], got16[tuple(bad[:5].T)], ref16[tuple(bad[:5].T)])
    assert np.array_equal(host(o8[0]), canvas_from(ref16, comp.pano_geom(), cfg["out_w"], cfg["out_h"]))
    assert "simple" not in comp.stitch_kernels()
    return o16[0]


# ---- A. oracle parity on maps no analytic context can produce ----------------------------------------------------
@pytest.mark.parametrize("rig", ["mini6", "mini4"])
@pytest.mark.parametrize("cpw", [False, True])
def test_distorted_maps_match_oracle(ms, cuda, oracle, rig, cpw):
    rois, maps = distorted_maps(ms, rig, specials=True)
    arois, _ = analytic_maps(ms, rig)
    assert all(r[:2] != a[:2] and r[2:] != a[2:] for r, a in zip(rois, arois))
    comp, cfg, gains, mesh_maps = custom_rig(ms, rig, rois, maps, enable_cpw=cpw, meshes=cpw)
    assert comp.map_source() == ms.MAPS_CUSTOM
    for i in range(cfg["n"]):      # ms_get_maps returns the stored maps, NaN for NaN; the geometry is the ROIs'
        assert comp.view_geom(i).roi.tuple() == rois[i]
        xm, ym = [host(t) for t in comp.maps(i)]
        assert np.array_equal(xm, maps[i][0], equal_nan=True) and np.array_equal(ym, maps[i][1], equal_nan=True)
    frames_np = [synth.frame(cfg["w"], cfg["h"], i, 0) for i in range(cfg["n"])]
    out = check_against_oracle(oracle, comp, cfg, gains, frames_np, mesh_maps)
    assert int(out.abs().max()) > 0
    comp.close()


@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_masks_from_custom_maps(ms, cuda, oracle, rig):
    """ms_build_masks on the caller's maps: mode 0 = remap(255, NEAREST, BORDER_CONSTANT) pixel for pixel; mode 1 (Voronoi seams) + ms_init_blender + stitch = the oracle
    built from the device masks"""
    rois, maps = distorted_maps(ms, rig)
    comp, cfg, gains, _ = custom_rig(ms, rig, rois, maps, masks=0)
    white = np.full((cfg["h"], cfg["w"]), 255, np.uint8)
    inside = []
    for i in range(cfg["n"]):
        want = oracle.remap_nearest_8uc1(white, maps[i][0], maps[i][1])
        assert np.array_equal(host(comp.mask(i)), want), i
        inside.append(float((want != 0).mean()))
    assert 0.2 < min(inside) < 0.4, inside      # the view that straddles +-pi keeps about 30 % of its pixels inside the source
    comp.build_masks(1)
    comp.init_blender()
    frames_np = [synth.frame(cfg["w"], cfg["h"], i, 1) for i in range(cfg["n"])]
    check_against_oracle(oracle, comp, cfg, gains, frames_np)
    comp.close()


# ---- B. every path, by identity -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair33(ms, cuda):
    a, cfg, _ = analytic_rig(ms, "mini6", max_frames=33)
    b = custom_twin(ms, a, "mini6", np.random.default_rng(5), max_frames=33)
    yield a, b, cfg
    a.close(); b.close()


def frames_for(cfg, nf):
    sets = [[to_dev(synth.frame(cfg["w"], cfg["h"], i, t)) for i in range(cfg["n"])] for t in range(min(nf, 4))]
    return [sets[t % len(sets)] for t in range(nf)]


def laid_out(t_dev, step_extra, offset):
    """the frame in a flat device buffer with row step = w * 3 + step_extra, `offset` bytes in"""
    h, w, _ = t_dev.shape
    step = w * 3 + step_extra
    flat = torch.full((offset + h * step + 64,), 201, dtype=torch.uint8, device="cuda")
    v = flat[offset:offset + h * step].as_strided((h, w, 3), (step, 3, 1))
    v.copy_(t_dev)
    return v


@pytest.mark.parametrize("nf", [1, 2, 3, 33])
def test_identity_stitch(ms, pair33, nf):
    a, b, cfg = pair33
    assert a.map_source() == ms.MAPS_ANALYTIC and b.map_source() == ms.MAPS_CUSTOM
    frames = frames_for(cfg, nf)
    a8, a16 = new_outs(a, cfg, nf)
    b8, b16 = new_outs(b, cfg, nf, fill16=11)
    a.stitch(frames, out8u=a8, out16s=a16)
    b.stitch(frames, out8u=b8, out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16, "16S"); assert_same(a8, b8, "8U")
    assert torch.equal(a.result_mask(), b.result_mask())
    assert int(a16[0].abs().max()) > 0
    assert b.stitch_kernels() == ("shared_aligned", "none") == a.stitch_kernels()


def test_identity_nv12_and_i420(ms, pair33):
    a, b, cfg = pair33
    nf = 3
    nv = [[to_dev(synth.nv12_frame(cfg["w"], cfg["h"], i + t)) for i in range(cfg["n"])] for t in range(nf)]
    frames = frames_for(cfg, nf)
    a8, a16 = new_outs(a, cfg, nf); b8, b16 = new_outs(b, cfg, nf, fill16=11)
    a.stitch_nv12(nv, out8u=a8, out16s=a16); b.stitch_nv12(nv, out8u=b8, out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16, "nv12 16S"); assert_same(a8, b8, "nv12 8U")
    assert b.stitch_kernels() == ("nv12", "none")
    ai, bi = a.new_i420(nf), b.new_i420(nf)
    a.stitch_i420(frames, ai); b.stitch_i420(frames, bi)
    torch.cuda.synchronize()
    assert_same(ai, bi, "i420")
    assert int(ai[0].max()) > 0
    ai, bi = a.new_i420(nf), b.new_i420(nf)
    a.stitch_nv12_i420(nv, ai); b.stitch_nv12_i420(nv, bi)
    torch.cuda.synchronize()
    assert_same(ai, bi, "nv12 -> i420")
    # the NV12 planes at an odd byte offset: the kernel's unaligned-read form
    big = [torch.zeros((cfg["h"] * 3 // 2, cfg["w"] + 64), dtype=torch.uint8, device="cuda") for _ in range(cfg["n"])]
    odd = []
    for i in range(cfg["n"]):
        big[i][:, 33:33 + cfg["w"]] = nv[0][i]
        odd.append(big[i][:, 33:33 + cfg["w"]])
    c8, c16 = new_outs(b, cfg, 1, fill16=11)
    b.stitch_nv12([odd], out8u=c8, out16s=c16)
    torch.cuda.synchronize()
    assert torch.equal(c16[0], a16[0])


def test_identity_frames_with_unequal_pitches(ms, pair33):
    """frames of one view with different row pitches: the per-frame kernels; equal pitches: the shared aligned form; never the reference kernels"""
    a, b, cfg = pair33
    nf = 3
    frames = frames_for(cfg, nf)
    a8, a16 = new_outs(a, cfg, nf)
    a.stitch(frames, out8u=a8, out16s=a16)
    for kind, layout in (("steps", lambda t: (4 * (1 + t), 4 * t)), ("steps_odd", lambda t: (1 + 2 * t, t)), ("offsets", lambda t: (8, t))):
        laid = [[laid_out(f, *layout(t)) for f in fr] for t, fr in enumerate(frames)]
        b8, b16 = new_outs(b, cfg, nf, fill16=11)
        b.stitch(laid, out8u=b8, out16s=b16)
        torch.cuda.synchronize()
        assert_same(a16, b16, kind); assert_same(a8, b8, kind)
        assert b.stitch_kernels() == ("per_frame_aligned", "none"), (kind, b.stitch_kernels())
    b.stitch(frames, out8u=b8, out16s=b16)
    assert b.stitch_kernels() == ("shared_aligned", "none")


def test_identity_active_views(ms, pair33):
    a, b, cfg = pair33
    n = cfg["n"]
    full = (1 << n) - 1
    widths = [a.view_geom(i).roi.width for i in range(n)]
    straddling = int(np.argmax(widths))
    frames = frames_for(cfg, 2)
    for mask in (full & ~1, full & ~(1 << straddling), full):
        a.set_active_views(mask); b.set_active_views(mask)
        a8, a16 = new_outs(a, cfg, 2); b8, b16 = new_outs(b, cfg, 2, fill16=11)
        a.stitch(frames, out8u=a8, out16s=a16); b.stitch(frames, out8u=b8, out16s=b16)
        torch.cuda.synchronize()
        assert_same(a16, b16, "mask %x" % mask); assert_same(a8, b8, "mask %x" % mask)
        assert torch.equal(a.result_mask(), b.result_mask())
        assert "simple" not in b.stitch_kernels()


def test_identity_exposure_tracking(ms, cuda):
    """the statistic's integers and the tracked gains (BGR and NV12 routes read the maps, whatever their source)"""
    a, cfg, _ = analytic_rig(ms, "mini6")
    b = custom_twin(ms, a, "mini6", np.random.default_rng(6))
    fr = [to_dev(np.clip(synth.frame(cfg["w"], cfg["h"], i, 0).astype(np.float32) * (0.8 + 0.08 * i), 0, 255).astype(np.uint8)) for i in range(cfg["n"])]
    nv = [to_dev(synth.nv12_frame(cfg["w"], cfg["h"], i)) for i in range(cfg["n"])]
    for stride in (1, 3):
        Na, Sa = a.gain_stats(fr, stride); Nb, Sb = b.gain_stats(fr, stride)
        assert np.array_equal(Na, Nb) and np.array_equal(Sa, Sb) and Na.sum() > 0
    Na, Sa = a.gain_stats_nv12(nv, 2); Nb, Sb = b.gain_stats_nv12(nv, 2)
    assert np.array_equal(Na, Nb) and np.array_equal(Sa, Sb) and Na.sum() > 0
    for _ in range(2):
        a.track_gains(fr, stride=2, smoothing=0.5); b.track_gains(fr, stride=2, smoothing=0.5)
    a.track_gains_nv12(nv, stride=2, smoothing=0.5); b.track_gains_nv12(nv, stride=2, smoothing=0.5)
    ga, gb = a.gains(), b.gains()
    assert np.array_equal(ga, gb) and not np.array_equal(ga, np.asarray(synth.gains(cfg["n"])))
    a8, a16 = new_outs(a, cfg, 1); b8, b16 = new_outs(b, cfg, 1, fill16=11)
    a.stitch([fr], out16s=a16); b.stitch([fr], out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16)
    a.close(); b.close()


def test_identity_cpw(ms, cuda):
    """CPW: the first remap reads the caller's maps (BGR: k_stage1_s / k_stage1_t; NV12: k_stage1_nv12), the mesh remap the context's stage images"""
    a, cfg, _ = analytic_rig(ms, "mini6", enable_cpw=True, max_frames=3)
    b = custom_twin(ms, a, "mini6", np.random.default_rng(7), enable_cpw=True, max_frames=3)
    meshes = [synth.mesh(a.view_geom(i).roi.width, a.view_geom(i).roi.height, 10, 12, phase=0.3 * i, amp=4.0) for i in range(cfg["n"])]
    a.set_meshes(meshes); b.set_meshes(meshes)
    for i in range(cfg["n"]):
        assert all(np.array_equal(host(x), host(y), equal_nan=True) for x, y in zip(a.mesh_maps(i), b.mesh_maps(i)))      # (NaN = a hole of convertMeshesToMap)
    for nf in (1, 2, 3):
        frames = frames_for(cfg, nf)
        a8, a16 = new_outs(a, cfg, nf); b8, b16 = new_outs(b, cfg, nf, fill16=11)
        a.stitch(frames, out8u=a8, out16s=a16); b.stitch(frames, out8u=b8, out16s=b16)
        torch.cuda.synchronize()
        assert_same(a16, b16, "cpw %d" % nf); assert_same(a8, b8, "cpw %d" % nf)
        assert b.stitch_kernels() == ("shared_aligned", "shared_aligned") == a.stitch_kernels()
    frames = frames_for(cfg, 3)
    laid = [[laid_out(f, 4 * (1 + t), 4 * t) for f in fr] for t, fr in enumerate(frames)]
    b8, b16 = new_outs(b, cfg, 3, fill16=11)
    b.stitch(laid, out8u=b8, out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16, "cpw, unequal pitches")
    assert b.stitch_kernels() == ("shared_aligned", "per_frame_aligned")
    nv = [[to_dev(synth.nv12_frame(cfg["w"], cfg["h"], i + t)) for i in range(cfg["n"])] for t in range(3)]
    a8, a16 = new_outs(a, cfg, 3); b8, b16 = new_outs(b, cfg, 3, fill16=11)
    a.stitch_nv12(nv, out8u=a8, out16s=a16); b.stitch_nv12(nv, out8u=b8, out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16, "cpw nv12"); assert_same(a8, b8, "cpw nv12")
    assert b.stitch_kernels() == ("shared_aligned", "nv12")
    a.close(); b.close()


def test_identity_column_shards(ms, cuda):
    """two column shards on the caller's maps: each equals the unsharded analytic context inside its window"""
    a, cfg, _ = analytic_rig(ms, "mini6", max_frames=2)
    frames = frames_for(cfg, 2)
    a8, a16 = new_outs(a, cfg, 2)
    a.stitch(frames, out8u=a8, out16s=a16)
    pg = a.pano_geom()
    fw, fh = pg.dst_roi_final.width, pg.dst_roi_final.height
    edges = []
    for k in range(2):
        s = custom_twin(ms, a, "mini6", np.random.default_rng(8 + k), max_frames=2, col_shards=2, col_shard_index=k)
        assert s.map_source() == ms.MAPS_CUSTOM
        lo, hi = s.col_window()
        edges.append((lo, hi))
        need = s.needed_views()
        mine = [[fr[v] if (need >> v) & 1 else None for v in range(cfg["n"])] for fr in frames]
        s8, s16 = new_outs(s, cfg, 2, fill16=11)
        s.stitch(mine, out8u=s8, out16s=s16)
        torch.cuda.synchronize()
        r0, r1 = max(pg.canvas_y, 0), min(pg.canvas_y + fh, cfg["out_h"])
        for t in range(2):
            assert torch.equal(s16[t][:, lo:hi], a16[t][:, lo:hi]), (k, t)
            assert torch.equal(s8[t][r0:r1, max(lo + pg.canvas_x, 0):hi + pg.canvas_x], a8[t][r0:r1, max(lo + pg.canvas_x, 0):hi + pg.canvas_x]), (k, t)
        assert "simple" not in s.stitch_kernels()
        s.close()
    assert edges[0][0] == 0 and edges[0][1] == edges[1][0] and edges[1][1] == fw
    a.close()


def test_identity_view_shards(ms, cuda):
    a, cfg, _ = analytic_rig(ms, "mini6", max_frames=2)
    frames = frames_for(cfg, 2)
    a8, a16 = new_outs(a, cfg, 2)
    a.stitch(frames, out8u=a8, out16s=a16)
    comps, parts = [], []
    for k in range(2):
        s = custom_twin(ms, a, "mini6", np.random.default_rng(10 + k), max_frames=2, shards=2, shard_index=k)
        lo, hi = k * cfg["n"] // 2, (k + 1) * cfg["n"] // 2
        mine = [[fr[v] if lo <= v < hi else None for v in range(cfg["n"])] for fr in frames]
        part = torch.full((2 * s.partial_bytes() // 2,), 12345, dtype=torch.int16, device="cuda")
        s.stitch_partial(mine, part)
        comps.append(s); parts.append(part)
    b8, b16 = new_outs(a, cfg, 2, fill16=11)
    comps[0].stitch_finish(2, parts, out8u=b8, out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16, "view shards 16S"); assert_same(a8, b8, "view shards 8U")
    for s in comps:
        s.close()
    a.close()


def test_identity_feather(ms, cuda):
    a, cfg, _ = analytic_rig(ms, "mini4", mask_mode=0, feather=True, num_bands=0, max_frames=2)
    b = custom_twin(ms, a, "mini4", np.random.default_rng(12), feather=True, num_bands=0, max_frames=2)
    frames = frames_for(cfg, 2)
    a8, a16 = new_outs(a, cfg, 2); b8, b16 = new_outs(b, cfg, 2, fill16=11)
    a.stitch(frames, out8u=a8, out16s=a16); b.stitch(frames, out8u=b8, out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16, "feather 16S"); assert_same(a8, b8, "feather 8U")
    assert a.stitch_kernels() == b.stitch_kernels()
    a.close(); b.close()


@pytest.mark.parametrize("knob", ["simple_kernels", "raster", "lds_stage", "cv_remap"])
def test_identity_developer_knobs(ms, cuda, knob):
    """debug_simple_kernels, raster_tile_order, warp_lds_stage = 1 (never stages on the caller's maps) and cpu_flavour_remap"""
    kw = {"simple_kernels": dict(simple_kernels=True), "raster": dict(raster_order=True), "lds_stage": dict(lds_stage=True), "cv_remap": dict(simple_kernels=True, cv_remap=True)}[knob]
    ref_kw = dict(kw) if knob == "cv_remap" else {}      # (cpu_flavour_remap changes results by design: compared with an analytic context that has it too)
    a, cfg, _ = analytic_rig(ms, "mini4", max_frames=3, **ref_kw)
    b = custom_twin(ms, a, "mini4", np.random.default_rng(13), max_frames=3, **kw)
    frames = frames_for(cfg, 3)
    a8, a16 = new_outs(a, cfg, 3); b8, b16 = new_outs(b, cfg, 3, fill16=11)
    a.stitch(frames, out8u=a8, out16s=a16); b.stitch(frames, out8u=b8, out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16, knob); assert_same(a8, b8, knob)
    want = "simple" if "simple_kernels" in kw else "shared_aligned"
    assert b.stitch_kernels()[0] == want, b.stitch_kernels()
    a.close(); b.close()


def test_map_source_follows_the_last_call(ms, cuda):
    a, cfg, _ = analytic_rig(ms, "mini4")
    b = custom_twin(ms, a, "mini4", np.random.default_rng(14))
    assert a.map_source() == ms.MAPS_ANALYTIC and b.map_source() == ms.MAPS_CUSTOM
    frames = frames_for(cfg, 1)
    a8, a16 = new_outs(a, cfg, 1)
    a.stitch(frames, out16s=a16)
    # back to the analytic source: cameras + ms_build_maps
    for i in range(cfg["n"]):
        b.set_camera(i, *synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i))
    b.build_maps()
    assert b.map_source() == ms.MAPS_ANALYTIC
    b.build_masks(1); b.init_blender()
    b8, b16 = new_outs(b, cfg, 1, fill16=11)
    b.stitch(frames, out16s=b16)
    torch.cuda.synchronize()
    assert_same(a16, b16)
    assert len(b.save_tables()) > 0      # (an analytic context again: the blob is allowed)
    # ... and custom again on the same context
    rois, maps = distorted_maps(ms, "mini4")
    b.set_maps(rois, [to_dev(m[0]) for m in maps], [to_dev(m[1]) for m in maps])
    assert b.map_source() == ms.MAPS_CUSTOM and b.view_geom(0).roi.tuple() == rois[0]
    a.close(); b.close()


# ---- C. the unaligned forms ---------------------------------------------------------------------------------------
def test_strong_minification_takes_the_unaligned_forms(ms, cuda, oracle):
    """The distorted maps with every coordinate x 3 on a 960 x 540 source: three source columns per output column, where the plan picks the unaligned 8-byte tap reads.
    With equal row pitches AND equal start alignment the library takes the shared ALIGNED form at every minification (warp_form: measured faster; unchanged here), so the
    shared unaligned form is reached the only way it can be: equal pitches, start addresses that differ modulo 4."""
    rois, maps = distorted_maps(ms, "mini6", scale=3.0)
    W, H = 960, 540
    comp, cfg, gains, _ = custom_rig(ms, "mini6", rois, maps, src=(W, H), max_frames=3)
    sets = [[synth.frame(W, H, i, t) for i in range(cfg["n"])] for t in range(3)]
    # oracle parity, one frame
    o8, o16 = new_outs(comp, cfg, 1)
    comp.stitch([[to_dev(f) for f in sets[0]]], out8u=o8, out16s=o16)
    torch.cuda.synchronize()
    ref16, refmask = run_oracle(oracle, comp, cfg, gains, sets[0])
    assert np.array_equal(host(o16[0]), ref16) and np.array_equal(host(comp.result_mask()), refmask)
    assert np.array_equal(host(o8[0]), canvas_from(ref16, comp.pano_geom(), cfg["out_w"], cfg["out_h"]))
    # three 1-frame calls
    singles = []
    for t in range(3):
        _, s16 = new_outs(comp, cfg, 1)
        comp.stitch([[to_dev(f) for f in sets[t]]], out16s=s16)
        singles.append(s16[0])
    expect = {"uniform": "shared_aligned", "offsets": "shared_unaligned", "steps": "per_frame_unaligned"}
    layouts = {"uniform": lambda t: (0, 0), "offsets": lambda t: (8, t), "steps": lambda t: (4 * (1 + t), 4 * t)}
    for kind in ("uniform", "offsets", "steps"):
        laid = [[laid_out(to_dev(f), *layouts[kind](t)) for f in sets[t]] for t in range(3)]
        _, b16 = new_outs(comp, cfg, 3, fill16=11)
        comp.stitch(laid, out16s=b16)
        torch.cuda.synchronize()
        assert comp.stitch_kernels() == (expect[kind], "none"), (kind, comp.stitch_kernels())
        assert_same(singles, b16, kind)
    assert not torch.equal(singles[0], singles[1])
    comp.close()


# ---- D. last-row safety by value --------------------------------------------------------------------------------
@pytest.mark.parametrize("cpw", [False, True])
def test_last_source_row_and_column_are_read_inside_the_image(ms, cuda, oracle, cpw):
    """A band of 48 rows of view 1's map samples the source's last two rows and, in its right half, the last two columns, at every sub-pixel phase and one step outside.
    The frames are the top-left ROI of larger allocations filled with 0xFF: a tap read that runs past the image -- the aligned 12-byte windows behind the last row --
    would put 255s into the result.  Bit-identical to the oracle, which only ever sees the frame."""
    rois, maps = distorted_maps(ms, "mini6")
    cfg = synth.CONFIGS["mini6"]
    w, h = cfg["w"], cfg["h"]
    xm, ym = maps[1]
    hh, ww = xm.shape
    assert hh >= 64 and ww >= 64
    ph = (np.arange(ww, dtype=np.float32) % 7) / np.float32(4)                     # 0 .. 1.5: inside the last row pair, on the last row, half a pixel outside
    ym[8:56, :] = np.float32(h - 2) + ph[None, :]
    pv = (np.arange(48, dtype=np.float32) % 5) / np.float32(3)
    xm[8:56, ww // 2:] = np.float32(w - 2) + pv[:, None] + np.zeros((1, ww - ww // 2), np.float32)
    comp, cfg, gains, mesh_maps = custom_rig(ms, "mini6", rois, maps, enable_cpw=cpw, meshes=cpw, max_frames=3)
    sets = [[synth.frame(w, h, i, t) for i in range(cfg["n"])] for t in range(3)]

    def in_ff(f):
        big = torch.full((h + 9, w + 23, 3), 255, dtype=torch.uint8, device="cuda")
        big[:h, :w] = to_dev(f)
        return big[:h, :w]
    check_against_oracle(oracle, comp, cfg, gains, sets[0], mesh_maps, frames_dev=[in_ff(f) for f in sets[0]])
    refs = [run_oracle(oracle, comp, cfg, gains, sets[t], mesh_maps)[0] for t in range(3)]
    _, o16 = new_outs(comp, cfg, 3)
    comp.stitch([[in_ff(f) for f in sets[t]] for t in range(3)], out16s=o16)      # three frames per lane: the shared-offset forms
    torch.cuda.synchronize()
    for t in range(3):
        assert np.array_equal(host(o16[t]), refs[t]), t
    assert comp.stitch_kernels()[0] == "shared_aligned"
    comp.close()


# ---- E. arguments and state ------------------------------------------------------------------------------------
def _img(t, **over):
    m = __import__("msstitch").img(t)
    for k, v in over.items():
        setattr(m, k, v)
    return m


def _set_maps_raw(ms, comp, rois, xs, ys):
    n = comp.n
    r = (ms.Rect * n)(*[ms.Rect(*t) for t in rois]) if rois is not None else None
    x = (ms.Image * n)(*xs) if xs is not None else None
    y = (ms.Image * n)(*ys) if ys is not None else None
    rc = ms.load().ms_set_maps(comp._ctx, r, x, y, None)
    return rc, ms.load().ms_last_error().decode()


def test_set_maps_refuses_bad_arguments(ms, cuda):
    n, w, h = 2, 64, 48
    comp = ms.Compositor(n, (w, h), ms.PROJ_SPHERICAL, 50.0, num_bands=2, out_size=(256, 128))
    rois = [(0, 0, 40, 30), (30, 2, 37, 30)]
    xs = [torch.zeros((r[3], r[2]), dtype=torch.float32, device="cuda") for r in rois]
    ys = [torch.zeros((r[3], r[2]), dtype=torch.float32, device="cuda") for r in rois]
    good_x, good_y = [_img(t) for t in xs], [_img(t) for t in ys]
    assert _set_maps_raw(ms, comp, rois, good_x, good_y)[0] == 0
    u8 = torch.zeros((30, 37), dtype=torch.uint8, device="cuda")
    wide = torch.zeros((30, 38), dtype=torch.float32, device="cuda")
    tall = torch.zeros((31, 37), dtype=torch.float32, device="cuda")
    cases = {
        "null rois": (None, good_x, good_y),
        "null xmaps": (rois, None, good_y),
        "null ymaps": (rois, good_x, None),
        "null data": (rois, good_x, [good_y[0], _img(ys[1], data=None)]),
        "other type": (rois, [good_x[0], _img(u8)], good_y),
        "type field": (rois, good_x, [good_y[0], _img(ys[1], type=ms.MS_8UC1)]),
        "wider than the ROI": (rois, [good_x[0], _img(wide)], good_y),
        "taller than the ROI": (rois, good_x, [good_y[0], _img(tall)]),
        "step below the row": (rois, [good_x[0], _img(xs[1], step=37 * 4 - 4)], good_y),
        "step not a multiple of 4": (rois, good_x, [good_y[0], _img(ys[1], step=37 * 4 + 2)]),
        "data not 4-byte aligned": (rois, [_img(xs[0], data=xs[0].data_ptr() + 2), good_x[1]], good_y),
    }
    for name, args in cases.items():
        rc, msg = _set_maps_raw(ms, comp, *args)
        assert rc == -1 and "ms_set_maps" in msg, (name, rc, msg)
    # a refused call leaves the context as it was
    assert comp.map_source() == ms.MAPS_CUSTOM and comp.view_geom(1).roi.tuple() == rois[1]
    comp.close()


@pytest.mark.parametrize("side,size,ok", [("width", 2, False), ("width", 3, True), ("height", 1, False), ("height", 2, True),
                                          ("width", 31744, True), ("width", 31745, False), ("height", 31744, True), ("height", 31745, False)])
def test_set_maps_roi_bounds(ms, cuda, side, size, ok):
    """MS_MAPS_MIN_WIDTH / MS_MAPS_MIN_HEIGHT / MS_MAPS_MAX_SIDE, at and just outside"""
    assert (ms.MAPS_MIN_WIDTH, ms.MAPS_MIN_HEIGHT, ms.MAPS_MAX_SIDE) == (3, 2, 31744)
    comp = ms.Compositor(2, (64, 48), ms.PROJ_SPHERICAL, 50.0, num_bands=2, out_size=(256, 128))
    rw, rh = (size, 4) if side == "width" else (5, size)
    rois = [(0, 0, 40, 30), (7, 3, rw, rh)]
    xs = [torch.zeros((r[3], r[2]), dtype=torch.float32, device="cuda") for r in rois]
    rc, msg = _set_maps_raw(ms, comp, rois, [_img(t) for t in xs], [_img(t) for t in xs])
    assert rc == (0 if ok else -1), (rc, msg)
    if not ok:
        assert "ms_set_maps" in msg and str(size) in msg
        with pytest.raises(ms.MsError):
            comp.pano_geom()      # (no maps were set)
    comp.close()


@pytest.mark.parametrize("shape", ["3x2", "31744x2"])
def test_views_at_the_size_limits_match_oracle(ms, cuda, oracle, shape):
    """a view of 3 x 2 pixels beside an ordinary one, and two views of 31744 x 2: the tiled kernels, bit-identical to the oracle"""
    n, w, h = 2, 64, 48
    rng = np.random.default_rng(31)
    if shape == "3x2":
        rois = [(0, 0, 70, 40), (33, 17, 3, 2)]
    else:
        rois = [(0, 0, 31744, 2), (5, 1, 31744, 2)]
    maps = []
    for (_, _, rw, rh) in rois:
        xm = (np.linspace(-3.0, w + 2.0, rw, dtype=np.float32)[None, :] + rng.uniform(-0.5, 0.5, (rh, rw)).astype(np.float32)).astype(np.float32)
        ym = (np.linspace(2.0, h - 3.0, rh, dtype=np.float32)[:, None] + rng.uniform(-4, 4, (rh, rw)).astype(np.float32)).astype(np.float32)
        maps.append((xm, ym))
    pano_w = max(r[0] + r[2] for r in rois)
    cfg = dict(n=n, w=w, h=h, num_bands=3, out_w=(pano_w + 15) // 16 * 16, out_h=64)
    comp = ms.Compositor(n, (w, h), ms.PROJ_SPHERICAL, 50.0, num_bands=3, out_size=(cfg["out_w"], cfg["out_h"]))
    comp.set_maps(rois, [to_dev(m[0]) for m in maps], [to_dev(m[1]) for m in maps])
    gains = [0.97, 1.05]
    for i in range(n):
        comp.set_gain(i, gains[i])
        comp.set_mask(i, np.full((rois[i][3], rois[i][2]), 255, np.uint8))
    comp.init_blender()
    cfg["num_bands"] = comp.pano_geom().num_bands
    frames_np = [synth.frame(w, h, i, 0) for i in range(n)]
    check_against_oracle(oracle, comp, cfg, gains, frames_np)
    comp.close()


def test_state_and_unsupported_calls(ms, cuda):
    rois, maps = distorted_maps(ms, "mini4")
    cfg = synth.CONFIGS["mini4"]
    comp = new_comp(ms, "mini4")
    lib = ms.load()
    xs, ys = [to_dev(m[0]) for m in maps], [to_dev(m[1]) for m in maps]
    comp.set_maps(rois, xs, ys)
    # the maps are copied: freed and overwritten right after the call
    for t in xs + ys:
        t.fill_(float("nan"))
    del xs, ys
    torch.cuda.empty_cache()
    scribble = torch.full((1 << 20,), -12345.0, dtype=torch.float32, device="cuda")
    frames = [to_dev(synth.frame(cfg["w"], cfg["h"], i, 0)) for i in range(cfg["n"])]
    o8, o16 = new_outs(comp, cfg, 1)
    views = (ms.Image * cfg["n"])(*[ms.img(t) for t in frames])
    out = (ms.Image * 1)(ms.img(o16[0]))
    assert lib.ms_stitch(comp._ctx, 1, views, None, out, None) == -5      # MS_ERR_STATE: before ms_init_blender
    # ms_calibrate_seam re-warps from cameras: MS_ERR_UNSUPPORTED
    prm = ms.SeamParams(0.5, 40.0, 0, 1)
    K = (C.c_float * (9 * cfg["n"]))(*([1.0] * (9 * cfg["n"])))
    assert lib.ms_calibrate_seam(comp._ctx, views, K, C.byref(prm), None, None) == -2
    assert "ms_set_maps" in lib.ms_last_error().decode()
    g = synth.gains(cfg["n"])
    for i in range(cfg["n"]):
        comp.set_mask(i, np.full((rois[i][3], rois[i][2]), 255, np.uint8)); comp.set_gain(i, g[i])
    comp.init_blender()
    nbytes = C.c_size_t(0)
    assert lib.ms_save_tables(comp._ctx, None, C.c_size_t(0), C.byref(nbytes)) == -2      # the blob replays cameras
    assert "ms_set_maps" in lib.ms_last_error().decode()
    comp.stitch([frames], out16s=o16)
    torch.cuda.synchronize()
    # the same maps in a fresh context, kept alive: same result
    comp2, _, _, _ = custom_rig(ms, "mini4", rois, maps)
    _, p16 = new_outs(comp2, cfg, 1, fill16=11)
    comp2.stitch([frames], out16s=p16)
    torch.cuda.synchronize()
    assert torch.equal(o16[0], p16[0]) and int(o16[0].abs().max()) > 0
    for i in range(cfg["n"]):
        assert np.array_equal(host(comp.maps(i)[0]), maps[i][0]) and np.array_equal(host(comp.maps(i)[1]), maps[i][1])
    assert float(scribble[0]) == -12345.0
    comp.close(); comp2.close()
