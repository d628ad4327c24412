"""NV12 sources end to end: ms_stitch_nv12_i420, ms_gain_stats_nv12 / ms_track_gains_nv12 and ms_nv12_resize_linear_batch on the device.  Everything is bit-exact:
each entry point is compared with the CPU references (oracle.nv12_to_bgr, oracle.resize_linear_8u, oracle.bgr_to_i420, the oracle blender, tests/gain_ref.py) AND
with the two-step path through the library that it replaces."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import gain_ref as G
import synth
from helpers import host, make_rig, oracle_blender_from, to_dev

pytestmark = pytest.mark.gpu

MS_ERR_INVALID, MS_ERR_UNSUPPORTED, MS_ERR_STATE = -1, -2, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "video-stitcher_amd", "stitch_app")


def _rc(ms, call):
    with pytest.raises(ms.MsError) as e:
        call()
    return int(str(e.value).split()[2].rstrip(":"))


def nv12_noise(rng, w, h):
    return rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)


def nv12_frames(cfg, offset=0):
    """synth.nv12_frame per view; `offset` shifts the view index so that the chroma ramps of neighbouring views differ from another set's"""
    return [synth.nv12_frame(cfg["w"], cfg["h"], i + offset) for i in range(cfg["n"])]


def strided(a, extra, offset=0):
    """the 2-D uint8 array in a device buffer with row step = width + extra, starting `offset` bytes in (address modulo 4 = offset modulo 4)"""
    h, w = a.shape
    step = w + extra
    flat = torch.full((offset + h * step + 64,), 201, dtype=torch.uint8, device="cuda")
    v = flat[offset:offset + h * step].as_strided((h, w), (step, 1))
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    assert v.data_ptr() % 4 == offset % 4 and v.stride(0) == step
    return v


def canvas_of(out16, pg, out_w, out_h):
    ref = np.zeros((out_h, out_w, 3), np.uint8)
    fh, fw = out16.shape[:2]
    x0, y0 = pg.canvas_x, pg.canvas_y
    xs0, ys0 = max(0, -x0), max(0, -y0)
    xs1, ys1 = min(fw, out_w - x0), min(fh, out_h - y0)
    ref[y0 + ys0:y0 + ys1, x0 + xs0:x0 + xs1] = np.clip(out16[ys0:ys1, xs0:xs1], 0, 255).astype(np.uint8)
    return ref


def oracle_i420(O, comp, cfg, gains, nv_np, active, meshes=None):
    """nv12_to_bgr -> the oracle's stitch_online of the active views + blend -> the 8U canvas -> bgr_to_i420 of the ms_get_i420_rows span, all on the CPU"""
    b, _ = oracle_blender_from(O, comp, cfg)
    for i in range(cfg["n"]):
        if (active >> i) & 1:
            xm, ym = [host(t) for t in comp.maps(i)]
            mx, my = meshes[i] if meshes is not None else (None, None)
            b.stitch_online(i, O.nv12_to_bgr(nv_np[i]), xm, ym, gains[i], mx, my)
    out16, _ = b.blend()
    b.close()
    y0, rows = comp.i420_rows()
    return O.bgr_to_i420(np.ascontiguousarray(canvas_of(out16, comp.pano_geom(), cfg["out_w"], cfg["out_h"])[y0:y0 + rows]))


# ---- I420 from NV12 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,proj,cpw,nf,drop", [("mini6", None, False, 1, 0), ("mini6", "cyl", False, 3, 0), ("mini6", None, True, 3, 0), ("mini6", "cyl", True, 1, 0),
                                                  ("mini4", None, False, 33, 0), ("mini6", None, False, 3, 0b010010), ("mini6", None, True, 1, 0b100001)],
                         ids=["sph_1", "cyl_3", "sph_cpw_3", "cyl_cpw_1", "mini4_33", "dropout_3", "dropout_cpw_1"])
def test_i420_from_nv12(ms, cuda, oracle, rig, proj, cpw, nf, drop):
    comp, cfg, gains = make_rig(ms, rig, enable_cpw=cpw, max_frames=nf, projection=ms.PROJ_CYLINDRICAL if proj == "cyl" else None)
    n = cfg["n"]
    meshes = None
    if cpw:
        for i in range(n):
            r = comp.view_geom(i).roi
            comp.set_mesh(i, *synth.mesh(r.width, r.height, 9, 11, phase=0.3 * i, amp=5.0))
        meshes = [[host(t) for t in comp.mesh_maps(i)] for i in range(n)]
    active = ((1 << n) - 1) & ~drop
    if drop:
        comp.set_active_views(active)
    rng = np.random.default_rng(31)
    nv_np = [nv12_frames(cfg)] + [[nv12_noise(rng, cfg["w"], cfg["h"]) for _ in range(n)] for _ in range(nf - 1)]
    nv = [[to_dev(a) if (active >> v) & 1 else None for v, a in enumerate(fr)] for fr in nv_np]
    outs = comp.new_i420(nf)
    comp.stitch_nv12_i420(nv, outs)
    torch.cuda.synchronize()
    assert comp.stitch_kernels()[1 if cpw else 0] == "nv12", comp.stitch_kernels()
    # the two-step path through the library
    canv = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device=cuda) for _ in range(nf)]
    comp.stitch_nv12(nv, out8u=canv)
    y0, rows = comp.i420_rows()
    for f in range(nf):
        want = host(ms.bgr_to_i420(canv[f][y0:y0 + rows]))
        got = host(outs[f])
        assert np.array_equal(got, want), "frame %d differs from stitch_nv12 + bgr_to_i420 at %s" % (f, np.argwhere(got != want)[:5])
    # the oracle, for the first and the last frame of the call
    for f in sorted({0, nf - 1}):
        want = oracle_i420(oracle, comp, cfg, gains, nv_np[f], active, meshes)
        got = host(outs[f])
        assert np.array_equal(got, want), "frame %d differs from the oracle at %s" % (f, np.argwhere(got != want)[:5])
    # outside the panorama the buffers stay black
    pg = comp.pano_geom()
    inside = np.zeros((cfg["out_h"], cfg["out_w"]), bool)
    fh, fw = pg.dst_roi_final.height, pg.dst_roi_final.width
    ys0, xs0 = max(0, -pg.canvas_y), max(0, -pg.canvas_x)
    ys1, xs1 = min(fh, cfg["out_h"] - pg.canvas_y), min(fw, cfg["out_w"] - pg.canvas_x)
    inside[pg.canvas_y + ys0:pg.canvas_y + ys1, pg.canvas_x + xs0:pg.canvas_x + xs1] = True       # (the whole ROI rectangle: pixels of the ROI no view covers are written as black too)
    inside = inside[y0:y0 + rows]
    got = host(outs[0])
    w, flat = cfg["out_w"], host(outs[0]).reshape(-1)
    Y = got[:rows]
    U, V = flat[rows * w:rows * w + rows * w // 4].reshape(rows // 2, w // 2), flat[rows * w + rows * w // 4:].reshape(rows // 2, w // 2)
    assert (~inside).any(), "the canvas has no pixel outside the panorama: nothing to check"
    assert (Y[~inside] == 16).all()
    blk = inside.reshape(rows // 2, 2, -1, 2).any(axis=(1, 3))
    assert (U[~blk] == 128).all() and (V[~blk] == 128).all()
    comp.close()


def test_i420_from_nv12_config_2_at_full_size(ms, cuda):
    comp, cfg, _ = make_rig(ms, "cfg2")
    nv = [[to_dev(a) for a in nv12_frames(cfg)]]
    outs = comp.new_i420(1)
    comp.stitch_nv12_i420(nv, outs)
    canv = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device=cuda)]
    comp.stitch_nv12(nv, out8u=canv)
    bgr = [ms.nv12_to_bgr_batch(nv[0])]
    outs_bgr = comp.new_i420(1)
    comp.stitch_i420(bgr, outs_bgr)
    torch.cuda.synchronize()
    y0, rows = comp.i420_rows()
    assert torch.equal(outs[0], ms.bgr_to_i420(canv[0][y0:y0 + rows]))
    assert torch.equal(outs[0], outs_bgr[0])
    assert int(outs[0][:rows].max()) > 16
    comp.close()


def test_i420_from_nv12_is_refused_where_either_parent_is(ms, cuda):
    cfg = synth.CONFIGS["mini6"]
    nv = [[to_dev(a) for a in nv12_frames(cfg)]]

    def buf(comp, out_w=cfg["out_w"]):
        try:
            return comp.new_i420(1)
        except ms.MsError:
            return [torch.zeros((cfg["out_h"] * 3 // 2, out_w), dtype=torch.uint8, device=cuda)]

    def both_refuse(comp):
        bgr = [ms.nv12_to_bgr_batch(nv[0])]
        rc = _rc(ms, lambda: comp.stitch_nv12_i420(nv, buf(comp)))
        assert ms.load().ms_last_error(), "a refusal carries a message"
        canv = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device=cuda)]
        parents = []
        for call in (lambda: comp.stitch_nv12(nv, out8u=canv), lambda: comp.stitch_i420(bgr, buf(comp))):
            try:
                call()
                parents.append(0)
            except ms.MsError as e:
                parents.append(int(str(e).split()[2].rstrip(":")))
        assert rc != 0 and rc in parents, "refused with %d, the parents say %s" % (rc, parents)
        return rc
    simple, _, _ = make_rig(ms, "mini6", simple_kernels=True)
    assert both_refuse(simple) == MS_ERR_UNSUPPORTED
    simple.close()
    shard, _, _ = make_rig(ms, "mini6", shards=2, shard_index=0)
    assert both_refuse(shard) in (MS_ERR_UNSUPPORTED, MS_ERR_STATE)
    shard.close()
    # 0 bands (FeatherBlender) and an odd panorama width
    for kw, out_w in ((dict(num_bands=0), cfg["out_w"]), (dict(num_bands=cfg["num_bands"]), cfg["out_w"] + 1)):
        c = ms.Compositor(cfg["n"], (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), out_size=(out_w, cfg["out_h"]), **kw)
        for i in range(cfg["n"]):
            c.set_camera(i, *synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i))
        c.build_maps(); c.build_masks(1)
        if kw["num_bands"] == 0:
            c.init_feather()
        else:
            c.init_blender()
        assert _rc(ms, lambda: c.stitch_i420([ms.nv12_to_bgr_batch(nv[0])], buf(c, out_w))) == MS_ERR_UNSUPPORTED
        assert _rc(ms, lambda: c.stitch_nv12_i420(nv, buf(c, out_w))) == MS_ERR_UNSUPPORTED
        c.close()


# ---- statistics from NV12 -----------------------------------------------------------------------------------------------------------------------------------------
def ref_stats_nv12(O, comp, cfg, nv_np, stride, active=None):
    n = cfg["n"]
    rois = [comp.view_geom(i).roi.tuple() for i in range(n)]
    T = comp.pano_geom().dst_roi_final.tuple()
    seen, q = [], []
    for i in range(n):
        xm, ym = [host(t) for t in comp.maps(i)]
        s, v = G.sample_view(xm, ym, O.nv12_to_bgr(nv_np[i]))
        seen.append(s); q.append(v)
    return G.stats(rois, seen, q, T, stride, active)


def sample_parities(comp, cfg, stride):
    """the set of (xx & 1, yy & 1) over the samples of the lattice that some view sees, from the maps alone"""
    T = comp.pano_geom().dst_roi_final.tuple()
    par = set()
    for i in range(cfg["n"]):
        x, y, w, h = comp.view_geom(i).roi.tuple()
        xm, ym = [host(t) for t in comp.maps(i)]
        tx, ty = np.trunc(np.nan_to_num(xm.astype(np.float64))), np.trunc(np.nan_to_num(ym.astype(np.float64)))
        seen = (tx >= 0) & (tx < cfg["w"]) & (ty >= 0) & (ty < cfg["h"])
        uu, vv = np.meshgrid(np.arange(x, x + w), np.arange(y, y + h))
        on = seen & ((uu - T[0]) % stride == 0) & ((vv - T[1]) % stride == 0)
        par |= set(zip((tx[on].astype(int) & 1).tolist(), (ty[on].astype(int) & 1).tolist()))
    return par


@pytest.mark.parametrize("rig,proj", [("mini6", None), ("mini6", "cyl"), ("mini4", None)], ids=["mini6", "mini6_cylindrical", "mini4"])
def test_statistics_from_nv12_are_exact(ms, cuda, oracle, rig, proj):
    comp, cfg, _ = make_rig(ms, rig, projection=ms.PROJ_CYLINDRICAL if proj == "cyl" else None)
    n = cfg["n"]
    nv_np = nv12_frames(cfg, offset=2)
    for a in nv_np:
        uv = a[cfg["h"]:]
        assert uv[:, 0::2].min() != uv[:, 0::2].max() and uv[:, 1::2].min() != uv[:, 1::2].max(), "constant chroma planes would not exercise the chroma addressing"
    assert any(not np.array_equal(nv_np[0][cfg["h"]:], a[cfg["h"]:]) for a in nv_np[1:]), "the views' chroma must differ (per-view offset of synth.nv12_frame)"
    all_ = (1 << n) - 1
    dev_plain = [to_dev(a) for a in nv_np]
    dev_step = [strided(a, 24 + 4 * i, offset=i % 4) for i, a in enumerate(nv_np)]            # row step larger than the width, every address alignment
    for active in (all_, all_ & ~(1 << 2)):
        comp.set_active_views(active)
        for stride in (1, 4, 7):
            rN, rS, cnt = ref_stats_nv12(oracle, comp, cfg, nv_np, stride, active)
            for i in range(n):
                j = (i + 1) % n
                if (active >> i) & (active >> j) & 1:
                    assert cnt[i, j] > 0, "views %d and %d share no sample at stride %d: the comparison would be empty" % (i, j, stride)
            assert sample_parities(comp, cfg, stride) == {(0, 0), (0, 1), (1, 0), (1, 1)}, "the samples must hit all four parities of (xx, yy)"
            for dev in (dev_plain, dev_step):
                views = [d if (active >> v) & 1 else None for v, d in enumerate(dev)]
                N, S = comp.gain_stats_nv12(views, stride)
                assert np.array_equal(N, rN), "N, stride %d, active 0x%x:\n%s\nwant\n%s" % (stride, active, N, rN)
                assert np.array_equal(S, rS), "S, stride %d, active 0x%x:\n%s\nwant\n%s" % (stride, active, S, rS)
            bgr = ms.nv12_to_bgr_batch(dev_plain)
            N2, S2 = comp.gain_stats([b if (active >> v) & 1 else None for v, b in enumerate(bgr)], stride)
            assert np.array_equal(N2, rN) and np.array_equal(S2, rS), "ms_gain_stats on the converted copies"
            if active != all_:
                assert not rN[2].any() and not rN[:, 2].any()
    comp.close()


# ---- tracking from NV12 -------------------------------------------------------------------------------------------------------------------------------------------
def darkened(nv_np, cfg, view, f):
    out = [a.copy() for a in nv_np]
    out[view][:cfg["h"]] = np.clip(np.rint(out[view][:cfg["h"]].astype(np.float64) * f), 0, 255).astype(np.uint8)        # the Y plane only
    return out


def stitch16(comp, cfg, cuda, views):
    pg = comp.pano_geom()
    o16 = [torch.full((pg.dst_roi_final.height, pg.dst_roi_final.width, 3), -7, dtype=torch.int16, device=cuda)]
    comp.stitch([views], out16s=o16)
    torch.cuda.synchronize()
    return host(o16[0])


@pytest.mark.parametrize("simple", [False, True], ids=["tiled", "simple_kernels"])
def test_tracking_from_nv12_equals_tracking_on_the_converted_copies(ms, cuda, oracle, simple):
    a, cfg, g0 = make_rig(ms, "mini6", simple_kernels=simple)
    b, _, _ = make_rig(ms, "mini6", simple_kernels=simple)
    c, _, _ = make_rig(ms, "mini6", simple_kernels=simple)
    sets = [darkened(nv12_frames(cfg, offset=k), cfg, (2 + k) % cfg["n"], 0.7 + 0.05 * k) for k in range(3)]
    steps = [(2, 1.0), (4, 0.25), (1, 0.5)]
    for k, (nv_np, (stride, lam)) in enumerate(zip(sets, steps)):
        nv = [to_dev(x) for x in nv_np]
        bgr = ms.nv12_to_bgr_batch(nv)
        a.track_gains_nv12(nv, stride=stride, smoothing=lam)
        b.track_gains(bgr, stride=stride, smoothing=lam)
        (c.track_gains_nv12 if k % 2 == 0 else c.track_gains)(nv if k % 2 == 0 else bgr, stride=stride, smoothing=lam)      # alternating forms on one context
    ga, gb, gc = a.gains(counters=True), b.gains(counters=True), c.gains(counters=True)
    print("nv12", ga[0], "bgr", gb[0])
    assert np.array_equal(ga[0], gb[0]) and ga[1:] == gb[1:] == (3, 0)
    assert np.array_equal(gc[0], gb[0]) and gc[1:] == (3, 0)
    assert np.abs(ga[0] - np.asarray(g0)).max() > 1e-3, "the gains did not move: the comparison would show nothing"
    frames = [to_dev(synth.frame(cfg["w"], cfg["h"], i, 0)) for i in range(cfg["n"])]
    pa = stitch16(a, cfg, cuda, frames)
    assert np.array_equal(pa, stitch16(b, cfg, cuda, frames)) and np.array_equal(pa, stitch16(c, cfg, cuda, frames))
    for x in (a, b, c):
        x.close()


def test_a_darkened_y_plane_raises_that_views_gain(ms, cuda, oracle):
    comp, cfg, g0 = make_rig(ms, "mini6")
    dim = 3
    nv_np = darkened(nv12_frames(cfg), cfg, dim, 0.7)
    rN, rS, _ = ref_stats_nv12(oracle, comp, cfg, nv_np, 2)
    _, want = G.solve(rN, rS)
    comp.track_gains_nv12([to_dev(x) for x in nv_np], stride=2, smoothing=1.0)
    got = comp.gains()
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
    assert got[dim] > g0[dim] and int(np.argmax(got)) == dim, got
    I = G.intensities(rN, rS)
    assert G.energy(rN, I, got) < G.energy(rN, I, np.asarray(g0, np.float64))
    comp.close()


def test_tracking_from_nv12_errors(ms, cuda):
    comp, cfg, _ = make_rig(ms, "mini6")
    n = cfg["n"]
    nv = [to_dev(a) for a in nv12_frames(cfg)]
    bgr = ms.nv12_to_bgr_batch(nv)
    assert _rc(ms, lambda: comp.track_gains_nv12(nv[:-1] + [bgr[-1]])) == MS_ERR_INVALID              # a BGR image handed to the NV12 call
    assert _rc(ms, lambda: comp.gain_stats_nv12(nv[:-1] + [bgr[-1]], 1)) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.track_gains(bgr[:-1] + [nv[-1]])) == MS_ERR_INVALID                   # ... and the other way round
    short = torch.zeros((cfg["h"] * 3 // 2 - 1, cfg["w"]), dtype=torch.uint8, device=cuda)
    assert _rc(ms, lambda: comp.track_gains_nv12(nv[:-1] + [short])) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.track_gains_nv12(nv[:-1] + [None])) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.track_gains_nv12(nv, stride=0)) == MS_ERR_INVALID
    assert comp.gains(counters=True)[1:] == (0, 0), "a refused call counts nothing"
    comp.close()
    # an odd source size
    ow, oh = 161, 90
    odd = ms.Compositor(n, (ow, oh), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"], out_size=(cfg["out_w"], cfg["out_h"]))
    for i in range(n):
        odd.set_camera(i, *synth.camera(n, ow, oh, cfg["hfov_deg"], i))
    odd.build_maps(); odd.build_masks(1); odd.init_blender()
    planes = [torch.zeros((oh * 3 // 2, ow), dtype=torch.uint8, device=cuda) for _ in range(n)]
    assert _rc(ms, lambda: odd.track_gains_nv12(planes)) == MS_ERR_INVALID
    assert _rc(ms, lambda: odd.gain_stats_nv12(planes, 1)) == MS_ERR_INVALID
    odd.close()
    # before ms_init_blender
    early = ms.Compositor(n, (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"], out_size=(cfg["out_w"], cfg["out_h"]))
    for i in range(n):
        early.set_camera(i, *synth.camera(n, cfg["w"], cfg["h"], cfg["hfov_deg"], i))
    early.build_maps(); early.build_masks(1)
    assert _rc(ms, lambda: early.track_gains_nv12(nv)) == MS_ERR_STATE
    assert _rc(ms, lambda: early.gain_stats_nv12(nv, 1)) == MS_ERR_STATE
    early.close()
    for kw in (dict(shards=2, shard_index=0), dict(col_shards=2, col_shard_index=1)):
        shard, _, _ = make_rig(ms, "mini6", **kw)
        assert _rc(ms, lambda: shard.track_gains_nv12(nv)) == MS_ERR_UNSUPPORTED
        assert _rc(ms, lambda: shard.gain_stats_nv12(nv, 1)) == MS_ERR_UNSUPPORTED
        shard.close()
    fe = ms.Compositor(n, (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=0, out_size=(cfg["out_w"], cfg["out_h"]))
    for i in range(n):
        fe.set_camera(i, *synth.camera(n, cfg["w"], cfg["h"], cfg["hfov_deg"], i))
    fe.build_maps(); fe.build_masks(1); fe.init_feather()
    assert _rc(ms, lambda: fe.track_gains_nv12(nv)) == MS_ERR_UNSUPPORTED
    fe.close()


# ---- fused resize ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_resize(ms, O, srcs_np, srcs_dev, dsize=None, fx=0.0, fy=0.0):
    got = ms.nv12_resize_linear_batch(srcs_dev, dsize=dsize, fx=fx, fy=fy)
    two = ms.resize_linear_batch(ms.nv12_to_bgr_batch(srcs_dev), dsize=dsize, fx=fx, fy=fy)
    torch.cuda.synchronize()
    for i, a in enumerate(srcs_np):
        want = O.resize_linear_8u(O.nv12_to_bgr(a), dsize=dsize, fx=fx, fy=fy)
        g = host(got[i])
        assert g.shape == want.shape
        assert np.array_equal(g, want), "image %d differs from the oracle at %s: got %s want %s" % (i, np.argwhere(g != want)[:5], g[g != want][:5], want[g != want][:5])
        assert np.array_equal(g, host(two[i])), "image %d differs from nv12_to_bgr_batch + resize_linear_batch" % i
    return got


def clamp_counts(cols, rows, dw, dh, fx=None, fy=None):
    """how many output columns / rows take the min(x1 + 1, cols - 1) / min(y1 + 1, rows - 1) clamp, with the kernel's fp32 coordinates"""
    ifx = np.float32(1.0 / (fx if fx else dw / cols)); ify = np.float32(1.0 / (fy if fy else dh / rows))
    x1 = np.floor(np.arange(dw, dtype=np.float32) * ifx).astype(int); y1 = np.floor(np.arange(dh, dtype=np.float32) * ify).astype(int)
    return int((x1 + 1 > cols - 1).sum()), int((y1 + 1 > rows - 1).sum())


def test_fused_resize_shipped_compose_size_both_call_forms(ms, cuda, oracle):
    rig = ms.calibrate_cameras(6, 1920, 1080)
    assert rig["resize_input"] and 1.0 < 1920 / rig["compose_width"] <= 1.6
    rng = np.random.default_rng(2)
    srcs_np = [synth.nv12_frame(1920, 1080, 0), nv12_noise(rng, 1920, 1080)]
    srcs = [to_dev(a) for a in srcs_np]
    a = check_resize(ms, oracle, srcs_np, srcs, fx=rig["compose_scale"], fy=rig["compose_scale"])
    assert tuple(a[0].shape) == (rig["compose_height"], rig["compose_width"], 3)
    b = check_resize(ms, oracle, srcs_np[:1], srcs[:1], dsize=(rig["compose_width"], rig["compose_height"]))
    assert b[0].shape == a[0].shape


@pytest.mark.parametrize("inv", [1.0, 1.25, 1.6, 1.61, 2.5, 0.6], ids=lambda v: "inv_fx_%g" % v)
def test_fused_resize_scales_on_both_sides_of_the_fast_path(ms, cuda, oracle, inv):
    rng = np.random.default_rng(int(inv * 100))
    w, h = 400, 122
    dw, dh = int(round(w / inv)), int(round(h / 1.3))
    if inv == 1.0:
        dw = w                                   # horizontal identity (1 / fx = 1.0 exactly), the rows still shrink
    srcs_np = [nv12_noise(rng, w, h) for _ in range(2)]
    edge = clamp_counts(w, h, dw, dh)
    check_resize(ms, oracle, srcs_np, [to_dev(a) for a in srcs_np], dsize=(dw, dh))
    check_resize(ms, oracle, srcs_np, [strided(a, 36, offset=1) for a in srcs_np], dsize=(dw, dh))          # step > width, odd base address
    check_resize(ms, oracle, srcs_np, [strided(a, 8, offset=2) for a in srcs_np], dsize=(dw, dh))
    if inv == 0.6:
        assert edge[0] > 0, "the upscale must take the right-edge clamp"


def test_fused_resize_takes_the_edge_clamps(ms, cuda, oracle):
    """sizes whose last output column / row sample beyond the last source column / row: x2, y2 are clamped (resize.cu:84-85)"""
    rng = np.random.default_rng(9)
    seen_x = seen_y = 0
    for (w, h), (dw, dh) in (((64, 48), (100, 70)), ((400, 122), (667, 94)), ((130, 50), (131, 77))):
        cx, cy = clamp_counts(w, h, dw, dh)
        seen_x += cx; seen_y += cy
        srcs_np = [nv12_noise(rng, w, h)]
        check_resize(ms, oracle, srcs_np, [to_dev(a) for a in srcs_np], dsize=(dw, dh))
    assert seen_x > 0 and seen_y > 0, "no output pixel took the right-edge / bottom-edge clamp"


@pytest.mark.parametrize("wh,dsize", [((16, 8), (13, 7)), ((18, 10), (15, 8)), ((16, 8), (10, 6)), ((18, 10), (29, 17))], ids=str)
def test_fused_resize_tiny_images(ms, cuda, oracle, wh, dsize):
    rng = np.random.default_rng(wh[0] * 100 + dsize[0])
    srcs_np = [nv12_noise(rng, *wh) for _ in range(3)]
    check_resize(ms, oracle, srcs_np, [to_dev(a) for a in srcs_np], dsize=dsize)
    check_resize(ms, oracle, srcs_np, [strided(a, 5, offset=3) for a in srcs_np], dsize=dsize)


@pytest.mark.parametrize("n", [1, 6, 65])           # 65 = one more than RESIZE_BATCH (prims.hip): two launches
def test_fused_resize_batch_sizes(ms, cuda, oracle, n):
    rng = np.random.default_rng(n)
    srcs_np = [nv12_noise(rng, 96, 54) for _ in range(n)]
    check_resize(ms, oracle, srcs_np, [to_dev(a) for a in srcs_np], fx=0.82, fy=0.82)


def test_fused_resize_every_chroma_pair(ms, cuda, oracle):
    """All 65 536 (U, V) pairs once (the construction of test_nv12_to_bgr_every_chroma_pair), through the fast path and the per-pixel one"""
    U, V = np.meshgrid(np.arange(256), np.arange(256))
    uv = np.empty((256, 512), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = U, V
    for yv in (0, 16, 128, 235, 255):
        Y = np.full((512, 512), yv, np.uint8)
        Y[1::2, 1::2] = (yv + 37) % 256
        src = np.vstack([Y, uv])
        for dsize in ((420, 400), (200, 190)):
            check_resize(ms, oracle, [src], [to_dev(src)], dsize=dsize)


def test_fused_resize_errors(ms, cuda):
    good = to_dev(np.zeros((72, 64), np.uint8))
    dst = lambda h=30, w=40: torch.zeros((h, w, 3), dtype=torch.uint8, device=cuda)

    def call(srcs, dsts, fx=0.0, fy=0.0):
        return _rc(ms, lambda: ms.nv12_resize_linear_batch_prepared(srcs, dsts, fx, fy)())
    assert call([to_dev(np.zeros((72, 63), np.uint8))], [dst()]) == MS_ERR_INVALID                 # odd width
    assert call([to_dev(np.zeros((71, 64), np.uint8))], [dst()]) == MS_ERR_INVALID                 # rows not 3/2 of an even height
    assert call([good, to_dev(np.zeros((72, 66), np.uint8))], [dst(), dst()]) == MS_ERR_INVALID    # mixed geometry
    assert call([good, good], [dst(), dst(31, 40)]) == MS_ERR_INVALID
    assert call([good], [dst(30, 40)], 0.5, 0.5) == MS_ERR_INVALID                                  # fx > 0 form: dst must be 32 x 24
    assert call([good], [dst(48, 64)]) == MS_ERR_INVALID                                            # equal sizes
    assert call([good], [torch.zeros((30, 40), dtype=torch.uint8, device=cuda)]) == MS_ERR_INVALID
    ms.nv12_resize_linear_batch_prepared([good], [dst(24, 32)], 0.5, 0.5)()
    torch.cuda.synchronize()


# ---- host app -----------------------------------------------------------------------------------------------------------------------------------------------------
def run_app(tmp_path, name, extra, dump_flag=None):
    cfg = synth.CONFIGS["mini6"]
    args = [str(a) for a in ["--views", cfg["n"], "--size", "%dx%d" % (cfg["w"], cfg["h"]), "--out", "%dx%d" % (cfg["out_w"], cfg["out_h"]),
                             "--hfov", cfg["hfov_deg"], "--bands", cfg["num_bands"], "--frames", 24]]
    dump = str(tmp_path / (name + ".bin"))
    p = subprocess.run([APP] + args + extra + ([dump_flag, dump] if dump_flag else []), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    info = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])
    return info, (open(dump, "rb").read() if dump_flag else None)


def test_host_app_nv12_direct_i420_in_one_call(cuda, tmp_path):
    one, one_bytes = run_app(tmp_path, "one", ["--nv12-direct", "--i420"], "--dump-i420")
    two, two_bytes = run_app(tmp_path, "two", ["--nv12", "--i420"], "--dump-i420")
    assert one["i420_call"] == "ms_stitch_nv12_i420" and two["i420_call"] == "ms_bgr_to_i420"
    assert len(one_bytes) > 0 and one_bytes == two_bytes
    assert max(one_bytes) > 128
    # a canvas consumer forces the two-step form; the planes are the same
    both, _ = run_app(tmp_path, "both", ["--nv12-direct", "--i420", "--dump-i420", str(tmp_path / "both_i420.bin")], "--dump")
    assert both["i420_call"] == "ms_bgr_to_i420"
    assert open(str(tmp_path / "both_i420.bin"), "rb").read() == one_bytes


def test_host_app_tracks_gains_from_nv12(cuda, tmp_path):
    direct, _ = run_app(tmp_path, "direct", ["--nv12-direct", "--track-gains", "1", "--exposure-ramp", "2:0.7"])
    conv, _ = run_app(tmp_path, "conv", ["--nv12", "--track-gains", "1", "--exposure-ramp", "2:0.7"])
    print("direct", direct["gains"], "converted", conv["gains"])
    assert direct["gains"] == conv["gains"]
    assert direct["gain_solves_ok"] == conv["gain_solves_ok"] == 24 and direct["gain_solves_singular"] == 0
    g = direct["gains"]
    assert all(g[2] > g[v] for v in range(len(g)) if v != 2), g


def test_host_app_resize_path_from_nv12(cuda, tmp_path):
    common = ["--views", "6", "--size", "640x360", "--hfov", "90", "--frames", "6", "--reference-calib", "--compose-megapix", "0.15"]

    def run(name, extra):
        dump = str(tmp_path / (name + ".bin"))
        p = subprocess.run([APP] + common + extra + ["--dump", dump], capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        assert "resized per frame" in p.stderr.decode()
        return json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1]), open(dump, "rb").read()
    conv, conv_bytes = run("conv", ["--nv12"])
    direct, direct_bytes = run("direct", ["--nv12-direct"])
    fused, fused_bytes = run("fused", ["--nv12-direct", "--fused-resize"])
    assert fused["fused_resize"] is True and direct["fused_resize"] is False
    assert conv_bytes == direct_bytes == fused_bytes and max(conv_bytes) > 0
