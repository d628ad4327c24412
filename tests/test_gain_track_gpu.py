"""Exposure tracking (ms_gain_stats / ms_track_gains / ms_get_gains) on the device against tests/gain_ref.py: the overlap statistics integer for integer, the
solve and the smoothing to the rounding of a double, and the published gains bit for bit what ms_set_gain of the same values gives -- through every path that
rebuilds or swaps a view table."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import gain_ref as G
import synth
from helpers import host, make_rig, to_dev, to_dev_roi

pytestmark = pytest.mark.gpu

MS_ERR_INVALID, MS_ERR_UNSUPPORTED, MS_ERR_STATE = -1, -2, -5
STRIDES = (1, 2, 4)


def frames_of(cfg, t=0, scale=None):
    fr = [synth.frame(cfg["w"], cfg["h"], i, t) for i in range(cfg["n"])]
    for v, f in (scale or {}).items():
        fr[v] = np.clip(np.rint(fr[v].astype(np.float64) * f), 0, 255).astype(np.uint8)
    return fr


def ref_stats(comp, cfg, frames_np, stride, active=None):
    """gain_ref's statistics from the context's maps (ms_get_maps), ROIs and pano ROI and the host frames."""
    n = cfg["n"]
    rois = [comp.view_geom(i).roi.tuple() for i in range(n)]
    T = comp.pano_geom().dst_roi_final.tuple()
    seen, q = [], []
    for i in range(n):
        xm, ym = [host(t) for t in comp.maps(i)]
        s, v = G.sample_view(xm, ym, frames_np[i])
        seen.append(s); q.append(v)
    return G.stats(rois, seen, q, T, stride, active)


def adjacent_pairs(n):
    return [(i, (i + 1) % n) for i in range(n)]


def outputs(comp, cfg, cuda, nf=1):
    pg = comp.pano_geom()
    o16 = [torch.full((pg.dst_roi_final.height, pg.dst_roi_final.width, 3), -7, dtype=torch.int16, device=cuda) for _ in range(nf)]
    o8 = [torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device=cuda) for _ in range(nf)]
    return o16, o8


def stitch_np(comp, cfg, cuda, batches_dev, sync=True):
    o16, o8 = outputs(comp, cfg, cuda, len(batches_dev))
    comp.stitch(batches_dev, out8u=o8, out16s=o16)
    if sync:
        torch.cuda.synchronize()
    return o16, o8


def same_outputs(a, b, what):
    for k, (x, y) in enumerate(zip(a[0] + a[1], b[0] + b[1])):
        assert np.array_equal(host(x), host(y)), "%s: output %d differs" % (what, k)


@pytest.mark.parametrize("rig,proj,cpw", [("mini6", None, False), ("mini4", None, False), ("mini6", "cyl", False), ("mini6", None, True)],
                         ids=["mini6", "mini4", "mini6_cylindrical", "mini6_cpw"])
def test_statistics_are_exact(ms, cuda, rig, proj, cpw):
    comp, cfg, _ = make_rig(ms, rig, enable_cpw=cpw, projection=ms.PROJ_CYLINDRICAL if proj == "cyl" else None)
    n = cfg["n"]
    if cpw:     # non-trivial meshes: the statistic ignores them by definition
        for i in range(n):
            r = comp.view_geom(i).roi
            comp.set_mesh(i, *synth.mesh(r.width, r.height, 9, 11, phase=0.3 * i, amp=5.0))
    rng = np.random.default_rng(17)
    frames_np = frames_of(cfg, 2, scale={1: 0.8})
    dev = [to_dev_roi(f, rng) for f in frames_np]
    all_ = (1 << n) - 1
    for active in (all_, all_ & ~(1 << 2)):
        comp.set_active_views(active)
        for stride in STRIDES:
            N, S = comp.gain_stats([d if (active >> v) & 1 else None for v, d in enumerate(dev)], stride)
            rN, rS, cnt = ref_stats(comp, cfg, frames_np, stride, active)
            if stride == max(STRIDES):
                for i, j in adjacent_pairs(n):
                    if (active >> i) & (active >> j) & 1:
                        assert cnt[i, j] > 0, "views %d and %d share no sample at stride %d: the comparison would be empty" % (i, j, stride)
            assert np.array_equal(N, rN), "N, stride %d, active 0x%x:\n%s\nwant\n%s" % (stride, active, N, rN)
            assert np.array_equal(S, rS), "S, stride %d, active 0x%x:\n%s\nwant\n%s" % (stride, active, S, rS)
            if active != all_:
                assert not N[2].any() and not N[:, 2].any() and not S[2].any() and not S[:, 2].any()
    comp.close()


@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_reproducible(ms, cuda, rig):
    comp, cfg, g0 = make_rig(ms, rig)
    dev = [to_dev(f) for f in frames_of(cfg, 1, scale={0: 0.75})]
    a, b = comp.gain_stats(dev, 1), comp.gain_stats(dev, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    comp.track_gains(dev, stride=2, smoothing=1.0)
    first = comp.gains()
    for i in range(cfg["n"]):
        comp.set_gain(i, g0[i])                 # the same state again
    assert np.array_equal(comp.gains(), np.asarray(g0, np.float64))
    comp.track_gains(dev, stride=2, smoothing=1.0)
    assert np.array_equal(comp.gains(), first)
    comp.close()


@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_solve_matches_numpy_and_lowers_the_energy(ms, cuda, rig):
    comp, cfg, g0 = make_rig(ms, rig)
    n, dim = cfg["n"], 2
    frames_np = frames_of(cfg, 0, scale={dim: 0.7})
    dev = [to_dev(f) for f in frames_np]
    N, S = comp.gain_stats(dev, 2)
    rN, rS, _ = ref_stats(comp, cfg, frames_np, 2)
    assert np.array_equal(N, rN) and np.array_equal(S, rS)
    _, want = G.solve(rN, rS)
    comp.track_gains(dev, stride=2, smoothing=1.0)
    got, ok, singular = comp.gains(counters=True)
    print("tracked", got, "numpy", want, "max rel", np.abs(got / want - 1).max())
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
    assert (ok, singular) == (1, 0)
    assert int(np.argmax(got)) == dim, "the dimmed view must get the largest gain: %s" % got
    I = G.intensities(rN, rS)
    e_before, e_after = G.energy(rN, I, np.asarray(g0, np.float64)), G.energy(rN, I, got)
    print("E before", e_before, "after", e_after)
    assert e_after < e_before
    comp.close()


def test_smoothing(ms, cuda):
    comp, cfg, g0 = make_rig(ms, "mini6")
    frames_np = frames_of(cfg, 3, scale={4: 0.7})
    dev = [to_dev(f) for f in frames_np]
    rN, rS, _ = ref_stats(comp, cfg, frames_np, 4)
    _, est = G.solve(rN, rS)
    comp.track_gains(dev, stride=4, smoothing=1.0)
    est_dev = comp.gains()                      # the device's own estimate: the smoothing is checked on its own, to its own rounding
    np.testing.assert_allclose(est_dev, est, rtol=1e-9, atol=0)
    for i in range(cfg["n"]):
        comp.set_gain(i, g0[i])
    comp.track_gains(dev, stride=4, smoothing=0.5)
    comp.track_gains(dev, stride=4, smoothing=0.5)
    got, ok, singular = comp.gains(counters=True)
    want = G.smooth(G.smooth(np.asarray(g0, np.float64), est_dev, 0.5), est_dev, 0.5)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got, g0 + 0.75 * (est_dev - g0), rtol=1e-9, atol=0)
    assert (ok, singular) == (3, 0)
    comp.close()


def fresh_with(ms, rig, gains, **kw):
    comp, cfg, _ = make_rig(ms, rig, **kw)
    for v, g in enumerate(gains):
        comp.set_gain(v, float(g))
    return comp


@pytest.mark.parametrize("simple", [False, True], ids=["tiled", "simple_kernels"])
@pytest.mark.parametrize("nf", [1, 32])
def test_tracked_equals_set(ms, cuda, simple, nf):
    """track_gains, then stitch on the same stream with no synchronisation in between == a fresh context given the same gains with ms_set_gain."""
    comp, cfg, _ = make_rig(ms, "mini6", max_frames=nf, simple_kernels=simple)
    batches = [[to_dev(f) for f in frames_of(cfg, t, scale={3: 0.7})] for t in range(nf)]
    torch.cuda.synchronize()
    comp.track_gains(batches[-1], stride=2, smoothing=1.0)
    got = stitch_np(comp, cfg, cuda, batches, sync=False)
    torch.cuda.synchronize()
    g = comp.gains()
    assert np.abs(g - synth.gains(cfg["n"])).max() > 1e-3, "the gains did not move: the comparison would show nothing"
    ref = fresh_with(ms, "mini6", g, max_frames=nf, simple_kernels=simple)
    same_outputs(got, stitch_np(ref, cfg, cuda, batches), "tracked vs set, %d frames" % nf)
    comp.close(); ref.close()


def test_no_old_gain_comes_back_dropout_and_tables(ms, cuda):
    comp, cfg, g0 = make_rig(ms, "mini6")
    n = cfg["n"]
    all_ = (1 << n) - 1
    frames = [to_dev(f) for f in frames_of(cfg, 0, scale={1: 0.7})]
    # a subset cached BEFORE tracking, one made for the first time AFTER it
    cached, first_time = all_ & ~(1 << 4), all_ & ~(1 << 5)
    comp.set_active_views(cached); comp.set_active_views(all_)
    comp.track_gains(frames, stride=2, smoothing=1.0)
    g = comp.gains()
    ref = fresh_with(ms, "mini6", g)
    want_full = stitch_np(ref, cfg, cuda, [frames])
    for sub in (cached, first_time):
        comp.set_active_views(sub); ref.set_active_views(sub)
        views = [f if (sub >> v) & 1 else None for v, f in enumerate(frames)]
        same_outputs(stitch_np(comp, cfg, cuda, [views]), stitch_np(ref, cfg, cuda, [views]), "subset 0x%x" % sub)
        assert np.array_equal(comp.gains(), g)
        comp.set_active_views(all_); ref.set_active_views(all_)
        same_outputs(stitch_np(comp, cfg, cuda, [frames]), want_full, "restored after 0x%x" % sub)
        assert np.array_equal(comp.gains(), g)
    # (d) an inactive view keeps its gain through a track call; the others move
    comp.set_active_views(cached)
    dimmer = [to_dev(f) for f in frames_of(cfg, 0, scale={1: 0.7, 2: 0.8})]
    comp.track_gains([f if (cached >> v) & 1 else None for v, f in enumerate(dimmer)], stride=2, smoothing=1.0)
    g2 = comp.gains()
    assert g2[4] == g[4] and np.abs(g2 - g).max() > 1e-3
    comp.set_active_views(all_)
    # ms_set_gain after tracking wins for its view, and only for it
    comp.set_gain(0, 1.25)
    g3 = comp.gains()
    assert g3[0] == 1.25 and np.array_equal(g3[1:], g2[1:])
    ref2 = fresh_with(ms, "mini6", g3)
    same_outputs(stitch_np(comp, cfg, cuda, [frames]), stitch_np(ref2, cfg, cuda, [frames]), "set_gain after tracking")
    # (c) ms_save_tables -> ms_load_tables carries the tracked gains
    loaded = ms.Compositor.from_tables(comp.save_tables())
    assert np.array_equal(loaded.gains(), g3) and np.array_equal(comp.gains(), g3)
    same_outputs(stitch_np(loaded, cfg, cuda, [frames]), stitch_np(ref2, cfg, cuda, [frames]), "loaded tables")
    # ms_init_blender again: the rebuilt tables hold the tracked gains
    comp.init_blender()
    assert np.array_equal(comp.gains(), g3)
    same_outputs(stitch_np(comp, cfg, cuda, [frames]), stitch_np(ref2, cfg, cuda, [frames]), "re-initialised")
    for c in (comp, ref, ref2, loaded):
        c.close()


@pytest.mark.parametrize("margin", [0, 16])
def test_no_old_gain_comes_back_update_mask(ms, cuda, margin):
    def rig():
        comp, cfg, _ = make_rig(ms, "mini6", enable_cpw=True, update_mask_margin=margin)
        for i in range(cfg["n"]):
            r = comp.view_geom(i).roi
            comp.set_mesh(i, *synth.mesh(r.width, r.height, 9, 11, phase=0.3 * i, amp=4.0))
        return comp, cfg
    comp, cfg = rig()
    frames = [to_dev(f) for f in frames_of(cfg, 0, scale={5: 0.7})]
    comp.track_gains(frames, stride=2, smoothing=1.0)
    g = comp.gains()
    assert np.abs(g - synth.gains(cfg["n"])).max() > 1e-3
    ref, _ = rig()
    for v in range(cfg["n"]):
        ref.set_gain(v, float(g[v]))
    for view in (1, 4):                  # (with a margin: both copies of the tables get used)
        comp.update_mask(view); ref.update_mask(view)
        assert np.array_equal(comp.gains(), g)
        same_outputs(stitch_np(comp, cfg, cuda, [frames]), stitch_np(ref, cfg, cuda, [frames]), "after update_mask(%d), margin %d" % (view, margin))
    comp.close(); ref.close()


def _rc(ms, call):
    with pytest.raises(ms.MsError) as e:
        call()
    return int(str(e.value).split()[2].rstrip(":"))


def test_errors_and_counters(ms, cuda):
    comp, cfg, _ = make_rig(ms, "mini6")
    n = cfg["n"]
    frames = [to_dev(f) for f in frames_of(cfg)]
    lib = ms.load()
    views = comp._one_frame(frames)
    prm = ms.gain_track_default_params()
    assert lib.ms_track_gains(comp._ctx, views, None, None) == MS_ERR_INVALID
    assert lib.ms_track_gains(comp._ctx, None, C.byref(prm), None) == MS_ERR_INVALID
    bad = ms.gain_track_default_params(); bad.struct_size += 8
    assert lib.ms_track_gains(comp._ctx, views, C.byref(bad), None) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.track_gains(frames, stride=0)) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.gain_stats(frames, 0)) == MS_ERR_INVALID
    for lam in (0.0, -0.5, 1.5, float("nan")):
        assert _rc(ms, lambda: comp.track_gains(frames, smoothing=lam)) == MS_ERR_INVALID
    small = torch.zeros((cfg["h"] - 1, cfg["w"], 3), dtype=torch.uint8, device=cuda)
    assert _rc(ms, lambda: comp.track_gains(frames[:-1] + [small])) == MS_ERR_INVALID
    gray = torch.zeros((cfg["h"], cfg["w"]), dtype=torch.uint8, device=cuda)
    assert _rc(ms, lambda: comp.track_gains(frames[:-1] + [gray])) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.track_gains(frames[:-1] + [None])) == MS_ERR_INVALID       # an ACTIVE view without an image
    assert comp.gains(counters=True)[1:] == (0, 0), "a refused call counts nothing"
    for k in range(3):
        comp.track_gains(frames, stride=4, smoothing=0.25)
    assert comp.gains(counters=True)[1:] == (3, 0)
    comp.close()
    # before ms_init_blender
    early = ms.Compositor(n, (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"], out_size=(cfg["out_w"], cfg["out_h"]))
    for i in range(n):
        early.set_camera(i, *synth.camera(n, cfg["w"], cfg["h"], cfg["hfov_deg"], i))
    early.build_maps(); early.build_masks(1)
    assert _rc(ms, lambda: early.track_gains(frames)) == MS_ERR_STATE
    assert _rc(ms, lambda: early.gain_stats(frames, 1)) == MS_ERR_STATE
    assert _rc(ms, lambda: early.gains()) == MS_ERR_STATE
    early.close()
    # shards and FeatherBlender contexts
    for kw in (dict(shards=2, shard_index=0), dict(col_shards=2, col_shard_index=1)):
        shard, _, _ = make_rig(ms, "mini6", **kw)
        assert _rc(ms, lambda: shard.track_gains(frames)) == MS_ERR_UNSUPPORTED
        assert _rc(ms, lambda: shard.gain_stats(frames, 1)) == MS_ERR_UNSUPPORTED
        shard.close()
    fe = ms.Compositor(n, (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=0, out_size=(cfg["out_w"], cfg["out_h"]))
    for i in range(n):
        fe.set_camera(i, *synth.camera(n, cfg["w"], cfg["h"], cfg["hfov_deg"], i))
    fe.build_maps(); fe.build_masks(1); fe.init_feather()
    assert _rc(ms, lambda: fe.track_gains(frames)) == MS_ERR_UNSUPPORTED
    fe.close()


def test_host_app_tracks_an_exposure_ramp(cuda, tmp_path):
    cfg = synth.CONFIGS["mini6"]
    app = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-stitcher_amd", "stitch_app")
    args = [str(a) for a in ["--views", cfg["n"], "--size", "%dx%d" % (cfg["w"], cfg["h"]), "--out", "%dx%d" % (cfg["out_w"], cfg["out_h"]),
                             "--hfov", cfg["hfov_deg"], "--bands", cfg["num_bands"], "--frames", 40]]

    def run(name, extra):
        dump = str(tmp_path / (name + ".bin"))
        p = subprocess.run([app, "--dump", dump] + args + extra, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        return json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1]), open(dump, "rb").read()
    plain, plain_bytes = run("plain", [])
    off, off_bytes = run("off", ["--track-gains", "0"])
    assert plain_bytes == off_bytes and plain["checksum"] == off["checksum"] and "gains" not in plain and "gains" not in off
    info, _ = run("ramp", ["--track-gains", "1", "--exposure-ramp", "2:0.7"])
    g = info["gains"]
    print("stitch_app gains", g)
    assert info["gain_solves_ok"] == 40 and info["gain_solves_singular"] == 0
    assert all(g[2] > g[v] for v in range(cfg["n"]) if v != 2), g
