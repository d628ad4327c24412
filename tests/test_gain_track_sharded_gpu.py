"""Exposure tracking on column shards (ms_gain_stats_partial / ms_track_gains_from_partials / ms_get_gain_views / ms_dist_track_gains) on the device, through the
C-ABI: the shards' partial statistics are the numpy restatement (tests/gain_partial_ref.py) integer for integer and add up to ms_gain_stats of an unsharded
context; every shard reaches the gains of ms_track_gains as float64 bit patterns and the unsharded panorama on its window; mismatching partials change nothing;
no path brings an older gain back; ranks of a column group agree over both transports; and a stitching thread never sees a torn update."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest
import torch

import gain_partial_ref as P
import gain_ref as G
import synth
from helpers import host, make_rig, to_dev, to_dev_roi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "video-stitcher_amd", "stitch_dist")
FAKE_RCCL = os.path.join(ROOT, "tests", "_fake_rccl", "libfake_rccl.so")
MS_ERR_INVALID, MS_ERR_UNSUPPORTED, MS_ERR_STATE = -1, -2, -5


def frames_of(cfg, t=0, scale=None):
    fr = [synth.frame(cfg["w"], cfg["h"], i, t) for i in range(cfg["n"])]
    for v, f in (scale or {}).items():
        fr[v] = np.clip(np.rint(fr[v].astype(np.float64) * f), 0, 255).astype(np.uint8)
    return fr


def geometry(comp, cfg):
    n = cfg["n"]
    rois = [comp.view_geom(i).roi.tuple() for i in range(n)]
    T = comp.pano_geom().dst_roi_final.tuple()
    maps = [[host(t) for t in comp.maps(i)] for i in range(n)]
    return rois, T, maps


def sampled(maps, frames_np):
    seen, q = zip(*[G.sample_view(xm, ym, f) for (xm, ym), f in zip(maps, frames_np)])
    return list(seen), list(q)


def only(frames, mask):
    return [f if (mask >> v) & 1 else None for v, f in enumerate(frames)]


def shards_of(ms, rig, S, **kw):
    return [make_rig(ms, rig, col_shards=S, col_shard_index=k, **kw)[0] for k in range(S)] if S > 1 else [make_rig(ms, rig, **kw)[0]]


def outputs(comp, cfg, cuda):
    pg = comp.pano_geom()
    return (torch.full((pg.dst_roi_final.height, pg.dst_roi_final.width, 3), -7, dtype=torch.int16, device=cuda),
            torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device=cuda))


def stitch16(comp, cfg, cuda, frames):
    o16, _ = outputs(comp, cfg, cuda)
    comp.stitch([frames], out16s=[o16])
    torch.cuda.synchronize()
    return host(o16)


def bits(g):
    return np.asarray(g, np.float64).view(np.uint64)


def track_group(shards, frames, stride, smoothing, nv12=False):
    """One tracking step of a column group on one GPU: every shard's partial (only the views ms_get_gain_views names), then every shard solves over all of them."""
    parts = [s.gain_stats_partial(only(frames, s.gain_views()), stride, nv12=nv12) for s in shards]
    for s in shards:
        s.track_gains_from_partials(parts, stride=stride, smoothing=smoothing)
    return parts


# ---- 1. partition --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_partials_partition_the_unsharded_statistic(ms, cuda, rig):
    comp, cfg, _ = make_rig(ms, rig)
    n = cfg["n"]
    rois, T, maps = geometry(comp, cfg)
    rng = np.random.default_rng(23)
    bgr_np = frames_of(cfg, 2, scale={1: 0.8})
    nv_np = [synth.nv12_frame(cfg["w"], cfg["h"], i) for i in range(n)]
    nv_dev = [to_dev(f) for f in nv_np]
    nv_as_bgr = [host(t) for t in ms.nv12_to_bgr_batch(nv_dev)]
    cases = {False: ([to_dev_roi(f, rng) for f in bgr_np], sampled(maps, bgr_np)), True: ([to_dev_roi(f, rng) for f in nv_np], sampled(maps, nv_as_bgr))}
    for S in (1, 2, 3, 4):
        shards = shards_of(ms, rig, S)
        windows = P.col_windows(T[2], S)
        assert [s.col_window() for s in shards] == windows
        for nv12, (dev, (seen, q)) in cases.items():
            for stride in (1, 4):
                want_N, want_S = (comp.gain_stats_nv12 if nv12 else comp.gain_stats)(dev, stride)
                csum, ssum = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
                for k, s in enumerate(shards):
                    hdr, cnt, Sm = ms.parse_gain_partial(s.gain_stats_partial(dev, stride, nv12=nv12), n)
                    torch.cuda.synchronize()
                    assert hdr == {"magic": ms.GAIN_PARTIAL_MAGIC, "num_views": n, "active": (1 << n) - 1, "stride": stride, "T": T}, hdr
                    rc, rs = P.window_stats(rois, seen, q, T, stride, windows[k])
                    assert np.array_equal(cnt, rc), "cnt of shard %d/%d, stride %d, nv12 %s:\n%s\nwant\n%s" % (k, S, stride, nv12, cnt, rc)
                    assert np.array_equal(Sm, rs), "S of shard %d/%d, stride %d, nv12 %s" % (k, S, stride, nv12)
                    if S >= 2:      # the condition of the test: a sum of partials without pair samples would prove nothing
                        assert P.has_cross_pair(cnt), "shard %d/%d holds no pair of different views with samples at stride %d" % (k, S, stride)
                    csum += cnt; ssum += Sm
                got_N, got_S = P.finish(rois, csum, ssum)
                assert np.array_equal(got_N, want_N) and np.array_equal(got_S, want_S), "sum of %d partials, stride %d, nv12 %s" % (S, stride, nv12)
        for s in shards:
            s.close()
    comp.close()


# ---- 2. views read -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_views_outside_the_gain_views_are_never_read(ms, cuda, rig):
    cfg = synth.CONFIGS[rig]
    n = cfg["n"]
    frames = [to_dev(f) for f in frames_of(cfg, 1)]
    zero = ms.Image()
    for S in (2, 3, 4):
        for active in ((1 << n) - 1, ((1 << n) - 1) & ~(1 << 1)):
            for k, s in enumerate(shards_of(ms, rig, S)):
                s.set_active_views(active)
                rois, T, _ = geometry(s, cfg)
                gv, need, reads = s.gain_views(), s.needed_views(), P.window_views(rois, T, s.col_window(), active)
                print("%s S=%d shard %d active 0x%x: gain_views 0x%x needed 0x%x roi-meets-window 0x%x (alone a superset of needed: %s)" % (rig, S, k, active, gv, need, reads, need & ~reads == 0))
                assert gv & ~active == 0
                assert need & ~gv == 0, "ms_get_gain_views 0x%x lacks views ms_stitch reads (0x%x)" % (gv, need)
                assert reads & ~gv == 0 and gv == reads | need
                full = s.gain_stats_partial(only(frames, active), 2)
                views = s._one_frame(only(frames, active))
                for v in range(n):
                    if not (reads >> v) & 1:
                        views[v] = zero                   # an all-zero ms_image for every view the statistic does not read ("these, and no others, are read")
                lean = s.new_gain_partial()
                assert ms.load().ms_gain_stats_partial(s._ctx, views, 2, ms.C.c_void_p(lean.data_ptr()), ms._stream()) == 0
                torch.cuda.synchronize()
                assert torch.equal(full, lean), "shard %d/%d: the partial changed when the views outside 0x%x were withheld" % (k, S, reads)
                if active == (1 << n) - 1:
                    assert P.has_cross_pair(ms.parse_gain_partial(full, n)[1]), "an empty partial would show nothing"
                s.close()


# ---- 3. gains ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", [False, True], ids=["all_views", "subset"])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("S", [2, 3])
def test_every_shard_reaches_the_unsharded_gains_bit_for_bit(ms, cuda, S, steps, subset):
    comp, cfg, g0 = make_rig(ms, "mini6")
    n = cfg["n"]
    active = ((1 << n) - 1) & ~(1 << 4) if subset else (1 << n) - 1
    shards = shards_of(ms, "mini6", S)
    route = make_rig(ms, "mini6")[0]                        # an unsharded context on the partial route: one partial
    for c in [comp, route] + shards:
        c.set_active_views(active)
    for t in range(steps):                                  # drifting frames: another view dims at every step
        frames = [to_dev(f) for f in frames_of(cfg, t, scale={(1 + 2 * t) % n: 0.7 + 0.05 * t, 0: 0.9})]
        comp.track_gains(only(frames, active), stride=2, smoothing=0.5)
        track_group(shards, frames, 2, 0.5)
        track_group([route], frames, 2, 0.5)
    want = comp.gains()
    assert np.abs(want - np.asarray(g0)).max() > 1e-3, "the gains did not move: the comparison would show nothing"
    if subset:
        assert want[4] == g0[4]
    ok_sing = comp.gains(counters=True)[1:]
    for k, s in enumerate([route] + shards):
        assert np.array_equal(bits(s.gains()), bits(want)), "context %d: %s want %s" % (k, s.gains(), want)
        assert s.gain_track_counters() == ok_sing + (0,) == (steps, 0, 0)
    final = [to_dev(f) for f in frames_of(cfg, 7)]
    ref16 = stitch16(comp, cfg, cuda, only(final, active))
    assert np.array_equal(stitch16(route, cfg, cuda, only(final, active)), ref16)
    for k, s in enumerate(shards):
        b0, b1 = s.col_window()
        assert np.array_equal(stitch16(s, cfg, cuda, only(final, s.needed_views()))[:, b0:b1], ref16[:, b0:b1]), "column shard %d/%d" % (k, S)
    for c in [comp, route] + shards:
        c.close()


def test_nv12_partials_track_like_ms_track_gains_nv12(ms, cuda):
    comp, cfg, g0 = make_rig(ms, "mini6")
    shards = shards_of(ms, "mini6", 2)
    nv = [to_dev(synth.nv12_frame(cfg["w"], cfg["h"], i)) for i in range(cfg["n"])]
    comp.track_gains_nv12(nv, stride=2, smoothing=1.0)
    track_group(shards, nv, 2, 1.0, nv12=True)
    want = comp.gains()
    assert np.abs(want - np.asarray(g0)).max() > 1e-3
    for s in shards:
        assert np.array_equal(bits(s.gains()), bits(want))
    for c in [comp] + shards:
        c.close()


# ---- 4. mismatch ---------------------------------------------------------------------------------------------------------------------------------------
def _rc(ms, call):
    with pytest.raises(ms.MsError) as e:
        call()
    return int(str(e.value).split()[2].rstrip(":"))


def test_mismatching_partials_change_nothing_and_are_counted(ms, cuda):
    a, cfg, g0 = make_rig(ms, "mini6", col_shards=2, col_shard_index=0)
    b = make_rig(ms, "mini6", col_shards=2, col_shard_index=1)[0]
    n = cfg["n"]
    all_ = (1 << n) - 1
    frames = [to_dev(f) for f in frames_of(cfg, 0, scale={2: 0.7})]
    before = a.gains()
    assert np.array_equal(before, np.asarray(g0, np.float64))
    # different strides
    a.track_gains_from_partials([a.gain_stats_partial(frames, 2), b.gain_stats_partial(frames, 4)], stride=2, smoothing=1.0)
    assert a.gain_track_counters() == (0, 0, 1) and np.array_equal(bits(a.gains()), bits(before))
    # the partials agree with each other but not with the call
    a.track_gains_from_partials([a.gain_stats_partial(frames, 4), b.gain_stats_partial(frames, 4)], stride=2, smoothing=1.0)
    assert a.gain_track_counters() == (0, 0, 2) and np.array_equal(bits(a.gains()), bits(before))
    # different active sets
    b.set_active_views(all_ & ~(1 << 3))
    a.track_gains_from_partials([a.gain_stats_partial(frames, 2), b.gain_stats_partial(only(frames, all_ & ~(1 << 3)), 2)], stride=2, smoothing=1.0)
    assert a.gain_track_counters() == (0, 0, 3) and np.array_equal(bits(a.gains()), bits(before))
    b.set_active_views(all_)
    # not a partial at all, and a partial of another rig
    a.track_gains_from_partials([a.gain_stats_partial(frames, 2), a.new_gain_partial()], stride=2, smoothing=1.0)
    other, ocfg, _ = make_rig(ms, "mini4")
    foreign = torch.zeros_like(a.new_gain_partial())
    po = other.gain_stats_partial([to_dev(f) for f in frames_of(ocfg)], 2)
    foreign[:po.numel()] = po
    a.track_gains_from_partials([a.gain_stats_partial(frames, 2), foreign], stride=2, smoothing=1.0)
    assert a.gain_track_counters() == (0, 0, 5) and np.array_equal(bits(a.gains()), bits(before))
    # no error surfaces later: the context stitches with the old gains and the next good update goes through
    ref = make_rig(ms, "mini6")[0]
    b0, b1 = a.col_window()
    assert np.array_equal(stitch16(a, cfg, cuda, only(frames, a.needed_views()))[:, b0:b1], stitch16(ref, cfg, cuda, frames)[:, b0:b1])
    track_group([a, b], frames, 2, 1.0)
    ref.track_gains(frames, stride=2, smoothing=1.0)
    assert a.gain_track_counters() == (1, 0, 5) and b.gain_track_counters() == (1, 0, 0)
    assert np.array_equal(bits(a.gains()), bits(ref.gains())) and np.array_equal(bits(b.gains()), bits(ref.gains()))
    assert a.gains(counters=True)[1:] == (1, 0)
    for c in (a, b, ref, other):
        c.close()


def test_a_singular_system_counts_as_before_and_changes_nothing(ms, cuda):
    """GainCompensator's system is positive definite for every statistic real frames can give (beta N > 0 on the diagonal), so the singular branch is driven
    with partials whose counts are set by hand: 2^31 in every cell of each of two partials.  Their sum, 2^32, passes max(1, cnt) and becomes 0 in the int the
    solver takes (gain_update_body, as k_gain_update): the matrix is all zero.  Every shard counts one singular system; gains, view tables and `rejected` stay."""
    shards = shards_of(ms, "mini6", 2)
    cfg = synth.CONFIGS["mini6"]
    n = cfg["n"]
    frames = [to_dev(f) for f in frames_of(cfg, 0, scale={2: 0.7})]
    ref = make_rig(ms, "mini6")[0]
    before = [s.gains() for s in shards]
    pano = [stitch16(s, cfg, cuda, only(frames, s.needed_views())) for s in shards]
    parts = [s.gain_stats_partial(only(frames, s.gain_views()), 2) for s in shards]
    torch.cuda.synchronize()
    for p in parts:
        p[4:4 + n * n] = 1 << 31                      # (4 int64 of header, then cnt)
    torch.cuda.synchronize()
    for k, s in enumerate(shards):
        s.track_gains_from_partials(parts, stride=2, smoothing=1.0)
        assert s.gain_track_counters() == (0, 1, 0), "shard %d: %s" % (k, s.gain_track_counters())
        assert s.gains(counters=True)[1:] == (0, 1)
        assert np.array_equal(bits(s.gains()), bits(before[k]))
        assert np.array_equal(stitch16(s, cfg, cuda, only(frames, s.needed_views())), pano[k]), "shard %d: the panorama changed" % k
    # a good update afterwards goes through, and the singular count stays
    track_group(shards, frames, 2, 1.0)
    ref.track_gains(frames, stride=2, smoothing=1.0)
    for s in shards:
        assert s.gain_track_counters() == (1, 1, 0) and np.array_equal(bits(s.gains()), bits(ref.gains()))
    for c in shards + [ref]:
        c.close()


def test_argument_checks_and_refusals_on_a_context(ms, cuda):
    comp, cfg, _ = make_rig(ms, "mini6", col_shards=2, col_shard_index=1)
    n = cfg["n"]
    lib = ms.load()
    frames = [to_dev(f) for f in frames_of(cfg)]
    part = comp.new_gain_partial()
    assert comp.gain_partial_bytes() == 32 + 16 * n * n == part.numel() * 8
    prm = ms.gain_track_default_params()
    arr = (ms.C.c_void_p * 1)(part.data_ptr())
    assert _rc(ms, lambda: comp.gain_stats_partial(frames, 0)) == MS_ERR_INVALID
    assert lib.ms_gain_stats_partial(comp._ctx, comp._one_frame(frames), 2, None, None) == MS_ERR_INVALID
    assert lib.ms_gain_stats_partial(comp._ctx, comp._one_frame(frames), 2, ms.C.c_void_p(part.data_ptr() + 4), None) == MS_ERR_INVALID
    assert lib.ms_gain_stats_partial(comp._ctx, None, 2, ms.C.c_void_p(part.data_ptr()), None) == MS_ERR_INVALID
    gv = comp.gain_views()
    inside = [v for v in range(n) if (gv >> v) & 1][0]
    small = torch.zeros((cfg["h"] - 1, cfg["w"], 3), dtype=torch.uint8, device=cuda)
    assert _rc(ms, lambda: comp.gain_stats_partial(frames[:inside] + [small] + frames[inside + 1:], 2)) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.gain_stats_partial(frames[:inside] + [None] + frames[inside + 1:], 2)) == MS_ERR_INVALID      # a view the statistic reads, without an image
    assert lib.ms_track_gains_from_partials(comp._ctx, arr, 0, ms.C.byref(prm), None) == MS_ERR_INVALID
    assert lib.ms_track_gains_from_partials(comp._ctx, arr, 17, ms.C.byref(prm), None) == MS_ERR_INVALID
    assert lib.ms_track_gains_from_partials(comp._ctx, None, 1, ms.C.byref(prm), None) == MS_ERR_INVALID
    assert lib.ms_track_gains_from_partials(comp._ctx, arr, 1, None, None) == MS_ERR_INVALID
    bad = ms.gain_track_default_params(); bad.struct_size += 8
    assert lib.ms_track_gains_from_partials(comp._ctx, arr, 1, ms.C.byref(bad), None) == MS_ERR_INVALID
    for lam in (0.0, 1.5, float("nan")):
        assert _rc(ms, lambda: comp.track_gains_from_partials([part], smoothing=lam)) == MS_ERR_INVALID
    k = ms.GainTrackCounters(struct_size=20)
    assert lib.ms_get_gain_track_counters(comp._ctx, ms.C.byref(k), None) == MS_ERR_INVALID
    assert comp.gain_track_counters() == (0, 0, 0), "a refused call counts nothing"
    # ms_track_gains / ms_gain_stats keep refusing a column shard
    assert _rc(ms, lambda: comp.track_gains(frames)) == MS_ERR_UNSUPPORTED and _rc(ms, lambda: comp.gain_stats(frames, 1)) == MS_ERR_UNSUPPORTED
    comp.close()
    # view shards and FeatherBlender contexts
    vs = make_rig(ms, "mini6", shards=2, shard_index=0)[0]
    fe = ms.Compositor(n, (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=0, out_size=(cfg["out_w"], cfg["out_h"]))
    early = ms.Compositor(n, (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"], out_size=(cfg["out_w"], cfg["out_h"]))
    for c in (fe, early):
        for i in range(n):
            c.set_camera(i, *synth.camera(n, cfg["w"], cfg["h"], cfg["hfov_deg"], i))
        c.build_maps(); c.build_masks(1)
    fe.init_feather()
    for c, want in ((vs, MS_ERR_UNSUPPORTED), (fe, MS_ERR_UNSUPPORTED), (early, MS_ERR_STATE)):
        assert _rc(ms, lambda: c.gain_stats_partial(frames, 2, partial=part)) == want
        assert _rc(ms, lambda: c.track_gains_from_partials([part])) == want
        assert _rc(ms, lambda: c.gain_views()) == want
        c.close()


# ---- 5. no older gain comes back (the cases of test_gain_track_gpu.py on the partial route, unsharded context) ----------------------------------------------
def track_one(comp, frames, stride, smoothing):
    comp.track_gains_from_partials([comp.gain_stats_partial(frames, stride)], stride=stride, smoothing=smoothing)


def fresh_with(ms, rig, gains, **kw):
    comp, cfg, _ = make_rig(ms, rig, **kw)
    for v, g in enumerate(gains):
        comp.set_gain(v, float(g))
    return comp


def same(comp, ref, cfg, cuda, frames, what):
    assert np.array_equal(stitch16(comp, cfg, cuda, frames), stitch16(ref, cfg, cuda, frames)), what


def test_no_old_gain_comes_back_dropout_and_tables(ms, cuda):
    comp, cfg, g0 = make_rig(ms, "mini6")
    n = cfg["n"]
    all_ = (1 << n) - 1
    frames = [to_dev(f) for f in frames_of(cfg, 0, scale={1: 0.7})]
    cached, first_time = all_ & ~(1 << 4), all_ & ~(1 << 5)      # a subset cached BEFORE tracking, one made for the first time AFTER it
    comp.set_active_views(cached); comp.set_active_views(all_)
    track_one(comp, frames, 2, 1.0)
    g = comp.gains()
    assert np.abs(g - np.asarray(g0)).max() > 1e-3
    ref = fresh_with(ms, "mini6", g)
    for sub in (cached, first_time):
        comp.set_active_views(sub); ref.set_active_views(sub)
        same(comp, ref, cfg, cuda, only(frames, sub), "subset 0x%x" % sub)
        assert np.array_equal(comp.gains(), g)
        comp.set_active_views(all_); ref.set_active_views(all_)
        same(comp, ref, cfg, cuda, frames, "restored after 0x%x" % sub)
        assert np.array_equal(comp.gains(), g)
    comp.set_active_views(cached)                               # an inactive view keeps its gain through an update; the others move
    dimmer = [to_dev(f) for f in frames_of(cfg, 0, scale={1: 0.7, 2: 0.8})]
    track_one(comp, only(dimmer, cached), 2, 1.0)
    g2 = comp.gains()
    assert g2[4] == g[4] and np.abs(g2 - g).max() > 1e-3
    comp.set_active_views(all_)
    comp.set_gain(0, 1.25)                                      # ms_set_gain after tracking wins for its view, and only for it
    g3 = comp.gains()
    assert g3[0] == 1.25 and np.array_equal(g3[1:], g2[1:])
    ref2 = fresh_with(ms, "mini6", g3)
    same(comp, ref2, cfg, cuda, frames, "set_gain after tracking")
    loaded = ms.Compositor.from_tables(comp.save_tables())      # ms_save_tables -> ms_load_tables carries the tracked gains
    assert np.array_equal(loaded.gains(), g3) and np.array_equal(comp.gains(), g3)
    same(loaded, ref2, cfg, cuda, frames, "loaded tables")
    comp.init_blender()                                         # the rebuilt tables hold the tracked gains
    assert np.array_equal(comp.gains(), g3)
    same(comp, ref2, cfg, cuda, frames, "re-initialised")
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
    track_one(comp, frames, 2, 1.0)
    g = comp.gains()
    assert np.abs(g - synth.gains(cfg["n"])).max() > 1e-3
    ref, _ = rig()
    for v in range(cfg["n"]):
        ref.set_gain(v, float(g[v]))
    for view in (1, 4):                  # (with a margin: both copies of the tables get used)
        comp.update_mask(view); ref.update_mask(view)
        assert np.array_equal(comp.gains(), g)
        same(comp, ref, cfg, cuda, frames, "after update_mask(%d), margin %d" % (view, margin))
    comp.close(); ref.close()


# ---- 6. ranks ------------------------------------------------------------------------------------------------------------------------------------------
def run_app(*args, rig="mini6", timeout=600):
    cfg = synth.CONFIGS[rig]
    base = ["--views", cfg["n"], "--size", "%dx%d" % (cfg["w"], cfg["h"]), "--out", "%dx%d" % (cfg["out_w"], cfg["out_h"]), "--hfov", cfg["hfov_deg"], "--bands", cfg["num_bands"]]
    out = subprocess.run([APP] + [str(a) for a in base + list(args)], capture_output=True, timeout=timeout)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    return json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("transport", ["host", "loopback_rccl"])
@pytest.mark.parametrize("ranks", [2, 4])
def test_ranks_of_a_column_group_track_the_single_gpu_gains(cuda, ranks, transport):
    """stitch_dist: `ranks` column shards of one group (one thread per rank, all on this GPU) track after every batch; the single-rank run takes the same route with
    one partial.  Gains and counters equal on every rank, the gains equal to one GPU's as float64 (printed with %.17g), and so are the frames."""
    args = ["--frames", 12, "--batch", 2, "--track-gains", 1]
    one = run_app("--gpus", 1, *args)
    off = run_app("--gpus", 1, "--frames", 12, "--batch", 2)
    assert "gains" not in off and one["gain_solves_ok"] == 6 and one["gain_solves_singular"] == 0 and one["gain_updates_rejected"] == 0
    assert one["checksum_all"] != off["checksum_all"] and one["first_frame_checksum"] == off["first_frame_checksum"], "tracking must change the frames after the first batch"
    if transport == "host":
        where = ["--gpus", ranks, "--share-gpu"]
    else:
        assert os.path.isfile(FAKE_RCCL), "tests/_fake_rccl/libfake_rccl.so is built by __graft_entry__.build()"
        where = ["--gpus", ranks, "--share-gpu", "--transport", "rccl", "--rccl-lib", FAKE_RCCL]
    many = run_app(*where, "--col-shards", ranks, *args)
    assert many["dist"]["transport"] == ("host" if transport == "host" else "rccl") and many["dist"]["nranks"] == ranks and many["groups"] == 1
    assert many["gain_ranks_equal"] is True
    assert (many["gain_solves_ok"], many["gain_solves_singular"], many["gain_updates_rejected"]) == (6, 0, 0)
    assert np.array_equal(bits(many["gains"]), bits(one["gains"])), (many["gains"], one["gains"])
    assert many["checksum_all"] == one["checksum_all"]


def test_stitch_dist_two_shards_report_gains(cuda):
    res = run_app("--gpus", 2, "--share-gpu", "--col-shards", 2, "--frames", 8, "--batch", 2, "--track-gains", 1)
    assert res["track_gains"] == 1 and len(res["gains"]) == synth.CONFIGS["mini6"]["n"] and res["gain_ranks_equal"] is True
    assert res["gain_solves_ok"] == 4 and res["gain_updates_rejected"] == 0
    every_other = run_app("--gpus", 2, "--share-gpu", "--col-shards", 2, "--frames", 8, "--batch", 2, "--track-gains", 2)
    assert every_other["gain_solves_ok"] == 2


def test_ms_dist_track_gains_through_the_binding(ms, cuda):
    """msdist.Dist.track_gains from two threads sharing the GPU (host transport): both ranks reach ms_track_gains' gains; a rank with a refused frame returns the
    error while both ranks count one rejected update and keep their gains."""
    import msdist
    cfg = synth.CONFIGS["mini6"]
    frames_np = frames_of(cfg, 0, scale={3: 0.7})
    ref = make_rig(ms, "mini6")[0]
    ref.track_gains([to_dev(f) for f in frames_np], stride=2, smoothing=1.0)
    want = ref.gains()
    idb = msdist.unique_id(2, msdist.HOST)
    res, errs = {}, []

    def rank(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                d = msdist.Dist(r, 2, idb, device=0)
                comp = make_rig(ms, "mini6", col_shards=2, col_shard_index=r)[0]
                frames = [to_dev(f) for f in frames_np]
                keep = d.track_gains(comp, [0, 1], only(frames, comp.gain_views()), stride=2, smoothing=1.0)
                g1, c1 = comp.gains(stream=torch.cuda.current_stream()), comp.gain_track_counters(stream=torch.cuda.current_stream())
                refused = None
                bad = list(frames)
                if r == 1:
                    bad[[v for v in range(cfg["n"]) if (comp.gain_views() >> v) & 1][0]] = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
                try:
                    keep2 = d.track_gains(comp, [0, 1], bad, stride=2, smoothing=1.0)
                except ms.MsError as e:
                    refused = str(e)
                g2, c2 = comp.gains(stream=torch.cuda.current_stream()), comp.gain_track_counters(stream=torch.cuda.current_stream())
                res[r] = (g1, c1, refused, g2, c2)
                d.barrier(); d.close(); comp.close()
                del keep
        except Exception as e:      # noqa: BLE001
            import traceback
            errs.append(traceback.format_exc()[-1500:] or repr(e))

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join(timeout=300) for t in ts]
    assert not errs, errs
    for r in range(2):
        g1, c1, refused, g2, c2 = res[r]
        assert np.array_equal(bits(g1), bits(want)) and c1 == (1, 0, 0), (r, g1, want, c1)
        assert np.array_equal(bits(g2), bits(g1)) and c2 == (1, 0, 1), (r, c2)      # the refusing rank counts the rejection too: the group's counters stay equal
        assert (refused is not None) == (r == 1), (r, refused)
    ref.close()


# ---- 7. concurrency ------------------------------------------------------------------------------------------------------------------------------------
def test_a_stitching_thread_sees_the_old_or_the_new_gains_never_a_mix(ms, cuda):
    """One thread stitches on its stream; another alternates ms_gain_stats_partial + ms_track_gains_from_partials over two frame sets (smoothing 1: the gains
    alternate between two vectors) on its own stream.  Every panorama equals that of one of the three gain vectors the context ever held."""
    comp, cfg, g0 = make_rig(ms, "mini6")
    fixed = [to_dev(f) for f in frames_of(cfg, 5)]
    sets = [[to_dev(f) for f in frames_of(cfg, 0, scale={3: 0.7})], [to_dev(f) for f in frames_of(cfg, 1, scale={0: 0.8})]]
    answers = [stitch16(comp, cfg, cuda, fixed)]
    for fs in sets:
        probe = make_rig(ms, "mini6")[0]
        track_one(probe, fs, 2, 1.0)
        answers.append(stitch16(probe, cfg, cuda, fixed))
        probe.close()
    assert not np.array_equal(answers[0], answers[1]) and not np.array_equal(answers[1], answers[2]) and not np.array_equal(answers[0], answers[2])
    errors, stop = [], threading.Event()

    def tracker():
        try:
            st = torch.cuda.Stream()
            part = comp.new_gain_partial()
            torch.cuda.synchronize()
            k = 0
            while not stop.is_set():
                comp.gain_stats_partial(sets[k % 2], 2, partial=part, stream=st)
                comp.track_gains_from_partials([part], stride=2, smoothing=1.0, stream=st)
                k += 1
                if k % 64 == 0:
                    st.synchronize()          # (bounds the queue of enqueued updates)
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=tracker)
    t.start()
    try:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            out = torch.zeros(answers[0].shape, dtype=torch.int16, device=cuda)
            kinds = []
            while len(kinds) < 60 or (len(kinds) < 600 and not (1 in kinds and 2 in kinds)):
                comp.stitch([fixed], out16s=[out]); st.synchronize()
                o = host(out)
                kinds.append(next((i for i, a in enumerate(answers) if np.array_equal(o, a)), -1))
    finally:
        stop.set(); t.join()
    assert not errors, errors
    assert -1 not in kinds, "a frame is none of the panoramas of the gain vectors the context held (frame %d of %d)" % (kinds.index(-1), len(kinds))
    assert 1 in kinds and 2 in kinds, "the updates never took effect in %d stitches" % len(kinds)
    comp.close()
