"""Exposure tracking on view shards (ms_gain_samples / ms_track_gains_from_samples / ms_gain_stats_from_samples / ms_dist_track_gains_views) on the device, through
the C-ABI: every shard's sample buffer is the numpy restatement (tests/gain_samples_ref.py) word for word; the pair sums formed from all shards' buffers are
ms_gain_stats of an unsharded context, in every buffer order; every shard reaches the gains of ms_track_gains as float64 bit patterns and the group composites the
unsharded panorama with them; unowned views are never read; sets that do not fit change nothing and are counted; ranks of a view-shard group agree over both
transports.  All comparisons are exact: both sides run the same integer arithmetic."""
import itertools
import os
import threading

import numpy as np
import pytest
import torch

import gain_ref as G
import gain_samples_ref as R
import synth
from helpers import host, make_rig, to_dev, to_dev_roi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def view_shards(ms, rig, S):
    return [make_rig(ms, rig, shards=S, shard_index=k)[0] for k in range(S)] if S > 1 else [make_rig(ms, rig)[0]]


def bits(g):
    return np.asarray(g, np.float64).view(np.uint64)


def words(t):
    return host(t).view(np.uint32)


def samples_of(shards, frames, stride, nv12=False):
    """Every shard's buffer from the views it owns alone."""
    return [s.gain_samples(only(frames, s.gain_sample_views()), stride, nv12=nv12) for s in shards]


def track_group(shards, frames, stride, smoothing, nv12=False):
    """One tracking step of a view-shard group on one GPU: every shard's sample vectors, then every shard pairs and solves over all of them."""
    bufs = samples_of(shards, frames, stride, nv12=nv12)
    for s in shards:
        s.track_gains_from_samples(bufs, stride=stride, smoothing=smoothing)
    return bufs


def stitch16(comp, cfg, cuda, frames):
    pg = comp.pano_geom()
    o16 = torch.full((pg.dst_roi_final.height, pg.dst_roi_final.width, 3), -7, dtype=torch.int16, device=cuda)
    comp.stitch([frames], out16s=[o16])
    torch.cuda.synchronize()
    return host(o16)


def stitch16_group(shards, cfg, cuda, frames):
    """ms_stitch_partial on every shard with its own views, ms_stitch_finish on the first."""
    parts = []
    for s in shards:
        part = torch.full((s.partial_bytes() // 2,), 12345, dtype=torch.int16, device=cuda)
        s.stitch_partial([only(frames, s.needed_views())], part)
        parts.append(part)
    pg = shards[0].pano_geom()
    o16 = torch.full((pg.dst_roi_final.height, pg.dst_roi_final.width, 3), -7, dtype=torch.int16, device=cuda)
    shards[0].stitch_finish(1, parts, out16s=[o16])
    torch.cuda.synchronize()
    return host(o16)


# ---- 1. the buffers --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_every_shards_buffer_equals_the_numpy_buffer_word_for_word(ms, cuda, rig):
    comp, cfg, _ = make_rig(ms, rig)
    n = cfg["n"]
    rois, T, maps = geometry(comp, cfg)
    rng = np.random.default_rng(31)
    bgr_np = frames_of(cfg, 2, scale={1: 0.8})
    dev = [to_dev_roi(f, rng) for f in bgr_np]
    seen, q = sampled(maps, bgr_np)
    wide = sorted(r[2] for r in rois)[-2]           # a stride of which only the view that wraps round the panorama holds two lattice columns: every other R_v is
                                                    # empty or one sample wide
    assert T[2] % 4 and T[3] % 4, "stride 4 must leave a partial last lattice row and column (stride 3 divides mini6's ROI, 639 x 105)"
    narrow = 0
    for S in (1, 2, 3):
        shards = view_shards(ms, rig, S)
        for stride in (1, 3, 4, wide):
            for k, s in enumerate(shards):
                own = R.shard_views(n, S, k)
                assert s.gain_sample_views() == own
                want = R.buffer(rois, seen, q, T, stride, own)
                assert [c.gain_samples_bytes(stride, k if S > 1 else -1) for c in shards] == [want.size * 4] * S, "every rank sizes shard %d's buffer alike" % k
                assert s.gain_samples_bytes(stride) == want.size * 4
                got = words(s.gain_samples(only(dev, own), stride))
                assert got.size == want.size
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, "%s shard %d/%d stride %d: %d words differ, first at %d: %d want %d" % (rig, k, S, stride, bad.size, bad[0], got[bad[0]], want[bad[0]])
                if stride == wide:
                    narrow += sum(1 for v in range(n) if (own >> v) & 1 and R.lattice_rect(rois[v], T, stride)[2] <= 1)
        for s in shards:
            s.close()
    assert narrow > 0, "no view with an empty or one-sample-wide rectangle was covered"
    comp.close()


# ---- 2. the statistic ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig,S", [("mini6", 2), ("mini6", 3), ("mini4", 3)])
def test_pair_sums_from_all_shards_buffers_equal_the_unsharded_statistic_in_every_order(ms, cuda, rig, S):
    comp, cfg, _ = make_rig(ms, rig)
    frames = [to_dev(f) for f in frames_of(cfg, 2, scale={1: 0.8})]
    shards = view_shards(ms, rig, S)
    for stride in (1, 3, 4):
        want_N, want_S = comp.gain_stats(frames, stride)
        off = want_N.copy()
        np.fill_diagonal(off, 0)
        assert (off > 1).any(), "no pair of different views has samples: the comparison would show nothing"
        bufs = samples_of(shards, frames, stride)
        for order in itertools.permutations(range(S)):
            for s in (shards[0], shards[-1], comp):          # (an unsharded context pairs foreign buffers too: it expects what they hold)
                N, Sm = s.gain_stats_from_samples([bufs[k] for k in order], stride)
                assert np.array_equal(N, want_N) and np.array_equal(Sm, want_S), "order %s, stride %d" % (order, stride)
    for s in shards:
        assert s.gain_track_counters() == (0, 0, 0)
    for c in [comp] + shards:
        c.close()


# ---- 3. gains --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("S", [2, 3])
def test_every_shard_reaches_the_unsharded_gains_bit_for_bit(ms, cuda, S, steps):
    comp, cfg, g0 = make_rig(ms, "mini6")
    n = cfg["n"]
    shards = view_shards(ms, "mini6", S)
    route = make_rig(ms, "mini6")[0]                        # an unsharded context on the sample route: one buffer
    for t in range(steps):                                  # drifting frames: another view dims at every step
        frames = [to_dev(f) for f in frames_of(cfg, t, scale={(1 + 2 * t) % n: 0.7 + 0.05 * t, 0: 0.9})]
        comp.track_gains(frames, stride=2, smoothing=0.5)
        track_group(shards, frames, 2, 0.5)
        track_group([route], frames, 2, 0.5)
    want = comp.gains()
    assert np.abs(want - np.asarray(g0)).max() > 1e-3, "the gains did not move: the comparison would show nothing"
    for k, s in enumerate([route] + shards):
        assert np.array_equal(bits(s.gains()), bits(want)), "context %d: %s want %s" % (k, s.gains(), want)
        assert s.gain_track_counters() == comp.gain_track_counters() == (steps, 0, 0)
    for c in [comp, route] + shards:
        c.close()


@pytest.mark.parametrize("steps", [1, 3])
def test_an_active_subset_on_the_unsharded_sample_route(ms, cuda, steps):
    comp, cfg, g0 = make_rig(ms, "mini6")
    route = make_rig(ms, "mini6")[0]
    n = cfg["n"]
    active = ((1 << n) - 1) & ~(1 << 4)
    rois, T, maps = geometry(comp, cfg)
    for c in (comp, route):
        c.set_active_views(active)
    assert route.gain_sample_views() == active
    for t in range(steps):
        np_frames = frames_of(cfg, t, scale={(1 + 2 * t) % n: 0.7 + 0.05 * t, 0: 0.9})
        frames = only([to_dev(f) for f in np_frames], active)
        comp.track_gains(frames, stride=3, smoothing=0.5)
        buf = route.gain_samples(frames, 3)
        seen, q = sampled(maps, np_frames)
        assert np.array_equal(words(buf), R.buffer(rois, seen, q, T, 3, (1 << n) - 1, active)), "the view left out is not written"
        route.track_gains_from_samples([buf], stride=3, smoothing=0.5)
    want = comp.gains()
    assert np.abs(want - np.asarray(g0)).max() > 1e-3 and want[4] == g0[4]
    assert np.array_equal(bits(route.gains()), bits(want)) and route.gain_track_counters() == (steps, 0, 0)
    comp.close(); route.close()


# ---- 4. NV12 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_nv12_samples_track_like_ms_track_gains_nv12(ms, cuda):
    comp, cfg, g0 = make_rig(ms, "mini6")
    shards = view_shards(ms, "mini6", 2)
    nv = [to_dev(synth.nv12_frame(cfg["w"], cfg["h"], i)) for i in range(cfg["n"])]
    comp.track_gains_nv12(nv, stride=2, smoothing=1.0)
    bufs = track_group(shards, nv, 2, 1.0, nv12=True)
    as_bgr = ms.nv12_to_bgr_batch(nv)
    for k, s in enumerate(shards):                          # the planes give the words of their BGR copies
        assert torch.equal(bufs[k], s.gain_samples(only(as_bgr, s.gain_sample_views()), 2)), "shard %d" % k
        assert torch.equal(bufs[k], s.gain_samples_nv12(only(nv, s.gain_sample_views()), 2))
    want = comp.gains()
    assert np.abs(want - np.asarray(g0)).max() > 1e-3
    for s in shards:
        assert np.array_equal(bits(s.gains()), bits(want))
    for c in [comp] + shards:
        c.close()


# ---- 5. publication --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3])
def test_the_group_composites_the_unsharded_panorama_with_the_tracked_gains(ms, cuda, S):
    comp, cfg, g0 = make_rig(ms, "mini6")
    shards = view_shards(ms, "mini6", S)
    frames = [to_dev(f) for f in frames_of(cfg, 0, scale={2: 0.7})]
    final = [to_dev(f) for f in frames_of(cfg, 7)]
    before = stitch16(comp, cfg, cuda, final)
    assert np.array_equal(stitch16_group(shards, cfg, cuda, final), before)
    comp.track_gains(frames, stride=2, smoothing=1.0)
    track_group(shards, frames, 2, 1.0)
    want = stitch16(comp, cfg, cuda, final)
    assert not np.array_equal(want, before), "tracking did not change the panorama: the comparison would show nothing"
    assert np.array_equal(stitch16_group(shards, cfg, cuda, final), want)
    for c in [comp] + shards:
        c.close()


# ---- 6. views read ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_unowned_views_are_never_read(ms, cuda, rig):
    cfg = synth.CONFIGS[rig]
    n = cfg["n"]
    frames = [to_dev(f) for f in frames_of(cfg, 1)]
    zero = ms.Image()
    for S in (2, 3):
        for k, s in enumerate(view_shards(ms, rig, S)):
            own = s.gain_sample_views()
            assert own == R.shard_views(n, S, k) and own & ~s.needed_views() == 0
            full = s.gain_samples(frames, 2)
            views = s._one_frame(frames)
            for v in range(n):
                if not (own >> v) & 1:
                    views[v] = zero                       # an all-zero ms_image for every view of another shard
            lean = torch.zeros_like(full)
            assert ms.load().ms_gain_samples(s._ctx, views, 2, ms.C.c_void_p(lean.data_ptr()), ms._stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(full, lean), "shard %d/%d: the buffer changed when the views outside 0x%x were withheld" % (k, S, own)
            assert (words(full)[R.HEADER_WORDS + n:] > 1).any(), "an empty buffer would show nothing"
            s.close()


# ---- 7. rejections ---------------------------------------------------------------------------------------------------------------------------------------
def _rc(ms, call):
    with pytest.raises(ms.MsError) as e:
        call()
    return int(str(e.value).split()[2].rstrip(":"))


def test_sets_that_do_not_fit_change_nothing_and_are_counted(ms, cuda):
    a, cfg, g0 = make_rig(ms, "mini6", shards=2, shard_index=0)
    b = make_rig(ms, "mini6", shards=2, shard_index=1)[0]
    ref = make_rig(ms, "mini6")[0]
    other, ocfg, _ = make_rig(ms, "mini4")
    frames = [to_dev(f) for f in frames_of(cfg, 0, scale={2: 0.7})]
    before = a.gains()
    assert np.array_equal(before, np.asarray(g0, np.float64))
    pano = stitch16_group([a, b], cfg, cuda, frames)
    A2, B2 = samples_of([a, b], frames, 2)
    B4 = b.gain_samples(only(frames, b.gain_sample_views()), 4)
    foreign = other.gain_samples([to_dev(f) for f in frames_of(ocfg)], 2)
    assert foreign.numel() * 4 >= 64 + 4 * cfg["n"]
    cases = {"one buffer missing": [A2], "the same buffer twice": [A2, A2], "a stride mismatch": [A2, B4], "a buffer of the other rig": [A2, foreign],
             "the buffers agree with each other but not with the call": [a.gain_samples(only(frames, a.gain_sample_views()), 4), B4]}
    for k, (what, bufs) in enumerate(cases.items()):
        a.track_gains_from_samples(bufs, stride=2, smoothing=1.0)
        assert a.gain_track_counters() == (0, 0, k + 1), what
        assert np.array_equal(bits(a.gains()), bits(before)), what
    k = len(cases)
    # no error surfaces later: the group stitches with the old gains, the accumulators are clear, and the next good update is the first update
    assert np.array_equal(stitch16_group([a, b], cfg, cuda, frames), pano)
    want_N, want_S = ref.gain_stats(frames, 2)
    N, Sm = a.gain_stats_from_samples([B2, A2], 2)
    assert np.array_equal(N, want_N) and np.array_equal(Sm, want_S)
    N, Sm = a.gain_stats_from_samples([A2], 2)              # the diagnostic rejects alike: zeros, one more counted
    assert not N.any() and not Sm.any() and a.gain_track_counters() == (0, 0, k + 1)
    track_group([a, b], frames, 2, 1.0)
    ref.track_gains(frames, stride=2, smoothing=1.0)
    assert a.gain_track_counters() == (1, 0, k + 1) and b.gain_track_counters() == (1, 0, 0)
    assert np.array_equal(bits(a.gains()), bits(ref.gains())) and np.array_equal(bits(b.gains()), bits(ref.gains()))
    assert np.array_equal(stitch16_group([a, b], cfg, cuda, frames), stitch16(ref, cfg, cuda, frames))
    for c in (a, b, ref, other):
        c.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_and_refusals_on_a_context(ms, cuda):
    comp, cfg, _ = make_rig(ms, "mini6", shards=2, shard_index=1)
    n = cfg["n"]
    lib = ms.load()
    frames = [to_dev(f) for f in frames_of(cfg)]
    buf = comp.gain_samples(frames, 2)
    prm = ms.gain_track_default_params()
    arr = (ms.C.c_void_p * 1)(buf.data_ptr())
    out = np.zeros((n, n), np.int64)
    outp = out.ctypes.data_as(ms.C.c_void_p)
    assert comp.gain_samples_bytes(2) == comp.gain_samples_bytes(2, 1) == buf.numel() * 4 > 64 + 4 * n
    assert comp.gain_samples_bytes(0) == 0 and comp.gain_samples_bytes(2, 2) == 0 and comp.gain_samples_bytes(2, -2) == 0
    assert comp.view_shard() == (2, 1)
    assert _rc(ms, lambda: comp.gain_samples(frames, 0)) == MS_ERR_INVALID
    assert lib.ms_gain_samples(comp._ctx, comp._one_frame(frames), 2, None, None) == MS_ERR_INVALID
    assert lib.ms_gain_samples(comp._ctx, comp._one_frame(frames), 2, ms.C.c_void_p(buf.data_ptr() + 2), None) == MS_ERR_INVALID
    assert lib.ms_gain_samples(comp._ctx, None, 2, ms.C.c_void_p(buf.data_ptr()), None) == MS_ERR_INVALID
    own = comp.gain_sample_views()
    inside = [v for v in range(n) if (own >> v) & 1][0]
    small = torch.zeros((cfg["h"] - 1, cfg["w"], 3), dtype=torch.uint8, device=cuda)
    assert _rc(ms, lambda: comp.gain_samples(frames[:inside] + [small] + frames[inside + 1:], 2)) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.gain_samples(frames[:inside] + [None] + frames[inside + 1:], 2)) == MS_ERR_INVALID      # a view that is read, without an image
    assert _rc(ms, lambda: comp.gain_samples_nv12(frames, 2)) == MS_ERR_INVALID                                       # 8UC3 where the planes are expected
    f = lib.ms_track_gains_from_samples
    assert f(comp._ctx, arr, 0, ms.C.byref(prm), None) == MS_ERR_INVALID
    assert f(comp._ctx, arr, 5, ms.C.byref(prm), None) == MS_ERR_INVALID
    assert f(comp._ctx, None, 1, ms.C.byref(prm), None) == MS_ERR_INVALID
    assert f(comp._ctx, arr, 1, None, None) == MS_ERR_INVALID
    assert f(comp._ctx, (ms.C.c_void_p * 1)(buf.data_ptr() + 2), 1, ms.C.byref(prm), None) == MS_ERR_INVALID
    bad = ms.gain_track_default_params(); bad.struct_size += 8
    assert f(comp._ctx, arr, 1, ms.C.byref(bad), None) == MS_ERR_INVALID
    for lam in (0.0, 1.5, float("nan")):
        assert _rc(ms, lambda: comp.track_gains_from_samples([buf], smoothing=lam)) == MS_ERR_INVALID
    assert _rc(ms, lambda: comp.track_gains_from_samples([buf], stride=0)) == MS_ERR_INVALID
    g = lib.ms_gain_stats_from_samples
    assert g(comp._ctx, arr, 0, 2, outp, outp, None) == MS_ERR_INVALID and g(comp._ctx, arr, 1, 0, outp, outp, None) == MS_ERR_INVALID
    assert g(comp._ctx, arr, 1, 2, None, outp, None) == MS_ERR_INVALID and g(comp._ctx, None, 1, 2, outp, outp, None) == MS_ERR_INVALID
    assert lib.ms_get_gain_sample_views(comp._ctx, None) == MS_ERR_INVALID
    assert comp.gain_track_counters() == (0, 0, 0), "a refused call counts nothing"
    # the entry points of the other routes keep refusing a view shard
    part = torch.zeros(comp.gain_partial_bytes() // 8, dtype=torch.int64, device=cuda)
    for call in (lambda: comp.track_gains(frames), lambda: comp.gain_stats(frames, 1), lambda: comp.track_gains_nv12(frames), lambda: comp.gain_stats_partial(frames, 2, partial=part),
                 lambda: comp.track_gains_from_partials([part]), lambda: comp.gain_views(), lambda: comp.set_active_views(1)):
        assert _rc(ms, call) == MS_ERR_UNSUPPORTED
    comp.close()
    # column shards, FeatherBlender contexts, and before ms_init_blender
    cs = make_rig(ms, "mini6", col_shards=2, col_shard_index=0)[0]
    fe = ms.Compositor(n, (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=0, out_size=(cfg["out_w"], cfg["out_h"]))
    early = ms.Compositor(n, (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=cfg["num_bands"], out_size=(cfg["out_w"], cfg["out_h"]))
    assert early.gain_samples_bytes(2) == 0, "before ms_build_maps there is no geometry"
    for c in (fe, early):
        for i in range(n):
            c.set_camera(i, *synth.camera(n, cfg["w"], cfg["h"], cfg["hfov_deg"], i))
        c.build_maps(); c.build_masks(1)
    fe.init_feather()
    assert early.gain_samples_bytes(2) > 0 and cs.gain_samples_bytes(2) == 0 and fe.gain_samples_bytes(2) == 0, "no size where every call is refused"
    assert cs.view_shard() == (1, 0)
    for c, want in ((cs, MS_ERR_UNSUPPORTED), (fe, MS_ERR_UNSUPPORTED), (early, MS_ERR_STATE)):
        assert _rc(ms, lambda: c.gain_samples(frames, 2, samples=buf)) == want
        assert _rc(ms, lambda: c.track_gains_from_samples([buf])) == want
        assert _rc(ms, lambda: c.gain_stats_from_samples([buf], 2)) == want
        assert _rc(ms, lambda: c.gain_sample_views()) == want
        c.close()


# ---- 9. ranks --------------------------------------------------------------------------------------------------------------------------------------------
def _two_ranks(transport, fake_lib, frames_np, q):
    """Two ranks of one view-shard group as two threads sharing the GPU: a tracked step, then one that rank 1 refuses.  Puts {rank: (gains, counters, refused,
    gains, counters)} or a traceback into q.  Over RCCL this runs in a process of its own, which alone names the loopback library."""
    try:
        import msdist
        import msstitch as ms
        if transport == "rccl":
            msdist.set_rccl_library(fake_lib)
        torch.cuda.set_device(0)
        cfg = synth.CONFIGS["mini6"]
        idb = msdist.unique_id(2, msdist.RCCL if transport == "rccl" else msdist.HOST)
        res, errs = {}, []

        def rank(r):
            try:
                torch.cuda.set_device(0)
                with torch.cuda.stream(torch.cuda.Stream()):
                    d = msdist.Dist(r, 2, idb, device=0)
                    assert d.info()["transport"] == transport
                    comp = make_rig(ms, "mini6", shards=2, shard_index=r)[0]
                    frames = [to_dev(f) for f in frames_np]
                    cur = torch.cuda.current_stream()
                    keep = d.track_gains_views(comp, [0, 1], only(frames, comp.gain_sample_views()), stride=2, smoothing=1.0)
                    g1, c1 = comp.gains(stream=cur), comp.gain_track_counters(stream=cur)
                    refused = None
                    bad = list(frames)
                    if r == 1:
                        bad[[v for v in range(cfg["n"]) if (comp.gain_sample_views() >> v) & 1][0]] = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
                    try:
                        keep2 = d.track_gains_views(comp, [0, 1], bad, stride=2, smoothing=1.0)
                    except ms.MsError as e:
                        refused = str(e)
                    g2, c2 = comp.gains(stream=cur), comp.gain_track_counters(stream=cur)
                    res[r] = (g1, c1, refused, g2, c2)
                    d.barrier(); d.close(); comp.close()
                    del keep
            except Exception as e:      # noqa: BLE001
                import traceback
                errs.append(traceback.format_exc()[-1500:] or repr(e))

        ts = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
        [t.start() for t in ts]; [t.join(timeout=300) for t in ts]
        q.put(errs if errs else res)
    except Exception as e:      # noqa: BLE001
        import traceback
        q.put([traceback.format_exc()[-1500:] or repr(e)])


@pytest.mark.parametrize("transport", ["host", "loopback_rccl"])
def test_ms_dist_track_gains_views_through_the_binding(ms, cuda, transport):
    """msdist.Dist.track_gains_views from two ranks sharing the GPU: both reach ms_track_gains' gains; when one rank's frame is refused it returns the error while
    both ranks count one rejected update and keep their gains."""
    cfg = synth.CONFIGS["mini6"]
    frames_np = frames_of(cfg, 0, scale={3: 0.7})
    ref, _, g0 = make_rig(ms, "mini6")
    ref.track_gains([to_dev(f) for f in frames_np], stride=2, smoothing=1.0)
    want = ref.gains()
    assert np.abs(want - np.asarray(g0)).max() > 1e-3
    if transport == "host":
        import queue
        q = queue.Queue()
        _two_ranks("host", None, frames_np, q)
        res = q.get(timeout=1)
    else:
        import torch.multiprocessing as mp
        assert os.path.isfile(FAKE_RCCL), "tests/_fake_rccl/libfake_rccl.so is built by __graft_entry__.build()"
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        p = ctx.Process(target=_two_ranks, args=("rccl", FAKE_RCCL, frames_np, q))      # (one process: this one keeps the real RCCL for the other tests)
        p.start()
        res = q.get(timeout=300)
        p.join(timeout=60)
        assert p.exitcode == 0, p.exitcode
    assert isinstance(res, dict), res
    for r in range(2):
        g1, c1, refused, g2, c2 = res[r]
        assert np.array_equal(bits(g1), bits(want)) and c1 == (1, 0, 0), (r, g1, want, c1)
        assert np.array_equal(bits(g2), bits(g1)) and c2 == (1, 0, 1), (r, c2)      # the refusing rank counts the rejection too: the group's counters stay equal
        assert (refused is not None) == (r == 1), (r, refused)
    ref.close()


def test_a_peer_list_that_does_not_match_the_shards_is_refused_before_anything_moves(ms, cuda):
    """The slots of the scratch buffer are sized per shard and differ in size: a context that is not shard `position in peers` of `len(peers)` would write
    another block's buffer into its slot.  Both ranks of a host-transport pair get MS_ERR_INVALID for peers out of shard order and for contexts of a three-shard
    rig in a group of two; nothing is posted (no rank waits), the scratch buffer is untouched, nothing is counted, and a correct call afterwards tracks."""
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
                cur = torch.cuda.current_stream()
                d = msdist.Dist(r, 2, idb, device=0)
                comp = make_rig(ms, "mini6", shards=2, shard_index=r)[0]
                three = make_rig(ms, "mini6", shards=3, shard_index=r)[0]
                frames = [to_dev(f) for f in frames_np]
                total = sum(comp.gain_samples_bytes(2, k) for k in range(2))
                scratch = torch.full((total // 4,), -5, dtype=torch.int32, device="cuda")
                rcs = [_rc(ms, lambda: d.track_gains_views(comp, [1, 0], frames, scratch=scratch, stride=2, smoothing=1.0)),
                       _rc(ms, lambda: d.track_gains_views(three, [0, 1], frames, scratch=scratch, stride=2, smoothing=1.0)),
                       _rc(ms, lambda: d.track_gains_views(comp, [r], frames, scratch=scratch, stride=2, smoothing=1.0)),
                       _rc(ms, lambda: d.track_gains_views(comp, [0, 0], frames, scratch=scratch, stride=2, smoothing=1.0)),
                       _rc(ms, lambda: d.track_gains_views(comp, [1 - r], frames, scratch=scratch, stride=2, smoothing=1.0))]
                cur.synchronize()
                untouched = bool((scratch == -5).all())
                counted = (comp.gain_track_counters(stream=cur), three.gain_track_counters(stream=cur))
                d.track_gains_views(comp, [0, 1], only(frames, comp.gain_sample_views()), scratch=scratch, stride=2, smoothing=1.0)
                res[r] = (rcs, untouched, counted, comp.gains(stream=cur), comp.gain_track_counters(stream=cur))
                d.barrier(); d.close(); comp.close(); three.close()
        except Exception as e:      # noqa: BLE001
            import traceback
            errs.append(traceback.format_exc()[-1500:] or repr(e))

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join(timeout=300) for t in ts]
    assert not errs, errs
    for r in range(2):
        rcs, untouched, counted, g, c = res[r]
        assert rcs == [MS_ERR_INVALID] * 5, (r, rcs)
        assert untouched, "rank %d: a refused call wrote into the scratch buffer" % r
        assert counted == ((0, 0, 0), (0, 0, 0))
        assert np.array_equal(bits(g), bits(want)) and c == (1, 0, 0), (r, g, want, c)
    ref.close()
