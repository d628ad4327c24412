"""Exposure tracking on column shards at the C-ABI, without a device: the entry points are declared, exported and bound; the argument checks that do not need a
context answer MS_ERR_INVALID with a message; and tests/gain_partial_ref.py, the numpy restatement the GPU tests compare against, is checked against
tests/gain_ref.py: the window partials of S = 2, 3, 4 column windows add up to the unsharded cnt and S exactly -- on random geometry and on the rigs the GPU
tests use (maps from the oracle's warper), where every window must also hold a pair of different views with samples."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gain_partial_ref as P
import gain_ref as G
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_get_gain_views", "ms_gain_stats_partial", "ms_gain_stats_partial_nv12", "ms_track_gains_from_partials", "ms_get_gain_track_counters")
DIST_NAMES = ("ms_dist_track_gains",)
MS_ERR_INVALID = -1


def test_declared_exported_and_bound(ms):
    import msdist
    lib = ms.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+ms_gain_track_counters\s*\{", text)
    assert re.search(r"MS_API\s+size_t\s+ms_gain_partial_bytes\s*\(", text) and hasattr(lib, "ms_gain_partial_bytes") and "ms_gain_partial_bytes" in ms.EXPORTS
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in ms_stitch.h" % n
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
        assert n in ms.EXPORTS
    dist = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_dist.h")).read(), flags=re.S)
    for n in DIST_NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, dist) and hasattr(lib, n) and n in msdist.EXPORTS
    for m in ("gain_partial_bytes", "new_gain_partial", "gain_views", "gain_stats_partial", "track_gains_from_partials", "gain_track_counters"):
        assert callable(getattr(ms.Compositor, m))
    assert callable(msdist.Dist.track_gains)
    assert C.sizeof(ms.GainTrackCounters) == 16


def _invalid(lib, rc, words):
    assert rc == MS_ERR_INVALID
    msg = lib.ms_last_error().decode()
    assert words in msg, msg


def test_argument_checks_without_a_context(ms):
    lib = ms.load()
    lib.ms_gain_partial_bytes.restype = C.c_size_t
    prm = ms.gain_track_default_params()
    views = (ms.Image * 2)()
    buf = C.c_void_p(0x1000)                        # never dereferenced: every call below is refused before it touches memory
    two = (C.c_void_p * 2)(0x1000, 0x2000)
    k = ms.GainTrackCounters(struct_size=C.sizeof(ms.GainTrackCounters))
    m = C.c_uint(0)
    # null context, everything else in order
    assert lib.ms_gain_partial_bytes(None) == 0 and b"null context" in lib.ms_last_error()
    for fn in (lib.ms_gain_stats_partial, lib.ms_gain_stats_partial_nv12):
        _invalid(lib, fn(None, views, 1, buf, None), "null context")
        _invalid(lib, fn(None, views, 1, None, None), "partial")
        _invalid(lib, fn(None, views, 1, C.c_void_p(0x1004), None), "8-byte aligned")
        _invalid(lib, fn(None, None, 1, buf, None), "null views")
        _invalid(lib, fn(None, views, 0, buf, None), "stride 0 < 1")
    f = lib.ms_track_gains_from_partials
    _invalid(lib, f(None, two, 2, C.byref(prm), None), "null context")
    _invalid(lib, f(None, two, 2, None, None), "null params")
    _invalid(lib, f(None, None, 2, C.byref(prm), None), "null partials")
    _invalid(lib, f(None, two, 0, C.byref(prm), None), "0 partials")
    _invalid(lib, f(None, two, 17, C.byref(prm), None), "17 partials")
    _invalid(lib, f(None, (C.c_void_p * 2)(0x1000, None), 2, C.byref(prm), None), "partial 1 is null")
    _invalid(lib, f(None, (C.c_void_p * 2)(0x1000, 0x2002), 2, C.byref(prm), None), "partial 1 is null or not 8-byte aligned")
    bad = ms.gain_track_default_params(); bad.struct_size += 8
    _invalid(lib, f(None, two, 2, C.byref(bad), None), "struct_size")
    for lam in (0.0, -0.5, 1.5, float("nan")):
        bad = ms.gain_track_default_params(); bad.smoothing = lam
        _invalid(lib, f(None, two, 2, C.byref(bad), None), "smoothing")
    bad = ms.gain_track_default_params(); bad.stride = 0
    _invalid(lib, f(None, two, 2, C.byref(bad), None), "stride 0 < 1")
    _invalid(lib, lib.ms_get_gain_track_counters(None, C.byref(k), None), "null context")
    _invalid(lib, lib.ms_get_gain_track_counters(None, None, None), "null output")
    k.struct_size += 4
    _invalid(lib, lib.ms_get_gain_track_counters(None, C.byref(k), None), "struct_size")
    _invalid(lib, lib.ms_get_gain_views(None, C.byref(m)), "null context")
    _invalid(lib, lib.ms_get_gain_views(None, None), "null output")
    _invalid(lib, lib.ms_dist_track_gains(None, None, None, 0, views, 0, C.byref(prm), buf, None), "null")


def test_col_windows_are_a_partition_on_multiples_of_16():
    for fw in (17, 100, 512, 640, 641, 3839, 7680):
        for S in (1, 2, 3, 4, 16):
            w = P.col_windows(fw, S)
            assert w[0][0] == 0 and w[-1][1] == fw and all(a[1] == b[0] for a, b in zip(w, w[1:]))
            assert all(b % 16 == 0 for b, _ in w[1:])


def _random_geometry(rng, n):
    rois = [(-60 + 45 * i + int(rng.integers(-5, 6)), int(rng.integers(-8, 9)), int(rng.integers(70, 100)), int(rng.integers(50, 70))) for i in range(n)]
    x0, y0 = min(r[0] for r in rois), min(r[1] for r in rois)
    T = (x0, y0, max(r[0] + r[2] for r in rois) - x0, max(r[1] + r[3] for r in rois) - y0)
    seen = [rng.random((r[3], r[2])) < 0.85 for r in rois]
    q = [np.where(s, rng.integers(0, 1 << 29, size=s.shape), 0).astype(np.int64) for s in seen]
    return rois, seen, q, T


@pytest.mark.parametrize("S", [2, 3, 4])
def test_window_partials_sum_to_the_unsharded_statistic_random_geometry(S):
    rng = np.random.default_rng(100 + S)
    for n in (3, 6):
        rois, seen, q, T = _random_geometry(rng, n)
        for active in ((1 << n) - 1, ((1 << n) - 1) & ~2):
            for stride in (1, 3, 4):
                N, Sm, cnt = G.stats(rois, seen, q, T, stride, active)
                parts = [P.window_stats(rois, seen, q, T, stride, w, active) for w in P.col_windows(T[2], S)]
                csum, ssum = sum(p[0] for p in parts), sum(p[1] for p in parts)
                assert np.array_equal(csum, cnt) and np.array_equal(ssum, Sm), (n, active, stride)
                fN, fS = P.finish(rois, csum, ssum, active)
                assert np.array_equal(fN, N) and np.array_equal(fS, Sm)
                one = P.window_stats(rois, seen, q, T, stride, (0, T[2]), active)
                assert np.array_equal(one[0], cnt) and np.array_equal(one[1], Sm)


def oracle_rig(oracle, name):
    """rois, maps and pano ROI of a synth rig as the compositor builds them, from the oracle's warper (spherical)."""
    c = synth.CONFIGS[name]
    sc = synth.warp_scale(c["out_w"])
    rois, maps = [], []
    for i in range(c["n"]):
        K, R = synth.camera(c["n"], c["w"], c["h"], c["hfov_deg"], i)
        r = oracle.warp_roi(2, K, R, sc, c["w"], c["h"])
        rois.append(r)
        maps.append(oracle.build_maps_cpu(2, oracle.projector(K, R, sc), r[0], r[1], r[3], r[2]))
    dst = oracle.result_roi([r[:2] for r in rois], [r[2:] for r in rois])
    T = oracle.blender_prepare(dst, c["num_bands"]).dst_roi_final.tuple()
    return c, rois, maps, T


@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_every_window_of_the_test_rigs_holds_a_pair_with_samples(oracle, rig):
    """The condition of the GPU partition test, checked here before the rig is fixed there: for S = 2, 3, 4 and strides 1 and 4 every window's partial
    has a pair i != j with cnt > 0 -- and the partials add up to gain_ref's statistic."""
    c, rois, maps, T = oracle_rig(oracle, rig)
    frames = [synth.frame(c["w"], c["h"], i, 2) for i in range(c["n"])]
    seen, q = zip(*[G.sample_view(mx, my, f) for (mx, my), f in zip(maps, frames)])
    for stride in (1, 4):
        N, Sm, cnt = G.stats(rois, seen, q, T, stride)
        for S in (2, 3, 4):
            parts = [P.window_stats(rois, seen, q, T, stride, w) for w in P.col_windows(T[2], S)]
            for k, p in enumerate(parts):
                assert P.has_cross_pair(p[0]), "%s: window %d of %d holds no pair of different views with samples at stride %d" % (rig, k, S, stride)
            assert np.array_equal(sum(p[0] for p in parts), cnt) and np.array_equal(sum(p[1] for p in parts), Sm)
