"""Exposure tracking on view shards at the C-ABI, without a device: the entry points are declared, exported and bound; the argument checks that do not need a
context answer MS_ERR_INVALID with a message; and tests/gain_samples_ref.py, the numpy restatement the GPU tests compare against, is checked against
tests/gain_ref.py: the pair sums formed from the per-view vectors of S = 2, 3, 4 shards' buffers equal the direct statistic exactly, on random geometry."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import gain_partial_ref as P
import gain_ref as G
import gain_samples_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_get_view_shard", "ms_get_gain_sample_views", "ms_gain_samples", "ms_gain_samples_nv12", "ms_gain_stats_from_samples", "ms_track_gains_from_samples")
MS_ERR_INVALID = -1


def test_declared_exported_and_bound(ms):
    import msdist
    lib = ms.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    assert re.search(r"MS_API\s+size_t\s+ms_gain_samples_bytes\s*\(", text) and hasattr(lib, "ms_gain_samples_bytes") and "ms_gain_samples_bytes" in ms.EXPORTS
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in ms_stitch.h" % n
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
        assert n in ms.EXPORTS
    dist = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_dist.h")).read(), flags=re.S)
    n = "ms_dist_track_gains_views"
    assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, dist) and hasattr(lib, n) and n in msdist.EXPORTS
    for m in ("gain_samples_bytes", "view_shard", "gain_sample_views", "gain_samples", "gain_samples_nv12", "gain_stats_from_samples", "track_gains_from_samples"):
        assert callable(getattr(ms.Compositor, m))
    assert callable(msdist.Dist.track_gains_views)
    assert ms.GAIN_SAMPLES_MAGIC == R.MAGIC != ms.GAIN_PARTIAL_MAGIC and ms.GAIN_SAMPLES_HEADER_WORDS == R.HEADER_WORDS == 16


def _invalid(lib, rc, words):
    assert rc == MS_ERR_INVALID
    msg = lib.ms_last_error().decode()
    assert words in msg, msg


def test_argument_checks_without_a_context(ms):
    lib = ms.load()
    lib.ms_gain_samples_bytes.restype = C.c_size_t
    prm = ms.gain_track_default_params()
    views = (ms.Image * 2)()
    buf = C.c_void_p(0x1000)                        # never dereferenced: every call below is refused before it touches memory
    two = (C.c_void_p * 2)(0x1000, 0x2000)
    N = (C.c_longlong * 4)()
    m = C.c_uint(0)
    assert lib.ms_gain_samples_bytes(None, 1, -1) == 0 and b"null context" in lib.ms_last_error()
    for fn in (lib.ms_gain_samples, lib.ms_gain_samples_nv12):
        _invalid(lib, fn(None, views, 1, buf, None), "null context")
        _invalid(lib, fn(None, views, 1, None, None), "samples")
        _invalid(lib, fn(None, views, 1, C.c_void_p(0x1002), None), "4-byte aligned")
        _invalid(lib, fn(None, None, 1, buf, None), "null views")
        _invalid(lib, fn(None, views, 0, buf, None), "stride 0 < 1")
    f = lib.ms_track_gains_from_samples
    _invalid(lib, f(None, two, 2, C.byref(prm), None), "null context")
    _invalid(lib, f(None, two, 2, None, None), "null params")
    _invalid(lib, f(None, None, 2, C.byref(prm), None), "null samples")
    _invalid(lib, f(None, two, 0, C.byref(prm), None), "0 sample buffers")
    _invalid(lib, f(None, two, 5, C.byref(prm), None), "5 sample buffers")
    _invalid(lib, f(None, (C.c_void_p * 2)(0x1000, None), 2, C.byref(prm), None), "sample buffer 1 is null")
    _invalid(lib, f(None, (C.c_void_p * 2)(0x1000, 0x2002), 2, C.byref(prm), None), "sample buffer 1 is null or not 4-byte aligned")
    bad = ms.gain_track_default_params(); bad.struct_size += 8
    _invalid(lib, f(None, two, 2, C.byref(bad), None), "struct_size")
    for lam in (0.0, -0.5, 1.5, float("nan")):
        bad = ms.gain_track_default_params(); bad.smoothing = lam
        _invalid(lib, f(None, two, 2, C.byref(bad), None), "smoothing")
    bad = ms.gain_track_default_params(); bad.stride = 0
    _invalid(lib, f(None, two, 2, C.byref(bad), None), "stride 0 < 1")
    g = lib.ms_gain_stats_from_samples
    _invalid(lib, g(None, two, 2, 1, N, N, None), "null context")
    _invalid(lib, g(None, two, 2, 1, None, N, None), "null output")
    _invalid(lib, g(None, None, 2, 1, N, N, None), "null samples")
    _invalid(lib, g(None, two, 5, 1, N, N, None), "5 sample buffers")
    _invalid(lib, g(None, two, 2, 0, N, N, None), "stride 0 < 1")
    _invalid(lib, lib.ms_get_gain_sample_views(None, C.byref(m)), "null context")
    _invalid(lib, lib.ms_get_gain_sample_views(None, None), "null output")
    a, b = C.c_int(0), C.c_int(0)
    _invalid(lib, lib.ms_get_view_shard(None, C.byref(a), C.byref(b)), "null context")
    _invalid(lib, lib.ms_get_view_shard(None, None, C.byref(b)), "null output")
    _invalid(lib, lib.ms_dist_track_gains_views(None, None, None, 0, views, 0, C.byref(prm), buf, None), "null")


def test_shard_blocks_partition_the_views():
    for n in (2, 4, 6, 12, 16):
        for S in (1, 2, 3, 4):
            if S > n:
                continue
            masks = [R.shard_views(n, S, k) for k in range(S)]
            assert sum(masks) == (1 << n) - 1 and all(a & b == 0 for a, b in itertools.combinations(masks, 2))


def test_lattice_rect_is_the_set_of_samples_inside_the_roi():
    rng = np.random.default_rng(5)
    for _ in range(200):
        T = (int(rng.integers(-50, 50)), int(rng.integers(-50, 50)), int(rng.integers(1, 90)), int(rng.integers(1, 90)))
        roi = (T[0] + int(rng.integers(0, T[2])), T[1] + int(rng.integers(0, T[3])), int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        roi = (roi[0], roi[1], min(roi[2], T[0] + T[2] - roi[0]), min(roi[3], T[1] + T[3] - roi[1]))
        stride = int(rng.integers(1, 12))
        sx0, sy0, w, h = R.lattice_rect(roi, T, stride)
        inside = {(sx, sy) for sx in range(-(-T[2] // stride)) for sy in range(-(-T[3] // stride))
                  if roi[0] <= T[0] + sx * stride < roi[0] + roi[2] and roi[1] <= T[1] + sy * stride < roi[1] + roi[3]}
        assert inside == {(sx0 + i, sy0 + j) for i in range(w) for j in range(h)}


def _random_geometry(rng, n):
    rois = [(-60 + 45 * i + int(rng.integers(-5, 6)), int(rng.integers(-8, 9)), int(rng.integers(70, 100)), int(rng.integers(50, 70))) for i in range(n)]
    x0, y0 = min(r[0] for r in rois), min(r[1] for r in rois)
    T = (x0, y0, max(r[0] + r[2] for r in rois) - x0, max(r[1] + r[3] for r in rois) - y0)
    seen = [rng.random((r[3], r[2])) < 0.85 for r in rois]
    q = [np.where(s, rng.integers(0, 1 << 29, size=s.shape), 0).astype(np.int64) for s in seen]
    return rois, seen, q, T


@pytest.mark.parametrize("S", [2, 3, 4])
def test_pair_sums_from_per_view_vectors_equal_the_direct_statistic_random_geometry(S):
    rng = np.random.default_rng(200 + S)
    for n in (4, 6):
        rois, seen, q, T = _random_geometry(rng, n)
        for active in ((1 << n) - 1, ((1 << n) - 1) & ~2):
            for stride in (1, 3, 4, 64):            # (64: rectangles one or two samples wide)
                N, Sm, cnt = G.stats(rois, seen, q, T, stride, active)
                bufs = [R.buffer(rois, seen, q, T, stride, R.shard_views(n, S, k), active) for k in range(S)]
                vectors, held_all = {}, 0
                for k, b in enumerate(bufs):
                    hdr, views = R.parse(b, rois, T)
                    assert hdr["magic"] == R.MAGIC and hdr["num_views"] == n and hdr["active"] == active and hdr["stride"] == stride and hdr["T"] == T
                    assert hdr["held"] == R.shard_views(n, S, k) & active and hdr["bytes"] == b.size * 4 and not any(hdr["rest"])
                    assert held_all & hdr["held"] == 0
                    held_all |= hdr["held"]
                    vectors.update(views)
                assert held_all == active
                c, s = R.pair_sums(rois, T, stride, vectors, active)
                # gain_ref keeps cnt and S on the pairs whose ROIs meet only; outside them no sample is shared, so the raw sums are 0 there anyway
                fN, fS = P.finish(rois, c, s, active)
                assert np.array_equal(fN, N) and np.array_equal(fS, Sm), (n, active, stride)
                meet = np.array([[G.rects_meet(rois[i], rois[j]) for j in range(n)] for i in range(n)])
                assert not c[~meet].any() and np.array_equal(np.where(meet, c, 0), cnt)
