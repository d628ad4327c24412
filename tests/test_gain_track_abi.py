"""Exposure tracking at the C-ABI: the five entry points are declared, exported and listed, refuse a null context without a device; and tests/gain_ref.py,
the numpy restatement the GPU tests compare against, is checked against itself (its solve minimises the energy) and against the oracle's GainCompensator."""
import ctypes as C
import os
import re

import numpy as np

import gain_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_gain_track_default_params", "ms_gain_stats", "ms_track_gains", "ms_get_gains")


def test_declared_exported_and_listed(ms):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ms_stitch.h")).read(), flags=re.S)
    lib = ms.load()
    assert re.search(r"typedef\s+struct\s+ms_gain_track_params\s*\{", text), "ms_gain_track_params is not declared in ms_stitch.h"
    for n in NAMES:
        assert re.search(r"MS_API\s+int\s+%s\s*\(" % n, text), "%s is not declared in ms_stitch.h" % n
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
        assert n in ms.EXPORTS


def test_null_context_is_invalid(ms):
    lib = ms.load()
    prm = ms.gain_track_default_params()
    n, s, g = (C.c_longlong * 4)(), (C.c_longlong * 4)(), (C.c_double * 2)()
    for rc in (lib.ms_gain_stats(None, None, 1, n, s, None), lib.ms_track_gains(None, None, C.byref(prm), None), lib.ms_get_gains(None, g, None, None, None)):
        assert rc == -1       # MS_ERR_INVALID
        assert b"null context" in lib.ms_last_error()
    assert lib.ms_gain_track_default_params(None) == -1


def test_default_params(ms):
    p = ms.gain_track_default_params()
    assert p.struct_size == C.sizeof(ms.GainTrackParams) == 16
    assert p.stride >= 1 and 0.0 < p.smoothing <= 1.0


def _random_system(rng, n):
    N = np.zeros((n, n), np.int64)
    I = np.zeros((n, n))
    for i in range(n):
        N[i, i] = rng.integers(2000, 9000)
        I[i, i] = rng.uniform(60, 200)
        for j in (i + 1, i + 2):                 # every view overlaps its next two (a ring): well covered
            j %= n
            if j == i or N[i, j]:
                continue
            N[i, j] = N[j, i] = rng.integers(300, 1500)
            base = rng.uniform(60, 200)
            I[i, j], I[j, i] = base * rng.uniform(0.7, 1.3), base * rng.uniform(0.7, 1.3)
    return N, I


def test_solve_minimises_the_energy():
    rng = np.random.default_rng(11)
    for n in (2, 3, 4, 6, 9):
        N, I = _random_system(rng, n)
        A, b = G.normal_equations(N, I)
        g = np.linalg.solve(A, b)
        e0 = G.energy(N, I, g)
        for k in range(n):
            for d in (-1e-3, 1e-3):
                h = g.copy(); h[k] += d
                assert e0 <= G.energy(N, I, h), "n=%d: E decreases along e_%d (%g)" % (n, k, d)


def test_agrees_with_the_oracle_gain_compensator(oracle):
    """The same pixels as full images: warped views with arbitrary masks at arbitrary corners (stride 1, T = their bounding box)."""
    rng = np.random.default_rng(3)
    n = 5
    corners = [(-40 + 37 * i + int(rng.integers(-4, 5)), int(rng.integers(-6, 7))) for i in range(n)]
    sizes = [(int(rng.integers(60, 80)), int(rng.integers(50, 64))) for _ in range(n)]
    imgs, masks = [], []
    for i, (w, h) in enumerate(sizes):
        base = rng.integers(40, 200, size=(h, w, 3)).astype(np.float64) * (0.75 + 0.1 * i)
        imgs.append(np.clip(base, 0, 255).astype(np.uint8))
        m = np.where(rng.random((h, w)) < 0.9, 255, 0).astype(np.uint8)
        masks.append(m)
    ref = np.array(oracle.gain_compensator(corners, imgs, masks))
    rois = [(c[0], c[1], s[0], s[1]) for c, s in zip(corners, sizes)]
    x0, y0 = min(r[0] for r in rois), min(r[1] for r in rois)
    T = (x0, y0, max(r[0] + r[2] for r in rois) - x0, max(r[1] + r[3] for r in rois) - y0)
    seen = [m == 255 for m in masks]
    q = [np.where(s, G.q_of(im), 0) for s, im in zip(seen, imgs)]
    N, S, cnt = G.stats(rois, seen, q, T, 1)
    assert all(cnt[i, (i + 1)] > 0 for i in range(n - 1)), "the comparison needs overlaps"
    _, g = G.solve(N, S)
    print("gain_ref", g, "oracle", ref, "max rel", np.abs(g / ref - 1).max())
    np.testing.assert_allclose(g, ref, rtol=1e-5, atol=0)
