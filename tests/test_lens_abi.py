"""The lens model (ms_lens) without a GPU: the numpy reference against closed forms, ms_lens_project against the reference, every refusal of ms_lens_check,
null arguments, and the binding's constants against the header."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lens_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[160.0, 0.25, 161.5], [0, 158.0, 88.25], [0, 0, 1]], np.float32)


def seeded_rays(n, seed):
    """unit rays over the whole sphere (Z < 0 included), a few on the axis, a band of them within a degree either side of 75 and of 100 degrees"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:4] = [[0, 0, 1], [0, 0, 2.5], [0, 0, -1], [1e-300, 0, 1]]
    m = n // 4
    for lo, centre in ((4, 75.0), (4 + m, 100.0)):
        th = np.radians(centre + rng.uniform(-1, 1, m))
        ph = rng.uniform(0, 2 * math.pi, m)
        d[lo:lo + m] = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1) * rng.uniform(0.5, 3, (m, 1))
    return d


# ---- the reference against closed forms ----------------------------------------------------------------------------
def test_reference_zero_coefficients_are_the_pinhole():
    d = seeded_rays(2000, 1)
    front = d[d[:, 2] > 0.05]
    X, Y, Z = front.T
    want_x = K[0, 0] * (X / Z) + K[0, 1] * (Y / Z) + K[0, 2]
    want_y = K[1, 1] * (Y / Z) + K[1, 2]
    for lens in (L.NONE, L.BROWN_ZERO):
        px, py, seen = L.project(K, lens, X, Y, Z)
        inside = np.arctan2(np.hypot(X, Y), Z) <= math.radians(89) if lens is L.BROWN_ZERO else np.ones(len(X), bool)
        assert np.array_equal(seen, inside)
        assert np.allclose(px[seen], want_x[seen], rtol=0, atol=1e-9) and np.allclose(py[seen], want_y[seen], rtol=0, atol=1e-9)
    _, _, seen = L.project(K, L.NONE, d[:, 0], d[:, 1], d[:, 2])
    assert np.array_equal(seen, d[:, 2] > 0)


def test_reference_equidistant_fisheye_and_the_axis():
    f = 100.0
    Kf = np.array([[f, 0, 0], [0, f, 0], [0, 0, 1]], np.float64)
    d = seeded_rays(2000, 2)
    X, Y, Z = d.T
    px, py, seen = L.project(Kf, ("fisheye", (0, 0, 0, 0), 0.0), X, Y, Z)
    assert seen.all()       # the default 180 degrees sees every ray
    theta = np.arctan2(np.hypot(X, Y), Z)
    off = np.hypot(X, Y) > 0
    assert np.allclose(np.hypot(px, py)[off], f * theta[off], rtol=0, atol=1e-9)      # r = f * theta
    assert (px[~off] == 0).all() and (py[~off] == 0).all() and (~off).sum() == 3      # rho = 0: (0, 0), straight behind included
    assert np.allclose(np.arctan2(py[off], px[off]), np.arctan2(Y[off], X[off]), rtol=0, atol=1e-9)
    for lens in (L.NONE, L.BROWN, L.FISH):                                 # rho = 0: the principal point
        px, py, seen = L.project(K, lens, [0.0], [0.0], [2.0])
        assert seen[0] and px[0] == K[0, 2] and py[0] == K[1, 2]
    px, py, seen = L.project(K, L.FISH, [0.0], [0.0], [-1.0])               # straight behind: theta = 180 > 100
    assert not seen[0] and px[0] == -1 and py[0] == -1


# ---- ms_lens_project against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["none", "brown", "fisheye"])
def test_lens_project_matches_the_reference(ms, name):
    """|delta| <= 1e-9 px: both sides are a dozen double operations on values <= 1e3"""
    lens = {"none": L.NONE, "brown": L.BROWN, "fisheye": L.FISH}[name]
    d = seeded_rays(3000, 3)
    px, py, seen = L.project(K, lens, d[:, 0], d[:, 1], d[:, 2])
    mt = L.max_theta(lens)
    theta = np.arctan2(np.hypot(d[:, 0], d[:, 1]), d[:, 2])
    if mt is not None:
        assert (np.abs(theta - mt) > 1e-9).all()
        assert seen.sum() > 500 and (~seen).sum() > 500 and (seen & (np.abs(theta - mt) < math.radians(1))).any() and (~seen & (np.abs(theta - mt) < math.radians(1))).any()
    if name == "fisheye":
        assert (seen & (d[:, 2] < 0)).sum() > 50       # past 90 degrees
    mslens = L.to_ms(ms, lens)
    worst = 0.0
    for i in range(len(d)):
        (gx, gy), gseen = ms.lens_project(K, mslens, d[i])
        assert gseen == bool(seen[i]), (i, d[i])
        if not gseen:
            assert (gx, gy) == (-1.0, -1.0)
        elif abs(px[i]) <= 1e3 and abs(py[i]) <= 1e3:
            worst = max(worst, abs(gx - px[i]), abs(gy - py[i]))
        else:
            assert abs(gx - px[i]) <= 1e-12 * abs(px[i]) + 1e-9 and abs(gy - py[i]) <= 1e-12 * abs(py[i]) + 1e-9
    assert worst <= 1e-9, worst


# ---- ms_lens_check ------------------------------------------------------------------------------------------------------
def _check(ms, lens):
    rc = ms.load().ms_lens_check(C.byref(lens) if lens is not None else None)
    return rc, ms.load().ms_last_error().decode()


def test_lens_check_accepts_and_refuses(ms):
    for lens in (L.BROWN, L.FISH, L.BROWN_ZERO, ("fisheye", (0, 0, 0, 0), 0.0), ("brown", (-0.18, 0.03, 1e-3, -5e-4, 0.01, 0.02, 0.001, 0.0), 60.0)):
        assert _check(ms, L.to_ms(ms, lens))[0] == 0, lens
    assert _check(ms, ms.Lens.make(ms.LENS_NONE, [float("nan")] * 8))[0] == 0      # MS_LENS_NONE: k is not looked at
    bad = {
        "null": None,
        "struct_size": ms.Lens(C.sizeof(ms.Lens) - 8, ms.LENS_BROWN),
        "unknown model": ms.Lens.make(3),
        "negative model": ms.Lens.make(-1),
        "nan coefficient": ms.Lens.brown(0.1, float("nan")),
        "inf coefficient": ms.Lens.fisheye(0.0, 0.0, float("inf")),
        "fisheye k[4]": ms.Lens.make(ms.LENS_FISHEYE, [0, 0, 0, 0, 1e-3]),
        "fisheye k[7]": ms.Lens.make(ms.LENS_FISHEYE, [0, 0, 0, 0, 0, 0, 0, -1e-9]),
        "brown theta above 89": ms.Lens.brown(0.0, max_theta_deg=89.5),
        "brown theta negative": ms.Lens.brown(0.0, max_theta_deg=-1.0),
        "fisheye theta above 180": ms.Lens.fisheye(0.0, max_theta_deg=180.5),
        "theta nan": ms.Lens.fisheye(0.0, max_theta_deg=float("nan")),
        "brown folds back": ms.Lens.brown(-0.5, max_theta_deg=60.0),
        "brown folds back at the default 89": ms.Lens.brown(-0.18, 0.03, 1e-3, -5e-4, -0.01),
        "fisheye folds back": ms.Lens.fisheye(-0.2, max_theta_deg=100.0),
        "brown pole of cdist": ms.Lens.brown(0, 0, 0, 0, 0, -1.0, max_theta_deg=60.0),
    }
    for name, lens in bad.items():
        rc, msg = _check(ms, lens)
        assert rc == -1 and "ms_lens_check" in msg, (name, rc, msg)
        if "folds" in name:
            assert "max_theta_deg" in msg and "lower" in msg, msg
    # k1 = -0.5: r (1 - 0.5 r^2) turns at r = sqrt(2 / 3) = 0.816 = tan 39.2 degrees
    assert _check(ms, ms.Lens.brown(-0.5, max_theta_deg=35.0))[0] == 0
    assert _check(ms, ms.Lens.brown(-0.5, max_theta_deg=39.0))[0] == 0 and _check(ms, ms.Lens.brown(-0.5, max_theta_deg=39.5))[0] == -1
    # the tangential terms are not part of the check
    assert _check(ms, ms.Lens.brown(0.0, 0.0, 5.0, -5.0, max_theta_deg=60.0))[0] == 0
    with pytest.raises(ms.MsError):
        ms.lens_check(ms.Lens.brown(-0.5, max_theta_deg=60.0))
    ms.lens_check(L.to_ms(ms, L.BROWN))


def test_null_arguments_and_host_side_refusals(ms):
    """everything that is refused before a device is looked for"""
    lib = ms.load()
    Kp = (C.c_float * 9)(*K.reshape(9))
    ray, px, seen = (C.c_double * 3)(0, 0, 1), (C.c_double * 2)(), C.c_int()
    good = L.to_ms(ms, L.BROWN)
    assert lib.ms_lens_project(Kp, C.byref(good), ray, px, C.byref(seen)) == 0 and seen.value == 1
    assert lib.ms_lens_project(Kp, None, ray, px, C.byref(seen)) == 0 and (px[0], px[1]) == (float(K[0, 2]), float(K[1, 2]))      # NULL lens = MS_LENS_NONE
    for args in ((None, C.byref(good), ray, px, C.byref(seen)), (Kp, C.byref(good), None, px, C.byref(seen)), (Kp, C.byref(good), ray, None, C.byref(seen)),
                 (Kp, C.byref(good), ray, px, None)):
        assert lib.ms_lens_project(*args) == -1 and b"ms_lens_project" in lib.ms_last_error()
    folded = ms.Lens.brown(-0.5, max_theta_deg=60.0)
    assert lib.ms_lens_project(Kp, C.byref(folded), ray, px, C.byref(seen)) == -1
    r = ms.Rect()
    im = ms.Image(None, 0, 0, 0, ms.MS_32FC1)
    assert lib.ms_warp_roi_lens(ms.PROJ_SPHERICAL, None, Kp, None, C.c_float(50.0), 64, 48, C.byref(r), None) == -1
    assert lib.ms_warp_roi_lens(ms.PROJ_SPHERICAL, Kp, Kp, None, C.c_float(50.0), 64, 48, None, None) == -1
    assert lib.ms_warp_roi_lens(ms.PROJ_SPHERICAL, Kp, Kp, None, C.c_float(50.0), 0, 48, C.byref(r), None) == -1
    assert lib.ms_warp_roi_lens(ms.PROJ_SPHERICAL, Kp, Kp, C.byref(folded), C.c_float(50.0), 64, 48, C.byref(r), None) == -1
    assert lib.ms_warp_roi_lens(ms.PROJ_PLANE, Kp, Kp, C.byref(good), C.c_float(50.0), 64, 48, C.byref(r), None) == -2      # MS_ERR_UNSUPPORTED
    assert lib.ms_build_warp_maps_lens(ms.PROJ_SPHERICAL, 0, 0, C.byref(im), C.byref(im), None, Kp, None, C.c_float(50.0), None) == -1
    assert lib.ms_build_warp_maps_lens(ms.PROJ_SPHERICAL, 0, 0, C.byref(im), C.byref(im), Kp, Kp, C.byref(folded), C.c_float(50.0), None) == -1
    assert lib.ms_build_warp_maps_lens(ms.PROJ_PLANE, 0, 0, C.byref(im), C.byref(im), Kp, Kp, C.byref(good), C.c_float(50.0), None) == -2
    assert lib.ms_set_lens(None, 0, C.byref(good)) == -1 and lib.ms_get_lens(None, 0, C.byref(good)) == -1


def test_binding_constants_equal_the_headers(ms, tmp_path):
    """the header's values as a C compiler sees them"""
    names = ["MS_LENS_NONE", "MS_LENS_BROWN", "MS_LENS_FISHEYE", "MS_MAPS_ANALYTIC", "MS_MAPS_CUSTOM", "MS_MAPS_LENS", "MS_LENS_CYL_MAX_ELEVATION_DEG"]
    src = tmp_path / "consts.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ms_stitch.h"\nint main(void) { printf("' + " ".join(["%d"] * len(names)) + ' %zu %zu %zu %zu %zu\\n", '
                   + ", ".join(names) + ", sizeof(ms_lens), offsetof(ms_lens, struct_size), offsetof(ms_lens, model), offsetof(ms_lens, k), offsetof(ms_lens, max_theta_deg)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "consts")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "consts")], text=True).split()]
    assert got[:7] == [ms.LENS_NONE, ms.LENS_BROWN, ms.LENS_FISHEYE, ms.MAPS_ANALYTIC, ms.MAPS_CUSTOM, ms.MAPS_LENS, ms.LENS_CYL_MAX_ELEVATION_DEG] == [0, 1, 2, 0, 1, 2, 80]
    assert ms.LENS_CYL_MAX_ELEVATION_DEG == int(L.CYL_MAX_ELEVATION_DEG)
    assert got[7:] == [C.sizeof(ms.Lens), ms.Lens.struct_size.offset, ms.Lens.model.offset, ms.Lens.k.offset, ms.Lens.max_theta_deg.offset] == [80, 0, 4, 8, 72]
    for name in ("ms_lens_check", "ms_lens_project", "ms_set_lens", "ms_get_lens", "ms_build_warp_maps_lens", "ms_warp_roi_lens"):
        assert name in ms.EXPORTS
    assert all(callable(f) for f in (ms.Compositor.set_lens, ms.Compositor.get_lens, ms.build_warp_maps_lens, ms.warp_roi_lens, ms.lens_check, ms.lens_project))
