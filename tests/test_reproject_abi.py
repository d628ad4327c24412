"""Virtual cameras (include/ms_stitch.h section 5) without a device: the host helpers against the header's formulas, and every refusal of ms_build_view_maps /
ms_reproject / ms_get_pano_frame -- status code, a message naming the argument, and no device touched (this container has none:
test_abi.py::test_compute_without_device_fails_loudly shows the no-device status every compute call ends in once its arguments pass)."""
import ctypes as C
import math

import numpy as np
import pytest

import lens_ref as L
import reproject_ref as RR

INVALID, UNSUPPORTED, NO_DEVICE, STATE = -1, -2, -4, -5


def mat(a):
    return np.array(list(a), np.float32).reshape(3, 3)


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------------------
def test_cube_faces_are_the_explicit_rotations(ms):
    axes = []
    for face, (yaw, pitch) in enumerate(RR.FACES):
        v = ms.cube_face_view(face, 64)
        R = mat(v.R)
        assert np.array_equal(R, np.float32(RR.look_at_R(yaw, pitch, 0.0))), face
        assert np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(3)).max() <= 1e-7, face
        assert v.struct_size == C.sizeof(ms.View) and v.kind == ms.VIEW_CAMERA and v.width == v.height == 64 and v.lens.model == ms.LENS_NONE
        K = mat(v.K)
        assert np.array_equal(K, np.float32([[32, 0, 31.5], [0, 32, 31.5], [0, 0, 1]]))      # f = size / 2, c = (size - 1) / 2
        axes.append(tuple(int(round(float(t))) for t in R[:, 2]))
        assert np.abs(R[:, 2] - np.float32(axes[-1])).max() <= 1e-7
    # front +z, right +x, back -z, left -x, up -y (v = 0 is the pole above), down +y: each axis of the rig once
    assert axes == [(0, 0, 1), (1, 0, 0), (0, 0, -1), (-1, 0, 0), (0, -1, 0), (0, 1, 0)]


@pytest.mark.parametrize("pose", [(0, 0, 0, 90, 64, 64), (200, 35, 10, 90, 37, 21), (-75.5, -80, 170, 179, 1, 1), (30, 10, 0, 1e-3, 320, 180), (359, 90, -45, 120, 32767, 2)])
def test_look_at_view_follows_the_formulas(ms, pose):
    yaw, pitch, roll, hfov, w, h = pose
    v = ms.look_at_view(*pose)
    assert np.array_equal(mat(v.R), np.float32(RR.look_at_R(yaw, pitch, roll)))
    assert np.array_equal(mat(v.K), np.float32(RR.look_at_K(hfov, w, h)))
    assert (v.width, v.height, v.kind) == (w, h, ms.VIEW_CAMERA)
    # yaw a puts the optical axis at u = a scale; positive pitch looks up, toward v = 0
    d = RR.look_at_R(yaw, pitch, 0.0)[:, 2]
    assert abs(math.remainder(math.atan2(d[0], d[2]) - math.radians(yaw), 2 * math.pi)) < 1e-12 or abs(abs(pitch) - 90) < 1e-9
    assert abs(math.atan2(math.hypot(d[0], d[2]), -d[1]) - (math.pi / 2 - math.radians(pitch))) < 1e-12


def refused(ms, rc, code, *words):
    msg = ms.load().ms_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_helper_refusals(ms):
    lib = ms.load()
    v = ms.View()
    la = lambda *a: lib.ms_look_at_view(*[C.c_double(x) for x in a[:4]], a[4], a[5], a[6])
    refused(ms, la(0, 0, 0, 90, 8, 8, None), INVALID, "ms_look_at_view", "out")
    refused(ms, la(float("nan"), 0, 0, 90, 8, 8, C.byref(v)), INVALID, "ms_look_at_view", "yaw")
    for hfov in (0.0, -1.0, 179.5, float("nan")):
        refused(ms, la(0, 0, 0, hfov, 8, 8, C.byref(v)), INVALID, "ms_look_at_view", "hfov_deg")
    for w, h in ((0, 8), (8, 0), (32768, 8), (8, 40000)):
        refused(ms, la(0, 0, 0, 90, w, h, C.byref(v)), INVALID, "ms_look_at_view", "width")
    refused(ms, lib.ms_cube_face_view(0, 8, None), INVALID, "ms_cube_face_view", "out")
    for face in (-1, 6):
        refused(ms, lib.ms_cube_face_view(face, 8, C.byref(v)), INVALID, "ms_cube_face_view", "face")
    for size in (0, 32768):
        refused(ms, lib.ms_cube_face_view(0, size, C.byref(v)), INVALID, "ms_cube_face_view", "size")
    p = ms.PanoFrame()
    refused(ms, lib.ms_get_pano_frame(None, ms.PANO_CANVAS, C.byref(p)), INVALID, "ms_get_pano_frame", "ctx")


# ---- ms_build_view_maps -----------------------------------------------------------------------------------------------------------------------------------
def fake_image(ms, cols, rows, typ, step=None, addr=0x10000):
    """an ms_image whose data pointer is never followed: every refusal comes before the device is touched"""
    esz = {ms.MS_8UC1: 1, ms.MS_8UC3: 3, ms.MS_32FC1: 4}[typ]
    return ms.Image(addr, cols * esz if step is None else step, cols, rows, typ)


def good_frame(ms):
    return ms.PanoFrame.make(ms.PROJ_SPHERICAL, 96 / (2 * math.pi), -48, 0, 96, 1)


def build(ms, frame, view, mx, my):
    p = lambda o: None if o is None else C.byref(o)
    return ms.load().ms_build_view_maps(p(frame), p(view), p(mx), p(my), None)


def test_build_view_maps_refusals(ms):
    fr, v = good_frame(ms), ms.look_at_view(10, 20, 0, 90, 37, 21)
    mx, my = fake_image(ms, 37, 21, ms.MS_32FC1), fake_image(ms, 37, 21, ms.MS_32FC1, addr=0x20000)
    who = "ms_build_view_maps"
    for args in ((None, v, mx, my), (fr, None, mx, my), (fr, v, None, my), (fr, v, mx, None)):
        refused(ms, build(ms, *args), INVALID, who, "null")

    def with_(obj, **kw):
        o = type(obj).from_buffer_copy(obj)
        for k, val in kw.items():
            if isinstance(val, tuple):
                i, x = val
                getattr(o, k)[i] = x
            else:
                setattr(o, k, val)
        return o
    refused(ms, build(ms, with_(fr, struct_size=4), v, mx, my), INVALID, who, "ms_pano_frame.struct_size")
    refused(ms, build(ms, fr, with_(v, struct_size=C.sizeof(ms.View) - 4), mx, my), INVALID, who, "ms_view.struct_size")
    refused(ms, build(ms, fr, with_(v, kind=2), mx, my), INVALID, who, "kind")
    refused(ms, build(ms, with_(fr, projection=ms.PROJ_PLANE), v, mx, my), UNSUPPORTED, who, "src projection", "MS_PROJ_PLANE")
    refused(ms, build(ms, with_(fr, projection=9), v, mx, my), INVALID, who, "src projection")
    for s in (0.0, -1.0, 8192.5, float("inf"), float("nan")):
        refused(ms, build(ms, with_(fr, scale=s), v, mx, my), INVALID, who, "src scale")
    refused(ms, build(ms, with_(fr, wrap_cols=-1), v, mx, my), INVALID, who, "wrap_cols")
    refused(ms, build(ms, with_(fr, clamp_rows=2), v, mx, my), INVALID, who, "clamp_rows")
    for w, h in ((0, 21), (37, 0), (32768, 21), (37, 32768)):
        refused(ms, build(ms, fr, with_(v, width=w, height=h), mx, my), INVALID, who, "view width x height")
    for bad in (float("nan"), float("inf")):
        refused(ms, build(ms, fr, with_(v, R=(4, bad)), mx, my), INVALID, who, "view R")
        refused(ms, build(ms, fr, with_(v, K=(2, bad)), mx, my), INVALID, who, "view K")
    refused(ms, build(ms, fr, with_(v, K=(0, 0.0)), mx, my), INVALID, who, "K[0]")
    refused(ms, build(ms, fr, with_(v, K=(4, 0.0)), mx, my), INVALID, who, "K[4]")
    bad_lens = ms.Lens.brown(5.0, 0, 0, 0, 0, 0, 0, 0)
    bad_lens.k[0] = -5.0                                                   # a profile that folds back
    refused(ms, build(ms, fr, with_(v, lens=bad_lens), mx, my), INVALID, who, "view lens")
    short_lens = ms.Lens.fisheye(0, 0, 0, 0)
    short_lens.struct_size = 8
    refused(ms, build(ms, fr, with_(v, lens=short_lens), mx, my), INVALID, who, "view lens", "struct_size")
    # maps: type, size, data
    refused(ms, build(ms, fr, v, fake_image(ms, 37, 21, ms.MS_8UC1), my), INVALID, who, "map_x", "32FC1")
    refused(ms, build(ms, fr, v, mx, fake_image(ms, 37, 21, ms.MS_8UC3)), INVALID, who, "map_y", "32FC1")
    refused(ms, build(ms, fr, v, fake_image(ms, 36, 21, ms.MS_32FC1), my), INVALID, who, "view's size")
    refused(ms, build(ms, fr, v, mx, fake_image(ms, 37, 22, ms.MS_32FC1)), INVALID, who, "view's size")
    refused(ms, build(ms, fr, v, fake_image(ms, 37, 21, ms.MS_32FC1, addr=0), my), INVALID, who, "map_x")
    refused(ms, build(ms, fr, v, mx, fake_image(ms, 37, 21, ms.MS_32FC1, step=37 * 4 - 4)), INVALID, who, "map_y", "step")
    # a surface view
    sv = ms.View.surface(96, 48, np.eye(3, dtype=np.float32).reshape(-1), ms.PROJ_SPHERICAL, 96 / (2 * math.pi), -48, 0)
    smx, smy = fake_image(ms, 96, 48, ms.MS_32FC1), fake_image(ms, 96, 48, ms.MS_32FC1, addr=0x40000)
    refused(ms, build(ms, fr, with_(sv, projection=ms.PROJ_PLANE), smx, smy), UNSUPPORTED, who, "view projection")
    refused(ms, build(ms, fr, with_(sv, scale=0.0), smx, smy), INVALID, who, "view scale")
    refused(ms, build(ms, fr, with_(sv, scale=float("nan")), smx, smy), INVALID, who, "view scale")
    # arguments that pass end at the missing device, not in a host fallback
    import torch
    if not torch.cuda.is_available():
        refused(ms, build(ms, fr, v, mx, my), NO_DEVICE, "no CPU fallback")
        refused(ms, build(ms, fr, sv, smx, smy), NO_DEVICE, "no CPU fallback")


# ---- ms_reproject -----------------------------------------------------------------------------------------------------------------------------------------
def reproject(ms, srcs, dsts, jobs, wrap=0, clamp=0, fmt=None, n_frames=None, n_jobs=None):
    a = (ms.Image * max(1, len(srcs)))(*srcs) if srcs is not None else None
    b = (ms.Image * max(1, len(dsts)))(*dsts) if dsts is not None else None
    j = (ms.ViewJob * max(1, len(jobs)))(*jobs) if jobs is not None else None
    return ms.load().ms_reproject(a, b, len(srcs) if n_frames is None else n_frames, j, len(jobs) if n_jobs is None else n_jobs, wrap, clamp,
                                  ms.VIEW_BGR if fmt is None else fmt, None)


def job(ms, w, h, x, y, addr=0x900000):
    return ms.ViewJob(fake_image(ms, w, h, ms.MS_32FC1, addr=addr), fake_image(ms, w, h, ms.MS_32FC1, addr=addr + 0x80000), x, y)


def test_reproject_refusals(ms):
    who = "ms_reproject"
    S = lambda i=0, **kw: fake_image(ms, kw.get("cols", 96), kw.get("rows", 48), kw.get("typ", ms.MS_8UC3), kw.get("step"), addr=0x100000 + 0x10000 * i)
    D = lambda i=0, **kw: fake_image(ms, kw.get("cols", 80), kw.get("rows", 40), kw.get("typ", ms.MS_8UC3), kw.get("step"), addr=0x400000 + 0x10000 * i)
    J = [job(ms, 37, 21, 0, 0)]
    refused(ms, reproject(ms, None, [D()], J, n_frames=1), INVALID, who, "null")
    refused(ms, reproject(ms, [S()], None, J, n_frames=1), INVALID, who, "null")
    refused(ms, reproject(ms, [S()], [D()], None, n_jobs=1), INVALID, who, "null")
    for n in (0, -1, 65):
        refused(ms, reproject(ms, [S()], [D()], J, n_frames=n), INVALID, who, "n_frames")
    for n in (0, 17):
        refused(ms, reproject(ms, [S()], [D()], J, n_jobs=n), INVALID, who, "n_jobs")
    refused(ms, reproject(ms, [S()], [D()], J, fmt=2), INVALID, who, "format")
    # the source frames
    refused(ms, reproject(ms, [S(typ=ms.MS_8UC1)], [D()], J), INVALID, who, "src frame 0", "8UC3")
    refused(ms, reproject(ms, [S(), S(1, cols=95)], [D(), D(1)], J), INVALID, who, "src frame 1", "geometry")
    refused(ms, reproject(ms, [S(), S(1, step=96 * 3 + 4)], [D(), D(1)], J), INVALID, who, "src frame 1", "geometry")
    refused(ms, reproject(ms, [S(step=1 << 24)], [D()], J), INVALID, who, "src step")
    refused(ms, reproject(ms, [S(rows=1 << 12, step=1 << 20)], [D()], J), INVALID, who, "rows * step")
    for w in (1, 95, -96):
        refused(ms, reproject(ms, [S()], [D()], J, wrap=w), INVALID, who, "wrap_cols")
    refused(ms, reproject(ms, [S()], [D()], J, clamp=2), INVALID, who, "clamp_rows")
    # the destination frames
    refused(ms, reproject(ms, [S()], [D(typ=ms.MS_8UC1)], J), INVALID, who, "dst frame 0", "8UC3")
    refused(ms, reproject(ms, [S(), S(1)], [D(), D(1, rows=41)], J), INVALID, who, "dst frame 1", "geometry")
    # the jobs
    bad = job(ms, 37, 21, 0, 0); bad.map_y.cols = 36
    refused(ms, reproject(ms, [S()], [D()], [bad]), INVALID, who, "jobs[0]", "map_x", "map_y")
    bad = job(ms, 37, 21, 0, 0); bad.map_x.type = ms.MS_8UC1
    refused(ms, reproject(ms, [S()], [D()], [J[0], bad]), INVALID, who, "jobs[1].map_x", "32FC1")
    bad = job(ms, 37, 21, 0, 0); bad.map_y.data = None
    refused(ms, reproject(ms, [S()], [D()], [bad]), INVALID, who, "jobs[0].map_y")
    for x, y in ((44, 0), (0, 20), (-1, 0), (0, -2)):
        refused(ms, reproject(ms, [S()], [D()], [job(ms, 37, 21, x, y)]), INVALID, who, "jobs[0]", "leaves")
    refused(ms, reproject(ms, [S()], [D()], [job(ms, 37, 21, 0, 0), job(ms, 10, 10, 36, 20, addr=0xb00000)]), INVALID, who, "jobs[0]", "jobs[1]", "overlap")
    # touching rectangles are fine: they end at the missing device
    import torch
    touching = [job(ms, 37, 21, 0, 0), job(ms, 10, 10, 37, 0, addr=0xb00000), job(ms, 37, 5, 0, 21, addr=0xd00000)]
    if not torch.cuda.is_available():
        refused(ms, reproject(ms, [S()], [D()], touching), NO_DEVICE, "no CPU fallback")
    # I420
    DI = lambda i=0, **kw: fake_image(ms, kw.get("cols", 80), kw.get("rows", 60), ms.MS_8UC1, kw.get("step"), addr=0x400000 + 0x10000 * i)
    I = ms.VIEW_I420
    EJ = [job(ms, 38, 22, 2, 4)]
    refused(ms, reproject(ms, [S()], [D()], EJ, fmt=I), INVALID, who, "dst frame 0", "I420")
    refused(ms, reproject(ms, [S()], [DI(step=96)], EJ, fmt=I), INVALID, who, "contiguous")
    refused(ms, reproject(ms, [S()], [DI(rows=61)], EJ, fmt=I), INVALID, who, "even-sized frame")
    refused(ms, reproject(ms, [S()], [DI(cols=81)], EJ, fmt=I), INVALID, who, "even-sized frame")
    for w, h, x, y in ((37, 22, 2, 4), (38, 21, 2, 4), (38, 22, 1, 4), (38, 22, 2, 3)):
        refused(ms, reproject(ms, [S()], [DI()], [job(ms, w, h, x, y)], fmt=I), INVALID, who, "jobs[0]", "even")
    refused(ms, reproject(ms, [S()], [DI()], [job(ms, 38, 22, 2, 20)], fmt=I), INVALID, who, "jobs[0]", "leaves")      # the frame is 80 x 40: rows 20 .. 41 leave it
    if not torch.cuda.is_available():
        refused(ms, reproject(ms, [S()], [DI()], EJ, fmt=I), NO_DEVICE, "no CPU fallback")
    # a destination that overlaps a source in memory
    src = S()
    over = fake_image(ms, 80, 40, ms.MS_8UC3, addr=src.data + 96 * 3 * 47)      # begins inside the source's last row
    refused(ms, reproject(ms, [src], [over], J), INVALID, who, "dst frame 0", "src frame 0", "overlaps")
    refused(ms, reproject(ms, [S(), S(1)], [D(), fake_image(ms, 80, 40, ms.MS_8UC3, addr=S().data - 80 * 3 * 40 + 1)], J), INVALID, who, "dst frame 1", "src frame 0")


def test_struct_layouts(ms):
    """the binding's structs against the header's: sizes the library itself checks (struct_size), and the constants the header states"""
    assert C.sizeof(ms.PanoFrame) == 28 and C.sizeof(ms.ViewJob) == 2 * C.sizeof(ms.Image) + 8
    v = ms.look_at_view(0, 0, 0, 90, 8, 8)
    assert v.struct_size == C.sizeof(ms.View) and v.lens.struct_size == C.sizeof(ms.Lens)
    assert (ms.VIEW_MAX_FRAMES, ms.VIEW_MAX_JOBS) == (64, 16)
