"""Moving virtual cameras (include/ms_stitch.h section 5: ms_view_pose_table, ms_reproject_poses) without a device: the pose table against the numpy product in
double, bit for bit, and every refusal of the two entry points -- status code, a word of the message, no device touched (the addresses are fake, as in
tests/test_reproject_abi.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import reproject_poses_cases as PC
import reproject_ref as RR

INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4


def refused(ms, rc, code, *words):
    msg = ms.load().ms_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def with_(obj, **kw):
    o = type(obj).from_buffer_copy(obj)
    for k, val in kw.items():
        if isinstance(val, tuple):
            i, x = val
            getattr(o, k)[i] = x
        else:
            setattr(o, k, val)
    return o


def fake_image(ms, cols, rows, typ, step=None, addr=0x10000):
    """an ms_image whose data pointer is never followed: every refusal comes before the device is touched"""
    esz = {ms.MS_8UC1: 1, ms.MS_8UC3: 3, ms.MS_32FC1: 4}[typ]
    return ms.Image(addr, cols * esz if step is None else step, cols, rows, typ)


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_and_constants(ms):
    assert C.sizeof(ms.ViewPoseJob) == C.sizeof(ms.View) + 8 and ms.ViewPoseJob.view.offset == 0
    assert ms.ViewPoseJob.dst_x.offset == C.sizeof(ms.View) and ms.ViewPoseJob.dst_y.offset == C.sizeof(ms.View) + 4
    assert (ms.VIEW_POSE_MAX_JOBS, ms.VIEW_POSE_FRAME_GROUP) == (8, 8)
    assert ms.VIEW_POSE_MAX_JOBS <= ms.VIEW_MAX_JOBS and ms.VIEW_MAX_FRAMES % ms.VIEW_POSE_FRAME_GROUP == 0
    assert {"ms_view_pose_table", "ms_reproject_poses"} <= set(ms.EXPORTS)


# ---- ms_view_pose_table ------------------------------------------------------------------------------------------------------------------------------------
def some_views(ms, n):
    names = sorted(PC.VIEWS)
    return [RR.to_ms_view(ms, PC.VIEWS[names[i % len(names)]]) for i in range(n)]


def numpy_table(views, P):
    """(float)(P_f (double)R_j), each product summed left to right in double"""
    out = np.empty((len(views), len(P), 9), np.float32)
    for j, v in enumerate(views):
        R = np.array(list(v.R), np.float32).astype(np.float64).reshape(3, 3)
        for f in range(len(P)):
            for i in range(3):
                for k in range(3):
                    out[j, f, 3 * i + k] = np.float32(P[f, i, 0] * R[0, k] + P[f, i, 1] * R[1, k] + P[f, i, 2] * R[2, k])
    return out


@pytest.mark.parametrize("n_jobs", [1, 2, 8])
@pytest.mark.parametrize("n_frames", [1, 9, 64])
def test_pose_table_equals_the_numpy_product(ms, n_jobs, n_frames):
    rng = np.random.default_rng(100 * n_jobs + n_frames)
    views = some_views(ms, n_jobs)
    P = np.stack([RR.look_at_R(rng.uniform(-180, 180), rng.uniform(-90, 90), rng.uniform(-180, 180)) for _ in range(n_frames)])
    P[0] = RR.look_at_R(90, 0, 0)      # (exact zeros and ones times float entries)
    got = ms.view_pose_table([(v, 0, 0) for v in views], P)
    want = numpy_table(views, P)
    assert got.shape == (n_jobs, n_frames, 9) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_pose_table_null_poses_give_the_views_own_rotations(ms):
    views = some_views(ms, 8)
    views[3].R[1] = -0.0      # the identity product would turn the zero's sign: NULL copies
    jobs = (ms.ViewPoseJob * 8)(*[ms.ViewPoseJob(v, 0, 0) for v in views])
    out = np.full((8, 9, 9), 7.0, np.float32)
    assert ms.load().ms_view_pose_table(jobs, 8, None, 9, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    for j, v in enumerate(views):
        own = np.array(list(v.R), np.float32)
        for f in range(9):
            assert np.array_equal(out[j, f].view(np.uint32), own.view(np.uint32)), (j, f)
    one = ms.view_pose_table([(views[0], 0, 0)])
    assert one.shape == (1, 1, 9) and np.array_equal(one[0, 0], np.array(list(views[0].R), np.float32))


def test_pose_table_refusals(ms):
    who = "ms_view_pose_table"
    fn = ms.load().ms_view_pose_table
    v = ms.look_at_view(10, 20, 0, 90, 37, 21)
    jobs = (ms.ViewPoseJob * 9)(*[ms.ViewPoseJob(v, 0, 0) for _ in range(9)])
    P = np.tile(np.eye(3).reshape(9), (65, 1))
    pp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(9 * 65 * 9, np.float32)
    po = out.ctypes.data_as(C.POINTER(C.c_float))
    refused(ms, fn(None, 1, pp(P), 1, po), INVALID, who, "null")
    refused(ms, fn(jobs, 1, pp(P), 1, None), INVALID, who, "null")
    for n in (0, -1, 9):
        refused(ms, fn(jobs, n, pp(P), 1, po), INVALID, who, "n_jobs")
    for n in (0, -3, 65):
        refused(ms, fn(jobs, 1, pp(P), n, po), INVALID, who, "n_frames")
    bad = (ms.ViewPoseJob * 2)(ms.ViewPoseJob(v, 0, 0), ms.ViewPoseJob(with_(v, struct_size=4), 0, 0))
    refused(ms, fn(bad, 2, pp(P), 1, po), INVALID, who, "jobs[1]", "struct_size")
    for x in (float("nan"), float("inf"), -float("inf")):
        bad = (ms.ViewPoseJob * 2)(ms.ViewPoseJob(v, 0, 0), ms.ViewPoseJob(with_(v, R=(5, x)), 0, 0))
        refused(ms, fn(bad, 2, pp(P), 1, po), INVALID, who, "jobs[1]", "R is not finite")
        Q = P.copy(); Q[2, 7] = x
        refused(ms, fn(jobs, 1, pp(Q), 3, po), INVALID, who, "rig_poses", "frame 2")
    assert (out == 0).all()      # a refused call writes nothing


# ---- ms_reproject_poses ------------------------------------------------------------------------------------------------------------------------------------
def good_frame(ms):
    return ms.PanoFrame.make(ms.PROJ_SPHERICAL, 96 / (2 * math.pi), -48, 0, 96, 1)


POSES = 0x7000000      # a fake, aligned device address


def call(ms, frame, srcs, dsts, jobs, poses=POSES, fmt=None, n_frames=None, n_jobs=None):
    a = (ms.Image * max(1, len(srcs)))(*srcs) if srcs is not None else None
    b = (ms.Image * max(1, len(dsts)))(*dsts) if dsts is not None else None
    j = (ms.ViewPoseJob * max(1, len(jobs)))(*jobs) if jobs is not None else None
    return ms.load().ms_reproject_poses(None if frame is None else C.byref(frame), a, b, len(srcs) if n_frames is None else n_frames, j,
                                        len(jobs) if n_jobs is None else n_jobs, C.c_void_p(poses), ms.VIEW_BGR if fmt is None else fmt, None)


def test_reproject_poses_refusals(ms):
    who = "ms_reproject_poses"
    fr = good_frame(ms)
    v = ms.look_at_view(10, 20, 0, 90, 37, 21)
    S = lambda i=0, **kw: fake_image(ms, kw.get("cols", 96), kw.get("rows", 48), kw.get("typ", ms.MS_8UC3), kw.get("step"), addr=0x100000 + 0x10000 * i)
    D = lambda i=0, **kw: fake_image(ms, kw.get("cols", 80), kw.get("rows", 40), kw.get("typ", ms.MS_8UC3), kw.get("step"), addr=0x400000 + 0x10000 * i)
    job = lambda view=v, x=0, y=0: ms.ViewPoseJob(view, x, y)
    J = [job()]
    # null pointers
    refused(ms, call(ms, None, [S()], [D()], J), INVALID, who, "null")
    refused(ms, call(ms, fr, None, [D()], J, n_frames=1), INVALID, who, "null")
    refused(ms, call(ms, fr, [S()], None, J, n_frames=1), INVALID, who, "null")
    refused(ms, call(ms, fr, [S()], [D()], None, n_jobs=1), INVALID, who, "null")
    refused(ms, call(ms, fr, [S()], [D()], J, poses=0), INVALID, who, "null")
    for off in (1, 2, 3):
        refused(ms, call(ms, fr, [S()], [D()], J, poses=POSES + off), INVALID, who, "poses_dev", "aligned")
    # the panorama frame: ms_build_view_maps' checks, and wrap_cols against the source
    refused(ms, call(ms, with_(fr, struct_size=4), [S()], [D()], J), INVALID, who, "ms_pano_frame.struct_size")
    refused(ms, call(ms, with_(fr, projection=ms.PROJ_PLANE), [S()], [D()], J), UNSUPPORTED, who, "src projection", "MS_PROJ_PLANE")
    refused(ms, call(ms, with_(fr, projection=9), [S()], [D()], J), INVALID, who, "src projection")
    for s in (0.0, -1.0, 8192.5, float("inf"), float("nan")):
        refused(ms, call(ms, with_(fr, scale=s), [S()], [D()], J), INVALID, who, "src scale")
    refused(ms, call(ms, with_(fr, wrap_cols=-1), [S()], [D()], J), INVALID, who, "wrap_cols")
    for w in (1, 95, 97):
        refused(ms, call(ms, with_(fr, wrap_cols=w), [S()], [D()], J), INVALID, who, "wrap_cols", "96 columns")
    refused(ms, call(ms, with_(fr, clamp_rows=2), [S()], [D()], J), INVALID, who, "clamp_rows")
    # the counts and the format
    for n in (0, -1, 65):
        refused(ms, call(ms, fr, [S()], [D()], J, n_frames=n), INVALID, who, "n_frames")
    for n in (0, -1, 9, 16):
        refused(ms, call(ms, fr, [S()], [D()], J, n_jobs=n), INVALID, who, "n_jobs", "[1, 8]")
    refused(ms, call(ms, fr, [S()], [D()], J, fmt=2), INVALID, who, "format")
    # the views: everything ms_build_view_maps refuses, named by job
    refused(ms, call(ms, fr, [S()], [D()], [job(with_(v, struct_size=C.sizeof(ms.View) - 4))]), INVALID, who, "jobs[0].view", "ms_view.struct_size")
    refused(ms, call(ms, fr, [S()], [D()], [job(v, 0, 0), job(with_(v, kind=2), 40, 0)]), INVALID, who, "jobs[1].view", "kind")
    for w, h in ((0, 21), (37, 0), (32768, 21), (37, 32768)):
        refused(ms, call(ms, fr, [S()], [D()], [job(with_(v, width=w, height=h))]), INVALID, who, "jobs[0].view width x height")
    for bad in (float("nan"), float("inf")):
        refused(ms, call(ms, fr, [S()], [D()], [job(with_(v, K=(2, bad)))]), INVALID, who, "jobs[0].view K")
    refused(ms, call(ms, fr, [S()], [D()], [job(with_(v, K=(0, 0.0)))]), INVALID, who, "K[0]")
    refused(ms, call(ms, fr, [S()], [D()], [job(with_(v, K=(4, 0.0)))]), INVALID, who, "K[4]")
    bad_lens = ms.Lens.brown(5.0, 0, 0, 0, 0, 0, 0, 0)
    bad_lens.k[0] = -5.0                                                   # a profile that folds back
    refused(ms, call(ms, fr, [S()], [D()], [job(with_(v, lens=bad_lens))]), INVALID, who, "jobs[0].view lens")
    short_lens = ms.Lens.fisheye(0, 0, 0, 0)
    short_lens.struct_size = 8
    refused(ms, call(ms, fr, [S()], [D()], [job(with_(v, lens=short_lens))]), INVALID, who, "jobs[0].view lens", "struct_size")
    sv = ms.View.surface(40, 20, np.eye(3, dtype=np.float32).reshape(-1), ms.PROJ_SPHERICAL, 96 / (2 * math.pi), -48, 0)
    refused(ms, call(ms, fr, [S()], [D()], [job(with_(sv, projection=ms.PROJ_PLANE))]), UNSUPPORTED, who, "jobs[0].view projection")
    refused(ms, call(ms, fr, [S()], [D()], [job(with_(sv, projection=7))]), INVALID, who, "jobs[0].view projection")
    for s in (0.0, float("nan"), 9000.0):
        refused(ms, call(ms, fr, [S()], [D()], [job(with_(sv, scale=s))]), INVALID, who, "jobs[0].view scale")
    # the source frames
    refused(ms, call(ms, fr, [S(typ=ms.MS_8UC1)], [D()], J), INVALID, who, "src frame 0", "8UC3")
    refused(ms, call(ms, fr, [S(), S(1, rows=47)], [D(), D(1)], J), INVALID, who, "src frame 1", "geometry")
    refused(ms, call(ms, fr, [S(), S(1, step=96 * 3 + 4)], [D(), D(1)], J), INVALID, who, "src frame 1", "geometry")
    nowrap = with_(fr, wrap_cols=0)
    refused(ms, call(ms, nowrap, [S(step=1 << 24)], [D()], J), INVALID, who, "src step")
    refused(ms, call(ms, nowrap, [S(rows=1 << 12, step=1 << 20)], [D()], J), INVALID, who, "rows * step")
    # the destination frames
    refused(ms, call(ms, fr, [S()], [D(typ=ms.MS_8UC1)], J), INVALID, who, "dst frame 0", "8UC3")
    refused(ms, call(ms, fr, [S(), S(1)], [D(), D(1, rows=41)], J), INVALID, who, "dst frame 1", "geometry")
    # the rectangles: view.width x view.height at (dst_x, dst_y)
    for x, y in ((44, 0), (0, 20), (-1, 0), (0, -2)):
        refused(ms, call(ms, fr, [S()], [D()], [job(v, x, y)]), INVALID, who, "jobs[0]", "leaves")
    small = ms.look_at_view(0, 0, 0, 90, 10, 10)
    refused(ms, call(ms, fr, [S()], [D()], [job(v, 0, 0), job(small, 36, 20)]), INVALID, who, "jobs[0]", "jobs[1]", "overlap")
    # I420
    DI = lambda i=0, **kw: fake_image(ms, kw.get("cols", 80), kw.get("rows", 60), ms.MS_8UC1, kw.get("step"), addr=0x400000 + 0x10000 * i)
    I = ms.VIEW_I420
    ev = ms.look_at_view(10, 20, 0, 90, 38, 22)
    refused(ms, call(ms, fr, [S()], [D()], [job(ev, 2, 4)], fmt=I), INVALID, who, "dst frame 0", "I420")
    refused(ms, call(ms, fr, [S()], [DI(step=96)], [job(ev, 2, 4)], fmt=I), INVALID, who, "contiguous")
    refused(ms, call(ms, fr, [S()], [DI(rows=61)], [job(ev, 2, 4)], fmt=I), INVALID, who, "even-sized frame")
    for w, h, x, y in ((37, 22, 2, 4), (38, 21, 2, 4), (38, 22, 1, 4), (38, 22, 2, 3)):
        refused(ms, call(ms, fr, [S()], [DI()], [job(with_(ev, width=w, height=h), x, y)], fmt=I), INVALID, who, "jobs[0]", "even")
    refused(ms, call(ms, fr, [S()], [DI()], [job(ev, 2, 20)], fmt=I), INVALID, who, "jobs[0]", "leaves")      # the frame is 80 x 40: rows 20 .. 41 leave it
    # a destination that overlaps a source in memory
    src = S()
    over = fake_image(ms, 80, 40, ms.MS_8UC3, addr=src.data + 96 * 3 * 47)      # begins inside the source's last row
    refused(ms, call(ms, fr, [src], [over], J), INVALID, who, "dst frame 0", "src frame 0", "overlaps")
    # what passes ends at the missing device, not in a host fallback: a non-finite view.R is NOT refused here (the table holds the rotations), touching
    # rectangles are fine, eight jobs are fine
    import torch
    if not torch.cuda.is_available():
        refused(ms, call(ms, fr, [S()], [D()], J), NO_DEVICE, "no CPU fallback")
        refused(ms, call(ms, fr, [S()], [D()], [job(with_(v, R=(4, float("nan"))))]), NO_DEVICE, "no CPU fallback")
        refused(ms, call(ms, fr, [S()], [D()], [job(v, 0, 0), job(small, 37, 0), job(small, 0, 21)]), NO_DEVICE, "no CPU fallback")
        refused(ms, call(ms, fr, [S()], [D()], [job(small, 10 * i, 0) for i in range(8)]), NO_DEVICE, "no CPU fallback")
        refused(ms, call(ms, fr, [S()], [DI()], [job(ev, 2, 4)], fmt=I), NO_DEVICE, "no CPU fallback")
        refused(ms, call(ms, nowrap, [S()], [D()], [job(sv, 0, 0)]), NO_DEVICE, "no CPU fallback")
