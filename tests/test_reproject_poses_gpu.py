"""Moving virtual cameras on the device (include/ms_stitch.h section 5, ms_reproject_poses): one launch for every frame and view of a call, each frame under its own
rotation, against the route its contract names -- ms_build_view_maps with that frame's rotation, then a one-frame ms_reproject -- bit for bit, inside guarded,
pitched, odd-offset buffers; against the float64 numpy statement (tests/reproject_ref.py); on a stitched canvas and through stitch_app --orbit."""
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import np_ref
import reproject_poses_cases as PC
import reproject_ref as RR
import synth
from helpers import host, make_rig, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "video-stitcher_amd", "stitch_app")
PAD = 0x5A


class Frames:
    """n images of one geometry inside ONE flat device buffer filled with `fill`: a pitched step, an odd byte offset of every base, guard bytes everywhere else"""
    def __init__(self, n, rows, cols, cn, fill, pad_step=7, contiguous=False):
        self.rows, self.cols, self.cn, self.n = rows, cols, cn, n
        self.step = cols * cn + (0 if contiguous else pad_step)
        self.stride = rows * self.step + 33
        self.off = [11 + i * self.stride for i in range(n)]
        self.flat = torch.full((11 + n * self.stride + 64,), fill, dtype=torch.uint8, device="cuda")
        shape, strides = ((rows, cols, cn), (self.step, cn, 1)) if cn > 1 else ((rows, cols), (self.step, 1))
        self.views = [torch.as_strided(self.flat, shape, strides, o) for o in self.off]

    def index(self, i):
        """flat indices of image i's pixels, shaped like the image"""
        r = np.arange(self.rows)[:, None, None] * self.step + np.arange(self.cols)[None, :, None] * self.cn + np.arange(self.cn)[None, None, :]
        return self.off[i] + (r if self.cn > 1 else r[..., 0])


def upload_sources(srcs):
    h, w = srcs[0].shape[:2]
    F = Frames(len(srcs), h, w, 3, 0xAB)
    assert F.step % 2 == 1 and F.off[0] % 2 == 1
    for t, s in zip(F.views, srcs):
        t.copy_(torch.from_numpy(s).cuda())
    return F


def sources_untouched(S, srcs):
    flat = host(S.flat)
    keep = np.ones(flat.shape, bool)
    for f in range(S.n):
        keep[S.index(f)] = False
        assert np.array_equal(flat[S.index(f)], srcs[f])
    return bool((flat[keep] == 0xAB).all())


def upload_poses(poses):
    """the table at a 4-byte aligned address that is not 8-byte aligned, inside a larger buffer whose other words must stay"""
    poses = np.ascontiguousarray(poses, np.float32)
    buf = torch.full((poses.size + 4,), 123.0, dtype=torch.float32, device="cuda")
    t = buf[1:1 + poses.size]
    t.copy_(torch.from_numpy(poses.reshape(-1)).cuda())
    assert t.data_ptr() % 8 == 4
    return buf, t


NAN_R = np.full(9, np.nan, np.float32)


def pose_jobs(ms, jobs):
    """the views with a NaN rotation: ms_reproject_poses reads the table, never view.R"""
    return [(RR.to_ms_view(ms, PC.with_R(v, NAN_R)), dx, dy) for v, dx, dy in jobs]


def numpy_maps(frame, view, R9):
    """float64 maps of the header's formulas rounded to float32 once, X == wrap_cols stored as 0"""
    with np.errstate(all="ignore"):
        rx, ry, _ = RR.view_maps(frame, PC.with_R(view, R9))
        mx, my = np.float32(rx), np.float32(ry)
    if frame["wrap"]:
        mx = np.where(mx == np.float32(frame["wrap"]), np.float32(0), mx)
    return mx, my


def route_maps(ms, pf, frame, view, R9):
    """the maps of the two-call route: ms_build_view_maps where it accepts the rotation; the numpy statement for a rotation that is not finite, which it refuses"""
    if np.isfinite(R9).all():
        return ms.build_view_maps(pf, RR.to_ms_view(ms, PC.with_R(view, R9)))
    mx, my = numpy_maps(frame, view, R9)
    return to_dev(mx), to_dev(my)


def two_call_route(ms, frame, S, jobs, poses, D, fmt):
    """frame f, job j: ms_build_view_maps(view_j with R = that frame's nine floats), then ms_reproject(&src[f], &dst[f], 1, {those maps, dst_x, dst_y}, 1, ...)"""
    pf = RR.to_ms_frame(ms, frame)
    for f in range(S.n):
        for j, (view, dx, dy) in enumerate(jobs):
            mx, my = route_maps(ms, pf, frame, view, poses[j, f])
            ms.reproject([S.views[f]], [D.views[f]], [(mx, my, dx, dy)], frame["wrap"], frame["clamp"], fmt=fmt)


def rect_mask(D, jobs, i420_wh=None):
    """True on the flat bytes the jobs may write"""
    m = np.zeros(tuple(D.flat.shape), bool)
    for f in range(D.n):
        idx = D.index(f)
        for view, dx, dy in jobs:
            w, h = view["w"], view["h"]
            if i420_wh is None:
                m[idx[dy:dy + h, dx:dx + w]] = True
            else:
                W, H = i420_wh
                flat = idx.reshape(-1)
                Y = flat[:W * H].reshape(H, W); U = flat[W * H:W * H + (W // 2) * (H // 2)].reshape(H // 2, W // 2); V = flat[W * H + (W // 2) * (H // 2):].reshape(H // 2, W // 2)
                m[Y[dy:dy + h, dx:dx + w]] = True
                m[U[dy // 2:(dy + h) // 2, dx // 2:(dx + w) // 2]] = True
                m[V[dy // 2:(dy + h) // 2, dx // 2:(dx + w) // 2]] = True
    return m


def run_against_two_calls(ms, frame, srcs, jobs, poses, atlas_wh, i420=False):
    """ms_reproject_poses in ONE call against the two-call route, over the WHOLE destination buffer: rectangles, the bytes around them, between rows and between
    frames.  jobs: [(view dict, dst_x, dst_y)], poses (n_jobs, n_frames, 9) float32.  Returns the destination Frames."""
    W, H = atlas_wh
    n = len(srcs)
    S = upload_sources(srcs)
    mk = (lambda: Frames(n, H * 3 // 2, W, 1, PAD, contiguous=True)) if i420 else (lambda: Frames(n, H, W, 3, PAD))
    D, E = mk(), mk()
    fmt = ms.VIEW_I420 if i420 else ms.VIEW_BGR
    buf, table = upload_poses(poses)
    ms.reproject_poses(RR.to_ms_frame(ms, frame), S.views, D.views, pose_jobs(ms, jobs), table, fmt=fmt)
    two_call_route(ms, frame, S, jobs, poses, E, fmt)
    torch.cuda.synchronize()
    got, want = host(D.flat), host(E.flat)
    bad = np.flatnonzero(got != want)
    if bad.size:
        where = [(f, j) for f in range(n) for j, (v, dx, dy) in enumerate(jobs)
                 if i420 or (got[D.index(f)[dy:dy + v["h"], dx:dx + v["w"]]] != want[D.index(f)[dy:dy + v["h"], dx:dx + v["w"]]]).any()]
        assert False, "%d bytes differ, first at flat offset %d (got %d, want %d); (frame, job) pairs: %s" % (bad.size, bad[0], got[bad[0]], want[bad[0]], where[:8])
    inside = rect_mask(D, jobs, (W, H) if i420 else None)
    assert (got[~inside] == PAD).all(), "a byte outside the jobs' rectangles was written"
    # (written at all: random bytes equal PAD once in 256; the unseen pixels of a view all repeat ONE source pixel, of whose three bytes one may be PAD)
    assert (got[inside] != PAD).mean() > 0.5, "the rectangles were not written"
    assert inside.sum() == n * sum(v["w"] * v["h"] * 3 // (2 if i420 else 1) for v, _, _ in jobs)
    assert sources_untouched(S, srcs)
    b = host(buf)
    assert b[0] == 123.0 and (b[-3:] == 123.0).all() and np.array_equal(b[1:-3].view(np.uint32), np.ascontiguousarray(poses, np.float32).reshape(-1).view(np.uint32))
    return D


# ---- 1. equals the two-call route ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(PC.FRAMES))
@pytest.mark.parametrize("vname", sorted(PC.VIEWS))
def test_equals_build_view_maps_then_reproject(ms, cuda, fname, vname):
    """1, G - 1, G, G + 1 and 2 G + 1 frames (G = MS_VIEW_POSE_FRAME_GROUP = 8), each frame under a rotation of its own; the first poses of every run put the
    optical axis on the +-pi seam and on both poles"""
    assert ms.VIEW_POSE_FRAME_GROUP == 8
    frame, view = PC.FRAMES[fname], PC.VIEWS[vname]
    rng = np.random.default_rng(sum(map(ord, fname + vname)))
    for n_frames in (1, 7, 8, 9, 17):
        srcs = PC.random_sources(rng, n_frames)
        poses = np.roll(PC.random_poses(rng, n_frames), 5, axis=0)[None]      # (the fixed poses at frames 5 to 8: on both sides of a group's edge from 9 frames on)
        run_against_two_calls(ms, frame, srcs, [(view, 3, 2)], poses, (view["w"] + 8, view["h"] + 5))


def test_equals_the_two_call_route_over_64_frames(ms, cuda):
    assert ms.VIEW_MAX_FRAMES == 64
    rng = np.random.default_rng(64)
    view = RR.look_at(10, 5, 0, 80, 9, 5)
    run_against_two_calls(ms, PC.FRAMES["sph"], PC.random_sources(rng, 64), [(view, 1, 1)], PC.random_poses(rng, 64)[None], (12, 7))


# ---- 2. job tables ----------------------------------------------------------------------------------------------------------------------------------------------
JOB_VIEWS = ["tiles", "pinhole", "fisheye", "up", "brown", "seam", "down", "pinhole"]


@pytest.mark.parametrize("n_jobs", [1, 2, 8])
def test_job_tables_of_differing_views(ms, cuda, n_jobs):
    rng = np.random.default_rng(2000 + n_jobs)
    views = [PC.VIEWS[JOB_VIEWS[j]] for j in range(n_jobs)]
    pos, bottom = PC.shelf_pack([(v["w"], v["h"]) for v in views], 2, 1, 150)
    jobs = [(v, x, y) for v, (x, y) in zip(views, pos)]
    poses = np.stack([PC.random_poses(rng, 4 + 5)[rng.permutation(9)] for _ in range(n_jobs)])      # every job its own nine rotations
    run_against_two_calls(ms, PC.FRAMES["sph"], PC.random_sources(rng, 9), jobs, poses, (2 + 150 + 3, bottom + 2))


def cube_views(size):
    return [(RR.cube_face(face, size), (face % 3) * size, (face // 3) * size) for face in range(6)]


def moving_rig(rng, n):
    return np.stack([RR.look_at_R(rng.uniform(-180, 180), rng.uniform(-30, 30), rng.uniform(-20, 20)) for _ in range(n)])


def test_cube_map_under_a_moving_rig(ms, cuda):
    """six jobs: the cube faces under the rig rotation P_f of frame f, the table from ms_view_pose_table; inside a larger atlas whose other bytes stay"""
    rng = np.random.default_rng(2600)
    jobs = [(v, x + 4, y + 2) for v, x, y in cube_views(18)]
    P = moving_rig(rng, 9)
    poses = ms.view_pose_table([(RR.to_ms_view(ms, v), x, y) for v, x, y in jobs], P)
    assert poses.shape == (6, 9, 9)
    run_against_two_calls(ms, PC.FRAMES["sph"], PC.random_sources(rng, 9), jobs, poses, (3 * 18 + 9, 2 * 18 + 5))


# ---- 3. I420 ----------------------------------------------------------------------------------------------------------------------------------------------------
def run_i420_against_bgr(ms, frame, srcs, jobs, poses, frame_wh):
    """MS_VIEW_I420 equals the two-call route's planes, and ms_bgr_to_i420 (np_ref.bgr_to_i420) of the BGR result of the same call"""
    W, H = frame_wh
    D = run_against_two_calls(ms, frame, srcs, jobs, poses, frame_wh, i420=True)
    B = run_against_two_calls(ms, frame, srcs, jobs, poses, frame_wh)
    got = host(D.flat)
    want = np.full(got.shape, PAD, np.uint8)
    for f in range(len(srcs)):
        bgr = host(B.views[f])
        for v, dx, dy in jobs:
            PC.expect_i420(np_ref, want, D.index(f), W, H, (dx, dy, v["w"], v["h"]), bgr[dy:dy + v["h"], dx:dx + v["w"]])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d bytes differ from ms_bgr_to_i420 of the BGR result, first at flat offset %d" % (bad.size, bad[0])
    return D, B


def test_i420_even_views(ms, cuda):
    rng = np.random.default_rng(4000)
    views = [PC.VIEWS_EVEN[k] for k in ("tiles", "pinhole", "fisheye", "brown")]
    pos, bottom = PC.shelf_pack([(v["w"], v["h"]) for v in views], 4, 2, 110, even=True)
    jobs = [(v, x, y) for v, (x, y) in zip(views, pos)]
    poses = np.stack([PC.random_poses(rng, 9)[rng.permutation(9)] for _ in jobs])
    run_i420_against_bgr(ms, PC.FRAMES["sph"], PC.random_sources(rng, 9), jobs, poses, (120, bottom + 4))
    run_i420_against_bgr(ms, PC.FRAMES["roi"], PC.random_sources(rng, 2), [(PC.VIEWS_EVEN["surface"], 0, 0)], PC.random_poses(rng, 2)[None], (96, 48))


def test_i420_cube_atlas(ms, cuda):
    """the 3 x 2 atlas of six 16 x 16 faces under a moving rig, 9 frames: the planes equal ms_bgr_to_i420 of the BGR atlas"""
    rng = np.random.default_rng(4100)
    jobs = cube_views(16)
    poses = ms.view_pose_table([(RR.to_ms_view(ms, v), x, y) for v, x, y in jobs], moving_rig(rng, 9))
    D, B = run_i420_against_bgr(ms, PC.FRAMES["sph"], PC.random_sources(rng, 9), jobs, poses, (48, 32))
    for f in range(9):
        assert torch.equal(ms.bgr_to_i420(B.views[f].contiguous()), D.views[f].contiguous()), f


# ---- 4. standing still ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vname", ["pinhole", "fisheye", "surface", "tiles"])
def test_standing_still_equals_reproject_over_the_same_frames(ms, cuda, vname):
    rng = np.random.default_rng(5000)
    frame, view = PC.FRAMES["sph"], PC.VIEWS[vname]
    srcs = PC.random_sources(rng, 9)
    S = upload_sources(srcs)
    D, E = Frames(9, view["h"] + 4, view["w"] + 6, 3, PAD), Frames(9, view["h"] + 4, view["w"] + 6, 3, PAD)
    pf = RR.to_ms_frame(ms, frame)
    v = RR.to_ms_view(ms, view)
    poses = np.repeat(ms.view_pose_table([(v, 3, 1)]), 9, axis=1)      # (NULL rig poses: the view's own R), nine times
    buf, table = upload_poses(poses)
    ms.reproject_poses(pf, S.views, D.views, pose_jobs(ms, [(view, 3, 1)]), table)
    mx, my = ms.build_view_maps(pf, v)
    ms.reproject(S.views, E.views, [(mx, my, 3, 1)], frame["wrap"], frame["clamp"])
    torch.cuda.synchronize()
    assert torch.equal(D.flat, E.flat)
    assert (host(D.flat) != PAD).any()


# ---- 5. hostile rotations ---------------------------------------------------------------------------------------------------------------------------------------
def hostile_poses(rng):
    """good frames mixed with nine floats no rotation has: NaN, +-inf, all zero, a rotation times 1e30, a reflection, one NaN entry, one inf entry"""
    good = PC.random_poses(rng, 8)
    R = good[5].astype(np.float64)
    one_nan, one_inf = good[6].copy(), good[7].copy()
    one_nan[4] = np.nan
    one_inf[2] = -np.inf
    rows = [good[0], NAN_R, np.full(9, np.inf, np.float32), good[4], np.float32([np.inf, -np.inf] * 4 + [np.inf]), np.zeros(9, np.float32), np.float32(R * 1e30),
            np.float32((np.diag([1.0, 1.0, -1.0]) @ R.reshape(3, 3)).reshape(9)), one_nan, good[1], one_inf, np.float32(-0.0 * np.ones(9))]
    return np.stack(rows)


@pytest.mark.parametrize("fname,vname", [("sph", "pinhole"), ("sph", "fisheye"), ("sph", "brown"), ("sph", "surface"), ("cyl", "pinhole"), ("cyl", "surface"), ("roi", "tiles")])
def test_hostile_rotations_are_harmless(ms, cuda, fname, vname):
    """The host cannot inspect the table: any nine floats give what the formulas give for them -- the two-call route where ms_build_view_maps accepts the matrix
    (zeros, 1e30 R, a reflection), its numpy statement where it refuses (NaN, inf) --, MS_OK, every guard byte intact.  Harmless by construction: the taps are made
    from the two floats alone (rp_make_taps), whatever they are."""
    rng = np.random.default_rng(6000 + sum(map(ord, fname + vname)))
    poses = hostile_poses(rng)
    view = PC.VIEWS[vname]
    run_against_two_calls(ms, PC.FRAMES[fname], PC.random_sources(rng, len(poses)), [(view, 2, 3)], poses[None], (view["w"] + 5, view["h"] + 7))


# ---- 6. against numpy -------------------------------------------------------------------------------------------------------------------------------------------
def compare_where_maps_agree(ms, frame, view, R9, src, got, label):
    """got against RR.reproject_view at the numpy maps, on the pixels where the device's ms_build_view_maps entries for that pose equal numpy's float32 entries in
    both maps.  The share left out may not exceed 4 %: tests/test_reproject_gpu.py asserts a mean bit-equal share above 0.98 over the two maps on these frames and
    views, so at most 4 % of the pixels can differ in either."""
    mx, my = numpy_maps(frame, view, R9)
    dx, dy = ms.build_view_maps(RR.to_ms_frame(ms, frame), RR.to_ms_view(ms, PC.with_R(view, R9)))
    same = (host(dx).view(np.uint32) == mx.view(np.uint32)) & (host(dy).view(np.uint32) == my.view(np.uint32))
    left_out = 1.0 - same.mean()
    print("%s: %.4f %% of the pixels left out" % (label, 100 * left_out))
    assert left_out <= 0.04, (label, left_out)
    ref = RR.reproject_view(src, mx, my, bool(frame["wrap"]), bool(frame["clamp"]))
    assert np.array_equal(got[same], ref[same]), label
    return ref, same


@pytest.mark.parametrize("vname", ["pinhole", "fisheye", "surface"])
def test_against_the_numpy_statement(ms, cuda, vname):
    rng = np.random.default_rng(7000)
    frame, view = PC.FRAMES["sph"], PC.VIEWS[vname]
    srcs = PC.random_sources(rng, 3)
    poses = PC.random_poses(rng, 7)[[0, 2, 5]]      # the seam, a pole, a random pose
    out = [torch.full((view["h"], view["w"], 3), PAD, dtype=torch.uint8, device=cuda) for _ in srcs]
    ms.reproject_poses(RR.to_ms_frame(ms, frame), [to_dev(s) for s in srcs], out, pose_jobs(ms, [(view, 0, 0)]), to_dev(poses.reshape(-1)))
    torch.cuda.synchronize()
    for f in range(3):
        compare_where_maps_agree(ms, frame, view, poses[f], srcs[f], host(out[f]), "%s frame %d" % (vname, f))


# ---- 7. the whole route -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stitched(ms, cuda):
    """the mini6 rig (config 2's shape at 1/6 of its size), its canvas of the noise-free frames stitch_app generates, and where that canvas lies on the sphere"""
    cfg = synth.CONFIGS["mini6"]
    comp, _, _ = make_rig(ms, "mini6")
    out8 = torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device=cuda)
    comp.stitch([[to_dev(synth.frame(cfg["w"], cfg["h"], i, 0, noise=False)) for i in range(cfg["n"])]], out8u=[out8])
    torch.cuda.synchronize()
    pf = comp.pano_frame()
    comp.close()
    return cfg, out8, pf


def rig_Ry(deg):
    """ms_look_at_view's Ry"""
    a = deg * (math.pi / 180.0)
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float64)


def test_cube_map_of_a_stitched_canvas_under_a_rig_rotation(ms, cuda, stitched):
    """a 32 x 32 cube map under Ry(25 degrees) against the numpy route on the canvas: bytes equal wherever the device's map entries equal numpy's (at most 4 % of a
    face left out, as above); where a coordinate is the neighbouring float -- an ulp of at most 2^-16 px at these coordinates, times a slope of at most 255 levels per
    pixel on either axis, far below one level -- the rounded byte may differ by one"""
    cfg, out8, pf = stitched
    N = 32
    frame = dict(proj="sph", scale=float(pf.scale), u0=pf.u0, v0=pf.v0, wrap=pf.wrap_cols, clamp=pf.clamp_rows)
    assert frame["wrap"] == cfg["out_w"] and frame["clamp"] == 1
    faces = cube_views(N)
    jobs = [(ms.cube_face_view(face, N), x, y) for face, (_, x, y) in enumerate(faces)]
    poses = ms.view_pose_table(jobs, rig_Ry(25.0)[None])
    atlas = torch.full((2 * N, 3 * N, 3), PAD, dtype=torch.uint8, device=cuda)
    ms.reproject_poses(pf, [out8], [atlas], jobs, to_dev(poses.reshape(-1)))
    torch.cuda.synchronize()
    got, canvas = host(atlas), host(out8)
    for j, (view, x, y) in enumerate(faces):
        face = got[y:y + N, x:x + N]
        ref, same = compare_where_maps_agree(ms, frame, view, poses[j, 0], canvas, face, "face %d" % j)
        assert np.abs(face.astype(int) - ref.astype(int)).max() <= 1, j
    assert (got.max(axis=2) > 0).mean() > 0.25      # (the four horizontal faces look at the stitched band)
    level = host(ms.reproject([out8], [torch.zeros_like(atlas)], [(*ms.build_view_maps(pf, v), x, y) for v, x, y in jobs], pf.wrap_cols, pf.clamp_rows)[0])
    assert not np.array_equal(level, got), "25 degrees of yaw changed nothing"


# ---- 8. stitch_app ----------------------------------------------------------------------------------------------------------------------------------------------
def run_app(*args, check=True):
    cfg = synth.CONFIGS["mini6"]
    cmd = [APP, "--views", str(cfg["n"]), "--size", "%dx%d" % (cfg["w"], cfg["h"]), "--out", "%dx%d" % (cfg["out_w"], cfg["out_h"]),
           "--hfov", str(cfg["hfov_deg"]), "--bands", str(cfg["num_bands"]), "--frames", "8"] + [str(a) for a in args]
    if not check:
        return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = subprocess.check_output(cmd, timeout=300)
    return json.loads([l for l in out.decode().splitlines() if l.startswith("{")][-1])


def binding_orbit_frame(ms, out8, pf, jobs, w, h, i420, deg):
    """the binding's render of canvas n = 7 of an orbit of `deg` degrees per canvas"""
    poses = ms.view_pose_table(jobs, rig_Ry(7 * deg)[None])
    dst = torch.zeros((h * 3 // 2, w) if i420 else (h, w, 3), dtype=torch.uint8, device="cuda")
    ms.reproject_poses(pf, [out8], [dst], jobs, to_dev(poses.reshape(-1)), fmt=ms.VIEW_I420 if i420 else ms.VIEW_BGR)
    torch.cuda.synchronize()
    return host(dst)


@pytest.mark.parametrize("i420", [False, True])
def test_stitch_app_orbit_cubemap(ms, cuda, stitched, i420):
    cfg, out8, pf = stitched
    info = run_app("--cubemap", 64, "--orbit", 7, *(["--i420"] if i420 else []))
    assert info["frames"] == 8 and info["view_out"] == "192x128" and info["i420"] is i420 and info["orbit_deg"] == 7
    jobs = [(ms.cube_face_view(face, 64), (face % 3) * 64, (face // 3) * 64) for face in range(6)]
    frame = binding_orbit_frame(ms, out8, pf, jobs, 192, 128, i420, 7.0)
    assert info["view_checksum"] == "%016x" % RR.fnv1a0(frame)
    still = run_app("--cubemap", 64, *(["--i420"] if i420 else []))
    assert "orbit_deg" not in still and still["view_checksum"] != info["view_checksum"]


def test_stitch_app_orbit_viewport(ms, cuda, stitched):
    cfg, out8, pf = stitched
    info = run_app("--viewport", "30,10,0,90,320x180", "--orbit", 7)
    assert info["frames"] == 8 and info["view_out"] == "320x180" and info["orbit_deg"] == 7
    frame = binding_orbit_frame(ms, out8, pf, [(ms.look_at_view(30, 10, 0, 90, 320, 180), 0, 0)], 320, 180, False, 7.0)
    assert (frame.max(axis=2) > 0).mean() > 0.5
    assert info["view_checksum"] == "%016x" % RR.fnv1a0(frame)


def test_stitch_app_orbit_excludes_aa(ms):
    for args in (("--viewport", "30,10,0,90,320x180", "--orbit", 7, "--aa", 2), ("--cubemap", 64, "--aa", 3, "--orbit", 7), ("--orbit", 7)):
        r = run_app(*args, check=False)
        assert r.returncode == 2 and b"--orbit" in r.stderr, (args, r.returncode, r.stderr)
