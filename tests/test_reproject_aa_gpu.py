"""Antialiased virtual cameras on the device (include/ms_stitch.h section 5), bit for bit against the numpy statement tests/reproject_aa_ref.py: the mip chain
on pitched, guarded buffers; the footprints (float64 on both sides: equal or adjacent floats); the trilinear sampler on real and synthetic footprints, hostile
maps, both formats and across frame groups; the whole route on a stitched canvas and through stitch_app --aa."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import np_ref
import reproject_aa_cases as CS
import reproject_aa_ref as AA
import reproject_ref as RR
import synth
from helpers import host, make_rig, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "video-stitcher_amd", "stitch_app")
PAD, SRC_PAD, MIP_PAD, FILL = 0x5A, 0xAB, 0xC3, 777.0
GUARD = 64      # guard bytes either side of a mips buffer (a multiple of 16: the buffer stays aligned)


# ---- buffers ------------------------------------------------------------------------------------------------------------------------------------------------
class Pitched:
    """n images of one geometry inside ONE flat device buffer filled with `fill`: a pitched step, an odd byte offset of every base, guard bytes everywhere else"""
    def __init__(self, n, rows, cols, cn, fill, contiguous=False):
        self.rows, self.cols, self.cn, self.n = rows, cols, cn, n
        self.step = cols * cn + (0 if contiguous else 7)
        self.stride = rows * self.step + 33
        self.off = [11 + i * self.stride for i in range(n)]
        self.flat = torch.full((11 + n * self.stride + 64,), fill, dtype=torch.uint8, device="cuda")
        shape, strides = ((rows, cols, cn), (self.step, cn, 1)) if cn > 1 else ((rows, cols), (self.step, 1))
        self.views = [torch.as_strided(self.flat, shape, strides, o) for o in self.off]

    def index(self, i):
        r = np.arange(self.rows)[:, None, None] * self.step + np.arange(self.cols)[None, :, None] * self.cn + np.arange(self.cn)[None, None, :]
        return self.off[i] + (r if self.cn > 1 else r[..., 0])


def upload(srcs):
    S = Pitched(len(srcs), srcs[0].shape[0], srcs[0].shape[1], 3, SRC_PAD)
    for t, s in zip(S.views, srcs):
        t.copy_(torch.from_numpy(s).cuda())
    return S


class Mips:
    """n mips buffers cut out of one allocation full of MIP_PAD, GUARD bytes before, between and after them"""
    def __init__(self, ms, n, cols, rows, levels):
        self.levels, (self.lv, self.nbytes) = levels, ms.pano_mips_layout(cols, rows, levels)
        self.stride = (self.nbytes + GUARD + 15) // 16 * 16
        self.flat = torch.full((GUARD + n * self.stride + GUARD,), MIP_PAD, dtype=torch.uint8, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        self.bufs = [self.flat[GUARD + i * self.stride:GUARD + i * self.stride + self.nbytes] for i in range(n)]

    def expect(self, chains):
        """the whole allocation as it must look after ms_build_pano_mips: the levels' pixels, MIP_PAD everywhere else (guards, row padding, between levels)"""
        want = np.full(self.flat.shape[0], MIP_PAD, np.uint8)
        for i, chain in enumerate(chains):
            for l, img in zip(self.lv, chain[1:]):
                assert img.shape == (l.rows, l.cols, 3)
                idx = GUARD + i * self.stride + l.offset + np.arange(l.rows)[:, None, None] * l.step + np.arange(l.cols)[None, :, None] * 3 + np.arange(3)[None, None, :]
                want[idx] = img
        return want


def build_mips(ms, S, srcs, levels):
    M = Mips(ms, len(srcs), S.cols, S.rows, levels)
    ms.build_pano_mips(S.views, levels, out=M.bufs)
    torch.cuda.synchronize()
    chains = [AA.mip_chain(s, levels) for s in srcs]
    got, want = host(M.flat), M.expect(chains)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d bytes of the mips allocation differ, first at %d (got %d, want %d)" % (bad.size, bad[0], got[bad[0]], want[bad[0]])
    return M, chains


def random_sources(rng, n, cols, rows):
    return [rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) for _ in range(n)]


# ---- 1. the mip chain ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,rows,levels", [(96, 48, 1), (96, 48, 3), (96, 48, 5), (45, 23, 4), (45, 23, 6), (2, 3, 2), (300, 70, 4)])
def test_mip_chain_is_the_cascaded_box(ms, cuda, cols, rows, levels):
    """3 frames, each a ROI of a pitched allocation at an odd address; the mips buffers over-allocated: every byte of the allocation -- levels, row padding, the
    bytes between levels, the guards -- against the expectation.  45 x 23: odd sizes, replicated edges at every level; 300 x 70: more than one workgroup each way,
    whole and edge blocks in one row; levels 4 to 6: the second launch, on level 3."""
    rng = np.random.default_rng(100 + cols + levels)
    srcs = random_sources(rng, 3, cols, rows)
    S = upload(srcs)
    assert S.views[0].data_ptr() % 2 == 1
    build_mips(ms, S, srcs, levels)
    src_flat = host(S.flat)
    keep = np.ones(src_flat.shape, bool)
    for f in range(3):
        keep[S.index(f)] = False
    assert (src_flat[keep] == SRC_PAD).all()


def test_mip_chain_of_aligned_sources_and_many_frames(ms, cuda):
    """contiguous, 4-byte aligned sources (the aligned loads shift by 0: the seventh word is never read) and MS_VIEW_MAX_FRAMES of them in one call"""
    rng = np.random.default_rng(150)
    srcs = random_sources(rng, ms.VIEW_MAX_FRAMES, 64, 16)
    devs = [to_dev(s) for s in srcs]
    M = Mips(ms, len(srcs), 64, 16, 4)
    ms.build_pano_mips(devs, 4, out=M.bufs)
    torch.cuda.synchronize()
    assert np.array_equal(host(M.flat), M.expect([AA.mip_chain(s, 4) for s in srcs]))


# ---- 2. footprints ------------------------------------------------------------------------------------------------------------------------------------------------
def device_maps(ms, frame, view):
    return ms.build_view_maps(RR.to_ms_frame(ms, frame), RR.to_ms_view(ms, view))


@pytest.mark.parametrize("fname", sorted(CS.FRAMES))
@pytest.mark.parametrize("fscale", [0.5, 1.0])
def test_footprints_match_the_float64_reference(ms, cuda, fname, fscale):
    """Bound (derived as test_reproject_gpu.py::test_view_maps_match_the_float64_reference's): both sides compute in double from the SAME float maps -- differences,
    floor, one sin, two hypot, a few ulps of double in all -- far below the half ulp of the one rounding to float, so the two floats are equal or adjacent.
    rho is exactly 0 on unseen pixels; nothing outside rho's ROI is written."""
    frame = CS.FRAMES[fname]
    equal = total = 0
    for vname in sorted(CS.VIEWS):
        view = CS.VIEWS[vname]
        mx, my = device_maps(ms, frame, view)
        big = torch.full((view["h"] + 5, view["w"] + 9), FILL, device="cuda")
        rho = big[2:2 + view["h"], 3:3 + view["w"]]
        ms.build_view_footprint(RR.to_ms_frame(ms, frame), mx, my, fscale, out=rho)
        torch.cuda.synchronize()
        guard = np.ones(tuple(big.shape), bool)
        guard[2:2 + view["h"], 3:3 + view["w"]] = False
        assert (host(big)[guard] == FILL).all(), vname
        hx, hy = host(mx), host(my)
        ref = AA.footprint(frame, hx, hy, fscale)
        got = host(rho)
        seen = AA.seen_entries(hx, hy)
        if vname == "brown":
            assert (~seen).any() and seen[view["h"] // 2, view["w"] // 2]
        else:
            assert seen.all(), vname
        assert (got[~seen] == 0).all(), vname
        r32 = np.float32(ref)
        ok = (got == r32) | (got == np.nextafter(r32, np.float32(np.inf))) | (got == np.nextafter(r32, np.float32(-np.inf)))
        assert ok.all(), (vname, np.argwhere(~ok)[:5], got[~ok][:5], ref[~ok][:5])
        equal += int((got == r32).sum()); total += got.size
        if vname in ("one",):
            assert got.shape == (1, 1) and got[0, 0] == 0      # no neighbour on either axis
        if vname == "column":
            assert got.shape == (9, 1) and (got > 0).all()
    print("bit-equal share %s: %.6f" % (fname, equal / total))
    assert equal / total > 0.98      # (roundings differ only where the double lies at a float32 rounding boundary)
    # the seam view's footprint does not see the jump of 96 columns
    if frame["wrap"]:
        mx, my = device_maps(ms, frame, CS.VIEWS["seam"])
        assert float(host(mx).max() - host(mx).min()) > 90 and float(host(ms.build_view_footprint(RR.to_ms_frame(ms, frame), mx, my)).max()) < 4


# ---- 3. the sampler -----------------------------------------------------------------------------------------------------------------------------------------------
def expect_i420(want_flat, idx, W, H, rect, bgr):
    x, y, w, h = rect
    planes = np_ref.bgr_to_i420(bgr)
    flat = idx.reshape(-1)
    Y = flat[:W * H].reshape(H, W); U = flat[W * H:W * H + (W // 2) * (H // 2)].reshape(H // 2, W // 2); V = flat[W * H + (W // 2) * (H // 2):].reshape(H // 2, W // 2)
    want_flat[Y[y:y + h, x:x + w]] = planes[:h]
    chroma = planes.reshape(-1)[w * h:]
    want_flat[U[y // 2:(y + h) // 2, x // 2:(x + w) // 2]] = chroma[:(w // 2) * (h // 2)].reshape(h // 2, w // 2)
    want_flat[V[y // 2:(y + h) // 2, x // 2:(x + w) // 2]] = chroma[(w // 2) * (h // 2):].reshape(h // 2, w // 2)


def run_aa(ms, srcs, jobs, atlas_wh, wrap, clamp, levels, i420=False, also_plain=()):
    """ms_build_pano_mips + ms_reproject_aa into pitched (BGR) or contiguous (I420) frames full of PAD; the WHOLE destination buffer against the reference.
    jobs: (mx, my, rho, dst_x, dst_y) numpy.  also_plain: indices of jobs whose result must also equal the device's own ms_reproject on the same maps."""
    W, H = atlas_wh
    S = upload(srcs)
    M, chains = build_mips(ms, S, srcs, levels)
    D = Pitched(len(srcs), H * 3 // 2, W, 1, PAD, contiguous=True) if i420 else Pitched(len(srcs), H, W, 3, PAD)
    dev_jobs = [(to_dev(mx), to_dev(my), to_dev(rho), dx, dy) for mx, my, rho, dx, dy in jobs]
    ms.reproject_aa(S.views, M.bufs, levels, D.views, dev_jobs, S.cols if wrap else 0, clamp, fmt=ms.VIEW_I420 if i420 else ms.VIEW_BGR)
    torch.cuda.synchronize()
    got = host(D.flat).copy()
    want = np.full(got.shape, PAD, np.uint8)
    for f in range(len(srcs)):
        idx = D.index(f)
        for mx, my, rho, dx, dy in jobs:
            ref = AA.reproject_aa_view(chains[f], mx, my, rho, wrap, clamp)
            if i420:
                expect_i420(want, idx, W, H, (dx, dy, mx.shape[1], mx.shape[0]), ref)
            else:
                want[idx[dy:dy + mx.shape[0], dx:dx + mx.shape[1]]] = ref
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d bytes differ, first at flat offset %d (got %d, want %d)" % (bad.size, bad[0], got[bad[0]], want[bad[0]])
    assert np.array_equal(host(M.flat), M.expect(chains)), "ms_reproject_aa wrote into the mips allocation"
    if also_plain:
        P = Pitched(len(srcs), H * 3 // 2, W, 1, PAD, contiguous=True) if i420 else Pitched(len(srcs), H, W, 3, PAD)
        ms.reproject(S.views, P.views, [(j[0], j[1], j[3], j[4]) for k, j in enumerate(dev_jobs) if k in also_plain], S.cols if wrap else 0, clamp,
                     fmt=ms.VIEW_I420 if i420 else ms.VIEW_BGR)
        torch.cuda.synchronize()
        plain = host(P.flat)
        for f in range(len(srcs)):
            idx = P.index(f)
            for k in also_plain:
                mx, dx, dy = jobs[k][0], jobs[k][3], jobs[k][4]
                r = idx[dy:dy + mx.shape[0], dx:dx + mx.shape[1]]
                assert np.array_equal(plain[r], got[r]), "ms_reproject_aa differs from ms_reproject where rho <= 1"
    return got


def view_job(ms, frame, view, fscale=1.0):
    mx, my = device_maps(ms, frame, view)
    rho = ms.build_view_footprint(RR.to_ms_frame(ms, frame), mx, my, fscale)
    return host(mx), host(my), host(rho)


@pytest.mark.parametrize("fname", sorted(CS.FRAMES))
@pytest.mark.parametrize("levels", [1, 3])
def test_sampler_on_real_footprints(ms, cuda, fname, levels):
    """each frame kind, the five 38 x 22 views -- rho below 1 everywhere, over two to three levels, at the poles, across the seam -- in one call, two frames"""
    frame = CS.FRAMES[fname]
    rng = np.random.default_rng(300 + levels)
    srcs = random_sources(rng, 2, *CS.SRC_SIZE)
    jobs, spans = [], {}
    names = sorted(CS.AA_VIEWS) + ["wide"]      # the wide view twice: as it is (levels 0 and 1) and with footprint_scale 4 (levels 1 to 3)
    for i, vname in enumerate(names):
        mx, my, rho = view_job(ms, frame, CS.AA_VIEWS[vname], 4.0 if i == len(names) - 1 else 1.0)
        spans[vname + str(i)] = (float(rho.min()), float(rho.max()))
        jobs.append((mx, my, rho, 3 + 40 * (i % 3), 2 + 24 * (i // 3)))
    print(fname, spans)
    fine, wide = names.index("fine"), names.index("wide")
    assert spans["fine%d" % fine][1] <= 1 and spans["wide%d" % wide][0] < 1 < spans["wide%d" % wide][1] and spans["wide5"][0] > 2 and spans["wide5"][1] > 4
    run_aa(ms, srcs, jobs, (3 + 120 + 2, 2 + 48 + 3), frame["wrap"] != 0, frame["clamp"], levels, also_plain=(fine,))


@pytest.mark.parametrize("n_frames", [1, 9])
@pytest.mark.parametrize("i420", [False, True])
def test_sampler_formats_and_frame_groups(ms, cuda, n_frames, i420):
    """BGR and I420, one frame and MS_VIEW_FRAME_GROUP + 1; two jobs with different footprints (fine: the one-level path; wide at footprint_scale 4) touching in one guarded atlas"""
    assert ms.VIEW_FRAME_GROUP == 8
    frame = CS.FRAMES["sph"]
    rng = np.random.default_rng(400 + n_frames)
    srcs = random_sources(rng, n_frames, *CS.SRC_SIZE)
    a, b = view_job(ms, frame, CS.AA_VIEWS["fine"]), view_job(ms, frame, CS.AA_VIEWS["wide"], 4.0)
    run_aa(ms, srcs, [a + (4, 2), b + (42, 2)], (84, 26), True, 1, 3, i420=i420, also_plain=(0,))


def random_maps(rng, w, h, cols, rows):
    return rng.uniform(-3, cols + 3, (h, w)).astype(np.float32), rng.uniform(-3, rows + 3, (h, w)).astype(np.float32)


@pytest.mark.parametrize("levels", [1, 3, 4])
@pytest.mark.parametrize("wrap,clamp", [(0, 0), (1, 1)])
def test_sampler_on_synthetic_footprints(ms, cuda, levels, wrap, clamp):
    """constant rho planes at every edge of the level choice, over one random map that reaches past every border; the planes not above 1 and the NaN plane also
    equal the device's own ms_reproject"""
    cols, rows = (96, 48) if wrap else (45, 23)
    rng = np.random.default_rng(500 + levels + wrap)
    srcs = random_sources(rng, 2, cols, rows)
    mx, my = random_maps(rng, 13, 7, cols, rows)
    top = np.float32(2 ** levels)
    values = [0, 0.5, 1, np.nextafter(np.float32(1), np.float32(2)), 1.5, 2, 3, 4, top, np.nextafter(top, np.float32(np.inf)), 1e30, np.inf, np.nan, -3]
    jobs = [(mx, my, np.full(mx.shape, v, np.float32), 1 + 14 * (i % 5), 1 + 8 * (i // 5)) for i, v in enumerate(values)]
    plain = tuple(i for i, v in enumerate(values) if not v > 1)
    assert len(plain) == 5
    run_aa(ms, srcs, jobs, (72, 26), wrap, clamp, levels, also_plain=plain)
    # one plane that mixes every value pixel by pixel: lanes of one wave on different levels
    mixed = np.float32(values)[rng.integers(0, len(values), mx.shape)]
    run_aa(ms, srcs[:1], [(mx, my, mixed, 0, 0)], (13, 7), wrap, clamp, levels)


@pytest.mark.parametrize("wrap,clamp", [(0, 0), (1, 1)])
def test_sampler_on_hostile_maps(ms, cuda, wrap, clamp):
    """maps full of NaN, +-inf, +-1e30 and the (-1, -1) marker under rho = 3: the output equals the reference, every guard byte -- destination, mips, source -- is intact"""
    cols, rows = 96, 48
    rng = np.random.default_rng(600 + wrap)
    srcs = random_sources(rng, 2, cols, rows)
    mx, my = random_maps(rng, 38, 22, cols, rows)
    xs = [np.nan, np.inf, -np.inf, 1e30, -1e30, -1.0, 0.0, cols - 0.5, cols, 2 * cols, -0.5, 5.25]
    ys = [np.nan, np.inf, -np.inf, 1e30, -1e30, -1.0, 0.0, rows - 0.5, rows, 2 * rows, -0.5, 3.75]
    grid = [(x, y) for y in ys for x in xs]
    for k, g in enumerate(rng.permutation(len(grid))):
        mx.reshape(-1)[k], my.reshape(-1)[k] = grid[g]
    mx[-1, -3:], my[-1, -3:] = -1, -1
    run_aa(ms, srcs, [(mx, my, np.full(mx.shape, 3, np.float32), 2, 1)], (43, 25), wrap, clamp, 3)
    run_aa(ms, srcs, [(mx, my, rng.uniform(0, 9, mx.shape).astype(np.float32), 0, 0)], (38, 22), wrap, clamp, 3, i420=True)


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stitched(ms, cuda):
    """the mini6 rig (the smallest of helpers.make_rig), its canvas of the noise-free frames stitch_app generates, and where that canvas lies on the sphere"""
    cfg = synth.CONFIGS["mini6"]
    comp, _, _ = make_rig(ms, "mini6")
    out8 = torch.zeros((cfg["out_h"], cfg["out_w"], 3), dtype=torch.uint8, device=cuda)
    comp.stitch([[to_dev(synth.frame(cfg["w"], cfg["h"], i, 0, noise=False)) for i in range(cfg["n"])]], out8u=[out8])
    torch.cuda.synchronize()
    pf = comp.pano_frame(ms.PANO_CANVAS)
    comp.close()
    return cfg, out8, pf


def python_route(ms, out8, pf, view, levels):
    mx, my = ms.build_view_maps(pf, view)
    rho = ms.build_view_footprint(pf, mx, my)
    mips = ms.build_pano_mips([out8], levels)
    dst = torch.full((view.height, view.width, 3), PAD, dtype=torch.uint8, device="cuda")
    ms.reproject_aa([out8], mips, levels, [dst], [(mx, my, rho, 0, 0)], pf.wrap_cols, pf.clamp_rows)
    torch.cuda.synchronize()
    return host(dst), host(mx), host(my), host(rho)


def test_whole_route_on_a_stitched_canvas(ms, cuda, stitched):
    """ms_stitch -> ms_get_pano_frame(MS_PANO_CANVAS) -> maps -> footprints -> mips -> ms_reproject_aa equals the reference applied to the downloaded canvas"""
    cfg, out8, pf = stitched
    assert pf.wrap_cols == cfg["out_w"] and pf.clamp_rows == 1
    got, mx, my, rho = python_route(ms, out8, pf, ms.look_at_view(30, 10, 0, 90, 64, 36), 3)
    assert rho.min() > 1.5 and rho.max() < 4
    want = AA.reproject_aa_view(AA.mip_chain(host(out8), 3), mx, my, rho, True, True)
    assert np.array_equal(got, want)
    assert (got.max(axis=2) > 0).mean() > 0.5


def run_app(*args):
    cfg = synth.CONFIGS["mini6"]
    out = subprocess.check_output([APP, "--views", str(cfg["n"]), "--size", "%dx%d" % (cfg["w"], cfg["h"]), "--out", "%dx%d" % (cfg["out_w"], cfg["out_h"]),
                                   "--hfov", str(cfg["hfov_deg"]), "--bands", str(cfg["num_bands"]), "--frames", "8"] + [str(a) for a in args], timeout=300)
    return json.loads([l for l in out.decode().splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("size", [(320, 180), (64, 36)])
def test_stitch_app_viewport_aa(ms, cuda, stitched, size):
    """stitch_app --viewport ... --aa 3 at the size the existing viewport test uses (footprint below 1: the one-level path) and at a fifth of it (footprint 3):
    the checksum of the last frame equals the same calls through the binding; without --aa the program prints what it printed before"""
    cfg, out8, pf = stitched
    w, h = size
    spec = "30,10,0,90,%dx%d" % (w, h)
    info = run_app("--viewport", spec, "--aa", 3)
    assert info["frames"] == 8 and info["view_out"] == "%dx%d" % (w, h) and info["aa_levels"] == 3
    got, mx, my, rho = python_route(ms, out8, pf, ms.look_at_view(30, 10, 0, 90, w, h), 3)
    assert info["view_checksum"] == "%016x" % RR.fnv1a0(got)
    plain = run_app("--viewport", spec)
    assert "aa_levels" not in plain
    dst = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    ms.reproject([out8], [dst], [(to_dev(mx), to_dev(my), 0, 0)], pf.wrap_cols, pf.clamp_rows)
    torch.cuda.synchronize()
    assert plain["view_checksum"] == "%016x" % RR.fnv1a0(host(dst))
    assert (plain["view_checksum"] == info["view_checksum"]) == (float(rho.max()) <= 1)
