"""Antialiased virtual cameras (include/ms_stitch.h section 5) without a device: ms_pano_mips_layout against the halving rule, every refusal of
ms_build_pano_mips / ms_build_view_footprint / ms_reproject_aa -- status code, a message naming the argument, no device touched (the data pointers are never
followed) --, the numpy statement's own consistency, and what antialiasing buys, asserted on the statement alone."""
import ctypes as C
import math

import numpy as np
import pytest

import np_ref
import reproject_aa_ref as AA
import reproject_ref as RR

INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -4


def refused(ms, rc, code, *words):
    msg = ms.load().ms_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def fake_image(ms, cols, rows, typ, step=None, addr=0x10000):
    """an ms_image whose data pointer is never followed: every refusal comes before the device is touched"""
    esz = {ms.MS_8UC1: 1, ms.MS_8UC3: 3, ms.MS_32FC1: 4}[typ]
    return ms.Image(addr, cols * esz if step is None else step, cols, rows, typ)


def with_(obj, **kw):
    o = type(obj).from_buffer_copy(obj)
    for k, val in kw.items():
        setattr(o, k, val)
    return o


# ---- ms_pano_mips_layout ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(96, 48), (45, 23), (1, 1), (2, 3)])
def test_layout_follows_the_halving_rule(ms, size):
    cols, rows = size
    for levels in range(1, ms.VIEW_MAX_LEVELS + 1):
        lv, nbytes = ms.pano_mips_layout(cols, rows, levels)
        assert [(l.cols, l.rows) for l in lv] == AA.level_sizes(cols, rows, levels)
        spans = []
        for l in lv:
            assert l.step >= 3 * l.cols and l.step % 16 == 0 and l.offset % 256 == 0      # the alignment the header states
            spans.append((l.offset, l.offset + (l.rows - 1) * l.step + 3 * l.cols))
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 <= b0, "levels overlap"
        assert spans[0][0] >= 0 and spans[-1][1] <= nbytes, "bytes does not cover the last level"
        # a shorter chain is a prefix of a longer one
        assert [(l.offset, l.step) for l in lv] == [(l.offset, l.step) for l in ms.pano_mips_layout(cols, rows, ms.VIEW_MAX_LEVELS)[0][:levels]]


def test_layout_refusals(ms):
    lib, who = ms.load(), "ms_pano_mips_layout"
    lv, n = (ms.MipLevel * ms.VIEW_MAX_LEVELS)(), C.c_size_t(0)
    refused(ms, lib.ms_pano_mips_layout(96, 48, 2, None, C.byref(n)), INVALID, who, "null")
    refused(ms, lib.ms_pano_mips_layout(96, 48, 2, lv, None), INVALID, who, "null")
    for levels in (0, -1, ms.VIEW_MAX_LEVELS + 1):
        refused(ms, lib.ms_pano_mips_layout(96, 48, levels, lv, C.byref(n)), INVALID, who, "levels")
    for cols, rows in ((0, 48), (96, 0), (32768, 48), (96, 32768), (-1, 5)):
        refused(ms, lib.ms_pano_mips_layout(cols, rows, 2, lv, C.byref(n)), INVALID, who, "cols x rows")
    assert lib.ms_pano_mips_layout(32767, 32767, ms.VIEW_MAX_LEVELS, lv, C.byref(n)) == 0 and n.value < 2 ** 32


# ---- ms_build_pano_mips ----------------------------------------------------------------------------------------------------------------------------------
def mips_call(ms, srcs, ptrs, n, levels):
    a = None if srcs is None else (ms.Image * len(srcs))(*srcs)
    p = None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)
    return ms.load().ms_build_pano_mips(a, p, n, levels, None)


def test_build_pano_mips_refusals(ms):
    who = "ms_build_pano_mips"
    _, nbytes = ms.pano_mips_layout(96, 48, 3)
    s = [fake_image(ms, 96, 48, ms.MS_8UC3, addr=0x100000 + i * 0x10000) for i in range(3)]
    m = [0x800000 + i * 0x10000 for i in range(3)]
    refused(ms, mips_call(ms, None, m, 3, 3), INVALID, who, "null")
    refused(ms, mips_call(ms, s, None, 3, 3), INVALID, who, "null")
    for n in (0, -1, ms.VIEW_MAX_FRAMES + 1):
        refused(ms, mips_call(ms, s, m, n, 3), INVALID, who, "n_frames")
    for levels in (0, ms.VIEW_MAX_LEVELS + 1):
        refused(ms, mips_call(ms, s, m, 3, levels), INVALID, who, "levels")
    refused(ms, mips_call(ms, [s[0], with_(s[1], type=ms.MS_8UC1), s[2]], m, 3, 3), INVALID, who, "src frame 1", "8UC3")
    refused(ms, mips_call(ms, [s[0], with_(s[1], data=None), s[2]], m, 3, 3), INVALID, who, "src frame 1")
    refused(ms, mips_call(ms, [s[0], s[1], with_(s[2], cols=95)], m, 3, 3), INVALID, who, "src frame 2", "geometry")
    refused(ms, mips_call(ms, [s[0], s[1], with_(s[2], step=300)], m, 3, 3), INVALID, who, "src frame 2", "geometry")
    refused(ms, mips_call(ms, [with_(s[0], step=1 << 24)], m, 1, 3), INVALID, who, "step")
    refused(ms, mips_call(ms, [fake_image(ms, 40000, 4, ms.MS_8UC3)], m, 1, 3), INVALID, who, "src cols x rows")
    refused(ms, mips_call(ms, s, [m[0], 0, m[2]], 3, 3), INVALID, who, "mips[1]", "null")
    refused(ms, mips_call(ms, s, [m[0], m[1] + 4, m[2]], 3, 3), INVALID, who, "mips[1]", "aligned")
    src_bytes = 47 * 288 + 288
    refused(ms, mips_call(ms, s, [m[0], s[2].data + src_bytes - 16, m[2]], 3, 3), INVALID, who, "mips[1] overlaps src frame 2")
    refused(ms, mips_call(ms, s, [m[0], m[1], m[0] + nbytes - 16], 3, 3), INVALID, who, "mips[2] overlaps mips[0]")
    assert mips_call(ms, s, [m[0], m[0] + nbytes, s[0].data - nbytes], 3, 3) == NO_DEVICE      # touching is not overlapping; past the checks: no device here


# ---- ms_build_view_footprint ---------------------------------------------------------------------------------------------------------------------------------
def foot_call(ms, frame, mx, my, fs, rho):
    p = lambda o: None if o is None else C.byref(o)
    return ms.load().ms_build_view_footprint(p(frame), p(mx), p(my), C.c_double(fs), p(rho), None)


def test_build_view_footprint_refusals(ms):
    who = "ms_build_view_footprint"
    fr = ms.PanoFrame.make(ms.PROJ_SPHERICAL, 96 / (2 * math.pi), -48, 0, 96, 1)
    mx, my, rho = [fake_image(ms, 37, 21, ms.MS_32FC1, addr=0x10000 * (i + 1)) for i in range(3)]
    for args in ((None, mx, my, 1.0, rho), (fr, None, my, 1.0, rho), (fr, mx, None, 1.0, rho), (fr, mx, my, 1.0, None)):
        refused(ms, foot_call(ms, *args), INVALID, who, "null")
    refused(ms, foot_call(ms, with_(fr, struct_size=4), mx, my, 1.0, rho), INVALID, who, "ms_pano_frame.struct_size")
    refused(ms, foot_call(ms, with_(fr, projection=ms.PROJ_PLANE), mx, my, 1.0, rho), UNSUPPORTED, who, "MS_PROJ_PLANE")
    refused(ms, foot_call(ms, with_(fr, projection=9), mx, my, 1.0, rho), INVALID, who, "src projection")
    for s in (0.0, -1.0, 8192.5, float("inf"), float("nan")):
        refused(ms, foot_call(ms, with_(fr, scale=s), mx, my, 1.0, rho), INVALID, who, "src scale")
    refused(ms, foot_call(ms, with_(fr, wrap_cols=-1), mx, my, 1.0, rho), INVALID, who, "wrap_cols")
    refused(ms, foot_call(ms, with_(fr, clamp_rows=2), mx, my, 1.0, rho), INVALID, who, "clamp_rows")
    for name, k in (("map_x", 0), ("map_y", 1), ("rho", 2)):
        def call(img):
            a = [mx, my, rho]
            a[k] = img
            return foot_call(ms, fr, a[0], a[1], 1.0, a[2])
        refused(ms, call(with_([mx, my, rho][k], type=ms.MS_8UC1)), INVALID, who, name, "32FC1")
        refused(ms, call(with_([mx, my, rho][k], data=None)), INVALID, who, name, "no data")
        refused(ms, call(with_([mx, my, rho][k], data=0x10002)), INVALID, who, name, "aligned")
        refused(ms, call(with_([mx, my, rho][k], step=37 * 4 + 2)), INVALID, who, name, "aligned")
        refused(ms, call(with_([mx, my, rho][k], step=36 * 4)), INVALID, who, name, "step")
        refused(ms, call(with_([mx, my, rho][k], cols=36, step=37 * 4)), INVALID, who, "one size")
        refused(ms, call(with_([mx, my, rho][k], rows=20)), INVALID, who, "one size")
    for fs in (0.0, -1.0, 16.5, float("inf"), float("nan")):
        refused(ms, foot_call(ms, fr, mx, my, fs, rho), INVALID, who, "footprint_scale")
    for fs in (1e-3, 1.0, 16.0):
        assert foot_call(ms, fr, mx, my, fs, rho) == NO_DEVICE


# ---- ms_reproject_aa -------------------------------------------------------------------------------------------------------------------------------------------
def aa_call(ms, srcs, mips, levels, dsts, jobs, wrap, clamp, fmt, n_frames=None, n_jobs=None):
    arr = lambda T, xs: None if xs is None else (T * len(xs))(*xs)
    p = None if mips is None else (C.c_void_p * len(mips))(*mips)
    return ms.load().ms_reproject_aa(arr(ms.Image, srcs), p, levels, arr(ms.Image, dsts), len(srcs) if n_frames is None else n_frames, arr(ms.ViewJobAA, jobs),
                                     (len(jobs) if jobs is not None else 1) if n_jobs is None else n_jobs, wrap, clamp, fmt, None)


def test_reproject_aa_refusals(ms):
    who = "ms_reproject_aa"
    _, nbytes = ms.pano_mips_layout(96, 48, 3)
    s = [fake_image(ms, 96, 48, ms.MS_8UC3, addr=0x100000 + i * 0x10000) for i in range(2)]
    d = [fake_image(ms, 64, 32, ms.MS_8UC3, addr=0x400000 + i * 0x10000) for i in range(2)]
    m = [0x800000, 0x810000]
    maps = lambda w, h, a: [fake_image(ms, w, h, ms.MS_32FC1, addr=a + i * 0x8000) for i in range(3)]
    job = lambda w, h, x, y, a=0x900000: ms.ViewJobAA(ms.ViewJob(maps(w, h, a)[0], maps(w, h, a)[1], x, y), maps(w, h, a)[2])
    J = [job(38, 22, 0, 0), job(20, 8, 40, 2, 0xa00000)]
    good = lambda **kw: aa_call(ms, kw.get("s", s), kw.get("m", m), kw.get("levels", 3), kw.get("d", d), kw.get("j", J), kw.get("wrap", 96), kw.get("clamp", 1),
                                kw.get("fmt", ms.VIEW_BGR), kw.get("n_frames"), kw.get("n_jobs"))
    assert good() == NO_DEVICE
    # its own
    refused(ms, good(m=None), INVALID, who, "null", "mips")
    for levels in (0, -2, ms.VIEW_MAX_LEVELS + 1):
        refused(ms, good(levels=levels), INVALID, who, "levels")
    refused(ms, good(m=[m[0], 0]), INVALID, who, "mips[1]", "null")
    refused(ms, good(m=[m[0], m[1] + 8]), INVALID, who, "mips[1]", "aligned")
    refused(ms, good(levels=6), INVALID, who, "2^levels", "96")                    # 96 = 32 x 3: five levels close the turn, six do not
    assert good(levels=5) == NO_DEVICE and good(levels=6, wrap=0) == NO_DEVICE
    refused(ms, good(j=[J[0], with_(J[1], rho=with_(J[1].rho, type=ms.MS_8UC1))]), INVALID, who, "jobs[1].rho", "32FC1")
    refused(ms, good(j=[J[0], with_(J[1], rho=with_(J[1].rho, data=None))]), INVALID, who, "jobs[1].rho", "no data")
    refused(ms, good(j=[J[0], with_(J[1], rho=with_(J[1].rho, data=0xa10002))]), INVALID, who, "jobs[1].rho", "aligned")
    refused(ms, good(j=[with_(J[0], rho=with_(J[0].rho, rows=21)), J[1]]), INVALID, who, "jobs[0]", "rho is 38 x 21")
    refused(ms, good(j=[with_(J[0], rho=with_(J[0].rho, cols=37)), J[1]]), INVALID, who, "jobs[0]", "rho is 37 x 22")
    d_bytes = 31 * 192 + 192
    refused(ms, good(m=[m[0], d[0].data + d_bytes - 16]), INVALID, who, "dst frame 0 overlaps mips[1]")
    refused(ms, good(m=[d[1].data - nbytes + 16, m[1]]), INVALID, who, "dst frame 1 overlaps mips[0]")
    refused(ms, good(s=[fake_image(ms, 40000, 4, ms.MS_8UC3)], m=m[:1], d=d[:1], wrap=0), INVALID, who, "src cols x rows")
    # everything ms_reproject refuses (tests/test_reproject_abi.py pins each message on ms_reproject; the same checks run here under this name)
    refused(ms, good(s=None, n_frames=2), INVALID, who, "null")
    refused(ms, good(d=None), INVALID, who, "null")
    refused(ms, good(j=None), INVALID, who, "null")
    for n in (0, ms.VIEW_MAX_FRAMES + 1):
        refused(ms, good(n_frames=n), INVALID, who, "n_frames")
    for n in (0, ms.VIEW_MAX_JOBS + 1):
        refused(ms, good(n_jobs=n), INVALID, who, "n_jobs")
    refused(ms, good(fmt=2), INVALID, who, "format")
    refused(ms, good(s=[s[0], with_(s[1], type=ms.MS_8UC1)]), INVALID, who, "src frame 1")
    refused(ms, good(s=[s[0], with_(s[1], rows=47)]), INVALID, who, "src frame 1", "geometry")
    refused(ms, good(s=[with_(s[0], step=1 << 24), with_(s[1], step=1 << 24)]), INVALID, who, "step")
    refused(ms, good(wrap=95), INVALID, who, "wrap_cols")
    refused(ms, good(clamp=2), INVALID, who, "clamp_rows")
    refused(ms, good(d=[d[0], with_(d[1], type=ms.MS_8UC1)]), INVALID, who, "dst frame 1")
    refused(ms, good(d=[d[0], with_(d[1], cols=63)]), INVALID, who, "dst frame 1", "geometry")
    refused(ms, good(j=[with_(J[0], job=with_(J[0].job, map_y=with_(J[0].job.map_y, cols=37))), J[1]]), INVALID, who, "jobs[0]", "map_x is 38 x 22")
    refused(ms, good(j=[with_(J[0], job=with_(J[0].job, map_x=with_(J[0].job.map_x, type=ms.MS_8UC1))), J[1]]), INVALID, who, "jobs[0].map_x", "32FC1")
    refused(ms, good(j=[with_(J[0], job=with_(J[0].job, map_x=with_(J[0].job.map_x, data=0x900002))), J[1]]), INVALID, who, "jobs[0].map_x", "aligned")
    refused(ms, good(j=[J[0], with_(J[1], job=with_(J[1].job, dst_x=50))]), INVALID, who, "jobs[1]", "leaves")
    refused(ms, good(j=[J[0], with_(J[1], job=with_(J[1].job, dst_x=30))]), INVALID, who, "jobs[0] and jobs[1] overlap")
    refused(ms, good(d=[with_(d[0], data=s[1].data + 64), d[1]]), INVALID, who, "dst frame 0 overlaps src frame 1")
    di = [fake_image(ms, 64, 48, ms.MS_8UC1, addr=0x400000 + i * 0x10000) for i in range(2)]
    assert good(d=di, fmt=ms.VIEW_I420) == NO_DEVICE
    refused(ms, good(d=di, fmt=ms.VIEW_I420, j=[J[0], with_(J[1], job=with_(J[1].job, dst_x=41))]), INVALID, who, "jobs[1]", "even")
    refused(ms, good(d=[with_(x, step=70) for x in di], fmt=ms.VIEW_I420), INVALID, who, "contiguous")


# ---- the numpy statement against itself ------------------------------------------------------------------------------------------------------------------------
def test_reference_level_choice_is_exact():
    L = 4
    one_up = np.nextafter(np.float32(1), np.float32(2))
    r = np.float32([0, 0.5, 1, one_up, 1.5, 2, 3, 4, 2 ** L, np.nextafter(np.float32(2 ** L), np.float32(np.inf)), 1e30, np.inf, np.nan, -3])
    l, t = AA.level_of(r, L)
    assert l.tolist() == [0, 0, 0, 0, 0, 1, 1, 2, L, L, L, L, 0, 0]
    assert t.tolist() == [0, 0, 0, float(one_up) - 1, 0.5, 0, 0.5, 0, 0, 0, 0, 0, 0, 0]
    # t = r 2^-l - 1 exactly, in [0, 1), over every binade below 2^L
    rr = np.random.default_rng(1).uniform(1, 2 ** L, 4000).astype(np.float32)
    rr = rr[rr < np.float32(2 ** L)]
    l, t = AA.level_of(rr, L)
    assert np.array_equal(l, np.floor(np.log2(rr.astype(np.float64))).astype(np.int64))
    assert np.array_equal(t.astype(np.float64), rr.astype(np.float64) / 2.0 ** l - 1) and (t >= 0).all() and (t < 1).all()


def test_reference_level_coordinates_map_pixel_centres():
    """level k's pixel x covers level-0 pixels 2^k x .. 2^k (x + 1) - 1: its centre, in level-0 coordinates, is 2^k (x + 1/2) - 1/2"""
    for k in range(AA.MAX_LEVELS + 1):
        x = np.arange(0, 50, dtype=np.float64)
        assert np.array_equal(AA.level_coords(np.float32(2.0 ** k * (x + 0.5) - 0.5), k), np.float32(x))


@pytest.mark.parametrize("wrap,clamp", [(0, 0), (1, 1)])
def test_reference_with_small_footprints_is_the_point_sampler(wrap, clamp):
    rng = np.random.default_rng(7 + wrap)
    src = rng.integers(0, 256, (48, 96, 3), dtype=np.uint8)
    mx = rng.uniform(-3, 99, (21, 37)).astype(np.float32); my = rng.uniform(-3, 51, (21, 37)).astype(np.float32)
    mx[0, :4] = [np.nan, np.inf, -1e30, -1]; my[0, :4] = [2, 3, 4, -1]
    chain = AA.mip_chain(src, 3)
    want = RR.reproject_view(src, mx, my, wrap, clamp)
    for rho in (np.zeros_like(mx), np.full_like(mx, 1), rng.uniform(-2, 1, mx.shape).astype(np.float32), np.full_like(mx, np.nan)):
        assert np.array_equal(AA.reproject_aa_view(chain, mx, my, rho, wrap, clamp), want)
    assert not np.array_equal(AA.reproject_aa_view(chain, mx, my, np.full_like(mx, 3), wrap, clamp), want)
    assert np.array_equal(np_ref.sat_u8(AA.chain_linear(RR.extend(src, wrap, clamp), RR.shifted(mx), RR.shifted(my))), want)


def test_reference_mip_chain_replicates_edges():
    src = np.arange(3 * 5 * 3, dtype=np.uint8).reshape(3, 5, 3) * 5
    l1 = AA.mip_chain(src, 2)[1]
    assert l1.shape == (2, 3, 3)
    q = src.astype(np.int64)
    assert l1[0, 0, 1] == (q[0, 0, 1] + q[0, 1, 1] + q[1, 0, 1] + q[1, 1, 1] + 2) >> 2
    assert l1[1, 2, 0] == q[2, 4, 0] and l1[0, 2, 2] == (2 * q[0, 4, 2] + 2 * q[1, 4, 2] + 2) >> 2 and l1[1, 0, 0] == (2 * q[2, 0, 0] + 2 * q[2, 1, 0] + 2) >> 2
    assert AA.mip_chain(src, 2)[2].shape == (1, 2, 3)
    assert (AA.mip_chain(np.full((7, 9, 3), 201, np.uint8), 3)[3] == 201).all()      # a constant image stays constant: the rounding has no drift


def test_reference_footprint_of_the_identity_and_the_poles():
    """an equirect resampled onto itself has a footprint of 1 on the equator and, with the spherical weight, 1 everywhere (the vertical step is always 1);
    halved in size, 2; a map with holes takes the backward difference, an isolated entry 0"""
    fr = dict(proj="sph", scale=float(np.float32(96 / (2 * math.pi))), u0=-48, v0=0, wrap=96, clamp=1)
    x, y = np.meshgrid(np.arange(96, dtype=np.float32), np.arange(48, dtype=np.float32))
    rho = AA.footprint(fr, x, y)
    assert np.allclose(rho, 1.0, atol=1e-12)
    assert np.allclose(AA.footprint(fr, x, y, 0.5), 0.5, atol=1e-12)
    rho2 = AA.footprint(fr, 2 * x[:24, :48], 2 * y[:24, :48])
    assert np.allclose(rho2, 2.0, atol=1e-12)
    cyl = dict(fr, proj="cyl")
    xs = np.roll(x, 5, axis=1)      # the seam inside the map: the jump of 95 columns unwraps to a step of 1
    assert np.allclose(AA.footprint(cyl, xs, y), 1.0, atol=1e-12)
    assert AA.footprint(dict(cyl, wrap=0), xs, y).max() == 95.0
    hx, hy = x.copy(), y.copy()
    hx[10, 11], hy[10, 11] = -1, -1
    hx[20, 20] = np.nan
    r = AA.footprint(cyl, hx, hy)
    assert r[10, 11] == 0 and r[20, 20] == 0 and r[10, 10] == 1 and r[9, 11] == 1 and r[20, 19] == 1
    lone = np.full((3, 3), -1, np.float32)
    lx, ly = lone.copy(), lone.copy()
    lx[1, 1], ly[1, 1] = 4, 5
    assert (AA.footprint(cyl, lx, ly) == 0).all()


# ---- what it buys ------------------------------------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_striped_sphere():
    """Stripes of period 3 panorama pixels on a 384 x 192 wrapped equirect, levels = 4, truth = an 8 x 8 supersample of the analytic scene.
    24 x 14 viewport of 90 degrees (footprint 3.3-5.1): the committed reference measures RMS 10.0 (antialiased) against 69.6 (point-sampled), ratio 0.144;
    the bound is twice that, 0.29, and below 1 in any case.  The moderate view (48 x 27 of 90 degrees, footprint 1.6-2.5) measures 32.2 against 30.3, ratio 1.06:
    isotropic trilinear over-blurs a signal barely above the view's Nyquist rate; printed and recorded in the README, not asserted below 1."""
    aa, point, (lo, hi) = AA.quality(RR.look_at(10, -10, 7, 90, 24, 14))
    print("coarse view: footprint %.2f-%.2f, RMS aa %.2f, point %.2f, ratio %.3f" % (lo, hi, aa, point, aa / point))
    assert 3.2 < lo < 3.4 and 5.0 < hi < 5.2
    assert aa / point < 0.29 and aa / point < 1
    aa2, point2, (lo2, hi2) = AA.quality(RR.look_at(10, -10, 7, 90, 48, 27))
    print("moderate view: footprint %.2f-%.2f, RMS aa %.2f, point %.2f, ratio %.3f" % (lo2, hi2, aa2, point2, aa2 / point2))
    assert 1.5 < lo2 < 1.7 and 2.4 < hi2 < 2.6
