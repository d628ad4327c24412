"""The panorama-writing kernels on the output layouts integrators hand over: pitched rows (step != cols * elemsize), images that start at any byte of a larger
allocation, another layout for every frame of a call.  shim/ms_shim.hpp passes a cv::cuda::GpuMat's data / step straight through, and GpuMats come from a pitched
allocator or are ROIs of a larger canvas; every other test of the suite writes into whole contiguous torch tensors.

Three kernels write the panorama: k_blend8 (the tiled level-0 band kernel: eight pixels per lane row as one 48-byte 16S / 24-byte 8U store where the whole group is
inside the image, pixel by pixel along the edges), k_blend at level 0 (debug_simple_kernels) and k_single_band (feather / zero bands).  Every case here

  * builds its outputs inside canary buffers (Canary): a position-dependent byte pattern in front of, between the rows of and behind the image,
  * asserts the image bit-equal to what the same context writes for the same frames into an ordinary contiguous tensor with the same in-image fill
    (pixels the contract leaves untouched must keep the fill in both), and
  * asserts that every byte outside the image's rows x row bytes still holds the pattern (guards and row padding).

One case per kernel is compared with the oracle as well.  All buffers of a call are sized for the largest step of the call, so a kernel that mixed up two frames'
steps would fail an assertion inside memory the test owns.  The second half pins the step rule of include/ms_stitch.h: what check_call refuses before anything is
enqueued."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from helpers import host, make_rig, oracle_blender_from, to_dev

pytestmark = pytest.mark.gpu

FILL8, FILL16 = 9, -7


# ---- canary buffers ------------------------------------------------------------------------------------------------------------------------------------------
def _base256():
    i = torch.arange(256, dtype=torch.int32, device="cuda")
    return ((i * 131 + 7) & 0xff).to(torch.uint8)          # byte i of every buffer = (i * 131 + 7) & 0xff: period 256, no two neighbours equal


def _round_up(a, m):
    return -(-a // m) * m


def pattern_buffer(nbytes, dtype=torch.uint8):
    """flat device buffer of nbytes (a multiple of 256) filled with the pattern; returns (tensor of dtype, its bytes)"""
    assert nbytes % 256 == 0
    es = torch.empty((), dtype=dtype).element_size()
    flat = torch.empty(nbytes // es, dtype=dtype, device="cuda")
    b = flat.view(torch.uint8)
    b.view(-1, 256).copy_(_base256().expand(nbytes // 256, 256))
    return flat, b


def pattern_intact(b):
    return bool((b.view(-1, 256) == _base256()).all())


class Canary:
    """An image of `shape` ((rows, cols, 3) or (rows, cols)) inside a flat pattern buffer: row step = row bytes + extra, first pixel `offset` bytes behind the front
    guard.  The guards are one row of the largest step plus 256 bytes, rounded up to 512 (torch allocations are 512-byte aligned: the image's address modulo 512 is
    `offset`); the rows are laid out for max(step, size_step), the largest step of the call this buffer takes part in.  16S buffers are allocated as int16, so
    offsets and steps are even by construction."""

    def __init__(self, shape, dtype, extra=0, offset=0, size_step=0, fill=None):
        self.rows, self.cols = shape[0], shape[1]
        cn = shape[2] if len(shape) == 3 else 1
        es = torch.empty((), dtype=dtype).element_size()
        assert extra % es == 0 and offset % es == 0 and 0 <= offset <= 16
        self.row_bytes = self.cols * cn * es
        self.step = self.row_bytes + extra
        big = max(self.step, size_step)
        guard = _round_up(big + 256, 512)
        self.total = _round_up(guard + 16 + self.rows * big + guard, 512)
        self.flat, self.bytes = pattern_buffer(self.total, dtype)
        self.start = guard + offset
        strides = (self.step // es, cn, 1) if cn > 1 else (self.step // es, 1)
        self.view = self.flat.as_strided(tuple(shape), strides, self.start // es)
        assert self.view.data_ptr() % 512 == offset and self.view.stride(0) * es == self.step
        if fill is not None:
            if torch.is_tensor(fill):
                self.view.copy_(fill)
            else:
                self.view.fill_(fill)
            self.check_outside("after the test's own fill")

    def check_outside(self, what):
        """every byte outside rows x row bytes of the image still holds the pattern: front guard, row padding, back guard"""
        idx = torch.arange(self.total, dtype=torch.int64, device="cuda") - self.start
        r = torch.div(idx, self.step, rounding_mode="floor")
        inside = (idx >= 0) & (r < self.rows) & (idx - r * self.step < self.row_bytes)
        want = _base256().repeat(self.total // 256)
        bad = torch.nonzero((self.bytes != want) & ~inside).flatten()
        if bad.numel():
            first = [(int(i) - self.start, divmod(int(i) - self.start, self.step)) for i in bad[:6]]
            raise AssertionError("%s: %d bytes outside the image were overwritten (step %d, row bytes %d, %d rows); first (byte from image start, (row, byte in row)): %s"
                                 % (what, bad.numel(), self.step, self.row_bytes, self.rows, first))


def same_pixels(got, want, what):
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        raise AssertionError("%s: %d elements differ from the contiguous result; first (y, x, c): %s" % (what, bad.shape[0], bad[:5].tolist()))


def pad512(row_bytes):
    return -row_bytes % 512          # what a pitched allocator that rounds rows up to 512 bytes adds (the GpuMat case)


def layouts8(cols):
    """(extra, offset) of the 8UC3 cases: the control, the 512 round-up, odd steps (every row at another address modulo 4) and every start address modulo 4; the
    24-byte stores of k_blend8 see addresses 0 / 1 / 2 / 3 / 5 / 9 + 3 * (x + canvas_x) modulo 16.  (2, 3) adds the step class 2 modulo 4, which the round-up and the
    odd extras do not reach."""
    p = pad512(cols * 3)
    return [(0, 0), (p, 0), (p, 3), (1, 1), (3, 2), (7, 5), (13, 9), (2, 3)]


def layouts16(cols):
    """(extra, offset) of the 16SC3 cases: even by construction; offsets 0 / 2 / 6 / 14 modulo 16 for the 48-byte stores, steps 0 and 2 modulo 4"""
    p = pad512(cols * 6)
    return [(0, 0), (p, 0), (p, 6), (2, 2), (6, 14), (10, 6), (2, 0), (10, 14)]


def check_layout_lists():
    for c in (640, 512, 2000):
        l8 = layouts8(c)
        assert {o % 4 for _, o in l8} == {0, 1, 2, 3} and {e % 4 for e, _ in l8} == {0, 1, 2, 3} and {o for _, o in l8} == {0, 1, 2, 3, 5, 9}
    for c in (639, 510, 777):
        l16 = layouts16(c)
        assert {o % 16 for _, o in l16} == {0, 2, 6, 14} and {e % 4 for e, _ in l16} == {0, 2} and all(e % 2 == 0 and o % 2 == 0 for e, o in l16)


check_layout_lists()


# ---- shared plumbing -----------------------------------------------------------------------------------------------------------------------------------------
_FRAMES = {}


def dev_frames(cfg, t):
    """the rig's synthetic frame set t on the device, made once per session and only ever read"""
    key = (cfg["w"], cfg["h"], cfg["n"], t)
    if key not in _FRAMES:
        _FRAMES[key] = [to_dev(synth.frame(cfg["w"], cfg["h"], i, t)) for i in range(cfg["n"])]
    return _FRAMES[key]


def shapes(comp, out_w, out_h):
    pg = comp.pano_geom()
    return (out_h, out_w, 3), (pg.dst_roi_final.height, pg.dst_roi_final.width, 3)


def contiguous(s8, s16):
    return torch.full(s8, FILL8, dtype=torch.uint8, device="cuda"), torch.full(s16, FILL16, dtype=torch.int16, device="cuda")


def canvas_ref(ref16, pg, out_w, out_h, fill):
    """the oracle's 16S panorama as the 8U canvas: saturate_cast<uchar> at (canvas_x, canvas_y), `fill` wherever the panorama ROI does not reach"""
    ref = np.full((out_h, out_w, 3), fill, np.uint8)
    fh, fw = ref16.shape[:2]
    x0, y0 = pg.canvas_x, pg.canvas_y
    xs0, ys0, xs1, ys1 = max(0, -x0), max(0, -y0), min(fw, out_w - x0), min(fh, out_h - y0)
    ref[y0 + ys0:y0 + ys1, x0 + xs0:x0 + xs1] = np.clip(ref16[ys0:ys1, xs0:xs1], 0, 255).astype(np.uint8)
    return ref


def run_layouts(call, s8, s16, what, l8=None, l16=None):
    """`call(out8u, out16s)` (either may be None) into contiguous tensors once, then into every layout pair: 8U and 16S together, and each alone.  Returns the last
    pair of canaries (both outputs written) for a comparison with the oracle."""
    want = {}
    for mode in ("both", "8u", "16s"):
        w8, w16 = contiguous(s8, s16)
        call(w8 if mode != "16s" else None, w16 if mode != "8u" else None)
        want[mode] = (w8, w16)
    torch.cuda.synchronize()
    l8, l16 = l8 or layouts8(s8[1]), l16 or layouts16(s16[1])
    last = None
    for (e8, o8), (e16, o16) in zip(l8, l16):
        size_step = max(s8[1] * 3 + e8, s16[1] * 6 + e16)
        for mode in ("both", "8u", "16s"):
            c8 = Canary(s8, torch.uint8, e8, o8, size_step, FILL8)
            c16 = Canary(s16, torch.int16, e16, o16, size_step, FILL16)
            call(c8.view if mode != "16s" else None, c16.view if mode != "8u" else None)
            torch.cuda.synchronize()
            tag = "%s, %s, 8U (extra %d, offset %d), 16S (extra %d, offset %d)" % (what, mode, e8, o8, e16, o16)
            c8.check_outside(tag + ": 8U canvas")          # (the guards first: a spill past a row end also corrupts the contiguous reference, where it lands in the next row)
            c16.check_outside(tag + ": 16S panorama")
            same_pixels(c8.view, want[mode][0], tag + ": 8U canvas")
            same_pixels(c16.view, want[mode][1], tag + ": 16S panorama")
            if mode == "both":
                last = (c8, c16)
    # the contiguous references themselves: an output that is not handed over stays at its fill, the ones written agree between the three calls
    assert torch.equal(want["both"][0], want["8u"][0]) and torch.equal(want["both"][1], want["16s"][1]), what
    assert bool((want["16s"][0] == FILL8).all()) and bool((want["8u"][1] == FILL16).all()), what
    return last, want["both"]


def oracle_pano(O, comp, cfg, gains, frames_np):
    b, _ = oracle_blender_from(O, comp, cfg)
    for i in range(cfg["n"]):
        xm, ym = [host(t) for t in comp.maps(i)]
        b.stitch_online(i, frames_np[i], xm, ym, gains[i])
    out, _ = b.blend()
    b.close()
    return out


# ---- k_blend8 and k_blend at level 0 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("simple", [False, True], ids=["k_blend8", "k_blend"])
@pytest.mark.parametrize("rig", ["mini6", "mini4"])
def test_band_kernels_on_pitched_offset_outputs(ms, cuda, oracle, rig, simple):
    """The level-0 band kernels of a multiband context: the tiled k_blend8 (default) and the one-pixel-per-lane k_blend (debug_simple_kernels).  On these rigs the
    panorama ROI is 639 x 105 / 510 x 134 at canvas (1, y > 0) of a 640 x 320 / 512 x 256 canvas: the ROI width is no multiple of 8, so k_blend8's last cell of a row
    stores pixel by pixel (nvalid = 7 / 6) while the others take the 48- / 24-byte stores, and the canvas has rows above and below the ROI and a column beside it
    that must keep the fill."""
    comp, cfg, gains = make_rig(ms, rig, simple_kernels=simple)
    pg = comp.pano_geom()
    s8, s16 = shapes(comp, cfg["out_w"], cfg["out_h"])
    fw, fh = s16[1], s16[0]
    assert fw % 8 != 0 and fw > 16, "both store forms of k_blend8: full groups of 8 pixels and a partial one at the row end"
    assert pg.canvas_x > 0 and pg.canvas_y > 0 and pg.canvas_y + fh < cfg["out_h"] and pg.canvas_x + fw <= cfg["out_w"], "the 8U canvas is larger than the ROI, at an offset"
    assert (3 * pg.canvas_x) % 4 != 0, "the 8U stores start off the dword grid even in an aligned canvas"
    st = comp.plan_stats()
    assert st["n_blend_tiles"][0] > 0, "level 0 has a tile list: the tiled band kernel runs it unless debug_simple_kernels is set"
    frames = dev_frames(cfg, 2)
    last, want = run_layouts(lambda o8, o16: comp.stitch([frames], out8u=None if o8 is None else [o8], out16s=None if o16 is None else [o16]), s8, s16, rig)
    # the pitched result itself against the oracle, and the canvas the fill was left in
    ref16 = oracle_pano(oracle, comp, cfg, gains, [synth.frame(cfg["w"], cfg["h"], i, 2) for i in range(cfg["n"])])
    assert np.array_equal(host(last[1].view), ref16)
    assert np.array_equal(host(last[0].view), canvas_ref(ref16, pg, cfg["out_w"], cfg["out_h"], FILL8))
    got8 = host(want[0])
    assert (got8[:pg.canvas_y] == FILL8).all() and (got8[pg.canvas_y + fh:] == FILL8).all() and (got8[:, :pg.canvas_x] == FILL8).all()
    comp.close()


# ---- k_single_band ---------------------------------------------------------------------------------------------------------------------------------------------
def test_feather_kernel_on_pitched_offset_outputs(ms, cuda, oracle):
    """k_single_band with FeatherBlender weights on BASELINE configs[0] (2 views 640 x 480 -> 2000 x 1000), as test_feather_blender_matches_oracle sets it up."""
    import math
    n, w, h, out = 2, 640, 480, (2000, 1000)
    sc = float(np.float32(2000.0 / (2 * math.pi)))
    cams = [synth.camera(1, w, h, 90.0, 0, yaw=math.radians(a)) for a in (-25.0, 25.0)]
    gains = [0.97, 1.04]
    comp = ms.Compositor(n, (w, h), ms.PROJ_SPHERICAL, sc, num_bands=0, out_size=out)
    for i, (K, R) in enumerate(cams):
        comp.set_camera(i, K, R); comp.set_gain(i, gains[i])
    comp.build_maps(); comp.build_masks(0); comp.init_feather(0.02)
    pg = comp.pano_geom()
    assert pg.num_bands == 0
    s8, s16 = shapes(comp, *out)
    frames_np = [synth.frame(w, h, i, 1) for i in range(n)]
    frames = [to_dev(f) for f in frames_np]
    last, _ = run_layouts(lambda o8, o16: comp.stitch([frames], out8u=None if o8 is None else [o8], out16s=None if o16 is None else [o16]), s8, s16, "feather")
    corners = [comp.view_geom(i).roi.tuple()[:2] for i in range(n)]
    masks = [host(comp.mask(i)) for i in range(n)]
    warped = []
    for i in range(n):
        xm, ym = [host(m) for m in comp.maps(i)]
        warped.append(oracle.convert_scale_8u(oracle.remap_linear_8uc3(frames_np[i], xm, ym), gains[i]))
    ref16, _, roi = oracle.feather_blend(corners, warped, masks, 0.02)
    assert roi == pg.dst_roi_final.tuple()
    assert np.array_equal(host(last[1].view), ref16)
    assert np.array_equal(host(last[0].view), canvas_ref(ref16, pg, out[0], out[1], FILL8))
    comp.close()


def test_zero_band_kernel_on_pitched_offset_outputs(ms, cuda):
    """k_single_band with the plain mask weights: a multiband context created with num_bands = 0 (ms_init_blender allows it)."""
    cfg = synth.CONFIGS["mini4"]
    comp = ms.Compositor(cfg["n"], (cfg["w"], cfg["h"]), ms.PROJ_SPHERICAL, synth.warp_scale(cfg["out_w"]), num_bands=0, out_size=(cfg["out_w"], cfg["out_h"]))
    g = synth.gains(cfg["n"])
    for i in range(cfg["n"]):
        comp.set_camera(i, *synth.camera(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], i)); comp.set_gain(i, g[i])
    comp.build_maps(); comp.build_masks(1); comp.init_blender()
    assert comp.pano_geom().num_bands == 0
    s8, s16 = shapes(comp, cfg["out_w"], cfg["out_h"])
    frames = dev_frames(cfg, 3)
    _, want = run_layouts(lambda o8, o16: comp.stitch([frames], out8u=None if o8 is None else [o8], out16s=None if o16 is None else [o16]), s8, s16, "zero bands")
    assert int(want[1].abs().max()) > 7
    comp.close()


# ---- another layout for every frame of a call ------------------------------------------------------------------------------------------------------------------
def _singles(comp, cfg, sets, s8, s16):
    out = []
    for t in sets:
        w8, w16 = contiguous(s8, s16)
        comp.stitch([dev_frames(cfg, t)], out8u=[w8], out16s=[w16])
        out.append((w8, w16))
    torch.cuda.synchronize()
    assert not torch.equal(out[0][1], out[1][1])
    return out


def _check_batch(c8, c16, singles, n_sets, what):
    for f, (a, b) in enumerate(zip(c8, c16)):
        tag = "%s, frame %d" % (what, f)
        if a is not None:
            a.check_outside(tag + ": 8U canvas")
            same_pixels(a.view, singles[f % n_sets][0], tag + ": 8U canvas")
        if b is not None:
            b.check_outside(tag + ": 16S panorama")
            same_pixels(b.view, singles[f % n_sets][1], tag + ": 16S panorama")


@pytest.mark.parametrize("simple", [False, True], ids=["k_blend8", "k_blend"])
def test_every_frame_of_a_call_with_its_own_layout(ms, cuda, simple):
    """OutTable carries a pointer and a step PER FRAME.  Four frames in one call, four different (extra, offset) pairs per type, no 8U canvas for frame 1 and no 16S
    panorama for frame 2: every frame equals the same frame stitched alone into contiguous tensors.  A kernel that took frame 0's step for every frame fails here."""
    comp, cfg, _ = make_rig(ms, "mini6", max_frames=4, simple_kernels=simple)
    s8, s16 = shapes(comp, cfg["out_w"], cfg["out_h"])
    singles = _singles(comp, cfg, range(4), s8, s16)
    l8, l16 = [(pad512(s8[1] * 3), 1), (7, 5), (0, 2), (13, 3)], [(pad512(s16[1] * 6), 6), (2, 14), (10, 0), (0, 2)]
    size_step = max([s8[1] * 3 + e for e, _ in l8] + [s16[1] * 6 + e for e, _ in l16])
    c8 = [None if f == 1 else Canary(s8, torch.uint8, *l8[f], size_step, FILL8) for f in range(4)]
    c16 = [None if f == 2 else Canary(s16, torch.int16, *l16[f], size_step, FILL16) for f in range(4)]
    assert len({c.step for c in c8 if c}) == 3 and len({c.step for c in c16 if c}) == 3
    comp.stitch([dev_frames(cfg, t) for t in range(4)], out8u=[c.view if c else None for c in c8], out16s=[c.view if c else None for c in c16])
    torch.cuda.synchronize()
    _check_batch(c8, c16, singles, 4, "4 frames")
    comp.close()


@pytest.mark.parametrize("cpw", [False, True], ids=["plain", "cpw"])
def test_two_chunks_of_frames_with_their_own_layouts(ms, cuda, cpw):
    """33 frames of a max_frames = 64 context: the launches that read the frames go out as a chunk of 32 and a chunk of one, each with its own source table, while the
    band chain writes all 33 outputs from one OutTable.  Frame 0 and frame 32 (the first of the tail chunk) have layouts of their own, the rest a third one."""
    comp, cfg, _ = make_rig(ms, "mini6", max_frames=64, enable_cpw=cpw)
    if cpw:
        for i in range(cfg["n"]):
            r = comp.view_geom(i).roi
            comp.set_mesh(i, *synth.mesh(r.width, r.height, 9, 11, phase=0.3 * i, amp=5.0))
    s8, s16 = shapes(comp, cfg["out_w"], cfg["out_h"])
    n_sets, nf = 5, 33
    singles = _singles(comp, cfg, range(n_sets), s8, s16)

    def lay(f):
        return {0: ((13, 9), (10, 14)), 32: ((pad512(s8[1] * 3), 3), (pad512(s16[1] * 6), 6))}.get(f, ((1, 1), (2, 2)))
    size_step = max(max(s8[1] * 3 + lay(f)[0][0], s16[1] * 6 + lay(f)[1][0]) for f in range(nf))
    c8 = [Canary(s8, torch.uint8, *lay(f)[0], size_step, FILL8) for f in range(nf)]
    c16 = [Canary(s16, torch.int16, *lay(f)[1], size_step, FILL16) for f in range(nf)]
    comp.stitch([dev_frames(cfg, f % n_sets) for f in range(nf)], out8u=[c.view for c in c8], out16s=[c.view for c in c16])
    torch.cuda.synchronize()
    _check_batch(c8, c16, singles, n_sets, "33 frames")
    comp.close()


# ---- the other ways of reaching the writers --------------------------------------------------------------------------------------------------------------------
L8, L16 = (7, 5), (10, 6)       # one pitched, offset layout per type for the cases below: odd 8U step and start, 16S start 6 modulo 16


def _against_contiguous(call, s8, s16, what):
    w8, w16 = contiguous(s8, s16)
    call(w8, w16)
    size_step = max(s8[1] * 3 + L8[0], s16[1] * 6 + L16[0])
    c8, c16 = Canary(s8, torch.uint8, *L8, size_step, FILL8), Canary(s16, torch.int16, *L16, size_step, FILL16)
    call(c8.view, c16.view)
    torch.cuda.synchronize()
    c8.check_outside(what + ": 8U canvas"); c16.check_outside(what + ": 16S panorama")
    same_pixels(c8.view, w8, what + ": 8U canvas"); same_pixels(c16.view, w16, what + ": 16S panorama")
    assert int(w16.abs().max()) > 7 and bool((w8 != FILL8).any())
    return w8, w16


def test_feed_then_blend_into_pitched_outputs(ms, cuda):
    comp, cfg, _ = make_rig(ms, "mini6")
    frames = dev_frames(cfg, 4)

    def call(o8, o16):
        for i in range(cfg["n"]):
            comp.feed(i, frames[i])
        comp.blend(out8u=o8, out16s=o16)
    _against_contiguous(call, *shapes(comp, cfg["out_w"], cfg["out_h"]), "ms_feed + ms_blend")
    comp.close()


def test_stitch_nv12_into_pitched_outputs(ms, cuda):
    comp, cfg, _ = make_rig(ms, "mini6")
    nv = [to_dev(synth.nv12_frame(cfg["w"], cfg["h"], i)) for i in range(cfg["n"])]
    _against_contiguous(lambda o8, o16: comp.stitch_nv12([nv], out8u=[o8], out16s=[o16]), *shapes(comp, cfg["out_w"], cfg["out_h"]), "ms_stitch_nv12")
    assert comp.stitch_kernels()[0] == "nv12"
    comp.close()


def test_dropout_subset_into_pitched_outputs(ms, cuda):
    comp, cfg, _ = make_rig(ms, "mini6")
    active = ((1 << cfg["n"]) - 1) & ~(1 << 2)
    comp.set_active_views(active)
    frames = [t if (active >> i) & 1 else None for i, t in enumerate(dev_frames(cfg, 5))]
    _against_contiguous(lambda o8, o16: comp.stitch([frames], out8u=[o8], out16s=[o16]), *shapes(comp, cfg["out_w"], cfg["out_h"]), "views 0x%x" % active)
    comp.close()


def test_stitch_finish_into_pitched_outputs(ms, cuda):
    """ms_stitch_finish (the sink of two view shards) writes through the same level-0 kernels in their finish form"""
    comps, parts = [], []
    for k in range(2):
        c, cfg, _ = make_rig(ms, "mini6", shards=2, shard_index=k)
        lo, hi = k * cfg["n"] // 2, (k + 1) * cfg["n"] // 2
        part = torch.full((c.partial_bytes() // 2,), 12345, dtype=torch.int16, device=cuda)
        c.stitch_partial([[t if lo <= v < hi else None for v, t in enumerate(dev_frames(cfg, 1))]], part)
        comps.append(c); parts.append(part)
    s8, s16 = shapes(comps[0], cfg["out_w"], cfg["out_h"])
    w8, w16 = _against_contiguous(lambda o8, o16: comps[0].stitch_finish(1, parts, out8u=[o8], out16s=[o16]), s8, s16, "ms_stitch_finish")
    full, _, _ = make_rig(ms, "mini6")
    f8, f16 = contiguous(s8, s16)
    full.stitch([dev_frames(cfg, 1)], out8u=[f8], out16s=[f16])
    torch.cuda.synchronize()
    assert torch.equal(w8, f8) and torch.equal(w16, f16)
    for c in comps + [full]:
        c.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_column_shards_into_the_same_pitched_outputs(ms, cuda, shards):
    """Column shards write their windows one after the other into ONE pair of pitched outputs (and, the same calls, into one contiguous pair): after every shard the
    two agree bit for bit and the padding is intact; what a shard writes stays inside the band tiles its window touches (the columns beyond them keep what was
    there), and every window holds the unsharded frame's columns."""
    full, cfg, _ = make_rig(ms, "mini6")
    s8, s16 = shapes(full, cfg["out_w"], cfg["out_h"])
    frames = dev_frames(cfg, 6)
    f8, f16 = contiguous(s8, s16)
    full.stitch([frames], out8u=[f8], out16s=[f16])
    tw = full.plan_stats()["blend_tile"][0]
    w8, w16 = contiguous(s8, s16)
    size_step = max(s8[1] * 3 + L8[0], s16[1] * 6 + L16[0])
    c8, c16 = Canary(s8, torch.uint8, *L8, size_step, FILL8), Canary(s16, torch.int16, *L16, size_step, FILL16)
    for k in range(shards):
        c, _, _ = make_rig(ms, "mini6", col_shards=shards, col_shard_index=k)
        b, e = c.col_window()
        need = c.needed_views()
        mine = [t if (need >> v) & 1 else None for v, t in enumerate(frames)]
        before = c16.view.clone()
        c.stitch([mine], out8u=[w8], out16s=[w16])
        c.stitch([mine], out8u=[c8.view], out16s=[c16.view])
        torch.cuda.synchronize()
        tag = "column shard %d of %d" % (k, shards)
        c8.check_outside(tag + ": 8U canvas"); c16.check_outside(tag + ": 16S panorama")
        same_pixels(c8.view, w8, tag + ": 8U canvas"); same_pixels(c16.view, w16, tag + ": 16S panorama")
        assert torch.equal(c16.view[:, b:e], f16[:, b:e]), tag
        lo, hi = b // tw * tw, _round_up(e, tw)
        assert torch.equal(c16.view[:, :lo], before[:, :lo]) and torch.equal(c16.view[:, hi:], before[:, hi:]), tag + " wrote beyond the tiles of its window"
        c.close()
    full.close()


# ---- I420 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_i420_slab_at_odd_addresses_and_the_pitched_slab_refused(ms, cuda):
    """ms_stitch_i420 writes the planes of one contiguous slab: a slab with step != out_width is refused (MS_ERR_INVALID) and keeps its bytes; a contiguous slab 1 / 2 / 3
    bytes into a guard-banded buffer gets the bytes of the aligned call (the 8-byte Y and 4-byte chroma stores then sit at every address modulo 4)."""
    comp, cfg, _ = make_rig(ms, "mini6")
    frames = dev_frames(cfg, 2)
    black = comp.new_i420(1)[0]
    want = black.clone()
    comp.stitch_i420([frames], [want])
    torch.cuda.synchronize()
    assert not torch.equal(want, black)
    shape = tuple(black.shape)
    for off in (1, 2, 3):
        c = Canary(shape, torch.uint8, 0, off, 0, black)
        comp.stitch_i420([frames], [c.view])
        torch.cuda.synchronize()
        same_pixels(c.view, want, "I420 slab %d bytes in" % off)
        c.check_outside("I420 slab %d bytes in" % off)
    c = Canary(shape, torch.uint8, 8, 0, 0, None)
    with pytest.raises(ms.MsError, match=r"error -1: ms_stitch_i420: out\[0\] must be a contiguous"):
        comp.stitch_i420([frames], [c.view])
    torch.cuda.synchronize()
    assert pattern_intact(c.bytes)
    comp.close()


# ---- the step rule of include/ms_stitch.h: refused on the host, nothing enqueued -------------------------------------------------------------------------------
def _raw_stitch(ms, comp, views, o8, o16, nv12=False):
    """ms_stitch over hand-made descriptor tables -> (status, message)"""
    fn = ms.load().ms_stitch_nv12 if nv12 else ms.load().ms_stitch
    rc = fn(comp._ctx, 1, views, o8, o16, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, ms.load().ms_last_error().decode()


_REFUSALS = [
    ("out8u", "short", r"ms_stitch: out8u\[0\] has row step 1917, below the 1920 bytes of its rows"),
    ("out16s", "short", r"ms_stitch: out16s\[0\] has row step 3832, below the 3834 bytes of its rows"),
    ("out16s", "odd_step", r"ms_stitch: out16s\[0\] needs 2-byte alignment"),
    ("out16s", "odd_data", r"ms_stitch: out16s\[0\] needs 2-byte alignment"),
    ("view", "short", r"ms_stitch: view\[3\] has row step 957, below the 960 bytes of its rows"),
]


# (ms_stitch_nv12 exists on the tiled path only: test_nv12_direct_is_refused_where_it_does_not_apply)
@pytest.mark.parametrize("which,step,msg,simple", [pytest.param(*r, s, id="%s-%s-%s" % (r[0], r[1], "simple" if s else "tiled")) for s in (False, True) for r in _REFUSALS] +
                         [pytest.param("nv12", "short", r"ms_stitch_nv12: view\[3\] has row step 319, below the 320 bytes of its rows", False, id="nv12-short-tiled")])
def test_bad_steps_are_refused_before_anything_runs(ms, cuda, which, step, msg, simple):
    """A step below the row's bytes (outputs and source views), an odd step or an odd address of a 16S output: MS_ERR_INVALID with a message that names the image, and
    neither output buffer touched.  The buffers are real and fully sized."""
    import re
    comp, cfg, _ = make_rig(ms, "mini6", simple_kernels=simple)
    s8, s16 = shapes(comp, cfg["out_w"], cfg["out_h"])
    c8, c16 = Canary(s8, torch.uint8, 0, 0, 0, None), Canary(s16, torch.int16, 2, 0, 0, None)
    if which == "nv12":
        frames = [to_dev(synth.nv12_frame(cfg["w"], cfg["h"], i)) for i in range(cfg["n"])]
    else:
        frames = dev_frames(cfg, 0)
    n, views, o8, o16 = comp._tables([frames], [c8.view], [c16.view])
    if which == "out8u":
        o8[0].step -= 3
    elif which == "out16s":
        if step == "short":
            o16[0].step = s16[1] * 6 - 2
        elif step == "odd_step":
            o16[0].step += 1
        else:
            o16[0].data += 1
    else:
        views[3].step -= 3 if which == "view" else 1
    rc, err = _raw_stitch(ms, comp, views, o8, o16, nv12=which == "nv12")
    torch.cuda.synchronize()
    assert rc == -1 and re.search(msg, err), (rc, err)
    assert pattern_intact(c8.bytes) and pattern_intact(c16.bytes)
    comp.close()


def test_a_short_step_fed_through_ms_feed_is_refused_by_ms_blend(ms, cuda):
    comp, cfg, _ = make_rig(ms, "mini6")
    frames = dev_frames(cfg, 0)
    s8, s16 = shapes(comp, cfg["out_w"], cfg["out_h"])
    c16 = Canary(s16, torch.int16, 0, 0, 0, None)
    for i in range(cfg["n"]):
        im = ms.img(frames[i])
        if i == 1:
            im.step -= 1
        assert ms.load().ms_feed(comp._ctx, i, C.byref(im), None) == 0
    with pytest.raises(ms.MsError, match=r"error -1: ms_stitch: view\[1\] has row step 959"):
        comp.blend(out16s=c16.view)
    torch.cuda.synchronize()
    assert pattern_intact(c16.bytes)
    comp.close()


@pytest.mark.parametrize("which", ["out16s", "out8u", "view"])
def test_a_step_of_16_mib_is_refused(ms, cuda, which):
    """step = 2^24 exactly: k_blend8's 24-bit multiply would put every row on row 0.  Refused with MS_ERR_INVALID; the buffer spans rows * 2^24 bytes, so even an
    unchecked call would stay inside it."""
    import re
    comp, cfg, _ = make_rig(ms, "mini6" if which == "out16s" else "mini4")
    s8, s16 = shapes(comp, cfg["out_w"], cfg["out_h"])
    step = 1 << 24
    rows = {"out16s": s16[0], "out8u": s8[0], "view": cfg["h"]}[which]
    flat, b = pattern_buffer(rows * step, torch.int16 if which == "out16s" else torch.uint8)
    frames = dev_frames(cfg, 0)
    c8, c16 = Canary(s8, torch.uint8, 0, 0, 0, None), Canary(s16, torch.int16, 0, 0, 0, None)
    n, views, o8, o16 = comp._tables([frames], [c8.view], [c16.view])
    tab = {"out16s": o16[0], "out8u": o8[0], "view": views[1]}[which]
    tab.data, tab.step = flat.data_ptr(), step
    rc, err = _raw_stitch(ms, comp, views, o8, o16)
    torch.cuda.synchronize()
    name = {"out16s": r"out16s\[0\]", "out8u": r"out8u\[0\]", "view": r"view\[1\]"}[which]
    assert rc == -1 and re.search(name + r" has row step 16777216: the row step must be below 2\^24 bytes", err), (rc, err)
    assert pattern_intact(b) and pattern_intact(c8.bytes) and pattern_intact(c16.bytes)
    comp.close()
    del flat, b
    torch.cuda.empty_cache()
