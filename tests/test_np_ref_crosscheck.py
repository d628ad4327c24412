"""The C oracle against tests/np_ref.py for every oracle kernel the GPU suite trusts beyond the pyramids / remap / blender checked in
test_oracle_crosscheck.py: bit for bit at the shapes (1 x 1, 1 x N, N x 1, 2 x 2, odd, prime, every width mod 8) and values (full ranges,
NaN / inf where the operation defines them) where kernels go wrong.  The warp maps, where the oracle is fp32, are held to a float64
statement of the same map instead; the colour conversions are additionally held to a float64 BT.601 statement."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest

import calib_cases
import np_ref
import synth

F32 = np.float32
SHAPES = [(1, 1), (1, 13), (17, 1), (2, 2), (3, 5), (7, 11), (31, 37), (64, 64), (9, 65)] + [(5, 8 * 3 + r) for r in range(1, 10)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]


def rng_for(*k):
    return np.random.default_rng(abs(hash(k)) % (2 ** 32))


def test_fmaf32_is_the_correctly_rounded_fma():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = rng_for("fma")
    n = 20000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(F32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(F32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.standard_normal(n) * 1e-7)).astype(F32)        # near-cancellation: the hard cases
    c[::3] = (rng.standard_normal(n // 3 + 1) * 1e3).astype(F32)[:len(c[::3])]
    got = np_ref.fmaf32(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got, want)
    sp = np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, 1e-45, 3e38], F32)
    A, B, C = [x.ravel() for x in np.meshgrid(sp, sp, sp)]
    got = np_ref.fmaf32(A, B, C)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(A, B, C)], F32)
    assert np.array_equal(got, want, equal_nan=True)


# ---- weight pyramid (K22) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_pyr_down_32f(oracle, shape):
    rng = rng_for("pd32", shape)
    w = rng.random(shape, dtype=np.float32)
    w[rng.random(shape) < 0.3] = 0.0
    w[rng.random(shape) < 0.2] = 1.0
    assert np.array_equal(oracle.pyr_down_32f(w), np_ref.pyr_down_32f(w))
    wild = (rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 30, shape)).astype(F32)
    wild[rng.random(shape) < 0.05] = np.nan
    wild[rng.random(shape) < 0.05] = np.inf
    wild[rng.random(shape) < 0.05] = -np.inf
    assert np.array_equal(oracle.pyr_down_32f(wild), np_ref.pyr_down_32f(wild), equal_nan=True)


def test_pyr_down_32f_chain_of_levels(oracle):
    """The weight pyramid of a mask, level after level, as MultiBandBlender builds it (blenders.cpp:412-423)."""
    m = np.zeros((97, 141), np.uint8)
    m[10:80, 20:130] = 255
    m[40:50, 60:70] = 0
    a = b = np_ref.convert_8u_32f_scale(m, 1.0 / 255.0)
    for _ in range(6):
        a, b = oracle.pyr_down_32f(a), np_ref.pyr_down_32f(b)
        assert np.array_equal(a, b)


# ---- resize (K2) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 13), (17, 1), (2, 2), (7, 11), (113, 157), (31, 37)], ids=str)
@pytest.mark.parametrize("scale", [0.5, 0.3, 1.0 / 3.0, 1.0, 2.0, 2.5])
def test_resize_linear_8u(oracle, shape, scale):
    rng = rng_for("rs", shape, scale)
    for cn in (1, 3):
        src = rng.integers(0, 256, size=shape + ((3,) if cn == 3 else ()), dtype=np.uint8)
        src.reshape(-1)[::7] = 255
        src.reshape(-1)[3::11] = 0
        dw, dh = int(np.rint(shape[1] * scale)), int(np.rint(shape[0] * scale))
        if dw == 0 or dh == 0:
            continue
        got = oracle.resize_linear_8u(src, fx=scale, fy=scale)
        assert got.shape[:2] == (dh, dw)
        assert np.array_equal(got, np_ref.resize_linear_8u(src, fx=scale, fy=scale))


@pytest.mark.parametrize("dsize", [(1, 1), (1, 40), (40, 1), (3, 2), (157, 113), (400, 9), (1578, 887)])
def test_resize_linear_8u_to_a_size(oracle, dsize):
    rng = rng_for("rsz", dsize)
    src = rng.integers(0, 256, size=(113, 157, 3), dtype=np.uint8)
    assert np.array_equal(oracle.resize_linear_8u(src, dsize=dsize), np_ref.resize_linear_8u(src, dsize=dsize))


# ---- colour conversions ----------------------------------------------------------------------------------------------------------------
def _nv12(h, w, rng):
    return rng.integers(0, 256, size=(h * 3 // 2, w), dtype=np.uint8)


@pytest.mark.parametrize("hw", [(2, 2), (2, 18), (18, 2), (6, 10), (34, 50), (58, 98), (2, 2 * 256)], ids=str)
def test_nv12_to_bgr(oracle, hw):
    src = _nv12(*hw, rng_for("nv12", hw))
    assert np.array_equal(oracle.nv12_to_bgr(src), np_ref.nv12_to_bgr(src))


def test_nv12_to_bgr_every_chroma_pair_and_the_float_bt601_statement(oracle):
    """All 65 536 (U, V) pairs, Y at the ends of the studio range and beyond it; the invoker equals np_ref exactly and stays within 1 of the
    float64 BT.601 inverse -- which ties CY, CUB, CUG, CVG, CVR, the U / V order and the 2 x 2 chroma siting to the standard."""
    U, V = np.meshgrid(np.arange(256), np.arange(256))
    for yv in (0, 15, 16, 17, 100, 235, 236, 255):
        h, w = 2 * 256, 2 * 256
        Y = np.full((h, w), yv, np.uint8)
        Y[1::2, 1::2] = (yv + 37) % 256                           # the four pixels of a block differ: the chroma must still be shared
        uv = np.empty((h // 2, w), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = U, V
        src = np.vstack([Y, uv])
        got = oracle.nv12_to_bgr(src)
        assert np.array_equal(got, np_ref.nv12_to_bgr(src))
        uu = np.repeat(np.repeat(U, 2, 0), 2, 1)
        vv = np.repeat(np.repeat(V, 2, 0), 2, 1)
        ref = np.clip(np.rint(np_ref.bt601_yuv_to_bgr_f64(Y, uu, vv)), 0, 255)
        assert np.abs(got.astype(int) - ref).max() <= 1


@pytest.mark.parametrize("hw", [(2, 2), (2, 18), (18, 2), (6, 10), (34, 50), (58, 98)], ids=str)
def test_bgr_to_i420(oracle, hw):
    rng = rng_for("i420", hw)
    src = rng.integers(0, 256, size=hw + (3,), dtype=np.uint8)
    src[0, 0] = (0, 0, 0)
    src[-1, -1] = (255, 255, 255)
    assert np.array_equal(oracle.bgr_to_i420(src), np_ref.bgr_to_i420(src))


def test_bgr_to_i420_within_one_of_the_float_bt601_statement(oracle):
    """A 2-px-per-block image whose top-left pixels run through a 64^3 lattice of BGR (ends included) and whose other three pixels are noise:
    Y of every pixel and U / V of every block's top-left pixel within 1 of float64 BT.601."""
    rng = rng_for("i420f")
    lv = np.round(np.linspace(0, 255, 64)).astype(np.uint8)
    B, G, R = [a.ravel() for a in np.meshgrid(lv, lv, lv, indexing="ij")]
    h, w = 2 * 256, 2 * 1024
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[0::2, 0::2] = np.stack([B, G, R], -1).reshape(256, 1024, 3)
    got = oracle.bgr_to_i420(img)
    assert np.array_equal(got, np_ref.bgr_to_i420(img))
    y, cb, cr = np_ref.bt601_bgr_to_yuv_f64(img)
    assert np.abs(got[:h].astype(int) - np.clip(np.rint(y), 0, 255)).max() <= 1
    plane = h // 2 * w // 2
    gu = got.reshape(-1)[h * w:h * w + plane].reshape(h // 2, w // 2).astype(int)
    gv = got.reshape(-1)[h * w + plane:].reshape(h // 2, w // 2).astype(int)
    assert np.abs(gu - np.clip(np.rint(cb[0::2, 0::2]), 0, 255)).max() <= 1
    assert np.abs(gv - np.clip(np.rint(cr[0::2, 0::2]), 0, 255)).max() <= 1


# ---- CPW: custom_resize (K19) and convertMeshesToMap ----------------------------------------------------------------------------------
@pytest.mark.parametrize("src_shape,t", [((2, 2), (1, 1)), ((2, 2), (5, 3)), ((2, 3000), (3000, 2)), ((10, 10), (1239, 886)), ((40, 40), (1240, 1100)),
                                         ((11, 9), (61, 47)), ((3, 7), (7, 3)), ((5, 5), (1, 9)), ((40, 40), (40, 40))], ids=str)
def test_custom_resize_32f(oracle, src_shape, t):
    rng = rng_for("cr", src_shape, t)
    src = (rng.standard_normal(src_shape) * 300).astype(F32)
    assert np.array_equal(oracle.custom_resize_32f(src, *t), np_ref.custom_resize_32f(src, *t))
    src[rng.random(src_shape) < 0.1] = np.nan                                 # holes propagate to every output that taps them
    src.reshape(-1)[0] = np.inf
    assert np.array_equal(oracle.custom_resize_32f(src, *t), np_ref.custom_resize_32f(src, *t), equal_nan=True)


@pytest.mark.parametrize("nm,wh", [((10, 10), (123, 97)), ((40, 40), (241, 180)), ((9, 11), (64, 48)), ((2, 2), (8, 6)), ((6, 5), (33, 17))], ids=str)
def test_convert_mesh_to_map(oracle, nm, wh):
    rng = rng_for("mesh", nm, wh)
    mx, my = synth.mesh(wh[0], wh[1], nm[0], nm[1], phase=0.7, amp=5.0)
    mx = (mx - 1.5 + rng.uniform(-0.5, 0.5, mx.shape)).astype(F32)            # vertices at negative coordinates: C truncation puts (-2, 0) in cell 0
    my = (my * 0.8 - 0.9).astype(F32)                                          # squeezed: empty cells (NaN holes) at the bottom
    a = oracle.convert_mesh_to_map(mx, my, *wh)
    b = np_ref.convert_mesh_to_map(mx, my, *wh)
    assert np.isnan(a[0]).any()
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    mx[1, 1] = np.nan                                                          # a hole in the mesh itself
    for x, y in zip(oracle.convert_mesh_to_map(mx, my, *wh), np_ref.convert_mesh_to_map(mx, my, *wh)):
        assert np.array_equal(x, y, equal_nan=True)


def _shipped_rois():
    import msstitch as ms
    cfg = synth.CONFIGS["cfg2"]
    rig = ms.calibrate_cameras(cfg["n"], cfg["w"], cfg["h"], cfg["hfov_deg"], 0.6, 0.01, 1.4)
    return [ms.warp_roi(ms.PROJ_CYLINDRICAL, rig["K_compose"][i], rig["R"][i], rig["compose_warp_scale"], rig["compose_width"], rig["compose_height"])
            for i in range(cfg["n"])]


def _config_rois(oracle):
    out = []
    for name in ("cfg2", "cfg5"):                                              # cfg3 composites cfg2's geometry
        c = synth.CONFIGS[name]
        for i in range(c["n"]):
            K, R = synth.camera(c["n"], c["w"], c["h"], c["hfov_deg"], i)
            out.append(oracle.warp_roi(2, K, R, synth.warp_scale(c["out_w"]), c["w"], c["h"]))
    return out + _shipped_rois()


def test_resize_axis_exact_float_quotient_is_the_integer_quotient(oracle):
    """mesh_maps.hip resize_axis_exact: while t * (n - 1) < 2^23, (int)((float)x * (float)(n - 1) / (float)t) == x * (n - 1) / t for every
    0 <= x < t.  numpy's fp32 division is correctly rounded, as the build's is (-fhip-fp32-correctly-rounded-divide-sqrt).  Exhaustive over x for
    every (n, t) of the shipped configurations (10 x 10 and 40 x 40 meshes to every ROI size, then the half-resolution cell means back to it),
    then random pairs up to the boundary."""
    pairs = set()
    for r in _config_rois(oracle):
        for t in (r[2], r[3]):
            pairs |= {(10, t), (40, t), (t // 2, t)}

    def check(n, t, x):
        q = (x.astype(F32) * F32(n - 1)).astype(F32) / F32(t)
        return np.array_equal(q.astype(np.int64), (x * (n - 1)) // t)
    shortcut = 0
    for n, t in sorted(pairs):
        if t * (n - 1) < 2 ** 23:
            shortcut += 1
            assert check(n, t, np.arange(t, dtype=np.int64)), (n, t)
    assert shortcut >= 20
    rng = rng_for("axis")
    for _ in range(300):
        t = int(rng.integers(2, 2 ** 22))
        n = int(min((2 ** 23 - 1) // t + 1, 2 ** 22))
        n = int(rng.integers(max(2, n // 2), n + 1))
        if t * (n - 1) >= 2 ** 23:
            continue
        x = np.unique(np.concatenate([rng.integers(0, t, 4000), np.arange(max(0, t - 50), t), (np.arange(1, 200) * t) // max(n - 1, 1)]))
        x = x[(x >= 0) & (x < t)].astype(np.int64)
        assert check(n, t, x), (n, t)


# ---- masks and seams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_remap_nearest_8uc1(oracle, shape):
    rng = rng_for("nn", shape)
    src = rng.integers(0, 256, size=(23, 29), dtype=np.uint8)
    mx = rng.uniform(-3, 32, size=shape).astype(F32)
    my = rng.uniform(-3, 26, size=shape).astype(F32)
    wild = rng.random(shape) < 0.2
    vals = np.array([np.nan, np.inf, -np.inf, 1e20, -1e20, -1.0, -0.999, -0.0, 0.0, 28.999, 29.0, 22.5, 23.0, 3e9, -3e9], F32)
    mx[wild] = rng.choice(vals, size=int(wild.sum()))
    wy = rng.random(shape) < 0.2
    my[wy] = rng.choice(vals, size=int(wy.sum()))
    assert np.array_equal(oracle.remap_nearest_8uc1(src, mx, my), np_ref.remap_nearest_8uc1(src, mx, my))


def test_remap_nearest_8uc1_every_special_coordinate(oracle):
    vals = np.array([np.nan, np.inf, -np.inf, 1e20, -1e20, -1.0, -0.999, -0.0, 0.0, 0.5, 28.999, 29.0, 22.5, 23.0, 3e9, -3e9], F32)
    mx, my = [a.astype(F32) for a in np.meshgrid(vals, vals)]
    src = np.arange(23 * 29, dtype=np.int64).reshape(23, 29).astype(np.uint8) | 1
    assert np.array_equal(oracle.remap_nearest_8uc1(src, mx, my), np_ref.remap_nearest_8uc1(src, mx, my))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_converts_border_and_dilate(oracle, shape):
    rng = rng_for("cv", shape)
    a8 = rng.integers(0, 256, size=shape, dtype=np.uint8)
    a8.reshape(-1)[::5] = 255
    a8.reshape(-1)[1::5] = 0
    for alpha in (0.0, 0.5, 0.98, 1.0, 1.0 + 1e-7, 1.02, 1.5, 3.7, 1.0 / 255.0):
        assert np.array_equal(oracle.convert_scale_8u(a8, alpha), np_ref.convert_scale_8u(a8, alpha)), alpha
        assert np.array_equal(oracle.convert_8u_32f_scale(a8, alpha), np_ref.convert_8u_32f_scale(a8, alpha)), alpha
    a3 = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    assert np.array_equal(oracle.convert_scale_8u(a3, 1.03), np_ref.convert_scale_8u(a3, 1.03))
    s16 = rng.integers(-32768, 32768, size=shape, dtype=np.int16)
    s16.reshape(-1)[:4] = [-32768, 32767, 255, 256][:s16.size]
    assert np.array_equal(oracle.convert_16s_8u(s16), np_ref.convert_16s_8u(s16))
    f = rng.standard_normal(shape).astype(F32)
    f.reshape(-1)[::4] = np.nan
    f.reshape(-1)[1::4] = -np.inf
    for pad in ((0, 0, 0, 0), (1, 2, 3, 4), (5, 0, 0, 7)):
        assert np.array_equal(oracle.copy_make_border_const_32f(f, *pad), np_ref.copy_make_border_const_32f(f, *pad), equal_nan=True)
    m = (rng.random(shape) < 0.1).astype(np.uint8) * rng.integers(1, 256, size=shape, dtype=np.uint8)
    assert np.array_equal(oracle.dilate3x3_8u(m), np_ref.dilate3x3_8u(m))
    assert np.array_equal(oracle.dilate3x3_8u(a8), np_ref.dilate3x3_8u(a8))


def test_convert_scale_8u_every_value_and_gain(oracle):
    a = np.tile(np.arange(256, dtype=np.uint8), (64, 1))
    for g in np.concatenate([np.linspace(0.5, 1.5, 61), [255.0 / 254.5, 2.0, 254.5 / 255.0, 0.1 + 1e-9]]):
        assert np.array_equal(oracle.convert_scale_8u(a, g), np_ref.convert_scale_8u(a, g)), g


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_add_src_weight_16s_and_normalize_16s(oracle, shape):
    """The 16S-weight blender's accumulate and normalise (multiband_blend.cu:10-24, 62-74) over the full int16 range, incl. the wrap of the
    short sums, weights of the fixed-point range 0..256 and beyond it; normalise with w != 0 (w == 0 is undefined in the reference)."""
    rng = rng_for("16s", shape)
    for wlo, whi in ((0, 257), (-32768, 32768)):
        src = rng.integers(-32768, 32768, size=shape + (3,), dtype=np.int16)
        src.reshape(-1)[:2] = [-32768, 32767][:src.size]
        w = rng.integers(wlo, whi, size=shape, dtype=np.int16)
        d1 = rng.integers(-32768, 32768, size=shape + (3,), dtype=np.int16)
        dw1 = rng.integers(-32768, 32768, size=shape, dtype=np.int16)
        d2, dw2 = d1.copy(), dw1.copy()
        oracle.add_src_weight_16s(src, w, d1, dw1)
        np_ref.add_src_weight_16s(src, w, d2, dw2)
        assert np.array_equal(d1, d2) and np.array_equal(dw1, dw2)
        nz = np.where(dw1 == 0, np.int16(1), dw1)
        oracle.normalize_16s(nz, d1)
        np_ref.normalize_16s(nz, d2)
        assert np.array_equal(d1, d2)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_distance_transform_l1(oracle, shape):
    rng = rng_for("dt", shape)
    for p in (0.02, 0.3, 0.9):
        m = (rng.random(shape) > p).astype(np.uint8) * 255
        m.reshape(-1)[int(rng.integers(0, m.size))] = 0
        assert np.array_equal(oracle.distance_transform_l1(m), np_ref.distance_transform_l1(m))
    full = np.full(shape, 7, np.uint8)                                         # no zero pixel: "infinity", farther than any real distance
    assert (oracle.distance_transform_l1(full) > sum(shape)).all() and np.isinf(np_ref.distance_transform_l1(full)).all()


def test_voronoi_seams(oracle):
    rng = rng_for("voronoi")
    for trial in range(4):
        n = 3 + trial % 2
        corners, masks = [], []
        for i in range(n):
            h, w = int(rng.integers(15, 40)), int(rng.integers(15, 45))
            corners.append((int(rng.integers(-5, 40)), int(rng.integers(-10, 20))))
            m = np.full((h, w), 255, np.uint8)
            m[rng.random((h, w)) < 0.05] = 0
            m[:, :int(rng.integers(0, 4))] = 0
            masks.append(m)
        a = oracle.voronoi_seams(corners, [m.copy() for m in masks])
        b = np_ref.voronoi_seams(corners, [m.copy() for m in masks])
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert any(not np.array_equal(x, m) for x, m in zip(a, masks)), "the seams cut nothing: the case is vacuous"


# ---- the per-op calibration tests' own inputs (tests/calib_cases.py): the two references agree on every case tests/test_calib_kernels_gpu.py runs -----------
@pytest.mark.parametrize("name", calib_cases.VORONOI_CASES)
def test_voronoi_seams_on_the_gpu_tests_inputs(oracle, name):
    rois, masks = calib_cases.voronoi_case(name)
    corners = [r[:2] for r in rois]
    a = oracle.voronoi_seams(corners, [m.copy() for m in masks])
    b = np_ref.voronoi_seams(corners, [m.copy() for m in masks])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    changed = any(not np.array_equal(x, m) for x, m in zip(a, masks))
    assert changed == (name not in calib_cases.VORONOI_UNTOUCHED), "the case does not do what its name says"
    if len(rois) == 2 and changed:                      # what is left of the overlap belongs to one view only
        ox, oy, ow, oh = calib_cases.overlap(*rois)
        s0, s1 = [m[oy - r[1]:oy - r[1] + oh, ox - r[0]:ox - r[0] + ow] for m, r in zip(a, rois)]
        assert not ((s0 != 0) & (s1 != 0)).any()
    if name == "nounique_both":                         # neither view has a pixel of its own: dist1 == dist2 everywhere, `<` is false, view i loses the overlap
        assert not a[0].any() and np.array_equal(a[1], masks[1])
    if name == "nounique_first":
        assert not a[0].any() and np.array_equal(a[1], masks[1])
    if name == "nounique_second":
        assert not a[1].any() and np.array_equal(a[0], masks[0])
    if name == "ties_columns":                          # overlap columns 25..39 of view 0: the middle one (32) is a tie and stays with view 1
        assert a[0][:, :32].all() and not a[0][:, 32:].any() and not a[1][:, :7].any() and a[1][:, 7:].all()
    if name == "ties_none_even":
        assert a[0][:, :32].all() and not a[0][:, 32:].any() and not a[1][:, :8].any() and a[1][:, 8:].all()


def test_voronoi_cases_cover_the_block_boundaries():
    """rw + 2 gap and rh + 2 gap take 21, 63, 64, 65, 128 and 129 among the two-view cases: either side of the 64-lane blocks of k_vor_cols / k_vor_rows"""
    seen_w, seen_h = set(), set()
    for name in calib_cases.VORONOI_CASES:
        rois, _ = calib_cases.voronoi_case(name)
        if name.startswith("pair_"):
            o = calib_cases.overlap(*rois)
            seen_w.add(o[2] + 2 * calib_cases.GAP); seen_h.add(o[3] + 2 * calib_cases.GAP)
            assert min(r[0] for r in rois) < 0 or min(r[1] for r in rois) < 0 or name == "pair_1x1"
    assert seen_w >= {21, 63, 64, 65, 128, 129} and seen_h >= {21, 63, 64, 65, 128, 129}


@pytest.mark.parametrize("name", calib_cases.GAIN_CASES)
def test_gain_compensator_on_the_gpu_tests_inputs(oracle, name):
    """oracle.gain_compensator == np_ref.gain_compensator, bit for bit, and np_ref's solve against numpy.linalg.solve as a sanity net under
    rtol = 64 cond(A) 2^-52 (64: room for the growth of n <= 16 elimination steps) -- the bound does not pin anything, the equality does."""
    rois, imgs, masks = calib_cases.gain_case(name)
    corners = [r[:2] for r in rois]
    g, N, I, swaps = np_ref.gain_compensator(corners, imgs, masks)
    ref = np.array(oracle.gain_compensator(corners, imgs, masks), np.float64)
    assert np.array_equal(g, ref), (name, g, ref)
    A, b = np_ref.gain_normal_equations(N, I)
    A, b = np.array(A), np.array(b)
    rtol = 64 * np.linalg.cond(A) * 2.0 ** -52
    np.testing.assert_allclose(g, np.linalg.solve(A, b), rtol=rtol, atol=0)
    n = len(rois)
    for i in range(n):
        for j in range(n):
            assert (N[i, j] == 0) == (calib_cases.overlap(rois[i], rois[j]) is None)
    assert (swaps > 0) == (name in calib_cases.GAIN_ROW_SWAP_CASES), "row exchanges: %d" % swaps
    if name == "no_common_255":
        assert N[0, 1] == 1 and I[0, 1] == 0.0 and I[1, 0] == 0.0 and N[0, 2] > 100 and N[1, 2] > 100
    if name == "views_1":
        assert g[0] == 1.0
    if n >= 2:
        assert len(set(g.tolist())) == n, "the views' exposures differ: so must their gains"


def test_gain_cases_cover_what_they_claim():
    ns = set()
    grey = 0
    for name in calib_cases.GAIN_CASES:
        rois, imgs, masks = calib_cases.gain_case(name)
        ns.add(len(rois))
        assert min(r[0] for r in rois) < 0 and min(r[1] for r in rois) < 0
        assert all((im == 0).all(axis=2).any() and (im == 255).all(axis=2).any() for im in imgs) or name == "lu_row_exchange"
        if len(rois) >= 2:              # sqrt(0) and sqrt(3 * 255^2) enter a pair sum: such pixels lie in an overlap, under 255 in both masks
            black, white = calib_cases.counted_extremes(rois, imgs, masks)
            assert black >= 10 and white >= 10, (name, black, white)
        grey += sum(int(((m == 254) | (m == 128)).sum()) for m in masks)
    assert ns >= {1, 2, 3, 4, 5, 8, 9, 16} and grey > 100


def test_solve_lu64_branches():
    """np_ref.solve_lu64 alone: every closed form against the LU path run on the same system (they differ in the last bits, not in the answer), the singular
    exits, and a permutation matrix that needs n - 1 exchanges."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 3):
        A = rng.uniform(-1, 1, (n, n)) + 3 * np.eye(n)
        b = rng.uniform(-1, 1, n)
        x, swaps = np_ref.solve_lu64(A.tolist(), b.tolist())
        np.testing.assert_allclose(x, np.linalg.solve(A, b), rtol=64 * np.linalg.cond(A) * 2.0 ** -52)
        assert swaps == 0 and np_ref.solve_lu64(np.zeros((n, n)).tolist(), b.tolist())[0] is None
    P = np.roll(np.eye(5), 1, axis=0) * 2.0
    x, swaps = np_ref.solve_lu64(P.tolist(), [2.0, 4.0, 6.0, 8.0, 10.0])
    assert swaps == 4 and x == [2.0, 3.0, 4.0, 5.0, 1.0]
    assert np_ref.solve_lu64(np.ones((4, 4)).tolist(), [1.0] * 4)[0] is None


# ---- warp maps (K18) against float64 truth ----------------------------------------------------------------------------------------------
def map_bounds(truth, k_rinv, w, h):
    """Per-coordinate error bounds of an fp32 evaluation of the backward map against its float64 truth: 1e-3 px where the point lands within
    2 px of the source image, relative 1e-4 elsewhere -- but never below the first-order rounding error of the fp32 formula itself,
    2^-21 (|k_row| + |c| |k_z|) / |z| (numerator and denominator are sums of terms of size |k|; as z -> 0 their rounding dominates).  Pixels with
    |z| < 1e-6 (the z <= 0 -> (-1, -1) discontinuity of the reference) get no bound: only the integer consequence is asserted there."""
    x, y, z = truth
    k = np.abs(np.asarray(k_rinv, np.float64).reshape(9))
    with np.errstate(invalid="ignore", divide="ignore"):
        near = (x >= -2) & (x <= w + 1) & (y >= -2) & (y <= h + 1)
        tol = []
        for c, row in ((x, k[0:3]), (y, k[3:6])):
            cond = 2.0 ** -21 * (row.sum() + np.abs(c) * k[6:9].sum()) / np.abs(z)
            tol.append(np.where(np.abs(z) < 1e-6, np.inf, np.maximum(np.where(near, 1e-3, 1e-4 * np.abs(c)), cond)))
    return near, tol[0], tol[1]


def map_errors(mx, my, truth, k_rinv, w, h):
    """(max |map - f64| where the point lands within 2 px of the source image, max of |map - f64| / bound over all pixels, the number of pixels
    where floor(map) or the nearest-neighbour valid mask differ from the f64 ones although the f64 coordinates are farther than the bound from an
    integer -- the image border included)."""
    x, y, _ = truth
    near, tx, ty = map_bounds(truth, k_rinv, w, h)
    with np.errstate(invalid="ignore", divide="ignore"):
        ex, ey = np.abs(mx - x), np.abs(my - y)
        e_near = float(np.maximum(ex, ey)[near & np.isfinite(tx)].max(initial=0))
        ratio = float(np.nan_to_num(np.maximum(ex / tx, ey / ty), nan=np.inf).max(initial=0))
        clear = np.isfinite(x) & np.isfinite(y) & (np.abs(x - np.rint(x)) > tx) & (np.abs(y - np.rint(y)) > ty)
        fl = (np.floor(mx) != np.floor(x)) | (np.floor(my) != np.floor(y))
        one = np.full((h, w), 255, np.uint8)
        vm = np_ref.remap_nearest_8uc1(one, mx, my) != np_ref.remap_nearest_8uc1(one, x, y)
    return e_near, ratio, int((clear & (fl | vm)).sum())


def warp_cases(oracle):
    """(name, proj, tl_u, tl_v, rows, cols, k_rinv, scale, src w, h): every view ROI of the hot-path rig and a small-focal rig per projection,
    a spherical view straddling the u wrap, strips at both poles, and a plane ROI wide enough that z crosses 0."""
    cases = []
    for rig, name, stride in (("cfg2", "hot", 1), ("mini6", "small", 1)):
        c = synth.CONFIGS[rig]
        sc = synth.warp_scale(c["out_w"])
        for proj in (0, 1, 2):
            views = (0, 1, 3) if proj else (0,)
            for i in views:
                K, R = synth.camera(c["n"], c["w"], c["h"], c["hfov_deg"], i)
                kr = oracle.k_rinv_gpu(K, R)
                r = oracle.warp_roi(proj, K, R, sc, c["w"], c["h"])
                cases.append(("%s/p%d/view%d" % (name, proj, i), proj, r[0], r[1], r[3], r[2], kr, sc, c["w"], c["h"]))
            K, R = synth.camera(c["n"], c["w"], c["h"], c["hfov_deg"], 1)
            kr = oracle.k_rinv_gpu(K, R)
            if proj == 2:
                pole = int(math.pi * sc)
                span = int(math.pi * sc) + 2
                cases.append(("%s/p2/north" % name, 2, -span, 0, 24, 2 * span, kr, sc, c["w"], c["h"]))
                cases.append(("%s/p2/south" % name, 2, -span, pole - 24, 30, 2 * span, kr, sc, c["w"], c["h"]))
            if proj == 0:
                cases.append(("%s/p0/z0" % name, 0, -int(1.2 * sc), -int(0.2 * sc), int(0.4 * sc), int(2.4 * sc), kr, sc, c["w"], c["h"]))
    return cases


def test_warp_maps_against_float64(oracle):
    """The oracle's fp32 buildWarpMaps against warp_maps_f64 under map_bounds, and floor(map) / the valid mask equal the f64 ones wherever the
    f64 coordinate is farther than that bound from an integer."""
    seen = set()
    for name, proj, tu, tv, rows, cols, kr, sc, w, h in warp_cases(oracle):
        mx, my = oracle.build_warp_maps(proj, tu, tv, rows, cols, kr, sc)
        truth = np_ref.warp_maps_f64(proj, tu, tv, rows, cols, kr, sc)
        e_near, ratio, bad = map_errors(mx, my, truth, kr, w, h)
        assert e_near <= 1e-3 and ratio <= 1.0 and bad == 0, (name, e_near, ratio, bad)
        if proj == 2 and tu < -math.pi * sc < tu + cols:
            seen.add("wrap")
        if proj == 0 and (truth[2] < 0).any() and (truth[2] > 0).any():
            seen.add("z0")
    assert seen == {"wrap", "z0"}
