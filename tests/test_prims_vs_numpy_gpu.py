"""The device against tests/np_ref.py directly (not through the C oracle): random sizes, padded-pitch ROIs, full value ranges, for the entry
points whose only other check is the oracle.  A mistake shared by the oracle and a kernel fails here.  Integer and fp32 outputs must be bit
identical to np_ref; the warp maps are held to their float64 truth under the bounds of test_np_ref_crosscheck.map_bounds."""
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

import np_ref
import synth
from helpers import host, make_rig, to_dev, to_dev_roi
from test_np_ref_crosscheck import map_errors, warp_cases

pytestmark = pytest.mark.gpu
FAST = settings(max_examples=int(os.environ.get("MS_TEST_EXAMPLES", 40)), deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
F32 = np.float32
dims = st.tuples(st.integers(1, 70), st.integers(1, 90))
seeds = st.integers(0, 2 ** 31 - 1)


def dev(a, rng, roi):
    return to_dev_roi(a, rng) if roi else to_dev(a)


@FAST
@given(size=dims, seed=seeds, roi=st.booleans())
def test_pyr_down_32f(ms, cuda, size, seed, roi):
    rng = np.random.default_rng(seed)
    w = rng.random(size, dtype=np.float32)
    w[rng.random(size) < 0.3] = 0.0
    w[rng.random(size) < 0.2] = 1.0
    assert np.array_equal(host(ms.pyr_down(dev(w, rng, roi))), np_ref.pyr_down_32f(w))
    wild = (rng.standard_normal(size) * 10.0 ** rng.integers(-30, 30, size)).astype(F32)
    wild[rng.random(size) < 0.05] = np.nan
    assert np.array_equal(host(ms.pyr_down(dev(wild, rng, roi))), np_ref.pyr_down_32f(wild), equal_nan=True)


def test_weight_levels_of_a_rig(ms, cuda):
    """Compositor.weight_level(v, l) for every view and level: the np_ref pyramid of the padded comp.mask(v) / 255 (blenders.cpp:412-423)."""
    comp, cfg, _ = make_rig(ms, "mini4")
    for v in range(cfg["n"]):
        g = comp.view_geom(v)
        m = host(comp.mask(v))
        w = np.pad(np_ref.convert_8u_32f_scale(m, 1.0 / 255.0), ((g.top, g.bottom), (g.left, g.right)))
        for l in range(comp.pano_geom().num_bands + 1):
            assert np.array_equal(host(comp.weight_level(v, l)), w), "view %d level %d" % (v, l)
            w = np_ref.pyr_down_32f(w)
    comp.close()


@FAST
@given(size=st.tuples(st.integers(1, 60), st.integers(1, 90)), scale=st.sampled_from([0.5, 0.3, 1.0 / 3.0, 1.0, 2.0, 2.5]), cn=st.sampled_from([1, 3]),
       seed=seeds, roi=st.booleans())
def test_resize_linear(ms, cuda, size, scale, cn, seed, roi):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=size + ((3,) if cn == 3 else ()), dtype=np.uint8)
    if int(np.rint(size[0] * scale)) == 0 or int(np.rint(size[1] * scale)) == 0:
        return
    assert np.array_equal(host(ms.resize_linear(dev(src, rng, roi), fx=scale, fy=scale)), np_ref.resize_linear_8u(src, fx=scale, fy=scale))


@FAST
@given(size=st.tuples(st.integers(1, 50), st.integers(1, 70)), dsize=st.tuples(st.integers(1, 67), st.integers(1, 45)), n=st.integers(1, 4), seed=seeds)
def test_resize_linear_batch_to_any_size(ms, cuda, size, dsize, n, seed):
    """Every output width mod 4: the ragged right edge of the 4-pixel k_resize_linear3_x4 and its single-pixel fallback; down to 1 x 1."""
    rng = np.random.default_rng(seed)
    srcs = [rng.integers(0, 256, size=size + (3,), dtype=np.uint8) for _ in range(n)]
    if dsize == (size[1], size[0]):
        return                                                 # cuda::resize copies; the batch entry point refuses the case
    got = ms.resize_linear_batch([to_dev_roi(s, np.random.default_rng(seed)) for s in srcs], dsize=dsize)     # one pitch for the batch
    for g, s in zip(got, srcs):
        assert np.array_equal(host(g), np_ref.resize_linear_8u(s, dsize=dsize))
    assert np.array_equal(host(ms.resize_linear(to_dev(srcs[0]), dsize=dsize)), np_ref.resize_linear_8u(srcs[0], dsize=dsize))


even = st.tuples(st.integers(1, 40), st.integers(1, 50)).map(lambda t: (2 * t[0], 2 * t[1]))


@FAST
@given(hw=even, n=st.integers(1, 3), seed=seeds, roi=st.booleans())
def test_nv12_to_bgr(ms, cuda, hw, n, seed, roi):
    rng = np.random.default_rng(seed)
    srcs = [rng.integers(0, 256, size=(hw[0] * 3 // 2, hw[1]), dtype=np.uint8) for _ in range(n)]
    assert np.array_equal(host(ms.nv12_to_bgr(dev(srcs[0], rng, roi))), np_ref.nv12_to_bgr(srcs[0]))
    for g, s in zip(ms.nv12_to_bgr_batch([dev(s, np.random.default_rng(seed), roi) for s in srcs]), srcs):     # one geometry (pitch) per batch
        assert np.array_equal(host(g), np_ref.nv12_to_bgr(s))


def test_nv12_to_bgr_every_chroma_pair(ms, cuda):
    U, V = np.meshgrid(np.arange(256), np.arange(256))
    for yv in (0, 16, 128, 235, 255):
        uv = np.empty((256, 512), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = U, V
        src = np.vstack([np.full((512, 512), yv, np.uint8), uv])
        assert np.array_equal(host(ms.nv12_to_bgr(to_dev(src))), np_ref.nv12_to_bgr(src))


@FAST
@given(hw=even, seed=seeds, roi=st.booleans())
def test_bgr_to_i420(ms, cuda, hw, seed, roi):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=hw + (3,), dtype=np.uint8)
    src.reshape(-1, 3)[:2] = [(0, 0, 0), (255, 255, 255)][:src.shape[0] * src.shape[1]]
    assert np.array_equal(host(ms.bgr_to_i420(dev(src, rng, roi))), np_ref.bgr_to_i420(src))


@FAST
@given(size=dims, cn=st.sampled_from([1, 3]), gain=st.one_of(st.floats(0.9, 1.1), st.floats(1.0, 4.0), st.sampled_from([1.0, 1.0 + 1e-7, 0.5, 2.0])),
       seed=seeds, roi=st.booleans())
def test_convert_scale_8u(ms, cuda, size, cn, gain, seed, roi):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=size + ((3,) if cn == 3 else ()), dtype=np.uint8)
    src.reshape(-1)[::5] = 255
    assert np.array_equal(host(ms.convert_scale_8u(dev(src, rng, roi), gain)), np_ref.convert_scale_8u(src, gain))


@FAST
@given(src=st.tuples(st.integers(2, 45), st.integers(2, 45)), t=st.tuples(st.integers(1, 700), st.integers(1, 500)), seed=seeds, roi=st.booleans(),
       holes=st.booleans())
def test_custom_resize(ms, cuda, src, t, seed, roi, holes):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(src) * 300).astype(F32)
    if holes:
        a[rng.random(src) < 0.1] = np.nan
    assert np.array_equal(host(ms.custom_resize(dev(a, rng, roi), *t)), np_ref.custom_resize_32f(a, *t), equal_nan=True)


@pytest.mark.parametrize("src,t", [((2, 3000), (3000, 2)), ((3000, 2), (2, 3000)), ((5, 4097), (4096, 7)), ((40, 40), (1240, 1100))], ids=str)
def test_custom_resize_integer_division_branch(ms, cuda, src, t):
    """t * (n - 1) >= 2^23: the kernel must take the integer division (resize_axis_exact is false on that axis)."""
    assert max(t[0] * (src[1] - 1), t[1] * (src[0] - 1)) >= 2 ** 23 or src == (40, 40)
    a = np.random.default_rng(1).standard_normal(src).astype(F32) * 100
    assert np.array_equal(host(ms.custom_resize(to_dev(a), *t)), np_ref.custom_resize_32f(a, *t))


def test_set_mesh_maps(ms, cuda):
    """ms_set_mesh -> mesh_maps (convertMeshesToMap on the device) against np_ref.convert_mesh_to_map: meshes that reach past the view
    (NaN holes), vertices at negative coordinates, a hole in the mesh itself; 10 x 10 and 40 x 40 meshes and a ragged one."""
    comp, cfg, _ = make_rig(ms, "mini4", enable_cpw=True)
    rng = np.random.default_rng(7)
    for i in range(cfg["n"]):
        r = comp.view_geom(i).roi
        n, m = [(10, 10), (40, 40), (9, 11), (40, 40)][i % 4]
        mx, my = synth.mesh(r.width, r.height, n, m, phase=0.3 * i, amp=4.0)
        mx = (mx - 1.5 + rng.uniform(-0.5, 0.5, mx.shape)).astype(F32)
        my = (my * 0.8 - 0.9).astype(F32)
        if i == 1:
            mx[2, 3] = np.nan
        comp.set_mesh(i, mx, my)
        want = np_ref.convert_mesh_to_map(mx, my, r.width, r.height)
        for g, w in zip(comp.mesh_maps(i), want):
            assert np.array_equal(host(g), w, equal_nan=True), "view %d" % i
    comp.close()


def test_build_warp_maps_against_float64(ms, cuda, oracle):
    """ms_build_warp_maps against warp_maps_f64 on the hot-path and a small-focal rig, three projections, the spherical u wrap, both poles, a
    plane ROI across z = 0: the bounds and the integer-consequence rule of test_np_ref_crosscheck.test_warp_maps_against_float64."""
    for name, proj, tu, tv, rows, cols, kr, sc, w, h in warp_cases(oracle):
        mx, my = [host(t) for t in ms.build_warp_maps(proj, tu, tv, rows, cols, kr, sc)]
        e_near, ratio, bad = map_errors(mx, my, np_ref.warp_maps_f64(proj, tu, tv, rows, cols, kr, sc), kr, w, h)
        print("device %s: max |map - f64| near the image %.3g px, max error / bound %.3g" % (name, e_near, ratio))
        assert e_near <= 1e-3 and ratio <= 1.0 and bad == 0, (name, e_near, ratio, bad)


@FAST
@given(size=dims, seed=seeds, roi=st.booleans(), full=st.booleans())
def test_add_src_weight_and_normalize_16s(ms, cuda, size, seed, roi, full):
    """multiband_blend.cu:10-24 / 62-74 over the full int16 range, weights 0..256 or any int16; normalise with w != 0."""
    rng = np.random.default_rng(seed)
    src = rng.integers(-32768, 32768, size=size + (3,), dtype=np.int16)
    w = rng.integers(-32768, 32768, size=size, dtype=np.int16) if full else rng.integers(0, 257, size=size, dtype=np.int16)
    dst = rng.integers(-32768, 32768, size=size + (3,), dtype=np.int16)
    dw = rng.integers(-32768, 32768, size=size, dtype=np.int16)
    d_dst, d_dw = dev(dst, rng, roi), dev(dw, rng, roi)
    ms.add_src_weight_16s(dev(src, rng, roi), dev(w, rng, roi), d_dst, d_dw)
    np_ref.add_src_weight_16s(src, w, dst, dw)
    assert np.array_equal(host(d_dst), dst) and np.array_equal(host(d_dw), dw)
    dw[dw == 0] = 1
    d_dw = dev(dw, rng, roi)
    ms.normalize_using_weight_16s(d_dw, d_dst)
    np_ref.normalize_16s(dw, dst)
    assert np.array_equal(host(d_dst), dst)
