"""Regenerates ref_pin_small.npz: what the reference's own header-only helpers (oracle/_ref/libref_pin.so, `make -C oracle ref`) return on a fixed,
structured sample of inputs -- the stand-in tests/test_ref_pin.py checks the oracle against where the reference (and so the harness) is not present.
Run from the repository root after build(): python tests/golden/make_ref_pin_golden.py"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_pin.so"))
ref.ref_pin_eval_f32.argtypes = [C.c_int, C.c_float]
ref.ref_pin_eval_i32.argtypes = [C.c_int, C.c_int]
ref.ref_pin_eval_f64.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
ref.ref_pin_eval_f64.restype = None
ref.ref_pin_app_int.argtypes = [C.c_char_p, C.POINTER(C.c_longlong)]
ref.ref_pin_app_double.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
rng = np.random.default_rng(2024)


def f32_bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# float32 bit patterns: 32 random mantissas for every sign / exponent, every tie k + 0.5 and every integer near the saturation limits, the neighbours of
# the int32 / int16 / uint8 bounds, zeros, denormals, infinities and NaNs with several payloads
se = np.arange(512, dtype=np.uint32) << 23
pat = [(se[:, None] | rng.integers(0, 1 << 23, size=(512, 32), dtype=np.uint32)).ravel(), se, se | 0x7FFFFF]
pat.append(f32_bits(np.arange(-1000, 1000, dtype=np.float32) + 0.5))
for edge in (0.0, 255.0, 256.0, 32767.0, -32768.0, 65535.0, 2147483648.0, -2147483648.0, 16777216.0):
    e = f32_bits(np.float32(edge) + np.arange(-3, 4, dtype=np.float32))
    pat += [e, f32_bits(-np.float32(edge) + np.arange(-3, 4, dtype=np.float32)), e - 1, e + 1, e - 2, e + 2]
    pat.append(f32_bits(np.float32(edge) + np.float32(0.5) * np.arange(-6, 7, dtype=np.float32)))
pat.append(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000, 0x00000001, 0x80000001, 0x007FFFFF], np.uint32))
f32 = np.unique(np.concatenate(pat).astype(np.uint32))
f32_out = np.array([[ref.ref_pin_eval_f32(w, float(v)) for v in f32.view(np.float32)] for w in range(5)], np.int32)

i32 = np.unique(np.concatenate([rng.integers(-(1 << 31), 1 << 31, size=8000, dtype=np.int64),
                                np.arange(-33000, -32500), np.arange(32500, 33000), np.arange(-300, 600),
                                [-(1 << 31), -(1 << 31) + 1, (1 << 31) - 2, (1 << 31) - 1]]).astype(np.int32))
i32_out = np.array([[ref.ref_pin_eval_i32(w, int(v)) for v in i32] for w in range(2)], np.int32)

# doubles: as tests/test_ref_pin.py::test_double_precision_rounding_helpers builds them, a fixed sample of each kind
bits = rng.integers(0, 1 << 64, size=20000, dtype=np.uint64).view(np.float64)
bits = bits[np.isfinite(bits) & (np.abs(bits) < 2147483000.0)]
ties = np.arange(-2000, 2000, dtype=np.float64) + 0.5
sizes = np.arange(1, 8193, 7, dtype=np.float64)[:, None] * np.sqrt(np.array([0.6, 0.01, 1.4, 2.2]) * 1e6 / (1920.0 * 1080.0))[None, :]
f64 = np.ascontiguousarray(np.concatenate([bits, ties, sizes.ravel(), rng.uniform(-70000, 70000, 5000)]))
f64_out = np.empty((6, f64.size), np.int32)
special = np.ascontiguousarray(np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 5e-324, 1.7976931348623157e308, np.float64(np.float32(np.nan))]))
special_out = np.empty((2, special.size), np.int32)
for w in range(6):
    if w in (2, 3):
        o = np.empty(special.size, np.int32)
        ref.ref_pin_eval_f64(w, special.ctypes.data, o.ctypes.data, special.size)
        special_out[w - 2] = o
    o = np.empty(f64.size, np.int32)
    ref.ref_pin_eval_f64(w, f64.ctypes.data, o.ctypes.data, f64.size)
    f64_out[w] = o

const_ids = np.array([0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 20, 21, 22, 30], np.int32)
const_vals = np.array([ref.ref_pin_const(int(i)) for i in const_ids], np.int32)
INT_NAMES = ["NUM_IMAGES", "OUTPUT_WIDTH", "OUTPUT_HEIGHT", "RECALIB_DEL", "RECALIB_THRESH", "RECALIB_INTERP", "HESS_THRESH", "NOCTAVES", "NOCTAVESLAYERS",
             "MAX_FEATURES_PER_IMAGE", "MAX_TEMPORAL_FEATURES_PER_IMAGE", "MESH_HEIGHT", "MESH_WIDTH", "GLOBAL_DIST", "CAPTURE_IMG_WIDTH", "CAPTURE_IMG_HEIGHT",
             "CAPTURE_IMG_CHANNELS", "wrapAround", "recalibrate", "enable_local", "keep_aspect_ratio", "add_black_bars", "USE_TEMPORAL", "skip_frames"]
DOUBLE_NAMES = ["WORK_MEGAPIX", "SEAM_MEAGPIX", "COMPOSE_MEGAPIX", "MATCH_CONF", "BLEND_STRENGTH", "PI", "ALPHAS0", "ALPHAS1", "ALPHAS2", "ALPHAS3"]


def app(fn, ctype, name):
    v = ctype(0)
    assert fn(name.encode(), C.byref(v)) == 1, name
    return v.value


np.savez_compressed(os.path.join(HERE, "ref_pin_small.npz"), f32_bits=f32, f32_out=f32_out, i32=i32, i32_out=i32_out, f64=f64, f64_out=f64_out,
                    f64_special=special, f64_special_out=special_out, const_ids=const_ids, const_vals=const_vals,
                    int_names=np.array(INT_NAMES), int_vals=np.array([app(ref.ref_pin_app_int, C.c_longlong, n) for n in INT_NAMES], np.int64),
                    double_names=np.array(DOUBLE_NAMES), double_vals=np.array([app(ref.ref_pin_app_double, C.c_double, n) for n in DOUBLE_NAMES], np.float64))
print("ref_pin_small.npz: %d floats, %d ints, %d doubles" % (f32.size, i32.size, f64.size))
