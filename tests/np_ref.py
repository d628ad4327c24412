"""Independent numpy restatements of the reference kernels, used ONLY to cross-check the C oracle
(tests/test_oracle_crosscheck.py, tests/test_np_ref_crosscheck.py) and the device (tests/test_prims_vs_numpy_gpu.py).  Deliberately written
differently from oracle/*.c: vectorised, integer arithmetic for the 16S pyramids (the CUDA fp32 sums are exact dyadics), an exactly rounded
fp32 fma (fmaf32) for the fused chains, definitions instead of algorithms where the reference's result is defined by them (distance transform)."""
import numpy as np


def r101(i, n):
    i = np.abs(i)
    return np.abs((n - 1) - np.abs((n - 1) - i)) % n


def reflect(i, n):
    last = n - 1
    hi = last - np.abs(last - i) + (i > last)
    return (np.abs(hi) - (hi < 0)) % n


def rne_shift(s, k):
    s = s.astype(np.int64)
    return (s + ((1 << (k - 1)) - 1) + ((s >> k) & 1)) >> k


def pyr_down_16s(src):
    """pyr_down.cu:55-174 as an integer 5x5 binomial with BORDER_REFLECT_101 and round-half-even."""
    h, w = src.shape[:2]
    k = np.array([1, 4, 6, 4, 1], np.int64)
    oy = np.arange((h + 1) // 2) * 2
    ox = np.arange((w + 1) // 2) * 2
    acc = 0
    s = src.astype(np.int64)
    for a in range(5):
        rows = s[r101(oy + a - 2, h)]
        for b in range(5):
            acc = acc + k[a] * k[b] * rows[:, r101(ox + b - 2, w)]
    return np.clip(rne_shift(acc, 8), -32768, 32767).astype(np.int16)


def pyr_up_16s(src):
    """pyr_up.cu:55-145: zero-insert, 5x5 binomial x4, source index min(n-1, |i|)."""
    h, w = src.shape[:2]
    s = src.astype(np.int64)
    z = np.zeros((2 * h + 4, 2 * w + 4) + src.shape[2:], np.int64)    # dst grid with 2-px apron, index = dst + 2
    ys = np.arange(-2, 2 * h + 2)
    xs = np.arange(-2, 2 * w + 2)
    ry = np.minimum(np.abs(ys >> 1), h - 1)
    rx = np.minimum(np.abs(xs >> 1), w - 1)
    full = s[ry][:, rx]
    ev_y = (ys % 2 == 0)
    ev_x = (xs % 2 == 0)
    m = ev_y[:, None] & ev_x[None, :]
    z = full * (m[..., None] if src.ndim == 3 else m)
    k = np.array([1, 4, 6, 4, 1], np.int64)
    acc = 0
    H, W = 2 * h, 2 * w
    for a in range(5):
        for b in range(5):
            acc = acc + k[a] * k[b] * z[a:a + H, b:b + W]
    return np.clip(rne_shift(acc, 6), -32768, 32767).astype(np.int16)


def remap_linear(src, mx, my):
    """filters.hpp:90-114 (`out = out + src_reg * w` in tap order, contracted to fma by nvcc) + border_interpolate.hpp:698-717 (taps outside
    the image read 0); the fma chain through fmaf32, so the result is exact."""
    h, w = src.shape[:2]
    x1 = np.floor(mx).astype(np.int64); y1 = np.floor(my).astype(np.int64)
    x2, y2 = x1 + 1, y1 + 1
    f = np.float32
    wts = [((x2.astype(f) - mx) * (y2.astype(f) - my)), ((mx - x1.astype(f)) * (y2.astype(f) - my)),
           ((x2.astype(f) - mx) * (my - y1.astype(f))), ((mx - x1.astype(f)) * (my - y1.astype(f)))]
    taps = [(y1, x1), (y1, x2), (y2, x1), (y2, x2)]
    out = np.zeros(mx.shape + (3,), np.float32)
    for (yy, xx), wt in zip(taps, wts):
        inb = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        v = np.where(inb[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0).astype(np.float32)
        out = fmaf32(v, wt.astype(np.float32)[..., None], out)
    return sat_u8(out)


def add_src_weight(src, w, dst, dst_w):
    t = np.trunc(src.astype(np.float32) * w[..., None].astype(np.float32)).astype(np.int64)
    dst[...] = ((dst.astype(np.int64) + t + 32768) % 65536 - 32768).astype(np.int16)
    dst_w += w


def normalize(w, src):
    den = (w + np.float32(1e-5)).astype(np.float32)
    src[...] = np.trunc(src.astype(np.float32) / den[..., None]).astype(np.int16)


def feather_blend_np(corners, imgs8u, masks, dt_l1, sharpness=0.02):
    """numpy restatement of FeatherBlender (blenders.cpp:139-186); dt_l1(mask) -> float32 L1 distance transform."""
    xs = [c[0] for c in corners]; ys = [c[1] for c in corners]
    x0, y0 = min(xs), min(ys)
    x1 = max(c[0] + m.shape[1] for c, m in zip(corners, masks)); y1 = max(c[1] + m.shape[0] for c, m in zip(corners, masks))
    dst = np.zeros((y1 - y0, x1 - x0, 3), np.int16); dw = np.zeros((y1 - y0, x1 - x0), np.float32)
    for (cx, cy), img, m in zip(corners, imgs8u, masks):
        w = np.minimum(dt_l1(m).astype(np.float32) * np.float32(sharpness), np.float32(1.0)).astype(np.float32)
        contrib = np.trunc(img.astype(np.float32) * w[:, :, None]).astype(np.int16)
        sl = (slice(cy - y0, cy - y0 + m.shape[0]), slice(cx - x0, cx - x0 + m.shape[1]))
        dst[sl] = (dst[sl].astype(np.int32) + contrib).astype(np.int16)
        dw[sl] = dw[sl] + w
    q = np.trunc(dst.astype(np.float32) / (dw + np.float32(1e-5))[:, :, None]).astype(np.int16)
    mask = np.where(dw > np.float32(1e-5), 255, 0).astype(np.uint8)
    q[mask == 0] = 0
    return q, mask


def cv_remap_linear_np(src, mapx, mapy):
    """Independent numpy statement of cv::remap's CPU arithmetic (INTER_LINEAR, float map pair, BORDER_CONSTANT 0, 8-bit):
    coordinates quantised to 1/32 px (round half to even), closed-form 15-bit weights (32-fy)(32-fx)*32 ..., except the all-integer entry,
    which OpenCV's table holds as {32767, 0, 0, 1} (32768 saturates to short and the fix-up adds the missing 1 to the last tap)."""
    src = np.asarray(src)
    img = src[..., None] if src.ndim == 2 else src
    h, w, cn = img.shape
    q = []
    for m in (mapx, mapy):
        r = np.rint(np.asarray(m, np.float32) * np.float32(32)).astype(np.float64)
        bad = ~np.isfinite(r) | (r >= 2.0 ** 31) | (r < -2.0 ** 31)
        q.append(np.where(bad, -2.0 ** 31, r).astype(np.int64))
    fx, fy = q[0] & 31, q[1] & 31
    sx, sy = np.clip(q[0] >> 5, -32768, 32767), np.clip(q[1] >> 5, -32768, 32767)
    wts = [(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32]
    whole = (fx == 0) & (fy == 0)
    wts[0] = np.where(whole, 32767, wts[0]); wts[3] = np.where(whole, 1, wts[3])
    acc = np.zeros(sx.shape + (cn,), np.int64)
    for t, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        xx, yy = sx + dx, sy + dy
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        px = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64)
        acc += np.where(ok[..., None], px, 0) * wts[t][..., None]
    out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    return out[..., 0] if src.ndim == 2 else out


# ---- the reference's CPU pyramids (cv::pyrDown / cv::pyrUp, OCV/imgproc/src/pyramids.cpp:851-1078), numpy statements --------------------
def cv_pyr_down_16s(src):
    """pyrDown_<FixPtCast<short,8>>: integer 5x5 binomial, BORDER_REFLECT_101, (sum + 128) >> 8 (ties round UP, unlike the CUDA kernel)."""
    h, w = src.shape[:2]
    k = np.array([1, 4, 6, 4, 1], np.int64)
    oy, ox = np.arange((h + 1) // 2) * 2, np.arange((w + 1) // 2) * 2
    s = src.astype(np.int64)
    acc = 0
    for a in range(5):
        rows = s[r101(oy + a - 2, h)]
        for b in range(5):
            acc = acc + k[a] * k[b] * rows[:, r101(ox + b - 2, w)]
    return ((acc + 128) >> 8).astype(np.int16)


def cv_pyr_up_16s(src):
    """pyrUp_<FixPtCast<short,6>> to twice the size: the same taps and source indexing (left / top mirrored, right / bottom replicated:
    pyramids.cpp:1013-1031 spell out 6a + 2b and b + 7c) as the CUDA kernel, (sum + 32) >> 6."""
    h, w = src.shape[:2]
    s = src.astype(np.int64)
    ys, xs = np.arange(-2, 2 * h + 2), np.arange(-2, 2 * w + 2)
    full = s[np.minimum(np.abs(ys >> 1), h - 1)][:, np.minimum(np.abs(xs >> 1), w - 1)]
    m = (ys % 2 == 0)[:, None] & (xs % 2 == 0)[None, :]
    z = full * (m[..., None] if src.ndim == 3 else m)
    k = np.array([1, 4, 6, 4, 1], np.int64)
    acc = 0
    for a in range(5):
        for b in range(5):
            acc = acc + k[a] * k[b] * z[a:a + 2 * h, b:b + 2 * w]
    return ((acc + 32) >> 6).astype(np.int16)


def cv_pyr_down_32f(src):
    """pyrDown_<FltCast<float,8>, PyrDownVec_32f> (x86 SSE build): fp32 throughout; horizontal ((6c + 4(b + d)) + a) + e; vertical in the SSE
    order ((r0 + r4) + (r2 + r2)) + 4((r1 + r3) + r2) for the first (width // 8) * 8 columns and ((6 r2 + 4 (r1 + r3)) + r0) + r4 for the rest;
    then * (1 / 256)."""
    f = np.float32
    h, w = src.shape
    oy, ox = np.arange((h + 1) // 2) * 2, np.arange((w + 1) // 2) * 2
    s = src.astype(f)
    col = [s[:, r101(ox + b - 2, w)] for b in range(5)]
    hrow = ((col[2] * f(6) + (col[1] + col[3]) * f(4)) + col[0]) + col[4]          # (h, dcols) fp32, evaluated op by op
    r = [hrow[r101(oy + a - 2, h)] for a in range(5)]
    vec = ((r[0] + r[4]) + (r[2] + r[2])) + ((r[1] + r[3]) + r[2]) * f(4)
    tail = ((r[2] * f(6) + (r[1] + r[3]) * f(4)) + r[0]) + r[4]
    nvec = (len(ox) // 8) * 8
    out = np.where(np.arange(len(ox))[None, :] < nvec, vec, tail).astype(f)
    return (out * f(1.0 / 256)).astype(f)


# ---- the remaining oracle kernels (CUDA flavour unless said otherwise), stated from the reference sources the oracle cites ------------------
F32 = np.float32


def fmaf32(a, b, c):
    """Correctly rounded fp32 fused multiply-add, elementwise.  a*b of two fp32 values is exact in fp64; s = p + c and its TwoSum error e
    give the exact sum s + e; rounding s to odd (step one ulp toward e when e != 0 and s has an even mantissa) keeps 53 - 24 > 2 guard bits,
    so the final cast to fp32 rounds once, correctly."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def sat_u8(v):
    """saturate_cast<uchar>(float) (cuda/saturate_cast.hpp): round to nearest even, clamp, NaN -> 0."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.rint(v), nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.uint8)


def f2i_rz(v):
    """__float2int_rz: toward zero, saturating to int32, NaN -> 0."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.trunc(v), nan=0.0), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def pyr_down_32f(src):
    """pyr_down.cu:55-174 instantiated for float (the weight pyramids, blenders.cpp:420-423): per source column the vertical chain
    sum = 0.0625 r[-2]; sum = sum + 0.25 r[-1]; ... (contracted to fma), then the same chain horizontally over the column sums;
    BORDER_REFLECT_101 on both axes, ((h + 1) / 2, (w + 1) / 2) outputs, every second row and column."""
    h, w = src.shape
    s = np.asarray(src, F32)
    k = [F32(0.0625), F32(0.25), F32(0.375), F32(0.25), F32(0.0625)]
    oy, ox = np.arange((h + 1) // 2) * 2, np.arange((w + 1) // 2) * 2

    def chain(taps):
        acc = (k[0] * taps[0]).astype(F32)
        for c, t in zip(k[1:], taps[1:]):
            acc = fmaf32(c, t, acc)
        return acc
    vert = chain([s[r101(oy + a - 2, h)] for a in range(5)])                 # (dh, w): the column sums of the rows the outputs use
    return chain([vert[:, r101(ox + b - 2, w)] for b in range(5)])


def resize_linear_8u(src, dsize=None, fx=0.0, fy=0.0):
    """cuda::resize INTER_LINEAR.  Host (resize.cpp): dsize = saturate_cast<int>(cols * fx) when not given, else fx = dsize.width / cols;
    dsize == src.size() is a copy; the kernel gets float(1 / fx).  Kernel resize.cu:71-106: src_x = dst_x * fx (fp32), x1 = floor, x2 = x1 + 1,
    reads of x2 / y2 clamped to the last column / row (the weights keep the unclamped x2, y2), out = out + src * w in tap order, saturate_cast."""
    rows, cols = src.shape[:2]
    if dsize is None:
        dsize = (int(np.rint(cols * fx)), int(np.rint(rows * fy)))
    else:
        fx, fy = dsize[0] / cols, dsize[1] / rows
    if (dsize[1], dsize[0]) == (rows, cols):
        return np.array(src, copy=True)
    ifx, ify = F32(1.0 / fx), F32(1.0 / fy)
    img = src[..., None] if src.ndim == 2 else src
    sx = (np.arange(dsize[0]).astype(F32) * ifx).astype(F32)
    sy = (np.arange(dsize[1]).astype(F32) * ify).astype(F32)
    x1, y1 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    x2, y2 = x1 + 1, y1 + 1
    x2r, y2r = np.minimum(x2, cols - 1), np.minimum(y2, rows - 1)
    wx1, wx2 = (x2.astype(F32) - sx)[None, :], (sx - x1.astype(F32))[None, :]
    wy1, wy2 = (y2.astype(F32) - sy)[:, None], (sy - y1.astype(F32))[:, None]
    out = np.zeros((dsize[1], dsize[0], img.shape[2]), F32)
    for ry, rx, wt in ((y1, x1, wx1 * wy1), (y1, x2r, wx2 * wy1), (y2r, x1, wx1 * wy2), (y2r, x2r, wx2 * wy2)):
        out = fmaf32(img[ry][:, rx].astype(F32), wt.astype(F32)[..., None], out)
    out = sat_u8(out)
    return out[..., 0] if src.ndim == 2 else out


# ITU-R BT.601 fixed point of OpenCV's YUV <-> RGB invokers (imgproc color.cpp, ITUR_BT_601_*: coefficient * 2^20, rounded)
_SH = 20
_CY, _CUB, _CUG, _CVG, _CVR = 1220542, 2116026, -409993, -852492, 1673527
_CRY, _CGY, _CBY, _CRU, _CGU, _CBU, _CGV, _CBV = 269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448


def nv12_to_bgr(src):
    """YUV420sp2RGB888Invoker<bIdx 0, uIdx 0>: Y plane (h rows) then h/2 rows of interleaved U, V shared by a 2x2 block;
    Y' = max(0, Y - 16) * CY; B = (Y' + CUB u + 2^19) >> 20, G = (Y' + CVG v + CUG u + 2^19) >> 20, R = (Y' + CVR v + 2^19) >> 20, saturated."""
    h = src.shape[0] * 2 // 3
    Y = src[:h].astype(np.int64)
    uv = src[h:].astype(np.int64)
    u = np.repeat(np.repeat(uv[:, 0::2], 2, axis=0), 2, axis=1)[:h] - 128
    v = np.repeat(np.repeat(uv[:, 1::2], 2, axis=0), 2, axis=1)[:h] - 128
    yy = np.maximum(Y - 16, 0) * _CY
    half = 1 << (_SH - 1)
    b = (yy + half + _CUB * u) >> _SH
    g = (yy + half + _CVG * v + _CUG * u) >> _SH
    r = (yy + half + _CVR * v) >> _SH
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def bgr_to_i420(src):
    """RGB888toYUV420pInvoker (planar, U before V): Y = (CRY r + CGY g + CBY b + 2^19 + 16 * 2^20) >> 20 per pixel; U, V from the TOP-LEFT pixel
    of each 2x2 block: U = (CRU r + CGU g + CBU b + 2^19 + 128 * 2^20) >> 20, V = (CBU r + CGV g + CBV b + ...) >> 20 (CRV = CBU); saturated.
    Output (h * 3 / 2, w): Y, then U (h/2 x w/2) and V (h/2 x w/2) back to back."""
    h, w = src.shape[:2]
    s = src.astype(np.int64)
    b, g, r = s[..., 0], s[..., 1], s[..., 2]
    half = 1 << (_SH - 1)
    Y = (_CRY * r + _CGY * g + _CBY * b + half + (16 << _SH)) >> _SH
    tl = (slice(0, h - h % 2, 2), slice(0, w - w % 2, 2))
    U = (_CRU * r[tl] + _CGU * g[tl] + _CBU * b[tl] + half + (128 << _SH)) >> _SH
    V = (_CBU * r[tl] + _CGV * g[tl] + _CBV * b[tl] + half + (128 << _SH)) >> _SH
    out = np.zeros((h * 3 // 2, w), np.uint8)
    out[:h] = np.clip(Y, 0, 255)
    chroma = np.concatenate([np.clip(U, 0, 255).ravel(), np.clip(V, 0, 255).ravel()]).astype(np.uint8)
    out.reshape(-1)[h * w:h * w + chroma.size] = chroma
    return out


# BT.601 in float64 from its definition (Kr = 0.299, Kb = 0.114; studio range: Y' 16..235 over 219 steps, chroma 128 +- 112 over 224)
_KR, _KB = 0.299, 0.114
_KG = 1.0 - _KR - _KB


def bt601_yuv_to_bgr_f64(Y, U, V):
    """R, G, B in 0..255 (float64, unrounded) of studio-range Y'CbCr; Y' below 16 is clamped to 16 (the footroom convention of the invoker)."""
    y = np.maximum(np.asarray(Y, np.float64) - 16.0, 0.0) * (255.0 / 219.0)
    cb = (np.asarray(U, np.float64) - 128.0) * (255.0 / 224.0)
    cr = (np.asarray(V, np.float64) - 128.0) * (255.0 / 224.0)
    r = y + 2.0 * (1.0 - _KR) * cr
    b = y + 2.0 * (1.0 - _KB) * cb
    g = (y - _KR * r - _KB * b) / _KG
    return np.stack([b, g, r], -1)


def bt601_bgr_to_yuv_f64(bgr):
    """(Y', Cb, Cr) float64, unrounded, of 8-bit full-range B, G, R."""
    s = np.asarray(bgr, np.float64)
    b, g, r = s[..., 0], s[..., 1], s[..., 2]
    yn = _KR * r + _KG * g + _KB * b
    return 16.0 + yn * (219.0 / 255.0), 128.0 + (b - yn) / (2.0 * (1.0 - _KB)) * (224.0 / 255.0), 128.0 + (r - yn) / (2.0 * (1.0 - _KR)) * (224.0 / 255.0)


def _cell(x, n, t):
    """custom_resize's cell index (APP/resize.cu:14-15, integer division) and fp32 fraction ((float)x * (n - 1) / t - index)."""
    i = (x * (n - 1)) // t
    q = ((x.astype(F32) * F32(n - 1)).astype(F32) / F32(t)).astype(F32)
    return i, (q - i.astype(F32)).astype(F32)


def custom_resize_32f(src, tx, ty):
    """APP/resize.cu:9-27: out = (1-uu)(1-vv) in[top][left] + uu(1-vv) in[top][left+1] + (1-uu)vv in[top+1][left] + uu vv in[top+1][left+1],
    left to right with the three additions contracted to fma; NaN in a tap propagates.  Needs rows, cols >= 2."""
    src = np.asarray(src, F32)
    rows, cols = src.shape
    left, uu = _cell(np.arange(tx), cols, tx)
    top, vv = _cell(np.arange(ty), rows, ty)
    U, V = uu[None, :], vv[:, None]
    one = F32(1)
    a, b, c, d = (one - U) * (one - V), U * (one - V), (one - U) * V, U * V
    T, L = top[:, None], left[None, :]
    with np.errstate(invalid="ignore"):
        r = (a * src[T, L]).astype(F32)
        r = fmaf32(b, src[T, L + 1], r)
        r = fmaf32(c, src[T + 1, L], r)
        return fmaf32(d, src[T + 1, L + 1], r)


def convert_mesh_to_map(mesh_x, mesh_y, width, height):
    """MeshWarper::convertMeshesToMap for one view (APP/meshwarper.cpp:823-886): the vertex mesh resized to the view (custom_resize), each
    pixel (x, y) dropped into the half-resolution cell ((int)mx / 2, (int)my / 2) (C truncation, so (-2, 0) lands in cell 0), every cell's
    mean of the x and y that landed there (0 / 0 = NaN for an empty cell), resized back to width x height."""
    bx, by = custom_resize_32f(mesh_x, width, height), custom_resize_32f(mesh_y, width, height)
    hw, hh = width // 2, height // 2
    with np.errstate(invalid="ignore"):
        ok = (bx > -2.0 ** 31) & (bx < 2.0 ** 31) & (by > -2.0 ** 31) & (by < 2.0 ** 31)
    ix = np.where(ok, np.trunc(np.where(ok, bx, 0)), 0).astype(np.int64)
    iy = np.where(ok, np.trunc(np.where(ok, by, 0)), 0).astype(np.int64)
    cx, cy = np.sign(ix) * (np.abs(ix) // 2), np.sign(iy) * (np.abs(iy) // 2)
    ok &= (cx >= 0) & (cy >= 0) & (cx < hw) & (cy < hh)
    yy, xx = np.mgrid[0:height, 0:width]
    sx, sy, cnt = (np.zeros((hh, hw)) for _ in range(3))       # integer sums, exact in fp64 (and in the fp32 of the reference while < 2^24)
    np.add.at(sx, (cy[ok], cx[ok]), xx[ok]); np.add.at(sy, (cy[ok], cx[ok]), yy[ok]); np.add.at(cnt, (cy[ok], cx[ok]), 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mx, my = (sx.astype(F32) / cnt.astype(F32)).astype(F32), (sy.astype(F32) / cnt.astype(F32)).astype(F32)
    return custom_resize_32f(mx, width, height), custom_resize_32f(my, width, height)


def remap_nearest_8uc1(src, mx, my):
    """PointFilter (filters.hpp:58-77): src(__float2int_rz(y), __float2int_rz(x)); BrdConstant(0) outside."""
    h, w = src.shape
    xi, yi = f2i_rz(mx), f2i_rz(my)
    inb = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    return np.where(inb, src[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], 0).astype(np.uint8)


def convert_scale_8u(src, alpha):
    """Convertor<uchar, uchar, float> (gpu_mat.cu): saturate_cast<uchar>(float(alpha) * src + 0)."""
    return sat_u8(F32(alpha) * np.asarray(src).astype(F32))


def convert_8u_32f_scale(src, alpha):
    """Convertor<uchar, float, float>: float(alpha) * src (the + 0 of beta is exact)."""
    return (F32(alpha) * np.asarray(src).astype(F32)).astype(F32)


def convert_16s_8u(src):
    """saturate_cast<uchar>(short)."""
    return np.clip(src, 0, 255).astype(np.uint8)


def copy_make_border_const_32f(src, top, bottom, left, right):
    """copyMakeBorder BORDER_CONSTANT(0) on 32FC1."""
    return np.pad(np.asarray(src, F32), ((top, bottom), (left, right)), mode="constant", constant_values=0)


def dilate3x3_8u(src):
    """3x3 maximum, the border replicated (a max filter's identity for the frame)."""
    h, w = src.shape
    p = np.pad(src, 1, mode="edge")
    return np.max(np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), axis=0)


def _wrap16(v):
    return ((np.asarray(v, np.int64) + 32768) % 65536 - 32768).astype(np.int16)


def add_src_weight_16s(src, w, dst, dst_w):
    """addSrcWeightKernel16S (multiband_blend.cu:10-24): dst += short((v * w) >> 8) (int product, arithmetic shift = floor), dst_w += w; short wraps."""
    ww = w.astype(np.int64)
    dst[...] = _wrap16(dst.astype(np.int64) + _wrap16((src.astype(np.int64) * ww[..., None]) >> 8))
    dst_w[...] = _wrap16(dst_w.astype(np.int64) + ww)


def normalize_16s(w, src):
    """normalizeUsingWeightKernel16S (multiband_blend.cu:62-74): short((v << 8) / w), C division (toward zero).  w == 0 is undefined there."""
    num = src.astype(np.int64) * 256
    den = np.broadcast_to(w.astype(np.int64)[..., None], num.shape)
    assert (den != 0).all(), "w == 0: undefined in the reference"
    q = np.abs(num) // np.abs(den) * np.sign(num) * np.sign(den)
    src[...] = _wrap16(q)


def distance_transform_l1(src):
    """cv::distanceTransform(DIST_L1): for every pixel, the taxicab distance |dx| + |dy| to the nearest zero pixel of the image (pixels outside
    the image are not zeros).  An image without a zero pixel: +inf everywhere (the reference holds a large sentinel there)."""
    src = np.asarray(src)
    h, w = src.shape
    zy, zx = np.nonzero(src == 0)
    if zy.size == 0:
        return np.full((h, w), np.inf, F32)
    py, px = np.mgrid[0:h, 0:w]
    py, px = py.ravel(), px.ravel()
    out = np.empty(h * w, np.int64)
    step = max(1, 4_000_000 // zy.size)
    for i in range(0, h * w, step):
        out[i:i + step] = (np.abs(py[i:i + step, None] - zy[None, :]) + np.abs(px[i:i + step, None] - zx[None, :])).min(axis=1)
    return out.reshape(h, w).astype(F32)


def voronoi_seams(corners, masks):
    """VoronoiSeamFinder (seam_finders.cpp:71-83, 111-160), masks edited in place: for every overlapping pair (i < j, in order), over the
    overlap grown by a 10-px gap (outside a view: 0), each view's 'unique' pixels (its mask minus the collision of the two) and the taxicab
    distance of every pixel to them; a pixel of the overlap strictly nearer to view i's unique pixels is cleared from view j, every other one
    from view i."""
    gap = 10
    n = len(masks)
    for i in range(n - 1):
        for j in range(i + 1, n):
            (x1, y1), (x2, y2) = corners[i], corners[j]
            (h1, w1), (h2, w2) = masks[i].shape, masks[j].shape
            tlx, tly = max(x1, x2), max(y1, y2)
            brx, bry = min(x1 + w1, x2 + w2), min(y1 + h1, y2 + h2)
            if not (tlx < brx and tly < bry):
                continue
            ys, xs = np.arange(tly - gap, bry + gap), np.arange(tlx - gap, brx + gap)

            def cut(m, cx, cy):
                yy, xx = ys - cy, xs - cx
                okr, okc = (yy >= 0) & (yy < m.shape[0]), (xx >= 0) & (xx < m.shape[1])
                sub = m[np.clip(yy, 0, m.shape[0] - 1)][:, np.clip(xx, 0, m.shape[1] - 1)]
                return np.where(okr[:, None] & okc[None, :], sub, 0)
            s1, s2 = cut(masks[i], x1, y1), cut(masks[j], x2, y2)
            both = (s1 != 0) & (s2 != 0)
            d1 = distance_transform_l1(np.where(both, 0, s1) == 0)
            d2 = distance_transform_l1(np.where(both, 0, s2) == 0)
            seam = (d1 < d2)[gap:-gap, gap:-gap]
            v2 = masks[j][tly - y2:bry - y2, tlx - x2:brx - x2]
            v1 = masks[i][tly - y1:bry - y1, tlx - x1:brx - x1]
            v2[seam] = 0
            v1[~seam] = 0
    return masks


def gain_overlap_stats(corners, images, masks):
    """GainCompensator::feed's overlap statistics (exposure_compensate.cpp:89-123): for every pair i <= j whose rectangles meet (overlapRoi, util.cpp:100-112),
    over the pixels where BOTH masks equal 255 (:101; feed's level value, :66), N = max(1, their number) (:103) and I(i, j), I(j, i) = the sum of
    sqrt(b^2 + g^2 + r^2) of view i, view j over them divided by N (:114-120).  The squares are summed as integers (sqr(int), util_inl.hpp:122) and the root is
    taken in double; the sum runs pixel by pixel in raster order, which np.cumsum reproduces (np.sum adds pairwise and differs in the last bit).  Pairs that
    do not meet stay 0 (:82-83).  Returns (N int64 n x n, I float64 n x n)."""
    n = len(images)
    N = np.zeros((n, n), np.int64)
    I = np.zeros((n, n), np.float64)
    for i in range(n):
        for j in range(i, n):
            (x1, y1), (x2, y2) = corners[i], corners[j]
            (h1, w1), (h2, w2) = masks[i].shape, masks[j].shape
            tlx, tly = max(x1, x2), max(y1, y2)
            brx, bry = min(x1 + w1, x2 + w2), min(y1 + h1, y2 + h2)
            if not (tlx < brx and tly < bry):
                continue
            sl1 = (slice(tly - y1, bry - y1), slice(tlx - x1, brx - x1))
            sl2 = (slice(tly - y2, bry - y2), slice(tlx - x2, brx - x2))
            both = (masks[i][sl1] == 255) & (masks[j][sl2] == 255)
            N[i, j] = N[j, i] = max(1, int(both.sum()))
            sums = []
            for im, sl in ((images[i], sl1), (images[j], sl2)):
                px = im[sl].astype(np.int64)
                root = np.sqrt((px * px).sum(axis=2).astype(np.float64))[both]          # (boolean indexing keeps raster order)
                sums.append(float(np.cumsum(root)[-1]) if root.size else 0.0)
            I[i, j] = sums[0] / float(N[i, j])
            I[j, i] = sums[1] / float(N[i, j])
    return N, I


def gain_normal_equations(N, I):
    """The normal equations of GainCompensator::feed (exposure_compensate.cpp:125-140), alpha = 0.01, beta = 100, in the reference's accumulation order and
    its left-to-right products, as Python floats (IEEE double, one rounding per operation).  Returns (A list of rows, b list)."""
    n = len(N)
    alpha, beta = 0.01, 100.0
    A = [[0.0] * n for _ in range(n)]
    b = [0.0] * n
    for i in range(n):
        for j in range(n):
            Nij, Iij, Iji = float(int(N[i][j])), float(I[i][j]), float(I[j][i])
            b[i] += beta * Nij
            A[i][i] += beta * Nij
            if j == i:
                continue
            A[i][i] += 2 * alpha * Iij * Iij * Nij
            A[i][j] -= 2 * alpha * Iij * Iji * Nij
    return A, b


def solve_lu64(A, b):
    """cv::solve(A, b, x, DECOMP_LU) on CV_64F with one right-hand side, in Python floats and the reference's operation order: the closed forms of
    lapack.cpp:1107-1237 for n <= 3 (n = 2: :1141-1148 with det2, :748; n = 3: :1188-1209 with det3, :749-751; n = 1: :1229-1231), LUImpl
    (matrix_decomp.cpp:52-107: partial pivoting, eps = 100 DBL_EPSILON, :127) above that.  A: list of rows, b: list; neither is modified.
    Returns (x list or None when the reference reports a singular system, the number of row exchanges LUImpl made)."""
    n = len(b)
    A = [list(map(float, r)) for r in A]
    b = list(map(float, b))
    if n == 1:
        return ([b[0] / A[0][0]] if A[0][0] != 0.0 else None), 0
    if n == 2:
        d = A[0][0] * A[1][1] - A[0][1] * A[1][0]
        if d == 0.0:
            return None, 0
        d = 1.0 / d
        return [(b[0] * A[1][1] - b[1] * A[0][1]) * d, (b[1] * A[0][0] - b[0] * A[1][0]) * d], 0
    if n == 3:
        d = (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
             A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))
        if d == 0.0:
            return None, 0
        d = 1.0 / d
        t0 = ((A[1][1] * A[2][2] - A[1][2] * A[2][1]) * b[0] + (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * b[1] + (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * b[2]) * d
        t1 = ((A[1][2] * A[2][0] - A[1][0] * A[2][2]) * b[0] + (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * b[1] + (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * b[2]) * d
        t2 = ((A[1][0] * A[2][1] - A[1][1] * A[2][0]) * b[0] + (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * b[1] + (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * b[2]) * d
        return [t0, t1, t2], 0
    eps = 100 * 2.0 ** -52
    swaps = 0
    for i in range(n):
        k = i
        for j in range(i + 1, n):
            if abs(A[j][i]) > abs(A[k][i]):
                k = j
        if abs(A[k][i]) < eps:
            return None, swaps
        if k != i:
            for j in range(i, n):                       # (the reference exchanges columns i.. only: what lies left of them is never read again)
                A[i][j], A[k][j] = A[k][j], A[i][j]
            b[i], b[k] = b[k], b[i]
            swaps += 1
        d = -1 / A[i][i]
        for j in range(i + 1, n):
            al = A[j][i] * d
            for q in range(i + 1, n):
                A[j][q] += al * A[i][q]
            b[j] += al * b[i]
    for i in range(n - 1, -1, -1):
        s = b[i]
        for q in range(i + 1, n):
            s -= A[i][q] * b[q]
        b[i] = s / A[i][i]
    return b, swaps


def gain_compensator(corners, images, masks):
    """GainCompensator::feed (exposure_compensate.cpp:71-145) -> (gains float64 (n,), N int64 (n, n), I float64 (n, n), row exchanges of the LU solve): the
    three restatements above, one after the other.  A singular system (the reference's solve returns false and leaves the gains undefined) raises."""
    N, I = gain_overlap_stats(corners, images, masks)
    A, b = gain_normal_equations(N, I)
    x, swaps = solve_lu64(A, b)
    if x is None:
        raise ValueError("singular gain system")
    return np.array(x, np.float64), N, I, swaps


def warp_maps_f64(proj, tl_u, tl_v, rows, cols, k_rinv, scale, t=(0, 0, 0)):
    """The backward maps of buildWarpMapsKernel (build_warp_maps.cu:67-152) in float64, from the same fp32 k_rinv, scale and t: the TRUE map
    the fp32 kernel approximates.  proj 0 plane, 1 cylindrical, 2 spherical (the ms_stitch.h / ORC_PROJ_* codes).  Returns (x, y, z) -- z is
    the denominator, whose sign decides the reference's (-1, -1) for points behind the camera (cylindrical, spherical; the plane divides)."""
    k = np.asarray(k_rinv, F32).astype(np.float64).reshape(9)
    sc = float(F32(scale))
    tt = np.asarray(t, F32).astype(np.float64)
    u = (tl_u + np.arange(cols, dtype=np.float64))[None, :] / sc
    v = (tl_v + np.arange(rows, dtype=np.float64))[:, None] / sc
    if proj == 0:
        x_, y_, z_ = u - tt[0], v - tt[1], 1.0 - tt[2]
    elif proj == 1:
        x_, y_, z_ = np.sin(u), v, np.cos(u)
    else:
        x_, y_, z_ = np.sin(v) * np.sin(u), -np.cos(v), np.sin(v) * np.cos(u)
    x_, y_, z_ = np.broadcast_arrays(x_, y_, z_)
    x = k[0] * x_ + k[1] * y_ + k[2] * z_
    y = k[3] * x_ + k[4] * y_ + k[5] * z_
    z = k[6] * x_ + k[7] * y_ + k[8] * z_
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = x / z, y / z
    if proj != 0:
        x, y = np.where(z > 0, x, -1.0), np.where(z > 0, y, -1.0)
    return x, y, z


# ---- ORB front end (cudafeatures2d: fast.cu, orb.cu, orb.cpp): definitions, not the algorithms oracle/orb_oracle.py and csrc/features.hip share ------------
def fast_ring():
    """The 16 pixels of the radius-3 Bresenham circle as (dy, dx), in circular order (by angle): FAST's contiguity is cyclic, so neither the
    starting point nor the direction matters."""
    pts = [(dy, dx) for dy in range(-3, 4) for dx in range(-3, 4) if max(abs(dy), abs(dx)) == 3 and min(abs(dy), abs(dx)) <= 1 or (abs(dy), abs(dx)) == (2, 2)]
    assert len(pts) == 16
    return sorted(pts, key=lambda p: np.arctan2(p[0], p[1]))


def has_arc_by_definition(masks, length=9):
    """masks: ints, bit k = circle pixel k.  True where some rotation of the 16-bit word has `length` consecutive set bits."""
    m = np.asarray(masks, np.int64)
    bits = ((m[..., None] >> np.arange(16)) & 1).astype(bool)
    out = np.zeros(m.shape, bool)
    for start in range(16):
        out |= bits[..., (start + np.arange(length)) % 16].all(axis=-1)
    return out


def fast_is_corner(img, t):
    """(h, w) bool: 9 contiguous circle pixels all > v + t or all < v - t; False within 3 px of the border."""
    h, w = img.shape
    im = img.astype(np.int64)
    v = im[3:h - 3, 3:w - 3]
    ring = np.stack([im[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dy, dx in fast_ring()], axis=-1)
    wts = 1 << np.arange(16)
    out = np.zeros((h, w), bool)
    out[3:h - 3, 3:w - 3] = has_arc_by_definition(((ring > v[..., None] + t) * wts).sum(-1)) | has_arc_by_definition(((ring < v[..., None] - t) * wts).sum(-1))
    return out


def fast_score_brute_force(img, mask=None, threshold=20):
    """What cornerScore's binary search (fast.cu:195-218) finds: the largest t in [threshold, 255] at which the pixel is still a corner; 0 where it
    is no corner at `threshold` or the mask is 0.  Every t is tried."""
    alive = fast_is_corner(img, threshold)
    if mask is not None:
        alive &= mask != 0
    score = np.where(alive, threshold, 0).astype(np.int32)
    for t in range(threshold + 1, 256):
        if not alive.any():
            break
        alive &= fast_is_corner(img, t)
        score[alive] = t
    return score


def nms_strict(score):
    """(n, 2) x, y in raster order: non-zero scores strictly greater than all 8 neighbours (outside the map counts as 0)."""
    s = np.pad(score.astype(np.int64), 1)
    h, w = score.shape
    keep = score != 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                keep &= s[1:-1, 1:-1] > s[dy:dy + h, dx:dx + w]
    ys, xs = np.nonzero(keep)             # row-major: raster order
    return np.stack([xs, ys], axis=1)


def fast_keypoints_with_overflow(score, max_points):
    """The detector's buffer holds max_points raw corners; here the first ones in raster order (the reference leaves which to an atomic counter).
    Suppression then reads the whole score map, also at corners that did not fit (fast.cu:346-371 reads score(), not the buffer)."""
    raw = np.argwhere(score != 0)[:max_points]
    fits = np.zeros(score.shape, bool)
    fits[raw[:, 0], raw[:, 1]] = True
    win = nms_strict(score)
    return win[fits[win[:, 1], win[:, 0]]]


U_MAX_15 = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]      # the circular patch of radius 15, orb.cpp:514-529 evaluated by hand


def harris_sums(img, x, y, block=7):
    """Exact integer sums of Ix^2, Iy^2, Ix Iy over the block x block window centred on (x, y); Ix, Iy = the 3 x 3 Sobel derivatives."""
    im = img.astype(np.int64)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int64)
    a = b = c = 0
    r = block // 2
    for yy in range(y - r, y + r + 1):
        for xx in range(x - r, x + r + 1):
            win = im[yy - 1:yy + 2, xx - 1:xx + 2]
            ix, iy = int((win * kx).sum()), int((win * kx.T).sum())
            a += ix * ix; b += iy * iy; c += ix * iy
    return a, b, c


def ic_moments(img, x, y, u_max=U_MAX_15):
    """(m01, m10) over the pixel set {(u, v): |u| <= u_max[|v|]}."""
    half = len(u_max) - 1
    m01 = m10 = 0
    for v in range(-half, half + 1):
        for u in range(-u_max[abs(v)], u_max[abs(v)] + 1):
            p = int(img[y + v, x + u])
            m01 += v * p; m10 += u * p
    return m01, m10


def orb_descriptor_f64(img, x, y, angle_deg, pattern, margin=1e-3):
    """(bits (256,) bool, sure (256,) bool): bit i = I(first point of pair i) < I(second), the pattern rotated by the angle in float64 and rounded to
    the nearest pixel; sure = both points of the pair further than `margin` from a rounding boundary in both coordinates."""
    a = np.deg2rad(np.float64(angle_deg))
    px, py = pattern[:, 0].astype(np.float64), pattern[:, 1].astype(np.float64)
    fx, fy = px * np.cos(a) - py * np.sin(a), px * np.sin(a) + py * np.cos(a)
    near = (np.abs(np.abs(fx - np.floor(fx)) - 0.5) <= margin) | (np.abs(np.abs(fy - np.floor(fy)) - 0.5) <= margin)
    val = img[y + np.rint(fy).astype(np.int64), x + np.rint(fx).astype(np.int64)].astype(np.int64)
    return val[0::2] < val[1::2], ~(near[0::2] | near[1::2])


def orb_level_size(cols, rows, scale_factor, level):
    """Size(cvRound(cols * scale), cvRound(rows * scale)), scale = 1.0f / (float)pow(scaleFactor, level)   orb.cpp:675-677"""
    scale = np.float32(1.0) / np.float32(float(np.float32(scale_factor)) ** level)
    return int(np.rint(np.float32(cols) * scale)), int(np.rint(np.float32(rows) * scale))


def feature_mask(bgr, a_x0, a_w, b_x0, b_w):
    x = np.arange(bgr.shape[1])
    band = ((x >= a_x0) & (x < a_x0 + a_w)) | ((x >= b_x0) & (x < b_x0 + b_w))
    return np.where(band[None, :] & bgr.any(axis=2), 255, 0).astype(np.uint8)
