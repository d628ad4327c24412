"""numpy statement of the antialiased virtual cameras of include/ms_stitch.h section 5 (ms_pano_mips_layout's sizes, ms_build_pano_mips, ms_build_view_footprint,
ms_reproject_aa): the reference of tests/test_reproject_aa_abi.py and tests/test_reproject_aa_gpu.py.  Written from the header's text; the fp32 chains go through
np_ref.fmaf32, the footprints are float64.  Nothing here calls the library."""
import math

import numpy as np

import np_ref
import reproject_ref as RR

F32 = np.float32
MAX_LEVELS = 6


# ---- the mip chain ------------------------------------------------------------------------------------------------------------------------------------
def level_sizes(cols, rows, levels):
    """[(cols_l, rows_l)] for l = 1..levels: halved, rounded up"""
    out = []
    for _ in range(levels):
        cols, rows = (cols + 1) // 2, (rows + 1) // 2
        out.append((cols, rows))
    return out


def mip_down(p):
    """one level: (p(2x, 2y) + p(2x+1, 2y) + p(2x, 2y+1) + p(2x+1, 2y+1) + 2) >> 2 per channel, an index past the last column or row reading the last one"""
    h, w = p.shape[:2]
    ys, xs = np.arange((h + 1) // 2) * 2, np.arange((w + 1) // 2) * 2
    y1, x1 = np.minimum(ys + 1, h - 1), np.minimum(xs + 1, w - 1)
    q = p.astype(np.int64)
    s = q[ys][:, xs] + q[ys][:, x1] + q[y1][:, xs] + q[y1][:, x1] + 2
    return (s >> 2).astype(np.uint8)


def mip_chain(src, levels):
    """[level 0 (the source itself), level 1, ..., level `levels`], cascaded: each from the stored bytes of the one before"""
    out = [np.asarray(src, np.uint8)]
    for _ in range(levels):
        out.append(mip_down(out[-1]))
    return out


# ---- the footprint -----------------------------------------------------------------------------------------------------------------------------------
def seen_entries(mx, my):
    mx, my = np.asarray(mx, F32), np.asarray(my, F32)
    return ~((mx == -1) & (my == -1)) & np.isfinite(mx) & np.isfinite(my)


def footprint(frame, mx, my, footprint_scale=1.0):
    """rho in float64 (the device rounds it to float once): the side, in level-0 panorama pixels, of the patch a view pixel covers"""
    mx, my = np.asarray(mx, F32), np.asarray(my, F32)
    h, w = mx.shape
    seen = seen_entries(mx, my)
    X, Y = np.where(seen, mx, 0).astype(np.float64), np.where(seen, my, 0).astype(np.float64)
    pad = lambda a, v: np.pad(a, 1, constant_values=v)
    Xp, Yp, Sp = pad(X, 0.0), pad(Y, 0.0), pad(seen, False)
    W = float(frame["wrap"])
    if frame["proj"] == "sph":
        s = np.sin(np.minimum(np.maximum((Y + float(frame["v0"])) / float(F32(frame["scale"])), 0.0), math.pi))
    else:
        s = np.ones((h, w))

    def step(sx, sy):
        f = (slice(1 + sy, 1 + sy + h), slice(1 + sx, 1 + sx + w))
        b = (slice(1 - sy, 1 - sy + h), slice(1 - sx, 1 - sx + w))
        dx = np.where(Sp[f], Xp[f] - X, np.where(Sp[b], X - Xp[b], 0.0))
        dy = np.where(Sp[f], Yp[f] - Y, np.where(Sp[b], Y - Yp[b], 0.0))
        if W > 0:
            dx = dx - W * np.floor(dx / W + 0.5)
        dx = dx * s
        return np.hypot(dx, dy)
    rho = float(footprint_scale) * np.maximum(step(1, 0), step(0, 1))
    return np.where(seen, rho, 0.0)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------------------
def level_of(rho, levels):
    """(l, t) of a float32 footprint: !(r > 1) -> (0, 0); r >= 2^levels -> (levels, 0); else l = the float's exponent, t = fmaf(r, 2^-l, -1)"""
    r = np.asarray(rho, F32)
    with np.errstate(invalid="ignore"):
        low = ~(r > 1)
        high = r >= F32(2.0 ** levels)
    safe = np.where(low | high, F32(1.5), r)
    _, e = np.frexp(safe)               # safe = m 2^e, m in [0.5, 1)
    l = np.where(low, 0, np.where(high, levels, e - 1)).astype(np.int64)
    t = np_ref.fmaf32(safe, np.exp2(-(e - 1).astype(np.float64)).astype(F32), F32(-1))
    return l, np.where(low | high, F32(0), t).astype(F32)


def chain_linear(src, mx, my):
    """np_ref.remap_linear's taps, weights and fma chain on `src` WITHOUT the saturation: float32 (h, w, 3)"""
    h, w = src.shape[:2]
    with np.errstate(all="ignore"):
        x1 = np.floor(mx).astype(np.int64); y1 = np.floor(my).astype(np.int64)
        x2, y2 = x1 + 1, y1 + 1
        f = F32
        wts = [((x2.astype(f) - mx) * (y2.astype(f) - my)), ((mx - x1.astype(f)) * (y2.astype(f) - my)),
               ((x2.astype(f) - mx) * (my - y1.astype(f))), ((mx - x1.astype(f)) * (my - y1.astype(f)))]
        taps = [(y1, x1), (y1, x2), (y2, x1), (y2, x2)]
        out = np.zeros(mx.shape + (3,), F32)
        for (yy, xx), wt in zip(taps, wts):
            inb = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            v = np.where(inb[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0).astype(F32)
            out = np_ref.fmaf32(v, wt.astype(F32)[..., None], out)
    return out


def level_coords(m, k):
    """X_k = fmaf(X, 2^-k, 2^-(k+1) - 0.5f)"""
    return np_ref.fmaf32(np.asarray(m, F32), F32(2.0 ** -k), F32(2.0 ** -(k + 1) - 0.5))


def level_sample(img, mx, my, k, wrap, clamp):
    """C_k: the unsaturated chain of ms_reproject on image level k -- the extended-source route with that level's size"""
    return chain_linear(RR.extend(img, wrap, clamp), RR.shifted(level_coords(mx, k)), RR.shifted(level_coords(my, k)))


def reproject_aa_view(chain, mx, my, rho, wrap, clamp):
    """ms_reproject_aa of one view and one frame: chain = mip_chain(src, levels); uint8 (h, w, 3)"""
    levels = len(chain) - 1
    l, t = level_of(rho, levels)
    C = np.stack([level_sample(chain[k], mx, my, k, wrap, clamp) for k in range(levels + 1)])
    pick = lambda idx: np.take_along_axis(C, np.broadcast_to(idx[None, ..., None], (1,) + C.shape[1:]), 0)[0]
    c0, c1 = pick(l), pick(np.minimum(l + 1, levels))
    with np.errstate(all="ignore"):
        mixed = np_ref.fmaf32(t[..., None], (c1 - c0).astype(F32), c0)
    return np_ref.sat_u8(np.where((t == 0)[..., None], c0, mixed))


# ---- the quality scene: stripes on the sphere ------------------------------------------------------------------------------------------------------------
STRIPE_PERIOD, STRIPE_TILT = 3.0, math.radians(30.0)


def stripes(X, Y):
    """the analytic scene at panorama coordinates (float64, pixels of the level-0 equirect): stripes of STRIPE_PERIOD pixels, tilted by STRIPE_TILT"""
    return 127.5 + 127.5 * np.sin(2 * math.pi / STRIPE_PERIOD * (X * math.cos(STRIPE_TILT) + Y * math.sin(STRIPE_TILT)))


def striped_equirect(cols, rows):
    """the scene point-sampled at the pixel centres of a cols x rows equirect (cols a multiple of the stripes' horizontal period would close the turn; 384 is not
    asked to: the seam is not in the test views)"""
    x, y = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    v = np.rint(stripes(x, y)).astype(np.uint8)
    return np.repeat(v[..., None], 3, 2)


def supersampled_truth(frame, view, n=8):
    """what the view's pixels should show: the mean of the analytic scene over n x n sub-pixel rays of every pixel"""
    h, w = view["h"], view["w"]
    offs = (np.arange(n) + 0.5) / n - 0.5
    acc = np.zeros((h, w))
    R = F32(view["R"]).astype(np.float64).reshape(3, 3)
    S = float(F32(frame["scale"]))
    x0 = np.arange(w, dtype=np.float64)[None, :] * np.ones((h, 1)); y0 = np.arange(h, dtype=np.float64)[:, None] * np.ones((1, w))
    for oy in offs:
        for ox in offs:
            c0, c1, c2, _ = RR.unproject(F32(view["K"]), view["lens"], x0 + ox, y0 + oy)
            d = [R[k, 0] * c0 + R[k, 1] * c1 + R[k, 2] * c2 for k in range(3)]
            X = S * np.arctan2(d[0], d[2]) - frame["u0"]
            Y = S * np.arctan2(np.hypot(d[0], d[2]), -d[1]) - frame["v0"]
            acc += stripes(X, Y)
    return acc / (n * n)


def quality(view, levels=4, cols=384, rows=192):
    """(RMS error of the antialiased reference, RMS error of the point-sampled reference, (min, max) footprint) of `view` on the striped equirect"""
    frame = dict(proj="sph", scale=float(F32(cols / (2 * math.pi))), u0=-cols // 2, v0=0, wrap=cols, clamp=1)
    src = striped_equirect(cols, rows)
    X, Y, seen = RR.view_maps(frame, view)
    assert seen.all()
    mx, my = F32(X), F32(Y)
    mx = np.where(mx == F32(cols), F32(0), mx)
    rho = F32(footprint(frame, mx, my))
    truth = supersampled_truth(frame, view)
    aa = reproject_aa_view(mip_chain(src, levels), mx, my, rho, True, True)[..., 0].astype(np.float64)
    point = RR.reproject_view(src, mx, my, True, True)[..., 0].astype(np.float64)
    rms = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
    return rms(aa), rms(point), (float(rho.min()), float(rho.max()))
