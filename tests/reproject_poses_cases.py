"""The frames, views and buffers the tests of ms_reproject_poses share (tests/test_reproject_poses_abi.py, tests/test_reproject_poses_gpu.py): the three 96 x 48
panorama frames and seven views tests/test_reproject_gpu.py pins ms_build_view_maps and ms_reproject on, one 67 x 35 pinhole that spans several tiles in both
directions with ragged edges, and the poses every run includes."""
import math

import numpy as np

import lens_ref as L
import reproject_ref as RR

SCALE = float(np.float32(96 / (2 * math.pi)))
FRAMES = {
    "sph": dict(proj="sph", scale=SCALE, u0=-48, v0=0, wrap=96, clamp=1),       # a 96 x 48 equirect: the full turn, pole to pole
    "cyl": dict(proj="cyl", scale=SCALE, u0=-48, v0=-24, wrap=96, clamp=0),
    "roi": dict(proj="sph", scale=SCALE, u0=-31, v0=7, wrap=0, clamp=0),        # a pano ROI: no wrap
}
SRC_COLS, SRC_ROWS = 96, 48
FISH_ALL = ("fisheye", (-0.02, 0.003, 0.0, 0.0), 100.0)                         # 37 x 21 at f = 18.5: theta_d <= 1.12 rad, every pixel is seen
BROWN_60 = ("brown", L.BROWN[1], 60.0)                                          # with f = 8 the corners lie past 60 degrees
VIEWS = {
    "pinhole": RR.look_at(200, 35, 10, 90, 37, 21),
    "up": RR.look_at(0, 90, 0, 90, 16, 16),
    "down": RR.look_at(0, -90, 0, 90, 16, 16),
    "seam": RR.look_at(180, 0, 0, 60, 33, 9),
    "fisheye": RR.look_at(40, -20, 5, 90, 37, 21, lens=FISH_ALL),
    "brown": dict(kind="camera", w=37, h=21, K=np.float32([[8, 0, 18], [0, 8, 10], [0, 0, 1]]), R=np.float32(RR.look_at_R(-30, 15, 0)), lens=BROWN_60),
    "surface": dict(kind="surface", w=96, h=48, R=np.float32(RR.look_at_R(0, 0, 10)), proj="sph", scale=SCALE, tl_u=-48, tl_v=0),      # the whole equirect under a roll
    "tiles": RR.look_at(75, -10, 20, 100, 67, 35),      # more than one 64 x 16 (BGR) tile each way, neither side a multiple of the tile or of a lane's four pixels
}
# even-sized forms for I420 (a lane owns a 2 x 2 block; tiles are 32 x 32): a pinhole over 2 x 2 tiles with ragged edges, a fisheye, a surface
VIEWS_EVEN = {
    "pinhole": RR.look_at(200, 35, 10, 90, 38, 22),
    "tiles": RR.look_at(75, -10, 20, 100, 66, 34),
    "fisheye": RR.look_at(40, -20, 5, 90, 38, 22, lens=FISH_ALL),
    "brown": dict(kind="camera", w=38, h=22, K=np.float32([[8, 0, 18], [0, 8, 10], [0, 0, 1]]), R=np.float32(RR.look_at_R(-30, 15, 0)), lens=BROWN_60),
    "surface": VIEWS["surface"],
}

# poses every run includes: the optical axis (a pinhole's; a surface view's u = 0 column) on the +-pi seam and on both poles
FIXED_POSES = [RR.look_at_R(180, 0, 0), RR.look_at_R(-180, 0, 33), RR.look_at_R(0, 90, 0), RR.look_at_R(17, -90, 0)]


def random_poses(rng, n):
    """n rotations (n, 9) float32: the fixed poses first (as many as fit), then look_at_R of random angles"""
    out = [np.float32(R).reshape(9) for R in FIXED_POSES[:n]]
    while len(out) < n:
        out.append(np.float32(RR.look_at_R(rng.uniform(-180, 180), rng.uniform(-90, 90), rng.uniform(-180, 180))).reshape(9))
    return np.stack(out)


def with_R(view, R9):
    v = dict(view)
    v["R"] = np.float32(R9).reshape(3, 3)
    return v


def random_sources(rng, n, cols=SRC_COLS, rows=SRC_ROWS):
    return [rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) for _ in range(n)]


def shelf_pack(sizes, x0, y0, max_w, even=False):
    """rectangles that touch but do not overlap: shelves left to right, top to bottom"""
    out, x, y, shelf_h = [], x0, y0, 0
    for w, h in sizes:
        if x + w > x0 + max_w and x > x0:
            x, y, shelf_h = x0, y + shelf_h, 0
        out.append((x, y))
        x += w
        shelf_h = max(shelf_h, h)
    assert not even or all(v % 2 == 0 for p in out for v in p)
    return out, y + shelf_h


def expect_i420(np_ref, want_flat, idx, W, H, rect, bgr):
    """write ms_bgr_to_i420 of `bgr` (the rectangle's pixels) into the three planes' sub-rectangles of the contiguous I420 frame whose flat indices are idx"""
    x, y, w, h = rect
    planes = np_ref.bgr_to_i420(bgr)
    flat = idx.reshape(-1)
    Y = flat[:W * H].reshape(H, W); U = flat[W * H:W * H + (W // 2) * (H // 2)].reshape(H // 2, W // 2); V = flat[W * H + (W // 2) * (H // 2):].reshape(H // 2, W // 2)
    want_flat[Y[y:y + h, x:x + w]] = planes[:h]
    chroma = planes.reshape(-1)[w * h:]
    want_flat[U[y // 2:(y + h) // 2, x // 2:(x + w) // 2]] = chroma[:(w // 2) * (h // 2)].reshape(h // 2, w // 2)
    want_flat[V[y // 2:(y + h) // 2, x // 2:(x + w) // 2]] = chroma[(w // 2) * (h // 2):].reshape(h // 2, w // 2)
