"""The panorama frames and views of the virtual-camera GPU tests (tests/test_reproject_gpu.py), restated for tests/test_reproject_aa_gpu.py, and the 38 x 22
views its sampler tests choose for their footprints."""
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
SRC_SIZE = (96, 48)                                                             # cols x rows of every frame's image
FISH_ALL = ("fisheye", (-0.02, 0.003, 0.0, 0.0), 100.0)                         # 37 x 21 at f = 18.5: every pixel is seen
BROWN_60 = ("brown", L.BROWN[1], 60.0)                                          # with f = 8 the corners lie past 60 degrees: unseen
VIEWS = {
    "pinhole": RR.look_at(200, 35, 10, 90, 37, 21),
    "up": RR.look_at(0, 90, 0, 90, 16, 16),
    "down": RR.look_at(0, -90, 0, 90, 16, 16),
    "seam": RR.look_at(180, 0, 0, 60, 33, 9),
    "fisheye": RR.look_at(40, -20, 5, 90, 37, 21, lens=FISH_ALL),
    "brown": dict(kind="camera", w=37, h=21, K=np.float32([[8, 0, 18], [0, 8, 10], [0, 0, 1]]), R=np.float32(RR.look_at_R(-30, 15, 0)), lens=BROWN_60),
    "surface": dict(kind="surface", w=96, h=48, R=np.float32(RR.look_at_R(0, 0, 10)), proj="sph", scale=SCALE, tl_u=-48, tl_v=0),
    "one": RR.look_at(15, 5, 0, 40, 1, 1),
    "column": RR.look_at(-60, 20, 0, 70, 1, 9),
}
# one size, 38 x 22 (even: I420 too), by what rho does on the 96 x 48 frames (15 pixels per radian)
AA_VIEWS = {
    "fine": RR.look_at(30, 5, 0, 20, 38, 22),          # rho below 1 everywhere: the one-level path
    "wide": RR.look_at(-40, 10, 5, 120, 38, 22),       # rho from 0.6 to 1.4 (levels 0 and 1); with footprint_scale 4, 2.3 to 5.6 (levels 1 to 3)
    "up": RR.look_at(0, 90, 0, 100, 38, 22),
    "down": RR.look_at(0, -90, 20, 100, 38, 22),
    "seam": RR.look_at(180, -5, 0, 100, 38, 22),
}
