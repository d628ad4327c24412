"""Inputs of the ms_dp_seams tests (tests/test_dp_seams_abi.py without a GPU, tests/test_dp_seams_gpu.py with one).  numpy only; every case is a pure function of its
name (fixed seeds).  A case is (rois, images, masks): rois = [(x, y, w, h)], images uint8 (h, w, 3), masks uint8 (h, w).

Layouts: every layout of calib_cases.VORONOI_CASES, three times --
  random    seeded random images: costs all over 0 .. 765, few ties
  same      every view cut from one canvas: every cost on B is 0, so the tie rules decide every step and the end column
  plateau   views made of flat blocks of two grey levels: pair costs take two or three values in plateaus, ties along every plateau
and two-view pairs whose overlap is exactly w x h, for the widths at which k_dp_seam changes what a lane does: 1, 2, 63 / 64 / 65 (one wave), 255 / 256 / 257 (the
workgroup: one position per lane, then two), 1100 (five positions per lane); heights 1 and 2; planes of more than one slab of 32768 cells (1100 x 70: slabs of 29
rows; 4096 x 20: the widest plane, slabs of 8 rows); the same as horizontal seams; view i on the second side (d < 0) for both orientations."""
import zlib

import numpy as np

import calib_cases

KINDS = ("random", "same", "plateau")
SLAB_CELLS = 32768


def _rng(name):
    return np.random.default_rng(zlib.crc32(("dp:" + name).encode()))


def _canvas(rois):
    x0, y0 = min(r[0] for r in rois), min(r[1] for r in rois)
    x1, y1 = max(r[0] + r[2] for r in rois), max(r[1] + r[3] for r in rois)
    return x0, y0, x1 - x0, y1 - y0


def images_for(name, rois, kind):
    rng = _rng(name + ":" + kind)
    if kind == "random":
        return [rng.integers(0, 256, size=(r[3], r[2], 3)).astype(np.uint8) for r in rois]
    if kind == "same":
        cx, cy, cw, ch = _canvas(rois)
        world = rng.integers(0, 256, size=(ch, cw, 3)).astype(np.uint8)
        return [np.ascontiguousarray(world[r[1] - cy:r[1] - cy + r[3], r[0] - cx:r[0] - cx + r[2]]) for r in rois]
    assert kind == "plateau"
    out = []
    for r in rois:
        by, bx = int(rng.integers(3, 8)), int(rng.integers(3, 8))
        blocks = rng.choice(np.array([60, 100], np.uint8), size=(r[3] // by + 1, r[2] // bx + 1))
        img = np.kron(blocks, np.ones((by, bx), np.uint8))[:r[3], :r[2]]
        out.append(np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2)))
    return out


def _layout_case(layout, kind):
    rois, masks = calib_cases.voronoi_case(layout)
    return rois, images_for(layout, rois, kind), masks


def _pair(name, w, h, horizontal=False, i_second=False, full=False):
    """two views whose overlap is exactly w x h (before `horizontal` transposes the layout), side by side: the centroids differ along x alone"""
    rng = _rng(name)
    e0, e1 = int(rng.integers(12, 20)), int(rng.integers(12, 20))
    ox, oy = int(rng.integers(-30, 10)), int(rng.integers(-30, 10))
    rois = [(ox, oy, e0 + w, h), (ox + e0, oy, w + e1, h)]
    if horizontal:
        rois = [(r[1], r[0], r[3], r[2]) for r in rois]
    if i_second:
        rois.reverse()
    masks = [calib_cases._full(r) for r in rois]
    if not full:        # small holes: the two centroids lie only 10 pixels apart along the seam's normal whatever the overlap's size, and the case's name promises their order
        for m in masks:
            for _ in range(3):
                hh, ww = int(rng.integers(1, min(5, m.shape[0]) + 1)), int(rng.integers(1, min(5, m.shape[1]) + 1))
                y, x = int(rng.integers(0, m.shape[0] - hh + 1)), int(rng.integers(0, m.shape[1] - ww + 1))
                m[y:y + hh, x:x + ww] = 0
    return rois, images_for(name, rois, "random"), masks


def _builders():
    b = {}
    for layout in calib_cases.VORONOI_CASES:
        for kind in KINDS:
            b["%s/%s" % (layout, kind)] = lambda n, layout=layout, kind=kind: _layout_case(layout, kind)
    for w in (1, 2, 63, 64, 65, 255, 256, 257):
        b["v_w%d" % w] = lambda n, w=w: _pair(n, w, 9)
        b["h_w%d" % w] = lambda n, w=w: _pair(n, w, 9, horizontal=True)
    for h in (1, 2):
        b["v_65x%d" % h] = lambda n, h=h: _pair(n, 65, h)
        b["h_65x%d" % h] = lambda n, h=h: _pair(n, 65, h, horizontal=True)
    b["v_1x1"] = lambda n: _pair(n, 1, 1, full=True)
    b["v_1100x7"] = lambda n: _pair(n, 1100, 7)
    b["v_1100x70_slabs"] = lambda n: _pair(n, 1100, 70)
    b["h_1100x70_slabs"] = lambda n: _pair(n, 1100, 70, horizontal=True)
    b["v_4096x20_slabs"] = lambda n: _pair(n, 4096, 20)
    b["h_4096x3"] = lambda n: _pair(n, 4096, 3, horizontal=True)
    b["v_40x900_slabs"] = lambda n: _pair(n, 40, 900)            # a tall, narrow plane: slabs of 819 rows
    b["v_i_second"] = lambda n: _pair(n, 37, 23, i_second=True)
    b["h_i_second"] = lambda n: _pair(n, 37, 23, horizontal=True, i_second=True)
    b["v_i_second_slabs"] = lambda n: _pair(n, 300, 120, i_second=True)
    return b


_CASES = _builders()
CASES = list(_CASES)
LAYOUT_CASES = [c for c in CASES if "/" in c]
PAIR_CASES = [c for c in CASES if "/" not in c]
# what a pair case's name promises: (horizontal, first)
PAIR_ORIENTATION = {c: (c.startswith("h_"), 1 if "i_second" in c else 0) for c in PAIR_CASES}
MULTI_SLAB_CASES = [c for c in PAIR_CASES if c.endswith("_slabs")]


def case(name):
    rois, imgs, masks = _CASES[name](name)
    return ([tuple(int(v) for v in r) for r in rois], [np.ascontiguousarray(i, np.uint8) for i in imgs], [np.ascontiguousarray(m, np.uint8) for m in masks])


# ---- the parallax scene: one background seen by both views, and an object only view 1 shows, standing in the middle of the overlap --------------------------
def parallax_scene():
    H = 64
    rois = [(0, 0, 100, H), (52, 0, 100, H)]
    rng = _rng("parallax")
    world = rng.integers(60, 201, size=(H, 152, 3))
    imgs = []
    for r in rois:
        v = world[:, r[0]:r[0] + r[2]] + rng.integers(-2, 3, size=(H, r[2], 3))
        imgs.append(np.clip(v, 0, 255).astype(np.uint8))
    imgs[1][20:44, 16:32] = 250
    return rois, [np.ascontiguousarray(i) for i in imgs], [calib_cases._full(r) for r in rois]
