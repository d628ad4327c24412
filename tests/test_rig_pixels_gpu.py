"""Rig rotation refinement end to end from pixels, and through the host application.

8. a scene fixed on the sphere, rendered through a rig with two views off the ring; warped with the ideal ring, then the library's own front end (ORB, 2-NN with
   ratio test, RANSAC homographies between neighbours) and ms_refine_rig
9. stitch_app --solve-mesh --rig-error 2:1.5:1:0 --refine-rig"""
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import rig_ref as rr
import synth
from helpers import to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "video-stitcher_amd", "stitch_app")

N, W, H, HFOV, OUT_W = 6, 640, 480, 90.0, 2048


def render(R, scale):
    """BGR view of a texture of random grey blocks fixed on the sphere (blocks of 32 warper pixels, a smooth ripple inside each), through the camera rotation R"""
    f = (W / 2.0) / math.tan(math.radians(HFOV) / 2.0)
    x, y = np.meshgrid((np.arange(W) - W / 2.0) / f, (np.arange(H) - H / 2.0) / f)
    d = np.stack([x, y, np.ones_like(x)], -1) @ R.T
    u = np.arctan2(d[..., 0], d[..., 2]) + math.pi
    v = math.pi - np.arccos(d[..., 1] / np.linalg.norm(d, axis=-1))
    cell = 32.0 / scale
    cu, cv = np.floor(u / cell).astype(np.int64), np.floor(v / cell).astype(np.int64)
    fu, fv = u / cell - cu, v / cell - cv
    out = np.empty((H, W, 3), np.uint8)
    for ch in range(3):
        h = ((cu * 73856093) ^ (cv * 19349663) ^ (ch * 83492791)).astype(np.uint64) & 0xffffffff
        h ^= h >> 13; h = (h * 0x5bd1e995) & 0xffffffff; h ^= h >> 15
        val = 40.0 + ((h >> 8) & 0xff).astype(np.float64) * 175.0 / 255.0 + 18.0 * np.sin(2 * math.pi * (fu + 0.3 * ch)) * np.sin(2 * math.pi * fv)
        out[..., ch] = np.clip(np.rint(val), 1, 255)
    return out


def true_rig():
    """the ring with view 2 off by 1.5 degrees in yaw and 1 in pitch, view 4 by 1 degree in roll (in the cameras' own frames)"""
    R = rr.ring(N)
    R[2] = R[2] @ rr.rot_y(math.radians(1.5)) @ rr.exp_so3(np.array([math.radians(1.0), 0, 0]))
    R[4] = R[4] @ rr.exp_so3(np.array([0, 0, math.radians(1.0)]))
    return R


def pixels_case(ms):
    """the whole pipeline; returns the figures the test asserts on"""
    scale = synth.warp_scale(OUT_W)
    Rt = true_rig()
    comp = ms.Compositor(N, (W, H), ms.PROJ_SPHERICAL, scale, num_bands=3, out_size=(OUT_W, OUT_W // 2))
    cams = [synth.camera(N, W, H, HFOV, v) for v in range(N)]
    for v in range(N):
        comp.set_camera(v, *cams[v])
    comp.build_maps()
    feats = []
    for v in range(N):
        xm, ym = comp.maps(v)
        warped = ms.remap(to_dev(render(Rt[v], scale)), xm.contiguous(), ym.contiguous())
        mask = ((warped.max(dim=2).values > 0).to(torch.uint8) * 255).contiguous()
        feats.append(ms.orb_detect_and_compute(ms.bgr_to_gray(warped), mask, nfeatures=2500) + (warped.shape,))
    lists = [[] for _ in range(N)]
    inliers = []
    for i, j in rr.ring_pairs(N):
        (k1, d1, s1), (k2, d2, s2) = feats[i], feats[j]
        idx, dist = ms.knn_match_hamming2(d1, d2)
        good = [q for q in range(len(k1)) if idx[q, 1] >= 0 and dist[q, 0] < 0.7 * dist[q, 1]]
        src = np.array([[k1[q, 0] - s1[1] * 0.5, k1[q, 1] - s1[0] * 0.5] for q in good], np.float32).reshape(-1, 2)
        dst = np.array([[k2[idx[q, 0], 0] - s2[1] * 0.5, k2[idx[q, 0], 1] - s2[0] * 0.5] for q in good], np.float32).reshape(-1, 2)
        Hm, inl = (None, np.zeros(0, np.uint8)) if len(good) < 4 else ms.find_homography_ransac(src, dst)
        inliers.append(int(inl.sum()) if Hm is not None else 0)
        for n, q in enumerate(good):
            if Hm is not None and inl[n]:
                lists[i].append((k1[q, 0], k1[q, 1], k2[idx[q, 0], 0], k2[idx[q, 0], 1], j))
    prm = ms.rig_refine_default_params(huber_rad=2.0 / scale)
    out = dict(scale=scale, inliers=inliers, min_pair_matches=prm.min_pair_matches)
    if min(inliers) >= prm.min_pair_matches:
        R, info = comp.refine_rig(lists, prm)
        R0 = np.array([c[1] for c in cams], np.float64)
        corner = [comp.view_geom(v).roi.tuple()[:2] for v in range(N)]
        rays = [(v, m[4], rr.warper_ray(rr.SPHERICAL, scale, R0[v], corner[v][0] + float(m[0]), corner[v][1] + float(m[1])),
                 rr.warper_ray(rr.SPHERICAL, scale, R0[m[4]], corner[m[4]][0] + float(m[2]), corner[m[4]][1] + float(m[3]))) for v in range(N) for m in lists[v]]
        Rr, ri = rr.refine(R0, rays, huber_rad=2.0 / scale)
        want = rr.expected(R0, Rt, 0)
        out.update(info=info, ref_info=ri, to_reference_rad=max(rr.angle(R[v].astype(np.float64), Rr[v].astype(np.float32).astype(np.float64)) for v in range(N)),
                   before_px=[rr.angle(R0[v], want[v]) * scale for v in range(N)], after_px=[rr.angle(R[v].astype(np.float64), want[v]) * scale for v in range(N)])
    comp.close()
    return out


def test_refinement_from_pixels(ms, cuda):
    """Measured on MI355X (profiles/rig_refine.jsonl, "rig_refine_pixels"): 23 to 114 RANSAC inliers a pair (401 in all), views 2 and 4 start 10.26 and 5.69 warped
    pixels from the truth, and the six views end 0, 0.24, 0.36, 0.40, 0.39 and 0.24 pixels from it: ORB's localisation on this scene is good for well under a pixel."""
    r = pixels_case(ms)
    print("inliers per neighbouring pair: %s" % r["inliers"])
    assert min(r["inliers"]) >= r["min_pair_matches"], "a neighbouring pair delivered %d inliers, fewer than min_pair_matches: %s" % (min(r["inliers"]), r["inliers"])
    print("angle to the truth in warped pixels, before: %s" % ["%.3f" % x for x in r["before_px"]])
    print("angle to the truth in warped pixels, after:  %s" % ["%.3f" % x for x in r["after_px"]])
    print("device against the reference: %.3e rad; info %s; reference %s" % (r["to_reference_rad"], r["info"], r["ref_info"]))
    assert max(r["before_px"]) >= 6.0
    assert r["to_reference_rad"] <= 1e-10
    assert r["info"]["cost_final"] <= r["info"]["cost_initial"]
    assert max(r["after_px"]) <= 1.0, "a view ends %.3f warped pixels from the truth" % max(r["after_px"])


def test_stitch_app_refines_an_injected_rig_error(ms, cuda, tmp_path):
    """stitch_app --solve-mesh --rig-error 2:1.5:1:0 --refine-rig: exits 0; its rig_refine line reports view 2 within one warped pixel of the injected rotation"""
    dump = str(tmp_path / "pano.bin")
    p = subprocess.run([APP, "--dump", dump, "--size", "960x540", "--out", "1920x960", "--frames", "40", "--solve-mesh", "--rig-error", "2:1.5:1:0", "--refine-rig"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("rig_refine: ")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0][len("rig_refine: "):])
    print(lines[0])
    px = r["warp_scale"]
    assert r["pairs_used"] == 6 and r["pairs_ignored"] == 0 and r["matches_used"] >= 6 * 4 and r["cost_final"] <= r["cost_initial"]
    assert r["angle_before_rad"][2] * px > 6.0                       # sqrt(1.5^2 + 1^2) degrees at this scale: 9.6 px
    assert r["angle_to_truth_rad"][2] * px <= 1.0, r
    info = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert info["frames"] == 40 and info["cpw"] is True
    got = np.fromfile(dump, np.uint8).reshape(960, 1920, 3)
    assert (got.max(axis=2) > 0).mean() > 0.25
