"""Run on the GPU box: what an ORB call costs, at the rig's shapes -> a JSON-lines file (profiles/orb_batch.jsonl holds one run).
      python tools/time_orb_batch.py [OUT.jsonl]
ms_orb_detect_and_compute is ms_orb_detect_and_compute_batch with one view, so the two sides of a row are the same code:
  orb_batch    one batch of N views against N batch-of-one calls (the single entry point, view after view).  The difference over N - 1 is the fixed cost of a
               call: the table upload, the clear, the nlevels + 10 launches, the copy back and the synchronisation.
  orb_single   with MSSTITCH_LIB=<libmsstitch.so of another build, e.g. the parent commit's>: the single call of this tree's library against the single call of
               that one, in one process, for one 1080p view and one 288 x 216 view (where the fixed launches weigh most), with and without masks.
Per row: the outputs are compared bit for bit first; then 5 rounds, the two sides alternating, host clock around the synchronous calls (results on the host when
they return); medians.  Views: crops of one textured scene (tools/bench_features.py's), the masks its two overlap bands (400 pixels at 1080p).
python tools/time_orb_batch.py --trace K: nothing but K + 1 calls of the 6-view batch, for a kernel trace (the launches and synchronisations of one call are
the difference of two traces with different K, divided by the difference in K)."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "video-stitcher_amd"))
import numpy as np
import torch
import msstitch as ms


def textured(w, h, seed):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.float32)
    for s in (4, 8, 16, 32):
        g = rng.random((h // s + 2, w // s + 2)).astype(np.float32)
        img += np.kron(g, np.ones((s, s), np.float32))[:h, :w] * s
    img = (img - img.min()) / (img.max() - img.min()) * 255
    return img.astype(np.uint8)


def views(n, w, h):
    scene = textured(w + 97 * n, h, 5)
    return [torch.from_numpy(scene[:, 97 * v:97 * v + w].copy()).cuda() for v in range(n)]


def band_masks(n, w, h):
    band = 400 * w // 1920
    m = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    m[:, :band] = 255; m[:, -band:] = 255
    return [m.clone() for _ in range(n)]


def libraries():
    """(this tree's library, the one MSSTITCH_LIB names or None, its label without the path of the box)"""
    this = C.CDLL(ms.LIB_PATH)
    other = os.environ.get("MSSTITCH_LIB")
    if not other or os.path.realpath(other) == os.path.realpath(ms.LIB_PATH):
        return this, None, None
    return this, C.CDLL(other), os.path.relpath(os.path.realpath(other), os.path.realpath(ROOT))


class Calls:
    """two routes (0 and 1) through the C ABI over buffers made once: what is timed is the library, not the binding"""

    def __init__(self, grays, masks, nfeatures=2500):
        self.n, self.grays, self.masks = len(grays), grays, masks
        self.prm = ms.orb_params(nfeatures=nfeatures)
        self.cap = nfeatures + self.prm.nlevels // 2
        self.kp = [np.zeros((self.n, self.cap, 6), np.float32) for _ in range(2)]
        self.desc = [[torch.zeros((self.cap, 32), dtype=torch.uint8, device="cuda") for _ in grays] for _ in range(2)]
        self.cnt = [(C.c_int * self.n)() for _ in range(2)]
        self.gi = (ms.Image * self.n)(*[ms.img(g) for g in grays])
        self.mi = None if masks is None else (ms.Image * self.n)(*[ms.img(m) for m in masks])
        self.di = [(ms.Image * self.n)(*[ms.img(d) for d in ds]) for ds in self.desc]
        self.stream = ms._stream()
        self.fp = C.POINTER(C.c_float)

    @staticmethod
    def check(lib, rc):
        if rc < 0:
            lib.ms_last_error.restype = C.c_char_p
            raise ms.MsError("msstitch error %d: %s" % (rc, lib.ms_last_error().decode()))

    def batch(self, lib, route=0):
        self.check(lib, lib.ms_orb_detect_and_compute_batch(self.n, self.gi, self.mi, C.byref(self.prm), self.kp[route].ctypes.data_as(self.fp), self.cap, self.di[route],
                                                            self.cnt[route], self.stream))

    def singles(self, lib, route=1):
        for v in range(self.n):
            one = C.c_int(0)
            self.check(lib, lib.ms_orb_detect_and_compute(C.byref(self.gi[v]), None if self.mi is None else C.byref(self.mi[v]), C.byref(self.prm),
                                                          self.kp[route][v].ctypes.data_as(self.fp), self.cap, C.byref(self.di[route][v]), C.byref(one), self.stream))
            self.cnt[route][v] = one.value

    def equal(self):
        if list(self.cnt[0]) != list(self.cnt[1]):
            return False
        return all(self.kp[0][v, :c].tobytes() == self.kp[1][v, :c].tobytes() and torch.equal(self.desc[0][v][:c], self.desc[1][v][:c]) for v, c in enumerate(self.cnt[0]))


def clock(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


def alternate(c, a, b):
    """both sides once for the comparison, once more so that both scratch routes are warm, then 5 alternating rounds: (equal, runs of a, runs of b)"""
    a(); b(); torch.cuda.synchronize()
    same = c.equal()
    a(); b()
    ra, rb = [], []
    for _ in range(5):
        ra.append(clock(a)); rb.append(clock(b))
    return same, ra, rb


def measure_batch(this, n, w, h, masked):
    c = Calls(views(n, w, h), band_masks(n, w, h) if masked else None)
    same, b, l = alternate(c, lambda: c.batch(this), lambda: c.singles(this))
    rec = {"what": "orb_batch", "views": n, "size": [w, h], "masks": masked, "orb": [2500, 1.2, 8], "keypoints": list(c.cnt[0]), "bit_equal_to_batch_of_one_calls": same,
           "batch_call_ms": sorted(b)[2], "batch_call_runs_ms": b, "batch_of_one_calls_ms": sorted(l)[2], "batch_of_one_calls_runs_ms": l}
    rec["batch_over_batch_of_one_calls"] = rec["batch_call_ms"] / rec["batch_of_one_calls_ms"]
    if n > 1:
        rec["fixed_cost_per_call_ms"] = (rec["batch_of_one_calls_ms"] - rec["batch_call_ms"]) / (n - 1)
    rec["launches"] = "nlevels + 10 = 18"; rec["synchronisations"] = 1
    return rec


def measure_single(this, other, label, w, h, masked):
    c = Calls(views(1, w, h), band_masks(1, w, h) if masked else None)
    same, a, b = alternate(c, lambda: c.singles(this, 0), lambda: c.singles(other, 1))
    rec = {"what": "orb_single", "views": 1, "size": [w, h], "masks": masked, "orb": [2500, 1.2, 8], "keypoints": list(c.cnt[0]), "other_library": label,
           "bit_equal_to_other_library": same, "single_call_ms": sorted(a)[2], "single_call_runs_ms": a, "other_single_call_ms": sorted(b)[2], "other_single_call_runs_ms": b}
    rec["single_over_other_single"] = rec["single_call_ms"] / rec["other_single_call_ms"]
    return rec


def main():
    this, other, label = libraries()
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        c = Calls(views(6, 1920, 1080), None)
        torch.cuda.synchronize()
        for _ in range(int(sys.argv[2]) + 1):
            c.batch(this)
        return
    with open(sys.argv[1] if len(sys.argv) > 1 else "orb_batch.jsonl", "w") as f:
        def put(rec, keys):
            f.write(json.dumps(rec) + "\n"); f.flush()
            print(json.dumps({k: rec[k] for k in ("what", "views", "size", "masks") + keys if k in rec}))
        for n, w, h, masked in ((6, 1920, 1080, False), (6, 1920, 1080, True), (16, 1920, 1080, False), (16, 1920, 1080, True), (8, 640, 480, False), (1, 1920, 1080, False)):
            put(measure_batch(this, n, w, h, masked), ("bit_equal_to_batch_of_one_calls", "batch_call_ms", "batch_of_one_calls_ms", "fixed_cost_per_call_ms"))
        for w, h, masked in ((1920, 1080, False), (1920, 1080, True), (288, 216, False), (288, 216, True)) if other is not None else ():
            put(measure_single(this, other, label, w, h, masked), ("other_library", "bit_equal_to_other_library", "single_call_ms", "other_single_call_ms"))


if __name__ == "__main__":
    main()
