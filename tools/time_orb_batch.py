"""Run on the GPU box: ms_orb_detect_and_compute_batch against the loop of ms_orb_detect_and_compute calls it replaces, at the rig's shapes ->
a JSON-lines file (profiles/orb_batch.jsonl holds one run).      python tools/time_orb_batch.py [OUT.jsonl]
Per shape: the outputs are compared bit for bit first; then 5 rounds, the batch and the loop alternating, host clock around the synchronous calls (results on the
host when they return); medians.  Views: crops of one textured scene (tools/bench_features.py's), the masks its two 400-pixel overlap bands.
python tools/time_orb_batch.py --trace K: nothing but K + 1 calls of the 6-view batch, for a kernel trace (the launches and synchronisations of one call are
the difference of two traces with different K, divided by the difference in K)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "video-stitcher_amd"))
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
    m = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    m[:, :400] = 255; m[:, -400:] = 255
    return [m.clone() for _ in range(n)]


class Calls:
    """both routes through the C ABI over buffers made once: what is timed is the library, not the binding"""

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
        self.lib, self.stream = ms.load(), ms._stream()
        self.fp = C.POINTER(C.c_float)

    def batch(self):
        ms._chk(self.lib.ms_orb_detect_and_compute_batch(self.n, self.gi, self.mi, C.byref(self.prm), self.kp[0].ctypes.data_as(self.fp), self.cap, self.di[0], self.cnt[0], self.stream))

    def loop(self):
        for v in range(self.n):
            one = C.c_int(0)
            ms._chk(self.lib.ms_orb_detect_and_compute(C.byref(self.gi[v]), None if self.mi is None else C.byref(self.mi[v]), C.byref(self.prm),
                                                       self.kp[1][v].ctypes.data_as(self.fp), self.cap, C.byref(self.di[1][v]), C.byref(one), self.stream))
            self.cnt[1][v] = one.value

    def equal(self):
        if list(self.cnt[0]) != list(self.cnt[1]):
            return False
        return all(self.kp[0][v, :c].tobytes() == self.kp[1][v, :c].tobytes() and torch.equal(self.desc[0][v][:c], self.desc[1][v][:c]) for v, c in enumerate(self.cnt[0]))


def clock(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


def measure(what, n, w, h, masked):
    c = Calls(views(n, w, h), band_masks(n, w, h) if masked else None)
    c.batch(); c.loop(); torch.cuda.synchronize()
    same = c.equal()
    c.batch(); c.loop()                                # both scratch routes warm
    b, l = [], []
    for _ in range(5):
        b.append(clock(c.batch)); l.append(clock(c.loop))
    rec = {"what": what, "views": n, "size": [w, h], "masks": masked, "orb": [2500, 1.2, 8], "keypoints": list(c.cnt[0]), "bit_equal_to_single_calls": same,
           "batch_call_ms": sorted(b)[2], "batch_call_runs_ms": b, "single_calls_ms": sorted(l)[2], "single_calls_runs_ms": l}
    rec["batch_over_single_calls"] = rec["batch_call_ms"] / rec["single_calls_ms"]
    rec["launches"] = "nlevels + 10 = 18"; rec["synchronisations"] = 1
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        c = Calls(views(6, 1920, 1080), None)
        torch.cuda.synchronize()
        for _ in range(int(sys.argv[2]) + 1):
            c.batch()
        return
    with open(sys.argv[1] if len(sys.argv) > 1 else "orb_batch.jsonl", "w") as f:
        for what, n, w, h, masked in (("orb_batch", 6, 1920, 1080, False), ("orb_batch", 6, 1920, 1080, True), ("orb_batch", 16, 1920, 1080, False),
                                      ("orb_batch", 16, 1920, 1080, True), ("orb_batch", 8, 640, 480, False), ("orb_batch", 1, 1920, 1080, False)):
            rec = measure(what, n, w, h, masked)
            f.write(json.dumps(rec) + "\n"); f.flush()
            print(json.dumps({k: rec[k] for k in ("views", "size", "masks", "bit_equal_to_single_calls", "batch_call_ms", "single_calls_ms", "batch_over_single_calls")}))


if __name__ == "__main__":
    main()
