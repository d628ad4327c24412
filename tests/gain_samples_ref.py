"""Numpy restatement of the sample buffers of view shards (ms_gain_samples / ms_track_gains_from_samples), written from the statement in include/ms_stitch.h:
the blocks of views of the shards, the lattice rectangle R_v of a view, its words (0 = not seen, q + 1 otherwise), header and offset table, and the pair sums
formed from per-view vectors alone.  Imports tests/gain_ref.py for the per-view sampling."""
import numpy as np

MAGIC = 0x56474d53
HEADER_WORDS = 16


def shard_views(n, S, k):
    """Bit mask of the views of shard k of S: the contiguous block [k n / S, (k + 1) n / S)."""
    return sum(1 << v for v in range(k * n // S, (k + 1) * n // S))


def lattice_rect(roi, T, stride):
    """R_v = (sx0, sy0, w, h) in lattice indices: the samples (T.x + sx stride, T.y + sy stride) of the lattice of T that lie in roi.  w or h may be 0."""
    us, vs = np.arange(T[0], T[0] + T[2], stride), np.arange(T[1], T[1] + T[3], stride)
    ix = np.nonzero((us >= roi[0]) & (us < roi[0] + roi[2]))[0]
    iy = np.nonzero((vs >= roi[1]) & (vs < roi[1] + roi[3]))[0]
    return (int(ix[0]) if len(ix) else 0, int(iy[0]) if len(iy) else 0, len(ix), len(iy))


def view_words(seen_v, q_v, roi, T, stride):
    """The words of one view: uint32 (h, w) over R_v.  seen_v / q_v roi-sized (gain_ref.sample_view)."""
    sx0, sy0, w, h = lattice_rect(roi, T, stride)
    if w == 0 or h == 0:
        return np.zeros((h, w), np.uint32)
    xs = T[0] + (sx0 + np.arange(w)) * stride - roi[0]
    ys = T[1] + (sy0 + np.arange(h)) * stride - roi[1]
    sub = np.ix_(ys, xs)
    assert int(q_v.max(initial=0)) < (1 << 29)
    return np.where(seen_v[sub], q_v[sub] + 1, 0).astype(np.uint32)


def buffer(rois, seen, q, T, stride, owned, active=None):
    """The whole buffer of a shard that owns the views `owned` (bit mask): uint32 array."""
    n = len(rois)
    active = (1 << n) - 1 if active is None else active
    held = owned & active
    data, off, at = [], [0] * n, HEADER_WORDS + n
    for v in range(n):
        if (held >> v) & 1:
            w = view_words(seen[v], q[v], rois[v], T, stride)
            off[v] = at
            at += w.size
            data.append(w.ravel())
    hdr = np.zeros(HEADER_WORDS, np.uint32)
    hdr[:4] = [MAGIC, n, active, stride]
    hdr[4:8] = np.array(T, np.int32).view(np.uint32)
    hdr[8], hdr[9] = held, at * 4
    return np.concatenate([hdr, np.array(off, np.uint32)] + data).astype(np.uint32)


def parse(buf, rois, T):
    """uint32 array -> (header dict, {view: (h, w) uint32 words}) by the buffer's own header and offset table."""
    buf = np.asarray(buf).view(np.uint32)
    n, stride = int(buf[1]), int(buf[3])
    hdr = {"magic": int(buf[0]), "num_views": n, "active": int(buf[2]), "stride": stride, "T": tuple(int(x) for x in buf[4:8].view(np.int32)),
           "held": int(buf[8]), "bytes": int(buf[9]), "rest": [int(x) for x in buf[10:HEADER_WORDS]]}
    views = {}
    for v in range(n):
        o = int(buf[HEADER_WORDS + v])
        if (hdr["held"] >> v) & 1:
            _, _, w, h = lattice_rect(rois[v], T, stride)
            views[v] = buf[o:o + w * h].reshape(h, w)
        else:
            assert o == 0
    return hdr, views


def pair_sums(rois, T, stride, vectors, active=None):
    """Raw (cnt, S), n x n int64, of every pair of active views from the per-view vectors {v: (h, w) words} alone: the consumer's side."""
    n = len(rois)
    active = (1 << n) - 1 if active is None else active
    nsx, nsy = -(-T[2] // stride), -(-T[3] // stride)
    see, val = [], []
    for v in range(n):
        m, qq = np.zeros((nsy, nsx), bool), np.zeros((nsy, nsx), np.int64)
        if (active >> v) & 1:
            sx0, sy0, w, h = lattice_rect(rois[v], T, stride)
            words = vectors[v].astype(np.int64)
            assert words.shape == (h, w)
            m[sy0:sy0 + h, sx0:sx0 + w] = words != 0
            qq[sy0:sy0 + h, sx0:sx0 + w] = np.where(words != 0, words - 1, 0)
        see.append(m); val.append(qq)
    cnt, S = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i, n):
            both = see[i] & see[j]
            cnt[i, j] = cnt[j, i] = int(both.sum())
            S[i, j] = int(val[i][both].sum())
            S[j, i] = int(val[j][both].sum())
    return cnt, S
