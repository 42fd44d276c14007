"""Detection confidence by its definition, in numpy, for the tests.

For a page-resolution probability map P and threshold thr: M = P > thr.  Every word rect belongs to one External
8-connected foreground component of M that survived area >= min_area; S = all pixels of that component (holes, and
islands inside holes, are not part of it).  Then

    pixels = |S|                                     uint32
    q(p)   = floor(clamp(p, 0, 1) * 2^24)            exact in float32
    sum    = sum over S of q(P)                      uint64
    score  = float32(float64(sum) / (float64(pixels) * 16777216.0))

The components come from the oracle's find_contours_external (discovery order; each contour starts at its component's
raster-first pixel); S is grown from that pixel by the 8-connected labelling below; which components survive is what the
oracle's component_rects says about them.
"""
import numpy as np

from oracle import clib

EXPAND = 3.0   # detection.rs:41-62 as the engine calls it


def quantise(p):
    """q(p) as int64; p float32."""
    p = np.asarray(p, np.float32)
    c = np.minimum(np.maximum(p, np.float32(0.0)), np.float32(1.0))   # +inf -> 1
    return np.floor(c * np.float32(16777216.0)).astype(np.int64)


def label8(mask):
    """8-connected components of a 0/1 mask by union-find over horizontal runs -> int32 [h, w], -1 on background, equal
    values inside one component (values are arbitrary run numbers)."""
    mask = np.asarray(mask, np.uint8)
    h, w = mask.shape
    lab = np.full((h, w), -1, np.int32)
    parent = []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    prev = []   # runs of the row above: (start, end exclusive, id), ascending
    for y in range(h):
        row = mask[y]
        if not row.any():
            prev = []
            continue
        d = np.diff(np.concatenate(([0], row != 0, [0])).astype(np.int8))
        cur = []
        j = 0
        for s, e in zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()):
            rid = len(parent)
            parent.append(rid)
            lab[y, s:e] = rid
            while j < len(prev) and prev[j][1] < s:        # ends left of s - 1: cannot touch this or any later run
                j += 1
            k = j
            while k < len(prev) and prev[k][0] <= e:       # [ps, pe) touches [s, e) diagonally too: ps <= e and pe >= s
                a, b = find(rid), find(prev[k][2])
                if a != b:
                    parent[max(a, b)] = min(a, b)
                k += 1
            cur.append((s, e, rid))
        prev = cur
    if parent:
        roots = np.array([find(i) for i in range(len(parent))], np.int32)
        fg = lab >= 0
        lab[fg] = roots[lab[fg]]
    return lab


def _kept(lab, ids, min_area):
    """Which of the components `ids` (labels, discovery order) survive, and their rects: component_rects on the
    one-component mask.  A rect depends on its own component alone and a subset of External components stays External
    and keeps its raster order, so a group whose members all survive, or all fail, is settled by one call on the group's
    mask; a mixed group is split down to single components."""
    n = len(ids)
    keep = np.zeros(n, bool)
    rects = np.zeros((n, 6), np.float32)
    sel = np.zeros(int(lab.max()) + 2, bool)   # [-1] = background

    def go(lo, hi):
        if lo >= hi:
            return
        sel[:] = False
        sel[ids[lo:hi]] = True
        r = clib.component_rects(sel[lab].astype(np.uint8), EXPAND, min_area)
        assert len(r) <= hi - lo
        if len(r) == hi - lo:
            keep[lo:hi] = True
            rects[lo:hi] = r
        elif len(r) and hi - lo > 1:
            mid = (lo + hi) // 2
            go(lo, mid)
            go(mid, hi)

    go(0, n)
    return keep, rects


def reference(P, thr, min_area, count=False):
    """-> (rects float32 [n, 6], score float32 [n], pixels uint32 [n]) of the words of the page whose probability map is P;
    count=True: plus the number of External components, kept or not, as a fourth value."""
    P = np.ascontiguousarray(P, np.float32)
    mask = clib.threshold(P, thr)          # strict p > thr; NaN never passes
    contours = clib.find_contours_external(mask)
    lab = label8(mask)
    ids = np.array([lab[c[0][0], c[0][1]] for c in contours], np.int64).reshape(-1)
    assert (ids >= 0).all() and len(set(ids.tolist())) == len(ids), "a contour start is a foreground pixel of its own component"
    keep, rects = _kept(lab, ids, min_area) if len(ids) else (np.zeros(0, bool), np.zeros((0, 6), np.float32))
    fg = lab >= 0
    n_lab = int(lab.max()) + 1 if fg.any() else 0
    pixels = np.zeros(n_lab, np.int64)
    sums = np.zeros(n_lab, np.int64)
    np.add.at(pixels, lab[fg], 1)
    np.add.at(sums, lab[fg], quantise(P[fg]))
    k = ids[keep]
    px = pixels[k]
    score = (sums[k].astype(np.float64) / (px.astype(np.float64) * 16777216.0)).astype(np.float32)
    out = (rects[keep], score, px.astype(np.uint32))
    return out + (len(ids),) if count else out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
