"""Despeckling, restated in numpy: the specification the library equals bit for bit.

A prepared page v (float32 [H, W], dark ink on light paper) comes back with its isolated dark specks overwritten by the
paper's level and, when asked for, the light pinholes inside its strokes by the ink's level; every other pixel keeps its
own 32-bit word.  All of it is integer and set arithmetic, every set is taken from the INPUT page and nothing is iterated.
despeckle(page, max_area, max_hole, keep_near, threshold, paper, ink_level) -> (out, mask, info).

  1 ink    = v < threshold (NaN is not ink, -inf is).
  2 ink components are 8-connected, the components of ~ink (NaN included) 4-connected; the page edge is a wall.  They are
    built here by an explicit union over the horizontal runs of rules_ref.runs (the library unites pixels).
  3 cand   = the pixels of ink components of area <= A; big = ink \\ cand.
  4 K > 0: a candidate component is kept when one of its pixels lies within Chebyshev distance K of a big pixel;
    speck = cand \\ kept.  K = 0: nothing is kept.
  5 hole   = the pixels of ~ink components of area <= Hm.
  6 paper_bin = pct(1, 2) of the histogram of the pixels that are neither ink nor NaN (bins as §7.4; 255 with nothing
    counted), paper_fill = (paper_bin + 1) / 256 - 0.5; ink_bin = pct(1, 2) of the ink pixels (0 with no ink), ink_fill =
    ink_bin / 256 - 0.5.  A given paper or ink_level replaces its fill, and its bin then reads -1.
  7 out    = paper_fill on speck, ink_fill on hole, the page's own word elsewhere.
  mask bits: 0 speck, 1 hole, 2 kept.
"""
import numpy as np

from rules_ref import bins, pct, runs

F = np.float32
INFO_KEYS = ("paper_bin", "ink_bin", "paper_fill", "ink_fill", "ink", "counted", "specks", "kept", "speck_pixels", "kept_pixels",
             "holes", "hole_pixels")
MAX_AREA = 4096
MAX_NEAR = 16


def default_params():
    return {"threshold": 0.0, "max_area": 4, "max_hole": 0, "keep_near": 0, "paper": None, "ink_level": None}


def valid_params(threshold=0.0, max_area=4, max_hole=0, keep_near=0, paper=None, ink_level=None):
    ints = all(isinstance(v, (int, np.integer)) for v in (max_area, max_hole, keep_near))
    return bool(ints and np.isfinite(threshold) and 0 <= max_area <= MAX_AREA and 0 <= max_hole <= MAX_AREA and 0 <= keep_near <= MAX_NEAR
                and (paper is None or not np.isinf(paper)) and (ink_level is None or not np.isinf(ink_level)))


def components(X, diagonal):
    """The components of the boolean [H, W] X, 8-connected when `diagonal`, 4-connected otherwise -> (label int32 [H, W],
    1 .. n on X in the order of each component's raster-first pixel and 0 elsewhere; area int64 [n + 1], area[0] = 0)."""
    X = np.asarray(X, bool)
    H, W = X.shape
    row, first, past = runs(X)
    n = len(row)
    parent = list(range(n))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    if n:
        # run i touches the runs j of the next row with first_j <= past_i - 1 + e and past_j - 1 >= first_i - e (e = 1 with
        # diagonals): runs of a row are disjoint and in order, so those j are consecutive
        e = 1 if diagonal else 0
        S = W + 4
        key_first = row.astype(np.int64) * S + first + 1
        key_past = row.astype(np.int64) * S + past + 1
        below = (row.astype(np.int64) + 1) * S + 1
        lo = np.searchsorted(key_past, below + first - e, side="right")
        hi = np.searchsorted(key_first, below + past - 1 + e, side="right")
        for i in np.nonzero(hi > lo)[0].tolist():
            for j in range(int(lo[i]), int(hi[i])):
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)   # the root is the component's first run in raster order
    root = np.array([find(i) for i in range(n)], np.int64)
    order = np.zeros(n, np.int64)
    is_root = root == np.arange(n)
    order[is_root] = np.arange(1, int(is_root.sum()) + 1)
    of_run = order[root] if n else order
    area = np.bincount(of_run, weights=None if not n else (past - first), minlength=int(is_root.sum()) + 1).astype(np.int64)
    label = np.zeros((H, W + 1), np.int64)
    np.add.at(label, (row, first), of_run)
    np.add.at(label, (row, past), -of_run)
    return np.cumsum(label, axis=1)[:, :-1].astype(np.int32), area


def dilate(X, k):
    """The pixels within Chebyshev distance k of a pixel of X."""
    rows = X.copy()
    for s in range(1, k + 1):
        rows[s:] |= X[:-s]
        rows[:-s] |= X[s:]
    out = rows.copy()
    for s in range(1, k + 1):
        out[:, s:] |= rows[:, :-s]
        out[:, :-s] |= rows[:, s:]
    return out


def analyse(page, threshold=0.0):
    """What depends on the page and the threshold alone: ink, both labellings, both histograms."""
    v = np.ascontiguousarray(page, F)
    with np.errstate(invalid="ignore"):
        ink = v < F(threshold)
    counted = ~ink & ~np.isnan(v)
    return {"v": v, "ink": ink, "counted": counted, "ink_cc": components(ink, True), "paper_cc": components(~ink, False),
            "paper_hist": np.bincount(bins(v[counted]).reshape(-1), minlength=256).astype(np.int64),
            "ink_hist": np.bincount(bins(v[ink]).reshape(-1), minlength=256).astype(np.int64)}


def sets(page, max_area=4, max_hole=0, keep_near=0, threshold=0.0, analysis=None):
    """Every set of the definition as a boolean [H, W], by name, and the numbers of components."""
    a = analysis if analysis is not None else analyse(page, threshold)
    A, Hm, K = int(max_area), int(max_hole), int(keep_near)
    ink = a["ink"]
    label, area = a["ink_cc"]
    small = area <= A
    small[0] = False
    cand = small[label]
    big = ink & ~cand
    kept_comp = np.zeros(len(area), bool)
    if K > 0:
        kept_comp[np.unique(label[cand & dilate(big, K)])] = True
    kept = kept_comp[label] & cand
    speck = cand & ~kept
    plabel, parea = a["paper_cc"]
    psmall = parea <= Hm
    psmall[0] = False
    hole = psmall[plabel]
    return {"ink": ink, "cand": cand, "big": big, "kept": kept, "speck": speck, "hole": hole,
            "n_specks": int(small.sum() - kept_comp.sum()), "n_kept": int(kept_comp.sum()), "n_holes": int(psmall.sum())}


def despeckle(page, max_area=4, max_hole=0, keep_near=0, threshold=0.0, paper=None, ink_level=None, analysis=None):
    """-> (out float32 [H, W], mask uint8 [H, W], info dict).  analysis: analyse(page, threshold), to share it between calls."""
    if not valid_params(threshold, max_area, max_hole, keep_near, paper, ink_level):
        raise ValueError("despeckle: parameters out of range")
    a = analysis if analysis is not None else analyse(page, threshold)
    v = a["v"]
    s = sets(v, max_area, max_hole, keep_near, threshold, a)
    if paper is None or np.isnan(paper):
        paper_bin = pct(a["paper_hist"], 1, 2)
        paper_bin = 255 if paper_bin < 0 else paper_bin
        paper_fill = F(F(paper_bin + 1) / F(256.0) - F(0.5))
    else:
        paper_bin, paper_fill = -1, F(paper)
    if ink_level is None or np.isnan(ink_level):
        ink_bin = pct(a["ink_hist"], 1, 2)
        ink_bin = 0 if ink_bin < 0 else ink_bin
        ink_fill = F(F(ink_bin) / F(256.0) - F(0.5))
    else:
        ink_bin, ink_fill = -1, F(ink_level)
    out = v.copy()
    out.view(np.uint32)[s["speck"]] = np.array([paper_fill], F).view(np.uint32)[0]
    out.view(np.uint32)[s["hole"]] = np.array([ink_fill], F).view(np.uint32)[0]
    mask = (s["speck"] * 1 + s["hole"] * 2 + s["kept"] * 4).astype(np.uint8)
    info = {"paper_bin": int(paper_bin), "ink_bin": int(ink_bin), "paper_fill": float(paper_fill), "ink_fill": float(ink_fill),
            "ink": int(s["ink"].sum()), "counted": int(a["counted"].sum()), "specks": s["n_specks"], "kept": s["n_kept"],
            "speck_pixels": int(s["speck"].sum()), "kept_pixels": int(s["kept"].sum()), "holes": s["n_holes"],
            "hole_pixels": int(s["hole"].sum())}
    return out, mask, info


def add_noise(clean, fraction, seed=11):
    """The noisy page of DESIGN.md §7.9: pepper at -0.5 on `fraction` of the pixels, then salt at +0.5 on as many more
    (default_rng(seed), pepper first) -> (noisy, pepper mask, salt mask)."""
    clean = np.ascontiguousarray(clean, F)
    rng = np.random.default_rng(seed)
    pepper = rng.random(clean.shape) < fraction
    salt = rng.random(clean.shape) < fraction
    noisy = clean.copy()
    noisy[pepper] = F(-0.5)
    noisy[salt] = F(0.5)
    return noisy, pepper, salt


def noise_counts(clean, noisy, out):
    """(stray ink before: ink of the noisy page that is not ink of the clean one; stray ink left in `out`; word ink lost: ink
    of both the clean and the noisy page that `out` lacks; word ink of the clean page), ink being < 0."""
    ink, got = clean < F(0), out < F(0)
    return int(((noisy < F(0)) & ~ink).sum()), int((got & ~ink).sum()), int((ink & (noisy < F(0)) & ~got).sum()), int(ink.sum())
