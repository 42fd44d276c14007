"""Page framing, restated in numpy: the specification the library equals bit for bit.

clean_frame(page, depth, sides, min_area, threshold, paper) -> (out, mask, info): a prepared page v (float32 [H, W], dark
ink on light paper) comes back with the ink that is connected to the page frame overwritten by the paper's level; every
other pixel keeps its own 32-bit word.  All of it is integer and set arithmetic, every set is taken from the INPUT page and
nothing is iterated.

  1 ink   = v < threshold (NaN is not ink, -inf is).
  2 ring  = the pixels with min(x, y, W - 1 - x, H - 1 - y) < depth; depth 0: the whole page.
  3 R     = ink & ring; its components are 8-connected (despeckle_ref.components); whatever is not R is a wall, the page
            edge and the ring's inner edge with it.
  4 seeds = the pixels of R on an enabled side: `sides` bit 0 x = 0, bit 1 y = 0, bit 2 x = W - 1, bit 3 y = H - 1.
  5 a component holding a seed is touching; its area counts its pixels (all in R).  removed = the pixels of touching
    components of area >= min_area, kept = those of touching components of area < min_area.
  6 paper_bin = pct(1, 2) of the histogram of the pixels of the whole page that are neither ink nor NaN (bins as §7.4; 255
    with nothing counted), paper_fill = (paper_bin + 1) / 256 - 0.5.  A given paper replaces the fill, and the bin then
    reads -1.
  7 out   = paper_fill on removed, the page's own word elsewhere.
  mask bits: 0 removed, 1 kept, 2 in R.

profiles(page, threshold) -> (col_ink uint32 [W], row_ink uint32 [H]); choose(h, w, col_ink, row_ink, ...) -> the content
box and the gutter; crop(page, rect, fill) -> the rectangle, `fill` outside the page; uncrop_rects / uncrop_boxes: the maps
back.
"""
import numpy as np

from despeckle_ref import components
from rules_ref import bins, pct

F = np.float32
INFO_KEYS = ("paper_bin", "paper_fill", "ink", "counted", "ring_ink", "removed", "removed_pixels", "kept", "kept_pixels")
CHOICE_KEYS = ("found", "x0", "y0", "x1", "y1", "gutter_x")
MAX_SIDE = 65535


def default_params():
    return {"threshold": 0.0, "depth": 128, "sides": 15, "min_area": 0, "paper": None}


def valid_params(threshold=0.0, depth=128, sides=15, min_area=0, paper=None):
    ints = all(isinstance(v, (int, np.integer)) for v in (depth, sides, min_area))
    return bool(ints and np.isfinite(threshold) and 0 <= depth <= MAX_SIDE and 1 <= sides <= 15 and 0 <= min_area < 2 ** 31
                and (paper is None or not np.isinf(paper)))


def ring_of(h, w, depth):
    if depth == 0:
        return np.ones((h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.minimum(np.minimum(xx, yy), np.minimum(w - 1 - xx, h - 1 - yy)) < depth


def side_of(h, w, sides):
    s = np.zeros((h, w), bool)
    if sides & 1:
        s[:, 0] = True
    if sides & 2:
        s[0, :] = True
    if sides & 4:
        s[:, w - 1] = True
    if sides & 8:
        s[h - 1, :] = True
    return s


def sets(page, depth=128, sides=15, min_area=0, threshold=0.0):
    """Every set of the definition as a boolean [H, W], by name, and the numbers of components."""
    v = np.ascontiguousarray(page, F)
    h, w = v.shape
    with np.errstate(invalid="ignore"):
        ink = v < F(threshold)
    R = ink & ring_of(h, w, int(depth))
    label, area = components(R, True)
    touching = np.zeros(len(area), bool)
    touching[np.unique(label[R & side_of(h, w, int(sides))])] = True
    touching[0] = False
    big = area >= int(min_area)
    removed_c, kept_c = touching & big, touching & ~big
    return {"ink": ink, "counted": ~ink & ~np.isnan(v), "R": R, "removed": removed_c[label] & R, "kept": kept_c[label] & R,
            "n_removed": int(removed_c.sum()), "n_kept": int(kept_c.sum())}


def clean_frame(page, depth=128, sides=15, min_area=0, threshold=0.0, paper=None):
    """-> (out float32 [H, W], mask uint8 [H, W], info dict)."""
    if not valid_params(threshold, depth, sides, min_area, paper):
        raise ValueError("clean_frame: parameters out of range")
    v = np.ascontiguousarray(page, F)
    s = sets(v, depth, sides, min_area, threshold)
    if paper is None or np.isnan(paper):
        paper_bin = pct(np.bincount(bins(v[s["counted"]]).reshape(-1), minlength=256).astype(np.int64), 1, 2)
        paper_bin = 255 if paper_bin < 0 else paper_bin
        paper_fill = F(F(paper_bin + 1) / F(256.0) - F(0.5))
    else:
        paper_bin, paper_fill = -1, F(paper)
    out = v.copy()
    out.view(np.uint32)[s["removed"]] = np.array([paper_fill], F).view(np.uint32)[0]
    mask = (s["removed"] * 1 + s["kept"] * 2 + s["R"] * 4).astype(np.uint8)
    info = {"paper_bin": int(paper_bin), "paper_fill": float(paper_fill), "ink": int(s["ink"].sum()), "counted": int(s["counted"].sum()),
            "ring_ink": int(s["R"].sum()), "removed": s["n_removed"], "removed_pixels": int(s["removed"].sum()), "kept": s["n_kept"],
            "kept_pixels": int(s["kept"].sum())}
    return out, mask, info


def profiles(page, threshold=0.0):
    with np.errstate(invalid="ignore"):
        ink = np.ascontiguousarray(page, F) < F(threshold)
    return ink.sum(axis=0).astype(np.uint32), ink.sum(axis=1).astype(np.uint32)


def default_choice_params():
    return {"min_count": 1, "pad": 16, "gutter_min_width": 8, "gutter_max_ink": 0}


def valid_choice_params(min_count=1, pad=16, gutter_min_width=8, gutter_max_ink=0):
    return bool(min_count >= 1 and 0 <= pad <= MAX_SIDE and gutter_min_width >= 1 and gutter_max_ink >= 0)


def choose(h, w, col_ink, row_ink, min_count=1, pad=16, gutter_min_width=8, gutter_max_ink=0):
    """-> {"found", "x0", "y0", "x1", "y1", "gutter_x"}: the definition of include/ocrs_amd.h, in whole numbers."""
    if not valid_choice_params(min_count, pad, gutter_min_width, gutter_max_ink):
        raise ValueError("choose: parameters out of range")
    cols, rows = np.asarray(col_ink, np.int64), np.asarray(row_ink, np.int64)
    assert cols.shape == (w,) and rows.shape == (h,)
    cx, cy = np.nonzero(cols >= min_count)[0], np.nonzero(rows >= min_count)[0]
    if not len(cx) or not len(cy):
        return {"found": 0, "x0": 0, "y0": 0, "x1": w, "y1": h, "gutter_x": -1}
    cx0, cx1, cy0, cy1 = int(cx[0]), int(cx[-1]) + 1, int(cy[0]), int(cy[-1]) + 1
    out = {"found": 1, "x0": max(cx0 - pad, 0), "y0": max(cy0 - pad, 0), "x1": min(cx1 + pad, w), "y1": min(cy1 + pad, h), "gutter_x": -1}
    b0, b1 = cx0 + 3 * (cx1 - cx0) // 8, cx0 + 5 * (cx1 - cx0) // 8
    quiet = np.concatenate([[False], cols[b0:b1] <= gutter_max_ink, [False]])
    starts, ends = np.nonzero(quiet[1:] & ~quiet[:-1])[0] + b0, np.nonzero(~quiet[1:] & quiet[:-1])[0] + b0
    runs = [(-(e - s), abs(2 * (s + (e - s) // 2) - (cx0 + cx1)), s) for s, e in zip(starts.tolist(), ends.tolist())]
    if runs:
        neg_len, _, start = min(runs)   # the longest, then the most central, then the leftmost
        if -neg_len >= gutter_min_width:
            out["gutter_x"] = start + (-neg_len) // 2
    return out


def crop(page, rect, fill):
    """rect = (x0, y0, x1, y1), half open -> float32 [y1 - y0, x1 - x0]: the page's words inside it, the word of `fill`
    (float32) outside."""
    v = np.ascontiguousarray(page, F)
    h, w = v.shape
    x0, y0, x1, y1 = (int(t) for t in rect)
    assert 1 <= x1 - x0 <= MAX_SIDE and 1 <= y1 - y0 <= MAX_SIDE
    out = np.empty((y1 - y0, x1 - x0), np.uint32)
    out[:] = np.array([fill], F).view(np.uint32)[0] if not isinstance(fill, np.float32) else fill.view(np.uint32)
    sx0, sx1, sy0, sy1 = max(x0, 0), min(x1, w), max(y0, 0), min(y1, h)
    if sx0 < sx1 and sy0 < sy1:
        out[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = v.view(np.uint32)[sy0:sy1, sx0:sx1]
    return out.view(F)


def uncrop_rects(rects, origin):
    """float32 [n, 6] (cx, cy, ux, uy, w, h) on a page cut out at origin = (x0, y0) -> in the frame of the page it was cut from."""
    a = np.array(rects, F).reshape(-1, 6)
    a[:, 0] = a[:, 0] + F(origin[0])
    a[:, 1] = a[:, 1] + F(origin[1])
    return a


def uncrop_boxes(boxes, origin):
    """int32 [n, 4] (top, left, bottom, right) likewise; integer addition that wraps."""
    b = np.array(boxes, np.int64).reshape(-1, 4)
    b += np.array([origin[1], origin[0], origin[1], origin[0]], np.int64)
    return ((b + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
