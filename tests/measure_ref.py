"""Page measurement, restated in numpy: the specification the library equals bit for bit.

A prepared page v (float32 [H, W], dark ink on light paper) is measured, not changed: how wide its strokes are and how
tall its text is, in pixels, without a detector.  Everything is integer and set arithmetic on one set taken from the
page, so the result depends on neither schedule nor batch.

measure(page, threshold, min_area) -> info, a dict of exact integers (INFO_KEYS, in the order of ocrs_measure_info):
  ink        the number of pixels with v < threshold (an ordinary float compare: NaN is not ink, v == threshold is not).
  components the number of 8-connected components of ink; the page edge is a wall.
  counted    the number of those of area >= min_area (a smaller one is a speck: it still is a component).
  run_h, run_v   uint32 [256]: the maximal horizontal / vertical runs of ink by their length L, at index min(L, 255); the
             page edge ends a run; index 0 stays 0.
  comp_h, comp_w uint32 [256]: the counted components by the height / width of their bounding box, at min(side, 255).
  area_by_h  uint64 [256]: the summed areas of the counted components, by the index of comp_h.

Two implementations that share nothing but the ink set: measure() is vectorised (runs by differences, components by a
union over the horizontal runs, boxes by minimum / maximum over the runs); measure_slow() walks the page pixel by pixel
(runs by scanning, components by flood fill).  test_measure_cpu.py holds them to each other.

choose(info, min_height_strokes) -> {"stroke", "text_height", "support", "blank"}: the host's choice of a scale.
  stroke     r[L] = run_h[L] + run_v[L]; the L in 1 .. 254 with the largest L * r[L] (the pixels that lie in runs of that
             length; a uint64 product, no overflow: 254 * 2^33), the smallest L on a tie; 0 when r[1 .. 254] is all zero.
  text_height min_height_strokes is taken in 1/256: q = floor(min_height_strokes * 256 + 0.5), 0 <= q <= 65280.  A height H
             in 1 .. 254 qualifies when 256 * H >= q * stroke, in integers (this is `2 H >= 2 min_height_strokes stroke`
             without a rounded product).  support = the sum of comp_h over the qualifying H, each component counting
             once.  text_height = the lower median of those heights BY INK: the smallest qualifying H at which the
             cumulative area_by_h reaches (A + 1) // 2, A being the sum of area_by_h over the qualifying H (Python
             integers; the library adds in 128 bits); 0 with no support.  Bin 255 (a picture, a rule, a frame) never
             qualifies.  Weighing by ink is what keeps dots, commas and dashes out: they hold next to no ink.  The first
             rule (each component counting once, min_height_strokes 1.5) called every page of solid word blocks blank,
             the project's own synthetic pages among them, because there the dominant run IS the text height
             (DESIGN.md §7.14); the default is therefore 0.5: only what is lower than half a stroke is debris.
  blank      support == 0.

work_scale_for_text(text_height, target_height, min_scale, max_scale): target / text_height clamped to the range, in
double; 1.0 for text_height <= 0 (a blank page).
"""
import math

import numpy as np

from despeckle_ref import components

F = np.float32
INFO_KEYS = ("ink", "components", "counted", "run_h", "run_v", "comp_h", "comp_w", "area_by_h")
CHOICE_KEYS = ("stroke", "text_height", "support", "blank")
MAX_MIN_AREA = 65535
MIN_HEIGHT_STROKES = 0.5
MAX_HEIGHT_STROKES = 255.0
WORK_TEXT_HEIGHT_DEFAULT = 14   # include/ocrs_amd.h OCRS_WORK_TEXT_HEIGHT_DEFAULT: DESIGN.md §7.14 says where it comes from
WORK_SCALE_RANGE = (0.125, 4.0)  # what detect_words(work_text_height=...) clamps to


def default_params():
    return {"threshold": 0.0, "min_area": 4}


def valid_params(threshold=0.0, min_area=4):
    return bool(isinstance(min_area, (int, np.integer)) and np.isfinite(threshold) and 0 <= min_area <= MAX_MIN_AREA)


def ink_of(page, threshold=0.0):
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(page, F) < F(threshold)


def run_lengths(X):
    """The lengths of the maximal horizontal runs of the boolean [H, W] X, by differences along the rows."""
    edge = np.zeros((X.shape[0], X.shape[1] + 2), np.int8)
    edge[:, 1:-1] = X
    d = np.diff(edge, axis=1)
    return np.nonzero(d == -1)[1] - np.nonzero(d == 1)[1]   # row-major: the k-th start and the k-th end are one run's


def hist256(values, weights=None):
    idx = np.minimum(np.asarray(values, np.int64), 255)
    if weights is None:
        return np.bincount(idx, minlength=256).astype(np.uint32)
    out = np.zeros(256, np.uint64)
    np.add.at(out, idx, np.asarray(weights, np.uint64))
    return out


def measure(page, threshold=0.0, min_area=4):
    if not valid_params(threshold, min_area):
        raise ValueError("measure: parameters out of range")
    ink = ink_of(page, threshold)
    label, area = components(ink, True)
    n = len(area) - 1
    ys, xs = np.nonzero(ink)
    lab = label[ys, xs]
    y0, x0 = np.full(n + 1, 1 << 30, np.int64), np.full(n + 1, 1 << 30, np.int64)
    y1, x1 = np.full(n + 1, -1, np.int64), np.full(n + 1, -1, np.int64)
    np.minimum.at(y0, lab, ys)
    np.maximum.at(y1, lab, ys)
    np.minimum.at(x0, lab, xs)
    np.maximum.at(x1, lab, xs)
    keep = np.nonzero(area[1:] >= int(min_area))[0] + 1
    bh, bw = (y1 - y0 + 1)[keep], (x1 - x0 + 1)[keep]
    return {"ink": int(ink.sum()), "components": int(n), "counted": int(len(keep)),
            "run_h": hist256(run_lengths(ink)), "run_v": hist256(run_lengths(ink.T)),
            "comp_h": hist256(bh), "comp_w": hist256(bw), "area_by_h": hist256(bh, area[keep])}


def measure_slow(page, threshold=0.0, min_area=4):
    """The same by walking: runs by scanning every row and column, components by flood fill from every unseen ink pixel."""
    v = np.ascontiguousarray(page, F)
    H, W = v.shape
    thr = F(threshold)
    ink = [[bool(v[y, x] < thr) for x in range(W)] for y in range(H)]   # NaN < thr is False
    out = {"ink": sum(sum(r) for r in ink), "components": 0, "counted": 0}
    for k in ("run_h", "run_v", "comp_h", "comp_w"):
        out[k] = np.zeros(256, np.uint32)
    out["area_by_h"] = np.zeros(256, np.uint64)

    def scan(line, hist):
        n = 0
        for b in line:
            if b:
                n += 1
            elif n:
                hist[min(n, 255)] += 1
                n = 0
        if n:
            hist[min(n, 255)] += 1

    for y in range(H):
        scan(ink[y], out["run_h"])
    for x in range(W):
        scan([ink[y][x] for y in range(H)], out["run_v"])
    seen = [[False] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if not ink[y][x] or seen[y][x]:
                continue
            seen[y][x] = True
            stack, area, ya, yb, xa, xb = [(y, x)], 0, y, y, x, x
            while stack:
                cy, cx = stack.pop()
                area += 1
                ya, yb, xa, xb = min(ya, cy), max(yb, cy), min(xa, cx), max(xb, cx)
                for ny in (cy - 1, cy, cy + 1):
                    for nx in (cx - 1, cx, cx + 1):
                        if 0 <= ny < H and 0 <= nx < W and ink[ny][nx] and not seen[ny][nx]:
                            seen[ny][nx] = True
                            stack.append((ny, nx))
            out["components"] += 1
            if area >= int(min_area):
                out["counted"] += 1
                out["comp_h"][min(yb - ya + 1, 255)] += 1
                out["comp_w"][min(xb - xa + 1, 255)] += 1
                out["area_by_h"][min(yb - ya + 1, 255)] += np.uint64(area)
    return out


def same(a, b):
    """Two info records are equal in every field and every bin."""
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in INFO_KEYS) and set(a) >= set(INFO_KEYS) <= set(b)


def height_q8(min_height_strokes):
    """min_height_strokes in 1/256, or None when it is refused (not finite, negative, over 255)."""
    m = float(min_height_strokes)
    if not math.isfinite(m) or m < 0.0 or m > MAX_HEIGHT_STROKES:
        return None
    return int(math.floor(m * 256.0 + 0.5))


def choose(info, min_height_strokes=MIN_HEIGHT_STROKES):
    q = height_q8(min_height_strokes)
    if q is None:
        raise ValueError("choose: min_height_strokes is 0 .. 255")
    run_h, run_v, comp_h = (np.asarray(info[k]).astype(np.int64).tolist() for k in ("run_h", "run_v", "comp_h"))
    stroke, best = 0, 0
    for L in range(1, 255):
        px = L * (run_h[L] + run_v[L])
        if px > best:   # strictly: the smallest L stays on a tie
            stroke, best = L, px
    heights = [H for H in range(1, 255) if 256 * H >= q * stroke]
    area = [int(a) for a in np.asarray(info["area_by_h"]).tolist()]
    support = sum(comp_h[H] for H in heights)
    total = sum(area[H] for H in heights)
    text_height, cum = 0, 0
    for H in heights:
        cum += area[H]
        if support and total and cum >= (total + 1) // 2:   # a record of the library's has ink wherever it has components
            text_height = H
            break
    return {"stroke": stroke, "text_height": text_height, "support": int(support), "blank": int(support == 0)}


def work_scale_for_text(text_height, target_height, min_scale=WORK_SCALE_RANGE[0], max_scale=WORK_SCALE_RANGE[1]):
    target_height, min_scale, max_scale = float(target_height), float(min_scale), float(max_scale)
    if not (math.isfinite(target_height) and target_height > 0.0 and math.isfinite(min_scale) and math.isfinite(max_scale)
            and 0.0 < min_scale <= max_scale):
        raise ValueError("work_scale_for_text: a positive target and a range 0 < min_scale <= max_scale")
    if int(text_height) <= 0:
        return 1.0
    return min(max(target_height / float(int(text_height)), min_scale), max_scale)
