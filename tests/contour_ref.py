"""The definition of the contour / rectangle stage, slot by slot, for test_contour_cases_cpu.py and test_gpu_contour.py.

For a mask, contour i of clib.find_contours_external is slot i (raster order of the components' first pixels); its
simplified polygon is clib.simplify_polygon(xy, 2), its rectangle clib.min_area_rect of that plus 2 * expand on both
sides, valid when the rectangle exists and w * h >= min_area in float32 (find_connected_component_rects,
detection.rs:41-62; oracle/csrc/ocrs_oracle.c orc_component_rects, which compacts the same slots).

rdp_f32 and edge_areas_f32 restate, in float32 numpy, the two searches whose result depends on which of several equal
values is taken: the RDP pivot (first maximum of the distances to a segment) and the rectangle's edge (first minimum of
the per-edge areas).  They are not a second definition: the CPU test holds them to clib bit for bit on every case, and
they exist to tell which ties a case contains — what the kernel's wave reductions must resolve towards the lowest
index.
"""
import numpy as np

from oracle import clib

EPS = 2.0
F = np.float32


def component_slots(mask, expand=3.0, min_area=100.0):
    """-> dict: n_roots, valid [k] uint8, rects [k, 6] float32 (zeros where there is no rectangle), n [k] border lengths,
    m [k] simplified counts."""
    contours = clib.find_contours_external(mask)
    k = len(contours)
    valid, rects = np.zeros(k, np.uint8), np.zeros((k, 6), np.float32)
    ns, ms = np.zeros(k, np.int64), np.zeros(k, np.int64)
    two_e, ma = F(2.0) * F(expand), F(min_area)
    for i, c in enumerate(contours):
        simp = clib.simplify_polygon(c[:, ::-1], EPS)
        ns[i], ms[i] = len(c), len(simp)
        rr = clib.min_area_rect(simp)
        if rr is None:
            continue
        rr[4] = rr[4] + two_e
        rr[5] = rr[5] + two_e
        rects[i] = rr
        valid[i] = 1 if F(rr[4] * rr[5]) >= ma else 0
    return {"n_roots": k, "valid": valid, "rects": rects, "n": ns, "m": ms}


def with_min_area(slots, min_area):
    """component_slots(mask, expand, 0) re-judged at another min_area (the rectangles do not depend on it)."""
    out = dict(slots)
    r = slots["rects"]
    out["valid"] = ((slots["valid"] == 1) & ((r[:, 4] * r[:, 5]).astype(np.float32) >= F(min_area))).astype(np.uint8)
    return out


def words(slots):
    """The slots as uint32 words: -0.0 and 0.0 differ."""
    return np.ascontiguousarray(slots, np.float32).view(np.uint32)


# ------------------------------------------------------------------ float32 restatements
def _seg_distance(a, b, p):
    """ocrs_oracle.c seg_distance of the points p [k, 2] to the segment a-b, one rounding per operation."""
    abx, aby = b[0] - a[0], b[1] - a[1]
    apx, apy = p[:, 0] - a[0], p[:, 1] - a[1]
    len2 = abx * abx + aby * aby
    if len2 == F(0.0):
        return np.sqrt(apx * apx + apy * apy)
    t = (apx * abx + apy * aby) / len2
    t = np.where(t < F(0.0), F(0.0), t)
    t = np.where(t > F(1.0), F(1.0), t)
    qx, qy = a[0] + t * abx, a[1] + t * aby
    dx, dy = p[:, 0] - qx, p[:, 1] - qy
    return np.sqrt(dx * dx + dy * dy)


def rdp_f32(xy, eps=EPS, last=False):
    """simplify_polygon restated: xy [n, 2] float32 (x, y) of a closed polygon -> (simplified [m, 2], ties).  ties: one
    (lo, hi, indices, split) per segment of the closed polyline whose maximum distance is positive and attained at more than
    one index (indices ascending; split: the maximum exceeds eps, so the first of them becomes a vertex).  last: the WRONG
    rule, the last of them becomes the vertex — to show that a case's rectangle depends on the rule."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    n = len(xy)
    if n == 0:
        return xy.copy(), []
    line = np.concatenate([xy, xy[:1]])
    keep = np.zeros(n + 1, bool)
    keep[0] = keep[n] = True
    ties, stack, eps = [], [(0, n)], F(eps)
    while stack:
        lo, hi = stack.pop()
        if hi - lo < 2:
            continue
        d = _seg_distance(line[lo], line[hi], line[lo + 1:hi])
        maxd = d.max()
        if not maxd > F(0.0):
            continue
        at = np.flatnonzero(d == maxd) + lo + 1
        split = bool(maxd > eps)
        if len(at) > 1:
            ties.append((lo, hi, [int(v) for v in at], split))
        if split:
            p = int(at[-1] if last else at[0])
            keep[p] = True
            stack.append((lo, p))
            stack.append((p, hi))
    return line[:n][keep[:n]].copy(), ties


def edge_areas_f32(hull):
    """min_area_rect's search restated on a hull [hn, 2] (clib.convex_hull's order) -> (areas [hn] float32, rect or None).
    The rectangle belongs to the FIRST edge whose area is below every earlier one's; a NaN area (one-point hull) never is."""
    hull = np.ascontiguousarray(hull, np.float32).reshape(-1, 2)
    hn = len(hull)
    if hn == 0:
        return np.zeros(0, np.float32), None
    a, b = hull, np.roll(hull, -1, axis=0)
    ex, ey = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt(ex * ex + ey * ey)
        parx, pary = ex / ln, ey / ln
        perx, pery = -pary, parx
        dx, dy = hull[None, :, 0] - a[:, None, 0], hull[None, :, 1] - a[:, None, 1]      # [edge, point]
        pp = parx[:, None] * dx + pary[:, None] * dy
        qq = perx[:, None] * dx + pery[:, None] * dy
        rows = np.arange(hn)
        # the C loop keeps the first element among equal ones (-0.0 == 0.0): so do argmin / argmax
        min_par, max_par = pp[rows, np.argmin(pp, axis=1)], pp[rows, np.argmax(pp, axis=1)]
        height = qq[rows, np.argmax(qq, axis=1)]
        width = max_par - min_par
        areas = height * width
        best, e = F(3.40282347e+38), -1
        for i in range(hn):
            if areas[i] < best:
                best, e = areas[i], i
        if e < 0:
            return areas, None
        along, half_h = min_par[e] + width[e] / F(2.0), height[e] / F(2.0)
        ul = np.sqrt(perx[e] * perx[e] + pery[e] * pery[e])
        rr = np.array([a[e, 0] + along * parx[e] + half_h * perx[e], a[e, 1] + along * pary[e] + half_h * pery[e],
                       perx[e] / ul, pery[e] / ul, width[e], height[e]], np.float32)
    return areas, rr


def hull_f32(xy, keep_collinear=False):
    """convex_hull restated (Andrew's monotone chain, float32 cross products, duplicates dropped).  keep_collinear: the WRONG
    rule `cross < 0` in place of `cross <= 0`, which leaves collinear points on the hull's edges — to show that a case's
    rectangle depends on the rule."""
    pts = sorted(set((float(x), float(y)) for x, y in np.asarray(xy, np.float32).reshape(-1, 2)))
    if len(pts) <= 2:
        return np.array(pts, np.float32).reshape(-1, 2)

    def pops(o, a, b):
        c = F(F(F(a[0]) - F(o[0])) * F(F(b[1]) - F(o[1]))) - F(F(F(a[1]) - F(o[1])) * F(F(b[0]) - F(o[0])))
        return c < 0 if keep_collinear else c <= 0

    h = []
    for p in pts:
        while len(h) >= 2 and pops(h[-2], h[-1], p):
            h.pop()
        h.append(p)
    lower = len(h) + 1
    for p in reversed(pts[:-1]):
        while len(h) >= lower and pops(h[-2], h[-1], p):
            h.pop()
        h.append(p)
    return np.array(h[:-1], np.float32)


def min_edges(areas):
    """The edges attaining the minimum area bit-equal (as float values), ascending; [] for a hull without a rectangle."""
    areas = np.asarray(areas, np.float32)
    ok = areas[~np.isnan(areas)]
    if len(ok) == 0:
        return []
    return [int(v) for v in np.flatnonzero(areas == ok.min())]


def component_facts(mask, slot=None):
    """What a case's branch depends on, for the component in `slot` (default: the one with the longest border): border
    length n, simplified count m, hull size hn, the RDP ties and the per-edge areas, all from clib and the restatements."""
    contours = clib.find_contours_external(mask)
    if slot is None:
        slot = int(np.argmax([len(c) for c in contours]))
    xy = contours[slot][:, ::-1].astype(np.float32)
    simp = clib.simplify_polygon(xy, EPS)
    hull = clib.convex_hull(simp)
    _, ties = rdp_f32(xy)
    areas, _ = edge_areas_f32(hull)
    return {"slot": slot, "n": len(xy), "m": len(simp), "hn": len(hull), "ties": ties, "areas": areas,
            "min_edges": min_edges(areas), "root": (int(contours[slot][0, 0]), int(contours[slot][0, 1]))}


def restatements_equal_clib(mask):
    """Every component of the mask: rdp_f32 == clib.simplify_polygon and edge_areas_f32's rectangle == clib.min_area_rect,
    bit for bit.  -> the number of components checked; raises AssertionError with the slot otherwise."""
    contours = clib.find_contours_external(mask)
    for i, c in enumerate(contours):
        xy = c[:, ::-1].astype(np.float32)
        simp = clib.simplify_polygon(xy, EPS)
        mine, _ = rdp_f32(xy)
        assert mine.shape == simp.shape and np.array_equal(words(mine), words(simp)), ("rdp", i)
        _, rr = edge_areas_f32(clib.convex_hull(simp))
        ref = clib.min_area_rect(simp)
        assert (rr is None) == (ref is None), ("rect", i)
        if ref is not None:
            assert np.array_equal(words(rr), words(ref)), ("rect", i, rr, ref)
    return len(contours)


# ------------------------------------------------------------------ the kernel's mask window, replayed on a contour
def window_loads(contour_yx, h, w, win_w=128, win_h=32):
    """trace_border_wave's window schedule on a border as the oracle walks it: the window starts one row above the root,
    centred on it in x, and is re-centred on the current pixel whenever that pixel's 3 x 3 neighbourhood is not inside.
    -> dict: loads, fast / edge (half rows copied by the 16-byte path / the bytewise path, over all loads), and which sides
    of the image a window hung over."""
    sy, sx = int(contour_yx[0][0]), int(contour_yx[0][1])
    wy0, wx0 = sy - 1, sx - win_w // 2
    origins = [(wy0, wx0)]
    for y, x in contour_yx:
        y, x = int(y), int(x)
        if y - 1 < wy0 or y + 1 >= wy0 + win_h or x - 1 < wx0 or x + 1 >= wx0 + win_w:
            wy0, wx0 = y - win_h // 2, x - win_w // 2
            origins.append((wy0, wx0))
    out = {"loads": len(origins), "fast": 0, "edge": 0, "left": False, "right": False, "top": False, "bottom": False}
    for wy0, wx0 in origins:
        out["left"] |= wx0 < 0
        out["right"] |= wx0 + win_w > w
        out["top"] |= wy0 < 0
        out["bottom"] |= wy0 + win_h > h
        for r in range(win_h):
            for x0 in (wx0, wx0 + win_w // 2):
                fast = 0 <= wy0 + r < h and x0 >= 0 and x0 + win_w // 2 <= w
                out["fast" if fast else "edge"] += 1
    return out
