"""Tiled detection by its definition, in numpy, for the tests.

The detector's input is Hm x Wm and v the overlap, 0 <= v <= min(Hm, Wm) // 2.  Along one axis of page length L with
model length M (integers, // floors):

    L <= M:  one tile, origin 0, bounds [0, L]
    L >  M:  n = ceil((L - v) / (M - v)) tiles, origins o_i = (i * (L - M)) // (n - 1),
             bounds b_0 = 0, b_n = L, b_i = (o_{i-1} + M + o_i) // 2   (the middle of the overlap of tiles i - 1 and i)

The tiles of a page are the product of the row plan and the column plan, row-major; tile (i, j) starts at
(oy_i, ox_j) and owns the page pixels by_i <= y < by_{i+1}, bx_j <= x < bx_{j+1}.  A tile's input is an Hm x Wm array of
-0.5 with grey[oy : oy + Hm, ox : ox + Wm] (clipped to the page) in its top-left corner; its output is the model's
[Hm, Wm] output for that input.  The stitched map takes every pixel from the tile that owns it.
"""
import numpy as np

BLACK_VALUE = np.float32(-0.5)
OVERLAP_DEFAULT = 100


def axis_plan(L, M, v):
    """-> (origins [n], bounds [n + 1]) as lists of ints."""
    L, M, v = int(L), int(M), int(v)
    assert L >= 1 and M >= 1 and 0 <= v <= M // 2
    if L <= M:
        return [0], [0, L]
    n = -((L - v) // -(M - v))
    o = [(i * (L - M)) // (n - 1) for i in range(n)]
    b = [0] + [(o[i - 1] + M + o[i]) // 2 for i in range(1, n)] + [L]
    return o, b


def check_axis_properties(L, M, v, o, b):
    """The properties the definition promises, asserted on one plan."""
    n = len(o)
    assert len(b) == n + 1 and o[0] == 0 and b[0] == 0 and b[n] == L
    if L <= M:
        assert n == 1
        return
    assert o[n - 1] + M == L, "no tile hangs over the page edge"
    for i in range(1, n):
        assert o[i] > o[i - 1], "strictly increasing origins"
        assert o[i - 1] + M - o[i] >= v, "neighbours overlap by at least v"
    for i in range(n):
        assert o[i] <= b[i] < b[i + 1] <= min(o[i] + M, L)
    # the smallest n for which that is possible: n - 1 tiles with overlaps >= v cover at most (n - 1) * M - (n - 2) * v < L
    assert n >= 2 and (n - 1) * M - (n - 2) * v < L


def page_plan(page_hw, model_hw, v):
    """-> (origin_y, bound_y, origin_x, bound_x)."""
    oy, by = axis_plan(page_hw[0], model_hw[0], v)
    ox, bx = axis_plan(page_hw[1], model_hw[1], v)
    return oy, by, ox, bx


def tile_input(grey, oy, ox, model_hw):
    hm, wm = model_hw
    h, w = grey.shape
    x = np.full((hm, wm), BLACK_VALUE, np.float32)
    part = grey[oy:min(oy + hm, h), ox:min(ox + wm, w)]
    x[:part.shape[0], :part.shape[1]] = part
    return x


def tile_inputs(grey, model_hw, overlap):
    """The tile inputs of a page in tile order (row-major)."""
    oy, by, ox, bx = page_plan(grey.shape, model_hw, overlap)
    return [tile_input(grey, y, x, model_hw) for y in oy for x in ox]


def stitched(grey, run_tile, model_hw, overlap=OVERLAP_DEFAULT):
    """The stitched probability map float32 [H, W]; run_tile: [Hm, Wm] tile input -> [Hm, Wm] model output."""
    grey = np.ascontiguousarray(grey, np.float32)
    hm, wm = model_hw
    oy, by, ox, bx = page_plan(grey.shape, model_hw, overlap)
    P = np.empty(grey.shape, np.float32)
    for i, y0 in enumerate(oy):
        for j, x0 in enumerate(ox):
            out = np.asarray(run_tile(tile_input(grey, y0, x0, model_hw)), np.float32).reshape(hm, wm)
            P[by[i]:by[i + 1], bx[j]:bx[j + 1]] = out[by[i] - y0:by[i + 1] - y0, bx[j] - x0:bx[j + 1] - x0]
    return P


def oracle_run_tile(detector):
    """run_tile through the CPU oracle's detector (oracle.pipeline.TextDetector): detect_text_pixels of an image of exactly
    the model's size pads nothing and resizes nothing — it is the model's output for that input."""
    return lambda x: detector.detect_text_pixels(x[None])


def seam_crossing(lab, ids, page_hw, model_hw, overlap):
    """How many of the components `ids` of the label image `lab` have pixels on both sides of an ownership boundary."""
    oy, by, ox, bx = page_plan(page_hw, model_hw, overlap)
    n = 0
    for k in ids:
        ys, xs = np.nonzero(lab == k)
        if any(ys.min() < b <= ys.max() for b in by[1:-1]) or any(xs.min() < b <= xs.max() for b in bx[1:-1]):
            n += 1
    return n
