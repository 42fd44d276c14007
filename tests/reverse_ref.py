"""Reverse-video repair, restated in numpy: the specification the library equals bit for bit.

A prepared page v (float32 [H, W], centred on 0) comes back with the solid dark panels that enclose light marks, and what
they enclose, turned to dark on light: the sign bit of those pixels is flipped, every other pixel keeps its own 32-bit
word.  Everything is integer and set arithmetic on sets taken from the INPUT page; nothing is iterated to a fixed point
except the labelling.  unreverse(page, threshold, min_height, min_width, min_fill, min_holes, max_hole) -> (out, mask, info).

  1 ink    = v < threshold (an ordinary float compare: NaN is not ink, v == threshold is not).  Its 8-connected components
    have an area A and a bounding box bh x bw; the page edge is a wall.
  2 a component is a candidate when bh >= min_height, bw >= min_width and 256 A >= q bh bw in integers,
    q = floor(256 min_fill + 0.5).  M = the pixels of the candidates.
  3 everything outside M (paper, NaN, the ink of non-candidates) is labelled with 4-connectivity.  Such a component is open
    when it holds a pixel of the page's first or last row or column, otherwise a hole of area a.  A hole's encloser is the
    candidate that owns the pixel west of the hole's raster-first pixel (the first pixel of its least row): that pixel is
    in M, or it would belong to the hole.  A hole counts when max_hole == 0 or a <= max_hole.
  4 a candidate is a panel when at least min_holes counting holes have it as their encloser.
  5 the sign bit is flipped on every pixel of a panel and of a counting hole whose encloser is a panel.
  mask bits: 0 inverted, 1 in M, 2 in a panel, 3 in a hole (counting or not, whatever its encloser).
  info (INFO_KEYS, in the order of ocrs_reverse_info): ink, components, candidates, panels, panel_pixels, holes (counting
  holes of panels), hole_pixels (theirs), skipped_holes (holes of panels over max_hole), inverted.

The five defaults (32, 64, 0.4, 3, 0) are UNCALIBRATED: no real scans exist here.

Two implementations that share nothing but the ink set's definition: unreverse() is vectorised (components by a union over
the horizontal runs, boxes by minimum / maximum, the raster-first pixel by a first occurrence); unreverse_slow() walks the
page pixel by pixel (flood fill, the encloser by stepping west).  test_reverse_cpu.py holds them to each other.
"""
import math

import numpy as np

from despeckle_ref import components

F = np.float32
INFO_KEYS = ("ink", "components", "candidates", "panels", "panel_pixels", "holes", "hole_pixels", "skipped_holes", "inverted")
MAX_SIDE = 65535
SIGN = np.uint32(0x80000000)


def default_params():
    return {"threshold": 0.0, "min_height": 32, "min_width": 64, "min_fill": 0.4, "min_holes": 3, "max_hole": 0}


def valid_params(threshold=0.0, min_height=32, min_width=64, min_fill=0.4, min_holes=3, max_hole=0):
    ints = all(isinstance(v, (int, np.integer)) for v in (min_height, min_width, min_holes, max_hole))
    return bool(ints and np.isfinite(threshold) and 1 <= min_height <= MAX_SIDE and 1 <= min_width <= MAX_SIDE
                and 0.0 <= float(min_fill) <= 1.0 and min_holes >= 0 and max_hole >= 0)


def fill_q8(min_fill):
    """min_fill in 1/256, computed in float32 as the library does."""
    return int(math.floor(float(F(F(256.0) * F(min_fill) + F(0.5)))))


def analyse(page, threshold=0.0):
    """What depends on the page and the threshold alone: ink, its labelling, the components' areas and boxes."""
    v = np.ascontiguousarray(page, F)
    with np.errstate(invalid="ignore"):
        ink = v < F(threshold)
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
    return {"v": v, "ink": ink, "label": label, "area": area, "bh": y1 - y0 + 1, "bw": x1 - x0 + 1, "holes_of": {}}


def finish(v, M, panel_px, hole_px, flip_hole_px, info):
    flip = panel_px | flip_hole_px
    out = v.copy()
    out.view(np.uint32)[flip] ^= SIGN
    mask = (flip * 1 + M * 2 + panel_px * 4 + hole_px * 8).astype(np.uint8)
    info["inverted"] = int(flip.sum())
    assert tuple(info) == INFO_KEYS
    return out, mask, info


def unreverse(page, threshold=0.0, min_height=32, min_width=64, min_fill=0.4, min_holes=3, max_hole=0, analysis=None):
    """-> (out float32 [H, W], mask uint8 [H, W], info dict).  analysis: analyse(page, threshold), to share it between calls."""
    if not valid_params(threshold, min_height, min_width, min_fill, min_holes, max_hole):
        raise ValueError("unreverse: parameters out of range")
    a = analysis if analysis is not None else analyse(page, threshold)
    v, label, area, bh, bw = a["v"], a["label"], a["area"], a["bh"], a["bw"]
    H, W = v.shape
    q = fill_q8(min_fill)
    cand = (bh >= int(min_height)) & (bw >= int(min_width)) & (256 * area >= q * bh * bw)   # int64: q bh bw < 2^41
    cand[0] = False
    M = cand[label]
    key = M.tobytes()
    if key not in a["holes_of"]:   # the complement's labelling depends on M alone
        clabel, carea = components(~M, False)
        n = len(carea) - 1
        is_open = np.zeros(n + 1, bool)
        for edge in (clabel[0], clabel[-1], clabel[:, 0], clabel[:, -1]):
            is_open[edge] = True
        is_open[0] = True   # label 0 is M: no component
        _, first = np.unique(clabel.reshape(-1), return_index=True)   # the raster-first pixel of 0 (if any), 1 .. n
        first = first[-n:] if n else first[:0]
        enc = np.zeros(n + 1, np.int64)
        holes = np.nonzero(~is_open)[0]
        fy, fx = first[holes - 1] // W, first[holes - 1] % W
        assert (fx >= 1).all() and M[fy, fx - 1].all(), "the pixel west of a hole's first pixel is in M"
        enc[holes] = label[fy, fx - 1]
        a["holes_of"][key] = (clabel, carea, is_open, enc)
    clabel, carea, is_open, enc = a["holes_of"][key]
    hole = ~is_open
    counting = hole & ((carea <= int(max_hole)) if int(max_hole) > 0 else True)
    per_cand = np.bincount(enc[counting], minlength=len(area))
    panel = cand & (per_cand >= int(min_holes))
    flipped = counting & panel[enc]
    skipped = hole & ~counting & panel[enc]
    panel_px = panel[label]
    info = {"ink": int(a["ink"].sum()), "components": int(len(area) - 1), "candidates": int(cand.sum()), "panels": int(panel.sum()),
            "panel_pixels": int(panel_px.sum()), "holes": int(flipped.sum()), "hole_pixels": int(carea[flipped].sum()),
            "skipped_holes": int(skipped.sum()), "inverted": 0}
    return finish(v, M, panel_px, hole[clabel], flipped[clabel], info)


def flood(member, H, W, diagonal):
    """Components by flood fill in raster order -> (label [H][W], 1 .. n on `member`, 0 elsewhere; the pixels of each)."""
    label = [[0] * W for _ in range(H)]
    comps = [None]
    for y in range(H):
        for x in range(W):
            if not member[y][x] or label[y][x]:
                continue
            k = len(comps)
            label[y][x] = k
            stack, px = [(y, x)], []
            while stack:
                cy, cx = stack.pop()
                px.append((cy, cx))
                near = [(cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)]
                if diagonal:
                    near += [(cy - 1, cx - 1), (cy - 1, cx + 1), (cy + 1, cx - 1), (cy + 1, cx + 1)]
                for ny, nx in near:
                    if 0 <= ny < H and 0 <= nx < W and member[ny][nx] and not label[ny][nx]:
                        label[ny][nx] = k
                        stack.append((ny, nx))
            comps.append(px)
    return label, comps


def unreverse_slow(page, threshold=0.0, min_height=32, min_width=64, min_fill=0.4, min_holes=3, max_hole=0):
    """The same by walking: flood fills, sets of pixels, the encloser by stepping west from the hole's first pixel."""
    if not valid_params(threshold, min_height, min_width, min_fill, min_holes, max_hole):
        raise ValueError("unreverse: parameters out of range")
    v = np.ascontiguousarray(page, F)
    H, W = v.shape
    thr = F(threshold)
    ink = [[bool(v[y, x] < thr) for x in range(W)] for y in range(H)]   # NaN < thr is False
    label, comps = flood(ink, H, W, True)
    q = fill_q8(min_fill)
    cands = set()
    for k in range(1, len(comps)):
        ys, xs = [p[0] for p in comps[k]], [p[1] for p in comps[k]]
        bh, bw = max(ys) - min(ys) + 1, max(xs) - min(xs) + 1
        if bh >= min_height and bw >= min_width and 256 * len(comps[k]) >= q * bh * bw:
            cands.add(k)
    inM = [[label[y][x] in cands for x in range(W)] for y in range(H)]
    _, others = flood([[not inM[y][x] for x in range(W)] for y in range(H)], H, W, False)
    holes = []   # (pixels, encloser, counting)
    for px in others[1:]:
        if any(y in (0, H - 1) or x in (0, W - 1) for y, x in px):
            continue
        fy, fx = min(px)   # the least row, then the least column
        x = fx - 1         # one step west: off the hole, so on a candidate
        assert x >= 0 and inM[fy][x]
        holes.append((px, label[fy][x], max_hole == 0 or len(px) <= max_hole))
    count = {k: 0 for k in cands}
    for px, k, counting in holes:
        count[k] += 1 if counting else 0
    panels = {k for k in cands if count[k] >= min_holes}
    M, panel_px, hole_px, flip_px = (np.zeros((H, W), bool) for _ in range(4))
    for k in cands:
        for y, x in comps[k]:
            M[y, x] = True
            panel_px[y, x] = k in panels
    info = {"ink": sum(sum(r) for r in ink), "components": len(comps) - 1, "candidates": len(cands), "panels": len(panels),
            "panel_pixels": int(panel_px.sum()), "holes": 0, "hole_pixels": 0, "skipped_holes": 0, "inverted": 0}
    for px, k, counting in holes:
        for y, x in px:
            hole_px[y, x] = True
            flip_px[y, x] = counting and k in panels
        if k in panels:
            info["holes" if counting else "skipped_holes"] += 1
            info["hole_pixels"] += len(px) if counting else 0
    return finish(v, M, panel_px, hole_px, flip_px, info)


def same(a, b):
    """Two results (out, mask, info) are equal word for word, byte for byte and count for count."""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and tuple(a[2]) == INFO_KEYS
