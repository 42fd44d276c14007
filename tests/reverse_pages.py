"""Planted pages for the reverse-video repair with their answers stated by hand, shared by
test_reverse_cpu.py (small canvases) and test_gpu_reverse.py (canvases of several 64 x 64 tiles, the bands placed across
word and tile boundaries).  Paper is +0.25, ink -0.25; a band is 12 x 40 and the parameters are SMALL unless stated."""
import numpy as np

F = np.float32
PAPER, INK = F(0.25), F(-0.25)
SMALL = {"min_height": 8, "min_width": 24}   # min_fill 0.4, min_holes 3, max_hole 0: the defaults
BAND_H, BAND_W = 12, 40
NEED = (31, 61)   # the canvas from (oy, ox) on that the largest pattern (nested, 30 x 60, a pixel of paper after it) takes


def canvas(h, w):
    return np.full((h, w), PAPER, F)


def box(h, w, y, x, hh, ww):
    m = np.zeros((h, w), bool)
    m[y:y + hh, x:x + ww] = True
    return m


def band_with_marks(h, w, oy, ox, marks):
    """A 12 x 40 band at (oy, ox) with 3 x 3 light marks at the given (dy, dx) inside it."""
    a = canvas(h, w)
    a[oy:oy + BAND_H, ox:ox + BAND_W] = INK
    for dy, dx in marks:
        a[oy + dy:oy + dy + 3, ox + dx:ox + dx + 3] = PAPER
    return a


FOUR = [(4, 3), (4, 12), (5, 21), (4, 30)]


def patterns(h, w, oy, ox):
    """-> [(name, page, params, flipped (bool [h, w]), info (the fields stated by hand))] on an h x w canvas, the bands' top
    left corner at (oy, ox) with oy, ox >= 1 and NEED more rows and columns after it."""
    assert oy >= 1 and ox >= 1 and oy + NEED[0] <= h and ox + NEED[1] <= w, (h, w, oy, ox)
    none = np.zeros((h, w), bool)
    band = box(h, w, oy, ox, BAND_H, BAND_W)
    out = []

    a = band_with_marks(h, w, oy, ox, FOUR)
    out.append(("band, four marks", a, SMALL, band,
                {"ink": 444, "components": 1, "candidates": 1, "panels": 1, "panel_pixels": 444, "holes": 4, "hole_pixels": 36,
                 "skipped_holes": 0, "inverted": 480}))
    a = band_with_marks(h, w, oy, ox, FOUR[:2])
    out.append(("band, two marks", a, SMALL, none, {"candidates": 1, "panels": 0, "inverted": 0}))
    out.append(("band, two marks, min_holes 2", a, dict(SMALL, min_holes=2), band, {"panels": 1, "holes": 2, "inverted": 480}))
    out.append(("band, two marks, min_holes 0", a, dict(SMALL, min_holes=0), band, {"panels": 1, "holes": 2, "inverted": 480}))
    out.append(("band, four marks, too low for min_height", band_with_marks(h, w, oy, ox, FOUR), dict(SMALL, min_height=13), none,
                {"components": 1, "candidates": 0, "inverted": 0}))

    a = canvas(h, w)   # a one-pixel outline: 100 pixels in a box of 480, 256 * 100 < 102 * 480
    a[oy:oy + BAND_H, ox:ox + BAND_W] = INK
    a[oy + 1:oy + BAND_H - 1, ox + 1:ox + BAND_W - 1] = PAPER
    out.append(("outline", a, SMALL, none, {"ink": 100, "components": 1, "candidates": 0, "inverted": 0}))
    out.append(("outline, min_fill 0.2 and min_holes 1", a, dict(SMALL, min_fill=0.2, min_holes=1), band,
                {"candidates": 1, "panels": 1, "holes": 1, "hole_pixels": 380, "inverted": 480}))

    marks = [(0, 3), (4, 12), (5, 21)]   # the first reaches the band's upper edge: it joins the paper outside and is open
    a = band_with_marks(h, w, oy, ox, marks)
    out.append(("band, a mark at its edge", a, SMALL, none, {"candidates": 1, "panels": 0, "inverted": 0}))
    out.append(("band, a mark at its edge, min_holes 2", a, dict(SMALL, min_holes=2), band & ~box(h, w, oy, ox + 3, 3, 3),
                {"panels": 1, "holes": 2, "hole_pixels": 18, "panel_pixels": 480 - 27, "inverted": 480 - 9}))

    a = canvas(h, w)   # a band along the page's upper edge, from its left edge to its right one
    a[:BAND_H] = INK
    for dy, dx in FOUR:
        a[dy:dy + 3, ox + dx:ox + dx + 3] = PAPER
    out.append(("band at three page edges", a, SMALL, box(h, w, 0, 0, BAND_H, w),
                {"candidates": 1, "panels": 1, "holes": 4, "hole_pixels": 36, "inverted": BAND_H * w}))

    # a 6 x 20 light card with a dark 2 x 2 island, and three marks: the card's hole holds the island, 120 pixels
    a = band_with_marks(h, w, oy, ox, [(4, 24), (4, 28), (4, 32)])
    a[oy + 3:oy + 9, ox + 2:ox + 22] = PAPER
    a[oy + 5:oy + 7, ox + 10:ox + 12] = INK
    card = box(h, w, oy + 3, ox + 2, 6, 20)
    out.append(("band, a card over max_hole", a, dict(SMALL, max_hole=50), band & ~card,
                {"components": 2, "candidates": 1, "panels": 1, "holes": 3, "hole_pixels": 27, "skipped_holes": 1, "inverted": 480 - 120}))
    out.append(("band, a card at max_hole", a, dict(SMALL, max_hole=120), band, {"holes": 4, "hole_pixels": 147, "skipped_holes": 0}))
    out.append(("band, a card under max_hole", a, dict(SMALL, max_hole=119), band & ~card, {"holes": 3, "skipped_holes": 1}))
    out.append(("band, a card, no limit", a, SMALL, band,
                {"panels": 1, "holes": 4, "hole_pixels": 147, "skipped_holes": 0, "panel_pixels": 480 - 147, "inverted": 480}))

    a = band_with_marks(h, w, oy, ox, [(4, 3), (4, 12)])   # a 5 x 5 mark with a dark pixel in it: the pixel is of the hole
    a[oy + 3:oy + 8, ox + 20:ox + 25] = PAPER
    a[oy + 5, ox + 22] = INK
    out.append(("band, an island in a hole", a, dict(SMALL, max_hole=25), band,
                {"components": 2, "candidates": 1, "panels": 1, "holes": 3, "hole_pixels": 43, "inverted": 480}))
    out.append(("band, an island in a hole, max_hole 24", a, dict(SMALL, max_hole=24), none, {"panels": 0, "holes": 0, "skipped_holes": 0}))

    # a candidate inside a hole of another: a 30 x 60 band, a 20 x 40 card in it, a 12 x 30 band with three 2 x 2 marks in that
    def nested(outer_marks):
        a = canvas(h, w)
        a[oy:oy + 30, ox:ox + 60] = INK
        a[oy + 5:oy + 25, ox + 10:ox + 50] = PAPER
        a[oy + 9:oy + 21, ox + 15:ox + 45] = INK
        for dx in (4, 12, 20):
            a[oy + 14:oy + 16, ox + 15 + dx:ox + 17 + dx] = PAPER
        for dx in outer_marks:
            a[oy + 1:oy + 3, ox + dx:ox + dx + 2] = PAPER
        return a

    inner = box(h, w, oy + 9, ox + 15, 12, 30)
    out.append(("nested, the inner band alone", nested(()), SMALL, inner,
                {"components": 2, "candidates": 2, "panels": 1, "holes": 3, "hole_pixels": 12, "inverted": 360}))
    out.append(("nested, both", nested((5, 15, 25)), SMALL, box(h, w, oy, ox, 30, 60),
                {"candidates": 2, "panels": 2, "holes": 7, "hole_pixels": 12 + 12 + (800 - 360), "inverted": 1800}))
    out.append(("nested, the card over max_hole", nested((5, 15, 25)), dict(SMALL, max_hole=100),
                (box(h, w, oy, ox, 30, 60) & ~box(h, w, oy + 5, ox + 10, 20, 40)) | inner,
                {"panels": 2, "holes": 6, "skipped_holes": 1}))
    return out
