"""Hand-made pages for the despeckling tests: paper at +0.4, ink at -0.4.  test_despeckle_cpu.py states
what the definition makes of each; test_gpu_despeckle.py holds the library to the definition on the same pages."""
import numpy as np

F = np.float32
PAPER, INK = F(0.4), F(-0.4)
PAPER_FILL = F(231.0 / 256.0 - 0.5)   # the level of that paper's bin: what a removed speck becomes
INK_FILL = F(25.0 / 256.0 - 0.5)      # the level of that ink's bin: what a filled hole becomes


def paper(h, w):
    return np.full((h, w), PAPER, F)


def page_of(ink):
    return np.where(ink, INK, PAPER).astype(F)


def blob(area):
    """`area` pixels of an 8-connected shape as (dy, dx): rows of three, filled in raster order."""
    return [(i // 3, i % 3) for i in range(area)]


def plant(page, y, x, area):
    for dy, dx in blob(area):
        page[y + dy, x + dx] = INK


def blob_sites(h, w, area):
    """Where a blob of `area` is planted: the four corners, across x = 63|64 and across y = 63|64 (top-left pixel of the
    blob's box), far enough apart that no two touch."""
    bh, bw = (area + 2) // 3, min(area, 3)
    sites = [(0, 0), (0, w - bw), (h - bh, 0), (h - bh, w - bw)]
    if w > 70:
        sites.append((20, 64 - (bw + 1) // 2 if bw > 1 else 63))
    if h > 70:
        sites.append((64 - (bh + 1) // 2 if bh > 1 else 63, 30))
    if w > 70 and h > 70:
        sites.append((63, 63))
    return sites


def planted_blobs(h, w, area):
    page = paper(h, w)
    for y, x in blob_sites(h, w, area):
        plant(page, y, x, area)
    return page


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return page_of((yy + xx) % 2 == 0)


def diagonals(h, w, step=4, anti=False):
    yy, xx = np.mgrid[0:h, 0:w]
    return page_of(((xx + yy) if anti else (xx - yy)) % step == 0)


def serpentine(h, w, invert=False):
    """Full rows of ink on every other row, joined at alternating ends: one component of ink that visits the whole page,
    the root of which is its first pixel and the last row of which is h * w / 2 unions away.  invert: the same of paper,
    where the joins are 4-connected."""
    ink = np.zeros((h, w), bool)
    ink[0::2, :] = True
    ink[1::4, w - 1] = True
    ink[3::4, 0] = True
    return page_of(~ink if invert else ink)


def spiral(h, w, invert=False):
    """A one-pixel line that spirals inwards clockwise from the top-left corner with one pixel between its turns."""
    ink = np.zeros((h, w), bool)
    y, x, dy, dx, turns = 0, 0, 0, 1, 0
    ink[0, 0] = True

    def is_ink(yy, xx):
        return 0 <= yy < h and 0 <= xx < w and ink[yy, xx]

    while turns < 2:
        ny, nx = y + dy, x + dx
        if 0 <= ny < h and 0 <= nx < w and not ink[ny, nx] and not is_ink(ny + dy, nx + dx):
            y, x, turns = ny, nx, 0
            ink[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return page_of(~ink if invert else ink)


def u_shape(h, w):
    """Two one-pixel arms the height of the page that meet only in the bottom row; a second U upside down beside it."""
    ink = np.zeros((h, w), bool)
    ink[:, 3] = ink[:, w // 2] = True
    ink[h - 1, 3:w // 2 + 1] = True
    ink[:h - 2, w // 2 + 3] = ink[:h - 2, w - 2] = True
    ink[0, w // 2 + 3:w - 1] = True
    return page_of(ink)


def corner_pairs(h, w):
    """(page with two ink pixels touching by a corner, twice; page of ink with two paper pixels touching by a corner)."""
    a = paper(h, w)
    a[5, 5] = a[6, 6] = INK
    a[10, 64] = a[11, 63] = INK
    b = np.full((h, w), INK, F)
    b[5, 5] = b[6, 6] = PAPER
    b[10, 64] = b[11, 63] = PAPER
    return a, b


NEAR_KINDS = ("word", "row", "diagonal", "edge", "pair")


def near_case(h, w, kind, d):
    """A 4 x 4 block of ink and one-pixel specks at Chebyshev distance d (1 .. 17) from it: across the word boundary
    x = 63|64, across the tile row y = 63|64, diagonally across both, or along the page's edges; "pair": two specks at
    distance d (at least 2) from each other and far from the block -> (page, [(y, x) of the specks])."""
    page = paper(h, w)
    if kind == "word":
        page[30:34, 64 - d - 3:64 - d + 1] = INK
        specks = [(31, 64)]
    elif kind == "row":
        page[64 - d - 3:64 - d + 1, 30:34] = INK
        specks = [(64, 31)]
    elif kind == "diagonal":
        page[64 - d - 3:64 - d + 1, 64 - d - 3:64 - d + 1] = INK
        specks = [(64, 64)]
    elif kind == "edge":
        page[h - 4:h, 0:4] = INK
        page[d:d + 4, w - 4:w] = INK
        specks = [(h - 1, 3 + d), (0, w - 1)]
    else:
        page[100:104, 100:104] = INK
        specks = [(50, 50), (50, 50 + d)]
    for y, x in specks:
        page[y, x] = INK
    return page, specks


def patterns(h, w):
    """(name, page, parameter sets) of every pattern, for a page of h x w (both over 100)."""
    small = [{"max_area": A, "max_hole": Hm, "keep_near": K} for A, Hm, K in ((1, 1, 0), (2, 2, 1), (4, 0, 3), (9, 4, 2))]
    big = [{"max_area": 4096, "max_hole": 4096, "keep_near": 16}, {"max_area": 100, "max_hole": 300, "keep_near": 1}]
    out = []
    for A in (1, 2, 4, 9):
        for area in (A, A + 1):
            out.append(("blobs of %d at A = %d" % (area, A), planted_blobs(h, w, area), [{"max_area": A}, {"max_area": A, "keep_near": 2}]))
    a, b = corner_pairs(h, w)
    out.append(("ink pixels touching by a corner", a, [{"max_area": 1}, {"max_area": 2}]))
    out.append(("paper pixels touching by a corner", b, [{"max_hole": 1, "max_area": 0}, {"max_hole": 2}]))
    out.append(("checkerboard", checkerboard(h, w), small + big))
    out.append(("diagonals", diagonals(h, w), small + big))
    out.append(("anti-diagonals", diagonals(h, w, 3, True), small + big))
    for inv in (False, True):
        out.append(("serpentine%s" % (" of paper" if inv else ""), serpentine(h, w, inv), small + big))
        out.append(("spiral%s" % (" of paper" if inv else ""), spiral(h, w, inv), small + big))
    out.append(("u", u_shape(h, w), small + big))
    for K in (1, 2, 8, 16):
        for kind in NEAR_KINDS:
            for d in (K, K + 1):
                if kind != "pair" or d >= 2:
                    out.append(("%s at %d, K = %d" % (kind, d, K), near_case(h, w, kind, d)[0], [{"max_area": 1, "keep_near": K}]))
    return out
