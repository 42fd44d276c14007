"""Named masks that drive contour_rect_kernel (kernels_ccl.hip) into each of its size-dependent branches, each as small
as its branch allows.  test_contour_cases_cpu.py proves from the oracle alone that every case reaches its branch (the
`expect` facts: border length n, simplified count m, hull size hn, tie positions); test_gpu_contour.py sends them through
ocrs_mask_component_rects and detect_words.  Parameters that needed a search (tooth counts, arm lengths, the dropped
tooth) were found on the CPU oracle and are committed as numbers; no generated data is.

The kernel's constants the cases straddle: kWalkBuf = 1024 border points in LDS, kSmallPoly = 64 simplified points with
LDS scratch, 64 lanes per stride of the RDP pivot search and of the rectangle's edge search, a 128 x 32 mask window.
"""
import numpy as np

WALK_BUF = 1024
SMALL_POLY = 64
LANES = 64
WIN_W, WIN_H = 128, 32


class Case:
    def __init__(self, name, group, mask, **expect):
        self.name, self.group, self.mask, self.expect = name, group, np.ascontiguousarray(mask, np.uint8), expect

    def __repr__(self):
        return "Case(%s)" % self.name


# ------------------------------------------------------------------ generators
def bar(a, b, clip=False, pad=2):
    """A solid a x b rectangle (n = 2 (a + b) - 4); clip: without its top right corner pixel (one point fewer)."""
    m = np.zeros((a + 2 * pad, b + 2 * pad), np.uint8)
    m[pad:pad + a, pad:pad + b] = 1
    if clip:
        m[pad, pad + b - 1] = 0
    return m


def comb(teeth, length, extra=0, spur=0):
    """A bar three rows thick with `teeth` one-pixel teeth of `length` rows hanging from every 4th column; extra: the bar
    runs on that many columns past the last tooth; spur: a one-pixel spur of that height standing on the bar at column 20."""
    m = np.zeros((length + 16, 4 * teeth + 8 + extra), np.uint8)
    m[8:11, 2:2 + 4 * (teeth - 1) + 1 + extra] = 1
    for i in range(teeth):
        m[11:11 + length, 2 + 4 * i] = 1
    if spur:
        m[8 - spur:8, 20] = 1
    return m


def long_comb():
    """test_gpu_r3's comb at 64 x 400: bar rows 2..4, teeth every 4th column over rows 5..29."""
    m = np.zeros((64, 400), np.uint8)
    m[2:5, 2:398] = 1
    m[5:30, 2:398:4] = 1
    return m


def toothed_ellipse(a, b, teeth, depth=6, rot=0.0, drop=None):
    """Pixel (y, x) of a square of side 2 max(a, b) + 12 is set when hypot(X / a, Y / b) < 1 - (depth / min(a, b)) *
    (cos(teeth * atan2(Y / b, X / a)) < 0), (X, Y) the offset from the centre (side / 2) turned by rot.  drop: tooth
    number `drop` (counted in the ellipse's own angle from its X axis) is cut down to the notches' depth."""
    s = 2 * max(a, b) + 12
    yy, xx = np.mgrid[0:s, 0:s].astype(np.float64)
    dx, dy = xx - s / 2.0, yy - s / 2.0
    X = dx * np.cos(rot) + dy * np.sin(rot)
    Y = -dx * np.sin(rot) + dy * np.cos(rot)
    ang = np.arctan2(Y / b, X / a)
    notch = np.cos(teeth * ang) < 0
    if drop is not None:
        notch |= np.floor(np.mod(teeth * ang / (2 * np.pi) + 0.5, teeth)) == drop
    return (np.hypot(X / a, Y / b) < 1 - (depth / min(a, b)) * notch).astype(np.uint8)


def bumps(spacing, mirrored=False, first=60):
    """A bar (rows 10..13, columns 10..389 of 40 x 400) with two bumps 4 columns wide and 3 rows tall, at columns `first`
    and `first + spacing`, hanging under it (mirrored: standing on it)."""
    m = np.zeros((40, 400), np.uint8)
    m[10:14, 10:390] = 1
    for c in (first, first + spacing):
        if mirrored:
            m[7:10, c:c + 4] = 1
        else:
            m[14:17, c:c + 4] = 1
    return m


def corner_l(arm, thick=1, inner=False):
    """An L whose corner is its raster-first pixel: arms of `arm` pixels to the right and down, `thick` wide; inner: the
    pixel in the inner corner is set as well (the walk cuts that corner: one point fewer between the two arm ends)."""
    m = np.zeros((arm + 6, arm + 6), np.uint8)
    m[3:3 + thick, 3:3 + arm] = 1
    m[3:3 + arm, 3:3 + thick] = 1
    if inner:
        m[3 + thick, 3 + thick] = 1
    return m


def fork(d):
    """A one-pixel diagonal from the root with a two-pixel fork at its end: the fork's pixels are equally far from the root
    and tie on the closing segment (root to root, distance |p - root|), one index apart.  The one that becomes a vertex
    leaves the other within eps of the polygon: m = 2, and WHICH one decides the rectangle's axis."""
    m = np.zeros((d + 6, d + 6), np.uint8)
    for i in range(d + 1):
        m[2 + i, 2 + i] = 1
    m[2 + d + 1, 2 + d] = m[2 + d, 2 + d + 1] = 1
    return m


def notched_band(length, thick, notch):
    """A band of slope 1/2 (pixels with 0 <= u < length, 0 <= 2 v - u <= 2 thick) with a notch (start, width, depth) cut
    into its upper side: the notch's rim survives simplification and lies ON the hull edge along that side — collinear
    points the hull must drop.  Kept, they split the edge the minimum-area rectangle rests on into pieces whose float32
    directions and base points differ in the last bits."""
    m = np.zeros((length // 2 + thick + 12, length + 12), np.uint8)
    yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    u, v = xx - 4, yy - 4
    m[(u >= 0) & (u < length) & (2 * v - u >= 0) & (2 * v - u <= 2 * thick)] = 1
    n0, nw, nd = notch
    m[(u >= n0) & (u < n0 + nw) & (2 * v - u < 2 * nd)] = 0
    return m


def degenerate_page():
    """Group d in one page: a pixel, 2 x 2 and 3 x 3 blocks, lines 1 x L and L x 1 for L = 2 .. 14, both diagonals, L-shaped
    and collinear triples, and the 5 x 5 square whose expanded rectangle has area exactly 100."""
    m = np.zeros((120, 128), np.uint8)
    m[2, 2] = 1                                   # slot 0: a single pixel
    m[2:4, 6:8] = 1                               # 2 x 2
    m[2:5, 11:14] = 1                             # 3 x 3
    m[2:7, 18:23] = 1                             # 5 x 5
    for i in range(8):                            # both diagonals
        m[2 + i, 28 + i] = 1
        m[2 + i, 47 - i] = 1
    for t, (dy1, dx1, dy2, dx2) in enumerate([(0, 1, 1, 1), (0, 1, 1, 0), (1, 0, 1, 1), (1, -1, 1, 0),      # L-shaped triples
                                              (0, 1, 0, 2), (1, 0, 2, 0), (1, 1, 2, 2), (1, -1, 2, -2)]):   # collinear triples
        y, x = 2, 54 + 8 * t
        m[y, x] = m[y + dy1, x + dx1] = m[y + dy2, x + dx2] = 1
    y = 14
    for L in range(2, 15):                        # 1 x L, two per row band
        m[y + 2 * ((L - 2) // 2), 2 + 20 * (L % 2):2 + 20 * (L % 2) + L] = 1
    for L in range(2, 15):                        # L x 1
        m[32:32 + L, 44 + 4 * (L - 2)] = 1
    return m


def window_shapes():
    """Group f, components that outgrow the 128 x 32 window from their root, 96 x 400: a bar 300 wide, a post 70 tall, and a
    spiral whose walk leaves the window and comes back several times."""
    m = np.zeros((96, 400), np.uint8)
    m[2:5, 2:302] = 1                             # wider than the window
    m[8:78, 4:7] = 1                              # taller than the window
    y0, y1, x0, x1 = 8, 92, 12, 396               # a rectangular spiral, arms 2 thick, 6 apart
    while y1 - y0 > 12 and x1 - x0 > 12:
        m[y0:y0 + 2, x0:x1] = 1
        m[y0:y1, x1 - 2:x1] = 1
        m[y1 - 2:y1, x0 + 8:x1] = 1
        m[y0 + 8:y1, x0 + 8:x0 + 10] = 1
        m[y0 + 8:y0 + 10, x0 + 8:x1 - 8] = 1
        y0, y1, x0, x1 = y0 + 8, y1 - 8, x0 + 8, x1 - 8
    return m


def corner_blobs(h=70, w=200):
    """The same blob (a 9 x 21 block with a notch and a spur) pushed into each of the four corners of the page: the window's
    bytewise edge path and the zeros outside the image, on every side."""
    blob = np.ones((9, 21), np.uint8)
    blob[0:3, 8:12] = 0
    blob[6:9, 0:2] = 0
    blob[4, 18:21] = 0
    m = np.zeros((h, w), np.uint8)
    m[:9, :21] = blob
    m[:9, w - 21:] = blob[:, ::-1]
    m[h - 9:, :21] = blob[::-1]
    m[h - 9:, w - 21:] = blob[::-1, ::-1]
    return m


NOISE_W = (1, 2, 63, 64, 65, 127, 128, 129, 193)
NOISE_H = (1, 2, 31, 32, 33)


def noise_masks():
    """Group f: full and 50 % noise masks at every w in NOISE_W by h in NOISE_H."""
    rng = np.random.default_rng(7)
    out = []
    for h in NOISE_H:
        for w in NOISE_W:
            out.append(Case("full_%dx%d" % (h, w), "f", np.ones((h, w), np.uint8)))
            out.append(Case("noise50_%dx%d" % (h, w), "f", rng.random((h, w)) < 0.5))
    return out


PATTERN_PAGES, PATTERN_SIDE, PATTERN_PITCH = 4, 768, 6


def pattern_pages():
    """Group g: all 65 536 patterns of 4 x 4 pixels, one per cell of a 6-pixel lattice (two empty rows and columns between
    neighbours: no two patterns touch), 128 x 128 cells per page, four pages [4, 768, 768].  Pattern p sits in cell p of
    the raster order over the pages; bit 4 r + c of p is pixel (r, c)."""
    per = PATTERN_SIDE // PATTERN_PITCH
    p = np.arange(65536, dtype=np.uint32).reshape(PATTERN_PAGES, per, per)
    pages = np.zeros((PATTERN_PAGES, PATTERN_SIDE, PATTERN_SIDE), np.uint8)
    for r in range(4):
        for c in range(4):
            pages[:, r::PATTERN_PITCH, c::PATTERN_PITCH] = (p >> (4 * r + c)) & 1
    return pages


def capacity_page():
    """Group h, 48 x 64: eleven components of known border lengths (blocks, lines, dots, a ring with an island)."""
    m = np.zeros((48, 64), np.uint8)
    m[2:8, 2:12] = 1
    m[2:4, 16:40] = 1
    m[2, 44] = m[4, 48] = m[6, 52] = 1
    m[12:30, 4:30] = 1
    m[16:26, 8:26] = 0
    m[19:23, 12:20] = 1                      # an island in the ring's hole: not an external component
    m[12:40, 36] = 1
    m[14:20, 42:60] = 1
    m[34:44, 6:9] = 1
    m[40:46, 20:50:3] = 1
    return m


def ordinary_page(seed):
    """A 48 x 64 page of a few blobs, group h's neighbours."""
    rng = np.random.default_rng(100 + seed)
    m = np.zeros((48, 64), np.uint8)
    for _ in range(6):
        y, x = int(rng.integers(1, 36)), int(rng.integers(1, 48))
        m[y:y + int(rng.integers(2, 11)), x:x + int(rng.integers(3, 15))] = 1
    return m


# ------------------------------------------------------------------ the list
def cases():
    """Groups a-f as single-page cases (g and h have their own builders above)."""
    out = [
        # a. walk buffer: n = 1024 exactly, the largest n below (a clipped corner saves one point), the smallest above
        Case("bar_n1024", "a", bar(4, 510), n=1024, m=4),
        Case("bar_n1023", "a", bar(4, 510, clip=True), n=1023),
        Case("bar_n1025", "a", bar(4, 511, clip=True), n=1025),
        Case("long_comb", "a", long_comb(), n=5547, m=298),
        # b. small-polygon scratch: m = 64 and 65, each with the border inside and beyond the walk buffer
        Case("comb_m64_lds", "b", comb(21, 6, extra=3), m=64, n_max=WALK_BUF),
        Case("comb_m65_lds", "b", comb(21, 6, extra=3, spur=1), m=65, n_max=WALK_BUF),
        Case("comb_m64_arena", "b", comb(21, 30, extra=3), m=64, n_min=WALK_BUF + 1),
        Case("comb_m65_arena", "b", comb(21, 30, extra=3, spur=1), m=65, n_min=WALK_BUF + 1),
        # c. hulls of more than 64 edges: the second stride of the rectangle search and its cross-lane tie rule
        Case("ellipse_120_96", "c", toothed_ellipse(120, 120, 96), n=1564, m=280, hn=76, min_edges=[18, 37, 56, 75]),
        Case("ellipse_160x100_110", "c", toothed_ellipse(160, 100, 110, rot=1.2), hn=78, min_edges=[30, 69]),
        Case("ellipse_140x60_90", "c", toothed_ellipse(140, 60, 90, rot=1.57), hn=66, min_edges=[16, 32, 49, 65]),
        Case("ellipse_hn64", "c", toothed_ellipse(140, 60, 90, rot=np.pi / 2), hn=64, min_edges=[16, 31, 48, 63]),
        # (found by a search over rot and the dropped tooth) the only minimum lies in the second stride: it decides the result
        Case("ellipse_first_min_74", "c", toothed_ellipse(160, 100, 110, rot=1.1, drop=27), hn=82, min_edges=[74]),
        # (found by a search over radii and tooth counts for hn = 128) tying edges 64 apart meet in one lane
        Case("ellipse_hn128", "c", toothed_ellipse(240, 240, 132), hn=128, min_edges=[31, 63, 95, 127]),
        # e. RDP ties
        Case("bumps_64", "e", bumps(64), n=772, tie=(61, 390, [123, 124, 125, 126])),
        Case("bumps_30", "e", bumps(30), tie=(61, 390, [89, 90, 91, 92])),
        Case("bumps_128", "e", bumps(128), tie=(61, 390, [187, 188, 189, 190])),
        Case("bumps_64_mirrored", "e", bumps(64, mirrored=True), tie=(437, 766, [701, 702, 703, 704])),
        Case("bumps_30_mirrored", "e", bumps(30, mirrored=True), tie=(437, 766, [735, 736, 737, 738])),
        Case("bumps_128_mirrored", "e", bumps(128, mirrored=True), tie=(437, 766, [637, 638, 639, 640])),
        # the closing segment of an L whose corner is the root runs from the root to the root: the distance is |p - root| and
        # the two arm ends tie; 63 apart they sit in different lanes, 64 apart (inner corner set) in the same lane
        Case("corner_l_33", "e", corner_l(33), tie=(0, 127, [32, 95])),
        Case("corner_l_34_inner", "e", corner_l(34, inner=True), tie=(0, 130, [33, 97])),
        # ties whose resolution shows in the rectangle: the fork's two ends, in neighbouring lanes of one stride and in lane 63 /
        # lane 0 of the next stride
        Case("fork_10", "e", fork(10), m=2, tie=(0, 23, [11, 12])),
        Case("fork_63", "e", fork(63), m=2, tie=(0, 129, [64, 65])),
        # d. collinear points on the hull edge that carries the rectangle
        Case("notched_band_40", "d", notched_band(40, 8, (20, 8, 5)), hn=4),
        Case("notched_band_50", "d", notched_band(50, 10, (15, 6, 4)), hn=4),
        Case("notched_band_60", "d", notched_band(60, 10, (20, 8, 5)), hn=4),
        # d, f
        Case("degenerate", "d", degenerate_page()),
        Case("window_shapes", "f", window_shapes()),
        Case("corner_blobs", "f", corner_blobs()),
    ]
    return out
