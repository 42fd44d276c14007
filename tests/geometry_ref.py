"""The three geometry steps every request passes through, restated in float64, and the case lists their tests walk:
the pad-and-resize of a page to the detector's input (kernels_image.hip resize_pages_kernel), the slice-and-resize of the
probability map back to the page (resize_threshold_kernel) and the plain line crop (kernels_lines.hip crop_lines_kernel).

Plain numpy and the oracle's polygon fill; nothing of the library under test is imported here.  tests/test_geometry_cpu.py
holds the oracle to these restatements and asserts that every case still exercises what it was made for;
tests/test_gpu_geometry.py holds the kernels to the oracle bit for bit and to the restatements within `tol`.
"""
import numpy as np

from oracle import clib

U = 2.0 ** -24                      # half an ulp of 1 in float32
MODEL_HW = (160, 128)               # the callback detector of the tests
FILL = -0.5                         # preprocess.rs:128
REC_H = 64
THR = np.float32(0.2)               # detection.rs:25-37
MIN_AREA = 100.0


# ------------------------------------------------------------------------------------------------ bilinear
def _axis64(out_len, in_len):
    o = np.arange(out_len, dtype=np.float64)
    c = np.clip((o + 0.5) * (float(in_len) / float(out_len)) - 0.5, 0.0, float(in_len - 1))
    i0 = np.minimum(np.floor(c).astype(np.int64), in_len - 1)
    return i0, np.minimum(i0 + 1, in_len - 1), c - i0


def bilinear64(src, out_h, out_w, virt_h=None, virt_w=None, fill=FILL):
    """ONNX Resize linear / half_pixel (bilinear.hpp) of the virtual [virt_h, virt_w] image that is `src` where src has
    pixels and `fill` elsewhere, evaluated in float64 on the float32 taps -> (out float64 [out_h, out_w], tol float64).

        c   = clamp((o + 0.5) * in / out - 0.5, 0, in - 1);  i0 = floor(c); i1 = min(i0 + 1, in - 1); w = c - i0
        out = (1 - wy) * ((1 - wx) * tl + wx * tr) + wy * ((1 - wx) * bl + wx * br)

    The bound on |float32 evaluation - out|, per pixel, derived:

        tol = 4 u (in_w + in_h) D + 8 u A,      u = 2^-24, D = max - min of the pixel's four taps, A = max |tap|

    * The coordinate.  float32 computes fl(fl((o + .5) * fl(in / out)) - .5); (o + .5) is exact.  fl(in / out) is off by a
      relative u, the product by another, and both are relative to a value of at most in_len, so the product is off by at
      most 2 u in_len; the subtraction rounds once more, a value below in_len: 3 u in_len per axis.  4 leaves room for the
      second-order terms.
    * The value.  Inside a cell the interpolant is linear in each coordinate with a slope that is a blend of tap
      differences, each at most D: a coordinate off by e moves the value by at most e D.  The interpolant is continuous
      across cells, so a coordinate whose floor lands on the other side of an integer costs nothing beyond its distance.
    * The blend.  1 - w, two products and a sum per pair, twice nested: five roundings on the way from a tap to the
      result, each at most u times a value no larger than A: below 8 u A.

    Measured over the case lists of this file: the oracle's float32 evaluation reaches at most 0.39 of tol (an 80 x 1 box
    stretched to 2400 columns), 0.27 on the other crops, 0.21 on the maps, 0.14 on the model inputs.  The bound is derived,
    not fitted to that.

    Where a tap is not finite the bound is not a number; the callers compare such pixels by position.  A weight that is
    exactly 0 in float32 and not in float64 (or the reverse) would move a NaN born of 0 * Inf: the case lists plant
    non-finite values only at scales that float32 holds exactly (1, 1/2, 300/128, 300/160), where the weights are the same
    numbers in both."""
    src = np.asarray(src, np.float64)
    sh, sw = src.shape
    vh = sh if virt_h is None else int(virt_h)
    vw = sw if virt_w is None else int(virt_w)
    if (vh, vw) != (sh, sw):
        v = np.full((vh, vw), float(fill), np.float64)
        v[:sh, :sw] = src
    else:
        v = src
    y0, y1, wy = _axis64(out_h, vh)
    x0, x1, wx = _axis64(out_w, vw)
    tl, tr = v[y0[:, None], x0[None, :]], v[y0[:, None], x1[None, :]]
    bl, br = v[y1[:, None], x0[None, :]], v[y1[:, None], x1[None, :]]
    wx, wy = wx[None, :], wy[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        out = (1.0 - wy) * ((1.0 - wx) * tl + wx * tr) + wy * ((1.0 - wx) * bl + wx * br)
        taps = np.stack([tl, tr, bl, br])
        D = taps.max(axis=0) - taps.min(axis=0)
        A = np.abs(taps).max(axis=0)
        tol = 4.0 * U * (vw + vh) * D + 8.0 * U * A
    return out, tol


def check64(what, got, ref, tol):
    """`got` (float32) against a float64 restatement: NaN at the same pixels, Inf wherever the restatement has one (with
    its sign), and within tol everywhere else.  -> the largest |got - ref| / tol over the finite pixels with tol > 0."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    g = got.astype(np.float64)
    gn, rn = np.isnan(g), np.isnan(ref)
    assert np.array_equal(gn, rn), "%s: NaN at %d pixels, the restatement has %d; first difference at %s" % (
        what, int(gn.sum()), int(rn.sum()), tuple(np.argwhere(gn != rn)[0]))
    ri = np.isinf(ref)
    assert np.array_equal(g[ri], ref[ri]), "%s: the restatement is infinite at %d pixels, the result is not the same there" % (what, int(ri.sum()))
    fin = ~rn & ~ri
    with np.errstate(invalid="ignore"):
        err = np.abs(g - ref)
        bad = fin & ~(err <= tol)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d pixels beyond the bound; first at %s: got %r, float64 %r, |diff| %.3e, tol %.3e" % (
            what, int(bad.sum()), bad.size, i, got[i], ref[i], err[i], tol[i]))
    pos = fin & (tol > 0)
    return float((err[pos] / tol[pos]).max()) if pos.any() else 0.0


def same_bits(got, exp, what):
    """detblock_util.same_bits: equal uint32 views outside NaN, NaN at the same positions (payloads are not compared)."""
    assert got.shape == exp.shape and got.dtype == np.float32 and exp.dtype == np.float32, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), "%s: NaN positions differ at %d elements (got %d NaN, expected %d), first %s" % (
        what, int((gn != en).sum()), int(gn.sum()), int(en.sum()), tuple(np.argwhere(gn != en)[0]))
    ne = (np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(exp).view(np.uint32)) & ~gn
    if ne.any():
        i = tuple(np.argwhere(ne)[0])
        raise AssertionError("%s: %d of %d elements differ in bits; first at %s: got %r, expected %r" % (
            what, int(ne.sum()), ne.size, i, got[i], exp[i]))


# ------------------------------------------------------------------------------------------------ the plain crop
def poly_box(poly):
    """(top, left, bh, bw) of a line polygon [(x, y)]: what the crop resizes from."""
    xs, ys = [p[0] for p in poly], [p[1] for p in poly]
    return min(ys), min(xs), max(ys) - min(ys), max(xs) - min(xs)


def line_image64(grey, poly, drop_out_p=True):
    """recognition.rs:91-118: the polygon's pixels gathered into a [bh, bw] image pre-filled with -0.5 -> (image float64,
    kept bool, in-page bool), or None for a box with an empty side.  A polygon pixel is taken when the page rect contains
    its page position (in_p, :100) AND its position in the line image (out_p, :112); drop_out_p=False leaves the second
    rule out (for the tests that show it matters)."""
    ph, pw = grey.shape
    top, left, bh, bw = poly_box(poly)
    if bh <= 0 or bw <= 0:
        return None
    inside = clib.polygon_fill_mask([(p[1], p[0]) for p in poly], top, left, bh, bw).astype(bool)
    r, c = np.arange(bh)[:, None], np.arange(bw)[None, :]
    y, x = top + r, left + c
    in_p = (y >= 0) & (y <= ph - 1) & (x >= 0) & (x <= pw - 1)
    out_p = (r <= ph - 1) & (c <= pw - 1)
    keep = inside & in_p & (out_p if drop_out_p else True)
    img = np.full((bh, bw), FILL, np.float64)
    yy, xx = np.broadcast_to(y, (bh, bw)), np.broadcast_to(x, (bh, bw))
    img[keep] = grey[yy[keep], xx[keep]]
    return img, keep, inside & in_p


def crop64(grey, poly, resized_w, out_h=REC_H, drop_out_p=True):
    """The plain line crop (recognition.rs:91-126) in float64 -> (crop [out_h, resized_w], tol)."""
    li = line_image64(grey, poly, drop_out_p)
    if li is None:
        return np.full((out_h, resized_w), FILL, np.float64), np.zeros((out_h, resized_w), np.float64)
    return bilinear64(li[0], out_h, resized_w)


# ------------------------------------------------------------------------------------------------ a. pages on the way in
IN_PAGES = [(37, 53), (160, 128), (100, 300), (300, 100), (517, 300), (1031, 2052), (1, 1), (1, 400), (400, 1), (161, 129)]
PLANT_PAGES = IN_PAGES[:4]          # identity with both pads, identity, and the two with one pad and the exact scales 300/128, 300/160
PLANT_VALUES = [("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("-0", -0.0)]


def pads(hw, model_hw=MODEL_HW):
    """(pad_bottom, pad_right) of detection.rs:155-156."""
    return max(model_hw[0] - hw[0], 0), max(model_hw[1] - hw[1], 0)


def plant_points(hw):
    """(0, 0), the last row and column, an interior pixel, the pixels beside the pad edges; with a pad on the right also
    the first pixel of a row, which is what the tap at column w of the row above reads if nothing keeps it
    out (the columns are at scale 1 whenever there is a pad on the right, so that tap's weight is 0 and only a value that
    is not finite shows it)."""
    h, w = hw
    pb, pr = pads(hw)
    pts = [(0, 0), (h - 1, w - 1), (h // 2, w // 3)]
    if pb:
        pts.append((h - 1, w // 2))
    if pr:
        pts += [(h // 3, w - 1), (h // 3 + 2, 0)]
    return sorted(set(pts))


def in_cases():
    """(id, grey page float32 [h, w] in [-0.5, 0.5), planted value or None)."""
    out = []
    for k, hw in enumerate(IN_PAGES):
        out.append(("%dx%d" % hw, (np.random.default_rng(100 + k).random(hw, dtype=np.float32) - np.float32(0.5)), None))
    for k, hw in enumerate(PLANT_PAGES):
        for name, v in PLANT_VALUES:
            page = np.random.default_rng(200 + k).random(hw, dtype=np.float32) - np.float32(0.5)
            for y, x in plant_points(hw):
                page[y, x] = v
            out.append(("%dx%d%s" % (hw + (name,)), page, v))
    return out


def is_identity_in(hw, model_hw=MODEL_HW):
    pb, pr = pads(hw, model_hw)
    return (hw[0] + pb, hw[1] + pr) == tuple(model_hw)


def model_input64(page, model_hw=MODEL_HW):
    """The detector's input (detection.rs:155-171) -> (float64, tol): the page padded with -0.5 to at least the model's
    size, and resized only if that is not the model's size: a same-size resize_image is a copy (detection.rs:167)."""
    pb, pr = pads(page.shape, model_hw)
    if is_identity_in(page.shape, model_hw):
        v = np.full(model_hw, FILL, np.float64)
        v[:page.shape[0], :page.shape[1]] = page
        return v, np.zeros(model_hw, np.float64)
    return bilinear64(page, model_hw[0], model_hw[1], page.shape[0] + pb, page.shape[1] + pr)


# ------------------------------------------------------------------------------------------------ b. maps on the way back
# widths at height 64: 64 / 128 / 256 threads per block on both sides of (w + 3) / 4 = 64 and 128, and every w % 4
BACK_PAGES = [(37, 53), (160, 128), (97, 211), (517, 300)] + [(64, w) for w in (256, 257, 258, 259, 260, 512, 516)] + [(1031, 2052)]


def back_slice(hw, model_hw=MODEL_HW):
    pb, pr = pads(hw, model_hw)
    return model_hw[0] - pb, model_hw[1] - pr


def is_identity_back(hw, model_hw=MODEL_HW):
    return back_slice(hw, model_hw) == tuple(hw)


def noise_map(hw, seed, model_hw=MODEL_HW):
    """Uniform [0, 1) noise over the model's output.  Inside the slice that belongs to the page, a grid of blobs keeps the
    noise as it is (four in five of their pixels pass the threshold, the rest are holes and ragged edges); around them it is
    scaled into [0, 0.21), so that one pixel in twenty still passes, as speckle too small to become a word."""
    m = np.random.default_rng(seed).random(model_hw, dtype=np.float32)
    sh, sw = back_slice(hw, model_hw)
    ny, nx = min(4, max(1, sh // 16)), min(4, max(1, sw // 20))
    blob = np.zeros(model_hw, bool)
    for j in range(ny):
        for i in range(nx):
            y0, y1 = sh * j / ny, sh * (j + 1) / ny
            x0, x1 = sw * i / nx, sw * (i + 1) / nx
            blob[int(y0 + 0.2 * (y1 - y0)):int(y1 - 0.2 * (y1 - y0)), int(x0 + 0.2 * (x1 - x0)):int(x1 - 0.2 * (x1 - x0))] = True
    return np.where(blob, m, m * np.float32(0.21)).astype(np.float32)


PLANTED_BLOCK = (60, 40, 14, 40)    # y, x, h, w of the block around the threshold
PLANTED_PIXELS = 14 * 20


def threshold_map(model_hw=MODEL_HW):
    """Zeros around a 14 x 40 block whose left half is exactly the threshold and whose right half is the next float32 above
    it: with a strict '>' the word is the right half alone, 280 pixels."""
    m = np.zeros(model_hw, np.float32)
    y, x, h, w = PLANTED_BLOCK
    m[y:y + h, x:x + w // 2] = THR
    m[y:y + h, x + w // 2:x + w] = np.nextafter(THR, np.float32(1))
    return m


def nonfinite_map(seed, model_hw=MODEL_HW):
    """Zeros around two noise blobs in [0.3, 1) with NaN, +Inf and -Inf inside the first and just outside the second."""
    m = np.zeros(model_hw, np.float32)
    rng = np.random.default_rng(seed)
    for y, x in ((8, 10), (36, 60)):
        m[y:y + 18, x:x + 40] = np.float32(0.3) + np.float32(0.7) * rng.random((18, 40), dtype=np.float32)
    m[12, 20], m[16, 30], m[20, 40] = np.nan, np.inf, -np.inf          # inside
    m[35, 70], m[44, 59], m[54, 80], m[40, 100] = np.nan, np.inf, -np.inf, np.inf   # above, left of, below, right of the second
    return m


def back_cases():
    """(id, page (h, w), model output float32 [160, 128], kind): kind "noise" | "threshold" | "nonfinite"."""
    out = [("%dx%d" % hw, hw, noise_map(hw, 300 + k), "noise") for k, hw in enumerate(BACK_PAGES)]
    out.append(("threshold-160x128", (160, 128), threshold_map(), "threshold"))
    out.append(("nonfinite-160x128", (160, 128), nonfinite_map(7), "nonfinite"))      # identity
    out.append(("nonfinite-64x256", (64, 256), nonfinite_map(8), "nonfinite"))        # rows at scale 1, columns at the exact scale 1/2
    return out


def back_map64(hw, out_map, model_hw=MODEL_HW):
    """The page's probability map (detection.rs:187-194) -> (float64, tol): the model's output without the padded region,
    resized to the page unless it has the page's size already (a copy, as on the way in)."""
    sh, sw = back_slice(hw, model_hw)
    if is_identity_back(hw, model_hw):
        return out_map[:sh, :sw].astype(np.float64), np.zeros(hw, np.float64)
    return bilinear64(out_map[:sh, :sw], hw[0], hw[1])


def mask_mismatch(got_map, ref, tol):
    """A map's strict threshold against the restatement's -> (pixels that differ outside the band |ref - thr| <= tol,
    share of the page inside the band).  NaN passes on neither side."""
    thr = float(THR)
    with np.errstate(invalid="ignore"):
        band = np.abs(ref - thr) <= tol
        diff = ((got_map > THR) != (ref > thr)) & ~band
    return int(diff.sum()), float(band.mean())


MAX_BAND = 1e-3     # at most 0.1 % of a page may sit inside the band


# ------------------------------------------------------------------------------------------------ c. lines
# key -> (seed, h, w).  wide: the hand-made lines run to x = 5447, on a narrower page less than 2 % of the longest crop is page
CROP_PAGES = {"big": (5, 1000, 1101), "w801": (801, 700, 801), "w802": (802, 700, 802), "w803": (803, 700, 803), "w804": (804, 700, 804),
              "small": (6, 40, 70), "mid": (7, 300, 517), "nf": (8, 120, 300), "wide": (9, 1000, 1600)}
ANGLES = (0, 1, -1, 3, -3, 10, -10, 30, -30, 45, -45, 60, 80, 90, -90)
OUT_P = np.array([[10.0, 5.0, 0.0, -1.0, 120.0, 70.0]], np.float32)          # polygon (-50, -30) .. (70, 40) on the 40 x 70 page
OUT_P_LEFT = np.array([[10.0, 20.0, 0.0, -1.0, 120.0, 30.0]], np.float32)    # over the left edge only


def crop_page(key):
    """The grey page [h, w] float32 in [-0.5, 0.5]: test_gpu_rectify.noise_page, every pixel unlike its neighbours, moved
    to the range of a prepared page."""
    from test_gpu_rectify import noise_page
    seed, h, w = CROP_PAGES[key]
    page = noise_page(seed, h, w)[0] - np.float32(0.5)
    if key == "nf":
        page[40:44, 50:200] = np.nan
        page[60, 90] = np.inf
        page[52, 140] = -np.inf
    return page


def _angled(rng, deg):
    from test_rectify_cpu import slanted_line
    return slanted_line(350.0, 500.0, deg, rng.uniform(30, 90, 7), height=26.0, jitter=rng.uniform(-2, 2, 7))


def crop_cases():
    """(id, page key, line float32 [n, 6], group): group "angle" | "edge" | "outside" | "hand" | "zero" | "out_p" |
    "small" | "tall" | "nf"."""
    from test_gpu_rectify import edge_lines
    from test_rectify_cpu import hand_made_lines, slanted_line
    out = []
    rng = np.random.default_rng(11)
    for deg in ANGLES:
        out.append(("angle%+d" % deg, "big", _angled(rng, deg), "angle"))
    for w in (801, 802, 803, 804):
        for deg in (0, 10, -30):
            out.append(("w%d-angle%+d" % (w, deg), "w%d" % w, _angled(rng, deg), "angle"))
    _, h, w = CROP_PAGES["big"]
    for name, line in edge_lines(h, w):
        out.append((name, "big", line, "outside" if name.startswith("outside") else "edge"))
    for name, line in hand_made_lines():
        if name == "huge" or name == "zero_size" or name.startswith("non_finite"):
            continue
        out.append((name, "wide", line, "zero" if name.startswith("zero") else "hand"))
    out.append(("out_p", "small", OUT_P, "out_p"))
    out.append(("out_p_left", "small", OUT_P_LEFT, "out_p"))
    out.append(("box80x1", "big", np.array([[400.0, 300.5, 0.0, -1.0, 80.0, 1.0]], np.float32), "small"))
    out.append(("box1x30", "big", np.array([[400.5, 300.0, 0.0, -1.0, 1.0, 30.0]], np.float32), "small"))
    out.append(("tall40x200", "big", np.array([[500.0, 400.0, 0.0, -1.0, 40.0, 200.0]], np.float32), "tall"))
    out.append(("nonfinite_page", "nf", slanted_line(20.0, 50.0, 3.0, [60.0, 50.0, 70.0], height=30.0), "nf"))
    return out


def batch_lines():
    """[(page key, [line, ...])]: three pages of different sizes with 4 to 8 of the lines above each, for one
    recognize_text_batch call."""
    from test_gpu_rectify import edge_lines
    from test_rectify_cpu import hand_made_lines, slanted_line
    hand = dict(hand_made_lines())
    rng = np.random.default_rng(12)
    small = [OUT_P, OUT_P_LEFT, np.array([[30.0, 20.0, 0.0, -1.0, 40.0, 16.0]], np.float32), slanted_line(5.0, 10.0, 10.0, [20.0, 25.0], height=12.0)]
    _, mh, mw = CROP_PAGES["mid"]
    mid_edges = dict(edge_lines(mh, mw))
    mid = [slanted_line(50.0, 150.0, deg, rng.uniform(30, 90, 4), height=26.0, jitter=rng.uniform(-2, 2, 4)) for deg in (0, 10, -30)]
    mid += [mid_edges["over_right"], mid_edges["over_corner"], mid_edges["outside_left"]]
    big = [_angled(rng, deg) for deg in (3, -10, 45, 90)] + [hand["forty_words"], hand["clamp_10"], hand["one_word"], hand["two_words_equal_cx"]]
    return [("small", small), ("mid", mid), ("big", big)]


def group_width(resized_w):
    return -(-resized_w // 50) * 50     # next_multiple_of(50), recognition.rs:437

