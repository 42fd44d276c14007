"""Rectified line crops, host side: the library's frame, width, map coefficients, word ranges and char
boxes equal tests/rectify_ref.py bit for bit, and the restatement's crop is held to a closed form.  No GPU."""
import glob
import math
import os

import numpy as np
import pytest

import rectify_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROTATED = sorted(glob.glob(os.path.join(HERE, "golden", "rotated", "*.npz")))
H = 64


def slanted_line(x0, y0, deg, widths, height=24.0, gap=8.0, jitter=None):
    """Word rects of one line that starts at (x0, y0) and runs at `deg` degrees: float32 [n, 6]."""
    th = math.radians(deg)
    dx, dy = math.cos(th), math.sin(th)
    out, s = [], 0.0
    for k, w in enumerate(widths):
        c = s + w / 2.0
        off = 0.0 if jitter is None else jitter[k]
        out.append([x0 + c * dx - off * dy, y0 + c * dy + off * dx, dy, -dx, w, height])
        s += w + gap
    return np.array(out, np.float32)


def assert_frame_equal(words, h=H):
    import ocrs_amd
    lib, ref = ocrs_amd.line_frame(words, h), R.line_frame(words, h)
    assert lib.empty == ref.empty
    assert lib.rw == ref.rw
    assert lib.axis.tobytes() == np.array(ref.a, np.float64).tobytes(), (lib.axis, ref.a)
    assert lib.extents.tobytes() == np.array(ref.extents, np.float64).tobytes(), (lib.extents, ref.extents)
    assert lib.coef.tobytes() == ref.coef.tobytes(), (lib.coef, ref.coef)
    assert np.array_equal(lib.ranges, ref.ranges), (lib.ranges, ref.ranges)
    return lib, ref


def assert_char_boxes_equal(words, ref, seed, h=H):
    import ocrs_amd
    gw = R.group_width(ref.rw)
    if gw == 0:
        return
    rng = np.random.default_rng(seed)
    for ctc_len in (gw // 4, max(gw // 4 - 1, 1)):   # downsample 4, and a quotient that has to be rounded
        n = int(rng.integers(1, min(ctc_len, 60) + 1))
        pos = np.sort(rng.choice(ctc_len, size=n, replace=False)).astype(np.uint32)
        rects, kept = ocrs_amd.line_char_boxes(words, ctc_len, pos, h)
        exp = R.char_boxes(ref, gw, ctc_len, [(1, int(p)) for p in pos])
        assert sorted(i for i, _ in exp) == list(np.nonzero(kept)[0])
        for i, box in exp:
            assert tuple(int(v) for v in rects[i]) == box, (i, rects[i], box)
        if ref.empty:
            assert not kept.any()


def test_line_frame_is_exported():
    from ocrs_amd import _lib
    for name in ("ocrs_line_frame", "ocrs_line_char_boxes", "ocrs_engine_prepare_recognition_input_rectified",
                 "ocrs_engine_recognize_text_rectified", "ocrs_engine_recognize_text_batch_rectified",
                 "ocrs_group_recognize_text_batch_rectified"):
        assert hasattr(_lib.lib(), name), name


@pytest.mark.parametrize("path", ROTATED, ids=[os.path.basename(p)[:-4] for p in ROTATED])
def test_fixture_lines_bit_for_bit(path):
    assert len(ROTATED) == 15
    z = np.load(path)
    lr, lo = z["line_rects"], z["line_offsets"]
    for i in range(len(lo) - 1):
        words = lr[lo[i]:lo[i + 1]]
        _, ref = assert_frame_equal(words)
        assert_char_boxes_equal(words, ref, seed=i)


def hand_made_lines():
    rng = np.random.default_rng(7)
    yield "one_word", np.array([[300.5, 200.25, 0.17364818, -0.98480775, 120.0, 30.0]], np.float32)
    yield "one_word_up_left", np.array([[300.5, 200.25, -0.5, 0.8660254, 120.0, 30.0]], np.float32)      # a.x < 0: negated
    yield "one_word_vertical", np.array([[300.5, 200.25, 1.0, 0.0, 120.0, 30.0]], np.float32)            # a.x == 0, a.y > 0
    yield "one_word_vertical_down", np.array([[300.5, 200.25, -1.0, 0.0, 120.0, 30.0]], np.float32)      # a.x == 0, a.y < 0: negated
    yield "two_words_equal_cx", np.array([[100.0, 50.0, 0.0, -1.0, 80.0, 20.0], [100.0, 90.0, 0.0, -1.0, 60.0, 22.0]], np.float32)
    yield "forty_words", slanted_line(40.3, 900.7, -7.0, rng.uniform(10, 60, 40), jitter=rng.uniform(-3, 3, 40))
    yield "forty_words_steep", slanted_line(40.3, 100.7, 30.0, rng.uniform(10, 60, 40), jitter=rng.uniform(-3, 3, 40))
    yield "clamp_2400", slanted_line(10.0, 500.0, 2.0, [900.0] * 6, height=20.0)
    yield "clamp_10", np.array([[50.0, 80.0, 0.0, -1.0, 4.0, 90.0]], np.float32)
    yield "gaps_wider_than_words", slanted_line(10.0, 300.0, 5.0, [12.0, 9.0, 15.0], gap=140.0)
    yield "zero_size", np.array([[50.0, 80.0, 0.0, -1.0, 0.0, 0.0]], np.float32)
    yield "zero_height", np.array([[50.0, 80.0, 0.0, -1.0, 40.0, 0.0]], np.float32)
    yield "zero_width", np.array([[50.0, 80.0, 0.0, -1.0, 0.0, 30.0]], np.float32)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        w = slanted_line(10.0, 300.0, 5.0, [40.0, 30.0, 50.0])
        w[1, k * 2] = bad
        yield "non_finite_%d" % k, w
    yield "huge", np.array([[1e30, -1e30, 0.0, -1.0, 3e38, 2e38], [3e38, 1e30, 0.6, -0.8, 1e38, 1e37]], np.float32)


@pytest.mark.parametrize("name,words", list(hand_made_lines()), ids=[n for n, _ in hand_made_lines()])
def test_hand_made_lines_bit_for_bit(name, words):
    for h in (64, 50):
        lib, ref = assert_frame_equal(words, h)
        assert_char_boxes_equal(words, ref, seed=len(name), h=h)
    ref = R.line_frame(words, 64)
    if name == "clamp_2400":
        assert ref.rw == 2400 and not ref.empty
    if name == "clamp_10":
        assert ref.rw == 10 and not ref.empty
    if name.startswith("non_finite") or name.startswith("zero"):
        assert ref.empty


def test_degenerate_width_is_the_plain_lines():
    """The empty line's width is what the plain crop gives a bounding box with a side of zero (recognition.rs:58-75 on
    0 x 0, 0 x h, w x 0), in the library and in the restatement."""
    import ocrs_amd
    cases = {"zero_size": 0, "zero_width": 10, "zero_height": 2400, "non_finite_0": 0}
    made = dict(hand_made_lines())
    for name, rw in cases.items():
        lib = ocrs_amd.line_frame(made[name], 64)
        assert lib.empty and lib.rw == rw == R.line_frame(made[name], 64).rw, name
        assert np.array_equal(R.crop(np.zeros((40, 40), np.float32), made[name], 64), np.full((64, rw), -0.5, np.float32))
    assert R.resized_line_width(0, 0, 64) == 0 and R.resized_line_width(0, 7, 64) == 10 and R.resized_line_width(7, 0, 64) == 2400


def test_upright_row_is_its_bounding_box():
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(2, 12))
        cy = np.float32(rng.uniform(20, 900))
        hgt = np.float32(rng.uniform(8, 40))
        cx = np.cumsum(rng.uniform(30, 90, n)).astype(np.float32)
        w = rng.uniform(5, 28, n).astype(np.float32)
        words = np.stack([cx, np.full(n, cy), np.zeros(n, np.float32), np.full(n, -1, np.float32), w, np.full(n, hgt)], 1).astype(np.float32)
        fr = R.line_frame(words, H)
        assert fr.a == (1.0, 0.0)
        left = min(float(c) - float(ww) / 2.0 for c, ww in zip(cx, w))
        right = max(float(c) + float(ww) / 2.0 for c, ww in zip(cx, w))
        assert fr.extents == (left, right, float(cy) - float(hgt) / 2.0, float(cy) + float(hgt) / 2.0)
        assert_frame_equal(words)


def test_quoted_fixture_line_width():
    z = np.load(os.path.join(HERE, "golden", "rotated", "polar-bears_+10.npz"))
    lr, lo = z["line_rects"], z["line_offsets"]
    words = lr[lo[1]:lo[2]]
    assert len(words) == 18 and tuple(z["crop_shapes"][1]) == (64, 426)
    lib, ref = assert_frame_equal(words)
    assert lib.rw == 1458
    s_min, s_max, t_min, t_max = ref.extents
    assert round(s_max - s_min) == 1321 and round(t_max - t_min) == 57   # the line in its own frame; rw comes from the ceils


@pytest.mark.parametrize("deg", [0, 3, -3, 10, -10, 30, -30])
def test_restatement_against_closed_form(deg):
    """On a page that is affine in (x, y) bilinear sampling is exact up to rounding, so the restatement's crop must equal
    the page function at the frame's sample positions, evaluated in float64 from the float64 frame.

    The bound, derived: the map rounds three coefficients and does two products and two sums per coordinate — seven
    roundings, each at most half an ulp of a value no larger than the page's largest coordinate M, i.e. 2^-24 M — so a
    position is off by at most 7 * 2^-24 * M per axis, which moves the value by at most (|gx| + |gy|) times that.  X -
    floor(X) is exact.  The interpolation rounds 1 - w, two products and a sum per row pair (4 roundings on values up to
    V = max |page|), twice nested: at most 8 * 2^-24 * V; the page values themselves are exact in float32 by
    construction (multiples of 2^-13 below 1)."""
    ph, pw = 1200, 1600
    gx, gy, p0 = 3.0 / 8192, -5.0 / 8192, -0.25
    yy, xx = np.mgrid[0:ph, 0:pw]
    page64 = p0 + gx * xx + gy * yy
    page = page64.astype(np.float32)
    assert np.array_equal(page.astype(np.float64), page64)
    rng = np.random.default_rng(deg + 100)
    words = slanted_line(200.0, 600.0, deg, rng.uniform(40, 160, 9), height=30.0, jitter=rng.uniform(-2, 2, 9))
    fr = R.line_frame(words, H)
    assert not fr.empty
    s_min, s_max, t_min, t_max = fr.extents
    ax, ay = fr.a
    s = s_min + (np.arange(fr.rw) + 0.5)[None, :] * (s_max - s_min) / fr.rw
    t = t_min + (np.arange(H) + 0.5)[:, None] * (t_max - t_min) / H
    X = s * ax + t * -ay - 0.5
    Y = s * ay + t * ax - 0.5
    assert X.min() >= 0 and X.max() <= pw - 1 and Y.min() >= 0 and Y.max() <= ph - 1, "the line stays on the page"
    exact = p0 + gx * X + gy * Y
    got = R.sample(page, fr.coef, fr.rw, H).astype(np.float64)
    u = 2.0 ** -24
    M, V = float(max(ph, pw)), float(np.abs(page64).max())
    bound = (abs(gx) + abs(gy)) * 7 * u * M + 8 * u * V
    err = float(np.abs(got - exact).max())
    print("angle %+d: rw %d, max |crop - closed form| %.3e, derived bound %.3e" % (deg, fr.rw, err, bound))
    assert err <= bound
    # and the masked crop is that sample wherever the mask keeps it
    lo, hi = R.column_table(fr, H)
    keep = (np.arange(H)[:, None] >= lo[None, :]) & (np.arange(H)[:, None] <= hi[None, :])
    full = R.crop(page, words, H, out_w=R.group_width(fr.rw))
    assert np.array_equal(full[:, :fr.rw][keep], got.astype(np.float32)[keep])
    assert np.all(full[:, :fr.rw][~keep] == -0.5) and np.all(full[:, fr.rw:] == -0.5)
    assert keep.mean() > 0.5


def test_column_table_rules():
    """Covered columns take min / max over their words; an uncovered one looks at the nearest covered column on each side."""
    fr = R.Frame(3)
    fr.empty, fr.rw = False, 20
    fr.ranges[:] = [(2, 5, 10, 20), (4, 8, 5, 15), (14, 16, 30, 40)]
    lo, hi = R.column_table(fr, 64)
    assert (lo[0], hi[0]) == (10, 20)              # left of everything: the nearest on the right only
    assert (lo[4], hi[4]) == (5, 20)               # two words
    assert (lo[10], hi[10]) == (5, 40)             # a gap: column 8 and column 14
    assert (lo[19], hi[19]) == (30, 40)            # right of everything
    fr.ranges[:] = [(1, 0, 1, 0)] * 3
    lo, hi = R.column_table(fr, 64)
    assert lo.tolist() == [0] * 20 and hi.tolist() == [63] * 20
