"""Working-resolution detection, host side: the library's work-size rule and rect map equal
tests/resample_ref.py, and the restatement's area filter has the properties its definition promises.  No GPU."""
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

import resample_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")
FIXTURES = sorted(glob.glob(os.path.join(G, "rotated", "*.npz"))) + [os.path.join(G, "bench_page_seed0.npz")]
IDS = [os.path.relpath(p, G)[:-4] for p in FIXTURES]
NEW_SYMBOLS = ["ocrs_engine_resize_page", "ocrs_engine_resize_pages", "ocrs_work_size", "ocrs_rescale_rects",
               "ocrs_engine_detect_words_at", "ocrs_engine_detect_words_batch_at"]
# (from, to) frames, (height, width): equal, 2 x up and down, the bench page at its squeezed work size, A4 at 300 dpi halved
# with the width rounded either way (sx != sy)
SIZE_PAIRS = [((1024, 1024), (1024, 1024)), ((1024, 1024), (2048, 2048)), ((2048, 2048), (1024, 1024)),
              ((1024, 1024), (600, 576)), ((600, 576), (1024, 1024)), ((3508, 2480), (1754, 1240)), ((1754, 1240), (3508, 2480)),
              ((3508, 2480), (1754, 1241)), ((1754, 1241), (3508, 2480))]


@pytest.fixture(scope="module")
def lib():
    from ocrs_amd import _lib, build
    build.build()
    return _lib.lib()


def test_new_symbols_are_exported_and_declared(lib):
    from ocrs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ocrs_amd.h")).read()
    declared = set(re.findall(r"OCRS_API[^;(]*?\b(ocrs_\w+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert [_lib.RESAMPLE_FILTERS[k] for k in ("auto", "bilinear", "area")] == \
        [int(re.search(r"OCRS_RESAMPLE_%s = (\d)" % k.upper(), hdr).group(1)) for k in ("auto", "bilinear", "area")]


# ---------------------------------------------------------------- work size
def test_work_size_equals_the_restatement(lib):
    import ocrs_amd
    pages = [(1, 1), (7, 7), (600, 800), (1024, 1024), (3508, 2480), (7016, 4960), (65535, 3), (3, 65535), (100000, 50)]
    scales = [1.0, 0.5, 2.0, 1.0 / 3.0, 0.25, 96.0 / 300.0, 1.5, 0.001, 1e-9, 1e9, 1e300, 0.4999999, 0.70710678, math.pi]
    for hw in pages:
        for s in scales:
            assert ocrs_amd.work_size(hw, scale=s) == R.work_size(hw, s), (hw, s)
        for n in (1, 512, 1024, 1400, 2048, 4096, 70000):
            got = ocrs_amd.work_size(hw, max_side=n)
            assert got == R.work_size(hw, R.max_side_scale(hw, n)), (hw, n)
            assert max(got) <= max(n, 1) or max(hw) <= n
            if max(hw) <= n:
                assert got == tuple(min(v, 65535) for v in hw), "a page within the side keeps its size"
    assert ocrs_amd.work_size((3508, 2480), scale=0.5) == (1754, 1240)
    assert ocrs_amd.work_size((3, 5), scale=0.5) == (2, 3), "floor(x + 0.5): halves round up"
    assert ocrs_amd.work_size((3508, 2480), max_side=1400) == (1400, 990)
    assert ocrs_amd.work_size((10, 10), scale=1e-9) == (1, 1) and ocrs_amd.work_size((10, 10), scale=1e9) == (65535, 65535)


def test_work_size_refuses_what_is_no_scale(lib):
    import ocrs_amd
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        with pytest.raises(ocrs_amd.OcrsError) as e:
            ocrs_amd.work_size((100, 100), scale=bad)
        assert e.value.status_name == "INVALID_ARGUMENT"
    for hw in ((0, 5), (5, -1)):
        with pytest.raises(ocrs_amd.OcrsError):
            ocrs_amd.work_size(hw, scale=1.0)
    with pytest.raises(ValueError):
        ocrs_amd.work_size((100, 100))
    with pytest.raises(ValueError):
        ocrs_amd.work_size((100, 100), scale=1.0, max_side=5)
    h, w = C.c_int(0), C.c_int(0)
    assert lib.ocrs_work_size(C.c_int(5), C.c_int(5), C.c_double(1.0), None, C.byref(w)) == 1


# ---------------------------------------------------------------- the rect map
def hand_made_rects():
    return np.array([
        [10.0, 20.0, 0.0, -1.0, 30.0, 8.0],
        [0.0, 0.0, -0.0, 1.0, 0.0, 0.0],                      # zero sizes, a negative zero
        [-0.5, -0.5, 0.0, -1.0, 0.0, 12.0],                   # the page's corner
        [5.0, 6.0, 0.0, 0.0, 7.0, 9.0],                       # zero up
        [5.0, 6.0, -0.0, 0.0, 7.0, 9.0],
        [100.0, 50.0, 0.6, -0.8, 40.0, 10.0],                 # tilted
        [100.0, 50.0, 1e-30, -1e-30, 40.0, 10.0],             # a tiny up: its length is far from 1
        [3e38, -3e38, 1e30, -1e30, 3e38, 2e38],               # huge: doubles hold what float32 does not
        [1e30, 3e38, 3e38, -3e38, 1e-30, 3e38],
        [np.nan, 1.0, 0.0, -1.0, 4.0, 4.0],
        [1.0, np.nan, np.nan, -1.0, 4.0, 4.0],
        [1.0, 2.0, 0.0, -1.0, np.nan, np.inf],
        [np.inf, -np.inf, np.inf, -np.inf, np.inf, np.nan],
        [2.0, 3.0, np.inf, 0.0, 5.0, 6.0],
    ], np.float32)


def assert_same_bits(got, exp, what):
    """uint32 equal wherever the expectation is a number, NaN exactly where it is NaN."""
    assert got.dtype == np.float32 and got.shape == exp.shape, what
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions")
    bad = np.argwhere((got.view(np.uint32) != exp.view(np.uint32)) & ~nan)
    assert len(bad) == 0, "%s: %d values differ, first at %s: got %r, expected %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_rescale_rects_on_fixture_words_bit_for_bit(lib, path):
    import ocrs_amd
    assert len(FIXTURES) == 16
    rects = np.load(path)["word_rects"]
    assert len(rects) > 20
    for a, b in SIZE_PAIRS:
        assert_same_bits(ocrs_amd.rescale_rects(rects, a, b), R.rescale_rects(rects, a, b), (os.path.basename(path), a, b))


def test_rescale_rects_on_hand_made_rects_bit_for_bit(lib):
    import ocrs_amd
    rects = hand_made_rects()
    for a, b in SIZE_PAIRS + [((1, 1), (65535, 65535)), ((65535, 1), (1, 65535))]:
        assert_same_bits(ocrs_amd.rescale_rects(rects, a, b), R.rescale_rects(rects, a, b), ("hand made", a, b))
    assert ocrs_amd.rescale_rects(np.zeros((0, 6), np.float32), (5, 5), (10, 10)).shape == (0, 6)
    # by hand: a 2 x 2 block of pixels becomes one; centres move as points of the pixel-index frame
    one = ocrs_amd.rescale_rects([[10.0, 20.0, 0.0, -1.0, 30.0, 8.0]], (200, 100), (100, 50))[0]
    assert one.tolist() == [4.75, 9.75, 0.0, -1.0, 15.0, 4.0]
    # sx != sy: an upright rect's width scales with x and its height with y; one lying on its side swaps them
    up, side = ocrs_amd.rescale_rects([[9.5, 9.5, 0.0, -1.0, 30.0, 8.0], [9.5, 9.5, 1.0, 0.0, 30.0, 8.0]], (100, 100), (200, 400))
    assert up.tolist() == [39.5, 19.5, 0.0, -1.0, 120.0, 16.0] and side.tolist() == [39.5, 19.5, 1.0, 0.0, 60.0, 32.0]
    # a zero up cannot be renormalised: it stays, and the sizes scale by axis
    zero = ocrs_amd.rescale_rects([[5.0, 6.0, 0.0, 0.0, 7.0, 9.0]], (100, 100), (200, 400))[0]
    assert zero.tolist() == [21.5, 12.5, 0.0, 0.0, 28.0, 18.0]
    for bad in ((0, 5), (5, 0), (-1, 5)):
        with pytest.raises(ocrs_amd.OcrsError) as e:
            ocrs_amd.rescale_rects(rects, bad, (5, 5))
        assert e.value.status_name == "INVALID_ARGUMENT"
        with pytest.raises(ocrs_amd.OcrsError):
            ocrs_amd.rescale_rects(rects, (5, 5), bad)


def test_equal_sizes_leave_every_bit_untouched(lib):
    import ocrs_amd
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 1 << 32, size=(64, 6), dtype=np.uint64).astype(np.uint32)
    bits[0] = [0x7FC12345, 0xFFA00001, 0x7F800001, 0x80000000, 0x00000001, 0xFF800000]   # NaN payloads, -0.0, a denormal
    rects = bits.view(np.float32)
    for hw in ((1, 1), (1024, 1024), (3508, 2480)):
        assert ocrs_amd.rescale_rects(rects, hw, hw).view(np.uint32).tobytes() == bits.tobytes()
        assert R.rescale_rects(rects, hw, hw).view(np.uint32).tobytes() == bits.tobytes()


def test_down_then_up_at_an_integer_ratio_is_the_identity_within_an_ulp(lib):
    """Axis-aligned rects: (c + 0.5) / k - 0.5 and back is c up to the two float32 roundings; sizes scale by a power of
    two or by k and 1 / k.  One ulp of the coordinate (of the value itself for the sizes)."""
    import ocrs_amd
    rects = np.load(os.path.join(G, "bench_page_seed0.npz"))["word_rects"].copy()
    rects[:, 2:4] = [0.0, -1.0]
    extra = rects.copy()
    extra[:, 2:4] = [1.0, 0.0]
    rects = np.concatenate([rects, extra])
    for k in (2, 3, 4, 7):
        big = (1024 * k, 1024 * k)
        for a, b in (((1024, 1024), big), (big, (1024, 1024))):
            there = ocrs_amd.rescale_rects(rects, a, b)
            back = ocrs_amd.rescale_rects(there, b, a)
            assert back[:, 2:4].tobytes() == rects[:, 2:4].tobytes()
            for col in (0, 1, 4, 5):
                ulp = np.spacing(np.abs(rects[:, col]))
                assert np.all(np.abs(back[:, col].astype(np.float64) - rects[:, col]) <= ulp), (k, col)


# ---------------------------------------------------------------- the restatement's area filter
def planted_page(seed, h, w):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


@pytest.fixture(scope="module")
def bench_page():
    from ocrs_amd import synth
    from oracle import pipeline as OP
    px = synth.synthetic_page(0, 1024, 1024, lines=80)
    return np.ascontiguousarray(np.asarray(OP.prepare_image(OP.ImageSource.from_tensor(px, "hwc")), np.float32)[0])


def test_area_axis_taps():
    for L, l in ((7, 7), (8, 4), (9, 3), (5, 1), (300, 7), (65, 64), (129, 128), (1024, 576), (3000, 375), (65535, 65534)):
        P, first, ov = R.axis_taps(L, l)   # asserts weights >= 1 on the taps, their sum P, the last tap L - 1
        g = math.gcd(L, l)
        assert P == L // g and first[0] == 0 and ov.shape[0] == l
    assert R.axis_taps(9, 3)[2].tolist() == [[1, 1, 1]] * 3
    assert R.axis_taps(3, 2)[2].tolist() == [[2, 1], [1, 2]]   # P = 3, q = 2: [0, 3) over [0, 2), [2, 4) and [3, 6) over [2, 4), [4, 6)
    assert R.axis_taps(65535, 65534)[2].shape[1] == 2


def test_area_is_the_identity_at_equal_sizes():
    bits = np.random.default_rng(5).integers(0, 1 << 32, size=(37, 41), dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] = 0x80000000      # no NaN / inf by chance; -0.0 instead
    page = bits.view(np.float32)
    assert R.area(page, 37, 41).view(np.uint32).tobytes() == bits.tobytes()
    assert np.array_equal(np.isnan(R.area(np.full((3, 3), np.nan, np.float32), 3, 3)), np.ones((3, 3), bool))


def test_area_two_by_two_closed_form():
    page = planted_page(1, 64, 96)
    a, b, c, d = page[0::2, 0::2], page[0::2, 1::2], page[1::2, 0::2], page[1::2, 1::2]
    two = np.float32(2.0)
    exp = (((a + b) / two) + ((c + d) / two)) / two
    assert R.area(page, 32, 48).tobytes() == exp.astype(np.float32).tobytes()


def test_area_undoes_a_pixel_doubling(bench_page):
    doubled = np.kron(bench_page, np.ones((2, 2), np.float32))
    assert doubled.shape == (2048, 2048)
    assert R.area(doubled, 1024, 1024).tobytes() == bench_page.tobytes()


def test_area_keeps_constant_pages():
    for c in (np.float32(-0.5), np.float32(0.5)):
        for L in range(1, 140):
            col = np.full((L, 1), c, np.float32)
            for l in range(1, L + 1):
                out = R.area(col, l, 1)
                assert out.shape == (l, 1) and np.all(out == c), (float(c), L, l)
    assert np.all(R.area(np.full((139, 137), np.float32(-0.5)), 100, 37) == np.float32(-0.5))


@pytest.mark.parametrize("src,dst", [((300, 211), (97, 64)), ((257, 259), (100, 37)), ((64, 65), (63, 64)), ((127, 129), (126, 128)),
                                      ((1024, 1024), (600, 576)), ((5, 5), (1, 1)), ((300, 1), (7, 1))],
                         ids=lambda s: "%dx%d" % s)
def test_area_is_within_its_rounding_bound_of_float64(src, dst):
    """K products, K - 1 sums and one division per axis, each within 2^-24 relative: to first order the result is within
    (Kx + Ky + 2) * 2^-24 * max|in| of the exact weighted average."""
    page = planted_page(src[0] * 1000 + src[1], *src)
    exact, (kx, ky) = R.area_f64(page, *dst)
    err = np.abs(R.area(page, *dst).astype(np.float64) - exact).max()
    bound = (kx + ky + 2) * 2.0 ** -24 * float(np.abs(page).max())
    print("%s -> %s: taps %d x %d, max error %.3g = %.2f of the bound" % (src, dst, kx, ky, err, err / bound))
    assert err <= bound


def test_composition_maps_the_work_pages_words_back():
    page = planted_page(2, 40, 60)
    seen = []

    def detect(work):
        seen.append(work)
        return np.array([[9.5, 4.5, 0.0, -1.0, 10.0, 4.0]], np.float32), np.array([0.5], np.float32)

    rects, score = R.detect_at(detect, page, (20, 30))
    assert seen[0].tobytes() == R.area(page, 20, 30).tobytes() and score.tolist() == [0.5]
    assert rects.tolist() == [[19.5, 9.5, 0.0, -1.0, 20.0, 8.0]]
    for own in (None, (0, 0), (40, 60)):
        rects, _ = R.detect_at(detect, page, own)
        assert seen[-1] is not None and seen[-1].tobytes() == page.tobytes() and rects.tolist() == [[9.5, 4.5, 0.0, -1.0, 10.0, 4.0]]
    R.detect_at(detect, page, (80, 120))
    from oracle import clib
    assert seen[-1].tobytes() == clib.resize_bilinear(page, 80, 120).tobytes()
