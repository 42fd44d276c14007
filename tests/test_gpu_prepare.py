"""Page preparation on the GPU (kernels_image.hip prepare_image / prepare_image_batch: the scalar kernels, the 4-pixel
u8 RGB kernels, their batch forms and the table split) against the oracle bit for bit and against the float64
restatement of tests/prepare_ref.py within its derived bound, at every format, on both sides of every grid cap, on every
RGB triple, from aligned and misaligned sources, from host, pinned and device memory, and from JPEG streams.

tests/test_prepare_cpu.py walks the same case lists on the oracle and asserts that they reach every branch of the dispatch.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import io

import numpy as np
import pytest

import prepare_ref as R
from ocrs_amd import DimOrder, EngineGroup, ImageSource, OcrEngine, _lib, synth
from oracle import pipeline as OP

pytestmark = pytest.mark.gpu

ORDER = {"hwc": DimOrder.Hwc, "chw": DimOrder.Chw}
STAGE = "prepare_image"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    e = OcrEngine()
    e.enable_timing(1)
    return e


@pytest.fixture(scope="module")
def group():
    g = EngineGroup([0])
    g.member(0)[0].enable_timing(1)
    return g


def oracle(px, order):
    return np.asarray(OP.prepare_image(OP.ImageSource.from_tensor(px, order)))


def prepared(eng, px, order):
    return eng.prepare_input(ImageSource.from_tensor(px, ORDER[order])).image()


def launches(engine, fn):
    """fn() -> (its result, the launches the stage timers counted for the conversion, or None if they do not report it)."""
    engine.stage_times(reset=True)
    out = fn()
    st = engine.stage_times(reset=True)
    return out, (st[STAGE][1] if STAGE in st else None)


class DeviceBytes:
    """n bytes of device memory (ocrs_device_malloc), freed on exit."""

    def __init__(self, nbytes):
        self.p = C.c_void_p()
        _lib.check(_lib.lib().ocrs_device_malloc(C.c_size_t(nbytes), C.byref(self.p)))
        self.nbytes = nbytes

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib.check(_lib.lib().ocrs_device_free(self.p))

    def put(self, offset, arr):
        """arr's bytes at `offset` -> the device address."""
        assert 0 <= offset and offset + arr.nbytes <= self.nbytes
        a = np.ascontiguousarray(arr)
        _lib.check(_lib.lib().ocrs_device_upload(C.c_void_p(self.p.value + offset), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))
        return self.p.value + offset


# ------------------------------------------------------------------------------------------------ every format x shape
@pytest.mark.parametrize("fmt", R.FORMATS, ids=[R.fmt_id(*f) for f in R.FORMATS])
def test_every_shape_of_a_format(eng, fmt):
    worst = 0.0
    for name, hw, px in R.format_pages(fmt):
        got, n = launches(eng, lambda: prepared(eng, px, fmt[1]))
        assert got.shape == (1,) + hw, name
        R.same_bits(got, oracle(px, fmt[1]), name + ": against the oracle")
        worst = max(worst, R.check_prepared(name, got, px, fmt[1]))
        assert n in (None, 1), name
    print("%s: largest |page - float64| / tol %.3f" % (R.fmt_id(*fmt), worst))
    assert worst <= 1.0


@pytest.mark.parametrize("order", ["hwc", "chw"])
def test_every_grey_byte(eng, order):
    px = R.grey_bytes(order)
    got = prepared(eng, px, order)
    R.same_bits(got, oracle(px, order), "every grey byte")
    print("every grey byte, %s: largest |page - float64| / tol %.3f" % (order, R.check_prepared("every grey byte", got, px, order)))


# ------------------------------------------------------------------------------------------------ every RGB triple
@pytest.fixture(scope="module")
def exhaustive():
    px = R.exhaustive_page()
    exp = oracle(px, "hwc")
    exp.setflags(write=False)
    return px, exp


def test_every_rgb_triple_on_the_four_pixel_path(eng, exhaustive):
    """prepare_input stages the pixels in a pool buffer, which is aligned: prepare_image_rgb8_x4_kernel, four trips."""
    px, exp = exhaustive
    got = prepared(eng, px, "hwc")
    R.same_bits(got, exp, "every RGB triple, x4: against the oracle")
    print("every RGB triple, x4: largest |page - float64| / tol %.3f" % R.check_prepared("every RGB triple", got, px, "hwc"))


@pytest.mark.parametrize("offset", (0,) + R.OFFSETS)
def test_every_rgb_triple_from_a_device_pointer(eng, exhaustive, offset):
    """The same page resident in HBM.  At offset 0 the 4-pixel kernel again (bench.py's call); 1, 2 or 3 bytes into a
    slightly larger buffer the source cannot be read as words and the scalar u8 kernel runs, past its cap (eight trips).
    The bits are the oracle's every time, and so each other's."""
    px, exp = exhaustive
    h, w = R.EXHAUSTIVE_HW
    assert R.x4_ok(*R.RGB8, h * w, offset) == (offset == 0)
    with DeviceBytes(px.nbytes + 16) as d:
        ptr = d.put(offset, px)
        assert ptr % 4 == offset
        got = eng.prepare_input_device(ptr, np.uint8, DimOrder.Hwc, h, w, 3).image()
    R.same_bits(got, exp, "every RGB triple, source at +%d: against the oracle" % offset)


# ------------------------------------------------------------------------------------------------ batches
@pytest.fixture(scope="module")
def batch_expected():
    cache = {}

    def get(case):
        if case not in cache:
            fmt, hw = case
            cache[case] = [oracle(p, fmt[1]) for p in R.batch_pages(fmt, hw)]
        return cache[case]
    return get


def assert_pages(what, got, exp, n):
    assert len(got) == n, what
    for i, g in enumerate(got):
        R.same_bits(g.image(), exp[i], "%s: page %d of %d" % (what, i, n))


@pytest.mark.parametrize("case", R.BATCH_CASES, ids=[R.batch_id(c) for c in R.BATCH_CASES])
def test_host_batches(eng, batch_expected, case):
    """prepare_input_batch_raw from ordinary and from page-locked memory: page i of the result is the oracle's page i, in
    every table, and the conversion is ceil(n / 32) launches."""
    (dt, order, chans), (h, w) = case
    pages, exp = R.batch_pages(*case), batch_expected(case)
    L = _lib.lib()
    pinned = []
    try:
        for p in pages:
            hp = C.c_void_p()
            _lib.check(L.ocrs_host_malloc(C.c_size_t(p.nbytes), C.byref(hp)))
            pinned.append(hp)
            C.memmove(hp, p.ctypes.data_as(C.c_void_p), p.nbytes)
        for kind, ptrs in (("ordinary", [p.ctypes.data for p in pages]), ("pinned", [hp.value for hp in pinned])):
            for n in R.BATCH_N:
                what = "%s, %s memory" % (R.batch_id(case), kind)
                got, count = launches(eng, lambda: eng.prepare_input_batch_raw(ptrs[:n], dt, ORDER[order], h, w, chans))
                assert_pages(what, got, exp, n)
                assert count in (None, R.tables(n)), (what, n, count)
    finally:
        for hp in pinned:
            _lib.check(L.ocrs_host_free(hp))


@pytest.mark.parametrize("case", R.BATCH_CASES, ids=[R.batch_id(c) for c in R.BATCH_CASES])
def test_device_batches_through_a_group(group, batch_expected, case):
    """prepare_input_device_batch of a one-device group (bench.py's call): every pointer aligned, then, for u8 sources,
    page 48 of 65 (the middle of the second table) one byte off its word boundary, which sends the whole call down the
    scalar path.  The same bits both times, and from the group's own upload of the host pages."""
    (dt, order, chans), (h, w) = case
    pages, exp = R.batch_pages(*case), batch_expected(case)
    member = group.member(0)[0]
    nbytes = pages[0].nbytes
    slot = -(-(nbytes + 4) // 256) * 256
    nmax = len(pages)
    with DeviceBytes((nmax + 1) * slot) as d:
        ptrs = [d.put(i * slot, p) for i, p in enumerate(pages)]
        assert all(p % 256 == 0 for p in ptrs)
        for n in R.BATCH_N:
            what = "%s, device memory" % R.batch_id(case)
            got, count = launches(member, lambda: group.prepare_input_device_batch(ptrs[:n], dt, ORDER[order], h, w, chans))
            assert_pages(what, got, exp, n)
            assert count in (None, R.tables(n)), (what, n, count)
        if np.dtype(dt) == np.uint8:     # never a float source: its loads need their alignment
            k = R.MISALIGNED_PAGE
            off = list(ptrs)
            off[k] = d.put(nmax * slot + 1, pages[k])
            assert off[k] % 4 == 1 and R.TABLE_PAGES <= k < 2 * R.TABLE_PAGES
            assert not R.batch_x4_ok(dt, order, chans, h * w, off)
            got, count = launches(member, lambda: group.prepare_input_device_batch(off, dt, ORDER[order], h, w, chans))
            assert_pages("%s, device memory, page %d at +1" % (R.batch_id(case), k), got, exp, nmax)
            assert count in (None, R.tables(nmax))
    # and the group's own upload of host pages: the same dealing, the same tables
    got, count = launches(member, lambda: group.prepare_input_batch(pages, ORDER[order]))
    assert_pages("%s, host pages through the group" % R.batch_id(case), got, exp, nmax)
    assert count in (None, R.tables(nmax))


@pytest.mark.parametrize("hw", R.BIG_BATCH_HW, ids=[R.hw_id(hw) for hw in R.BIG_BATCH_HW])
def test_batch_kernels_past_their_grid_caps(eng, hw):
    """Two u8 HWC RGB pages in one call, each past the cap of its kernel family (2049 x 2048: the 4-pixel batch kernel;
    1025 x 2051: the scalar one): the stride loops of the batch kernels, with a second page in blockIdx.y."""
    pages = R.big_batch_pages(hw)
    got, count = launches(eng, lambda: eng.prepare_input_batch_raw([p.ctypes.data for p in pages], np.uint8, DimOrder.Hwc, hw[0], hw[1], 3))
    assert_pages("two pages of %s" % R.hw_id(hw), got, [oracle(p, "hwc") for p in pages], 2)
    assert count in (None, 1)


# ------------------------------------------------------------------------------------------------ float specials
@pytest.mark.parametrize("fc", R.FLOAT_FORMATS, ids=["%s-%d" % f for f in R.FLOAT_FORMATS])
def test_planted_float_words(eng, fc):
    """NaN (quiet and signalling), +-Inf, -0.0, a denormal, +-1e30, 2 and -1 in every channel position; with four
    channels in alpha only, where nothing of them may reach the result."""
    order, chans = fc
    base, page, plants = R.planted_page(order, chans)
    got = prepared(eng, page, order)
    R.same_bits(got, oracle(page, order), "planted %s-%d: against the oracle" % fc)
    R.check_prepared("planted %s-%d" % fc, got, page, order)
    got_base = prepared(eng, base, order)
    if chans == 4:
        R.same_bits(got, got_base, "alpha-only plants: against the unplanted page")
        R.same_bits(got, prepared(eng, R.alpha_zeroed(page, order), order), "alpha-only plants: against alpha zeroed")
        assert np.isfinite(got).all()
    else:
        touched = np.zeros(got.size, bool)
        touched[[p for _, p, _ in plants]] = True
        R.same_bits(got.reshape(-1)[~touched], got_base.reshape(-1)[~touched], "pixels beside the plants")
        assert not np.isfinite(got.reshape(-1)[touched]).all() and np.isfinite(got.reshape(-1)[~touched]).all()


@pytest.mark.parametrize("fc", R.FLOAT_FORMATS, ids=["%s-%d" % f for f in R.FLOAT_FORMATS])
def test_negative_zero_and_denormal_pages(eng, fc):
    order, chans = fc
    for name, page in R.tiny_pages(order, chans):
        R.same_bits(prepared(eng, page, order), oracle(page, order), "%s %s-%d" % ((name,) + fc))


# ------------------------------------------------------------------------------------------------ JPEG
def test_jpeg_streams(eng):
    """prepare_input_jpeg hands its decoded RGB to the same conversion: the bits of prepare_input on PIL's pixels, at a
    plane that is not a multiple of four (scalar kernel), at an odd 4:2:0 page and at a grey stream."""
    PIL_Image = pytest.importorskip("PIL.Image")

    def encode(px, **kw):
        b = io.BytesIO()
        PIL_Image.fromarray(px).save(b, "JPEG", **kw)
        return b.getvalue()

    odd = synth.synthetic_page(5, 211, 97, lines=5, columns=1)
    grey = np.asarray(PIL_Image.fromarray(synth.synthetic_page(1, 64, 64, lines=2, columns=1)).convert("L"))
    streams = [("9x2", (9, 2), encode(np.random.default_rng(0).integers(0, 256, (9, 2, 3), dtype=np.uint8), quality=90, subsampling=0)),
               ("211x97 4:2:0", (211, 97), encode(odd, quality=90, subsampling=2)),
               ("64x64 grey", (64, 64), encode(grey, quality=80))]
    assert (9 * 2) % 4 != 0
    for name, hw, data in streams:
        rgb = np.ascontiguousarray(np.asarray(PIL_Image.open(io.BytesIO(data)).convert("RGB")))
        assert rgb.shape == hw + (3,), name
        got = eng.prepare_input_jpeg(data)[0].image()
        R.same_bits(got, prepared(eng, rgb, "hwc"), name + ": against prepare_input on PIL's pixels")
        R.same_bits(got, oracle(rgb, "hwc"), name + ": against the oracle on PIL's pixels")
