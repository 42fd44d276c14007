"""Reverse-video repair on the GPU, bit for bit against tests/reverse_ref.py.

Pages are put on the device with input_from_grey; results are compared as 32-bit words (every pixel is the page's own word
or that word with its sign bit flipped, NaN payloads included, so the words are compared as they are); the mask and what
the passes counted (ocrs_reverse_info) are compared as bytes and integers.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import models_util as M
import reverse_pages as P
import reverse_ref as R
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, OcrInput, _lib, output, synth
from oracle import pipeline as OP
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu
F = np.float32
# (height, width): the shapes of test_gpu_despeckle.py: one pixel, one row, one column; around one word and one 64 x 64 tile
# either way; several tiles with partial edges; every width % 4 (the 16-byte path needs % 4 == 0)
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (65, 63), (127, 129), (129, 127), (97, 211), (70, 256), (70, 257), (70, 258),
          (70, 259)]
# at 0.7 the 8-connected ink percolates and encloses paper: that is where panels arise
DENSITIES = (0.05, 0.3, 0.5, 0.7, 0.95)
SWEEP = [{"min_height": mh, "min_width": mw, "min_fill": mf, "min_holes": n, "max_hole": Hm}
         for mh, mw, mf, n, Hm in itertools.product((1, 2, 5), (1, 2, 5), (0.0, 0.3, 0.6), (0, 1, 2), (0, 1, 3))]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    return OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(M.recognition_model_bytes()))


@pytest.fixture(scope="module")
def ora():
    return OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                        recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))


def image_of(page):
    return np.ascontiguousarray(page.image()[0])


def planted(a, seed):
    """NaN (quiet and signalling), +-inf, -0.0, values far outside [-0.5, 0.5] and denormals written over random places of
    the page as 32-bit words (fewer on a page of fewer pixels)."""
    words = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x40400000, 0xC0400000, 0x7F7FFFFF,
                      0xFF7FFFFF, 0x00000001, 0x80000001], np.uint32)
    flat = a.reshape(-1).view(np.uint32)
    n = min(len(words), max(1, flat.size // 8))
    flat[np.random.default_rng(seed).choice(flat.size, size=n, replace=False)] = words[:n]
    return a


def noise(seed, h, w, plant=False, ink=0.5):
    """[h, w] float32, uniform in [-0.5, 0.5) shifted so that a share `ink` of it lies under 0; plant: see planted()."""
    rng = np.random.default_rng(seed)
    a = (rng.random((h, w), dtype=np.float32) - np.float32(ink)).astype(np.float32)
    return planted(a, seed) if plant else a


def assert_same(got, exp, what):
    """(page, mask, info) of the library against the restatement's."""
    out, mask, info = got
    assert info == exp[2], (what, info, exp[2])
    assert out.dtype == np.float32 and out.shape == exp[0].shape and mask.dtype == np.uint8 and mask.shape == exp[1].shape, what
    bad = np.argwhere(out.view(np.uint32) != exp[0].view(np.uint32))
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r (%#x), expected %r (%#x)"
                             % (what, len(bad), out.size, at, out[at], out.view(np.uint32)[at], exp[0][at], exp[0].view(np.uint32)[at]))
    bad = np.argwhere(mask != exp[1])
    assert not len(bad), "%s: %d mask bytes differ; first at %s: got %d, expected %d" % (what, len(bad), tuple(bad[0]), mask[tuple(bad[0])], exp[1][tuple(bad[0])])


def expected(pages, params):
    """The restatement of every page; pages that are the same array share one labelling of the ink."""
    exps, analyses = [], {}
    for page, p in zip(pages, params):
        key = (id(page), (p or {}).get("threshold", 0.0))
        if key not in analyses:
            analyses[key] = R.analyse(page, key[1])
        exps.append(R.unreverse(page, analysis=analyses[key], **(p or {})))
    return exps


def check_batch(eng, pages, params, what, exps=None):
    """One call for all the pages against the restatement of each -> the restatement's results."""
    exps = expected(pages, params) if exps is None else exps
    made, masks, infos = eng.unreverse_batch([eng.input_from_grey(p) for p in pages], params, mask=True, info=True)
    for i, (page, p) in enumerate(zip(pages, params)):
        assert made[i].shape == (1,) + page.shape
        assert_same((image_of(made[i]), masks[i], infos[i]), exps[i], "%s, page %d %s" % (what, i, p))
    return exps


def check(eng, page, what, **params):
    return check_batch(eng, [page], [params], what)[0]


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_noise_at_every_density_and_small_parameter_equals_the_restatement(eng, shape):
    h, w = shape
    pages = [noise(h * 1000 + w + 7 * i, h, w, plant=plant, ink=ink) for i, (ink, plant) in enumerate(itertools.product(DENSITIES, (False, True)))]
    dealt = [pages[i % len(pages)] for i in range(len(SWEEP))]   # the sweep dealt round the pages: 243 pages in one call
    exps = expected(dealt, SWEEP)
    most = {k: max(e[2][k] for e in exps) for k in R.INFO_KEYS}
    print(shape, most)
    if h >= 63 and w >= 63:   # of the restatement, before the GPU is asked: every counter occurs
        assert all(v > 0 for v in most.values()), most
    check_batch(eng, dealt, SWEEP, "noise %dx%d" % shape, exps)


PLANTED = [((97, 211), 61, 62), ((129, 127), 64, 64), ((129, 127), 52, 1), ((97, 211), 63, 127)]


@pytest.mark.parametrize("shape,oy,ox", PLANTED, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_every_planted_pattern_equals_the_restatement_and_its_hand_stated_answer(eng, shape, oy, ox):
    """The bands, their holes and the holes' first pixels across word and tile boundaries: a band whose own first pixel is
    bit 0 of a word in row 0 of a tile (64, 64), bands that straddle the corner of four tiles, a band at the page's first
    column."""
    pats = P.patterns(shape[0], shape[1], oy, ox)
    exps = check_batch(eng, [p[1] for p in pats], [p[2] for p in pats], "planted %s at %d, %d" % (shape, oy, ox))
    for (name, page, kw, flipped, info), exp in zip(pats, exps):
        assert np.array_equal((exp[1] & 1).astype(bool), flipped) and {k: exp[2][k] for k in info} == info, name


def test_a_hole_at_bit_0_of_row_0_of_a_tile_and_bands_over_many_tiles(eng):
    pages, params = [], []
    a = P.band_with_marks(129, 127, 60, 61, P.FOUR)   # the first mark's first pixel: row 64, column 64
    assert a[64, 64] == P.PAPER and a[64, 63] == P.INK and a[63, 64] == P.INK
    pages.append(a)
    params.append(P.SMALL)
    for shape in ((97, 211), (129, 127), (200, 330)):   # a band over every tile of the page but its outermost pixels, marks in every tile
        h, w = shape
        a = P.canvas(h, w)
        a[1:h - 1, 1:w - 1] = P.INK
        for y in range(5, h - 8, 23):
            for x in range(4, w - 8, 29):
                a[y:y + 3, x:x + 4] = P.PAPER
        a[64:70, 64:90] = P.PAPER   # a card whose first pixel is bit 0 of a word in row 0 of a tile
        a[66, 70] = P.INK
        pages += [a, a, a]
        params += [None, {"max_hole": 12}, {"min_holes": 10 ** 6}]
    exps = check_batch(eng, pages, params, "tiles")
    assert exps[0][2]["panels"] == 1 and exps[0][2]["inverted"] == 480
    for i in (1, 4, 7):
        h, w = pages[i].shape
        assert exps[i][2]["panels"] == 1 and exps[i][2]["inverted"] == (h - 2) * (w - 2) and exps[i][2]["skipped_holes"] == 0
        assert exps[i + 1][2]["skipped_holes"] == 1 and exps[i + 1][2]["inverted"] == (h - 2) * (w - 2) - 6 * 26
        assert exps[i + 2][2]["candidates"] == 1 and exps[i + 2][2]["panels"] == 0 and exps[i + 2][2]["inverted"] == 0


def test_edge_shapes(eng):
    small = {"min_height": 1, "min_width": 1}
    for shape in ((1, 1), (1, 7), (1, 130), (9, 1), (130, 1), (2, 2), (3, 3), (70, 130)):
        n = shape[0] * shape[1]
        for kw in (small, dict(small, min_holes=0), {}):
            exp = check(eng, np.full(shape, -0.5, F), "all ink", **kw)
            assert exp[2]["ink"] == n and exp[2]["components"] == 1 and exp[2]["inverted"] == (n if kw.get("min_holes") == 0 else 0)
            exp = check(eng, np.full(shape, 0.4, F), "all paper", **kw)
            assert exp[2] == dict.fromkeys(R.INFO_KEYS, 0)
            exp = check(eng, np.full(shape, np.nan, F), "all NaN", **kw)
            assert exp[2] == dict.fromkeys(R.INFO_KEYS, 0)
        check(eng, np.zeros(shape, F), "zero is not ink")
    a = np.full((3, 3), -0.5, F)
    a[1, 1] = np.nan
    exp = check(eng, a, "a NaN hole", min_height=3, min_width=3, min_holes=1)
    assert exp[2]["inverted"] == 9 and exp[2]["holes"] == 1


def test_the_longest_row_and_the_longest_column(eng):
    row = np.full((1, 65535), 0.25, F)
    row[0, 100:5000] = row[0, 40000:40003] = row[0, 63] = row[0, 64] = row[0, 65534] = -0.25
    row[0, 2000] = 0.25
    pages = [row, row, np.ascontiguousarray(row.T), np.ascontiguousarray(row.T)]
    params = [{"min_height": 1, "min_width": 100, "min_holes": 0}, {"min_height": 1, "min_width": 100}, {"min_height": 100, "min_width": 1, "min_holes": 0},
              {"min_height": 1, "min_width": 1, "min_holes": 0, "min_fill": 1.0}]
    exps = check_batch(eng, pages, params, "65535")
    assert exps[0][2]["panels"] == 2 and exps[0][2]["inverted"] == 4899 and exps[1][2]["inverted"] == 0   # a row has no holes
    assert exps[2][2]["inverted"] == 4899 and exps[3][2]["panels"] == exps[3][2]["components"] == 5


def test_threshold(eng):
    page = planted(noise(12, 97, 211, ink=0.7) * np.float32(0.5), 12)
    for thr in (-0.05, 0.1, 1e30, -1e30):
        exp = check(eng, page, "threshold %g" % thr, threshold=thr, min_height=2, min_width=2, min_fill=0.3, min_holes=1, max_hole=3)
        assert exp[2]["panels"] > 0 or abs(thr) > 1


MIXED = [((97, 211), {"min_height": 2, "min_width": 2, "min_fill": 0.3, "min_holes": 1}), ((128, 256), {"min_height": 5, "min_width": 5, "max_hole": 2, "min_holes": 2}),
         ((1, 300), {"min_height": 1, "min_width": 1, "min_holes": 0}), ((70, 258), {"min_height": 1, "min_width": 1, "min_fill": 0.0, "min_holes": 0, "threshold": 0.1}),
         ((65, 63), {"min_height": 2, "min_width": 1, "threshold": -0.2, "min_holes": 1}), ((260, 130), None)]


def test_mixed_batch_equals_each_page_alone_ten_times(eng):
    srcs = [noise(40 + i, *s, plant=i % 2 == 0, ink=0.7) for i, (s, _) in enumerate(MIXED)]
    srcs[5][20:200, 10:120] = -0.4   # the defaults find a panel on the last page
    for y in range(40, 180, 30):
        srcs[5][y:y + 6, 30:50] = 0.4
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in MIXED]
    exp = [R.unreverse(s, **(p or {})) for s, p in zip(srcs, params)]
    assert exp[5][2]["panels"] == 1 and all(e[2]["inverted"] > 0 for e in exp)
    first = None
    for rep in range(10):
        pages, masks, infos = eng.unreverse_batch(inputs, params, mask=True, info=True)
        got = [(image_of(p), m, i) for p, m, i in zip(pages, masks, infos)]
        if first is None:
            first = got
            for i, g in enumerate(got):
                assert_same(g, exp[i], "batch page %d" % i)
                alone = eng.unreverse(inputs[i], mask=True, info=True, **(params[i] or {}))
                assert alone[2] == g[2] and image_of(alone[0]).tobytes() == g[0].tobytes() and alone[1].tobytes() == g[1].tobytes(), "page %d alone" % i
        else:
            assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(got, first)), "repeat %d" % rep
    one = {"min_height": 2, "min_width": 2, "min_holes": 1}
    assert [image_of(p).tobytes() for p in eng.unreverse_batch(inputs[:2], one)] == \
        [image_of(eng.unreverse(i, **one)).tobytes() for i in inputs[:2]], "one parameter set for all"
    assert eng.unreverse_batch([], None) == [] and eng.unreverse_batch([], None, mask=True, info=True) == ([], [], [])
    with pytest.raises(ValueError):
        eng.unreverse_batch(inputs, params[:2])


def test_mask_alone_info_alone_and_neither(eng):
    src = noise(21, 70, 130, ink=0.7)
    inp = eng.input_from_grey(src)
    kw = {"min_height": 2, "min_width": 2, "min_fill": 0.3, "min_holes": 1, "max_hole": 3}
    exp = R.unreverse(src, **kw)
    assert exp[2]["inverted"] > 0 and exp[2]["skipped_holes"] > 0
    page = eng.unreverse(inp, **kw)
    assert isinstance(page, OcrInput) and image_of(page).tobytes() == exp[0].tobytes()
    page, mask = eng.unreverse(inp, mask=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and mask.tobytes() == exp[1].tobytes()
    page, info = eng.unreverse(inp, info=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and info == exp[2] and tuple(info) == R.INFO_KEYS
    src4 = noise(22, 70, 132, ink=0.7)   # the 16-byte path without a byte mask
    assert image_of(eng.unreverse(eng.input_from_grey(src4), **kw)).tobytes() == R.unreverse(src4, **kw)[0].tobytes()


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = P.band_with_marks(131, 70, 60, 20, P.FOUR)
    inp = eng.input_from_grey(src)
    exp = R.unreverse(src, **P.SMALL)[0]
    out = eng.unreverse(inp, **P.SMALL)
    assert image_of(inp).tobytes() == src.tobytes()
    del out   # ocrs_page_free of the result: the source is a page of its own
    assert image_of(inp).tobytes() == src.tobytes()
    out = eng.unreverse(inp, **P.SMALL)
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == exp.tobytes() and exp.tobytes() != src.tobytes()
    again, info = eng.unreverse(out, info=True, **P.SMALL)   # a repaired page is an ordinary page, and the repair is idempotent
    assert image_of(again).tobytes() == exp.tobytes() and info["panels"] == 0


def test_bad_parameters_have_their_status(eng):
    inp = eng.input_from_grey(noise(1, 20, 20))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    nan, inf = float("nan"), float("inf")
    for kw in ({"min_height": 0}, {"min_height": 65536}, {"min_height": -3}, {"min_width": 0}, {"min_width": 65536}, {"min_fill": -0.01},
               {"min_fill": 1.01}, {"min_fill": nan}, {"min_fill": inf}, {"min_holes": -1}, {"max_hole": -1}, {"threshold": nan},
               {"threshold": inf}, {"threshold": -inf}):
        refused(lambda: eng.unreverse(inp, **kw))
    refused(lambda: eng.unreverse_batch([inp, inp], [None, {"min_holes": -1}]))   # one bad page refuses the call
    live = _lib.pool_stats()["device_live"]
    L = _lib.lib()
    pages = (C.c_void_p * 2)(inp._h, inp._h)
    ok = (_lib.ReverseParams * 2)(_lib.ReverseParams(0.0, 32, 64, 0.4, 3, 0), _lib.ReverseParams(0.0, 32, 64, 0.4, 3, 0))
    ps = (_lib.ReverseParams * 2)(_lib.ReverseParams(0.0, 32, 64, 0.4, 3, 0), _lib.ReverseParams(0.0, 32, 64, 0.4, 3, -1))
    out = (C.c_void_p * 2)()
    masks = (C.POINTER(C.c_uint8) * 2)()
    infos = (_lib.ReverseInfo * 2)()
    C.memset(infos, 0xAB, C.sizeof(infos))
    assert L.ocrs_engine_unreverse_pages(eng._h, pages, C.c_size_t(2), ps, out, masks, infos) == 1, "INVALID_ARGUMENT"
    assert L.ocrs_engine_unreverse_pages(eng._h, None, C.c_size_t(2), ok, out, masks, infos) == 1
    assert L.ocrs_engine_unreverse_pages(eng._h, pages, C.c_size_t(2), None, out, masks, infos) == 1
    assert L.ocrs_engine_unreverse_pages(eng._h, pages, C.c_size_t(2), ok, None, masks, infos) == 1
    assert L.ocrs_engine_unreverse_pages(None, pages, C.c_size_t(2), ok, out, masks, infos) == 1
    assert L.ocrs_engine_unreverse_pages(eng._h, (C.c_void_p * 2)(inp._h, None), C.c_size_t(2), ok, out, masks, infos) == 1, "a null page"
    assert [out[i] for i in range(2)] == [None, None] and not masks[0] and not masks[1], "a failed call writes nothing"
    assert bytes(infos) == b"\xab" * C.sizeof(infos)
    assert L.ocrs_engine_unreverse_pages(eng._h, None, C.c_size_t(0), None, None, None, None) == 0, "an empty batch"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    one = C.c_void_p()
    assert L.ocrs_engine_unreverse_page(eng._h, inp._h, None, None, None, None) == 1
    assert L.ocrs_engine_unreverse_page(eng._h, inp._h, None, C.byref(one), None, None) == 0, "NULL: the default"
    assert image_of(OcrInput(one)).tobytes() == image_of(eng.unreverse(inp)).tobytes()   # (the OcrInput frees the page)
    wide = eng.input_from_grey(np.zeros((1, 65536), F))
    refused(lambda: eng.unreverse(wide))


# ------------------------------------------------------------------ 2. the text page
@pytest.fixture(scope="module")
def text_page(ora):
    """The 512 x 512 text page of DESIGN.md §7.9 with 20 lines in one column, and the same with a rectangle of several lines
    of words, and 6 pixels of margin around them, in reverse video."""
    px = synth.synthetic_page(3, 512, 512, 20, 1, 1)
    clean = np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), np.float32)[0])
    ink = clean < 0
    rows = np.nonzero(ink.any(axis=1))[0]
    breaks = np.nonzero(np.diff(rows) > 1)[0]
    tops = np.concatenate([rows[:1], rows[breaks + 1]])   # the first row of every line of text
    bottoms = np.concatenate([rows[breaks], rows[-1:]])
    assert len(tops) >= 10
    y0, y1 = int(tops[4]) - 6, int(bottoms[8]) + 7   # five lines
    cols = np.nonzero(ink[y0:y1].any(axis=0))[0]
    x0, x1 = max(int(cols[0]) - 6, 1), min(int(cols[-1]) + 7, 511)
    assert y0 >= 1 and y1 <= 511 and not ink[y0:y0 + 6, x0:x1].any() and not ink[y1 - 6:y1, x0:x1].any()
    reversed_ = clean.copy()
    reversed_.view(np.uint32)[y0:y1, x0:x1] ^= np.uint32(0x80000000)
    return clean, reversed_, (y0, y1, x0, x1)


def test_a_reversed_block_of_text_comes_back(eng, text_page):
    """DESIGN.md §7.15 records the counts: of the original page's word boxes, how many the detector gives back within 2 pixels
    on the reversed and on the repaired page (the synthetic detector; a trained one is uncalibrated)."""
    clean, rev, (y0, y1, x0, x1) = text_page
    exp = check(eng, rev, "the reversed block")
    assert exp[2]["panels"] == 1 and exp[2]["holes"] >= 3
    margin = np.zeros(clean.shape, bool)
    margin[y0:y1, x0:x1] = True
    margin[y0 + 6:y1 - 6, x0 + 6:x1 - 6] = False
    differs = exp[0].view(np.uint32) != clean.view(np.uint32)
    assert not differs[~margin].any(), "the original page bit for bit, but for the planted margin"
    print("reversed block %d x %d: %d pixels inverted, %d of the margin's %d differ from the original"
          % (y1 - y0, x1 - x0, exp[2]["inverted"], int(differs.sum()), int(margin.sum())))
    back = check(eng, clean, "the original page")
    assert back[2]["panels"] == 0 and back[0].tobytes() == clean.tobytes()
    native = eng.detect_words(eng.input_from_grey(clean))

    def recovered(page):
        rects = eng.detect_words(page)
        n = 0
        for r in native:
            d = np.abs(rects[:, [0, 1, 4, 5]] - r[[0, 1, 4, 5]]).max(axis=1) if len(rects) else np.array([np.inf])
            n += bool(d.min() <= 2.0)
        return n, len(rects)

    on_reversed, on_repaired = recovered(eng.input_from_grey(rev)), recovered(eng.unreverse(eng.input_from_grey(rev)))
    print("detection effect: %d original boxes; on the reversed page %d of %d boxes match, on the repaired page %d of %d"
          % (len(native), on_reversed[0], on_reversed[1], on_repaired[0], on_repaired[1]))
    assert len(native) > 50 and on_repaired[0] >= on_reversed[0]


# ------------------------------------------------------------------ 3. composition
def reversed_picture(seed, h, w, lines):
    """A synthetic page as a picture with a band of its lines in reverse video and a dark sidebar with light marks at its
    left edge, which clean_frame would remove as a bar."""
    px = synth.synthetic_page(seed, h, w, lines=lines, columns=1)
    grey = px.reshape(h, w, -1).astype(np.int32).mean(axis=2)
    rows = np.nonzero((grey < 128).any(axis=1))[0]
    y0, y1 = int(rows[len(rows) // 3]) - 8, int(rows[2 * len(rows) // 3]) + 8
    px[y0:y1, 12:w - 8] = 255 - px[y0:y1, 12:w - 8]
    px[20:h - 20, 0:10] = 0   # two pixels of paper lie between it and the band, and the words begin further right
    for y in range(40, h - 40, 50):
        px[y:y + 6, 3:7] = 255
    return px


def test_get_text_with_unreverse_is_the_manual_chain(eng):
    inp = eng.prepare_input(ImageSource.from_tensor(reversed_picture(5, 600, 500, 24), DimOrder.Hwc))
    for params in (True, {"min_height": 16, "min_width": 8, "max_hole": 4000}):   # the defaults take the band; these the sidebar and some solid words too
        kw = {} if params is True else params
        page, info = eng.unreverse(inp, info=True, **kw)
        assert info["panels"] == 1 if params is True else info["panels"] > 2
        assert image_of(page).tobytes() == R.unreverse(image_of(inp), **kw)[0].tobytes()
        assert eng.get_text(inp, unreverse=params) == eng.get_text(page) and eng.get_text(page) != eng.get_text(inp)
        assert eng.get_text(inp, unreverse=params, rectify=True) == eng.get_text(page, rectify=True)
        binar = eng.binarize(eng.normalize(inp))   # after normalisation and binarisation ...
        fixed = eng.unreverse(binar, **kw)
        assert eng.get_text(inp, unreverse=params, normalize=True, binarize=True) == eng.get_text(fixed)
        framed = eng.frame(fixed)[0]               # ... before frame ...
        assert eng.get_text(inp, unreverse=params, normalize=True, binarize=True, frame=True) == eng.get_text(framed)
        assert eng.get_text(inp, unreverse=params, normalize=True, binarize=True, frame=True, despeckle=True) == eng.get_text(eng.despeckle(framed))
        assert eng.get_text(inp, unreverse=params, despeckle=True) == eng.get_text(eng.despeckle(page))   # ... and despeckling
    assert eng.get_text(inp, unreverse=None) == eng.get_text(inp) == eng.get_text(inp, unreverse=False)


def test_cli_unreverse(tmp_path, monkeypatch, capsys):
    from PIL import Image

    from ocrs_amd import cli, models
    px = reversed_picture(9, 700, 600, 30)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("fixed", "tuned", "plain")}
    assert cli.main([path, "--unreverse", "-j", "--debug", "-o", files["fixed"]]) == 0
    assert "Unreverse: " in capsys.readouterr().out
    assert cli.main([path, "--unreverse", "--unreverse-min-height", "16", "--unreverse-min-width", "20", "--unreverse-min-fill", "0.5",
                     "--unreverse-min-holes", "2", "--unreverse-max-hole", "5000", "-j", "-o", files["tuned"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in (["--unreverse-min-height", "9"], ["--unreverse-min-width", "9"], ["--unreverse-min-fill", "0.5"], ["--unreverse-min-holes", "1"],
                ["--unreverse-max-hole", "1"], ["--unreverse", "--unreverse-min-height", "0"], ["--unreverse", "--unreverse-min-width", "65536"],
                ["--unreverse", "--unreverse-min-fill", "1.5"], ["--unreverse", "--unreverse-min-holes", "-1"],
                ["--unreverse", "--unreverse-max-hole", "-1"], ["--unreverse", "--unreverse-min-fill", "x"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def document(**kw):
        page, info = eng.unreverse(inp, info=True, **kw)
        lines = eng.find_text_lines(page, eng.detect_words(page))
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(page, lines), unreverse=info), info

    plain = output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "unreverse" not in json.loads(plain), "without the flag nothing changes"
    exp, info = document()
    assert text["fixed"] == exp and info["panels"] == 1
    assert json.loads(text["fixed"])["unreverse"] == info and set(info) == set(R.INFO_KEYS)
    assert text["tuned"] == document(min_height=16, min_width=20, min_fill=0.5, min_holes=2, max_hole=5000)[0]


# ------------------------------------------------------------------ 4. beside other callers
def test_unreverse_callers_beside_plain_callers(eng, ora):
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    rev = []
    for i, p in enumerate(pages):
        a = image_of(p).copy()
        a.view(np.uint32)[60 + 10 * i:200, 20:380 - 10 * i] ^= np.uint32(0x80000000)
        rev.append(eng.input_from_grey(a))
    params = [{}, {"min_height": 16, "max_hole": 300}, {"min_holes": 1}, {"min_fill": 0.6, "min_width": 100}]

    def fixed(i):
        page, mask, info = eng.unreverse(rev[i], mask=True, info=True, **params[i])
        return image_of(page).tobytes(), mask.tobytes(), tuple(sorted(info.items()))

    def plain(i):
        return eng.detect_words(pages[i]).tobytes()

    quiet_fixed, quiet_plain = [fixed(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        out, mask, info = R.unreverse(image_of(rev[i]), **params[i])
        assert quiet_fixed[i] == (out.tobytes(), mask.tobytes(), tuple(sorted(info.items())))
        words = ora.detect_words(ora.prepare_input(OP.ImageSource.from_tensor(pxs[i], "hwc")))
        assert len(words) > 5 and quiet_plain[i] == np.array([w.to_array() for w in words], np.float32).tobytes()
    assert sum(dict(q[2])["panels"] for q in quiet_fixed) >= 2
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, fixed(i) if t < 4 else plain(i))
        except Exception as e:   # pragma: no cover - reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert len(results) == 24
    for (t, r), (i, got) in results.items():
        assert got == (quiet_fixed[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)
