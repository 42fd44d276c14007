"""Page framing on the GPU: ocrs_engine_clean_frame_page[s], ocrs_engine_ink_profiles and
ocrs_engine_crop_page[s] equal tests/frame_ref.py on 32-bit words, bytes and integers, whatever the batch; frame,
split_spread, get_text(frame=...) and the CLI are the chains they are documented to be."""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import despeckle_pages as P
import frame_ref as FR
import models_util as M
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, OcrInput, _lib, output, synth, uncrop_rects
from test_gpu_binarize import SHAPES, planted

pytestmark = pytest.mark.gpu
F = np.float32
DENSITIES = (0.05, 0.5, 0.95)
DEPTHS = (0, 1, 2, 63, 64, 65)      # around the tile of 64: the ring ends inside the first tile, at its edge, in the second
SIDES = (15, 1, 2, 4, 8, 5)
MIN_AREAS = (0, 3)
COMBOS = [{"depth": d, "sides": s, "min_area": a} for d, s, a in itertools.product(DEPTHS, SIDES, MIN_AREAS)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    return OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(M.recognition_model_bytes()))


def image_of(page):
    return np.ascontiguousarray(page.image()[0])


def noise(seed, h, w, plant=False, ink=0.5):
    """[h, w] float32, uniform in [-0.5, 0.5) shifted so that a share `ink` of it lies under 0; plant: test_gpu_binarize.planted."""
    a = (np.random.default_rng(seed).random((h, w), dtype=F) - F(ink)).astype(F)
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


def check_batch(eng, pages, params, what):
    """One call for all the pages against the restatement of each -> the restatement's results."""
    made, masks, infos = eng.clean_frame_batch([eng.input_from_grey(p) for p in pages], params, mask=True, info=True)
    exps = []
    for i, (page, p) in enumerate(zip(pages, params)):
        exps.append(FR.clean_frame(page, **(p or {})))
        assert made[i].shape == (1,) + page.shape
        assert_same((image_of(made[i]), masks[i], infos[i]), exps[-1], "%s, page %d %s" % (what, i, p))
    return exps


def check(eng, page, what, **params):
    return check_batch(eng, [page], [params], what)[0]


# ------------------------------------------------------------------ 1. frame cleanup
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["%dx%d" % s for s in SHAPES])
def test_noise_at_every_depth_side_and_min_area(eng, k):
    """The product of ink shares, depths, sides and min_areas dealt round the shapes: every combination on some shape, every
    shape with every depth."""
    h, w = SHAPES[k]
    every = [dict(c, **({"paper": 0.125, "threshold": -0.125} if i % 5 == 0 else {})) for i, c in enumerate(COMBOS)]
    combos = [every[(k + 13 * j) % len(every)] for j in range(6)]   # over the shapes: all of them; an odd stride, so both min_areas
    combos += [{"depth": d, "sides": SIDES[(k + j) % 6]} for j, d in enumerate(DEPTHS)]
    pages = [noise(1000 * k + i, h, w, plant=True, ink=DENSITIES[(i + k) % 3]) for i in range(len(combos))]
    exps = check_batch(eng, pages, combos, "noise %dx%d" % (h, w))
    if h * w > 4000:
        assert sum(e[2]["removed"] for e in exps) > 10 and sum(e[2]["kept"] for e in exps) > 0


@pytest.mark.parametrize("shape", ((97, 211), (129, 127)), ids=lambda s: "%dx%d" % s)
def test_every_pattern(eng, shape):
    pages, params, names = [], [], []
    for i, (name, page, _) in enumerate(P.patterns(*shape)):
        for depth in (0, 17):
            pages.append(page)
            params.append({"depth": depth, "sides": SIDES[i % 6], "min_area": MIN_AREAS[(i // 6) % 2]})
            names.append(name)
    exps = check_batch(eng, pages, params, "patterns %dx%d" % shape)
    whole = {n: e[2] for n, p, e in zip(names, params, exps) if p["depth"] == 0 and p["sides"] == 15}
    assert any(i["removed_pixels"] > 1000 for i in whole.values()), "some pattern is one component that visits the whole page"


def test_a_j_leaves_the_ring_and_comes_back(eng):
    h, w, depth = 200, 200, 20
    page = P.paper(h, w)
    page[0:61, 100] = P.INK          # arm A: from the top edge down, far below the ring
    page[60, 100:111] = P.INK        # the turn, outside the ring
    page[5:61, 110] = P.INK          # arm B: back up into the ring, not as far as the edge
    out, mask, info = check(eng, page, "J", depth=depth)
    got = image_of(eng.clean_frame(eng.input_from_grey(page), depth=depth))
    assert got.tobytes() == out.tobytes()
    assert (got[0:depth, 100] == P.PAPER_FILL).all() and (got[depth:61, 100] == P.INK).all(), "arm A is removed down to row depth - 1 only"
    assert (got[5:61, 110] == P.INK).all() and (got[60, 100:111] == P.INK).all(), "arm B is untouched"
    assert (mask[5:depth, 110] == 4).all() and (mask[0:depth, 100] == 5).all() and (mask[depth:, :] == 0).all()
    assert info["removed"] == 1 and info["removed_pixels"] == depth and info["ring_ink"] == depth + (depth - 5) and info["kept"] == 0
    whole = check(eng, page, "J, no ring", depth=0)[2]
    assert whole["removed"] == 1 and whole["removed_pixels"] == 61 + 10 + 55 == whole["ink"], "without a ring the J is one component"


def test_a_one_pixel_outline_is_one_component_touching_every_side(eng):
    for h, w in ((97, 211), (129, 127), (2, 2), (3, 3)):
        page = P.paper(h, w)
        page[0, :] = page[h - 1, :] = page[:, 0] = page[:, w - 1] = P.INK
        n = h * w if min(h, w) <= 2 else 2 * (h + w) - 4
        exps = check_batch(eng, [page] * 30, [{"depth": d, "sides": s} for d in (0, 1) for s in range(1, 16)], "outline %dx%d" % (h, w))
        for _, mask, info in exps:
            assert info["removed"] == 1 and info["removed_pixels"] == n == info["ring_ink"] and mask[0, 0] == 5


def test_areas_at_min_area_and_inside_the_ring_only(eng):
    page = P.paper(100, 150)
    P.plant(page, 0, 62, 5)      # five pixels at the top edge, across the word boundary
    P.plant(page, 63, 0, 4)      # four at the left edge, across the tile boundary
    P.plant(page, 98, 62, 5)     # five at the bottom edge, across the word boundary
    P.plant(page, 40, 40, 5)     # not touching
    _, mask, info = check(eng, page, "min_area", min_area=5)
    assert (info["removed"], info["removed_pixels"], info["kept"], info["kept_pixels"]) == (2, 10, 1, 4)
    assert mask[0, 62] == 5 and mask[63, 0] == 6 and mask[98, 62] == 5 and mask[40, 40] == 4
    assert check(eng, page, "min_area + 1", min_area=6)[2]["kept"] == 3
    assert check(eng, page, "min_area 0", min_area=0)[2]["removed"] == 3
    bar = P.paper(160, 90)
    bar[0:100, 40:43] = P.INK    # 3 wide, 100 deep: 30 pixels of it lie in a ring of 10
    for min_area, removed in ((30, 1), (31, 0)):
        out, _, info = check(eng, bar, "bar", depth=10, min_area=min_area)
        assert (info["removed"], info["kept"]) == (removed, 1 - removed) and info["removed_pixels"] + info["kept_pixels"] == 30 == info["ring_ink"]
        assert (out[10:100, 40:43] == P.INK).all(), "nothing deeper than the ring changes"


def test_degenerate_pages(eng):
    one = np.full((1, 1), P.INK, F)
    for sides in range(1, 16):
        assert check(eng, one, "1x1", sides=sides)[2]["removed_pixels"] == 1
    assert check(eng, one, "1x1 kept", min_area=2)[2]["kept_pixels"] == 1
    for shape in ((1, 300), (300, 1), (2, 2), (1, 64), (64, 1), (1, 65)):
        for i, depth in enumerate((0, 1, 128)):
            check(eng, noise(7 + i, *shape, plant=True, ink=0.6), "%dx%d" % shape, depth=depth, sides=SIDES[i])
    for h, w in ((70, 130), (64, 64)):
        ink, nan = np.full((h, w), F(-0.25), F), np.full((h, w), np.nan, F)
        info = check(eng, ink, "all ink", depth=3)[2]
        assert info["removed"] == 1 and info["removed_pixels"] == h * w - (h - 6) * (w - 6) and info["counted"] == 0 and info["paper_bin"] == 255
        assert check(eng, ink, "all ink, no ring", depth=0, sides=8)[2]["removed_pixels"] == h * w
        assert check(eng, P.paper(h, w), "all paper")[2]["ring_ink"] == 0
        info = check(eng, nan, "all NaN")[2]
        assert info["ink"] == 0 and info["counted"] == 0 and info["paper_bin"] == 255
    page = P.paper(90, 90)
    page[0:30, 20:23] = P.INK
    info = check(eng, page, "no ink on that side", sides=1 | 4 | 8)[2]
    assert info["removed"] == 0 and info["kept"] == 0 and info["ring_ink"] == 90


def test_the_longest_row_and_the_longest_column(eng):
    line = np.full(65535, P.PAPER, F)
    line[100:100 + 64 * 1001 + 7] = P.INK      # one run over more than 1000 mask words
    line[0:2] = P.INK                          # touching the first pixel
    line[65535 - 1] = P.INK                    # the last pixel alone
    line[64 * 1010 + 63:64 * 1010 + 65] = P.INK   # across a word boundary, touching nothing but the long sides
    row, col = line.reshape(1, -1), line.reshape(-1, 1)
    exps = check_batch(eng, [row, col, row, col], [{"depth": 0, "sides": 1 | 4}, {"depth": 0, "sides": 2 | 8}, {"depth": 0}, {"depth": 0, "sides": 1}],
                       "longest")
    assert [(e[2]["removed"], e[2]["removed_pixels"]) for e in exps] == [(2, 3), (2, 3), (4, 64 * 1001 + 7 + 5), (4, 64 * 1001 + 7 + 5)]


MIXED = [((97, 211), {"depth": 17, "sides": 5}), ((128, 256), {"depth": 0, "min_area": 3, "paper": 0.25}), ((1, 300), {"depth": 1}),
         ((70, 258), {"depth": 64, "sides": 8, "threshold": 0.125}), ((65, 63), {"depth": 2, "min_area": 2}), ((260, 130), None)]


def test_mixed_batch_equals_each_page_alone_ten_times(eng):
    srcs = [noise(40 + i, *s, plant=i % 2 == 0, ink=0.6) for i, (s, _) in enumerate(MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in MIXED]
    exp = [FR.clean_frame(s, **(p or {})) for s, p in zip(srcs, params)]
    first = None
    for rep in range(10):
        pages, masks, infos = eng.clean_frame_batch(inputs, params, mask=True, info=True)
        got = [(image_of(p), m, i) for p, m, i in zip(pages, masks, infos)]
        if first is None:
            first = got
            for i, g in enumerate(got):
                assert_same(g, exp[i], "batch page %d" % i)
                alone = eng.clean_frame(inputs[i], mask=True, info=True, **(params[i] or {}))
                assert alone[2] == g[2] and image_of(alone[0]).tobytes() == g[0].tobytes() and alone[1].tobytes() == g[1].tobytes(), "page %d alone" % i
        else:
            assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(got, first)), "repeat %d" % rep
    assert [image_of(p).tobytes() for p in eng.clean_frame_batch(inputs[:2], {"depth": 2})] == \
        [image_of(eng.clean_frame(i, depth=2)).tobytes() for i in inputs[:2]], "one parameter set for all"
    assert eng.clean_frame_batch([], None) == [] and eng.clean_frame_batch([], None, mask=True, info=True) == ([], [], [])
    with pytest.raises(ValueError):
        eng.clean_frame_batch(inputs, params[:2])


def test_mask_alone_info_alone_and_neither(eng):
    src = noise(21, 70, 130, ink=0.6)
    inp = eng.input_from_grey(src)
    exp = FR.clean_frame(src, depth=5, sides=3)
    kw = {"depth": 5, "sides": "lt"}
    page = eng.clean_frame(inp, **kw)
    assert isinstance(page, OcrInput) and image_of(page).tobytes() == exp[0].tobytes()
    page, mask = eng.clean_frame(inp, mask=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and mask.tobytes() == exp[1].tobytes()
    page, info = eng.clean_frame(inp, info=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and info == exp[2] and tuple(info) == FR.INFO_KEYS
    assert image_of(eng.clean_frame(inp)).tobytes() == FR.clean_frame(src)[0].tobytes(), "the defaults"


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = noise(99, 131, 70, ink=0.6)
    inp = eng.input_from_grey(src)
    exp = FR.clean_frame(src, depth=4)[0]
    out = eng.clean_frame(inp, depth=4)
    assert image_of(inp).tobytes() == src.tobytes()
    del out   # ocrs_page_free of the result: the source is a page of its own
    assert image_of(inp).tobytes() == src.tobytes()
    out = eng.clean_frame(inp, depth=4)
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == exp.tobytes()
    again = eng.clean_frame(out, depth=9)   # a cleaned page is an ordinary page
    assert image_of(again).tobytes() == FR.clean_frame(exp, depth=9)[0].tobytes()


def test_bad_parameters_have_their_status(eng):
    inp = eng.input_from_grey(noise(1, 20, 20))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    inf, nan = float("inf"), float("nan")
    for kw in ({"depth": -1}, {"depth": 65536}, {"sides": 0}, {"sides": 16}, {"min_area": -1}, {"threshold": inf}, {"threshold": nan},
               {"paper": inf}, {"paper": -inf}):
        refused(lambda: eng.clean_frame(inp, **kw))
    refused(lambda: eng.clean_frame_batch([inp, inp], [None, {"sides": 16}]))   # one bad page refuses the call
    live = _lib.pool_stats()["device_live"]
    pages = (C.c_void_p * 2)(inp._h, inp._h)
    for bad in (_lib.FrameParams(0.0, 65536, 15, 0, nan), _lib.FrameParams(0.0, 128, 0, 0, nan), _lib.FrameParams(0.0, 128, 15, 0, inf)):
        ps = (_lib.FrameParams * 2)(_lib.FrameParams(0.0, 128, 15, 0, nan), bad)
        out = (C.c_void_p * 2)()
        masks = (C.POINTER(C.c_uint8) * 2)()
        assert _lib.lib().ocrs_engine_clean_frame_pages(eng._h, pages, C.c_size_t(2), ps, out, masks, None) == 1, "INVALID_ARGUMENT"
        assert [out[i] for i in range(2)] == [None, None] and not masks[0] and not masks[1], "a failed call writes nothing"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    one = C.c_void_p()
    assert _lib.lib().ocrs_engine_clean_frame_page(eng._h, inp._h, None, None, None, None) == 1
    assert _lib.lib().ocrs_engine_clean_frame_page(eng._h, inp._h, None, C.byref(one), None, None) == 0, "NULL: the default"
    assert image_of(OcrInput(one)).tobytes() == image_of(eng.clean_frame(inp)).tobytes()   # (the OcrInput frees the page)
    wide = eng.input_from_grey(np.zeros((1, 65536), F))
    refused(lambda: eng.clean_frame(wide))
    refused(lambda: eng.ink_profiles(wide))
    refused(lambda: eng.ink_profiles(inp, threshold=nan))


# ------------------------------------------------------------------ 2. ink profiles
def test_ink_profiles_equal_numpy(eng):
    for k, (h, w) in enumerate(SHAPES + [(1, 65535), (2000, 3)]):
        src = noise(300 + k, h, w, plant=True, ink=DENSITIES[k % 3])
        inp = eng.input_from_grey(src)
        for thr in (0.0, 0.25):
            cols, rows = eng.ink_profiles(inp, thr)
            ec, er = FR.profiles(src, thr)
            assert cols.dtype == np.uint32 and rows.dtype == np.uint32 and np.array_equal(cols, ec) and np.array_equal(rows, er), (h, w, thr)
        c, r = eng.ink_profiles(inp, rows=False)
        assert r is None and np.array_equal(c, FR.profiles(src)[0])
        c, r = eng.ink_profiles(inp, cols=False)
        assert c is None and np.array_equal(r, FR.profiles(src)[1])
        assert eng.ink_profiles(inp, cols=False, rows=False) == (None, None)
    assert image_of(inp).tobytes() == src.tobytes()


# ------------------------------------------------------------------ 3. crop
def crop_rects(h, w):
    """Inside, flush with each side, overhanging each side, wholly outside, 1 x 1; x0 % 4 in {0, 1, 3} with widths that are
    and are not multiples of 4."""
    out = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, w, h), (-1, -1, 0, 0), (w, h, w + 1, h + 1), (w + 5, 0, w + 13, 3), (0, -9, 8, -2),
           (-3, -2, w + 3, h + 1), (min(2, w - 1), -3, w, h + 3), (-70, -70, w + 70, h + 70), (-5, 0, 3, h), (w - 3, 0, w + 5, h), (0, -5, w, 2), (0, h - 2, w, h + 6)]
    for x0 in (0, 1, 3, 4, 65, 67):
        for cw in (4, 8, 64, 68, 5, 63, 130):
            out.append((x0, 1, x0 + cw, 1 + min(h, 67)))
    return out


@pytest.mark.parametrize("shape", ((97, 211), (70, 256), (1, 300), (300, 1)), ids=lambda s: "%dx%d" % s)
def test_crop_equals_numpy(eng, shape):
    src = noise(5, *shape, plant=True)
    inp = eng.input_from_grey(src)
    rects = crop_rects(*shape)
    fills = [np.array([0x7F812345 + i], np.uint32).view(F)[0] if i % 2 else np.float32(0.5 - i) for i in range(len(rects))]   # signalling NaNs with payloads
    made = eng.crop_batch([inp] * len(rects), rects, fills)
    for page, rect, fill in zip(made, rects, fills):
        exp = FR.crop(src, rect, fill)
        got = image_of(page)
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), (rect, fill)
    alone = eng.crop(inp, rects[7], fills[7])
    assert image_of(alone).tobytes() == FR.crop(src, rects[7], fills[7]).tobytes() and image_of(inp).tobytes() == src.tobytes()
    assert image_of(eng.crop(inp, (-2, -2, 2, 2))).tobytes() == FR.crop(src, (-2, -2, 2, 2), 0.5).tobytes(), "the default fill is white"


def test_crop_of_a_mixed_batch_and_bad_rectangles(eng):
    srcs = [noise(60 + i, *s, plant=True) for i, s in enumerate(((97, 211), (1, 1), (300, 3), (64, 64), (5, 1000)))]
    inputs = [eng.input_from_grey(s) for s in srcs]
    rects = [(-3, 5, 129, 60), (-1, -1, 3, 2), (1, 100, 2, 299), (0, 0, 64, 64), (997, -2, 1003, 9)]
    exp = [FR.crop(s, r, 0.25) for s, r in zip(srcs, rects)]
    for rep in range(3):
        made = eng.crop_batch(inputs, rects, 0.25)
        assert [image_of(p).tobytes() for p in made] == [e.tobytes() for e in exp], rep
    assert eng.crop_batch([], []) == []
    with pytest.raises(ValueError):
        eng.crop_batch(inputs, rects[:2])
    live = _lib.pool_stats()["device_live"]
    for bad in ((0, 0, 0, 5), (5, 0, 5, 5), (3, 0, 2, 5), (0, 4, 5, 4), (0, 0, 65536, 1), (0, 0, 1, 65536), (-2 ** 31, 0, 2 ** 31 - 1, 1)):
        with pytest.raises(_lib.OcrsError) as e:
            eng.crop_batch(inputs[:2], [(0, 0, 4, 4), bad])
        assert e.value.status_name == "INVALID_ARGUMENT", bad
    assert _lib.pool_stats()["device_live"] == live, "a failing call leaves no page behind"
    far = eng.crop(inputs[0], (2 ** 31 - 9, -2 ** 31, 2 ** 31 - 1, -2 ** 31 + 3), 0.125)
    assert (image_of(far) == F(0.125)).all() and far.shape == (1, 3, 8)


# ------------------------------------------------------------------ 4. a text page and a spread
def grey_of(eng, px):
    return image_of(eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc)))


def test_a_text_page_loses_its_bar_wedge_and_slice_and_no_text(eng):
    clean = grey_of(eng, synth.synthetic_page(3, 512, 512, 30, 2, 1))
    text = clean < 0
    assert int(text.sum()) == 63704
    frame = np.zeros(clean.shape, bool)
    frame[:, :9] = True                           # a 9-pixel bar down the left
    for y in range(14):
        frame[y, 9:9 + 490 - 28 * y] = True       # a 14-row wedge along the top
    frame[1:511, 506:512] = True                  # a slice of the neighbouring page on the right
    assert int((frame & ~text).sum()) == 11980 and int(frame[:, 500:].sum()) == 3060
    page = clean.copy()
    page[frame] = F(-0.45)
    out, mask, info = check(eng, page, "text page")
    assert info["removed_pixels"] == 11980 and info["removed"] == 2 and info["kept"] == 0
    assert np.array_equal(mask & 1 > 0, frame & ~text) and not ((mask & 1 > 0) & text).any(), "exactly the planted pixels, no text ink"
    assert np.array_equal(out < 0, text) and out[text].tobytes() == clean[text].tobytes()
    out, mask, info = check(eng, page, "text page, slice kept", min_area=5000)
    assert (info["removed"], info["removed_pixels"], info["kept"], info["kept_pixels"]) == (1, 11980 - 3060, 1, 3060)
    assert (mask[1:511, 506:512] == 6).all()
    # frame(): the cleaned page cut down to the text and its margin
    framed, origin, finfo = eng.frame(eng.input_from_grey(page), info=True, pad=4)
    cols, rows = FR.profiles(FR.clean_frame(page)[0])
    c = FR.choose(512, 512, cols, rows, pad=4)
    assert finfo["choice"] == c and origin == (c["x0"], c["y0"]) and c["found"] == 1 and c["x0"] > 0 and c["y0"] > 0
    assert image_of(framed).tobytes() == FR.crop(FR.clean_frame(page)[0], (c["x0"], c["y0"], c["x1"], c["y1"]), 0.5).tobytes()
    blank, origin = eng.frame(eng.input_from_grey(P.paper(40, 50)))
    assert origin == (0, 0) and image_of(blank).tobytes() == P.paper(40, 50).tobytes(), "a page without ink comes back whole"
    with pytest.raises(TypeError):
        eng.frame(eng.input_from_grey(page), radius=3)


def spread_picture():
    """Two synthetic pages side by side, a gap between them and in it a gutter shadow from the top edge to the bottom."""
    left, right = synth.synthetic_page(11, 300, 260, lines=10, columns=1), synth.synthetic_page(12, 300, 260, lines=10, columns=1)
    px = np.full((300, 560, 3), 255, np.uint8)
    px[:, :260], px[:, 300:] = left, right
    px[:, 277:283] = 40
    return px


def test_a_spread_splits_into_its_two_pages(eng):
    px = spread_picture()
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    grey = image_of(inp)
    cleaned, _, cinfo = FR.clean_frame(grey, depth=0)
    assert cinfo["removed"] == 1 and cinfo["removed_pixels"] == 6 * 300, "the shadow alone touches the frame"
    c = FR.choose(300, 560, *FR.profiles(cleaned))
    assert 260 <= c["gutter_x"] <= 300 and c["found"] == 1
    parts, info = eng.split_spread(inp, depth=0, info=True)
    assert info["choice"] == c and [o for _, o in parts] == [(c["x0"], c["y0"]), (c["gutter_x"], c["y0"])]
    for (page, origin), x1 in zip(parts, (c["gutter_x"], c["x1"])):
        alone = FR.crop(cleaned, (origin[0], origin[1], x1, c["y1"]), 0.5)
        assert image_of(page).tobytes() == alone.tobytes()
        words = eng.detect_words(page)
        shifted = uncrop_rects(eng.detect_words(eng.input_from_grey(alone)), origin)
        assert len(words) > 10 and uncrop_rects(words, origin).tobytes() == shifted.tobytes() == FR.uncrop_rects(words, origin).tobytes()
        assert ((shifted[:, 0] < c["gutter_x"]) == (origin[0] < c["gutter_x"])).all(), "every word lies on its own page"
    assert len(eng.split_spread(inp, depth=0, gutter_min_width=200)) == 1, "no run that long: one page"
    one = eng.split_spread(eng.input_from_grey(grey_of(eng, synth.synthetic_page(11, 300, 260, lines=10, columns=1))))
    assert len(one) == 1
    # the manual chain, and where get_text applies it
    framed = eng.frame(inp, depth=0)[0]
    assert eng.get_text(inp, frame={"depth": 0}) == eng.get_text(framed)
    assert eng.get_text(inp, frame=True) == eng.get_text(eng.frame(inp)[0])
    norm = eng.normalize(inp)
    assert eng.get_text(inp, normalize=True, frame=True, despeckle=True) == eng.get_text(eng.despeckle(eng.frame(norm)[0])), "after normalisation, before despeckling"
    assert eng.get_text(inp, frame=True, orientation=2) == eng.get_text(eng.rotate(eng.frame(inp)[0], 2)), "before the turn"
    assert eng.get_text(inp, frame=None) == eng.get_text(inp) == eng.get_text(inp, frame=False)


def test_cli_frame_crop_and_split_spread(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models, uncrop_lines
    px = spread_picture()
    path = str(tmp_path / "spread.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("frame", "tuned", "crop", "spread", "plain")}
    assert cli.main([path, "--frame", "-j", "--debug", "-o", files["frame"]]) == 0
    assert cli.main([path, "--frame", "--frame-depth", "0", "--frame-sides", "TB", "--frame-min-area", "100", "--frame-pad", "3", "-j", "-o", files["tuned"]]) == 0
    assert cli.main([path, "--crop", "290,-10,570,200", "-j", "-o", files["crop"]]) == 0
    assert cli.main([path, "--split-spread", "--frame-depth", "0", "-j", "-o", files["spread"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in (["--frame-depth", "9"], ["--frame-sides", "L"], ["--frame", "--frame-sides", "X"], ["--frame", "--frame-depth", "65536"],
                ["--crop", "1,2,3"], ["--crop", "0,0,0,5"], ["--crop", "a,b,c,d"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def read(page, origin):
        lines = eng.find_text_lines(page, eng.detect_words(page))
        return uncrop_lines(eng.recognize_text(page, lines), origin)

    def document(parts, info):
        finfo = {k: v for k, v in info.items() if k != "choice"}
        finfo["boxes"] = [[o[0], o[1], o[0] + p.shape[-1], o[1] + p.shape[-2]] for p, o in parts]
        return output.format_json_output(path, px.shape[:2], sum((read(p, o) for p, o in parts), []), frame=finfo)

    plain = output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "frame" not in json.loads(plain), "without the flags nothing changes"
    page, origin, info = eng.frame(inp, info=True)
    assert text["frame"] == document([(page, origin)], info)
    assert set(json.loads(text["frame"])["frame"]) == set(FR.INFO_KEYS) | {"boxes"}
    page, origin, info = eng.frame(inp, info=True, depth=0, sides="TB", min_area=100, pad=3)
    assert text["tuned"] == document([(page, origin)], info) and info["removed"] == 1
    parts, info = eng.split_spread(inp, info=True, depth=0)
    assert len(parts) == 2 and text["spread"] == document(parts, info)
    zone = eng.crop(inp, (290, -10, 570, 200))
    assert text["crop"] == output.format_json_output(path, px.shape[:2], read(zone, (290, -10)))
    assert len(json.loads(text["crop"])["paragraphs"][0]["lines"]) > 0


# ------------------------------------------------------------------ 5. beside other callers
def test_framing_callers_beside_plain_callers(eng):
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    barred = []
    for i, p in enumerate(pages):
        g = image_of(p).copy()
        g[:, :7 + i] = F(-0.4)
        g[:5, :] = F(-0.4)
        barred.append(g)
    inputs = [eng.input_from_grey(s) for s in barred]
    params = [{}, {"depth": 0, "min_area": 3}, {"depth": 3, "sides": 1}, {"depth": 64, "paper": 0.25}]

    def cut(i):
        page, mask, info = eng.clean_frame(inputs[i], mask=True, info=True, **params[i])
        cols, rows = eng.ink_profiles(page)
        part = eng.crop(page, (-3, 2, 200 + i, 131))
        return image_of(page).tobytes(), mask.tobytes(), tuple(sorted(info.items())), cols.tobytes(), rows.tobytes(), image_of(part).tobytes()

    def plain(i):
        return eng.detect_words(pages[i]).tobytes()

    quiet_cut, quiet_plain = [cut(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        out, mask, info = FR.clean_frame(barred[i], **params[i])
        cols, rows = FR.profiles(out)
        assert quiet_cut[i] == (out.tobytes(), mask.tobytes(), tuple(sorted(info.items())), cols.tobytes(), rows.tobytes(),
                                FR.crop(out, (-3, 2, 200 + i, 131), 0.5).tobytes())
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, cut(i) if t < 4 else plain(i))
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
        assert got == (quiet_cut[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)
