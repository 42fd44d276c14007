"""Grain removal on the GPU, bit for bit against tests/rank_ref.py.

Pages are put on the device with input_from_grey; results are compared as 32-bit words (a result pixel is the word of a
source pixel and NaN pixels keep their payloads, so the words are compared as they are); the mask and what the kernel
counted (ocrs_rank_info) are compared as integers.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import models_util as M
import morph_ref
import rank_ref as R
import ocrs_amd
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, OcrInput, _lib, output, synth
from test_gpu_binarize import SHAPES as BIN_SHAPES, level, planted, two_level

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
TILE_H, TILE_W = 16, 64   # kernels.hpp RANK_TILE_H, RANK_TILE_W: the pixels a block decides
LDS_H, LDS_W = TILE_H + 2 * R.MAX_RADIUS, TILE_W + 2 * R.MAX_RADIUS   # the region a block stages at the largest radii: 30 x 78
# test_gpu_binarize's shapes (one pixel, one row, one column, around a wave of 64, several blocks), and one under, at and one
# over each side of the tile and of the staged region
SHAPES = BIN_SHAPES + [(TILE_H - 1, LDS_W - 1), (TILE_H, LDS_W), (TILE_H + 1, LDS_W + 1), (LDS_H - 1, TILE_W - 1), (LDS_H, TILE_W), (LDS_H + 1, TILE_W + 1)]
# (rx, ry): the issue's, and both sides of the radii at which the kernel changes how it holds the window (kernels.hpp
# rank_class: the larger radius <= 1 a 3 x 3 window in registers, <= 2 a 5 x 5 one, above that the LDS loop)
RADII = [(1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3), (3, 1), (7, 0), (0, 7), (7, 7)]
PERCENTS = (0, 1, 35, 50, 99, 100)
TAILS = (0, 10, 20, 50)
DENSITIES = (0.05, 0.5, 0.95)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    return OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(M.recognition_model_bytes()))


def image_of(page):
    return np.ascontiguousarray(page.image()[0])


def noise(seed, h, w, plant=True, ink=0.5):
    """[h, w] float32, uniform in [-0.5, 0.5) shifted so that a share `ink` of it lies under 0; plant: NaN of both kinds,
    +-inf, +-0, denormals and huge values over random places (test_gpu_binarize.planted)."""
    a = (np.random.default_rng(seed).random((h, w), dtype=F) - F(ink)).astype(F)
    return planted(a, seed) if plant else a


def ramp(h, w, axis, rising):
    """Strictly monotone along `axis`: every key of a window is another one along that axis."""
    n = (h, w)[axis]
    v = (np.arange(n, dtype=np.float64) / max(n - 1, 1) - 0.5).astype(F)
    v = v if rising else v[::-1]
    return np.ascontiguousarray(np.broadcast_to(v[:, None] if axis == 0 else v[None, :], (h, w)))


def assert_same(got, exp, what):
    """(page, mask, info) of the library against the restatement's."""
    out, mask, info = got
    assert info == exp[2], (what, info, exp[2])
    assert out.dtype == np.float32 and out.shape == exp[0].shape and mask.dtype == np.uint8 and mask.shape == exp[1].shape, what
    bad = np.argwhere(out.view(U) != exp[0].view(U))
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r (%#x), expected %r (%#x)"
                             % (what, len(bad), out.size, at, out[at], out.view(U)[at], exp[0][at], exp[0].view(U)[at]))
    bad = np.argwhere(mask != exp[1])
    assert not len(bad), "%s: %d mask bytes differ; first at %s: got %d, expected %d" % (what, len(bad), tuple(bad[0]), mask[tuple(bad[0])], exp[1][tuple(bad[0])])


def check_batch(eng, pages, params, what):
    """One call for all the pages against the restatement of each -> the restatement's results.  Pages that are the same
    object with the same radii share the restatement's windows."""
    made, masks, infos = eng.rank_batch([eng.input_from_grey(p) for p in pages], params, mask=True, info=True)
    exps, wins = [], {}
    for i, (page, p) in enumerate(zip(pages, params)):
        q = dict(R.default_params(), **(p or {}))
        key = (id(page), q["rx"], q["ry"])
        if key not in wins:
            wins[key] = R.windows(page, q["rx"], q["ry"])
        exps.append(R.rank(page, win=wins[key], **q))
        assert made[i].shape == (1,) + page.shape
        assert_same((image_of(made[i]), masks[i], infos[i]), exps[-1], "%s, page %d %s" % (what, i, p))
    return exps


def check(eng, page, what, **params):
    return check_batch(eng, [page], [params], what)[0]


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_parameter_on_noise_two_level_pages_and_ramps(eng, shape):
    h, w = shape
    fixed = [noise(h * 1000 + w + 7 * i, h, w, ink=ink) for i, ink in enumerate(DENSITIES)]
    fixed += [two_level("halves", h, w, 1), two_level("checkerboard", h, w, 1), ramp(h, w, 0, True), ramp(h, w, 1, False)]
    exps, turn = [], 0
    for rx, ry in RADII:   # a call per radius; every page with every tail, the percents going round: all 24 pairs, many times over
        pages, params = [], []
        every = fixed + [two_level("stripes", h, w, rx), two_level("rows", h, w, ry)]
        if h * w > 40000 and (2 * rx + 1) * (2 * ry + 1) > 100:   # the restatement sorts 225 planes of the page: every other page
            every = every[::2]
        for page in every:
            for j, tail in enumerate(TAILS):
                pages.append(page)
                params.append({"rx": rx, "ry": ry, "percent": PERCENTS[(turn + j) % len(PERCENTS)], "tail": tail})
            turn += 1
        exps += check_batch(eng, pages, params, "%dx%d" % shape)
    moved, spared = sum(e[2]["changed"] > 0 for e in exps), sum(e[2]["spared"] > 0 for e in exps)
    print(shape, len(exps), "pages;", moved, "of them changed,", spared, "with spared pixels")
    if h * w > 1:   # an identity kernel does not pass, and neither does one that never spares
        assert moved > 0 and spared > 0 and any(0 < e[2]["counted"] < h * w for e in exps)
        assert any(0 < e[2]["spared"] < e[2]["counted"] for e in exps)


@pytest.mark.parametrize("radius", [(7, 7), (2, 2), (1, 1)], ids=lambda r: "r%d" % r[0])
def test_library_against_library_percent_0_is_thicken_and_100_is_thin(eng, radius):
    rx, ry = radius
    srcs = [noise(300 + i, *s, ink=0.4) for i, s in enumerate([(97, 211), (TILE_H + 1, LDS_W + 1), (1, 300), (300, 1), (65, 63), (33, 70)])]
    inputs = [eng.input_from_grey(s) for s in srcs]
    for percent, op in ((0, "thicken"), (100, "thin")):
        for r in ((rx, ry), (rx, 0), (0, ry), (max(rx - 1, 1), ry)):
            a, ai = eng.rank_batch(inputs, {"rx": r[0], "ry": r[1], "percent": percent, "tail": 0}, info=True)
            b, bi = eng.morph_batch(inputs, {"op": op, "rx": r[0], "ry": r[1]}, info=True)
            for i in range(len(inputs)):
                assert image_of(a[i]).tobytes() == image_of(b[i]).tobytes(), (op, r, i)
                assert {k: ai[i][k] for k in morph_ref.INFO_KEYS} == bi[i] and ai[i]["spared"] == 0


def test_the_longest_row_and_the_longest_column(eng):
    row = noise(8, 1, 65535, ink=0.4)
    col = np.ascontiguousarray(row.reshape(65535, 1))
    params = [{"rx": 7, "ry": 7, "percent": 50, "tail": 0}, {"rx": 7, "ry": 7, "percent": 35, "tail": 20}, {"rx": 7, "ry": 7, "percent": 100, "tail": 10}]
    wide = check_batch(eng, [row] * 3, params, "1 x 65535")
    tall = check_batch(eng, [col] * 3, params, "65535 x 1")
    # the least that changes: at percent 100 with tail 10 a window of 15 distinct keys spares the ranks 1 .. 13 and its
    # greatest key is the filter's value already, so only the pixel of rank 0 moves: one in 15 of 65 535, 4 369
    for a, b in zip(wide, tall):
        assert a[2] == b[2] and a[2]["changed"] > 4000 and a[0].tobytes() == b[0].tobytes()
    check_batch(eng, [ramp(1, 65535, 1, True), ramp(65535, 1, 0, False)], [{"rx": 7, "ry": 0, "percent": 0, "tail": 0}, {"rx": 0, "ry": 7, "percent": 99, "tail": 50}], "ramps")


def test_nan_beside_dark_and_pages_that_are_nearly_all_nan(eng):
    page, rx, ry = morph_ref.nan_beside_dark()
    for percent, tail in itertools.product(PERCENTS, TAILS):
        check(eng, page, "the NaN beside the dark pixel", rx=rx, ry=ry, percent=percent, tail=tail)
    exp = check(eng, page, "the NaN beside the dark pixel", rx=rx, ry=ry, percent=0, tail=0)
    assert exp[0].view(U)[0, 1] == page.view(U)[1, 0] and exp[2] == {"counted": 8, "changed": 4, "ink_before": 1, "ink_after": 5, "spared": 0}
    for shape in ((70, 130), (5, 300)):
        nans = np.full(shape, np.nan, F)
        nans.view(U)[3, 4] = 0xFFC12345   # payloads are kept
        nans.view(U)[0, 0] = 0x7F800001
        one = nans.copy()
        one[2, 100] = F(-0.5)
        flat = np.full(shape, level(40), F)
        for (percent, tail), (rx, ry) in itertools.product(((50, 20), (0, 0), (100, 50)), ((1, 1), (2, 2), (7, 7))):
            exp = check(eng, nans, "all NaN", rx=rx, ry=ry, percent=percent, tail=tail)
            assert exp[2] == dict.fromkeys(R.INFO_KEYS, 0) and exp[0].view(U).tobytes() == nans.view(U).tobytes()
            exp = check(eng, one, "one counted pixel", rx=rx, ry=ry, percent=percent, tail=tail)
            assert exp[2] == {"counted": 1, "changed": 0, "ink_before": 1, "ink_after": 1, "spared": 1 if tail else 0}
            assert exp[0].view(U).tobytes() == one.view(U).tobytes()
            exp = check(eng, flat, "flat", rx=rx, ry=ry, percent=percent, tail=tail)
            assert exp[2]["changed"] == 0 and exp[0].tobytes() == flat.tobytes()


# ------------------------------------------------------------------ 2. batches
MIXED = [((97, 211), {"rx": 3, "ry": 1, "percent": 50, "tail": 0}), ((128, 256), {"rx": 7, "ry": 7, "percent": 35, "tail": 20}),
         ((1, 300), {"rx": 5, "ry": 0, "percent": 99, "tail": 10}), ((70, 258), {"rx": 0, "ry": 2, "percent": 1, "tail": 50}),
         ((65, 63), {"rx": 1, "ry": 1, "percent": 50, "tail": 20}), ((260, 130), None), ((33, 70), {"rx": 2, "ry": 2, "percent": 100, "tail": 0})]


def test_mixed_batch_equals_each_page_alone_ten_times(eng):
    srcs = [noise(40 + i, *s, ink=0.3) for i, (s, _) in enumerate(MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in MIXED]
    exp = [R.rank(s, **(p or {})) for s, p in zip(srcs, params)]
    first = None
    for rep in range(10):
        pages, masks, infos = eng.rank_batch(inputs, params, mask=True, info=True)
        got = [(image_of(p), m, i) for p, m, i in zip(pages, masks, infos)]
        if first is None:
            first = got
            for i, g in enumerate(got):
                assert_same(g, exp[i], "batch page %d" % i)
                alone = eng.rank(inputs[i], mask=True, info=True, **(params[i] or {}))
                assert alone[2] == g[2] and image_of(alone[0]).tobytes() == g[0].tobytes() and alone[1].tobytes() == g[1].tobytes(), "page %d alone" % i
        else:
            assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(got, first)), "repeat %d" % rep
    for order in (slice(None, None, -1), slice(0, 1), slice(1, 2), slice(3, 5)):
        pages = eng.rank_batch(inputs[order], params[order])
        assert [image_of(p).tobytes() for p in pages] == [e[0].tobytes() for e in exp[order]]
    assert [image_of(p).tobytes() for p in eng.rank_batch(inputs[:2], {"rx": 2, "percent": 35})] == \
        [image_of(eng.rank(i, rx=2, percent=35)).tobytes() for i in inputs[:2]], "one parameter set for all"
    assert eng.rank_batch([], None) == [] and eng.rank_batch([], None, mask=True, info=True) == ([], [], [])
    with pytest.raises(ValueError):
        eng.rank_batch(inputs, params[:2])


def test_mask_alone_info_alone_and_neither(eng):
    src = noise(21, 70, 130, ink=0.3)
    inp = eng.input_from_grey(src)
    exp = R.rank(src, 5, 2, 35, 10)
    kw = {"rx": 5, "ry": 2, "percent": 35, "tail": 10}
    page = eng.rank(inp, **kw)
    assert isinstance(page, OcrInput) and image_of(page).tobytes() == exp[0].tobytes()
    page, mask = eng.rank(inp, mask=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and mask.tobytes() == exp[1].tobytes()
    page, info = eng.rank(inp, info=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and info == exp[2] and tuple(info) == R.INFO_KEYS
    assert image_of(eng.rank(inp)).tobytes() == R.rank(src)[0].tobytes(), "the defaults: the median of 3 x 3 on outliers"
    assert image_of(eng.rank(inp, rx=3)).tobytes() == R.rank(src, 3, 3)[0].tobytes(), "ry follows rx"


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = noise(99, 131, 70, ink=0.3)
    inp = eng.input_from_grey(src)
    exp = R.rank(src, 4, 4)[0]
    out = eng.rank(inp, rx=4)
    assert image_of(inp).tobytes() == src.tobytes()
    del out   # ocrs_page_free of the result: the source is a page of its own
    assert image_of(inp).tobytes() == src.tobytes()
    out = eng.rank(inp, rx=4)
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == exp.tobytes()
    again = eng.rank(out, rx=7, ry=1, percent=99, tail=0)   # a filtered page is an ordinary page
    assert image_of(again).tobytes() == R.rank(exp, 7, 1, 99, 0)[0].tobytes()


def test_bad_parameters_have_their_status(eng):
    inp = eng.input_from_grey(noise(1, 20, 20))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    for kw in ({"rx": 0}, {"rx": 8}, {"rx": -1}, {"rx": 1, "ry": 8}, {"rx": 1, "ry": -1}, {"rx": 0, "ry": 0}, {"percent": 101}, {"percent": -1},
               {"tail": 51}, {"tail": -1}):
        refused(lambda: eng.rank(inp, **kw))
    refused(lambda: eng.rank_batch([inp, inp], [None, {"rx": 8}]))   # one bad page refuses the call
    live = _lib.pool_stats()["device_live"]
    pages = (C.c_void_p * 2)(inp._h, inp._h)
    for bad in (_lib.RankParams(8, 1, 50, 20), _lib.RankParams(1, -1, 50, 20), _lib.RankParams(0, 0, 50, 20), _lib.RankParams(1, 1, 101, 20),
                _lib.RankParams(1, 1, 50, 51)):
        ps = (_lib.RankParams * 2)(_lib.RankParams(1, 1, 50, 20), bad)
        out = (C.c_void_p * 2)()
        masks = (C.POINTER(C.c_uint8) * 2)()
        assert _lib.lib().ocrs_engine_rank_pages(eng._h, pages, C.c_size_t(2), ps, out, masks, None) == 1, "INVALID_ARGUMENT"
        assert [out[i] for i in range(2)] == [None, None] and not masks[0] and not masks[1], "a failed call writes nothing"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    one = C.c_void_p()
    assert _lib.lib().ocrs_engine_rank_page(eng._h, inp._h, None, None, None, None) == 1
    ok = (_lib.RankParams * 1)(_lib.RankParams(1, 1, 50, 20))
    assert _lib.lib().ocrs_engine_rank_pages(eng._h, None, C.c_size_t(1), ok, C.byref(one), None, None) == 1
    assert _lib.lib().ocrs_engine_rank_pages(eng._h, pages, C.c_size_t(1), None, C.byref(one), None, None) == 1
    assert _lib.lib().ocrs_engine_rank_page(eng._h, inp._h, None, C.byref(one), None, None) == 0, "NULL: the default"
    assert image_of(OcrInput(one)).tobytes() == image_of(eng.rank(inp)).tobytes()   # (the OcrInput frees the page)
    wide = eng.input_from_grey(np.zeros((1, 65536), F))
    refused(lambda: eng.rank(wide))
    # a page belongs to a device: another engine of this device serves it, an engine of another device refuses it
    dbuf, rbuf = M.detection_model_bytes(), M.recognition_model_bytes()
    same = OcrEngine(detection_model=Model.load_bytes(dbuf), recognition_model=Model.load_bytes(rbuf))
    assert image_of(same.rank(inp)).tobytes() == image_of(eng.rank(inp)).tobytes()
    if _lib.device_count() >= 2:
        other = OcrEngine(detection_model=Model.load_bytes(dbuf, device=1), recognition_model=Model.load_bytes(rbuf, device=1))
        refused(lambda: other.rank(inp))


# ------------------------------------------------------------------ 3. composition
def grainy_picture(seed, h, w, lines):
    """A synthetic page with salt and pepper over it, as a picture."""
    px = synth.synthetic_page(seed, h, w, lines=lines, columns=1)
    u = np.random.default_rng(seed).random((h, w))
    px[u < 0.03] = 0
    px[u > 0.97] = 255
    return px


def test_get_text_with_rank_is_the_manual_chain(eng):
    inp = eng.prepare_input(ImageSource.from_tensor(grainy_picture(5, 600, 500, 24), DimOrder.Hwc))
    for params in (True, {"rx": 1, "ry": 0, "percent": 50, "tail": 0}, {"rx": 2}):
        kw = {} if params is True else params
        page, info = eng.rank(inp, info=True, **kw)
        assert info["changed"] > 1000
        assert image_of(page).tobytes() == R.rank(image_of(inp), **dict(R.default_params(), **ocrs_amd.rank_params(**kw)))[0].tobytes()
        lines = eng.find_text_lines(page, eng.detect_words(page))
        text = "\n".join(str(t) for t in eng.recognize_text(page, lines) if t is not None)
        assert eng.get_text(inp, rank=params) == text
        norm = eng.normalize(inp)
        assert eng.get_text(inp, rank=params, normalize=True) == eng.get_text(eng.rank(norm, **kw))   # after normalisation ...
        assert eng.get_text(inp, rank=params, normalize=True, binarize=True) == eng.get_text(eng.binarize(eng.rank(norm, **kw)))   # ... before binarisation
        assert eng.get_text(inp, rank=params, binarize=True, despeckle=True) == eng.get_text(eng.despeckle(eng.binarize(eng.rank(inp, **kw))))
    assert eng.get_text(inp, rank=None) == eng.get_text(inp) == eng.get_text(inp, rank=False)


def test_without_rank_get_text_launches_what_it_launched(eng):
    inp = eng.prepare_input(ImageSource.from_tensor(grainy_picture(6, 400, 500, 16), DimOrder.Hwc))
    eng.get_text(inp)
    eng.enable_timing(2)
    try:
        counts = []
        for kw in ({}, {"rank": None}, {"rank": False}):
            eng.kernel_stats(reset=True)
            text = eng.get_text(inp, **kw)
            counts.append((text, {name: s["launches"] for name, s in eng.kernel_stats(reset=True).items()}))
    finally:
        eng.enable_timing(0)
    assert counts[0] == counts[1] == counts[2] and sum(counts[0][1].values()) > 0


def test_cli_rank(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    px = grainy_picture(9, 700, 600, 30)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("default", "two", "row", "plain")}
    assert cli.main([path, "--rank", "-j", "--debug", "-o", files["default"]]) == 0
    assert cli.main([path, "--rank", "2", "-j", "-o", files["two"]]) == 0
    assert cli.main([path, "--rank", "1x0:50:0", "-j", "-o", files["row"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in ("median", "8", "0", "0x0", "1x", "x1", "1x2x3", "1:101", "1:50:51", "1:50:20:1", "1:", ":", "-1"):
        with pytest.raises(SystemExit):
            cli.main([path, "--rank=" + bad])
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def document(**kw):
        page, info = eng.rank(inp, info=True, **kw)
        lines = eng.find_text_lines(page, eng.detect_words(page))
        record = dict(info, **ocrs_amd.rank_params(**kw))
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(page, lines), rank=record), record

    plain = output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "rank" not in json.loads(plain), "without the flag nothing changes"
    exp, record = document()
    assert text["default"] == exp and record["changed"] > 1000 and record["spared"] > 1000
    assert json.loads(text["default"])["rank"] == record == dict(record, rx=1, ry=1, percent=50, tail=20)
    assert set(record) == set(R.INFO_KEYS) | {"rx", "ry", "percent", "tail"}
    exp, record = document(rx=2)
    assert text["two"] == exp and json.loads(text["two"])["rank"] == dict(record, rx=2, ry=2, percent=50, tail=20)
    exp, record = document(rx=1, ry=0, percent=50, tail=0)
    assert text["row"] == exp and json.loads(text["row"])["rank"] == dict(record, rx=1, ry=0, percent=50, tail=0, spared=0)


# ------------------------------------------------------------------ 4. beside other callers
def test_rank_callers_beside_plain_callers(eng):
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    damaged = [R.salt_and_pepper(image_of(p), 0.1, 7 + i) for i, p in enumerate(pages)]
    inputs = [eng.input_from_grey(s) for s in damaged]
    params = [{}, {"rx": 7, "ry": 7, "percent": 35, "tail": 10}, {"rx": 2, "ry": 0, "percent": 50, "tail": 0}, {"rx": 0, "ry": 3, "percent": 99, "tail": 50}]

    def clean(i):
        page, mask, info = eng.rank(inputs[i], mask=True, info=True, **params[i])
        return image_of(page).tobytes(), mask.tobytes(), tuple(sorted(info.items()))

    def plain(i):
        return eng.get_text(pages[i])

    quiet_clean, quiet_plain = [clean(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        out, mask, info = R.rank(damaged[i], **params[i])
        assert quiet_clean[i] == (out.tobytes(), mask.tobytes(), tuple(sorted(info.items())))
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, clean(i) if t < 4 else plain(i))
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
        assert got == (quiet_clean[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)
