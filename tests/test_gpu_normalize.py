"""Page normalisation on the GPU, bit for bit against tests/normalize_ref.py.

Pages are put on the device with input_from_grey; results are compared as 32-bit words, NaN positions equal (a NaN
compares as NaN, not by payload, except where the result is defined as the page's own words); what the passes counted
(ocrs_normalize_info) is compared as integers.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import models_util as M
import normalize_ref as N
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, output, synth
from oracle import pipeline as OP
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden", "reference")
PAGES = ("polar-bears", "why-rust", "rust-book")
DARK = {"polar-bears": 0, "why-rust": 1, "rust-book": 0}
ONE_FILE_INK = (0.3, 1.0, 1)
# (height, width): one pixel, one row, one column; around one tile of 64 either way; several tiles with partial edges; every
# width % 4 (the 16-byte path needs % 4 == 0)
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (65, 63), (127, 129), (97, 211), (70, 256), (70, 257), (70, 258), (70, 259)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    return OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(M.recognition_model_bytes()))


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


def noise(seed, h, w, plant=False, spread=1.0):
    """[h, w] float32, uniform in [-0.5, 0.5) * spread; plant: see planted()."""
    rng = np.random.default_rng(seed)
    a = ((rng.random((h, w), dtype=np.float32) - np.float32(0.5)) * np.float32(spread)).astype(np.float32)
    return planted(a, seed) if plant else a


def text_like(seed, h, w):
    """Paper with a tenth of ink under a light that falls off to the left: decidedly a light page."""
    rng = np.random.default_rng(seed)
    g = np.where(rng.random((h, w)) < 0.1, 0.2, 0.85) + 0.1 * (rng.random((h, w)) - 0.5)
    return (g * (0.6 + 0.4 * np.arange(w) / w)[None, :] - 0.5).astype(np.float32)


def assert_same_words(got, exp, what):
    assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.shape, exp.shape)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ at %s" % (what, np.argwhere(np.isnan(got) != nan)[:4].tolist())
    bad = np.argwhere((got.view(np.uint32) != exp.view(np.uint32)) & ~nan)
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r (%#x), expected %r (%#x)"
                             % (what, len(bad), got.size, at, got[at], got.view(np.uint32)[at], exp[at], exp.view(np.uint32)[at]))


def check(eng, page, what, **params):
    """normalize(page) on the device against the restatement: the page's bits and what was counted."""
    out, info = eng.normalize(eng.input_from_grey(page), info=True, **params)
    exp, exp_info = N.normalize(page, **params)
    assert out.shape == (1,) + page.shape
    assert info == exp_info, (what, params, info, exp_info)
    assert_same_words(image_of(out), exp, "%s %s" % (what, params))
    return image_of(out), info


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("tile", [16, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_equal_the_restatement(eng, shape, tile):
    h, w = shape
    check(eng, noise(h * 1000 + w, h, w), "noise", tile=tile)
    check(eng, noise(h * 1000 + w + 1, h, w, plant=True, spread=1.25), "planted", tile=tile)


@pytest.mark.parametrize("tile", [16, 64])
def test_a_page_of_a_million_pixels(eng, tile):
    page = noise(7, 1024, 1024)
    page[:, :512] = text_like(7, 1024, 512)    # a page on the left, noise on the right
    page = planted(page, 7)
    _, info = check(eng, page, "1024 x 1024", tile=tile)
    assert info["counted"] == 1024 * 1024 - 3


def test_a_page_smaller_than_its_tile(eng):
    check(eng, noise(3, 16, 16, plant=True), "16 x 16", tile=256)
    check(eng, noise(4, 16, 16), "16 x 16", tile=256, polarity="invert")


def test_planted_values_keep_their_place(eng):
    page = noise(11, 40, 52, plant=True, spread=1.5)
    nan = np.isnan(page)
    assert nan.sum() == 3 and np.isinf(page).sum() == 2
    for pol in ("keep", "invert"):
        out, info = check(eng, page, "planted", polarity=pol)
        keep = ~nan
        assert info["counted"] == keep.sum() and np.all(out[keep] >= np.float32(-0.5)) and np.all(out[keep] <= np.float32(0.5))
    out, _ = check(eng, page, "planted", polarity="keep", levels=False, flatten=False)
    assert out.view(np.uint32).tobytes() == page.view(np.uint32).tobytes(), "neither: a bit copy, NaN payloads included"
    out, _ = check(eng, page, "planted", polarity="invert", levels=False, flatten=False)
    assert out.view(np.uint32).tobytes() == (page.view(np.uint32) ^ np.uint32(0x80000000)).tobytes()


@pytest.mark.parametrize("shape", [(200, 300), (201, 301), (64, 1024)], ids=lambda s: "%dx%d" % s)
def test_one_bin_dominated_pages_count_exactly(eng, shape):
    """97 % of the page is one value: nearly every add of a tile goes to one bin, merged lanes and all."""
    h, w = shape
    rng = np.random.default_rng(h)
    page = np.full(shape, 0.4, np.float32)
    ink = rng.random(shape) < 0.03
    page[ink] = (rng.random(int(ink.sum()), dtype=np.float32) * np.float32(0.3) - np.float32(0.45)).astype(np.float32)
    for tile in (16, 64, 256):
        for pol in ("auto", "invert"):
            _, info = check(eng, page, "paper", tile=tile, polarity=pol)
            assert info["counted"] == h * w
    blank = np.full(shape, 0.4, np.float32)
    _, info = check(eng, blank, "blank")
    assert info["hi"] <= info["lo"] and info["counted"] == h * w
    _, info = check(eng, np.full(shape, np.nan, np.float32), "all NaN")
    assert info == {"dark": 0, "vote": 0, "white": -1, "lo": -1, "hi": -1, "counted": 0}
    for c in (-0.5, 0.0, 0.25, 0.5):
        check(eng, np.full((70, 130), c, np.float32), "constant %g" % c)


def test_switches(eng):
    for seed, shape in enumerate(((97, 211), (128, 256))):
        page = text_like(20 + seed, *shape)
        assert N.normalize(page, tile=32)[1]["dark"] == 0
        outs = set()
        for pol in N.POLARITIES:
            for flatten in (True, False):
                for levels in (True, False):
                    out, info = check(eng, page, "switches", tile=32, polarity=pol, flatten=flatten, levels=levels)
                    outs.add(out.tobytes())
                    assert (info["lo"], info["hi"]) == (-1, -1) or levels
        assert len(outs) == 8   # auto decides light here, as keep does: 2 polarities x 4 switch settings
        assert check(eng, page, "keep", polarity="keep", flatten=False, levels=False)[0].tobytes() == page.tobytes()


MIXED = [((97, 211), {"tile": 16}), ((128, 256), {"tile": 64, "polarity": "invert"}), ((1, 300), {"tile": 32, "levels": False}),
         ((70, 258), {"tile": 256, "flatten": False}), ((65, 63), {"flatten": False, "levels": False, "polarity": "invert"}),
         ((260, 130), None)]


def test_mixed_batch_equals_each_page_alone_twenty_times(eng):
    srcs = [noise(40 + i, *s, plant=i % 2 == 0) for i, (s, _) in enumerate(MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in MIXED]
    exp = [N.normalize(s, **(p or {})) for s, p in zip(srcs, params)]
    first = None
    for rep in range(20):
        pages, infos = eng.normalize_batch(inputs, params, info=True)
        got = [image_of(p) for p in pages]
        if first is None:
            first = got
            for i, (g, info) in enumerate(zip(got, infos)):
                assert info == exp[i][1], (i, info, exp[i][1])
                assert_same_words(g, exp[i][0], "batch page %d" % i)
                alone, alone_info = eng.normalize(inputs[i], info=True, **(params[i] or {}))
                assert alone_info == info and image_of(alone).tobytes() == g.tobytes(), "page %d alone" % i
        else:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first)), "repeat %d" % rep
    assert [image_of(p).tobytes() for p in eng.normalize_batch(inputs[:2], {"tile": 32})] == \
        [image_of(eng.normalize(i, tile=32)).tobytes() for i in inputs[:2]], "one parameter set for all"
    assert eng.normalize_batch([], None) == [] and eng.normalize_batch([], None, info=True) == ([], [])
    with pytest.raises(ValueError):
        eng.normalize_batch(inputs, params[:2])


# a page boundary inside, on and just past a 64-tile edge; 64 x 64 takes the 16-byte accesses, 130 x 7 cannot
EDGE_MIXED = [((1, 1), {"tile": 16}), ((63, 65), {"tile": 64}), ((64, 64), {"tile": 16}), ((65, 63), {"tile": 64}), ((130, 7), {"tile": 16})]


def test_edge_sized_batch_equals_each_page_alone(eng):
    srcs = [noise(60 + i, *s, plant=i % 2 == 1) for i, (s, _) in enumerate(EDGE_MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in EDGE_MIXED]
    pages, infos = eng.normalize_batch(inputs, params, info=True)
    for i, (src, inp, p, out, info) in enumerate(zip(srcs, inputs, params, pages, infos)):
        alone, alone_info = eng.normalize(inp, info=True, **p)
        assert alone_info == info and image_of(alone).tobytes() == image_of(out).tobytes(), "page %d alone" % i
        exp, exp_info = N.normalize(src, **p)
        assert info == exp_info, (i, info, exp_info)
        assert_same_words(image_of(out), exp, "batch page %d" % i)


def test_a_bad_page_in_the_middle_returns_nothing_and_leaks_nothing(eng):
    inputs = [eng.input_from_grey(noise(80 + i, 40, 50)) for i in range(3)]
    pages = (C.c_void_p * 3)(*[i._h for i in inputs])
    ps = (_lib.NormalizeParams * 3)(_lib.NormalizeParams(64, 0, 1, 1), _lib.NormalizeParams(48, 0, 1, 1), _lib.NormalizeParams(64, 0, 1, 1))
    out = (C.c_void_p * 3)()
    live = _lib.pool_stats()["device_live"]
    assert _lib.lib().ocrs_engine_normalize_pages(eng._h, pages, C.c_size_t(3), ps, out, None) == 1, "INVALID_ARGUMENT"
    assert [out[i] for i in range(3)] == [None] * 3, "a failed call writes no page"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    with pytest.raises(_lib.OcrsError) as e:
        eng.normalize_batch(inputs, [None, {"tile": 48}, None])
    assert e.value.status_name == "INVALID_ARGUMENT", e.value
    assert _lib.pool_stats()["device_live"] == live


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = noise(99, 131, 70)
    inp = eng.input_from_grey(src)
    exp = N.normalize(src)[0]
    out = eng.normalize(inp)
    assert image_of(inp).tobytes() == src.tobytes()
    del out   # ocrs_page_free of the result: the source is a page of its own
    assert image_of(inp).tobytes() == src.tobytes()
    out = eng.normalize(inp)
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == exp.tobytes()
    again = eng.normalize(out, polarity="keep", flatten=False, levels=False)   # a normalised page is an ordinary page
    assert image_of(again).tobytes() == exp.tobytes()


def test_bad_parameters_have_their_status(eng):
    inp = eng.input_from_grey(noise(1, 20, 20))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    for tile in (0, 8, 15, 48, 65, 512, -64):
        refused(lambda: eng.normalize(inp, tile=tile))
    refused(lambda: eng.normalize_batch([inp, inp], [None, {"tile": 48}]))   # one bad page refuses the call
    out = C.c_void_p()
    bad = _lib.NormalizeParams(64, 7, 1, 1)
    assert _lib.lib().ocrs_engine_normalize_page(eng._h, inp._h, C.byref(bad), C.byref(out), None) == 1, "an unknown polarity"
    assert _lib.lib().ocrs_engine_normalize_page(eng._h, inp._h, None, None, None) == 1
    assert _lib.lib().ocrs_engine_normalize_page(eng._h, inp._h, None, C.byref(out), None) == 0, "NULL: the default"
    from ocrs_amd import OcrInput
    assert image_of(OcrInput(out)).tobytes() == image_of(eng.normalize(inp)).tobytes()   # (the OcrInput frees the page)
    with pytest.raises(ValueError):
        eng.normalize(inp, polarity="negative")
    wide = eng.input_from_grey(np.zeros((1, 65536), np.float32))
    refused(lambda: eng.normalize(wide))
    assert eng.normalize(eng.input_from_grey(np.zeros((1, 65535), np.float32))).shape == (1, 1, 65535)


# ------------------------------------------------------------------ 2. the three real pages, one detection file
class RealPages:
    def __init__(self):
        dbuf, rbuf = M.detection_model_bytes(ink=ONE_FILE_INK), M.recognition_model_bytes()
        self.eng = OcrEngine(detection_model=Model.load_bytes(dbuf), recognition_model=Model.load_bytes(rbuf))
        self.ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(dbuf), "exact"), recognition_model=OracleModel(OracleGraph(rbuf), "exact"))
        self.page, self.words = {}, {}
        for name in PAGES:
            z = np.load(os.path.join(G, name + ".npz"))
            inp = self.ora.prepare_input(OP.ImageSource.from_tensor(z["pixels"], "hwc"))
            self.page[name] = np.ascontiguousarray(np.asarray(inp, np.float32)[0])
            self.words[name] = len(z["word_rects"])


@pytest.fixture(scope="module")
def real():
    return RealPages()


@pytest.mark.parametrize("name", PAGES)
def test_real_pages_and_their_shaded_twins_equal_the_restatement(real, name):
    eng, page = real.eng, real.page[name]
    out, info = check(eng, page, name)
    _, shaded_info = check(eng, N.shade(page), name + " shaded")
    print(name, info, "shaded:", shaded_info)
    assert info["dark"] == shaded_info["dark"] == DARK[name]
    # one operating point: the engine's words on the normalised page are the oracle's on the restatement's page
    words = eng.detect_words(eng.normalize(eng.input_from_grey(page)))
    exp = np.array([w.to_array() for w in real.ora.detect_words(N.normalize(page)[0][None])], np.float32).reshape(-1, 6)
    print("%s: %d words on the normalised page, %d in the fixture of its own hand-tuned file" % (name, len(words), real.words[name]))
    assert words.shape == exp.shape and words.tobytes() == exp.tobytes()
    assert 2 * len(words) >= real.words[name]
    if name == "why-rust":
        raw = eng.detect_words(eng.input_from_grey(page))
        print("why-rust as given: %d words" % len(raw))
        assert len(raw) <= 5


# ------------------------------------------------------------------ 3. composition
def dark_mode_page(seed, h, w, lines):
    """A synthetic page as a dark-mode screenshot with a shadow across it: what the plain pipeline reads nothing on."""
    px = synth.synthetic_page(seed, h, w, lines=lines, columns=1)
    ramp = (0.55 + 0.45 * np.arange(w, dtype=np.float64) / w)[None, :, None]
    return np.ascontiguousarray(((255 - px.astype(np.float64)) * ramp).astype(np.uint8))


def test_get_text_with_normalize_is_the_manual_chain(eng):
    px = dark_mode_page(5, 600, 500, 24)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    grey = image_of(inp)
    for params in (True, {"tile": 32, "polarity": "invert"}):
        kw = {} if params is True else params
        page = eng.normalize(inp, **kw)
        assert_same_words(image_of(page), N.normalize(grey, **kw)[0], "the prepared page")
        lines = eng.find_text_lines(page, eng.detect_words(page))
        text = "\n".join(str(t) for t in eng.recognize_text(page, lines) if t is not None)
        print("%d lines on the normalised page, %d on the page as given" % (len(lines), len(eng.find_text_lines(inp, eng.detect_words(inp)))))
        assert len(lines) > 0 and eng.get_text(inp, normalize=params) == text
        assert eng.get_text(inp, normalize=params, rectify=True) == eng.get_text(page, rectify=True)
        assert eng.get_text(inp, normalize=params, orientation=2, work_size=(300, 250)) == eng.get_text(page, orientation=2, work_size=(300, 250))
    assert eng.get_text(inp, normalize=None) == eng.get_text(inp) == eng.get_text(inp, normalize=False)


def test_cli_normalize(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    px = dark_mode_page(9, 900, 700, 40)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("norm", "tile", "plain")}
    assert cli.main([path, "--normalize", "-j", "--text-map", "-o", files["norm"]]) == 0
    assert cli.main([path, "--normalize", "--normalize-tile", "32", "--normalize-polarity", "invert", "-j", "-o", files["tile"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in (["--normalize-tile", "32"], ["--normalize-polarity", "keep"], ["--normalize", "--normalize-polarity", "dark"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def document(**kw):
        page, info = eng.normalize(inp, info=True, **kw)
        lines = eng.find_text_lines(page, eng.detect_words(page))
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(page, lines), normalize=info), info

    plain = output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "normalize" not in json.loads(plain), "without the flag nothing changes"
    exp, info = document()
    assert text["norm"] == exp and info["dark"] == 1
    assert json.loads(text["norm"])["normalize"] == info and set(info) == {"counted", "dark", "hi", "lo", "vote", "white"}
    assert text["tile"] == document(tile=32, polarity="invert")[0]
    assert len(json.loads(text["norm"])["paragraphs"][0]["lines"]) > len(json.loads(plain)["paragraphs"][0]["lines"])
    # --text-map with --normalize: the map of the normalised page
    want = eng.detect_text_pixels(eng.normalize(inp))
    want = (np.clip(want, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "text-map.png"))), want)


# ------------------------------------------------------------------ 4. beside other callers
def test_normalising_callers_beside_plain_callers(eng):
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                       recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    params = [{"tile": 16}, {"tile": 64, "polarity": "invert"}, {"tile": 32, "levels": False}, {"tile": 128}]

    def normalised(i):
        page, info = eng.normalize(pages[i], info=True, **params[i])
        return image_of(page).tobytes(), tuple(sorted(info.items()))

    def plain(i):
        return eng.detect_words(pages[i]).tobytes()

    quiet_norm, quiet_plain = [normalised(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        exp, exp_info = N.normalize(image_of(pages[i]), **params[i])
        assert quiet_norm[i] == (exp.tobytes(), tuple(sorted(exp_info.items())))
        words = ora.detect_words(ora.prepare_input(OP.ImageSource.from_tensor(pxs[i], "hwc")))
        assert len(words) > 5 and quiet_plain[i] == np.array([w.to_array() for w in words], np.float32).tobytes()
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, normalised(i) if t < 4 else plain(i))
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
        assert got == (quiet_norm[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)
