"""Despeckling on the GPU, bit for bit against tests/despeckle_ref.py.

Pages are put on the device with input_from_grey; results are compared as 32-bit words (every pixel outside speck and hole
is the page's own word, NaN payloads included, so the words are compared as they are); the mask and what the passes
counted (ocrs_speckle_info) are compared as integers.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import despeckle_pages as P
import despeckle_ref as D
import models_util as M
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, OcrInput, _lib, output, synth
from oracle import pipeline as OP
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu
# (height, width): one pixel, one row, one column; around one word and one 64 x 64 tile either way; several tiles with
# partial edges; every width % 4 (the 16-byte path needs % 4 == 0)
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (65, 63), (127, 129), (129, 127), (97, 211), (70, 256), (70, 257), (70, 258),
          (70, 259)]
# at 0.5 the 8-connected ink percolates and the 4-connected paper shatters; at 0.05 and 0.95 one class is dust in the other
DENSITIES = (0.05, 0.3, 0.5, 0.7, 0.95)
SWEEP = [{"max_area": A, "max_hole": Hm, "keep_near": K} for A, Hm, K in itertools.product((0, 1, 2, 5), (0, 1, 3), (0, 1, 3))]


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


def check_batch(eng, pages, params, what):
    """One call for all the pages against the restatement of each -> the restatement's results.  Pages that are the same
    array share one labelling of the restatement."""
    made, masks, infos = eng.despeckle_batch([eng.input_from_grey(p) for p in pages], params, mask=True, info=True)
    exps, analyses = [], {}
    for i, (page, p) in enumerate(zip(pages, params)):
        key = (id(page), (p or {}).get("threshold", 0.0))
        if key not in analyses:
            analyses[key] = D.analyse(page, key[1])
        exps.append(D.despeckle(page, analysis=analyses[key], **(p or {})))
        assert made[i].shape == (1,) + page.shape
        assert_same((image_of(made[i]), masks[i], infos[i]), exps[-1], "%s, page %d %s" % (what, i, p))
    return exps


def check(eng, page, what, **params):
    return check_batch(eng, [page], [params], what)[0]


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_noise_at_every_density_and_small_parameter_equals_the_restatement(eng, shape):
    h, w = shape
    pages = [noise(h * 1000 + w + 7 * i, h, w, plant=plant, ink=ink) for i, (ink, plant) in enumerate(itertools.product(DENSITIES, (False, True)))]
    exps = check_batch(eng, [p for p in pages for _ in SWEEP], SWEEP * len(pages), "noise %dx%d" % shape)
    most = {k: max(e[2][k] for e in exps) for k in ("specks", "holes", "kept")}
    print(shape, most)
    if h >= 63 and w >= 63:   # removed specks, filled holes and kept candidates all occur
        assert all(v > 0 for v in most.values()), most


def test_every_planted_pattern_equals_the_restatement(eng):
    pats = P.patterns(129, 127)
    pages, params, names = [], [], []
    for name, page, sets in pats:
        for kw in sets:
            pages.append(page)
            params.append(kw)
            names.append(name)
    exps = check_batch(eng, pages, params, "patterns")
    found = {n: e[2] for n, e in zip(names, exps)}
    assert found["checkerboard"]["holes"] > 8000 and found["serpentine"]["ink"] > 8000 and found["spiral of paper"]["counted"] > 4000


@pytest.mark.parametrize("ink", [0.97, 0.03])
def test_the_largest_parameters(eng, ink):
    pages = [noise(77, 97, 211, plant=True, ink=ink), noise(78, 129, 127, ink=ink)]
    sets = [{"max_area": 4096, "max_hole": 4096, "keep_near": K} for K in (0, 16)] + [{"max_area": 4096}, {"max_hole": 4096, "max_area": 0}]
    exps = check_batch(eng, [p for p in pages for _ in sets], sets * 2, "largest parameters at %g ink" % ink)
    assert max(e[2]["hole_pixels" if ink > 0.5 else "speck_pixels"] for e in exps) > 100


@pytest.fixture(scope="module")
def text_page(ora):
    """The 512 x 512 page of DESIGN.md §7.9, clean and with 0.2 % of pepper and of salt."""
    px = synth.synthetic_page(3, 512, 512, 30, 2, 1)
    clean = np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), np.float32)[0])
    return clean, D.add_noise(clean, 0.002)[0]


def test_a_noisy_text_page(eng, text_page):
    clean, noisy = text_page
    exps = check_batch(eng, [noisy, noisy, noisy, clean], [None, {"max_area": 9, "keep_near": 2}, {"max_hole": 2}, None], "512 x 512")
    assert exps[0][2]["specks"] > 300 and exps[1][2]["kept"] > 0 and exps[2][2]["hole_pixels"] == 384 and exps[3][2]["specks"] == 0
    assert exps[3][0].tobytes() == clean.tobytes()


def test_the_longest_row(eng):
    row = np.full((1, 65535), 0.25, np.float32)
    row[0, 40000:40003] = row[0, 63] = row[0, 64] = row[0, 65534] = -0.25
    row[0, 100:5000] = -0.25
    row[0, 2000] = 0.25
    exp = check(eng, row, "1 x 65535", max_area=2, max_hole=1)
    assert exp[2]["specks"] == 2 and exp[2]["speck_pixels"] == 3 and exp[2]["holes"] == 1


def test_degenerate_pages(eng):
    for shape in ((70, 130), (5, 200)):
        n = shape[0] * shape[1]
        for kw in ({}, {"max_area": 4096, "max_hole": 4096, "keep_near": 16}):
            exp = check(eng, np.full(shape, 0.4, np.float32), "blank", **kw)
            assert exp[2]["ink"] == 0 and exp[2]["counted"] == n and exp[2]["ink_bin"] == 0 and exp[2]["holes"] == (1 if kw and n <= 4096 else 0)
            exp = check(eng, np.full(shape, -0.5, np.float32), "all ink", **kw)
            assert exp[2]["ink"] == n and exp[2]["counted"] == 0 and exp[2]["paper_bin"] == 255 and exp[2]["specks"] == (1 if kw and n <= 4096 else 0)
            exp = check(eng, np.full(shape, np.nan, np.float32), "all NaN", **kw)
            assert exp[2]["ink"] == 0 and exp[2]["counted"] == 0 and (exp[2]["paper_bin"], exp[2]["ink_bin"]) == (255, 0)
        for c in (0.0, 0.5):
            check(eng, np.full(shape, c, np.float32), "constant %g" % c)


def test_fills_given_and_threshold(eng):
    page = planted(noise(12, 97, 211, ink=0.3) * np.float32(0.5), 12)
    for kw in ({"paper": 0.25}, {"ink_level": -0.0}, {"paper": -0.125, "ink_level": 0.125}, {"threshold": -0.05}, {"threshold": 0.1, "paper": 0.125}):
        exp = check(eng, page, "fills / threshold", max_area=3, max_hole=3, **kw)
        assert (exp[2]["paper_bin"] == -1) == ("paper" in kw) and (exp[2]["ink_bin"] == -1) == ("ink_level" in kw)
        assert exp[2]["specks"] > 0 and exp[2]["holes"] > 0


MIXED = [((97, 211), {"max_area": 3, "max_hole": 2}), ((128, 256), {"max_area": 5, "keep_near": 2, "paper": 0.25}),
         ((1, 300), {"max_area": 1, "max_hole": 1}), ((70, 258), {"max_area": 4096, "max_hole": 4096, "keep_near": 16, "threshold": 0.1}),
         ((65, 63), {"max_area": 2, "keep_near": 1, "threshold": -0.2, "ink_level": -0.25}), ((260, 130), None)]


def test_mixed_batch_equals_each_page_alone_twenty_times(eng):
    srcs = [noise(40 + i, *s, plant=i % 2 == 0, ink=0.3) for i, (s, _) in enumerate(MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in MIXED]
    exp = [D.despeckle(s, **(p or {})) for s, p in zip(srcs, params)]
    first = None
    for rep in range(20):
        pages, masks, infos = eng.despeckle_batch(inputs, params, mask=True, info=True)
        got = [(image_of(p), m, i) for p, m, i in zip(pages, masks, infos)]
        if first is None:
            first = got
            for i, g in enumerate(got):
                assert_same(g, exp[i], "batch page %d" % i)
                alone = eng.despeckle(inputs[i], mask=True, info=True, **(params[i] or {}))
                assert alone[2] == g[2] and image_of(alone[0]).tobytes() == g[0].tobytes() and alone[1].tobytes() == g[1].tobytes(), "page %d alone" % i
        else:
            assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(got, first)), "repeat %d" % rep
    assert [image_of(p).tobytes() for p in eng.despeckle_batch(inputs[:2], {"max_area": 2})] == \
        [image_of(eng.despeckle(i, max_area=2)).tobytes() for i in inputs[:2]], "one parameter set for all"
    assert eng.despeckle_batch([], None) == [] and eng.despeckle_batch([], None, mask=True, info=True) == ([], [], [])
    with pytest.raises(ValueError):
        eng.despeckle_batch(inputs, params[:2])


def test_mask_alone_info_alone_and_neither(eng):
    src = noise(21, 70, 130, ink=0.3)
    inp = eng.input_from_grey(src)
    kw = {"max_area": 3, "max_hole": 1, "keep_near": 1}
    exp = D.despeckle(src, **kw)
    page = eng.despeckle(inp, **kw)
    assert isinstance(page, OcrInput) and image_of(page).tobytes() == exp[0].tobytes()
    page, mask = eng.despeckle(inp, mask=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and mask.tobytes() == exp[1].tobytes()
    page, info = eng.despeckle(inp, info=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and info == exp[2] and tuple(info) == D.INFO_KEYS
    src4 = noise(22, 70, 132, ink=0.3)   # the 16-byte path without a byte mask
    assert image_of(eng.despeckle(eng.input_from_grey(src4), **kw)).tobytes() == D.despeckle(src4, **kw)[0].tobytes()


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = noise(99, 131, 70, ink=0.3)
    inp = eng.input_from_grey(src)
    exp = D.despeckle(src, max_area=3)[0]
    out = eng.despeckle(inp, max_area=3)
    assert image_of(inp).tobytes() == src.tobytes()
    del out   # ocrs_page_free of the result: the source is a page of its own
    assert image_of(inp).tobytes() == src.tobytes()
    out = eng.despeckle(inp, max_area=3)
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == exp.tobytes()
    again = eng.despeckle(out, max_area=6, max_hole=2)   # a cleaned page is an ordinary page
    assert image_of(again).tobytes() == D.despeckle(exp, max_area=6, max_hole=2)[0].tobytes()


def test_bad_parameters_have_their_status(eng):
    inp = eng.input_from_grey(noise(1, 20, 20))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    for kw in ({"max_area": -1}, {"max_area": 4097}, {"max_hole": -1}, {"max_hole": 4097}, {"keep_near": -1}, {"keep_near": 17},
               {"threshold": float("nan")}, {"threshold": float("inf")}, {"threshold": float("-inf")}, {"paper": float("inf")},
               {"paper": float("-inf")}, {"ink_level": float("inf")}, {"ink_level": float("-inf")}):
        refused(lambda: eng.despeckle(inp, **kw))
    refused(lambda: eng.despeckle_batch([inp, inp], [None, {"keep_near": 17}]))   # one bad page refuses the call
    live = _lib.pool_stats()["device_live"]
    pages = (C.c_void_p * 2)(inp._h, inp._h)
    nan = float("nan")
    ps = (_lib.SpeckleParams * 2)(_lib.SpeckleParams(0.0, 4, 0, 0, nan, nan), _lib.SpeckleParams(0.0, 4, 4097, 0, nan, nan))
    out = (C.c_void_p * 2)()
    masks = (C.POINTER(C.c_uint8) * 2)()
    assert _lib.lib().ocrs_engine_despeckle_pages(eng._h, pages, C.c_size_t(2), ps, out, masks, None) == 1, "INVALID_ARGUMENT"
    assert [out[i] for i in range(2)] == [None, None] and not masks[0] and not masks[1], "a failed call writes nothing"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    one = C.c_void_p()
    assert _lib.lib().ocrs_engine_despeckle_page(eng._h, inp._h, None, None, None, None) == 1
    assert _lib.lib().ocrs_engine_despeckle_page(eng._h, inp._h, None, C.byref(one), None, None) == 0, "NULL: the default"
    assert image_of(OcrInput(one)).tobytes() == image_of(eng.despeckle(inp)).tobytes()   # (the OcrInput frees the page)
    wide = eng.input_from_grey(np.zeros((1, 65536), np.float32))
    refused(lambda: eng.despeckle(wide))
    copy = eng.despeckle(inp, max_area=0, max_hole=0)   # valid: a copy
    assert image_of(copy).tobytes() == image_of(inp).tobytes()


# ------------------------------------------------------------------ 2. composition
def test_words_on_the_cleaned_page_are_the_oracles(eng, ora, text_page):
    _, noisy = text_page
    exp = D.despeckle(noisy)
    words = eng.detect_words(eng.despeckle(eng.input_from_grey(noisy)))
    want = np.array([w.to_array() for w in ora.detect_words(exp[0][None])], np.float32).reshape(-1, 6)
    assert len(want) > 100 and words.shape == want.shape and words.tobytes() == want.tobytes()


def noisy_picture(seed, h, w, lines):
    """A synthetic page with pepper on 0.3 % of its pixels, and a table grid for the rule removal, as a picture."""
    px = synth.synthetic_page(seed, h, w, lines=lines, columns=1)
    px[np.random.default_rng(seed).random((h, w)) < 0.003] = 0
    for r in range(20, h - 2, 90):
        px[r:r + 2, 10:w - 10] = 0
    return px


def test_get_text_with_despeckle_is_the_manual_chain(eng):
    inp = eng.prepare_input(ImageSource.from_tensor(noisy_picture(5, 600, 500, 24), DimOrder.Hwc))
    for params in (True, {"max_area": 6, "keep_near": 2}):
        kw = {} if params is True else params
        page, info = eng.despeckle(inp, info=True, **kw)
        assert info["specks"] > 100
        assert image_of(page).tobytes() == D.despeckle(image_of(inp), **kw)[0].tobytes()
        lines = eng.find_text_lines(page, eng.detect_words(page))
        text = "\n".join(str(t) for t in eng.recognize_text(page, lines) if t is not None)
        assert len(lines) > 0 and eng.get_text(inp, despeckle=params) == text
        assert eng.get_text(inp, despeckle=params, rectify=True) == eng.get_text(page, rectify=True)
        norm = eng.despeckle(eng.normalize(inp), **kw)   # after normalisation ...
        assert eng.get_text(inp, despeckle=params, normalize=True) == eng.get_text(norm)
        upright = eng.deskew(norm, 1.5)[0]               # ... before deskew ...
        assert eng.get_text(inp, despeckle=params, normalize=True, deskew=1.5) == eng.get_text(upright)
        assert eng.get_text(inp, despeckle=params, normalize=True, deskew=1.5, rules=True) == eng.get_text(eng.remove_rules(upright))
        assert eng.get_text(inp, despeckle=params, rules={"min_length": 200}) == eng.get_text(eng.remove_rules(page, min_length=200))   # ... and rules
    assert eng.get_text(inp, despeckle=None) == eng.get_text(inp) == eng.get_text(inp, despeckle=False)


def test_cli_despeckle(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    px = noisy_picture(9, 700, 600, 30)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("clean", "tuned", "plain")}
    assert cli.main([path, "--despeckle", "-j", "--debug", "-o", files["clean"]]) == 0
    assert cli.main([path, "--despeckle", "--speck-max-area", "9", "--speck-fill-holes", "1", "--speck-keep-near", "2", "-j", "-o", files["tuned"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in (["--speck-max-area", "9"], ["--speck-fill-holes", "1"], ["--speck-keep-near", "1"], ["--despeckle", "--speck-keep-near", "17"],
                ["--despeckle", "--speck-max-area", "4097"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def document(**kw):
        page, info = eng.despeckle(inp, info=True, **kw)
        lines = eng.find_text_lines(page, eng.detect_words(page))
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(page, lines), despeckle=info), info

    plain = output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "despeckle" not in json.loads(plain), "without the flag nothing changes"
    exp, info = document()
    assert text["clean"] == exp and info["specks"] > 100
    assert json.loads(text["clean"])["despeckle"] == info and set(info) == set(D.INFO_KEYS)
    assert text["tuned"] == document(max_area=9, max_hole=1, keep_near=2)[0]


# ------------------------------------------------------------------ 3. beside other callers
def test_despeckling_callers_beside_plain_callers(eng, ora):
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    noisy = [eng.input_from_grey(D.add_noise(image_of(p), 0.004, seed=i)[0]) for i, p in enumerate(pages)]
    params = [{}, {"max_area": 9, "keep_near": 2}, {"max_hole": 2}, {"max_area": 6, "max_hole": 1, "keep_near": 16, "paper": 0.25}]

    def cleaned(i):
        page, mask, info = eng.despeckle(noisy[i], mask=True, info=True, **params[i])
        return image_of(page).tobytes(), mask.tobytes(), tuple(sorted(info.items()))

    def plain(i):
        return eng.detect_words(pages[i]).tobytes()

    quiet_clean, quiet_plain = [cleaned(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        out, mask, info = D.despeckle(image_of(noisy[i]), **params[i])
        assert quiet_clean[i] == (out.tobytes(), mask.tobytes(), tuple(sorted(info.items())))
        words = ora.detect_words(ora.prepare_input(OP.ImageSource.from_tensor(pxs[i], "hwc")))
        assert len(words) > 5 and quiet_plain[i] == np.array([w.to_array() for w in words], np.float32).tobytes()
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, cleaned(i) if t < 4 else plain(i))
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
