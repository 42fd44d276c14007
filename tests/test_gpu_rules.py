"""Ruled-line removal on the GPU, bit for bit against tests/rules_ref.py.

Pages are put on the device with input_from_grey; results are compared as 32-bit words (every pixel outside D is the
page's own word, NaN payloads included, so the words are compared as they are); the mask and what the passes counted
(ocrs_rules_info) are compared as integers.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import models_util as M
import rules_ref as R
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, OcrInput, _lib, output, synth
from oracle import pipeline as OP
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu
# (height, width): one pixel, one row, one column; around one word and one 64 x 64 transpose block either way; several blocks
# with partial edges; every width % 4 (the 16-byte path needs % 4 == 0)
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (65, 63), (127, 129), (129, 127), (97, 211), (70, 256), (70, 257), (70, 258),
          (70, 259)]
# uniform noise has no long runs: short rules, thin blocks, narrow margins, where every set of the definition is non-empty
NOISE_PARAMS = [{"min_length": L, "max_thickness": T, "margin": m} for L, T, m in itertools.product((2, 3, 5, 8), (1, 2, 3), (0, 1, 2))]
# nearly all ink: runs that span two and three words
DENSE_PARAMS = [{"min_length": L, "max_thickness": T, "margin": 1} for L, T in itertools.product((64, 65, 130), (2, 64))]


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
    """One call for all the pages against the restatement of each -> the restatement's results."""
    made, masks, infos = eng.remove_rules_batch([eng.input_from_grey(p) for p in pages], params, mask=True, info=True)
    exps = []
    for i, (page, p) in enumerate(zip(pages, params)):
        exps.append(R.remove_rules(page, **(p or {})))
        assert made[i].shape == (1,) + page.shape
        assert_same((image_of(made[i]), masks[i], infos[i]), exps[-1], "%s, page %d %s" % (what, i, p))
    return exps


def check(eng, page, what, **params):
    return check_batch(eng, [page], [params], what)[0]


def margin_count(exp):
    return int(((exp[1] & 4) != 0).sum())


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_noise_at_every_small_parameter_equals_the_restatement(eng, shape):
    h, w = shape
    pages = [noise(h * 1000 + w, h, w), noise(h * 1000 + w + 1, h, w, plant=True)]
    exps = check_batch(eng, [p for p in pages for _ in NOISE_PARAMS], NOISE_PARAMS * 2, "noise %dx%d" % shape)
    most = {k: max(e[2][k] for e in exps) for k in ("h_removed", "v_removed", "kept")}
    most["margin"] = max(margin_count(e) for e in exps)
    print(shape, most)
    if h >= 63 and w >= 63:   # every set of the definition is exercised
        assert all(v > 0 for v in most.values()), most
    elif h * w > 1:           # one row or one column: rules along it; a margin lies beside a rule and a crossing needs both sides
        assert most["h_removed" if h == 1 else "v_removed"] > 0 and most["margin"] == 0 and most["kept"] == 0, most


@pytest.mark.parametrize("shape", [(129, 127), (97, 211), (70, 256), (70, 257), (70, 258), (70, 259)], ids=lambda s: "%dx%d" % s)
def test_runs_over_two_and_three_words_equal_the_restatement(eng, shape):
    h, w = shape
    pages = [noise(h * 2000 + w, h, w, ink=0.97), noise(h * 2000 + w + 1, h, w, plant=True, ink=0.97)]
    exps = check_batch(eng, [p for p in pages for _ in DENSE_PARAMS], DENSE_PARAMS * 2, "dense %dx%d" % shape)
    assert max(e[2]["h_removed"] + e[2]["v_removed"] for e in exps) > 0 and max(e[2]["kept"] for e in exps) > 0


def test_extreme_parameters(eng):
    page = noise(5, 97, 211, plant=True, ink=0.9)
    for L in (8, 40):
        exp = check(eng, page, "T 64, M 8", min_length=L, max_thickness=64, margin=8)
        assert exp[2]["overwritten"] > 0 and margin_count(exp) > 0
    check(eng, page, "L 65535", min_length=65535)
    long = np.full((3, 4200), -0.3, np.float32)   # 66 words to a row: runs of 100, 4049 and 49, of 2050 and 2149, and paper
    long[0, 100] = long[0, 4150] = long[1, 2050] = 0.3
    long[2, :] = 0.3
    assert check(eng, long, "rows of more than 64 words", min_length=2000, max_thickness=2)[2]["h_removed"] == 4049 + 2050 + 2149
    assert check(eng, np.ascontiguousarray(long.T), "columns of more than 64 words", min_length=2000, max_thickness=2)[2]["v_removed"] == 8248
    assert check(eng, long, "rows of more than 64 words, too thick", min_length=2000, max_thickness=1)[2]["h_removed"] == 152


@pytest.fixture(scope="module")
def table(ora):
    """The 512 x 512 table page of DESIGN.md §7.8 and its 1024 x 1024 sibling with underlines: (clean, ruled, rule pixels)."""
    def make(seed, size, lines, underlines):
        px = synth.synthetic_page(seed, size, size, lines, 2, 1)
        clean = np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), np.float32)[0])
        return (clean,) + R.draw_grid(clean, underlines)
    return {512: make(3, 512, 30, ()), 1024: make(4, 1024, 60, [(r, 40, 40 + 300) for r in range(60, 1000, 97)])}


def test_a_page_of_a_million_pixels(eng, table):
    clean, ruled, rule = table[1024]
    exp = check(eng, planted(ruled.copy(), 3), "1024 x 1024")
    out, _, info = R.remove_rules(ruled)
    left, lost, word_ink = R.grid_counts(clean, rule, out)
    print("1024 x 1024: %s; rule ink left %d, word ink lost %d of %d" % (info, left, lost, word_ink))
    assert lost * 100 <= word_ink and exp[2]["h_removed"] > 0 and exp[2]["v_removed"] > 0 and exp[2]["kept"] > 0
    check(eng, clean, "1024 x 1024 without rules")


def test_degenerate_pages(eng):
    for shape in ((70, 130), (5, 200)):
        exp = check(eng, np.full(shape, 0.4, np.float32), "blank")
        assert exp[2]["overwritten"] == 0 and exp[2]["ink"] == 0 and exp[2]["counted"] == shape[0] * shape[1]
        for c in (-0.5, 0.0, 0.5):
            check(eng, np.full(shape, c, np.float32), "constant %g" % c)
        exp = check(eng, np.full(shape, -0.5, np.float32), "all ink")
        assert exp[2]["ink"] == shape[0] * shape[1] and exp[2]["counted"] == 0 and exp[2]["paper_bin"] == 255
        assert exp[2]["overwritten"] == (0 if shape[0] > 8 else shape[0] * shape[1]), "a block thicker than T is not a rule"
        exp = check(eng, np.full(shape, np.nan, np.float32), "all NaN")
        assert exp[2] == {"paper_bin": 255, "fill": 0.5, "ink": 0, "counted": 0, "h_removed": 0, "v_removed": 0, "overwritten": 0, "kept": 0}


def test_paper_given_and_threshold(eng):
    page = planted(noise(12, 97, 211) * np.float32(0.5), 12)
    for kw in ({"paper": 0.25}, {"paper": -0.0}, {"threshold": -0.1}, {"threshold": 0.2, "paper": 0.125}):
        exp = check(eng, page, "paper / threshold", min_length=3, max_thickness=2, **kw)
        assert exp[2]["paper_bin"] == (-1 if "paper" in kw else exp[2]["paper_bin"]) and exp[2]["overwritten"] > 0


MIXED = [((97, 211), {"min_length": 3, "max_thickness": 2}), ((128, 256), {"min_length": 5, "max_thickness": 1, "margin": 2, "paper": 0.25}),
         ((1, 300), {"min_length": 2, "margin": 0}), ((70, 258), {"min_length": 8, "max_thickness": 64, "margin": 8, "threshold": 0.1}),
         ((65, 63), {"min_length": 2, "max_thickness": 3, "threshold": -0.2}), ((260, 130), None)]


def test_mixed_batch_equals_each_page_alone_twenty_times(eng):
    srcs = [noise(40 + i, *s, plant=i % 2 == 0, ink=0.6) for i, (s, _) in enumerate(MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in MIXED]
    exp = [R.remove_rules(s, **(p or {})) for s, p in zip(srcs, params)]
    first = None
    for rep in range(20):
        pages, masks, infos = eng.remove_rules_batch(inputs, params, mask=True, info=True)
        got = [(image_of(p), m, i) for p, m, i in zip(pages, masks, infos)]
        if first is None:
            first = got
            for i, g in enumerate(got):
                assert_same(g, exp[i], "batch page %d" % i)
                alone = eng.remove_rules(inputs[i], mask=True, info=True, **(params[i] or {}))
                assert alone[2] == g[2] and image_of(alone[0]).tobytes() == g[0].tobytes() and alone[1].tobytes() == g[1].tobytes(), "page %d alone" % i
        else:
            assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(got, first)), "repeat %d" % rep
    assert [image_of(p).tobytes() for p in eng.remove_rules_batch(inputs[:2], {"min_length": 4})] == \
        [image_of(eng.remove_rules(i, min_length=4)).tobytes() for i in inputs[:2]], "one parameter set for all"
    assert eng.remove_rules_batch([], None) == [] and eng.remove_rules_batch([], None, mask=True, info=True) == ([], [], [])
    with pytest.raises(ValueError):
        eng.remove_rules_batch(inputs, params[:2])


def test_mask_alone_info_alone_and_neither(eng):
    src = noise(21, 70, 130, ink=0.6)
    inp = eng.input_from_grey(src)
    kw = {"min_length": 4, "max_thickness": 2}
    exp = R.remove_rules(src, **kw)
    page = eng.remove_rules(inp, **kw)
    assert isinstance(page, OcrInput) and image_of(page).tobytes() == exp[0].tobytes()
    page, mask = eng.remove_rules(inp, mask=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and mask.tobytes() == exp[1].tobytes()
    page, info = eng.remove_rules(inp, info=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and info == exp[2] and tuple(info) == R.INFO_KEYS


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = noise(99, 131, 70, ink=0.6)
    inp = eng.input_from_grey(src)
    exp = R.remove_rules(src, min_length=4)[0]
    out = eng.remove_rules(inp, min_length=4)
    assert image_of(inp).tobytes() == src.tobytes()
    del out   # ocrs_page_free of the result: the source is a page of its own
    assert image_of(inp).tobytes() == src.tobytes()
    out = eng.remove_rules(inp, min_length=4)
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == exp.tobytes()
    again = eng.remove_rules(out, min_length=4, max_thickness=64, margin=0)   # a cleaned page is an ordinary page
    assert image_of(again).tobytes() == R.remove_rules(exp, min_length=4, max_thickness=64, margin=0)[0].tobytes()


def test_bad_parameters_have_their_status(eng):
    inp = eng.input_from_grey(noise(1, 20, 20))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    for kw in ({"min_length": 1}, {"min_length": 0}, {"min_length": 65536}, {"min_length": -96}, {"max_thickness": 0}, {"max_thickness": 65},
               {"margin": -1}, {"margin": 9}, {"threshold": float("nan")}, {"threshold": float("inf")}, {"threshold": float("-inf")},
               {"paper": float("inf")}, {"paper": float("-inf")}):
        refused(lambda: eng.remove_rules(inp, **kw))
    refused(lambda: eng.remove_rules_batch([inp, inp], [None, {"margin": 9}]))   # one bad page refuses the call
    live = _lib.pool_stats()["device_live"]
    pages = (C.c_void_p * 2)(inp._h, inp._h)
    ps = (_lib.RulesParams * 2)(_lib.RulesParams(0.0, 96, 8, 1, float("nan")), _lib.RulesParams(0.0, 96, 65, 1, float("nan")))
    out = (C.c_void_p * 2)()
    masks = (C.POINTER(C.c_uint8) * 2)()
    assert _lib.lib().ocrs_engine_remove_rules_pages(eng._h, pages, C.c_size_t(2), ps, out, masks, None) == 1, "INVALID_ARGUMENT"
    assert [out[i] for i in range(2)] == [None, None] and not masks[0] and not masks[1], "a failed call writes nothing"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    one = C.c_void_p()
    assert _lib.lib().ocrs_engine_remove_rules_page(eng._h, inp._h, None, None, None, None) == 1
    assert _lib.lib().ocrs_engine_remove_rules_page(eng._h, inp._h, None, C.byref(one), None, None) == 0, "NULL: the default"
    assert image_of(OcrInput(one)).tobytes() == image_of(eng.remove_rules(inp)).tobytes()   # (the OcrInput frees the page)
    wide = eng.input_from_grey(np.zeros((1, 65536), np.float32))
    refused(lambda: eng.remove_rules(wide))
    row = np.full((1, 65535), -0.25, np.float32)
    row[0, 40000] = 0.5
    exp = check(eng, row, "1 x 65535")
    assert exp[2]["h_removed"] == 65534


# ------------------------------------------------------------------ 2. composition
def test_words_on_the_cleaned_table_are_the_oracles(eng, ora, table):
    clean, ruled, rule = table[512]
    exp = check(eng, ruled, "the table page")
    words = eng.detect_words(eng.remove_rules(eng.input_from_grey(ruled)))
    want = np.array([w.to_array() for w in ora.detect_words(exp[0][None])], np.float32).reshape(-1, 6)
    assert len(want) > 100 and words.shape == want.shape and words.tobytes() == want.tobytes()


def ruled_picture(seed, h, w, lines):
    """A synthetic page with a table grid drawn over it, as a picture."""
    px = synth.synthetic_page(seed, h, w, lines=lines, columns=1)
    for r in range(20, h - 2, 90):
        px[r:r + 2, 10:w - 10] = 0
    for c in (10, w // 2, w - 12):
        px[20:h - 20, c:c + 2] = 0
    return px


def test_get_text_with_rules_is_the_manual_chain(eng):
    inp = eng.prepare_input(ImageSource.from_tensor(ruled_picture(5, 600, 500, 24), DimOrder.Hwc))
    for params in (True, {"min_length": 200, "margin": 2}):
        kw = {} if params is True else params
        page, info = eng.remove_rules(inp, info=True, **kw)
        assert info["h_removed"] > 0 and info["v_removed"] > 0
        assert image_of(page).tobytes() == R.remove_rules(image_of(inp), **kw)[0].tobytes()
        lines = eng.find_text_lines(page, eng.detect_words(page))
        text = "\n".join(str(t) for t in eng.recognize_text(page, lines) if t is not None)
        assert len(lines) > 0 and eng.get_text(inp, rules=params) == text
        assert eng.get_text(inp, rules=params, rectify=True) == eng.get_text(page, rectify=True)
        norm = eng.normalize(inp)
        assert eng.get_text(inp, rules=params, normalize=True) == eng.get_text(eng.remove_rules(norm, **kw))
        upright = eng.deskew(norm, 1.5)[0]
        assert eng.get_text(inp, rules=params, normalize=True, deskew=1.5) == eng.get_text(eng.remove_rules(upright, **kw))
    assert eng.get_text(inp, rules=None) == eng.get_text(inp) == eng.get_text(inp, rules=False)


def test_cli_remove_rules(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    px = ruled_picture(9, 700, 600, 30)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("rules", "tuned", "plain")}
    assert cli.main([path, "--remove-rules", "-j", "--debug", "-o", files["rules"]]) == 0
    assert cli.main([path, "--remove-rules", "--rules-min-length", "200", "--rules-max-thickness", "4", "--rules-margin", "2", "-j", "-o", files["tuned"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in (["--rules-min-length", "200"], ["--rules-max-thickness", "4"], ["--rules-margin", "1"], ["--remove-rules", "--rules-margin", "9"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def document(**kw):
        page, info = eng.remove_rules(inp, info=True, **kw)
        lines = eng.find_text_lines(page, eng.detect_words(page))
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(page, lines), rules=info), info

    plain = output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "rules" not in json.loads(plain), "without the flag nothing changes"
    exp, info = document()
    assert text["rules"] == exp and info["h_removed"] > 0 and info["v_removed"] > 0
    assert json.loads(text["rules"])["rules"] == info and set(info) == set(R.INFO_KEYS)
    assert text["tuned"] == document(min_length=200, max_thickness=4, margin=2)[0]


# ------------------------------------------------------------------ 3. beside other callers
def test_rule_removing_callers_beside_plain_callers(eng, ora):
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    ruled = [eng.input_from_grey(R.draw_grid(image_of(p))[0]) for p in pages]
    params = [{}, {"min_length": 64, "margin": 2}, {"max_thickness": 1}, {"min_length": 200, "paper": 0.25}]

    def removed(i):
        page, mask, info = eng.remove_rules(ruled[i], mask=True, info=True, **params[i])
        return image_of(page).tobytes(), mask.tobytes(), tuple(sorted(info.items()))

    def plain(i):
        return eng.detect_words(pages[i]).tobytes()

    quiet_rules, quiet_plain = [removed(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        out, mask, info = R.remove_rules(image_of(ruled[i]), **params[i])
        assert quiet_rules[i] == (out.tobytes(), mask.tobytes(), tuple(sorted(info.items())))
        words = ora.detect_words(ora.prepare_input(OP.ImageSource.from_tensor(pxs[i], "hwc")))
        assert len(words) > 5 and quiet_plain[i] == np.array([w.to_array() for w in words], np.float32).tobytes()
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, removed(i) if t < 4 else plain(i))
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
        assert got == (quiet_rules[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)
