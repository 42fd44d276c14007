"""Working-resolution detection on the GPU, bit for bit against tests/resample_ref.py.

The area filter is compared with the restatement and the bilinear filter with the oracle's resize as 32-bit words, NaN
positions equal (a NaN compares as NaN, not by payload); detection at a work size is compared with the oracle's detector
run on the restatement's work page and mapped back by the restatement, and with the public calls composed by hand.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import json
import threading

import numpy as np
import pytest

import confidence_ref as CR
import detscore_ref as DR
import models_util as M
import resample_ref as R
import tiled_ref as TR
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, output, rescale_rects, synth, work_size
from oracle import clib
from oracle import pipeline as OP
from oracle.geometry import RotatedRect
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu
BENCH_PAGE = (0, 1024, 1024, 80, 2)   # bench.py's page: synth.synthetic_page(seed, 1024, 1024, lines=80)
MODEL_HW = (800, 600)
MIN_AREA = 100.0
# (source, result), (height, width): the identity; exact boxes; one output pixel; one row, one column; near-unit ratios
# (two taps, overlaps of 1 in P); ratios with no common factor, several blocks, odd widths; every width % 4 in and out;
# the bench page at the detector's squeeze; an 8 x 8 footprint over a page of more than 2^22 pixels
AREA_CASES = [((7, 7), (7, 7)), ((8, 8), (4, 4)), ((9, 6), (3, 2)), ((5, 5), (1, 1)), ((1, 300), (1, 7)), ((300, 1), (7, 1)),
              ((64, 65), (63, 64)), ((127, 129), (126, 128)), ((300, 211), (97, 64)), ((257, 259), (100, 37)),
              ((70, 256), (35, 128)), ((70, 257), (35, 129)), ((70, 258), (35, 130)), ((70, 259), (35, 131)),
              ((1024, 1024), (600, 576)), ((2200, 3000), (275, 375))]
BILINEAR_CASES = [((1, 1), (5, 5)), ((3, 2), (9, 6)), ((97, 211), (300, 400)), ((600, 800), (1024, 1024)), ((300, 211), (97, 64))]


def ids(case):
    return "%dx%d-%dx%d" % (case[0] + case[1])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def models():
    return M.detection_model_bytes(), M.recognition_model_bytes()


@pytest.fixture(scope="module")
def eng(models):
    return OcrEngine(detection_model=Model.load_bytes(models[0]), recognition_model=Model.load_bytes(models[1]))


def prepare(engine, px):
    return engine.prepare_input(ImageSource.from_tensor(np.ascontiguousarray(px), DimOrder.Hwc))


def image_of(page):
    return np.ascontiguousarray(page.image()[0])


# ------------------------------------------------------------------ 1. the kernel
def planted_page(seed, h, w, plant=True):
    """[h, w] float32, uniform in [-0.5, 0.5), with NaN, +inf, -inf and -0.0 planted (fewer on a page of fewer pixels)."""
    rng = np.random.default_rng(seed)
    a = (rng.random((h, w), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    if plant:
        planted = np.array([-0.0, np.nan, np.inf, -np.inf, -0.0, np.nan], np.float32)
        flat = a.reshape(-1)
        n = min(len(planted), max(1, flat.size // 8))
        flat[rng.choice(flat.size, size=n, replace=False)] = planted[:n]
    return a


def assert_same_words(got, exp, what):
    assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.shape, exp.shape)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ at %s" % (what, np.argwhere(np.isnan(got) != nan)[:4].tolist())
    bad = np.argwhere((got.view(np.uint32) != exp.view(np.uint32)) & ~nan)
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r (%#x), expected %r (%#x)"
                             % (what, len(bad), got.size, at, got[at], got.view(np.uint32)[at], exp[at], exp.view(np.uint32)[at]))


@pytest.mark.parametrize("case", AREA_CASES, ids=ids)
def test_area_equals_the_restatement(eng, case):
    (h, w), out_hw = case
    for plant in (True, False):
        src = planted_page(h * 1000 + w, h, w, plant)
        inp = eng.input_from_grey(src)
        exp = R.area(src, *out_hw)
        if plant and h * w > 100:
            assert not np.isnan(exp).all() and np.isnan(exp).any()
        out = eng.resize(inp, out_hw, "area")
        assert out.shape == (1,) + out_hw
        assert_same_words(image_of(out), exp, "area %s, planted %s" % (ids(case), plant))
    if out_hw == (h, w):   # equal sizes: the identity, -0.0 included
        src = planted_page(1, h, w)
        keep = ~np.isnan(src)
        assert np.array_equal(image_of(eng.resize(eng.input_from_grey(src), out_hw, "area")).view(np.uint32)[keep], src.view(np.uint32)[keep])


@pytest.mark.parametrize("case", BILINEAR_CASES, ids=ids)
def test_bilinear_equals_the_oracles_resize(eng, case):
    (h, w), out_hw = case
    for plant in (True, False):
        src = planted_page(h * 1000 + w + 1, h, w, plant)
        out = eng.resize(eng.input_from_grey(src), out_hw, "bilinear")
        assert out.shape == (1,) + out_hw
        assert_same_words(image_of(out), clib.resize_bilinear(src, *out_hw), "bilinear %s, planted %s" % (ids(case), plant))


MIXED = [((97, 211), (300, 400), "bilinear"), ((300, 211), (97, 64), "area"), ((64, 65), (63, 64), "auto"), ((3, 2), (9, 6), "auto"),
         ((257, 259), (100, 37), "bilinear"), ((70, 258), (70, 258), "area")]


def test_mixed_batch_equals_each_page_alone(eng):
    srcs = [planted_page(40 + i, *s) for i, (s, _, _) in enumerate(MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    batch = eng.resize_batch(inputs, [o for _, o, _ in MIXED], [f for _, _, f in MIXED])
    for src, inp, (_, out_hw, filt), out in zip(srcs, inputs, MIXED, batch):
        exp = R.resize(src, out_hw, filt)
        assert_same_words(image_of(out), exp, "batch %s %s" % (out_hw, filt))
        assert_same_words(image_of(eng.resize(inp, out_hw, filt)), exp, "alone %s %s" % (out_hw, filt))
    one_filter = eng.resize_batch(inputs[:2], [(50, 60), (50, 60)], "bilinear")
    assert_same_words(image_of(one_filter[1]), clib.resize_bilinear(srcs[1], 50, 60), "one filter for all")
    assert eng.resize_batch([], []) == []
    with pytest.raises(ValueError):
        eng.resize_batch(inputs, [(5, 5)])


# a page boundary inside, on and just past a 64-column block edge; a grow, a shrink, an identity, a grow and a shrink
EDGE_MIXED = [((1, 1), (3, 2), "auto"), ((63, 65), (31, 33), "area"), ((64, 64), (64, 64), "auto"), ((65, 63), (70, 64), "bilinear"),
              ((130, 7), (65, 7), "auto")]


def test_edge_sized_batch_equals_each_page_alone(eng):
    srcs = [planted_page(60 + i, *s) for i, (s, _, _) in enumerate(EDGE_MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    batch = eng.resize_batch(inputs, [o for _, o, _ in EDGE_MIXED], [f for _, _, f in EDGE_MIXED])
    for src, inp, (_, out_hw, filt), out in zip(srcs, inputs, EDGE_MIXED, batch):
        assert_same_words(image_of(out), image_of(eng.resize(inp, out_hw, filt)), "batch against alone %s %s" % (out_hw, filt))
        assert_same_words(image_of(out), R.resize(src, out_hw, filt), "batch %s %s" % (out_hw, filt))


def test_a_bad_page_in_the_middle_returns_nothing_and_leaks_nothing(eng):
    inputs = [eng.input_from_grey(planted_page(80 + i, 40, 50)) for i in range(3)]
    pages = (C.c_void_p * 3)(*[i._h for i in inputs])
    hw = (C.c_int * 6)(20, 25, 0, 25, 20, 25)
    fl = (C.c_int * 3)(0, 0, 0)
    out = (C.c_void_p * 3)()
    live = _lib.pool_stats()["device_live"]
    assert _lib.lib().ocrs_engine_resize_pages(eng._h, pages, C.c_size_t(3), hw, fl, out) == 1, "INVALID_ARGUMENT"
    assert [out[i] for i in range(3)] == [None] * 3, "a failed call writes no page"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    with pytest.raises(_lib.OcrsError) as e:
        eng.resize_batch(inputs, [(20, 25), (0, 25), (20, 25)])
    assert e.value.status_name == "INVALID_ARGUMENT", e.value
    assert _lib.pool_stats()["device_live"] == live


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = planted_page(99, 131, 70, plant=False)
    inp = eng.input_from_grey(src)
    for hw, filt in (((131, 70), "area"), ((60, 33), "area"), ((200, 90), "bilinear")):
        out = eng.resize(inp, hw, filt)
        assert image_of(inp).tobytes() == src.tobytes()
        del out   # ocrs_page_free of the result: the source is a page of its own (equal sizes included)
        assert image_of(inp).tobytes() == src.tobytes()
        assert image_of(eng.resize(inp, hw, filt)).tobytes() == R.resize(src, hw, filt).tobytes()
    out = eng.resize(inp, (131, 70))
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == src.tobytes()


def test_auto_picks_the_filter_and_errors_have_their_status(eng):
    src = planted_page(5, 90, 120, plant=False)
    inp = eng.input_from_grey(src)
    for hw, filt in (((45, 60), "area"), ((90, 120), "area"), ((90, 60), "area"), ((91, 60), "bilinear"), ((45, 121), "bilinear"),
                     ((180, 240), "bilinear")):
        assert R.resolve_filter(src.shape, hw, "auto") == filt
        got = image_of(eng.resize(inp, hw))
        assert got.tobytes() == image_of(eng.resize(inp, hw, filt)).tobytes() == R.resize(src, hw, filt).tobytes(), hw
    # (at a halving the bilinear taps are the box's four pixels at weight 1/2 each: the two filters differ from a third on)
    assert R.area(src, 30, 40).tobytes() != clib.resize_bilinear(src, 30, 40).tobytes(), "the two filters differ where both apply"
    assert image_of(eng.resize(inp, (30, 40))).tobytes() == R.area(src, 30, 40).tobytes()

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    for hw in ((0, 5), (5, 0), (-1, 5), (65536, 5), (5, 65536)):
        for filt in ("auto", "bilinear", "area"):
            refused(lambda: eng.resize(inp, hw, filt))
    for hw in ((91, 60), (45, 121), (180, 240)):
        refused(lambda: eng.resize(inp, hw, "area"))          # the area filter only shrinks
    refused(lambda: eng.resize_batch([inp, inp], [(45, 60), (0, 1)]))   # one bad page refuses the call
    assert eng.resize(inp, (65535, 1), "bilinear").shape == (1, 65535, 1) and eng.resize(inp, (1, 1), "area").shape == (1, 1, 1)
    out = C.c_void_p()
    assert _lib.lib().ocrs_engine_resize_page(eng._h, inp._h, 5, 5, 7, C.byref(out)) == 1, "an unknown filter"
    for hw in ((0, 5), (5, 0), (65536, 1)):
        refused(lambda: eng.detect_words(inp, work_size=hw))
    refused(lambda: eng.detect_words(inp, work_size=(91, 60), work_filter="area"))
    rects, n = C.POINTER(C.c_float)(), C.c_size_t(0)
    assert _lib.lib().ocrs_engine_detect_words_at(eng._h, inp._h, 0, 0, 7, 0, -1, C.byref(rects), C.byref(n), None, None) == 1
    sc = C.POINTER(C.c_float)()
    assert _lib.lib().ocrs_engine_detect_words_at(eng._h, inp._h, 0, 0, 0, 0, -1, C.byref(rects), C.byref(n), C.byref(sc), None) == 1, \
        "score and pixels come together"


# ------------------------------------------------------------------ 2. detection at a work size, end to end
class EndToEnd:
    """The bench page, the oracle on it, and per case the reference: the oracle's detector on the restatement's work page
    (tiled: tiled_ref's stitched map), detscore_ref's words of that map, mapped back by the restatement."""
    CASES = {"512-area": ((512, 512), "area", False), "1536-bilinear-tiled": ((1536, 1536), "bilinear", True)}

    def __init__(self, eng, models):
        self.eng = eng
        self.rbuf = models[1]
        self.ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(models[0]), "exact"),
                                recognition_model=OracleModel(OracleGraph(models[1]), "exact"))
        self.px = synth.synthetic_page(*BENCH_PAGE)
        self.inp = prepare(eng, self.px)
        self.oin = self.ora.prepare_input(OP.ImageSource.from_tensor(self.px, "hwc"))
        self.grey = np.ascontiguousarray(np.asarray(self.oin, np.float32)[0])
        assert self.grey.tobytes() == image_of(self.inp).tobytes()
        self.thr = float(eng.detection_threshold())
        self._refs = {}

    def ref(self, name):
        if name not in self._refs:
            hw, filt, tiled = self.CASES[name]
            work = R.resize(self.grey, hw, filt)
            if tiled:
                P = TR.stitched(work, TR.oracle_run_tile(self.ora.detector), MODEL_HW, TR.OVERLAP_DEFAULT)
            else:
                P = self.ora.detector.detect_text_pixels(work[None])
            rects, score, pixels = DR.reference(P, self.thr, MIN_AREA)
            self._refs[name] = (work, rects, R.rescale_rects(rects, hw, self.grey.shape), score, pixels)
        return self._refs[name]


@pytest.fixture(scope="module")
def e2e(eng, models):
    return EndToEnd(eng, models)


def assert_detection(what, got, rects, score, pixels):
    gr, gs, gp = got
    assert gr.shape == rects.shape, "%s: %d words, expected %d" % (what, len(gr), len(rects))
    assert gr.dtype == np.float32 and gr.tobytes() == rects.tobytes(), what + ": rects"
    assert gp.dtype == np.uint32 and np.array_equal(gp, pixels), what + ": pixels"
    assert gs.dtype == np.float32 and np.array_equal(DR.bits(gs), DR.bits(score)), what + ": scores"


@pytest.mark.parametrize("name", list(EndToEnd.CASES))
def test_detection_at_a_work_size_equals_the_oracle_on_the_restatements_page(e2e, name):
    eng = e2e.eng
    hw, filt, tiled = e2e.CASES[name]
    work, work_rects, rects, score, pixels = e2e.ref(name)
    print("%s: %d words at %s; the page at its own size has %d" % (name, len(rects), hw, len(eng.detect_words(e2e.inp, tiled=tiled))))
    assert len(rects) >= 50 and work_rects.tobytes() != rects.tobytes()
    # the call, scored and not, filter named and auto
    assert_detection(name, eng.detect_words(e2e.inp, scores=True, tiled=tiled, work_size=hw, work_filter=filt), rects, score, pixels)
    assert_detection(name + " auto", eng.detect_words(e2e.inp, scores=True, tiled=tiled, work_size=hw), rects, score, pixels)
    assert eng.detect_words(e2e.inp, tiled=tiled, work_size=hw).tobytes() == rects.tobytes()
    if tiled:
        assert eng.detect_words(e2e.inp, tiled=TR.OVERLAP_DEFAULT, work_size=hw).tobytes() == rects.tobytes()
        assert eng.detect_words(e2e.inp, work_size=hw).tobytes() != rects.tobytes(), "the tiled flag reaches the work page"
    # the public calls composed by hand
    page = eng.resize(e2e.inp, hw, filt)
    assert image_of(page).tobytes() == work.tobytes()
    wr, ws, wp = eng.detect_words(page, scores=True, tiled=tiled)
    assert wr.tobytes() == work_rects.tobytes()
    assert_detection(name + " by hand", (rescale_rects(wr, hw, e2e.grey.shape), ws, wp), rects, score, pixels)
    # the mapped words lie on the page: the work page is the same picture
    assert np.all((rects[:, 0] > -1) & (rects[:, 0] < 1024) & (rects[:, 1] > -1) & (rects[:, 1] < 1024))


@pytest.mark.parametrize("name", list(EndToEnd.CASES))
def test_lines_and_scored_recognition_on_the_original_page_equal_the_oracle(e2e, name):
    eng, ora = e2e.eng, e2e.ora
    hw, filt, tiled = e2e.CASES[name]
    rects = e2e.ref(name)[2]
    words = eng.detect_words(e2e.inp, tiled=tiled, work_size=hw, work_filter=filt)
    assert words.tobytes() == rects.tobytes()
    lines = eng.find_text_lines(e2e.inp, words)
    olines = ora.find_text_lines(e2e.oin, [RotatedRect.from_array(r) for r in rects])
    assert len(lines) == len(olines) >= 40
    for a, b in zip(lines, olines):
        assert np.array_equal(a, np.array([w.to_array() for w in b], np.float32).reshape(-1, 6))
    # recognition: every tenth line through the oracle (its rows are independent, so a subset has the whole request's bits)
    got = eng.recognize_text(e2e.inp, lines, scores=True)
    pick = list(range(0, len(olines), 10))
    exp = ora.recognize_text(e2e.oin, [olines[i] for i in pick])
    logits = M.oracle_line_logits(e2e.rbuf, ora, e2e.oin, [olines[i] for i in pick])
    assert len(got) == len(lines) and len(exp) == len(logits) == len(pick) >= 5
    n_chars = 0
    for i, e, L in zip(pick, exp, logits):
        g = got[i]
        assert (g is None) == (e is None)
        if g is None:
            continue
        assert str(g) == str(e)
        assert [c.rect for c in g.chars()] == [c.rect.tlbr() for c in e.chars]
        steps, slp, line_score = CR.greedy(CR.masked(L, ora.excluded_char_labels))
        assert CR.bits_equal(g.score, line_score)
        assert np.array_equal(np.array([c.logp for c in g.chars()], np.float32), slp[:len(g.chars())])
        n_chars += len(e.chars)
    assert n_chars > 50
    assert eng.get_text(e2e.inp, work_size=hw) == "\n".join(str(t) for t in eng.recognize_text(e2e.inp, eng.find_text_lines(
        e2e.inp, eng.detect_words(e2e.inp, work_size=hw))) if t is not None)


def test_the_pages_own_size_gives_the_plain_calls_bits(eng, e2e):
    small = prepare(eng, synth.synthetic_page(5, 400, 500, lines=30, columns=1))
    for inp, own in ((e2e.inp, (1024, 1024)), (small, (400, 500))):
        for tiled in (False, True):
            plain = eng.detect_words(inp, scores=True, tiled=tiled)
            assert len(plain[0]) > 20
            for ws in (own, (0, 0)):
                for filt in ("auto", "area", "bilinear"):
                    got = eng.detect_words(inp, scores=True, tiled=tiled, work_size=ws, work_filter=filt)
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, plain)), (own, tiled, ws, filt)
                assert eng.detect_words(inp, tiled=tiled, work_size=ws).tobytes() == plain[0].tobytes()
    batch = eng.detect_words_batch([e2e.inp, small], work_sizes=[None, (0, 0)])
    assert batch[0].tobytes() == eng.detect_words(e2e.inp).tobytes() and batch[1].tobytes() == eng.detect_words(small).tobytes()
    assert eng.get_text(small, work_size=(400, 500)) == eng.get_text(small)


def test_batch_of_four_page_sizes_equals_each_page_alone(eng, e2e):
    specs = [(21, 600, 800, 24, 1), (22, 1024, 1024, 80, 2), (23, 400, 500, 30, 1), (24, 1400, 1100, 110, 2)]
    inputs = [prepare(eng, synth.synthetic_page(*s)) for s in specs]
    sizes = [(300, 400), (1536, 1536), None, work_size((1400, 1100), max_side=1000)]
    assert sizes[3] == (1000, 786)
    for tiled in (False, True):
        words, score, pixels = eng.detect_words_batch(inputs, scores=True, tiled=tiled, work_sizes=sizes)
        plain = eng.detect_words_batch(inputs, tiled=tiled, work_sizes=sizes)
        for i, (inp, ws) in enumerate(zip(inputs, sizes)):
            alone = eng.detect_words(inp, scores=True, tiled=tiled, work_size=ws)
            assert len(alone[0]) > 10
            assert all(a.tobytes() == b.tobytes() for a, b in zip((words[i], score[i], pixels[i]), alone)), (tiled, i)
            assert plain[i].tobytes() == alone[0].tobytes()
    assert eng.detect_words_batch([], work_sizes=[]) == []
    with pytest.raises(ValueError):
        eng.detect_words_batch(inputs, work_sizes=sizes[:2])


def test_work_resolution_callers_beside_plain_callers(eng):
    pages = [prepare(eng, synth.synthetic_page(30 + i, 600, 800, 24, 1)) for i in range(4)]
    sizes = [(300, 400), (450, 600), (900, 1200), (600, 799)]

    def at(i):
        return tuple(a.tobytes() for a in eng.detect_words(pages[i], scores=True, work_size=sizes[i]))

    def plain(i):
        return tuple(a.tobytes() for a in eng.detect_words(pages[i], scores=True))

    quiet_at, quiet_plain = [at(i) for i in range(4)], [plain(i) for i in range(4)]
    assert all(a != b for a, b in zip(quiet_at, quiet_plain))
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, at(i) if t < 4 else plain(i))
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
        assert got == (quiet_at[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)


# ------------------------------------------------------------------ 3. the CLI
def test_cli_work_resolution(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    px = synth.synthetic_page(9, 900, 700, lines=40, columns=1)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("scale", "side", "plain", "tiled", "up")}
    assert cli.main([path, "--work-scale", "0.5", "-j", "--detection-confidence", "--text-map", "-o", files["scale"]]) == 0
    assert cli.main([path, "--work-max-side", "600", "-j", "--detection-confidence", "-o", files["side"]]) == 0
    assert cli.main([path, "-j", "--detection-confidence", "-o", files["plain"]]) == 0
    assert cli.main([path, "--work-scale", "1.5", "--tiled", "-j", "--detection-confidence", "--rectify", "-o", files["tiled"]]) == 0
    assert cli.main([path, "--work-scale", "0.5", "--orientation", "90", "-j", "-o", files["up"]]) == 0
    with pytest.raises(SystemExit):
        cli.main([path, "--work-scale", "0.5", "--work-max-side", "600"])
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = prepare(eng, cli.load_image(path))

    def document(ws, tiled=False, rectify=False):
        words, score, pixels = eng.detect_words(inp, scores=True, tiled=tiled, work_size=ws)
        lines, index = eng.find_text_lines(inp, words, index=True)
        boxes = [[(words[k], score[k], pixels[k]) for k in idx] for idx in index]
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, lines, rectify=rectify), word_boxes=boxes)

    assert work_size((900, 700), scale=0.5) == (450, 350) and work_size((900, 700), max_side=600) == (600, 467)
    assert document((450, 350)) == text["scale"] and document((600, 467)) == text["side"]
    assert document((1350, 1050), tiled=True, rectify=True) == text["tiled"]
    assert document(None) == text["plain"], "without the flags nothing changes"
    assert len({text["scale"], text["side"], text["plain"], text["tiled"]}) == 4
    # vertices are in the file's frame
    doc = json.loads(text["scale"])
    assert doc["image_height"] == 900 and doc["image_width"] == 700
    lines = doc["paragraphs"][0]["lines"]
    assert len(lines) > 10 and max(v[1] for l in lines for v in l["vertices"]) > 450
    # --text-map with a working resolution: the map of the work page
    want = eng.detect_text_pixels(eng.resize(inp, (450, 350)))
    want = (np.clip(want, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "text-map.png"))), want)
    # after --orientation: the work size is that of the turned page
    turned = eng.rotate(inp, 1)
    assert turned.shape == (1, 700, 900)
    tlines = eng.find_text_lines(turned, eng.detect_words(turned, work_size=(350, 450)))
    from ocrs_amd import unrotate_lines
    back = unrotate_lines(eng.recognize_text(turned, tlines), px.shape[:2], 1)
    assert output.format_json_output(path, px.shape[:2], back, orientation=90) == text["up"]
