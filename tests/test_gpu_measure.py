"""Page measurement on the GPU, every field and every bin against tests/measure_ref.py.

Pages are put on the device with input_from_grey; what the passes counted (ocrs_measure_info) is compared with the
restatement as integers, bin by bin.  The shapes are the smallest at which the kernels can go wrong: the word boundary
x = 63|64, the tile boundary y = 63|64, widths that are and are not multiples of 4 and 64, several tiles either way.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import json

import numpy as np
import pytest

import despeckle_pages as P
import measure_ref as MR
import models_util as M
import resample_ref as RR
from ocrs_amd import (DimOrder, ImageSource, Model, OcrEngine, TextScale, _lib, measure_choose, rescale_rects, synth, work_scale_for_text,
                      work_size)

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(1, 1), (1, 64), (1, 65), (64, 1), (65, 1), (63, 63), (64, 64), (65, 129), (130, 67), (200, 256)]
DENSITIES = (0.05, 0.5, 0.95)   # dust, percolating 8-connected ink, ink with pinholes


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    return OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(M.recognition_model_bytes()))


def image_of(page):
    return np.ascontiguousarray(page.image()[0])


def random_page(seed, h, w, density):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < density, F(-0.3), F(0.3)).astype(F)


def assert_same(got, ref, what):
    assert tuple(got) == MR.INFO_KEYS, what
    for k in MR.INFO_KEYS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if a.ndim:
            assert a.dtype == b.dtype and a.shape == (256,), (what, k)
            bad = np.nonzero(a != b)[0]
            assert len(bad) == 0, "%s: %s differs at bins %s: got %s, expected %s" % (what, k, bad[:8].tolist(), a[bad[:8]].tolist(), b[bad[:8]].tolist())
        else:
            assert int(a) == int(b), "%s: %s is %d, expected %d" % (what, k, int(a), int(b))


def check_batch(eng, pages, params, what):
    """One call for all the pages, each held to the restatement -> the records."""
    params = [dict(p or {}) for p in params]
    got = eng.measure_batch([eng.input_from_grey(p) for p in pages], params)
    assert len(got) == len(pages)
    for i, (g, page, kw) in enumerate(zip(got, pages, params)):
        assert_same(g, MR.measure(page, **kw), "%s, page %d of %dx%d %r" % (what, i, page.shape[0], page.shape[1], kw))
    return got


# ------------------------------------------------------------------ 1. shapes and patterns
def test_random_ink_at_every_shape_and_density(eng):
    pages = [random_page(100 * i + j, h, w, d) for i, (h, w) in enumerate(SHAPES) for j, d in enumerate(DENSITIES)]
    got = check_batch(eng, pages, [{"min_area": i % 3} for i in range(len(pages))], "random ink")
    assert sum(g["components"] for g in got) > 1000 and any(g["counted"] < g["components"] for g in got)


def test_the_despeckle_patterns_at_130_by_200(eng):
    h, w = 130, 200
    a, b = P.corner_pairs(h, w)
    pages = [P.planted_blobs(h, w, 1), P.planted_blobs(h, w, 4), P.planted_blobs(h, w, 9), P.checkerboard(h, w), P.diagonals(h, w),
             P.diagonals(h, w, 3, True), P.serpentine(h, w), P.spiral(h, w), P.u_shape(h, w), a, b, P.serpentine(h, w, True), P.spiral(h, w, True)]
    got = check_batch(eng, pages, [{"min_area": m} for m in (4, 4, 4, 1, 2, 2, 4, 4, 4, 2, 4, 0, 9)], "patterns")
    assert got[6]["components"] == 1 and got[6]["comp_h"][h] == 1 and got[6]["comp_w"][w] == 1, "the serpentine visits every tile"
    assert got[7]["components"] == 1 and got[7]["comp_h"][h] == 1, "the spiral is one component"
    assert got[8]["components"] == 2 and got[8]["comp_h"][h] == 1 and got[8]["comp_h"][h - 2] == 1, "the arms of a U meet far from its root"
    assert got[9]["components"] == 2 and got[9]["comp_h"][2] == 2 and got[9]["comp_w"][2] == 2, "touching by a corner: one component, a 2 x 2 box"
    assert got[3]["components"] == 1, "a checkerboard is one 8-connected component"


def test_boxes_and_runs_that_cross_tiles(eng):
    cross = P.paper(200, 200)        # the root at (70, 70); x0, x1 and y1 each in another tile than the root
    cross[70:200, 70] = P.INK
    cross[130, 10:191] = P.INK
    far = P.paper(300, 300)          # runs that start in one word / tile and end three further on
    far[10, 50:251] = P.INK
    far[40:241, 20] = P.INK
    edges = P.paper(12, 300)         # runs of 254, 255, 256 and of the full side, across and (transposed) down
    edges[2, 3:257] = edges[4, 3:258] = edges[6, 3:259] = P.INK
    edges[8, :] = P.INK
    edges[10, 0:64] = edges[10, 64:128] = P.INK   # whole words side by side: one run of 128
    full, empty = np.full((130, 67), P.INK, F), P.paper(130, 67)
    wide = np.full((70, 300), P.INK, F)
    got = check_batch(eng, [cross, far, edges, np.ascontiguousarray(edges.T), full, empty, wide, np.ascontiguousarray(wide.T)], [None] * 8, "crossing")
    assert got[0]["components"] == 1 and got[0]["comp_h"][130] == 1 and got[0]["comp_w"][181] == 1 and got[0]["area_by_h"][130] == 130 + 180
    assert got[1]["run_h"][201] == 1 and got[1]["run_v"][201] == 1
    assert got[2]["run_h"][254] == 1 and got[2]["run_h"][255] == 3 and got[2]["run_h"][128] == 1 and got[3]["run_v"][255] == 3
    assert got[4]["run_h"][67] == 130 and got[4]["run_v"][130] == 67 and got[4]["components"] == 1 and got[4]["comp_w"][67] == 1
    assert got[5]["ink"] == 0 and got[5]["components"] == 0 and not any(np.asarray(got[5][k]).any() for k in MR.INFO_KEYS[3:])
    assert got[6]["run_h"][255] == 70 and got[6]["run_v"][70] == 300 and got[6]["comp_w"][255] == 1 and got[6]["area_by_h"][70] == 21000


def test_nan_negative_zero_and_the_threshold_edge(eng):
    vals = np.array([np.nan, -0.0, 0.0, 0.25, np.nextafter(F(0.25), F(-1)), -np.inf, np.inf, -1e-45, 1e-45, -0.1, np.nextafter(F(-0.1), F(-1))], F)
    page = np.tile(vals, (70, 7))[:, :70].copy()
    page.view(np.uint32)[3, 0] = 0xFFC00001   # a negative NaN
    got = check_batch(eng, [page] * 4, [{"threshold": t, "min_area": 1} for t in (0.0, 0.25, -0.1, 1e-45)], "edges")
    assert got[0]["ink"] < got[3]["ink"] < got[1]["ink"] and got[2]["ink"] > 0


def test_min_area_at_its_edges(eng):
    page = P.paper(130, 200)
    for i, area in enumerate(range(1, 10)):
        P.plant(page, 10, 10 + 20 * i, area)
        P.plant(page, 62, 10 + 20 * i, area)   # across y = 63|64
    got = check_batch(eng, [page] * 6, [{"min_area": m} for m in (0, 1, 4, 5, 9, 65535)], "min_area")
    assert [g["counted"] for g in got] == [18, 18, 12, 10, 2, 0] and all(g["components"] == 18 for g in got)


# ------------------------------------------------------------------ 2. batches
def mixed_batch():
    specs = [(97, 211, 0.3), (1, 1, 0.95), (300, 3, 0.5), (64, 64, 0.5), (5, 1000, 0.4), (130, 67, 0.05), (200, 256, 0.6), (65, 129, 0.95)]
    pages = [random_page(900 + i, h, w, d) for i, (h, w, d) in enumerate(specs)]
    params = [{"threshold": t, "min_area": m} for t, m in ((0.0, 4), (0.0, 0), (0.1, 1), (-0.1, 2), (0.0, 65535), (0.5, 3), (0.0, 9), (0.0, 1))]
    return pages, params


def as_bytes(info):
    return b"".join(np.asarray(info[k]).tobytes() for k in MR.INFO_KEYS)


def test_a_mixed_batch_equals_its_pages_alone_and_itself_in_reverse(eng):
    pages, params = mixed_batch()
    inputs = [eng.input_from_grey(p) for p in pages]
    before = [image_of(i).tobytes() for i in inputs]
    together = check_batch(eng, pages, params, "mixed batch")
    again = eng.measure_batch(inputs, params)
    reverse = eng.measure_batch(inputs[::-1], params[::-1])[::-1]
    alone = [eng.measure(i, **kw) for i, kw in zip(inputs, params)]
    for t, a, r, o in zip(together, again, reverse, alone):
        assert as_bytes(t) == as_bytes(a) == as_bytes(r) == as_bytes(o)
    assert [image_of(i).tobytes() for i in inputs] == before, "measuring leaves the page's bits alone"
    assert eng.measure_batch([]) == []
    assert _lib.lib().ocrs_engine_measure_pages(eng._h, None, C.c_size_t(0), None, None) == 0, "an empty batch launches nothing"
    with pytest.raises(ValueError):
        eng.measure_batch(inputs, params[:2])


# ------------------------------------------------------------------ 3. the public interface
def planted_page():
    """test_measure_cpu.py's: six bars 5 wide and 21 tall, six boxes 21 tall and 30 to 40 wide drawn with strokes of 5, specks."""
    page = P.paper(120, 300)
    x = 10
    for i in range(6):
        page[10:31, 10 + 30 * i:15 + 30 * i] = P.INK
        w = 30 + 2 * i
        page[60:81, x:x + w] = P.INK
        page[65:76, x + 5:x + w - 5] = P.PAPER
        x += w + 8
        page[100, 10 + 30 * i] = P.INK
    return page


@pytest.fixture(scope="module")
def text_page(eng):
    """The 512 x 512 text page of DESIGN.md §7.14 on the device, and its grey levels."""
    inp = eng.prepare_input(ImageSource.from_tensor(synth.synthetic_page(3, 512, 512, 20, 1, 1), DimOrder.Hwc))
    return inp, image_of(inp)


def test_text_scale_and_the_measured_work_size(eng, text_page):
    inp, grey = text_page
    info = MR.measure(grey)
    assert_same(eng.measure(inp), info, "the text page")
    ref = MR.choose(info)
    scale = eng.text_scale(inp)
    assert eng.text_scale(eng.input_from_grey(planted_page())) == TextScale(5, 21, 12, False), "a stroke thinner than the text, from a page"
    assert isinstance(scale, TextScale) and scale == TextScale(ref["stroke"], ref["text_height"], ref["support"], bool(ref["blank"]))
    assert scale == measure_choose(eng.measure(inp)) and scale.text_height == 14 and not scale.blank
    assert eng.text_scale(inp, min_height_strokes=1.5, min_area=9) == TextScale(*[MR.choose(MR.measure(grey, min_area=9), 1.5)[k] for k in MR.CHOICE_KEYS])
    plain = eng.detect_words(inp, scores=True)
    for target in (20, 9, True, 200):
        hand = RR.work_size(grey.shape, MR.work_scale_for_text(ref["text_height"], MR.WORK_TEXT_HEIGHT_DEFAULT if target is True else target))
        want = eng.detect_words(inp, scores=True, work_size=hand)
        got = eng.detect_words(inp, scores=True, work_text_height=target)
        assert len(got[0]) > 10 and all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), target
        if target is True:
            assert hand == grey.shape and all(a.tobytes() == b.tobytes() for a, b in zip(got, plain)), "measured at its target the page is read as it is"
    assert eng.detect_words(inp, work_text_height=200, tiled=True).tobytes() == eng.detect_words(inp, work_size=(2048, 2048), tiled=True).tobytes()
    blank = eng.input_from_grey(P.paper(100, 120))
    assert eng.text_scale(blank) == TextScale(0, 0, 0, True)
    assert eng.detect_words(blank, work_text_height=30).tobytes() == eng.detect_words(blank).tobytes(), "a blank page keeps its size"
    with pytest.raises(ValueError):
        eng.detect_words(inp, work_size=(256, 256), work_text_height=20)
    with pytest.raises(ValueError):
        eng.get_text(inp, work_size=(256, 256), work_text_height=True)


def test_get_text_with_a_measured_work_size(eng, text_page):
    inp, grey = text_page
    plain = eng.get_text(inp)
    assert len(plain) > 20 and eng.get_text(inp, work_text_height=None) == plain
    hand = RR.work_size(grey.shape, MR.work_scale_for_text(MR.choose(MR.measure(grey))["text_height"], 21))
    lines = eng.find_text_lines(inp, eng.detect_words(inp, work_size=hand))
    manual = "\n".join(str(t) for t in eng.recognize_text(inp, lines) if t is not None)
    assert eng.get_text(inp, work_text_height=21) == manual
    # measured after the other page operations: the despeckled page is what is measured
    noisy = eng.input_from_grey(np.where(np.random.default_rng(4).random(grey.shape) < 0.002, F(-0.5), grey).astype(F))
    clean = eng.despeckle(noisy)
    lines = eng.find_text_lines(clean, eng.detect_words(clean, work_size=RR.work_size(grey.shape, MR.work_scale_for_text(eng.text_scale(clean).text_height, 21))))
    assert eng.get_text(noisy, despeckle=True, work_text_height=21) == "\n".join(str(t) for t in eng.recognize_text(clean, lines) if t is not None)


def test_bad_arguments_have_their_status(eng):
    inp = eng.input_from_grey(random_page(1, 20, 20, 0.3))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    for kw in ({"threshold": float("nan")}, {"threshold": float("inf")}, {"threshold": float("-inf")}, {"min_area": -1}, {"min_area": 65536}):
        refused(lambda: eng.measure(inp, **kw))
    refused(lambda: eng.measure_batch([inp, inp], [None, {"min_area": 65536}]))   # one bad page refuses the call
    live = _lib.pool_stats()["device_live"]
    L = _lib.lib()
    pages = (C.c_void_p * 2)(inp._h, inp._h)
    infos = (_lib.MeasureInfo * 2)()
    C.memset(infos, 0xAB, C.sizeof(infos))
    ps = (_lib.MeasureParams * 2)(_lib.MeasureParams(0.0, 4), _lib.MeasureParams(0.0, 65536))
    assert L.ocrs_engine_measure_pages(eng._h, pages, C.c_size_t(2), ps, infos) == 1, "INVALID_ARGUMENT"
    assert bytes(infos) == b"\xab" * C.sizeof(infos), "a failed call writes nothing"
    ok = (_lib.MeasureParams * 2)(_lib.MeasureParams(0.0, 4), _lib.MeasureParams(0.0, 4))
    assert L.ocrs_engine_measure_pages(eng._h, None, C.c_size_t(2), ok, infos) == 1 and L.ocrs_engine_measure_pages(eng._h, pages, C.c_size_t(2), None, infos) == 1
    assert L.ocrs_engine_measure_pages(eng._h, pages, C.c_size_t(2), ok, None) == 1 and L.ocrs_engine_measure_pages(None, pages, C.c_size_t(2), ok, infos) == 1
    assert L.ocrs_engine_measure_pages(eng._h, (C.c_void_p * 2)(inp._h, None), C.c_size_t(2), ok, infos) == 1, "a null page"
    assert L.ocrs_engine_measure_page(eng._h, inp._h, None, None) == 1 and L.ocrs_engine_measure_page(eng._h, None, None, infos) == 1
    assert bytes(infos) == b"\xab" * C.sizeof(infos)
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    assert L.ocrs_engine_measure_page(eng._h, inp._h, None, infos) == 0, "NULL: the default"
    assert as_bytes(infos[0].as_dict()) == as_bytes(eng.measure(inp))
    wide = eng.input_from_grey(np.zeros((1, 65536), F))
    refused(lambda: eng.measure(wide))
    # a page belongs to a device: another engine of this device serves it, an engine of another device refuses it
    dbuf, rbuf = M.detection_model_bytes(), M.recognition_model_bytes()
    same = OcrEngine(detection_model=Model.load_bytes(dbuf), recognition_model=Model.load_bytes(rbuf))
    assert as_bytes(same.measure(inp)) == as_bytes(eng.measure(inp))
    if _lib.device_count() >= 2:
        other = OcrEngine(detection_model=Model.load_bytes(dbuf, device=1), recognition_model=Model.load_bytes(rbuf, device=1))
        refused(lambda: other.measure(inp))


# ------------------------------------------------------------------ 4. what the measured scale does to detection
def test_detection_of_an_enlarged_page_is_not_worse_with_the_measured_scale(eng, text_page):
    """DESIGN.md §7.14 records the counts: of the native page's word boxes, how many each run on the page enlarged x 2 gives
    back within 2 pixels (centre and both sides, after rescale_rects to the native frame).  Measured on an MI355X: 182 native
    boxes; 39 recovered as given, 140 with the measured scale (the synthetic detector; a trained one is uncalibrated)."""
    inp, grey = text_page
    native = eng.detect_words(inp)
    big = eng.resize(inp, (1024, 1024))
    assert eng.text_scale(big).text_height == 28

    def recovered(rects):
        back = rescale_rects(rects, (1024, 1024), (512, 512))
        n = 0
        for r in native:
            d = np.abs(back[:, [0, 1, 4, 5]] - r[[0, 1, 4, 5]]).max(axis=1) if len(back) else np.array([np.inf])
            n += bool(d.min() <= 2.0)
        return n

    as_given, measured = recovered(eng.detect_words(big)), recovered(eng.detect_words(big, work_text_height=True))
    print("detection effect: %d native boxes; recovered as given %d, with the measured scale %d" % (len(native), as_given, measured))
    assert len(native) > 50 and measured >= as_given


def test_cli_measure(tmp_path, monkeypatch, capsys):
    from PIL import Image

    from ocrs_amd import cli, models
    px = synth.synthetic_page(9, 300, 400, lines=12, columns=1)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    Image.fromarray(np.full((60, 80, 3), 255, np.uint8)).save(str(tmp_path / "blank.png"))
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("measure", "plain", "work", "blank")}
    assert cli.main([path, "--measure", "-j", "-o", files["measure"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    assert cli.main([path, "--work-text-height", "21", "-j", "--detection-confidence", "-o", files["work"]]) == 0
    assert cli.main([str(tmp_path / "blank.png"), "--measure", "--work-text-height", "-j", "-o", files["blank"]]) == 0
    capsys.readouterr()
    assert cli.main([path, "--measure", "-o", str(tmp_path / "text.txt")]) == 0
    assert "Measure: strokes of " in capsys.readouterr().out
    for bad in (["--work-text-height", "20", "--work-scale", "0.5"], ["--work-text-height", "--work-max-side", "300"], ["--work-text-height", "-3"], ["--work-text-height", "0"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    docs = {k: json.load(open(v, encoding="utf-8")) for k, v in files.items()}
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))
    info = MR.measure(image_of(inp))
    ref = MR.choose(info)
    want = {"stroke": ref["stroke"], "text_height": ref["text_height"], "support": ref["support"], "blank": False, "ink": info["ink"], "components": info["components"]}
    assert docs["measure"]["measure"] == want and docs["work"]["measure"] == want and ref["text_height"] > 8
    assert "measure" not in docs["plain"] and {k: v for k, v in docs["measure"].items() if k != "measure"} == docs["plain"], "--measure changes nothing else"
    words = eng.detect_words(inp, work_size=work_size((300, 400), scale=work_scale_for_text(ref["text_height"], 21)))
    lines = eng.find_text_lines(inp, words)
    assert [ln["text"] for ln in docs["work"]["paragraphs"][0]["lines"]] == [str(t) for t in eng.recognize_text(inp, lines) if t is not None]
    assert docs["blank"]["measure"] == {"stroke": 0, "text_height": 0, "support": 0, "blank": True, "ink": 0, "components": 0}
