"""Page deskew on the GPU, bit for bit against tests/deskew_ref.py.

Pages are put on the device with input_from_grey.  Scores are compared as integers (uint64).  Warped pages are compared as
32-bit words, NaN positions equal (a NaN compares as NaN, not by payload: arithmetic on a NaN keeps its being one, not its
bits).

Run with:  python -m pytest tests -m gpu
"""
import json
import threading

import numpy as np
import pytest

import deskew_ref as D
import models_util as M
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, output, synth
import ocrs_amd

pytestmark = pytest.mark.gpu
# (height, width): one pixel, one row, one column, two rows; around one 64 x 64 tile either way; several tiles with partial
# edges; a work page
SHAPES = [(1, 1), (1, 300), (300, 1), (2, 3), (63, 65), (64, 64), (65, 63), (127, 129), (97, 211), (1024, 768)]
EXTREMES = np.array([[0, 65536], [65536, 0], [-65536, 0], [0, -65536], [46341, 46341], [-46341, 46341], [65536, 65536], [-65536, -65536]],
                    np.int32)


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


def noise(seed, h, w, plant=True):
    """[h, w] float32, uniform in [-0.6, 0.6) (a tenth of it clamps either way); plant: see planted()."""
    rng = np.random.default_rng(seed)
    a = ((rng.random((h, w), dtype=np.float32) - np.float32(0.5)) * np.float32(1.2)).astype(np.float32)
    return planted(a, seed) if plant else a


def random_bits(seed, h, w):
    """Every bit random: a 256th of the pixels are NaN or infinite, most of the rest clamp."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(h, w), dtype=np.uint64).astype(np.uint32).view(np.float32)


def tables():
    return {"0": D.skew_table(0, 1, 0.1), "+-0.1": D.skew_table(-1, 3, 0.1), "+-15": np.concatenate([D.skew_table(5 * k, 1, 0.1) for k in range(-30, 31)]),
            "+-45": D.skew_table(-100, 200, 0.45), "extremes": EXTREMES}


def check_scores(eng, page, table, what):
    got = eng.skew_scores([eng.input_from_grey(page)], table)
    assert got.dtype == np.uint64 and got.shape == (1, len(table))
    exp = D.skew_scores(page, table)
    assert [int(v) for v in got[0]] == exp, (what, [(i, int(g), e) for i, (g, e) in enumerate(zip(got[0], exp)) if int(g) != e][:4])
    return got[0]


# ------------------------------------------------------------------ 1. the skew scores
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_scores_equal_the_restatement(eng, shape):
    h, w = shape
    T = tables()
    assert [len(T[k]) for k in ("0", "+-15", "+-45")] == [1, 61, 200]
    big = h * w > 100000   # the restatement takes a second per sixty angles there
    page = noise(h * 1000 + w, h, w)
    for name in (("0", "+-0.1", "+-15", "extremes") if big else T):
        check_scores(eng, page, T[name], "noise %s" % name)
    if not big:
        bits = random_bits(h * 1000 + w + 1, h, w)
        for name in ("+-0.1", "+-45", "extremes"):
            check_scores(eng, bits, T[name], "random bits %s" % name)


def test_scores_of_a_striped_page_peak_at_its_angle(eng):
    h, w = 300, 400
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    th = np.deg2rad(3.0)
    page = np.where(np.mod(x * np.sin(th) + y * np.cos(th), 11.0) < 4.4, -0.3, 0.35).astype(np.float32)
    table = tables()["+-15"]
    s = check_scores(eng, page, table, "stripes")
    assert int(np.argmax(s)) == 30 + 6 and s.max() > 2 * np.sort(s)[-3]
    flat = check_scores(eng, np.full((70, 90), 0.25, np.float32), table, "flat")
    assert not flat.any()


def test_a_mixed_batch_equals_each_page_alone(eng):
    shapes = [(97, 211), (1, 1), (64, 64), (300, 1), (127, 129), (65, 63)]
    pages = [noise(50 + i, h, w) for i, (h, w) in enumerate(shapes)]
    inputs = [eng.input_from_grey(p) for p in pages]
    table = tables()["+-15"]
    batch = eng.skew_scores(inputs, table)
    assert batch.shape == (6, 61)
    for i, p in enumerate(pages):
        assert np.array_equal(batch[i], eng.skew_scores([inputs[i]], table)[0]), shapes[i]
        assert [int(v) for v in batch[i]] == D.skew_scores(p, table), shapes[i]
    assert eng.skew_scores([], table).shape == (0, 61)


def test_twenty_repeats_are_equal(eng):
    inp = eng.input_from_grey(noise(77, 200, 333))
    table = tables()["+-45"]
    first = eng.skew_scores([inp], table)
    for _ in range(19):
        assert np.array_equal(eng.skew_scores([inp], table), first)


def test_score_refusals(eng):
    inp = eng.input_from_grey(noise(1, 4, 4))
    ok = np.array([[0, 65536]], np.int32)
    for bad in ([[65537, 0]], [[0, -65537]], [[0, 65536], [2 ** 31 - 1, 0]]):
        with pytest.raises(_lib.OcrsError) as ei:
            eng.skew_scores([inp], np.array(bad, np.int32))
        assert ei.value.status_name == "INVALID_ARGUMENT", bad
    with pytest.raises(_lib.OcrsError) as ei:
        eng.skew_scores([inp], np.zeros((0, 2), np.int32))
    assert ei.value.status_name == "INVALID_ARGUMENT"
    for hw in ((1, 4097), (4097, 1)):
        with pytest.raises(_lib.OcrsError) as ei:
            eng.skew_scores([eng.input_from_grey(np.zeros(hw, np.float32))], ok)
        assert ei.value.status_name == "INVALID_ARGUMENT", hw
    assert eng.skew_scores([eng.input_from_grey(np.zeros((1, 4096), np.float32))], ok).tolist() == [[0]]
    assert eng.skew_scores([inp], ok).shape == (1, 1), "the engine works after a refusal"


def test_scoring_callers_beside_plain_callers(eng):
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    table = tables()["+-15"]

    def scored(i):
        return eng.skew_scores([pages[i]], table).tobytes()

    def plain(i):
        return eng.detect_words(pages[i]).tobytes()

    quiet_scores, quiet_plain = [scored(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        assert np.frombuffer(quiet_scores[i], np.uint64).tolist() == D.skew_scores(image_of(pages[i]), table)
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, scored(i) if t < 4 else plain(i))
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
        assert got == (quiet_scores[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)


# ------------------------------------------------------------------ 2. the warp
def assert_same_words(got, exp, what):
    assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.shape, exp.shape)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ at %s" % (what, np.argwhere(np.isnan(got) != nan)[:4].tolist())
    bad = np.argwhere((got.view(np.uint32) != exp.view(np.uint32)) & ~nan)
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r (%#x), expected %r (%#x)"
                             % (what, len(bad), got.size, at, got[at], got.view(np.uint32)[at], exp[at], exp.view(np.uint32)[at]))


ODD_FILL = float(np.array([0x3EABCDEF], np.uint32).view(np.float32)[0])


def warp_maps(h, w):
    """(name, m, out_hw): the identity; rotations that hold the page and rotations that cut its corners (taps beyond all four
    edges either way: the expanded page shows fill all round, the unexpanded one reaches outside); a scale with shear."""
    out = [("identity", D.deskew_map(h, w, 0.0)[1], (h, w))]
    for a in (0.1, 3.0, -3.0, 10.0, -10.0, 45.0, -45.0):
        for expand in (True, False):
            hw, m = D.deskew_map(h, w, a, expand=expand)
            out.append(("%+g%s" % (a, " expanded" if expand else ""), m, hw))
    out.append(("scale and shear", np.array([-3.25, 0.75, 0.125, -2.5, -0.0625, 1.5], np.float32), (h + 9, w + 7)))
    return out


@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (150, 258)], ids=lambda s: "%dx%d" % s)
def test_warp_equals_the_restatement(eng, shape):
    h, w = shape
    page = noise(h * 7 + w, h, w)
    inp = eng.input_from_grey(page)
    cases = warp_maps(h, w)
    fills = [0.5, -0.5, ODD_FILL]
    made = eng.warp_batch([inp] * len(cases), [m for _, m, _ in cases], [hw for _, _, hw in cases], [fills[i % 3] for i in range(len(cases))])
    for i, (name, m, hw) in enumerate(cases):
        exp = D.warp(page, m, hw, fills[i % 3])
        assert made[i].shape == (1,) + tuple(hw)
        assert_same_words(image_of(made[i]), exp, "%s fill %r" % (name, fills[i % 3]))
    # all four edges were crossed
    out = image_of(eng.warp(eng.input_from_grey(np.zeros((h, w), np.float32)), D.deskew_map(h, w, 45.0)[1], D.deskew_map(h, w, 45.0)[0], fill=0.25))
    if h > 8:
        assert all(np.any(edge == np.float32(0.25)) for edge in (out[0], out[-1], out[:, 0], out[:, -1]))


@pytest.mark.parametrize("out_w", [256, 257, 258, 259])
def test_warp_output_widths_and_fills(eng, out_w):
    """Every width % 4 (the 16-byte store needs % 4 == 0), one pixel, and a block boundary at 256 columns and 16 rows."""
    page = noise(out_w, 61, 83)
    inp = eng.input_from_grey(page)
    m = np.array([-20.5, 0.48, 0.11, -9.25, -0.07, 0.52], np.float32)
    for fill in (-0.5, 0.5, ODD_FILL):
        for hw in ((1, 1), (17, out_w), (1, out_w), (33, out_w + 256)):
            assert_same_words(image_of(eng.warp(inp, m, hw, fill=fill)), D.warp(page, m, hw, fill), "%s fill %r" % (hw, fill))
    # positions that are far away, huge or not finite read as fill
    far = np.array([1e30, 1.0, 0.0, -1e30, 0.0, 1.0], np.float32)
    assert_same_words(image_of(eng.warp(inp, far, (5, out_w), fill=0.125)), D.warp(page, far, (5, out_w), 0.125), "far")
    huge = np.array([0.0, 3e38, 3e38, 0.0, 3e38, 3e38], np.float32)
    assert_same_words(image_of(eng.warp(inp, huge, (5, out_w), fill=0.125)), D.warp(page, huge, (5, out_w), 0.125), "overflowing")


def test_warp_mixed_batch_and_lifetimes(eng):
    shapes = [(97, 211), (1, 1), (64, 64), (300, 5), (40, 256)]
    pages = [noise(90 + i, h, w, plant=i % 2 == 0) for i, (h, w) in enumerate(shapes)]
    inputs = [eng.input_from_grey(p) for p in pages]
    maps = [D.deskew_map(h, w, a) for (h, w), a in zip(shapes, (3.0, 10.0, -45.0, -3.0, 0.1))]
    fills = [0.5, -0.5, ODD_FILL, 0.0, 0.5]
    made = eng.warp_batch(inputs, [m for _, m in maps], [hw for hw, _ in maps], fills)
    exps = [D.warp(p, m, hw, f) for p, (hw, m), f in zip(pages, maps, fills)]
    for i in range(5):
        assert_same_words(image_of(made[i]), exps[i], "batch %d" % i)
        assert_same_words(image_of(eng.warp(inputs[i], maps[i][1], maps[i][0], fill=fills[i])), exps[i], "alone %d" % i)
    assert eng.warp_batch([], [], []) == []
    # the warped page and its source are independent: either is alive after the other is freed
    keep = made[0]
    del inputs[0]
    assert_same_words(image_of(keep), exps[0], "the warped page after its source was freed")
    src = eng.input_from_grey(pages[1])
    w2 = eng.warp(src, maps[1][1], maps[1][0])
    del w2
    assert image_of(src).tobytes() == pages[1].tobytes(), "the source after its warped page was freed"
    for bad_hw in ((0, 5), (5, 65536)):
        with pytest.raises(_lib.OcrsError) as ei:
            eng.warp(src, maps[1][1], bad_hw)
        assert ei.value.status_name == "INVALID_ARGUMENT"
    with pytest.raises(_lib.OcrsError):
        eng.warp(src, np.array([np.nan, 1, 0, 0, 0, 1], np.float32), (5, 5))


# ------------------------------------------------------------------ 3. the estimate and the whole chain
@pytest.fixture(scope="module")
def bench_grey(eng):
    """The bench page, prepared; and the page skewed by +3 and by -10 degrees by the RESTATEMENT's warp (turning the content
    counter-clockwise by t is the deskew of -t), paper around it."""
    px = synth.synthetic_page(0, 1024, 1024, lines=80)
    grey = image_of(eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc)))
    skewed = {}
    for t in (3.0, -10.0):
        hw, m = D.deskew_map(1024, 1024, -t)
        skewed[t] = D.warp(grey, m, hw, float(grey.max()))
    return grey, skewed


@pytest.mark.parametrize("turn", [3.0, -10.0])
def test_estimate_skew_equals_the_restatement(eng, bench_grey, turn):
    page = bench_grey[1][turn]
    inp = eng.input_from_grey(page)
    sk = eng.estimate_skew(inp)
    work_hw = ocrs_amd.work_size(page.shape, max_side=1024)
    assert sk.work_hw == work_hw and max(work_hw) == 1024 < max(page.shape)
    work = image_of(eng.resize(inp, work_hw, filter="area"))
    assert work.tobytes() == D.work_page(page).tobytes()
    # the restatement's search over the library's primitive, then over its own
    lib_e = D.estimate(work, scores=lambda p, t: eng.skew_scores([eng.input_from_grey(p)], t)[0])
    ref_e = D.estimate(work)
    for e in (lib_e, ref_e):
        assert (sk.angle, sk.coarse_index, sk.fine_index, sk.scores) == (e["angle"], e["coarse_index"], e["fine_index"], e["scores"])
    assert abs(sk.angle - turn) <= 0.1 + 1e-9, "and it is the angle the page was turned by"
    assert sk.scores[0] > sk.scores[1]
    small = eng.estimate_skew(inp, work_max_side=512, max_deg=12.0, coarse_step_deg=1.0, fine_step_deg=0.25)
    e = D.estimate(D.work_page(page, 512), {"work_max_side": 512, "max_deg": 12.0, "coarse_step_deg": 1.0, "fine_step_deg": 0.25})
    assert (small.angle, small.scores, small.work_hw) == (e["angle"], e["scores"], e["work_hw"])


def test_a_blank_page_has_angle_zero_and_is_not_warped(eng):
    for page in (np.full((300, 200), 0.5, np.float32), np.full((40, 2000), np.nan, np.float32)):
        inp = eng.input_from_grey(page)
        sk = eng.estimate_skew(inp)
        assert sk.angle == 0.0 and sk.fine_index == 0 and sk.scores == (0, 0, 0)
        out, m, angle = eng.deskew(inp)
        assert out is inp and angle == 0.0 and m.tolist() == [-0.5, 1.0, 0.0, -0.5, 0.0, 1.0]
    with pytest.raises(_lib.OcrsError) as ei:
        eng.estimate_skew(inp, max_deg=50.0)
    assert ei.value.status_name == "INVALID_ARGUMENT"


def test_get_text_with_deskew_is_the_manual_chain(eng, bench_grey):
    grey, skewed = bench_grey
    page = skewed[3.0]
    inp = eng.input_from_grey(page)
    # by hand, through the public calls
    sk = eng.estimate_skew(inp)
    out_hw, m = ocrs_amd.deskew_map(page.shape, sk.angle)
    upright = eng.warp(inp, m, out_hw, fill=0.5)
    assert_same_words(image_of(upright), D.warp(page, D.deskew_map(page.shape[0], page.shape[1], sk.angle)[1], out_hw, 0.5), "the upright page")
    words = eng.detect_words(upright)
    lines = eng.find_text_lines(upright, words)
    texts = eng.recognize_text(upright, lines)
    text = "\n".join(str(t) for t in texts if t is not None)
    assert len(lines) > 0 and eng.get_text(inp, deskew="auto") == text
    assert eng.get_text(inp, deskew=sk.angle) == text
    assert eng.get_text(inp, deskew=sk.angle, rectify=True) == eng.get_text(upright, rectify=True)
    assert eng.get_text(inp, deskew=None) == eng.get_text(inp)
    assert eng.get_text(inp, deskew=0.1) == eng.get_text(inp), "under min_deg the page is left alone"
    got, gm, ga = eng.deskew(inp)
    assert ga == sk.angle and gm.tobytes() == m.tobytes() and image_of(got).tobytes() == image_of(upright).tobytes()
    # the words of the upright page are those of the bench page, and come back to where the skewed page shows them
    straight = eng.detect_words(eng.input_from_grey(grey))
    print("%d words on the upright page, %d on the bench page, %d on the skewed page" % (len(words), len(straight), len(eng.detect_words(inp))))
    assert len(words) > 0
    back = ocrs_amd.unwarp_rects(words, m)
    assert back.view(np.uint32).tobytes() == D.unwarp_rects(words, m).view(np.uint32).tobytes()
    assert np.all(back[:, 0] > -1) and np.all(back[:, 0] < page.shape[1]) and np.all(back[:, 1] > -1) and np.all(back[:, 1] < page.shape[0])
    def bearing(up):
        return np.rad2deg(np.arctan2(up[:, 0].astype(np.float64), -up[:, 1].astype(np.float64)))

    turned = (bearing(back[:, 2:4]) - bearing(words[:, 2:4]) + 180.0) % 360.0 - 180.0
    assert np.all(np.abs(turned + sk.angle) < 1e-3), "every up vector is turned by the page's skew"
    assert np.allclose(back[:, 4:], words[:, 4:], rtol=1e-6), "a rotation keeps sizes"
    lines_back = ocrs_amd.unwarp_lines(texts, m)
    assert [None if t is None else str(t) for t in lines_back] == [None if t is None else str(t) for t in texts]
    boxes = np.array([c.rect for t in texts if t is not None for c in t.chars()], np.int32).reshape(-1, 4)
    got_boxes = np.array([c.rect for t in lines_back if t is not None for c in t.chars()], np.int32).reshape(-1, 4)
    assert len(boxes) > 0 and np.array_equal(got_boxes, D.unwarp_boxes(boxes, m))


def test_cli_deskew(tmp_path, monkeypatch, bench_grey, capsys):
    from PIL import Image

    from ocrs_amd import cli, models
    px8 = np.clip((bench_grey[1][3.0] + np.float32(0.5)) * np.float32(255.0), 0, 255).astype(np.uint8)
    path = str(tmp_path / "page.png")
    Image.fromarray(px8, "L").save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("auto", "three", "plain")}
    assert cli.main([path, "--deskew", "auto", "-j", "--detection-confidence", "--debug", "-o", files["auto"]]) == 0
    assert "Skew: " in capsys.readouterr().out
    assert cli.main([path, "--deskew", "3", "--deskew-fill", "0.5", "-j", "-o", files["three"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in (["--deskew-fill", "0.5"], ["--deskew", "sideways"], ["--deskew", "60"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))
    hw = px8.shape[:2]
    plain = output.format_json_output(path, hw, eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "skew" not in json.loads(plain), "without the flag nothing changes"
    upright, m, angle = eng.deskew(inp, 3.0)
    lines = eng.find_text_lines(upright, eng.detect_words(upright))
    exp = output.format_json_output(path, hw, ocrs_amd.unwarp_lines(eng.recognize_text(upright, lines), m), skew=3.0)
    assert text["three"] == exp
    doc = json.loads(text["auto"])
    assert doc["skew"] == eng.estimate_skew(inp).angle and abs(doc["skew"] - 3.0) <= 0.1 + 1e-9
    assert (doc["image_height"], doc["image_width"]) == hw
    got_lines = doc["paragraphs"][0]["lines"]
    assert len(got_lines) > 0
    for line in got_lines:   # vertices and word boxes are in the frame of the file
        for x, y in line["vertices"] + [v for b in line["word_boxes"] for v in b["vertices"]]:
            assert -16 <= x <= hw[1] + 16 and -16 <= y <= hw[0] + 16
