"""Quarter turns and auto-orientation on the GPU, bit for bit against tests/orient_ref.py.

The turn is compared with np.rot90 as 32-bit words on pages of random bits; a turned page is compared, through every stage,
with a page prepared from numpy-turned pixels; detect_orientation is compared with the restatement computed through the
public calls on numpy-turned pixels.

Run with:  python -m pytest tests -m gpu
"""
import json
import threading

import numpy as np
import pytest

import models_util as M
import orient_ref as R
from ocrs_amd import DecodeMethod, DimOrder, ImageSource, Model, OcrEngine, _lib, output, synth, unrotate_lines

pytestmark = pytest.mark.gpu
BENCH_PAGE = (0, 1024, 1024, 80, 2)   # bench.py's page: synth.synthetic_page(seed, 1024, 1024, lines=80)
SMALL_PAGE = (30, 600, 800, 24, 1)
SIZES = [(1, 1), (1, 300), (300, 1), (2, 3), (63, 65), (64, 64), (65, 63), (127, 129), (97, 211),
         (70, 256), (70, 257), (70, 258), (70, 259), (1024, 1024)]
KS = range(-1, 5)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def models():
    return M.detection_model_bytes(), M.recognition_model_bytes()


@pytest.fixture(scope="module")
def eng(models):
    return OcrEngine(detection_model=Model.load_bytes(models[0]), recognition_model=Model.load_bytes(models[1]))


@pytest.fixture(scope="module")
def beam_eng(models):
    return OcrEngine(detection_model=Model.load_bytes(models[0]), recognition_model=Model.load_bytes(models[1]),
                     decode_method=DecodeMethod.BeamSearch(8))


def prepare(engine, px):
    return engine.prepare_input(ImageSource.from_tensor(np.ascontiguousarray(px), DimOrder.Hwc))


def words_of(page):
    """The page's image as 32-bit words [h, w]."""
    return np.ascontiguousarray(page.image()[0]).view(np.uint32)


# ------------------------------------------------------------------ 1. the kernel
def bits_page(seed, h, w):
    """[h, w] float32 of random bits, with NaNs (quiet and signalling, with payloads), infinities and -0.0 planted."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, size=(h, w), dtype=np.uint64).astype(np.uint32)
    planted = np.array([0x7FC12345, 0xFFA00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], np.uint32)
    flat = bits.reshape(-1)
    at = rng.choice(flat.size, size=min(flat.size, len(planted)), replace=False)
    flat[at] = planted[:len(at)]
    return bits.view(np.float32)


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_rotate_equals_rot90_on_random_bits(eng, hw):
    src = bits_page(hw[0] * 1000 + hw[1], *hw)
    inp = eng.input_from_grey(src)
    assert words_of(inp).tobytes() == src.view(np.uint32).tobytes()
    for k in KS:
        out = eng.rotate(inp, k)
        exp = np.rot90(src.view(np.uint32), k)
        assert out.shape == (1,) + exp.shape, (k, out.shape)
        got = words_of(out)
        if got.tobytes() != np.ascontiguousarray(exp).tobytes():
            bad = np.argwhere(got != exp)
            raise AssertionError("k = %d: %d of %d words differ; first at %s: got %#x, expected %#x"
                                 % (k, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])]))


def test_mixed_batch_equals_each_page_alone(eng):
    sizes = [(97, 211), (64, 64), (300, 1), (70, 258), (129, 127), (200, 260)]
    ks = [1, 2, 3, 0, -1, 6]
    srcs = [bits_page(7 + i, *hw) for i, hw in enumerate(sizes)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    batch = eng.rotate_batch(inputs, ks)
    for src, inp, k, out in zip(srcs, inputs, ks, batch):
        exp = np.ascontiguousarray(np.rot90(src.view(np.uint32), k))
        assert words_of(out).tobytes() == exp.tobytes(), (src.shape, k)
        assert words_of(eng.rotate(inp, k)).tobytes() == exp.tobytes(), (src.shape, k)
    assert eng.rotate_batch([], []) == []
    with pytest.raises(ValueError):
        eng.rotate_batch(inputs, ks[:2])


EDGE_SIZES = [(1, 1), (63, 65), (64, 64), (65, 63), (130, 7)]   # a page boundary inside, on and just past a 64-tile edge


def test_edge_sized_batch_equals_each_page_alone(eng):
    """One launch over pages that end inside, on and just past a tile edge, with and without 16-byte accesses (64 x 64 at an
    even k takes them, 130 x 7 cannot), each by its own k: every page is the page turned alone, bit for bit."""
    ks = [5, 1, 2, 3, 0]
    srcs = [bits_page(70 + i, *hw) for i, hw in enumerate(EDGE_SIZES)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    for src, inp, k, out in zip(srcs, inputs, ks, eng.rotate_batch(inputs, ks)):
        assert words_of(out).tobytes() == words_of(eng.rotate(inp, k)).tobytes(), (src.shape, k)
        assert words_of(out).tobytes() == np.ascontiguousarray(np.rot90(src.view(np.uint32), k)).tobytes(), (src.shape, k)


def test_source_is_unchanged_and_outlives_the_turned_page(eng):
    src = bits_page(99, 131, 70)
    inp = eng.input_from_grey(src)
    for k in (0, 1):
        out = eng.rotate(inp, k)
        assert words_of(inp).tobytes() == src.view(np.uint32).tobytes()
        del out   # ocrs_page_free of the turned page: the source is a page of its own (k = 0 included)
        assert words_of(inp).tobytes() == src.view(np.uint32).tobytes()
        again = eng.rotate(inp, k)
        assert words_of(again).tobytes() == np.ascontiguousarray(np.rot90(src.view(np.uint32), k)).tobytes()
    out = eng.rotate(inp, 0)
    del inp   # ... and the other way round
    assert words_of(out).tobytes() == src.view(np.uint32).tobytes()


# ------------------------------------------------------------------ 2. the turn commutes with prepare_input
@pytest.fixture(scope="module")
def bench_px():
    return synth.synthetic_page(*BENCH_PAGE)


@pytest.fixture(scope="module")
def small_px():
    return synth.synthetic_page(*SMALL_PAGE)


def test_rotate_commutes_with_prepare_input(eng, bench_px):
    odd = synth.synthetic_page(5, 301, 403, 10, 1)
    for px in (bench_px, odd):
        inp = prepare(eng, px)
        for k in KS:
            assert words_of(eng.rotate(inp, k)).tobytes() == words_of(prepare(eng, np.rot90(px, k))).tobytes(), (px.shape, k)


# ------------------------------------------------------------------ 3. a turned page is an ordinary page
def pack(lines):
    offs = [0]
    for l in lines:
        offs.append(offs[-1] + len(l))
    rects = np.concatenate([np.asarray(l, np.float32).reshape(-1, 6) for l in lines]) if lines else np.zeros((0, 6), np.float32)
    return rects, np.array(offs, np.uintp), np.array([0, len(lines)], np.uintp)


def raw(engine, inp, lines, rectify=False):
    """recognize_text_batch_raw(scores=True) as bytes: chars with boxes, char offsets, char log-probs, line scores."""
    rects, lo, plo = pack(lines)
    out = engine.recognize_text_batch_raw([inp], rects, lo, plo, scores=True, rectify=rectify)
    return tuple(np.ascontiguousarray(a).tobytes() for a in out), len(out[0])


@pytest.mark.parametrize("k", [1, 2, 3])
def test_every_stage_on_a_turned_page_equals_the_page_of_turned_pixels(eng, beam_eng, bench_px, k):
    for engine in (eng, beam_eng):
        a, b = engine.rotate(prepare(engine, bench_px), k), prepare(engine, np.rot90(bench_px, k))
        wa, wb = engine.detect_words(a), engine.detect_words(b)
        assert wa.tobytes() == wb.tobytes() and len(wa) > 20, k
        la, lb = engine.find_text_lines(a, wa), engine.find_text_lines(b, wb)
        assert len(la) == len(lb) and all(x.tobytes() == y.tobytes() for x, y in zip(la, lb))
        for rectify in (False, True):
            ra, na = raw(engine, a, la, rectify)
            rb, nb = raw(engine, b, lb, rectify)
            assert ra == rb, (k, rectify)
            if k == 2:   # upside down the lines are still lines: something is read (what, the scores of §4 are for)
                assert na > 0


# ------------------------------------------------------------------ 4. detect_orientation
class Restatement:
    """detect_orientation restated through the public calls on numpy-turned pixels; detection and layout are cached per
    (page, turn)."""

    def __init__(self, engine):
        self.eng = engine
        self.cache = {}

    def lines(self, name, px, turn):
        key = (name, turn % 4)
        if key not in self.cache:
            inp = prepare(self.eng, np.rot90(px, turn))
            words = self.eng.detect_words(inp)
            self.cache[key] = (inp, words, self.eng.find_text_lines(inp, words))
        return self.cache[key]

    def expected(self, name, px, j, max_lines):
        """For the page np.rot90(px, j): (vote, candidates, scores [4], n_chars [4], chosen turn)."""
        _, words, _ = self.lines(name, px, j)
        vote = R.vote(words)
        cands = R.candidates(vote)
        scores, n_chars = np.full(4, np.nan, np.float64), np.zeros(4, np.uint32)
        for k in cands:
            inp, _, lines = self.lines(name, px, j + k)
            picked = [lines[i] for i in R.sample_lines(lines, max_lines)]
            texts = self.eng.recognize_text(inp, picked, scores=True)
            scores[k], n_chars[k] = R.score([[c.logp for c in t.chars()] for t in texts if t is not None])
        return vote, cands, scores, n_chars, R.choose(cands, scores)


@pytest.fixture(scope="module")
def restatement(eng):
    return Restatement(eng)


@pytest.mark.parametrize("j", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["bench", "small"])
def test_detect_orientation_equals_the_restatement(eng, restatement, bench_px, small_px, name, j):
    px = bench_px if name == "bench" else small_px
    inp = restatement.lines(name, px, j)[0]
    for max_lines in (0, 1, 8):
        vote, cands, scores, n_chars, turn = restatement.expected(name, px, j, max_lines)
        got = eng.detect_orientation(inp, max_lines=max_lines)
        print("%s j=%d max_lines=%d: vote %s scores %s chars %s -> %d" % (name, j, max_lines, got.vote, got.scores, got.n_chars, got.quarter_turns))
        assert got.vote.tobytes() == vote.tobytes(), (got.vote, vote)
        assert cands == ((0, 2) if j % 2 == 0 else (1, 3))
        assert got.scores.view(np.uint64).tolist() == scores.view(np.uint64).tolist(), (max_lines, got.scores, scores)
        assert got.n_chars.tolist() == n_chars.tolist(), (max_lines, got.n_chars, n_chars)
        assert np.isnan(got.scores[[k for k in range(4) if k not in cands]]).all()
        assert got.quarter_turns == turn
        if max_lines == 0:
            assert min(n_chars[list(cands)]) > 0, "both candidates read something: the scores decide"
    assert eng.detect_orientation(inp).scores.tobytes() == eng.detect_orientation(inp, max_lines=8).scores.tobytes()


def test_blank_page_reads_as_given(eng):
    inp = prepare(eng, np.full((300, 400, 3), 255, np.uint8))
    got = eng.detect_orientation(inp)
    assert got.quarter_turns == 0 and got.vote.tolist() == [0.0, 0.0] and got.n_chars.tolist() == [0, 0, 0, 0]
    assert got.scores[0] == -np.inf and got.scores[2] == -np.inf and np.isnan(got.scores[1]) and np.isnan(got.scores[3])


def test_get_text_with_orientation(eng, small_px):
    inp = prepare(eng, np.rot90(small_px, 1))
    for k in (0, 3, -1):
        assert eng.get_text(inp, orientation=k) == eng.get_text(eng.rotate(inp, k))
    auto = eng.detect_orientation(inp).quarter_turns
    assert eng.get_text(inp, orientation="auto") == eng.get_text(eng.rotate(inp, auto))
    assert eng.get_text(inp, orientation=None) == eng.get_text(inp)


# ------------------------------------------------------------------ 5. beside other traffic
def test_detect_orientation_beside_plain_traffic(eng):
    pages = [synth.synthetic_page(30 + i, 600, 800, 24, 1) for i in range(4)]
    turned = [prepare(eng, np.rot90(p, i)) for i, p in enumerate(pages)]
    plain = [prepare(eng, p) for p in pages]

    def probe(i):
        o = eng.detect_orientation(turned[i])
        return (o.quarter_turns, o.vote.tobytes(), o.scores.tobytes(), o.n_chars.tobytes())

    def read(i):
        words = eng.detect_words(plain[i])
        lines = eng.find_text_lines(plain[i], words)
        return (words.tobytes(),) + raw(eng, plain[i], lines)[0]

    quiet_probe, quiet_read = [probe(i) for i in range(4)], [read(i) for i in range(4)]
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, probe(i) if t < 4 else read(i))
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
        assert got == (quiet_probe[i] if t < 4 else quiet_read[i]), "thread %d call %d" % (t, r)


# ------------------------------------------------------------------ 6. the CLI
def test_cli_orientation(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    upright = synth.synthetic_page(3, 256, 384, lines=8, columns=1)
    px = np.ascontiguousarray(np.rot90(upright, 3))   # the file: the page turned by 270 degrees
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    fixed, auto, plain = (str(tmp_path / n) for n in ("fixed.json", "auto.json", "plain.json"))
    assert cli.main([path, "--orientation", "90", "-j", "-o", fixed]) == 0
    assert cli.main([path, "--orientation", "auto", "-j", "-o", auto]) == 0
    assert cli.main([path, "-j", "-o", plain]) == 0
    engine = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                       recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = prepare(engine, cli.load_image(path))
    hw = px.shape[:2]

    def explicit(k):
        page = inp if k is None else engine.rotate(inp, k)
        lines = engine.find_text_lines(page, engine.detect_words(page))
        texts = engine.recognize_text(page, lines)
        if k is None:
            return texts, output.format_json_output(path, hw, texts)
        back = unrotate_lines(texts, hw, k)
        return back, output.format_json_output(path, hw, back, orientation=90 * k)

    texts, doc = explicit(1)
    assert doc == open(fixed, encoding="utf-8").read()
    parsed = json.loads(doc)
    assert parsed["orientation"] == 90 and parsed["image_height"] == hw[0] and parsed["image_width"] == hw[1]
    assert len([t for t in texts if t is not None]) >= 4
    # the turned page is the upright one: what is read there, boxes mapped back, lies inside the file's frame ...
    upright_texts = engine.recognize_text(prepare(engine, upright), engine.find_text_lines(None, engine.detect_words(prepare(engine, upright))))
    assert [str(t) for t in texts if t is not None] == [str(t) for t in upright_texts if t is not None]
    for t in texts:
        if t is not None:
            top, left, bottom, right = t.bounding_rect()
            assert -1 <= top <= bottom <= hw[0] and -1 <= left <= right <= hw[1]   # an exclusive bound at the page's edge maps to -1
            assert bottom - top > right - left, "a line of the upright page runs down the file"
    k_auto = engine.detect_orientation(inp).quarter_turns
    assert explicit(k_auto)[1] == open(auto, encoding="utf-8").read()
    assert json.loads(open(auto, encoding="utf-8").read())["orientation"] == 90 * k_auto
    # ... and without the flag nothing changes
    plain_doc = open(plain, encoding="utf-8").read()
    assert explicit(None)[1] == plain_doc and "orientation" not in json.loads(plain_doc)
