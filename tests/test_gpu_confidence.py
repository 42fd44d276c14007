"""Recognition confidence on the GPU (DESIGN.md "Recognition confidence"): per-char log-probs and line scores of the
scored entry points (ocrs_engine_recognize_text[_batch]_scored, ocrs_ctc_beam_search_scored impl 2) against values
computed from the oracle's log-probs by the definitions (confidence_ref.py), bit for bit, through every route a
recognition request takes: one packed batch, the two-stream long / short split, sub-requests, the coalescer, beam
search on the GPU and on the host, and a caller-implemented (`trait Model`) recognition model.  Scoring must not
change anybody's chars.

Run with:  python -m pytest tests -m gpu
"""
import gc
import json
import math
import threading

import numpy as np
import pytest

import confidence_ref as CR
import kat_util as K
import models_util as M
from ocrs_amd import DecodeMethod, DimOrder, ImageSource, Model, OcrEngine, _lib, output, synth
from test_confidence_cpu import MATRICES
from test_gpu_recognition_logits import PAGE_HW, Case, _rect, sweep_lines

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _pack(lines_per_page):
    all_lines = [l for lines in lines_per_page for l in lines]
    plo = [0]
    for lines in lines_per_page:
        plo.append(plo[-1] + len(lines))
    offs = [0]
    for l in all_lines:
        offs.append(offs[-1] + len(l))
    rects = np.concatenate([np.asarray(l, np.float32).reshape(-1, 6) for l in all_lines]) if all_lines \
        else np.zeros((0, 6), np.float32)
    return rects, np.array(offs, np.uintp), np.array(plo, np.uintp)


def raw(engine, inputs, lines_per_page, scores):
    """recognize_text_batch_raw over several pages -> per line (chars array, char_logp or None), line scores or None."""
    rects, lo, plo = _pack(lines_per_page)
    out = engine.recognize_text_batch_raw(inputs, rects, lo, plo, scores=scores)
    chars, co = out[0], out[1]
    per_line = []
    for i in range(len(co) - 1):
        a, b = int(co[i]), int(co[i + 1])
        per_line.append((chars[a:b], out[2][a:b] if scores else None))
    return per_line, (out[3] if scores else None)


def expected_greedy(case, lines):
    """Per line (steps, step log-probs, score) of greedy decoding on the oracle's masked log-probs."""
    excl = case.ora.excluded_char_labels
    return [CR.greedy(CR.masked(e, excl)) for e in case.oracle(lines)]


def check_against(what, per_line, scores, exp):
    """Scored output == the definitions on the oracle's log-probs: line scores bit for bit, every char's logp the
    step's (chars are the first steps of the line: steps starting in the padding form a suffix and are dropped)."""
    assert len(per_line) == len(exp) == len(scores), what
    for i, ((chars, clp), (steps, slp, score)) in enumerate(zip(per_line, exp)):
        assert CR.bits_equal(scores[i], score), "%s: line %d: score %r, expected %r" % (what, i, scores[i], score)
        n = len(chars)
        assert n <= len(steps), (what, i)
        assert clp.dtype == np.float32 and np.array_equal(clp, slp[:n]), "%s: line %d: char log-probs" % (what, i)


def assert_same(what, a, b):
    """Two raw() results equal: chars, char log-probs and line scores (bit for bit)."""
    (pa, sa), (pb, sb) = a, b
    assert len(pa) == len(pb), what
    for i, ((ca, la), (cb, lb)) in enumerate(zip(pa, pb)):
        assert np.array_equal(ca, cb), "%s: line %d: chars differ" % (what, i)
        assert (la is None and lb is None) or np.array_equal(la, lb), "%s: line %d: char log-probs differ" % (what, i)
    if sa is not None or sb is not None:
        assert sa.tobytes() == sb.tobytes(), "%s: line scores differ" % what


def assert_chars_of(what, scored, unscored):
    assert [c.tobytes() for c, _ in scored[0]] == [c.tobytes() for c, _ in unscored[0]], what


@pytest.fixture(scope="module")
def prod():
    case = Case(M.recognition_model_bytes(), synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40))
    h, w = PAGE_HW
    # every width group 50 .. 2400, plus a line over the page edge and a 0 x 0 line (no rows: score 0)
    case.lines = sweep_lines(case) + [_rect(w - 10, h - 5, 120, 20), _rect(300, 300, 0, 0)]
    case.exp = expected_greedy(case, case.lines)
    return case


# ------------------------------------------------------------------ greedy
def test_greedy_scores_equal_the_definition(prod):
    scored = raw(prod.gpu, [prod.inp], [prod.lines], True)
    unscored = raw(prod.gpu, [prod.inp], [prod.lines], False)
    assert_chars_of("sweep", scored, unscored)
    check_against("sweep", *scored, prod.exp)
    assert CR.bits_equal(scored[1][-1], 0.0)          # the 0 x 0 line
    assert sum(len(c) > 0 for c, _ in scored[0]) >= 20
    # some line drops steps that start in the padding: their log-probs go with them
    assert any(len(c) < len(e[0]) for (c, _), e in zip(scored[0], prod.exp))


def test_greedy_scores_single_page_entry_point(prod):
    lines = prod.lines[::4]
    got = prod.gpu.recognize_text(prod.inp, lines, scores=True)
    plain = prod.gpu.recognize_text(prod.inp, lines)
    exp = prod.exp[::4]
    for i, (g, p, (steps, slp, score)) in enumerate(zip(got, plain, exp)):
        assert (g is None) == (p is None)
        if g is None:
            continue
        assert str(g) == str(p) and [c.rect for c in g.chars()] == [c.rect for c in p.chars()]
        assert p.score is None and all(c.logp is None for c in p.chars())
        assert CR.bits_equal(g.score, score), i
        assert np.array_equal(np.array([c.logp for c in g.chars()], np.float32), slp[:len(g.chars())]), i
        assert g.confidence == math.exp(math.fsum(float(c.logp) for c in g.chars()) / len(g.chars()))


def test_greedy_scores_with_allowed_chars(prod):
    case = Case(prod.rbuf, synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40), allowed_chars="0123456789.")
    lines = prod.lines[::3]
    scored = raw(case.gpu, [case.inp], [lines], True)
    assert_chars_of("allowed_chars", scored, raw(case.gpu, [case.inp], [lines], False))
    check_against("allowed_chars", *scored, expected_greedy(case, lines))
    assert sum(len(c) > 0 for c, _ in scored[0]) >= 5


# ------------------------------------------------------------------ request routes
def test_multi_page_batch_equals_single_pages(prod):
    pages = [synth.synthetic_page(s, PAGE_HW[0], PAGE_HW[1], lines=40) for s in (71, 72, 73)]
    inputs = [prod.gpu.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pages]
    lpp = [prod.lines[0::3], prod.lines[1::3], prod.lines[2::3]]
    batch = raw(prod.gpu, inputs, lpp, True)
    singles = [raw(prod.gpu, [inp], [l], True) for inp, l in zip(inputs, lpp)]
    joined = ([x for s in singles for x in s[0]], np.concatenate([s[1] for s in singles]))
    assert_same("3-page batch", batch, joined)
    assert_chars_of("3-page batch", batch, raw(prod.gpu, inputs, lpp, False))


def test_sub_requests_equal_one_request(prod):
    whole = raw(prod.gpu, [prod.inp], [prod.lines], True)
    try:
        for budget in (64 * 50, 64 * 1200 * 12):
            prod.gpu.set_option("rec_max_pixels", budget)
            assert_same("rec_max_pixels %d" % budget, raw(prod.gpu, [prod.inp], [prod.lines], True), whole)
    finally:
        prod.gpu.set_option("rec_max_pixels", 0)


def _split_lines():
    rng = np.random.default_rng(5)
    lines = []
    for i in range(72):
        ww, hh = int(rng.integers(20, 150)), int(rng.integers(16, 24))
        lines.append(_rect(20 + (i % 6) * 160 + ww / 2, 12 + (i // 6) * 26, ww, hh))
    for i in range(5):
        ww = 600 + 80 * i
        lines.append(_rect(20 + ww / 2, 400 + 30 * i, ww, 14.0))
    return lines


def test_long_short_split_equals_the_definition(prod):
    lines = _split_lines()
    logits = prod.oracle(lines)
    assert sum(e.shape[0] <= 160 for e in logits) >= 64 and sum(e.shape[0] > 160 for e in logits) == 5
    exp = [CR.greedy(CR.masked(e, None)) for e in logits]
    got = raw(prod.gpu, [prod.inp], [lines], True)
    check_against("long/short split", *got, exp)
    # parts alone (no split): the same bits
    for a, b in ((0, 40), (72, 77)):
        alone = raw(prod.gpu, [prod.inp], [lines[a:b]], True)
        assert_same("split part %d..%d" % (a, b), alone, (got[0][a:b], got[1][a:b]))


def test_coalesced_scored_and_unscored_callers(prod):
    """8 threads of one-page calls through the coalescer, scored and unscored mixed: everybody gets their solo bits."""
    eng = OcrEngine(recognition_model=Model.load_bytes(prod.rbuf))
    pages = [synth.synthetic_page(80 + k, PAGE_HW[0], PAGE_HW[1], lines=40) for k in range(4)]
    inputs = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pages]
    lpp = [prod.lines[k::4] for k in range(4)]
    try:
        eng.set_option("coalesce", 0)
        solo = {(k, s): raw(eng, [inputs[k]], [lpp[k]], s) for k in range(4) for s in (False, True)}
    finally:
        eng.set_option("coalesce", 2)
    s0 = eng.coalesce_stats()["recognize"]
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(w):
        try:
            barrier.wait()
            for r in range(6):
                k, s = (w + r) % 4, (w + r) % 2 == 0
                results[(w, r)] = (k, s, raw(eng, [inputs[k]], [lpp[k]], s))
        except Exception as e:   # pragma: no cover - reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(w,)) for w in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    s1 = eng.coalesce_stats()["recognize"]
    assert s1[1] - s0[1] == 48 and s1[0] - s0[0] < 48, (s0, s1)   # calls were merged
    for (w, r), (k, s, got) in results.items():
        assert_same("thread %d call %d" % (w, r), got, solo[(k, s)])
        if not s:
            assert all(lp is None for _, lp in got[0]) and got[1] is None
    for k in range(4):
        assert_chars_of("page %d" % k, solo[(k, True)], solo[(k, False)])


# ------------------------------------------------------------------ beam search
@pytest.mark.parametrize("name,lp,w", MATRICES, ids=[m[0] for m in MATRICES])
def test_beam_hook_gpu_equals_host(name, lp, w):
    (s2, c2, l2), (s0, c0, l0) = _lib.ctc_beam_search_scored(lp, w, 2), _lib.ctc_beam_search_scored(lp, w, 0)
    assert s2 == s0
    assert CR.bits_equal(c2, c0), (c2, c0)
    assert l2.dtype == np.float32 and np.array_equal(l2, l0)


@pytest.mark.parametrize("beam_gpu", [1, 0])
@pytest.mark.parametrize("allowed", [None, "0123456789."])
def test_beam_scores_equal_the_definition(prod, beam_gpu, allowed):
    width = 8
    case = Case(prod.rbuf, synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40), allowed_chars=allowed)
    case.gpu = OcrEngine(recognition_model=Model.load_bytes(prod.rbuf), allowed_chars=allowed,
                         decode_method=DecodeMethod.BeamSearch(width))
    case.inp = case.gpu.prepare_input(ImageSource.from_tensor(synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40),
                                                              DimOrder.Hwc))
    lines = [prod.lines[i] for i in (0, 3, 7, 12)] + prod.lines[-2:]     # T up to 150, an edge line, a 0 x 0 line
    excl = case.ora.excluded_char_labels
    exp = []
    for e in case.oracle(lines):
        L = CR.masked(e, excl)
        steps, score = CR.beam_search(L, width)
        exp.append((steps, CR.step_logps(L, steps), score))
    try:
        case.gpu.set_option("beam_gpu", beam_gpu)
        got = raw(case.gpu, [case.inp], [lines], True)
        plain = raw(case.gpu, [case.inp], [lines], False)
    finally:
        case.gpu.set_option("beam_gpu", 1)
    assert_chars_of("beam", got, plain)
    check_against("beam_gpu %d" % beam_gpu, *got, exp)
    assert CR.bits_equal(got[1][-1], 0.0)


# ------------------------------------------------------------------ caller-implemented model
@pytest.mark.parametrize("beam", [False, True])
@pytest.mark.parametrize("allowed", [None, "123456789"])
def test_callback_model_scores(beam, allowed):
    """lib.rs:527-577's fake recognition model (kat_util): scores from the model output the engine handed back."""
    seen = []

    def run(x):
        y = K.fake_recognition_run(x)
        seen.append(y.copy())
        return y

    rec = Model.from_callable(K.FAKE_RECOGNITION_SHAPE, run)
    eng = OcrEngine(recognition_model=rec, alphabet=K.make_alphabet(), allowed_chars=allowed,
                    decode_method=DecodeMethod.BeamSearch(5) if beam else DecodeMethod.Greedy)
    image = np.zeros((1, 64, 32), np.float32)
    image[:, 2, :8] = 0.7
    image[:, 3, 8:] = 0.3
    image[:, 5, 16:24] = 0.9
    inp = eng.prepare_input(ImageSource.from_tensor(image, DimOrder.Chw))
    line = [_rect(16, 32, 32, 64)[0]]
    (got,) = eng.recognize_text(inp, [line], scores=True)
    (plain,) = eng.recognize_text(inp, [line])
    assert len(seen) == 2 and np.array_equal(seen[0], seen[1])
    out = seen[0][:, 0, :]                      # [T, C] of the one line
    C = out.shape[1]
    L = out.copy()
    if allowed is not None:
        alphabet = K.make_alphabet()
        for c in range(C):
            if c > 0 and alphabet[c - 1] not in allowed:
                L[:, c] = -np.inf
    if beam:
        steps, score = CR.beam_search(L, 5)
    else:
        steps, _, score = CR.greedy(L)
    assert got is not None and str(got) == str(plain)
    assert [c.rect for c in got.chars()] == [c.rect for c in plain.chars()]
    assert CR.bits_equal(got.score, score), (got.score, score)
    assert np.array_equal(np.array([c.logp for c in got.chars()], np.float32), CR.step_logps(L, steps)[:len(got.chars())])


# ------------------------------------------------------------------ CLI
def test_cli_json_confidence(tmp_path):
    from PIL import Image

    from ocrs_amd import cli
    px = synth.synthetic_page(3, 256, 384, lines=8, columns=1)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    plain_file, conf_file = str(tmp_path / "plain.json"), str(tmp_path / "conf.json")
    assert cli.main([path, "-j", "-o", plain_file]) == 0
    assert cli.main([path, "-j", "--confidence", "-o", conf_file]) == 0
    plain = open(plain_file, encoding="utf-8").read()
    doc = json.loads(open(conf_file, encoding="utf-8").read())
    lines = doc["paragraphs"][0]["lines"]
    assert lines, "no text found"
    for ln in lines:
        assert 0.0 < ln["confidence"] <= 1.0
        for w in ln["words"]:
            assert 0.0 < w["confidence"] <= 1.0
            del w["confidence"]
        del ln["confidence"]
    # without the confidence keys, the scored document is the plain one; the plain one is what the unscored path writes
    assert json.dumps(doc, indent=2, ensure_ascii=False, sort_keys=True) == plain
    from ocrs_amd import models
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))
    texts = eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp)))
    assert output.format_json_output(path, px.shape[:2], texts) == plain


# ------------------------------------------------------------------ relaxed numerics
def test_relaxed_mode_scores(prod):
    eng = OcrEngine(recognition_model=Model.load_bytes(prod.rbuf), numerics="relaxed")
    try:
        inp = eng.prepare_input(ImageSource.from_tensor(synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40),
                                                        DimOrder.Hwc))
        lines = prod.lines[::2]
        scored = raw(eng, [inp], [lines], True)
        assert_chars_of("relaxed", scored, raw(eng, [inp], [lines], False))
        assert np.all(np.isfinite(scored[1])) and np.all(scored[1] <= 0.0)
        for chars, clp in scored[0]:
            assert len(clp) == len(chars) and np.all(clp <= 0.0)
    finally:
        del eng
        gc.collect()
