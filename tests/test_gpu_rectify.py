"""Rectified line crops on the GPU, bit for bit against tests/rectify_ref.py.

Crops come through prepare_recognition_input(rectify=True); full recognition is checked against the oracle's recogniser
run by this file on the restatement's crops (tokens, chars, boxes, char log-probs and line scores, greedy and beam).
Lines are built here, not by the detector.

Run with:  python -m pytest tests -m gpu
"""
import json
import math
import threading

import numpy as np
import pytest

import confidence_ref as CR
import models_util as M
import rectify_ref as R
import stub_util
from ocrs_amd import DEFAULT_ALPHABET, DecodeMethod, DimOrder, EngineGroup, ImageSource, Model, OcrEngine, _lib, output, synth
from oracle import pipeline as OP
from oracle.geometry import RotatedRect
from oracle.nn import OracleGraph, OracleModel
from test_rectify_cpu import hand_made_lines, slanted_line

pytestmark = pytest.mark.gpu
H = 64
ANGLES = (0, 3, -3, 10, -10, 30, -30)
BENCH_PAGE = (0, 1024, 1024, 80, 2)   # bench.py's page: synth.synthetic_page(seed, 1024, 1024, lines=80)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


# ------------------------------------------------------------------ pages and lines
def page_word_boxes(seed, height, width, lines, columns):
    """The word boxes (x, y, w, h) that synth.synthetic_page draws, line by line, by replaying its generator."""
    rng = np.random.default_rng(seed)
    rows = max(1, lines // columns)
    margin = 16
    col_w = (width - margin * (columns + 1)) // columns
    pitch = (height - 2 * margin) / rows
    out = []
    for c in range(columns):
        x_left = margin + c * (col_w + margin)
        for r in range(rows):
            lh = int(rng.integers(12, max(13, min(19, int(pitch) - 6))))
            y0 = int(margin + r * pitch + rng.integers(0, max(1, int(pitch) - lh - 5)))
            n_words = int(rng.integers(6, 11))
            x = x_left + int(rng.integers(0, 12))
            line = []
            for _ in range(n_words):
                ww = int(rng.integers(22, 58))
                if x + ww >= x_left + col_w:
                    break
                rng.integers(0, 70)
                wh = lh - int(rng.integers(0, 3))
                yy = y0 + int(rng.integers(0, 2))
                rng.integers(4, 8)
                line.append((x, yy, ww, wh))
                x += ww + int(rng.integers(9, 15))
            if line:
                out.append(line)
    return out


def lines_of_page(spec, pad=2.0):
    """One list of word rects [n, 6] per text line of the synthetic page `spec`; every box is checked to be ink."""
    px = synth.synthetic_page(*spec)
    lines = []
    for boxes in page_word_boxes(*spec):
        for x, y, w, h in boxes:
            assert px[y + h // 2, x + 1, 0] < 128 and px[y + h // 2, x + w - 2, 0] < 128, "the replayed boxes are the page's words"
        lines.append(np.array([[x + w / 2.0, y + h / 2.0, 0.0, -1.0, w + 2 * pad, h + 2 * pad] for x, y, w, h in boxes], np.float32))
    return px, lines


def rotate_page(px, lines, deg):
    """The page turned by `deg` degrees about its centre (bilinear, white outside), and its lines turned with it."""
    th = math.radians(deg)
    c, s = math.cos(th), math.sin(th)
    h, w = px.shape[:2]
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sx = c * (xx - cx) + s * (yy - cy) + cx        # the source of every output pixel: the inverse rotation
    sy = -s * (xx - cx) + c * (yy - cy) + cy
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = sx - x0, sy - y0
    src = px[:, :, 0].astype(np.float64)

    def tap(y, x):
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        return np.where(ok, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 255.0)

    img = (1 - fy) * ((1 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)) + fy * ((1 - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1))
    out = np.repeat(np.clip(np.rint(img), 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)
    turned = []
    for l in lines:
        r = np.array(l, np.float64)
        x, y, ux, uy = r[:, 0] - cx, r[:, 1] - cy, r[:, 2].copy(), r[:, 3].copy()
        r[:, 0], r[:, 1] = c * x - s * y + cx, s * x + c * y + cy
        r[:, 2], r[:, 3] = c * ux - s * uy, s * ux + c * uy
        turned.append(r.astype(np.float32))
    return np.ascontiguousarray(out), turned


def grey_of(px, order="hwc"):
    """The prepared page as the oracle has it: [h, w] float32 in [-0.5, 0.5]."""
    return np.asarray(OP.prepare_image(OP.ImageSource.from_tensor(px, order)))[0]


def noise_page(seed, h, w):
    """[1, h, w] float32 in [0, 1]: every pixel differs from its neighbours, so a wrong tap shows."""
    return np.random.default_rng(seed).random((1, h, w), dtype=np.float32)


# ------------------------------------------------------------------ the expected recognition
class Rig:
    def __init__(self, allowed_chars=None, beam=None):
        self.rbuf = M.recognition_model_bytes()
        self.graph = OracleGraph(self.rbuf)
        self.allowed = allowed_chars
        self.beam = beam
        self.eng = OcrEngine(recognition_model=Model.load_bytes(self.rbuf), allowed_chars=allowed_chars,
                             decode_method=DecodeMethod.BeamSearch(beam) if beam else DecodeMethod.Greedy)
        self.excl = None if allowed_chars is None else [i + 1 for i, ch in enumerate(DEFAULT_ALPHABET) if ch not in allowed_chars]

    def page(self, px, order="hwc"):
        return self.eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc if order == "hwc" else DimOrder.Chw))

    def logits(self, grey, lines):
        """The oracle's recogniser on the restatement's crops: per line (frame, group width, [T, C] log-probs)."""
        frames = [R.line_frame(l, H) for l in lines]
        groups = {}
        for i, fr in enumerate(frames):
            groups.setdefault(R.group_width(fr.rw), []).append(i)
        out = [None] * len(lines)
        for gw, members in groups.items():
            if gw == 0:
                for i in members:
                    out[i] = (frames[i], 0, None)
                continue
            step = max(1, (1 << 20) // (H * gw))
            for c0 in range(0, len(members), step):
                chunk = members[c0:c0 + step]
                batch = np.stack([R.crop(grey, lines[i], H, out_w=gw) for i in chunk])[:, None]
                y = self.graph.run_exact(batch)   # [T, N, C]
                for bi, i in enumerate(chunk):
                    out[i] = (frames[i], gw, np.ascontiguousarray(y[:, bi]))
        return out

    def expected(self, logits):
        """Per line: (tokens [(label, pos)], chars [(char, (top, left, bottom, right))], char log-probs float32, score)."""
        exp = []
        for fr, gw, y in logits:
            if y is None:
                exp.append(([], [], np.zeros(0, np.float32), 0.0))
                continue
            L = CR.masked(y, self.excl)
            if self.beam:
                steps, score = CR.beam_search(L, self.beam)
                slp = CR.step_logps(L, steps)
            else:
                steps, slp, score = CR.greedy(L)
            kept = R.char_boxes(fr, gw, L.shape[0], steps)
            chars = [(DEFAULT_ALPHABET[steps[i][0] - 1] if steps[i][0] - 1 < len(DEFAULT_ALPHABET) else "?", box) for i, box in kept]
            exp.append((list(steps), chars, np.array([slp[i] for i, _ in kept], np.float32), score))
        return exp


def pack(lines_per_page):
    all_lines = [l for lines in lines_per_page for l in lines]
    plo, offs = [0], [0]
    for lines in lines_per_page:
        plo.append(plo[-1] + len(lines))
    for l in all_lines:
        offs.append(offs[-1] + len(l))
    rects = np.concatenate([np.asarray(l, np.float32).reshape(-1, 6) for l in all_lines]) if all_lines else np.zeros((0, 6), np.float32)
    return rects, np.array(offs, np.uintp), np.array(plo, np.uintp)


def raw(engine, inputs, lines_per_page, rectify, scores=True):
    """recognize_text_batch_raw -> per line (chars array, char log-probs), line scores."""
    rects, lo, plo = pack(lines_per_page)
    out = engine.recognize_text_batch_raw(inputs, rects, lo, plo, scores=scores, rectify=rectify)
    chars, co = out[0], out[1]
    per_line = [(chars[int(co[i]):int(co[i + 1])], out[2][int(co[i]):int(co[i + 1])] if scores else None) for i in range(len(co) - 1)]
    return per_line, (out[3] if scores else None)


def assert_same(what, a, b):
    (pa, sa), (pb, sb) = a, b
    assert len(pa) == len(pb), what
    for i, ((ca, la), (cb, lb)) in enumerate(zip(pa, pb)):
        assert ca.tobytes() == cb.tobytes(), "%s: line %d: chars differ" % (what, i)
        assert (la is None and lb is None) or la.tobytes() == lb.tobytes(), "%s: line %d: char log-probs differ" % (what, i)
    assert (sa is None and sb is None) or sa.tobytes() == sb.tobytes(), "%s: line scores differ" % what


def check_recognition(what, rig, inp, lines, exp):
    """Everything the rectified calls return, against `exp` (Rig.expected)."""
    per_line, scores = raw(rig.eng, [inp], [lines], True)
    assert len(per_line) == len(exp) == len(scores), what
    for i, ((chars, clp), (_, echars, elp, escore)) in enumerate(zip(per_line, exp)):
        got = [(chr(int(c["ch"])), (int(c["top"]), int(c["left"]), int(c["bottom"]), int(c["right"]))) for c in chars]
        assert got == echars, "%s: line %d: chars / boxes %s, expected %s" % (what, i, got[:3], echars[:3])
        assert clp.dtype == np.float32 and clp.tobytes() == elp.tobytes(), "%s: line %d: char log-probs" % (what, i)
        assert CR.bits_equal(scores[i], escore), "%s: line %d: score %r, expected %r" % (what, i, scores[i], escore)
    unscored = raw(rig.eng, [inp], [lines], True, scores=False)[0]
    assert [c.tobytes() for c, _ in per_line] == [c.tobytes() for c, _ in unscored], what + ": the unscored call's chars"
    if not rig.beam:   # the token call decodes greedily whatever the engine's method
        toks = rig.eng.recognize_tokens(inp, lines, rectify=True)
        assert toks == [e[0] for e in exp], "%s: CTC steps" % what
    texts = rig.eng.recognize_text(inp, lines, scores=True, rectify=True)
    for i, (t, (_, echars, _, escore)) in enumerate(zip(texts, exp)):
        assert (t is None) == (not echars), (what, i)
        if t is not None:
            assert str(t) == "".join(c for c, _ in echars) and [c.rect for c in t.chars()] == [b for _, b in echars]
            assert CR.bits_equal(t.score, escore)
            assert t.rotated_rect().shape == (6,) and len(output.format_json_output("x", (1, 1), [t])) > 0
    return sum(len(e[1]) for e in exp)


@pytest.fixture(scope="module")
def rig():
    return Rig()


# ------------------------------------------------------------------ 1. crops
def assert_crop(eng, inp, grey, line, what):
    got = eng.prepare_recognition_input(inp, line, rectify=True)
    exp = R.crop(grey, line, H)
    assert got.shape == exp.shape, "%s: shape %s, expected %s" % (what, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = np.argwhere(got != exp)
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r, expected %r"
                             % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])]))
    return exp


@pytest.mark.parametrize("width", [801, 802, 803, 804], ids=lambda w: "W%%4=%d" % (w % 4))
def test_crops_at_every_angle_on_noise(rig, width):
    px = noise_page(width, 700, width)
    inp, grey = rig.page(px, "chw"), grey_of(px, "chw")
    rng = np.random.default_rng(width)
    for deg in ANGLES:
        line = slanted_line(150.0, 350.0, deg, rng.uniform(30, 90, 7), height=26.0, jitter=rng.uniform(-2, 2, 7))
        exp = assert_crop(rig.eng, inp, grey, line, "angle %+d" % deg)
        assert (exp != -0.5).mean() > 0.5
        plain = rig.eng.prepare_recognition_input(inp, line)
        if deg in (10, -10, 30, -30):   # what the feature is for: the line's own frame is far wider than its bounding box's crop
            assert exp.shape[1] > 1.5 * plain.shape[1], (deg, exp.shape, plain.shape)


def edge_lines(h, w):
    yield "over_left", slanted_line(-60.0, 300.0, 8.0, [50.0, 40.0, 60.0])
    yield "over_right", slanted_line(w - 100.0, 300.0, -8.0, [50.0, 40.0, 60.0])
    yield "over_top", slanted_line(200.0, 6.0, -12.0, [50.0, 40.0, 60.0, 45.0])
    yield "over_bottom", slanted_line(200.0, h - 8.0, 12.0, [50.0, 40.0, 60.0, 45.0])
    yield "over_corner", slanted_line(w - 60.0, h - 30.0, 30.0, [50.0, 40.0, 60.0])
    yield "outside_left", slanted_line(-900.0, 300.0, 3.0, [50.0, 40.0, 60.0])
    yield "outside_below", slanted_line(100.0, h + 200.0, -3.0, [50.0, 40.0, 60.0])
    yield "outside_far", slanted_line(1.0e6, -2.0e6, 10.0, [50.0, 40.0, 60.0])


def test_crops_at_the_page_edges_and_hand_made_lines(rig):
    h, w = 1000, 1101
    px = noise_page(5, h, w)
    inp, grey = rig.page(px, "chw"), grey_of(px, "chw")
    for name, line in edge_lines(h, w):
        exp = assert_crop(rig.eng, inp, grey, line, name)
        if name.startswith("outside"):
            assert np.all(exp == -0.5)
        else:
            assert 0.02 < (exp != -0.5).mean() < 0.99, name
    for name, line in hand_made_lines():
        if name == "huge":   # positions beyond float32's integers: the sample weights are not numbers; the host side is pinned on the CPU
            continue
        exp = assert_crop(rig.eng, inp, grey, line, name)
        if name in ("clamp_2400", "clamp_10", "forty_words", "gaps_wider_than_words", "one_word"):
            assert exp.shape[1] == {"clamp_2400": 2400, "clamp_10": 10}.get(name, exp.shape[1]) and (exp != -0.5).any(), name
    # gaps wider than the words, the words at different heights: the mask bridges a gap with both neighbours' rows
    gaps = slanted_line(40.0, 500.0, -6.0, [14.0, 10.0, 16.0, 12.0], height=18.0, gap=150.0, jitter=[-9.0, 7.0, -4.0, 10.0])
    exp = assert_crop(rig.eng, inp, grey, gaps, "gaps with jitter")
    fr = R.line_frame(gaps, H)
    lo, hi = R.column_table(fr, H)
    covered = np.zeros(fr.rw, bool)
    for c0, c1, _, _ in fr.ranges:
        covered[c0:c1 + 1] = True
    assert (~covered).mean() > 0.5 and len({(int(a), int(b)) for a, b in zip(lo, hi)}) >= 5
    assert (exp[:, :fr.rw][:, ~covered] != -0.5).any() and (exp[:, :fr.rw] == -0.5).any()


# ------------------------------------------------------------------ 2. full recognition
@pytest.fixture(scope="module")
def bench_page():
    return lines_of_page(BENCH_PAGE)


@pytest.mark.parametrize("deg", [0, 10, -10])
def test_recognition_on_the_bench_page(rig, bench_page, deg):
    px, lines = bench_page
    if deg:
        px, lines = rotate_page(px, lines, deg)
        lines = lines[::2]
    inp, grey = rig.page(px), grey_of(px)
    logits = rig.logits(grey, lines)
    n = check_recognition("greedy %+d" % deg, rig, inp, lines, rig.expected(logits))
    assert n > 10 * len(lines), "the lines decode to text"
    if deg:   # a skewed line's own frame is several times wider than its bounding box's crop
        wide = [fr.rw for fr, _, _ in logits]
        plain = [rig.eng.prepare_recognition_input(inp, l).shape[1] for l in lines[:8]]
        assert np.mean(wide[:8]) > 2 * np.mean(plain), (wide[:8], plain)
    # allowed_chars, greedy and beam, on the same log-probs
    sub = list(range(0, len(lines), 8))
    for beam in (None, 8):
        r2 = Rig(allowed_chars="0123456789abcdefghij .", beam=beam)
        n2 = check_recognition("allowed %s %+d" % (beam, deg), r2, r2.page(px), [lines[i] for i in sub], r2.expected([logits[i] for i in sub]))
        assert n2 > 0


# ------------------------------------------------------------------ 3. batching and repeatability
def test_batch_of_four_sizes_equals_each_page_alone_and_repeats(rig):
    specs = [(11, 640, 800, 30, 1), (12, 700, 901, 30, 1), (13, 1024, 1024, 80, 2), (14, 500, 1302, 20, 2)]
    pages, lpp = [], []
    for k, spec in enumerate(specs):
        px, lines = lines_of_page(spec)
        px, lines = rotate_page(px, lines, (7, -5, 10, -12)[k])
        pages.append(px)
        lpp.append(lines[::3] + [np.array([[50.0, 80.0, 0.0, -1.0, 0.0, 0.0]], np.float32)])   # and an empty line each
    inputs = [rig.page(p) for p in pages]
    batch = raw(rig.eng, inputs, lpp, True)
    singles = [raw(rig.eng, [inp], [l], True) for inp, l in zip(inputs, lpp)]
    assert_same("four sizes", batch, ([x for s in singles for x in s[0]], np.concatenate([s[1] for s in singles])))
    assert sum(len(c) for c, _ in batch[0]) > 200
    for r in range(20):
        assert_same("repeat %d" % r, raw(rig.eng, inputs, lpp, True), batch)
    # sub-requests within the activation budget: the same bits
    try:
        rig.eng.set_option("rec_max_pixels", 64 * 1200 * 6)
        assert_same("rec_max_pixels", raw(rig.eng, inputs, lpp, True), batch)
    finally:
        rig.eng.set_option("rec_max_pixels", 0)


# ------------------------------------------------------------------ 4. mixed plain and rectified traffic
def test_mixed_traffic_through_the_coalescer(rig):
    eng = OcrEngine(recognition_model=Model.load_bytes(rig.rbuf))
    ora = OP.OcrEngine(recognition_model=OracleModel(rig.graph, "exact"))
    pages, lpp = [], []
    for k in range(4):
        px, lines = lines_of_page((30 + k, 600, 800, 24, 1))
        pages.append(px)
        lpp.append(lines)
    inputs = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pages]
    try:
        eng.set_option("coalesce", 0)
        solo = {(k, r): raw(eng, [inputs[k]], [lpp[k]], r) for k in range(4) for r in (False, True)}
    finally:
        eng.set_option("coalesce", 2)
    s0 = eng.coalesce_stats()["recognize"]
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(w):
        try:
            barrier.wait()
            for r in range(6):
                k, rect = (w + r) % 4, (w + r // 2) % 2 == 0
                results[(w, r)] = (k, rect, raw(eng, [inputs[k]], [lpp[k]], rect))
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
    kinds = {rect for _, rect, _ in results.values()}
    assert kinds == {False, True}
    for (w, r), (k, rect, got) in results.items():
        assert_same("thread %d call %d" % (w, r), got, solo[(k, rect)])
    # the plain results of that traffic are the oracle pipeline's (as test_gpu_parity.py has them) ...
    for k in range(4):
        oin = ora.prepare_input(OP.ImageSource.from_tensor(pages[k], "hwc"))
        exp = ora.recognize_text(oin, [[RotatedRect.from_array(r) for r in l] for l in lpp[k]])
        got = solo[(k, False)][0]
        assert len(got) == len(exp)
        for (chars, _), e in zip(got, exp):
            assert (len(chars) == 0) == (e is None)
            if e is not None:
                assert "".join(chr(int(c)) for c in chars["ch"]) == str(e)
                assert [(int(c["top"]), int(c["left"]), int(c["bottom"]), int(c["right"])) for c in chars] == [c.rect.tlbr() for c in e.chars]
        # ... and the rectified ones the restatement's
        grey = grey_of(pages[k])
        exp_r = rig.expected(rig.logits(grey, lpp[k][:6]))
        for (chars, clp), (_, echars, elp, _) in zip(solo[(k, True)][0][:6], exp_r):
            assert [(chr(int(c["ch"])), (int(c["top"]), int(c["left"]), int(c["bottom"]), int(c["right"]))) for c in chars] == echars
            assert clp.tobytes() == elp.tobytes()


# ------------------------------------------------------------------ 5. an engine group
@pytest.mark.parametrize("gather", ["host", "rccl"])
def test_group_equals_single_engine(rig, gather, monkeypatch):
    if gather == "rccl":   # the librccl test double (tests/stubs)
        monkeypatch.setenv("OCRS_RCCL_LIB", stub_util.rccl_stub_path())
    group = EngineGroup([0, 0], None, rig.rbuf, gather=gather, shared_block=2)
    pages, lpp = [], []
    for k in range(5):
        px, lines = lines_of_page((40 + k, 600, 800, 24, 1))
        px, lines = rotate_page(px, lines, (-8, 4, 9, -3, 6)[k])
        pages.append(px)
        lpp.append(lines[::2])
    inputs = group.prepare_input_batch(pages)
    rects, lo, plo = pack(lpp)
    chars, co = group.recognize_text_batch_raw(inputs, rects, lo, plo, rectify=True)
    assert group.last_gather()["transport"] == gather
    singles = [rig.page(p) for p in pages]
    per_line, _ = raw(rig.eng, singles, lpp, True, scores=False)
    assert len(co) == len(per_line) + 1
    for i, (c, _) in enumerate(per_line):
        assert chars[int(co[i]):int(co[i + 1])].tobytes() == c.tobytes(), i
    assert len(chars) > 200
    plain_chars, _ = group.recognize_text_batch_raw(inputs, rects, lo, plo)
    assert plain_chars.tobytes() != chars.tobytes()


# ------------------------------------------------------------------ 6. the CLI
def test_cli_rectify(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    px = synth.synthetic_page(3, 256, 384, lines=8, columns=1)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    rect_file, plain_file = str(tmp_path / "rect.json"), str(tmp_path / "plain.json")
    assert cli.main([path, "--rectify", "-j", "--confidence", "--text-line-images", "-o", rect_file]) == 0
    assert cli.main([path, "-j", "--confidence", "-o", plain_file]) == 0
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))
    lines = eng.find_text_lines(inp, eng.detect_words(inp))
    assert len(lines) >= 4
    for rectify, f in ((True, rect_file), (False, plain_file)):
        texts = eng.recognize_text(inp, lines, scores=True, rectify=rectify)
        assert output.format_json_output(path, px.shape[:2], texts, confidence=True) == open(f, encoding="utf-8").read()
    assert json.loads(open(rect_file, encoding="utf-8").read())["paragraphs"][0]["lines"]
    eng_grey = np.asarray(inp.image())[0]
    for i, line in enumerate(lines):
        crop = eng.prepare_recognition_input(inp, line, rectify=True)
        assert crop.tobytes() == R.crop(eng_grey, line, H).tobytes(), i
        want = (np.clip(crop + np.float32(0.5), np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / "lines" / ("line-%d.png" % i)))), want)
    assert eng.get_text(inp, rectify=True) == "\n".join(str(t) for t in eng.recognize_text(inp, lines, rectify=True) if t is not None)
