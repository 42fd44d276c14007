"""The engine's recognition log-probs against the oracle, bit for bit (ocrs_engine_recognize_logits).

The engine runs recognition as one ragged batch over all width groups of a request (HipModel::run_recognition_packed:
conv12_fused_ragged / conv3x3_ragged patch tables, pool_ragged, avgpool_to_seq_ragged, the GRU input GEMMs and the
persistent recurrence with per-row sequence lengths), optionally as two batches on two streams (long / short lines) and
as several sub-requests (rec_max_pixels).  A greedy decode tolerates small errors in its log-probs, so every case here
compares the log-probs themselves: per line [T_i, C], unmasked, equal to the oracle's (models_util.oracle_line_logits)
with np.array_equal, NaN positions included.  Lines that decode to text also give the oracle's greedy CTC steps through
ocrs_engine_recognize_tokens.

Run with:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

import f64_ref as R
import models_util as M
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, numerics_report as NR, synth
from oracle import pipeline as OP
from oracle.geometry import RotatedRect
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu
PAGE_HW = (1100, 1400)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()   # fail loudly: there is no CPU fallback to "pass" on


class Case:
    """One recognition model on the GPU and in the oracle, over one synthetic page."""

    def __init__(self, rbuf, px, order="hwc", allowed_chars=None):
        self.rbuf = rbuf
        self.gpu = OcrEngine(recognition_model=Model.load_bytes(rbuf), allowed_chars=allowed_chars)
        self.ora = OP.OcrEngine(recognition_model=OracleModel(OracleGraph(rbuf), "exact"), allowed_chars=allowed_chars)
        self.inp = self.gpu.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc if order == "hwc" else DimOrder.Chw))
        self.oin = self.ora.prepare_input(OP.ImageSource.from_tensor(px, order))

    def oracle(self, lines):
        return M.oracle_line_logits(self.rbuf, self.ora, self.oin, lines)

    def resized_width(self, line):
        return self.ora.recognizer._line_geometry([RotatedRect.from_array(r) for r in line])[1]

    def check(self, lines, exp=None, what=""):
        """recognize_logits == the oracle's log-probs, and recognize_tokens == greedy CTC of them (masked as the
        reference masks for decoding, recognition.rs:547-561).  Returns the number of lines that decode to text."""
        exp = self.oracle(lines) if exp is None else exp
        got = self.gpu.recognize_logits(self.inp, lines)
        M.assert_logits_equal(got, exp, what)
        excl = self.ora.excluded_char_labels
        toks = self.gpu.recognize_tokens(self.inp, lines)
        assert len(toks) == len(lines)
        n_text = 0
        for i, e in enumerate(exp):
            if excl is not None:
                e = e.copy()
                e[:, excl] = -np.inf
            want = R.ctc_greedy(e)
            if want:
                n_text += 1
                assert toks[i] == want, "%s: line %d: CTC steps %s, oracle %s" % (what, i, toks[i], want)
        return n_text


def _rect(cx, cy, w, h):
    return RotatedRect.new((np.float32(cx), np.float32(cy)), (np.float32(0.0), np.float32(1.0)), np.float32(w),
                           np.float32(h)).to_array()[None]


def line_of_width(case, rw, x0, y0):
    """A horizontal one-word line at (x0, y0) whose resized width is exactly rw (resized_line_width of its integral
    bounding rect at the model's input height)."""
    in_h = case.ora.recognizer.input_height()
    for h in (16, 20, 24, 12, 28, 32, 10, 40, 48, 64, 8):
        w0 = rw * h / in_h
        for w in sorted({int(w0), int(w0) + 1, int(w0) - 1, int(w0) + 2}):
            if w < 1:
                continue
            line = _rect(x0 + w / 2, y0 + h / 2, w, h)
            if case.resized_width(line) == rw:
                return line
    raise AssertionError("no line of resized width %d" % rw)


def sweep_widths():
    """Resized widths reaching every width group 50 .. 2400 (T = 12 .. 600): the clamp floor 10, full groups
    (rw = gw), groups one short (gw - 1), groups of odd pooled width (50, 150, 250), and ragged widths elsewhere."""
    rws = [10]
    for k, gw in enumerate(range(50, 2401, 50)):
        rws.append(gw - (7 + 13 * k) % 49)
    for gw in (50, 100, 150, 250, 300, 650, 1200, 2400):
        rws += [gw, gw - 1]
    return rws


def sweep_lines(case):
    """One line per entry of sweep_widths(), all inside the page (1100 x 1400; the longest are 600 px wide)."""
    return [line_of_width(case, rw, 5 + 97 * (i % 7), 5 + 16 * i) for i, rw in enumerate(sweep_widths())]


@pytest.fixture(scope="module")
def prod():
    case = Case(M.recognition_model_bytes(), synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40))
    case.lines = sweep_lines(case)
    case.exp = case.oracle(case.lines)
    return case


# ------------------------------------------------------------------ width groups of the production model
def test_width_group_sweep_in_one_request(prod):
    gws = {-(-prod.resized_width(l) // 50) * 50 for l in prod.lines}
    assert gws == set(range(50, 2401, 50))
    assert [prod.resized_width(l) for l in prod.lines] == sweep_widths()
    assert prod.check(prod.lines, prod.exp, "sweep") >= 20


def test_width_group_sweep_one_group_per_request(prod):
    by_gw = {}
    for i, l in enumerate(prod.lines):
        by_gw.setdefault(-(-prod.resized_width(l) // 50) * 50, []).append(i)
    for gw, idx in sorted(by_gw.items()):
        prod.check([prod.lines[i] for i in idx], [prod.exp[i] for i in idx], "group %d alone" % gw)


OPTION_SETS = [dict(conv12_fuse=f, conv_flat=c, gru_mode=g) for f in (0, 1) for c in (0, 1) for g in (0, 1)] + \
              [dict(gru_gates=0), dict(gru_local=0)]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
def test_option_matrix_equals_oracle(prod, opts):
    """Every recognition kernel choice must equal the oracle itself, not only the other choices."""
    saved = {k: prod.gpu.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            prod.gpu.set_option(k, v)
        prod.check(prod.lines, prod.exp, str(opts))
    finally:
        for k, v in saved.items():
            prod.gpu.set_option(k, v)


# ------------------------------------------------------------------ other model shapes
@pytest.mark.parametrize("hidden,in_h,seed,chans,modes", [
    (64, 64, 21, (32, 64, 128, 128, 128, 128), (0,)),
    (64, 32, 21, (32, 64, 64, 64, 64, 64), (0,)),
    (64, 16, 21, (32, 64, 64, 64, 64, 64), (0,)),      # H = 2 after the pools: the per-group run_device path
    (32, 64, 33, (32, 64, 64, 64, 64, 64), (0,)),      # no persistent kernel: two launches per step
    (64, 64, 33, (32, 64, 64, 64, 64, 64), (0, 1)),    # persistent, and the fused step kernel with gru_mode = 1
    (128, 64, 33, (32, 64, 64, 64, 64, 64), (0,)),
])
def test_other_model_shapes(prod, hidden, in_h, seed, chans, modes):
    case = Case(M.small_recognition_bytes(hidden, in_h, seed=seed, chans=chans),
                synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40))
    lines = prod.lines[::2] + prod.lines[-4:]   # the same rects: at other input heights, other widths and groups
    exp = case.oracle(lines)
    try:
        for mode in modes:
            case.gpu.set_option("gru_mode", mode)
            case.check(lines, exp, "hidden %d H %d gru_mode %d" % (hidden, in_h, mode))
    finally:
        case.gpu.set_option("gru_mode", 0)


# ------------------------------------------------------------------ request shapes
def test_one_line_and_row_tiles_of_equal_length(prod):
    """1 line; 15, 16 and 17 lines of one width group (T = 125) around the recurrence's 16-row tile."""
    prod.check(prod.lines[5:6], prod.exp[5:6], "one line")
    same = [line_of_width(prod, 460 + 2 * i, 20 + 300 * (i % 4), 10 + 60 * (i // 4)) for i in range(17)]
    exp = prod.oracle(same)
    assert {e.shape[0] for e in exp} == {125}
    for n in (15, 16, 17):
        prod.check(same[:n], exp[:n], "%d lines of T 125" % n)


def test_lines_of_distinct_lengths(prod):
    idx = [i for i, l in enumerate(prod.lines[1:49], 1)]       # one line per group, T 12 .. 600 all distinct
    assert len({prod.exp[i].shape[0] for i in idx}) == len(idx)
    order = np.random.default_rng(3).permutation(idx)
    prod.check([prod.lines[i] for i in order], [prod.exp[i] for i in order], "distinct T")


def test_long_short_split_request(prod):
    """>= 64 short lines (T <= 160) with long ones: two ragged batches on two streams (engine.cpp T_SPLIT)."""
    rng = np.random.default_rng(5)
    lines = []
    for i in range(72):
        ww, hh = int(rng.integers(20, 150)), int(rng.integers(16, 24))
        lines.append(_rect(20 + (i % 6) * 160 + ww / 2, 12 + (i // 6) * 26, ww, hh))
    for i in range(5):
        ww = 600 + 80 * i
        lines.append(_rect(20 + ww / 2, 400 + 30 * i, ww, 14.0))
    exp = prod.oracle(lines)
    assert sum(e.shape[0] <= 160 for e in exp) >= 64 and sum(e.shape[0] > 160 for e in exp) == 5
    prod.check(lines, exp, "long/short")


def test_sub_requests(prod):
    """rec_max_pixels forced down to one line and to ~12 lines per sub-request."""
    try:
        for budget in (64 * 50, 64 * 1200 * 12):
            prod.gpu.set_option("rec_max_pixels", budget)
            prod.check(prod.lines, prod.exp, "rec_max_pixels %d" % budget)
    finally:
        prod.gpu.set_option("rec_max_pixels", 0)


def test_edge_and_zero_width_lines(prod):
    """A line hanging over the page edge, and a 0 x 0 line (NaN aspect, resized width 0) amid others: (0, C)."""
    h, w = PAGE_HW
    edge = _rect(w - 10, h - 5, 120, 20)
    zero = _rect(300, 300, 0, 0)
    assert prod.resized_width(zero) == 0
    lines = [prod.lines[3], edge, zero, prod.lines[20], _rect(-20, 40, 90, 18)]
    exp = prod.oracle(lines)
    assert exp[2].shape == (0, 97)
    prod.check(lines, exp, "edge / zero width")


def test_allowed_chars_leave_log_probs_unmasked(prod):
    """The reference masks excluded classes only for decoding (recognition.rs:547-561): the log-probs are the model's
    output as it is, the steps those of the masked sequence."""
    case = Case(prod.rbuf, synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40), allowed_chars="0123456789.")
    lines = prod.lines[::3]
    assert case.check(lines, [prod.exp[i] for i in range(0, len(prod.lines), 3)], "allowed_chars") >= 5


# ------------------------------------------------------------------ bench scale, sampled
def test_bench_page_lines():
    """One bench page (1024 x 1024, 80 lines): detect and group on the GPU, then every line's log-probs."""
    dbuf, rbuf = M.detection_model_bytes(), M.recognition_model_bytes()
    px = synth.synthetic_page(0, 1024, 1024, lines=80)
    case = Case(rbuf, px)
    det = OcrEngine(detection_model=Model.load_bytes(dbuf))
    dinp = det.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    lines = det.find_text_lines(dinp, det.detect_words(dinp))
    assert len(lines) > 60
    assert case.check(lines, what="bench page") > 60


def _sample(n, rng):
    return sorted(set(range(32)) | set(range(n - 32, n)) | set(rng.choice(np.arange(32, n - 32), 64, replace=False)))


def test_bench_crop_requests_sampled():
    """configs[2] (2 048 crops, group 300) and 2 560 lines (a second wave of GRU clusters, lines 2048.. repeating the
    first crops): a fixed sample of each against the oracle, the repeats bit for bit against what they repeat."""
    rbuf = M.recognition_model_bytes()
    gpu = OcrEngine(recognition_model=Model.load_bytes(rbuf))
    inp, lines = NR.crops_request(gpu, synth)
    n = len(lines)
    crops = synth.synthetic_line_crops(1000, n=n)
    page = (crops.reshape(1, n * 64, 256) + 0.5).astype(np.float32)
    ora = OP.OcrEngine(recognition_model=OracleModel(OracleGraph(rbuf), "exact"))
    oin = ora.prepare_input(OP.ImageSource.from_tensor(page, "chw"))
    rng = np.random.default_rng(2048)
    lines2 = lines + lines[:512]
    s1, s2 = _sample(n, rng), _sample(len(lines2), rng)
    crop_idx = sorted({i for i in s1} | {i % n for i in s2})
    ref = dict(zip(crop_idx, M.oracle_line_logits(rbuf, ora, oin, [lines[i] for i in crop_idx])))
    got1 = gpu.recognize_logits(inp, lines)
    M.assert_logits_equal([got1[i] for i in s1], [ref[i] for i in s1], "2048 crops, sampled")
    got2 = gpu.recognize_logits(inp, lines2)
    M.assert_logits_equal([got2[i] for i in s2], [ref[i % n] for i in s2], "2560 lines, sampled")
    M.assert_logits_equal(got2[n:], got2[:512], "2560 lines, repeats")
    M.assert_logits_equal(got2[:n], got1, "2560 lines against 2048")
