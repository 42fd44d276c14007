"""The three geometry kernels every request passes through, on noise, against the oracle bit for bit and against the
float64 restatements of tests/geometry_ref.py within their derived bound:

  a. resize_pages_kernel (kernels_image.hip): the detector's input, seen by a callback model that records its argument;
  b. resize_threshold_kernel<false|true>: the probability map a callback model returns, resized back to the page, and the
     mask through the words' pixel counts (detscore_ref), on both sides of the launch choice and at every W % 4;
  c. crop_lines_kernel (kernels_lines.hip): the plain line crop, and its page table and offsets through the rows a
     callback recognition model is given for one batch over three pages.

tests/test_geometry_cpu.py walks the same case lists on the oracle and asserts that each case exercises its branch.

Run with:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

import detscore_ref as DR
import geometry_ref as G
import kat_util as K
from ocrs_amd import Model, OcrEngine, _lib
from oracle import pipeline as OP
from oracle.geometry import RotatedRect

pytestmark = pytest.mark.gpu

IN_CASES = G.in_cases()
BACK_CASES = G.back_cases()
CROP_CASES = G.crop_cases()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def rects_of(words):
    return np.array([w.to_array() for w in words], np.float32).reshape(-1, 6)


def words_of(line):
    return [RotatedRect.from_array(r) for r in line]


class Det:
    """An engine and an oracle engine whose detection model (input 160 x 128) records a copy of its argument and returns
    `prob`: the model stage costs nothing and shows what the resize handed to it."""

    def __init__(self):
        self.seen, self.oseen = [], []
        self.prob = np.zeros(G.MODEL_HW, np.float32)
        shape = [None, 1, G.MODEL_HW[0], G.MODEL_HW[1]]
        rig = self

        def run(x):
            rig.seen.append(np.array(x, np.float32).reshape(G.MODEL_HW))
            return rig.prob.reshape((1, 1) + G.MODEL_HW)

        class Fake:
            def input_shape(self):
                return shape

            def run(self, x):
                rig.oseen.append(np.array(x, np.float32).reshape(G.MODEL_HW))
                return rig.prob.reshape((1, 1) + G.MODEL_HW)

        self.eng = OcrEngine(detection_model=Model.from_callable(shape, run))
        self.ora = OP.OcrEngine(detection_model=Fake())

    def reset(self, prob=None):
        del self.seen[:], self.oseen[:]
        self.prob = np.zeros(G.MODEL_HW, np.float32) if prob is None else prob


@pytest.fixture(scope="module")
def det():
    return Det()


# ------------------------------------------------------------------------------------------------ a. the model input
@pytest.mark.parametrize("case", IN_CASES, ids=[c[0] for c in IN_CASES])
def test_model_input(det, case):
    name, page, planted = case
    det.reset()
    det.eng.detect_text_pixels(det.eng.input_from_grey(page))
    det.ora.detect_text_pixels(page[None])
    (x,), (ox,) = det.seen, det.oseen
    G.same_bits(x, ox, name + ": model input against the oracle's")
    if planted is None:
        ref, tol = G.model_input64(page)
        print("%s: largest |input - float64| / tol %.3f" % (name, G.check64(name, x, ref, tol)))


def test_model_inputs_of_one_batch_in_page_order(det):
    """Every page of the list in one detect_words_batch call (ten sizes: ten launches of the resize into one tensor): the
    model is called once per page, in the caller's order, with the bits of the single calls."""
    det.reset()
    inputs = [det.eng.input_from_grey(page) for _, page, _ in IN_CASES]
    words = det.eng.detect_words_batch(inputs)
    for _, page, _ in IN_CASES:
        det.ora.detect_text_pixels(page[None])
    assert len(det.seen) == len(det.oseen) == len(IN_CASES) and all(len(w) == 0 for w in words)
    for (name, _, _), x, ox in zip(IN_CASES, det.seen, det.oseen):
        G.same_bits(x, ox, name + ": model input of the batch")


# ------------------------------------------------------------------------------------------------ b. the way back
def assert_words(what, got, exp):
    """(rects, score, pixels) equal bit for bit, in order."""
    (gr, gs, gp), (er, es, ep) = got, exp
    assert gr.shape == er.shape, "%s: %d words, expected %d" % (what, len(gr), len(er))
    assert np.ascontiguousarray(gr, np.float32).tobytes() == np.ascontiguousarray(er, np.float32).tobytes(), what + ": rects"
    assert gp.dtype == np.uint32 and np.array_equal(gp, ep), "%s: pixel counts %s, expected %s" % (what, gp[:8], ep[:8])
    assert gs.dtype == np.float32 and np.array_equal(DR.bits(gs), DR.bits(es)), "%s: scores %s, expected %s" % (what, gs[:8], es[:8])


@pytest.mark.parametrize("case", BACK_CASES, ids=[c[0] for c in BACK_CASES])
def test_map_back(det, case):
    name, hw, out_map, kind = case
    det.reset(out_map)
    page = np.zeros(hw, np.float32)
    inp = det.eng.input_from_grey(page)
    oP = det.ora.detect_text_pixels(page[None])
    owords = rects_of(det.ora.detect_words(page[None]))
    ref, tol = G.back_map64(hw, out_map)
    exp = DR.reference(oP, float(G.THR), G.MIN_AREA)     # the definition of pixels and score, on the oracle's map
    assert exp[0].tobytes() == owords.tobytes(), name + ": the definition's words are the oracle's"
    if kind == "noise":
        assert len(owords) >= 3, name
    if kind == "threshold":
        assert exp[2].tolist() == [G.PLANTED_PIXELS]
    # the fused kernel (it writes the component stage's initial labels too) needs W % 4 == 0; such widths run both ways
    modes = (1, 0) if hw[1] % 4 == 0 else (1,)
    try:
        for quad in modes:
            det.eng.set_option("ccl_quad", quad)
            what = "%s, ccl_quad %d" % (name, quad)
            P = det.eng.detect_text_pixels(inp)
            G.same_bits(P, oP, what + ": map against the oracle's")
            ratio = G.check64(what, P, ref, tol)
            differ, band = G.mask_mismatch(P, ref, tol)
            print("%s: largest |map - float64| / tol %.3f; %.4f %% of the page within tol of the threshold; %d words" % (
                what, ratio, 100 * band, len(owords)))
            assert differ == 0, "%s: %d mask pixels differ from the float64 mask outside the band" % (what, differ)
            if kind == "noise":
                assert band <= G.MAX_BAND, what
            got = det.eng.detect_words(inp, scores=True)
            assert_words(what, got, (owords, exp[1], exp[2]))
            assert np.array_equal(det.eng.detect_words(inp), owords), what + ": the unscored call"
    finally:
        det.eng.set_option("ccl_quad", 1)


# ------------------------------------------------------------------------------------------------ c. plain crops
class Rec:
    def __init__(self):
        self.rows = []
        rig = self

        def run(x):
            rig.rows += [(x.shape[3], x[i, 0].tobytes()) for i in range(x.shape[0])]
            return K.fake_recognition_run(x)

        class Fake:
            def input_shape(self):
                return K.FAKE_RECOGNITION_SHAPE

            def run(self, x):
                return K.fake_recognition_run(x)

        self.eng = OcrEngine(recognition_model=Model.from_callable(K.FAKE_RECOGNITION_SHAPE, run), alphabet=K.make_alphabet())
        self.ora = OP.OcrEngine(recognition_model=Fake(), alphabet=K.make_alphabet())
        self.grey = {key: G.crop_page(key) for key in G.CROP_PAGES}
        self.inp = {key: self.eng.input_from_grey(g) for key, g in self.grey.items()}


@pytest.fixture(scope="module")
def rec():
    return Rec()


@pytest.mark.parametrize("case", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_plain_crop(rec, case):
    name, key, line, group = case
    grey = rec.grey[key]
    words = words_of(line)
    got = rec.eng.prepare_recognition_input(rec.inp[key], line)
    exp = rec.ora.prepare_recognition_input(grey[None], words)
    G.same_bits(got, exp, name + ": crop against the oracle's")
    poly, rw = rec.ora.recognizer._line_geometry(words)
    ref, tol = G.crop64(grey, poly, rw)
    print("%s: crop %s, largest |crop - float64| / tol %.3f" % (name, got.shape, G.check64(name, got, ref, tol)))


def test_batch_rows_across_three_pages(rec):
    """One recognize_text_batch call over three pages of different sizes: every row the recognition model is given is the
    oracle's crop of its (page, line), right-padded with -0.5 to its group width — the page table and the rows' offsets."""
    batch = G.batch_lines()
    del rec.rows[:]
    out = rec.eng.recognize_text_batch([rec.inp[key] for key, _ in batch], [lines for _, lines in batch])
    assert [len(o) for o in out] == [len(lines) for _, lines in batch]
    exp = []
    for key, lines in batch:
        for l in lines:
            crop = rec.ora.prepare_recognition_input(rec.grey[key][None], words_of(l))
            gw = G.group_width(crop.shape[1])
            row = np.full((G.REC_H, gw), G.FILL, np.float32)
            row[:, :crop.shape[1]] = crop
            exp.append((gw, row.tobytes()))
    assert len(rec.rows) == len(exp), "%d rows, expected %d" % (len(rec.rows), len(exp))
    missing = sorted(set(exp) - set(rec.rows))
    assert sorted(rec.rows) == sorted(exp), "%d rows are not the oracle's crops; group widths of the first: %s" % (len(missing), [m[0] for m in missing[:4]])
