"""The oracle's three geometry steps (the page resized to the detector's input, the probability map resized back, the
plain line crop) against their float64 restatements in tests/geometry_ref.py, over the case lists that
tests/test_gpu_geometry.py walks on the GPU — and the conditions under which those cases test anything, asserted on the
oracle's results, so that a case that stops exercising its branch fails here.  No GPU."""
import numpy as np
import pytest

import geometry_ref as G
import kat_util as K
from oracle import clib
from oracle import pipeline as OP
from oracle.geometry import RotatedRect

IN_CASES = G.in_cases()
BACK_CASES = G.back_cases()
CROP_CASES = G.crop_cases()


class Recorder:
    """A detection model that records its input and returns a chosen map."""

    def __init__(self):
        self.seen = []
        self.prob = np.zeros(G.MODEL_HW, np.float32)

    def input_shape(self):
        return [None, 1, G.MODEL_HW[0], G.MODEL_HW[1]]

    def run(self, x):
        self.seen.append(np.array(x, np.float32).reshape(G.MODEL_HW))
        return self.prob.reshape((1, 1) + G.MODEL_HW)


class FakeRec:
    def __init__(self):
        self.rows = []

    def input_shape(self):
        return K.FAKE_RECOGNITION_SHAPE

    def run(self, x):
        self.rows += [(x.shape[3], x[i, 0].tobytes()) for i in range(x.shape[0])]
        return K.fake_recognition_run(x)


def words_of(line):
    return [RotatedRect.from_array(r) for r in line]


# ------------------------------------------------------------------------------------------------ a. the way in
@pytest.mark.parametrize("case", IN_CASES, ids=[c[0] for c in IN_CASES])
def test_model_input(case):
    name, page, planted = case
    h, w = page.shape
    pb, pr = G.pads((h, w))
    # the resize itself, at every size, identity included: the formula, non-finite values by position
    ref, tol = G.bilinear64(page, G.MODEL_HW[0], G.MODEL_HW[1], h + pb, w + pr)
    direct = clib.resize_bilinear(page, G.MODEL_HW[0], G.MODEL_HW[1], h + pb, w + pr, G.FILL)
    ratio = G.check64(name + ": resize_bilinear", direct, ref, tol)
    # what the detector hands to the model: that, or a copy where the padded page has the model's size
    rec = Recorder()
    OP.OcrEngine(detection_model=rec).detect_text_pixels(page[None])
    (x,) = rec.seen
    ref_in, tol_in = G.model_input64(page)
    G.check64(name + ": model input", x, ref_in, tol_in)
    print("%s: largest |oracle - float64| / tol %.3f" % (name, ratio))
    if G.is_identity_in((h, w)):
        exp = np.full(G.MODEL_HW, G.FILL, np.float32)
        exp[:h, :w] = page
        G.same_bits(x, exp, name + ": a same-size resize is a copy")
        if planted is not None and planted != planted:
            # the case is there because the formula at scale 1 is NOT a copy: 0 * NaN spreads the NaN up and to the left
            assert np.isnan(direct).sum() > np.isnan(x).sum() == len(G.plant_points((h, w))), name
        if planted is not None and planted == 0:
            assert np.signbit(x[0, 0]) and not np.signbit(direct[0, 0]), "the formula loses the sign of -0.0, the copy keeps it"
    else:
        G.same_bits(x, direct, name + ": the model input is the resize")
        assert (h + pb, w + pr) != G.MODEL_HW
    if planted is not None and not np.isfinite(planted):
        assert not np.isfinite(x).all(), name + ": the planted value reaches the model input"


def test_in_cases_cover_what_they_name():
    ids = [c[0] for c in IN_CASES]
    assert len(ids) == len(set(ids)) == len(G.IN_PAGES) + 16
    assert [G.is_identity_in(hw) for hw in G.IN_PAGES] == [True, True, False, False, False, False, True, False, False, False]
    assert G.pads((100, 300)) == (60, 0) and G.pads((300, 100)) == (0, 28) and G.pads((37, 53)) == (123, 75)
    # the scales of the planted pages are float32 numbers, so the weights are the same in float32 and float64
    for hw in G.PLANT_PAGES:
        pb, pr = G.pads(hw)
        for a, b in ((hw[0] + pb, G.MODEL_HW[0]), (hw[1] + pr, G.MODEL_HW[1])):
            assert float(np.float32(a) / np.float32(b)) == a / b, (hw, a, b)
        assert len(G.plant_points(hw)) == 3 + (pb > 0) + 2 * (pr > 0)


# ------------------------------------------------------------------------------------------------ b. the way back
@pytest.mark.parametrize("case", BACK_CASES, ids=[c[0] for c in BACK_CASES])
def test_map_back(case):
    name, hw, out_map, kind = case
    rec = Recorder()
    rec.prob = out_map
    ora = OP.OcrEngine(detection_model=rec)
    page = np.zeros((1,) + hw, np.float32)
    P = ora.detect_text_pixels(page)
    assert P.shape == hw and P.dtype == np.float32
    ref, tol = G.back_map64(hw, out_map)
    ratio = G.check64(name, P, ref, tol)
    sh, sw = G.back_slice(hw)
    if G.is_identity_back(hw):
        G.same_bits(P, np.ascontiguousarray(out_map[:sh, :sw]), name + ": a same-size resize is a copy")
    else:
        G.same_bits(P, clib.resize_bilinear(np.ascontiguousarray(out_map[:sh, :sw]), hw[0], hw[1]), name + ": the map is the resize of the slice")
    differ, band = G.mask_mismatch(P, ref, tol)
    print("%s: largest |oracle - float64| / tol %.3f; %.4f %% of the page within tol of the threshold" % (name, ratio, 100 * band))
    assert differ == 0, "%s: %d mask pixels differ from the float64 mask outside the band" % (name, differ)
    words = ora.detect_words(page)
    if kind == "noise":
        assert band <= G.MAX_BAND, name
        assert len(words) >= 3, "%s: %d words" % (name, len(words))
        fg = float((P > G.THR).mean())
        assert 0.05 < fg < 0.95, "%s: %.3f of the page is text" % (name, fg)
    elif kind == "threshold":
        y, x, bh, bw = G.PLANTED_BLOCK
        assert (P[y:y + bh, x:x + bw // 2] == G.THR).all() and (P[y:y + bh, x + bw // 2:x + bw] > G.THR).all()
        mask = clib.threshold(P, float(G.THR))
        assert int(mask.sum()) == G.PLANTED_PIXELS == 280 and len(words) == 1, "the planted component is the right half alone"
    else:
        assert np.isnan(P).any() and np.isposinf(P).any() and np.isneginf(P).any() and len(words) >= 2, name
        if not G.is_identity_back(hw):   # the resize spreads them: 0 * Inf is NaN at the rows' scale of 1
            assert np.isnan(P).sum() > np.isnan(out_map).sum(), name


def test_back_cases_cover_what_they_name():
    widths = [hw[1] for hw in G.BACK_PAGES if hw[0] == 64]
    assert {w % 4 for w in widths} == {0, 1, 2, 3}
    quads = sorted({(w + 3) // 4 for w in widths})
    assert quads == [64, 65, 128, 129], "both sides of the 64- and the 128-quad launch choice (a 256-quad row: the 2052 page)"
    assert [G.is_identity_back(hw) for hw in G.BACK_PAGES[:4]] == [True, True, False, False]
    assert G.back_slice((97, 211)) == (97, 128) and G.back_slice((64, 256)) == (64, 128) and G.back_slice((1031, 2052)) == G.MODEL_HW


# ------------------------------------------------------------------------------------------------ c. plain crops
@pytest.fixture(scope="module")
def pages():
    return {key: G.crop_page(key) for key in G.CROP_PAGES}


@pytest.fixture(scope="module")
def rec_engine():
    return OP.OcrEngine(recognition_model=FakeRec(), alphabet=K.make_alphabet())


@pytest.mark.parametrize("case", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_plain_crop(case, pages, rec_engine):
    name, key, line, group = case
    grey = pages[key]
    words = words_of(line)
    exp = rec_engine.prepare_recognition_input(grey[None], words)
    poly, rw = rec_engine.recognizer._line_geometry(words)
    assert exp.shape == (G.REC_H, rw) and exp.dtype == np.float32
    ref, tol = G.crop64(grey, poly, rw)
    ratio = G.check64(name, exp, ref, tol)
    top, left, bh, bw = G.poly_box(poly)
    ink = float((exp != np.float32(G.FILL)).mean()) if exp.size else 0.0
    print("%s: crop %s from a %d x %d box, %.3f of it page pixels, largest |oracle - float64| / tol %.3f" % (name, exp.shape, bh, bw, ink, ratio))
    if group in ("angle", "hand", "edge", "tall", "small"):
        assert ink > 0.02, "%s: %.4f of the crop is not padding" % (name, ink)
    if group == "edge":
        assert ink < 0.99, name
    if group in ("outside", "zero"):
        assert exp.size and (exp == np.float32(G.FILL)).all(), name
    if group == "zero":
        assert bh <= 0 or bw <= 0
    if group == "out_p":
        _, keep, in_page = G.line_image64(grey, poly)
        dropped = 1.0 - keep.sum() / in_page.sum()
        without, _ = G.crop64(grey, poly, rw, drop_out_p=False)
        share = float((without != ref).mean())
        print("%s: the out_p rule drops %d of %d in-page pixels; %.3f of the crop differs from one without the rule" % (
            name, int(in_page.sum() - keep.sum()), int(in_page.sum()), share))
        if name == "out_p":
            assert (int(in_page.sum()), int(keep.sum())) == (2800, 200) and dropped > 0.9
            assert share > 0.25
        else:
            assert top >= 0 and top + bh <= grey.shape[0] and left < 0, "over the left edge only"
            assert dropped > 0.5 and share > 0.25
    if name == "box80x1":
        assert bh == 1 and bw > 1
    if name == "box1x30":
        assert bw == 1 and bh > 1
    if group == "tall":
        assert bh >= 3 * G.REC_H
    if group == "nf":
        assert np.isnan(exp).any() and np.isposinf(exp).any() and np.isfinite(exp).mean() > 0.5


def test_crop_cases_cover_what_they_name():
    ids = [c[0] for c in CROP_CASES]
    assert len(ids) == len(set(ids))
    groups = {g: [c[0] for c in CROP_CASES if c[3] == g] for g in {c[3] for c in CROP_CASES}}
    assert len(groups["angle"]) == len(G.ANGLES) + 12 and len(groups["edge"]) == 5 and len(groups["outside"]) == 3
    assert len(groups["hand"]) == 10 and len(groups["zero"]) == 2 and len(groups["out_p"]) == 2
    assert {G.CROP_PAGES["w%d" % w][2] % 4 for w in (801, 802, 803, 804)} == {0, 1, 2, 3}


def test_batch_rows_are_the_padded_crops(pages):
    """The rows the recognition model is given for a batch of three pages are the single crops, right-padded with -0.5 to
    their group width: the expectation of the GPU test, computed both ways on the oracle."""
    fake = FakeRec()
    ora = OP.OcrEngine(recognition_model=fake, alphabet=K.make_alphabet())
    batch = G.batch_lines()
    assert len({pages[k].shape for k, _ in batch}) == 3 and all(4 <= len(ls) <= 8 for _, ls in batch)
    exp = []
    for key, lines in batch:
        ora.recognize_text(pages[key][None], [words_of(l) for l in lines])
        exp += expected_rows(ora, pages[key], lines)
    assert sorted(fake.rows) == sorted(exp) and len(exp) == sum(len(ls) for _, ls in batch)
    assert len({gw for gw, _ in exp}) >= 5, "several width groups"


def expected_rows(ora, grey, lines):
    out = []
    for l in lines:
        crop = ora.prepare_recognition_input(grey[None], words_of(l))
        gw = G.group_width(crop.shape[1])
        row = np.full((G.REC_H, gw), G.FILL, np.float32)
        row[:, :crop.shape[1]] = crop
        out.append((gw, row.tobytes()))
    return out
