"""Recognition confidence on the host (DESIGN.md "Recognition confidence"): the scored beam-search hook
(ocrs_ctc_beam_search_scored, impl 0 = the engine's host search, 1 = the textbook formulation) against the Python
restatement in confidence_ref.py, bit for bit; and the confidence of TextChar / TextWord / TextLine from hand-built
chars.  The GPU side is tests/test_gpu_confidence.py."""
import math

import numpy as np
import pytest

import confidence_ref as CR
import ctc_cases as CC
from oracle import pipeline as OP


@pytest.fixture(scope="module")
def lib():
    from ocrs_amd import _lib
    return _lib


def _random_logp(rng, T, C, peak):
    z = rng.normal(0, 3, (T, C))
    for t in range(T):
        z[t, (t // 3) % C] += peak
    return (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


def beam_matrices():
    """Seeded [T, C] matrices: masked (-inf) columns, a step where only the blank is allowed, exact ties (values
    quantised to a few levels), T = 0 and T = 1, for widths 1, 8 and 100; and lines with revived prefixes (ctc_cases.py)."""
    rng = np.random.default_rng(1234)
    out = []
    for T, C in [(0, 97), (1, 97), (1, 5), (12, 6), (30, 12), (40, 97), (60, 20)]:
        for w in (1, 8, 100):
            lp = _random_logp(rng, T, C, float(rng.choice([0.3, 3.0, 8.0])))
            if C > 6 and T > 1:
                lp[:, 5] = -np.inf
                lp[T // 2, 1:] = -np.inf
            out.append(("T%d-C%d-w%d" % (T, C, w), lp, w))
    for T, C in [(20, 6), (25, 12)]:        # exact ties: every row holds the same few levels
        for w in (1, 8, 100):
            lv = np.log(np.array([0.5, 0.25, 0.25], np.float32))
            lp = lv[rng.integers(0, 3, (T, C))].astype(np.float32)
            lp[:, 3] = -np.inf
            out.append(("ties-T%d-C%d-w%d" % (T, C, w), lp, w))
    # a prefix falls out of the beams and comes back beside a beam that extends it: the two must merge
    return out + CC.revived_matrices()


MATRICES = beam_matrices()


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("name,lp,w", MATRICES, ids=[m[0] for m in MATRICES])
def test_scored_beam_search_hook(lib, impl, name, lp, w):
    steps, score, slp = lib.ctc_beam_search_scored(lp, w, impl)
    assert steps == lib.ctc_beam_search(lp, w, impl)
    assert steps == [(int(a), int(b)) for a, b in OP.ctc_beam_search(lp, w)]
    want_steps, want_score = CR.beam_search(lp, w)
    assert steps == want_steps
    assert CR.bits_equal(score, want_score), (score, want_score)
    assert slp.dtype == np.float32 and np.array_equal(slp, CR.step_logps(lp, steps))
    if lp.shape[0] == 0:
        assert steps == [] and CR.bits_equal(score, 0.0)


def test_scored_beam_search_rejects_null_outputs(lib):
    import ctypes as C
    from ocrs_amd._lib import OcrsError, check
    a = np.zeros((3, 4), np.float32)
    lab, pos, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_size_t(0)
    with pytest.raises(OcrsError):
        check(lib.lib().ocrs_ctc_beam_search_scored(a.ctypes.data_as(C.POINTER(C.c_float)), 3, 4, C.c_uint32(2), 0,
                                                    C.byref(lab), C.byref(pos), C.byref(n), None, None))


# ---------------------------------------------------------------- text items
def _chars(text, logps=None):
    from ocrs_amd import TextChar
    out = []
    for i, ch in enumerate(text):
        rect = (10, 10 + 8 * i, 20, 17 + 8 * i)
        out.append(TextChar(ch, rect) if logps is None else TextChar(ch, rect, np.float32(logps[i])))
    return out


def test_text_item_confidence():
    from ocrs_amd import TextLine
    lps = [-0.1, -0.5, -2.0, -0.25, -0.75, -1.5]
    line = TextLine(_chars("ab cde", lps), score=-12.5)
    assert line.score == -12.5
    f = [float(np.float32(v)) for v in lps]
    assert line.confidence == math.exp(math.fsum(f) / 6)           # spaces included
    words = line.words()
    assert [str(w) for w in words] == ["ab", "cde"]
    assert words[0].confidence == math.exp(math.fsum(f[:2]) / 2)
    assert words[1].confidence == math.exp(math.fsum(f[3:]) / 3)
    c = line.chars()[2]
    assert c.logp == np.float32(-2.0) and c.confidence == math.exp(-2.0)
    assert isinstance(line.confidence, float) and 0.0 < line.confidence < 1.0


def test_unscored_text_items_behave_as_before():
    from ocrs_amd import TextChar, TextLine
    c = TextChar("x", (1, 2, 3, 4))
    assert (c.char, c.rect, c.logp, c.confidence) == ("x", (1, 2, 3, 4), None, None)
    line = TextLine(_chars("ab c"))
    assert line.score is None and line.confidence is None
    assert [w.confidence for w in line.words()] == [None, None]
    assert str(line) == "ab c" and [str(w) for w in line.words()] == ["ab", "c"]
    assert line.bounding_rect() == (10, 10, 20, 41)
    with pytest.raises(AttributeError):
        c.other = 1   # still a slotted record
    with pytest.raises(AssertionError):
        TextLine([])


def test_json_output_confidence_keys():
    from ocrs_amd import TextLine, output
    lines = [TextLine(_chars("ab cd", [-0.5, -0.5, -1.0, -0.25, -0.25])), None]
    plain = output.format_json_output("x.png", (100, 200), lines)
    assert "confidence" not in plain
    doc = output.ocr_json("x.png", (100, 200), lines, confidence=True)
    (ln,) = doc["paragraphs"][0]["lines"]
    assert ln["confidence"] == lines[0].confidence
    assert [w["confidence"] for w in ln["words"]] == [math.exp(-0.5), math.exp(-0.25)]
    # the rest of the document is the unscored one
    for w in ln["words"]:
        del w["confidence"]
    del ln["confidence"]
    assert doc == output.ocr_json("x.png", (100, 200), lines)


def test_cli_confidence_needs_json():
    from ocrs_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["nothing.png", "--confidence"])
