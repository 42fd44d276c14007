"""The CTC decode kernels on packed batches, against their definitions (confidence_ref.py: greedy, beam_search, masked,
row_argmax, step_logps) and not against the project's host implementation: ctc_beam_kernel, the two packed greedy
collapses and the maxlp variant of log_softmax_argmax, through ocrs_ctc_decode_packed — the engine's own plan
(make_packed_plan), layout (row off[t] + m) and decode stage (decode_packed) on head outputs this file chooses
(ctc_cases.py; test_ctc_cases_cpu.py shows that each case reaches the branch it is named for).

Every line's result is the definition's on the log-probs the hook returned for that line, bit for bit, and has the bits
of that line run alone.  The opt-in launch above 64 KB of LDS runs on three lines at the largest pairs the kernel takes
(W = 128 with C = 119, C = 128 with W = 120); W = 128 with C = 128 would need 173632 bytes and is refused, which
test_refusals pins.  The (3, 4, quant) cases and ctc_cases.revived_matrices hold the merge of a prefix that left the beams
and came back beside a beam that extends it: the kernel and the host search used to miss it.  NaN log-probs stay unpinned and out of scope; the numerics of LogSoftmax itself belong to
test_gpu_operators.py.

Run with:  python -m pytest tests/test_gpu_ctc_decode.py -m gpu
"""
import ctypes as C
import time

import numpy as np
import pytest

import confidence_ref as CR
import ctc_cases as CC
from ocrs_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def same_line(what, a, b):
    """Two results of the hook for one line: equal bits in everything they hold."""
    assert a.keys() == b.keys(), what
    assert a["steps"] == b["steps"], what
    assert a["logp"].shape == b["logp"].shape and a["logp"].tobytes() == b["logp"].tobytes(), "%s: log-prob rows" % what
    if "score" in a:
        assert a["step_logp"].tobytes() == b["step_logp"].tobytes(), "%s: step log-probs" % what
        assert CR.bits_equal(a["score"], b["score"]), "%s: score %r / %r" % (what, a["score"], b["score"])


def check_batch(case, method):
    """One case through the hook with `method`; every line against the definition and against the line run alone.
    Returns the seconds the definition took."""
    beam, scored = method in ("beam", "beam_scored"), method.endswith("scored")
    width = case.width if beam else 1
    got = _lib.ctc_decode_packed(case.mats, case.excluded, method, width)
    assert len(got) == len(case.mats)
    spent = 0.0
    for i, (z, g) in enumerate(zip(case.mats, got)):
        what = "%s %s line %d (T = %d)" % (case.name, method, i, z.shape[0])
        lp = g["logp"]
        assert lp.dtype == np.float32 and lp.shape == z.shape, what
        assert not np.isnan(lp).any(), what
        # the returned log-probs are unmasked: an excluded column is as finite as its logits
        if case.excluded is not None:
            assert np.array_equal(np.isfinite(lp[:, case.excluded]), np.isfinite(z[:, case.excluded])), what
        assert np.array_equal(np.isneginf(lp), np.isneginf(z)), what
        L = CR.masked(lp, case.excluded)
        t0 = time.perf_counter()
        steps, slp, score = CC.define_beam(L, width) if beam else CC.define_greedy(L)
        spent += time.perf_counter() - t0
        assert g["steps"] == steps, what
        if not beam:   # the greedy labels are the first maxima of the masked rows
            lab = [CR.row_argmax(r)[0] for r in L]
            assert all(lab[p] == l for l, p in steps), what
        if scored:
            assert g["step_logp"].dtype == np.float32 and g["step_logp"].tobytes() == slp.tobytes(), "%s: step log-probs" % what
            assert CR.bits_equal(g["score"], score), "%s: score %r, expected %r" % (what, g["score"], score)
        if z.shape[0] == 0:   # a line without rows comes back empty, in its place
            assert g["steps"] == [] and lp.shape == (0, case.C), what
            assert not scored or (len(g["step_logp"]) == 0 and CR.bits_equal(g["score"], 0.0)), what
        # the same line as a batch of its own
        same_line(what + " alone", g, _lib.ctc_decode_packed([z], case.excluded, method, width)[0])
    return spent


@pytest.mark.parametrize("method", ["greedy", "greedy_scored"])
@pytest.mark.parametrize("case", CC.GREEDY_CASES, ids=repr)
def test_greedy_collapse_on_packed_batches(case, method):
    check_batch(case, method)


@pytest.mark.parametrize("case", CC.BEAM_CASES, ids=repr)
def test_beam_search_on_packed_batches(case):
    spent = check_batch(case, "beam_scored")
    print("%s: definition %.3f s" % (case.name, spent))
    scored = _lib.ctc_decode_packed(case.mats, case.excluded, "beam_scored", case.width)
    plain = _lib.ctc_decode_packed(case.mats, case.excluded, "beam", case.width)
    for i, (a, b) in enumerate(zip(scored, plain)):   # the unscored launch: the same steps and rows, no scores
        assert "score" not in b and a["steps"] == b["steps"] and a["logp"].tobytes() == b["logp"].tobytes(), (case.name, i)


def test_greedy_without_the_log_probs():
    """The caller does not ask for the log-probs (the engine's plain request): the same steps and scores."""
    case = next(c for c in CC.GREEDY_CASES if c.name == "blank_between-C97-g4")
    for method in ("greedy", "greedy_scored"):
        full = _lib.ctc_decode_packed(case.mats, case.excluded, method)
        bare = _lib.ctc_decode_packed(case.mats, case.excluded, method, want_logp=False)
        for a, b in zip(full, bare):
            assert b["logp"] is None
            same_line(case.name, dict(a, logp=np.zeros(0)), dict(b, logp=np.zeros(0)))


def _blob(res):
    out = []
    for r in res:
        out += [repr(r["steps"]).encode(), r["logp"].tobytes(), r["step_logp"].tobytes(), np.float64(r["score"]).tobytes()]
    return b"|".join(out)


def test_beam_answer_does_not_depend_on_the_node_numbering():
    """Node numbers inside the beam kernel follow the order of its atomics: twenty runs of one batch, equal bytes."""
    case = next(c for c in CC.BEAM_CASES if c.name == "quant-C20-W32-g5")
    first = _blob(_lib.ctc_decode_packed(case.mats, case.excluded, "beam_scored", case.width))
    for _ in range(19):
        assert _blob(_lib.ctc_decode_packed(case.mats, case.excluded, "beam_scored", case.width)) == first


# ---------------------------------------------------------------- refusals
def _raw_call(logits, lengths, n, c, method, width, labels=True, offsets=True, scores=True):
    lab, pos, slp = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)()
    offs, sc = (C.c_size_t * (n + 1))(), (C.c_double * max(n, 1))()
    st = _lib.lib().ocrs_ctc_decode_packed(
        logits.ctypes.data_as(C.POINTER(C.c_float)) if logits is not None else None,
        lengths.ctypes.data_as(C.POINTER(C.c_int32)) if lengths is not None else None, C.c_size_t(n), c, None, method,
        C.c_uint32(width), C.byref(lab) if labels else None, C.byref(pos), offs if offsets else None,
        C.byref(slp) if scores else None, sc if scores else None, None)
    if st == 0:
        for p in (lab, pos) + ((slp,) if method in (1, 3) else ()):
            _lib.lib().ocrs_buffer_free(p)
    return _lib.STATUS_NAMES[st]


def test_refusals():
    z = np.zeros((3, 129), np.float32)
    one = np.array([3], np.int32)
    assert _raw_call(z, one, 1, 129, 2, 4) == "CAPACITY"                 # more than 128 classes
    assert _raw_call(z, one, 1, 5, 2, 129) == "CAPACITY"                 # width above 128
    assert _raw_call(z, one, 1, 5, 3, 0) == "CAPACITY"                   # no width
    assert _raw_call(z, one, 1, 1, 2, 4) == "CAPACITY"                   # beam search needs a label besides the blank
    for c, w in CC.UNSUPPORTED_PAIRS:                                    # LDS above a CU's 160 KB
        assert _raw_call(z, one, 1, c, 2, w) == "CAPACITY", (c, w)
    assert _raw_call(z, one, 1, 0, 0, 1) == "INVALID_ARGUMENT"           # C < 1
    assert _raw_call(z, one, 1, 0, 2, 4) == "INVALID_ARGUMENT"
    assert _raw_call(z, np.array([2, -1], np.int32), 2, 5, 0, 1) == "INVALID_ARGUMENT"   # a negative length
    assert _raw_call(None, one, 1, 5, 0, 1) == "INVALID_ARGUMENT"        # null pointers
    assert _raw_call(z, None, 1, 5, 0, 1) == "INVALID_ARGUMENT"
    assert _raw_call(z, one, 1, 5, 0, 1, labels=False) == "INVALID_ARGUMENT"
    assert _raw_call(z, one, 1, 5, 0, 1, offsets=False) == "INVALID_ARGUMENT"
    assert _raw_call(z, one, 1, 5, 1, 1, scores=False) == "INVALID_ARGUMENT"
    assert _raw_call(z, one, 1, 5, 7, 1) == "INVALID_ARGUMENT"           # no such method
    assert _raw_call(z, one, 1, 5, 0, 1, scores=False) == "OK"           # unscored: the score outputs are not needed
    assert _raw_call(z, one, 1, 5, 3, 128) == "OK"
    with pytest.raises(_lib.OcrsError) as e:
        _lib.ctc_decode_packed([np.zeros((2, 200), np.float32)], None, "beam", 8)
    assert e.value.status_name == "CAPACITY"
    # a batch without rows is not an error
    for r in _lib.ctc_decode_packed([np.zeros((0, 7), np.float32)] * 2, None, "beam_scored", 8):
        assert r["steps"] == [] and r["logp"].shape == (0, 7) and len(r["step_logp"]) == 0 and CR.bits_equal(r["score"], 0.0)


# ---------------------------------------------------------------- the one-line hook against the definition
def _logp(rng, T, Cn, scale=2.0):
    return CC.log_softmax32(rng.normal(0.0, scale, (T, Cn)))


def one_line_matrices():
    rng = np.random.default_rng(99)
    out = []
    for w in (1, 4, 100):                      # one row entirely -inf: every hypothesis dies there
        lp = _logp(rng, 9, 6)
        lp[4, :] = -np.inf
        out.append(("dead-row-w%d" % w, lp, w))
    lp = _logp(rng, 7, 5)
    lp[0, :] = -np.inf                         # ... in the first row
    out.append(("dead-first-row-w8", lp, 8))
    for w in (1, 3, 128):                      # C = 2
        out.append(("C2-w%d" % w, _logp(rng, 24, 2, 1.0), w))
    out.append(("wide-C3-w128", _logp(rng, 4, 3), 128))       # width above the candidate count at every step
    out.append(("wide-C5-w100", _logp(rng, 2, 5), 100))
    return out + CC.revived_matrices()         # a prefix leaves the beams and comes back beside its child


ONE_LINE = one_line_matrices()


@pytest.mark.parametrize("impl", [2, 0])
@pytest.mark.parametrize("name,lp,w", ONE_LINE, ids=[m[0] for m in ONE_LINE])
def test_one_line_hook_equals_the_definition(name, lp, w, impl):
    stats = {}
    want_steps, want_score = CR.beam_search(lp, w, stats)
    if name.startswith("dead"):                # the definition: the path stops at the dead row, the score is -inf
        dead = int(np.flatnonzero(np.isneginf(lp).all(axis=1))[0])
        assert want_score == -np.inf and all(p < dead for _, p in want_steps)
    if name.startswith("wide"):
        assert stats["short"] == stats["steps"] == lp.shape[0]
    steps, score, slp = _lib.ctc_beam_search_scored(lp, w, impl)
    assert steps == want_steps
    assert CR.bits_equal(score, want_score), (score, want_score)
    assert slp.dtype == np.float32 and slp.tobytes() == CR.step_logps(lp, steps).tobytes()
    assert _lib.ctc_beam_search(lp, w, impl) == want_steps
