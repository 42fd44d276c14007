"""Detection confidence, host side: the new entry points are exported and declared, the indexed layout
calls return the plain calls' lines plus the permutation that produced them, and the numpy statement of the score
definition (detscore_ref.py) gives the answers worked out by hand on small maps.  No GPU is used here.

Run with:  python -m pytest tests -m "not gpu"
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import detscore_ref as DR
import kat_util as K
from ocrs_amd import _lib
from oracle.geometry import Rect, RotatedRect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

NEW_SYMBOLS = ["ocrs_engine_detect_words_scored", "ocrs_engine_detect_words_batch_scored",
               "ocrs_group_detect_words_batch_scored", "ocrs_engine_find_text_lines_indexed",
               "ocrs_engine_find_text_lines_batch_indexed"]


@pytest.fixture(scope="module")
def lib():
    from ocrs_amd import build
    build.build()
    return _lib.lib()


def test_new_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "ocrs_amd.h")).read()
    declared = set(re.findall(r"OCRS_API[^;(]*?\b(ocrs_\w+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6


# ---------------------------------------------------------------- find_text_lines_indexed
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _one(lib, a, indexed):
    """ocrs_engine_find_text_lines[_indexed] on [n, 6] -> (rects [n, 6], offsets list, word_index or None)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 6)
    lr, lo, nl, wi = C.POINTER(C.c_float)(), C.POINTER(C.c_size_t)(), C.c_size_t(0), C.POINTER(C.c_size_t)()
    args = (None, None, _fp(a), C.c_size_t(len(a)), C.byref(lr), C.byref(lo), C.byref(nl))
    if indexed:
        _lib.check(lib.ocrs_engine_find_text_lines_indexed(*args, C.byref(wi)))
    else:
        _lib.check(lib.ocrs_engine_find_text_lines(*args))
    offs = [lo[i] for i in range(nl.value + 1)]
    flat = np.ctypeslib.as_array(lr, shape=(max(len(a), 1) * 6,))[: len(a) * 6].reshape(-1, 6).copy()
    idx = np.array([wi[i] for i in range(len(a))], np.int64) if indexed else None
    for p in (lr, lo) + ((wi,) if indexed else ()):
        lib.ocrs_buffer_free(p)
    return flat, offs, idx


def _batch(lib, pages, indexed):
    """ocrs_engine_find_text_lines_batch[_indexed] -> (rects, line offsets, page line offsets, word_index or None)."""
    n = len(pages)
    woffs = np.zeros(n + 1, np.uintp)
    for i, w in enumerate(pages):
        woffs[i + 1] = woffs[i] + len(w)
    allw = np.ascontiguousarray(np.concatenate([np.asarray(w, np.float32).reshape(-1, 6) for w in pages]))
    lr, lo, po, wi = C.POINTER(C.c_float)(), C.POINTER(C.c_size_t)(), C.POINTER(C.c_size_t)(), C.POINTER(C.c_size_t)()
    args = (None, C.c_size_t(n), _fp(allw), woffs.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(lr), C.byref(lo), C.byref(po))
    if indexed:
        _lib.check(lib.ocrs_engine_find_text_lines_batch_indexed(*args, C.byref(wi)))
    else:
        _lib.check(lib.ocrs_engine_find_text_lines_batch(*args))
    poffs = [po[i] for i in range(n + 1)]
    loffs = [lo[i] for i in range(poffs[n] + 1)]
    flat = np.ctypeslib.as_array(lr, shape=(max(len(allw), 1) * 6,))[: len(allw) * 6].reshape(-1, 6).copy()
    idx = np.array([wi[i] for i in range(len(allw))], np.int64) if indexed else None
    for p in (lr, lo, po) + ((wi,) if indexed else ()):
        lib.ocrs_buffer_free(p)
    return flat, loffs, poffs, idx


def _check_indexed(lib, a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 6)
    plain = _one(lib, a, False)
    rects, offs, idx = _one(lib, a, True)
    assert rects.tobytes() == plain[0].tobytes() and offs == plain[1]
    assert sorted(idx.tolist()) == list(range(len(a))), "word_index is a permutation"
    assert a[idx].tobytes() == rects.tobytes(), "input[word_index[k]] is output rect k, bit for bit"
    return idx


def _kat_words():
    left = K.gen_rect_grid((0, 0), (10, 5), (5, 5), (3, 2))
    lb = K.union_rects(left)
    right = K.gen_rect_grid((0, lb[3] + 20), (10, 5), (5, 5), (3, 2))
    words = K.xorshift_shuffle([RotatedRect.from_rect(Rect(*r)) for r in left + right], 1234)
    return np.array([w.to_array() for w in words], np.float32).reshape(-1, 6)


def _random_layout(seed):
    """The random multi-column layouts of the existing layout tests (test_host_cpu.py)."""
    rng = np.random.default_rng(seed)
    words = []
    for c in range(int(rng.integers(1, 4))):
        x0, y = 20 + c * 330, 20
        for _ in range(int(rng.integers(8, 25))):
            h = int(rng.integers(10, 22))
            x = x0 + int(rng.integers(0, 20))
            for _ in range(int(rng.integers(2, 8))):
                w = int(rng.integers(15, 60))
                if x + w > x0 + 300:
                    break
                words.append([x + w / 2, y + h / 2, 0.0, 1.0, w + 6, h + 6])
                x += w + int(rng.integers(4, 14))
            y += h + int(rng.integers(4, 30))
    a = np.array(words, np.float32).reshape(-1, 6)
    return a[rng.permutation(len(a))]


def test_find_text_lines_indexed_on_the_layout_fixtures(lib):
    idx = _check_indexed(lib, _kat_words())
    assert len(idx) == 100
    for seed in (0, 1):
        a = np.load(os.path.join(GOLDEN, "bench_page_words_seed%d.npy" % seed))
        assert len(a) > 600
        idx = _check_indexed(lib, a)
        assert not np.array_equal(idx, np.arange(len(a))), "reading order is not detection order on these pages"
    for seed in (0, 1, 2, 3):
        _check_indexed(lib, _random_layout(seed))
    assert _one(lib, np.zeros((0, 6), np.float32), True)[1] == [0]


def test_find_text_lines_indexed_keeps_identical_rects_apart(lib):
    a = _random_layout(5)
    a = np.concatenate([a, a[3:4], a[3:4]])          # three copies of one rect
    idx = _check_indexed(lib, a)
    dup = {3, len(a) - 2, len(a) - 1}
    assert dup <= set(idx.tolist())                   # each copy has its own index (a match by value could not tell them apart)
    two = np.array([[50, 20, 0, 1, 40, 16], [50, 20, 0, 1, 40, 16]], np.float32)
    assert sorted(_check_indexed(lib, two).tolist()) == [0, 1]


def test_find_text_lines_batch_indexed(lib):
    pages = [np.load(os.path.join(GOLDEN, "bench_page_words_seed0.npy")), _kat_words(), np.zeros((0, 6), np.float32),
             _random_layout(2), np.load(os.path.join(GOLDEN, "bench_page_words_seed1.npy"))]
    plain = _batch(lib, pages, False)
    rects, loffs, poffs, idx = _batch(lib, pages, True)
    assert rects.tobytes() == plain[0].tobytes() and loffs == plain[1] and poffs == plain[2]
    at = 0
    for p, words in enumerate(pages):
        n = len(words)
        mine = idx[at:at + n]
        assert sorted(mine.tolist()) == list(range(n)), "page %d: a permutation of its own words" % p
        assert np.asarray(words, np.float32).reshape(-1, 6)[mine].tobytes() == rects[at:at + n].tobytes()
        one = _one(lib, words, True)                   # the batch is the single call, page by page
        assert np.array_equal(one[2], mine) and one[0].tobytes() == rects[at:at + n].tobytes()
        assert loffs[poffs[p]] == at
        at += n
    assert at == len(rects)


# ---------------------------------------------------------------- the definition on hand-made maps
THR, MIN_AREA = 0.2, 100.0


def test_reference_ring_with_an_island_in_its_hole():
    P = np.zeros((48, 56), np.float32)
    P[5:31, 5:31] = 0.5
    P[10:26, 10:26] = 0.0          # the hole ...
    P[13:23, 13:23] = 0.875        # ... and a 10 x 10 island in it: a component of its own, not External
    rects, score, pixels, n_ext = DR.reference(P, THR, MIN_AREA, count=True)
    assert n_ext == 1 and len(rects) == 1
    assert pixels.dtype == np.uint32 and pixels.tolist() == [26 * 26 - 16 * 16]
    assert score.dtype == np.float32 and score.tolist() == [0.5]          # neither hole nor island weigh in
    assert rects[0][4] * rects[0][5] == 31.0 * 31.0                       # 25 + 2 * 3 a side
    # the island alone is a word
    Q = np.zeros_like(P)
    Q[13:23, 13:23] = 0.875
    r2, s2, p2 = DR.reference(Q, THR, MIN_AREA)
    assert p2.tolist() == [100] and s2.tolist() == [0.875]


def test_reference_diagonal_only_contacts_join_components():
    P = np.zeros((40, 64), np.float32)
    P[4:16, 4:16] = 0.25
    P[16:28, 16:28] = 0.75         # touches the first square at one corner, diagonally: 8-connected
    P[4:16, 30:42] = 0.5           # two pixels of background away from anything
    P[17:29, 43:55] = 0.5          # NOT touching [4:16, 30:42]: a row and a column apart
    rects, score, pixels, n_ext = DR.reference(P, THR, MIN_AREA, count=True)
    assert n_ext == 3
    assert pixels.tolist() == [288, 144, 144]
    assert score.tolist() == [0.5, 0.5, 0.5]
    lab = DR.label8(P > THR)
    assert lab[4, 4] == lab[27, 27] and lab[4, 30] != lab[17, 43] and lab[0, 0] == -1


def test_reference_threshold_one_above_one_and_infinity():
    thr = np.float32(0.2)
    P = np.zeros((40, 80), np.float32)
    P[4:16, 4:16] = 1.0
    P[4:16, 24:36] = 1.5
    P[4:16, 44:56] = np.inf
    P[20:32, 4:16] = 0.6
    P[24:28, 8:12] = thr            # exactly the threshold: not text (strict >), a 16-pixel hole
    P[20:32, 24:36] = np.nextafter(thr, np.float32(1.0))    # the smallest value that is text
    P[20:32, 44:56] = thr           # a whole blob at the threshold: no component
    P[20:32, 62:74] = np.nan        # NaN never passes
    rects, score, pixels, n_ext = DR.reference(P, float(thr), MIN_AREA, count=True)
    assert n_ext == 5
    assert pixels.tolist() == [144, 144, 144, 144 - 16, 144]
    assert score[:3].tolist() == [1.0, 1.0, 1.0]             # 1, above 1 and +inf all count as 2^24
    q = int(DR.quantise(np.float32(0.6)))
    assert q == int(np.floor(float(np.float32(0.6)) * 2 ** 24))
    assert DR.bits(score[3:4])[0] == DR.bits(np.float32(q * 128 / (128 * 16777216.0)))[0]
    low = np.nextafter(thr, np.float32(1.0))                 # below 1/2 the fixed point drops bits (floor): less than 2^-24 a pixel
    assert score[4] == np.float32(np.floor(float(low) * 2 ** 24) / 2 ** 24) and float(thr) - 2.0 ** -24 < score[4] < low
    assert DR.quantise(np.array([-1.0, 0.0, 1.0, 2.0, np.inf], np.float32)).tolist() == [0, 0, 2 ** 24, 2 ** 24, 2 ** 24]


def test_reference_drops_components_below_min_area_and_keeps_alignment():
    P = np.zeros((40, 90), np.float32)
    P[4:16, 4:16] = 0.3125
    P[6:9, 24:27] = 0.9            # 3 x 3: (2 + 6)^2 = 64 < 100, dropped
    P[4:16, 34:46] = 0.4375
    P[20:22, 4:6] = 0.9            # dropped
    P[20:32, 34:46] = 0.6875
    rects, score, pixels, n_ext = DR.reference(P, THR, MIN_AREA, count=True)
    assert n_ext == 5 and len(rects) == 3
    assert pixels.tolist() == [144, 144, 144]
    assert [DR.bits(s).item() for s in score] == [DR.bits(np.float32(v)).item() for v in (0.3125, 0.4375, 0.6875)]
    from oracle import clib
    assert np.array_equal(rects, clib.component_rects((P > THR).astype(np.uint8), 3.0, MIN_AREA))
