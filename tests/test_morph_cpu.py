"""Stroke repair, host side: the new symbols and parameter checks of the library, and the properties the
definition in tests/morph_ref.py promises: against plain loops over the rectangle, on the page with a NaN beside a dark
pixel, its algebra bit for bit, and what it repairs on the damaged text page.  No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import models_util as M
import morph_ref as R
from test_gpu_binarize import planted

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["ocrs_morph_params_default", "ocrs_morph_params_check", "ocrs_engine_morph_page", "ocrs_engine_morph_pages"]
F = np.float32
U = np.uint32
PAGES = [(1, 1), (5, 9), (9, 5), (17, 23), (20, 20), (33, 31)]
RADII = [(1, 1), (3, 0), (0, 3), (2, 5), (63, 63), (7, 1)]   # (rx, ry)


@pytest.fixture(scope="module")
def lib():
    from ocrs_amd import _lib, build
    build.build()
    return _lib.lib()


def noise(seed, h, w, ink=0.5):
    """[h, w] float32 noise with the planted words: both NaN kinds, +-inf, +-0, denormals, huge values."""
    return planted((np.random.default_rng(seed).random((h, w), dtype=F) - F(ink)).astype(F), seed)


def same(a, b):
    return a[0].view(U).tobytes() == b[0].view(U).tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ---------------------------------------------------------------- 1. symbols, sources, parameters
def test_new_symbols_are_exported_and_declared(lib):
    from ocrs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ocrs_amd.h")).read()
    declared = set(re.findall(r"OCRS_API[^;(]*?\b(ocrs_\w+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(lib, name), name
    for name in ("ocrs_morph_params", "ocrs_morph_info"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    for i, name in enumerate(R.OPS):
        assert re.search(r"#define\s+OCRS_MORPH_%s\s+%d\b" % (name.upper(), i), hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert C.sizeof(_lib.MorphParams) == 12 and C.sizeof(_lib.MorphInfo) == 32
    assert [f[0] for f in _lib.MorphInfo._fields_] == list(R.INFO_KEYS)


def test_sources_are_built():
    from ocrs_amd import build
    assert "kernels_morph.hip" in build.SOURCES and "morph.cpp" in build.SOURCES
    for name in ("kernels_morph.hip", "morph.cpp"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name


def test_default_params_and_refused_params(lib):
    import ocrs_amd
    from ocrs_amd import _lib
    p = _lib.MorphParams(7, 7, 7)
    assert lib.ocrs_morph_params_default(C.byref(p)) == 0
    assert (p.op, p.rx, p.ry) == (R.OPS.index("close"), 1, 1)
    assert ocrs_amd.morph_params() == R.default_params() == {"op": "close", "rx": 1, "ry": 1}
    assert ocrs_amd.MORPH_OPS == R.OPS
    assert lib.ocrs_morph_params_default(None) == 1 and lib.ocrs_morph_params_check(None) == 1

    def checked(op=2, rx=1, ry=1):
        q = _lib.MorphParams(op, rx, ry)
        return lib.ocrs_morph_params_check(C.byref(q))

    for op, (rx, ry) in itertools.product(range(4), ((1, 1), (63, 63), (0, 1), (1, 0), (63, 0), (0, 63), (2, 5))):
        assert R.valid_params(R.OPS[op], rx, ry) and checked(op, rx, ry) == 0, (op, rx, ry)
        R.morph(np.zeros((3, 3), F), R.OPS[op], rx, ry)
    for kw in ({"op": -1}, {"op": 4}, {"op": 1 << 30}, {"rx": -1}, {"rx": 64}, {"ry": -1}, {"ry": 64}, {"rx": 0, "ry": 0}, {"rx": 1 << 30},
               {"rx": 64, "ry": 0}):
        assert checked(**kw) == 1, kw   # OCRS_ERR_INVALID_ARGUMENT
        if "op" not in kw:
            assert not R.valid_params(**kw), kw
            with pytest.raises(ValueError):
                R.morph(np.zeros((3, 3), F), **kw)
    assert not R.valid_params(op="dilate")
    # the Python side: op by name, ry follows rx unless given, and what is out of range is the library's to refuse
    assert ocrs_amd.morph_params(op="thicken", rx=1, ry=0) == {"op": "thicken", "rx": 1, "ry": 0}
    assert ocrs_amd.morph_params(rx=5) == {"op": "close", "rx": 5, "ry": 5}
    assert ocrs_amd.morph_params(op="open", ry=7) == {"op": "open", "rx": 1, "ry": 7}
    for kw in ({"rx": 0}, {"rx": 64}, {"ry": 64}, {"rx": -1, "ry": 1}, {"rx": 0, "ry": 0}):
        with pytest.raises(ocrs_amd.OcrsError) as e:
            ocrs_amd.morph_params(**kw)
        assert e.value.status_name == "INVALID_ARGUMENT", kw
    with pytest.raises(ValueError):
        ocrs_amd.morph_params(op="dilate")


# ---------------------------------------------------------------- 2. the restatement against plain loops
def test_keys_order_every_word_that_is_not_nan():
    w = np.array([0xFF800000, 0xFF7FFFFF, 0xC0400000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x40400000, 0x7F7FFFFF, 0x7F800000], U)
    k = R.keys(w)
    assert (np.diff(k.astype(np.int64)) > 0).all(), "-inf < -max < -3 < -denormal < -0.0 < +0.0 < denormal < 3 < max < +inf"
    assert np.array_equal(R.unkeys(k), w)
    assert k.min() > 0 and k.max() < 0xFFFFFFFF, "the empty keys belong to no counted word"
    assert R.is_nan(np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0xFFFFFFFF], U)).all() and not R.is_nan(w).any()
    assert np.array_equal(R.keys(w ^ R.SIGN), ~k), "key(-v) = ~key(v)"


@pytest.mark.parametrize("shape", PAGES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_plain_loops_over_the_rectangle(shape):
    page = noise(shape[0] * 100 + shape[1], *shape, ink=0.4)
    for (rx, ry), op in itertools.product(RADII, R.OPS):
        assert same(R.morph(page, op, rx, ry), R.brute(page, op, rx, ry)), (shape, op, rx, ry)


# ---------------------------------------------------------------- 3. the named case
def test_nan_beside_dark():
    page, rx, ry = R.nan_beside_dark()
    dark = page.view(U)[1, 0]
    for fn in (R.morph, R.brute):
        out, mask, info = fn(page, "thicken", rx, ry)
        got = out.view(U)
        assert got[0, 1] == dark, "(0, 1) sees the dark pixel across the NaN"
        assert got[1, 1] == page.view(U)[1, 1] and mask[1, 1] == 0, "the NaN pixel keeps its word"
        assert (got[:, 0] == dark).all() and got[2, 1] == dark and (got[:, 2] == page.view(U)[:, 2]).all()
        assert info == {"counted": 8, "changed": 4, "ink_before": 1, "ink_after": 5}
    assert same(R.morph(page, "close", rx, ry), R.brute(page, "close", rx, ry))


# ---------------------------------------------------------------- 4. algebra, bit for bit
@pytest.mark.parametrize("shape", PAGES, ids=lambda s: "%dx%d" % s)
def test_algebra(shape):
    page = noise(shape[0] * 100 + shape[1], *shape, ink=0.4)
    w = page.view(U)
    nan = R.is_nan(w)
    k = R.keys(w).astype(np.int64)
    flipped = (w ^ R.SIGN).view(F)   # the sign of every word flipped: a NaN stays a NaN
    for rx, ry in RADII:
        closed, opened = R.morph(page, "close", rx, ry)[0], R.morph(page, "open", rx, ry)[0]
        again = R.morph(closed, "close", rx, ry)
        assert again[0].view(U).tobytes() == closed.view(U).tobytes() and again[2]["changed"] == 0, "close is idempotent"
        again = R.morph(opened, "open", rx, ry)
        assert again[0].view(U).tobytes() == opened.view(U).tobytes() and again[2]["changed"] == 0, "open is idempotent"
        assert (R.keys(closed.view(U)).astype(np.int64)[~nan] <= k[~nan]).all(), "close never raises a key"
        assert (R.keys(opened.view(U)).astype(np.int64)[~nan] >= k[~nan]).all(), "open never lowers one"
        thin = R.morph(page, "thin", rx, ry)[0].view(U)
        dual = R.morph(flipped, "thicken", rx, ry)[0].view(U) ^ R.SIGN
        assert np.array_equal(thin[~nan], dual[~nan]) and np.array_equal(thin[nan], w[nan]), "thin is thicken of the flipped page"
        for op in R.OPS:
            flat = np.full(shape, F(-0.125), F)
            out, mask, info = R.morph(flat, op, rx, ry)
            assert out.tobytes() == flat.tobytes() and info == {"counted": flat.size, "changed": 0, "ink_before": flat.size, "ink_after": flat.size}
            assert (mask == 1).all()
            nans = np.full(shape, np.nan, F)
            nans.view(U)[0, 0] = 0xFFC12345
            out, mask, info = R.morph(nans, op, rx, ry)
            assert out.view(U).tobytes() == nans.view(U).tobytes() and not mask.any() and info == dict.fromkeys(R.INFO_KEYS, 0)


# ---------------------------------------------------------------- 5. what it is for
@pytest.fixture(scope="module")
def text_page():
    """The 512 x 512 text page of DESIGN.md §7.9 prepared by the oracle."""
    from ocrs_amd import synth
    from oracle import pipeline as OP
    from oracle.nn import OracleGraph, OracleModel
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                       recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))
    px = synth.synthetic_page(3, 512, 512, 30, 2, 1)
    return np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), F)[0])


def test_close_repairs_broken_strokes_on_the_text_page(text_page):
    clean = text_page
    truth = clean < F(0)
    whole = R.components(truth)
    for name, damaged in (("30 % of the ink pixels lost", R.break_strokes(clean, 0.3, 7)), ("every third column lost", R.drop_columns(clean, 3))):
        ink = damaged < F(0)
        f_damaged, n_damaged = R.f_measure(ink, truth), R.components(ink)
        closed = R.morph(damaged, "close", 1, 1)[1] & 1 == 1
        thick = R.morph(damaged, "thicken", 1, 1)[1] & 1 == 1
        f_closed, n_closed, f_thick = R.f_measure(closed, truth), R.components(closed), R.f_measure(thick, truth)
        print("%s: %d components (clean %d), F %.3f; after close at radius 1: %d components, F %.3f; after thicken alone: F %.3f"
              % (name, n_damaged, whole, f_damaged, n_closed, f_closed, f_thick))
        assert f_closed > f_damaged, name
        assert n_closed <= whole, name
        assert f_thick < f_closed, name
