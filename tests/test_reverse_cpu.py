"""Reverse-video repair, host side: the two implementations of tests/reverse_ref.py against each other and
against hand-stated answers on planted pages; every result word the source's or the source's with the sign bit flipped;
idempotence; the library's parameter checks and its new symbols against the restatement.  No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import reverse_pages as P
import reverse_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["ocrs_reverse_params_default", "ocrs_reverse_params_check", "ocrs_engine_unreverse_page", "ocrs_engine_unreverse_pages"]
F = np.float32
SWEEP = [{"min_height": mh, "min_width": mw, "min_fill": mf, "min_holes": n, "max_hole": Hm}
         for mh, mw, mf, n, Hm in itertools.product((1, 2, 5), (1, 2, 5), (0.0, 0.3, 0.6), (0, 1, 2), (0, 1, 3))]
SPECIAL = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x80000001], np.uint32)


@pytest.fixture(scope="module")
def lib():
    from ocrs_amd import _lib, build
    build.build()
    return _lib.lib()


def test_new_symbols_are_exported_and_declared(lib):
    from ocrs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ocrs_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"OCRS_API ocrs_status %s\(" % name, hdr), name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(lib, name), name
    for name in ("ocrs_reverse_params", "ocrs_reverse_info"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert C.sizeof(_lib.ReverseParams) == 24 and C.sizeof(_lib.ReverseInfo) == 72
    assert [f[0] for f in _lib.ReverseInfo._fields_] == list(R.INFO_KEYS)
    assert [f[0] for f in _lib.ReverseParams._fields_] == list(R.default_params())


# ------------------------------------------------------------------ the two implementations of the restatement
def random_page(seed, h, w, density, special=False):
    rng = np.random.default_rng(seed)
    a = np.where(rng.random((h, w)) < density, F(-0.3), F(0.3)).astype(F)
    if special:   # NaNs, infinities, zeros of both signs and denormals among them
        flat = a.reshape(-1).view(np.uint32)
        n = min(len(SPECIAL), flat.size)
        flat[rng.choice(flat.size, size=n, replace=False)] = SPECIAL[:n]
    return a


def assert_words(page, out, mask):
    """Every result word is the source's, or the source's with the sign bit flipped exactly where mask bit 0 says."""
    diff = page.view(np.uint32) ^ out.view(np.uint32)
    assert np.array_equal(diff, (mask & 1).astype(np.uint32) << np.uint32(31))


def test_the_two_implementations_agree_on_random_pages():
    shapes = [(24, 24), (17, 23), (1, 1), (1, 19), (20, 1), (2, 2), (24, 9), (13, 24), (24, 24)]
    pages = [random_page(100 + i, h, w, d, special=i % 2 == 1) for i, ((h, w), d) in enumerate(zip(shapes * 2, (0.45, 0.65, 0.85) * 6))]
    most = dict.fromkeys(R.INFO_KEYS, 0)
    for i, kw in enumerate(SWEEP * 2):
        page = pages[i % len(pages)]
        fast, slow = R.unreverse(page, **kw), R.unreverse_slow(page, **kw)
        assert R.same(fast, slow), (i, kw, fast[2], slow[2])
        assert_words(page, fast[0], fast[1])
        for k in R.INFO_KEYS:
            most[k] = max(most[k], fast[2][k])
    assert all(v > 0 for v in most.values()), most   # the sweep reaches every counter


def test_threshold_nan_and_equality():
    page = np.array([[-0.5, -0.5, -0.5, -0.5, -0.5], [-0.5, np.nan, -0.5, 0.1, -0.5], [-0.5, -0.5, -0.5, -0.5, -0.5]], F)
    kw = {"min_height": 3, "min_width": 5, "min_fill": 0.5, "min_holes": 2}
    for thr, holes in ((0.0, 2), (0.1, 2), (0.2, 0)):   # NaN is never ink; v == threshold is not ink; above it the mark is ink
        fast, slow = R.unreverse(page, threshold=thr, **kw), R.unreverse_slow(page, threshold=thr, **kw)
        assert R.same(fast, slow) and fast[2]["holes"] == holes and fast[2]["inverted"] == (15 if holes else 0), (thr, fast[2])
        assert_words(page, fast[0], fast[1])
    out = R.unreverse(page, **kw)[0]
    assert np.isnan(out[1, 1]) and out.view(np.uint32)[1, 1] == page.view(np.uint32)[1, 1] ^ 0x80000000   # the payload with its sign flipped


# ------------------------------------------------------------------ hand-stated answers
@pytest.fixture(scope="module")
def planted():
    return P.patterns(36, 70, 2, 3)


def test_planted_pages_have_their_hand_stated_answers(planted):
    assert len(planted) >= 16
    for name, page, kw, flipped, info in planted:
        fast, slow = R.unreverse(page, **kw), R.unreverse_slow(page, **kw)
        assert R.same(fast, slow), name
        out, mask, got = fast
        assert np.array_equal((mask & 1).astype(bool), flipped), name
        assert {k: got[k] for k in info} == info, (name, got)
        assert_words(page, out, mask)
        assert got["inverted"] == int(flipped.sum()) == got["panel_pixels"] + got["hole_pixels"], name
        assert np.array_equal((mask & 4) != 0, ((mask & 2) != 0) & flipped), name   # a panel's pixels are flipped pixels of M
        assert not ((mask & 2) != 0)[(mask & 8) != 0].any(), name                   # a hole lies outside M


def test_a_second_application_changes_nothing(planted):
    for name, page, kw, flipped, _ in planted:
        once = R.unreverse(page, **kw)[0]
        twice, mask, info = R.unreverse(once, **kw)
        assert twice.tobytes() == once.tobytes() and info["panels"] == 0 and info["inverted"] == 0 and not (mask & 5).any(), name


def test_the_defaults_leave_small_print_alone():
    """A 31-high band is under min_height 32; at 32 x 64 with three marks it is a panel: the defaults, as stated."""
    assert R.default_params() == {"threshold": 0.0, "min_height": 32, "min_width": 64, "min_fill": 0.4, "min_holes": 3, "max_hole": 0}
    for hh, ww, panels in ((31, 64, 0), (32, 63, 0), (32, 64, 1)):
        a = P.canvas(40, 72)
        a[2:2 + hh, 3:3 + ww] = P.INK
        for dx in (5, 15, 25):
            a[10:14, 3 + dx:7 + dx] = P.PAPER
        assert R.unreverse(a)[2]["panels"] == panels, (hh, ww)


# ------------------------------------------------------------------ the library's checks
def test_parameter_checks_against_the_restatement(lib):
    from ocrs_amd import _lib, reverse_params
    p = _lib.ReverseParams()
    assert lib.ocrs_reverse_params_default(C.byref(p)) == 0
    d = R.default_params()
    assert {k: getattr(p, k) for k in d if k != "min_fill"} == {k: v for k, v in d.items() if k != "min_fill"} and p.min_fill == F(0.4)
    assert lib.ocrs_reverse_params_default(None) == 1 and lib.ocrs_reverse_params_check(None) == 1
    nan, inf = float("nan"), float("inf")
    ok = (0.0, 32, 64, 0.4, 3, 0)
    cases = [(ok, 0), ((-0.25, 1, 1, 0.0, 0, 0), 0), ((1e30, 65535, 65535, 1.0, 2 ** 31 - 1, 2 ** 31 - 1), 0),
             ((nan,) + ok[1:], 1), ((inf,) + ok[1:], 1), ((-inf,) + ok[1:], 1),
             ((0.0, 0, 64, 0.4, 3, 0), 1), ((0.0, 65536, 64, 0.4, 3, 0), 1), ((0.0, -1, 64, 0.4, 3, 0), 1),
             ((0.0, 32, 0, 0.4, 3, 0), 1), ((0.0, 32, 65536, 0.4, 3, 0), 1), ((0.0, 32, -5, 0.4, 3, 0), 1),
             ((0.0, 32, 64, -0.001, 3, 0), 1), ((0.0, 32, 64, 1.001, 3, 0), 1), ((0.0, 32, 64, nan, 3, 0), 1), ((0.0, 32, 64, inf, 3, 0), 1),
             ((0.0, 32, 64, 0.4, -1, 0), 1), ((0.0, 32, 64, 0.4, 3, -1), 1)]
    for vals, status in cases:
        assert lib.ocrs_reverse_params_check(C.byref(_lib.ReverseParams(*vals))) == status, vals
        assert R.valid_params(*vals) == (status == 0), vals
    got = reverse_params()
    assert {k: got[k] for k in got if k != "min_fill"} == {k: v for k, v in d.items() if k != "min_fill"} and got["min_fill"] == float(F(0.4))
    assert reverse_params(min_height=8, min_width=24, min_fill=0.5, min_holes=0, max_hole=9, threshold=0.25) == \
        {"min_height": 8, "min_width": 24, "min_fill": 0.5, "min_holes": 0, "max_hole": 9, "threshold": 0.25}
    for kw in ({"min_height": 0}, {"min_width": 65536}, {"min_fill": 1.5}, {"min_fill": nan}, {"min_holes": -1}, {"max_hole": -1},
               {"threshold": nan}, {"min_height": 2 ** 40}):
        with pytest.raises(_lib.OcrsError) as e:
            reverse_params(**kw)
        assert e.value.status_name == "INVALID_ARGUMENT", kw
    assert [R.fill_q8(f) for f in (0.0, 0.3, 0.4, 0.6, 1.0)] == [0, 77, 102, 154, 256]
