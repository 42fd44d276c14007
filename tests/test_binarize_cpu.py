"""Adaptive binarisation, host side: the new symbols and parameter checks of the library, and the
properties the definition in tests/binarize_ref.py promises: against an independent float64 form, on hand-made pages, on
exact ties and on the shaded text page.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import binarize_ref as B
import models_util as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["ocrs_binarize_params_default", "ocrs_binarize_params_check", "ocrs_engine_binarize_page", "ocrs_engine_binarize_pages"]
F = np.float32
MARGIN = 1e-6   # of |b - T| in bins under which the float64 form is not asked: its sums are exact (integers under 2^53), so
                # its error is that of a dozen float64 operations on values under 2^16, some 1e-11; 1e-6 is far above it


def level(b):
    """A grey level in the middle of bin b."""
    return F((b + 0.5) / 256.0 - 0.5)


@pytest.fixture(scope="module")
def lib():
    from ocrs_amd import _lib, build
    build.build()
    return _lib.lib()


def test_new_symbols_are_exported_and_declared(lib):
    from ocrs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ocrs_amd.h")).read()
    declared = set(re.findall(r"OCRS_API[^;(]*?\b(ocrs_\w+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(lib, name), name
    for name in ("ocrs_binarize_params", "ocrs_binarize_info"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert C.sizeof(_lib.BinarizeParams) == 20 and C.sizeof(_lib.BinarizeInfo) == 24
    assert [f[0] for f in _lib.BinarizeInfo._fields_] == list(B.INFO_KEYS)


def test_sources_are_built():
    from ocrs_amd import build
    assert "kernels_binarize.hip" in build.SOURCES and "binarize.cpp" in build.SOURCES
    for name in ("kernels_binarize.hip", "binarize.cpp"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name


def test_default_params_and_refused_params(lib):
    import ocrs_amd
    from ocrs_amd import _lib
    p = _lib.BinarizeParams(1, 1, 1, 1.0, 1.0)
    assert lib.ocrs_binarize_params_default(C.byref(p)) == 0
    assert (p.radius, p.k_q8, p.keep_ink) == (15, 87, 0) and p.ink_level != p.ink_level and p.paper != p.paper
    assert ocrs_amd.binarize_params() == B.default_params() == {"radius": 15, "k_q8": 87, "keep_ink": False, "ink_level": None, "paper": None}
    assert B.k_to_q8(0.34) == 87 and ocrs_amd.binarize_params(k=0.34)["k_q8"] == 87
    assert lib.ocrs_binarize_params_default(None) == 1 and lib.ocrs_binarize_params_check(None) == 1
    nan, inf = float("nan"), float("inf")

    def checked(radius=15, k_q8=87, keep_ink=0, ink_level=nan, paper=nan):
        q = _lib.BinarizeParams(radius, k_q8, keep_ink, ink_level, paper)
        return lib.ocrs_binarize_params_check(C.byref(q))

    for kw in ({"radius": 1}, {"radius": 127}, {"k_q8": 0}, {"k_q8": 256}, {"keep_ink": 1}, {"ink_level": -0.0}, {"ink_level": 3.0e38},
               {"paper": -7.0}, {"paper": nan}, {"ink_level": nan}, {"radius": 31, "k_q8": 128, "keep_ink": 1, "ink_level": -0.25, "paper": 0.25}):
        assert B.valid_params(**kw), kw
        assert checked(**kw) == 0, kw
        B.binarize(np.zeros((3, 3), F), **kw)
    for kw in ({"radius": 0}, {"radius": 128}, {"radius": -1}, {"radius": 1 << 30}, {"k_q8": -1}, {"k_q8": 257}, {"keep_ink": 2}, {"keep_ink": -1},
               {"ink_level": inf}, {"ink_level": -inf}, {"paper": inf}, {"paper": -inf}):
        assert not B.valid_params(**kw), kw
        assert checked(**kw) == 1, kw   # OCRS_ERR_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            B.binarize(np.zeros((3, 3), F), **kw)
    # the Python side: k is rounded to 1/256, and what is out of range is the library's to refuse
    for k, kq in ((0.0, 0), (1.0, 256), (0.5, 128), (0.001, 0), (0.002, 1), (0.998, 255), (0.9981, 256)):
        assert ocrs_amd.binarize_params(k=k)["k_q8"] == kq == B.k_to_q8(k), k
    assert ocrs_amd.binarize_params(radius=127, k=1.0, keep_ink=True, ink_level=-0.25, paper=0.25) == \
        {"radius": 127, "k_q8": 256, "keep_ink": True, "ink_level": -0.25, "paper": 0.25}
    for kw in ({"k": -0.01}, {"k": 1.01}, {"k": 100.0}, {"radius": 0}, {"radius": 128}, {"paper": inf}, {"ink_level": -inf}):
        with pytest.raises(ocrs_amd.OcrsError) as e:
            ocrs_amd.binarize_params(**kw)
        assert e.value.status_name == "INVALID_ARGUMENT", kw


# ---------------------------------------------------------------- the restatement against an independent float64 form
def float_form(page, r, k):
    """Sauvola's formula as written, in float64, box sums by scipy's uniform_filter over a zero-padded page -> (b, T), NaN
    where nothing is counted."""
    from scipy.ndimage import uniform_filter
    b = B.bins(page)
    c = (b >= 0).astype(np.float64)
    bb = np.where(b >= 0, b, 0).astype(np.float64)
    size = 2 * r + 1

    def box(a):
        return np.rint(uniform_filter(a, size=size, mode="constant", cval=0.0) * (size * size))   # sums of integers: integers

    n, S, Q = box(c), box(bb), box(bb * bb)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = S / n
        s = np.sqrt(np.maximum(Q / n - m * m, 0.0))
        T = m * (1.0 + k * (s / 128.0 - 1.0))
    return b, T


def noise(seed, h, w, ink=0.5):
    return (np.random.default_rng(seed).random((h, w), dtype=F) - F(ink)).astype(F)


@pytest.fixture(scope="module")
def text_pages():
    """The 512 x 512 text page of DESIGN.md §7.9 prepared by the oracle, and the same under the shade of §7.10."""
    from ocrs_amd import synth
    from oracle import pipeline as OP
    from oracle.nn import OracleGraph, OracleModel
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                       recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))
    px = synth.synthetic_page(3, 512, 512, 30, 2, 1)
    clean = np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), F)[0])
    return clean, B.shade(clean)


def test_restatement_equals_the_float64_form_outside_a_small_margin(text_pages):
    pages = [("noise", noise(1, 97, 211)), ("dark noise", noise(2, 129, 127, ink=0.9)), ("shaded text", text_pages[1]),
             ("noise with holes", np.where(noise(3, 97, 211) > F(0.3), F(np.nan), noise(4, 97, 211)).astype(F))]
    for name, page in pages:
        for r, kq in ((1, 87), (2, 256), (15, 87), (31, 1), (127, 128)):
            _, mask, _ = B.binarize(page, radius=r, k_q8=kq)
            b, T = float_form(page, r, kq / 256.0)
            asked = (b >= 0) & (np.abs(b - T) > MARGIN)
            left_out = 1.0 - asked.sum() / max(int((b >= 0).sum()), 1)
            print("%s, r = %d, kq = %d: %.4f %% of the counted pixels within %g of their threshold" % (name, r, kq, 100.0 * left_out, MARGIN))
            assert left_out <= 0.01, (name, r, kq, left_out)
            assert np.array_equal(mask.astype(bool)[asked], (b < T)[asked]), (name, r, kq)


def test_limbs_equal_python_integers_at_the_largest_window():
    # two-level pages at r = 127 on 300 x 300: the whole window inside the page, the products at their largest
    rng = np.random.default_rng(5)
    for lo, hi, kq in ((0, 255, 256), (254, 255, 256), (3, 250, 87), (255, 255, 256), (1, 255, 1)):
        page = np.where(rng.random((300, 300)) < 0.5, level(lo), level(hi)).astype(F)
        b, n, S, Q = B.window_sums(page, 127)
        assert n.max() == 255 * 255
        got = B.decide(b, n, S, Q, kq)
        want = np.array([B.decide_int(*t, kq) for t in zip(b.ravel().tolist(), n.ravel().tolist(), S.ravel().tolist(), Q.ravel().tolist())])
        assert np.array_equal(got.ravel(), want), (lo, hi, kq)


# ---------------------------------------------------------------- the window is clipped, not padded
@pytest.mark.parametrize("r", [1, 2, 15])
def test_a_single_dark_pixel_at_each_corner_and_edge(r):
    H, W = 41, 53
    sites = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    yy, xx = np.mgrid[0:H, 0:W]
    for y0, x0 in sites:
        page = np.full((H, W), level(200), F)
        page[y0, x0] = level(10)
        b, n, S, Q = B.window_sums(page, r)
        # by hand: the clipped window's sides, and whether it holds the dark pixel
        hy = np.minimum(yy + r, H - 1) - np.maximum(yy - r, 0) + 1
        hx = np.minimum(xx + r, W - 1) - np.maximum(xx - r, 0) + 1
        holds = (np.abs(yy - y0) <= r) & (np.abs(xx - x0) <= r)
        assert np.array_equal(n, hy * hx)
        assert np.array_equal(S, 200 * hy * hx - 190 * holds) and np.array_equal(Q, 40000 * hy * hx - (40000 - 100) * holds)
        corner = (y0 in (0, H - 1)) and (x0 in (0, W - 1))
        assert n[y0, x0] == ((r + 1) ** 2 if corner else (r + 1) * (2 * r + 1))   # a padded window would count (2 r + 1)^2
        _, mask, info = B.binarize(page, radius=r)
        assert mask[y0, x0] == 1 and info["ink"] == 1 and info["counted"] == H * W, (y0, x0)


# ---------------------------------------------------------------- ties and degenerate pages
def test_flat_pages_have_no_ink_and_degenerate_pages_go_through():
    with np.errstate(all="raise"):
        for b in (0, 128, 255):
            for kq in (0, 87, 256):
                page = np.full((37, 70), level(b), F)
                out, mask, info = B.binarize(page, radius=15, k_q8=kq)
                assert not mask.any() and info == {"counted": 37 * 70, "ink": 0, "ink_fill": -0.5, "paper_fill": 0.5}
                assert (out == F(0.5)).all()
        nans = np.full((20, 33), np.nan, F)
        nans.view(np.uint32)[3, 4] = 0xFFC12345
        out, mask, info = B.binarize(nans, radius=2)
        assert out.view(np.uint32).tobytes() == nans.view(np.uint32).tobytes() and not mask.any() and info["counted"] == 0 and info["ink"] == 0
        one = nans.copy()
        one[10, 10] = F(-0.5)
        for keep in (False, True):
            out, mask, info = B.binarize(one, radius=15, keep_ink=keep)
            assert info["counted"] == 1 and info["ink"] == 0 and out[10, 10] == F(0.5)   # n = 1: V = 0, a tie
            rest = np.ones(one.shape, bool)
            rest[10, 10] = False
            assert np.array_equal(out.view(np.uint32)[rest], one.view(np.uint32)[rest]) and not mask.any()
        out, mask, info = B.binarize(np.full((1, 1), F(-0.25), F), radius=127)
        assert info == {"counted": 1, "ink": 0, "ink_fill": -0.5, "paper_fill": 0.5} and out[0, 0] == F(0.5)


def test_the_planted_tie_is_paper_and_a_float64_evaluation_gets_it_wrong_or_right_by_luck():
    page, r, kq, ys, xs = B.tie_page()
    b, n, S, Q = B.window_sums(page, r)
    bb, nn, SS, QQ = (int(a[150, 150]) for a in (b, n, S, Q))
    assert (bb, nn, SS) == (32, 65025, 64 * 65025)
    V, A, Bq = nn * QQ - SS * SS, nn * 128 * (256 * (bb * nn - SS) + kq * SS), kq * SS
    assert A > 0 and A * A == Bq * Bq * V, "an exact tie"
    _, mask, _ = B.binarize(page, radius=r, k_q8=kq)
    assert not mask[ys, xs].any(), "the strict < makes a tie paper"
    assert mask[ys, xs].size == 46 * 46
    # one bin darker, or k one step larger... the same pixels are ink: the tie is the boundary
    darker = page.copy()
    darker[150, 150] = level(31)
    assert B.binarize(darker, radius=r, k_q8=kq)[1][150, 150] == 1
    f64 = float(A) < float(Bq) * float(np.sqrt(np.float64(V)))
    print("float64 evaluation of A < B sqrt(V) at the tie: %s (exact: False)" % f64)


# ---------------------------------------------------------------- keep_ink
def test_keep_ink_keeps_the_bits_of_ink_and_whitens_the_rest():
    page = np.full((40, 60), F(0.4), F)
    words = page.view(np.uint32)
    planted = {(5, 5): 0x80000000, (10, 20): 0xC0400000, (20, 30): 0xFF7FFFFF, (30, 40): 0xFF800000, (35, 50): 0xBE000001}   # -0.0, -3, -max, -inf, -0.125..
    nans = {(7, 7): 0x7FC00000, (8, 50): 0x7F800001, (25, 25): 0xFFC12345}
    for at, wd in list(planted.items()) + list(nans.items()):
        words[at] = wd
    page[15, 15] = F(3.0)   # out of range on the bright side: bin 255, not ink
    for r in (2, 15):
        out, mask, info = B.binarize(page, radius=r, keep_ink=True, paper=0.25)
        got = out.view(np.uint32)
        for at, wd in planted.items():
            assert mask[at] == 1 and got[at] == wd, (at, hex(got[at]))
        for at, wd in nans.items():
            assert mask[at] == 0 and got[at] == wd, (at, hex(got[at]))
        assert info["ink"] == len(planted) and info["counted"] == page.size - len(nans)
        rest = np.ones(page.shape, bool)
        for at in list(planted) + list(nans):
            rest[at] = False
        assert (got[rest] == np.array([0.25], F).view(np.uint32)[0]).all()
        flat, fmask, finfo = B.binarize(page, radius=r, ink_level=-0.25)
        assert np.array_equal(fmask, mask) and finfo["ink"] == info["ink"]
        for at in planted:
            assert flat[at] == F(-0.25)
        for at, wd in nans.items():
            assert flat.view(np.uint32)[at] == wd
        assert (flat[rest] == F(0.5)).all()


# ---------------------------------------------------------------- the shaded page
def test_the_local_decision_beats_every_global_threshold_on_the_shaded_page(text_pages):
    clean, shaded = text_pages
    truth = clean < F(0)
    _, mask, info = B.binarize(shaded)
    local = B.f_measure(mask.astype(bool), truth)
    best, at = B.best_global(shaded, truth)
    print("shaded 512 x 512 text page: F of the local decision %.4f, best F of a global bin threshold %.4f (b < %d)" % (local, best, at))
    assert local > best
    _, cmask, _ = B.binarize(clean)
    cm = cmask.astype(bool)
    print("clean page: %.4f %% of its ink pixels kept, %d pixels of ink added (%d of ink)" % (100.0 * (cm & truth).sum() / truth.sum(), (cm & ~truth).sum(),
                                                                                      truth.sum()))
