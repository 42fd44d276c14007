"""Grain removal, host side: the new symbols and parameter checks of the library, and the properties the
definition in tests/rank_ref.py promises: against plain loops over the rectangle, against stroke repair at percent 0 and
100, its named cases bit for bit, and what it repairs on the damaged text page.  No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import models_util as M
import morph_ref
import rank_ref as R
from test_gpu_binarize import planted

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["ocrs_rank_params_default", "ocrs_rank_params_check", "ocrs_engine_rank_page", "ocrs_engine_rank_pages"]
F = np.float32
U = np.uint32
PAGES = [(1, 1), (5, 9), (9, 5), (17, 23), (20, 20), (33, 31)]
RADII = [(1, 1), (3, 0), (0, 3), (2, 5), (7, 7), (7, 1)]   # (rx, ry)
PERCENTS = (0, 1, 35, 50, 99, 100)
TAILS = (0, 10, 20, 50)


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
    for name in ("ocrs_rank_params", "ocrs_rank_info"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert C.sizeof(_lib.RankParams) == 16 and C.sizeof(_lib.RankInfo) == 40
    assert [f[0] for f in _lib.RankInfo._fields_] == list(R.INFO_KEYS)
    assert [f[0] for f in _lib.RankParams._fields_] == ["rx", "ry", "percent", "tail"]


def test_sources_are_built():
    from ocrs_amd import build
    assert "kernels_rank.hip" in build.SOURCES and "rank.cpp" in build.SOURCES
    for name in ("kernels_rank.hip", "rank.cpp"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name


def test_default_params_and_refused_params(lib):
    import ocrs_amd
    from ocrs_amd import _lib
    p = _lib.RankParams(9, 9, 9, 9)
    assert lib.ocrs_rank_params_default(C.byref(p)) == 0
    assert (p.rx, p.ry, p.percent, p.tail) == (1, 1, 50, 20)
    assert ocrs_amd.rank_params() == R.default_params() == {"rx": 1, "ry": 1, "percent": 50, "tail": 20}
    assert lib.ocrs_rank_params_default(None) == 1 and lib.ocrs_rank_params_check(None) == 1
    accepted = 0
    for rx, ry, percent, tail in itertools.product((-1, 0, 1, 7, 8), (-1, 0, 1, 7, 8), (-1, 0, 50, 100, 101), (-1, 0, 50, 51)):
        q = _lib.RankParams(rx, ry, percent, tail)
        ok = R.valid_params(rx, ry, percent, tail)
        assert lib.ocrs_rank_params_check(C.byref(q)) == (0 if ok else 1), (rx, ry, percent, tail)
        accepted += ok
        if not ok:
            with pytest.raises(ValueError):
                R.rank(np.zeros((3, 3), F), rx, ry, percent, tail)
    assert accepted == 8 * 3 * 2
    # the Python side: ry follows rx unless given, and what is out of range is the library's to refuse
    assert ocrs_amd.rank_params(rx=2) == {"rx": 2, "ry": 2, "percent": 50, "tail": 20}
    assert ocrs_amd.rank_params(rx=1, ry=0, percent=35, tail=0) == {"rx": 1, "ry": 0, "percent": 35, "tail": 0}
    assert ocrs_amd.rank_params(ry=7) == {"rx": 1, "ry": 7, "percent": 50, "tail": 20}
    for kw in ({"rx": 0}, {"rx": 8}, {"ry": 8}, {"rx": -1, "ry": 1}, {"percent": 101}, {"percent": -1}, {"tail": 51}, {"tail": -1}):
        with pytest.raises(ocrs_amd.OcrsError) as e:
            ocrs_amd.rank_params(**kw)
        assert e.value.status_name == "INVALID_ARGUMENT", kw


# ---------------------------------------------------------------- 2. the restatement against plain loops and against stroke repair
@pytest.mark.parametrize("shape", PAGES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_plain_loops_over_the_rectangle(shape):
    page = noise(shape[0] * 100 + shape[1], *shape, ink=0.4)
    # every radius, percent and tail; percents and tails go round together so that plain loops stay affordable, and every
    # pair of them is met at some radius
    pairs = list(itertools.product(PERCENTS, TAILS))
    for i, (rx, ry) in enumerate(RADII):
        win = R.windows(page, rx, ry)
        for percent, tail in pairs[i::len(RADII)] + [(50, 20), (0, 0), (100, 50)]:
            assert same(R.rank(page, rx, ry, percent, tail, win=win), R.brute(page, rx, ry, percent, tail)), (shape, rx, ry, percent, tail)


@pytest.mark.parametrize("shape", PAGES, ids=lambda s: "%dx%d" % s)
def test_percent_0_and_100_are_thicken_and_thin(shape):
    page = noise(shape[0] * 100 + shape[1], *shape, ink=0.4)
    for rx, ry in RADII:
        win = R.windows(page, rx, ry)
        for percent, op in ((0, "thicken"), (100, "thin")):
            got, exp = R.rank(page, rx, ry, percent, 0, win=win), morph_ref.morph(page, op, rx, ry)
            assert got[0].view(U).tobytes() == exp[0].view(U).tobytes() and got[1].tobytes() == exp[1].tobytes(), (shape, rx, ry, op)
            assert {k: got[2][k] for k in morph_ref.INFO_KEYS} == exp[2] and got[2]["spared"] == 0


# ---------------------------------------------------------------- 3. properties, bit for bit
@pytest.mark.parametrize("shape", PAGES, ids=lambda s: "%dx%d" % s)
def test_properties(shape):
    page = noise(shape[0] * 100 + shape[1] + 1, *shape, ink=0.4)
    counted = int((~R.is_nan(R.words(page))).sum())
    for rx, ry in RADII:
        win = R.windows(page, rx, ry)
        a, b = R.rank(page, rx, ry, 50, 50, win=win), R.rank(page, rx, ry, 50, 0, win=win)
        assert a[0].view(U).tobytes() == b[0].view(U).tobytes() and a[1].tobytes() == b[1].tobytes(), "(50, 50) is (50, 0)"
        assert {k: a[2][k] for k in morph_ref.INFO_KEYS} == {k: b[2][k] for k in morph_ref.INFO_KEYS} and b[2]["spared"] == 0
        # at(tail) = 0 for every window when tail (n - 1) + 50 < 100 at the largest n
        tail = 49 // ((2 * rx + 1) * (2 * ry + 1) - 1)
        if tail >= 1:
            out, mask, info = R.rank(page, rx, ry, 50, tail, win=win)
            assert out.view(U).tobytes() == page.view(U).tobytes() and info["changed"] == 0 and info["spared"] == counted, (rx, ry, tail)
        for percent, tail in itertools.product((0, 50, 100), (0, 20)):
            flat = np.full(shape, F(-0.125), F)
            out, mask, info = R.rank(flat, rx, ry, percent, tail)
            assert out.tobytes() == flat.tobytes() and (mask == 1).all()
            assert info == {"counted": flat.size, "changed": 0, "ink_before": flat.size, "ink_after": flat.size, "spared": flat.size if tail else 0}
            nans = np.full(shape, np.nan, F)
            nans.view(U)[0, 0] = 0xFFC12345
            out, mask, info = R.rank(nans, rx, ry, percent, tail)
            assert out.view(U).tobytes() == nans.view(U).tobytes() and not mask.any() and info == dict.fromkeys(R.INFO_KEYS, 0)
            one = nans.copy()
            one[shape[0] // 2, shape[1] // 2] = F(-0.5)
            out, mask, info = R.rank(one, rx, ry, percent, tail)
            assert out.view(U).tobytes() == one.view(U).tobytes()
            assert info == {"counted": 1, "changed": 0, "ink_before": 1, "ink_after": 1, "spared": 1 if tail else 0}


def test_the_corner_takes_the_upper_median():
    page = np.array([[0.1, 0.2, 0.9], [0.3, 0.4, 0.9], [0.9, 0.9, 0.9]], F)
    for fn in (R.rank, R.brute):
        out = fn(page, 1, 1, 50, 0)[0]
        assert out[0, 0] == F(0.3), "n = 4: at(50) = (50 * 3 + 50) // 100 = 2, the third of 0.1 0.2 0.3 0.4"
        assert fn(page, 1, 1, 0, 0)[0][0, 0] == F(0.1) and fn(page, 1, 1, 100, 0)[0][0, 0] == F(0.4)
    assert R.at(50, 4) == 2 and R.at(50, 9) == 4 and R.at(20, 9) == 2 and R.at(80, 9) == 6 and R.at(1, 225) == 2


def test_runs_of_equal_keys_and_the_two_zeros():
    # two levels in long runs: lt < le by the length of the run.  A dark line one pixel wide (3 of the 9 keys of a window) is
    # spared at tail 20 (lt = 0, le - 1 = 2 = at(20)) and erased at tail 0; a single dark pixel is erased by both
    page = np.full((9, 12), F(0.5), F)
    page[4, :] = F(-0.5)
    page[1, 7] = F(-0.5)
    for fn in (R.rank, R.brute):
        plain, kept = fn(page, 1, 1, 50, 0), fn(page, 1, 1, 50, 20)
        assert (plain[0] == F(0.5)).all() and plain[2]["changed"] == 13
        assert (kept[0][4, :] == F(-0.5)).all() and kept[0][1, 7] == F(0.5) and kept[2]["changed"] == 1
        assert kept[2]["spared"] == page.size - 1
    # -0.0 and +0.0 are two keys, -0.0 the lesser: a window of five +0.0 and four -0.0 has +0.0 for its median
    zeros = np.zeros((3, 3), F)
    zeros.view(U)[[0, 0, 2, 2], [0, 2, 0, 2]] = 0x80000000
    for fn in (R.rank, R.brute):
        out, mask, info = fn(zeros, 1, 1, 50, 0)
        assert out.view(U)[1, 1] == 0 and fn(zeros, 1, 1, 0, 0)[0].view(U)[1, 1] == 0x80000000
        assert not mask[1, 1] & 1 and info["ink_after"] == 0, "neither zero is ink"
        assert fn(zeros, 1, 1, 100, 0)[0].view(U)[0, 0] == 0 and fn(zeros, 1, 1, 100, 0)[2]["changed"] == 4


# ---------------------------------------------------------------- 4. what it is for
@pytest.fixture(scope="module")
def text_page():
    """The 512 x 512 text page of DESIGN.md §7.13 prepared by the oracle."""
    from ocrs_amd import synth
    from oracle import pipeline as OP
    from oracle.nn import OracleGraph, OracleModel
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                       recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))
    px = synth.synthetic_page(3, 512, 512, 20, 1, 1)
    return np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), F)[0])


def sauvola_f(page, truth):
    return R.f_measure(R.binarize(page)[1] & 1 == 1, truth)


def test_the_median_removes_grain_salt_and_pepper_and_a_halftone_screen(text_page):
    clean = text_page
    truth = clean < F(0)
    print("clean page: %d components, Sauvola F %.3f" % (R.components(truth), sauvola_f(clean, truth)))
    for name, damaged in (("Gaussian grain, sigma 0.25", R.grain(clean, 0.25, 11)), ("10 % salt and pepper", R.salt_and_pepper(clean, 0.10, 12)),
                          ("halftone screen of pitch 4", R.halftone(clean, 4))):
        median = R.rank(damaged, 1, 1, 50, 0)[0]
        opened, closed = R.morph(damaged, "open", 1, 1)[0], R.morph(damaged, "close", 1, 1)[0]
        f = {k: sauvola_f(v, truth) for k, v in (("none", damaged), ("median", median), ("open", opened), ("close", closed))}
        n = {k: R.components(v < F(0)) for k, v in (("none", damaged), ("median", median), ("open", opened))}
        g = {k: R.best_global(v, truth)[0] for k, v in (("none", damaged), ("median", median))}
        print("%s: components at cut 0: none %d, median %d, open %d; Sauvola F: none %.3f, median %.3f, open %.3f, close %.3f; "
              "best global F: none %.3f, median %.3f" % (name, n["none"], n["median"], n["open"], f["none"], f["median"], f["open"], f["close"],
                                                         g["none"], g["median"]))
        assert f["median"] > f["none"] and f["median"] > f["open"] and f["median"] > f["close"], name
        assert n["median"] < n["none"], name


def test_sparing_keeps_the_hairlines_that_the_plain_median_erases(text_page):
    page, lines = R.hairlines(text_page)
    truth = page < F(0)
    assert lines.sum() > 4000

    def kept(v):
        return float(((v < F(0)) & truth).sum()) / float(truth.sum())

    plain_clean = R.rank(page, 1, 1, 50, 0)[0]
    print("hairlines: %d pixels; clean page: plain median keeps %.1f %% of the ink, best global F %.3f"
          % (lines.sum(), 100 * kept(plain_clean), R.best_global(plain_clean, truth)[0]))
    noisy = R.salt_and_pepper(page, 0.06, 13)
    plain, spared = R.rank(noisy, 1, 1, 50, 0)[0], R.rank(noisy, 1, 1, 50, 20)[0]
    res = {k: (kept(v), R.best_global(v, truth)[0], R.components(v < F(0))) for k, v in (("none", noisy), ("tail 0", plain), ("tail 20", spared))}
    for k, (share, f, n) in res.items():
        print("6 %% salt and pepper, %s: %.1f %% of the ink kept, best global F %.3f, %d components at cut 0" % (k, 100 * share, f, n))
    assert res["tail 20"][0] > res["tail 0"][0] and res["tail 20"][0] > res["none"][0], "more true ink kept than by the plain median or by no filter"
    assert res["tail 20"][1] > res["tail 0"][1] and res["tail 20"][1] > res["none"][1], "and a higher best global F than either"
    assert kept(plain_clean) < 1.0
