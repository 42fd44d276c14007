"""Page measurement, host side: the two implementations of tests/measure_ref.py against each other and
against hand-stated answers; the rule of choose; the library's ocrs_measure_choose and ocrs_work_scale_for_text, its
parameter checks and its new symbols against the restatement; the scale-recovery experiment; the chooser's header clean under
-fsanitize=address,undefined in a stand-alone program.  No GPU."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import despeckle_pages as P
import measure_ref as MR
import models_util as M
import resample_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["ocrs_measure_params_default", "ocrs_measure_params_check", "ocrs_engine_measure_page", "ocrs_engine_measure_pages",
               "ocrs_measure_choice_params_default", "ocrs_measure_choice_params_check", "ocrs_measure_choose", "ocrs_work_scale_for_text"]
F = np.float32
SHAPES = [(1, 1), (1, 70), (70, 1), (65, 129), (130, 67)]


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
    for name in ("ocrs_measure_params", "ocrs_measure_info", "ocrs_measure_choice_params", "ocrs_text_scale"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert re.search(r"#define\s+OCRS_WORK_TEXT_HEIGHT_DEFAULT\s+%d\b" % MR.WORK_TEXT_HEIGHT_DEFAULT, hdr)
    assert _lib.WORK_TEXT_HEIGHT_DEFAULT == MR.WORK_TEXT_HEIGHT_DEFAULT and re.search(r"#define\s+OCRS_MEASURE_BINS\s+256\b", hdr)
    assert C.sizeof(_lib.MeasureParams) == 8 and C.sizeof(_lib.MeasureInfo) == 16 + 4 * 1024 + 8 * 256
    assert C.sizeof(_lib.MeasureChoiceParams) == 8 and C.sizeof(_lib.TextScaleC) == 16
    assert [f[0] for f in _lib.MeasureInfo._fields_] == list(MR.INFO_KEYS)
    assert [f[0] for f in _lib.TextScaleC._fields_] == list(MR.CHOICE_KEYS)


# ------------------------------------------------------------------ the two implementations of the restatement
def random_page(seed, h, w, density):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < density, F(-0.3), F(0.3)).astype(F)


def assert_agree(page, what, **kw):
    a, b = MR.measure(page, **kw), MR.measure_slow(page, **kw)
    for k in MR.INFO_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k, np.asarray(a[k]).tolist(), np.asarray(b[k]).tolist())
    assert MR.same(a, b) and a["run_h"].dtype == np.uint32 and a["area_by_h"].dtype == np.uint64 and a["run_h"][0] == a["comp_h"][0] == 0
    assert int((a["run_h"].astype(np.int64) * np.arange(256))[:255].sum()) <= a["ink"] and a["counted"] == a["comp_h"].sum() == a["comp_w"].sum()
    return a


@pytest.mark.parametrize("density", (0.05, 0.5, 0.95))
def test_the_two_implementations_agree_on_random_pages(density):
    for i, (h, w) in enumerate(SHAPES):
        for min_area in (0, 1, 4):
            assert_agree(random_page(int(density * 100) + i, h, w, density), (h, w, density, min_area), min_area=min_area)


def test_the_two_implementations_agree_on_the_despeckle_patterns():
    h, w = 70, 90
    a, b = P.corner_pairs(h, w)
    pages = {"blobs 1": P.planted_blobs(h, w, 1), "blobs 4": P.planted_blobs(h, w, 4), "blobs 9": P.planted_blobs(h, w, 9),
             "checkerboard": P.checkerboard(h, w), "diagonals": P.diagonals(h, w), "anti-diagonals": P.diagonals(h, w, 3, True),
             "serpentine": P.serpentine(h, w), "spiral": P.spiral(h, w), "u": P.u_shape(h, w), "corner pairs": a, "corner pairs of paper": b}
    got = {name: assert_agree(page, name, min_area=2) for name, page in pages.items()}
    assert got["checkerboard"]["components"] == 1 and got["serpentine"]["components"] == 1 and got["spiral"]["components"] == 1
    assert got["u"]["components"] == 2 and got["u"]["comp_h"][h] == 1 and got["u"]["comp_h"][h - 2] == 1
    assert got["corner pairs"]["components"] == 2 and got["corner pairs"]["comp_h"][2] == 2 and got["corner pairs"]["comp_w"][2] == 2
    assert got["blobs 1"]["counted"] == 0 and got["blobs 1"]["components"] == len(P.blob_sites(h, w, 1))


def hist(**bins):
    """{"3": 2} -> a uint32 [256] with 2 at index 3."""
    out = np.zeros(256, np.uint32)
    for k, v in bins.items():
        out[int(k)] = v
    return out


def test_hand_stated_answers():
    empty = MR.measure(P.paper(9, 11))
    assert empty["ink"] == empty["components"] == empty["counted"] == 0 and not any(np.asarray(empty[k]).any() for k in MR.INFO_KEYS[3:])
    for h, w in ((5, 7), (3, 300), (300, 3)):
        full = assert_agree(np.full((h, w), F(-0.4), F), "full")
        assert full["ink"] == h * w and full["components"] == full["counted"] == 1
        assert np.array_equal(full["run_h"], hist(**{str(min(w, 255)): h})) and np.array_equal(full["run_v"], hist(**{str(min(h, 255)): w}))
        assert np.array_equal(full["comp_h"], hist(**{str(min(h, 255)): 1})) and np.array_equal(full["comp_w"], hist(**{str(min(w, 255)): 1}))
        assert full["area_by_h"][min(h, 255)] == h * w and full["area_by_h"].sum() == h * w
    for n, at in ((254, 254), (255, 255), (256, 255)):
        page = P.paper(3, 300)
        page[1, 7:7 + n] = P.INK
        got = assert_agree(page, n)
        assert got["run_h"][at] == 1 and got["run_h"].sum() == 1 and got["run_v"][1] == n and got["comp_w"][at] == 1 and got["comp_h"][1] == 1
        got = assert_agree(np.ascontiguousarray(page.T), n)
        assert got["run_v"][at] == 1 and got["run_v"].sum() == 1 and got["run_h"][1] == n and got["comp_h"][at] == 1 and got["area_by_h"][at] == n
    # NaN, -0.0 and v == threshold are not ink; the next float below the threshold is
    page = np.array([[np.nan, -0.0, 0.0, 0.25, np.nextafter(F(0.25), F(-1)), -np.inf, 1.0]], F)
    page.view(np.uint32)[0, 0] = 0xFFC00000   # a NaN with its sign set
    assert assert_agree(page, "edges", min_area=0)["ink"] == 1 and assert_agree(page, "edges", threshold=0.25, min_area=0)["ink"] == 4
    assert MR.measure(page, threshold=0.25, min_area=0)["run_h"].tolist() == hist(**{"2": 2}).tolist()   # . X X . X X .
    # min_area at area - 1, area, area + 1
    page = P.paper(20, 20)
    P.plant(page, 5, 5, 7)
    for min_area, counted in ((6, 1), (7, 1), (8, 0)):
        got = assert_agree(page, min_area, min_area=min_area)
        assert got["components"] == 1 and got["counted"] == counted and got["comp_h"][3] == counted and got["area_by_h"][3] == 7 * counted
    # two pixels touching by a corner: one component with a 2 x 2 box
    page = P.paper(6, 6)
    page[2, 2] = page[3, 3] = P.INK
    got = assert_agree(page, "corner", min_area=2)
    assert got["components"] == 1 and got["comp_h"][2] == 1 and got["comp_w"][2] == 1 and got["area_by_h"][2] == 2 and got["run_h"][1] == 2
    for bad in ({"threshold": float("nan")}, {"threshold": float("inf")}, {"min_area": -1}, {"min_area": 65536}, {"min_area": 1.5}):
        assert not MR.valid_params(**bad)
        with pytest.raises(ValueError):
            MR.measure(page, **bad)


# ------------------------------------------------------------------ the choice
def info_of(run_h=None, run_v=None, comp_h=None, area_by_h=None, comp_w=None):
    z = np.zeros(256, np.uint32)
    comp_h = z if comp_h is None else comp_h
    area = np.asarray(comp_h, np.uint64) * np.arange(256, dtype=np.uint64) if area_by_h is None else np.asarray(area_by_h, np.uint64)
    return {"ink": 0, "components": int(np.asarray(comp_h).sum()), "counted": int(np.asarray(comp_h).sum()), "run_h": z if run_h is None else run_h,
            "run_v": z if run_v is None else run_v, "comp_h": comp_h, "comp_w": comp_h if comp_w is None else comp_w, "area_by_h": area}


def planted_page(square=False, solid=False):
    """Six bars 5 wide and 21 tall; six boxes 21 tall drawn with strokes of 5, 30 to 40 wide (square: 21 wide; solid:
    filled); six one-pixel specks."""
    page = P.paper(120, 300)
    x = 10
    for i in range(6):
        page[10:31, 10 + 30 * i:15 + 30 * i] = P.INK
        w = 21 if square else 30 + 2 * i
        page[60:81, x:x + w] = P.INK
        if not solid:
            page[65:76, x + 5:x + w - 5] = P.PAPER
        x += w + 8
        page[100, 10 + 30 * i] = P.INK
    return page


def planted_choices():
    """(name, info, min_height_strokes, expected or None) of the hand-made cases."""
    cases = [("no ink", info_of(), 0.5, {"stroke": 0, "text_height": 0, "support": 0, "blank": 1})]
    cases.append(("a tie goes to the smaller L", info_of(run_h=hist(**{"3": 4, "4": 3, "6": 2, "12": 1})), 0.5, {"stroke": 3, "text_height": 0, "support": 0, "blank": 1}))
    cases.append(("both directions add up", info_of(run_h=hist(**{"3": 4, "5": 2}), run_v=hist(**{"5": 1})), 0.5, None))   # 12 < 15
    cases.append(("bin 255 holds no stroke", info_of(run_h=hist(**{"255": 1000, "254": 1})), 0.5, None))
    cases.append(("only runs of 255 and more", info_of(run_h=hist(**{"255": 9}), comp_h=hist(**{"255": 1, "7": 2})), 0.5, None))
    cases.append(("only pictures", info_of(run_h=hist(**{"2": 9}), comp_h=hist(**{"255": 3})), 0.5, {"stroke": 2, "text_height": 0, "support": 0, "blank": 1}))
    # strokes of 4: a height qualifies at 256 H >= q * 4
    ch = hist(**{"1": 50, "2": 40, "3": 5, "5": 3, "6": 2, "20": 10, "30": 4})
    for m, name in ((0.5, "at 2 exactly"), (0.5 + 1 / 256, "one step over 2"), (0.75, "at 3"), (1.5, "at 6"), (1.5 + 1 / 512, "rounds up past 6"), (0.0, "all"),
                    (255.0, "none: only specks")):
        cases.append(("min_height_strokes %s" % name, info_of(run_h=hist(**{"4": 100}), comp_h=ch), m, None))
    # the median is by ink: many dots, few letters
    cases.append(("dots outnumber letters", info_of(run_h=hist(**{"3": 50}), comp_h=hist(**{"3": 100, "20": 30}), area_by_h=hist(**{"3": 900, "20": 6000})), 0.5, None))
    cases.append(("the lower median on an even split", info_of(run_h=hist(**{"2": 5}), comp_h=hist(**{"10": 1, "12": 1}), area_by_h=hist(**{"10": 40, "12": 40})), 0.5, None))
    cases.append(("one over the split", info_of(run_h=hist(**{"2": 5}), comp_h=hist(**{"10": 1, "12": 1}), area_by_h=hist(**{"10": 40, "12": 41})), 0.5, None))
    cases.append(("components without ink", info_of(run_h=hist(**{"2": 5}), comp_h=hist(**{"10": 3}), area_by_h=hist()), 0.5, None))
    big = np.zeros(256, np.uint64)
    big[1:255] = np.uint64(2 ** 64 - 1)
    cases.append(("sums beyond 64 bits", info_of(run_h=np.full(256, 2 ** 32 - 1, np.uint32), run_v=np.full(256, 2 ** 32 - 1, np.uint32),
                                                comp_h=np.full(256, 2 ** 32 - 1, np.uint32), area_by_h=big), 0.0, None))
    # bars of one width and boxes of one height, measured: strokes of 5, text 21 tall
    cases.append(("a planted page", MR.measure(planted_page()), 0.5, {"stroke": 5, "text_height": 21, "support": 12, "blank": 0}))
    cases.append(("the planted page's specks alone", MR.measure(np.where(np.arange(120)[:, None] < 90, P.PAPER, planted_page()).astype(F), min_area=2), 0.5,
                  {"stroke": 1, "text_height": 0, "support": 0, "blank": 1}))
    # What the rule cannot do: where every long run of a page has one length, that length holds as much ink
    # as the stroke does and wins.  Square outlines and solid blocks give their height as the stroke; the height stays right.
    cases.append(("square outlines: a known limit", MR.measure(planted_page(square=True)), 0.5, {"stroke": 21, "text_height": 21, "support": 12, "blank": 0}))
    cases.append(("solid blocks: a known limit", MR.measure(planted_page(solid=True)), 0.5, {"stroke": 21, "text_height": 21, "support": 12, "blank": 0}))
    return cases


def lib_choose(lib, info, m=None):
    from ocrs_amd import _lib
    rec = _lib.MeasureInfo.from_dict(info)
    out = _lib.TextScaleC()
    p = None
    if m is not None:
        p = C.byref(_lib.MeasureChoiceParams(float(m)))
    st = lib.ocrs_measure_choose(C.byref(rec), p, C.byref(out))
    assert st == 0, st
    return {k: int(getattr(out, k)) for k in MR.CHOICE_KEYS}


def test_the_choice_on_planted_cases(lib):
    seen = {}
    for name, info, m, exp in planted_choices():
        ref = MR.choose(info, m)
        if exp is not None:
            assert ref == exp, (name, ref)
        support = ref["support"]
        ref["support"] = min(support, 2 ** 32 - 1)   # ocrs_text_scale.support saturates
        got = lib_choose(lib, info, m)
        assert got == ref and tuple(got) == MR.CHOICE_KEYS, (name, got, ref)
        seen[name] = (ref["stroke"], ref["text_height"], support)
    assert seen["both directions add up"][0] == 5 and seen["bin 255 holds no stroke"][0] == 254 and seen["only runs of 255 and more"] == (0, 7, 2)
    assert seen["min_height_strokes at 2 exactly"][2] == 64 and seen["min_height_strokes one step over 2"][2] == 24
    assert seen["min_height_strokes at 3"][2] == 24 and seen["min_height_strokes at 6"][2] == 16 and seen["min_height_strokes rounds up past 6"][2] == 14
    assert seen["min_height_strokes all"][2] == 114 and seen["min_height_strokes none: only specks"] == (4, 0, 0)
    assert seen["min_height_strokes at 2 exactly"][1] == 20, "by ink the ten tall components outweigh ninety specks"
    assert seen["dots outnumber letters"][1:] == (20, 130) and seen["the lower median on an even split"][1] == 10 and seen["one over the split"][1] == 12
    assert seen["components without ink"] == (2, 0, 3) and seen["sums beyond 64 bits"] == (254, 127, 254 * (2 ** 32 - 1))


def random_infos(n, seed):
    rng = np.random.default_rng(seed)
    for i in range(n):
        kind = i % 4
        top = (5, 1000, 2 ** 31, 2 ** 32)[kind]
        lo, hi = sorted(int(v) for v in rng.integers(1, 256, 2))
        dens = float(rng.choice([0.05, 0.5, 1.0]))

        def h32():
            v = (rng.random(256) < dens) * rng.integers(0, top, 256)
            v[:lo] = 0
            v[hi + 1:] = 0
            return v.astype(np.uint32)

        comp_h = h32()
        area = (comp_h.astype(np.uint64) * rng.integers(1, 5000, 256).astype(np.uint64)) if kind < 3 else rng.integers(0, 2 ** 63, 256).astype(np.uint64) * np.uint64(2)
        info = {"ink": int(rng.integers(0, 2 ** 40)), "components": int(rng.integers(0, 2 ** 32)), "counted": int(rng.integers(0, 2 ** 32)),
                "run_h": h32(), "run_v": h32(), "comp_h": comp_h, "comp_w": h32(), "area_by_h": area}
        yield info, float(rng.choice([0.0, 0.5, 0.75, 1.5, 3.0, 254.99, rng.random() * 4]))


def test_the_choice_on_random_histograms(lib):
    blanks = 0
    for info, m in random_infos(100, 3):
        ref = MR.choose(info, m)
        ref["support"] = min(ref["support"], 2 ** 32 - 1)
        assert lib_choose(lib, info, m) == ref, (m, {k: np.asarray(v).tolist() for k, v in info.items()})
        blanks += ref["blank"]
    assert 5 < blanks < 95
    from ocrs_amd import TextScale, measure_choose
    info = MR.measure(planted_page())
    assert measure_choose(info) == TextScale(5, 21, 12, False) and measure_choose(info, 255.0) == TextScale(5, 0, 0, True)
    with pytest.raises(ValueError):
        measure_choose(dict(info, run_h=np.zeros(255, np.uint32)))


def test_the_work_scale(lib):
    from ocrs_amd import _lib, work_scale_for_text, work_size

    def lib_scale(*args):
        out = C.c_double(-1.0)
        st = lib.ocrs_work_scale_for_text(C.c_int(args[0]), *[C.c_double(v) for v in args[1:]], C.byref(out))
        return st, out.value

    rng = np.random.default_rng(9)
    cases = [(14, 14.0, 0.125, 4.0), (28, 14.0, 0.125, 4.0), (7, 14.0, 0.125, 4.0), (3, 14.0, 0.125, 4.0), (1, 14.0, 0.125, 4.0), (254, 14.0, 0.125, 4.0),
             (113, 14.0, 0.125, 4.0), (0, 14.0, 0.125, 4.0), (-5, 14.0, 0.125, 4.0), (0, 14.0, 2.0, 3.0), (10, 33.0, 1.0, 1.0), (3, 1e-3, 1e-9, 1e9)]
    cases += [(int(rng.integers(1, 255)), float(rng.random() * 60 + 0.5), 0.125, 4.0) for _ in range(50)]
    for c in cases:
        st, got = lib_scale(*c)
        assert st == 0 and got == MR.work_scale_for_text(*c), c
    assert lib_scale(14, 14.0, 0.125, 4.0)[1] == 1.0 and lib_scale(28, 14.0, 0.125, 4.0)[1] == 0.5 and lib_scale(3, 14.0, 0.125, 4.0)[1] == 4.0
    assert lib_scale(254, 14.0, 0.125, 4.0)[1] == 0.125 and lib_scale(0, 14.0, 0.125, 4.0)[1] == 1.0 and lib_scale(0, 14.0, 2.0, 3.0)[1] == 1.0, "a blank page keeps its size"
    nan, inf = float("nan"), float("inf")
    for bad in ((14, 0.0, 0.125, 4.0), (14, -1.0, 0.125, 4.0), (14, nan, 0.125, 4.0), (14, inf, 0.125, 4.0), (14, 14.0, 0.0, 4.0), (14, 14.0, -1.0, 4.0),
                (14, 14.0, 4.0, 0.125), (14, 14.0, nan, 4.0), (14, 14.0, 0.125, nan), (14, 14.0, 0.125, inf), (0, 14.0, 4.0, 0.125)):
        assert lib_scale(*bad) == (1, -1.0), bad
        with pytest.raises(ValueError):
            MR.work_scale_for_text(*bad)
    assert lib.ocrs_work_scale_for_text(C.c_int(14), C.c_double(14.0), C.c_double(0.125), C.c_double(4.0), None) == 1
    assert work_scale_for_text(28) == 0.5 and work_scale_for_text(28, 21) == 0.75 and work_scale_for_text(0) == 1.0
    assert work_size((1000, 800), scale=work_scale_for_text(28, 21)) == (750, 600)
    with pytest.raises(_lib.OcrsError):
        work_scale_for_text(14, -2)


def test_parameter_checks(lib):
    from ocrs_amd import _lib, measure_params
    nan, inf = float("nan"), float("inf")
    p = _lib.MeasureParams()
    assert lib.ocrs_measure_params_default(C.byref(p)) == 0 and (p.threshold, p.min_area) == (0.0, 4) == tuple(MR.default_params().values())
    assert lib.ocrs_measure_params_default(None) == 1 and lib.ocrs_measure_params_check(None) == 1
    for vals, status in (((0.0, 0), 0), ((-0.25, 65535), 0), ((1e30, 4), 0), ((nan, 4), 1), ((inf, 4), 1), ((-inf, 4), 1), ((0.0, -1), 1), ((0.0, 65536), 1)):
        assert lib.ocrs_measure_params_check(C.byref(_lib.MeasureParams(*vals))) == status, vals
        assert MR.valid_params(*vals) == (status == 0), vals
    assert measure_params() == {"threshold": 0.0, "min_area": 4} and measure_params(threshold=0.25, min_area=0) == {"threshold": 0.25, "min_area": 0}
    with pytest.raises(_lib.OcrsError):
        measure_params(min_area=65536)
    q = _lib.MeasureChoiceParams()
    assert lib.ocrs_measure_choice_params_default(C.byref(q)) == 0 and q.min_height_strokes == MR.MIN_HEIGHT_STROKES == 0.5
    assert lib.ocrs_measure_choice_params_default(None) == 1 and lib.ocrs_measure_choice_params_check(None) == 1
    rec, out = _lib.MeasureInfo(), _lib.TextScaleC()
    for m, status in ((0.0, 0), (0.5, 0), (255.0, 0), (-0.001, 1), (255.001, 1), (nan, 1), (inf, 1), (-inf, 1)):
        assert lib.ocrs_measure_choice_params_check(C.byref(_lib.MeasureChoiceParams(m))) == status, m
        assert (MR.height_q8(m) is not None) == (status == 0), m
        assert lib.ocrs_measure_choose(C.byref(rec), C.byref(_lib.MeasureChoiceParams(m)), C.byref(out)) == status, m
    assert lib.ocrs_measure_choose(None, None, C.byref(out)) == 1 and lib.ocrs_measure_choose(C.byref(rec), None, None) == 1
    assert lib.ocrs_measure_choose(C.byref(rec), None, C.byref(out)) == 0 and (out.stroke, out.text_height, out.support, out.blank) == (0, 0, 0, 1)


# ------------------------------------------------------------------ the experiments of DESIGN.md §7.14
@pytest.fixture(scope="module")
def prepared():
    """picture -> the page the oracle's prepare_input makes of it, as the text_page fixtures of the other page operations do."""
    from oracle import pipeline as OP
    from oracle.nn import OracleGraph, OracleModel
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                       recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))
    return lambda px: np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), F)[0])


@pytest.fixture(scope="module")
def text_page(prepared):
    """The 512 x 512 text page of DESIGN.md §7.13 / §7.14."""
    from ocrs_amd import synth
    return prepared(synth.synthetic_page(3, 512, 512, 20, 1, 1))


def test_the_scale_of_a_resampled_page_is_recovered(text_page):
    """The page resampled by 0.5, 2 and 3 (tests/resample_ref.py).  Measured with the restatement first:
    stroke 6 / 13 / 26 / 39 and text_height 6 / 14 / 28 / 42 at 0.5 / 1 / 2 / 3, that is measured / (scale x native) of
    0.92 / 1 / 1 / 1 and 0.86 / 1 / 1 / 1: off by 0.5 and 1 pixel at 0.5, by nothing at 2 and 3.  The band asserted is one
    histogram bin wider than that: 2 pixels at 0.5, 1 pixel at 2 and 3."""
    got = {}
    for scale in (0.5, 1, 2, 3):
        page = text_page if scale == 1 else RR.resize(text_page, RR.work_size(text_page.shape, scale))
        got[scale] = MR.choose(MR.measure(page))
        print("scale %g: %r" % (scale, got[scale]))
        assert not got[scale]["blank"] and got[scale]["support"] > 100
    for key in ("stroke", "text_height"):
        vals = [got[s][key] for s in (0.5, 1, 2, 3)]
        assert vals == sorted(vals), (key, vals)
    assert got[2]["text_height"] > got[1]["text_height"] and got[3]["text_height"] > got[1]["text_height"]
    for scale, band in ((0.5, 2.0), (2, 1.0), (3, 1.0)):
        for key in ("stroke", "text_height"):
            assert abs(got[scale][key] - scale * got[1][key]) <= band, (scale, key, got[scale][key], got[1][key])


def test_the_default_target_is_the_text_height_of_the_benchmark_pages(prepared):
    """OCRS_WORK_TEXT_HEIGHT_DEFAULT is the median over the benchmark's sixteen seeds (DESIGN.md §7.14 lists them all); three
    of them, the two that are not 14 among them, are measured again here."""
    from ocrs_amd import synth
    heights = [MR.choose(MR.measure(prepared(synth.synthetic_page(seed, 1024, 1024, lines=80))))["text_height"] for seed in (0, 1, 10)]
    assert heights == [14, 13, 13] and MR.WORK_TEXT_HEIGHT_DEFAULT == 14


# ------------------------------------------------------------------ the chooser under the sanitizers
def test_the_chooser_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/measure_harness.cpp, a stand-alone program over measure_choose.hpp, on this file's cases."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "measure_harness")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(HERE, "sanitize", "measure_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, "building the sanitizer harness failed:\n" + r.stderr[-3000:]
    scales = [(14.0, 0.125, 4.0), (21.0, 0.5, 2.0), (0.0, 0.125, 4.0), (14.0, 4.0, 0.125)]
    cases = [(info, m) + scales[i % 4] for i, (_, info, m, _) in enumerate(planted_choices())]
    cases += [(info, m) + scales[i % 4] for i, (info, m) in enumerate(random_infos(100, 4))]
    cases += [(cases[0][0], bad, 14.0, 0.125, 4.0) for bad in (-1.0, 256.0, float("nan"))]
    from ocrs_amd import _lib
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for info, m, target, lo, hi in cases:
            f.write(np.array([m, target, lo, hi], np.float64).tobytes())
            f.write(bytes(_lib.MeasureInfo.from_dict(info)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases) + 1 and lines[-1].startswith("extremes ")
    for line, (info, m, target, lo, hi) in zip(lines, cases):
        if MR.height_q8(m) is None:
            assert line == "refused", (line, m)
            continue
        ref = MR.choose(info, m)
        words = line.split()
        assert [int(v) for v in words[:4]] == [ref["stroke"], ref["text_height"], min(ref["support"], 2 ** 32 - 1), ref["blank"]], (line, ref)
        if math.isfinite(target) and target > 0 and 0 < lo <= hi:
            assert float.fromhex(words[4]) == MR.work_scale_for_text(ref["text_height"], target, lo, hi), (line, ref)
        else:
            assert words[4] == "refused", line
