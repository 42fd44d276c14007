"""Ruled-line removal, host side: the new symbols and parameter checks of the library, and the properties
the definition in tests/rules_ref.py promises, on hand-made pages and on the table page through the oracle's detector.
No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import models_util as M
import rules_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["ocrs_rules_params_default", "ocrs_rules_params_check", "ocrs_engine_remove_rules_page", "ocrs_engine_remove_rules_pages"]
F = np.float32


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
    for name in ("ocrs_rules_params", "ocrs_rules_info"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert C.sizeof(_lib.RulesParams) == 20 and C.sizeof(_lib.RulesInfo) == 56
    assert [f[0] for f in _lib.RulesInfo._fields_] == list(R.INFO_KEYS)


def test_sources_are_built():
    from ocrs_amd import build
    assert "kernels_rules.hip" in build.SOURCES and "rules.cpp" in build.SOURCES
    for name in ("kernels_rules.hip", "rules.cpp"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name


def test_default_params_and_refused_params(lib):
    import ocrs_amd
    from ocrs_amd import _lib
    p = _lib.RulesParams(1.0, 1, 1, 7, 1.0)
    assert lib.ocrs_rules_params_default(C.byref(p)) == 0
    assert (p.threshold, p.min_length, p.max_thickness, p.margin) == (0.0, 96, 8, 1) and p.paper != p.paper
    assert ocrs_amd.rules_params() == R.default_params() == {"threshold": 0.0, "min_length": 96, "max_thickness": 8, "margin": 1, "paper": None}
    assert lib.ocrs_rules_params_default(None) == 1 and lib.ocrs_rules_params_check(None) == 1
    for kw in ({"min_length": 2}, {"min_length": 65535}, {"max_thickness": 1}, {"max_thickness": 64}, {"margin": 0}, {"margin": 8},
               {"threshold": -0.25}, {"threshold": 2.0 ** 100}, {"paper": 0.5}, {"paper": -0.0}, {"paper": float("nan")},
               {"min_length": 5, "max_thickness": 3, "margin": 2, "threshold": 0.125, "paper": 0.25}):
        assert R.valid_params(**kw), kw
        exp = dict(R.default_params(), **kw)
        if exp["paper"] is not None and exp["paper"] != exp["paper"]:
            exp["paper"] = None   # NaN: measured
        assert ocrs_amd.rules_params(**kw) == exp, kw
    for kw in ({"min_length": 1}, {"min_length": 0}, {"min_length": -96}, {"min_length": 65536}, {"min_length": 1 << 30}, {"max_thickness": 0},
               {"max_thickness": -1}, {"max_thickness": 65}, {"margin": -1}, {"margin": 9}, {"threshold": float("nan")},
               {"threshold": float("inf")}, {"threshold": float("-inf")}, {"paper": float("inf")}, {"paper": float("-inf")}):
        assert not R.valid_params(**kw), kw
        with pytest.raises(ocrs_amd.OcrsError) as e:
            ocrs_amd.rules_params(**kw)
        assert e.value.status_name == "INVALID_ARGUMENT", kw
        with pytest.raises(ValueError):
            R.remove_rules(np.zeros((4, 4), F), **kw)


# ---------------------------------------------------------------- the restatement on hand-made pages
def paper(h, w):
    return np.full((h, w), 0.4, F)


FILL = F(231.0 / 256.0 - 0.5)   # the level of that paper's bin: what a removed pixel becomes


@pytest.mark.parametrize("L", [64, 65])
@pytest.mark.parametrize("x0", [0, 1, 63, 64])
def test_runs_around_the_minimum_length(L, x0):
    for n in (L - 1, L, L + 1):
        page = paper(5, 200)
        page[2, x0:x0 + n] = -0.4
        out, mask, info = R.remove_rules(page, min_length=L, margin=0)
        assert info["h_removed"] == (n if n >= L else 0) and info["v_removed"] == 0, (L, x0, n)
        assert np.array_equal(mask == 1, (page < 0) if n >= L else np.zeros_like(mask, bool))
        out, mask, info = R.remove_rules(np.ascontiguousarray(page.T), min_length=L, margin=0)
        assert info["v_removed"] == (n if n >= L else 0) and info["h_removed"] == 0, (L, x0, n)
        assert np.array_equal(mask == 2, (page.T < 0) if n >= L else np.zeros_like(mask, bool))


@pytest.mark.parametrize("T", [1, 3, 8, 64])
def test_blocks_around_the_maximum_thickness(T):
    for thick in (T, T + 1):
        page = paper(T + 12, 150)
        page[5:5 + thick, 10:130] = -0.4
        out, mask, info = R.remove_rules(page, min_length=100, max_thickness=T, margin=0)
        if thick <= T:
            assert info["h_removed"] == thick * 120 and np.all(out[5:5 + thick, 10:130] == FILL) and info["overwritten"] == thick * 120
        else:
            assert info["overwritten"] == 0 and out.tobytes() == page.tobytes(), "a solid dark block is not a rule"
        out, mask, info = R.remove_rules(np.ascontiguousarray(page.T), min_length=100, max_thickness=T, margin=0)
        assert info["v_removed"] == (thick * 120 if thick <= T else 0) and info["h_removed"] == 0


def underlined():
    """The 40 x 200 page: an underline two pixels thick, a stroke that crosses it, one that ends on it, one that stops short."""
    page = paper(40, 200)
    page[20:22, 10:190] = -0.4        # the underline
    page[10:30, 50:53] = -0.4         # crosses it
    page[10:20, 100:103] = -0.4       # ends on it
    page[10:19, 150:153] = -0.4       # stops a pixel above it
    return page


def test_a_crossing_stroke_is_kept_and_an_ending_stroke_is_not():
    page = underlined()
    out, mask, info = R.remove_rules(page, margin=0)
    assert np.all(mask[20:22, 50:53] == 8) and info["kept"] == 6, "the stroke that crosses keeps the rule's pixels under it"
    assert np.all(out[10:30, 50:53] == F(-0.4)), "the crossing stroke is whole"
    assert np.all(mask[20:22, 100:103] == 1) and np.all(out[20:22, 100:103] == FILL), "under the stroke that ends on it the rule goes"
    assert np.all(out[10:20, 100:103] == F(-0.4)) and np.all(out[10:19, 150:153] == F(-0.4)), "the strokes stay"
    assert info["h_removed"] == 2 * 180 - 6 and info["v_removed"] == 0 and info["overwritten"] == info["h_removed"]
    ink_left = (out < 0)
    ink_left[10:30, 50:53] = ink_left[10:20, 100:103] = ink_left[10:19, 150:153] = False
    assert not ink_left.any(), "nothing of the underline is left elsewhere"
    # with the margin, the paper above and below the removed rule is overwritten too (with its own level here)
    out1, mask1, info1 = R.remove_rules(page, margin=1)
    assert info1["overwritten"] == info["overwritten"] + int(((mask1 & 4) != 0).sum()) and ((mask1 & 4) != 0).sum() == 2 * 180 - 6 - 3
    assert not ((mask1 & 4) != 0)[page < 0].any(), "a margin never takes ink"


def test_a_grid_intersection_is_removed():
    page = paper(300, 300)
    page[100:102, 20:280] = -0.4
    page[20:280, 150:152] = -0.4
    out, mask, info = R.remove_rules(page, margin=0)
    assert info["kept"] == 0 and not (out < 0).any(), "text holds no candidate: an intersection is no crossing"
    assert np.all(mask[100:102, 150:152] == 3) and info["h_removed"] == 2 * 260 and info["v_removed"] == 2 * 260
    assert info["overwritten"] == 4 * 260 - 4


@pytest.fixture(scope="module")
def table():
    """The 512 x 512 table page of DESIGN.md §7.8: the oracle's engine, the rule-free page, the ruled page, the rules' pixels."""
    from ocrs_amd import synth
    from oracle import pipeline as OP
    from oracle.nn import OracleGraph, OracleModel
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                       recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))
    px = synth.synthetic_page(3, 512, 512, 30, 2, 1)
    clean = np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), F)[0])
    ruled, rule = R.draw_grid(clean)
    return ora, clean, ruled, rule


def test_a_page_without_rules_comes_back_as_its_own_words(table):
    _, clean, _, _ = table
    out, mask, info = R.remove_rules(clean)
    assert info["overwritten"] == 0 and info["kept"] == 0 and not mask.any()
    assert out.view(np.uint32).tobytes() == clean.view(np.uint32).tobytes()


def test_degenerate_pages_go_through():
    with np.errstate(all="raise"):   # no invalid operation on a number, no overflow
        for shape in ((70, 130), (5, 200), (1, 1)):
            n = shape[0] * shape[1]
            out, mask, info = R.remove_rules(np.full(shape, 0.4, F))
            assert info == {"paper_bin": 230, "fill": float(FILL), "ink": 0, "counted": n, "h_removed": 0, "v_removed": 0,
                            "overwritten": 0, "kept": 0}
            for c in (-0.5, 0.0, 0.25, 0.5):
                out, mask, info = R.remove_rules(np.full(shape, c, F))
                assert info["ink"] == (n if c < 0 else 0) and info["counted"] == n - info["ink"]
            out, mask, info = R.remove_rules(np.full(shape, -0.5, F))
            assert info["paper_bin"] == 255 and info["fill"] == 0.5, "nothing counted: white"
            assert info["overwritten"] == (n if shape == (5, 200) else 0), "five rows of ink are a rule, seventy are a block"
            out, mask, info = R.remove_rules(np.full(shape, np.nan, F))
            assert np.isnan(out).all() and not mask.any()
            assert info == {"paper_bin": 255, "fill": 0.5, "ink": 0, "counted": 0, "h_removed": 0, "v_removed": 0, "overwritten": 0, "kept": 0}


def test_paper_given_against_paper_measured():
    page = underlined()
    measured, mask_m, info_m = R.remove_rules(page)
    assert info_m["paper_bin"] == 230 and info_m["fill"] == float(FILL) and info_m["counted"] == int((page >= 0).sum())
    given, mask_g, info_g = R.remove_rules(page, paper=0.25)
    assert info_g["paper_bin"] == -1 and info_g["fill"] == 0.25
    assert {k: v for k, v in info_g.items() if k not in ("paper_bin", "fill")} == {k: v for k, v in info_m.items() if k not in ("paper_bin", "fill")}
    assert np.array_equal(mask_g, mask_m)
    gone = (mask_m & 7) != 0
    assert np.all(measured[gone] == F(info_m["fill"])) and np.all(given[gone] == F(0.25)) and np.array_equal(measured[~gone], given[~gone])
    nan_paper = R.remove_rules(page, paper=float("nan"))
    assert nan_paper[2] == info_m and nan_paper[0].tobytes() == measured.tobytes(), "NaN: measured"


def test_every_pixel_outside_d_keeps_its_planted_bits():
    rng = np.random.default_rng(8)
    page = (rng.random((97, 211), dtype=F) - F(0.6)).astype(F)
    words = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x40400000, 0xC0400000, 0x7F7FFFFF,
                      0xFF7FFFFF, 0x00000001, 0x80000001], np.uint32)
    flat = page.reshape(-1).view(np.uint32)
    flat[rng.choice(flat.size, size=20 * len(words), replace=False)] = np.tile(words, 20)
    for kw in ({"min_length": 3, "max_thickness": 2, "margin": 2}, {"min_length": 8, "max_thickness": 64, "margin": 8, "paper": -0.0}):
        out, mask, info = R.remove_rules(page, **kw)
        gone = (mask & 7) != 0
        assert 0 < info["overwritten"] == int(gone.sum()) < page.size
        assert np.array_equal(out.view(np.uint32)[~gone], page.view(np.uint32)[~gone]), "NaN payloads, -0.0 and infinities survive"
        assert np.all(out.view(np.uint32)[gone] == np.array([info["fill"]], F).view(np.uint32)[0])
        s = R.sets(page, kw["min_length"], kw["max_thickness"], kw["margin"])
        assert not (s["Mh"] | s["Mv"])[s["ink"]].any(), "a margin never takes ink"
        assert not (s["Kh"] & s["Dh"]).any() and not (s["Kv"] & s["Dv"]).any()


# ---------------------------------------------------------------- the table page through the oracle's detector
def test_the_table_page(table):
    ora, clean, ruled, rule = table
    out, mask, info = R.remove_rules(ruled)
    left, lost, word_ink = R.grid_counts(clean, rule, out)
    print("table page: %s; rule ink left %d, word ink lost %d of %d" % (info, left, lost, word_ink))
    assert left == 0, "no rule ink is left"
    assert lost * 100 <= word_ink, "word ink lost is at most 1 %"

    def boxes(page):
        return {np.array(w.to_array(), F).tobytes() for w in ora.detect_words(page[None])}

    want, on_ruled, on_cleaned = boxes(clean), boxes(ruled), boxes(out)
    print("table page: %d words on the rule-free page; reproduced exactly: %d on the ruled page, %d on the cleaned page"
          % (len(want), len(want & on_ruled), len(want & on_cleaned)))
    assert len(want & on_cleaned) > len(want & on_ruled)
