"""Page framing, host side: tests/frame_ref.py against a brute-force flood fill; the library's choice of
the content box and the gutter, its parameter checks and its maps back against the restatement; the new symbols; the
chooser's header clean under -fsanitize=address,undefined in a stand-alone program.  No GPU."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frame_ref as FR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["ocrs_frame_params_default", "ocrs_frame_params_check", "ocrs_engine_clean_frame_page", "ocrs_engine_clean_frame_pages",
               "ocrs_engine_ink_profiles", "ocrs_frame_choice_params_default", "ocrs_frame_choice_params_check", "ocrs_frame_choose",
               "ocrs_engine_crop_page", "ocrs_engine_crop_pages", "ocrs_uncrop_rects", "ocrs_uncrop_chars"]
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
    for name in ("ocrs_frame_params", "ocrs_frame_info", "ocrs_frame_choice_params", "ocrs_frame_choice", "ocrs_crop_rect"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert C.sizeof(_lib.FrameParams) == 20 and C.sizeof(_lib.FrameInfo) == 64
    assert C.sizeof(_lib.FrameChoiceParams) == 16 and C.sizeof(_lib.FrameChoice) == 24 and C.sizeof(_lib.CropRect) == 16
    assert [f[0] for f in _lib.FrameInfo._fields_] == list(FR.INFO_KEYS)
    assert [f[0] for f in _lib.FrameChoice._fields_] == list(FR.CHOICE_KEYS)


# ------------------------------------------------------------------ the restatement against a flood fill
def flood(ink, depth, sides, min_area):
    """(removed, kept, R) by walking from every seed over the 8 neighbours that are ink in the ring, one pixel at a time."""
    h, w = ink.shape
    R = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            R[y, x] = ink[y, x] and (depth == 0 or min(x, y, w - 1 - x, h - 1 - y) < depth)
    seen = np.zeros((h, w), bool)
    removed, kept = np.zeros((h, w), bool), np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            on_side = (sides & 1 and x == 0) or (sides & 2 and y == 0) or (sides & 4 and x == w - 1) or (sides & 8 and y == h - 1)
            if not (R[y, x] and on_side) or seen[y, x]:
                continue
            seen[y, x] = True
            comp, stack = [], [(y, x)]
            while stack:
                cy, cx = stack.pop()
                comp.append((cy, cx))
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ny, nx = cy + dy, cx + dx
                        if 0 <= ny < h and 0 <= nx < w and R[ny, nx] and not seen[ny, nx]:
                            seen[ny, nx] = True
                            stack.append((ny, nx))
            for p in comp:
                (removed if len(comp) >= min_area else kept)[p] = True
    return removed, kept, R


@pytest.mark.parametrize("density", (0.3, 0.6))
def test_the_restatement_equals_a_flood_fill_from_the_seeds(density):
    rng = np.random.default_rng(int(density * 10))
    n = 0
    for depth, sides in itertools.product((0, 1, 3), range(1, 16)):
        h, w = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        ink = rng.random((h, w)) < density
        page = np.where(ink, F(-0.3), F(0.3)).astype(F)
        for min_area in (0, 4):
            s = FR.sets(page, depth, sides, min_area)
            removed, kept, R = flood(ink, depth, sides, min_area)
            assert np.array_equal(s["R"], R) and np.array_equal(s["removed"], removed) and np.array_equal(s["kept"], kept), (h, w, depth, sides, min_area)
            out, mask, info = FR.clean_frame(page, depth, sides, min_area)
            assert np.array_equal(mask, removed * 1 + kept * 2 + R * 4)
            assert np.array_equal(out, np.where(removed, F(205.0 / 256.0 - 0.5), page)) or not (~ink).any()
            assert info["removed_pixels"] == removed.sum() and info["kept_pixels"] == kept.sum() and info["ring_ink"] == R.sum()
            n += int(removed.any()) + int(kept.any())
    assert n > 40, "the cases exercise both classes"


def test_the_restatement_on_a_bar_a_wedge_and_a_cut_glyph():
    page = np.full((60, 80), F(0.4), F)
    page[:, :5] = F(-0.4)                      # a bar down the left
    page[20:30, 30:50] = F(-0.4)               # text in the middle
    page[57:60, 40:42] = F(-0.4)               # a glyph cut by the bottom edge: 6 pixels
    page[5, 2] = np.nan
    out, mask, info = FR.clean_frame(page, depth=10, min_area=7)
    assert info["removed"] == 1 and info["removed_pixels"] == 60 * 5 - 1 and info["kept"] == 1 and info["kept_pixels"] == 6
    assert info["ink"] == 300 - 1 + 200 + 6 and info["ring_ink"] == 300 - 1 + 6 and info["counted"] == 60 * 80 - info["ink"] - 1
    assert (out[:, :5][~np.isnan(page[:, :5])] == F(231.0 / 256.0 - 0.5)).all() and np.isnan(out[5, 2])
    assert np.array_equal(out[:, 5:], page[:, 5:]) and (mask[57:60, 40:42] == 6).all() and (mask[20:30, 30:50] == 0).all()
    out, _, info = FR.clean_frame(page, depth=10, sides=2 | 4)   # the bar touches the top too; the glyph only the bottom
    assert info["removed"] == 1 and info["kept"] == 0 and np.array_equal(out[57:60], np.where(np.arange(80) < 5, F(231.0 / 256.0 - 0.5), page[57:60]))
    assert FR.clean_frame(page, depth=10, paper=0.25)[0][0, 0] == F(0.25) and FR.clean_frame(page, paper=0.25)[2]["paper_bin"] == -1


# ------------------------------------------------------------------ the choice
def lib_choose(lib, h, w, cols, rows, **kw):
    from ocrs_amd import _lib
    p = _lib.FrameChoiceParams()
    assert lib.ocrs_frame_choice_params_default(C.byref(p)) == 0
    for k, v in kw.items():
        setattr(p, k, v)
    out = _lib.FrameChoice()
    cols, rows = np.ascontiguousarray(cols, np.uint32), np.ascontiguousarray(rows, np.uint32)
    st = lib.ocrs_frame_choose(h, w, cols.ctypes.data_as(C.POINTER(C.c_uint32)), rows.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(p), C.byref(out))
    assert st == 0, st
    return out.as_dict()


def planted_choices():
    """(name, h, w, cols, rows, params, expected or None) of the hand-made cases."""
    cases = []
    z = lambda n: np.zeros(n, np.uint32)   # noqa: E731
    cases.append(("no ink", 30, 40, z(40), z(30), {}, {"found": 0, "x0": 0, "y0": 0, "x1": 40, "y1": 30, "gutter_x": -1}))
    c, r = z(40), z(30)
    r[3] = 5   # ink in a row but in no column of min_count
    cases.append(("rows alone", 30, 40, c, r, {}, {"found": 0, "x0": 0, "y0": 0, "x1": 40, "y1": 30, "gutter_x": -1}))
    c, r = z(200), z(100)
    c[77], r[40] = 1, 1
    cases.append(("one inked column", 100, 200, c, r, {}, {"found": 1, "x0": 61, "y0": 24, "x1": 94, "y1": 57, "gutter_x": -1}))
    cases.append(("one inked column, a gutter of width 0 is none", 100, 200, c, r, {"gutter_min_width": 1, "pad": 0},
                  {"found": 1, "x0": 77, "y0": 40, "x1": 78, "y1": 41, "gutter_x": -1}))
    for name, x, y in (("left", 3, 50), ("top", 100, 5), ("right", 196, 50), ("bottom", 100, 97)):
        c, r = z(200), z(100)
        c[x], r[y] = 9, 9
        cases.append(("pad clipped at the %s" % name, 100, 200, c, r, {"pad": 16},
                      {"found": 1, "x0": max(x - 16, 0), "y0": max(y - 16, 0), "x1": min(x + 17, 200), "y1": min(y + 17, 100), "gutter_x": -1}))
    # content [100, 900): the band is [400, 600), its centre 500
    def spread(quiet):
        c = np.full(1000, 3, np.uint32)
        c[:100] = 0
        c[900:] = 0
        for a, b in quiet:
            c[a:b] = 0
        return c
    rows = np.full(50, 7, np.uint32)
    cases.append(("two equal runs: the more central", 50, 1000, spread([(420, 440), (520, 540)]), rows, {}, None))   # |2*430-1000| = 140, |2*530-1000| = 60
    cases.append(("two equal runs at the same distance: the leftmost", 50, 1000, spread([(460, 480), (520, 540)]), rows, {}, None))   # 60 and 60
    cases.append(("the longer run wins over the more central", 50, 1000, spread([(410, 440), (495, 505)]), rows, {}, None))
    cases.append(("a run one short of gutter_min_width", 50, 1000, spread([(500, 507)]), rows, {"gutter_min_width": 8}, None))
    cases.append(("a run of exactly gutter_min_width", 50, 1000, spread([(500, 508)]), rows, {"gutter_min_width": 8}, None))
    cases.append(("a quiet run crossing the band's end", 50, 1000, spread([(590, 700)]), rows, {}, None))
    cases.append(("a quiet run crossing the band's start", 50, 1000, spread([(300, 410)]), rows, {}, None))
    cases.append(("quiet by gutter_max_ink", 50, 1000, spread([]), rows, {"gutter_max_ink": 3}, None))
    cases.append(("min_count above the bar's ink", 50, 1000, spread([(480, 520)]) + np.where(np.arange(1000) < 10, 2, 0).astype(np.uint32), rows,
                  {"min_count": 3}, None))
    return cases


def test_the_choice_on_planted_cases(lib):
    seen = {}
    for name, h, w, cols, rows, kw, exp in planted_choices():
        ref = FR.choose(h, w, cols, rows, **kw)
        if exp is not None:
            assert ref == exp, (name, ref)
        got = lib_choose(lib, h, w, cols, rows, **kw)
        assert got == ref and tuple(got) == FR.CHOICE_KEYS, (name, got, ref)
        seen[name] = ref["gutter_x"]
    assert seen["two equal runs: the more central"] == 530 and seen["two equal runs at the same distance: the leftmost"] == 470
    assert seen["the longer run wins over the more central"] == 425
    assert seen["a run one short of gutter_min_width"] == -1 and seen["a run of exactly gutter_min_width"] == 504
    assert seen["a quiet run crossing the band's end"] == 595 and seen["a quiet run crossing the band's start"] == 405
    assert seen["quiet by gutter_max_ink"] == 500 and seen["min_count above the bar's ink"] == 500


def random_choices(n, seed):
    rng = np.random.default_rng(seed)
    for i in range(n):
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 400))
        dens = rng.choice([0.02, 0.3, 0.9])
        cols = (rng.random(w) < dens) * rng.integers(1, 6, w)
        rows = (rng.random(h) < dens) * rng.integers(1, 6, h)
        kw = {"min_count": int(rng.integers(1, 4)), "pad": int(rng.integers(0, 40)), "gutter_min_width": int(rng.integers(1, 12)),
              "gutter_max_ink": int(rng.integers(0, 4))}
        yield h, w, cols.astype(np.uint32), rows.astype(np.uint32), kw


def test_the_choice_on_random_profiles(lib):
    gutters = 0
    for h, w, cols, rows, kw in random_choices(400, 5):
        got, ref = lib_choose(lib, h, w, cols, rows, **kw), FR.choose(h, w, cols, rows, **kw)
        assert got == ref, (h, w, kw, cols.tolist(), rows.tolist())
        gutters += ref["gutter_x"] >= 0
    assert 50 < gutters < 350


def test_parameter_checks(lib):
    from ocrs_amd import _lib, frame_params
    nan, inf = float("nan"), float("inf")
    p = _lib.FrameParams()
    assert lib.ocrs_frame_params_default(C.byref(p)) == 0
    assert (p.threshold, p.depth, p.sides, p.min_area) == (0.0, 128, 15, 0) and p.paper != p.paper
    assert lib.ocrs_frame_params_default(None) == 1 and lib.ocrs_frame_params_check(None) == 1
    good = [(0.0, 0, 1, 0, nan), (-0.25, 65535, 15, 2 ** 31 - 1, 0.5), (0.1, 128, 8, 0, -3.0)]
    bad = [(nan, 128, 15, 0, nan), (inf, 128, 15, 0, nan), (0.0, -1, 15, 0, nan), (0.0, 65536, 15, 0, nan), (0.0, 128, 0, 0, nan),
           (0.0, 128, 16, 0, nan), (0.0, 128, -1, 0, nan), (0.0, 128, 15, -1, nan), (0.0, 128, 15, 0, inf), (0.0, 128, 15, 0, -inf)]
    for vals, status in [(g, 0) for g in good] + [(b, 1) for b in bad]:
        assert lib.ocrs_frame_params_check(C.byref(_lib.FrameParams(*vals))) == status, vals
        paper = None if vals[4] != vals[4] else vals[4]
        assert FR.valid_params(vals[0], vals[1], vals[2], vals[3], paper) == (status == 0), vals
    assert frame_params() == {"depth": 128, "sides": 15, "min_area": 0, "threshold": 0.0, "paper": None}
    assert frame_params(sides="lb", depth=0, paper=0.25) == {"depth": 0, "sides": 9, "min_area": 0, "threshold": 0.0, "paper": 0.25}
    with pytest.raises(ValueError):
        frame_params(sides="LX")
    with pytest.raises(_lib.OcrsError):
        frame_params(depth=65536)
    q = _lib.FrameChoiceParams()
    assert lib.ocrs_frame_choice_params_default(C.byref(q)) == 0
    assert (q.min_count, q.pad, q.gutter_min_width, q.gutter_max_ink) == (1, 16, 8, 0)
    assert lib.ocrs_frame_choice_params_default(None) == 1 and lib.ocrs_frame_choice_params_check(None) == 1
    cols, rows = np.ones(4, np.uint32), np.ones(3, np.uint32)
    pc, pr = cols.ctypes.data_as(C.POINTER(C.c_uint32)), rows.ctypes.data_as(C.POINTER(C.c_uint32))
    out = _lib.FrameChoice()
    for vals, status in (((1, 0, 1, 0), 0), ((2 ** 31 - 1, 65535, 2 ** 31 - 1, 2 ** 31 - 1), 0), ((0, 16, 8, 0), 1), ((1, -1, 8, 0), 1),
                         ((1, 65536, 8, 0), 1), ((1, 16, 0, 0), 1), ((1, 16, 8, -1), 1)):
        assert lib.ocrs_frame_choice_params_check(C.byref(_lib.FrameChoiceParams(*vals))) == status, vals
        assert FR.valid_choice_params(*vals) == (status == 0), vals
        assert lib.ocrs_frame_choose(3, 4, pc, pr, C.byref(_lib.FrameChoiceParams(*vals)), C.byref(out)) == status, vals
    assert lib.ocrs_frame_choose(3, 4, pc, pr, None, C.byref(out)) == 0 and out.as_dict() == FR.choose(3, 4, cols, rows), "NULL: the default"
    for h, w in ((0, 4), (3, 0), (65536, 4), (3, 65536), (-1, 4)):
        assert lib.ocrs_frame_choose(h, w, pc, pr, None, C.byref(out)) == 1, (h, w)
    assert lib.ocrs_frame_choose(3, 4, None, pr, None, C.byref(out)) == 1 and lib.ocrs_frame_choose(3, 4, pc, pr, None, None) == 1


def test_uncrop_maps_equal_numpy(lib):
    from ocrs_amd import TextChar, TextLine, uncrop_boxes, uncrop_lines, uncrop_rects
    rng = np.random.default_rng(8)
    rects = (rng.random((50, 6)) * 2000 - 500).astype(F)
    rects.view(np.uint32)[3, 0] = 0x7FC12345   # a NaN centre stays NaN; the other fields keep their bits
    rects[4, 2:] = [np.inf, -0.0, 1e-40, -1e30]
    boxes = rng.integers(-3000, 3000, (50, 4)).astype(np.int32)
    boxes[0] = [2 ** 31 - 1, -2 ** 31, 0, 5]   # wraps
    for origin in ((0, 0), (17, 3), (-40, 1000), (65534, -65534), (2 ** 31 - 1, -2 ** 31)):
        got, ref = uncrop_rects(rects, origin), FR.uncrop_rects(rects, origin)
        assert got.dtype == np.float32 and got.tobytes() == ref.tobytes(), origin
        assert got[:, 2:].tobytes() == rects[:, 2:].tobytes(), "only the centre moves"
        assert np.array_equal(uncrop_boxes(boxes, origin), FR.uncrop_boxes(boxes, origin)), origin
    assert uncrop_rects(np.zeros((0, 6), F), (3, 4)).shape == (0, 6) and uncrop_boxes(np.zeros((0, 4), np.int32), (3, 4)).shape == (0, 4)
    assert lib.ocrs_uncrop_rects(None, C.c_size_t(2), 1, 1) == 1 and lib.ocrs_uncrop_chars(None, C.c_size_t(2), 1, 1) == 1
    assert lib.ocrs_uncrop_rects(None, C.c_size_t(0), 1, 1) == 0
    line = TextLine([TextChar("a", (1, 2, 11, 9), -0.5), TextChar("b", (1, 10, 11, 18), -0.25)], -0.75)
    moved = uncrop_lines([line, None], (100, 1000))
    assert moved[1] is None and str(moved[0]) == "ab" and moved[0].score == line.score
    assert [c.rect for c in moved[0].chars()] == [(1001, 102, 1011, 109), (1001, 110, 1011, 118)]
    assert [c.logp for c in moved[0].chars()] == [-0.5, -0.25]


def test_the_restatements_crop_and_profiles():
    page = np.arange(12, dtype=F).reshape(3, 4) - F(5)
    assert np.array_equal(FR.crop(page, (1, 1, 3, 3), 9.0), page[1:3, 1:3])
    assert np.array_equal(FR.crop(page, (-1, -1, 2, 1), 9.0), np.array([[9, 9, 9], [9, -5, -4]], F)) and FR.crop(page, (10, 10, 11, 12), 9.0).tolist() == [[9.0], [9.0]]
    assert np.array_equal(FR.crop(page, (3, 2, 6, 4), 9.0), np.array([[6, 9, 9], [9, 9, 9]], F))
    nan = np.array([0x7F812345], np.uint32).view(F)[0]
    assert FR.crop(page, (4, 0, 5, 1), nan).view(np.uint32)[0, 0] == 0x7F812345
    cols, rows = FR.profiles(page)
    assert cols.tolist() == [2, 1, 1, 1] and rows.tolist() == [4, 1, 0] and cols.dtype == np.uint32


# ------------------------------------------------------------------ the chooser under the sanitizers
def test_the_chooser_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/sanitize/frame_harness.cpp, a stand-alone program over frame_choose.hpp, on this file's cases."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "frame_harness")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(HERE, "sanitize", "frame_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, "building the sanitizer harness failed:\n" + r.stderr[-3000:]
    cases = [(h, w, cols, rows, dict(FR.default_choice_params(), **kw)) for _, h, w, cols, rows, kw, _ in planted_choices()]
    cases += [(h, w, cols, rows, kw) for h, w, cols, rows, kw in random_choices(100, 6)]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for h, w, cols, rows, kw in cases:
            f.write(np.array([h, w, kw["min_count"], kw["pad"], kw["gutter_min_width"], kw["gutter_max_ink"]], np.int32).tobytes())
            f.write(np.ascontiguousarray(cols, np.uint32).tobytes() + np.ascontiguousarray(rows, np.uint32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases) + 1 and lines[-1].startswith("extremes ")
    for line, (h, w, cols, rows, kw) in zip(lines, cases):
        ref = FR.choose(h, w, cols, rows, **kw)
        assert [int(v) for v in line.split()] == [ref[k] for k in FR.CHOICE_KEYS], (line, ref)
