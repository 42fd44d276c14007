"""Perspective correction, host side: the library's outline choice, quad map, unproject maps and parameter
checks equal tests/perspective_ref.py bit for bit; the restatement recovers the corners of planted quads, and the library's
choice over the restatement's peaks of those photos equals the restatement's; the host
arithmetic is clean under -fsanitize=address,undefined in a stand-alone program.  No GPU."""
import ctypes as C
import functools
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import perspective_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")
FIXTURES = sorted(p for p in glob.glob(os.path.join(G, "**", "*.npz"), recursive=True) if "word_rects" in np.load(p).files)
IDS = [os.path.relpath(p, G)[:-4] for p in FIXTURES]
NEW_SYMBOLS = ["ocrs_outline_params_default", "ocrs_outline_params_check", "ocrs_engine_edge_peaks", "ocrs_outline_choose",
               "ocrs_engine_find_outline", "ocrs_quad_map", "ocrs_engine_project_page", "ocrs_engine_project_pages", "ocrs_unproject_rects",
               "ocrs_unproject_chars"]
NAMES = ("why-rust", "polar-bears", "rust-book")
WH, WW = 400, 480   # the work page of the hand-made peaks


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
    for name in ("ocrs_outline_params", "ocrs_outline_info"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    # a code object of its own, in the build; the deskew kernels' file does not know of it
    from ocrs_amd import build
    assert "kernels_perspective.hip" in build.SOURCES and "perspective.cpp" in build.SOURCES
    assert "perspective" not in open(os.path.join(ROOT, "ocrs_amd", "csrc", "kernels_deskew.hip")).read()


def test_outline_params_default_and_refusals(lib):
    import ocrs_amd
    from ocrs_amd._lib import OcrsError
    assert ocrs_amd.outline_params() == P.default_params()
    assert P.plan(P.default_params()) == 30 and len(P.table_of(P.default_params())) == 61
    good = [{}, {"work_max_side": 1}, {"work_max_side": 4096}, {"max_deg": 45.0}, {"step_deg": 0.1}, {"max_deg": 0.5}, {"min_step": 1}, {"min_step": 256},
            {"min_cover": 1.0}, {"min_span": 1.0}, {"min_area": 0.0}, {"min_area": 1.0}, {"min_cover": 1e-6}]
    bad = [{"work_max_side": 0}, {"work_max_side": 4097}, {"max_deg": 0.0}, {"max_deg": 45.5}, {"max_deg": float("nan")}, {"step_deg": 0.0},
           {"step_deg": -0.1}, {"step_deg": float("inf")}, {"step_deg": float("nan")}, {"step_deg": 16.0}, {"step_deg": 0.001}, {"min_step": 0},
           {"min_step": 257}, {"min_cover": 0.0}, {"min_cover": 1.5}, {"min_cover": float("nan")}, {"min_span": 0.0}, {"min_span": 1.01},
           {"min_span": float("nan")}, {"min_area": -0.1}, {"min_area": 1.1}, {"min_area": float("nan")}]
    for kw in good:
        assert P.plan(dict(P.default_params(), **kw)) is not None, kw
        ocrs_amd.outline_params(**kw)
    for kw in bad:
        assert P.plan(dict(P.default_params(), **kw)) is None, kw
        with pytest.raises(OcrsError) as ei:
            ocrs_amd.outline_params(**kw)
        assert ei.value.status_name == "INVALID_ARGUMENT", kw
    with pytest.raises(TypeError):
        ocrs_amd.outline_params(fine_step_deg=0.1)


# ---------------------------------------------------------------- choose
def peak_of(table, family, sign, a, pos, count, wh=WH, ww=WW):
    """(family, sign, a, band, entry): the peak a line of angle index a and position pos leaves."""
    S, C = [int(v) for v in table[a]]
    fw, fh = (ww, wh) if family == 0 else (wh, ww)
    t0 = min(0, (fw - 1) * S) + min(0, (fh - 1) * C)
    b = (int(round(((fw - 1) / 2.0 * S + pos * C))) - t0) >> 16
    nb = wh + ww
    band = [k for k in range(16) if k * nb // 16 <= b < (k + 1) * nb // 16][0]
    return family, sign, a, band, (count << 32) | (0xFFFFFFFF - b)


def peaks_of(table, entries):
    pk = np.zeros((2, 2, len(table), 16), np.uint64)
    for f, s, a, band, e in entries:
        pk[f, s, a, band] = max(int(pk[f, s, a, band]), e)
    return pk


def hand_made_cases():
    """(name, peaks, table, work_hw, page_hw, params, expected found)."""
    t = P.table_of(P.default_params())
    Z = 30   # the index of angle 0
    frame = [(0, 0, Z, 50.0, 300), (0, 1, Z, 350.0, 310), (1, 0, Z + 2, 40.0, 280), (1, 1, Z - 3, 440.0, 290)]
    mk = lambda lines: peaks_of(t, [peak_of(t, *l) for l in lines])
    hw = (WH, WW)
    out = [("no candidate", mk([]), t, hw, hw, {}, 0),
           ("counts under min_cover", mk([(f, s, a, p, 90) for f, s, a, p, _ in frame]), t, hw, hw, {}, 0),
           ("a sheet lighter than the desk", mk(frame), t, hw, hw, {}, 1),
           ("a sheet darker than the desk", mk([(f, 1 - s, a, p, c) for f, s, a, p, c in frame]), t, hw, hw, {}, 1),
           ("family V missing", mk(frame[:2]), t, hw, hw, {}, 0),
           ("family H missing", mk(frame[2:]), t, hw, hw, {}, 0),
           ("one side missing", mk(frame[:3]), t, hw, hw, {}, 0),
           ("sides too close", mk([frame[0], (0, 1, Z, 140.0, 310)] + frame[2:]), t, hw, hw, {}, 0),
           ("sides in the wrong order", mk([(0, 0, Z, 350.0, 300), (0, 1, Z, 50.0, 310)] + frame[2:]), t, hw, hw, {}, 0),
           # both sign orders hold a frame of the same sum: `+` first wins
           ("sign tie", mk(frame + [(0, 1, Z + 1, 60.0, 300), (0, 0, Z + 1, 340.0, 310), (1, 1, Z, 50.0, 280), (1, 0, Z, 430.0, 290)]), t, hw, hw, {}, 1),
           # `-` first has the larger sum
           ("the other order wins", mk(frame + [(0, 1, Z + 1, 60.0, 301), (0, 0, Z + 1, 340.0, 310), (1, 1, Z, 50.0, 280), (1, 0, Z, 430.0, 290)]), t, hw, hw, {}, 1),
           # two tops and two lefts of equal count: the lower (angle index, bin) is taken
           ("pair ties", mk(frame + [(0, 0, Z - 4, 80.0, 300), (0, 0, Z, 20.0, 300), (1, 0, Z + 2, 90.0, 280), (1, 0, Z - 1, 60.0, 280)]), t, hw, hw, {}, 1),
           # top and bottom cross between the left side and the page's middle: TL lies below BL
           ("not convex", mk([(0, 0, 60, 150.0, 300), (0, 1, 0, 260.0, 300), (1, 0, Z, 10.0, 280), (1, 1, Z, 440.0, 290)]), t, hw, hw, {}, 0),
           ("too small a quad", mk(frame), t, hw, hw, {"min_area": 0.9}, 0),
           ("a work copy of a larger page", mk(frame), t, hw, (3000, 2200), {}, 1),
           ("a looser cover", mk([(f, s, a, p, 90) for f, s, a, p, _ in frame]), t, hw, hw, {"min_cover": 0.15}, 1)]
    # a cosine of zero: no finite position
    t90 = np.array([[65536, 0], [0, 65536]], np.int32)
    out.append(("a table with a right angle", peaks_of(t90, [peak_of(t90, *l) for l in [(0, 0, 1, 50.0, 300), (0, 1, 1, 350.0, 310), (1, 0, 1, 40.0, 280), (1, 1, 1, 440.0, 290),
                                                                                   (0, 0, 0, 50.0, 900), (1, 1, 0, 50.0, 900)]]), t90, hw, hw, {}, 1))
    rng = np.random.default_rng(3)
    for i in range(24):   # peaks of random counts and bins: whatever is chosen, it is chosen alike
        A = int(rng.integers(1, 9))
        tr = P.table_of(dict(P.default_params(), step_deg=15.0 / max(A // 2, 1)))[:A] if i % 2 else np.stack(
            [rng.integers(-30000, 30001, A), rng.integers(40000, 65537, A)], axis=1).astype(np.int32)
        A = len(tr)
        wh, ww = int(rng.integers(20, 600)), int(rng.integers(20, 600))
        nb = wh + ww
        pk = np.zeros((2, 2, A, 16), np.uint64)
        for idx in np.ndindex(2, 2, A, 16):
            lo, hi = idx[3] * nb // 16, (idx[3] + 1) * nb // 16
            if rng.random() < 0.5 and hi > lo:
                pk[idx] = (int(rng.integers(1, 700)) << 32) | (0xFFFFFFFF - int(rng.integers(lo, hi)))
        out.append(("random %d" % i, pk, tr, (wh, ww), (wh * (1 + i % 3), ww * (1 + i % 2)), {"min_cover": 0.05 + 0.1 * (i % 4), "min_area": 0.02}, None))
    return out


def info_tuple(o):
    """Outline (the library's) or dict (the restatement's) -> comparable."""
    if isinstance(o, dict):
        return (int(o["found"]), int(o["polarity"]), np.asarray(o["corners"], np.float32).tobytes(), tuple(o["counts"]), tuple(o["angles"]), tuple(o["work_hw"]))
    return (int(o.found), o.polarity, o.corners.astype(np.float32).tobytes(), o.counts, o.angles, o.work_hw)


def test_choose_on_hand_made_peaks_bit_for_bit(lib):
    import ocrs_amd
    found = 0
    for name, pk, table, work_hw, page_hw, params, expect in hand_made_cases():
        ref = P.choose(pk, table, work_hw, page_hw, params)
        got = ocrs_amd.outline_choose(pk, table, work_hw, page_hw, **params)
        assert info_tuple(got) == info_tuple(ref), (name, got, ref)
        if expect is not None:
            assert ref["found"] == expect, (name, ref)
        found += ref["found"]
        if not ref["found"]:
            assert not got.corners.any() and got.counts == (0, 0, 0, 0)
    assert found >= 12, "the random cases choose outlines too"
    cases = {c[0]: P.choose(*c[1:6]) for c in hand_made_cases()[:17]}
    assert cases["a sheet lighter than the desk"]["polarity"] == 0 and cases["a sheet darker than the desk"]["polarity"] == 1
    assert cases["a sheet lighter than the desk"]["counts"] == (300, 310, 280, 290) and cases["a sheet lighter than the desk"]["angles"] == (30, 30, 32, 27)
    assert cases["sign tie"]["polarity"] == 0 and cases["the other order wins"]["polarity"] == 1
    assert cases["pair ties"]["angles"][0] == 26 and cases["pair ties"]["angles"][2] == 29, cases["pair ties"]
    # the corners of an axis-parallel frame: the edge lies between the two pixels of the difference, at bin + 1 (a
    # horizontal line's pixels all project onto the bin's lower end, half a pixel under the bin's middle)
    t = P.table_of(P.default_params())
    box = P.choose(peaks_of(t, [peak_of(t, 0, 0, 30, 50.0, 300), peak_of(t, 0, 1, 30, 350.0, 300), peak_of(t, 1, 0, 30, 40.0, 300), peak_of(t, 1, 1, 30, 440.0, 300)]),
                   t, (WH, WW), (WH, WW))
    assert box["corners"].tolist() == [41.0, 51.0, 441.0, 51.0, 441.0, 351.0, 41.0, 351.0]
    big = P.choose(peaks_of(t, [peak_of(t, 0, 0, 30, 50.0, 300), peak_of(t, 0, 1, 30, 350.0, 300), peak_of(t, 1, 0, 30, 40.0, 300), peak_of(t, 1, 1, 30, 440.0, 300)]),
                   t, (WH, WW), (4 * WH, 2 * WW))
    assert big["corners"].tolist() == [82.5, 205.5, 882.5, 205.5, 882.5, 1405.5, 82.5, 1405.5], "(p + 0.5) * scale - 0.5 per axis"


def test_choose_refusals(lib):
    import ocrs_amd
    from ocrs_amd._lib import OcrsError
    t = P.table_of(P.default_params())
    pk = np.zeros((2, 2, 61, 16), np.uint64)
    for args, kw in (((pk, t, (0, 5), (5, 5)), {}), ((pk, t, (5, 4097), (5, 5)), {}), ((pk, t, (5, 5), (0, 5)), {}), ((pk, t, (5, 5), (5, 5)), {"min_cover": 0.0})):
        with pytest.raises(OcrsError) as ei:
            ocrs_amd.outline_choose(*args, **kw)
        assert ei.value.status_name == "INVALID_ARGUMENT"
    with pytest.raises(OcrsError):
        ocrs_amd.outline_choose(np.zeros((2, 2, 1, 16), np.uint64), np.array([[65537, 0]], np.int32), (5, 5), (5, 5))
    with pytest.raises(ValueError):
        ocrs_amd.outline_choose(pk[:, :, :3], t, (5, 5), (5, 5))
    # the pair search is quadratic in the peaks: the choice takes the 4095 angles find_outline's own table can hold
    many = np.tile(np.array([[0, 65536]], np.int32), (4096, 1))
    with pytest.raises(OcrsError) as ei:
        ocrs_amd.outline_choose(np.zeros((2, 2, 4096, 16), np.uint64), many, (5, 5), (5, 5))
    assert ei.value.status_name == "INVALID_ARGUMENT"
    assert not ocrs_amd.outline_choose(np.zeros((2, 2, 4095, 16), np.uint64), many[:4095], (5, 5), (5, 5)).found


# ---------------------------------------------------------------- quad_map
QUADS = {"keystone": [70, 40, 410, 40, 445, 360, 35, 360], "mild": [60, 50, 420, 44, 430, 352, 52, 360], "tilted": [95, 38, 425, 70, 398, 372, 52, 335]}


def quads():
    out = [P.page_corners(300, 400), P.page_corners(1, 1), P.page_corners(65535, 17), P.page_corners(3000, 2200)]
    out += [np.array(q, np.float32) for q in QUADS.values()]
    out += [np.array([-40.5, -30.25, 5000.75, 100.0, 5200.0, 7000.5, -300.0, 6500.0], np.float32),      # corners outside any page
            np.array([0.1, 0.1, 0.6, 0.1, 0.6, 0.4, 0.1, 0.4], np.float32),                              # under a pixel: sizes clamp to 1
            np.array([0, 0, 1e5, 0, 1e5, 1e5, 0, 1e5], np.float32),                                     # sizes clamp to 65535
            np.array([10, 10, 200, 10, 10, 200, 200, 200], np.float32),                                 # a bow tie
            np.array([200, 10, 10, 10, 10, 200, 200, 200], np.float32),                                 # mirrored
            np.array([5, 5, 5, 5, 5, 5, 5, 5], np.float32), np.array([0, 0, 10, 0, 20, 0, 30, 0], np.float32),   # no area
            np.array([0, 0, 10, 10, 10, 0, 0, 10], np.float32),
            np.array([np.nan, 0, 10, 0, 10, 10, 0, 10], np.float32), np.array([0, 0, np.inf, 0, 10, 10, 0, 10], np.float32),
            np.array([3e38, 3e38, -3e38, 3e38, -3e38, -3e38, 3e38, -3e38], np.float32),
            np.array([0, 0, 3e38, 0, 3e38, 1, 0, 1], np.float32)]
    rng = np.random.default_rng(8)
    out += [(rng.random(8) * 1000.0 - 200.0).astype(np.float32) for _ in range(40)]
    return out


def lib_quad_map(q):
    import ocrs_amd
    from ocrs_amd._lib import OcrsError
    try:
        return ocrs_amd.quad_map(q)
    except OcrsError as e:
        assert e.status_name == "INVALID_ARGUMENT"
        return None


def test_quad_map_equals_the_restatement_bit_for_bit(lib):
    made = 0
    for q in quads():
        got, ref = lib_quad_map(q), P.quad_map(q)
        assert (got is None) == (ref is None), q.tolist()
        if ref is not None:
            made += 1
            assert got[0] == ref[0] and got[1].dtype == np.float32 and got[1].tobytes() == ref[1].tobytes(), q.tolist()
    assert made >= 40
    for i in (12, 13, 15, 16):
        assert P.quad_map(quads()[i]) is None, "no area, or a value that is not finite: %s" % quads()[i].tolist()
    assert P.quad_map(quads()[8])[0] == (1, 1) and P.quad_map(quads()[9])[0] == (65535, 65535)


@pytest.mark.parametrize("hw", [(300, 400), (1, 1), (65535, 17), (3000, 2200), (776, 2320)])
def test_the_pages_own_corners_give_the_identity_map(lib, hw):
    import ocrs_amd
    out_hw, m = ocrs_amd.quad_map(ocrs_amd.page_corners(hw))
    assert out_hw == hw and m.tolist() == [-0.5, 1.0, 0.0, -0.5, 0.0, 1.0, 0.0, 0.0]   # X = ox, Y = oy
    assert np.array_equal(ocrs_amd.page_corners(hw).reshape(-1), P.page_corners(*hw))


def ulp32(v):
    return float(np.spacing(np.abs(np.float32(v))))


@pytest.mark.parametrize("name", list(QUADS) + ["outside"])
def test_quad_map_sends_the_output_corners_onto_the_quad(lib, name):
    """The map in exact arithmetic sends (0, 0), (W', 0), (W', H'), (0, H') onto the quad.  Its float32 coefficients are
    each off by at most half an ulp: e_i = ulp(m_i) / 2.  At an output corner (fx, fy), in double: the numerator is off by at
    most eN = e0 + e1 fx + e2 fy (rows 3 .. 5 for y), the denominator dn by eD = e6 fx + e7 fy; X = N / dn moves by at most
    (eN + |X| eD) / (dn - eD) to first order, and the double arithmetic of the check itself adds far less than the factor
    1.01 this bound is widened by."""
    import ocrs_amd
    q = np.array(QUADS[name] if name in QUADS else quads()[7], np.float32)
    (oh, ow), m = ocrs_amd.quad_map(q)
    md = m.astype(np.float64)
    e = np.array([ulp32(v) / 2.0 for v in m])
    for (fx, fy), (qx, qy) in zip(((0.0, 0.0), (ow, 0.0), (ow, oh), (0.0, oh)), q.astype(np.float64).reshape(4, 2)):
        dn = 1.0 + md[6] * fx + md[7] * fy
        X, Y = (md[0] + md[1] * fx + md[2] * fy) / dn, (md[3] + md[4] * fx + md[5] * fy) / dn
        eD = e[6] * fx + e[7] * fy
        assert dn - eD > 0.0
        bx = 1.01 * ((e[0] + e[1] * fx + e[2] * fy) + abs(qx) * eD) / (dn - eD)
        by = 1.01 * ((e[3] + e[4] * fx + e[5] * fy) + abs(qy) * eD) / (dn - eD)
        assert abs(X - qx) <= bx and abs(Y - qy) <= by, (name, (fx, fy), X - qx, bx, Y - qy, by)
        assert bx < 2e-3 and by < 2e-3


# ---------------------------------------------------------------- unproject
def maps():
    out = [P.quad_map(P.page_corners(1024, 1024))[1]] + [P.quad_map(np.array(q, np.float32))[1] for q in QUADS.values()]
    out.append(P.quad_map(quads()[7])[1])
    out.append(np.array([3.25, 1.5, 0.25, -7.5, -0.125, 0.75, 0.0, 0.0], np.float32))          # affine: an anisotropic scale with shear
    out.append(np.array([10.0, 0.9, 0.1, 20.0, -0.05, 1.1, -0.002, 0.0005], np.float32))       # dn crosses zero at fx = 500 + fy / 4
    out.append(np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], np.float32))                 # a degenerate map: up stays
    out.append(np.array([0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 3e38, 3e38], np.float32))               # dn overflows a float, not a double
    out.append(np.array([3e38, 3e38, 3e38, -3e38, 3e38, 3e38, 1e-30, 1e-30], np.float32))
    return out


def hand_made_rects():
    return np.array([
        [10.0, 20.0, 0.0, -1.0, 30.0, 8.0],
        [0.0, 0.0, -0.0, 1.0, 0.0, 0.0],                      # zero sizes, a negative zero
        [-0.0, 5.5, 0.0, -1.0, 0.0, 12.0],
        [5.0, 6.0, 0.0, 0.0, 3.0, 4.0],                       # no up vector
        [600.0, 100.0, 0.6, -0.8, 40.0, 9.0],                 # behind the horizon of the map whose dn crosses zero
        [499.5, -0.5, 0.0, -1.0, 40.0, 9.0],                  # on it: dn = 0
        [3e38, -3e38, 1e30, -1e30, 3e38, 2e38],               # huge
        [1e30, 3e38, 0.0, -1.0, 1e-30, 3e38],
        [np.nan, 1.0, 0.0, -1.0, 4.0, 4.0],
        [1.0, np.nan, np.nan, -1.0, 4.0, 4.0],
        [1.0, 2.0, 0.0, -1.0, np.inf, 4.0],
        [np.inf, -np.inf, np.inf, -np.inf, np.inf, np.nan],
    ], np.float32)


def assert_unproject_equal(rects, what):
    import ocrs_amd
    rects = np.asarray(rects, np.float32)
    for m in maps():
        got, exp = ocrs_amd.unproject_rects(rects, m), P.unproject_rects(rects, m)
        assert got.dtype == np.float32 and got.shape == exp.shape
        assert got.view(np.uint32).tobytes() == exp.view(np.uint32).tobytes(), (what, m.tolist())
        bad = ~np.all(np.isfinite(rects), axis=1)
        assert got[bad].view(np.uint32).tobytes() == rects[bad].view(np.uint32).tobytes(), "what is not finite passes through"


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_unproject_rects_on_fixture_words_bit_for_bit(lib, path):
    assert len(FIXTURES) == 37
    assert_unproject_equal(np.load(path)["word_rects"], os.path.basename(path))


def test_unproject_rects_on_hand_made_rects_bit_for_bit(lib):
    import ocrs_amd
    from ocrs_amd._lib import OcrsError
    assert_unproject_equal(hand_made_rects(), "hand made")
    assert ocrs_amd.unproject_rects(np.zeros((0, 6), np.float32), maps()[1]).shape == (0, 6)
    one = [[1.0, 2.0, 0.0, -1.0, 30.0, 10.0]]
    assert ocrs_amd.unproject_rects(one, maps()[0]).tolist() == one, "the identity"
    crossing = maps()[6]
    r = hand_made_rects()
    back = ocrs_amd.unproject_rects(r, crossing)
    assert back[4].tobytes() == r[4].tobytes() and back[5].tobytes() == r[5].tobytes(), "dn <= 0 passes through"
    assert back[0].tobytes() != r[0].tobytes()
    # with m6 = m7 = 0 the centre and up are unwarp_rects'; the sizes follow up, so they agree for an upright rect
    import deskew_ref as D
    aff = maps()[5]
    assert np.array_equal(ocrs_amd.unproject_rects(one, aff)[:, :4], D.unwarp_rects(one, aff[:6])[:, :4])
    for bad in ([np.nan, 1, 0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 0, 1, 0, np.inf]):
        with pytest.raises(OcrsError) as ei:
            ocrs_amd.unproject_rects(one, np.array(bad, np.float32))
        assert ei.value.status_name == "INVALID_ARGUMENT"
        with pytest.raises(OcrsError):
            ocrs_amd.unproject_boxes([[1, 2, 3, 4]], np.array(bad, np.float32))
    with pytest.raises(ValueError):
        ocrs_amd.unproject_rects(one, aff[:6])


def fixture_boxes():
    z = np.load(os.path.join(G, "bench_page_seed0.npz"))
    return np.concatenate([np.ascontiguousarray(z["chars"][:300, 1:5]).astype(np.int32),
                           np.array([[0, 0, 0, 0], [0, 0, 1, 1], [-5, -7, 2000, 3000], [7, 9, 7, 9], [100, 480, 120, 530],
                                     [-2**31, -2**31, 2**31 - 1, 2**31 - 1], [2**31 - 1, 0, 2**31 - 1, 5]], np.int32)])


def test_unproject_boxes_equal_the_restatement(lib):
    import ocrs_amd
    boxes = fixture_boxes()
    for m in maps():
        got = ocrs_amd.unproject_boxes(boxes, m)
        assert got.dtype == np.int32 and np.array_equal(got, P.unproject_boxes(boxes, m)), m.tolist()
        assert np.all(got[:, 0] <= got[:, 2]) and np.all(got[:, 1] <= got[:, 3]), "top <= bottom and left <= right are kept"
    assert np.array_equal(ocrs_amd.unproject_boxes(boxes, maps()[0]), boxes), "the identity"
    assert np.array_equal(ocrs_amd.unproject_boxes(boxes, maps()[6])[304], boxes[304]), "a box across the horizon passes through"
    # a box of the straightened page holds its corners: the photo's box holds the four mapped corners
    m = maps()[1].astype(np.float64)
    t, l, b, r = ocrs_amd.unproject_boxes([[10, 20, 30, 60]], maps()[1])[0].tolist()
    for x, y in ((20, 10), (60, 10), (20, 30), (60, 30)):
        dn = 1.0 + m[6] * (x + 0.5) + m[7] * (y + 0.5)
        X, Y = (m[0] + m[1] * (x + 0.5) + m[2] * (y + 0.5)) / dn, (m[3] + m[4] * (x + 0.5) + m[5] * (y + 0.5)) / dn
        assert l <= X <= r and t <= Y <= b


@pytest.mark.parametrize("name", list(QUADS))
def test_a_point_mapped_into_the_straightened_page_comes_back(lib, name):
    """A point P of the photo inside the quad has an exact position p on the straightened page under the map the library
    returned (its float32 coefficients taken as exact: the inverse homography, here in double).  unproject_rects(p) returns
    P but for: p given in float32 (each coordinate off by at most 2^-24 D, D = the larger output side; the map's Jacobian
    has entries of size at most s = max |J| over the page, so this moves P by at most 2 s 2^-24 D per axis), the result
    rounded to float32 (2^-24 |P|, |P| <= Q = the largest corner coordinate), and double rounding in between (smaller by
    2^-29).  The bound per axis: 2^-24 (2 s D + Q), widened by 1.01."""
    import ocrs_amd
    q = np.array(QUADS[name], np.float32)
    (oh, ow), m = ocrs_amd.quad_map(q)
    md = m.astype(np.float64)
    Hm = np.array([[md[1], md[2], md[0]], [md[4], md[5], md[3]], [md[6], md[7], 1.0]])
    inv = np.linalg.inv(Hm)
    rng = np.random.default_rng(5)
    uv = rng.random((200, 2)) * [ow, oh]
    uv[:4] = [[0.5, 0.5], [ow - 0.5, 0.5], [ow - 0.5, oh - 0.5], [0.5, oh - 0.5]]
    dn = 1.0 + md[6] * uv[:, 0] + md[7] * uv[:, 1]
    Pts = np.stack([(md[0] + md[1] * uv[:, 0] + md[2] * uv[:, 1]) / dn, (md[3] + md[4] * uv[:, 0] + md[5] * uv[:, 1]) / dn], axis=1)
    back_h = (inv @ np.concatenate([Pts, np.ones((200, 1))], axis=1).T).T
    p = back_h[:, :2] / back_h[:, 2:3]
    assert np.abs(p - uv).max() < 1e-8, "the inverse in double returns the point"
    rects = np.zeros((200, 6), np.float32)
    rects[:, 0], rects[:, 1], rects[:, 3], rects[:, 4], rects[:, 5] = p[:, 0] - 0.5, p[:, 1] - 0.5, -1.0, 10.0, 5.0
    back = ocrs_amd.unproject_rects(rects, m)
    X, Y = Pts[:, 0], Pts[:, 1]
    s = max(np.abs((md[1] - md[6] * X) / dn).max(), np.abs((md[2] - md[7] * X) / dn).max(), np.abs((md[4] - md[6] * Y) / dn).max(),
            np.abs((md[5] - md[7] * Y) / dn).max())
    bound = 1.01 * 2.0 ** -24 * (2.0 * s * max(oh, ow) + float(np.abs(q).max()))
    assert bound < 1e-3
    err = np.abs(back[:, :2].astype(np.float64) - Pts).max()
    assert err <= bound, (name, err, bound)
    assert np.all(back[:, 4:] > 0) and np.all(np.abs(np.hypot(back[:, 2], back[:, 3]) - 1.0) < 1e-6)


# ---------------------------------------------------------------- the restatement finds planted quads
DESKS = {"dark": -0.35, "grey": 0.1, "light": 0.3}


def outline_both(page, params=None):
    """The outline of a page by the restatement, and by the LIBRARY's choice (ocrs_outline_choose, host only) over the
    restatement's peaks of the same work copy: the two are held equal bit for bit here, on the realistic peaks of every
    photo, blank page and reference image below.  -> the restatement's dict."""
    import deskew_ref as D
    import ocrs_amd
    p = dict(P.default_params(), **(params or {}))
    page = np.ascontiguousarray(page, np.float32)
    work = D.work_page(page, p["work_max_side"])
    table = P.table_of(p)
    peaks = P.edge_peaks(work, table, int(p["min_step"]))
    ref = P.choose(peaks, table, work.shape, page.shape, p)
    assert info_tuple(ref) == info_tuple(P.find_outline(page, params)), "find_outline is these steps"
    got = ocrs_amd.outline_choose(peaks, table, work.shape, page.shape, **(params or {}))
    assert info_tuple(got) == info_tuple(ref), (got, ref)
    return ref


@functools.lru_cache(maxsize=None)
def planted(name, desk, dark_sheet):
    paper, ink = (-0.3, 0.45) if dark_sheet else (0.45, -0.4)
    photo = P.plant((400, 480), QUADS[name], P.sheet(400, 320, paper=paper, ink=ink, seed=1), desk=DESKS[desk], seed=2)
    return photo, outline_both(photo)


@pytest.mark.parametrize("desk", list(DESKS))
@pytest.mark.parametrize("name", list(QUADS))
def test_restatement_recovers_planted_corners(lib, name, desk):
    """Measured: 0.80 .. 1.35 pixels against bounds of 4.5 .. 4.8."""
    photo, o = planted(name, desk, False)
    assert o["found"] == 1 and o["polarity"] == 0, "a light sheet: `+` first"
    err = np.hypot(*(o["corners"].reshape(4, 2).astype(np.float64) - np.array(QUADS[name], np.float64).reshape(4, 2)).T).max()
    bound = P.corner_bound(QUADS[name], photo.shape)
    print("%s on a %s desk: corners within %.2f pixels (bound %.2f), counts %s, angles %s" % (name, desk, err, bound, o["counts"], o["angles"]))
    assert err <= bound and bound < 6.0, (name, desk, err, bound)
    assert min(o["counts"]) >= 120 and o["work_hw"] == (400, 480)


@pytest.mark.parametrize("name", list(QUADS))
def test_restatement_recovers_a_dark_sheet_on_a_light_desk(lib, name):
    photo, o = planted(name, "light", True)
    assert o["found"] == 1 and o["polarity"] == 1, "a dark sheet: `-` first"
    err = np.hypot(*(o["corners"].reshape(4, 2).astype(np.float64) - np.array(QUADS[name], np.float64).reshape(4, 2)).T).max()
    print("%s, a dark sheet: corners within %.2f pixels" % (name, err))
    assert err <= P.corner_bound(QUADS[name], photo.shape)
    # the negative of the light sheet's photo is found at the same corners, with the other polarity
    light = planted(name, "dark", False)
    neg = outline_both((-light[0]).astype(np.float32))
    assert neg["found"] == 1 and neg["polarity"] == 1
    assert np.abs(neg["corners"] - light[1]["corners"]).max() <= 2.0, "q(-v) is 255 - q(v) but for the bin's open end"


def test_restatement_on_a_larger_photo_works_on_a_copy(lib):
    quad = [v * 2.5 for v in QUADS["keystone"]]
    photo = P.plant((1000, 1200), quad, P.sheet(1000, 800, seed=1), desk=-0.35, seed=2)
    o = outline_both(photo)
    assert o["found"] == 1 and max(o["work_hw"]) == 512 and o["work_hw"] != photo.shape
    err = np.hypot(*(o["corners"].reshape(4, 2).astype(np.float64) - np.array(quad, np.float64).reshape(4, 2)).T).max()
    bound = P.corner_bound(quad, photo.shape)
    print("keystone at 1000 x 1200: corners within %.2f pixels (bound %.2f)" % (err, bound))
    assert err <= bound, (err, bound)


def test_restatement_finds_nothing_on_blank_pages(lib):
    for page in (np.zeros((50, 70), np.float32), np.full((50, 70), np.nan, np.float32), np.full((1, 1), 0.25, np.float32), P.sheet(300, 240)):
        o = outline_both(page)
        assert o["found"] == 0 and not o["corners"].any(), "a sheet that fills the photo has no outline in it"


@pytest.mark.parametrize("name", NAMES)
def test_report_what_the_restatement_finds_on_the_reference_images(lib, name):
    """Recorded, not asserted: these images show no desk.  On why-rust and polar-bears the text block's
    own edges are read as a sheet; on rust-book, a photograph of a book page, a quad inside the page."""
    sys.path.insert(0, ROOT)
    from oracle import pipeline as OP
    px = np.load(os.path.join(G, "reference", name + ".npz"))["pixels"]
    grey = OP.prepare_image(OP.ImageSource.from_tensor(px, "hwc"))
    o = outline_both(grey.reshape(grey.shape[-2], grey.shape[-1]))
    print("%s %s: found %d, polarity %d, corners %s, counts %s, angles %s, taken at %s"
          % (name, grey.shape[-2:], o["found"], o["polarity"], np.round(o["corners"], 1).tolist(), o["counts"], o["angles"], o["work_hw"]))
    assert o["found"] in (0, 1)


# ---------------------------------------------------------------- host memory safety
def fnv(chunks):
    h = 14695981039346656037
    for b in chunks:
        for x in b:
            h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_host_arithmetic_is_clean_under_asan_and_ubsan(lib, tmp_path):
    """tests/sanitize/perspective_harness.cpp, a stand-alone program over perspective_math.hpp, on this file's cases and on
    hostile inputs; what it computes hashes like what the library returns."""
    import ocrs_amd
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "perspective_harness")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", os.path.join(HERE, "sanitize", "perspective_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, "building the sanitizer harness failed:\n" + r.stderr[-3000:]
    cases, qs, ms, rects, boxes = hand_made_cases(), quads(), maps(), hand_made_rects(), fixture_boxes()[250:]
    rects = np.concatenate([rects, np.asarray(np.load(FIXTURES[0])["word_rects"], np.float32).reshape(-1, 6)[:50]])
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for _, pk, table, work_hw, page_hw, params, _ in cases:
            p = dict(P.default_params(), **params)
            f.write(np.uint32(len(table)).tobytes() + np.array([work_hw[0], work_hw[1], page_hw[0], page_hw[1]], np.int32).tobytes())
            f.write(np.array([p["max_deg"], p["step_deg"], p["min_cover"], p["min_span"], p["min_area"]], np.float64).tobytes())
            f.write(np.array([p["work_max_side"], p["min_step"]], np.int32).tobytes())
            f.write(np.ascontiguousarray(table, np.int32).tobytes() + np.ascontiguousarray(pk, np.uint64).tobytes())
        f.write(np.uint32(len(qs)).tobytes() + np.concatenate(qs).astype(np.float32).tobytes())
        f.write(np.uint32(len(ms)).tobytes() + np.concatenate(ms).astype(np.float32).tobytes())
        f.write(np.uint32(len(rects)).tobytes() + rects.tobytes())
        f.write(np.uint32(len(boxes)).tobytes() + np.ascontiguousarray(boxes, np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert not any(m in out for m in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")), out[-6000:]
    assert r.returncode == 0 and "hostile: ok" in r.stdout, out[-3000:]
    got = dict(l.split(": ") for l in r.stdout.splitlines() if ": " in l)
    # the same through the product library
    chunks = []
    for _, pk, table, work_hw, page_hw, params, _ in cases:
        o = ocrs_amd.outline_choose(pk, table, work_hw, page_hw, **params)
        chunks += [np.array([int(o.found), o.polarity], np.int32).tobytes(), o.corners.tobytes(), np.array(o.counts, np.uint32).tobytes(),
                   np.array(o.angles, np.int32).tobytes()]
    assert got["choose"] == fnv(chunks)
    chunks = []
    for q in qs:
        made = lib_quad_map(q)
        chunks += [np.array([0 if made is None else 1] + ([0, 0] if made is None else list(made[0])), np.int32).tobytes(),
                   (np.zeros(8, np.float32) if made is None else made[1]).tobytes()]
    assert got["quad"] == fnv(chunks)
    assert got["rects"] == fnv([ocrs_amd.unproject_rects(rects, m).tobytes() for m in ms])
    assert got["boxes"] == fnv([ocrs_amd.unproject_boxes(boxes, m).tobytes() for m in ms])
