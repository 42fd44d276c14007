"""Despeckling, host side: the new symbols and parameter checks of the library, and the properties the
definition in tests/despeckle_ref.py promises, on hand-made pages and on the noisy text page through the oracle's
detector.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import despeckle_pages as P
import despeckle_ref as D
import models_util as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ["ocrs_speckle_params_default", "ocrs_speckle_params_check", "ocrs_engine_despeckle_page", "ocrs_engine_despeckle_pages"]
F = np.float32
H, W = 129, 127   # the hand-made pages: three tile rows and two words, both with a partial edge


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
    for name in ("ocrs_speckle_params", "ocrs_speckle_info"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert C.sizeof(_lib.SpeckleParams) == 24 and C.sizeof(_lib.SpeckleInfo) == 80
    assert [f[0] for f in _lib.SpeckleInfo._fields_] == list(D.INFO_KEYS)


def test_sources_are_built():
    from ocrs_amd import build
    assert "kernels_speckle.hip" in build.SOURCES and "speckle.cpp" in build.SOURCES
    for name in ("kernels_speckle.hip", "speckle.cpp"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name


def test_default_params_and_refused_params(lib):
    import ocrs_amd
    from ocrs_amd import _lib
    p = _lib.SpeckleParams(1.0, 1, 1, 7, 1.0, 1.0)
    assert lib.ocrs_speckle_params_default(C.byref(p)) == 0
    assert (p.threshold, p.max_area, p.max_hole, p.keep_near) == (0.0, 4, 0, 0) and p.paper != p.paper and p.ink_level != p.ink_level
    assert ocrs_amd.speckle_params() == D.default_params() == {"threshold": 0.0, "max_area": 4, "max_hole": 0, "keep_near": 0, "paper": None,
                                                               "ink_level": None}
    assert lib.ocrs_speckle_params_default(None) == 1 and lib.ocrs_speckle_params_check(None) == 1
    for kw in ({"max_area": 0}, {"max_area": 4096}, {"max_hole": 0}, {"max_hole": 4096}, {"keep_near": 0}, {"keep_near": 16},
               {"max_area": 0, "max_hole": 0}, {"threshold": -0.25}, {"threshold": 2.0 ** 100}, {"paper": 0.5}, {"paper": -0.0},
               {"paper": float("nan")}, {"ink_level": -0.5}, {"ink_level": float("nan")},
               {"max_area": 9, "max_hole": 3, "keep_near": 2, "threshold": 0.125, "paper": 0.25, "ink_level": -0.25}):
        assert D.valid_params(**kw), kw
        exp = dict(D.default_params(), **kw)
        for k in ("paper", "ink_level"):
            if exp[k] is not None and exp[k] != exp[k]:
                exp[k] = None   # NaN: measured
        assert ocrs_amd.speckle_params(**kw) == exp, kw
    for kw in ({"max_area": -1}, {"max_area": 4097}, {"max_area": 1 << 30}, {"max_hole": -1}, {"max_hole": 4097}, {"keep_near": -1},
               {"keep_near": 17}, {"threshold": float("nan")}, {"threshold": float("inf")}, {"threshold": float("-inf")},
               {"paper": float("inf")}, {"paper": float("-inf")}, {"ink_level": float("inf")}, {"ink_level": float("-inf")}):
        assert not D.valid_params(**kw), kw
        with pytest.raises(ocrs_amd.OcrsError) as e:
            ocrs_amd.speckle_params(**kw)
        assert e.value.status_name == "INVALID_ARGUMENT", kw
        with pytest.raises(ValueError):
            D.despeckle(np.zeros((4, 4), F), **kw)


# ---------------------------------------------------------------- the restatement against scipy
def scipy_despeckle(v, A, Hm, K, threshold=0.0):
    """(speck, hole, kept) by scipy.ndimage: label with the 8- and the 4-structure, binary_dilation with a box."""
    ndi = pytest.importorskip("scipy.ndimage")
    with np.errstate(invalid="ignore"):
        ink = v < F(threshold)
    l8, _ = ndi.label(ink, np.ones((3, 3), int))
    small = np.bincount(l8.ravel()) <= A
    small[0] = False
    cand = small[l8]
    big = ink & ~cand
    kept = np.zeros_like(ink)
    if K > 0 and big.any():
        near = ndi.binary_dilation(big, np.ones((2 * K + 1, 2 * K + 1), bool))
        kept_labels = np.unique(l8[cand & near])
        kept = np.isin(l8, kept_labels) & cand
    l4, _ = ndi.label(~ink)
    psmall = np.bincount(l4.ravel()) <= Hm
    psmall[0] = False
    return cand & ~kept, psmall[l4], kept


@pytest.mark.parametrize("density", [0.05, 0.3, 0.5, 0.7, 0.95])
def test_restatement_equals_scipy_on_noise(density):
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 100))
    v = (rng.random((97, 211), dtype=F) - F(density)).astype(F)
    v.reshape(-1)[rng.choice(v.size, 12, replace=False)] = np.nan
    a = D.analyse(v)
    assert abs(a["ink"].mean() - density) < 0.02
    n8, n4 = len(a["ink_cc"][1]) - 1, len(a["paper_cc"][1]) - 1
    print("density %g: %d ink components (largest %d), %d paper components (largest %d)" % (
        density, n8, a["ink_cc"][1].max(), n4, a["paper_cc"][1].max()))
    if density == 0.5:   # the 8-connected ink percolates, the 4-connected paper shatters
        assert a["ink_cc"][1].max() > 0.8 * a["ink"].sum() and n4 > 1000 and a["paper_cc"][1].max() < 0.2 * (~a["ink"]).sum()
    for A, Hm, K in ((0, 0, 0), (1, 1, 1), (2, 3, 0), (5, 2, 3), (30, 30, 16), (4096, 4096, 2)):
        out, mask, info = D.despeckle(v, max_area=A, max_hole=Hm, keep_near=K, analysis=a)
        speck, hole, kept = scipy_despeckle(v, A, Hm, K)
        assert np.array_equal(mask & 1 != 0, speck) and np.array_equal(mask & 2 != 0, hole) and np.array_equal(mask & 4 != 0, kept), (A, Hm, K)
        assert info["speck_pixels"] == speck.sum() and info["hole_pixels"] == hole.sum() and info["kept_pixels"] == kept.sum()


# ---------------------------------------------------------------- the restatement on hand-made pages
@pytest.mark.parametrize("A", [1, 2, 4, 9])
def test_planted_components_around_the_maximum_area(A):
    for area in (A, A + 1):
        page = P.planted_blobs(H, W, area)
        sites = P.blob_sites(H, W, area)
        assert len(sites) == 7 and (page < 0).sum() == 7 * area, "corners, across x = 63|64, across y = 63|64, across both"
        out, mask, info = D.despeckle(page, max_area=A)
        if area <= A:
            assert info["specks"] == 7 and info["speck_pixels"] == 7 * area and np.array_equal(mask == 1, page < 0)
            assert np.all(out[mask == 0] == P.PAPER) and np.all(out[mask == 1] == P.PAPER_FILL)
            assert not (out < 0).any()
        else:
            assert info["specks"] == 0 and not mask.any() and out.tobytes() == page.tobytes(), "one pixel more: not a speck"
        # the same shapes as holes in ink
        inv = np.where(page < 0, P.PAPER, P.INK).astype(F)
        out, mask, info = D.despeckle(inv, max_area=0, max_hole=A)
        assert info["holes"] == (7 if area <= A else 0) and info["hole_pixels"] == info["holes"] * area   # rows of three are 4-connected, too
        assert np.all(out[mask == 2] == P.INK_FILL) and np.all(out[mask == 0] == inv[mask == 0])


def test_ink_touching_by_a_corner_is_one_component_and_paper_is_two():
    a, b = P.corner_pairs(H, W)
    out, mask, info = D.despeckle(a, max_area=1)
    assert info["specks"] == 0 and out.tobytes() == a.tobytes(), "8-connected: a component of two, kept at A = 1"
    out, mask, info = D.despeckle(a, max_area=2)
    assert info["specks"] == 2 and info["speck_pixels"] == 4 and not (out < 0).any(), "removed at A = 2"
    out, mask, info = D.despeckle(b, max_area=0, max_hole=1)
    assert info["holes"] == 4 and info["hole_pixels"] == 4 and not (out >= 0).any(), "4-connected: two holes of one pixel each, twice"


def test_stress_patterns():
    n = H * W
    out, mask, info = D.despeckle(P.checkerboard(H, W), max_area=4096, max_hole=1)
    assert info["specks"] == 0 and info["holes"] == n // 2 == info["hole_pixels"], "one component of ink, every paper pixel a hole"
    assert not (out >= 0).any()
    out, mask, info = D.despeckle(P.diagonals(H, W), max_area=50, max_hole=0)
    assert info["specks"] == sum(1 for k in range(-(H - 1), W, 4) if min(W, H + k) - max(0, k) <= 50), "a diagonal is one component"
    for inv in (False, True):
        for page in (P.serpentine(H, W, inv), P.spiral(H, W, inv)):
            line = (page >= 0) if inv else (page < 0)
            lab, area = D.components(line, not inv)
            assert len(area) == 2 and area[1] == line.sum() > n // 3, "one line through the whole page is one component"
            out, mask, info = D.despeckle(page, max_area=4096, max_hole=4096)
            assert (info["holes"] if inv else info["specks"]) == 0
    u = P.u_shape(H, W)
    lab, area = D.components(u < 0, True)
    assert len(area) == 3, "the arms of either U meet only at one end"
    assert lab[0, 3] == lab[0, W // 2] == 1 and lab[0, W // 2 + 3] == lab[H - 3, W - 2] == 2
    assert area.min(initial=H * W, where=area > 0) > 300 and D.despeckle(u, max_area=200)[2]["specks"] == 0, "an arm alone would be a speck at 200"


@pytest.mark.parametrize("K", [1, 2, 8, 16])
def test_keep_near_at_exact_distances(K):
    for kind in P.NEAR_KINDS:
        for d in (K, K + 1):
            if kind == "pair" and d < 2:
                continue
            page, specks = P.near_case(H, W, kind, d)
            ys, xs = np.nonzero(page < 0)
            block = [(y, x) for y, x in zip(ys, xs) if (y, x) not in specks]
            for y, x in specks if kind != "pair" else []:   # the distance is what the name says
                assert min(max(abs(y - by), abs(x - bx)) for by, bx in block) == d, (kind, d)
            out, mask, info = D.despeckle(page, max_area=1, keep_near=K)
            if kind == "pair":
                assert info["specks"] == 2 and info["kept"] == 0, "candidates do not protect each other"
            elif d == 1:
                assert info["specks"] == 0 and info["kept"] == 0, "a speck that touches big ink is part of it"
            elif d <= K:
                assert info["kept"] == len(specks) and info["specks"] == 0 and all(mask[y, x] == 4 for y, x in specks), (kind, d)
                assert out.tobytes() == page.tobytes()
            else:
                assert info["specks"] == len(specks) and info["kept"] == 0 and all(mask[y, x] == 1 for y, x in specks), (kind, d)
            assert D.despeckle(page, max_area=1, keep_near=0)[2]["kept"] == 0


def test_degenerate_pages_go_through():
    with np.errstate(all="raise"):   # no invalid operation on a number, no overflow
        for shape in ((70, 130), (5, 200), (1, 1)):
            n = shape[0] * shape[1]
            for kw in ({}, {"max_area": 4096, "max_hole": 4096, "keep_near": 16}):
                whole, speck = int(n <= kw.get("max_hole", 0)), int(n <= kw.get("max_area", 4))   # the whole page is one small component
                out, mask, info = D.despeckle(np.full(shape, 0.4, F), **kw)
                assert info == {"paper_bin": 230, "ink_bin": 0, "paper_fill": float(P.PAPER_FILL), "ink_fill": -0.5, "ink": 0, "counted": n,
                                "specks": 0, "kept": 0, "speck_pixels": 0, "kept_pixels": 0, "holes": whole, "hole_pixels": whole * n}
                out, mask, info = D.despeckle(np.full(shape, -0.5, F), **kw)
                assert info["paper_bin"] == 255 and info["paper_fill"] == 0.5 and info["ink"] == n and info["counted"] == 0
                assert info["specks"] == speck and np.all(out == (0.5 if speck else -0.5))
                out, mask, info = D.despeckle(np.full(shape, np.nan, F), **kw)
                assert info["ink"] == 0 and info["counted"] == 0 and (info["paper_bin"], info["ink_bin"]) == (255, 0)
                assert info["holes"] == whole and (np.all(out == -0.5) if whole else np.isnan(out).all())


def test_every_pixel_outside_speck_and_hole_keeps_its_planted_bits():
    rng = np.random.default_rng(8)
    page = (rng.random((97, 211), dtype=F) - F(0.4)).astype(F)
    words = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x40400000, 0xC0400000, 0x7F7FFFFF,
                      0xFF7FFFFF, 0x00000001, 0x80000001], np.uint32)
    flat = page.reshape(-1).view(np.uint32)
    flat[rng.choice(flat.size, size=20 * len(words), replace=False)] = np.tile(words, 20)
    for kw in ({"max_area": 3, "max_hole": 2, "keep_near": 1}, {"max_area": 8, "max_hole": 8, "paper": -0.0, "ink_level": 0.25}):
        out, mask, info = D.despeckle(page, **kw)
        speck, hole = (mask & 1) != 0, (mask & 2) != 0
        gone = speck | hole
        assert 0 < info["speck_pixels"] == int(speck.sum()) and 0 < info["hole_pixels"] == int(hole.sum()) and not (speck & hole).any()
        assert np.array_equal(out.view(np.uint32)[~gone], page.view(np.uint32)[~gone]), "NaN payloads, -0.0 and infinities survive"
        assert np.all(out.view(np.uint32)[speck] == np.array([info["paper_fill"]], F).view(np.uint32)[0])
        assert np.all(out.view(np.uint32)[hole] == np.array([info["ink_fill"]], F).view(np.uint32)[0])
        with np.errstate(invalid="ignore"):
            assert np.all(page[speck] < 0) and not np.any(page[hole] < 0), "specks are ink, holes are not (NaN included)"


def test_fills_given_against_fills_measured():
    page = P.planted_blobs(H, W, 2)
    page[40:50, 40:50] = P.INK
    page[44, 44] = P.PAPER
    measured, mask_m, info_m = D.despeckle(page, max_area=2, max_hole=1)
    assert (info_m["paper_bin"], info_m["ink_bin"]) == (230, 25) and (F(info_m["paper_fill"]), F(info_m["ink_fill"])) == (P.PAPER_FILL, P.INK_FILL)
    assert info_m["specks"] == 7 and info_m["holes"] == 1 and measured[44, 44] == P.INK_FILL
    given, mask_g, info_g = D.despeckle(page, max_area=2, max_hole=1, paper=0.25, ink_level=-0.125)
    assert (info_g["paper_bin"], info_g["ink_bin"], info_g["paper_fill"], info_g["ink_fill"]) == (-1, -1, 0.25, -0.125)
    skip = ("paper_bin", "ink_bin", "paper_fill", "ink_fill")
    assert {k: v for k, v in info_g.items() if k not in skip} == {k: v for k, v in info_m.items() if k not in skip}, "the counts are still made"
    assert np.array_equal(mask_g, mask_m) and np.all(given[mask_m == 1] == F(0.25)) and np.all(given[mask_m == 2] == F(-0.125))
    assert np.array_equal(measured[mask_m == 0], given[mask_m == 0])
    nan = D.despeckle(page, max_area=2, max_hole=1, paper=float("nan"), ink_level=float("nan"))
    assert nan[2] == info_m and nan[0].tobytes() == measured.tobytes(), "NaN: measured"
    half = D.despeckle(page, max_area=2, max_hole=1, paper=0.25)[2]
    assert (half["paper_bin"], half["ink_bin"]) == (-1, 25)


# ---------------------------------------------------------------- the noisy text page through the oracle's detector
@pytest.fixture(scope="module")
def text_page():
    """The 512 x 512 page of DESIGN.md §7.9: the oracle's engine, the clean page, the page with 0.2 % pepper and 0.2 % salt."""
    from ocrs_amd import synth
    from oracle import pipeline as OP
    from oracle.nn import OracleGraph, OracleModel
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                       recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))
    px = synth.synthetic_page(3, 512, 512, 30, 2, 1)
    clean = np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), F)[0])
    return ora, clean, D.add_noise(clean, 0.002)[0]


def test_the_clean_page_is_unaltered_by_the_defaults(text_page):
    _, clean, _ = text_page
    out, mask, info = D.despeckle(clean)
    assert info["specks"] == 0 and info["holes"] == 0 and not mask.any()
    assert out.view(np.uint32).tobytes() == clean.view(np.uint32).tobytes()


def test_the_noisy_page(text_page):
    ora, clean, noisy = text_page
    out, mask, info = D.despeckle(noisy)
    before, left, lost, word_ink = D.noise_counts(clean, noisy, out)
    print("noisy page: %s; stray ink %d -> %d, word ink lost %d of %d" % (info, before, left, lost, word_ink))
    assert lost == 0, "no word ink is lost"
    assert before > 0 and left * 100 <= 15 * before, "stray ink left is at most 15 % of the stray ink before"

    def boxes(page):
        return {np.array(w.to_array(), F).tobytes() for w in ora.detect_words(page[None])}

    want, on_noisy, on_cleaned = boxes(clean), boxes(noisy), boxes(out)
    print("noisy page: %d words on the clean page; reproduced exactly: %d on the noisy page, %d on the cleaned page"
          % (len(want), len(want & on_noisy), len(want & on_cleaned)))
