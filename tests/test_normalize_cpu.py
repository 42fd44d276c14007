"""Page normalisation, host side: the new symbols and parameter checks of the library, and the properties
the definition in tests/normalize_ref.py promises, on hand-made pages and on the three pages of tests/golden/reference
with one detection file for all of them.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import models_util as M
import normalize_ref as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = os.path.join(HERE, "golden", "reference")
NEW_SYMBOLS = ["ocrs_normalize_params_default", "ocrs_normalize_params_check", "ocrs_engine_normalize_page",
               "ocrs_engine_normalize_pages"]
PAGES = ("polar-bears", "why-rust", "rust-book")
DARK = {"polar-bears": 0, "why-rust": 1, "rust-book": 0}
ONE_FILE_INK = (0.3, 1.0, 1)   # the operating point of dark text on a light page: polar-bears' own


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
    for name in ("ocrs_normalize_params", "ocrs_normalize_info"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert [_lib.POLARITIES[k] for k in ("auto", "keep", "invert")] == \
        [int(re.search(r"OCRS_POLARITY_%s = (\d)" % k.upper(), hdr).group(1)) for k in ("auto", "keep", "invert")]
    assert C.sizeof(_lib.NormalizeParams) == 16 and C.sizeof(_lib.NormalizeInfo) == 32


def test_default_params_and_refused_params(lib):
    import ocrs_amd
    from ocrs_amd import _lib
    p = _lib.NormalizeParams(1, 1, 0, 0)
    assert lib.ocrs_normalize_params_default(C.byref(p)) == 0
    assert (p.tile, p.polarity, p.flatten, p.levels) == (64, 0, 1, 1)
    assert ocrs_amd.normalize_params() == N.default_params() == {"tile": 64, "polarity": "auto", "flatten": True, "levels": True}
    assert lib.ocrs_normalize_params_default(None) == 1 and lib.ocrs_normalize_params_check(None) == 1
    for tile in (16, 32, 64, 128, 256):
        assert N.valid_tile(tile)
        for pol in N.POLARITIES:
            got = ocrs_amd.normalize_params(tile=tile, polarity=pol, flatten=False, levels=False)
            assert got == {"tile": tile, "polarity": pol, "flatten": False, "levels": False}
    for tile in (0, 1, 8, 15, 17, 48, 63, 65, 96, 255, 257, 512, -64, 1 << 30):
        assert not N.valid_tile(tile)
        with pytest.raises(ocrs_amd.OcrsError) as e:
            ocrs_amd.normalize_params(tile=tile)
        assert e.value.status_name == "INVALID_ARGUMENT", tile
    for pol in (-1, 3, 7):
        assert lib.ocrs_normalize_params_check(C.byref(_lib.NormalizeParams(64, pol, 1, 1))) == 1
    with pytest.raises(ValueError):
        ocrs_amd.normalize_params(polarity="negative")


# ---------------------------------------------------------------- hand-made pages
def noise(seed, h, w):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def test_pct_is_the_smallest_bin_that_reaches_the_share():
    h = np.zeros(256, np.int64)
    assert N.pct(h, 1, 2) == -1 and N.pct_many(h[None], 1, 2).tolist() == [-1]
    h[10], h[20], h[200] = 5, 90, 5
    assert [N.pct(h, *f) for f in ((1, 20), (1, 2), (19, 20), (3, 4), (1, 100))] == [10, 20, 20, 20, 10]
    h[10] = 4    # 4 of 99 is under a twentieth
    assert N.pct(h, 1, 20) == 20 and N.pct(h, 1, 100) == 10
    rng = np.random.default_rng(1)
    many = rng.integers(0, 50, size=(40, 256)) * (rng.random((40, 256)) < 0.1)
    for num, den in ((1, 20), (1, 2), (3, 4), (19, 20), (1, 100)):
        assert N.pct_many(many, num, den).tolist() == [N.pct(row, num, den) for row in many]


@pytest.mark.parametrize("tile", [16, 64, 256])
def test_result_lies_in_range_and_only_nan_stays_nan(tile):
    for seed, (h, w) in enumerate(((1, 1), (63, 65), (97, 211), (300, 1))):
        page = noise(seed, h, w) * np.float32(1.5)    # a third of it outside [-0.5, 0.5]
        flat = page.reshape(-1)
        plant = np.array([np.nan, np.inf, -np.inf, -0.0, 3.0, -3.0], np.float32)[:max(1, flat.size // 8)]
        flat[np.random.default_rng(seed).choice(flat.size, len(plant), replace=False)] = plant
        for pol in N.POLARITIES:
            for flatten, levels in ((True, True), (True, False), (False, True)):
                out, info = N.normalize(page, tile, pol, flatten, levels)
                assert out.dtype == np.float32 and out.shape == page.shape
                assert np.array_equal(np.isnan(out), np.isnan(page)), "NaN stays NaN, and only NaN does"
                keep = ~np.isnan(out)
                assert np.all(out[keep] >= np.float32(-0.5)) and np.all(out[keep] <= np.float32(0.5)), (h, w, pol, flatten, levels)
                assert info["counted"] == int(keep.sum())
            out, info = N.normalize(page, tile, pol, False, False)   # neither: the page's own words
            flip = np.uint32(0x80000000) if info["dark"] else np.uint32(0)
            assert np.array_equal(out.view(np.uint32), page.view(np.uint32) ^ flip)


def test_constant_and_all_nan_pages_go_through():
    with np.errstate(all="raise"):   # no division by zero, no invalid operation on a number
        for c in (-0.5, 0.0, 0.25, 0.5):
            page = np.full((70, 130), c, np.float32)
            for pol in N.POLARITIES:
                out, info = N.normalize(page, 64, pol)
                assert info["hi"] <= info["lo"], "one value: no levels to stretch"
                assert info["counted"] == page.size and (info["vote"] == 0)
                g = (0.5 - c) if info["dark"] else (c + 0.5)
                # the page is its own background: u = g / (upper edge of its bin), within a bin's width of white; on a dark
                # page the bin is the mirror of the bin of c + 0.5
                b = min(int((c + 0.5) * 256), 255)
                b = 255 - b if info["dark"] else b
                assert info["white"] == b
                exp = np.float32(min(np.float32(g) / np.float32((b + 1) / 256.0), 1.0)) - np.float32(0.5)
                assert np.all(out == exp) and (g == 0 or exp > 0.49), (c, pol, out[0, 0], exp)
    page = np.full((70, 130), np.nan, np.float32)
    out, info = N.normalize(page)
    assert np.isnan(out).all()
    assert info == {"dark": 0, "vote": 0, "white": -1, "lo": -1, "hi": -1, "counted": 0}


def test_a_dark_figure_is_not_blown_up_and_a_heading_is_not_background():
    page = np.full((320, 320), 0.4, np.float32)
    page[128:192, 128:192] = -0.45            # a tile that is all figure: floored at Wg // 2 and lifted by its neighbours
    page[0:64, 0:64] = -0.4                   # a tile that a heading fills but for every eighth row: its own white bin is
    page[0:64:8, 0:64] = 0.4                  # the ink's, its neighbours' paper is its background
    out, info = N.normalize(page, 64, "keep", True, False)
    assert info["dark"] == 0 and info["white"] == int((0.4 + 0.5) * 256)
    assert out[160, 160] < -0.4, "the figure stays dark"
    assert out[1, 10] < -0.35 and out[0, 10] > 0.45, "the heading stays ink on paper"


# ---------------------------------------------------------------- the three real pages, one operating point
class RealPages:
    def __init__(self):
        from oracle import pipeline as OP
        from oracle.nn import OracleGraph, OracleModel
        dbuf, rbuf = M.detection_model_bytes(ink=ONE_FILE_INK), M.recognition_model_bytes()
        self.ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(dbuf), "exact"),
                                recognition_model=OracleModel(OracleGraph(rbuf), "exact"))
        self.page, self.words, self.norm, self.info, self.shaded, self.shaded_norm, self.shaded_info = {}, {}, {}, {}, {}, {}, {}
        for name in PAGES:
            z = np.load(os.path.join(G, name + ".npz"))
            inp = self.ora.prepare_input(OP.ImageSource.from_tensor(z["pixels"], "hwc"))
            self.page[name] = np.ascontiguousarray(np.asarray(inp, np.float32)[0])
            self.words[name] = len(z["word_rects"])
            self.norm[name], self.info[name] = N.normalize(self.page[name])
            self.shaded[name] = N.shade(self.page[name])
            self.shaded_norm[name], self.shaded_info[name] = N.normalize(self.shaded[name])

    def count(self, page):
        return len(self.ora.detect_words(page[None]))


@pytest.fixture(scope="module")
def real():
    return RealPages()


@pytest.mark.parametrize("name", PAGES)
def test_polarity_of_the_real_pages_with_and_without_a_shadow(real, name):
    print(name, real.info[name], "shaded:", real.shaded_info[name])
    assert real.info[name]["dark"] == DARK[name]
    assert real.shaded_info[name]["dark"] == DARK[name], "the shadow does not flip the page"
    assert (real.info[name]["vote"] > 0) == bool(DARK[name])


@pytest.mark.parametrize("name", PAGES)
def test_the_negated_page_normalises_to_the_same_bits(real, name):
    out, info = N.normalize(-real.page[name])
    assert info["dark"] == 1 - DARK[name] and (info["vote"] > 0) != (real.info[name]["vote"] > 0)
    assert np.array_equal(out.view(np.uint32), real.norm[name].view(np.uint32))


@pytest.mark.parametrize("name", PAGES)
def test_a_shadow_shrinks_by_more_than_four(real, name):
    before = float(np.abs(real.shaded[name].astype(np.float64) - real.page[name]).mean())
    after = float(np.abs(real.shaded_norm[name].astype(np.float64) - real.norm[name]).mean())
    print("%s: mean |shaded - clean| %.4f before, %.4f after normalisation (%.1f x)" % (name, before, after, before / after))
    assert after < before / 4


@pytest.mark.parametrize("name", PAGES)
def test_one_detection_file_reads_every_normalised_page(real, name):
    found = real.count(real.norm[name])
    print("%s: %d words on the normalised page, %d in the fixture of its own hand-tuned file" % (name, found, real.words[name]))
    assert 2 * found >= real.words[name]


def test_the_same_file_reads_nothing_on_the_raw_dark_page(real):
    found = real.count(real.page["why-rust"])
    print("why-rust as given: %d words" % found)
    assert found <= 5
