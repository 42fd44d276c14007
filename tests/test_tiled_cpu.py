"""Tiled detection, host side: the new entry points are exported and declared, the plan the engine uses
(ocrs_detection_tile_plan) equals the numpy statement of the definition (tiled_ref.py) over a brute-force sweep and has the
properties the definition promises, and the reference's own stitching is an identity under an identity model.  No GPU is
used here.

Run with:  python -m pytest tests -m "not gpu"
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tiled_ref as TR
from ocrs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ocrs_detection_tile_plan", "ocrs_engine_detect_words_tiled", "ocrs_engine_detect_words_batch_tiled",
               "ocrs_engine_detect_text_pixels_tiled", "ocrs_group_detect_words_batch_tiled"]


@pytest.fixture(scope="module")
def lib():
    from ocrs_amd import build
    build.build()
    return _lib.lib()


def test_new_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "ocrs_amd.h")).read()
    declared = set(re.findall(r"OCRS_API[^;(]*?\b(ocrs_\w+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+OCRS_ABI_VERSION\s+6u", hdr)   # no struct or existing argument list changed
    lib.ocrs_abi_version.restype = C.c_uint32
    assert lib.ocrs_abi_version() == 6
    assert re.search(r"#define\s+OCRS_TILE_OVERLAP_DEFAULT\s+100\b", hdr) and _lib.TILE_OVERLAP_DEFAULT == TR.OVERLAP_DEFAULT == 100


class Planner:
    """ocrs_detection_tile_plan with its out-arguments allocated once."""

    def __init__(self, lib):
        self.lib = lib
        self.ny, self.nx = C.c_size_t(0), C.c_size_t(0)
        self.p = [C.POINTER(C.c_int32)() for _ in range(4)]
        self.refs = [C.byref(self.ny), C.byref(self.nx)] + [C.byref(x) for x in self.p]

    def status(self, page_hw, model_hw, v):
        return self.lib.ocrs_detection_tile_plan(page_hw[0], page_hw[1], model_hw[0], model_hw[1], v, *self.refs)

    def __call__(self, page_hw, model_hw, v):
        """-> (origin_y, bound_y, origin_x, bound_x) as lists."""
        s = self.status(page_hw, model_hw, v)
        assert s == 0, (page_hw, model_hw, v, self.lib.ocrs_last_error())
        ny, nx = self.ny.value, self.nx.value
        out = (self.p[0][:ny], self.p[1][:ny + 1], self.p[2][:nx], self.p[3][:nx + 1])
        for x in self.p:
            self.lib.ocrs_buffer_free(x)
        return out


def sweep_lengths(M):
    return list(range(1, 4 * M + 50)) + [65535]


# Both axes of one call carry a case each, so that the sweep takes half the calls: (model rows, model columns, overlaps).
# An overlap is bounded by the SHORTER model side, so the longer side's overlaps beyond that run against a square model.
SWEEP = [(800, 600, range(0, 301)), (800, 800, range(301, 401)), (64, 33, range(0, 17)), (64, 64, range(17, 33))]


@pytest.mark.parametrize("mh,mw,overlaps", SWEEP, ids=["800x600", "800 v>300", "64x33", "64 v>16"])
def test_plan_equals_the_definition_over_the_sweep(lib, mh, mw, overlaps):
    """Every L in 1 .. 4M + 49 and L = 65535, M in {600, 800, 64, 33}, every v in 0 .. M // 2: the library's plan is the
    definition's, and the definition's plan has the promised properties."""
    plan = Planner(lib)
    ly, lx = sweep_lengths(mh), sweep_lengths(mw)
    n = 0
    for v in overlaps:
        ref_y = {L: TR.axis_plan(L, mh, v) for L in ly}
        ref_x = ref_y if mw == mh else {L: TR.axis_plan(L, mw, v) for L in lx}
        for L, (o, b) in ref_y.items():
            TR.check_axis_properties(L, mh, v, o, b)
        if ref_x is not ref_y:
            for L, (o, b) in ref_x.items():
                TR.check_axis_properties(L, mw, v, o, b)
        for k in range(max(len(ly), len(lx))):
            Ly, Lx = ly[min(k, len(ly) - 1)], lx[min(k, len(lx) - 1)]
            oy, by, ox, bx = plan((Ly, Lx), (mh, mw), v)
            assert (oy, by) == ref_y[Ly], (Ly, mh, v)
            assert (ox, bx) == ref_x[Lx], (Lx, mw, v)
            n += 1
    print("%d plans" % n)


def test_worked_examples_default_and_errors(lib):
    plan = Planner(lib)
    oy, by, ox, bx = plan((3508, 2480), (800, 600), 100)
    assert oy == [0, 677, 1354, 2031, 2708] and by == [0, 738, 1415, 2092, 2769, 3508]
    assert ox == [0, 470, 940, 1410, 1880] and bx == [0, 535, 1005, 1475, 1945, 2480]
    oy, by, ox, bx = plan((1024, 1024), (800, 600), 100)
    assert oy == [0, 224] and by == [0, 512, 1024]
    assert plan((3508, 2480), (800, 600), -1) == plan((3508, 2480), (800, 600), 100)   # negative: the default
    assert plan((1400, 1100), (800, 600), -7) == plan((1400, 1100), (800, 600), 100)
    assert plan((600, 800), (800, 600), 100) == ([0], [0, 600], [0, 200], [0, 400, 800])
    # the Python wrapper
    from ocrs_amd import tile_plan
    got = tile_plan((3508, 2480), (800, 600))
    assert [a.dtype for a in got] == [np.int32] * 4
    assert [a.tolist() for a in got] == [list(x) for x in plan((3508, 2480), (800, 600), 100)]
    assert [a.tolist() for a in tile_plan((100, 300), (64, 48), 0)] == [list(x) for x in TR.page_plan((100, 300), (64, 48), 0)]
    # errors: an overlap beyond half the shorter model side, page sides <= 0
    assert plan.status((1000, 1000), (800, 600), 300) == 0
    for x in plan.p:
        lib.ocrs_buffer_free(x)
    assert plan.status((1000, 1000), (800, 600), 600 // 2 + 1) == 1 and b"overlap" in lib.ocrs_last_error()
    assert plan.status((1000, 1000), (64, 48), -1) == 1, "the default overlap does not fit a 64 x 48 model"
    for hw in ((0, 100), (100, 0), (-5, 100), (100, -1)):
        assert plan.status(hw, (800, 600), 100) == 1, hw
    assert plan.status((100, 100), (0, 600), 0) == 1


@pytest.mark.parametrize("model_hw", [(600, 800), (64, 48), (33, 47)], ids=["600x800", "64x48", "33x47"])
def test_reference_stitching_is_the_identity_under_an_identity_model(model_hw):
    """tiled_ref.stitched with x -> x + 0.5 returns grey + 0.5 exactly: a check of the reference itself."""
    hm, wm = model_hw
    rng = np.random.default_rng(hm)
    sizes = [(hm, wm), (hm + 1, wm), (hm - 1, 3 * wm + 7), (hm + 1, wm + 1), (2 * hm + 3, wm - 5), (hm // 2, wm // 3), (1, 1),
             (2 * hm - 1, 2 * wm + 1)]
    for h, w in sizes:
        grey = (rng.integers(0, 256, (h, w)).astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
        for v in sorted({0, min(hm, wm) // 2, min(TR.OVERLAP_DEFAULT, min(hm, wm) // 2), 7}):
            calls = []

            def model(x):
                calls.append(x)
                return x + np.float32(0.5)

            P = TR.stitched(grey, model, model_hw, v)
            oy, by, ox, bx = TR.page_plan((h, w), model_hw, v)
            assert len(calls) == len(oy) * len(ox)
            assert P.dtype == np.float32 and P.tobytes() == (grey + np.float32(0.5)).tobytes(), (h, w, v)
            # what lies outside the page in a tile input is BLACK_VALUE
            last = calls[-1]
            assert last.shape == (hm, wm)
            assert (last[min(h - oy[-1], hm):, :] == TR.BLACK_VALUE).all() and (last[:, min(w - ox[-1], wm):] == TR.BLACK_VALUE).all()
