"""The two host decisions behind conv_rows = 2 (ocrs_amd/csrc/conv_rows.hpp), through ocrs_conv_rows_selftest: no GPU.

1. Per conv layer, from the model file alone: may the matrix-core work of tap rows outside the image be dropped without
   changing a bit?  Only if every weight is finite (0 x Inf = NaN) and either a ReLU follows or no bias is -0.0 (the spec's
   fmaf(0, w, -0.0) can give +0 where the skip leaves -0).
2. Per block of a 4 x 32 patch at image row y0: which 16-deep chunks of the tap-major K loop leave out which patch row.
"""
import ctypes as C

import numpy as np
import pytest

from ocrs_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def selftest(lib, w, b, relu, y0, h, cin):
    w, b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    out = (C.c_int32 * 6)()
    rc = lib.ocrs_conv_rows_selftest(w.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(w.size), b.ctypes.data_as(C.POINTER(C.c_float)),
                                     C.c_size_t(b.size), int(relu), int(y0), int(h), int(cin), out)
    assert rc == 0, lib.ocrs_last_error()
    return list(out)


def weights(cin=32, cout=8, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((9 * cin, cout)).astype(np.float32), rng.standard_normal(cout).astype(np.float32)


@pytest.mark.parametrize("relu", [0, 1])
def test_flag_needs_finite_weights(lib, relu):
    w, b = weights()
    assert selftest(lib, w, b, relu, 0, 8, 32)[0] == 1
    for bad in (np.inf, -np.inf, np.nan):
        for at in (0, w.size // 2, w.size - 1):    # a ky = 0 tap, the centre tap, the last ky = 2 tap
            w2 = w.copy()
            w2.flat[at] = bad
            assert selftest(lib, w2, b, relu, 0, 8, 32)[0] == 0, (bad, at)
    # denormals, zeros of both signs and the largest finite value are finite
    w2 = w.copy()
    w2.flat[:4] = [np.float32(1e-45), 0.0, -0.0, np.finfo(np.float32).max]
    assert selftest(lib, w2, b, relu, 0, 8, 32)[0] == 1
    # a non-finite BIAS is no obstacle: the accumulator starts from it with or without the skip
    b2 = b.copy()
    b2[1] = np.inf
    assert selftest(lib, w, b2, relu, 0, 8, 32)[0] == 1


def test_flag_negative_zero_bias_needs_relu(lib):
    w, b = weights()
    b2 = b.copy()
    b2[3] = -0.0
    assert selftest(lib, w, b2, 1, 0, 8, 32)[0] == 1     # ReLU writes +0 for both zeros
    assert selftest(lib, w, b2, 0, 0, 8, 32)[0] == 0
    b2[3] = 0.0
    assert selftest(lib, w, b2, 0, 0, 8, 32)[0] == 1     # +0.0 + (+-0) = +0.0 either way
    assert selftest(lib, w, np.full_like(b, -0.0), 0, 0, 8, 32)[0] == 0


@pytest.mark.parametrize("cin", [32, 64, 128])
@pytest.mark.parametrize("h", [4, 8, 16])
def test_phase_table(lib, h, cin):
    w, b = weights(cin=cin)
    per_tap = cin // 16
    for y0 in range(0, h, 4):
        flag, c_top, c_bot, p0, p1, p2 = selftest(lib, w, b, 1, y0, h, cin)
        top, bot = y0 == 0, y0 + 4 == h
        assert flag == 1
        assert (c_top, c_bot) == (3 * per_tap if top else 0, 6 * per_tap if bot else 9 * per_tap)
        assert c_top % 2 == 0 and c_bot % 2 == 0            # the K loop takes chunks in pairs
        assert (p0, p1, p2) == (0 if top else -1, -1, 3 if bot else -1)
        # chunk by chunk against the definition: chunk c holds tap c // per_tap, ky = tap // 3; patch row j reads image row
        # y0 + j + ky - 1, and sits the chunk out exactly when that row is outside the image
        for c in range(9 * per_tap):
            ky = (c // per_tap) // 3
            out_rows = [j for j in range(4) if not 0 <= y0 + j + ky - 1 < h]
            skipped = [0] if c < c_top else [3] if c >= c_bot else []
            assert skipped == out_rows, (y0, h, cin, c)
    # a layer without the flag leaves nothing out
    w[0, 0] = np.inf
    assert selftest(lib, w, b, 1, 0, h, cin) == [0, 0, 9 * per_tap, -1, -1, -1]


def test_conv_rows_is_no_process_option(lib):
    """"conv_rows" belongs to an engine (ocrs_engine_set_option): the table of process options does not list or take it."""
    assert "conv_rows" not in _lib.option_names()
    assert lib.ocrs_set_option(b"conv_rows", C.c_long(1)) == 1
    assert b"conv_rows" in lib.ocrs_last_error()


def test_bad_arguments(lib):
    w, b = weights()
    out = (C.c_int32 * 6)()
    wp, bp = w.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_float))
    for y0, h, cin in ((0, 6, 32), (2, 8, 32), (8, 8, 32), (0, 8, 16), (0, 8, 48), (-4, 8, 32), (0, 0, 32)):
        assert lib.ocrs_conv_rows_selftest(wp, C.c_size_t(w.size), bp, C.c_size_t(b.size), 1, y0, h, cin, out) == 1, (y0, h, cin)
    assert lib.ocrs_conv_rows_selftest(wp, C.c_size_t(w.size), bp, C.c_size_t(b.size), 1, 0, 8, 32, None) == 1
