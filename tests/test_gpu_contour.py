"""contour_rect_kernel (kernels_ccl.hip) against the definition, branch by branch: every case of contour_cases.py — walk
buffer, small-polygon scratch, hulls beyond one 64-lane stride, degenerate hulls, RDP ties, the mask window, every 4 x 4
pattern, the capacity exits — through ocrs_mask_component_rects (min_area 0: the rectangles of ALL components, and 100;
the four-pixel and the byte labelling kernels) and through detect_words of a callback-model engine (the `prepared` path).
Per slot: n_roots, the valid bytes, and on valid slots the six floats as uint32 words (-0.0 is a difference).  Invalid
slots' floats are not compared: the kernel does not write them.  test_contour_cases_cpu.py shows that each case reaches
its branch."""
import numpy as np
import pytest

import contour_cases as CC
import contour_ref as R
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib

pytestmark = pytest.mark.gpu

EXPAND = 3.0
CASES = CC.cases() + CC.noise_masks()
BY_NAME = {c.name: c for c in CASES}
_DEFN, _SINGLE = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()  # fail loudly: there is no CPU fallback to "pass" on
    yield
    _lib.set_option("ccl_quad", 1)


def definition(name, mask, min_area):
    if name not in _DEFN:       # computed once per mask, shared by every test, never modified
        _DEFN[name] = R.component_slots(mask, EXPAND, 0.0)
    return R.with_min_area(_DEFN[name], min_area)


def assert_page(got, exp, label):
    assert got["n_roots"] == exp["n_roots"], (label, got["n_roots"], exp["n_roots"])
    assert not got["overflow"], label
    bad = np.flatnonzero(got["valid"] != exp["valid"])
    assert bad.size == 0, (label, "valid", bad[:8].tolist(), got["valid"][bad[:8]].tolist(), exp["valid"][bad[:8]].tolist())
    ok = exp["valid"] == 1
    gw, ew = R.words(got["rects"][ok]), R.words(exp["rects"][ok])
    diff = np.flatnonzero((gw != ew).any(axis=1))
    assert diff.size == 0, (label, "rects", np.flatnonzero(ok)[diff[:4]].tolist(), got["rects"][ok][diff[:4]].tolist(),
                            exp["rects"][ok][diff[:4]].tolist())


def quads(w):
    return (1, 0) if w % 4 == 0 else (1,)


def hook(masks, min_area, quad, **kw):
    _lib.set_option("ccl_quad", quad)
    try:
        return _lib.mask_component_rects(masks, EXPAND, min_area, **kw)
    finally:
        _lib.set_option("ccl_quad", 1)


def single(case, min_area, quad):
    key = (case.name, min_area, quad)
    if key not in _SINGLE:
        _SINGLE[key] = hook(case.mask, min_area, quad)[0]
    return _SINGLE[key]


@pytest.mark.parametrize("min_area", [0.0, 100.0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_hook_equals_the_definition(case, min_area):
    for quad in quads(case.mask.shape[1]):
        assert_page(single(case, min_area, quad), definition(case.name, case.mask, min_area), (case.name, min_area, quad))


_ENGINES = {}


def mask_engine(h, w):
    """An engine whose detection 'model' returns a chosen probability map at the page's own size: threshold, components and
    rectangles only (test_gpu_parity._mask_engine_pair's GPU half), one per page size."""
    if (h, w) not in _ENGINES:
        box = {}
        gpu = OcrEngine(detection_model=Model.from_callable([None, 1, h, w], lambda x: box["prob"].reshape(1, 1, h, w)))
        inp = gpu.prepare_input(ImageSource.from_tensor(np.zeros((1, h, w), np.float32), DimOrder.Chw))
        _ENGINES[(h, w)] = (box, gpu, inp)
    return _ENGINES[(h, w)]


def assert_words(got, exp, label):
    want = exp["rects"][exp["valid"] == 1]
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert np.array_equal(R.words(got), R.words(want)), label


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_detect_words_equals_the_definition(case):
    h, w = case.mask.shape
    box, gpu, inp = mask_engine(h, w)
    box["prob"] = case.mask.astype(np.float32)
    exp = definition(case.name, case.mask, 100.0)
    try:
        for quad in quads(w):       # quad 1 at w % 4 == 0: the labels come prepared from the threshold kernel
            gpu.set_option("ccl_quad", quad)
            assert_words(gpu.detect_words(inp), exp, (case.name, quad))
    finally:
        gpu.set_option("ccl_quad", 1)


def _stacks():
    by_shape = {}
    for c in CASES:
        by_shape.setdefault(c.mask.shape, []).append(c)
    return [g for g in by_shape.values() if len(g) > 1]


@pytest.mark.parametrize("group", _stacks(), ids=lambda g: "%dx%d" % g[0].mask.shape)
def test_stacked_pages_give_the_bits_of_single_calls(group):
    """Cases of one page size in ONE multi-page call: every page's slots equal the definition and, word for word over the
    page's slots (invalid ones' valid bytes included), the call on that page alone."""
    stack = np.stack([c.mask for c in group])
    for min_area in (0.0, 100.0):
        for quad in quads(stack.shape[2]):
            got = hook(stack, min_area, quad)
            assert len(got) == len(group)
            for c, page in zip(group, got):
                assert_page(page, definition(c.name, c.mask, min_area), ("stacked", c.name, min_area, quad))
                alone = single(c, min_area, quad)
                assert page["n_roots"] == alone["n_roots"] and np.array_equal(page["valid"], alone["valid"])
                ok = alone["valid"] == 1
                assert np.array_equal(R.words(page["rects"][ok]), R.words(alone["rects"][ok])), c.name


# ------------------------------------------------------------------ g. every 4 x 4 pattern
@pytest.fixture(scope="module")
def patterns():
    pages = CC.pattern_pages()
    return pages, [R.component_slots(p, EXPAND, 0.0) for p in pages]


@pytest.mark.parametrize("min_area", [0.0, 100.0])
def test_every_4x4_pattern_through_the_hook(patterns, min_area):
    """All 65 536 patterns on four pages in one call.  Nearly every component here is below min_area 100: only the hook with
    min_area 0 shows their rectangles."""
    pages, slots = patterns
    assert sum(s["n_roots"] for s in slots) > 100000 and sum(int(s["valid"].sum()) for s in slots) > 50000
    for quad in (1, 0):
        got = hook(pages, min_area, quad)
        for i in range(len(pages)):
            assert_page(got[i], R.with_min_area(slots[i], min_area), ("patterns", i, min_area, quad))


def test_every_4x4_pattern_through_detect_words(patterns):
    pages, slots = patterns
    h, w = pages.shape[1:]
    box, gpu, inp = mask_engine(h, w)
    for i in range(len(pages)):
        box["prob"] = pages[i].astype(np.float32)
        assert_words(gpu.detect_words(inp), R.with_min_area(slots[i], 100.0), ("patterns", i))


# ------------------------------------------------------------------ h. capacity exits
@pytest.fixture(scope="module")
def capacity():
    pages = np.stack([CC.ordinary_page(0), CC.capacity_page(), CC.ordinary_page(1)])
    slots = [R.component_slots(p, EXPAND, 0.0) for p in pages]
    return pages, slots


@pytest.mark.parametrize("quad", [1, 0])
@pytest.mark.parametrize("short", ["fits", "max_comp", "arena"])
def test_capacity_exits_between_ordinary_pages(capacity, short, quad):
    """max_comp equal to the page's component count and arena equal to the sum of its border lengths: the page fits, exactly.
    One less of either: the overflow flag is set and n_roots is still the true count; the pages before and after it in
    the batch are untouched.  Which slots of an overflowed page were filled is not defined (the arena bump order is not),
    so nothing is asserted about them."""
    pages, slots = capacity
    count, border = slots[1]["n_roots"], int(slots[1]["n"].sum())
    assert all(s["n_roots"] < count and int(s["n"].sum()) < border for s in (slots[0], slots[2]))
    exact = hook(pages, 0.0, quad, max_comp=count, arena=border)
    for i in range(3):
        assert_page(exact[i], slots[i], ("exact", i))
    if short == "fits":
        return
    got = hook(pages, 0.0, quad, max_comp=count - (short == "max_comp"), arena=border - (short == "arena"))
    assert got[1]["overflow"] and got[1]["n_roots"] == count
    for i in (0, 2):
        assert_page(got[i], slots[i], (short, i))


def test_unwritten_slots_are_recognisable():
    """The hook's sentinel: what lies beyond a page's components was not written by the kernel."""
    lib = _lib.lib()
    import ctypes as C
    m = CC.capacity_page()[None]
    n_roots, overflow = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rects, valid = np.zeros((1, 32, 6), np.float32), np.zeros((1, 32), np.uint8)
    _lib.check(lib.ocrs_mask_component_rects(m.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(1), 48, 64, C.c_float(3.0), C.c_float(0.0),
                                             32, C.c_int64(4096), n_roots.ctypes.data_as(C.POINTER(C.c_int32)),
                                             overflow.ctypes.data_as(C.POINTER(C.c_int32)), rects.ctypes.data_as(C.POINTER(C.c_float)),
                                             valid.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert n_roots[0] == 18 and set(valid[0, :18].tolist()) <= {0, 1} and (valid[0, 18:] == 0xEE).all()
