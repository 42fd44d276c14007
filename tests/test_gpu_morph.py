"""Stroke repair on the GPU, bit for bit against tests/morph_ref.py.

Pages are put on the device with input_from_grey; results are compared as 32-bit words (a result pixel is the word of a
source pixel and NaN pixels keep their payloads, so the words are compared as they are); the mask and what the passes
counted (ocrs_morph_info) are compared as integers.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import models_util as M
import morph_ref as R
import ocrs_amd
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, OcrInput, _lib, output, synth
from test_gpu_binarize import SHAPES as BIN_SHAPES, level, planted, two_level

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
# test_gpu_binarize's shapes (one pixel, one row, one column, around a wave of 64, around 256 columns, several blocks), a
# page whose side is exactly the window of radius 63, and one smaller than it
SHAPES = BIN_SHAPES + [(130, 127), (64, 126)]
RADII = [(1, 0), (0, 1), (1, 1), (2, 5), (31, 3), (63, 63)]   # (rx, ry)
DENSITIES = (0.05, 0.5, 0.95)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    return OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(M.recognition_model_bytes()))


def image_of(page):
    return np.ascontiguousarray(page.image()[0])


def noise(seed, h, w, plant=True, ink=0.5):
    """[h, w] float32, uniform in [-0.5, 0.5) shifted so that a share `ink` of it lies under 0; plant: NaN of both kinds,
    +-inf, +-0, denormals and huge values over random places (test_gpu_binarize.planted)."""
    a = (np.random.default_rng(seed).random((h, w), dtype=F) - F(ink)).astype(F)
    return planted(a, seed) if plant else a


def ramp(h, w, axis, rising):
    """Strictly monotone along `axis`: every extremum of a window sits at its end, at the boundary of every block of a
    sliding scheme."""
    n = (h, w)[axis]
    v = (np.arange(n, dtype=np.float64) / max(n - 1, 1) - 0.5).astype(F)
    v = v if rising else v[::-1]
    return np.ascontiguousarray(np.broadcast_to(v[:, None] if axis == 0 else v[None, :], (h, w)))


def assert_same(got, exp, what):
    """(page, mask, info) of the library against the restatement's."""
    out, mask, info = got
    assert info == exp[2], (what, info, exp[2])
    assert out.dtype == np.float32 and out.shape == exp[0].shape and mask.dtype == np.uint8 and mask.shape == exp[1].shape, what
    bad = np.argwhere(out.view(U) != exp[0].view(U))
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r (%#x), expected %r (%#x)"
                             % (what, len(bad), out.size, at, out[at], out.view(U)[at], exp[0][at], exp[0].view(U)[at]))
    bad = np.argwhere(mask != exp[1])
    assert not len(bad), "%s: %d mask bytes differ; first at %s: got %d, expected %d" % (what, len(bad), tuple(bad[0]), mask[tuple(bad[0])], exp[1][tuple(bad[0])])


def check_batch(eng, pages, params, what):
    """One call for all the pages against the restatement of each -> the restatement's results."""
    made, masks, infos = eng.morph_batch([eng.input_from_grey(p) for p in pages], params, mask=True, info=True)
    exps = []
    for i, (page, p) in enumerate(zip(pages, params)):
        exps.append(R.morph(page, **(p or {})))
        assert made[i].shape == (1,) + page.shape
        assert_same((image_of(made[i]), masks[i], infos[i]), exps[-1], "%s, page %d %s" % (what, i, p))
    return exps


def check(eng, page, what, **params):
    return check_batch(eng, [page], [params], what)[0]


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_op_and_radius_on_noise_two_level_pages_and_ramps(eng, shape):
    h, w = shape
    fixed = [noise(h * 1000 + w + 7 * i, h, w, ink=ink) for i, ink in enumerate(DENSITIES)]
    fixed += [two_level("halves", h, w, 1), two_level("checkerboard", h, w, 1)]
    fixed += [ramp(h, w, axis, rising) for axis, rising in itertools.product((0, 1), (True, False))]
    exps = []
    for rx, ry in RADII:   # a call per radius: the vertical pass sizes its LDS by the largest ry of a call
        pages, params = [], []
        for op in R.OPS:
            for page in fixed + [two_level("stripes", h, w, rx), two_level("rows", h, w, ry)]:
                pages.append(page)
                params.append({"op": op, "rx": rx, "ry": ry})
        exps += check_batch(eng, pages, params, "%dx%d" % shape)
    moved = sum(e[2]["changed"] > 0 for e in exps)
    print(shape, len(exps), "pages;", moved, "of them changed")
    if h * w > 1:
        assert moved > 0 and any(0 < e[2]["counted"] < h * w for e in exps)


@pytest.mark.parametrize("ry", [7, 8, 31, 32], ids=lambda r: "ry%d" % r)
def test_the_radii_at_which_the_vertical_pass_changes_its_kernel(eng, ry):
    # 2 ry + 1 = 15 and 63 are the largest windows of the two smaller LDS arrays
    pages, params = [], []
    for h, w in ((97, 211), (300, 70), (2 * ry + 1, 65), (4 * ry + 3, 64)):
        for op, page in itertools.product(R.OPS, (noise(h + w + ry, h, w, ink=0.3), ramp(h, w, 0, True), ramp(h, w, 0, False), two_level("rows", h, w, ry))):
            pages.append(page)
            params.append({"op": op, "rx": 2, "ry": ry})
    exps = check_batch(eng, pages, params, "ry = %d" % ry)
    assert sum(e[2]["changed"] > 0 for e in exps) > len(exps) // 2


def test_the_longest_row_and_the_longest_column(eng):
    row = noise(8, 1, 65535, ink=0.4)
    col = np.ascontiguousarray(row.reshape(65535, 1))
    params = [{"op": op, "rx": 63, "ry": 63} for op in R.OPS]
    wide = check_batch(eng, [row] * 4, params, "1 x 65535")
    tall = check_batch(eng, [col] * 4, params, "65535 x 1")
    for a, b in zip(wide, tall):
        assert a[2] == b[2] and a[2]["changed"] > 60000 and a[0].tobytes() == b[0].tobytes()
    check_batch(eng, [ramp(1, 65535, 1, True), ramp(65535, 1, 0, False)], [{"op": "open", "rx": 63, "ry": 0}, {"op": "close", "rx": 0, "ry": 63}], "ramps")


def test_nan_beside_dark_and_pages_that_are_nearly_all_nan(eng):
    page, rx, ry = R.nan_beside_dark()
    for op in R.OPS:
        exp = check(eng, page, "the NaN beside the dark pixel", op=op, rx=rx, ry=ry)
    exp = check(eng, page, "the NaN beside the dark pixel", op="thicken", rx=rx, ry=ry)
    assert exp[0].view(U)[0, 1] == page.view(U)[1, 0] and exp[2] == {"counted": 8, "changed": 4, "ink_before": 1, "ink_after": 5}
    for shape in ((70, 130), (5, 300)):
        nans = np.full(shape, np.nan, F)
        nans.view(U)[3, 4] = 0xFFC12345
        one = nans.copy()
        one[2, 100] = F(-0.5)
        flat = np.full(shape, level(40), F)
        for op, (rx, ry) in itertools.product(R.OPS, ((2, 2), (63, 63))):
            exp = check(eng, nans, "all NaN", op=op, rx=rx, ry=ry)
            assert exp[2] == dict.fromkeys(R.INFO_KEYS, 0) and exp[0].view(U).tobytes() == nans.view(U).tobytes()
            exp = check(eng, one, "one counted pixel", op=op, rx=rx, ry=ry)
            assert exp[2] == {"counted": 1, "changed": 0, "ink_before": 1, "ink_after": 1} and exp[0].view(U).tobytes() == one.view(U).tobytes()
            exp = check(eng, flat, "flat", op=op, rx=rx, ry=ry)
            assert exp[2]["changed"] == 0 and exp[0].tobytes() == flat.tobytes()


# ------------------------------------------------------------------ 2. batches
MIXED = [((97, 211), {"op": "close", "rx": 3, "ry": 1}), ((128, 256), {"op": "thin", "rx": 63, "ry": 63}), ((1, 300), {"op": "open", "rx": 15, "ry": 0}),
         ((70, 258), {"op": "thicken", "rx": 0, "ry": 31}), ((65, 63), {"op": "thicken", "rx": 1, "ry": 1}), ((260, 130), None),
         ((33, 70), {"op": "thin", "rx": 2, "ry": 5})]


def test_mixed_batch_equals_each_page_alone_ten_times(eng):
    srcs = [noise(40 + i, *s, ink=0.3) for i, (s, _) in enumerate(MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in MIXED]
    exp = [R.morph(s, **(p or {})) for s, p in zip(srcs, params)]
    first = None
    for rep in range(10):
        pages, masks, infos = eng.morph_batch(inputs, params, mask=True, info=True)
        got = [(image_of(p), m, i) for p, m, i in zip(pages, masks, infos)]
        if first is None:
            first = got
            for i, g in enumerate(got):
                assert_same(g, exp[i], "batch page %d" % i)
                alone = eng.morph(inputs[i], mask=True, info=True, **(params[i] or {}))
                assert alone[2] == g[2] and image_of(alone[0]).tobytes() == g[0].tobytes() and alone[1].tobytes() == g[1].tobytes(), "page %d alone" % i
        else:
            assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(got, first)), "repeat %d" % rep
    for order in (slice(None, None, -1), slice(0, 1), slice(1, 2), slice(3, 5)):   # two-stage pages first, last, alone, absent
        pages = eng.morph_batch(inputs[order], params[order])
        assert [image_of(p).tobytes() for p in pages] == [e[0].tobytes() for e in exp[order]]
    assert [image_of(p).tobytes() for p in eng.morph_batch(inputs[:2], {"op": "open", "rx": 2})] == \
        [image_of(eng.morph(i, op="open", rx=2)).tobytes() for i in inputs[:2]], "one parameter set for all"
    assert eng.morph_batch([], None) == [] and eng.morph_batch([], None, mask=True, info=True) == ([], [], [])
    with pytest.raises(ValueError):
        eng.morph_batch(inputs, params[:2])


def test_mask_alone_info_alone_and_neither(eng):
    src = noise(21, 70, 130, ink=0.3)
    inp = eng.input_from_grey(src)
    exp = R.morph(src, "open", 5, 2)
    kw = {"op": "open", "rx": 5, "ry": 2}
    page = eng.morph(inp, **kw)
    assert isinstance(page, OcrInput) and image_of(page).tobytes() == exp[0].tobytes()
    page, mask = eng.morph(inp, mask=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and mask.tobytes() == exp[1].tobytes()
    page, info = eng.morph(inp, info=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and info == exp[2] and tuple(info) == R.INFO_KEYS
    assert image_of(eng.morph(inp)).tobytes() == R.morph(src)[0].tobytes(), "the defaults: close at radius 1"
    assert image_of(eng.morph(inp, rx=3)).tobytes() == R.morph(src, "close", 3, 3)[0].tobytes(), "ry follows rx"


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = noise(99, 131, 70, ink=0.3)
    inp = eng.input_from_grey(src)
    exp = R.morph(src, "close", 4, 4)[0]
    out = eng.morph(inp, rx=4)
    assert image_of(inp).tobytes() == src.tobytes()
    del out   # ocrs_page_free of the result: the source is a page of its own
    assert image_of(inp).tobytes() == src.tobytes()
    out = eng.morph(inp, rx=4)
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == exp.tobytes()
    again = eng.morph(out, op="thin", rx=9, ry=1)   # a repaired page is an ordinary page
    assert image_of(again).tobytes() == R.morph(exp, "thin", 9, 1)[0].tobytes()


def test_bad_parameters_have_their_status(eng):
    inp = eng.input_from_grey(noise(1, 20, 20))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    for kw in ({"rx": 0}, {"rx": 64}, {"rx": -1}, {"rx": 1, "ry": 64}, {"rx": 1, "ry": -1}, {"rx": 0, "ry": 0}):
        refused(lambda: eng.morph(inp, **kw))
    with pytest.raises(ValueError):
        eng.morph(inp, op="dilate")
    refused(lambda: eng.morph_batch([inp, inp], [None, {"rx": 64}]))   # one bad page refuses the call
    live = _lib.pool_stats()["device_live"]
    pages = (C.c_void_p * 2)(inp._h, inp._h)
    for bad in (_lib.MorphParams(4, 1, 1), _lib.MorphParams(-1, 1, 1), _lib.MorphParams(2, 0, 0), _lib.MorphParams(0, 64, 1)):
        ps = (_lib.MorphParams * 2)(_lib.MorphParams(2, 1, 1), bad)
        out = (C.c_void_p * 2)()
        masks = (C.POINTER(C.c_uint8) * 2)()
        assert _lib.lib().ocrs_engine_morph_pages(eng._h, pages, C.c_size_t(2), ps, out, masks, None) == 1, "INVALID_ARGUMENT"
        assert [out[i] for i in range(2)] == [None, None] and not masks[0] and not masks[1], "a failed call writes nothing"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    one = C.c_void_p()
    assert _lib.lib().ocrs_engine_morph_page(eng._h, inp._h, None, None, None, None) == 1
    ok = (_lib.MorphParams * 1)(_lib.MorphParams(2, 1, 1))
    assert _lib.lib().ocrs_engine_morph_pages(eng._h, None, C.c_size_t(1), ok, C.byref(one), None, None) == 1
    assert _lib.lib().ocrs_engine_morph_pages(eng._h, pages, C.c_size_t(1), None, C.byref(one), None, None) == 1
    assert _lib.lib().ocrs_engine_morph_page(eng._h, inp._h, None, C.byref(one), None, None) == 0, "NULL: the default"
    assert image_of(OcrInput(one)).tobytes() == image_of(eng.morph(inp)).tobytes()   # (the OcrInput frees the page)
    wide = eng.input_from_grey(np.zeros((1, 65536), F))
    refused(lambda: eng.morph(wide))
    # a page belongs to a device: another engine of this device serves it, an engine of another device refuses it
    dbuf, rbuf = M.detection_model_bytes(), M.recognition_model_bytes()
    same = OcrEngine(detection_model=Model.load_bytes(dbuf), recognition_model=Model.load_bytes(rbuf))
    assert image_of(same.morph(inp)).tobytes() == image_of(eng.morph(inp)).tobytes()
    if _lib.device_count() >= 2:
        other = OcrEngine(detection_model=Model.load_bytes(dbuf, device=1), recognition_model=Model.load_bytes(rbuf, device=1))
        refused(lambda: other.morph(inp))


# ------------------------------------------------------------------ 3. composition
def damaged_picture(seed, h, w, lines):
    """A synthetic page with every third column of its ink lost, pepper and a table grid, as a picture."""
    px = synth.synthetic_page(seed, h, w, lines=lines, columns=1)
    px[:, np.arange(w) % 3 == 2] = np.maximum(px[:, np.arange(w) % 3 == 2], 230)
    px[np.random.default_rng(seed).random((h, w)) < 0.003] = 0
    for r in range(20, h - 2, 90):
        px[r:r + 2, 10:w - 10] = 0
    return px


def test_get_text_with_morph_is_the_manual_chain(eng):
    inp = eng.prepare_input(ImageSource.from_tensor(damaged_picture(5, 600, 500, 24), DimOrder.Hwc))
    for params in (True, {"op": "thicken", "rx": 1, "ry": 0}):
        kw = {} if params is True else params
        page, info = eng.morph(inp, info=True, **kw)
        assert info["changed"] > 1000
        assert image_of(page).tobytes() == R.morph(image_of(inp), **kw)[0].tobytes()
        lines = eng.find_text_lines(page, eng.detect_words(page))
        text = "\n".join(str(t) for t in eng.recognize_text(page, lines) if t is not None)
        assert eng.get_text(inp, morph=params) == text
        norm = eng.normalize(inp)
        assert eng.get_text(inp, morph=params, normalize=True) == eng.get_text(eng.morph(norm, **kw))   # after normalisation ...
        clean = eng.despeckle(norm)
        assert eng.get_text(inp, morph=params, normalize=True, despeckle=True) == eng.get_text(eng.morph(clean, **kw))   # ... despeckling ...
        ruled = eng.remove_rules(clean)
        assert eng.get_text(inp, morph=params, normalize=True, despeckle=True, rules=True) == eng.get_text(eng.morph(ruled, **kw))   # ... and rules
        assert eng.get_text(inp, morph=params, rules={"min_length": 200}) == eng.get_text(eng.morph(eng.remove_rules(inp, min_length=200), **kw))
    assert eng.get_text(inp, morph=None) == eng.get_text(inp) == eng.get_text(inp, morph=False)


def test_without_morph_get_text_launches_what_it_launched(eng):
    inp = eng.prepare_input(ImageSource.from_tensor(damaged_picture(6, 400, 500, 16), DimOrder.Hwc))
    eng.get_text(inp)
    eng.enable_timing(2)
    try:
        counts = []
        for kw in ({}, {"morph": None}, {"morph": False}):
            eng.kernel_stats(reset=True)
            text = eng.get_text(inp, **kw)
            counts.append((text, {name: s["launches"] for name, s in eng.kernel_stats(reset=True).items()}))
    finally:
        eng.enable_timing(0)
    assert counts[0] == counts[1] == counts[2] and sum(counts[0][1].values()) > 0


def test_cli_morph(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    px = damaged_picture(9, 700, 600, 30)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("closed", "thick", "plain")}
    assert cli.main([path, "--morph", "close:1", "-j", "--debug", "-o", files["closed"]]) == 0
    assert cli.main([path, "--morph", "thicken:1x0", "-j", "-o", files["thick"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in ("dilate", "close:64", "close:0", "close:1x", "thin:0x0", "open:1x2x3", "close:x", ""):
        with pytest.raises(SystemExit):
            cli.main([path, "--morph", bad])
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def document(**kw):
        page, info = eng.morph(inp, info=True, **kw)
        lines = eng.find_text_lines(page, eng.detect_words(page))
        record = dict(info, **ocrs_amd.morph_params(**kw))
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(page, lines), morph=record), record

    plain = output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "morph" not in json.loads(plain), "without the flag nothing changes"
    exp, record = document(op="close", rx=1)
    assert text["closed"] == exp and record["changed"] > 1000
    assert json.loads(text["closed"])["morph"] == record == dict(record, op="close", rx=1, ry=1) and set(record) == set(R.INFO_KEYS) | {"op", "rx", "ry"}
    exp, record = document(op="thicken", rx=1, ry=0)
    assert text["thick"] == exp and json.loads(text["thick"])["morph"] == dict(record, op="thicken", rx=1, ry=0)
    assert cli.main([path, "--morph", "open", "-j", "-o", files["plain"]]) == 0
    assert json.loads(open(files["plain"], encoding="utf-8").read())["morph"]["op"] == "open", "the radius is optional"


# ------------------------------------------------------------------ 4. beside other callers
def test_morph_callers_beside_plain_callers(eng):
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    damaged = [R.break_strokes(image_of(p), 0.3, 7 + i) for i, p in enumerate(pages)]
    inputs = [eng.input_from_grey(s) for s in damaged]
    params = [{}, {"op": "open", "rx": 63, "ry": 63}, {"op": "thicken", "rx": 2, "ry": 0}, {"op": "thin", "rx": 0, "ry": 31}]

    def repair(i):
        page, mask, info = eng.morph(inputs[i], mask=True, info=True, **params[i])
        return image_of(page).tobytes(), mask.tobytes(), tuple(sorted(info.items()))

    def plain(i):
        return eng.get_text(pages[i])

    quiet_repair, quiet_plain = [repair(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        out, mask, info = R.morph(damaged[i], **params[i])
        assert quiet_repair[i] == (out.tobytes(), mask.tobytes(), tuple(sorted(info.items())))
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, repair(i) if t < 4 else plain(i))
        except Exception as e:   # pragma: no cover - reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert len(results) == 24
    for (t, r), (i, got) in results.items():
        assert got == (quiet_repair[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)
