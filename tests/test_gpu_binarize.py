"""Adaptive binarisation on the GPU, bit for bit against tests/binarize_ref.py.

Pages are put on the device with input_from_grey; results are compared as 32-bit words (NaN pixels keep their payloads and,
with keep_ink, ink keeps its own word, so the words are compared as they are); the mask and what the passes counted
(ocrs_binarize_info) are compared as integers.

Run with:  python -m pytest tests -m gpu
"""
import ctypes as C
import itertools
import json
import threading

import numpy as np
import pytest

import binarize_ref as B
import despeckle_ref as D
import models_util as M
import rules_ref as R
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, OcrInput, _lib, output, synth
from oracle import pipeline as OP
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu
F = np.float32
# (height, width): one pixel, one row, one column; around one wave of 64 pixels either way; odd sizes of several blocks;
# around the 256 columns of a strip of the vertical pass; a page that holds a whole window of the largest radius
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (65, 63), (127, 129), (129, 127), (97, 211), (70, 256), (70, 257), (70, 258),
          (70, 259), (300, 300)]
RADII = (1, 2, 15, 31, 127)
KQS = (0, 1, 87, 128, 256)
DENSITIES = (0.05, 0.5, 0.95)
# every radius with every k; both keep_ink modes and given fills go round with them
COMBOS = [dict({"radius": r, "k_q8": kq, "keep_ink": bool(i % 2)}, **({"ink_level": -0.25, "paper": 0.125} if i % 3 == 0 else {}))
          for i, (r, kq) in enumerate(itertools.product(RADII, KQS))]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    return OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(M.recognition_model_bytes()))


@pytest.fixture(scope="module")
def text_pages():
    """The 512 x 512 text page of DESIGN.md §7.9 prepared by the oracle, and the same under the shade of §7.10."""
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(M.detection_model_bytes()), "exact"),
                       recognition_model=OracleModel(OracleGraph(M.recognition_model_bytes()), "exact"))
    px = synth.synthetic_page(3, 512, 512, 30, 2, 1)
    clean = np.ascontiguousarray(np.asarray(ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc")), F)[0])
    return clean, B.shade(clean)


def image_of(page):
    return np.ascontiguousarray(page.image()[0])


def level(b):
    return F((b + 0.5) / 256.0 - 0.5)


def planted(a, seed):
    """NaN (quiet and signalling), +-inf, -0.0, values far outside [-0.5, 0.5] and denormals written over random places of
    the page as 32-bit words (fewer on a page of fewer pixels)."""
    words = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x40400000, 0xC0400000, 0x7F7FFFFF,
                      0xFF7FFFFF, 0x00000001, 0x80000001], np.uint32)
    flat = a.reshape(-1).view(np.uint32)
    n = min(len(words), max(1, flat.size // 8))
    flat[np.random.default_rng(seed).choice(flat.size, size=n, replace=False)] = words[:n]
    return a


def noise(seed, h, w, plant=False, ink=0.5):
    """[h, w] float32, uniform in [-0.5, 0.5) shifted so that a share `ink` of it lies under 0; plant: see planted()."""
    a = (np.random.default_rng(seed).random((h, w), dtype=F) - F(ink)).astype(F)
    return planted(a, seed) if plant else a


def two_level(kind, h, w, r):
    """Halves, a checkerboard, or stripes of period 2 r + 1 (every window then holds the same share of either level)."""
    yy, xx = np.mgrid[0:h, 0:w]
    dark = {"halves": xx * 2 < w, "checkerboard": (yy + xx) % 2 == 0, "stripes": (xx % (2 * r + 1)) <= r // 2,
            "rows": (yy % (2 * r + 1)) == 0}[kind]
    return np.where(dark, level(40), level(210)).astype(F)


def kw_of(p):
    """The keywords of OcrEngine.binarize for a parameter set of the restatement: k = k_q8 / 256 rounds back to k_q8."""
    p = dict(p or {})
    if "k_q8" in p:
        p["k"] = p.pop("k_q8") / 256.0
    return p


def assert_same(got, exp, what):
    """(page, mask, info) of the library against the restatement's."""
    out, mask, info = got
    assert info == exp[2], (what, info, exp[2])
    assert out.dtype == np.float32 and out.shape == exp[0].shape and mask.dtype == np.uint8 and mask.shape == exp[1].shape, what
    bad = np.argwhere(out.view(np.uint32) != exp[0].view(np.uint32))
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r (%#x), expected %r (%#x)"
                             % (what, len(bad), out.size, at, out[at], out.view(np.uint32)[at], exp[0][at], exp[0].view(np.uint32)[at]))
    bad = np.argwhere(mask != exp[1])
    assert not len(bad), "%s: %d mask bytes differ; first at %s: got %d, expected %d" % (what, len(bad), tuple(bad[0]), mask[tuple(bad[0])], exp[1][tuple(bad[0])])


def check_batch(eng, pages, params, what):
    """One call for all the pages against the restatement of each -> the restatement's results.  Pages that are the same
    array share the window sums of the restatement at one radius."""
    made, masks, infos = eng.binarize_batch([eng.input_from_grey(p) for p in pages], [kw_of(p) for p in params], mask=True, info=True)
    exps, sums = [], {}
    for i, (page, p) in enumerate(zip(pages, params)):
        key = (id(page), (p or {}).get("radius", 15))
        if key not in sums:
            sums[key] = B.window_sums(page, key[1])
        exps.append(B.binarize(page, sums=sums[key], **(p or {})))
        assert made[i].shape == (1,) + page.shape
        assert_same((image_of(made[i]), masks[i], infos[i]), exps[-1], "%s, page %d %s" % (what, i, p))
    return exps


def check(eng, page, what, **params):
    return check_batch(eng, [page], [params], what)[0]


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_radius_and_k_on_noise_text_and_two_level_pages(eng, text_pages, shape):
    h, w = shape
    fixed = [noise(h * 1000 + w + 7 * i, h, w, plant=plant, ink=ink) for i, (ink, plant) in enumerate(itertools.product(DENSITIES, (False, True)))]
    fixed.append(np.ascontiguousarray(text_pages[1][100:100 + h, 50:50 + w]))
    fixed.append(planted(fixed[-1].copy(), 3))
    fixed += [two_level("halves", h, w, 1), two_level("checkerboard", h, w, 1)]
    by_radius = {r: [two_level("stripes", h, w, r), two_level("rows", h, w, r)] for r in RADII}
    stride = 3 if h * w > 50000 else 1   # the largest page takes every third combination per page, each page another third
    pages, params = [], []
    for j, combo in enumerate(COMBOS):
        for i, page in enumerate(fixed + by_radius[combo["radius"]]):
            if (i + j) % stride == 0:
                pages.append(page)
                params.append(combo)
    exps = check_batch(eng, pages, params, "%dx%d" % shape)
    share = [e[2]["ink"] / max(e[2]["counted"], 1) for e in exps]
    print(shape, len(pages), "pages; ink share %.3f .. %.3f" % (min(share), max(share)))
    if h * w > 1:
        assert max(share) > 0.2 and any(e[2]["ink"] > 0 and e[2]["counted"] < h * w for e in exps)


def test_the_largest_window_and_the_planted_tie(eng):
    page, r, kq, ys, xs = B.tie_page()
    exp = check(eng, page, "the tie", radius=r, k_q8=kq)
    assert not exp[1][ys, xs].any() and exp[1][ys, xs].size == 46 * 46
    darker = page.copy()
    darker[ys, xs] = level(31)
    exp = check(eng, darker, "one bin under the tie", radius=r, k_q8=kq)
    assert exp[1][ys, xs].all()
    rng = np.random.default_rng(5)
    pages = [np.where(rng.random((300, 300)) < 0.5, level(lo), level(hi)).astype(F) for lo, hi in ((0, 255), (254, 255), (3, 250), (1, 255))]
    check_batch(eng, pages, [{"radius": 127, "k_q8": kq} for kq in (256, 256, 87, 1)], "two levels at r = 127")


def test_the_longest_row_and_the_longest_column(eng):
    row = noise(8, 1, 65535, plant=True, ink=0.4)
    exps = check_batch(eng, [row, row, row], [{"radius": 127}, {"radius": 1, "k_q8": 0}, {"radius": 15, "keep_ink": True}], "1 x 65535")
    assert all(e[2]["ink"] > 1000 for e in exps)
    col = np.ascontiguousarray(row.reshape(65535, 1))
    assert check(eng, col, "65535 x 1", radius=127)[2]["ink"] == exps[0][2]["ink"]


def test_degenerate_pages(eng):
    for shape in ((70, 130), (5, 300)):
        n = shape[0] * shape[1]
        for b, kq in itertools.product((0, 128, 255), (0, 87, 256)):
            exp = check(eng, np.full(shape, level(b), F), "flat at bin %d" % b, k_q8=kq)
            assert exp[2] == {"counted": n, "ink": 0, "ink_fill": -0.5, "paper_fill": 0.5}
        nans = np.full(shape, np.nan, F)
        nans.view(np.uint32)[3, 4] = 0xFFC12345
        exp = check(eng, nans, "all NaN", radius=2)
        assert exp[2]["counted"] == 0 and exp[0].view(np.uint32).tobytes() == nans.view(np.uint32).tobytes()
        one = nans.copy()
        one[2, 100] = F(-0.5)
        for keep in (False, True):
            exp = check(eng, one, "one counted pixel", keep_ink=keep)
            assert exp[2]["counted"] == 1 and exp[2]["ink"] == 0 and exp[0][2, 100] == F(0.5)


def test_keep_ink_and_fills(eng):
    page = planted(noise(12, 97, 211, ink=0.3), 12)
    for kw in ({"keep_ink": True}, {"keep_ink": True, "paper": 0.25}, {"ink_level": -0.0}, {"ink_level": -0.125, "paper": 3.0e38},
               {"keep_ink": True, "ink_level": 0.3}, {"paper": float("nan"), "ink_level": float("nan")}):
        exp = check(eng, page, "fills", radius=7, **kw)
        assert 1000 < exp[2]["ink"] < exp[2]["counted"] < page.size
        if kw.get("keep_ink"):
            ink = exp[1].astype(bool)
            assert exp[0].view(np.uint32)[ink].tobytes() == page.view(np.uint32)[ink].tobytes()


MIXED = [((97, 211), {"radius": 3, "k_q8": 50}), ((128, 256), {"radius": 127, "k_q8": 256, "keep_ink": True, "paper": 0.25}),
         ((1, 300), {"radius": 15, "k_q8": 0}), ((70, 258), {"radius": 31, "ink_level": -0.125}),
         ((65, 63), {"radius": 1, "k_q8": 128, "keep_ink": True}), ((260, 130), None)]


def test_mixed_batch_equals_each_page_alone_ten_times(eng):
    srcs = [noise(40 + i, *s, plant=i % 2 == 0, ink=0.3) for i, (s, _) in enumerate(MIXED)]
    inputs = [eng.input_from_grey(s) for s in srcs]
    params = [p for _, p in MIXED]
    kws = [kw_of(p) for p in params]
    exp = [B.binarize(s, **(p or {})) for s, p in zip(srcs, params)]
    first = None
    for rep in range(10):
        pages, masks, infos = eng.binarize_batch(inputs, kws, mask=True, info=True)
        got = [(image_of(p), m, i) for p, m, i in zip(pages, masks, infos)]
        if first is None:
            first = got
            for i, g in enumerate(got):
                assert_same(g, exp[i], "batch page %d" % i)
                alone = eng.binarize(inputs[i], mask=True, info=True, **kws[i])
                assert alone[2] == g[2] and image_of(alone[0]).tobytes() == g[0].tobytes() and alone[1].tobytes() == g[1].tobytes(), "page %d alone" % i
        else:
            assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(got, first)), "repeat %d" % rep
    assert [image_of(p).tobytes() for p in eng.binarize_batch(inputs[:2], {"radius": 2})] == \
        [image_of(eng.binarize(i, radius=2)).tobytes() for i in inputs[:2]], "one parameter set for all"
    assert eng.binarize_batch([], None) == [] and eng.binarize_batch([], None, mask=True, info=True) == ([], [], [])
    with pytest.raises(ValueError):
        eng.binarize_batch(inputs, kws[:2])


def test_mask_alone_info_alone_and_neither(eng):
    src = noise(21, 70, 130, ink=0.3)
    inp = eng.input_from_grey(src)
    exp = B.binarize(src, radius=5, k_q8=100)
    kw = {"radius": 5, "k": 100 / 256.0}
    page = eng.binarize(inp, **kw)
    assert isinstance(page, OcrInput) and image_of(page).tobytes() == exp[0].tobytes()
    page, mask = eng.binarize(inp, mask=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and mask.tobytes() == exp[1].tobytes()
    page, info = eng.binarize(inp, info=True, **kw)
    assert image_of(page).tobytes() == exp[0].tobytes() and info == exp[2] and tuple(info) == B.INFO_KEYS
    assert image_of(eng.binarize(inp)).tobytes() == B.binarize(src)[0].tobytes(), "the defaults: k = 0.34 is k_q8 = 87"


def test_source_is_unchanged_and_outlives_the_result(eng):
    src = noise(99, 131, 70, ink=0.3)
    inp = eng.input_from_grey(src)
    exp = B.binarize(src, radius=4)[0]
    out = eng.binarize(inp, radius=4)
    assert image_of(inp).tobytes() == src.tobytes()
    del out   # ocrs_page_free of the result: the source is a page of its own
    assert image_of(inp).tobytes() == src.tobytes()
    out = eng.binarize(inp, radius=4)
    del inp   # ... and the other way round
    assert image_of(out).tobytes() == exp.tobytes()
    again = eng.binarize(out, radius=9)   # a binarised page is an ordinary page
    assert image_of(again).tobytes() == B.binarize(exp, radius=9)[0].tobytes()


def test_bad_parameters_have_their_status(eng):
    inp = eng.input_from_grey(noise(1, 20, 20))

    def refused(call):
        with pytest.raises(_lib.OcrsError) as e:
            call()
        assert e.value.status_name == "INVALID_ARGUMENT", e.value

    inf = float("inf")
    for kw in ({"radius": 0}, {"radius": 128}, {"radius": -1}, {"k": -0.01}, {"k": 1.01}, {"ink_level": inf}, {"ink_level": -inf},
               {"paper": inf}, {"paper": -inf}):
        refused(lambda: eng.binarize(inp, **kw))
    refused(lambda: eng.binarize_batch([inp, inp], [None, {"radius": 128}]))   # one bad page refuses the call
    live = _lib.pool_stats()["device_live"]
    pages = (C.c_void_p * 2)(inp._h, inp._h)
    nan = float("nan")
    for bad in (_lib.BinarizeParams(15, 257, 0, nan, nan), _lib.BinarizeParams(15, 87, 2, nan, nan), _lib.BinarizeParams(15, 87, 0, nan, inf)):
        ps = (_lib.BinarizeParams * 2)(_lib.BinarizeParams(15, 87, 0, nan, nan), bad)
        out = (C.c_void_p * 2)()
        masks = (C.POINTER(C.c_uint8) * 2)()
        assert _lib.lib().ocrs_engine_binarize_pages(eng._h, pages, C.c_size_t(2), ps, out, masks, None) == 1, "INVALID_ARGUMENT"
        assert [out[i] for i in range(2)] == [None, None] and not masks[0] and not masks[1], "a failed call writes nothing"
    assert _lib.pool_stats()["device_live"] == live, "nothing stays allocated"
    one = C.c_void_p()
    assert _lib.lib().ocrs_engine_binarize_page(eng._h, inp._h, None, None, None, None) == 1
    assert _lib.lib().ocrs_engine_binarize_page(eng._h, inp._h, None, C.byref(one), None, None) == 0, "NULL: the default"
    assert image_of(OcrInput(one)).tobytes() == image_of(eng.binarize(inp)).tobytes()   # (the OcrInput frees the page)
    wide = eng.input_from_grey(np.zeros((1, 65536), F))
    refused(lambda: eng.binarize(wide))


# ------------------------------------------------------------------ 2. composition
def test_despeckle_and_rule_removal_at_threshold_zero_use_the_local_decision(eng, text_pages):
    shaded = text_pages[1].copy()
    shaded[200:202, 30:480] = F(-0.45)   # a rule across the shade
    shaded[np.random.default_rng(4).random(shaded.shape) < 0.002] = F(-0.5)   # pepper
    exp = B.binarize(shaded)[0]
    page = eng.binarize(eng.input_from_grey(shaded))
    assert image_of(page).tobytes() == exp.tobytes()
    got = eng.despeckle(page, mask=True, info=True, threshold=0.0)
    want = D.despeckle(exp, threshold=0.0)
    assert got[2] == want[2] and got[2]["specks"] > 50 and image_of(got[0]).tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    got = eng.remove_rules(page, mask=True, info=True, threshold=0.0)
    want = R.remove_rules(exp, threshold=0.0)
    assert got[2] == want[2] and got[2]["h_removed"] > 400 and image_of(got[0]).tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def shaded_picture(seed, h, w, lines):
    """A synthetic page under the shade of §7.10, with pepper and a table grid, as a picture."""
    px = synth.synthetic_page(seed, h, w, lines=lines, columns=1)
    px[np.random.default_rng(seed).random((h, w)) < 0.003] = 0
    for r in range(20, h - 2, 90):
        px[r:r + 2, 10:w - 10] = 0
    for c in range(px.shape[2]):
        grey = px[:, :, c].astype(F) / F(255.0) - F(0.5)
        px[:, :, c] = np.clip(np.rint((B.shade(grey).astype(np.float64) + 0.5) * 255.0), 0, 255).astype(np.uint8)
    return px


def test_get_text_with_binarize_is_the_manual_chain(eng):
    inp = eng.prepare_input(ImageSource.from_tensor(shaded_picture(5, 600, 500, 24), DimOrder.Hwc))
    for params in (True, {"radius": 31, "k": 0.2, "keep_ink": True}):
        kw = {} if params is True else params
        ref_kw = {} if params is True else {"radius": 31, "k_q8": B.k_to_q8(0.2), "keep_ink": True}
        page, info = eng.binarize(inp, info=True, **kw)
        assert info["ink"] > 1000
        assert image_of(page).tobytes() == B.binarize(image_of(inp), **ref_kw)[0].tobytes()
        lines = eng.find_text_lines(page, eng.detect_words(page))
        text = "\n".join(str(t) for t in eng.recognize_text(page, lines) if t is not None)
        assert eng.get_text(inp, binarize=params) == text
        norm = eng.binarize(eng.normalize(inp), **kw)   # after normalisation ...
        assert eng.get_text(inp, binarize=params, normalize=True) == eng.get_text(norm)
        clean = eng.despeckle(norm)                      # ... before despeckling ...
        assert eng.get_text(inp, binarize=params, normalize=True, despeckle=True) == eng.get_text(clean)
        assert eng.get_text(inp, binarize=params, normalize=True, despeckle=True, rules=True) == eng.get_text(eng.remove_rules(clean))   # ... and rules
        assert eng.get_text(inp, binarize=params, rules={"min_length": 200}) == eng.get_text(eng.remove_rules(page, min_length=200))
    assert eng.get_text(inp, binarize=None) == eng.get_text(inp) == eng.get_text(inp, binarize=False)


def test_cli_binarize(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models
    px = shaded_picture(9, 700, 600, 30)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("cut", "tuned", "plain")}
    assert cli.main([path, "--binarize", "-j", "--debug", "-o", files["cut"]]) == 0
    assert cli.main([path, "--binarize", "--binarize-radius", "31", "--binarize-k", "0.2", "--binarize-keep-ink", "-j", "-o", files["tuned"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in (["--binarize-radius", "9"], ["--binarize-k", "0.1"], ["--binarize-keep-ink"], ["--binarize", "--binarize-radius", "128"],
                ["--binarize", "--binarize-k", "1.5"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def document(**kw):
        page, info = eng.binarize(inp, info=True, **kw)
        lines = eng.find_text_lines(page, eng.detect_words(page))
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(page, lines), binarize=info), info

    plain = output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "binarize" not in json.loads(plain), "without the flag nothing changes"
    exp, info = document()
    assert text["cut"] == exp and info["ink"] > 1000
    assert json.loads(text["cut"])["binarize"] == info and set(info) == set(B.INFO_KEYS)
    assert text["tuned"] == document(radius=31, k=0.2, keep_ink=True)[0]


# ------------------------------------------------------------------ 3. beside other callers
def test_binarising_callers_beside_plain_callers(eng):
    pxs = [synth.synthetic_page(30 + i, 300, 400, lines=12, columns=1) for i in range(4)]
    pages = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pxs]
    shaded = [B.shade(image_of(p)) for p in pages]
    inputs = [eng.input_from_grey(s) for s in shaded]
    params = [{}, {"radius": 127, "k_q8": 256}, {"radius": 2, "k_q8": 0, "keep_ink": True}, {"radius": 31, "paper": 0.25}]

    def cut(i):
        page, mask, info = eng.binarize(inputs[i], mask=True, info=True, **kw_of(params[i]))
        return image_of(page).tobytes(), mask.tobytes(), tuple(sorted(info.items()))

    def plain(i):
        return eng.detect_words(pages[i]).tobytes()

    quiet_cut, quiet_plain = [cut(i) for i in range(4)], [plain(i) for i in range(4)]
    for i in range(4):
        out, mask, info = B.binarize(shaded[i], **params[i])
        assert quiet_cut[i] == (out.tobytes(), mask.tobytes(), tuple(sorted(info.items())))
    results, errors = {}, []
    barrier = threading.Barrier(8)

    def worker(t):
        try:
            barrier.wait()
            for r in range(3):
                i = (t + r) % 4
                results[(t, r)] = (i, cut(i) if t < 4 else plain(i))
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
        assert got == (quiet_cut[i] if t < 4 else quiet_plain[i]), "thread %d call %d" % (t, r)
