"""Tiled detection on the GPU: the tiled entry points (ocrs_engine_detect_words[_batch]_tiled,
ocrs_engine_detect_text_pixels_tiled, ocrs_group_detect_words_batch_tiled) against the definition in numpy (tiled_ref.py)
driven by the CPU oracle's exact executor or by a Python callable, followed by detscore_ref.reference for rects, scores and
pixel counts.  Every comparison is bit for bit and nothing is filtered out of a comparison.

Run with:  python -m pytest tests -m gpu
"""
import json
import threading
import time

import numpy as np
import pytest

import detscore_ref as DR
import models_util as M
import stub_util
import tiled_ref as TR
from ocrs_amd import DimOrder, EngineGroup, ImageSource, Model, OcrEngine, _lib, synth
from oracle import clib
from oracle import pipeline as OP
from oracle.geometry import RotatedRect
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu

MIN_AREA = 100.0        # TextDetectorParams::default() (detection.rs:25-37), as the engine and the oracle have it
MODEL_HW = (800, 600)   # the detection model's input
V = TR.OVERLAP_DEFAULT

# (seed, height, width, lines, columns) of synth.synthetic_page
PAGE_2X2 = (11, 1400, 1100, 110, 2)
PAGE_1X4 = (12, 700, 2000, 50, 3)
PAGE_3X3 = (14, 2048, 1536, 150, 2)
PAGE_A4 = (13, 3508, 2480, 200, 2)     # 5 x 5 tiles
PAGE_BENCH = (0, 1024, 1024, 80, 2)    # 2 x 2; its seams fall between lines and into the gutter: exempt from the seam condition
PAGE_SMALL = (5, 400, 500, 30, 1)      # smaller than the model input both ways
PAGE_EXACT = (7, 800, 600, 40, 1)      # exactly the model input


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def assert_same(what, got, exp):
    """(rects, score, pixels) equal bit for bit; nothing is filtered out of the comparison."""
    gr, gs, gp = got
    er, es, ep = exp
    assert gr.shape == er.shape, "%s: %d words, expected %d" % (what, len(gr), len(er))
    assert np.ascontiguousarray(gr, np.float32).tobytes() == np.ascontiguousarray(er, np.float32).tobytes(), what + ": rects"
    assert gp.dtype == np.uint32 and np.array_equal(gp, ep), "%s: pixels differ at %s" % (what, np.flatnonzero(gp != ep)[:8])
    assert gs.dtype == np.float32 and np.array_equal(DR.bits(gs), DR.bits(es)), \
        "%s: scores differ at %s" % (what, np.flatnonzero(DR.bits(gs) != DR.bits(es))[:8])


def seam_crossers(P, thr, model_hw, v, min_pixels=100):
    """Components of at least min_pixels pixels with pixels on both sides of an ownership boundary.  Every one of them is a
    kept word: the min-area rect of n >= 100 pixel centres, grown by 2 * 3 pixels each way, covers those n unit squares, so
    its area is at least 100 = min_area.  The count is therefore a lower bound of the kept seam-crossing words.
    A connected component with pixels on both sides of the boundary before row b has pixels in rows b - 1 and b."""
    lab = DR.label8(clib.threshold(np.ascontiguousarray(P, np.float32), thr))
    size = np.bincount(lab[lab >= 0].ravel(), minlength=max(int(lab.max()) + 1, 1))
    oy, by, ox, bx = TR.page_plan(P.shape, model_hw, v)
    crossing = set()
    for b in by[1:-1]:
        crossing |= set(np.intersect1d(lab[b - 1], lab[b]).tolist())
    for b in bx[1:-1]:
        crossing |= set(np.intersect1d(lab[:, b - 1], lab[:, b]).tolist())
    return sum(1 for k in crossing if k >= 0 and size[k] >= min_pixels)


class Prod:
    def __init__(self):
        self.dbuf = M.detection_model_bytes()
        self.eng = OcrEngine(detection_model=Model.load_bytes(self.dbuf))
        assert tuple(Model.load_bytes(self.dbuf).input_shape()[2:]) == MODEL_HW
        self.ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(self.dbuf), "exact"))
        self.thr = float(self.eng.detection_threshold())
        assert self.thr == float(self.ora.detection_threshold())
        self._pages = {}

    def page(self, spec, keep=True):
        """-> (pixels, engine input, the reference's stitched map, the reference's (rects, score, pixels)): tiled_ref on
        the oracle's exact executor, then detscore_ref."""
        if spec in self._pages:
            return self._pages[spec]
        seed, h, w, lines, cols = spec
        px = synth.synthetic_page(seed, h, w, lines=lines, columns=cols)
        inp = self.eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
        oin = self.ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc"))
        assert np.asarray(oin, np.float32).tobytes() == inp.image().tobytes()
        t0 = time.time()
        P = TR.stitched(np.asarray(oin, np.float32)[0], TR.oracle_run_tile(self.ora.detector), MODEL_HW, V)
        t1 = time.time()
        ref = DR.reference(P, self.thr, MIN_AREA)
        print("%r: oracle tiles %.1f s, reference words %.1f s, %d kept words" % (spec, t1 - t0, time.time() - t1, len(ref[0])))
        out = (px, inp, P, ref)
        if keep:
            self._pages[spec] = out
        return out


@pytest.fixture(scope="module")
def prod():
    return Prod()


# ------------------------------------------------------------------ 1. indexing, with callable models
def callable_engine(model_hw, fn):
    calls = []

    def model(x):
        calls.append(x.reshape(model_hw).copy())
        return fn(x.reshape(model_hw)).reshape(1, 1, *model_hw)

    return OcrEngine(detection_model=Model.from_callable([1, 1, model_hw[0], model_hw[1]], model)), calls


def grey_page(eng, rng, h, w):
    inp = eng.prepare_input(ImageSource.from_tensor(rng.integers(0, 256, (h, w, 1)).astype(np.uint8), DimOrder.Hwc))
    return inp, inp.image()[0]


def index_cases(model_hw):
    """(page sizes, overlaps): a side <= the model, a side of M + 1 (two tiles that overlap in all but one pixel), every
    W % 4, many tiles both ways; overlaps 0, the maximum, the default where the model admits it."""
    hm, wm = model_hw
    sizes = [(hm, wm), (hm - 3, 3 * wm + 7), (hm + 1, wm), (hm, wm + 1), (hm + 1, wm + 1), (2 * hm + 5, wm // 2)]
    sizes += [(hm + 9, 4 * wm + k) for k in range(4)] + [(3 * hm + 2, 2 * wm + 3)]
    assert {w % 4 for _, w in sizes} == {0, 1, 2, 3}
    vmax = min(hm, wm) // 2
    return sizes, sorted({0, vmax, 5} | ({V} if V <= vmax else set()))


@pytest.mark.parametrize("model_hw", [(64, 48), (33, 47), (208, 256)], ids=["64x48", "33x47", "208x256"])
def test_identity_model_returns_the_page(model_hw):
    """x -> x + 0.5: the tiled map is grey + 0.5; the model is run ny * nx times, on the tile inputs of the definition, in
    tile order."""
    eng, calls = callable_engine(model_hw, lambda x: x + np.float32(0.5))
    rng = np.random.default_rng(model_hw[0])
    sizes, overlaps = index_cases(model_hw)
    assert (V in overlaps) == (model_hw == (208, 256))
    for h, w in sizes:
        inp, grey = grey_page(eng, rng, h, w)
        for v in overlaps:
            del calls[:]
            P = eng.detect_text_pixels(inp, tiled=v)
            exp_inputs = TR.tile_inputs(grey, model_hw, v)
            assert len(calls) == len(exp_inputs), (h, w, v, len(calls))
            for t, (a, b) in enumerate(zip(calls, exp_inputs)):
                assert a.tobytes() == b.tobytes(), "page %dx%d overlap %d: input of tile %d" % (h, w, v, t)
            assert P.dtype == np.float32 and P.tobytes() == (grey + np.float32(0.5)).tobytes(), (h, w, v)
    # tiled=True is the default overlap
    if V <= min(model_hw) // 2:
        inp, grey = grey_page(eng, rng, 2 * model_hw[0], 3 * model_hw[1] + 1)
        assert eng.detect_text_pixels(inp, tiled=True).tobytes() == eng.detect_text_pixels(inp, tiled=V).tobytes() == \
            (grey + np.float32(0.5)).tobytes()
    else:   # ... and is refused where the model does not admit it, as any overlap beyond half the shorter side is
        inp, _ = grey_page(eng, rng, 100, 100)
        for bad in (True, min(model_hw) // 2 + 1):
            with pytest.raises(_lib.OcrsError) as e:
                eng.detect_text_pixels(inp, tiled=bad)
            assert e.value.status_name == "INVALID_ARGUMENT"


@pytest.mark.parametrize("model_hw", [(64, 48), (33, 47)], ids=["64x48", "33x47"])
def test_position_model_decodes_to_the_plans_ownership(model_hw):
    """A model whose output encodes the tile-local position, (r * Wm + c) / 2^20 (exact in fp32): every page pixel carries
    the position it has in the tile that owns it."""
    hm, wm = model_hw
    code = ((np.arange(hm)[:, None] * wm + np.arange(wm)[None, :]).astype(np.float32) / np.float32(2 ** 20)).astype(np.float32)
    eng, calls = callable_engine(model_hw, lambda x: code)
    rng = np.random.default_rng(7)
    sizes, overlaps = index_cases(model_hw)
    for h, w in sizes:
        inp, _ = grey_page(eng, rng, h, w)
        for v in overlaps:
            P = eng.detect_text_pixels(inp, tiled=v)
            oy, by, ox, bx = TR.page_plan((h, w), model_hw, v)
            E = np.empty((h, w), np.float32)
            for i in range(len(oy)):
                for j in range(len(ox)):
                    E[by[i]:by[i + 1], bx[j]:bx[j + 1]] = code[by[i] - oy[i]:by[i + 1] - oy[i], bx[j] - ox[j]:bx[j + 1] - ox[j]]
            assert P.tobytes() == E.tobytes(), (h, w, v, np.argwhere(P != E)[:4])
            got = np.rint(P * np.float32(2 ** 20)).astype(np.int64)
            assert np.array_equal(got // wm + np.repeat(oy, np.diff(by))[:, None], np.broadcast_to(np.arange(h)[:, None], (h, w)))
            assert np.array_equal(got % wm + np.repeat(ox, np.diff(bx))[None, :], np.broadcast_to(np.arange(w)[None, :], (h, w)))


# ------------------------------------------------------------------ 2. the production detector against the oracle
@pytest.mark.parametrize("spec,tiles,min_crossers", [(PAGE_2X2, (2, 2), 10), (PAGE_1X4, (1, 4), 10), (PAGE_3X3, (3, 3), 10),
                                                     (PAGE_A4, (5, 5), 10), (PAGE_BENCH, (2, 2), 0)],
                         ids=["1400x1100", "700x2000", "2048x1536", "a4", "1024x1024"])
def test_production_detector_equals_the_oracle(prod, spec, tiles, min_crossers):
    px, inp, P, ref = prod.page(spec, keep=spec != PAGE_A4)
    oy, by, ox, bx = TR.page_plan(P.shape, MODEL_HW, V)
    assert (len(oy), len(ox)) == tiles
    # conditions on the input, asserted on the reference alone
    assert len(ref[0]) >= 50, "%r: %d kept words" % (spec, len(ref[0]))
    crossers = seam_crossers(P, prod.thr, MODEL_HW, V)
    print("%r: %d kept words, %d seam-crossing components of at least 100 pixels" % (spec, len(ref[0]), crossers))
    assert crossers >= min_crossers, "a wrong seam could pass"
    got_map = prod.eng.detect_text_pixels(inp, tiled=True)
    diff = np.argwhere(DR.bits(got_map) != DR.bits(P))
    assert len(diff) == 0, "%r: %d map pixels differ, first at %s" % (spec, len(diff), diff[:4])
    words = prod.eng.detect_words(inp, tiled=True)
    assert words.tobytes() == ref[0].tobytes() and words.shape == ref[0].shape, "%r: unscored rects" % (spec,)
    assert_same("%r scored" % (spec,), prod.eng.detect_words(inp, scores=True, tiled=True), ref)
    assert_same("%r scored, overlap given" % (spec,), prod.eng.detect_words(inp, scores=True, tiled=V), ref)


# ------------------------------------------------------------------ 3. a page no larger than the model input
@pytest.mark.parametrize("spec", [PAGE_SMALL, PAGE_EXACT], ids=["400x500", "800x600"])
def test_one_tile_page_equals_the_untiled_call(prod, spec):
    seed, h, w, lines, cols = spec
    inp = prod.eng.prepare_input(ImageSource.from_tensor(synth.synthetic_page(seed, h, w, lines=lines, columns=cols), DimOrder.Hwc))
    assert [len(a) for a in TR.page_plan((h, w), MODEL_HW, V)] == [1, 2, 1, 2]
    untiled = prod.eng.detect_words(inp, scores=True)
    assert len(untiled[0]) >= 25
    for v in (True, 0, 300):
        assert prod.eng.detect_text_pixels(inp, tiled=v).tobytes() == prod.eng.detect_text_pixels(inp).tobytes()
        assert_same("%r overlap %r" % (spec, v), prod.eng.detect_words(inp, scores=True, tiled=v), untiled)
        assert prod.eng.detect_words(inp, tiled=v).tobytes() == untiled[0].tobytes() == prod.eng.detect_words(inp).tobytes()


# ------------------------------------------------------------------ 4. batches, chunks, run to run
def test_batch_equals_each_page_alone_whatever_the_chunking(prod):
    specs = [PAGE_2X2, PAGE_1X4, PAGE_BENCH, PAGE_2X2, PAGE_SMALL]      # 4 + 4 + 4 + 4 + 1 = 17 tiles: two chunks of 16
    pages = [prod.page(s) for s in specs]
    inputs = [p[1] for p in pages]
    assert len({(s[1], s[2]) for s in specs}) == 4
    small_ref = prod.eng.detect_words(inputs[4], scores=True)
    refs = [p[3] for p in pages[:4]] + [small_ref]
    assert prod.eng.get_option("det_tile_batch") == 16
    try:
        for chunk in (16, 1, 5):
            prod.eng.set_option("det_tile_batch", chunk)
            words, score, pixels = prod.eng.detect_words_batch(inputs, scores=True, tiled=True)
            plain = prod.eng.detect_words_batch(inputs, tiled=True)
            for i, s in enumerate(specs):
                assert_same("det_tile_batch %d, batch page %d %r" % (chunk, i, s), (words[i], score[i], pixels[i]), refs[i])
                assert plain[i].tobytes() == refs[i][0].tobytes()
            assert prod.eng.detect_text_pixels(inputs[0], tiled=True).tobytes() == pages[0][2].tobytes()
    finally:
        prod.eng.set_option("det_tile_batch", 16)
    for bad in (0, 1025):
        with pytest.raises(_lib.OcrsError):
            prod.eng.set_option("det_tile_batch", bad)


def test_twenty_identical_runs(prod):
    specs = [PAGE_BENCH, PAGE_2X2]
    inputs = [prod.page(s)[1] for s in specs]
    first = prod.eng.detect_words_batch(inputs, scores=True, tiled=True)
    for i, s in enumerate(specs):
        assert_same("page %d" % i, (first[0][i], first[1][i], first[2][i]), prod.page(s)[3])
    first_map = prod.eng.detect_text_pixels(inputs[1], tiled=True)
    for run in range(19):
        again = prod.eng.detect_words_batch(inputs, scores=True, tiled=True)
        for i in range(len(specs)):
            assert again[0][i].tobytes() == first[0][i].tobytes(), (run, i)
            assert again[1][i].tobytes() == first[1][i].tobytes() and again[2][i].tobytes() == first[2][i].tobytes(), (run, i)
        assert prod.eng.detect_text_pixels(inputs[1], tiled=True).tobytes() == first_map.tobytes(), run


# ------------------------------------------------------------------ 5. the overflow re-run, in tiled form
@pytest.mark.parametrize("w", [704, 702], ids=["quad", "byte"])
def test_salt_noise_takes_the_overflow_rerun(w):
    """A page of salt noise on a stride-2 lattice (more than 65 536 components) under the model x -> x + 0.5, whose tiled
    map is the page itself: the component stage does not fit its first-pass buffers and is re-run."""
    h, model_hw, v = 512, (200, 256), 40
    rng = np.random.default_rng(w)
    px = np.zeros((h, w), np.uint8)
    ys, xs = np.meshgrid(np.arange(0, h, 2), np.arange(0, w, 2), indexing="ij")
    px[ys, xs] = rng.integers(64, 256, ys.shape)
    px[200:240, :] = 0
    n_salt = int((px > 0).sum())
    for k in range(6):
        px[210:224, 20 + 60 * k:20 + 60 * k + 16] = 80 + 25 * k
        px[212:214, 50 + 60 * k:52 + 60 * k] = 230
    fn = lambda x: x + np.float32(0.5)   # noqa: E731
    eng, calls = callable_engine(model_hw, fn)
    inp = eng.prepare_input(ImageSource.from_tensor(px[:, :, None], DimOrder.Hwc))
    grey = inp.image()[0]
    P = TR.stitched(grey, fn, model_hw, v)
    assert P.tobytes() == (grey + np.float32(0.5)).tobytes() and ((P > 0.2) == (px > 51)).all()
    ref = DR.reference(P, 0.2, MIN_AREA, count=True)
    assert ref[3] == n_salt + 12 > 65536, "more components than the first pass has room for"
    assert len(ref[0]) == 6
    got = eng.detect_words(inp, scores=True, tiled=v)
    plain = eng.detect_words(inp, tiled=v)
    ny, nx = len(TR.axis_plan(h, model_hw[0], v)[0]), len(TR.axis_plan(w, model_hw[1], v)[0])
    assert (ny, nx) == (3, 4) and len(calls) == 2 * ny * nx
    assert eng.detect_text_pixels(inp, tiled=v).tobytes() == P.tobytes()
    assert_same("salt noise, w = %d" % w, got, ref[:3])
    assert plain.tobytes() == got[0].tobytes()
    assert got[2].tolist() == [14 * 16] * 6


# ------------------------------------------------------------------ 6. untiled callers beside tiled traffic
def test_untiled_callers_keep_their_solo_bits_beside_tiled_requests(prod):
    eng = OcrEngine(detection_model=Model.load_bytes(prod.dbuf))
    specs = [PAGE_BENCH, PAGE_SMALL, PAGE_2X2]
    inputs = [eng.prepare_input(ImageSource.from_tensor(prod.page(s)[0] if s != PAGE_SMALL else
                                                        synth.synthetic_page(5, 400, 500, lines=30, columns=1), DimOrder.Hwc))
              for s in specs]
    solo = [eng.detect_words(i, scores=True) for i in inputs]
    solo_plain = [eng.detect_words(i) for i in inputs]
    solo_tiled = [eng.detect_words(i, scores=True, tiled=True) for i in inputs]
    assert_same("tiled solo", solo_tiled[0], prod.page(PAGE_BENCH)[3])
    assert_same("tiled solo", solo_tiled[2], prod.page(PAGE_2X2)[3])
    for i in range(len(inputs)):
        assert solo_plain[i].tobytes() == solo[i][0].tobytes()
    base = eng.coalesce_stats()["detect"]
    bad, n_untiled, n_tiled = [], [0] * 5, [0] * 5
    gate = threading.Barrier(5)
    deadline = [0.0]

    def worker(k):
        gate.wait()
        if k == 0:
            deadline[0] = time.time() + 3.0
        it = 0
        while it < 4 or time.time() < deadline[0]:
            j = (it * 2 + k) % len(inputs)
            if k >= 3:                      # two threads of tiled requests, scored and unscored
                if it % 2:
                    got = eng.detect_words(inputs[j], scores=True, tiled=True)
                    ok = all(a.tobytes() == b.tobytes() for a, b in zip(got, solo_tiled[j]))
                else:
                    ok = eng.detect_words(inputs[j], tiled=True).tobytes() == solo_tiled[j][0].tobytes()
                n_tiled[k] += 1
            else:                           # three threads of untiled one-page requests: these go through the coalescer
                if (it + k) % 2:
                    got = eng.detect_words(inputs[j], scores=True)
                    ok = all(a.tobytes() == b.tobytes() for a, b in zip(got, solo[j]))
                else:
                    ok = eng.detect_words(inputs[j]).tobytes() == solo_plain[j].tobytes()
                n_untiled[k] += 1
            if not ok:
                bad.append((k, it, j))
            it += 1

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(5)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not bad, bad[:8]
    merged = eng.coalesce_stats()["detect"]
    batches, requests = merged[0] - base[0], merged[1] - base[1]
    print("coalescer: %d untiled requests in %d batches beside %d tiled requests" % (requests, batches, sum(n_tiled)))
    assert sum(n_tiled) >= 8 and sum(n_untiled) >= 12
    assert requests == sum(n_untiled), "the coalescer saw every untiled request and no tiled one"
    assert 1 <= batches <= requests


# ------------------------------------------------------------------ 7. an engine group
@pytest.mark.parametrize("gather", ["host", "rccl"])
def test_group_equals_single_engine(prod, gather, monkeypatch):
    if gather == "rccl":   # the librccl test double (tests/stubs): the device-to-device transport carries the same payload
        monkeypatch.setenv("OCRS_RCCL_LIB", stub_util.rccl_stub_path())
    group = EngineGroup([0, 0], prod.dbuf, None, gather=gather, shared_block=2)
    pages = [synth.synthetic_page(60 + s, 1400, 1100, lines=110, columns=2) for s in range(5)] + [prod.page(PAGE_2X2)[0]]   # one size per group call
    inputs = group.prepare_input_batch(pages)
    words, score, pixels = group.detect_words_batch(inputs, scores=True, tiled=True)
    assert group.last_gather()["transport"] == gather
    plain = group.detect_words_batch(inputs, tiled=V)
    singles = [prod.eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pages]
    ew, es, ep = prod.eng.detect_words_batch(singles, scores=True, tiled=True)
    assert sum(len(x) for x in ew) >= 50 * len(pages)
    for i in range(len(pages)):
        assert_same("group page %d" % i, (words[i], score[i], pixels[i]), (ew[i], es[i], ep[i]))
        assert plain[i].tobytes() == ew[i].tobytes()
    assert_same("group page 5 against the definition", (words[5], score[5], pixels[5]), prod.page(PAGE_2X2)[3])
    untiled = group.detect_words_batch(inputs)
    assert untiled[0].tobytes() == prod.eng.detect_words(singles[0]).tobytes() != ew[0].tobytes()


# ------------------------------------------------------------------ 8. end to end, and the CLI
def test_tiled_words_through_layout_and_recognition(prod):
    rbuf = M.recognition_model_bytes()
    gpu = OcrEngine(detection_model=Model.load_bytes(prod.dbuf), recognition_model=Model.load_bytes(rbuf))
    ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(prod.dbuf), "exact"),
                       recognition_model=OracleModel(OracleGraph(rbuf), "exact"))
    px, _, _, ref = prod.page(PAGE_3X3)
    inp = gpu.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    oin = ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc"))
    words = gpu.detect_words(inp, tiled=True)
    assert words.tobytes() == ref[0].tobytes()
    owords = [RotatedRect.from_array(r) for r in ref[0]]      # the oracle pipeline, fed the reference's tiled words
    lines = gpu.find_text_lines(inp, words)
    olines = ora.find_text_lines(oin, owords)
    assert len(lines) == len(olines) > 100
    for a, b in zip(lines, olines):
        assert np.array_equal(a, np.array([w.to_array() for w in b], np.float32).reshape(-1, 6))
    got = gpu.recognize_text(inp, lines)
    exp = ora.recognize_text(oin, olines)
    assert len(got) == len(exp)
    n_chars = 0
    for g, e in zip(got, exp):
        assert (g is None) == (e is None)
        if g is None:
            continue
        assert str(g) == str(e)
        assert [c.rect for c in g.chars()] == [c.rect.tlbr() for c in e.chars]
        n_chars += len(e.chars)
    assert n_chars > 500


def test_cli_tiled(tmp_path, monkeypatch):
    from PIL import Image

    from ocrs_amd import cli, models, output
    px = synth.synthetic_page(9, 900, 700, lines=40, columns=1)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("tiled", "overlap", "plain", "cut")}
    assert cli.main([path, "--tiled", "-j", "--detection-confidence", "--text-map", "--text-mask", "-o", files["tiled"]]) == 0
    assert cli.main([path, "-j", "--detection-confidence", "--tiled", "60", "-o", files["overlap"]]) == 0
    assert cli.main([path, "-j", "--detection-confidence", "-o", files["plain"]]) == 0
    text = {k: open(files[k], encoding="utf-8").read() for k in ("tiled", "overlap", "plain")}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))

    def document(tiled, min_score=None):
        words, score, pixels = eng.detect_words(inp, scores=True, tiled=tiled)
        if min_score is not None:
            keep = score >= np.float32(min_score)
            words, score, pixels = words[keep], score[keep], pixels[keep]
        lines, index = eng.find_text_lines(inp, words, index=True)
        boxes = [[(words[k], score[k], pixels[k]) for k in idx] for idx in index]
        return output.format_json_output(path, px.shape[:2], eng.recognize_text(inp, lines), word_boxes=boxes), score

    assert document(True)[0] == text["tiled"] and document(60)[0] == text["overlap"] and document(False)[0] == text["plain"]
    assert text["tiled"] != text["plain"] and len(json.loads(text["tiled"])["paragraphs"][0]["lines"]) > 10
    # --tiled governs --text-map / --text-mask: the stitched map, written as the reference writes its maps
    P = eng.detect_text_pixels(inp, tiled=True)
    assert P.tobytes() != eng.detect_text_pixels(inp).tobytes()
    want = (np.clip(P, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "text-map.png"))), want)
    mask = np.asarray(Image.open(str(tmp_path / "text-mask.png")))
    assert np.array_equal(mask > 0, P > np.float32(eng.detection_threshold()))
    # ... and combines with --min-word-score
    score = document(True)[1]
    cut = float(np.sort(score)[len(score) // 3])
    assert cli.main([path, "-j", "--detection-confidence", "--tiled", "--min-word-score", repr(cut), "-o", files["cut"]]) == 0
    assert document(True, cut)[0] == open(files["cut"], encoding="utf-8").read()
