"""The stream plan of a device on the GPU (option "stream_budget", ocrs_amd/csrc/stream_plan.hpp): calls that
share lanes, wait for the conv and recurrence lanes on the host and split their long lines onto a second lane give the
bytes of the same requests run one at a time on one thread with a stream per call (budget 0), at every budget.

Every comparison is byte equality of word rects, line grouping, characters and character boxes.  Pages are small
(512 x 512, six lines) so that a case takes a second or two; the lanes, the host waits and the plan's accounting do not
depend on the size of a request.

The request that is refused mid-pipeline is one whose recognition model has 700 classes: the LogSoftmax kernel refuses it
with OCRS_ERR_CAPACITY after the request's conv stack and recurrences have been queued on the shared lanes.  (Forcing
"rec_max_pixels" below one line refuses nothing: a sub-request always holds at least one line and a line is refused only
beyond the fixed 2e9-pixel memory budget, ocrs_engine::recognize_now / recognize_lines.)
"""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import models_util as M
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, synth
from ocrs_amd import modelfile as mf

pytestmark = pytest.mark.gpu
BUDGETS = (0, 3, 4, 8)
N_PAGES = 6


def _batch(engine, pages):
    """one request of several pages through the batch entry points -> everything it returns, as arrays"""
    inputs = [engine.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pages]
    words = engine.detect_words_batch(inputs)
    rects, loffs, poffs = engine.find_text_lines_batch_raw(words)
    chars, coffs = engine.recognize_text_batch_raw(inputs, rects, loffs, poffs)
    return [np.asarray(w) for w in words] + [rects, loffs, poffs, chars, coffs]


def _one_page(engine, page):
    """the reference's call pattern: one page per call"""
    inp = engine.prepare_input(ImageSource.from_tensor(page, DimOrder.Hwc))
    words = engine.detect_words(inp)
    lines = engine.find_text_lines(inp, words)
    text = [(str(t), [c.rect for c in t.chars()]) if t else None for t in engine.recognize_text(inp, lines)]
    return np.asarray(words), [np.asarray(l) for l in lines], text


def _same(got, exp):
    if isinstance(exp, np.ndarray):
        return isinstance(got, np.ndarray) and got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()
    if isinstance(exp, (list, tuple)):
        return len(got) == len(exp) and all(_same(g, e) for g, e in zip(got, exp))
    return got == exp


def _split_request():
    """64 lines 200 wide (T = 50) and two 760 wide (T = 190 > T_SPLIT = 160) on one page, one line per 64-pixel row: the
    request that recognize_packed splits into a long and a short batch"""
    crops = synth.synthetic_line_crops(77, n=70) + 0.5
    n, w = 66, 768
    page = np.ones((1, n * 64, w), np.float32)
    rects = np.zeros((n, 6), np.float32)
    for i in range(n):
        lw = 200 if i < 64 else 760
        strip = np.concatenate([crops[i], crops[(i + 1) % 70], crops[(i + 2) % 70]], axis=1)[:, :lw]
        page[0, i * 64:(i + 1) * 64, :lw] = strip
        rects[i] = (lw / 2.0, i * 64.0 + 32.0, 0.0, 1.0, float(lw), 64.0)
    return page, rects


def _run_split(engine, inp, rects):
    n = len(rects)
    chars, coffs = engine.recognize_text_batch_raw([inp], rects, np.arange(n + 1, dtype=np.uintp), np.array([0, n], dtype=np.uintp))
    return [chars, coffs]


@pytest.fixture(scope="module")
def rig():
    """engine, pages and the reference: every request of this file run once, one at a time on this thread, at budget 0"""
    _lib.require_gpu()
    dbuf, rbuf = M.detection_model_bytes(), M.recognition_model_bytes()

    class Rig:
        pass
    r = Rig()
    r.dbuf, r.rbuf = dbuf, rbuf
    r.engine = OcrEngine(detection_model=Model.load_bytes(dbuf), recognition_model=Model.load_bytes(rbuf))
    r.pages = [synth.synthetic_page(s, 512, 512, lines=6) for s in range(N_PAGES)]
    r.split_page, r.split_rects = _split_request()
    _lib.set_option("stream_budget", 0)
    try:
        r.pairs = [(a, (a + 1) % N_PAGES) for a in range(N_PAGES)]
        r.ref_pairs = [_batch(r.engine, [r.pages[a], r.pages[b]]) for a, b in r.pairs]
        r.ref_one = [_one_page(r.engine, p) for p in r.pages]
        r.ref_grey = [r.engine.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)).image() for p in r.pages]
        r.split_inp = r.engine.prepare_input(ImageSource.from_tensor(r.split_page, DimOrder.Chw))
        r.ref_split = _run_split(r.engine, r.split_inp, r.split_rects)
    finally:
        _lib.set_option("stream_budget", 4)
    print("reference: lines per two-page request %s, characters %s; lines with text per page %s; split request characters %d"
          % ([len(x[3]) - 1 for x in r.ref_pairs], [len(x[-2]) for x in r.ref_pairs], [sum(1 for t in x[2] if t) for x in r.ref_one],
             len(r.ref_split[0])))
    assert all(len(x[3]) - 1 >= 2 and len(x[-2]) >= 2 for x in r.ref_pairs)          # lines and characters were found
    assert all(sum(1 for t in x[2] if t) >= 1 for x in r.ref_one)
    assert len(r.ref_split[0]) >= 66
    return r


@pytest.fixture(params=BUDGETS)
def budget(request, rig):
    _lib.set_option("stream_budget", request.param)
    yield request.param
    _lib.set_option("stream_budget", 4)


def test_three_threads_of_two_page_requests_beside_a_thread_of_prepare_input(rig, budget):
    stop = threading.Event()
    bad_grey = []

    def uploader():
        k = 0
        while not stop.is_set():
            got = rig.engine.prepare_input(ImageSource.from_tensor(rig.pages[k % N_PAGES], DimOrder.Hwc)).image()
            if not _same(got, rig.ref_grey[k % N_PAGES]):
                bad_grey.append(k)
            k += 1
        return k

    def requests(t):
        out = []
        for j in range(4):
            i = (4 * t + j) % N_PAGES
            a, b = rig.pairs[i]
            out.append((i, _batch(rig.engine, [rig.pages[a], rig.pages[b]])))
        return out

    with ThreadPoolExecutor(max_workers=4) as ex:
        up = ex.submit(uploader)
        try:
            outs = list(ex.map(requests, range(3)))
        finally:
            stop.set()
        assert up.result() >= 1 and not bad_grey
    for per_thread in outs:
        assert len(per_thread) == 4
        for i, got in per_thread:
            assert _same(got, rig.ref_pairs[i]), (budget, i)


def test_six_threads_of_one_page_calls_with_the_coalescer_on(rig, budget):
    s0 = rig.engine.coalesce_stats()
    with ThreadPoolExecutor(max_workers=6) as ex:
        outs = list(ex.map(lambda k: (k % N_PAGES, _one_page(rig.engine, rig.pages[k % N_PAGES])), range(24)))
    s1 = rig.engine.coalesce_stats()
    assert s1["detect"][1] - s0["detect"][1] == 24 and s1["recognize"][1] - s0["recognize"][1] == 24   # all went through the queues
    for pi, got in outs:
        assert _same(got, rig.ref_one[pi]), (budget, pi)


def test_long_and_short_lines_split_onto_two_lanes(rig, budget):
    assert _same(_run_split(rig.engine, rig.split_inp, rig.split_rects), rig.ref_split), budget
    # and beside other requests (the long batch then has a host thread of its own)
    with ThreadPoolExecutor(max_workers=3) as ex:
        f = [ex.submit(_run_split, rig.engine, rig.split_inp, rig.split_rects), ex.submit(_one_page, rig.engine, rig.pages[0]),
             ex.submit(_run_split, rig.engine, rig.split_inp, rig.split_rects)]
        got = [x.result() for x in f]
    assert _same(got[0], rig.ref_split) and _same(got[2], rig.ref_split) and _same(got[1], rig.ref_one[0]), budget


def test_an_exact_and_a_relaxed_engine_alive_together(rig, budget):
    assert _lib.isolation()["mode"] == "free"
    relaxed = OcrEngine(detection_model=Model.load_bytes(rig.dbuf), recognition_model=Model.load_bytes(rig.rbuf), numerics="relaxed")
    try:
        assert _lib.isolation()["mode"] == "serial"          # the one-stream regime, whatever the budget
        with ThreadPoolExecutor(max_workers=3) as ex:
            f = [ex.submit(_one_page, rig.engine, rig.pages[k]) for k in range(3)] + [ex.submit(_one_page, relaxed, rig.pages[3])]
            got = [x.result() for x in f]
        for k in range(3):
            assert _same(got[k], rig.ref_one[k]), (budget, k)
        assert sum(1 for t in got[3][2] if t) >= 1
    finally:
        del relaxed                                          # the last such engine goes: the regime switch drains the device
    assert _lib.isolation()["mode"] == "free"
    with ThreadPoolExecutor(max_workers=3) as ex:
        got = list(ex.map(lambda k: _one_page(rig.engine, rig.pages[k]), range(3)))
    for k in range(3):
        assert _same(got[k], rig.ref_one[k]), (budget, k)


def test_a_request_refused_mid_pipeline_and_then_a_request_on_every_lane(rig, budget):
    n_classes = 700    # the LogSoftmax kernel stages at most ~630 classes
    big = mf.build_recognition(n_classes=n_classes, seed=5).to_bytes()
    eng = OcrEngine(detection_model=Model.load_bytes(rig.dbuf), recognition_model=Model.load_bytes(big),
                    alphabet="".join(chr(0x4E00 + i) for i in range(n_classes - 1)))

    def refused(k):
        inp = eng.prepare_input(ImageSource.from_tensor(rig.pages[k], DimOrder.Hwc))
        lines = eng.find_text_lines(inp, eng.detect_words(inp))
        assert len(lines) >= 1
        with pytest.raises(_lib.OcrsError) as e:
            eng.recognize_text(inp, lines)
        return e.value.status_name

    assert refused(0) == "CAPACITY"
    # beside good requests, then one good request per lane of the plan (and a few more): the refused request's scratch
    # went back to the pool only after its queued kernels, and no lane is left waiting for anything
    with ThreadPoolExecutor(max_workers=4) as ex:
        f = [ex.submit(refused, 1)] + [ex.submit(_one_page, rig.engine, rig.pages[k]) for k in range(3)]
        got = [x.result() for x in f]
    assert got[0] == "CAPACITY"
    for k in range(3):
        assert _same(got[1 + k], rig.ref_one[k]), (budget, k)
    lanes = max(1, budget - 2) if budget else 4
    with ThreadPoolExecutor(max_workers=lanes) as ex:
        got = list(ex.map(lambda k: _one_page(rig.engine, rig.pages[k % N_PAGES]), range(2 * lanes)))
    for k, g in enumerate(got):
        assert _same(g, rig.ref_one[k % N_PAGES]), (budget, k)


def test_the_budget_cannot_change_under_a_request_and_not_for_one_engine(rig):
    with pytest.raises(_lib.OcrsError, match="devices, not to an engine"):
        rig.engine.set_option("stream_budget", 8)
    refused = []
    stop = threading.Event()

    def requests():
        while not stop.is_set():
            _one_page(rig.engine, rig.pages[0])

    t = threading.Thread(target=requests)
    t.start()
    try:
        for _ in range(200):      # a request is in flight nearly all the time: most of these meet one
            try:
                _lib.set_option("stream_budget", 8)
                _lib.set_option("stream_budget", 4)
            except _lib.OcrsError as e:
                assert e.status_name == "INVALID_ARGUMENT" and "in flight" in str(e)
                refused.append(1)
    finally:
        stop.set()
        t.join()
        _lib.set_option("stream_budget", 4)
    assert refused


@pytest.fixture(scope="module")
def pixels():
    rng = np.random.default_rng(11)
    u8 = rng.integers(0, 256, 5 * 1024 * 1024 * 4, dtype=np.uint8)
    return {np.uint8: u8, np.float32: (u8.astype(np.float32) / np.float32(255.0))}


@pytest.mark.parametrize("budget_", BUDGETS)
def test_batched_prepare_input_equals_the_per_page_kernels(rig, pixels, budget_):
    _lib.set_option("stream_budget", budget_)
    try:
        for dtype in (np.uint8, np.float32):
            for order in (DimOrder.Hwc, DimOrder.Chw):
                for c in (1, 3, 4):
                    for h, w in ((97, 211), (1024, 1024)):
                        imgs = []
                        for i in range(5):
                            flat = pixels[dtype][i * h * w * c:(i + 1) * h * w * c]
                            imgs.append(np.ascontiguousarray(flat.reshape((h, w, c) if order == DimOrder.Hwc else (c, h, w))))
                        single = [rig.engine.prepare_input(ImageSource.from_tensor(im, order)).image() for im in imgs]
                        for n in (1, 2, 5):
                            got = rig.engine.prepare_input_batch_raw([im.ctypes.data for im in imgs[:n]], dtype, order, h, w, c)
                            assert len(got) == n
                            for i in range(n):
                                assert np.array_equal(got[i].image(), single[i]), (budget_, dtype, order, c, h, w, n, i)
    finally:
        _lib.set_option("stream_budget", 4)
