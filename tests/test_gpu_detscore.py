"""Detection confidence on the GPU: per-word scores and pixel counts of the scored entry points
(ocrs_engine_detect_words[_batch]_scored, ocrs_group_detect_words_batch_scored) against the definition in numpy
(detscore_ref.py), bit for bit — `score` as a float32 bit pattern — through every route a detection request takes: the
four-pixel and the one-pixel kernels, pages smaller than the model input, batches of mixed sizes, the overflow re-run,
the coalescer, an engine group, a caller-implemented (`trait Model`) detection model that serves crafted maps, and the
CLI.  Scoring must not change anybody's rects, and an unscored request must launch what it launched before.

Run with:  python -m pytest tests -m gpu
"""
import json
import threading

import numpy as np
import pytest

import detscore_ref as DR
import models_util as M
import stub_util
from ocrs_amd import DimOrder, EngineGroup, ImageSource, Model, OcrEngine, _lib, synth
from oracle import pipeline as OP
from oracle.nn import OracleGraph, OracleModel

pytestmark = pytest.mark.gpu

MIN_AREA = 100.0   # TextDetectorParams::default() (detection.rs:25-37), as the engine and the oracle have it

# (seed, height, width, lines, columns) of the synthetic pages; each has at least 50 kept words (asserted on the reference)
PAGE_1024_A = (0, 1024, 1024, 80, 2)
PAGE_1024_B = (1, 1024, 1024, 80, 2)
PAGE_W1022 = (3, 700, 1022, 60, 2)     # width % 4 == 2: the one-pixel (byte) kernels
PAGE_W1023 = (4, 1000, 1023, 60, 2)    # odd width
PAGE_SMALL = (5, 400, 500, 30, 1)      # smaller than the 800 x 600 model input both ways
PAGE_MID = (6, 640, 768, 50, 2)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


class Prod:
    def __init__(self):
        self.dbuf = M.detection_model_bytes()
        self.eng = OcrEngine(detection_model=Model.load_bytes(self.dbuf))
        self.ora = OP.OcrEngine(detection_model=OracleModel(OracleGraph(self.dbuf), "exact"))
        self.thr = float(self.eng.detection_threshold())
        self._pages = {}

    def page(self, spec):
        """-> (pixels, engine input, reference (rects, score, pixels) on the engine's own map).  The reference on the
        ORACLE's map is checked to be the same the first time a page is used."""
        if spec not in self._pages:
            seed, h, w, lines, cols = spec
            px = synth.synthetic_page(seed, h, w, lines=lines, columns=cols)
            inp = self.eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
            P = self.eng.detect_text_pixels(inp)
            ref = DR.reference(P, self.thr, MIN_AREA)
            assert len(ref[0]) >= 50, "%r: %d kept words" % (spec, len(ref[0]))
            oin = self.ora.prepare_input(OP.ImageSource.from_tensor(px, "hwc"))
            PO = np.asarray(self.ora.detect_text_pixels(oin), np.float32).reshape(h, w)
            oref = ref if PO.tobytes() == P.tobytes() else DR.reference(PO, float(self.ora.detection_threshold()), MIN_AREA)
            assert len(oref[0]) >= 50
            assert_same("%r: engine map against oracle map" % (spec,), ref, oref)
            self._pages[spec] = (px, inp, ref)
        return self._pages[spec]


@pytest.fixture(scope="module")
def prod():
    return Prod()


def assert_same(what, got, exp):
    """(rects, score, pixels) equal bit for bit; nothing is filtered out of the comparison."""
    gr, gs, gp = got
    er, es, ep = exp
    assert gr.shape == er.shape, "%s: %d words, expected %d" % (what, len(gr), len(er))
    assert np.ascontiguousarray(gr, np.float32).tobytes() == np.ascontiguousarray(er, np.float32).tobytes(), what + ": rects"
    assert gp.dtype == np.uint32 and np.array_equal(gp, ep), "%s: pixels differ at %s" % (what, np.flatnonzero(gp != ep)[:8])
    assert gs.dtype == np.float32 and np.array_equal(DR.bits(gs), DR.bits(es)), \
        "%s: scores differ at %s" % (what, np.flatnonzero(DR.bits(gs) != DR.bits(es))[:8])


# ------------------------------------------------------------------ 1. against the definition
@pytest.mark.parametrize("spec", [PAGE_1024_A, PAGE_1024_B, PAGE_W1022, PAGE_W1023, PAGE_SMALL],
                         ids=["1024a", "1024b", "w1022", "w1023", "small"])
def test_scores_match_the_definition(prod, spec):
    px, inp, ref = prod.page(spec)
    got = prod.eng.detect_words(inp, scores=True)
    print("%r: %d words, score %.4f..%.4f, pixels %d..%d" % (spec, len(got[0]), got[1].min(), got[1].max(), got[2].min(), got[2].max()))
    assert_same(repr(spec), got, ref)
    assert (got[1] > 0).all() and (got[1] <= 1).all() and (got[2] > 0).all()


def test_batch_of_three_page_sizes(prod):
    specs = [PAGE_1024_A, PAGE_W1022, PAGE_SMALL, PAGE_1024_B, PAGE_W1022]
    pages = [prod.page(s) for s in specs]
    words, score, pixels = prod.eng.detect_words_batch([p[1] for p in pages], scores=True)
    assert len({(s[1], s[2]) for s in specs}) == 3
    for i, (spec, p) in enumerate(zip(specs, pages)):
        assert_same("batch page %d %r" % (i, spec), (words[i], score[i], pixels[i]), p[2])


# ------------------------------------------------------------------ 2. crafted maps through a `trait Model` detection model
def crafted_shapes(w):
    """A 160 x w map (w >= 2304) and what it was built to hold: (the model's map, the page map it becomes, external
    components, kept words).
    Row 80 and column 1200 carry a one-pixel cross that touches all four edges."""
    h = 160
    P = np.zeros((h, w), np.float32)
    ext = kept = 0

    def blob(y, x, hh, ww, v):
        P[y:y + hh, x:x + ww] = v

    # the cross: one component, one word
    P[80, :] = 0.5
    P[:, 1200] = 0.625
    ext += 1; kept += 1
    # nested rings and an island: only the outer ring is External
    blob(10, 10, 40, 40, 0.5); blob(14, 14, 32, 32, 0.0)
    blob(20, 20, 20, 20, 0.9375); blob(23, 23, 14, 14, 0.0)
    blob(27, 27, 6, 6, 0.75)
    ext += 1; kept += 1
    # a ring across the 2 048-pixel block boundary with a kept-size island in its hole
    blob(10, 2020, 50, 60, 0.25); blob(15, 2025, 40, 50, 0.0); blob(22, 2036, 20, 20, 0.8125)
    ext += 1; kept += 1
    # components at the four corners and on the edges (top and left ones start at pixel 0, the right one ends at w - 1)
    blob(0, 0, 8, 8, 0.3125); blob(0, w - 14, 12, 14, 0.4375); blob(h - 12, 0, 12, 16, 0.5625); blob(h - 10, w - 12, 10, 12, 0.6875)
    blob(0, 600, 12, 12, 0.75); blob(h - 12, 600, 12, 12, 0.75); blob(100, 0, 12, 12, 0.75); blob(100, w - 12, 12, 12, 0.75)
    ext += 8; kept += 8
    # one-pixel lines: vertical, diagonal and anti-diagonal across the 256- and 1 024-pixel boundaries
    P[90:130, 300] = 0.40625
    for i in range(40):
        P[10 + i, 240 + i] = 0.28125 + i / 256.0       # crosses x = 255 | 256
        P[10 + i, 1010 + i] = 0.46875                  # crosses x = 1023 | 1024
        P[90 + i, 780 - i] = 0.34375                   # crosses x = 768 | 767
    ext += 4; kept += 4
    # diagonal-only contacts across the boundaries: two 12 x 12 squares sharing a corner are ONE component
    for bx in (256, 576, 1024):
        blob(100, bx - 12, 12, 12, 0.5); blob(112, bx, 12, 12, 0.25)
        ext += 1; kept += 1
    blob(130, 1536, 12, 12, 0.5); blob(142, 1524, 12, 12, 0.25)      # anti-diagonal contact
    ext += 1; kept += 1
    # specks below min_area between kept components (alignment after the compaction by valid[])
    for k in range(12):
        blob(20, 1300 + 40 * k, 12, 14, 0.3 + k / 32.0)
        blob(22, 1300 + 40 * k + 20, 3, 3, 0.9)
        ext += 2; kept += 1
    blob(140, 1300, 2, 2, 0.95); blob(140, 1310, 1, 5, 0.95)
    ext += 2
    # exactly 1.0, above 1, and isolated +inf pixels, each with three NaN neighbours (NaN is not text: holes).  A page of the
    # model's size takes the model's map as it is (a same-size resize is a copy): +inf and NaN come back
    # where the model put them, and nowhere else
    blob(100, 1400, 12, 12, 1.0); blob(100, 1440, 12, 12, 1.5); blob(100, 1480, 12, 12, 0.75)
    P[101:111:3, 1481:1491:3] = np.inf
    for y, x in zip(*np.nonzero(np.isinf(P))):
        P[y - 1, x] = P[y, x - 1] = P[y - 1, x - 1] = np.nan
    blob(100, 1520, 12, 12, 1.0); P[104:108, 1524:1528] = 3.0
    ext += 4; kept += 4
    return P, P.copy(), ext, kept


def crafted_salt(w):
    """A 512 x w map of salt noise on a stride-2 lattice (more than 65 536 components: the overflow re-run) with a
    noise-free band holding kept blobs and specks."""
    h = 512
    rng = np.random.default_rng(w)
    P = np.zeros((h, w), np.float32)
    ys, xs = np.meshgrid(np.arange(0, h, 2), np.arange(0, w, 2), indexing="ij")
    P[ys, xs] = rng.uniform(0.25, 2.0, ys.shape).astype(np.float32)
    P[200:240, :] = 0.0
    n_salt = int((P > 0).sum())
    kept = 0
    for k in range(6):
        P[210:224, 20 + 60 * k:20 + 60 * k + 16] = 0.3 + k / 16.0
        P[212:214, 50 + 60 * k:52 + 60 * k] = 0.9
        kept += 1
    return P, n_salt + 12, kept


def run_crafted(P, thr_expected=None):
    """detect_words(scores=True) of an engine whose detection model returns P for a page of P's size ->
    (scored result, unscored rects, the map the engine reports)."""
    h, w = P.shape
    calls = []

    def model(x):
        calls.append(x.shape)
        return P.reshape(1, 1, h, w)

    eng = OcrEngine(detection_model=Model.from_callable([1, 1, h, w], model))
    inp = eng.prepare_input(ImageSource.from_tensor(np.zeros((h, w, 1), np.uint8), DimOrder.Hwc))
    plain = eng.detect_words(inp)
    got = eng.detect_words(inp, scores=True)
    seen = eng.detect_text_pixels(inp)
    assert len(calls) == 3 and all(c == (1, 1, h, w) for c in calls)
    return got, plain, seen, float(eng.detection_threshold())


@pytest.mark.parametrize("w", [2304, 2305], ids=["quad", "byte"])
def test_crafted_shapes(w):
    P, back, n_ext, n_kept = crafted_shapes(w)
    ref = DR.reference(back, 0.2, MIN_AREA, count=True)
    assert ref[3] == n_ext and len(ref[0]) == n_kept, (ref[3], len(ref[0]), n_ext, n_kept)
    assert np.isinf(back).sum() == 16 and (back == 1.0).sum() > 100 and ((back > 1) & np.isfinite(back)).sum() > 100
    got, plain, seen, thr = run_crafted(P)
    assert np.array_equal(seen, back, equal_nan=True), "a page of the model's size comes back as the model's map, +inf included"
    assert np.isinf(seen).sum() == 16 and np.isnan(seen).sum() == 48
    assert thr == np.float32(0.2)
    assert_same("crafted shapes, w = %d, the map read back" % w, got, DR.reference(seen, thr, MIN_AREA))
    assert_same("crafted shapes, w = %d" % w, got, ref[:3])
    assert plain.tobytes() == got[0].tobytes()
    # what the shapes were built to show, from the engine's own numbers
    byp = {tuple(r[:2]): (s, n) for r, s, n in zip(*got)}
    assert (got[2] == 160 + w - 1).sum() == 1                              # the cross: every pixel of both bars once
    ring = [n for r, s, n in zip(*got) if abs(r[0] - 29.5) < 1e-3 and abs(r[1] - 29.5) < 1e-3]
    assert ring == [40 * 40 - 32 * 32]                                     # hole, inner ring and island left out
    assert (got[1] == 1.0).sum() == 3                                      # 1.0, 1.5 and the 1.0 blob with a 3.0 core
    assert len(byp) == n_kept


@pytest.mark.parametrize("w", [704, 702], ids=["quad", "byte"])
def test_crafted_salt_noise_takes_the_overflow_rerun(w):
    P, n_ext, n_kept = crafted_salt(w)
    assert n_ext > 65536, "more components than the first pass has room for"
    ref = DR.reference(P, 0.2, MIN_AREA, count=True)
    assert ref[3] == n_ext and len(ref[0]) == n_kept == 6
    got, plain, seen, thr = run_crafted(P)
    assert seen.tobytes() == P.tobytes()
    assert_same("salt noise, w = %d" % w, got, ref[:3])
    assert plain.tobytes() == got[0].tobytes()
    assert got[2].tolist() == [14 * 16] * 6


def second_trip_pages(w):
    """Two 128 x w maps.  A: six kept blobs with a speck beside each.  B: the same below salt on the stride-2 lattice
    over rows 0..63 — more components than the 2 048 that travel with the counts, fewer than the first pass has room
    for: the page is fetched in a second round trip, and its kept words come after all the salt in component order."""
    h = 128
    A = np.zeros((h, w), np.float32)
    for k in range(6):
        A[90:104, 20 + 60 * k:20 + 60 * k + 16] = 0.3 + k / 16.0
        A[92:94, 50 + 60 * k:52 + 60 * k] = 0.9
    B = A.copy()
    rng = np.random.default_rng(w)
    ys, xs = np.meshgrid(np.arange(0, 64, 2), np.arange(0, w, 2), indexing="ij")
    B[ys, xs] = rng.uniform(0.25, 2.0, ys.shape).astype(np.float32)
    return A, B


@pytest.mark.parametrize("w", [704, 702], ids=["quad", "byte"])
def test_second_round_trip_page_in_a_batch_with_a_prefix_page(w):
    A, B = second_trip_pages(w)
    h = A.shape[0]
    refA = DR.reference(A, 0.2, MIN_AREA, count=True)
    refB = DR.reference(B, 0.2, MIN_AREA, count=True)
    capacity = min(65536, h * w // 2 + 16)
    print("w = %d: A %d components, %d kept; B %d components, %d kept, capacity %d"
          % (w, refA[3], len(refA[0]), refB[3], len(refB[0]), capacity))
    assert refA[3] == 12 and refA[3] <= 2048, "A travels with the counts"
    assert refB[3] == 32 * (w // 2) + 12 and 2048 < refB[3] <= capacity, "B needs the second trip and no re-run"
    assert len(refA[0]) == len(refB[0]) == 6 and refB[2].tolist() == [14 * 16] * 6
    maps = {"A": A, "B": B}
    ref = {"A": refA[:3], "B": refB[:3]}
    queue = []

    def model(x):   # its k-th map on its k-th call
        assert x.shape == (1, 1, h, w)
        return queue.pop(0).reshape(1, 1, h, w)

    eng = OcrEngine(detection_model=Model.from_callable([1, 1, h, w], model))
    inp = eng.prepare_input(ImageSource.from_tensor(np.zeros((h, w, 1), np.uint8), DimOrder.Hwc))

    def run(names, scores):
        queue[:] = [maps[n] for n in names]
        out = eng.detect_words_batch([inp] * len(names), scores=scores) if len(names) > 1 else \
            [[x] for x in eng.detect_words(inp, scores=True)] if scores else [eng.detect_words(inp)]
        assert not queue, "one run per page, in the caller's order"
        return out

    single = {n: run([n], True) for n in "AB"}
    for n in "AB":
        assert_same("w = %d, page %s alone" % (w, n), tuple(x[0] for x in single[n]), ref[n])
        assert run([n], False)[0].tobytes() == single[n][0][0].tobytes(), "page %s alone, unscored" % n
    for names in ("AB", "BA"):
        words, score, pixels = run(names, True)
        plain = run(names, False)
        for i, n in enumerate(names):
            what = "w = %d, batch %s, page %s" % (w, names, n)
            assert_same(what, (words[i], score[i], pixels[i]), ref[n])
            assert_same(what + " against its single-page call", (words[i], score[i], pixels[i]), tuple(x[0] for x in single[n]))
            assert plain[i].tobytes() == words[i].tobytes(), what + ": unscored rects"
            assert plain[i].tobytes() == run([n], False)[0].tobytes(), what + ": unscored against its single-page call"


# ------------------------------------------------------------------ 3. scoring changes nobody's rects or launches
DET_STAGES = ("resize_to_model", "detection_cnn", "resize_threshold", "ccl", "contour_rects")


def test_unscored_requests_are_untouched_by_scored_traffic(prod):
    eng = OcrEngine(detection_model=Model.load_bytes(prod.dbuf))
    specs = [PAGE_1024_A, PAGE_W1022, PAGE_SMALL]
    inputs = [eng.prepare_input(ImageSource.from_tensor(prod.page(s)[0], DimOrder.Hwc)) for s in specs]
    eng.enable_timing(1)

    def launches(scores):
        eng.stage_times(reset=True)
        out = [eng.detect_words(i, scores=scores) for i in inputs] + [eng.detect_words_batch(inputs, scores=scores)]
        st = eng.stage_times(reset=True)
        return out, {k: st[k][1] for k in DET_STAGES}

    before, n_before = launches(False)
    scored, n_scored = launches(True)
    after, n_after = launches(False)
    eng.enable_timing(0)
    print("launches unscored", n_before, "scored", n_scored)
    assert n_before == n_after, "an unscored request launches what it launched before scored traffic"
    # two fills and one kernel per size-dependent pass, counted with the component stage; nothing else moves
    passes = len(inputs) + len({(s[1], s[2]) for s in specs})
    assert n_scored["ccl"] == n_before["ccl"] + 3 * passes
    assert {k: v for k, v in n_scored.items() if k != "ccl"} == {k: v for k, v in n_before.items() if k != "ccl"}
    for i in range(len(inputs)):
        assert before[i].tobytes() == after[i].tobytes() == scored[i][0].tobytes()
        assert before[-1][i].tobytes() == after[-1][i].tobytes() == scored[-1][0][i].tobytes()
        assert_same("page %d" % i, scored[i], prod.page(specs[i])[2])
        assert_same("batch page %d" % i, (scored[-1][0][i], scored[-1][1][i], scored[-1][2][i]), prod.page(specs[i])[2])


# ------------------------------------------------------------------ 4. the coalescer
def test_coalesced_scored_and_unscored_callers_get_their_solo_bits(prod):
    eng = OcrEngine(detection_model=Model.load_bytes(prod.dbuf))
    specs = [PAGE_1024_A, PAGE_W1022, PAGE_SMALL, PAGE_1024_B, PAGE_MID, PAGE_W1023]
    inputs = [eng.prepare_input(ImageSource.from_tensor(prod.page(s)[0], DimOrder.Hwc)) for s in specs]
    solo = [eng.detect_words(i, scores=True) for i in inputs]
    solo_plain = [eng.detect_words(i) for i in inputs]
    for i, s in enumerate(specs):
        assert_same("solo %d" % i, solo[i], prod.page(s)[2])
        assert solo_plain[i].tobytes() == solo[i][0].tobytes()
    base = eng.coalesce_stats()["detect"]
    bad = []
    gate = threading.Barrier(6)

    def worker(k):
        gate.wait()
        for it in range(16):
            j = (it * 5 + k) % len(inputs)
            if (it + k) % 2:
                got = eng.detect_words(inputs[j], scores=True)
                ok = got[0].tobytes() == solo[j][0].tobytes() and np.array_equal(DR.bits(got[1]), DR.bits(solo[j][1])) \
                    and np.array_equal(got[2], solo[j][2])
            else:
                ok = eng.detect_words(inputs[j]).tobytes() == solo_plain[j].tobytes()
            if not ok:
                bad.append((k, it, j))

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(6)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not bad, bad[:8]
    merged = eng.coalesce_stats()["detect"]
    batches, requests = merged[0] - base[0], merged[1] - base[1]
    print("coalescer: %d requests in %d batches" % (requests, batches))
    assert requests == 6 * 16 and 1 <= batches < requests, "requests shared batches"


# ------------------------------------------------------------------ 5. an engine group
@pytest.mark.parametrize("gather", ["host", "rccl"])
def test_group_equals_single_engine(prod, gather, monkeypatch):
    if gather == "rccl":   # the librccl test double (tests/stubs): the device-to-device transport carries the same payload
        monkeypatch.setenv("OCRS_RCCL_LIB", stub_util.rccl_stub_path())
    group = EngineGroup([0, 0], prod.dbuf, None, gather=gather, shared_block=2)
    pages = [synth.synthetic_page(40 + s, 400, 500, lines=30, columns=1) for s in range(7)]
    inputs = group.prepare_input_batch(pages)
    words, score, pixels = group.detect_words_batch(inputs, scores=True)
    assert group.last_gather()["transport"] == gather
    plain = group.detect_words_batch(inputs)
    singles = [prod.eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pages]
    ew, es, ep = prod.eng.detect_words_batch(singles, scores=True)
    assert sum(len(x) for x in ew) >= 50 * len(pages)
    for i in range(len(pages)):
        assert_same("group page %d" % i, (words[i], score[i], pixels[i]), (ew[i], es[i], ep[i]))
        assert plain[i].tobytes() == ew[i].tobytes()
    assert_same("group page 0 against the definition", (words[0], score[0], pixels[0]),
                DR.reference(prod.eng.detect_text_pixels(singles[0]), prod.thr, MIN_AREA))


# ------------------------------------------------------------------ 6. run to run
def test_twenty_identical_runs(prod):
    specs = [PAGE_1024_A, PAGE_1024_B] * 4
    inputs = [prod.page(s)[1] for s in specs]
    first = prod.eng.detect_words_batch(inputs, scores=True)
    for i, s in enumerate(specs):
        assert_same("page %d" % i, (first[0][i], first[1][i], first[2][i]), prod.page(s)[2])
    for run in range(19):
        again = prod.eng.detect_words_batch(inputs, scores=True)
        for i in range(len(specs)):
            assert again[0][i].tobytes() == first[0][i].tobytes(), (run, i)
            assert np.array_equal(DR.bits(again[1][i]), DR.bits(first[1][i])) and np.array_equal(again[2][i], first[2][i]), (run, i)


# ------------------------------------------------------------------ 7. the CLI
def test_cli_detection_confidence(tmp_path):
    from PIL import Image

    from ocrs_amd import cli, models, output
    px = synth.synthetic_page(3, 256, 384, lines=8, columns=1)
    path = str(tmp_path / "page.png")
    Image.fromarray(px).save(path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("plain", "conf", "det", "both", "cut")}
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    assert cli.main([path, "-j", "--confidence", "-o", files["conf"]]) == 0
    assert cli.main([path, "-j", "--detection-confidence", "-o", files["det"]]) == 0
    assert cli.main([path, "-j", "--confidence", "--detection-confidence", "-o", files["both"]]) == 0
    text = {k: open(files[k], encoding="utf-8").read() for k in ("plain", "conf", "det", "both")}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))
    words, score, pixels = eng.detect_words(inp, scores=True)
    assert len(words) >= 20
    lines, index = eng.find_text_lines(inp, words, index=True)
    # -j --confidence is what it was: the scored-recognition document of the unscored detection path
    texts = eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp)), scores=True)
    assert output.format_json_output(path, px.shape[:2], texts, confidence=True) == text["conf"]
    assert output.format_json_output(path, px.shape[:2], texts) == text["plain"]

    def strip(doc):
        for ln in doc["paragraphs"][0]["lines"]:
            del ln["word_boxes"]
        return json.dumps(doc, indent=2, ensure_ascii=False, sort_keys=True)

    assert strip(json.loads(text["det"])) == text["plain"] and strip(json.loads(text["both"])) == text["conf"]
    doc_lines = json.loads(text["det"])["paragraphs"][0]["lines"]
    kept_lines = [k for k, t in enumerate(texts) if t is not None]
    assert len(doc_lines) == len(kept_lines) > 0
    n_boxes = 0
    for ln, k in zip(doc_lines, kept_lines):
        assert len(ln["word_boxes"]) == len(index[k])
        for box, wi in zip(ln["word_boxes"], index[k]):              # reading order; values round-trip to the API's
            assert np.float32(box["confidence"]).view(np.uint32) == score[wi].view(np.uint32)
            assert box["pixels"] == int(pixels[wi])
            assert box["vertices"] == output.rounded_vertex_coords(words[wi])
            n_boxes += 1
    assert n_boxes == sum(len(index[k]) for k in kept_lines)

    # --min-word-score removes exactly the words below it, before the lines are formed
    cut = float(np.sort(score)[len(score) // 3])
    assert (score < cut).any() and (score >= cut).any()
    assert cli.main([path, "-j", "--detection-confidence", "--min-word-score", repr(cut), "-o", files["cut"]]) == 0
    keep = score >= np.float32(cut)
    kl, kidx = eng.find_text_lines(inp, words[keep], index=True)
    ktexts = eng.recognize_text(inp, kl)
    boxes = [[(words[keep][j], score[keep][j], pixels[keep][j]) for j in idx] for idx in kidx]
    assert output.format_json_output(path, px.shape[:2], ktexts, word_boxes=boxes) == open(files["cut"], encoding="utf-8").read()
    got_boxes = [b for ln in json.loads(open(files["cut"], encoding="utf-8").read())["paragraphs"][0]["lines"] for b in ln["word_boxes"]]
    assert all(np.float32(b["confidence"]) >= np.float32(cut) for b in got_boxes)
    assert len(got_boxes) == sum(len(kidx[k]) for k, t in enumerate(ktexts) if t is not None) <= int(keep.sum())
