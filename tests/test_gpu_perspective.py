"""Perspective correction on the GPU, bit for bit against tests/perspective_ref.py.

Pages are put on the device with input_from_grey.  Peaks are compared as integers (uint64).  Projected pages are compared
as 32-bit words, NaN positions equal (a NaN compares as NaN, not by payload).

Run with:  python -m pytest tests -m gpu
"""
import json

import numpy as np
import pytest

import deskew_ref as D
import models_util as M
import perspective_ref as P
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, output, synth
import ocrs_amd

pytestmark = pytest.mark.gpu
# (height, width): one pixel, one row, one column, two rows; around one 64 x 64 tile either way; several tiles with partial
# edges; a work page
SHAPES = [(1, 1), (1, 300), (300, 1), (2, 3), (63, 65), (64, 64), (65, 63), (127, 129), (97, 211), (512, 384)]
EXTREMES = np.array([[0, 65536], [65536, 0], [-65536, 0], [0, -65536], [46341, 46341], [-46341, 46341], [65536, 65536], [-65536, -65536]],
                    np.int32)
MIN_STEPS = (1, 8, 255, 256)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.fixture(scope="module")
def eng():
    return OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(M.recognition_model_bytes()))


def image_of(page):
    return np.ascontiguousarray(page.image()[0])


def planted(a, seed):
    """NaN (quiet and signalling), +-inf, -0.0, values far outside [-0.5, 0.5] and denormals written over random places of
    the page as 32-bit words (fewer on a page of fewer pixels)."""
    words = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x40400000, 0xC0400000, 0x7F7FFFFF,
                      0xFF7FFFFF, 0x00000001, 0x80000001], np.uint32)
    flat = a.reshape(-1).view(np.uint32)
    n = min(len(words), max(1, flat.size // 8))
    flat[np.random.default_rng(seed).choice(flat.size, size=n, replace=False)] = words[:n]
    return a


def noise(seed, h, w, plant=True):
    """[h, w] float32, uniform in [-0.6, 0.6) (a tenth of it clamps either way, so steps of 255 bins occur); plant: see
    planted()."""
    rng = np.random.default_rng(seed)
    a = ((rng.random((h, w), dtype=np.float32) - np.float32(0.5)) * np.float32(1.2)).astype(np.float32)
    return planted(a, seed) if plant else a


def random_bits(seed, h, w):
    """Every bit random: a 256th of the pixels are NaN or infinite, most of the rest clamp."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(h, w), dtype=np.uint64).astype(np.uint32).view(np.float32)


def tables():
    return {"0": D.skew_table(0, 1, 0.5), "+-0.5": D.skew_table(-1, 3, 0.5), "+-15": P.table_of(P.default_params()), "extremes": EXTREMES}


def check_peaks(eng, page, table, min_step, what):
    got = eng.edge_peaks([eng.input_from_grey(page)], table, min_step)
    assert got.dtype == np.uint64 and got.shape == (1, 2, 2, len(table), 16)
    exp = P.edge_peaks(page, table, min_step)
    bad = np.argwhere(got[0] != exp)
    assert not len(bad), (what, min_step, len(bad), [(tuple(i), hex(int(got[0][tuple(i)])), hex(int(exp[tuple(i)]))) for i in bad[:4]])
    return got[0]


# ------------------------------------------------------------------ 1. the edge peaks
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_peaks_equal_the_restatement(eng, shape):
    h, w = shape
    T = tables()
    assert [len(T[k]) for k in ("0", "+-0.5", "+-15")] == [1, 3, 61]
    page = noise(h * 1000 + w, h, w)
    seen = 0
    for name in T:   # every table with every min_step, at every size
        for ms in MIN_STEPS:
            pk = check_peaks(eng, page, T[name], ms, "noise %s" % name)
            seen += int(pk.any())
            if ms == 256:
                assert not pk.any(), "no step reaches 256 bins"
    if h * w > 1000:
        assert seen == 3 * len(T), "steps of 1, 8 and 255 bins occur in the noise"
    bits = random_bits(h * 1000 + w + 1, h, w)
    for name, ms in (("+-0.5", 1), ("+-0.5", 255), ("+-15", 8), ("extremes", 8), ("extremes", 1)):
        check_peaks(eng, bits, T[name], ms, "random bits %s" % name)


def test_peaks_of_a_framed_page_are_its_frame(eng):
    """A light rectangle on a dark page: one `+` and one `-` peak per family at angle 0, of the rectangle's side, at the
    bins of its edges; a flat page has none."""
    page = np.full((200, 300), -0.3, np.float32)
    page[40:150, 60:260] = 0.4
    t = tables()["+-0.5"]
    pk = check_peaks(eng, page, t, 8, "frame")

    def peaks(f, s):
        return sorted((int(e) >> 32, 0xFFFFFFFF - (int(e) & 0xFFFFFFFF)) for e in pk[f, s, 1] if e)

    assert peaks(0, 0) == [(200, 39)] and peaks(0, 1) == [(200, 149)]
    assert peaks(1, 0) == [(110, 59)] and peaks(1, 1) == [(110, 259)]
    assert not check_peaks(eng, np.full((70, 90), 0.25, np.float32), t, 1, "flat").any()


def test_a_mixed_batch_equals_each_page_alone(eng):
    shapes = [(97, 211), (1, 1), (64, 64), (300, 1), (127, 129), (65, 63)]
    pages = [noise(50 + i, h, w) for i, (h, w) in enumerate(shapes)]
    inputs = [eng.input_from_grey(p) for p in pages]
    table = tables()["+-15"]
    batch = eng.edge_peaks(inputs, table, 8)
    assert batch.shape == (6, 2, 2, 61, 16)
    for i, p in enumerate(pages):
        assert np.array_equal(batch[i], eng.edge_peaks([inputs[i]], table, 8)[0]), shapes[i]
        assert np.array_equal(batch[i], P.edge_peaks(p, table, 8)), shapes[i]
    assert eng.edge_peaks([], table).shape == (0, 2, 2, 61, 16)


def test_twenty_repeats_are_equal(eng):
    inp = eng.input_from_grey(noise(77, 200, 333))
    table = tables()["+-15"]
    first = eng.edge_peaks([inp], table, 8)
    assert first.any()
    for _ in range(19):
        assert np.array_equal(eng.edge_peaks([inp], table, 8), first)


def test_peak_refusals(eng):
    inp = eng.input_from_grey(noise(1, 4, 4))
    ok = np.array([[0, 65536]], np.int32)
    for bad in ([[65537, 0]], [[0, -65537]], [[0, 65536], [2 ** 31 - 1, 0]]):
        with pytest.raises(_lib.OcrsError) as ei:
            eng.edge_peaks([inp], np.array(bad, np.int32))
        assert ei.value.status_name == "INVALID_ARGUMENT", bad
    with pytest.raises(_lib.OcrsError) as ei:
        eng.edge_peaks([inp], np.zeros((0, 2), np.int32))
    assert ei.value.status_name == "INVALID_ARGUMENT"
    for ms in (0, 257, -1):
        with pytest.raises(_lib.OcrsError) as ei:
            eng.edge_peaks([inp], ok, ms)
        assert ei.value.status_name == "INVALID_ARGUMENT", ms
    for hw in ((1, 4097), (4097, 1)):
        with pytest.raises(_lib.OcrsError) as ei:
            eng.edge_peaks([eng.input_from_grey(np.zeros(hw, np.float32))], ok)
        assert ei.value.status_name == "INVALID_ARGUMENT", hw
    assert not eng.edge_peaks([eng.input_from_grey(np.zeros((1, 4096), np.float32))], ok).any()
    assert eng.edge_peaks([inp], ok).shape == (1, 2, 2, 1, 16), "the engine works after a refusal"


# ------------------------------------------------------------------ 2. the projective warp
def assert_same_words(got, exp, what):
    assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.shape, exp.shape)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ at %s" % (what, np.argwhere(np.isnan(got) != nan)[:4].tolist())
    bad = np.argwhere((got.view(np.uint32) != exp.view(np.uint32)) & ~nan)
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d pixels differ; first at %s: got %r (%#x), expected %r (%#x)"
                             % (what, len(bad), got.size, at, got[at], got.view(np.uint32)[at], exp[at], exp.view(np.uint32)[at]))


ODD_FILL = float(np.array([0x3EABCDEF], np.uint32).view(np.float32)[0])
FILLS = [0.5, -0.5, ODD_FILL]


def keystones(h, w):
    """Three quads on (and a little beyond) an h x w page, as fractions of its sides."""
    out = []
    for fr in ([0.15, 0.1, 0.85, 0.1, 0.93, 0.9, 0.07, 0.9], [0.1, 0.12, 0.9, 0.05, 0.95, 0.88, 0.04, 0.97], [0.2, -0.05, 1.04, 0.15, 0.83, 1.02, -0.03, 0.8]):
        out.append(np.array([v * (w if i % 2 == 0 else h) for i, v in enumerate(fr)], np.float32))
    return out


def project_maps(h, w):
    """(name, m, out_hw): the identity; three keystones; a map whose dn crosses zero inside the output; an affine one."""
    out = [("identity", P.quad_map(P.page_corners(h, w))[1], (h, w))]
    for i, q in enumerate(keystones(h, w)):
        made = P.quad_map(q)
        if made is not None:
            out.append(("keystone %d" % i, made[1], made[0]))
    out.append(("dn crosses zero", np.array([1.0, 0.9, 0.1, 2.0, -0.05, 1.1, -2.0 / (w + 9), 0.5 / (h + 7)], np.float32), (h + 7, w + 9)))
    out.append(("scale and shear", np.array([-3.25, 0.75, 0.125, -2.5, -0.0625, 1.5, 0.0, 0.0], np.float32), (h + 9, w + 7)))
    return out


@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (150, 258)], ids=lambda s: "%dx%d" % s)
def test_project_equals_the_restatement(eng, shape):
    h, w = shape
    page = noise(h * 7 + w, h, w)
    inp = eng.input_from_grey(page)
    cases = project_maps(h, w)
    assert len(cases) >= (6 if h > 1 else 3)
    made = eng.project_batch([inp] * len(cases), [m for _, m, _ in cases], [hw for _, _, hw in cases], [FILLS[i % 3] for i in range(len(cases))])
    for i, (name, m, hw) in enumerate(cases):
        exp = P.project(page, m, hw, FILLS[i % 3])
        assert made[i].shape == (1,) + tuple(hw)
        assert_same_words(image_of(made[i]), exp, "%s fill %r" % (name, FILLS[i % 3]))
        if name == "dn crosses zero" and h > 1:
            fx, fy = np.meshgrid(np.arange(hw[1]) + 0.5, np.arange(hw[0]) + 0.5)
            behind = (1.0 + float(m[6]) * fx + float(m[7]) * fy) < -1e-3
            assert behind.any() and (~behind).any() and np.all(exp[behind] == np.float32(FILLS[i % 3])), "fill behind the horizon"
    clean = noise(5, h, w, plant=False)
    ident = eng.project(eng.input_from_grey(clean), cases[0][1], (h, w))
    assert image_of(ident).tobytes() == clean.tobytes(), "the identity keeps every bit of a finite page"


@pytest.mark.parametrize("shape", [(37, 53), (150, 258)], ids=lambda s: "%dx%d" % s)
def test_project_without_perspective_has_the_bits_of_warp(eng, shape):
    h, w = shape
    page = noise(h * 3 + w, h, w)
    inp = eng.input_from_grey(page)
    maps = [D.deskew_map(h, w, a, expand=e) for a in (0.0, 3.0, -10.0, 45.0) for e in (True, False)]
    maps.append(((h + 9, w + 7), np.array([-3.25, 0.75, 0.125, -2.5, -0.0625, 1.5], np.float32)))
    for tail in ([0.0, 0.0], [-0.0, -0.0]):
        proj = eng.project_batch([inp] * len(maps), [np.concatenate([m, np.array(tail, np.float32)]) for _, m in maps], [hw for hw, _ in maps], FILLS * 3)
        warp = eng.warp_batch([inp] * len(maps), [m for _, m in maps], [hw for hw, _ in maps], FILLS * 3)
        for i in range(len(maps)):
            assert_same_words(image_of(proj[i]), image_of(warp[i]), "map %d" % i)


@pytest.mark.parametrize("out_w", [256, 257, 258, 259])
def test_project_output_widths_and_fills(eng, out_w):
    """Every width % 4 (the 16-byte store needs % 4 == 0), one pixel, and a block boundary at 256 columns and 16 rows."""
    page = noise(out_w, 61, 83)
    inp = eng.input_from_grey(page)
    m = np.array([-20.5, 0.48, 0.11, -9.25, -0.07, 0.52, 0.0011, -0.0007], np.float32)
    for fill in FILLS:
        for hw in ((1, 1), (17, out_w), (1, out_w), (33, out_w + 256)):
            assert_same_words(image_of(eng.project(inp, m, hw, fill=fill)), P.project(page, m, hw, fill), "%s fill %r" % (hw, fill))
    # positions that are far away, huge or not finite read as fill; so does a dn that overflows or is NaN (inf - inf)
    for name, mm in (("far", [1e30, 1.0, 0.0, -1e30, 0.0, 1.0, 1e-4, 0.0]), ("overflowing", [0.0, 3e38, 3e38, 0.0, 3e38, 3e38, 1e-3, 1e-3]),
                     ("tiny dn", [5.0, 1.0, 0.0, 5.0, 0.0, 1.0, -1.0 / 128.5, 0.0]), ("dn overflows", [5.0, 1.0, 0.0, 5.0, 0.0, 1.0, 3e38, 3e38]),
                     ("dn is inf - inf", [5.0, 1.0, 0.0, 5.0, 0.0, 1.0, 3e38, -3e38]), ("0 / 0 and inf / inf", [0.0, 3e38, 0.0, 0.0, 0.0, 3e38, 3e36, 0.0])):
        mm = np.array(mm, np.float32)
        assert_same_words(image_of(eng.project(inp, mm, (5, out_w), fill=0.125)), P.project(page, mm, (5, out_w), 0.125), name)


def test_project_mixed_batch_and_lifetimes(eng):
    shapes = [(97, 211), (1, 1), (64, 64), (300, 5), (40, 256)]
    pages = [noise(90 + i, h, w, plant=i % 2 == 0) for i, (h, w) in enumerate(shapes)]
    inputs = [eng.input_from_grey(p) for p in pages]
    maps = [P.quad_map(keystones(h, w)[i % 3]) for i, (h, w) in enumerate(shapes)]
    maps[1] = ((3, 2), np.array([0.25, 0.5, 0.0, 0.25, 0.0, 0.5, 0.1, 0.2], np.float32))
    fills = [0.5, -0.5, ODD_FILL, 0.0, 0.5]
    made = eng.project_batch(inputs, [m for _, m in maps], [hw for hw, _ in maps], fills)
    exps = [P.project(p, m, hw, f) for p, (hw, m), f in zip(pages, maps, fills)]
    for i in range(5):
        assert_same_words(image_of(made[i]), exps[i], "batch %d" % i)
        assert_same_words(image_of(eng.project(inputs[i], maps[i][1], maps[i][0], fill=fills[i])), exps[i], "alone %d" % i)
    assert eng.project_batch([], [], []) == []
    # the projected page and its source are independent: either is alive after the other is freed
    keep = made[0]
    del inputs[0]
    assert_same_words(image_of(keep), exps[0], "the projected page after its source was freed")
    src = eng.input_from_grey(pages[1])
    p2 = eng.project(src, maps[1][1], maps[1][0])
    del p2
    assert image_of(src).tobytes() == pages[1].tobytes(), "the source after its projected page was freed"
    for bad_hw in ((0, 5), (5, 65536)):
        with pytest.raises(_lib.OcrsError) as ei:
            eng.project(src, maps[1][1], bad_hw)
        assert ei.value.status_name == "INVALID_ARGUMENT"
    for bad in ([np.nan, 1, 0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 0, 1, np.inf, 0]):
        with pytest.raises(_lib.OcrsError):
            eng.project(src, np.array(bad, np.float32), (5, 5))
    with pytest.raises(ValueError):
        eng.project(src, np.zeros(6, np.float32), (5, 5))


# ------------------------------------------------------------------ 3. the outline and the whole chain
QUAD = np.array([150, 120, 1050, 160, 1120, 1290, 90, 1230], np.float32)   # of the bench page on a 1400 x 1200 photo
PHOTO_HW = (1400, 1200)


@pytest.fixture(scope="module")
def photo(eng):
    """The bench page, prepared, seen through QUAD on a dark desk with a little noise, by the RESTATEMENT's projection."""
    px = synth.synthetic_page(0, 1024, 1024, lines=80)
    grey = image_of(eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc)))
    shot = P.project(grey, P.plant_map(QUAD, grey.shape), PHOTO_HW, -0.2)
    shot = (shot + (np.random.default_rng(4).random(PHOTO_HW, dtype=np.float32) - np.float32(0.5)) * np.float32(0.03)).astype(np.float32)
    return grey, shot


def outline_tuple(o):
    if isinstance(o, dict):
        return (bool(o["found"]), int(o["polarity"]), np.asarray(o["corners"], np.float32).tobytes(), tuple(o["counts"]), tuple(o["angles"]), tuple(o["work_hw"]))
    return (o.found, o.polarity, o.corners.astype(np.float32).tobytes(), o.counts, o.angles, o.work_hw)


def test_find_outline_equals_the_restatement(eng, photo):
    grey, shot = photo
    inp = eng.input_from_grey(shot)
    o = eng.find_outline(inp)
    work_hw = ocrs_amd.work_size(shot.shape, max_side=512)
    assert o.work_hw == work_hw and max(work_hw) == 512 < max(shot.shape)
    work = image_of(eng.resize(inp, work_hw, filter="area"))
    assert work.tobytes() == D.work_page(shot, 512).tobytes()
    # the restatement's choice over the library's primitive, then over its own
    lib_o = P.find_outline(shot, peaks=lambda p, t, ms: eng.edge_peaks([eng.input_from_grey(p)], t, ms)[0])
    ref_o = P.find_outline(shot)
    assert outline_tuple(o) == outline_tuple(lib_o) == outline_tuple(ref_o)
    assert o.found and o.polarity == 0
    err = np.hypot(*(o.corners.astype(np.float64) - QUAD.astype(np.float64).reshape(4, 2)).T).max()
    bound = P.corner_bound(QUAD, shot.shape)
    print("the bench page on a desk: corners within %.2f pixels of the planted ones (bound %.2f)" % (err, bound))
    assert err <= bound, "and they are the corners the page was planted at"
    chosen = ocrs_amd.outline_choose(eng.edge_peaks([eng.input_from_grey(work)], P.table_of(P.default_params()))[0], P.table_of(P.default_params()), work_hw, shot.shape)
    assert outline_tuple(chosen) == outline_tuple(o)
    small = eng.find_outline(inp, work_max_side=300, max_deg=10.0, step_deg=1.0, min_step=16, min_cover=0.3)
    params = dict(P.default_params(), work_max_side=300, max_deg=10.0, step_deg=1.0, min_step=16, min_cover=0.3)
    assert outline_tuple(small) == outline_tuple(P.find_outline(shot, params)) and small.work_hw == (300, 257)
    with pytest.raises(_lib.OcrsError) as ei:
        eng.find_outline(inp, max_deg=50.0)
    assert ei.value.status_name == "INVALID_ARGUMENT"


def test_a_blank_page_has_no_outline_and_comes_back_itself(eng):
    for page in (np.full((300, 200), 0.5, np.float32), np.full((40, 2000), np.nan, np.float32), np.zeros((1, 1), np.float32)):
        inp = eng.input_from_grey(page)
        o = eng.find_outline(inp)
        assert not o.found and not o.corners.any() and o.counts == (0, 0, 0, 0)
        out, m, found = eng.straighten(inp)
        assert out is inp and not found.found and m.tolist() == [-0.5, 1.0, 0.0, -0.5, 0.0, 1.0, 0.0, 0.0]
    assert eng.get_text(inp, perspective="auto") == eng.get_text(inp)


def test_straighten_and_get_text_are_the_manual_chain(eng, photo):
    grey, shot = photo
    inp = eng.input_from_grey(shot)
    # by hand, through the public calls
    o = eng.find_outline(inp)
    out_hw, m = ocrs_amd.quad_map(o.corners)
    ref_hw, ref_m = P.quad_map(o.corners)
    assert out_hw == ref_hw and m.tobytes() == ref_m.tobytes()
    flat = eng.project(inp, m, out_hw, fill=0.5)
    assert_same_words(image_of(flat), P.project(shot, ref_m, ref_hw, 0.5), "the straightened sheet")
    assert abs(out_hw[0] - 1130) < 40 and abs(out_hw[1] - 1030) < 140, out_hw
    got, gm, go = eng.straighten(inp)
    assert outline_tuple(go) == outline_tuple(o) and gm.tobytes() == m.tobytes() and image_of(got).tobytes() == image_of(flat).tobytes()
    given, gm2, none = eng.straighten(inp, o.corners)
    assert none is None and gm2.tobytes() == m.tobytes() and image_of(given).tobytes() == image_of(flat).tobytes()
    words = eng.detect_words(flat)
    lines = eng.find_text_lines(flat, words)
    texts = eng.recognize_text(flat, lines)
    text = "\n".join(str(t) for t in texts if t is not None)
    assert len(lines) > 0 and eng.get_text(inp, perspective="auto") == text
    assert eng.get_text(inp, perspective=o.corners) == text
    assert eng.get_text(inp, perspective=o.corners, rectify=True) == eng.get_text(flat, rectify=True)
    assert eng.get_text(inp, perspective=None) == eng.get_text(inp)
    # perspective comes first: the chain with normalisation and deskew is theirs on the straightened sheet
    assert eng.get_text(inp, perspective="auto", normalize=True, deskew="auto") == eng.get_text(flat, normalize=True, deskew="auto")
    # the words of the straightened sheet come back to where the photo shows them: inside the planted quad
    print("%d words on the straightened sheet, %d on the bench page, %d on the photo" % (len(words), len(eng.detect_words(eng.input_from_grey(grey))),
                                                                                        len(eng.detect_words(inp))))
    assert len(words) > 0
    back = ocrs_amd.unproject_rects(words, m)
    assert back.view(np.uint32).tobytes() == P.unproject_rects(words, m).view(np.uint32).tobytes()
    q = QUAD.astype(np.float64).reshape(4, 2)
    for i in range(4):   # to the right of every side, walking TL, TR, BR, BL with y down; 12 pixels of slack for the outline
        e, r = q[(i + 1) % 4] - q[i], back[:, :2].astype(np.float64) - q[i]
        assert np.all((e[0] * r[:, 1] - e[1] * r[:, 0]) / np.hypot(*e) > -12.0), "side %d" % i
    assert np.all(np.abs(np.hypot(back[:, 2], back[:, 3]) - 1.0) < 1e-6)
    lines_back = ocrs_amd.unproject_lines(texts, m)
    assert [None if t is None else str(t) for t in lines_back] == [None if t is None else str(t) for t in texts]
    boxes = np.array([c.rect for t in texts if t is not None for c in t.chars()], np.int32).reshape(-1, 4)
    got_boxes = np.array([c.rect for t in lines_back if t is not None for c in t.chars()], np.int32).reshape(-1, 4)
    assert len(boxes) > 0 and np.array_equal(got_boxes, P.unproject_boxes(boxes, m))


def test_cli_perspective(tmp_path, monkeypatch, photo, capsys):
    from PIL import Image

    from ocrs_amd import cli, models
    px8 = np.clip((photo[1] + np.float32(0.5)) * np.float32(255.0), 0, 255).astype(np.uint8)
    path = str(tmp_path / "photo.png")
    Image.fromarray(px8, "L").save(path)
    monkeypatch.chdir(tmp_path)
    files = {k: str(tmp_path / (k + ".json")) for k in ("auto", "given", "plain")}
    corners = "150,120,1050,160,1120,1290,90,1230"
    assert cli.main([path, "--perspective", "auto", "-j", "--detection-confidence", "--debug", "-o", files["auto"]]) == 0
    assert "Outline: found" in capsys.readouterr().out
    assert cli.main([path, "--perspective", corners, "--perspective-fill", "0.5", "-j", "-o", files["given"]]) == 0
    assert cli.main([path, "-j", "-o", files["plain"]]) == 0
    for bad in (["--perspective-fill", "0.5"], ["--perspective", "sideways"], ["--perspective", "1,2,3"], ["--perspective", "5,5,5,5,5,5,5,5"]):
        with pytest.raises(SystemExit):
            cli.main([path] + bad)
    text = {k: open(v, encoding="utf-8").read() for k, v in files.items()}

    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inp = eng.prepare_input(ImageSource.from_tensor(cli.load_image(path), DimOrder.Hwc))
    hw = px8.shape[:2]
    plain = output.format_json_output(path, hw, eng.recognize_text(inp, eng.find_text_lines(inp, eng.detect_words(inp))))
    assert text["plain"] == plain and "outline" not in json.loads(plain), "without the flag nothing changes"
    flat, m, _ = eng.straighten(inp, QUAD.reshape(4, 2))
    lines = eng.find_text_lines(flat, eng.detect_words(flat))
    exp = output.format_json_output(path, hw, ocrs_amd.unproject_lines(eng.recognize_text(flat, lines), m),
                                    outline={"found": True, "corners": QUAD.reshape(4, 2).tolist()})
    assert text["given"] == exp
    doc = json.loads(text["auto"])
    o = eng.find_outline(inp)
    assert doc["outline"] == {"found": True, "corners": [[float(x), float(y)] for x, y in o.corners]}
    assert (doc["image_height"], doc["image_width"]) == hw
    got_lines = doc["paragraphs"][0]["lines"]
    assert len(got_lines) > 0
    for line in got_lines:   # vertices and word boxes are in the frame of the file
        for x, y in line["vertices"] + [v for b in line["word_boxes"] for v in b["vertices"]]:
            assert 60 <= x <= 1150 and 90 <= y <= 1320, "inside the planted quad's bounding box, with slack"
