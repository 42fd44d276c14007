"""contour_cases.py reaches the branches it claims, shown on the CPU oracle alone (no GPU): border lengths against the
kernel's walk buffer, simplified counts against its small-polygon scratch, hull sizes and tie positions against its
64-lane strides, window schedules against its 128 x 32 mask window — and contour_ref.py's float32 restatements equal
the oracle bit for bit on every component of every case.  A case that stops reaching its branch fails here, whatever the GPU
does with it."""
import numpy as np
import pytest

import contour_cases as CC
import contour_ref as R
from oracle import clib

CASES = CC.cases()
BY_NAME = {c.name: c for c in CASES}
FACTS = {}


def facts(name):
    if name not in FACTS:
        FACTS[name] = R.component_facts(BY_NAME[name].mask)
    return FACTS[name]


def lanes(lo, indices):
    """The lane of rdp_mark's strided loop that meets index k of a segment starting at lo, and the stride it does so in."""
    return [((k - lo - 1) % CC.LANES, (k - lo - 1) // CC.LANES) for k in indices]


def test_case_names_are_unique():
    assert len(BY_NAME) == len(CASES)
    assert {c.group for c in CASES} == set("abcdef")


@pytest.mark.parametrize("case", [c for c in CASES if c.expect], ids=lambda c: c.name)
def test_case_has_the_facts_it_states(case):
    f = facts(case.name)
    e = case.expect
    for key in ("n", "m", "hn", "min_edges"):
        if key in e:
            assert f[key] == e[key], (key, f[key])
    if "n_max" in e:
        assert f["n"] <= e["n_max"], f["n"]
    if "n_min" in e:
        assert f["n"] >= e["n_min"], f["n"]
    if "tie" in e:
        lo, hi, idx = e["tie"]
        assert (lo, hi, idx, True) in f["ties"], f["ties"]


def test_group_a_straddles_the_walk_buffer():
    n = {name: facts(name)["n"] for name in ("bar_n1023", "bar_n1024", "bar_n1025", "long_comb")}
    assert n["bar_n1023"] == CC.WALK_BUF - 1 and n["bar_n1024"] == CC.WALK_BUF and n["bar_n1025"] == CC.WALK_BUF + 1
    assert n["long_comb"] > 5 * CC.WALK_BUF and facts("long_comb")["m"] > CC.SMALL_POLY


def test_group_b_pairs_both_boundaries():
    seen = set()
    for name in ("comb_m64_lds", "comb_m65_lds", "comb_m64_arena", "comb_m65_arena"):
        f = facts(name)
        seen.add((f["m"], f["n"] <= CC.WALK_BUF))
    assert seen == {(CC.SMALL_POLY, True), (CC.SMALL_POLY + 1, True), (CC.SMALL_POLY, False), (CC.SMALL_POLY + 1, False)}


def test_group_c_enters_the_second_stride_of_the_edge_search():
    for name in ("ellipse_120_96", "ellipse_160x100_110", "ellipse_140x60_90", "ellipse_hn128"):
        f = facts(name)
        e = f["min_edges"]
        # the minimum is attained in the first stride and, bit-equal, in the second: the cross-lane rule must pick the first
        assert f["hn"] > CC.LANES and e[0] < CC.LANES <= e[-1], (name, f["hn"], e)
        assert len({k % CC.LANES for k in e}) > 1
        a = f["areas"]
        assert all(a[k].tobytes() == a[e[0]].tobytes() for k in e)
    f = facts("ellipse_first_min_74")     # the second stride decides the result: nothing in the first attains the minimum
    assert f["hn"] > CC.LANES and len(f["min_edges"]) == 1 and f["min_edges"][0] >= CC.LANES
    f = facts("ellipse_hn128")            # two tying edges meet in ONE lane (64 apart): the lane-local `<` keeps the first
    assert f["hn"] == 2 * CC.LANES and {31, 95} <= set(f["min_edges"]) and {63, 127} <= set(f["min_edges"])
    assert facts("ellipse_hn64")["hn"] == CC.LANES      # one stride, every lane busy


def test_group_d_degenerate_hulls():
    m = CC.degenerate_page()
    s = R.component_slots(m, 3.0, 100.0)
    contours = clib.find_contours_external(m)
    by_root = {(int(c[0, 0]), int(c[0, 1])): i for i, c in enumerate(contours)}
    assert s["n_roots"] == 40
    pixel, b2, b3, sq5 = by_root[(2, 2)], by_root[(2, 6)], by_root[(2, 11)], by_root[(2, 18)]
    assert s["n"][pixel] == 1 and s["m"][pixel] == 1 and clib.min_area_rect(np.array([[2, 2]], np.float32)) is None
    # 2 x 2 simplifies to one point: no rectangle.  3 x 3 does not: its far corner lies 2 sqrt(2) > eps from the root, so it
    # keeps two points and gets the rectangle of a diagonal line, too small to count at min_area 100
    assert s["m"][b2] == 1 and not s["valid"][b2] and not s["rects"][b2].any()
    assert s["m"][b3] == 2 and not s["valid"][b3] and s["rects"][b3][4] * s["rects"][b3][5] < 100
    # the 5 x 5 square: 4 + 2 * 3 = 10 a side, area exactly 100.0, valid under >= and only under >=
    assert s["rects"][sq5][4:].tolist() == [10.0, 10.0] and s["valid"][sq5] == 1
    assert np.float32(s["rects"][sq5][4] * s["rects"][sq5][5]) == np.float32(100.0)
    # lines: hulls of two points, a rectangle of height 0 + 2 * expand
    zero = R.component_slots(m, 3.0, 0.0)
    two = [i for i in range(40) if zero["m"][i] == 2]
    assert len(two) >= 26 and all(zero["valid"][i] for i in two)
    assert sum(1 for i in range(40) if zero["m"][i] == 1) >= 10     # and components without any rectangle
    assert not zero["valid"][pixel] and zero["valid"].sum() < 40


def test_group_e_ties_cross_lanes_and_strides():
    lo, hi, idx = BY_NAME["bumps_64"].expect["tie"]
    assert lanes(lo, idx) == [(61, 0), (62, 0), (63, 0), (0, 1)]          # the last three lanes and lane 0 of the next stride
    lo, hi, idx = BY_NAME["bumps_30"].expect["tie"]
    assert lanes(lo, idx) == [(27, 0), (28, 0), (29, 0), (30, 0)]          # within one stride
    lo, hi, idx = BY_NAME["bumps_128"].expect["tie"]
    assert lanes(lo, idx) == [(61, 1), (62, 1), (63, 1), (0, 2)]          # the same lanes one stride later
    a, b = lanes(0, BY_NAME["corner_l_33"].expect["tie"][2])
    assert a[0] != b[0] and a[1] < b[1]                                    # different lanes: the cross-lane rule
    a, b = lanes(0, BY_NAME["corner_l_34_inner"].expect["tie"][2])
    assert a[0] == b[0] and a[1] + 1 == b[1]                               # the same lane, a stride apart: the lane-local `>`
    for c in CASES:
        if c.group == "e":      # every tie listed splits its segment: taking another index changes the polygon
            lo, hi, idx = c.expect["tie"]
            assert (lo, hi, idx, True) in facts(c.name)["ties"]


def _rect_words(simp, keep_collinear=False):
    _, rr = R.edge_areas_f32(R.hull_f32(simp, keep_collinear))
    return None if rr is None else R.words(rr).tolist()


@pytest.mark.parametrize("name", ["fork_10", "fork_63"])
def test_group_e_forks_show_the_tie_rule_in_the_rectangle(name):
    """On the bumps and the L-shapes every tied point ends up a vertex or inside the hull whichever is split first: their
    rectangles do not tell the rules apart.  The forks' do."""
    c = BY_NAME[name]
    xy = clib.find_contours_external(c.mask)[0][:, ::-1].astype(np.float32)
    first, _ = R.rdp_f32(xy)
    last, _ = R.rdp_f32(xy, last=True)
    assert len(first) == len(last) == 2 and _rect_words(first) != _rect_words(last)
    assert np.array_equal(R.words(first), R.words(clib.simplify_polygon(xy, 2.0)))
    lo, hi, idx = c.expect["tie"]
    want = [(10, 0), (11, 0)] if name == "fork_10" else [(63, 0), (0, 1)]      # one stride / lane 63 and lane 0 of the next
    assert lanes(lo, idx) == want


@pytest.mark.parametrize("name", ["notched_band_40", "notched_band_50", "notched_band_60"])
def test_group_d_collinear_points_on_the_winning_edge(name):
    c = BY_NAME[name]
    xy = clib.find_contours_external(c.mask)[0][:, ::-1].astype(np.float32)
    simp = clib.simplify_polygon(xy, 2.0)
    hull = R.hull_f32(simp)
    assert np.array_equal(R.words(hull), R.words(clib.convex_hull(simp)))
    kept = R.hull_f32(simp, keep_collinear=True)
    assert len(hull) == 4 and len(kept) == 6                     # the notch's rim lies on a hull edge
    assert _rect_words(simp) == R.words(clib.min_area_rect(simp)).tolist()
    assert _rect_words(simp, keep_collinear=True) != _rect_words(simp)      # and the rectangle's bits depend on dropping it


def test_group_f_windows():
    m = CC.window_shapes()
    contours = clib.find_contours_external(m)
    assert len(contours) == 3
    ext = [(c[:, 0].max() - c[0, 0], c[:, 1].max() - c[:, 1].min()) for c in contours]
    loads = [R.window_loads(c, *m.shape)["loads"] for c in contours]
    assert ext[0][1] > 2 * CC.WIN_W and loads[0] >= 4                      # the wide bar
    assert any(e[0] > 2 * CC.WIN_H and e[1] < 8 for e in ext)              # the tall post
    assert max(loads) >= 20 and max(len(c) for c in contours) > CC.WALK_BUF   # the spiral: the window comes back many times
    m = CC.corner_blobs()
    sides = [R.window_loads(c, *m.shape) for c in clib.find_contours_external(m)]
    assert len(sides) == 4
    assert [(s["left"], s["right"], s["top"], s["bottom"]) for s in sides] == [
        (True, False, True, False), (False, True, True, False), (True, False, False, True), (False, True, False, True)]
    fast = edge = 0
    for c in CC.noise_masks():
        for contour in clib.find_contours_external(c.mask):
            s = R.window_loads(contour, *c.mask.shape)
            fast, edge = fast + s["fast"], edge + s["edge"]
    assert fast > 0 and edge > 0        # both copy paths of load_window


def test_group_g_holds_every_pattern_once():
    pages = CC.pattern_pages()
    assert pages.shape == (4, 768, 768)
    per = CC.PATTERN_SIDE // CC.PATTERN_PITCH
    cells = pages.reshape(4, per, CC.PATTERN_PITCH, per, CC.PATTERN_PITCH)
    assert not cells[:, :, 4:].any() and not cells[:, :, :, :, 4:].any()       # two empty rows / columns between patterns
    bits = cells[:, :, :4, :, :4].transpose(0, 1, 3, 2, 4).reshape(-1, 16).astype(np.uint32)
    assert np.array_equal((bits << np.arange(16, dtype=np.uint32)).sum(axis=1), np.arange(65536))


def test_group_h_capacity_page():
    s = R.component_slots(CC.capacity_page(), 3.0, 0.0)
    assert s["n_roots"] == 18 and int(s["n"].sum()) == 385
    for i in range(2):
        assert 2 <= R.component_slots(CC.ordinary_page(i), 3.0, 0.0)["n_roots"] <= 8


def test_negative_zero_occurs_in_valid_rects():
    """Why the GPU comparison is on uint32 words: the definition itself produces -0.0 in rectangles that count."""
    s = R.component_slots(CC.degenerate_page(), 3.0, 0.0)
    w = R.words(s["rects"][s["valid"] == 1])
    assert (w == 0x80000000).any()


@pytest.mark.parametrize("case", CASES + CC.noise_masks(), ids=lambda c: c.name)
def test_restatements_equal_the_oracle(case):
    R.restatements_equal_clib(case.mask)


@pytest.mark.parametrize("page", range(CC.PATTERN_PAGES))
def test_restatements_equal_the_oracle_on_every_pattern(page):
    assert R.restatements_equal_clib(CC.pattern_pages()[page]) > 16384


def test_restatements_equal_the_oracle_on_the_capacity_pages():
    for m in (CC.capacity_page(), CC.ordinary_page(0), CC.ordinary_page(1)):
        R.restatements_equal_clib(m)


@pytest.mark.parametrize("min_area", [0.0, 100.0])
def test_slots_compact_to_component_rects(min_area):
    """The per-slot definition is the oracle's find_connected_component_rects before its compaction."""
    for c in CASES + CC.noise_masks()[::7]:
        s = R.component_slots(c.mask, 3.0, min_area)
        exp = clib.component_rects(c.mask, 3.0, min_area)
        assert np.array_equal(R.words(s["rects"][s["valid"] == 1]), R.words(exp)), c.name


def test_hook_refuses_bad_arguments_with_a_status():
    """ocrs_mask_component_rects: sizes outside 1 .. 65535, max_comp < 1, arena < 1 or >= 2^31 -> OCRS_ERR_INVALID_ARGUMENT
    before any device work (this test needs no GPU)."""
    from ocrs_amd import _lib
    m = np.zeros((1, 4, 4), np.uint8)
    for kw in ({"max_comp": 0}, {"max_comp": -5}, {"arena": 0}, {"arena": -1}, {"arena": 2 ** 31}, {"arena": 2 ** 40}):
        with pytest.raises(_lib.OcrsError) as e:
            _lib.mask_component_rects(m, **{"max_comp": 8, "arena": 64, **kw})
        assert e.value.status_name == "INVALID_ARGUMENT", kw
    import ctypes as C
    out = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(48, np.float32), np.zeros(8, np.uint8))
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in out]
    for h, w in ((0, 4), (4, 0), (-1, 4), (65536, 1), (1, 65536)):
        st = _lib.lib().ocrs_mask_component_rects(m.ctypes.data_as(C.c_void_p), C.c_size_t(1), h, w, C.c_float(3.0), C.c_float(0.0), 8,
                                                  C.c_int64(64), *ptrs)
        assert st != 0 and b"page size" in _lib.lib().ocrs_last_error(), (h, w)
