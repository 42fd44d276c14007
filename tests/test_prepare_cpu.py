"""The oracle's page preparation (oracle.pipeline.prepare_image) against its float64 restatement in tests/prepare_ref.py,
over the case lists that tests/test_gpu_prepare.py walks on the GPU, and the branches of the host dispatch
(kernels_image.hip prepare_image / prepare_image_batch) those lists are there to reach, asserted on the restated
predicates: if someone trims a list, the coverage tests below say which branch went dark.  No GPU."""
import numpy as np
import pytest

import prepare_ref as R
from oracle import pipeline as OP


def oracle(px, order):
    return np.asarray(OP.prepare_image(OP.ImageSource.from_tensor(px, order)))


# ------------------------------------------------------------------------------------------------ the oracle against float64
@pytest.mark.parametrize("fmt", R.FORMATS, ids=[R.fmt_id(*f) for f in R.FORMATS])
def test_oracle_within_the_bound_at_every_shape(fmt):
    worst = 0.0
    for name, hw, px in R.format_pages(fmt):
        out = oracle(px, fmt[1])
        assert out.shape == (1,) + hw and out.dtype == np.float32, name
        worst = max(worst, R.check_prepared(name, out, px, fmt[1]))
    print("%s: largest |oracle - float64| / tol %.3f" % (R.fmt_id(*fmt), worst))
    assert worst <= 1.0


def test_oracle_within_the_bound_on_every_rgb_triple():
    px = R.exhaustive_page()
    flat = px.reshape(-1, 3).astype(np.uint32)
    assert np.array_equal(np.sort(flat[:, 0] | (flat[:, 1] << 8) | (flat[:, 2] << 16)), np.arange(1 << 24, dtype=np.uint32)), "not every triple once"
    quads = px.reshape(-1, 4, 3)
    assert (quads[:, 0, :2] != quads[:, 1, :2]).any(axis=1).mean() > 0.99, "neighbours of a quad share R and G: channel mix-ups would pass"
    ratio = R.check_prepared("every RGB triple", oracle(px, "hwc"), px, "hwc")
    print("every RGB triple: largest |oracle - float64| / tol %.3f" % ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("order", ["hwc", "chw"])
def test_oracle_within_the_bound_on_every_grey_byte(order):
    px = R.grey_bytes(order)
    ratio = R.check_prepared("every grey byte", oracle(px, order), px, order)
    print("every grey byte, %s: largest |oracle - float64| / tol %.3f" % (order, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ float specials
@pytest.mark.parametrize("fc", R.FLOAT_FORMATS, ids=["%s-%d" % f for f in R.FLOAT_FORMATS])
def test_planted_float_words(fc):
    order, chans = fc
    base, page, plants = R.planted_page(order, chans)
    out, out_base = oracle(page, order), oracle(base, order)
    # within tol where the restatement is finite, NaN and Inf at the restatement's positions
    R.check_prepared("planted %s-%d" % fc, out, page, order)
    names = {n for n, _, _ in plants}
    assert names >= {n for n, _ in R.PLANT_WORDS}
    assert len({p for _, p, _ in plants}) == len(plants), "two plants share a pixel"
    if chans == 4:
        assert {c for _, _, c in plants} == {3}
        R.same_bits(out, out_base, "alpha-only plants against the unplanted page")
        R.same_bits(out, oracle(R.alpha_zeroed(page, order), order), "alpha-only plants against alpha zeroed")
        assert np.isfinite(out).all()
        return
    assert {c for _, _, c in plants} == set(range(chans))
    flat, flat_base = out.reshape(-1), out_base.reshape(-1)
    touched = np.zeros(flat.size, bool)
    for name, p, c in plants:
        touched[p] = True
        if name in ("qnan", "snan", "inf-inf"):
            assert np.isnan(flat[p]), (name, p, c)
        elif name in ("+inf", "-inf"):
            assert flat[p] == (np.inf if name == "+inf" else -np.inf), (name, p, c)
        else:
            assert np.isfinite(flat[p]), (name, p, c)
    R.same_bits(flat[~touched], flat_base[~touched], "pixels beside the plants")
    assert np.isfinite(flat[~touched]).all()


@pytest.mark.parametrize("fc", R.FLOAT_FORMATS, ids=["%s-%d" % f for f in R.FLOAT_FORMATS])
def test_negative_zero_and_denormal_pages(fc):
    """-0.5 + (-0.0) * w and -0.5 + denormal * w are both -0.5: neither can be told from +0.0 in the result."""
    order, chans = fc
    for name, page in R.tiny_pages(order, chans):
        out = oracle(page, order)
        assert out.view(np.uint32).tolist() == np.full((1, 5, 7), -0.5, np.float32).view(np.uint32).tolist(), name
        R.check_prepared(name, out, page, order)


# ------------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("case", R.BATCH_CASES, ids=[R.batch_id(c) for c in R.BATCH_CASES])
def test_batch_pages_are_distinct_and_within_the_bound(case):
    fmt, hw = case
    pages = R.batch_pages(fmt, hw)
    assert len(pages) == max(R.BATCH_N) and len({p.tobytes() for p in pages}) == len(pages)
    outs = [oracle(p, fmt[1]) for p in pages]
    assert len({o.tobytes() for o in outs}) == len(outs), "two pages prepare to the same bits: an order mix-up would pass"
    for i, (p, o) in enumerate(zip(pages, outs)):
        R.check_prepared("%s page %d" % (R.batch_id(case), i), o, p, fmt[1])


# ------------------------------------------------------------------------------------------------ coverage of the dispatch
def test_predicates():
    assert R.x4_ok(np.uint8, "hwc", 3, 4) and R.x4_ok(np.uint8, "hwc", 3, 1 << 24, 0x7F00, 0x100)
    for bad in ((np.float32, "hwc", 3, 4), (np.uint8, "chw", 3, 4), (np.uint8, "hwc", 1, 4), (np.uint8, "hwc", 4, 4), (np.uint8, "hwc", 3, 6)):
        assert not R.x4_ok(*bad), bad
    assert not any(R.x4_ok(np.uint8, "hwc", 3, 4, off) for off in R.OFFSETS)
    assert not any(R.x4_ok(np.uint8, "hwc", 3, 4, 0, off) for off in (4, 8, 12))
    assert [R.scalar_blocks(p) for p in (1, 256, 257, 8192 * 256, 8192 * 256 + 1)] == [1, 1, 2, 8192, 8192]
    assert [R.quad_blocks(p) for p in (4, 1024, 1028, 4096 * 1024, 4096 * 1024 + 4)] == [1, 1, 2, 4096, 4096]
    assert [R.tables(n) for n in (1, 32, 33, 64, 65)] == [1, 1, 2, 2, 3]
    assert [R.scalar_trips(p) for p in (1, 8192 * 256, 8192 * 256 + 1)] == [1, 1, 2]
    assert [R.quad_trips(p) for p in (4, 4096 * 1024, 4096 * 1024 + 4)] == [1, 1, 2]


def test_single_page_cases_reach_every_branch():
    assert len(R.FORMATS) == len(set(R.FORMATS)) == 12
    for fmt in R.FORMATS:
        planes = [hw[0] * hw[1] for hw in R.shapes_of(fmt)]
        scalar = [p for p in planes if not R.x4_ok(*fmt, p)]
        what = R.fmt_id(*fmt)
        # every plane % 4 is in the list; u8 HWC RGB takes the scalar kernel at the three that are not whole quads
        assert {p % 4 for p in planes} == {0, 1, 2, 3}, what
        assert {p % 4 for p in scalar} == ({1, 2, 3} if fmt == R.RGB8 else {0, 1, 2, 3}), what
        # one thread; one pixel short of, on and past one block
        assert {1, 255, 256, 257} <= set(planes), what
        assert {R.scalar_blocks(p) for p in scalar} >= {1, 2}, what
        # both sides of the scalar cap, and a second trip of the stride loop made by some threads only
        assert any(-(-p // R.BLOCK) < R.SCALAR_CAP for p in scalar) and any(-(-p // R.BLOCK) > R.SCALAR_CAP for p in scalar), what
        big = R.PAST_SCALAR_CAP[0] * R.PAST_SCALAR_CAP[1]
        assert big in scalar and big % 2 == 1 and R.scalar_trips(big) == 2 and big - R.SCALAR_CAP * R.BLOCK == 5123, what
    # the 4-pixel path: u8 HWC RGB alone, both values of the predicate among its cases
    quads = [hw[0] * hw[1] for hw in R.shapes_of(R.RGB8) if R.x4_ok(*R.RGB8, hw[0] * hw[1])] + [R.EXHAUSTIVE_HW[0] * R.EXHAUSTIVE_HW[1]]
    assert {R.x4_ok(*R.RGB8, hw[0] * hw[1]) for hw in R.shapes_of(R.RGB8)} == {True, False}
    assert all(not R.x4_ok(*fmt, hw[0] * hw[1]) for fmt in R.FORMATS if fmt != R.RGB8 for hw in R.shapes_of(fmt))
    assert {4, 1024, 1028} <= set(quads)                           # one quad; one full block of quads; one live thread in a second block
    assert [R.quad_blocks(p) for p in (4, 1024, 1028)] == [1, 1, 2]
    assert any(-(-(p // 4) // R.BLOCK) < R.QUAD_CAP for p in quads) and any(-(-(p // 4) // R.BLOCK) > R.QUAD_CAP for p in quads)
    past = 2049 * 2048
    assert past in quads and past // 4 - R.QUAD_CAP * R.BLOCK == 512 and R.quad_trips(past) == 2
    assert R.quad_trips(1 << 24) == 4 and R.exhaustive_page().shape == R.EXHAUSTIVE_HW + (3,)
    # the exhaustive page again off its word boundary: the scalar kernel, past its cap too
    assert all(not R.x4_ok(*R.RGB8, 1 << 24, off) for off in R.OFFSETS) and set(R.OFFSETS) == {1, 2, 3}
    assert R.scalar_trips(1 << 24) == 8


def test_batch_cases_reach_every_branch():
    assert {R.tables(n) for n in R.BATCH_N} == {1, 2, 3}
    assert {32, 33, 65} <= set(R.BATCH_N) and 1 in R.BATCH_N          # a full table, one page into a second, one into a third
    taken = {(fmt, R.x4_ok(*fmt, hw[0] * hw[1])) for fmt, hw in R.BATCH_CASES}
    assert (R.RGB8, True) in taken and (R.RGB8, False) in taken
    assert {fmt for fmt, _ in taken} == set(R.BATCH_FORMATS) and (np.float32, "chw", 3) in R.BATCH_FORMATS and (np.uint8, "chw", 1) in R.BATCH_FORMATS
    # one page off its word boundary sends the whole batch down the scalar path; the page sits in the second table
    x4_hw = [hw for fmt, hw in R.BATCH_CASES if fmt == R.RGB8 and R.x4_ok(*fmt, hw[0] * hw[1])]
    assert x4_hw
    n = max(R.BATCH_N)
    aligns = [0] * n
    assert R.batch_x4_ok(*R.RGB8, x4_hw[0][0] * x4_hw[0][1], aligns)
    aligns[R.MISALIGNED_PAGE] = 1
    assert not R.batch_x4_ok(*R.RGB8, x4_hw[0][0] * x4_hw[0][1], aligns)
    assert R.TABLE_PAGES <= R.MISALIGNED_PAGE < 2 * R.TABLE_PAGES < n
    # the batch kernels past their grid caps: one size for each family
    big = [(R.x4_ok(*R.RGB8, hw[0] * hw[1]), hw[0] * hw[1]) for hw in R.BIG_BATCH_HW]
    assert sorted(x for x, _ in big) == [False, True]
    assert all((R.quad_trips(p) if x else R.scalar_trips(p)) == 2 for x, p in big)
    for hw in R.BIG_BATCH_HW:
        a, b = R.big_batch_pages(hw)
        assert a.shape == b.shape == hw + (3,) and not np.array_equal(a, b)
