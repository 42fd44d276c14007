"""Page preparation (kernels_image.hip prepare_image / prepare_image_batch; preprocess.rs:201-248) restated in float64,
the host dispatch restated as predicates, and the case lists the tests walk:

    out = ((-0.5 + px[0] * w[0]) + px[1] * w[1]) + px[2] * w[2]        (grey: the first term alone; alpha is never read)

Plain numpy; nothing of the library under test is imported here.  tests/test_prepare_cpu.py holds the oracle to the
restatement and asserts that the case lists still reach every branch of the dispatch; tests/test_gpu_prepare.py holds the
kernels to the oracle bit for bit and to the restatement within `tol`.
"""
import functools

import numpy as np

from geometry_ref import check64, same_bits   # noqa: F401  (same_bits is re-exported for the two test files)

U = 2.0 ** -24                      # half an ulp of 1 in float32
ITU = np.array([0.299, 0.587, 0.114], np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
def weights(dtype, chans):
    """The float32 weights of preprocess.rs:229-233, computed in float32 as the host code computes them."""
    u8 = np.dtype(dtype) == np.uint8
    if chans == 1:
        return np.array([np.float32(1) / np.float32(255) if u8 else np.float32(1)], np.float32)
    return (ITU / np.float32(255)).astype(np.float32) if u8 else ITU.copy()


def channels(px, order):
    return px.shape[2] if order == "hwc" else px.shape[0]


def plane_of(px, order):
    h, w = px.shape[:2] if order == "hwc" else px.shape[1:]
    return h * w


def prepare64(px, order):
    """-> (ref, tol), float64 [h, w].  ref = ((-0.5 + p0) + p1) + p2 with p_c = float64(px[c]) * float64(w_c).

    float32 rounds once per product and once per add, each time by at most 2^-24 of the value it rounds, and an error
    made early is carried to the end unchanged (the later operations are additions):

        tol = 2^-24 * (sum |p_c| + sum |partial sums|)

    Derived from the inputs, not measured.  What the oracle's float32 evaluation reaches of it: 0.81 over all 2^24 RGB
    triples, 0.73 over the 256 grey bytes, 0.80 on [0, 1) float noise.  Where a pixel is not finite neither is the bound; check64 compares such
    pixels by position."""
    px = np.asarray(px)
    hwc = order == "hwc"
    w = weights(px.dtype, channels(px, order)).astype(np.float64)
    shape = px.shape[:2] if hwc else px.shape[1:]
    ref = np.full(shape, -0.5, np.float64)
    acc = np.zeros(shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(len(w)):
            p = (px[..., c] if hwc else px[c]).astype(np.float64) * w[c]
            ref = ref + p
            acc += np.abs(p) + np.abs(ref)
    return ref, U * acc


CHUNK_ROWS = 512


def check_prepared(what, got, px, order, rows=CHUNK_ROWS):
    """A prepared page `got` ([h, w] or [1, h, w] float32) against prepare64 of its pixels, `rows` rows at a time so that
    a 4096 x 4096 page never needs its float64 planes whole.  -> the largest |got - ref| / tol."""
    px = np.asarray(px)
    got = got.reshape(got.shape[-2], got.shape[-1])
    h = got.shape[0]
    worst = 0.0
    for r0 in range(0, h, rows):
        r1 = min(h, r0 + rows)
        ref, tol = prepare64(px[r0:r1] if order == "hwc" else px[:, r0:r1], order)
        worst = max(worst, check64("%s rows %d..%d" % (what, r0, r1), got[r0:r1], ref, tol))
    return worst


# ------------------------------------------------------------------------------------------------ the host dispatch
BLOCK = 256
SCALAR_CAP = 8192                   # blocks of prepare_image_kernel / prepare_image_batch_kernel, one pixel per thread and trip
QUAD_CAP = 4096                     # blocks of the rgb8_x4 kernels, four pixels per thread and trip
TABLE_PAGES = 32                    # PrepareTable::kPages


def x4_ok(dtype, order, chans, plane, src_align=0, dst_align=0):
    """prepare_x4_ok: u8 RGB HWC, whole quads, a source readable as 32-bit words, a destination writable as float4.
    src_align / dst_align: the addresses, or their offsets from a 16-byte boundary."""
    return bool(np.dtype(dtype) == np.uint8 and order == "hwc" and chans == 3 and plane % 4 == 0
                and src_align % 4 == 0 and dst_align % 16 == 0)


def batch_x4_ok(dtype, order, chans, plane, src_aligns):
    """prepare_image_batch: one page that cannot take the 4-pixel path sends every page of the call down the scalar one."""
    return all(x4_ok(dtype, order, chans, plane, a) for a in src_aligns)


def _ceil(a, b):
    return -(-a // b)


def scalar_blocks(plane):
    return max(1, min(_ceil(plane, BLOCK), SCALAR_CAP))


def quad_blocks(plane):
    return min(_ceil(plane // 4, BLOCK), QUAD_CAP)


def scalar_trips(plane):
    """Trips of the stride loop made by thread 0 of block 0."""
    return _ceil(plane, scalar_blocks(plane) * BLOCK)


def quad_trips(plane):
    return _ceil(plane // 4, quad_blocks(plane) * BLOCK)


def tables(n):
    return _ceil(n, TABLE_PAGES)


# ------------------------------------------------------------------------------------------------ formats and shapes
FORMATS = [(dt, order, chans) for dt in (np.uint8, np.float32) for order in ("hwc", "chw") for chans in (1, 3, 4)]
RGB8 = (np.uint8, "hwc", 3)
# every plane % 4; one thread; one pixel short of, on and past one 256-thread block
SHAPES = [(1, 1), (1, 3), (3, 1), (1, 255), (1, 256), (1, 257), (37, 53), (2, 1023), (3, 341), (16, 64)]
# plane 2 102 275, odd: every format takes the scalar kernels, whose first 5 123 threads make a second trip
PAST_SCALAR_CAP = (1025, 2051)
# u8 HWC RGB, plane % 4 == 0: one quad; exactly one block of quads; a second block with one live thread; 512 quads past the cap
X4_SHAPES = [(2, 2), (32, 32), (4, 257), (2049, 2048)]
EXHAUSTIVE_HW = (4096, 4096)        # four trips of the x4 stride loop
OFFSETS = (1, 2, 3)                 # bytes a u8 source is moved off its word boundary: the scalar kernel


def fmt_id(dtype, order, chans):
    return "%s-%s-%d" % ("u8" if np.dtype(dtype) == np.uint8 else "f32", order, chans)


def hw_id(hw):
    return "%dx%d" % hw


def noise(dtype, order, chans, hw, seed):
    """u8: uniform bytes; f32: uniform [0, 1)."""
    shape = hw + (chans,) if order == "hwc" else (chans,) + hw
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.random(shape, dtype=np.float32)


def shapes_of(fmt):
    """The shapes a format is run at: SHAPES and the one past the scalar cap; u8 HWC RGB also the x4 ones."""
    return SHAPES + [PAST_SCALAR_CAP] + (X4_SHAPES if fmt == RGB8 else [])


def format_pages(fmt):
    """[(id, hw, pixels)] of one format, made when asked for (the largest is 34 MB)."""
    dt, order, chans = fmt
    for k, hw in enumerate(shapes_of(fmt)):
        yield "%s %s" % (fmt_id(*fmt), hw_id(hw)), hw, noise(dt, order, chans, hw, 1000 * FORMATS.index(fmt) + k)


@functools.lru_cache(maxsize=None)
def exhaustive_page():
    """Every RGB triple once, [4096, 4096, 3] u8 HWC, in a seeded random permutation: in counting order the four pixels of
    a quad would share R and G, and a mix-up between neighbouring pixels' channels would pass."""
    t = np.random.default_rng(24).permutation(1 << 24).astype(np.uint32)
    px = np.stack([t & 0xFF, (t >> 8) & 0xFF, t >> 16], axis=-1).astype(np.uint8).reshape(EXHAUSTIVE_HW + (3,))
    px.setflags(write=False)
    return px


def grey_bytes(order):
    """The 256 grey bytes as a 16 x 16 x 1 page."""
    a = np.arange(256, dtype=np.uint8)
    return a.reshape(16, 16, 1) if order == "hwc" else a.reshape(1, 16, 16)


# ------------------------------------------------------------------------------------------------ float pages
PLANT_HW = (37, 53)
PLANT_WORDS = [("qnan", 0x7FC00000), ("snan", 0x7FA00001), ("+inf", 0x7F800000), ("-inf", 0xFF800000), ("-0", 0x80000000),
               ("denormal", 0x00012345), ("+1e30", int(np.float32(1e30).view(np.uint32))),
               ("-1e30", int(np.float32(-1e30).view(np.uint32))), ("2", int(np.float32(2).view(np.uint32))),
               ("-1", int(np.float32(-1).view(np.uint32)))]
FLOAT_FORMATS = [(order, chans) for order in ("hwc", "chw") for chans in (1, 3, 4)]
OPPOSITE_INF_PIXEL = 1900           # flat index of the RGB pixel with +inf in R and -inf in G: their sum is a NaN


def _word_at(page, order, p, c):
    """The uint32 view of channel c of pixel p (flat index) of a float32 page."""
    v = page.view(np.uint32)
    y, x = divmod(p, PLANT_HW[1])
    return (v, (y, x, c)) if order == "hwc" else (v, (c, y, x))


def planted_page(order, chans):
    """-> (base, planted, plants): uniform noise at 37 x 53, and a copy with every word of PLANT_WORDS written once into
    every channel position, each at a pixel of its own (the words go in as bits: a signalling NaN stays one).  With four
    channels the words go into alpha ONLY: nothing of them may reach the result.  plants: [(name, pixel, channel)]."""
    base = noise(np.float32, order, chans, PLANT_HW, 500 + 10 * chans + (order == "hwc"))
    page = base.copy()
    targets = (3,) if chans == 4 else tuple(range(chans))
    plants, k = [], 0
    for name, word in PLANT_WORDS:
        for c in targets:
            p = 5 + 59 * k
            v, i = _word_at(page, order, p, c)
            v[i] = word
            plants.append((name, p, c))
            k += 1
    if chans == 3:
        for c, word in ((0, 0x7F800000), (1, 0xFF800000)):
            v, i = _word_at(page, order, OPPOSITE_INF_PIXEL, c)
            v[i] = word
        plants.append(("inf-inf", OPPOSITE_INF_PIXEL, 0))
    assert 5 + 59 * (k - 1) < OPPOSITE_INF_PIXEL < PLANT_HW[0] * PLANT_HW[1]
    return base, page, plants


def alpha_zeroed(page, order):
    out = page.copy()
    if order == "hwc":
        out[..., 3] = 0
    else:
        out[3] = 0
    return out


def tiny_pages(order, chans):
    """[(name, page)] at 5 x 7: every word -0.0, and every word a denormal of either sign."""
    shape = (5, 7, chans) if order == "hwc" else (chans, 5, 7)
    rng = np.random.default_rng(77 + chans)
    den = (rng.integers(1, 1 << 23, shape, dtype=np.uint32) | (rng.integers(0, 2, shape, dtype=np.uint32) << 31)).view(np.float32)
    return [("all -0", np.full(shape, -0.0, np.float32)), ("all denormal", den)]


# ------------------------------------------------------------------------------------------------ batches
BATCH_N = (1, 2, 32, 33, 65)        # pages 32 and 64 are the first of a second and third table
BATCH_HW = [(16, 17), (37, 53)]     # plane 272: x4 for u8 HWC RGB; plane 1961: scalar
BATCH_FORMATS = [RGB8, (np.float32, "chw", 3), (np.uint8, "chw", 1)]
BATCH_CASES = [(fmt, hw) for fmt in BATCH_FORMATS for hw in BATCH_HW]
MISALIGNED_PAGE = 48                # of 65: in the middle, and in the second table


def batch_id(case):
    return "%s %s" % (fmt_id(*case[0]), hw_id(case[1]))


@functools.lru_cache(maxsize=None)
def batch_pages(fmt, hw):
    """max(BATCH_N) distinct pages of one format and size; a batch of n is the first n."""
    dt, order, chans = fmt
    k = 100 * BATCH_FORMATS.index(fmt) + BATCH_HW.index(hw)
    pages = [noise(dt, order, chans, hw, 7000 + 1000 * k + i) for i in range(max(BATCH_N))]
    for p in pages:
        p.setflags(write=False)
    return pages


# two u8 HWC RGB pages per call past a grid cap: the batch kernels' stride loops, with a second page in blockIdx.y
BIG_BATCH_HW = [X4_SHAPES[-1], PAST_SCALAR_CAP]


def big_batch_pages(hw):
    return [noise(np.uint8, "hwc", 3, hw, 9000 + 10 * BIG_BATCH_HW.index(hw) + i) for i in range(2)]
