"""Stroke repair, restated in numpy: the specification the library equals bit for bit.

A prepared page v (float32 [H, W], dark ink on light paper) comes back with its ink thickened, thinned, closed or opened by
grey-level morphology over a rectangle.  Nothing is computed: a result pixel is the 32-bit word of some pixel of the source.
morph(page, op, rx, ry) -> (out, mask, info).

  1 order    pixels are ordered as 32-bit words w through the key k(w) = ~w if the sign bit is set, else w | 0x80000000:
             -inf < ... < -0.0 < +0.0 < ... < +inf, denormals in their places.  NaN of any payload is not counted: it
             enters no window, and a NaN pixel keeps its word.  The keys 0 and 0xFFFFFFFF belong to NaN words alone and
             stand for the empty window.
  2 window   of pixel (y, x): [y - ry, y + ry] x [x - rx, x + rx] clipped to the page (the edge is a wall).  0 <= rx, ry <=
             63, not both 0.  A counted pixel is in its own window.
  3 stages   lo: every counted pixel becomes the word of least key among the counted pixels of its window; hi: of the
             greatest.  A second stage reads the first stage's page under the same rules.
  4 ops      named for what happens to the (dark) ink: thicken = lo, thin = hi, close = lo then hi, open = hi then lo.
  mask bit 0: ink after (counted and < 0.0f); bit 1: the word changed.  info: counted, changed, ink_before, ink_after.

stage() takes the rows first and then the columns, which gives the rectangle because the row result is kept at every pixel,
NaN ones included (nan_beside_dark() is the page on which leaving the NaN word in place would lose a pixel); brute() walks
the rectangle itself.
"""
import numpy as np

from binarize_ref import f_measure   # noqa: F401  (part of this module's interface)
import despeckle_ref

F = np.float32
U = np.uint32
INFO_KEYS = ("counted", "changed", "ink_before", "ink_after")
OPS = ("thicken", "thin", "close", "open")
STAGES = {"thicken": ("lo",), "thin": ("hi",), "close": ("lo", "hi"), "open": ("hi", "lo")}
MAX_RADIUS = 63
SIGN = U(0x80000000)
EMPTY = {"lo": U(0xFFFFFFFF), "hi": U(0)}


def default_params():
    return {"op": "close", "rx": 1, "ry": 1}


def valid_params(op="close", rx=1, ry=1):
    ints = all(isinstance(v, (int, np.integer)) for v in (rx, ry))
    return bool(ints and op in OPS and 0 <= rx <= MAX_RADIUS and 0 <= ry <= MAX_RADIUS and (rx, ry) != (0, 0))


def words(page):
    return np.ascontiguousarray(page, F).view(U)


def is_nan(w):
    return (w & U(0x7FFFFFFF)) > U(0x7F800000)


def keys(w):
    """The ordered keys of uint32 words (of NaN words too: the caller masks them)."""
    return np.where(w & SIGN != 0, ~w, w | SIGN).astype(U)


def unkeys(k):
    return np.where(k & SIGN != 0, k ^ SIGN, ~k).astype(U)


def running(k, r, axis, which):
    """The extremum (`which`: "lo" the least, "hi" the greatest) of the uint32 keys k over [i - r, i + r] along `axis`, beyond
    the page the empty key.  Spans are doubled while they fit the window; two of them, overlapping, make it."""
    if r == 0:
        return k
    pick = np.minimum if which == "lo" else np.maximum
    k = np.moveaxis(k, axis, 0)
    n, win = k.shape[0], 2 * r + 1
    m = np.full((n + 2 * r,) + k.shape[1:], EMPTY[which], U)
    m[r:r + n] = k
    span = 1
    while span * 2 <= win:   # m[i]: the extremum of `span` keys from i on
        m = pick(m[:-span], m[span:])
        span *= 2
    return np.moveaxis(pick(m[:n], m[win - span:win - span + n]), 0, axis)


def stage(w, which, rx, ry):
    """One stage on uint32 words -> uint32 words."""
    nan = is_nan(w)
    k = np.where(nan, EMPTY[which], keys(w)).astype(U)
    k = running(running(k, rx, 1, which), ry, 0, which)   # the row result stands at NaN pixels too
    return np.where(nan, w, unkeys(k)).astype(U)


def finish(src, out):
    """(out as float32, mask, info) of the result words `out` of the source words `src`."""
    counted = ~is_nan(src)
    with np.errstate(invalid="ignore"):
        before, after = counted & (src.view(F) < F(0)), counted & (out.view(F) < F(0))
    changed = out != src
    info = {"counted": int(counted.sum()), "changed": int(changed.sum()), "ink_before": int(before.sum()), "ink_after": int(after.sum())}
    return out.view(F), (after.astype(np.uint8) | (changed.astype(np.uint8) << 1)).astype(np.uint8), info


def morph(page, op="close", rx=1, ry=1):
    """-> (out float32 [H, W], mask uint8 [H, W], info dict)."""
    if not valid_params(op, rx, ry):
        raise ValueError("morph: parameters out of range")
    src = words(page)
    out = src
    for which in STAGES[op]:
        out = stage(out, which, int(rx), int(ry))
    return finish(src, np.ascontiguousarray(out))


def brute(page, op="close", rx=1, ry=1):
    """morph() by plain loops over the rectangle of every pixel, for pages of a few hundred pixels."""
    if not valid_params(op, rx, ry):
        raise ValueError("morph: parameters out of range")
    src = words(page)
    H, W = src.shape
    cur = src
    for which in STAGES[op]:
        nan = is_nan(cur)
        k = np.where(nan, EMPTY[which], keys(cur)).astype(U)   # the empty key never wins against a counted pixel's
        nxt = cur.copy()
        for y in range(H):
            for x in range(W):
                if nan[y, x]:
                    continue
                y0, y1, x0, x1 = max(y - ry, 0), min(y + ry, H - 1) + 1, max(x - rx, 0), min(x + rx, W - 1) + 1
                window = k[y0:y1, x0:x1]
                at = np.unravel_index(np.argmin(window) if which == "lo" else np.argmax(window), window.shape)
                nxt[y, x] = cur[y0 + at[0], x0 + at[1]]
        cur = nxt
    return finish(src, cur)


def nan_beside_dark():
    """(page 3 x 3, rx 1, ry 1): paper with NaN in the centre and one dark pixel at (1, 0).  The window of (0, 1) holds the
    dark pixel, two rows and one column away; a row pass that left the NaN word in place at (1, 1) would lose it."""
    page = np.full((3, 3), F(0.25), F)
    page[1, 1] = np.nan
    page[1, 0] = F(-0.375)
    return page, 1, 1


# ---------------------------------------------------------------- the damages of DESIGN.md §7.11 and their measures
def break_strokes(clean, share, seed):
    """A share of the ink pixels (< 0) of the page, drawn with default_rng(seed), turned to paper (+0.5): broken strokes."""
    clean = np.ascontiguousarray(clean, F)
    out = clean.copy()
    out[(clean < F(0)) & (np.random.default_rng(seed).random(clean.shape) < share)] = F(0.5)
    return out


def drop_columns(clean, period):
    """The ink pixels of every `period`-th column turned to paper (+0.5): a dot-matrix or thermal head with a dead pitch."""
    clean = np.ascontiguousarray(clean, F)
    out = clean.copy()
    cols = np.arange(clean.shape[1]) % period == period - 1
    out[(clean < F(0)) & cols[None, :]] = F(0.5)
    return out


def components(ink):
    """The number of 8-connected components of the boolean [H, W] ink."""
    return len(despeckle_ref.components(ink, True)[1]) - 1
