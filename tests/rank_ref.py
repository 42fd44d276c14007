"""Grain removal, restated in numpy: the specification the library equals bit for bit.

A prepared page v (float32 [H, W], dark ink on light paper) comes back with its grain removed by a rank filter over a
rectangle: a median, a percentile, or either applied to outliers only.  Nothing is computed: a result pixel is the 32-bit
word of some pixel of the source.  rank(page, rx, ry, percent, tail) -> (out, mask, info).

  1 order    stroke repair's (morph_ref): words w are ordered through the key k(w) = ~w if the sign bit is set, else
             w | 0x80000000.  NaN of any payload is not counted: it enters no window, and a NaN pixel keeps its word.
  2 window   of pixel (y, x): [y - ry, y + ry] x [x - rx, x + rx] clipped to the page.  0 <= rx, ry <= 7, not both 0: at
             most 225 keys.  A counted pixel is in its own window, so the number n of counted pixels in it is >= 1.
  3 rank     at(p) = (p (n - 1) + 50) div 100 in integers; s[0 .. n - 1] the window's counted keys in ascending order.  The
             filter's value is the word of s[at(percent)], percent 0 .. 100: 0 the least key, 100 the greatest, 50 the
             median (of an even n the upper one).  Equal keys are equal words: ties need no rule.
  4 sparing  tail 0 .. 50.  0: every counted pixel takes the filter's value.  tail >= 1: with lt the number of window keys
             under the pixel's own and le the number under or equal, the pixel is spared (keeps its word) iff
             lt <= at(100 - tail) and le - 1 >= at(tail): its own ranks meet the central part of its window.
  mask bit 0: ink after (counted and < 0.0f); bit 1: the word changed.  info: counted, changed, ink_before, ink_after,
  spared (counted pixels kept by rule 4; 0 at tail 0).

rank() sorts the stacked planes of the window; brute() walks the rectangle of every pixel with plain loops.
"""
import numpy as np

from binarize_ref import best_global, binarize, f_measure   # noqa: F401  (part of this module's interface)
from morph_ref import components, is_nan, keys, morph, unkeys, words   # noqa: F401
import morph_ref

F = np.float32
U = np.uint32
INFO_KEYS = ("counted", "changed", "ink_before", "ink_after", "spared")
MAX_RADIUS = 7
EMPTY = U(0xFFFFFFFF)


def default_params():
    return {"rx": 1, "ry": 1, "percent": 50, "tail": 20}


def valid_params(rx=1, ry=1, percent=50, tail=20):
    ints = all(isinstance(v, (int, np.integer)) for v in (rx, ry, percent, tail))
    return bool(ints and 0 <= rx <= MAX_RADIUS and 0 <= ry <= MAX_RADIUS and (rx, ry) != (0, 0) and 0 <= percent <= 100 and 0 <= tail <= 50)


def at(p, n):
    """The rank that percent p names among n >= 1 keys (n: an int or an integer array)."""
    return (p * (n - 1) + 50) // 100


def windows(page, rx, ry):
    """What rank() needs of the page's windows, for sharing between calls of other percents and tails -> (s, n, lt, le): the
    keys of every pixel's window in ascending order [H, W, (2 ry + 1)(2 rx + 1)] (empty keys last), the number of counted
    ones, and the numbers under and under or equal the pixel's own key."""
    src = words(page)
    H, W = src.shape
    k = np.where(is_nan(src), EMPTY, keys(src)).astype(U)
    padded = np.full((H + 2 * ry, W + 2 * rx), EMPTY, U)
    padded[ry:ry + H, rx:rx + W] = k
    planes = np.stack([padded[dy:dy + H, dx:dx + W] for dy in range(2 * ry + 1) for dx in range(2 * rx + 1)], axis=-1)
    own = k[..., None]
    lt, le = (planes < own).sum(-1), ((planes <= own) & (planes != EMPTY)).sum(-1)
    return np.sort(planes, axis=-1), (planes != EMPTY).sum(-1), lt, le


def finish(src, out, spared):
    out, mask, info = morph_ref.finish(src, np.ascontiguousarray(out))
    info["spared"] = int(spared.sum())
    return out, mask, info


def rank(page, rx=1, ry=1, percent=50, tail=20, win=None):
    """-> (out float32 [H, W], mask uint8 [H, W], info dict).  win: windows(page, rx, ry), to share it between calls."""
    if not valid_params(rx, ry, percent, tail):
        raise ValueError("rank: parameters out of range")
    src = words(page)
    nan = is_nan(src)
    s, n, lt, le = windows(page, int(rx), int(ry)) if win is None else win
    n = np.maximum(n, 1)   # of a NaN pixel's window, which decides nothing
    value = np.take_along_axis(s, at(percent, n)[..., None], -1)[..., 0]
    spared = np.zeros(src.shape, bool)
    if tail >= 1:
        spared = ~nan & (lt <= at(100 - tail, n)) & (le - 1 >= at(tail, n))
    return finish(src, np.where(nan | spared, src, unkeys(value)).astype(U), spared)


def brute(page, rx=1, ry=1, percent=50, tail=20):
    """rank() by plain loops over the rectangle of every pixel, for pages of a few hundred pixels."""
    if not valid_params(rx, ry, percent, tail):
        raise ValueError("rank: parameters out of range")
    src = words(page)
    H, W = src.shape
    nan = is_nan(src)
    k = keys(src)
    out = src.copy()
    spared = np.zeros(src.shape, bool)
    for y in range(H):
        for x in range(W):
            if nan[y, x]:
                continue
            s = []
            for yy in range(max(y - ry, 0), min(y + ry, H - 1) + 1):
                for xx in range(max(x - rx, 0), min(x + rx, W - 1) + 1):
                    if not nan[yy, xx]:
                        s.append((int(k[yy, xx]), int(src[yy, xx])))
            s.sort()
            n, own = len(s), int(k[y, x])
            lt, le = sum(1 for q, _ in s if q < own), sum(1 for q, _ in s if q <= own)
            if tail >= 1 and lt <= (((100 - tail) * (n - 1) + 50) // 100) and le - 1 >= ((tail * (n - 1) + 50) // 100):
                spared[y, x] = True
            else:
                out[y, x] = s[(percent * (n - 1) + 50) // 100][1]
    return finish(src, out, spared)


# ---------------------------------------------------------------- the damages of DESIGN.md §7.13
def grain(clean, sigma, seed):
    """Gaussian noise of standard deviation `sigma` (default_rng(seed)) added to the page, clipped to [-0.5, 0.5]: sensor
    noise of a photo taken in poor light."""
    clean = np.ascontiguousarray(clean, F)
    g = np.random.default_rng(seed).normal(0.0, sigma, clean.shape)
    return np.clip(clean.astype(np.float64) + g, -0.5, 0.5).astype(F)


def salt_and_pepper(clean, share, seed):
    """A share of the pixels, drawn with default_rng(seed), set to paper (+0.5, salt) or to ink (-0.5, pepper), half each."""
    clean = np.ascontiguousarray(clean, F)
    out = clean.copy()
    u = np.random.default_rng(seed).random(clean.shape)
    out[u < share / 2] = F(0.5)
    out[(u >= share / 2) & (u < share)] = F(-0.5)
    return out


def halftone(clean, pitch):
    """A screen of one-pixel dots of ink (-0.5) every `pitch` pixels both ways, every other row of dots shifted by half the
    pitch, under the text: a pixel of the clean page that is ink stays as it is."""
    clean = np.ascontiguousarray(clean, F)
    yy, xx = np.mgrid[0:clean.shape[0], 0:clean.shape[1]]
    dots = (yy % pitch == 0) & ((xx + (yy // pitch % 2) * (pitch // 2)) % pitch == 0)
    out = clean.copy()
    out[dots & (clean >= F(0))] = F(-0.5)
    return out


def hairlines(clean):
    """-> (page, lines): one-pixel lines of ink (-0.5) drawn over the page: a horizontal one every 64 rows, a vertical one
    every 64 columns, and the diagonals from the corners of every 128-pixel square; `lines` is the boolean mask of their pixels."""
    clean = np.ascontiguousarray(clean, F)
    yy, xx = np.mgrid[0:clean.shape[0], 0:clean.shape[1]]
    lines = (yy % 64 == 32) | (xx % 64 == 32) | ((yy - xx) % 128 == 0) | ((yy + xx) % 128 == 0)
    out = clean.copy()
    out[lines] = F(-0.5)
    return out, lines
