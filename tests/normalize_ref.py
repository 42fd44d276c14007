"""Page normalisation, restated in numpy: the specification the library equals bit for bit.

A prepared page v (float32 [H, W], nominally -0.5 = black .. 0.5 = white) becomes a page of the same size with ink at
-0.5 and paper at +0.5, dark text on a light page whatever came in.  Every float32 operation is rounded on its own; all
counting is in integers.  normalize(page, tile, polarity, flatten, levels) -> (out float32 [H, W], info dict).

  bins      g = clamp(v + 0.5f, 0, 1) (NaN stays NaN); bin = floor(g * 256f) kept within 0 .. 255; NaN is not counted.
            Tiles are T x T from the page origin, edge tiles partial.  pct(h, num, den): the smallest bin whose cumulative
            count c has c * den >= num * n; -1 for an empty histogram.
  polarity  auto: every non-empty tile adds pct(19,20) + pct(1,20) - 2 pct(1,2) to the vote; dark iff the vote > 0.  keep:
            light, invert: dark; both leave the vote 0.  On a dark page g = clamp(0.5f - v, 0, 1) and every histogram
            of pass 1 is read mirrored (bin 255 - b).
  flatten   white bin of a tile: pct(3,4) of its effective histogram; Wg the same of the page's.  A present tile's value is
            max(white, Wg // 2), then the maximum over the present tiles of its 3 x 3 neighbourhood; an empty tile takes
            max(Wg, 0).  Level L = (bin + 1) / 256.  B = the bilinear interpolation of L over tile centres;
            u = min(g / B, 1).  Off: u = g.
  levels    histogram of u, binned as above, over the page; lo = pct(1,100), hi = pct(1,2); if hi > lo >= 0:
            out = clamp((u - lo/256) / (hi/256 - lo/256), 0, 1) - 0.5f, else out = u - 0.5f.  Off: out = u - 0.5f.
  neither   flatten and levels both off: the page's own words, the sign bit flipped on a dark page (no arithmetic).
"""
import numpy as np

F = np.float32
POLARITIES = ("auto", "keep", "invert")


def default_params():
    return {"tile": 64, "polarity": "auto", "flatten": True, "levels": True}


def valid_tile(t):
    return isinstance(t, (int, np.integer)) and 16 <= t <= 256 and (t & (t - 1)) == 0


def clamp01(a):
    """0 below 0, 1 above 1, NaN stays."""
    a = np.asarray(a, F)
    with np.errstate(invalid="ignore"):
        return np.where(a < F(0), F(0), np.where(a > F(1), F(1), a)).astype(F)


def grey(v, dark):
    with np.errstate(invalid="ignore", over="ignore"):
        return clamp01((F(0.5) - v) if dark else (v + F(0.5)))


def bins(g):
    """int64 bins, -1 for NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(g, F) * F(256.0)).astype(F)
        nan = np.isnan(t)
        b = np.floor(np.where(nan, F(0), t))
        b = np.clip(b, 0.0, 255.0).astype(np.int64)
    b[nan] = -1
    return b


def hist(b):
    b = b[b >= 0]
    return np.bincount(b.reshape(-1), minlength=256).astype(np.int64)


def pct(h, num, den):
    h = [int(x) for x in h]
    n = sum(h)
    if n == 0:
        return -1
    c = 0
    for b in range(256):
        c += h[b]
        if c * den >= num * n:
            return b
    raise AssertionError("unreachable")


def pct_many(h, num, den):
    """pct over the last axis of int64 [..., 256] -> int64 [...]."""
    c = np.cumsum(h, axis=-1)
    n = c[..., -1]
    first = np.argmax(c * den >= (num * n)[..., None], axis=-1)
    return np.where(n > 0, first, -1).astype(np.int64)


def tile_hists(b, T):
    """[th, tw, 256] int64."""
    H, W = b.shape
    th, tw = -(-H // T), -(-W // T)
    tile = (np.arange(H)[:, None] // T) * tw + np.arange(W)[None, :] // T
    keep = b >= 0
    return np.bincount((tile * 256 + b)[keep], minlength=th * tw * 256).astype(np.int64).reshape(th, tw, 256)


def level_grid(th_eff, wg, T):
    """th_eff [th, tw, 256] effective tile histograms -> level bins int64 [th, tw]."""
    th, tw = th_eff.shape[:2]
    white = pct_many(th_eff, 3, 4)
    present = white >= 0
    floored = np.where(present, np.maximum(white, wg // 2), -1)
    grid = np.zeros((th, tw), np.int64)
    for i in range(th):
        for j in range(tw):
            if present[i, j]:
                grid[i, j] = floored[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2].max()
            else:
                grid[i, j] = max(wg, 0)
    return grid


def background(grid, H, W, T):
    th, tw = grid.shape
    L = ((grid + 1).astype(F) / F(256.0)).astype(F)
    inv = F(1.0) / F(T)

    def axis(n, cells):
        f = (np.arange(n, dtype=F) + F(0.5)) * inv - F(0.5)
        f = np.clip(f, F(0), F(cells - 1)).astype(F)
        i0 = np.floor(f).astype(np.int64)
        i1 = np.minimum(i0 + 1, cells - 1)
        return i0, i1, (f - i0.astype(F)).astype(F)

    y0, y1, wy = axis(H, th)
    x0, x1, wx = axis(W, tw)
    wy, wx = wy[:, None], wx[None, :]
    one = F(1.0)
    top = ((one - wx) * L[y0][:, x0] + wx * L[y0][:, x1]).astype(F)
    bot = ((one - wx) * L[y1][:, x0] + wx * L[y1][:, x1]).astype(F)
    return ((one - wy) * top + wy * bot).astype(F)


def normalize(page, tile=64, polarity="auto", flatten=True, levels=True):
    v = np.ascontiguousarray(page, F)
    assert v.ndim == 2 and valid_tile(tile) and polarity in POLARITIES
    H, W = v.shape
    T = int(tile)
    th = tile_hists(bins(grey(v, False)), T)
    counted = int(th.sum())
    vote = 0
    if polarity == "auto":
        per_tile = pct_many(th, 19, 20) + pct_many(th, 1, 20) - 2 * pct_many(th, 1, 2)
        vote = int(per_tile[th.sum(axis=-1) > 0].sum())
        dark = vote > 0
    else:
        dark = polarity == "invert"
    eff = th[:, :, ::-1] if dark else th
    wg = pct(eff.reshape(-1, 256).sum(axis=0), 3, 4)
    info = {"dark": int(dark), "vote": int(vote), "white": int(wg), "lo": -1, "hi": -1, "counted": counted}
    if not flatten and not levels:
        out = v.copy()
        if dark:
            out = (out.view(np.uint32) ^ np.uint32(0x80000000)).view(F)
        return out, info
    g = grey(v, dark)
    if flatten:
        B = background(level_grid(eff, wg, T), H, W, T)
        with np.errstate(invalid="ignore"):
            q = (g / B).astype(F)
            u = np.where(q > F(1), F(1), q).astype(F)
    else:
        u = g
    half = F(0.5)
    if levels:
        hu = hist(bins(u))
        lo, hi = pct(hu, 1, 100), pct(hu, 1, 2)
        info["lo"], info["hi"] = lo, hi
        if hi > lo >= 0:
            a = F(lo) / F(256.0)
            d = F(hi) / F(256.0) - a
            return (clamp01(((u - a) / d).astype(F)) - half).astype(F), info
    return (u - half).astype(F), info


def shade(page):
    """The issue's synthetic shadow and contrast cut on a prepared page: g (0.45 + 0.55 (x/W) (0.5 + 0.5 y/H)) 0.8 + 0.05
    on g = page + 0.5, in float64, rounded once to float32."""
    H, W = page.shape
    g = page.astype(np.float64) + 0.5
    x = np.arange(W, dtype=np.float64)[None, :] / W
    y = np.arange(H, dtype=np.float64)[:, None] / H
    return (g * (0.45 + 0.55 * x * (0.5 + 0.5 * y)) * 0.8 + 0.05 - 0.5).astype(F)
