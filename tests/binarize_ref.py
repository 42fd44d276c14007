"""Adaptive binarisation, restated in numpy: the specification the library equals bit for bit.

A prepared page v (float32 [H, W], dark ink on light paper) comes back cut into ink and paper by Sauvola's local threshold.
Integers only: no floating-point arithmetic decides anything (the one float step is the bin of a pixel, §7.4).
binarize(page, radius, k_q8, keep_ink, ink_level, paper) -> (out, mask, info).  With r = radius, kq = k_q8, R = 128:

  1 bins    g = clamp(v + 0.5f, 0, 1), b = floor(g * 256f) within 0 .. 255 (+inf is bin 255, -inf bin 0); NaN is not counted.
  2 window  of pixel (y, x): [y - r, y + r] x [x - r, x + r] clipped to the page (the edge is a wall: nothing is mirrored or
            padded).  Over its counted pixels: n their number, S the sum of their bins, Q the sum of the squares.
  3 Sauvola T = m (1 + k (s / R - 1)), m = S / n, s = sqrt(Q / n - m^2), k = kq / 256; ink is b < T.  Multiplied out:
            V = n Q - S^2, A = n R (256 (b n - S) + kq S), B = kq S;  ink <=> A < B sqrt(V) <=> A < 0 or A^2 < B^2 V.
            |A| < 2^56, B^2 < 2^64, V < 2^48: the last comparison takes 128 bits.  decide() makes it with 32-bit limbs in
            uint64 arrays, decide_int() with Python integers; the tests hold one to the other.
            The strict < decides ties: a flat window (V = 0) has no ink.  kq = 0 is the plain local mean, b n < S.
  4 output  keep_ink false: ink_level (None: -0.5) on ink, paper (None: +0.5) on every other counted pixel.  keep_ink true:
            the page's own word on ink, paper elsewhere.  NaN pixels keep their word in both modes.
  mask bit 0: ink.  info: counted (pixels that are not NaN), ink, ink_fill, paper_fill.
"""
import numpy as np

F = np.float32
U = np.uint64
INFO_KEYS = ("counted", "ink", "ink_fill", "paper_fill")
MAX_RADIUS = 127
MAX_KQ = 256
R = 128


def default_params():
    return {"radius": 15, "k_q8": 87, "keep_ink": False, "ink_level": None, "paper": None}


def valid_params(radius=15, k_q8=87, keep_ink=False, ink_level=None, paper=None):
    ints = all(isinstance(v, (int, np.integer)) for v in (radius, k_q8))
    return bool(ints and 1 <= radius <= MAX_RADIUS and 0 <= k_q8 <= MAX_KQ and keep_ink in (0, 1, False, True)
                and (ink_level is None or not np.isinf(ink_level)) and (paper is None or not np.isinf(paper)))


def k_to_q8(k):
    """Sauvola's k in 1/256, rounded half up: what OcrEngine.binarize makes of its k."""
    return int(np.floor(float(k) * 256.0 + 0.5))


def bins(v):
    """int64 bins of a page, -1 for NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(v, F)
        nan = np.isnan(v)
        g = (v + F(0.5)).astype(F)
        g = np.where(g < F(0), F(0), np.where(g > F(1), F(1), g)).astype(F)
        t = (g * F(256.0)).astype(F)
        b = np.clip(np.floor(np.where(nan, F(0), t)), 0.0, 255.0).astype(np.int64)
    b[nan] = -1
    return b


def box(a, r):
    """The sum of the int64 [H, W] a over [y - r, y + r] x [x - r, x + r] clipped to the page, for every (y, x)."""
    H, W = a.shape
    I = np.zeros((H + 1, W + 1), np.int64)
    I[1:, 1:] = np.cumsum(np.cumsum(a, axis=0), axis=1)
    y0 = np.clip(np.arange(H) - r, 0, H)[:, None]
    y1 = np.clip(np.arange(H) + r + 1, 0, H)[:, None]
    x0 = np.clip(np.arange(W) - r, 0, W)[None, :]
    x1 = np.clip(np.arange(W) + r + 1, 0, W)[None, :]
    return I[y1, x1] - I[y0, x1] - I[y1, x0] + I[y0, x0]


def window_sums(page, radius):
    """-> (b, n, S, Q) as int64 [H, W]: the bins (-1: NaN) and the three sums over every pixel's window."""
    b = bins(page)
    c = b >= 0
    bb = np.where(c, b, 0)
    return b, box(c.astype(np.int64), radius), box(bb, radius), box(bb * bb, radius)


def _mul128(a, b):
    """uint64 a * b -> (high, low) 64-bit words of the 128-bit product, by 32-bit limbs (uint64 arithmetic wraps)."""
    M = U(0xFFFFFFFF)
    s = U(32)
    a0, a1, b0, b1 = a & M, a >> s, b & M, b >> s
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> s) + (p01 & M) + (p10 & M)
    return p11 + (p01 >> s) + (p10 >> s) + (mid >> s), (p00 & M) | ((mid & M) << s)


def decide(b, n, S, Q, kq):
    """The local rule on int64 arrays (b >= 0) -> bool array; exact: 128-bit products by limbs."""
    b, n, S, Q = (np.asarray(a, np.int64) for a in (b, n, S, Q))
    kq = np.int64(kq)
    V = n * Q - S * S                                # < 2^48
    A = n * np.int64(R) * (np.int64(256) * (b * n - S) + kq * S)   # |A| < 2^56
    neg = A < 0
    a = np.where(neg, 0, A).astype(U)
    Bq = (kq * S).astype(U)                          # < 2^32
    B2 = Bq * Bq                                     # < 2^64
    lh, ll = _mul128(a, a)
    rh, rl = _mul128(B2, V.astype(U))
    return neg | (lh < rh) | ((lh == rh) & (ll < rl))


def decide_int(b, n, S, Q, kq):
    """The local rule on Python integers, as the definition writes it."""
    b, n, S, Q, kq = int(b), int(n), int(S), int(Q), int(kq)
    V = n * Q - S * S
    A = n * R * (256 * (b * n - S) + kq * S)
    B = kq * S
    return A < 0 or A * A < B * B * V


def fill_word(given, otherwise):
    return np.array([otherwise if given is None or np.isnan(given) else given], F).view(np.uint32)[0]


def binarize(page, radius=15, k_q8=87, keep_ink=False, ink_level=None, paper=None, sums=None):
    """-> (out float32 [H, W], mask uint8 [H, W], info dict).  sums: window_sums(page, radius), to share it between calls."""
    if not valid_params(radius, k_q8, keep_ink, ink_level, paper):
        raise ValueError("binarize: parameters out of range")
    v = np.ascontiguousarray(page, F)
    b, n, S, Q = sums if sums is not None else window_sums(v, int(radius))
    counted = b >= 0
    ink = counted & decide(np.where(counted, b, 0), n, S, Q, int(k_q8))
    ink_word, paper_word = fill_word(ink_level, -0.5), fill_word(paper, 0.5)
    out = v.copy()
    words = out.view(np.uint32)
    words[counted & ~ink] = paper_word
    if not keep_ink:
        words[ink] = ink_word
    info = {"counted": int(counted.sum()), "ink": int(ink.sum()), "ink_fill": float(np.array([ink_word], np.uint32).view(F)[0]),
            "paper_fill": float(np.array([paper_word], np.uint32).view(F)[0])}
    return out, ink.astype(np.uint8), info


def shade(clean, low=0.3, blotch=(0.55, 0.35), depth=0.8, sigma=40.0):
    """The shaded page of DESIGN.md §7.10: the grey levels g = v + 0.5 of a clean page multiplied by an illumination that
    falls smoothly from 1 at the left edge to `low` at the right one, and by a dark blotch (a Gaussian dip of `depth`, `sigma`
    pixels wide) centred at the fractions `blotch` of the height and the width."""
    clean = np.ascontiguousarray(clean, F)
    H, W = clean.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    light = 1.0 - (1.0 - low) * xx / max(W - 1, 1)
    cy, cx = blotch[0] * H, blotch[1] * W
    light = light * (1.0 - depth * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sigma * sigma)))
    return ((clean.astype(np.float64) + 0.5) * light - 0.5).astype(F)


def tie_page():
    """(page 300 x 300, radius 127, k_q8 256, slice of rows, slice of columns): paper of bin 32 with a band of 51 columns of
    bin 192.  The window of every pixel of [127, 172] x [127, 172] lies inside the page and holds the whole band: n = 65 025,
    13 005 of them bright, so m = 64, s = 64 and T = m (1 + (s / 128 - 1)) = 32 is the pixel's own bin: A^2 = B^2 V exactly.
    The strict < makes them paper."""
    page = np.full((300, 300), F(32.5 / 256.0 - 0.5), F)
    page[:, 200:251] = F(192.5 / 256.0 - 0.5)
    return page, 127, 256, slice(127, 173), slice(127, 173)


def f_measure(got, truth):
    """F1 of the boolean `got` against the boolean `truth` (0 when nothing is found)."""
    tp = int((got & truth).sum())
    if tp == 0:
        return 0.0
    p, r = tp / int(got.sum()), tp / int(truth.sum())
    return 2.0 * p * r / (p + r)


def best_global(page, truth):
    """(the best F-measure that a global cut b < t reaches over the 255 bin thresholds t = 1 .. 255, that t)."""
    b = bins(page)
    best = (0.0, 0)
    for t in range(1, 256):
        f = f_measure((b >= 0) & (b < t), truth)
        if f > best[0]:
            best = (f, t)
    return best
