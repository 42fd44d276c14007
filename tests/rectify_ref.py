"""Rectified line crops by their definition, in numpy, for the tests.  This file is the specification:
the library equals it bit for bit.

A line is n >= 1 word rects (cx, cy, upx, upy, w, h), float32, in the given order; H is the recogniser's input height.

Frame — float64 from the float32 values, every operation as written, sums in word order, only + - * / sqrt:

    mx = sum(cx) / n, my = sum(cy) / n, Sxx = sum((cx - mx)^2), Sxy = sum((cx - mx) * (cy - my))
    n >= 2 and Sxx > 0:  m = Sxy / Sxx, L = sqrt(1 + m * m), a = (1 / L, m / L)
    otherwise:           a = (-upy0, upx0) of the first word, negated if a.x < 0, or a.x == 0 and a.y < 0
    nv = (-a.y, a.x)                              (down the page for an upright line)
    word corners:  px = cx + sw * ((w / 2) * -upy) + sh * ((h / 2) * upx)
                   py = cy + sw * ((w / 2) * upx)  + sh * ((h / 2) * upy)       sw, sh in {-1, +1}
    s = px * a.x + py * a.y, t = px * nv.x + py * nv.y; per word [sa, sb], [ta, tb]; over the line s_min .. t_max
    Wl = s_max - s_min, Hl = t_max - t_min, cw = ceil(Wl), ch = ceil(Hl) (capped at 2^31 - 1)
    rw = resized_line_width(cw, ch, H)            (recognition.rs:58-75, clamp to 10 .. 2400)

Empty line — an input value that is not finite, cw <= 0 or ch <= 0: every pixel is -0.5, there are no char boxes, and
the width is what the plain crop gives a line whose bounding box has a side of zero: resized_line_width(max(cw, 0),
max(ch, 0), H) with cw = ch = 0 for input that is not finite — 0 (no input, no text) for 0 x 0, 10 for 0 x ch, 2400
for cw x 0.

Sampling map — six float32 coefficients, each the rounding of a float64:

    x0 = s_min * a.x + t_min * nv.x - 0.5,  ax = a.x * Wl / rw,  bx = nv.x * Hl / H;  y0, ay, by with .y

and, in float32 with every operation rounded on its own, for output pixel (oy, ox), ox < rw:

    fx = ox + 0.5, fy = oy + 0.5, X = (x0 + ax * fx) + bx * fy, Y likewise
    ix = floor(X), wx = X - ix, iy = floor(Y), wy = Y - iy
    taps t00 = page[iy, ix], t01 = page[iy, ix + 1], t10 = page[iy + 1, ix], t11 = page[iy + 1, ix + 1]; outside: -0.5
    top = (1 - wx) * t00 + wx * t01, bot = (1 - wx) * t10 + wx * t11, v = (1 - wy) * top + wy * bot

Mask — per word, float64: c0 = ceil((sa - s_min) * rw / Wl - 0.5), c1 = floor((sb - s_min) * rw / Wl - 0.5) clipped to
[0, rw - 1]; r0, r1 the same with t, H, Hl, clipped to [0, H - 1]; a word with c0 > c1 or r0 > r1 covers nothing.  lo(c) /
hi(c): min r0 / max r1 over the words covering column c; an uncovered column takes them over the nearest covered column
on its left and the nearest on its right, whichever exist; no covered column at all: [0, H - 1] everywhere.  The output
is v where lo(ox) <= oy <= hi(ox), else -0.5; columns rw .. out_w - 1 are -0.5.

Char boxes — start_x = pos * downsample, end_x = the next step's, rw for the last (text_line_from_result); a char with
start_x >= rw is dropped; the quad s in [s_min + start_x * Wl / rw, s_min + end_x * Wl / rw], t in [t_min, t_max] is
mapped to the page in float64 (x = s * a.x + t * nv.x, y = s * a.y + t * nv.y); left / top = floor of the minimum,
right / bottom = ceil of the maximum (clamped to int32).
"""
import math

import numpy as np

BLACK_VALUE = np.float32(-0.5)
F32 = np.float32
I32_MAX = 2147483647


def resized_line_width(orig_width, orig_height, height):
    """recognition.rs:58-75 in float32."""
    with np.errstate(all="ignore"):
        v = F32(height) * (F32(orig_width) / F32(orig_height))
    if v != v:
        return 0
    return int(min(max(v, F32(10.0)), F32(2400.0)))


class Frame:
    """empty, a (ax, ay), extents (s_min, s_max, t_min, t_max), rw, coef float32 [6] (x0, ax, bx, y0, ay, by), ranges int32
    [n, 4] (c0, c1, r0, r1 per word; c0 > c1: covers nothing).  An empty frame has zeros everywhere but rw."""

    def __init__(self, n):
        self.empty = True
        self.a = (0.0, 0.0)
        self.extents = (0.0, 0.0, 0.0, 0.0)
        self.rw = 0
        self.coef = np.zeros(6, np.float32)
        self.ranges = np.zeros((n, 4), np.int32)
        self.ranges[:, 0] = 1
        self.ranges[:, 2] = 1


def _capped_ceil(v):
    return int(min(math.ceil(v), float(I32_MAX)))


def line_frame(words, H):
    w32 = np.asarray(words, np.float32).reshape(-1, 6)
    n = len(w32)
    assert n >= 1
    H = int(H)
    fr = Frame(n)
    if not np.all(np.isfinite(w32)):
        fr.rw = resized_line_width(0, 0, H)
        return fr
    W = [[float(v) for v in row] for row in w32]   # float64 from the float32 values
    sx = sy = 0.0
    for r in W:
        sx = sx + r[0]
        sy = sy + r[1]
    mx, my = sx / n, sy / n
    Sxx = Sxy = 0.0
    for r in W:
        Sxx = Sxx + (r[0] - mx) * (r[0] - mx)
        Sxy = Sxy + (r[0] - mx) * (r[1] - my)
    if n >= 2 and Sxx > 0.0:
        m = Sxy / Sxx
        L = math.sqrt(1.0 + m * m)
        ax, ay = 1.0 / L, m / L
    else:
        ax, ay = -W[0][3], W[0][2]
        if ax < 0.0 or (ax == 0.0 and ay < 0.0):
            ax, ay = -ax, -ay
    nx, ny = -ay, ax
    ext = []
    for cx, cy, upx, upy, w, h in W:
        hx, hy = (w / 2.0) * -upy, (w / 2.0) * upx
        vx, vy = (h / 2.0) * upx, (h / 2.0) * upy
        ss, ts = [], []
        for sw in (-1.0, 1.0):
            for sh in (-1.0, 1.0):
                px = cx + sw * hx + sh * vx
                py = cy + sw * hy + sh * vy
                ss.append(px * ax + py * ay)
                ts.append(px * nx + py * ny)
        ext.append((min(ss), max(ss), min(ts), max(ts)))
    s_min, s_max = min(e[0] for e in ext), max(e[1] for e in ext)
    t_min, t_max = min(e[2] for e in ext), max(e[3] for e in ext)
    Wl, Hl = s_max - s_min, t_max - t_min
    cw, ch = _capped_ceil(Wl), _capped_ceil(Hl)
    if cw <= 0 or ch <= 0:
        fr.rw = resized_line_width(max(cw, 0), max(ch, 0), H)
        return fr
    rw = resized_line_width(cw, ch, H)
    fr.empty = False
    fr.a = (ax, ay)
    fr.extents = (s_min, s_max, t_min, t_max)
    fr.rw = rw
    with np.errstate(over="ignore"):
        fr.coef = np.array([s_min * ax + t_min * nx - 0.5, ax * Wl / rw, nx * Hl / H,
                            s_min * ay + t_min * ny - 0.5, ay * Wl / rw, ny * Hl / H], np.float64).astype(np.float32)

    def clip(lo, hi, top):   # float64 -> ints in [0, top]
        return int(max(lo, 0.0)), int(min(hi, float(top)))

    for i, (sa, sb, ta, tb) in enumerate(ext):
        c0, c1 = clip(math.ceil((sa - s_min) * rw / Wl - 0.5), math.floor((sb - s_min) * rw / Wl - 0.5), rw - 1)
        r0, r1 = clip(math.ceil((ta - t_min) * H / Hl - 0.5), math.floor((tb - t_min) * H / Hl - 0.5), H - 1)
        if c0 > c1 or r0 > r1:
            c0, c1, r0, r1 = 1, 0, 1, 0
        fr.ranges[i] = (c0, c1, r0, r1)
    return fr


def column_table(fr, H):
    """-> lo [rw], hi [rw] (int): the rows of every column that the mask keeps."""
    rw = fr.rw
    lo = np.full(rw, H, np.int64)
    hi = np.full(rw, -1, np.int64)
    for c0, c1, r0, r1 in fr.ranges:
        if c0 > c1:
            continue
        lo[c0:c1 + 1] = np.minimum(lo[c0:c1 + 1], r0)
        hi[c0:c1 + 1] = np.maximum(hi[c0:c1 + 1], r1)
    covered = hi >= 0
    if not covered.any():
        return np.zeros(rw, np.int64), np.full(rw, H - 1, np.int64)
    cols = np.nonzero(covered)[0]
    out_lo, out_hi = lo.copy(), hi.copy()
    for c in np.nonzero(~covered)[0]:
        k = np.searchsorted(cols, c)
        near = ([cols[k - 1]] if k > 0 else []) + ([cols[k]] if k < len(cols) else [])
        out_lo[c] = min(lo[j] for j in near)
        out_hi[c] = max(hi[j] for j in near)
    return out_lo, out_hi


def sample(page, coef, rw, H):
    """The bilinear gather of the definition, unmasked: [H, rw] float32."""
    page = np.asarray(page, np.float32)
    ph, pw = page.shape
    x0, ax, bx, y0, ay, by = (F32(c) for c in coef)
    fx = (np.arange(rw, dtype=np.float32) + F32(0.5))[None, :]
    fy = (np.arange(H, dtype=np.float32) + F32(0.5))[:, None]
    with np.errstate(all="ignore"):
        X = ((x0 + ax * fx) + bx * fy).astype(np.float32)
        Y = ((y0 + ay * fx) + by * fy).astype(np.float32)
        fix, fiy = np.floor(X), np.floor(Y)
        wx, wy = (X - fix).astype(np.float32), (Y - fiy).astype(np.float32)
        inside = (fix >= -1) & (fix <= pw) & (fiy >= -1) & (fiy <= ph)   # else no tap is on the page
        ix = np.where(inside, fix, -2).astype(np.int64)
        iy = np.where(inside, fiy, -2).astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < ph) & (xx >= 0) & (xx < pw)
        return np.where(ok, page[np.clip(yy, 0, ph - 1), np.clip(xx, 0, pw - 1)], BLACK_VALUE).astype(np.float32)

    t00, t01, t10, t11 = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        top = ((one - wx) * t00).astype(np.float32) + (wx * t01).astype(np.float32)
        bot = ((one - wx) * t10).astype(np.float32) + (wx * t11).astype(np.float32)
        return (((one - wy) * top).astype(np.float32) + (wy * bot).astype(np.float32)).astype(np.float32)


def crop(page, words, H, out_w=None):
    """The rectified crop of one line: [H, out_w] float32 (out_w=None: rw, the prepare_recognition_input form)."""
    fr = line_frame(words, H)
    out_w = fr.rw if out_w is None else int(out_w)
    out = np.full((H, out_w), BLACK_VALUE, np.float32)
    if fr.empty or fr.rw == 0:
        return out
    v = sample(page, fr.coef, fr.rw, H)
    lo, hi = column_table(fr, H)
    oy = np.arange(H)[:, None]
    keep = (oy >= lo[None, :]) & (oy <= hi[None, :])
    out[:, :fr.rw] = np.where(keep, v, BLACK_VALUE)
    return out


def group_width(rw):
    return -(-rw // 50) * 50   # next_multiple_of(50), recognition.rs:437


def char_boxes(fr, group_w, ctc_len, steps):
    """steps: [(label, pos)] -> [(step index, (top, left, bottom, right))] of the chars that are kept."""
    if fr.empty or not steps or ctc_len == 0:
        return []
    s_min, s_max, t_min, t_max = fr.extents
    ax, ay = fr.a
    nx, ny = -ay, ax
    Wl, rw = s_max - s_min, fr.rw
    downsample = int(np.round(F32(group_w) / F32(ctc_len)))   # (never a tie away from numpy's rounding: checked below)
    q = float(F32(group_w) / F32(ctc_len))
    if q - math.floor(q) == 0.5:
        downsample = int(math.floor(q)) + 1   # f32::round: half away from zero
    out = []

    def to_i32(v):
        return int(min(max(v, -2147483648.0), float(I32_MAX)))

    for i, (_, pos) in enumerate(steps):
        start_x = pos * downsample
        end_x = steps[i + 1][1] * downsample if i + 1 < len(steps) else rw
        if start_x >= rw:
            continue
        s0, s1 = s_min + start_x * Wl / rw, s_min + end_x * Wl / rw
        xs = [s * ax + t * nx for s in (s0, s1) for t in (t_min, t_max)]
        ys = [s * ay + t * ny for s in (s0, s1) for t in (t_min, t_max)]
        out.append((i, (to_i32(math.floor(min(ys))), to_i32(math.floor(min(xs))), to_i32(math.ceil(max(ys))),
                        to_i32(math.ceil(max(xs))))))
    return out
