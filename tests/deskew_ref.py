"""Page deskew, restated in numpy: the specification the library equals bit for bit.

  scores    skew_scores(page float32 [H, W], table int32 [A, 2]) -> A Python ints.  Per angle (S, C), Q16 sine and cosine:
            q = §7.4's bin of a pixel (normalize_ref.bins of clamp(v + 0.5f)); d(x, y) = |q(x, y) - q(x, y + 1)|, 0 on the
            last row and beside a NaN; bin = (x S + y C - t0) >> 16 with t0 the minimum of x S + y C over the four corner
            pixels; P[b] = the sum of d over the pixels of bin b; score = the sum of P[b]^2.  All integers.
  table     skew_table(first, n, step_deg): S, C = rint(sin / cos((first + i) * step_deg degrees) * 65536).
  estimate  estimate(work page, params): the coarse angles k r * fine (k = -K .. K, r = coarse / fine, K = floor(max_deg /
            coarse)), then the 2 r + 1 angles a fine step apart around the best coarse one; arg max with ties to the smaller
            |angle|, then to the negative one.  work_page(): the copy the scores are taken on (resample_ref's area filter).
  warp      warp(page, m, out_hw, fill): float32, every operation rounded on its own: fx = ox + 0.5f, X = (m0 + m1 fx) +
            m2 fy, Y likewise; ix = floor(X), wx = X - ix; taps (ix, iy) .. (ix + 1, iy + 1), `fill` outside the page;
            top = (1 - wx) t00 + wx t01, bot likewise, v = (1 - wy) top + wy bot.
  map       deskew_map(h, w, angle_deg, expand): in double, each coefficient rounded once to float32.
  unwarp    unwarp_rects / unwarp_boxes: in double from the float32 coefficients; see the functions.
"""
import math

import numpy as np

import normalize_ref as N
import resample_ref as R

F = np.float32
Q16 = 65536
MAX_SIDE = 4096


def default_params():
    return {"work_max_side": 1024, "max_deg": 15.0, "coarse_step_deg": 0.5, "fine_step_deg": 0.1}


def plan(params):
    """(r, K) of valid parameters, None of invalid ones."""
    p = params
    if not (1 <= p["work_max_side"] <= MAX_SIDE):
        return None
    fine, coarse, mx = float(p["fine_step_deg"]), float(p["coarse_step_deg"]), float(p["max_deg"])
    if not (fine > 0.0 and math.isfinite(fine)) or not (0.0 < mx <= 45.0):
        return None
    ratio = coarse / fine
    r = math.floor(ratio + 0.5) if math.isfinite(ratio) else 0
    if r < 1 or r > 1e6 or abs(ratio - r) > 1e-6 * r:
        return None
    K = math.floor(mx / coarse + 1e-9)
    if K < 1 or 2 * K + 1 > 65535 or 2 * r + 1 > 65535:
        return None
    return int(r), int(K)


def skew_table(first, n, step_deg):
    deg = (first + np.arange(n, dtype=np.int64)).astype(np.float64) * np.float64(step_deg)
    th = deg * (np.pi / 180.0)
    return np.stack([np.rint(np.sin(th) * 65536.0), np.rint(np.cos(th) * 65536.0)], axis=1).astype(np.int32)


def weights(page):
    """d [H, W] int64."""
    q = N.bins(N.grey(np.ascontiguousarray(page, F), False))
    d = np.zeros(q.shape, np.int64)
    both = (q[:-1] >= 0) & (q[1:] >= 0)
    d[:-1] = np.where(both, np.abs(q[:-1] - q[1:]), 0)
    return d


def skew_scores(page, table):
    page = np.ascontiguousarray(page, F)
    h, w = page.shape
    assert h <= MAX_SIDE and w <= MAX_SIDE
    d = weights(page)
    ys, xs = np.nonzero(d)
    dv = d[ys, xs].astype(np.float64)   # sums stay far below 2^53: exact
    out = []
    for S, C in np.asarray(table, np.int64).reshape(-1, 2).tolist():
        assert abs(S) <= Q16 and abs(C) <= Q16
        t0 = min(0, (w - 1) * S) + min(0, (h - 1) * C)
        b = (xs * S + ys * C - t0) >> 16
        P = np.bincount(b, weights=dv).astype(np.uint64) if len(b) else np.zeros(1, np.uint64)
        out.append(sum(int(v) * int(v) for v in P[P > 0].tolist()))
    return out


def best_angle(scores, first, stride):
    best = 0
    for i in range(1, len(scores)):
        a, b = first + i * stride, first + best * stride
        if scores[i] > scores[best] or (scores[i] == scores[best] and (abs(a) < abs(b) or (abs(a) == abs(b) and a < b))):
            best = i
    return best


def work_page(page, work_max_side=1024):
    page = np.ascontiguousarray(page, F)
    if max(page.shape) <= work_max_side:
        return page
    return R.area(page, *R.work_size(page.shape, float(work_max_side) / float(max(page.shape))))


def estimate(work, params=None, scores=skew_scores):
    """What estimate_skew finds on a work page -> dict.  scores(page, table): the primitive (the library's, in a GPU test)."""
    p = dict(default_params(), **(params or {}))
    r, K = plan(p)
    fine = float(p["fine_step_deg"])
    table = np.concatenate([skew_table(k * r, 1, fine) for k in range(-K, K + 1)])
    coarse = [int(v) for v in scores(work, table)]
    cb = best_angle(coarse, -K * r, r)
    ck = (cb - K) * r
    fs = [int(v) for v in scores(work, skew_table(ck - r, 2 * r + 1, fine))]
    fk = ck - r + best_angle(fs, ck - r, 1)
    return {"angle": fk * fine, "coarse_index": ck, "fine_index": fk, "work_hw": tuple(work.shape),
            "scores": (coarse[cb], max([v for i, v in enumerate(coarse) if i != cb] or [0]), fs[fk - (ck - r)]), "coarse": coarse}


# ---------------------------------------------------------------------------------------------------------------- warp
def warp(page, m, out_hw, fill=0.5):
    page = np.ascontiguousarray(page, F)
    ph, pw = page.shape
    m = np.asarray(m, F).reshape(6)
    fill = F(fill)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    with np.errstate(all="ignore"):
        fx = (np.arange(ow, dtype=F) + F(0.5))[None, :]
        fy = (np.arange(oh, dtype=F) + F(0.5))[:, None]
        X = ((m[0] + m[1] * fx).astype(F) + (m[2] * fy).astype(F)).astype(F)
        Y = ((m[3] + m[4] * fx).astype(F) + (m[5] * fy).astype(F)).astype(F)
        fix, fiy = np.floor(X), np.floor(Y)
        wx, wy = (X - fix).astype(F), (Y - fiy).astype(F)
        onpage = (fix >= F(-1)) & (fix <= F(pw)) & (fiy >= F(-1)) & (fiy <= F(ph))
        ix = np.where(onpage, fix, F(-2)).astype(np.int64)
        iy = np.where(onpage, fiy, F(-2)).astype(np.int64)

        def tap(dy, dx):
            y, x = iy + dy, ix + dx
            inside = (y >= 0) & (y < ph) & (x >= 0) & (x < pw)
            return np.where(inside, page[np.clip(y, 0, ph - 1), np.clip(x, 0, pw - 1)], fill).astype(F)

        one = F(1.0)
        top = (((one - wx) * tap(0, 0)).astype(F) + (wx * tap(0, 1)).astype(F)).astype(F)
        bot = (((one - wx) * tap(1, 0)).astype(F) + (wx * tap(1, 1)).astype(F)).astype(F)
        return (((one - wy) * top).astype(F) + (wy * bot).astype(F)).astype(F)


def deskew_map(h, w, angle_deg, expand=True):
    """((H', W'), m float32 [6]): the output is the page turned clockwise by the angle about its centre."""
    assert abs(angle_deg) <= 45.0
    th = np.float64(angle_deg) * (np.pi / 180.0)
    c, s = np.cos(th), np.sin(th)
    ow, oh = np.float64(w), np.float64(h)
    if expand:
        ow = np.ceil(w * abs(c) + h * abs(s))
        oh = np.ceil(w * abs(s) + h * abs(c))
    m = [((w / 2.0 - 0.5) - c * ow / 2.0) - s * oh / 2.0, c, s, ((h / 2.0 - 0.5) + s * ow / 2.0) - c * oh / 2.0, -s, c]
    return (int(oh), int(ow)), np.array(m, np.float64).astype(F)


def unwarp_rects(rects, m):
    """[n, 6] float32 (cx, cy, up.x, up.y, w, h) found on a page warped with m -> in the frame of the warp's source.  A
    rect with a value that is not finite stays as it is."""
    a = np.array(rects, F).reshape(-1, 6)
    m0, m1, m2, m3, m4, m5 = [np.float64(v) for v in np.asarray(m, F).reshape(6)]
    lw, lh = np.sqrt(m1 * m1 + m4 * m4), np.sqrt(m2 * m2 + m5 * m5)
    out = a.copy()
    with np.errstate(all="ignore"):
        for i in range(len(a)):
            if not np.all(np.isfinite(a[i])):
                continue
            cx, cy, ux, uy, w, h = [np.float64(v) for v in a[i]]
            fx, fy = cx + 0.5, cy + 0.5
            out[i, 0] = F((m0 + m1 * fx) + m2 * fy)
            out[i, 1] = F((m3 + m4 * fx) + m5 * fy)
            vx, vy = m1 * ux + m2 * uy, m4 * ux + m5 * uy
            lv = np.sqrt(vx * vx + vy * vy)
            if lv > 0.0 and np.isfinite(lv):
                out[i, 2], out[i, 3] = F(vx / lv), F(vy / lv)
            out[i, 4], out[i, 5] = F(w * lw), F(h * lh)
    return out


def _i32(v):
    return int(min(max(v, -2147483648.0), 2147483647.0))


def unwarp_boxes(boxes, m):
    """[n, 4] int32 (top, left, bottom, right): the four corners through the map; floor of the minimum, ceil of the maximum."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    m0, m1, m2, m3, m4, m5 = [float(np.float64(v)) for v in np.asarray(m, F).reshape(6)]
    out = np.zeros((len(b), 4), np.int32)
    for i, (t, l, bo, r) in enumerate(b.tolist()):
        X = [(m0 + m1 * (x + 0.5)) + m2 * (y + 0.5) for y in (t, bo) for x in (l, r)]
        Y = [(m3 + m4 * (x + 0.5)) + m5 * (y + 0.5) for y in (t, bo) for x in (l, r)]
        out[i] = (_i32(math.floor(min(Y))), _i32(math.floor(min(X))), _i32(math.ceil(max(Y))), _i32(math.ceil(max(X))))
    return out
