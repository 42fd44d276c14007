"""Perspective correction, restated in numpy: the specification the library equals bit for bit.

  peaks     edge_peaks(page float32 [H, W], table int32 [A, 2], min_step) -> uint64 [2 families, 2 signs, A, 16].  q = §7.4's
            bin of a pixel.  Family 0 (H): g(x, y) = q(x, y + 1) - q(x, y), 0 on the last row and beside a NaN; bin = (x S +
            y C - t0) >> 16.  Family 1 (V) is family 0 of the transposed page.  Sign 0: g >= min_step, sign 1: g <= -min_step;
            such a pixel adds 1 to P[family][sign][a][bin].  A row of H + W bins is cut into 16 bands [k nb / 16, (k + 1) nb /
            16); per band the largest count and the smallest bin that has it, (count << 32) | (0xFFFFFFFF - bin), 0 for none.
  choose    choose(peaks, table, work_hw, page_hw, params) -> dict: see the function; double, no trigonometry.
  outline   find_outline(page, params): the work copy (deskew_ref.work_page), the table of the angles -K .. K steps, the
            peaks, the choice.
  map       quad_map(corners8) -> ((H', W'), m float32 [8]): Heckbert's square-to-quad coefficients in double, each rounded
            once to float32.  None for a quad without area or a value that is not finite.
  project   project(page, m, out_hw, fill): float32, every operation rounded on its own: nx = (m0 + m1 fx) + m2 fy, ny
            likewise, dn = (1 + m6 fx) + m7 fy; where dn is finite and > 0, X = nx / dn, Y = ny / dn and deskew_ref.warp's taps;
            elsewhere `fill`.
  unproject unproject_rects / unproject_boxes: in double from the float32 coefficients; see the functions.
  plant     plant(...) / plant_map(...): a synthetic photo, a sheet seen through a quad on a desk; corner_bound(...): how far
            a planted corner may come back (fixtures of the tests, not part of the specification).
"""
import math

import numpy as np

import deskew_ref as D
import normalize_ref as N

F = np.float32
Q16 = 65536
MAX_SIDE = 4096
BANDS = 16
FULL = 0xFFFFFFFF


def default_params():
    return {"work_max_side": 512, "max_deg": 15.0, "step_deg": 0.5, "min_step": 8, "min_cover": 0.25, "min_span": 0.25, "min_area": 0.1}


def plan(params):
    """K of valid parameters, None of invalid ones."""
    p = params
    if not (1 <= p["work_max_side"] <= MAX_SIDE) or not (1 <= p["min_step"] <= 256):
        return None
    step, mx = float(p["step_deg"]), float(p["max_deg"])
    if not (step > 0.0 and math.isfinite(step)) or not (0.0 < mx <= 45.0):
        return None
    if not (0.0 < p["min_cover"] <= 1.0) or not (0.0 < p["min_span"] <= 1.0) or not (0.0 <= p["min_area"] <= 1.0):
        return None
    K = math.floor(mx / step + 1e-9)
    if K < 1 or 2 * K + 1 > 4095:
        return None
    return int(K)


def table_of(params):
    K = plan(params)
    return D.skew_table(-K, 2 * K + 1, float(params["step_deg"]))


# --------------------------------------------------------------------------------------------------------------- peaks
def steps(page):
    """g [H, W] int64 of family 0."""
    q = N.bins(N.grey(np.ascontiguousarray(page, F), False))
    g = np.zeros(q.shape, np.int64)
    both = (q[:-1] >= 0) & (q[1:] >= 0)
    g[:-1] = np.where(both, q[1:].astype(np.int64) - q[:-1].astype(np.int64), 0)
    return g


def family_profiles(page, table, min_step):
    """P [2 signs, A, H + W] int64 of family 0 of `page`."""
    h, w = page.shape
    g = steps(page)
    out = np.zeros((2, len(table), h + w), np.int64)
    for sign, mask in enumerate((g >= min_step, g <= -min_step)):
        ys, xs = np.nonzero(mask)
        for a, (S, C) in enumerate(np.asarray(table, np.int64).reshape(-1, 2).tolist()):
            assert abs(S) <= Q16 and abs(C) <= Q16
            t0 = min(0, (w - 1) * S) + min(0, (h - 1) * C)
            b = (xs * S + ys * C - t0) >> 16
            if len(b):
                out[sign, a] = np.bincount(b, minlength=h + w)
    return out


def band_peaks(P):
    """[..., nb] counts -> uint64 [..., 16]."""
    nb = P.shape[-1]
    out = np.zeros(P.shape[:-1] + (BANDS,), np.uint64)
    for k in range(BANDS):
        lo, hi = k * nb // BANDS, (k + 1) * nb // BANDS
        if hi <= lo:
            continue
        band = P[..., lo:hi]
        at = np.argmax(band, axis=-1)   # the first of the largest: the smallest bin
        cnt = np.take_along_axis(band, at[..., None], axis=-1)[..., 0]
        packed = (cnt.astype(np.uint64) << np.uint64(32)) | (np.uint64(FULL) - (at + lo).astype(np.uint64))
        out[..., k] = np.where(cnt > 0, packed, np.uint64(0))
    return out


def edge_peaks(page, table, min_step):
    page = np.ascontiguousarray(page, F)
    h, w = page.shape
    assert h <= MAX_SIDE and w <= MAX_SIDE and 1 <= min_step <= 256
    table = np.asarray(table, np.int32).reshape(-1, 2)
    return np.stack([band_peaks(family_profiles(page, table, min_step)), band_peaks(family_profiles(np.ascontiguousarray(page.T), table, min_step))])


# -------------------------------------------------------------------------------------------------------------- choose
def _candidates(peaks, table, family, sign, wh, ww, min_cover):
    """Lists in ascending (angle index, bin): (a, b, d, pos, count, angle)."""
    L = float(ww if family == 0 else wh)
    need = math.ceil(min_cover * L)
    fw, fh = (ww, wh) if family == 0 else (wh, ww)
    out = []
    for a, (S, C) in enumerate(np.asarray(table, np.int64).reshape(-1, 2).tolist()):
        t0 = min(0, (fw - 1) * S) + min(0, (fh - 1) * C)
        s, c = S / 65536.0, C / 65536.0
        for k in range(BANDS):
            e = int(peaks[family, sign, a, k])
            if e == 0:
                continue
            count, b = e >> 32, FULL - (e & FULL)
            if not float(count) >= need:
                continue
            rho = float(b * 65536 + 32768 + t0) / 65536.0
            d = rho + 0.5 * c
            mid = (float(fw) - 1.0) / 2.0
            with np.errstate(all="ignore"):
                pos = float((np.float64(d) - np.float64(s) * np.float64(mid)) / np.float64(c))
            if math.isfinite(pos):
                out.append(((s, c, d) if family == 0 else (c, s, d)) + (pos, count, a))
    return out


def _best_pair(first, second, span):
    if not first or not second:
        return None
    p1 = np.array([f[3] for f in first], np.float64)[:, None]
    p2 = np.array([s[3] for s in second], np.float64)[None, :]
    c1 = np.array([f[4] for f in first], np.int64)[:, None]
    c2 = np.array([s[4] for s in second], np.int64)[None, :]
    ok = (p2 - p1) >= span
    if not ok.any():
        return None
    i, j = np.unravel_index(np.argmax(np.where(ok, c1 + c2, -1)), ok.shape)   # the first of the largest, row-major
    return int(i), int(j)


def _intersect(p, q):
    with np.errstate(all="ignore"):
        a1, b1, d1, a2, b2, d2 = [np.float64(v) for v in p[:3] + q[:3]]
        det = a1 * b2 - a2 * b1
        return (d1 * b2 - d2 * b1) / det, (a1 * d2 - a2 * d1) / det


NONE = {"found": 0, "corners": np.zeros(8, F), "polarity": 0, "counts": (0, 0, 0, 0), "angles": (0, 0, 0, 0)}


def choose(peaks, table, work_hw, page_hw, params=None):
    p = dict(default_params(), **(params or {}))
    wh, ww = int(work_hw[0]), int(work_hw[1])
    ph, pw = int(page_hw[0]), int(page_hw[1])
    peaks = np.asarray(peaks, np.uint64).reshape(2, 2, -1, BANDS)
    none = dict(NONE, work_hw=(wh, ww))
    cand = [[_candidates(peaks, table, f, s, wh, ww, float(p["min_cover"])) for s in range(2)] for f in range(2)]
    span = (float(p["min_span"]) * (float(wh) - 1.0), float(p["min_span"]) * (float(ww) - 1.0))
    best = None
    for sigma in range(2):
        pairs = [_best_pair(cand[f][sigma], cand[f][1 - sigma], span[f]) for f in range(2)]
        if pairs[0] is None or pairs[1] is None:
            continue
        total = sum(cand[f][sigma][pairs[f][0]][4] + cand[f][1 - sigma][pairs[f][1]][4] for f in range(2))
        if best is None or total > best[0]:
            best = (total, sigma, pairs)
    if best is None:
        return none
    _, sg, pairs = best
    top, bottom = cand[0][sg][pairs[0][0]], cand[0][1 - sg][pairs[0][1]]
    left, right = cand[1][sg][pairs[1][0]], cand[1][1 - sg][pairs[1][1]]
    kx, ky = np.float64(pw) / np.float64(ww), np.float64(ph) / np.float64(wh)
    corners = np.zeros(8, F)
    with np.errstate(all="ignore"):
        for q, (hl, vl) in enumerate(((top, left), (top, right), (bottom, right), (bottom, left))):
            x, y = _intersect(hl, vl)
            corners[2 * q] = F((x + 0.5) * kx - 0.5)
            corners[2 * q + 1] = F((y + 0.5) * ky - 0.5)
    if not np.all(np.isfinite(corners)):
        return none
    c = corners.astype(np.float64)
    area2 = np.float64(0.0)
    for q in range(4):
        r, t = (q + 1) & 3, (q + 2) & 3
        e1x, e1y = c[2 * r] - c[2 * q], c[2 * r + 1] - c[2 * q + 1]
        e2x, e2y = c[2 * t] - c[2 * r], c[2 * t + 1] - c[2 * r + 1]
        if not (e1x * e2y - e1y * e2x > 0.0):
            return none
        area2 = area2 + (c[2 * q] * c[2 * r + 1] - c[2 * r] * c[2 * q + 1])
    if not (0.5 * area2 >= np.float64(p["min_area"]) * np.float64(ph) * np.float64(pw)):
        return none
    four = (top, bottom, left, right)
    return {"found": 1, "corners": corners, "polarity": sg, "counts": tuple(int(l[4]) for l in four), "angles": tuple(int(l[5]) for l in four),
            "work_hw": (wh, ww)}


def find_outline(page, params=None, peaks=edge_peaks):
    """What find_outline finds on a page -> dict.  peaks(page, table, min_step): the primitive (the library's, in a GPU test)."""
    p = dict(default_params(), **(params or {}))
    page = np.ascontiguousarray(page, F)
    work = D.work_page(page, p["work_max_side"])
    table = table_of(p)
    return choose(peaks(work, table, int(p["min_step"])), table, work.shape, page.shape, p)


# ----------------------------------------------------------------------------------------------------------------- map
def page_corners(h, w):
    """The page's own outline in its pixel-index frame: quad_map of it is the identity."""
    return np.array([-0.5, -0.5, w - 0.5, -0.5, w - 0.5, h - 0.5, -0.5, h - 0.5], F)


def _side(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return np.sqrt(dx * dx + dy * dy)


def _out_side(l1, l2):
    v = np.floor(max(l1, l2) + 0.5)
    if not v >= 1.0:
        return 1
    return 65535 if v > 65535.0 else int(v)


def quad_map(corners8):
    c = np.asarray(corners8, F).reshape(8)
    if not np.all(np.isfinite(c)):
        return None
    x0, y0, x1, y1, x2, y2, x3, y3 = [np.float64(v) for v in c]
    with np.errstate(all="ignore"):
        ow = _out_side(_side(x0, y0, x1, y1), _side(x3, y3, x2, y2))
        oh = _out_side(_side(x0, y0, x3, y3), _side(x1, y1, x2, y2))
        dx1, dx2, sx = x1 - x2, x3 - x2, ((x0 - x1) + x2) - x3
        dy1, dy2, sy = y1 - y2, y3 - y2, ((y0 - y1) + y2) - y3
        det = dx1 * dy2 - dy1 * dx2
        if det == 0.0 or not np.isfinite(det):
            return None
        g = (sx * dy2 - sy * dx2) / det
        h = (dx1 * sy - dy1 * sx) / det
        a, b = (x1 - x0) + g * x1, (x3 - x0) + h * x3
        d, e = (y1 - y0) + g * y1, (y3 - y0) + h * y3
        W, H = np.float64(ow), np.float64(oh)
        m = np.array([x0, a / W, b / H, y0, d / W, e / H, g / W, h / H], np.float64).astype(F)
    if not np.all(np.isfinite(m)):
        return None
    return (oh, ow), m


# ------------------------------------------------------------------------------------------------------------- project
def project(page, m, out_hw, fill=0.5):
    page = np.ascontiguousarray(page, F)
    ph, pw = page.shape
    m = np.asarray(m, F).reshape(8)
    fill = F(fill)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    with np.errstate(all="ignore"):
        fx = (np.arange(ow, dtype=F) + F(0.5))[None, :]
        fy = (np.arange(oh, dtype=F) + F(0.5))[:, None]
        nx = ((m[0] + m[1] * fx).astype(F) + (m[2] * fy).astype(F)).astype(F)
        ny = ((m[3] + m[4] * fx).astype(F) + (m[5] * fy).astype(F)).astype(F)
        dn = ((F(1.0) + m[6] * fx).astype(F) + (m[7] * fy).astype(F)).astype(F)
        seen = np.isfinite(dn) & (dn > F(0.0))
        safe = np.where(seen, dn, F(1.0))
        X, Y = (nx / safe).astype(F), (ny / safe).astype(F)
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
        v = (((one - wy) * top).astype(F) + (wy * bot).astype(F)).astype(F)
        return np.where(seen, v, fill).astype(F)


# ----------------------------------------------------------------------------------------------------------- unproject
def _map_point(m, fx, fy):
    with np.errstate(all="ignore"):
        nx = (m[0] + m[1] * fx) + m[2] * fy
        ny = (m[3] + m[4] * fx) + m[5] * fy
        dn = (np.float64(1.0) + m[6] * fx) + m[7] * fy
        if not (dn > 0.0) or not np.isfinite(dn):
            return None
        return nx / dn, ny / dn, dn


def unproject_rects(rects, m):
    """[n, 6] float32 (cx, cy, up.x, up.y, w, h) found on a page projected with m -> in the frame of its source.  A rect
    with a value that is not finite, or whose centre the map does not reach (dn <= 0), stays as it is."""
    a = np.array(rects, F).reshape(-1, 6)
    m = [np.float64(v) for v in np.asarray(m, F).reshape(8)]
    out = a.copy()
    with np.errstate(all="ignore"):
        for i in range(len(a)):
            if not np.all(np.isfinite(a[i])):
                continue
            cx, cy, ux, uy, w, h = [np.float64(v) for v in a[i]]
            at = _map_point(m, cx + 0.5, cy + 0.5)
            if at is None:
                continue
            X, Y, dn = at
            j00, j01 = (m[1] - m[6] * X) / dn, (m[2] - m[7] * X) / dn
            j10, j11 = (m[4] - m[6] * Y) / dn, (m[5] - m[7] * Y) / dn
            vx, vy = j00 * ux + j01 * uy, j10 * ux + j11 * uy
            lv = np.sqrt(vx * vx + vy * vy)
            px, py = j00 * (-uy) + j01 * ux, j10 * (-uy) + j11 * ux
            lp = np.sqrt(px * px + py * py)
            out[i, 0], out[i, 1] = F(X), F(Y)
            if lv > 0.0 and np.isfinite(lv):
                out[i, 2], out[i, 3] = F(vx / lv), F(vy / lv)
            out[i, 4], out[i, 5] = F(w * lp), F(h * lv)
    return out


def _i32(v):
    return int(min(max(v, -2147483648.0), 2147483647.0))


def unproject_boxes(boxes, m):
    """[n, 4] int32 (top, left, bottom, right): the four corners through the map; floor of the minimum, ceil of the maximum.
    A box with a corner the map does not reach stays as it is."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    m = [np.float64(v) for v in np.asarray(m, F).reshape(8)]
    out = np.zeros((len(b), 4), np.int32)
    for i, (t, l, bo, r) in enumerate(b.tolist()):
        pts = [_map_point(m, np.float64(x) + 0.5, np.float64(y) + 0.5) for y in (t, bo) for x in (l, r)]
        if any(p is None for p in pts):
            out[i] = (t, l, bo, r)
            continue
        X, Y = [float(p[0]) for p in pts], [float(p[1]) for p in pts]
        out[i] = (_i32(math.floor(min(Y))), _i32(math.floor(min(X))), _i32(math.ceil(max(Y))), _i32(math.ceil(max(X))))
    return out


# --------------------------------------------------------------------------------------------------------------- plant
def sheet(h, w, paper=0.45, ink=-0.4, seed=0):
    """A sheet of `paper` with rows of word-like bars of `ink`, float32 [h, w]."""
    rng = np.random.default_rng(seed)
    a = np.full((h, w), paper, F)
    y = h // 12
    while y + 6 < h - h // 12:
        x = w // 10
        while x < w - w // 10 - 12:
            n = int(rng.integers(12, 48))
            a[y:y + 5, x:min(x + n, w - w // 10)] = ink
            x += n + int(rng.integers(6, 14))
        y += 13
    return a


def plant(photo_hw, quad, sheet_px, desk=-0.35, noise=0.02, seed=0):
    """The sheet seen through `quad` (TL, TR, BR, BL as (x, y), the photo's pixel-index frame) on a desk of level `desk`
    with uniform noise of +-`noise`, float32 [photo_hw].  float64 arithmetic; bilinear taps, the desk beyond the sheet."""
    h, w = photo_hw
    sh, sw = sheet_px.shape
    q = np.asarray(quad, np.float64).reshape(4, 2)
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = q
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    det = dx1 * dy2 - dy1 * dx2
    g, hh = (sx * dy2 - sy * dx2) / det, (dx1 * sy - dy1 * sx) / det
    Hm = np.array([[x1 - x0 + g * x1, x3 - x0 + hh * x3, x0], [y1 - y0 + g * y1, y3 - y0 + hh * y3, y0], [g, hh, 1.0]])   # unit square -> photo
    inv = np.linalg.inv(Hm)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    den = inv[2, 0] * xs + inv[2, 1] * ys + inv[2, 2]
    u = (inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2]) / den
    v = (inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2]) / den
    rng = np.random.default_rng(seed)
    bg = desk + (rng.random((h, w)) - 0.5) * 2.0 * noise
    X, Y = u * sw - 0.5, v * sh - 0.5   # the sheet's pixel-index frame: its outline is the quad
    ix, iy = np.floor(X), np.floor(Y)
    wx, wy = X - ix, Y - iy
    pad = np.full((sh + 2, sw + 2), np.nan)
    pad[1:-1, 1:-1] = sheet_px
    inside = (den > 0) & (ix >= -1) & (ix < sw) & (iy >= -1) & (iy < sh)
    jx, jy = np.clip(ix, -1, sw - 1).astype(np.int64) + 1, np.clip(iy, -1, sh - 1).astype(np.int64) + 1

    def tap(dy, dx):
        t = pad[jy + dy, jx + dx]
        return np.where(np.isnan(t), bg, t)

    val = (1 - wy) * ((1 - wx) * tap(0, 0) + wx * tap(0, 1)) + wy * ((1 - wx) * tap(1, 0) + wx * tap(1, 1))
    return np.where(inside, val, bg).astype(F)


def plant_map(quad, sheet_hw):
    """m float32 [8] for project(sheet, m, photo_hw, desk): the photo that shows the sheet_hw sheet through `quad` (TL, TR,
    BR, BL as (x, y), the photo's pixel-index frame).  The inverse of the quad's map, in float64."""
    sh, sw = sheet_hw
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = np.asarray(quad, np.float64).reshape(4, 2)
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    det = dx1 * dy2 - dy1 * dx2
    g, hh = (sx * dy2 - sy * dx2) / det, (dx1 * sy - dy1 * sx) / det
    Hq = np.array([[x1 - x0 + g * x1, x3 - x0 + hh * x3, x0], [y1 - y0 + g * y1, y3 - y0 + hh * y3, y0], [g, hh, 1.0]])
    Fi = np.linalg.inv(Hq @ np.diag([1.0 / sw, 1.0 / sh, 1.0]))   # the photo's index frame -> the sheet's (fx, fy)
    half = np.array([[1.0, 0.0, -0.5], [0.0, 1.0, -0.5], [0.0, 0.0, 1.0]])
    Gm = half @ Fi @ half
    Gm = Gm / Gm[2, 2]
    return np.array([Gm[0, 2], Gm[0, 0], Gm[0, 1], Gm[1, 2], Gm[1, 0], Gm[1, 1], Gm[2, 0], Gm[2, 1]], np.float64).astype(F)


def corner_bound(quad, photo_hw, work_max_side=512, step_deg=0.5):
    """How far a corner may come back from where it was planted, in pixels of the photo.  A side's line is off its edge by at
    most: 1 pixel, the width of a bin (the edge's pixels project anywhere within the bin whose middle the line takes); plus
    0.5, half the ramp plant()'s bilinear taps spread the edge over; plus (L / 2) tan(step / 2): the nearest angle of the
    table is within half a step of the edge's, and the line of most edge pixels at that angle crosses the edge at its
    middle, so it leaves it by that much at the ends of a side of length L (the longest of the quad, to be safe).  Two such
    lines that meet at an angle phi put their intersection within (e1 + e2) / sin(phi) of the corner: phi is the smallest
    corner angle of the quad.  All of it at the work scale, times photo / work to come back to the photo."""
    q = np.asarray(quad, np.float64).reshape(4, 2)
    sides = [q[(i + 1) % 4] - q[i] for i in range(4)]
    L = max(np.hypot(*s) for s in sides)
    scale = max(1.0, max(photo_hw) / float(work_max_side))
    e = 1.0 + 0.5 + (L / scale / 2.0) * np.tan(np.deg2rad(step_deg / 2.0))
    sin_phi = min(abs(sides[i][0] * sides[(i + 1) % 4][1] - sides[i][1] * sides[(i + 1) % 4][0]) / (np.hypot(*sides[i]) * np.hypot(*sides[(i + 1) % 4]))
                  for i in range(4))
    return 2.0 * e / sin_phi * scale
