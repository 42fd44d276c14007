"""Working-resolution detection restated in numpy: the specification the library is held to.

  axis_taps(L, l)              the taps and integer weights of the area filter along one axis
  area(page, out_h, out_w)     the area filter, float32, every operation rounded on its own
  area_f64(page, out_h, out_w) the same weighted average in float64 (what the float32 result is within a bound of)
  work_size(page_hw, scale)    the work size of a scale
  rescale_rects(r, from, to)   word rects of one frame of a picture in another
  detect_at(...)               the composition: resample, detect, map back

The area filter along one axis L -> l (l <= L): g = gcd(L, l), P = L / g, q = l / g.  On a common grid of L * l / g units
output j covers [jP, (j+1)P) and source x covers [xq, (x+1)q).  The taps of j are x = (jP) // q .. ((j+1)P - 1) // q in
ascending order, each with the integer weight ov = min((j+1)P, (x+1)q) - max(jP, xq) >= 1; the weights of an output sum
to P.  acc = float(ov0) * in[x0]; acc = acc + float(ov) * in[x] per further tap; value = acc / float(P).  In two
dimensions the horizontal rule gives a value per source row, and the same rule runs vertically over those values.

Coordinates of rects are points of the pixel-index frame: pixel i covers [i - 0.5, i + 0.5).
"""
import math

import numpy as np

F = np.float32
MAX_SIDE = 65535
AUTO, BILINEAR, AREA = "auto", "bilinear", "area"


def axis_taps(L, l):
    """(P, first [l], weights [l, K]): the first tap of every output and the integer weights of its K = max tap count
    consecutive taps, 0 beyond an output's last tap (a tap of weight zero is never visited)."""
    assert 1 <= l <= L
    g = math.gcd(L, l)
    P, q = L // g, l // g
    j = np.arange(l, dtype=np.int64)
    lo, hi = j * P, (j + 1) * P
    first, last = lo // q, (hi - 1) // q
    K = int((last - first).max()) + 1
    x = first[:, None] + np.arange(K, dtype=np.int64)[None, :]
    ov = np.minimum(hi[:, None], (x + 1) * q) - np.maximum(lo[:, None], x * q)
    ov = np.where(x <= last[:, None], ov, 0)
    assert np.all(ov[x <= last[:, None]] >= 1) and np.all(ov.sum(axis=1) == P) and int(last.max()) == L - 1
    return P, first, ov


def _area_axis(a, l):
    """The rule along the LAST axis of float32 [..., L] -> [..., l]."""
    P, first, ov = axis_taps(a.shape[-1], l)
    with np.errstate(all="ignore"):
        acc = ov[:, 0].astype(F) * a[..., first]
        for t in range(1, ov.shape[1]):
            live = ov[:, t] > 0
            x = np.where(live, first + t, first)
            acc = np.where(live, acc + ov[:, t].astype(F) * a[..., x], acc)
        return (acc / F(P)).astype(F)


def area(page, out_h, out_w):
    a = np.ascontiguousarray(page, F)
    assert a.ndim == 2 and out_h <= a.shape[0] and out_w <= a.shape[1]
    rows = _area_axis(a, out_w)                                      # [H, out_w]: a value per source row
    return np.ascontiguousarray(_area_axis(np.ascontiguousarray(rows.T), out_h).T)


def area_f64(page, out_h, out_w):
    """The weighted average sum(ov_y * ov_x * in) / (P_y * P_x) in float64, and the largest tap counts (Kx, Ky)."""
    a = np.asarray(page, np.float64)

    def axis(b, l):
        P, first, ov = axis_taps(b.shape[-1], l)
        acc = np.zeros(b.shape[:-1] + (l,), np.float64)
        for t in range(ov.shape[1]):
            x = np.minimum(first + t, b.shape[-1] - 1)
            acc += ov[:, t].astype(np.float64) * b[..., x]
        return acc / P, ov.shape[1]

    rows, kx = axis(a, out_w)
    out, ky = axis(np.ascontiguousarray(rows.T), out_h)
    return np.ascontiguousarray(out.T), (kx, ky)


def resolve_filter(page_hw, out_hw, filt):
    shrinks = out_hw[0] <= page_hw[0] and out_hw[1] <= page_hw[1]
    if filt == AUTO:
        return AREA if shrinks else BILINEAR
    assert filt in (AREA, BILINEAR) and (filt == BILINEAR or shrinks)
    return filt


def resize(page, out_hw, filt=AUTO):
    """The resampled page; bilinear is the oracle's resize (the detection path's arithmetic, no padding)."""
    from oracle import clib
    a = np.ascontiguousarray(page, F)
    if resolve_filter(a.shape, out_hw, filt) == AREA:
        return area(a, *out_hw)
    return clib.resize_bilinear(a, int(out_hw[0]), int(out_hw[1]))


def work_size(page_hw, scale):
    """(h, w) = clamp(floor(side * scale + 0.5), 1, 65535), in double."""
    assert math.isfinite(scale) and scale > 0
    return tuple(int(min(max(math.floor(float(s) * float(scale) + 0.5), 1.0), float(MAX_SIDE))) for s in page_hw)


def max_side_scale(page_hw, n):
    return min(1.0, float(n) / float(max(page_hw)))


def rescale_rects(rects, from_hw, to_hw):
    """[n, 6] float32 (cx, cy, up.x, up.y, w, h) of the from_hw frame -> the to_hw frame.  Equal sizes: the bits as they
    are.  Else in double from the float32 values, each operation as written, rounded to float32 at the end."""
    a = np.array(rects, F).reshape(-1, 6).copy()
    if tuple(from_hw) == tuple(to_hw):
        return a
    d = a.astype(np.float64)
    sx, sy = np.float64(to_hw[1]) / np.float64(from_hw[1]), np.float64(to_hw[0]) / np.float64(from_hw[0])
    cx, cy, upx, upy, w, h = (d[:, i] for i in range(6))
    with np.errstate(all="ignore"):
        ncx, ncy = (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5
        vx, vy = upx * sx, upy * sy
        lv = np.sqrt(vx * vx + vy * vy)
        ax, ay = -upy * sx, upx * sy
        la = np.sqrt(ax * ax + ay * ay)
        ok = np.isfinite(lv) & (lv > 0)
        out = np.stack([ncx, ncy, np.where(ok, vx / lv, upx), np.where(ok, vy / lv, upy),
                        np.where(ok, w * la, w * sx), np.where(ok, h * lv, h * sy)], axis=1)
        res = out.astype(F)
    keep = ~ok                        # "up stays": its bits, not a round trip through double (a NaN keeps its payload)
    res[keep, 2:4] = a[keep, 2:4]
    return res


def detect_at(detect, page, work_hw, filt=AUTO):
    """The composition: `detect(work page) -> (rects [n, 6], ...)` on the page resampled to work_hw (None or the page's own
    size: the page itself, not resampled), the rects mapped back to the page's frame; whatever else detect returns (scores,
    pixel counts: those of the work page) is passed through."""
    a = np.ascontiguousarray(page, F)
    hw = tuple(a.shape) if work_hw is None or tuple(work_hw) == (0, 0) else tuple(work_hw)
    work = a if hw == tuple(a.shape) else resize(a, hw, filt)
    out = detect(work)
    rects = out[0] if isinstance(out, tuple) else out
    mapped = rescale_rects(rects, hw, a.shape)
    return (mapped,) + tuple(out[1:]) if isinstance(out, tuple) else mapped
