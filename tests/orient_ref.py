"""Quarter turns and auto-orientation restated in numpy: the specification the library is held to.

  rot90(page, k)            the turned page: np.rot90, counter-clockwise, any integer k
  unrotate_rects / _boxes   results found on rot90(page, k) mapped back to the page's own frame
  vote(rects)               the word-shape vote: which way the words read
  sample_lines(lines, m)    which lines of a candidate turn are recognised
  score(char_logps)         a candidate's score from its lines' char log-probs
  choose(candidates, s)     the turn that wins

Coordinates are points of the pixel-index frame: pixel (row y, column x) of an H x W page is pixel
(W-1-x, y) of rot90(page, 1), (H-1-y, W-1-x) of rot90(page, 2) and (x, H-1-y) of rot90(page, 3)  [(row, column)].
"""
import numpy as np

F = np.float32


def turns(k):
    return ((int(k) % 4) + 4) % 4


def rot90(page, k):
    return np.ascontiguousarray(np.rot90(page, turns(k)))


def turned_hw(page_hw, k):
    h, w = page_hw
    return (w, h) if turns(k) & 1 else (h, w)


def unrotate_rects(rects, page_hw, k):
    """[n, 6] float32 (cx, cy, up.x, up.y, w, h) in the frame of rot90(page, k) -> in the frame of the page_hw page.
    float32 arithmetic: one subtraction from float32(W - 1) or float32(H - 1), or a sign flip."""
    a = np.array(rects, F).reshape(-1, 6).copy()
    k = turns(k)
    xm, ym = F(page_hw[1] - 1), F(page_hw[0] - 1)
    x, y, ux, uy = a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy()
    with np.errstate(all="ignore"):
        if k == 1:
            a[:, 0], a[:, 1], a[:, 2], a[:, 3] = xm - y, x, -uy, ux
        elif k == 2:
            a[:, 0], a[:, 1], a[:, 2], a[:, 3] = xm - x, ym - y, -ux, -uy
        elif k == 3:
            a[:, 0], a[:, 1], a[:, 2], a[:, 3] = y, ym - x, uy, -ux
    return a


def unrotate_boxes(boxes, page_hw, k):
    """[n, 4] int32 (top, left, bottom, right) in the frame of rot90(page, k) -> in the frame of the page_hw page; the
    bounds swap so that left <= right and top <= bottom stay true."""
    b = np.array(boxes, np.int64).reshape(-1, 4)
    k = turns(k)
    xm, ym = page_hw[1] - 1, page_hw[0] - 1
    t, l, bo, r = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    if k == 1:
        out = np.stack([l, xm - bo, r, xm - t], axis=1)
    elif k == 2:
        out = np.stack([ym - bo, xm - r, ym - t, xm - l], axis=1)
    elif k == 3:
        out = np.stack([ym - r, t, ym - l, bo], axis=1)
    else:
        out = b
    return out.astype(np.int32).reshape(-1, 4)


def corners(r):
    """RotatedRect::corners in float32, every operation rounded on its own: 4 x (x, y)."""
    cx, cy, ux, uy, w, h = (F(v) for v in r)
    with np.errstate(all="ignore"):
        hw, hh = w / F(2), h / F(2)
        parx, pary = uy * hw, (-ux) * hw
        perx, pery = ux * hh, uy * hh
        return [(cx - perx - parx, cy - pery - pary), (cx - perx + parx, cy - pery + pary),
                (cx + perx + parx, cy + pery + pary), (cx + perx - parx, cy + pery - pary)]


def vote(rects):
    """float64 [2]: the summed widths of the words whose corners span more in x than in y, the summed heights of the
    others, word by word in order.  A word with a value, a corner or an extent that is not finite is skipped.  The page
    reads horizontally iff vote[0] >= vote[1]."""
    out = np.zeros(2, np.float64)
    for r in np.asarray(rects, F).reshape(-1, 6):
        if not np.all(np.isfinite(r)):
            continue
        c = corners(r)
        xs, ys = [p[0] for p in c], [p[1] for p in c]
        if not (np.all(np.isfinite(xs)) and np.all(np.isfinite(ys))):
            continue
        with np.errstate(all="ignore"):
            bw, bh = F(max(xs)) - F(min(xs)), F(max(ys)) - F(min(ys))
        if not (np.isfinite(bw) and np.isfinite(bh)):
            continue
        if bw >= bh:
            out[0] += np.float64(bw)
        else:
            out[1] += np.float64(bh)
    return out


def candidates(v):
    return (0, 2) if v[0] >= v[1] else (1, 3)


def sample_lines(lines, max_lines):
    """Indices of the lines a candidate is scored on: up to max_lines (0 = all), those of the most words first, ties to
    the lower index; returned ascending (the order they are recognised and summed in)."""
    idx = list(range(len(lines)))
    if max_lines == 0 or max_lines >= len(lines):
        return idx
    idx.sort(key=lambda i: (-len(lines[i]), i))
    return sorted(idx[:max_lines])


def score(char_logps_per_line):
    """(score, n_chars): the float64 sum of the char log-probs (float32 values), line by line and char by char, over
    their number; -inf without chars."""
    total, n = np.float64(0.0), 0
    for lp in char_logps_per_line:
        for x in np.asarray(lp, F):
            total = total + np.float64(x)
            n += 1
    return (total / np.float64(n) if n else -np.inf), n


def choose(cands, scores):
    """The candidate of the larger score; a tie, and -inf twice, go to the smaller turn."""
    a, b = cands
    return b if scores[b] > scores[a] else a
