"""Ruled-line removal, restated in numpy: the specification the library equals bit for bit.

A prepared page v (float32 [H, W], dark ink on light paper) comes back with its long thin rules (table grids, form
lines, underlines) overwritten by the paper's level; every other pixel keeps its own 32-bit word.  All of it is integer
and set arithmetic.  remove_rules(page, min_length, max_thickness, margin, threshold, paper) -> (out, mask, info).

  open_h(X, n): the pixels of X that lie in a maximal horizontal run of X of length >= n; open_v the same along columns.
  The page edge ends a run.  Runs are enumerated one by one here (the library shifts and scans words of 64 pixels).

  1 ink   = v < threshold (NaN is not ink, -inf is).
  2 Ch    = open_h(ink, L), Cv = open_v(ink, L); text = ink \\ (Ch | Cv).
  3 Rh    = Ch \\ open_v(Ch, T + 1), Rv = Cv \\ open_h(Cv, T + 1): a solid block is not a rule.
  4 Kh    = the pixels of Rh whose vertical run of Rh has a text pixel right above and right below it (a stroke crossing
            the rule); Dh = Rh \\ Kh.  Kv, Dv likewise with rows and columns exchanged.
  5 Mh    = the pixels that are not ink within M rows of a Dh pixel of their column; Mv likewise along rows.
  6 fill  = (pct(1, 2) of the histogram of the pixels that are neither ink nor NaN, + 1) / 256 - 0.5 (bins as §7.4; bin
            255 with nothing counted); or `paper` when given (paper_bin is then -1).
  7 out   = fill on D = Dh | Dv | Mh | Mv, the page's own word elsewhere.
  mask bits: 0 Dh, 1 Dv, 2 Mh | Mv, 3 Kh | Kv.
"""
import numpy as np

F = np.float32
INFO_KEYS = ("paper_bin", "fill", "ink", "counted", "h_removed", "v_removed", "overwritten", "kept")


def default_params():
    return {"threshold": 0.0, "min_length": 96, "max_thickness": 8, "margin": 1, "paper": None}


def valid_params(threshold=0.0, min_length=96, max_thickness=8, margin=1, paper=None):
    ints = all(isinstance(v, (int, np.integer)) for v in (min_length, max_thickness, margin))
    return bool(ints and np.isfinite(threshold) and 2 <= min_length <= 65535 and 1 <= max_thickness <= 64 and 0 <= margin <= 8
                and (paper is None or not np.isinf(paper)))


def runs(X):
    """Every maximal horizontal run of the boolean [H, W] X as (row, first, past the last), one entry per run."""
    X = np.asarray(X, bool)
    edge = np.zeros((X.shape[0], X.shape[1] + 2), np.int8)
    edge[:, 1:-1] = X
    d = np.diff(edge, axis=1)
    r0, first = np.nonzero(d == 1)      # row-major order: the k-th start and the k-th end belong to the same run
    r1, past = np.nonzero(d == -1)
    assert np.array_equal(r0, r1)
    return r0, first, past


def paint(shape, row, first, past):
    """The boolean mask of the given runs."""
    edge = np.zeros((shape[0], shape[1] + 1), np.int32)
    np.add.at(edge, (row, first), 1)
    np.add.at(edge, (row, past), -1)
    return np.cumsum(edge, axis=1)[:, :-1] > 0


def open_h(X, n):
    row, first, past = runs(X)
    long = past - first >= n
    return paint(X.shape, row[long], first[long], past[long])


def open_v(X, n):
    return open_h(np.asarray(X, bool).T, n).T


def crossed_v(R, text):
    """The pixels of R whose vertical run of R has a text pixel right above and right below it."""
    H = R.shape[0]
    col, y0, y1 = runs(R.T)              # the run covers rows y0 .. y1 - 1 of column col
    ok = (y0 >= 1) & (y1 <= H - 1)
    col, y0, y1 = col[ok], y0[ok], y1[ok]
    ok = text[y0 - 1, col] & text[y1, col]
    return paint(R.T.shape, col[ok], y0[ok], y1[ok]).T


def near_v(D, m):
    """The pixels within m rows of a pixel of D in the same column (D included)."""
    out = D.copy()
    for k in range(1, m + 1):
        out[k:] |= D[:-k]
        out[:-k] |= D[k:]
    return out


def bins(v):
    """bin(clamp(v + 0.5f, 0, 1)) as int64; the caller leaves NaN out."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = (np.asarray(v, F) + F(0.5)).astype(F)
        g = np.where(g < F(0), F(0), np.where(g > F(1), F(1), g)).astype(F)
        t = (g * F(256.0)).astype(F)
        return np.clip(np.floor(np.where(np.isnan(t), F(0), t)), 0.0, 255.0).astype(np.int64)


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


def sets(page, min_length=96, max_thickness=8, margin=1, threshold=0.0):
    """Every set of the definition as a boolean [H, W], by name."""
    v = np.ascontiguousarray(page, F)
    L, T, M = int(min_length), int(max_thickness), int(margin)
    with np.errstate(invalid="ignore"):
        ink = v < F(threshold)
    Ch, Cv = open_h(ink, L), open_v(ink, L)
    text = ink & ~(Ch | Cv)
    Rh = Ch & ~open_v(Ch, T + 1)
    Rv = Cv & ~open_h(Cv, T + 1)
    Kh = crossed_v(Rh, text)
    Kv = crossed_v(Rv.T, text.T).T
    Dh, Dv = Rh & ~Kh, Rv & ~Kv
    Mh = near_v(Dh, M) & ~ink
    Mv = near_v(Dv.T, M).T & ~ink
    return {"ink": ink, "Ch": Ch, "Cv": Cv, "text": text, "Rh": Rh, "Rv": Rv, "Kh": Kh, "Kv": Kv, "Dh": Dh, "Dv": Dv, "Mh": Mh, "Mv": Mv,
            "D": Dh | Dv | Mh | Mv}


def remove_rules(page, min_length=96, max_thickness=8, margin=1, threshold=0.0, paper=None):
    """-> (out float32 [H, W], mask uint8 [H, W], info dict)."""
    if not valid_params(threshold, min_length, max_thickness, margin, paper):
        raise ValueError("rules: parameters out of range")
    v = np.ascontiguousarray(page, F)
    s = sets(v, min_length, max_thickness, margin, threshold)
    counted = ~s["ink"] & ~np.isnan(v)
    h = np.bincount(bins(v[counted]).reshape(-1), minlength=256).astype(np.int64)
    if paper is None or np.isnan(paper):
        paper_bin = pct(h, 1, 2)
        paper_bin = 255 if paper_bin < 0 else paper_bin
        fill = F(F(paper_bin + 1) / F(256.0) - F(0.5))
    else:
        paper_bin, fill = -1, F(paper)
    out = v.copy()
    out.view(np.uint32)[s["D"]] = np.array([fill], F).view(np.uint32)[0]
    mask = (s["Dh"] * 1 + s["Dv"] * 2 + (s["Mh"] | s["Mv"]) * 4 + (s["Kh"] | s["Kv"]) * 8).astype(np.uint8)
    info = {"paper_bin": int(paper_bin), "fill": float(fill), "ink": int(s["ink"].sum()), "counted": int(counted.sum()),
            "h_removed": int(s["Dh"].sum()), "v_removed": int(s["Dv"].sum()), "overwritten": int(s["D"].sum()),
            "kept": int((s["Kh"] | s["Kv"]).sum())}
    return out, mask, info


def draw_grid(clean, underlines=()):
    """The table page of DESIGN.md §7.8 from a prepared page (512 x 512 there, synth.synthetic_page(3, 512, 512, 30, 2, 1)): a
    2-pixel table grid drawn at -0.5, its rows and columns placed in proportion to the page, and 1-pixel underlines
    (row, first column, past the last) -> (the ruled page, the rules' pixels)."""
    clean = np.ascontiguousarray(clean, F)
    H, W = clean.shape
    rule = np.zeros((H, W), bool)
    rows, cols = [r * H // 512 for r in (8, 130, 260, 400)], [c * W // 512 for c in (6, 250, 504)]
    for r in rows:
        rule[r:r + 2, cols[0]:cols[-1] + 2] = True
    for c in cols:
        rule[rows[0]:rows[-1] + 2, c:c + 2] = True
    for r, a, b in underlines:
        rule[r, a:b] = True
    ruled = clean.copy()
    ruled[rule] = F(-0.5)
    return ruled, rule


def grid_counts(clean, rule, out):
    """(rule ink left, word ink lost, word ink) of a cleaned page, ink being < 0."""
    ink = clean < F(0)
    return int(((out < F(0)) & rule & ~ink).sum()), int((ink & ~(out < F(0))).sum()), int(ink.sum())
