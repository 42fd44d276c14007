"""One-block graphs of the detection U-Net's DoubleConv blocks, and the case list that the block tests walk.

The fused blocks (kernels_det.hip, kernels_det_stream.hip, kernels_det_rows.hip) are otherwise reached only through
whole models of one form (modelfile.build_detection: ReLU after the pointwise convs only, 2x2 pools, so the decoder's
pad offset is always 0, and a sigmoid of a logit that one hand-set channel dominates).  Here each block stands alone in a
graph whose output IS the block's output, every weight is seeded random (He scale, small non-zero biases), and the four
ReLU flags, the pool that makes the decoder's low-resolution input and the tensor sizes are free.

  encoder (cs -> cmid -> cout):   [lift 1 -> cs]  dw3 -> pw -> dw3 -> pw -> y -> MaxPool 2x2 -> ypool
                                  two graphs from the same weights: out = ypool, and out = y with the pool kept as a consumer
                                  (both fuse with the pool: model_load.cpp's matcher takes the pool whoever else reads y)
  decoder (cs, cx -> cmid -> cout):  skip = lift 1 -> cs;  x1 = MaxPool(kh, kw)(lift 1 -> cx);
                                  ConvT2(x1) -> PADCAT(skip, up) -> dw3 -> pw -> dw3 -> pw -> y [-> conv 1x1 -> 1 [-> sigmoid]]

`companion` is the same block in a detection-shaped graph (fixed input size, one output channel at the input's size) that
an OcrEngine can run, so that its per-launch kernel counters show which kernel family took the block.

`expected_family` restates, from the kernels' query functions, which family takes which request; the GPU test asserts it
against the counters, so a request that silently takes another path fails there.
"""
from collections import namedtuple

import numpy as np

from ocrs_amd import modelfile as mf

# name -> (cs, cx, cmid, cout, final conv).  The nine shapes of the OCRS_DC table in double_conv_fused, and one outside it.
SHAPES = {
    "enc1": (1, 0, 8, 8, False), "enc8": (8, 0, 16, 16, False), "enc16": (16, 0, 32, 32, False), "enc32": (32, 0, 32, 32, False),
    "dec8f": (8, 16, 8, 8, True), "dec8": (8, 16, 8, 8, False), "dec16": (16, 32, 16, 16, False),
    "dec32": (32, 32, 32, 32, False), "dec64": (32, 64, 32, 32, False),
    "enc8x8": (8, 0, 8, 8, False),
}
TABLE = [s for s in SHAPES if s != "enc8x8"]
TILE = {"enc1": (16, 32), "enc8": (8, 32), "enc16": (8, 16), "enc32": (8, 16), "dec8f": (8, 32), "dec8": (8, 32),
        "dec16": (8, 16), "dec32": (8, 16), "dec64": (8, 16)}           # LDS-tiled blocks: TH x TW
WAVE = ("enc1", "dec8f", "dec8")                                         # double_conv_stream's table
ROWS = ("enc8", "dec16", "dec32", "dec64")                               # double_conv_rows' table
WAVE_S, ROWS_S = (8, 14, 32), (8, 14, 20, 32)                            # segment heights
STRIP = 60                                                               # kValid: output columns of a 64-lane strip
KERNEL_CLASS = {"tiled": "det_fused_block", "wave": "det_stream_wave_block", "rows": "det_stream_rows_block"}

# tail: "pool" (encoder), "y" (decoder without a final conv), "fin" / "finsig" (final 1x1 conv -> 1 [-> sigmoid])
# pool: the (kh, kw) of the MaxPool that makes x1 (decoder);  values: "normal" | "nonfinite" | "tiny"
Case = namedtuple("Case", "id shape tail relu n h w pool values")


def is_dec(shape):
    return SHAPES[shape][1] > 0


def modes(shape):
    """The (det_fuse, det_stream, det_rows) settings a case runs under: the per-operator kernels, the tiled block, every
    segment height of the streaming family that has the shape, and the defaults."""
    m = [(0, 1, 1), (1, 0, 0)]
    if shape in WAVE:
        m += [(1, s, 0) for s in WAVE_S] + [(1, 1, 0)]
    if shape in ROWS:
        m += [(1, 0, s) for s in ROWS_S] + [(1, 0, 1)]
    return m + [(1, 1, 1)]


def expected_family(case, mode):
    """-> "rows" | "wave" | "tiled" | None (per-operator kernels): double_conv_fused's order and double_conv_rows_takes."""
    fuse, stream, rows = mode
    if not fuse or case.shape not in TABLE:
        return None
    if rows >= 1 and case.shape in ROWS:
        pxo = (case.w - 2 * (case.w // case.pool[1])) // 2 if is_dec(case.shape) else 0
        if not (rows == 1 and case.n > 8) and not (pxo & 1):
            return "rows"
    if stream >= 1 and case.shape in WAVE:
        return "wave"
    return "tiled"


def pad_of(case):
    """(h - 2 h1, w - 2 w1) of a decoder case."""
    return case.h - 2 * (case.h // case.pool[0]), case.w - 2 * (case.w // case.pool[1])


# ------------------------------------------------------------------------------------------------ the case list
RELUS = [(d1, p1, d2, p2) for d1 in (0, 1) for p1 in (0, 1) for d2 in (0, 1) for p2 in (0, 1)]
# h: 2, 3; T - 1, T, T + 1, 2 T + 1 of the tile heights 8 and 16; S - 1, S, S + 1 of the segment heights 8, 14, 20, 32.
# w: 2, 3, 5 (narrower than a strip); the same of the tile widths 16 and 32; 59, 60, 61, 119, 120, 121 around one and two strips.
SIZES = [(2, 2), (3, 3), (7, 15), (8, 16), (9, 17), (13, 31), (14, 32), (15, 33), (16, 59), (17, 60), (19, 61), (20, 65),
         (21, 119), (31, 120), (32, 121), (33, 5)]
# (h, w, kh, kw) -> (h - 2 h1, w - 2 w1): (2,2) (3,2) (2,3) (4,4) (5,1) (1,5) and two larger, (14,44): pxo 22, (7,42): pxo 21;
# (0,0) (1,1) (0,1) (1,0) come with the 2x2 pool of the size list
PADS = [(6, 6, 3, 3), (7, 4, 3, 3), (4, 7, 3, 3), (12, 12, 3, 3), (13, 61, 3, 2), (33, 13, 2, 3), (40, 130, 3, 3), (21, 126, 3, 3)]
PAD_PAIRS = [(0, 0), (1, 1), (0, 1), (2, 2), (3, 2), (2, 3), (4, 4), (5, 1), (1, 5), (14, 44), (7, 42)]


def _tails(shape):
    if not is_dec(shape):
        return ["pool"]
    return ["fin", "finsig"] if SHAPES[shape][4] else ["y"]


def _cases():
    out = []

    def add(shape, tail, relu, n, h, w, pool, values):
        cid = "%s-%s-r%d%d%d%d-n%d-%dx%d-p%dx%d-%s" % ((shape, tail) + tuple(relu) + (n, h, w) + tuple(pool) + (values,))
        out.append(Case(cid, shape, tail, tuple(relu), n, h, w, tuple(pool), values))

    for si, shape in enumerate(SHAPES):
        for tail in _tails(shape):
            off = si + (tail == "finsig")
            # every ReLU placement, each at another size of the size list and another page count (1 .. 9)
            for r, relu in enumerate(RELUS):
                h, w = SIZES[(r + off) % len(SIZES)]
                add(shape, tail, relu, 1 + (r + 2 * off) % 9, h, w, (2, 2), "normal")
            if is_dec(shape):
                for p, (h, w, kh, kw) in enumerate(PADS):
                    add(shape, tail, RELUS[(5 * p + 3 * off + 1) % 16], 1 + (p + off) % 3, h, w, (kh, kw), "normal")
            if shape == "enc8x8":
                continue
            # NaN / Inf: with no ReLU at all (a NaN spreads through both depthwise convs and the pool), with every ReLU
            # (v > 0 ? v : 0 turns NaN and -Inf into 0, +Inf stays), and with the placement of the real models
            for relu, (h, w), pool in [((0, 0, 0, 0), (33, 121), (3, 3)), ((1, 1, 1, 1), (21, 65), (2, 2)), ((0, 1, 0, 1), (33, 121), (2, 2))]:
                add(shape, tail, relu, 2, h, w, pool if is_dec(shape) else (2, 2), "nonfinite")
            for relu, (h, w) in [((0, 1, 0, 1), (17, 33)), ((0, 0, 0, 0), (20, 61))]:
                add(shape, tail, relu, 2, h, w, (2, 2), "tiny")
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------------ graphs
def _neg0(case):
    """The tiny group's case without any ReLU: every weight positive and every bias -0.0, so the inside of the input's -0.0
    patch is -0.0 in every tensor up to the output (all terms of every chain are -0.0) while the +0.0 patch gives +0.0: a
    kernel whose accumulator starts from +0.0 instead of the bias, or that adds a +0.0 anywhere, loses the sign."""
    return case.values == "tiny" and case.relu == (0, 0, 0, 0)


def _he(rng, shape, fan_in, neg0=False):
    w = (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
    return np.abs(w) if neg0 else w


def _bias(rng, n, values, neg0=False):
    b = (rng.standard_normal(n) * 0.1).astype(np.float32)
    if values == "tiny":          # +0.0 and -0.0 biases only: an all-zero patch stays exactly zero through the block, and
        b = np.where((b > 0) & (not neg0), np.float32(0.0), np.float32(-0.0)).astype(np.float32)   # the zero's sign follows the chain
    return b


def nonfinite_points(h, w):
    """(page, y, x, value): the corners, and rows / columns on both sides of the tile, strip and segment boundaries.  The
    last rows and columns also put them into x1's border, next to the decoder's zero padding."""
    rows = [r for r in (7, 8, 13, 14, 15, 16, 19, 20, 31, 32) if r < h - 2]
    cols = [c for c in (15, 16, 31, 32, 59, 60, 61, 63, 64, 119, 120) if c < w - 2]
    vals = [np.nan, np.inf, -np.inf]
    pts = [(0, 0, 0), (0, 0, w - 1), (0, h - 1, 0), (0, h - 1, w - 1), (0, h - 2, w - 2), (1, 1, 1), (1, h - 2, 1)]
    for i, r in enumerate(rows):
        pts.append((i % 2, r, cols[(3 * i) % len(cols)] if cols else (5 * i) % w))
    for i, c in enumerate(cols):
        pts.append(((i + 1) % 2, rows[(5 * i + 1) % len(rows)] if rows else (3 * i) % h, c))
    return [(p, y, x, vals[i % 3]) for i, (p, y, x) in enumerate(pts)]


def make_input(case, rng):
    """-> (x, the same with every non-finite element replaced by a finite one)."""
    n, h, w = case.n, case.h, case.w
    x = rng.standard_normal((n, 1, h, w)).astype(np.float32)
    if case.values == "tiny":
        x[:, :, :h // 3, :w // 4] = -0.0                        # all-zero patches: one of -0.0, one of +0.0
        x[:, :, :h // 3, w // 4:w // 2] = 0.0
        x[:, :, :h // 2, w // 2:] *= np.float32(1e-41)          # subnormal inputs
        if _neg0(case):            # (all weights are positive there: a max-pooled x1 would push every output above zero)
            x[:, :, h // 2:] -= np.float32(0.7)
        assert (np.abs(x[x != 0]) < 2.0 ** -126).any()
    fin = x.copy()
    if case.values == "nonfinite":
        for p, yy, xx, v in nonfinite_points(h, w):
            x[p, 0, yy, xx] = v
    return x, fin


Built = namedtuple("Built", "graphs companion x x_finite slots")


def build(case):
    """graphs: {name: (model bytes, output slot)} — the outputs to compare ("ypool" and "y" for an encoder block, one for a
    decoder block); companion: the detection-shaped model bytes; slots: names of the slots of interest."""
    cs, cx, cmid, cout, final = SHAPES[case.shape]
    rng = np.random.default_rng([list(SHAPES).index(case.shape), ["pool", "y", "fin", "finsig"].index(case.tail)] + list(case.relu) +
                                [case.n, case.h, case.w] + list(case.pool) + [["normal", "nonfinite", "tiny"].index(case.values)])
    v = case.values
    z0 = _neg0(case)
    rd1, rp1, rd2, rp2 = case.relu
    ops = []
    ns = [1]

    def slot():
        ns[0] += 1
        return ns[0] - 1

    def lift(c, relu=0):
        o = slot()
        ops.append(mf.Op(mf.OP_CONV, 0, o, relu=relu, kh=1, kw=1, cin=1, cout=c,
                         weights=(_he(rng, (1, 1, 1, c), 2, z0), _bias(rng, c, v, z0) * 5)))
        return o

    names = {}
    dec = cx > 0
    if dec:
        # non-finite group: the skip lift has a ReLU, so NaN and -Inf reach the block through x1 alone at those pixels
        skip = lift(cs, relu=1 if v == "nonfinite" else 0)
        xl = lift(cx)
        x1 = slot()
        ops.append(mf.Op(mf.OP_MAXPOOL, xl, x1, kh=case.pool[0], kw=case.pool[1]))
        up = slot()
        ops.append(mf.Op(mf.OP_CONVT2, x1, up, kh=2, kw=2, cin=cx, cout=cs, weights=(_he(rng, (2, 2, cx, cs), cx, z0), _bias(rng, cs, v, z0))))
        src = slot()
        ops.append(mf.Op(mf.OP_PADCAT, skip, src, in1=up))
        names.update(skip=skip, x1=x1, up=up)
        cin = 2 * cs
    else:
        src = lift(cs) if cs > 1 else 0
        cin = cs
    wp1, wp2 = _he(rng, (1, 1, cin, cmid), cin, z0), _he(rng, (1, 1, cmid, cout), cmid, z0)
    if v == "nonfinite":          # exact zeros among the pointwise weights: 0 * Inf and 0 * NaN are NaN, not 0
        wp1[0, 0, ::3, 0] = 0.0
        wp2[0, 0, 1::3, :2] = 0.0
    a, b, c, y = slot(), slot(), slot(), slot()
    ops.append(mf.Op(mf.OP_DWCONV3, src, a, relu=rd1, kh=3, kw=3, cin=cin, cout=cin, weights=(_he(rng, (3, 3, cin), 9, z0), _bias(rng, cin, v, z0))))
    ops.append(mf.Op(mf.OP_CONV, a, b, relu=rp1, kh=1, kw=1, cin=cin, cout=cmid, weights=(wp1, _bias(rng, cmid, v, z0))))
    ops.append(mf.Op(mf.OP_DWCONV3, b, c, relu=rd2, kh=3, kw=3, cin=cmid, cout=cmid, weights=(_he(rng, (3, 3, cmid), 9, z0), _bias(rng, cmid, v, z0))))
    ops.append(mf.Op(mf.OP_CONV, c, y, relu=rp2, kh=1, kw=1, cin=cmid, cout=cout, weights=(wp2, _bias(rng, cout, v, z0))))
    names.update(src=src, y=y)
    # the conv to one channel: seeded random, drawn again until its weights do not all pull one way (after a ReLU the block's
    # output is >= 0, and a logit of one sign everywhere would make the sign checks and the sigmoid's range vacuous)
    while True:
        wf = _he(rng, (1, 1, cout, 1), cout)
        u = wp2[0, 0] @ wf[0, 0, :, 0]           # what the logit sees of the second depthwise conv's output
        if abs(float(wf.sum())) < 0.25 * float(np.abs(wf).sum()) and abs(float(u.sum())) < 0.25 * float(np.abs(u).sum()):
            break
    close_w = (wf, _bias(rng, 1, v))

    def to_bytes(kind, oplist, n_slots, out):
        shape = [-1, 1, case.h, case.w] if kind == mf.KIND_DETECTION else [-1, 1, -1, -1]
        return mf.Graph(kind, shape, oplist, n_slots, out).to_bytes()

    graphs = {}
    if not dec:
        yp = slot()
        ops.append(mf.Op(mf.OP_MAXPOOL, y, yp, kh=2, kw=2))
        names["ypool"] = yp
        graphs["ypool"] = (to_bytes(mf.KIND_RECOGNITION, ops, ns[0], yp), yp)
        graphs["y"] = (to_bytes(mf.KIND_RECOGNITION, ops, ns[0], y), y)
        z = slot()      # the companion reads y: one channel at the input's size; the pool stays a consumer of y
        comp = ops + [mf.Op(mf.OP_CONV, y, z, relu=1, kh=1, kw=1, cin=cout, cout=1, weights=close_w)]
        companion = to_bytes(mf.KIND_DETECTION, comp, ns[0], z)
    elif case.tail == "y":
        graphs["y"] = (to_bytes(mf.KIND_RECOGNITION, ops, ns[0], y), y)
        z = slot()      # closed by a conv WITH a ReLU: one without would be matched as the block's final conv
        comp = ops + [mf.Op(mf.OP_CONV, y, z, relu=1, kh=1, kw=1, cin=cout, cout=1, weights=close_w)]
        companion = to_bytes(mf.KIND_DETECTION, comp, ns[0], z)
    else:
        z = slot()
        ops.append(mf.Op(mf.OP_CONV, y, z, relu=0, kh=1, kw=1, cin=cout, cout=1, weights=close_w))
        names["logit"] = out = z
        if case.tail == "finsig":
            out = slot()
            ops.append(mf.Op(mf.OP_SIGMOID, z, out))
        graphs[case.tail] = (to_bytes(mf.KIND_RECOGNITION, ops, ns[0], out), out)
        companion = to_bytes(mf.KIND_DETECTION, ops, ns[0], out)
    x, fin = make_input(case, rng)
    return Built(graphs, companion, x, fin, names)


# ------------------------------------------------------------------------------------------------ checks shared by the CPU and GPU tests
def same_bits(got, exp, what):
    """uint32 views equal outside NaN positions (so -0.0 is not +0.0), NaN positions identical; NaN payload and sign are not
    compared (the host's and the GPU's default NaNs differ)."""
    assert got.shape == exp.shape and got.dtype == np.float32 and exp.dtype == np.float32, (what, got.shape, exp.shape)
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), "%s: NaN positions differ at %d elements, first %s" % (
        what, int((gn != en).sum()), tuple(np.argwhere(gn != en)[0]))
    ne = (np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(exp).view(np.uint32)) & ~gn
    if ne.any():
        i = tuple(np.argwhere(ne)[0])
        raise AssertionError("%s: %d of %d elements differ in bits; first at %s: got %r, expected %r" % (
            what, int(ne.sum()), ne.size, i, got[i], exp[i]))


def self_checks(case, built, slots):
    """The case is not vacuous: asserted on the oracle's slots, for every case."""
    cs, cx, cmid, cout, final = SHAPES[case.shape]
    if is_dec(case.shape):
        sk, up = slots[built.slots["skip"]], slots[built.slots["up"]]
        assert (sk.shape[1] - up.shape[1], sk.shape[2] - up.shape[2]) == pad_of(case), case.id
        assert sk.shape[1] == case.h and sk.shape[2] == case.w
    # the last op with a ReLU flag: pw2, or the final conv (never a ReLU).  The sigmoid is judged by its logit.
    outs = []
    if case.tail in ("fin", "finsig"):
        outs.append((slots[built.slots["logit"]], 0))
    else:
        outs.append((slots[built.slots["y"]], case.relu[3]))
        if case.tail == "pool":
            outs.append((slots[built.slots["ypool"]], case.relu[3]))
    for o, relu in outs:
        if o.shape[1] * o.shape[2] < 16:      # 2x2 and 3x3 images (1x1 pooled): too few values for a share or a sign to mean anything
            continue
        if relu:
            share = float((o == 0).mean())
            assert share <= 0.75, "%s: %.2f of the output is exactly zero" % (case.id, share)
            assert (o > 0).any(), case.id
        else:
            assert (o < 0).any() and (o > 0).any(), "%s: the output has one sign only" % case.id


def coverage(cases=None):
    """What the case list covers, computed from the list: per shape the ReLU placements, the pad pairs, the page counts,
    and per kernel family that takes the shape the heights, widths and (family, segment height) pairs it ran at."""
    cases = CASES if cases is None else cases
    cov = {}
    for c in cases:
        s = cov.setdefault(c.shape, dict(relu={}, pads=set(), n=set(), fam={}, declined=set()))
        s["relu"].setdefault(c.tail, set()).add(c.relu)
        if is_dec(c.shape):
            s["pads"].add(pad_of(c))
        s["n"].add(c.n)
        for m in modes(c.shape):
            f = expected_family(c, m)
            seg = m[1] if f == "wave" else m[2] if f == "rows" else 0
            d = s["fam"].setdefault((f, seg), dict(h=set(), w=set(), n=set(), pads=set(), relu=set()))
            d["h"].add(c.h); d["w"].add(c.w); d["n"].add(c.n); d["relu"].add(c.relu)
            if is_dec(c.shape):
                d["pads"].add(pad_of(c))
            if c.shape in ROWS and m[0] and m[2] >= 1 and f != "rows":
                s["declined"].add("n>8" if (m[2] == 1 and c.n > 8) else "odd pxo")
    return cov
