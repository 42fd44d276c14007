"""The relaxed / reduced recognition kernels against float64, op by op.

The bf16-split contractions — conv3x3_ragged_kernel<..., NP>, conv2 of conv12_fused_split_kernel, gemm_split_kernel<NP> (the
GRU input projections) and gru_split_kernel<H, NP> (the recurrence) — are reached one launch at a time through the engine's
own packed path (ocrs_engine_run_recognition_ops: same options, numerics, stream lease, ragged packing and launches as a
request).  Three kinds of check:

  a. bound: every output element within the float64 bound of f64_ref (split_bound, the fast gates), computed from the op's own
     fp32 input.  Worst-case and loose by design: they catch indexing, tile, tail, chunk and direction faults;
  b. exact probes: one product per output with operands whose bf16 planes are known (f64_ref.SPLIT_PROBES, premises checked on
     the CPU in test_numeric_spec.py), on the activation side (cut by the staging thread) and on the weight side (cut at load),
     spread over rows, columns, taps and K chunks: relaxed must return the exact product, reduced its two-plane value;
  c. relaxed is fp32-class: its RMS and max error against float64 within RELAXED_FACTOR of the exact kernel's on the same
     input, and reduced's larger than relaxed's — the only check that sees a recurrence that lost a state plane.

The hook itself is validated first: the whole range equals recognize_logits in every mode, and every launch-aligned range of
the exact engine equals the oracle's slots bit for bit.

Run with:  python -m pytest -m gpu tests/test_gpu_numerics_split.py
"""
import gc

import numpy as np
import pytest

import f64_ref as R
import models_util as M
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, OcrsError, _lib, synth
from ocrs_amd import modelfile as mf
from oracle import pipeline as OP
from oracle.nn import OracleGraph

pytestmark = pytest.mark.gpu
MODES = {"relaxed": 3, "reduced": 2}
OP_CONV, OP_MAXPOOL, OP_AVGPOOL, OP_TOSEQ, OP_GRU = 0, 2, 3, 7, 8
# relaxed / exact error against float64 (RMS and max over an op's output), measured on an MI355X over the ops of
# test_relaxed_is_fp32_class: 0.80-1.15 (RMS) and 0.85-1.34 (max); reduced 9.8-20.4 and 4.2-17.4.  The limit is 1.5x the
# measured worst of relaxed.
RELAXED_FACTOR = 2.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()   # fail loudly: there is no CPU fallback to "pass" on


def make_engine(buf, numerics="exact", **opts):
    return OcrEngine(recognition_model=Model.load_bytes(buf), numerics=numerics, options=opts or None)


def release():
    """Collect the engines the caller has dropped (`del eng` first): one engine per mode at a time, since a relaxed engine puts
    the device into the serial regime while it exists."""
    gc.collect()


def graph_ops(buf):
    return OracleGraph(buf).ops


def conv_w(op):
    return op["w"][0].reshape(op["kh"], op["kw"], op["cin"], op["cout"]), op["w"][1]


def gru_w(op, d):
    I, H = op["cin"], op["hidden"]
    wi, bi, wh, bh = op["w"][4 * d:4 * d + 4]
    return wi.reshape(I, 3 * H), bi, wh.reshape(H, 3 * H), bh


def pooled(ref, kh, kw):
    """A max pool of a bounded value: the pool is 1-Lipschitz in the max norm, so the bound is the window's largest."""
    y, b = ref
    return R._windows(y, kh, kw).max(axis=(2, 4)), R._windows(b, kh, kw).max(axis=(2, 4))


def conv_ref(x, op, np_, pool):
    w, b = conv_w(op)
    ref = R.conv_split(x[None], w, b, np_, op["relu"]) if np_ else R.conv(x[None], w, b, op["relu"])
    return pooled(ref, *pool) if pool else ref


def shapes_at(buf, widths, slot):
    """The per-line shape of a slot (without the batch axis: [H, W, C], or [T, 1, C] for sequences) for lines of
    model-input widths `widths` (the graph's shape rules: 'same' convs, floor pools)."""
    out = []
    for w in widths:
        shp = {0: (IN_H, w, 1)}
        for o in graph_ops(buf):
            h, ww, c = shp[o["in0"]]
            if o["type"] == OP_CONV:
                shp[o["out"]] = (h, ww, o["cout"])
            elif o["type"] in (OP_MAXPOOL, OP_AVGPOOL):
                shp[o["out"]] = (h // o["kh"], ww // o["kw"], c)
            elif o["type"] == OP_TOSEQ:
                shp[o["out"]] = (ww, 1, c)
            elif o["type"] == OP_GRU:
                shp[o["out"]] = (h, 1, 2 * o["hidden"])
            else:
                shp[o["out"]] = (h, 1, o["cout"] or c)
        out.append(shp[slot])
    return out


def relu_input(rng, shape, scale=1.0):
    x = rng.standard_normal(shape).astype(np.float32) * np.float32(scale)
    return np.maximum(x, 0).astype(np.float32)


def check_bound(got, ref, what):
    R.check(got, ref, what)
    y64, b = ref
    return float(np.max(np.abs(np.asarray(got, np.float64) - y64) / np.maximum(b, 1e-300), initial=0))


# ------------------------------------------------------------------ models
IN_H = 64


@pytest.fixture(scope="module")
def prod():
    return M.recognition_model_bytes()


def wide_model():
    """Cin 64 / 128 / 256, Cout 128 / 256, a split conv with the fused 2 x 2 pool (conv2: conv1 has 64 channels, so there is
    no conv1 + conv2 launch), H = 128."""
    return mf.build_recognition(n_classes=97, in_h=IN_H, seed=5, hidden=128, chans=(64, 128, 256, 256, 128, 256)).to_bytes()


# Line widths (model input) for the split convs.  Which <TW, PH, PW, FLAT> a conv runs is decided per request: 16-column
# patches where they make fewer tiles than 32-column ones, flat tiling with conv_flat = 1 when every pooled width is >= 11
# (conv_variant below mirrors that choice; test_width_sets_reach_every_split_conv_instantiation checks the sets together
# reach all of them).
#   RAGGED: pooled widths 1-4, widths that end inside 16- and 32-column tiles, several tiles, one line alone in its group and
#           a group of many (never flat: widths below 11);
#   NARROW: every pooled width below 11 (16-column patches, never flat);
#   WIDE:   pooled widths 32 / 64 / 96 (32-column patches; flat under conv_flat = 1);
#   FLAT16: pooled widths 12-16 (16-column patches, flat under conv_flat = 1);
#   GROUPS: the width groups of real requests (multiples of 50: 16-column patches, flat under conv_flat = 1, conv2 of the wide
#           model included).
RAGGED_WIDTHS = [4, 8, 12, 16, 44, 68, 132, 180, 260] + [200] * 9
NARROW_WIDTHS = [4, 8, 12, 16, 24, 28, 40]
WIDE_WIDTHS = [128, 256, 384, 128]
FLAT16_WIDTHS = [48, 52, 56, 64]
GROUP_WIDTHS = [50, 100, 150, 150, 200, 250]
BOUND_WIDTH_SETS = (RAGGED_WIDTHS, NARROW_WIDTHS, WIDE_WIDTHS, FLAT16_WIDTHS, GROUP_WIDTHS, [40])
PROBE_WIDTH_SETS = (RAGGED_WIDTHS, WIDE_WIDTHS, FLAT16_WIDTHS, GROUP_WIDTHS)


def launches(buf):
    """The launch boundaries of the packed path under the default options: [(first, last)] op ranges."""
    ops = graph_ops(buf)
    ts = next(i for i, o in enumerate(ops) if o["type"] == OP_TOSEQ)
    out, i = [], 0
    while i < len(ops):
        o = ops[i]
        if o["type"] == OP_CONV and o["cin"] == 1:
            # conv1 + conv2 in one launch: 32 and 64 channels (kernels_rec.hip F12_MID, F12_COUT) and pooled widths >= 11
            j = i + 3 if (i + 3 < ts and ops[i + 2]["type"] == OP_CONV and o["cout"] == 32 and ops[i + 2]["cout"] == 64
                          and ops[i + 3]["type"] == OP_MAXPOOL) else i + 1
        elif o["type"] == OP_CONV and i + 1 < ts and ops[i + 1]["type"] == OP_MAXPOOL and ops[i + 1]["kh"] == 2:
            j = i + 1
        elif o["type"] == OP_AVGPOOL and i + 1 == ts:
            j = ts
        else:
            j = i
        out.append((i, j))
        i = j + 1
    return out


def conv_variant(buf, widths, op, pool, conv_flat):
    """(TW, PH, PW, FLAT) of the conv3x3_ragged_kernel a request of these line widths runs at conv `op` (the choice of
    HipModel::run_prefix_ragged's view and k::conv3x3_ragged; lines of equal width form one group)."""
    h, _, _ = shapes_at(buf, widths[:1], graph_ops(buf)[op]["in0"])[0]
    groups = {}
    for w in widths:
        groups[w] = groups.get(w, 0) + 1
    cols = {w: shapes_at(buf, [w], graph_ops(buf)[op]["in0"])[0][1] for w in groups}
    nt32 = sum(n * (h // 4) * -(-cols[w] // 32) for w, n in groups.items())
    nt16 = sum(n * (h // 8) * -(-cols[w] // 16) for w, n in groups.items())
    tw = 16 if h % 8 == 0 and (h % 4 != 0 or nt16 < nt32) else 32
    flat = bool(conv_flat) and min(cols.values()) >= 11
    return (tw,) + (pool or (1, 1)) + (flat,)


def split_convs(buf):
    """(op index, fused pool or None) of every conv the split kernel takes: Cin % 64 == 0, Cout % 128 == 0."""
    ops = graph_ops(buf)
    res = []
    for a, b in launches(buf):
        o = ops[a]
        if o["type"] == OP_CONV and o["cin"] > 1 and o["cin"] % 64 == 0 and o["cout"] % 128 == 0:
            res.append((a, (ops[b]["kh"], ops[b]["kw"]) if b > a else None))
    return res


# ------------------------------------------------------------------ 1. the hook
@pytest.fixture(scope="module")
def page_lines(prod):
    """Lines of a synthetic page and their model inputs: the crop (prepare_recognition_input) padded to its width group
    (a multiple of 50) with the black value, as a request lays them out."""
    eng = OcrEngine(detection_model=Model.load_bytes(M.detection_model_bytes()), recognition_model=Model.load_bytes(prod))
    px = synth.synthetic_page(71, 800, 1000, lines=16)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    lines, widths, xs = [], [], []
    for line in eng.find_text_lines(inp, eng.detect_words(inp)):
        crop = eng.prepare_recognition_input(inp, line)
        if crop.shape[1] == 0 or len(lines) == 24:
            continue
        gw = -(-crop.shape[1] // 50) * 50
        x = np.full((crop.shape[0], gw), OP.BLACK_VALUE, np.float32)
        x[:, :crop.shape[1]] = crop
        lines.append(line)
        widths.append(gw)
        xs.append(x[:, :, None])
    del eng
    release()
    return px, lines, widths, xs


@pytest.mark.parametrize("mode", ["exact", "relaxed", "reduced"])
def test_hook_whole_range_equals_recognize_logits(prod, page_lines, mode):
    px, lines, widths, xs = page_lines
    eng = make_engine(prod, mode)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    want = eng.recognize_logits(inp, lines)
    n_ops = len(graph_ops(prod))
    got = eng.run_recognition_ops(widths, 0, n_ops - 1, xs)
    del eng
    release()
    assert len(got) == len(want) and len(want) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        g = g.reshape(w.shape)
        assert np.array_equal(g, w, equal_nan=True), "%s: line %d: ops [0, %d] differ from recognize_logits" % (mode, i, n_ops - 1)


def test_hook_op_ranges_equal_the_oracle_slots(prod):
    """Exact engine: every launch alone, and runs of several, equal the oracle's run_exact slots bit for bit — the packed
    path's intermediates, not only its end."""
    g = OracleGraph(prod)
    ops = g.ops
    widths = RAGGED_WIDTHS
    slots = []
    for w in widths:
        rng = np.random.default_rng(w)
        x = (rng.random((1, 1, IN_H, w), np.float32) - np.float32(0.5)).astype(np.float32)
        slots.append(g.run_exact(x, return_slots=True)[1])

    def per_line(slot):
        return [s[slot][0] if s[slot].ndim == 4 else s[slot] for s in slots]

    eng = make_engine(prod)
    spans = launches(prod)
    ranges = spans + [(spans[0][0], spans[2][1]), (spans[3][0], spans[-1][1]), (spans[-4][0], spans[-2][1])]
    try:
        for a, b in ranges:
            got = eng.run_recognition_ops(widths, a, b, per_line(ops[a]["in0"]))
            want = per_line(ops[b]["out"])
            for i, (gg, ww) in enumerate(zip(got, want)):
                assert gg.shape == ww.shape, (a, b, i, gg.shape, ww.shape)
                assert np.array_equal(gg, ww, equal_nan=True), "ops [%d, %d], line %d (width %d) differ from the oracle" % (
                    a, b, i, widths[i])
    finally:
        del eng
        release()


def test_hook_refuses_ranges_inside_fused_launches(prod):
    ops = graph_ops(prod)
    eng = make_engine(prod)
    widths = [200, 200]
    try:
        for a, b in launches(prod):
            if b == a:
                continue
            for first, last in ((a + 1, b), (a, b - 1)):
                shp = shapes_at(prod, widths, ops[first]["in0"])
                xs = [np.zeros(s, np.float32) for s in shp]
                with pytest.raises(OcrsError, match="inside the fused launch of ops %d..%d" % (a, b)):
                    eng.run_recognition_ops(widths, first, last, xs)
        with pytest.raises(OcrsError):
            eng.run_recognition_ops(widths, 5, 4, [np.zeros(1, np.float32)] * 2)
    finally:
        del eng
        release()


# ------------------------------------------------------------------ 2a. bounds on random data, 2c. relaxed vs exact
def run_conv_case(buf, eng, np_, widths, rng, errs=None, tag=""):
    """Every split conv launch of the model on random ReLU'd inputs, each element within the bound; returns worst ratios."""
    ops = graph_ops(buf)
    worst = {}
    for i, pool in split_convs(buf):
        last = i + 1 if pool else i
        shp = shapes_at(buf, widths, ops[i]["in0"])
        xs = [relu_input(rng, s) for s in shp]
        got = eng.run_recognition_ops(widths, i, last, xs)
        r = 0.0
        for li, (x, y) in enumerate(zip(xs, got)):
            ref = conv_ref(x, ops[i], np_, pool)
            r = max(r, check_bound(y[None], ref, "%s conv op %d (%d->%d) line %d width %d" % (
                tag, i, ops[i]["cin"], ops[i]["cout"], li, widths[li])))
            if errs is not None:
                errs.setdefault(("conv", i, li), []).append((x, y))
        worst["conv%d" % i] = r
    return worst


@pytest.mark.parametrize("conv_flat", [0, 1])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("model", ["prod", "wide"])
def test_split_convs_within_float64_bound(prod, model, mode, conv_flat):
    buf = prod if model == "prod" else wide_model()
    eng = make_engine(buf, mode, conv_flat=conv_flat)
    rng = np.random.default_rng(11 + conv_flat)
    try:
        for widths in BOUND_WIDTH_SETS:
            w = run_conv_case(buf, eng, MODES[mode], widths, rng, tag="%s %s flat %d" % (model, mode, conv_flat))
            print("%s %s conv_flat=%d widths %s: worst error / bound %s" % (model, mode, conv_flat, widths[:3], w))
    finally:
        del eng
        release()


def test_width_sets_reach_every_split_conv_instantiation(prod):
    """The bound test's width sets, over the two models and conv_flat 0 / 1, reach every <TW, PH, PW, FLAT> the dispatcher
    can pick for a split conv (x NP 2 / 3 by the mode parameter: the 24 instantiations); the probe sets reach every one the
    default conv_flat = 1 can."""
    every = {(tw, ph, pw, fl) for tw in (16, 32) for ph, pw in ((1, 1), (2, 1), (2, 2)) for fl in (False, True)}
    bound, probe = set(), set()
    for buf in (prod, wide_model()):
        for i, pool in split_convs(buf):
            for flat in (0, 1):
                bound |= {conv_variant(buf, ws, i, pool, flat) for ws in BOUND_WIDTH_SETS}
            probe |= {conv_variant(buf, ws, i, pool, 1) for ws in PROBE_WIDTH_SETS}
    assert bound == every, sorted(every - bound)
    assert {v for v in every if v[3]} <= probe, sorted({v for v in every if v[3]} - probe)


@pytest.mark.parametrize("mode", list(MODES))
def test_conv12_split_within_float64_bound(prod, mode):
    """conv1 (exact, the spec's chain: the oracle's bits) + pool + conv2 (split) + pool in one launch; narrow lines (pooled
    width 11-13: the gap tiles put images one column apart) and wide ones."""
    g = OracleGraph(prod)
    ops = g.ops
    a, b = launches(prod)[0]
    assert b == a + 3
    widths = [22, 24, 26, 44, 100, 150, 300, 52, 52, 52]
    rng = np.random.default_rng(3)
    xs = [(rng.random((IN_H, w, 1), np.float32) - np.float32(0.5)).astype(np.float32) for w in widths]
    eng = make_engine(prod, mode)
    try:
        got = eng.run_recognition_ops(widths, a, b, xs)
    finally:
        del eng
        release()
    worst = 0.0
    for li, (x, y) in enumerate(zip(xs, got)):
        mid = g.run_exact(x[None, :, :, 0][:, None], return_slots=True)[1][ops[a + 1]["out"]][0]
        ref = conv_ref(mid, ops[a + 2], MODES[mode], (2, 2))
        worst = max(worst, check_bound(y[None], ref, "conv12 %s line %d width %d" % (mode, li, widths[li])))
    print("conv12 %s: worst error / bound %.3g" % (mode, worst))


def gru_ops(buf):
    return [i for i, o in enumerate(graph_ops(buf)) if o["type"] == OP_GRU]


def seq_inputs(rng, Ts, I, scale=0.5):
    return [(rng.standard_normal((T, 1, I)) * scale).astype(np.float32) for T in Ts]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", ["prod_l0", "prod_l1", "k64"])
def test_gemm_split_within_float64_bound(prod, mode, case):
    """The GRU input projections alone (gx of both directions): M = 1, 127, 128, 129 and > 16 384 rows; K = 128, 512 and 64
    (every chunk peeled); N = 3H for H = 256 and 128."""
    if case == "k64":
        buf = mf.build_recognition(n_classes=97, in_h=IN_H, seed=6, hidden=128, chans=(32, 64, 64, 64, 64, 64)).to_bytes()
        gi = gru_ops(buf)[0]
    else:
        buf = prod
        gi = gru_ops(buf)[0 if case == "prod_l0" else 1]
    op = graph_ops(buf)[gi]
    I, H = op["cin"], op["hidden"]
    assert (3 * H) % 128 == 0 and I % 64 == 0
    rng = np.random.default_rng(gi)
    requests = [[1], [127], [128], [129], [600] * 28 + [300] * 2, [5, 17, 33, 64, 200, 600, 1]]
    eng = make_engine(buf, mode)
    worst = 0.0
    try:
        for Ts in requests:
            xs = seq_inputs(rng, Ts, I)
            got = eng.run_recognition_ops([4 * T for T in Ts], gi, gi, xs, gx_only=True)
            for li, (x, y) in enumerate(zip(xs, got)):
                assert y.shape == (2, Ts[li], 3 * H)
                for d in range(2):
                    wi, bi, _, _ = gru_w(op, d)
                    ref = R.linear_split(x[:, 0], wi, bi, MODES[mode])
                    worst = max(worst, check_bound(y[d], ref, "gemm %s %s M=%d line %d dir %d" % (case, mode, sum(Ts), li, d)))
    finally:
        del eng
        release()
    print("gemm_split %s %s: worst error / bound %.3g" % (case, mode, worst))


def recurrence_bound(op, x, y, proj_np, hid_np, fast):
    ws = []
    for d in range(2):
        ws += list(gru_w(op, d))
    return R.gru_bidir(x, ws, y, proj_np=proj_np, hid_np=hid_np, fast_gates=fast)


def gru_model(H):
    chans = (32, 64, 64, 64, 64, 64) if H == 64 else (32, 64, 128, 128, 128, 128)
    return mf.build_recognition(n_classes=97, in_h=IN_H, seed=7 + H, hidden=H, chans=chans).to_bytes()


def recurrence_lengths(n):
    if n == 1:
        return [600]
    rng = np.random.default_rng(n)
    return sorted({int(v) for v in rng.integers(1, 600, 4 * n)}, reverse=True)[:n - 1] + [600]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("H", [64, 128, 256])
def test_recurrence_within_float64_bound(mode, H):
    """A whole GRU op (projection + gru_split_kernel<H, NP>) per step against the float64 cell applied to the kernel's own
    fp32 state: 1, 16, 17 and ~330 lines of distinct lengths up to T = 600.  H = 64: the projection is not split
    (3H % 128 != 0), the recurrence is."""
    buf = gru_model(H)
    gi = gru_ops(buf)[0]
    op = graph_ops(buf)[gi]
    np_ = MODES[mode]
    proj_np = np_ if (3 * H) % 128 == 0 and op["cin"] % 64 == 0 else 0
    rng = np.random.default_rng(H)
    eng = make_engine(buf, mode)
    worst = 0.0
    try:
        for n in (1, 16, 17, 330):
            Ts = recurrence_lengths(n)
            xs = seq_inputs(rng, Ts, op["cin"])
            got = eng.run_recognition_ops([4 * T for T in Ts], gi, gi, xs)
            for li in range(0, len(Ts), max(1, len(Ts) // 24)):   # every line's row is checked on the smaller requests
                ref = recurrence_bound(op, xs[li], got[li], proj_np, np_, True)
                worst = max(worst, check_bound(got[li], ref, "GRU H=%d %s %d lines, line %d (T %d)" % (H, mode, n, li, Ts[li])))
    finally:
        del eng
        release()
    print("recurrence H=%d %s: worst error / bound %.3g" % (H, mode, worst))


@pytest.mark.parametrize("H", [64, 128, 256])
def test_split_recurrence_ran(H):
    """Zero inputs make gx the bias exactly in every mode, so relaxed and reduced differ only if the recurrence itself cut the
    state into three and two planes: gru_split_kernel ran (gru_split_supported can decline a shape, and the fp32 persistent
    kernel it falls back to would give both modes the same bits).  Every line of eight steps or more must differ."""
    buf = gru_model(H)
    gi = gru_ops(buf)[0]
    op = graph_ops(buf)[gi]
    requests = [recurrence_lengths(n) for n in (1, 16, 17, 330)]
    got = {}
    for mode in MODES:
        eng = make_engine(buf, mode)
        try:
            got[mode] = [eng.run_recognition_ops([4 * T for T in Ts], gi, gi, [np.zeros((T, 1, op["cin"]), np.float32) for T in Ts])
                         for Ts in requests]
        finally:
            del eng
            release()
    for Ts, rel, red in zip(requests, got["relaxed"], got["reduced"]):
        for li, T in enumerate(Ts):
            if T >= 8:
                assert not np.array_equal(rel[li], red[li]), "H=%d, %d lines: line %d (T %d) has the same bits in both modes" % (
                    H, len(Ts), li, T)


@pytest.mark.parametrize("opts,proj,hid,fast", [
    (dict(gru_mode=1), True, False, False),     # per-step fp32 kernels, spec gates; the projection is still split
    (dict(gru_gates=0), True, True, True),      # the split recurrence does not use the gate-per-wave kernel: the same
    (dict(gru_local=0), True, True, True),
], ids=["gru_mode1", "gru_gates0", "gru_local0"])
def test_recurrence_options_under_relaxed(prod, opts, proj, hid, fast):
    gi = gru_ops(prod)[0]
    op = graph_ops(prod)[gi]
    rng = np.random.default_rng(5)
    Ts = recurrence_lengths(17)
    xs = seq_inputs(rng, Ts, op["cin"])
    eng = make_engine(prod, "relaxed", **opts)
    try:
        got = eng.run_recognition_ops([4 * T for T in Ts], gi, gi, xs)
    finally:
        del eng
        release()
    for li in range(len(Ts)):
        ref = recurrence_bound(op, xs[li], got[li], 3 if proj else 0, 3 if hid else 0, fast)
        R.check(got[li], ref, "GRU %s line %d" % (opts, li))


# ------------------------------------------------------------------ 2b. exact probes
PROBE_CLASSES = len(R.SPLIT_PROBES)


def probe_table(np_):
    return {float(np.float64(a) * np.float64(w)): (rel if np_ == 3 else red) for a, w, rel, red in R.SPLIT_PROBES}


def probe_expect(exact, np_):
    """The float64 result of one-product-per-element probes, each product replaced by what an NP-plane contraction keeps."""
    t = probe_table(np_)
    out = np.array(exact, np.float64)
    for k, v in t.items():
        out[out == k] = v
    assert set(np.unique(out)) <= {0.0} | set(t.values()), "a probe output holds more than one product"
    return out


def conv_probe_model(base_chans, seed, layer_op, w_factory):
    g = mf.build_recognition(n_classes=97, in_h=IN_H, seed=seed, hidden=128, chans=base_chans)
    op = g.ops[layer_op]
    kh, kw, cin, cout = op.kh, op.kw, op.cin, op.cout
    w, b = w_factory(kh, kw, cin, cout)
    op.weights[0] = w.reshape(op.weights[0].shape)
    op.weights[1] = b
    return g


def spread_weights(kh, kw, cin, cout):
    """Output channel j reads exactly one (tap, input channel): channel j % cin at tap (5 j) % 9, with the weight of the
    channel's class — so every output is one product (or zero), and the probes cover every channel and tap: every 16-deep K
    chunk of a tap-major K order holds some (16 consecutive channels meet every tap), and so do most of a channel-major one."""
    w = np.zeros((kh, kw, cin, cout), np.float32)
    for j in range(cout):
        c = j % cin
        t = (5 * j) % 9
        w[t // 3, t % 3, c, j] = R.SPLIT_PROBES[c % PROBE_CLASSES][1]
    return w, np.zeros(cout, np.float32)


def probe_image(shape, rng, n_points=6):
    """Activations nonzero at a few isolated pixels (3+ apart, so their outputs never meet), channel c of class c % 3."""
    H, W, C = shape
    x = np.zeros(shape, np.float32)
    vals = np.array([R.SPLIT_PROBES[c % PROBE_CLASSES][0] for c in range(C)], np.float32)
    ys = list(range(1, H - 1, 4)) or [0]
    xs_ = list(range(0, W, 4))
    pts = [(ys[k % len(ys)], xs_[(k * 7) % len(xs_)]) for k in range(n_points)]
    pts += [(0, W - 1), (H - 1, 0)] if W >= 4 and H >= 4 else []
    for (py, px) in pts:
        x[py, px] = vals
    return x


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("layer", [2, 4, 5, 7, 8])
def test_conv_split_exact_probes(mode, layer):
    """Exact plane probes through each split conv (wide model: Cin 64..256, taps and chunks all covered)."""
    chans = (64, 128, 256, 256, 128, 256)
    g = conv_probe_model(chans, 9, layer, spread_weights)
    buf = g.to_bytes()
    ops = graph_ops(buf)
    pool = None
    for a, b in launches(buf):
        if a == layer:
            pool = (ops[b]["kh"], ops[b]["kw"]) if b > a else None
            last = b
    assert ops[layer]["type"] == OP_CONV
    np_ = MODES[mode]
    rng = np.random.default_rng(layer)
    eng = make_engine(buf, mode)
    try:
        for widths in PROBE_WIDTH_SETS:
            shp = shapes_at(buf, widths, ops[layer]["in0"])
            xs = [probe_image(s, rng) for s in shp]
            got = eng.run_recognition_ops(widths, layer, last, xs)
            for li, (x, y) in enumerate(zip(xs, got)):
                w, b = conv_w(ops[layer])
                exact = R.conv(x[None], w, b, 1)[0]
                if pool:
                    exact = R.maxpool(exact, *pool)[0]
                want = probe_expect(exact, np_)[0]
                if not np.array_equal(np.asarray(y, np.float64), want):
                    bad = np.argwhere(np.asarray(y, np.float64) != want)
                    i = tuple(bad[0])
                    raise AssertionError("%s conv op %d line %d (width %d): %d of %d probe outputs wrong; first at %s: %r, "
                                         "expected %r" % (mode, layer, li, widths[li], len(bad), y.size, i, y[i], want[i]))
    finally:
        del eng
        release()


@pytest.mark.parametrize("mode", list(MODES))
def test_conv12_split_exact_probes(prod, mode):
    """conv2 of the fused conv1 + conv2 launch: conv1's output is its bias (weights zero), so conv2's activations are the
    probe values, cut as conv1 writes them; conv2's weights carry one probe per output channel."""
    g = mf.build_recognition(n_classes=97, in_h=IN_H, seed=2, hidden=256, chans=(32, 64, 128, 128, 128, 128))
    c1, c2 = g.ops[0], g.ops[2]
    c1.weights[0] = np.zeros_like(c1.weights[0])
    c1.weights[1] = np.array([R.SPLIT_PROBES[c % PROBE_CLASSES][0] for c in range(c1.cout)], np.float32)
    w, b = spread_weights(3, 3, c2.cin, c2.cout)
    c2.weights[0] = w.reshape(c2.weights[0].shape)
    c2.weights[1] = b
    buf = g.to_bytes()
    og = OracleGraph(buf)
    ops = og.ops
    widths = [22, 26, 44, 150, 52, 52, 300]
    xs = [np.zeros((IN_H, w_, 1), np.float32) for w_ in widths]
    eng = make_engine(buf, mode)
    try:
        got = eng.run_recognition_ops(widths, 0, 3, xs)
    finally:
        del eng
        release()
    for li, (x, y) in enumerate(zip(xs, got)):
        mid = og.run_exact(x[None, :, :, 0][:, None], return_slots=True)[1][ops[1]["out"]]
        exact = R.maxpool(R.conv(mid, *conv_w(ops[2]), 1)[0], 2, 2)[0]
        want = probe_expect(exact, MODES[mode])[0]
        assert np.array_equal(np.asarray(y, np.float64), want), "conv12 %s line %d (width %d): %d probe outputs wrong" % (
            mode, li, widths[li], int(np.sum(np.asarray(y, np.float64) != want)))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("I,H", [(128, 256), (512, 256), (64, 128)])
def test_gemm_split_exact_probes(mode, I, H):
    """gx = A Wi of both directions with one product per element: row r reads k_r = (7 r) % I, column n of direction d
    k = (5 n + d) % I — the two directions' weights differ — and operand classes follow k % 3, so a row and a column meet on a
    probe pair or not at all.  Every K chunk, the peeled four included, holds probes."""
    chans = (32, 64, 128, 128, 128, I) if I != 64 else (32, 64, 64, 64, 64, 64)
    g = mf.build_recognition(n_classes=97, in_h=IN_H, seed=4, hidden=H, chans=chans)
    gi = [i for i, o in enumerate(g.ops) if o.type == OP_GRU][0 if I != 512 else 1]
    op = g.ops[gi]
    assert op.cin == I
    for d in range(2):
        wi = np.zeros((I, 3 * H), np.float32)
        for n in range(3 * H):
            k = (5 * n + d) % I
            wi[k, n] = R.SPLIT_PROBES[k % PROBE_CLASSES][1]
        op.weights[4 * d] = wi.reshape(op.weights[4 * d].shape)
        op.weights[4 * d + 1] = np.zeros_like(op.weights[4 * d + 1])
    buf = g.to_bytes()
    Ts = [600] * 28 + [129, 1, 3]    # > 16 384 rows
    xs = []
    row = 0
    for T in Ts:
        x = np.zeros((T, 1, I), np.float32)
        for t in range(T):
            k = (7 * (row + t)) % I
            x[t, 0, k] = R.SPLIT_PROBES[k % PROBE_CLASSES][0]
        row += T
        xs.append(x)
    eng = make_engine(buf, mode)
    try:
        got = eng.run_recognition_ops([4 * T for T in Ts], gi, gi, xs, gx_only=True)
    finally:
        del eng
        release()
    ops = graph_ops(buf)
    for li, (x, y) in enumerate(zip(xs, got)):
        for d in range(2):
            wi = gru_w(ops[gi], d)[0]
            want = probe_expect(np.asarray(x[:, 0], np.float64) @ np.asarray(wi, np.float64), MODES[mode])
            assert np.array_equal(np.asarray(y[d], np.float64), want), "gemm %s I=%d line %d dir %d: %d probe outputs wrong" % (
                mode, I, li, d, int(np.sum(np.asarray(y[d], np.float64) != want)))


# ------------------------------------------------------------------ 2c. relaxed is fp32-class
def err_stats(got, y64):
    e = np.abs(np.asarray(got, np.float64) - y64)
    scale = np.abs(y64).max()
    return float(np.sqrt(np.mean(e ** 2)) / scale), float(e.max() / scale)


def test_relaxed_is_fp32_class(prod):
    """On the same inputs, per split op: relaxed's RMS and max error against float64 within RELAXED_FACTOR of the exact
    kernel's, and reduced's larger than relaxed's (the recurrence included: a relaxed recurrence on two state planes fails)."""
    ops = graph_ops(prod)
    rng = np.random.default_rng(99)
    cases = []
    widths = RAGGED_WIDTHS
    for i, pool in split_convs(prod):
        shp = shapes_at(prod, widths, ops[i]["in0"])
        xs = [relu_input(rng, s) for s in shp]
        cases.append(("conv%d" % i, widths, i, i + 1 if pool else i, xs, False,
                      [conv_ref(x, ops[i], 0, pool)[0] for x in xs]))
    g = OracleGraph(prod)
    a, b = launches(prod)[0]
    cw = [22, 44, 100, 300]
    cx = [(rng.random((IN_H, w, 1), np.float32) - np.float32(0.5)).astype(np.float32) for w in cw]
    mids = [g.run_exact(x[None, :, :, 0][:, None], return_slots=True)[1][ops[a + 1]["out"]][0] for x in cx]
    cases.append(("conv12", cw, a, b, cx, False, [conv_ref(m, ops[a + 2], 0, (2, 2))[0] for m in mids]))
    gi = gru_ops(prod)[0]
    Ts = recurrence_lengths(16)
    sx = seq_inputs(rng, Ts, ops[gi]["cin"])
    gx_ref = [np.stack([R.linear(x[:, 0], *gru_w(ops[gi], d)[:2])[0] for d in range(2)]) for x in sx]
    cases.append(("gemm", [4 * T for T in Ts], gi, gi, sx, True, gx_ref))
    cases.append(("gru", [4 * T for T in Ts], gi, gi, sx, False, None))
    stats = {}
    for mode in ("exact", "relaxed", "reduced"):
        eng = make_engine(prod, mode)
        try:
            for name, w, first, last, xs, gx, refs in cases:
                got = eng.run_recognition_ops(w, first, last, xs, gx_only=gx)
                if refs is None:   # the recurrence: float64 of the whole sequence from the same inputs (no fp32 state feedback)
                    refs = [gru_f64(ops[gi], x) for x in xs]
                    got = [y[:, 0] for y in got]
                g_all = np.concatenate([np.ravel(y) for y in got])
                r_all = np.concatenate([np.ravel(r) for r in refs])
                stats[(name, mode)] = err_stats(g_all, r_all)
        finally:
            del eng
            release()
    lines = []
    for name in [c[0] for c in cases]:
        ex, rl, rd = stats[(name, "exact")], stats[(name, "relaxed")], stats[(name, "reduced")]
        f_rel = (rl[0] / max(ex[0], 1e-30), rl[1] / max(ex[1], 1e-30))
        f_red = (rd[0] / max(ex[0], 1e-30), rd[1] / max(ex[1], 1e-30))
        lines.append("%-7s exact rms %.3g max %.3g | relaxed x%.2f / x%.2f | reduced x%.1f / x%.1f" % (
            name, ex[0], ex[1], f_rel[0], f_rel[1], f_red[0], f_red[1]))
    print("\n" + "\n".join(lines))
    for name in [c[0] for c in cases]:
        ex, rl, rd = stats[(name, "exact")], stats[(name, "relaxed")], stats[(name, "reduced")]
        assert rl[0] <= RELAXED_FACTOR * ex[0] and rl[1] <= RELAXED_FACTOR * ex[1], (name, ex, rl)
        assert rd[0] > rl[0] and rd[1] > rl[1], (name, rl, rd)


def gru_f64(op, x):
    """Bidirectional GRU in float64 from the input sequence alone -> [T][2H]."""
    H = op["hidden"]
    out = []
    for d in range(2):
        wi, bi, wh, bh = (np.asarray(v, np.float64) for v in gru_w(op, d))
        xs = np.asarray(x[:, 0], np.float64)
        T = xs.shape[0]
        h = np.zeros(H)
        y = np.zeros((T, H))
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            gx = xs[t] @ wi + bi
            gh = h @ wh + bh
            r = 1 / (1 + np.exp(-(gx[:H] + gh[:H])))
            z = 1 / (1 + np.exp(-(gx[H:2 * H] + gh[H:2 * H])))
            n = np.tanh(gx[2 * H:] + r * gh[2 * H:])
            h = (1 - z) * n + z * h
            y[t] = h
        out.append(y)
    return np.concatenate(out, axis=1)


# ------------------------------------------------------------------ kernels that decline the split weights
@pytest.mark.parametrize("chans", [(32, 64, 96, 96, 96, 128), (32, 64, 64, 64, 64, 64)], ids=["cin96", "cout64"])
def test_declined_split_equals_the_oracle(chans):
    """Cin % 32 == 0 but Cin % 64 != 0 with Cout % 128 == 0, and Cout = 64: the model may carry split weights, the kernel
    declines them, and the relaxed engine's conv stack equals the oracle bit for bit."""
    buf = mf.build_recognition(n_classes=97, in_h=IN_H, seed=8, hidden=64, chans=chans).to_bytes()
    g = OracleGraph(buf)
    ops = g.ops
    spans = launches(buf)
    first = spans[1][0]
    last = spans[-6][1]   # the stack up to the average pool + TOSEQ launch
    assert ops[last + 1]["type"] == OP_AVGPOOL
    widths = RAGGED_WIDTHS
    slots = [g.run_exact((np.random.default_rng(w).random((1, 1, IN_H, w), np.float32) - 0.5).astype(np.float32),
                         return_slots=True)[1] for w in widths]
    eng = make_engine(buf, "relaxed")
    try:
        got = eng.run_recognition_ops(widths, first, last, [s[ops[first]["in0"]][0] for s in slots])
    finally:
        del eng
        release()
    for li, (y, s) in enumerate(zip(got, slots)):
        assert np.array_equal(y, s[ops[last]["out"]][0]), "%s: line %d (width %d) differs from the oracle" % (chans, li, widths[li])
