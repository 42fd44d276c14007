"""The row-owning form of the exact 3x3 ragged conv (conv3x3_ragged_kernel<..., ROWS = 1>, an engine's "conv_rows").

conv_rows = 1: a block's four waves each own all four image rows of a 4 x 32 patch and 32 of its 128 columns; conv_rows = 2:
the same, and where the model allows (conv_rows.hpp) the accumulator of the image row above / below the image takes no MFMA in
the chunks of the ky = 0 / ky = 2 taps.  Every comparison here is bit for bit, NaN positions included: against the oracle's
slot (oracle.clib.conv2d [+ maxpool] on the launch's input) and against conv_rows = 0, launch by launch through
ocrs_engine_run_recognition_ops, and on whole requests through Case.check of the logits tests.

Run with:  python -m pytest tests -m gpu
"""
import gc
import threading

import numpy as np
import pytest

import models_util as M
from ocrs_amd import Model, OcrEngine, OcrsError, _lib, synth
from ocrs_amd import modelfile as mf
from oracle import clib
from oracle.nn import OracleGraph
from test_gpu_recognition_logits import PAGE_HW, Case, sweep_lines

pytestmark = pytest.mark.gpu
OP_CONV, OP_MAXPOOL = 0, 2
SETTINGS = (0, 1, 2)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()   # fail loudly: there is no CPU fallback to "pass" on


def graph(in_h, chans, seed=5):
    return mf.build_recognition(n_classes=97, in_h=in_h, seed=seed, hidden=64, chans=chans)


def row_convs(buf):
    """(first op, last op, conv op, fused pool or None, input height divisor, input width divisor) of every launch the
    row-owning kernel takes: a 3x3 conv with Cin % 32 == 0 and Cout % 128 == 0, with the 2x1 / 2x2 MaxPool that follows it."""
    ops = OracleGraph(buf).ops
    res, dh, dw = [], 1, 1
    for i, o in enumerate(ops):
        if o["type"] == OP_CONV and o["kh"] == 3 and o["cin"] % 32 == 0 and o["cout"] % 128 == 0:
            nxt = ops[i + 1]
            pool = (nxt["kh"], nxt["kw"]) if nxt["type"] == OP_MAXPOOL and nxt["kh"] == 2 and nxt["kw"] in (1, 2) else None
            res.append((i, i + 1 if pool else i, o, pool, dh, dw))
        if o["type"] == OP_MAXPOOL:
            dh, dw = dh * o["kh"], dw * o["kw"]
    return res


def oracle_launch(op, pool, x):
    y = clib.conv2d(np.ascontiguousarray(x[None]), op["w"][0].reshape(3, 3, op["cin"], op["cout"]), op["w"][1], op["relu"])
    return (clib.maxpool(y, *pool) if pool else y)[0]


def same_bits(a, b):
    """Equal bit for bit, except that any NaN equals any NaN (the matrix core and fmaf name their NaNs differently)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def check_launches(buf, in_h, widths, make_input, what, flats=(0, 1), only=None, engine=None):
    """Every row-owning launch of the model over lines of these model-input widths: each setting equals the oracle's slot and
    setting 0.  Returns the launches checked."""
    eng = engine or OcrEngine(recognition_model=Model.load_bytes(buf))
    n = 0
    try:
        for first, last, op, pool, dh, dw in row_convs(buf):
            if only is not None and first not in only:
                continue
            h = in_h // dh
            assert h % 4 == 0
            xs = [make_input((h, w // dw, op["cin"]), li) for li, w in enumerate(widths)]
            want = [oracle_launch(op, pool, x) for x in xs]
            for flat in flats:
                eng.set_option("conv_flat", flat)
                base = None
                for rows in SETTINGS:
                    eng.set_option("conv_rows", rows)
                    got = eng.run_recognition_ops(widths, first, last, xs)
                    for li, (g, e) in enumerate(zip(got, want)):
                        tag = "%s: conv op %d (%d->%d, H %d, pool %s) conv_flat %d conv_rows %d line %d (W %d)" % (
                            what, first, op["cin"], op["cout"], h, pool, flat, rows, li, xs[li].shape[1])
                        assert same_bits(g, e), tag + " differs from the oracle"
                        if base is not None:
                            assert same_bits(g, base[li]), tag + " differs from conv_rows 0"
                    base = got if rows == 0 else base
            n += 1
    finally:
        if engine is None:
            del eng
            gc.collect()
    return n


def normal(seed):
    def make(shape, li):
        return np.random.default_rng(seed + 1000 * li).standard_normal(shape).astype(np.float32)
    return make


# Model-input widths; conv3 .. conv6 see a quarter of them, conv2 of the wide model half.  At a quarter: 11 (the flat floor, three
# images in one 32-column patch, the group's second patch ragged), 31 / 32 / 33 around one patch, 65 (three patches, one
# column in the last), five images of 16 (two images per patch, 80 columns: the last patch half empty).
WIDTHS = [44, 44, 44, 124, 128, 132, 260] + [64] * 5
# at a half, under the 2 x 2 pool: odd widths 23 and 15 (the pool drops the odd column, the image pitch is rounded up to even:
# two and three images per patch), and 22 .. 130
WIDTHS_HALF = [46, 46, 30, 30, 30] + WIDTHS[2:7]
NARROW = [4, 20, 40, 40]   # 1, 5 and 10 columns at a quarter: below the flat floor, every image on its own


@pytest.mark.parametrize("in_h", [32, 64])
def test_widths_pools_and_column_blocks(in_h):
    """conv3 .. conv6 with Cout 128 and 256 (two column blocks), unpooled and under the 2 x 1 pool; in_h 32: H = 8 and 4 (a
    block that is top and bottom at once), in_h 64: H = 16 and 8 (middle blocks that skip nothing)."""
    buf = graph(in_h, (32, 64, 128, 256, 256, 128)).to_bytes()
    assert [(o["cin"], o["cout"], p, in_h // dh) for _, _, o, p, dh, _ in row_convs(buf)] == [
        (64, 128, None, in_h // 4), (128, 256, (2, 1), in_h // 4), (256, 256, None, in_h // 8), (256, 128, (2, 1), in_h // 8)]
    assert check_launches(buf, in_h, WIDTHS, normal(in_h), "widths") == 4
    assert check_launches(buf, in_h, NARROW, normal(7), "narrow", flats=(1,)) == 4


def test_two_by_two_pool():
    """conv2 as a 64 -> 128 conv under the 2 x 2 pool (conv1 has 64 channels: no conv1 + conv2 launch), H = 16, odd widths."""
    buf = graph(32, (64, 128, 128, 128, 128, 128)).to_bytes()
    convs = row_convs(buf)
    assert (convs[0][3], convs[0][4], convs[0][5]) == ((2, 2), 2, 2)
    assert check_launches(buf, 32, WIDTHS_HALF, normal(3), "2x2 pool", only=(convs[0][0],)) == 1


def inf_weight_model(tap, relu):
    g = graph(32, (32, 64, 128, 128, 128, 128))
    conv = [o for o in g.ops if o.type == OP_CONV][4]       # conv5: 128 -> 128 at H = 4, unpooled
    conv.weights[0].reshape(9, conv.cin, conv.cout)[tap, 5, 17] = np.inf
    conv.relu = relu
    return g.to_bytes()


@pytest.mark.parametrize("tap", [1, 7])
def test_inf_weight_keeps_every_tap(tap):
    """One Inf weight in a ky = 0 (ky = 2) tap: 0 x Inf = NaN in the accumulators of the first (last) image row, which the
    ReLU turns into +0 — a dropped tap would leave an ordinary number there.  The layer does not get the flag: setting 2 runs
    it without the skip."""
    buf = inf_weight_model(tap, 1)
    first, _, op, _, _, _ = row_convs(buf)[2]
    assert np.isinf(op["w"][0]).sum() == 1
    ref = oracle_launch(op, None, normal(11)((4, 33, 128), 0))
    assert not np.isnan(ref).any() and (ref[0 if tap == 1 else 3, :, 17] == 0).all() and (ref[:, :, 16] != 0).any(axis=1).all()
    assert check_launches(buf, 32, [132, 44, 44], normal(11), "Inf weight in tap %d" % tap, only=(first,)) == 1


def negative_zero_model():
    g = graph(32, (32, 64, 128, 128, 128, 128))
    conv = [o for o in g.ops if o.type == OP_CONV][4]
    conv.weights[0][:] = np.abs(conv.weights[0]) + np.float32(0.5)
    conv.weights[1][:] = np.float32(-0.0)
    conv.relu = 0
    return g.to_bytes()


def test_layers_without_relu():
    """What the flag's second condition is about, in the oracle: -0.0 biases, no ReLU, positive weights, inputs all -0.0 —
    every in-image tap adds a -0 product, every out-of-image tap (operand +0) a +0 one, which turns the spec's accumulator
    into +0 for good: -0 inside the image, +0 along its border, where dropping the out-of-image taps would leave -0.
    The ragged conv stack takes models whose every conv has its ReLU; a model with a ReLU-less conv (this one; an Inf weight
    whose NaN no ReLU removes) runs the per-group kernels, whatever conv_rows says — the same log-probs as the oracle, NaN
    positions included, at every setting."""
    buf = negative_zero_model()
    op = row_convs(buf)[2][2]
    ref = oracle_launch(op, None, np.full((4, 33, 128), -0.0, np.float32))
    inside = np.zeros((4, 33, 128), bool)
    inside[1:-1, 1:-1] = True
    assert op["relu"] == 0 and (ref == 0).all() and np.array_equal(np.signbit(ref), inside)
    inf_ref = oracle_launch(row_convs(inf_weight_model(1, 0))[2][2], None, normal(11)((4, 33, 128), 0))
    assert [bool(v) for v in np.isnan(inf_ref).any(axis=(1, 2))] == [True, False, False, False]
    page = synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40)
    for what, rbuf in (("-0.0 bias", buf), ("Inf weight, tap 1", inf_weight_model(1, 0)), ("Inf weight, tap 7", inf_weight_model(7, 0))):
        case = Case(rbuf, page)
        lines = sweep_lines(case)[::8]
        exp = case.oracle(lines)
        with pytest.raises(OcrsError, match="no ragged form"):
            case.gpu.run_recognition_ops([132], row_convs(rbuf)[2][0], row_convs(rbuf)[2][0], [np.zeros((4, 33, 128), np.float32)])
        for rows in SETTINGS:
            case.gpu.set_option("conv_rows", rows)
            case.check(lines, exp, "%s, no ReLU, conv_rows %d" % (what, rows))
        del case
        gc.collect()


def test_nan_activations_in_the_edge_rows():
    """NaN inputs in rows 0 and H - 1: the skipped taps never read them (they read the rows outside the image), every tap
    that does read them still runs."""
    def make(shape, li):
        x = normal(23)(shape, li)
        x[0, ::3, 1::7] = np.nan
        x[-1, 1::4, ::5] = np.nan
        return x
    buf = graph(32, (32, 64, 128, 128, 128, 128)).to_bytes()
    assert check_launches(buf, 32, [132, 44, 44, 64, 64], make, "NaN rows") == 4


@pytest.mark.parametrize("in_h", [32, 64])
def test_whole_requests_at_two_heights(in_h):
    """Requests through recognize_logits (Case.check of the logits tests) at every setting, given to the engine when it is made
    and changed while it lives."""
    case = Case(M.small_recognition_bytes(64, in_h, seed=21, chans=(32, 64, 128, 128, 128, 128)),
                synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40))
    lines = sweep_lines(case)[::4]
    exp = case.oracle(lines)
    for rows in SETTINGS:
        case.gpu.set_option("conv_rows", rows)
        assert case.gpu.get_option("conv_rows") == rows
        case.check(lines, exp, "in_h %d conv_rows %d" % (in_h, rows))
    assert OcrEngine(recognition_model=Model.load_bytes(case.rbuf)).get_option("conv_rows") == 2   # the default
    for field, stored in ((1, 1), (0, 0)):
        case.gpu = OcrEngine(recognition_model=Model.load_bytes(case.rbuf), options={"conv_rows": field})   # (the page stays: same device)
        assert case.gpu.get_option("conv_rows") == stored
        case.check(lines, exp, "in_h %d, engine made with conv_rows %d" % (in_h, field))


def test_settings_change_while_the_engine_serves():
    """The sweep lines of test_option_matrix_equals_oracle on the production model, one engine: a run at each setting, then
    one more while another thread keeps changing the setting — options are per engine and may change while it serves."""
    case = Case(M.recognition_model_bytes(), synth.synthetic_page(71, PAGE_HW[0], PAGE_HW[1], lines=40))
    lines = sweep_lines(case)
    exp = case.oracle(lines)
    for rows in SETTINGS:
        case.gpu.set_option("conv_rows", rows)
        case.check(lines, exp, "sweep, conv_rows %d" % rows)
    stop = threading.Event()

    def flip():
        i = 0
        while not stop.is_set():
            case.gpu.set_option("conv_rows", SETTINGS[i % 3])
            i += 1
    t = threading.Thread(target=flip)
    t.start()
    try:
        case.check(lines, exp, "sweep, conv_rows changing")
    finally:
        stop.set()
        t.join()
    with pytest.raises(Exception):
        case.gpu.set_option("conv_rows", 3)
