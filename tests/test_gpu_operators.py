"""Every executor operator on the GPU at its dispatch edges, against the oracle AND float64.

One-op graphs (a lift to C channels + the op where the op needs C > 1) run through Model.load_bytes(...).run.  Each
case asserts (a) bit equality with the C oracle, NaN positions included, and (b) the float64 bound of
tests/f64_ref.py.  The cases sit on both sides of the predicates that pick a kernel (kernels_nn.hip k::gemm, the
conv dispatch of model.cpp HipModel::run_device), so a kernel that is only reached by the synthetic models'
power-of-two shapes cannot be wrong unnoticed.

Run with:  python -m pytest -m gpu tests/test_gpu_operators.py
"""
import numpy as np
import pytest

import f64_ref as R
import models_util as M
from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, synth
from ocrs_amd import modelfile as mf
from oracle.nn import OracleGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _lift(rng, c, x_scale=None, relu=0):
    """Slot 0 (1 channel) -> slot 1 (c channels).  A 1x1 conv where the executor has a kernel for it (c == 1 or
    c % 4 == 0), else a Linear 1 -> c (the K = 1 tail of gemm_mfma)."""
    w = rng.standard_normal((1, 1, 1, c)).astype(np.float32) if x_scale is None else x_scale.reshape(1, 1, 1, c)
    b = rng.standard_normal(c).astype(np.float32) if x_scale is None else np.zeros(c, np.float32)
    if c == 1 or c % 4 == 0:
        return mf.Op(mf.OP_CONV, 0, 1, relu=relu, kh=1, kw=1, cin=1, cout=c, weights=(w, b))
    return mf.Op(mf.OP_LINEAR, 0, 1, relu=relu, cin=1, cout=c, weights=(w.reshape(1, c), b))


def _run(ops, n_slots, out_slot, x):
    """-> (gpu output in the oracle's layout, oracle slots).  NHWC outputs come back NCHW from the executor."""
    buf = mf.Graph(mf.KIND_RECOGNITION, [-1, 1, -1, -1], ops, n_slots, out_slot).to_bytes()
    got = Model.load_bytes(buf).run(x)
    _, slots = OracleGraph(buf).run_exact(x, return_slots=True)
    if got.ndim == 4:
        got = np.ascontiguousarray(got.transpose(0, 2, 3, 1))
    return got, slots


def _check(got, slots, out, ref, what):
    exp = slots[out]
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert np.array_equal(got, exp, equal_nan=True), "%s: differs from the oracle at %d elements" % (
        what, int((~((got == exp) | (np.isnan(got) & np.isnan(exp)))).sum()))
    if ref is not None:
        y64, bound = ref
        fin = np.isfinite(y64)
        R.check(np.where(fin, got, 0.0), (np.where(fin, y64, 0.0), np.where(fin, bound, 0.0)), what)


def _image(rng, n, h, w):
    return rng.standard_normal((n, 1, h, w)).astype(np.float32)


# ---------------------------------------------------------------- k::gemm
# (M, K, N, via): gemm_small (M <= 16384, 16 <= K <= 512, K % 4 == 0); gemm_tiled<64|128> (N >= 64, K % 16 == 0,
# M >= 256, past gemm_small); gemm_mfma<1|2|4> (N <= 32 | <= 64 | more) for everything else.
GEMM_CASES = [
    (16384, 16, 33, "conv"), (16385, 16, 33, "conv"), (16384, 512, 31, "conv"), (300, 516, 65, "conv"),
    (256, 528, 64, "conv"), (256, 528, 65, "conv"), (256, 528, 128, "conv"), (256, 528, 129, "conv"),
    (255, 528, 64, "conv"), (255, 528, 129, "conv"), (16385, 16, 64, "conv"),
    (77, 30, 1, "linear"), (77, 30, 31, "linear"), (77, 30, 33, "linear"), (77, 30, 63, "linear"),
    (77, 30, 65, "linear"), (300, 2, 33, "linear"), (130, 516, 7, "linear"),
]


@pytest.mark.parametrize("M,K,N,via", GEMM_CASES)
def test_gemm_dispatch_edges(M, K, N, via):
    rng = np.random.default_rng([M, K, N])
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    relu = (M + N) % 2
    if via == "conv":
        op = mf.Op(mf.OP_CONV, 1, 2, relu=relu, kh=1, kw=1, cin=K, cout=N, weights=(w.reshape(1, 1, K, N), b))
    else:
        op = mf.Op(mf.OP_LINEAR, 1, 2, relu=relu, cin=K, cout=N, weights=(w, b))
    got, s = _run([_lift(rng, K, relu=1), op], 3, 2, _image(rng, 1, 1, M))
    _check(got, s, 2, R.linear(s[1], w, b, relu), "gemm M %d K %d N %d" % (M, K, N))


@pytest.mark.parametrize("cin", [1, 2, 30])
def test_linear_k_tail_keeps_nan_in_its_row(cin):
    """K % 4 != 0: the A loads past column K-1 must not pick up the next row's NaN / Inf (gemm_mfma K tail)."""
    rng = np.random.default_rng(cin)
    x = _image(rng, 2, 3, 37)
    x[0, 0, 1, 5] = np.nan
    x[1, 0, 2, 36] = np.inf          # the last row of the tensor
    x[0, 0, 0, 0] = -np.inf
    w = rng.standard_normal((cin, 33)).astype(np.float32)
    b = rng.standard_normal(33).astype(np.float32)
    if cin == 1:
        ops, src, out, ns = [mf.Op(mf.OP_LINEAR, 0, 1, cin=1, cout=33, weights=(w, b))], 0, 1, 2
    else:
        ops, src, out, ns = [_lift(rng, cin), mf.Op(mf.OP_LINEAR, 1, 2, cin=cin, cout=33, weights=(w, b))], 1, 2, 3
    got, s = _run(ops, ns, out, x)
    bad_px = ~np.isfinite(x[:, 0]).reshape(-1)
    rows = got.reshape(-1, 33)
    assert np.isfinite(rows[~bad_px]).all(), "a non-finite input leaked into another row"
    _check(got, s, out, R.linear(s[src], w, b), "linear K %d with NaN / Inf" % cin)


@pytest.mark.parametrize("hid,inp", [(15, 30), (7, 5), (33, 64)])
def test_gru_odd_sizes(hid, inp):
    rng = np.random.default_rng([hid, inp])
    ws = []
    for _ in range(2):
        ws += [(rng.standard_normal((inp, 3 * hid)) / np.sqrt(inp)).astype(np.float32),
               (rng.standard_normal(3 * hid) * 0.5).astype(np.float32),
               (rng.standard_normal((hid, 3 * hid)) / np.sqrt(hid)).astype(np.float32),
               (rng.standard_normal(3 * hid) * 0.5).astype(np.float32)]
    ops = [_lift(rng, inp), mf.Op(mf.OP_TOSEQ, 1, 2), mf.Op(mf.OP_GRU, 2, 3, cin=inp, hidden=hid, weights=ws)]
    got, s = _run(ops, 4, 3, _image(rng, 3, 1, 17))
    _check(got, s, 3, R.gru_bidir(s[2], ws, got), "gru H %d I %d" % (hid, inp))


def test_convt_and_im2col_edges():
    rng = np.random.default_rng(9)
    for cin, cout, h, w in [(516, 8, 3, 5), (30, 12, 5, 3), (32, 40, 7, 9)]:   # K > 512; K % 4 != 0; NT 2
        wt = (rng.standard_normal((2, 2, cin, cout)) / np.sqrt(cin)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        got, s = _run([_lift(rng, cin), mf.Op(mf.OP_CONVT2, 1, 2, cin=cin, cout=cout, weights=(wt, b))], 3, 2,
                      _image(rng, 2, h, w))
        _check(got, s, 2, R.convt2x2(s[1], wt, b), "convt %d->%d" % (cin, cout))
    for cin, cout, h, w in [(32, 32, 8, 8), (64, 40, 5, 11), (32, 72, 15, 17)]:        # im2col with M < 256
        wt = (rng.standard_normal((3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        got, s = _run([_lift(rng, cin), mf.Op(mf.OP_CONV, 1, 2, relu=1, kh=3, kw=3, cin=cin, cout=cout, weights=(wt, b))],
                      3, 2, _image(rng, 1, h, w))
        _check(got, s, 2, R.conv(s[1], wt, b, 1), "im2col %d->%d %dx%d" % (cin, cout, h, w))


# ---------------------------------------------------------------- conv dispatch
@pytest.mark.parametrize("kh,kw,cin,cout", [(1, 1, 8, 1), (1, 1, 5, 1), (5, 5, 8, 8), (1, 3, 20, 4), (3, 1, 20, 12),
                                            (3, 3, 20, 8), (7, 1, 3, 4), (3, 3, 1, 16)])
def test_conv_dispatch(kh, kw, cin, cout):
    rng = np.random.default_rng([kh, kw, cin, cout])
    wt = (rng.standard_normal((kh, kw, cin, cout)) / np.sqrt(kh * kw * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    for h, w in [(1, 1), (3, 2), (13, 9)]:
        conv = mf.Op(mf.OP_CONV, 1, 2, relu=(h + cin) % 2, kh=kh, kw=kw, cin=cin, cout=cout, weights=(wt, b))
        ops = [_lift(rng, cin), conv]
        got, s = _run(ops, 3, 2, _image(rng, 2, h, w))
        _check(got, s, 2, R.conv(s[1], wt, b, conv.relu), "conv %dx%d %d->%d %dx%d" % (kh, kw, cin, cout, h, w))
        if cout == 1 and kh == 1:      # conv1x1_cout1 with the sigmoid fused into it
            got, s = _run(ops + [mf.Op(mf.OP_SIGMOID, 2, 3)], 4, 3, _image(rng, 2, h, w))
            y64 = R.conv(s[1], wt, b, conv.relu)
            _check(got, s, 3, R.sigmoid(s[2]), "conv1x1 + sigmoid")
            R.check(s[2], y64, "conv1x1 before the sigmoid")


def test_conv_unsupported_shape_is_refused():
    rng = np.random.default_rng(3)
    for kh, cin, cout in [(3, 20, 6), (1, 5, 6)]:
        ops = [_lift(rng, cin), mf.Op(mf.OP_CONV, 1, 2, kh=kh, kw=kh, cin=cin, cout=cout,
                                      weights=(np.zeros((kh, kh, cin, cout)), np.zeros(cout)))]
        m = Model.load_bytes(mf.Graph(mf.KIND_RECOGNITION, [-1, 1, -1, -1], ops, 3, 2).to_bytes())
        with pytest.raises(_lib.OcrsError) as e:
            m.run(_image(rng, 1, 4, 4))
        assert "unsupported conv shape" in str(e.value)


# ---------------------------------------------------------------- depthwise, concat, pools
def test_depthwise_vec4_vec1_and_fused_concat():
    rng = np.random.default_rng(4)
    for c in (8, 5):
        wt = rng.standard_normal((3, 3, c)).astype(np.float32)
        b = rng.standard_normal(c).astype(np.float32)
        got, s = _run([_lift(rng, c), mf.Op(mf.OP_DWCONV3, 1, 2, relu=1, kh=3, kw=3, cin=c, cout=c, weights=(wt, b))],
                      3, 2, _image(rng, 2, 7, 5))
        _check(got, s, 2, R.dwconv3x3(s[1], wt, b, 1), "dwconv3 c %d" % c)
    # PADCAT read directly by the depthwise conv (dwconv3x3_cat) when both channel counts are % 4, else the fallback
    for cs, cx in [(8, 4), (8, 3), (5, 4)]:
        for (h, ph), (w, pw) in [((6, 2), (5, 1)), ((2, 2), (6, 2)), ((9, 3), (7, 2))]:
            ct = cs + cx
            wt = rng.standard_normal((3, 3, ct)).astype(np.float32)
            b = rng.standard_normal(ct).astype(np.float32)
            ops = [_lift(rng, cs), _lift(rng, cx), mf.Op(mf.OP_MAXPOOL, 2, 3, kh=ph, kw=pw),
                   mf.Op(mf.OP_PADCAT, 1, 4, in1=3), mf.Op(mf.OP_DWCONV3, 4, 5, kh=3, kw=3, cin=ct, cout=ct, weights=(wt, b))]
            ops[1].out = 2
            got, s = _run(ops, 6, 5, _image(rng, 2, h, w))
            assert np.array_equal(s[4], R.padcat(s[1], s[3])[0])
            _check(got, s, 5, R.dwconv3x3(s[4], wt, b), "padcat+dwconv %d+%d %dx%d" % (cs, cx, h, w))


@pytest.mark.parametrize("op", [mf.OP_MAXPOOL, mf.OP_AVGPOOL])
def test_pools(op):
    rng = np.random.default_rng(op)
    h, w = 7, 5
    for kh, kw in [(2, 2), (2, 1), (1, 2), (3, 3), (4, 1), (h, 1)]:
        got, s = _run([_lift(rng, 12), mf.Op(op, 1, 2, kh=kh, kw=kw)], 3, 2, _image(rng, 2, h, w))
        ref = R.maxpool(s[1], kh, kw) if op == mf.OP_MAXPOOL else R.avgpool(s[1], kh, kw)
        _check(got, s, 2, ref, "pool %d %dx%d" % (op, kh, kw))


# ---------------------------------------------------------------- LogSoftmax, sigmoid
@pytest.mark.parametrize("c", [1, 2, 63, 64, 65, 638, 639])
def test_log_softmax_argmax(c):
    rng = np.random.default_rng(c)
    lift = _lift(rng, c)
    lift.weights[1] = np.linspace(-100, 10, c).astype(np.float32)[rng.permutation(c)]   # rows span more than 87
    for n, width in [(1, 67), (3, 43)]:       # 67 and 129 rows: not multiples of 64
        got, s = _run([lift, mf.Op(mf.OP_TOSEQ, 1, 2), mf.Op(mf.OP_LOGSOFTMAX, 2, 3)], 4, 3, _image(rng, n, 1, width))
        _check(got, s, 3, R.log_softmax(s[2]), "log_softmax C %d" % c)


def test_log_softmax_capacity_refusal():
    rng = np.random.default_rng(640)
    ops = [_lift(rng, 640), mf.Op(mf.OP_TOSEQ, 1, 2), mf.Op(mf.OP_LOGSOFTMAX, 2, 3)]
    m = Model.load_bytes(mf.Graph(mf.KIND_RECOGNITION, [-1, 1, -1, -1], ops, 4, 3).to_bytes())
    with pytest.raises(_lib.OcrsError) as e:
        m.run(_image(rng, 1, 1, 10))
    assert e.value.status_name == "CAPACITY", e.value


def _fp32_window(center, half):
    """Every fp32 within `half` steps of `center`."""
    c = np.array([center], np.float32).view(np.int32)[0]
    return (c + np.arange(-half, half + 1, dtype=np.int64)).astype(np.int32).view(np.float32)


def test_sigmoid_whole_range_bit_exact():
    rng = np.random.default_rng(13)
    parts = [np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32),
             np.arange(0, 1 << 20, dtype=np.int32).view(np.float32),                 # +0 and the subnormals up
             (np.arange(0, 1 << 20, dtype=np.int64) | 0x80000000).astype(np.uint32).view(np.float32)]
    for c in (1e-3, -1e-3, 1.0, -1.0, 87.0, -87.0, 88.0, -88.0):
        parts.append(_fp32_window(c, 1 << 16))
    special = np.concatenate(parts)
    x = rng.uniform(-90, 90, 4096 * 4096).astype(np.float32)
    x[:special.size] = special
    x = x.reshape(1, 1, 4096, 4096)
    got, s = _run([mf.Op(mf.OP_SIGMOID, 0, 1)], 2, 1, x)
    _check(got, s, 1, R.sigmoid(s[0]), "sigmoid")


# ---------------------------------------------------------------- the MFMA chain premise at the edges of fp32
def test_mfma_chain_subnormals_zeros_and_non_finite():
    """Subnormal operands, subnormal and underflowing products, +-0 biases with zero products, one row with Inf and
    one with NaN: the matrix-core GEMMs (gemm_small, gemm_tiled, gemm_mfma) equal the fmaf chain.  Pins that f32
    subnormals are kept (a build that flushes them fails here)."""
    rng = np.random.default_rng(21)
    for K, N, M, via in [(64, 64, 200, "conv"), (528, 64, 300, "conv"), (30, 33, 90, "linear")]:
        scale = (2.0 ** rng.integers(-140, -100, K)).astype(np.float32)          # subnormal .. tiny channels
        scale[::3] = 1.0
        w = (rng.standard_normal((K, N)) * 2.0 ** rng.integers(-40, 0, (K, N))).astype(np.float32)
        w[:, 0] = 0.0
        b = rng.standard_normal(N).astype(np.float32) * 1e-38
        b[1::2] = 0.0
        b[1::4] = -0.0
        x = _image(rng, 1, 1, M)
        x[0, 0, 0, :7] = 0.0
        x[0, 0, 0, 50] = np.inf
        x[0, 0, 0, 61] = np.nan
        if via == "conv":
            op = mf.Op(mf.OP_CONV, 1, 2, kh=1, kw=1, cin=K, cout=N, weights=(w.reshape(1, 1, K, N), b))
        else:
            op = mf.Op(mf.OP_LINEAR, 1, 2, cin=K, cout=N, weights=(w, b))
        got, s = _run([_lift(rng, K, x_scale=scale), op], 3, 2, x)
        assert (np.abs(s[1]) < R.MIN_NORMAL).any() and (s[1] != 0).any()
        _check(got, s, 2, R.linear(s[1], w, b), "MFMA chain K %d N %d" % (K, N))


# ---------------------------------------------------------------- isolation of non-finite pages and crops
def test_non_finite_page_and_crop_do_not_leak_into_the_batch():
    det = M.detection_model_bytes((160, 128), (8, 16, 32, 32))
    eng = OcrEngine(detection_model=Model.load_bytes(det), recognition_model=Model.load_bytes(M.recognition_model_bytes()))
    pages = [synth.synthetic_page(s, 192, 256, lines=6, columns=1).astype(np.float32) / 255.0 for s in range(4)]
    pages[2][40:80, 30:90] = np.nan
    pages[2][100:110, 10:200] = np.inf
    inps = [eng.prepare_input(ImageSource.from_tensor(p, DimOrder.Hwc)) for p in pages]
    batch = eng.detect_words_batch(inps)
    for i in (0, 1, 3):
        assert np.array_equal(batch[i], eng.detect_words(inps[i])), i

    # one line crop with a NaN band through it, recognised in a batch with the page's other lines
    lines = eng.find_text_lines(inps[0], eng.detect_words(inps[0]))
    assert len(lines) >= 3
    bad = pages[0].copy()
    bad[60:64, :] = np.nan
    binp = eng.prepare_input(ImageSource.from_tensor(bad, DimOrder.Hwc))
    batch = eng.recognize_text_batch([binp], [lines])[0]

    def norm(line):
        return None if line is None else [(c.char, tuple(c.rect)) for c in line._chars]
    for i, ln in enumerate(lines):
        assert norm(batch[i]) == norm(eng.recognize_text(binp, [ln])[0]), i


# ---------------------------------------------------------------- Model.run(timing=True)
@pytest.mark.parametrize("det_fuse", [1, 0])
def test_timed_run_prints_one_line_per_op_and_computes_the_same(det_fuse, capfd):
    """The print_timing branch of HipModel::run_device (model.cpp): an event behind every op, ops covered by a fused
    DoubleConv launch (det_fuse = 1) included, then one line per graph op in op order and a `total` line on the process's
    stdout.  The outputs equal those of an untimed run."""
    import ctypes
    dbuf = M.detection_model_bytes((160, 128), (8, 16, 32, 32))
    model = Model.load_bytes(dbuf)
    x = _image(np.random.default_rng(160), 1, 160, 128) * np.float32(0.25)
    libc = ctypes.CDLL(None)
    try:
        _lib.set_option("det_fuse", det_fuse)
        plain = model.run(x)
        libc.fflush(None)
        capfd.readouterr()
        timed = model.run(x, timing=True)
        libc.fflush(None)   # the table goes through C stdio
        out = capfd.readouterr().out
    finally:
        _lib.set_option("det_fuse", 1)
    assert np.array_equal(timed, plain, equal_nan=True)
    names = [mf.OP_NAMES[op["type"]] for op in OracleGraph(dbuf).ops]
    lines = out.splitlines()
    assert len(lines) == len(names) + 1, out
    for line, name in zip(lines, names):
        assert line.split()[0] == name and line.endswith("ms"), (line, name)
    assert lines[-1].split()[0] == "total" and lines[-1].endswith("ms"), lines[-1]
