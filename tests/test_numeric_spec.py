"""The numeric spec against float64 (CPU; runs without a GPU).

Every fp32 GPU test compares the HIP path with the C oracle bit for bit.  These tests check the oracle itself against
an independent float64 definition of each operation (tests/f64_ref.py) within an elementwise error bound, so that
an oracle and kernels that agree on the wrong operation (a swapped gate, a padding off by one, a dropped term of a
polynomial) fail here.  One-op graphs (plus a 1x1 "lift" conv where the op needs C > 1) run through
OracleGraph.run_exact; the float64 op is applied to the oracle's own input slot.
"""
import numpy as np
import pytest

import f64_ref as R
import models_util as M
from ocrs_amd import modelfile as mf
from ocrs_amd import synth
from oracle import clib
from oracle import pipeline as OP
from oracle.nn import OracleGraph

RNG_SEED = 20261015


def _ulp_err(y, y64):
    return np.abs(np.asarray(y, np.float64) - y64) / R.ulp(y64)


# ---------------------------------------------------------------- transcendentals
def test_spec_exp_within_one_ulp():
    x = np.linspace(-87.0, 88.0, 8_000_001, dtype=np.float64).astype(np.float32)
    e = _ulp_err(clib.spec_exp(x), np.exp(x.astype(np.float64)))
    assert e.max() <= R.EXP_ULP, e.max()


def test_spec_log_within_three_ulp_on_sums():
    # LogSoftmax only takes the log of a sum of exponentials whose largest term is exp(0) = 1
    x = np.linspace(1.0, 1024.0, 8_000_001, dtype=np.float64).astype(np.float32)
    x = np.unique(np.concatenate([x, np.nextafter(np.float32(1.0), np.float32(2.0)) + np.arange(100000, dtype=np.float32) * np.float32(2 ** -23)]))
    y64 = np.log(x.astype(np.float64))
    y = clib.spec_log(x).astype(np.float64)
    assert y[x == 1.0][0] == 0.0
    nz = y64 > 0
    e = _ulp_err(y[nz], y64[nz])
    assert e.max() <= R.LOG_ULP, e.max()


def test_spec_sigmoid_within_three_ulp():
    x = np.linspace(-88.0, 88.0, 8_000_001, dtype=np.float64).astype(np.float32)
    x = np.concatenate([x, np.float32(np.arange(-2 ** 16, 2 ** 16) * 2.0 ** -24)])   # every fp32 step near 0 is not
    y = clib.sigmoid(x).astype(np.float64)                                             # needed: a dense window is
    y64, bound = R.sigmoid(x)
    normal = y64 >= R.MIN_NORMAL
    assert (_ulp_err(y[normal], y64[normal]) <= R.SIGMOID_ULP).all()
    assert (np.abs(y - y64)[~normal] <= R.MIN_NORMAL).all()
    R.check(y, (y64, bound), "sigmoid")


def test_spec_tanh_absolute_error():
    x = np.linspace(-30.0, 30.0, 8_000_001, dtype=np.float64).astype(np.float32)
    y = clib.spec_tanh(x).astype(np.float64)
    err = np.abs(y - np.tanh(x.astype(np.float64)))
    assert err.max() <= R.TANH_ABS, err.max()


def test_spec_transcendentals_special_values():
    """NaN in, NaN out; the exponent clamp at [-87, 88] for +-Inf and beyond; tanh's saturation."""
    f = np.float32
    sp = np.array([np.nan, np.inf, -np.inf, 100.0, -100.0], f)
    ex = clib.spec_exp(sp)
    assert np.isnan(ex[0])
    assert ex[1] == ex[3] == clib.spec_exp(np.array([88.0], f))[0] and np.isfinite(ex[1])
    assert ex[2] == ex[4] == clib.spec_exp(np.array([-87.0], f))[0] and ex[2] > 0
    sg = clib.sigmoid(sp)
    assert np.isnan(sg[0]) and sg[1] == sg[3] == 1.0
    assert sg[2] == sg[4] == clib.sigmoid(np.array([-88.0], f))[0] and 0 < sg[2] < R.MIN_NORMAL
    th = clib.spec_tanh(sp)
    assert np.isnan(th[0]) and th[1] == th[3] == 1.0 and th[2] == th[4] == -1.0


def test_spec_tanh_small_argument_behaviour_is_pinned():
    """tanh = (e^2x - 1) / (e^2x + 1) cancels for small |x|: the ABSOLUTE error stays below TANH_ABS (all the GRU
    needs), the relative error does not.  Pinned as it is today: a cancellation-free form would
    change bits on every model."""
    f = np.float32
    t = clib.spec_tanh(np.array([1e-8, -1e-8, 1e-6, 3e-6, 1e-4], f)).astype(np.float64)
    assert t[0] == 0.0 and t[1] == 0.0                       # tanh(+-1e-8) flushes to 0
    assert 0.005 < t[2] / 1e-6 - 1 < 0.02                      # tanh(1e-6) is ~1.3 % high
    assert abs(t[3] - np.tanh(np.float64(f(3e-6)))) > 1000 * R.ulp(3e-6)   # tens of thousands of ulp near 3e-6
    assert np.all(np.abs(t - np.tanh(np.array([1e-8, -1e-8, 1e-6, 3e-6, 1e-4], f).astype(np.float64))) <= R.TANH_ABS)


# ---------------------------------------------------------------- one-op graphs through the oracle
def _lift(rng, c, kind):
    """1x1 conv from the 1-channel image to c channels: the op under test sees inputs of the given kind."""
    w = rng.standard_normal((1, 1, 1, c)).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    relu = 0
    if kind == "sparse":
        relu = 1
    elif kind == "range":        # channel scales 1e-20 .. 1e20
        w = (10.0 ** rng.uniform(-20, 20, (1, 1, 1, c))).astype(np.float32)
        b = np.zeros(c, np.float32)
    return mf.Op(mf.OP_CONV, 0, 1, relu=relu, kh=1, kw=1, cin=1, cout=c, weights=(w, b))


def _image(rng, n, h, w, kind):
    if kind == "zeros":
        return np.zeros((n, 1, h, w), np.float32)
    return rng.standard_normal((n, 1, h, w)).astype(np.float32)


def _run(ops, n_slots, out_slot, x):
    buf = mf.Graph(mf.KIND_RECOGNITION, [-1, 1, -1, -1], ops, n_slots, out_slot).to_bytes()   # no output transpose
    _, slots = OracleGraph(buf).run_exact(x, return_slots=True)
    return slots


KINDS = ["normal", "sparse", "zeros", "range"]
CONV_KERNELS = [(1, 1), (3, 3), (5, 5), (1, 3), (3, 1), (7, 1)]
IMAGES = [(1, 1), (1, 9), (6, 1), (2, 3), (9, 7)]     # 1x1, 1xW, Hx1, smaller than most kernels, general


@pytest.mark.parametrize("kh,kw", CONV_KERNELS)
def test_oracle_conv_against_float64(kh, kw):
    rng = np.random.default_rng([RNG_SEED, kh, kw])
    i = 0
    for cin in (1, 3, 20, 32, 64):
        for h, w in IMAGES:
            kind = KINDS[i % len(KINDS)]
            i += 1
            cout = int(rng.choice([1, 4, 8, 12]))
            wt = (rng.standard_normal((kh, kw, cin, cout)) / np.sqrt(kh * kw * cin)).astype(np.float32)
            b = rng.standard_normal(cout).astype(np.float32)
            relu = i % 2
            if cin == 1:
                ops = [mf.Op(mf.OP_CONV, 0, 1, relu=relu, kh=kh, kw=kw, cin=1, cout=cout, weights=(wt, b))]
                src, out, ns = 0, 1, 2
            else:
                ops = [_lift(rng, cin, kind),
                       mf.Op(mf.OP_CONV, 1, 2, relu=relu, kh=kh, kw=kw, cin=cin, cout=cout, weights=(wt, b))]
                src, out, ns = 1, 2, 3
            s = _run(ops, ns, out, _image(rng, 2, h, w, kind))
            R.check(s[out], R.conv(s[src], wt, b, relu), "conv %dx%d cin %d image %dx%d %s" % (kh, kw, cin, h, w, kind))


def test_oracle_depthwise_and_convt_against_float64():
    rng = np.random.default_rng([RNG_SEED, 1])
    for j, (c, h, w) in enumerate([(1, 1, 1), (5, 1, 7), (8, 6, 1), (20, 3, 5), (32, 9, 4)]):
        kind = KINDS[j % len(KINDS)]
        wt = rng.standard_normal((3, 3, c)).astype(np.float32)
        b = rng.standard_normal(c).astype(np.float32)
        s = _run([_lift(rng, c, kind), mf.Op(mf.OP_DWCONV3, 1, 2, relu=j % 2, kh=3, kw=3, cin=c, cout=c, weights=(wt, b))],
                 3, 2, _image(rng, 2, h, w, kind))
        R.check(s[2], R.dwconv3x3(s[1], wt, b, j % 2), "dwconv3 c %d %dx%d" % (c, h, w))
    for j, (cin, cout, h, w) in enumerate([(1, 4, 1, 1), (3, 8, 3, 5), (20, 12, 7, 3), (64, 32, 5, 5)]):
        kind = KINDS[j % len(KINDS)]
        wt = (rng.standard_normal((2, 2, cin, cout)) / np.sqrt(cin)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        s = _run([_lift(rng, cin, kind), mf.Op(mf.OP_CONVT2, 1, 2, cin=cin, cout=cout, weights=(wt, b))], 3, 2,
                 _image(rng, 2, h, w, kind))
        R.check(s[2], R.convt2x2(s[1], wt, b), "convt %d->%d %dx%d" % (cin, cout, h, w))


@pytest.mark.parametrize("op", [mf.OP_MAXPOOL, mf.OP_AVGPOOL])
def test_oracle_pools_against_float64(op):
    rng = np.random.default_rng([RNG_SEED, 2, op])
    h, w = 7, 5
    for kh, kw in [(2, 2), (2, 1), (1, 2), (3, 3), (4, 1), (h, 1)]:
        for kind in ("normal", "range"):
            s = _run([_lift(rng, 3, kind), mf.Op(op, 1, 2, kh=kh, kw=kw)], 3, 2, _image(rng, 2, h, w, kind))
            ref = R.maxpool(s[1], kh, kw) if op == mf.OP_MAXPOOL else R.avgpool(s[1], kh, kw)
            R.check(s[2], ref, "pool %d %dx%d" % (op, kh, kw))
            if op == mf.OP_MAXPOOL:
                assert np.array_equal(s[2], ref[0])


def test_oracle_padcat_against_float64():
    """Size differences 0, 1 and 3 on each axis: the skip input at full size, the other input max-pooled down."""
    rng = np.random.default_rng([RNG_SEED, 3])
    per_axis = {0: (5, 1), 1: (2, 2), 3: (6, 2)}          # difference -> (size, pool window)
    for dy, (h, ph) in per_axis.items():
        for dx, (w, pw) in per_axis.items():
            ops = [_lift(rng, 3, "normal"),
                   mf.Op(mf.OP_CONV, 0, 2, kh=1, kw=1, cin=1, cout=5,
                         weights=(rng.standard_normal((1, 1, 1, 5)), rng.standard_normal(5))),
                   mf.Op(mf.OP_MAXPOOL, 2, 3, kh=ph, kw=pw),
                   mf.Op(mf.OP_PADCAT, 1, 4, in1=3)]
            s = _run(ops, 5, 4, _image(rng, 2, h, w, "normal"))
            assert (h - s[3].shape[1], w - s[3].shape[2]) == (dy, dx)
            y64, _ = R.padcat(s[1], s[3])
            assert np.array_equal(s[4], y64), (dy, dx)


def test_oracle_sigmoid_and_toseq_against_float64():
    rng = np.random.default_rng([RNG_SEED, 4])
    x = (rng.standard_normal((2, 1, 1, 33)) * 30).astype(np.float32)
    ops = [_lift(rng, 6, "normal"), mf.Op(mf.OP_SIGMOID, 1, 2), mf.Op(mf.OP_TOSEQ, 2, 3)]
    s = _run(ops, 4, 3, x)
    R.check(s[2], R.sigmoid(s[1]), "sigmoid")
    assert np.array_equal(s[3], R.to_seq(s[2])[0])


def _gru_ops(rng, cin, hid, kind):
    ws = []
    for _ in range(2):
        ws += [(rng.standard_normal((cin, 3 * hid)) / np.sqrt(cin)).astype(np.float32),
               (rng.standard_normal(3 * hid) * 0.5).astype(np.float32),
               (rng.standard_normal((hid, 3 * hid)) / np.sqrt(hid)).astype(np.float32),
               (rng.standard_normal(3 * hid) * 0.5).astype(np.float32)]
    ops = [_lift(rng, cin, kind), mf.Op(mf.OP_TOSEQ, 1, 2), mf.Op(mf.OP_GRU, 2, 3, cin=cin, hidden=hid, weights=ws)]
    return ops, ws


@pytest.mark.parametrize("hid", [1, 7, 15, 32, 33, 64])
def test_oracle_gru_against_float64_step_by_step(hid):
    rng = np.random.default_rng([RNG_SEED, 5, hid])
    i = 0
    for T in (1, 2, 17):
        for N in (1, 3):
            cin = (1, 5, 30, 64)[i % 4]
            kind = ("normal", "sparse", "zeros")[i % 3]
            i += 1
            ops, ws = _gru_ops(rng, cin, hid, kind)
            s = _run(ops, 4, 3, _image(rng, N, 1, T, kind))
            assert s[3].shape == (T, N, 2 * hid)
            R.check(s[3], R.gru_bidir(s[2], ws, s[3]), "gru H %d T %d N %d I %d" % (hid, T, N, cin))


@pytest.mark.parametrize("c", [1, 2, 31, 97, 639])
def test_oracle_log_softmax_against_float64(c):
    rng = np.random.default_rng([RNG_SEED, 6, c])
    # lift biases spread over [-120, 10]: rows span more than 87, so some exp terms underflow (clamped at -87)
    w = rng.standard_normal((1, 1, 1, c)).astype(np.float32)
    b = np.linspace(-120, 10, c).astype(np.float32)[rng.permutation(c)]
    for lift_w, lift_b in ((w, b), (w * 0.01, np.zeros(c, np.float32)), (np.zeros_like(w), np.round(b / 20))):
        ops = [mf.Op(mf.OP_CONV, 0, 1, kh=1, kw=1, cin=1, cout=c, weights=(lift_w, lift_b)),
               mf.Op(mf.OP_LOGSOFTMAX, 1, 2)]
        s = _run(ops, 3, 2, _image(rng, 3, 2, 5, "normal"))
        R.check(s[2], R.log_softmax(s[1]), "log_softmax C %d" % c)


def test_oracle_ctc_greedy_against_definition():
    rng = np.random.default_rng([RNG_SEED, 7])
    # ties: the first maximum wins; a label repeated across a blank is emitted twice, without one it merges
    seq = np.full((8, 5), -5.0, np.float32)
    for t, best in enumerate([2, 2, 0, 2, 3, 3, 1, 0]):
        seq[t, best] = -0.1
    seq[4, 4] = -0.1         # tie with 3 at t = 4: 3 wins
    seq[7, 0] = seq[7, 1] = -0.2   # tie of blank and 1: blank wins
    got = clib.ctc_greedy(seq)
    assert got == R.ctc_greedy(seq) == [(2, 0), (2, 3), (3, 4), (1, 6)]
    for _ in range(50):
        T, C = int(rng.integers(1, 40)), int(rng.integers(1, 12))
        m = np.round(rng.standard_normal((T, C)), 1).astype(np.float32)    # coarse values: many exact ties
        assert clib.ctc_greedy(m) == R.ctc_greedy(m)


def test_oracle_linear_against_float64():
    """Linear over the last axis for K % 4 != 0 and with the op's relu flag (applied as the executor's GEMM does)."""
    rng = np.random.default_rng([RNG_SEED, 8])
    for j, (cin, cout) in enumerate([(1, 33), (2, 7), (30, 1), (64, 65)]):
        for relu in (0, 1):
            w = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
            b = rng.standard_normal(cout).astype(np.float32)
            lin = mf.Op(mf.OP_LINEAR, 1, 2, relu=relu, cin=cin, cout=cout, weights=(w, b))
            s = _run([_lift(rng, cin, KINDS[j]), lin], 3, 2, _image(rng, 2, 3, 5, KINDS[j]))
            R.check(s[2], R.linear(s[1], w, b, relu), "linear %d->%d relu %d" % (cin, cout, relu))


# ---------------------------------------------------------------- whole models, op by op
def _rec_input(in_h, width, seed):
    """Two synthetic line crops of height in_h in a row of `width` padded with BLACK_VALUE (-0.5), the second crop
    repeated to the right so that long rows carry text beyond 256 px."""
    crops = synth.synthetic_line_crops(seed, n=2)[:, ::64 // in_h, ::64 // in_h]
    x = np.full((2, 1, in_h, width), -0.5, np.float32)
    cw = crops.shape[2]
    for i in range(2):
        for x0 in range(0, width if i else min(width, cw), cw):
            w = min(cw, width - x0)
            x[i, 0, :, x0:x0 + w] = crops[i, :, :w]
    return x


@pytest.mark.parametrize("width", [50, 300, 2400])
def test_production_recognition_model_within_float64_bounds(width):
    """The production CRNN (H 64, K = 1152 convs, hidden 256, 97 classes) at T = 12, 75 and 600: every op of the
    oracle's run within its float64 bound, on its own fp32 inputs."""
    R.check_graph(M.recognition_model_bytes(), _rec_input(64, width, 3), "recognition W %d" % width)


@pytest.mark.parametrize("hidden,in_h,chans", [(32, 64, (32, 64, 64, 64, 64, 64)), (64, 64, (32, 64, 64, 64, 64, 64)),
                                               (128, 64, (32, 64, 64, 64, 64, 64)),
                                               (64, 32, (32, 64, 64, 64, 64, 64))])
def test_small_recognition_models_within_float64_bounds(hidden, in_h, chans):
    buf = M.small_recognition_bytes(hidden, in_h, chans=chans)
    R.check_graph(buf, _rec_input(in_h, 450, 4), "recognition hidden %d H %d" % (hidden, in_h))


@pytest.mark.parametrize("in_hw,depths", [((800, 600), (8, 16, 32, 32, 64, 128, 256)), ((96, 64), (8, 16, 32, 32))])
def test_detection_model_within_float64_bounds(in_hw, depths):
    """The U-Net (depthwise DoubleConvs, pools, ConvT, pad-and-concat with odd sizes, sigmoid) on a synthetic page."""
    buf = M.detection_model_bytes(in_hw, depths)
    px = synth.synthetic_page(6, in_hw[0], in_hw[1], lines=max(2, in_hw[0] // 40))
    page = OP.prepare_image(OP.ImageSource.from_tensor(px, "hwc"))
    R.check_graph(buf, page[None], "detection %dx%d" % in_hw)


def test_graph_walk_fails_on_an_op_without_a_definition():
    """An op type the float64 reference does not define fails the walk instead of being skipped."""
    class _Op(dict):
        pass
    with pytest.raises(AssertionError, match="no float64 definition"):
        R._op_ref(_Op(type=11, in0=0, out=1, w=[], kh=0, kw=0, cin=0, cout=0, hidden=0, relu=0), {0: np.zeros(1)})


# ------------------------------------------------------------------ premises of the split-contraction probes
def test_split_probe_premises():
    """The exact probes of tests/test_gpu_numerics_split.py: every operand's bf16 planes (numpy round-to-nearest-even of the
    running residual) are the documented ones, the kept plane products of each mode add up to the stated result, every
    partial sum of them is exact in fp32, and relaxed equals the true product.  (Each probe output holds one product, so its
    partial sums are those of the kept plane products: non-negative half-integers whose total is below 2^24 — a partial sum
    in any order is then a half-integer in [0, total], which fp32 holds exactly.)"""
    planes = {257.0: (256.0, 1.0, 0.0), 1.0: (1.0, 0.0, 0.0), 65664.5: (65536.0, 128.0, 0.5)}
    for v, want in planes.items():
        got = tuple(float(p) for p in R.bf16_planes(np.float32(v)))
        assert got == want, (v, got, want)
        assert sum(got) == v
    assert float(R.bf16_rne(np.float32(128.5))) == 128.0          # the tie goes to the even 128, not 129
    for a, w, relaxed, reduced in R.SPLIT_PROBES:
        for np_, want in ((3, relaxed), (2, reduced)):
            total, kept = R.split_probe_value(a, w, np_)
            assert total == want, (a, w, np_, total, want)
            assert all(k >= 0 and 2 * k == int(2 * k) for k in kept), kept
            assert sum(kept) < 2 ** 24
        assert relaxed == float(np.float64(a) * np.float64(w)) and relaxed != reduced
        assert np.float32(relaxed) == relaxed and np.float32(reduced) == reduced


def test_split_bounds_cover_the_dropped_terms():
    """split_bound is at least the documented dropped-term fraction of |a w| and grows with the number of additions."""
    mag = np.array([1.0, 100.0])
    for np_ in (3, 2):
        b = R.split_bound(mag, 0.0, 64, np_)
        assert np.all(b >= R.SPLIT_DROP[np_] * mag)
        assert np.all(R.split_bound(mag, 0.0, 1152, np_) > b)
    assert R.SPLIT_DROP[2] > 100 * R.SPLIT_DROP[3]
