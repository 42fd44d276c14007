"""Float64 definitions of the graph ops and elementwise error bounds for their fp32 evaluation.

An independent yardstick for the C oracle (oracle/csrc/ocrs_oracle.c) and, through it, for the HIP kernels that
match the oracle bit for bit.  Each function is written from the ONNX / PyTorch operator definition in numpy
float64, not from the oracle's loops, and returns (y64, bound): the exact value and a per-element bound that any
fp32 evaluation in the numeric spec of DESIGN.md §4 must stay within, |y - y64| <= bound.

Bounds (u = 2^-24, gamma(n) = n u / (1 - n u)):
  * contractions (conv, depthwise, ConvT, Linear, GRU projections): a chain acc = b; acc = fmaf(a_k, w_k, acc) of K
    terms rounds K times, so |y - y64| <= gamma(K + 1) (|b| + sum_k |w_k x_k|), plus K * 2^-150 for products that
    fall below the normal range (Higham, Accuracy and Stability of Numerical Algorithms, §3.1 and §2.1);
  * average pool: the same bound with the 1 / (kh kw) scale (sum of K terms, the rounded reciprocal, the product);
  * max pool, pad-and-concat, the to-sequence reshape: exact;
  * exp, log, sigmoid, tanh: the spec polynomials' bounds below, measured over dense grids of their domains
    (tests/test_numeric_spec.py asserts them) with at most 1.5x headroom;
  * LogSoftmax and the GRU cell: propagated from the above (see those functions).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -150     # half the smallest subnormal: the underflow error of one fmaf
MIN_NORMAL = 2.0 ** -126

# Error bounds of the spec transcendentals.  Measured maxima on 4 M-point grids:
# exp 0.91 ulp on [-87, 88]; log 2.75 ulp on [1, 1024]; sigmoid 2.46 ulp on [-88, 88] where the value is normal;
# tanh 1.34e-7 absolute on [-30, 30].
EXP_ULP = 1.0
LOG_ULP = 3.0
SIGMOID_ULP = 3.0
TANH_ABS = 1.5e-7


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def ulp(v):
    """fp32 unit in the last place of float64 values (the subnormal spacing below 2^-126)."""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return 2.0 ** (np.maximum(e, -126) - 23)


def _f64(a):
    return np.asarray(a, np.float64)


def _relu(y, relu):
    return np.maximum(y, 0.0) if relu else y


# ---------------------------------------------------------------- contractions
def conv(x, w, b, relu=0):
    """ONNX Conv, stride 1, 'same' zero padding (kh // 2, kw // 2) for odd kh, kw.  x NHWC, w [KH][KW][Cin][Cout]."""
    x, w, b = _f64(x), _f64(w), _f64(b)
    kh, kw, cin, cout = w.shape
    n, h, wd, c = x.shape
    assert c == cin and kh % 2 == 1 and kw % 2 == 1
    xp = np.zeros((n, h + kh - 1, wd + kw - 1, cin))
    xp[:, kh // 2:kh // 2 + h, kw // 2:kw // 2 + wd] = x
    y = np.broadcast_to(b, (n, h, wd, cout)).copy()
    mag = np.broadcast_to(np.abs(b), (n, h, wd, cout)).copy()
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, ky:ky + h, kx:kx + wd]
            y += win @ w[ky, kx]
            mag += np.abs(win) @ np.abs(w[ky, kx])
    k = kh * kw * cin
    return _relu(y, relu), gamma(k + 1) * mag + k * TINY


def dwconv3x3(x, w, b, relu=0):
    """Depthwise (group = channel) 3x3 convolution, pad 1.  w [3][3][C]."""
    x, w, b = _f64(x), _f64(w), _f64(b)
    n, h, wd, c = x.shape
    xp = np.zeros((n, h + 2, wd + 2, c))
    xp[:, 1:h + 1, 1:wd + 1] = x
    y = np.broadcast_to(b, x.shape).copy()
    mag = np.broadcast_to(np.abs(b), x.shape).copy()
    for ky in range(3):
        for kx in range(3):
            win = xp[:, ky:ky + h, kx:kx + wd]
            y += win * w[ky, kx]
            mag += np.abs(win * w[ky, kx])
    return _relu(y, relu), gamma(10) * mag + 9 * TINY


def convt2x2(x, w, b):
    """ConvTranspose 2x2, stride 2 (no overlap: output (2i + dy, 2j + dx) = b + sum_ci x[i, j, ci] w[dy, dx, ci])."""
    x, w, b = _f64(x), _f64(w), _f64(b)
    n, h, wd, cin = x.shape
    cout = w.shape[3]
    y = np.empty((n, 2 * h, 2 * wd, cout))
    mag = np.empty_like(y)
    for dy in range(2):
        for dx in range(2):
            y[:, dy::2, dx::2] = x @ w[dy, dx] + b
            mag[:, dy::2, dx::2] = np.abs(x) @ np.abs(w[dy, dx]) + np.abs(b)
    return y, gamma(cin + 1) * mag + cin * TINY


def linear(x, w, b, relu=0):
    """y = x W + b over the last axis.  w [K][O]."""
    x, w, b = _f64(x), _f64(w), _f64(b)
    k = w.shape[0]
    return _relu(x @ w + b, relu), gamma(k + 1) * (np.abs(x) @ np.abs(w) + np.abs(b)) + k * TINY


# ---------------------------------------------------------------- pools, layout
def _windows(x, kh, kw):
    n, h, wd, c = x.shape
    oh, ow = h // kh, wd // kw
    return x[:, :oh * kh, :ow * kw].reshape(n, oh, kh, ow, kw, c)


def maxpool(x, kh, kw):
    """MaxPool, kernel = stride, floor (rows / columns the window does not reach are dropped).  Exact."""
    y = _windows(_f64(x), kh, kw).max(axis=(2, 4))
    return y, np.zeros_like(y)


def avgpool(x, kh, kw):
    """AveragePool, kernel = stride, floor.  Bound: gamma(K + 1) * mean |x| (sum, rounded 1/K, product)."""
    win = _windows(_f64(x), kh, kw)
    k = kh * kw
    return win.mean(axis=(2, 4)), gamma(k + 1) * np.abs(win).mean(axis=(2, 4)) + TINY


def padcat(skip, up):
    """Zero-pad `up` to the spatial size of `skip` (before = d // 2, after = d - d // 2 per axis, as PyTorch's
    F.pad(x, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2]) in the U-Net's Up block) and concatenate [skip, up]
    along channels.  Exact."""
    skip, up = _f64(skip), _f64(up)
    n, sh, sw, _ = skip.shape
    _, h, w, cx = up.shape
    dy, dx = sh - h, sw - w
    pad = np.zeros((n, sh, sw, cx))
    pad[:, dy // 2:dy // 2 + h, dx // 2:dx // 2 + w] = up
    y = np.concatenate([skip, pad], axis=3)
    return y, np.zeros_like(y)


def to_seq(x):
    """[N, 1, W, C] (NHWC, height 1) -> [T = W, N, C].  Exact."""
    x = _f64(x)
    assert x.shape[1] == 1
    y = np.ascontiguousarray(x[:, 0].transpose(1, 0, 2))
    return y, np.zeros_like(y)


# ---------------------------------------------------------------- elementwise transcendentals
def _sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def sigmoid(x):
    """1 / (1 + e^-x).  Bound: SIGMOID_ULP ulp where the value is normal, one smallest-normal below (the spec clamps
    its exponent to [-87, 88], so sigmoid(x < -88) is ~6e-39, not the true subnormal or zero)."""
    y = _sigmoid64(_f64(x))
    return y, np.where(y >= MIN_NORMAL, SIGMOID_ULP * ulp(y), MIN_NORMAL)


def tanh(x):
    x = _f64(x)
    return np.tanh(x), np.full(x.shape, TANH_ABS)


# ---------------------------------------------------------------- LogSoftmax
def log_softmax(x):
    """LogSoftmax over the last axis, y_j = x_j - (m + log sum_c exp(x_c - m)).

    Bound, per row, for the spec's evaluation order (m = max; s = sum_c exp(x_c - m) sequentially from 0;
    lse = m + log(s); y_j = x_j - lse):
      * the rounded difference x_c - m is off by at most u |x_c - m|, a relative error of that size (and a little
        more) in its exponential; the exp polynomial adds EXP_ULP ulp (<= 2^-23 EXP_ULP relative); arguments below
        -87 are clamped, so their term is up to 2^-125 instead of ~0;
      * the sum of C terms rounds C - 1 times: gamma(C - 1) relative;
      * so s = s64 (1 + e_s) + C 2^-125 with e_s bounded below, and log(s) = log(s64) + e_s' with s >= 1;
      * the log polynomial adds LOG_ULP ulp of log(s); m + log(s) and x_j - lse round once each."""
    x = _f64(x)
    m = x.max(axis=-1, keepdims=True)
    d = x - m
    s64 = np.exp(d).sum(axis=-1, keepdims=True)
    L = np.log(s64)
    y = d - L
    c = x.shape[-1]
    e_arg = 1.01 * U * np.abs(d).max(axis=-1, keepdims=True)
    e_s = gamma(c - 1) + e_arg + EXP_ULP * 2.0 ** -23 + c * 2.0 ** -125
    e_s = 1.01 * e_s   # log(1 + e) <= e, and the products of these small terms
    lse = m + L
    bound = e_s + LOG_ULP * ulp(L) + U * np.abs(lse) + U * np.abs(y) + U * U * np.abs(x)
    return y, np.broadcast_to(bound, y.shape).copy()


# ---------------------------------------------------------------- relaxed / reduced numerics
# A bf16-split contraction (split_mfma.hpp, kernels_gru_split.hip) cuts both operands of every product into NP bf16 planes by
# round-to-nearest of the running residual, x = hi + mid + lo, and sums the kept plane products in fp32 in the matrix core's
# order.  Per product a w:
#   * the dropped plane products are at most SPLIT_DROP[NP] |a w| (NP 3 keeps hh hm mh mm hl lh: <= 2^-23; NP 2 keeps hh hm mh:
#     <= 1.5 * 2^-15), and the kept ones add up, in magnitude, to at most (1 + 2^-9 + 2^-8 + 2^-16)^2 |a w| < SPLIT_MAG |a w|
#     (|hi| <= (1 + 2^-9) |x|, |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|);
#   * each kept plane product is exact in fp32 (8 x 8 significant bits);
#   * the bias and the SPLIT_TERMS[NP] K partial products are summed in an unspecified order: any order of n additions
#     rounds at most n times, so the sum is within gamma(n) of the sum of their magnitudes (Higham §4.2, order-free form);
#   * partial products below the normal range may be flushed: one 2^-126 per addition.
SPLIT_DROP = {3: 2.0 ** -23, 2: 1.5 * 2.0 ** -15}
SPLIT_TERMS = {3: 6, 2: 3}
SPLIT_MAG = 1.02


def split_bound(mag, bias_mag, k, np_):
    """Bound of b + sum_k a_k w_k as a bf16-split contraction of NP planes; mag = sum_k |a_k w_k|, bias_mag = |b|."""
    n = SPLIT_TERMS[np_] * k
    return SPLIT_DROP[np_] * mag + gamma(n) * (bias_mag + SPLIT_MAG * mag) + n * MIN_NORMAL


def conv_split(x, w, b, np_, relu=0):
    """conv() under the bf16-split contraction of NP planes (conv3x3_ragged_kernel<..., NP>, conv2 of conv12_fused_split)."""
    y, _ = conv(x, w, b, relu)
    x, w, b = _f64(x), _f64(w), _f64(b)
    kh, kw, cin, cout = w.shape
    n, h, wd, _ = x.shape
    xp = np.zeros((n, h + kh - 1, wd + kw - 1, cin))
    xp[:, kh // 2:kh // 2 + h, kw // 2:kw // 2 + wd] = np.abs(x)
    mag = np.zeros((n, h, wd, cout))
    for ky in range(kh):
        for kx in range(kw):
            mag += xp[:, ky:ky + h, kx:kx + wd] @ np.abs(w[ky, kx])
    return y, split_bound(mag, np.abs(b), kh * kw * cin, np_)


def linear_split(x, w, b, np_):
    """linear() under the bf16-split contraction (gemm_split_kernel<NP>: the GRU input projections)."""
    x, w, b = _f64(x), _f64(w), _f64(b)
    return x @ w + b, split_bound(np.abs(x) @ np.abs(w), np.abs(b), w.shape[0], np_)


# The gates of the relaxed and reduced recurrences (kernels_gru_split.hip; the FAST path of kernels_gru.hip) use the hardware
# v_exp_f32 (exp2) and v_rcp_f32, 1 ulp (<= 2^-23 relative) each:
#   sigmoid(x) = rcp(1 + exp2(x * -log2 e)):  the product rounds (u |x log2 e| in the exponent: u |x| relative in the power, and
#     as much again for the rounded constant), exp2 and rcp 2^-23 each, the sum u.  s = 1 / (1 + E) has |ds / s| <= |dE / E|, so
#     the relative error is FAST_EXP_REL + FAST_RCP_REL + u + 2 u |x|; an exponent beyond the range (E = inf or a flushed
#     power) costs at most one smallest normal absolutely.
#   tanh(x) = (t - 1) rcp(t + 1), t = exp2(min(x, 40) * 2 log2 e):  t is off by (2^-23 + 4 u |x|) relative; d tanh / dt =
#     2 / (t + 1)^2 <= 1 / (2 t), so that moves tanh by at most half of it absolutely; t - 1, t + 1, rcp and the product add
#     3 u + 2^-23 relative to |tanh| (t - 1 is exact where it cancels).
FAST_EXP_REL = 2.0 ** -23
FAST_RCP_REL = 2.0 ** -23


def fast_sigmoid_bound(x, s):
    x, s = np.abs(_f64(x)), _f64(s)
    return (FAST_EXP_REL + FAST_RCP_REL + U + 2 * U * x) * 1.01 * s + MIN_NORMAL


def fast_tanh_bound(x, t):
    x, t = np.minimum(np.abs(_f64(x)), 40.0), np.abs(_f64(t))
    return 0.5 * (FAST_EXP_REL + 4 * U * x) * 1.01 + (3 * U + FAST_RCP_REL) * 1.01 * t + MIN_NORMAL


# ---------------------------------------------------------------- GRU
def gru_dir(x, wi, bi, wh, bh, h_prev_fp32, reverse=False, proj_np=0, hid_np=0, fast_gates=False):
    """One direction of an ONNX / PyTorch GRU (gate order r, z, n; linear_before_reset = 1; h0 = 0), bounded one step
    at a time: h_t is compared with the float64 cell applied to the fp32 h_{t-1} that the evaluation under test
    produced itself (`h_prev_fp32` [T][N][H], its own output of this direction), so the bound does not grow with T.

        r = sigmoid(x Wi_r + bi_r + h Wh_r + bh_r)
        z = sigmoid(x Wi_z + bi_z + h Wh_z + bh_z)
        n = tanh(x Wi_n + bi_n + r (h Wh_n + bh_n))
        h' = (1 - z) n + z h

    Bound: the two projections by the contraction bound; the gate pre-activations add one rounding; sigmoid is
    1/4-Lipschitz and tanh 1-Lipschitz, plus their own bounds; the spec's h' = fmaf(z, h - n, n) rounds twice.

    The relaxed / reduced numerics: proj_np / hid_np = NP (3 or 2) bounds the input projection / the recurrence's h Wh by
    split_bound instead of the k-ascending chain (0), fast_gates the gates by fast_sigmoid_bound / fast_tanh_bound instead of
    the spec's.  The rest of the step is the same arithmetic."""
    x, wi, bi, wh, bh = _f64(x), _f64(wi), _f64(bi), _f64(wh), _f64(bh)
    hs = _f64(h_prev_fp32)
    T, N, I = x.shape
    H = wh.shape[0]
    y = np.empty((T, N, H))
    bound = np.empty((T, N, H))
    order = range(T - 1, -1, -1) if reverse else range(T)
    h = np.zeros((N, H))
    for t in order:
        gx = x[t] @ wi + bi
        mx = np.abs(x[t]) @ np.abs(wi)
        ex = split_bound(mx, np.abs(bi), I, proj_np) if proj_np else gamma(I + 1) * (mx + np.abs(bi)) + I * TINY
        gh = h @ wh + bh
        mh = np.abs(h) @ np.abs(wh)
        eh = split_bound(mh, np.abs(bh), H, hid_np) if hid_np else gamma(H + 1) * (mh + np.abs(bh)) + H * TINY
        ar, az = gx[:, :H] + gh[:, :H], gx[:, H:2 * H] + gh[:, H:2 * H]
        r, z = _sigmoid64(ar), _sigmoid64(az)
        if fast_gates:
            sr, sz = fast_sigmoid_bound(ar, r), fast_sigmoid_bound(az, z)
        else:
            sr, sz = SIGMOID_ULP * ulp(np.maximum(r, MIN_NORMAL)), SIGMOID_ULP * ulp(np.maximum(z, MIN_NORMAL))
        er = 0.25 * (ex[:, :H] + eh[:, :H] + U * np.abs(ar)) + sr
        ez = 0.25 * (ex[:, H:2 * H] + eh[:, H:2 * H] + U * np.abs(az)) + sz
        an = gx[:, 2 * H:] + r * gh[:, 2 * H:]
        n = np.tanh(an)
        # (the argument's own error, at most ea below, also moves the fast tanh's argument-dependent term: negligible)
        ea = ex[:, 2 * H:] + er * np.abs(gh[:, 2 * H:]) + (r + er) * eh[:, 2 * H:] + U * np.abs(an)
        en = ea + (fast_tanh_bound(np.abs(an) + ea, n) if fast_gates else TANH_ABS)
        hn = (1 - z) * n + z * h
        e = ez * np.abs(h - n) + (z + ez) * (en + U * np.abs(h - n)) + en + U * np.abs(hn)
        y[t] = hn
        bound[t] = 1.01 * e   # second-order products of the terms above
        h = hs[t]             # the next step starts from the evaluation's own fp32 state
    return y, bound


def gru_bidir(x, ws, y_fp32, **numerics):
    """Bidirectional GRU -> [T][N][2H] (forward, then backward); ws = (wi, bi, wh, bh) x 2 as in the model file;
    y_fp32 is the fp32 output under test, whose halves supply each direction's previous state; numerics: gru_dir's flags."""
    H = _f64(ws[2]).shape[0]
    yf, bf = gru_dir(x, *ws[0:4], y_fp32[..., :H], reverse=False, **numerics)
    yb, bb = gru_dir(x, *ws[4:8], y_fp32[..., H:], reverse=True, **numerics)
    return np.concatenate([yf, yb], axis=-1), np.concatenate([bf, bb], axis=-1)


# ---------------------------------------------------------------- CTC greedy
def ctc_greedy(logp):
    """Greedy CTC decoding: per step the arg max (the first of equal maxima), merge repeats, drop the blank (0).
    Returns [(label, step)] for the first step of each emitted label."""
    out, last = [], 0
    for t, row in enumerate(np.asarray(logp)):
        best = int(np.argmax(row))      # numpy returns the first maximum
        if best != last and best != 0:
            out.append((best, t))
        last = best
    return out


def check(y, ref, what=""):
    """Assert |y - y64| <= bound elementwise (both finite where the reference is)."""
    y64, bound = ref
    y = np.asarray(y, np.float64)
    assert y.shape == y64.shape, (what, y.shape, y64.shape)
    err = np.abs(y - y64)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), y.shape)
        raise AssertionError("%s: %d of %d elements outside the float64 bound; worst at %s: got %r, float64 %r, "
                             "bound %.3g" % (what, bad.sum(), y.size, i, y[i], y64[i], bound[i]))


# ---------------------------------------------------------------- whole graphs
def _op_ref(op, slots):
    """The float64 reference of one op of an OracleGraph, applied to the oracle's own fp32 input slot(s)."""
    t, x, W = op["type"], slots[op["in0"]], op["w"]
    kh, kw, cin, cout, hid = op["kh"], op["kw"], op["cin"], op["cout"], op["hidden"]
    if t == 0:
        return conv(x, W[0].reshape(kh, kw, cin, cout), W[1], op["relu"])
    if t == 1:
        return dwconv3x3(x, W[0].reshape(3, 3, cin), W[1], op["relu"])
    if t == 2:
        return maxpool(x, kh, kw)
    if t == 3:
        return avgpool(x, kh, kw)
    if t == 4:
        return convt2x2(x, W[0].reshape(2, 2, cin, cout), W[1])
    if t == 5:
        return padcat(x, slots[op["in1"]])
    if t == 6:
        return sigmoid(x)
    if t == 7:
        return to_seq(x)
    if t == 8:
        ws = []
        for d in range(2):
            wi, bi, wh, bh = W[4 * d:4 * d + 4]
            ws += [wi.reshape(cin, 3 * hid), bi, wh.reshape(hid, 3 * hid), bh]
        return gru_bidir(x, ws, slots[op["out"]])
    if t == 9:
        return linear(x, W[0].reshape(cin, cout), W[1], op["relu"])
    if t == 10:
        return log_softmax(x)
    raise AssertionError("op type %d has no float64 definition" % t)


def check_graph(buf, x, what=""):
    """Run a whole model file through the oracle (OracleGraph.run_exact, every slot kept) and check each op's fp32
    output slot, in graph order, against the float64 op applied to the oracle's fp32 input slot(s).  Each op is
    bounded on its own inputs, so the bound does not grow with depth; an op without a float64 definition fails.
    Returns the per-op list of (op name, worst |y - y64| / bound)."""
    from oracle.nn import OracleGraph
    g = OracleGraph(buf)
    _, slots = g.run_exact(x, return_slots=True)
    names = ["conv", "dwconv3", "maxpool", "avgpool", "convt2", "padcat", "sigmoid", "toseq", "gru", "linear",
             "logsoftmax"]
    worst = []
    for i, op in enumerate(g.ops):
        ref = _op_ref(op, slots)
        name = names[op["type"]]
        check(slots[op["out"]], ref, "%s: op %d (%s)" % (what, i, name))
        err = np.abs(np.asarray(slots[op["out"]], np.float64) - ref[0])
        worst.append((name, float(np.max(np.where(ref[1] > 0, err / np.maximum(ref[1], 1e-300), 0), initial=0))))
    return worst


# ---------------------------------------------------------------- exact probes of the split contractions
def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32 (v_cvt_pk_bf16_f32 and split_weights for finite values)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def bf16_planes(x):
    """(hi, mid, lo): each the bf16 nearest to the running residual of the fp32 value x (the residuals are exact)."""
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_rne(r)
    lo = bf16_rne((r - mid).astype(np.float32))
    return hi, mid, lo


# (activation, weight, relaxed result, reduced result): one product each, operands whose planes are known, every partial
# sum an integer or half-integer below 2^24, so each result is exact in fp32 in any order.  257 = 256 + 1 (hi, mid): relaxed
# keeps mid x mid, reduced drops it; 65664.5 = 65536 + 128 + 0.5 (128.5 ties to the even 128): relaxed keeps lo x hi,
# reduced has no lo plane.  tests/test_numeric_spec.py checks these premises on the CPU.
SPLIT_PROBES = [(257.0, 257.0, 66049.0, 66048.0), (65664.5, 1.0, 65664.5, 65664.0), (1.0, 65664.5, 65664.5, 65664.0)]


def split_probe_value(a, w, np_):
    """The sum of the plane products an NP-plane contraction keeps, in float64, for one product a w."""
    ah, am, al = (float(v) for v in bf16_planes(a))
    wh, wm, wl = (float(v) for v in bf16_planes(w))
    kept = [ah * wh, ah * wm, am * wh] + ([am * wm, ah * wl, al * wh] if np_ == 3 else [])
    return sum(kept), kept
