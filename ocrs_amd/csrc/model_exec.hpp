// What the three parts of the model executor share (model_load.cpp, model.cpp, model_packed.cpp): the op names, the
// launch timer and the one set of GEMM descriptors.  Internal: not installed, not included by kernels.hpp.
#pragma once
#include "kernels.hpp"
#include "model.hpp"

namespace ocrs {

inline const char* const kOpNames[OP_COUNT] = {"conv", "dwconv3", "maxpool", "avgpool", "convt2", "padcat",
                                               "sigmoid", "toseq", "gru", "linear", "logsoftmax"};

// per-launch kernel timing on stream `st` (only when the engine asked for it)
template <class Launch>
inline void timed_launch(StageTimers* timers, hipStream_t st, int cls, double flops, double bytes, Launch&& launch,
                         double mfma_flops = -1.0) {
    int tok = timers ? timers->kbegin(cls, st, flops, bytes, mfma_flops) : -1;
    launch();
    if (tok >= 0) timers->end(tok, st);
}

inline double weight_bytes(const GraphOp& o, int j) { return (double)o.wcount[j] * 4.0; }

namespace desc {
// y[rows][cout] = act(x[rows][cin] . w0 + w1): a pointwise conv over `rows` pixels, or a Linear over `rows` rows
inline k::GemmDesc dense(const GraphOp& op, const float* x, float* y, int64_t rows) {
    k::GemmDesc d{};
    d.A = x; d.lda = op.cin; d.B = op.w[0]; d.ldb = op.cout; d.bias = op.w[1];
    d.C = y; d.ldc = op.cout; d.M = (int)rows; d.N = op.cout; d.K = op.cin; d.relu = op.relu;
    return d;
}
inline k::GemmDesc conv3x3(const GraphOp& op, const float* x, float* y, const TensorShape& a) {
    k::GemmDesc d{};
    d.A = x; d.B = op.w[0]; d.ldb = op.cout; d.bias = op.w[1];
    d.C = y; d.ldc = op.cout; d.M = (int)((int64_t)a.n * a.h * a.w); d.N = op.cout; d.K = 9 * op.cin; d.relu = op.relu;
    d.im2col = 1; d.H = a.h; d.W = a.w; d.Cin = op.cin;
    return d;
}
inline k::GemmDesc convt(const GraphOp& op, const float* x, float* y, const TensorShape& a) {
    k::GemmDesc d{};
    d.A = x; d.lda = op.cin; d.B = op.aux0; d.ldb = 4 * op.cout; d.bias = op.aux1;
    d.C = y; d.M = (int)((int64_t)a.n * a.h * a.w); d.N = 4 * op.cout; d.K = op.cin;
    d.convt = 1; d.H = a.h; d.W = a.w; d.Cout = op.cout;
    return d;
}
// gx[2][rows][3H] = x[rows][I] . Wi[dir] + bi[dir], both directions as one batched launch; with_split: the weights'
// bf16 terms ride along for the relaxed-numerics kernels
inline k::GemmDesc gru_input(const GraphOp& op, const float* x, float* gx, int64_t rows, bool with_split) {
    const int H = op.hidden, I = op.cin;
    k::GemmDesc d{};
    d.A = x; d.lda = I; d.B = op.aux0; d.ldb = 3 * H; d.bias = op.aux1; d.C = gx; d.ldc = 3 * H;
    d.M = (int)rows; d.N = 3 * H; d.K = I; d.batch = 2;
    d.strideA = 0; d.strideB = (int64_t)I * 3 * H; d.strideBias = 3 * H; d.strideC = rows * 3 * H;
    if (with_split) {
        d.Bsplit = op.wsplit; d.strideBsplit = (int64_t)(3 * H / 128) * (I / 16) * 3 * 128 * 16;   // (uint16 units per direction)
    }
    return d;
}
// gh[2][rows][3H] = hs[2][rows][H] . Wh[dir] + bh[dir]; M = rows (a packed step lowers it to its active lines)
inline k::GemmDesc gru_hidden(const GraphOp& op, const float* hs, float* gh, int rows) {
    const int H = op.hidden;
    k::GemmDesc r{};
    r.A = hs; r.lda = H; r.B = op.aux2; r.ldb = 3 * H; r.bias = op.aux3; r.C = gh; r.ldc = 3 * H;
    r.M = rows; r.N = 3 * H; r.K = H; r.batch = 2;
    r.strideA = (int64_t)rows * H; r.strideB = (int64_t)H * 3 * H; r.strideBias = 3 * H; r.strideC = (int64_t)rows * 3 * H;
    return r;
}
}  // namespace desc

}  // namespace ocrs
