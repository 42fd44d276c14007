// Row-owning tiles of the exact 3x3 ragged conv (kernels_rec.hip, an engine's "conv_rows"): the two decisions the host and the
// kernel share.  No HIP call in here; ocrs_conv_rows_selftest drives both without a GPU.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

namespace ocrs {

constexpr int kConvRowsChunk = 16;   // K chunk of conv3x3_ragged_kernel (RG_BK)
constexpr int kConvRowsPatchH = 4;   // image rows of a 4 x 32 patch: one accumulator each

// Dropping an out-of-image tap instead of accumulating fmaf(0, w, acc) (the numeric spec) gives the same
// bits unless
//   * w is not finite: 0 x Inf = NaN;
//   * acc is -0.0 at that point — a -0.0 bias with only -0 products before it: the spec may then turn it into +0 where
//     the skip leaves -0, which reaches the output only when no ReLU follows (ReLU writes +0 for both).
// Decided once per conv op when the model is loaded: it depends on the model file alone.
inline bool conv_rows_skip_exact(const float* w, size_t n_w, const float* bias, size_t n_bias, bool relu) {
    for (size_t i = 0; i < n_w; i++)
        if (!std::isfinite(w[i])) return false;
    if (relu) return true;
    for (size_t i = 0; i < n_bias; i++) {
        unsigned u;
        memcpy(&u, &bias[i], 4);
        if (u == 0x80000000u) return false;
    }
    return true;
}

// The K loop of a block whose patch starts at image row y0: chunks [0, c_top) are the ky = 0 taps of a top block (the
// accumulator of patch row 0 sits them out), chunks [c_bot, 9 cin / 16) the ky = 2 taps of a bottom block (patch row 3
// sits them out); in between every row takes every chunk.  Chunks are tap-major and cin % 32 == 0, so no chunk straddles a
// tap and both bounds are even.  skip off: c_top = 0, c_bot = the chunk count.
struct RowPhases { int c_top, c_bot; };
constexpr RowPhases conv_row_phases(int y0, int H, int cin, bool skip) {
    const int per_tap = cin / kConvRowsChunk;
    return RowPhases{skip && y0 == 0 ? 3 * per_tap : 0, skip && y0 + kConvRowsPatchH == H ? 6 * per_tap : 9 * per_tap};
}

}  // namespace ocrs
