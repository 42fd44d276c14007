// Rectified text-line crops: every line is sampled in its own frame — an affine map from output pixel
// to page position, bilinear taps, a per-column row mask from the words' ranges — straight into its [out_h, out_w] image
// of the batch tensor that crop_lines fills for the plain lines.  A code object of its own, so that the plain crop's
// stays what it was.
//
// One block = 128 output columns of one line, all rows.  The block first builds the columns' [lo, hi] row table in LDS
// from the line's word ranges (once per block; the words are read with uniform addresses), then wave w takes rows w,
// w + 4, ...; a lane owns two neighbouring columns of every row and writes them with one 8-byte store (out_w is a
// multiple of 50 and every image starts at a multiple of out_w floats: 8-byte alignment is what a row is sure to have).
// A gather: neighbouring columns step by (ax, ay), at most about a page pixel, so a wave's taps of one row fall in a
// few page rows.  Reads the line's page pixels about once from HBM (L2 serves the taps' reuse), writes 4 B per pixel.
#include "kernels.hpp"

namespace ocrs {
namespace k {

constexpr int RECT_COLS = 128;   // columns per block: 64 lanes x 2
constexpr int RECT_WAVES = 4;

// One output pixel of the map: (Xc, Yc) = (x0 + ax * fx, y0 + ay * fx) of its column, fy = oy + 0.5.  Every operation is
// rounded on its own (the tree is built with -ffp-contract=off).
__device__ __forceinline__ float rectify_sample(const float* __restrict__ page, int ph, int pw, float Xc, float Yc, float bx,
                                                float by, float fy) {
    const float X = Xc + bx * fy, Y = Yc + by * fy;
    const float fix = floorf(X), fiy = floorf(Y);
    const float wx = X - fix, wy = Y - fiy;
    // outside [-1, size]: no tap is on the page (also what keeps a huge or non-finite position out of the int conversion)
    const bool onpage = fix >= -1.0f && fix <= (float)pw && fiy >= -1.0f && fiy <= (float)ph;
    const int ix = onpage ? (int)fix : -2, iy = onpage ? (int)fiy : -2;
    const bool x0in = ix >= 0 && ix < pw, x1in = ix + 1 >= 0 && ix + 1 < pw;
    const bool y0in = iy >= 0 && iy < ph, y1in = iy + 1 >= 0 && iy + 1 < ph;
    const float fill = -0.5f;
    const int64_t at = (int64_t)iy * pw + ix;
    const float t00 = (y0in && x0in) ? page[at] : fill;
    const float t01 = (y0in && x1in) ? page[at + 1] : fill;
    const float t10 = (y1in && x0in) ? page[at + pw] : fill;
    const float t11 = (y1in && x1in) ? page[at + pw + 1] : fill;
    const float top = (1.0f - wx) * t00 + wx * t01;
    const float bot = (1.0f - wx) * t10 + wx * t11;
    return (1.0f - wy) * top + wy * bot;
}

__global__ void __launch_bounds__(64 * RECT_WAVES)
rectify_lines_kernel(const float* const* __restrict__ pages, const int32_t* __restrict__ page_hw,
                     const RectLineDesc* __restrict__ lines, const int32_t* __restrict__ ranges, int out_h,
                     float* __restrict__ batch) {
    __shared__ int s_lo[RECT_COLS], s_hi[RECT_COLS];
    const RectLineDesc ln = lines[blockIdx.y];
    const int out_w = ln.out_w, rw = ln.resized_w;
    const int cb = blockIdx.x * RECT_COLS;
    if (cb >= out_w) return;   // (the grid is as wide as the widest line of the launch)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = cb + 2 * lane;   // out_w is even: c < out_w means c + 1 < out_w
    float* __restrict__ dst = batch + ln.out_off;
    const float fill = -0.5f;
    if (ln.mode != 0 || cb >= rw) {   // an empty line, or a block wholly in the padding
        if (c < out_w)
            for (int oy = wave; oy < out_h; oy += RECT_WAVES)
                *reinterpret_cast<float2*>(dst + (int64_t)oy * out_w + c) = make_float2(fill, fill);
        return;
    }
    // ---- the row table of this block's columns
    const int4* __restrict__ wr = reinterpret_cast<const int4*>(ranges) + ln.range_off;   // (c0, c1, r0, r1) per word
    if (threadIdx.x < RECT_COLS) {
        const int col = cb + (int)threadIdx.x;
        int lo = out_h, hi = -1;
        int left = -1, right = 0x7fffffff;   // nearest covered column on either side of an uncovered one
        for (int i = 0; i < ln.range_n; i++) {
            const int4 r = wr[i];
            if (r.x > r.y) continue;
            if (r.x <= col && col <= r.y) {
                lo = min(lo, r.z);
                hi = max(hi, r.w);
            } else if (r.y < col) {
                left = max(left, r.y);
            } else {
                right = min(right, r.x);
            }
        }
        if (hi < 0) {
            if (left < 0 && right == 0x7fffffff) {   // no word covers anything
                lo = 0;
                hi = out_h - 1;
            } else {
                for (int i = 0; i < ln.range_n; i++) {
                    const int4 r = wr[i];
                    if (r.x > r.y) continue;
                    if ((r.x <= left && left <= r.y) || (r.x <= right && right <= r.y)) {
                        lo = min(lo, r.z);
                        hi = max(hi, r.w);
                    }
                }
            }
        }
        s_lo[threadIdx.x] = lo;
        s_hi[threadIdx.x] = hi;
    }
    __syncthreads();
    if (c >= out_w) return;
    const float* __restrict__ page = pages[ln.page];
    const int ph = page_hw[2 * ln.page], pw = page_hw[2 * ln.page + 1];
    const int lo0 = s_lo[2 * lane], hi0 = s_hi[2 * lane], lo1 = s_lo[2 * lane + 1], hi1 = s_hi[2 * lane + 1];
    const bool in0 = c < rw, in1 = c + 1 < rw;
    const float fx0 = (float)c + 0.5f, fx1 = (float)(c + 1) + 0.5f;
    const float Xc0 = ln.x0 + ln.ax * fx0, Yc0 = ln.y0 + ln.ay * fx0;
    const float Xc1 = ln.x0 + ln.ax * fx1, Yc1 = ln.y0 + ln.ay * fx1;
#pragma unroll 2
    for (int oy = wave; oy < out_h; oy += RECT_WAVES) {
        const float fy = (float)oy + 0.5f;
        float v0 = fill, v1 = fill;
        if (in0 && lo0 <= oy && oy <= hi0) v0 = rectify_sample(page, ph, pw, Xc0, Yc0, ln.bx, ln.by, fy);
        if (in1 && lo1 <= oy && oy <= hi1) v1 = rectify_sample(page, ph, pw, Xc1, Yc1, ln.bx, ln.by, fy);
        *reinterpret_cast<float2*>(dst + (int64_t)oy * out_w + c) = make_float2(v0, v1);
    }
}

void rectify_lines(const float* const* d_pages, const int32_t* d_page_hw, const RectLineDesc* d_lines, const int32_t* d_ranges,
                   int n_lines, int max_out_w, int out_h, float* d_out, hipStream_t s) {
    if (n_lines <= 0 || max_out_w <= 0) return;
    hipLaunchKernelGGL(rectify_lines_kernel, dim3((max_out_w + RECT_COLS - 1) / RECT_COLS, n_lines), dim3(64 * RECT_WAVES), 0, s,
                       d_pages, d_page_hw, d_lines, d_ranges, out_h, d_out);
}

}  // namespace k
}  // namespace ocrs
