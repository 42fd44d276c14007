// Resampling of resident pages: dst [dh, dw] from src [sh, sw], for a batch of pages of any mix of sizes
// and filters in one launch.  A code object of its own, as kernels_rotate.hip is.  Built with -ffp-contract=off: every
// operation below is float32 and rounded on its own, so the result is defined to the bit (tests/resample_ref.py).
//
//   bilinear  resize_axis / bilerp of bilinear.hpp on the page itself (no virtual padding): the oracle's resize_bilinear.
//   area      along one axis L -> l (l <= L): g = gcd(L, l), P = L / g, q = l / g.  Output j covers [jP, (j+1)P) and source x
//             covers [xq, (x+1)q) on a common grid of L * l / g units.  The taps are x = (jP) / q .. ((j+1)P - 1) / q,
//             ascending; the weight of a tap is the integer overlap ov = min((j+1)P, (x+1)q) - max(jP, xq) >= 1 (the weights
//             of an output sum to P; all are exact in float32).  acc = float(ov0) * in[x0]; acc = acc + float(ov) * in[x] per
//             further tap; value = acc / float(P).  In two dimensions the horizontal rule gives one value per source row of
//             the vertical footprint, and the same rule runs vertically over those values.  Equal lengths are the identity
//             (1 * x / 1); L = 2 l is the box (a + b) / 2.
//
// One block = 4 rows x 64 columns of an OUTPUT page: a wave per row, a lane per pixel; blocks find their page by bisecting
// the descriptors' block prefix (block0, ascending; uniform loads).  Every thread gathers its own taps.  Neighbouring lanes'
// footprints are neighbouring source pixels, so a wave's loads of one source row cover one contiguous run of about
// 256 * (sw / dw) bytes, every line of which is used; rows of a vertical footprint that two waves share (a footprint
// straddles an output boundary whenever q > 1) come from L2 the second time.  Traffic: 4 B read per source pixel the
// footprints touch + 4 B written per output pixel (descriptors: 56 B per page, through the scalar cache).  No LDS.
// Index arithmetic is unsigned 32-bit: the largest grid coordinate is L * l / g <= 65535 * 65534 < 2^32.
#include "bilinear.hpp"
#include "find_desc.hpp"
#include "kernels.hpp"

namespace ocrs {
namespace k {

constexpr int RS_COLS = 64;   // a wave's row segment
constexpr int RS_ROWS = 4;    // waves per block

// The page pointers come out of a descriptor in memory, where the compiler cannot see their address space: say it, so that
// the accesses are global_ instructions and not flat_ ones.
typedef __attribute__((address_space(1))) float gfloat;

__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

__global__ void __launch_bounds__(RS_COLS * RS_ROWS)
resample_pages_kernel(const ResampleDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x;
    const ResampleDesc d = descs[find_desc(descs, n_pages, b)];
    const int sw = d.sw, dh = d.dh, dw = d.dw;
    const int blocks_x = (dw + RS_COLS - 1) / RS_COLS;
    const int t = b - d.block0;
    const int oy = (t / blocks_x) * RS_ROWS + (int)(threadIdx.x >> 6);
    const int ox = (t % blocks_x) * RS_COLS + (int)(threadIdx.x & 63);
    if (oy >= dh || ox >= dw) return;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gfloat* __restrict__ dst = (gfloat*)(uintptr_t)d.dst;
    float value;
    if (d.area) {   // uniform in the block
        const uint32_t py = d.py, qy = d.qy, px = d.px, qx = d.qx;
        const uint32_t y_lo = (uint32_t)oy * py, y_hi = y_lo + py, x_lo = (uint32_t)ox * px, x_hi = x_lo + px;
        const uint32_t ya = y_lo / qy, yb = (y_hi - 1u) / qy, xa = x_lo / qx, xb = (x_hi - 1u) / qx;
        const float fpx = (float)px, fpy = (float)py;
        float vacc = 0.0f;
        for (uint32_t y = ya; y <= yb; y++) {
            const gfloat* __restrict__ row = src + (int64_t)y * sw;
            float hacc = (float)(umin(x_hi, (xa + 1u) * qx) - x_lo) * row[xa];   // max(x_lo, xa * qx) = x_lo
            for (uint32_t x = xa + 1u; x <= xb; x++) hacc = hacc + (float)(umin(x_hi, (x + 1u) * qx) - x * qx) * row[x];
            const float hv = hacc / fpx;
            const float ovy = (float)(umin(y_hi, (y + 1u) * qy) - umax(y_lo, y * qy));
            vacc = y == ya ? ovy * hv : vacc + ovy * hv;
        }
        value = vacc / fpy;
    } else {
        int y0, y1, x0, x1;
        float wy, wx;
        resize_axis(oy, d.sh, dh, y0, y1, wy);
        resize_axis(ox, sw, dw, x0, x1, wx);
        const float tl = src[(int64_t)y0 * sw + x0], tr = src[(int64_t)y0 * sw + x1];
        const float bl = src[(int64_t)y1 * sw + x0], br = src[(int64_t)y1 * sw + x1];
        value = bilerp(tl, tr, bl, br, wx, wy);
    }
    dst[(int64_t)oy * dw + ox] = value;
}

int64_t resample_blocks(int dh, int dw) {
    return (int64_t)((dh + RS_ROWS - 1) / RS_ROWS) * ((dw + RS_COLS - 1) / RS_COLS);
}

void resample_pages(const ResampleDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(resample_pages_kernel, dim3(total_blocks), dim3(RS_COLS * RS_ROWS), 0, s, d_descs, n_pages);
}

}  // namespace k
}  // namespace ocrs
