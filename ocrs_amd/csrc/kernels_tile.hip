// Tiled detection: a page larger than the detector's input is cut into model-sized tiles at its own
// resolution, the tiles run through the U-Net as a batch, and every tile writes the page pixels it owns into one
// page-resolution mask / map.  Both kernels move values and compare against the threshold; neither does arithmetic on a
// probability.  A translation unit of its own for the reason kernels_score.hip is one (§7.1, "Cost").
#include "common.hpp"
#include "kernels.hpp"

namespace ocrs {
namespace k {

// One tile's model input [mh, mw]: page[oy + r, ox + c] where that is inside the page, BLACK_VALUE (-0.5) elsewhere.
// QUAD (mw % 4 == 0): four columns per thread.  A tile origin is arbitrary, so the source row is only dword-aligned: four
// dword loads per thread (the wave's four loads cover one contiguous 1 KiB run of the page row), one dwordx4 store to the
// 16-byte-aligned destination row.  Otherwise one column per thread.
// Algorithmic bytes per tile: 4 * (rows x columns inside the page) read + 4 * mh * mw written.
template <bool QUAD>
__global__ void __launch_bounds__(256)
gather_tiles_kernel(const TileDesc* __restrict__ tiles, float* __restrict__ dst, int mh, int mw) {
    constexpr int PX = QUAD ? 4 : 1;
    const int c0 = (blockIdx.x * blockDim.x + threadIdx.x) * PX;
    const int r = blockIdx.y;
    if (c0 >= mw) return;
    const TileDesc d = tiles[blockIdx.z];
    const int y = d.oy + r;
    const int inside = y < d.h ? min(d.w - d.ox, mw) : 0;   // columns [0, inside) of this row come from the page
    const float* __restrict__ src = d.page + (int64_t)y * d.w + d.ox;
    float v[PX];
#pragma unroll
    for (int j = 0; j < PX; j++) v[j] = c0 + j < inside ? src[c0 + j] : -0.5f;
    float* o = dst + ((int64_t)blockIdx.z * mh + r) * mw + c0;
    if (QUAD) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    else *o = v[0];
}

void gather_tiles(const TileDesc* d_tiles, int n_tiles, float* d_dst, int mh, int mw, hipStream_t s) {
    if (n_tiles <= 0) return;
    const bool quad = (mw & 3) == 0 && (((uintptr_t)d_dst) & 15) == 0;
    const int per_row = quad ? mw / 4 : mw;
    const int block = per_row <= 64 ? 64 : per_row <= 128 ? 128 : 256;
    const dim3 grid((per_row + block - 1) / block, mh, n_tiles);
    if (quad) hipLaunchKernelGGL((gather_tiles_kernel<true>), grid, dim3(block), 0, s, d_tiles, d_dst, mh, mw);
    else hipLaunchKernelGGL((gather_tiles_kernel<false>), grid, dim3(block), 0, s, d_tiles, d_dst, mh, mw);
}

// Every tile writes the page pixels it owns, rows [y0, y1) x columns [x0, x1): mask = p > thr (strict; NaN never passes, as
// resize_threshold has it) and, where the tile carries a map pointer, p itself.  Owned rectangles are disjoint, so tiles —
// of one launch or of several — need no ordering among themselves.
// A thread takes four consecutive page columns.  Where the page rows are word-aligned (w % 4 == 0, aligned buffers) the
// groups of four are aligned to the PAGE, so the mask leaves as one dword and the map as one dwordx4; the tile row is read
// with dword loads (its columns start at x0 - ox, any alignment).  The group that straddles an ownership boundary, and every
// group of a page without that alignment, is written pixel by pixel — a neighbouring tile owns the other bytes of that word.
// Algorithmic bytes per owned pixel: 4 read + 1 (mask) [+ 4 (map)] written.
__global__ void __launch_bounds__(256)
stitch_threshold_kernel(const TileDesc* __restrict__ tiles, const float* __restrict__ prob, int mh, int mw, float thr) {
    const TileDesc d = tiles[blockIdx.z];
    const int y = d.y0 + blockIdx.y;
    if (y >= d.y1) return;
    const bool wide = (d.w & 3) == 0 && (((uintptr_t)d.mask) & 3) == 0 && (!d.map || (((uintptr_t)d.map) & 15) == 0);
    const int x = (wide ? d.x0 & ~3 : d.x0) + (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x >= d.x1) return;
    const float* __restrict__ src = prob + ((int64_t)blockIdx.z * mh + (y - d.oy)) * mw;   // tile column = page column - ox
    float v[4];
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool own = x + j >= d.x0 && x + j < d.x1;
        v[j] = own ? src[x + j - d.ox] : 0.0f;
        if (v[j] > thr) bits |= 1u << (8 * j);
    }
    const int64_t o = (int64_t)y * d.w + x;
    if (wide && x >= d.x0 && x + 3 < d.x1) {
        *reinterpret_cast<uint32_t*>(d.mask + o) = bits;
        if (d.map) *reinterpret_cast<float4*>(d.map + o) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (x + j < d.x0 || x + j >= d.x1) continue;
        d.mask[o + j] = (bits >> (8 * j)) & 1;
        if (d.map) d.map[o + j] = v[j];
    }
}

void stitch_threshold(const TileDesc* d_tiles, int n_tiles, const float* d_prob, int mh, int mw, float thr, hipStream_t s) {
    if (n_tiles <= 0) return;
    const int quads = (mw + 3) / 4 + 1;   // an owned row is at most mw wide and starts up to 3 pixels into its first group
    const int block = quads <= 64 ? 64 : quads <= 128 ? 128 : 256;
    hipLaunchKernelGGL(stitch_threshold_kernel, dim3((quads + block - 1) / block, mh, n_tiles), dim3(block), 0, s, d_tiles, d_prob,
                       mh, mw, thr);
}

}  // namespace k
}  // namespace ocrs
