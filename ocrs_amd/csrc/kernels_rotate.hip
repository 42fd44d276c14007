// Quarter turns of resident pages: dst = np.rot90(src, k), counter-clockwise, for a batch of pages of any
// mix of sizes and turns in one launch.  Pure data movement: pixels travel as 32-bit words, so every bit pattern (NaN
// payloads, -0.0) arrives as it left.  A code object of its own, as kernels_rectify.hip is.
//
// One block = one 64 x 64 tile of a SOURCE page; blocks find their page by bisecting the descriptors' tile prefix
// (block0, ascending; uniform loads).  Four waves.
//   k = 1, 3  the tile goes through LDS.  In: wave w reads source rows w, w + 4, ... of the tile, lane = column: 256
//             contiguous bytes per wave-instruction.  Out: a source column is a destination row, so wave w writes the
//             destination rows of columns w, w + 4, ..., lane = source row (k = 3: row 63 - lane, so that addresses
//             ascend with the lane): again 256 contiguous bytes.  Edge tiles predicate both halves; the one barrier is at
//             the top level of the kernel and every thread of every block reaches it.
//             LDS pitch: the accesses are ds_write_b32 (row-wise: dword r * P + lane) and ds_read_b32 (column-wise: dword
//             lane * P + c), which a read pair fused into ds_read2_b32 does not change.  Both bank a dword address by
//             mod 32 and resolve conflicts within each 32-lane half (cdna_hip_programming.md §2).  The write's 32 lanes hold
//             32 consecutive dwords: 32 banks for any P.  The read's hold lane * P + c: with P = 65 = 1 (mod 32) that is
//             lane + c (mod 32), 32 banks again.  P = 64 would put a whole half on one bank (32-way).
//   k = 0, 2  no LDS: a copy, or rows and columns both reversed.  When the page width is a multiple of 4 and both
//             buffers are 16-byte aligned (desc.vec, decided on the host) every row starts 16-byte aligned and so does
//             the mirrored quad W - 4 - c: 16-byte loads and stores, a thread per quad, a wave per 4 rows x 256 bytes.
//             Otherwise the scalar path: lane = column, as the k = 1, 3 read.
// Traffic: 4 B read + 4 B written per pixel, nothing else (descriptors: 40 B per page, through the scalar cache).
#include "find_desc.hpp"
#include "kernels.hpp"

namespace ocrs {
namespace k {

constexpr int ROT_TILE = 64;
constexpr int ROT_PITCH = 65;   // dwords; = 1 (mod 32): see above
constexpr int ROT_WAVES = 4;

// The page pointers come out of a descriptor in memory, where the compiler cannot see their address space: say it, so that
// the accesses are global_ instructions and not flat_ ones.
typedef __attribute__((address_space(1))) uint32_t gword;
typedef uint32_t word4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) word4 gquad;

__global__ void __launch_bounds__(64 * ROT_WAVES)
rotate_pages_kernel(const RotateDesc* __restrict__ descs, int n_pages) {
    __shared__ uint32_t tile[ROT_TILE * ROT_PITCH];
    const int b = (int)blockIdx.x;
    const RotateDesc d = descs[find_desc(descs, n_pages, b)];
    const int h = d.h, w = d.w, k = d.k;
    const int tiles_x = (w + ROT_TILE - 1) / ROT_TILE;
    const int t = b - d.block0;
    const int r0 = (t / tiles_x) * ROT_TILE, c0 = (t % tiles_x) * ROT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ dst = (gword*)(uintptr_t)d.dst;
    const bool turn = (k & 1) != 0;   // uniform in the block

    if (turn) {
        const int c = c0 + lane;
#pragma unroll 4
        for (int lr = wave; lr < ROT_TILE; lr += ROT_WAVES) {
            const int r = r0 + lr;
            if (r < h && c < w) tile[lr * ROT_PITCH + lane] = src[(int64_t)r * w + c];
        }
    }
    __syncthreads();
    if (turn) {
        // destination [w, h]: k = 1: dst[w - 1 - c][r] = src[r][c]; k = 3: dst[c][h - 1 - r] = src[r][c]
        const int lr = k == 1 ? lane : ROT_TILE - 1 - lane;
        const int r = r0 + lr;
        const int j = k == 1 ? r : h - 1 - r;
#pragma unroll 4
        for (int lc = wave; lc < ROT_TILE; lc += ROT_WAVES) {
            const int c = c0 + lc;
            const int i = k == 1 ? w - 1 - c : c;
            if (r < h && c < w) dst[(int64_t)i * h + j] = tile[lr * ROT_PITCH + lc];
        }
    } else if (d.vec) {
        const int q = threadIdx.x & 15, rr = threadIdx.x >> 4;   // 16 quads x 16 rows per pass
        const int c = c0 + 4 * q;                                 // w % 4 == 0: c < w means c + 3 < w
#pragma unroll
        for (int pass = 0; pass < ROT_TILE / 16; pass++) {
            const int r = r0 + rr + 16 * pass;
            if (r < h && c < w) {
                const word4 v = *(const gquad*)(src + (int64_t)r * w + c);
                const int64_t at = k == 0 ? (int64_t)r * w + c : (int64_t)(h - 1 - r) * w + (w - 4 - c);
                *(gquad*)(dst + at) = k == 0 ? v : v.wzyx;
            }
        }
    } else {
        const int c = c0 + lane;
#pragma unroll 4
        for (int lr = wave; lr < ROT_TILE; lr += ROT_WAVES) {
            const int r = r0 + lr;
            if (r < h && c < w) {
                const int64_t at = k == 0 ? (int64_t)r * w + c : (int64_t)(h - 1 - r) * w + (w - 1 - c);
                dst[at] = src[(int64_t)r * w + c];
            }
        }
    }
}

int64_t rotate_tiles(int h, int w) {
    return (int64_t)((h + ROT_TILE - 1) / ROT_TILE) * ((w + ROT_TILE - 1) / ROT_TILE);
}

void rotate_pages(const RotateDesc* d_descs, int n_pages, int total_tiles, hipStream_t s) {
    if (n_pages <= 0 || total_tiles <= 0) return;
    hipLaunchKernelGGL(rotate_pages_kernel, dim3(total_tiles), dim3(64 * ROT_WAVES), 0, s, d_descs, n_pages);
}

}  // namespace k
}  // namespace ocrs
