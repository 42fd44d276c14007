// Page deskew: the skew profile scores of resident pages and the affine page warp, each for a batch of
// pages of any mix of sizes in one launch.  A code object of its own, as kernels_normalize.hip is.  tests/deskew_ref.py is
// the definition.  The scores are integer arithmetic from the quantised page onwards and every sum is an integer atomic, so
// they do not depend on schedule, batch or launch shape; the warp is float32 with every operation rounded on its own (the
// tree is built with -ffp-contract=off).
//
// skew_profiles_kernel  One block = one 64 x 64 tile of a page, four waves; blocks find their page by bisecting the
//   descriptors' block prefix (block0, ascending; uniform loads).
//   In:    wave w takes the tile's rows 16 w .. 16 w + 15, lane = column: 256 contiguous bytes per wave-instruction.  It
//          carries the bin of the row above in a register, so 17 loads give 16 rows of d = |q(x, y) - q(x, y + 1)|; the
//          page is read 17/16 times for all the angles a block walks (all of them, unless the batch is so small that the
//          launcher deals the angles of a tile over several blocks: see skew_scores()).  d goes into an LDS tile at pitch
//          65 dwords.
//   Walk:  per angle the wave walks COLUMNS of the tile, lane = row: wave w takes columns w, w + 4, ...  The read is dword
//          lane * 65 + c: with 65 = 1 (mod 32) the 32 lanes of a half hit 32 banks (cdna_hip_programming.md §2), as in
//          rotate_pages_kernel.  The bin of (x, y) is (x S + y C - t0) >> 16; down a column it grows by C >> 16 ~ cos per
//          lane, so for |angle| <= 45 degrees a wave's 64 ds_add_u32 land on 45 .. 64 consecutive dwords: few lanes share an
//          address.  A row-wise walk at a small angle would put 64 lanes into <= 17 bins.  Pixels with d = 0 (flat paper,
//          most of a page) add nothing.
//   Bins:  the tile's bins span <= 127 + 2: a shared LDS sub-profile of SKEW_BINS dwords whose bin 0 is the smallest bin
//          the tile's 64 x 64 extent can reach.  Two of them, used alternately: the threads that flush angle a's non-zero
//          bins to the global profile (atomicAdd, uint32) zero them in the same step, and the other buffer, zeroed an angle
//          earlier, takes angle a + 1 meanwhile: one barrier per angle.  The barriers are at the top level of the angle
//          loop, whose trip count is uniform, and every thread of every block reaches them.
// skew_scores_kernel    One block per (page, angle): sum of P[b]^2 in uint64 over the page's bins.
// Bounds: a side is at most 4096 and |S|, |C| <= 65536, so |x S + y C| < 2^29 and, minus t0, < 2^30: int32 holds.  A page's
// bin is at most ((w - 1) |S| + (h - 1) |C|) >> 16 <= h + w - 2; its profile row has h + w dwords.  A profile bin is at most
// 255 h w < 2^32, a score at most (h + w) (255 * 5793)^2 < 2^55.
//
// warp_pages_kernel     One block = 16 rows x 256 columns of an OUTPUT page; wave w takes rows w, w + 4, ..., a lane owns
//   four neighbouring columns and writes them with one 16-byte store where the output's rows start 16-byte aligned
//   (desc.vec, decided on the host), else with four predicated dword stores.  Direct global gathers, as
//   rectify_lines_kernel: neighbouring columns step by (m1, m4), about a page pixel, so L2 serves the taps' re-use.
#include "find_desc.hpp"
#include "kernels.hpp"

namespace ocrs {
namespace k {

constexpr int SKEW_TILE = 64;
constexpr int SKEW_PITCH = 65;    // dwords; = 1 (mod 32): see above
constexpr int SKEW_WAVES = 4;
constexpr int SKEW_ROWS = SKEW_TILE / SKEW_WAVES;   // rows a wave loads
constexpr int SKEW_BINS = 132;    // >= ((63 * 2 * 65536 + 65535) >> 16) + 2
constexpr int SKEW_MIN_ANGLES = 8;       // angles a block walks at least (but for the last block of a tile)
constexpr int SKEW_GRID_BLOCKS = 2048;   // blocks the angle deal aims at: 8 per CU

constexpr int WARP_COLS = 256;    // 64 lanes x 4
constexpr int WARP_ROWS = 16;
constexpr int WARP_WAVES = 4;

// The pointers come out of a descriptor in memory, where the compiler cannot see their address space: say it, so that
// the accesses are global_ instructions and not flat_ ones.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) uint32_t gword;
typedef float float4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float4v gquad;

// §7.4's bin of a pixel; -1: NaN
__device__ __forceinline__ int skew_bin(float v) {
    float g = v + 0.5f;
    g = g < 0.0f ? 0.0f : (g > 1.0f ? 1.0f : g);   // NaN stays
    const float t = g * 256.0f;
    if (t != t) return -1;
    float f = floorf(t);
    f = f > 255.0f ? 255.0f : f;
    return (int)f;
}

__global__ void __launch_bounds__(64 * SKEW_WAVES)
skew_profiles_kernel(const SkewDesc* __restrict__ descs, int n_pages, const int32_t* __restrict__ sc_table, int n_angles, int angles_per_block) {
    __shared__ uint32_t tile[SKEW_TILE * SKEW_PITCH];
    __shared__ uint32_t prof[2][SKEW_BINS];
    const int b = (int)blockIdx.x;
    const SkewDesc d = descs[find_desc(descs, n_pages, b)];
    const int h = d.h, w = d.w;
    const int tiles_x = (w + SKEW_TILE - 1) / SKEW_TILE;
    const int t = b - d.block0;
    const int r0 = (t / tiles_x) * SKEW_TILE, c0 = (t % tiles_x) * SKEW_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gword* __restrict__ out = (gword*)(uintptr_t)d.prof;

    // ---- d of the tile: 0 outside the page, on the page's last row and beside a NaN
    {
        const int c = c0 + lane;
        const int rw = r0 + wave * SKEW_ROWS;
        int q0 = (c < w && rw < h) ? skew_bin(src[(int64_t)rw * w + c]) : -1;
#pragma unroll 4
        for (int i = 0; i < SKEW_ROWS; i++) {
            const int r = rw + i;
            const int q1 = (c < w && r + 1 < h) ? skew_bin(src[(int64_t)(r + 1) * w + c]) : -1;
            const int diff = q0 - q1;
            tile[(wave * SKEW_ROWS + i) * SKEW_PITCH + lane] = (q0 >= 0 && q1 >= 0) ? (uint32_t)(diff < 0 ? -diff : diff) : 0u;
            q0 = q1;
        }
    }
    for (int i = threadIdx.x; i < 2 * SKEW_BINS; i += 64 * SKEW_WAVES) prof[0][i] = 0u;
    __syncthreads();

    // this lane's row of the tile, for every angle
    uint32_t dcol[SKEW_TILE / SKEW_WAVES];
#pragma unroll
    for (int j = 0; j < SKEW_TILE / SKEW_WAVES; j++) dcol[j] = tile[lane * SKEW_PITCH + wave + SKEW_WAVES * j];

    const int a_begin = (int)blockIdx.y * angles_per_block, a_end = min(n_angles, a_begin + angles_per_block);
    for (int a = a_begin; a < a_end; a++) {
        const int S = sc_table[2 * a], C = sc_table[2 * a + 1];
        const int t0 = min(0, (w - 1) * S) + min(0, (h - 1) * C);
        // the tile's smallest value over its whole 64 x 64 extent, on the page or not
        const int base = c0 * S + r0 * C - t0;
        const int b0 = (base + min(0, (SKEW_TILE - 1) * S) + min(0, (SKEW_TILE - 1) * C)) >> 16;
        uint32_t* __restrict__ p = prof[a & 1];
        const int row_v = base + lane * C;
#pragma unroll
        for (int j = 0; j < SKEW_TILE / SKEW_WAVES; j++) {
            const int lc = wave + SKEW_WAVES * j;
            const int local = ((row_v + lc * S) >> 16) - b0;
            if (dcol[j] != 0u && (unsigned)local < (unsigned)SKEW_BINS) atomicAdd(&p[local], dcol[j]);
        }
        __syncthreads();
        if (threadIdx.x < SKEW_BINS) {
            const uint32_t v = p[threadIdx.x];
            const int bin = b0 + (int)threadIdx.x;
            if (v != 0u) {
                p[threadIdx.x] = 0u;
                if ((unsigned)bin < (unsigned)d.nb)
                    __hip_atomic_fetch_add(out + (int64_t)a * d.nb + bin, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

__global__ void __launch_bounds__(256)
skew_scores_kernel(const SkewDesc* __restrict__ descs, int n_angles, unsigned long long* __restrict__ scores) {
    __shared__ unsigned long long wave_sum[4];
    const int page = (int)blockIdx.y, a = (int)blockIdx.x;
    const SkewDesc d = descs[page];
    const gword* __restrict__ p = (const gword*)(uintptr_t)d.prof + (int64_t)a * d.nb;
    unsigned long long s = 0ull;
    for (int i = threadIdx.x; i < d.nb; i += 256) {
        const unsigned long long v = p[i];
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) scores[(int64_t)page * n_angles + a] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// One output pixel: X = (m0 + m1 fx) + m2 fy, Y likewise; taps (ix, iy) .. (ix + 1, iy + 1), `fill` outside the page.
__device__ __forceinline__ float warp_sample(const gfloat* __restrict__ page, int ph, int pw, const WarpDesc& d, float fx, float fy) {
    const float X = (d.m[0] + d.m[1] * fx) + d.m[2] * fy, Y = (d.m[3] + d.m[4] * fx) + d.m[5] * fy;
    const float fix = floorf(X), fiy = floorf(Y);
    const float wx = X - fix, wy = Y - fiy;
    // outside [-1, size]: no tap is on the page (also what keeps a huge or non-finite position out of the int conversion)
    const bool onpage = fix >= -1.0f && fix <= (float)pw && fiy >= -1.0f && fiy <= (float)ph;
    const int ix = onpage ? (int)fix : -2, iy = onpage ? (int)fiy : -2;
    const bool x0in = ix >= 0 && ix < pw, x1in = ix + 1 >= 0 && ix + 1 < pw;
    const bool y0in = iy >= 0 && iy < ph, y1in = iy + 1 >= 0 && iy + 1 < ph;
    const float fill = d.fill;
    const int64_t at = (int64_t)iy * pw + ix;
    const float t00 = (y0in && x0in) ? page[at] : fill;
    const float t01 = (y0in && x1in) ? page[at + 1] : fill;
    const float t10 = (y1in && x0in) ? page[at + pw] : fill;
    const float t11 = (y1in && x1in) ? page[at + pw + 1] : fill;
    const float top = (1.0f - wx) * t00 + wx * t01;
    const float bot = (1.0f - wx) * t10 + wx * t11;
    return (1.0f - wy) * top + wy * bot;
}

__global__ void __launch_bounds__(64 * WARP_WAVES)
warp_pages_kernel(const WarpDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x;
    const WarpDesc d = descs[find_desc(descs, n_pages, b)];
    const int dh = d.dh, dw = d.dw;
    const int blocks_x = (dw + WARP_COLS - 1) / WARP_COLS;
    const int t = b - d.block0;
    const int r0 = (t / blocks_x) * WARP_ROWS, c0 = (t % blocks_x) * WARP_COLS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gfloat* __restrict__ dst = (gfloat*)(uintptr_t)d.dst;
    const int c = c0 + 4 * lane;
    if (c >= dw) return;   // no barrier below
    float fx[4];
#pragma unroll
    for (int q = 0; q < 4; q++) fx[q] = (float)(c + q) + 0.5f;
#pragma unroll 2
    for (int lr = wave; lr < WARP_ROWS; lr += WARP_WAVES) {
        const int r = r0 + lr;
        if (r >= dh) break;
        const float fy = (float)r + 0.5f;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = (c + q < dw) ? warp_sample(src, d.sh, d.sw, d, fx[q], fy) : 0.0f;
        gfloat* row = dst + (int64_t)r * dw + c;
        if (d.vec) {   // dw % 4 == 0: c < dw means c + 3 < dw
            float4v o;
            o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
            *(gquad*)row = o;
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (c + q < dw) row[q] = v[q];
        }
    }
}

int64_t skew_tiles(int h, int w) {
    return (int64_t)((h + SKEW_TILE - 1) / SKEW_TILE) * ((w + SKEW_TILE - 1) / SKEW_TILE);
}

void skew_scores(const SkewDesc* d_descs, int n_pages, int total_tiles, const int32_t* d_sc_table, int n_angles,
                 unsigned long long* d_scores, hipStream_t s) {
    if (n_pages <= 0 || total_tiles <= 0 || n_angles <= 0) return;
    // A small batch leaves most CUs one block, which then walks every angle on its own: the angles are dealt over
    // blockIdx.y, at least SKEW_MIN_ANGLES to a block, until the grid has about SKEW_GRID_BLOCKS blocks.  Each block of a
    // tile loads the tile again (from L2); the sums are integers, so the deal does not show in the result.
    const int want_y = max(1, SKEW_GRID_BLOCKS / total_tiles), max_y = (n_angles + SKEW_MIN_ANGLES - 1) / SKEW_MIN_ANGLES;
    const int per_block = (n_angles + min(want_y, max_y) - 1) / min(want_y, max_y);
    const int grid_y = (n_angles + per_block - 1) / per_block;
    hipLaunchKernelGGL(skew_profiles_kernel, dim3(total_tiles, grid_y), dim3(64 * SKEW_WAVES), 0, s, d_descs, n_pages, d_sc_table, n_angles,
                       per_block);
    hipLaunchKernelGGL(skew_scores_kernel, dim3(n_angles, n_pages), dim3(256), 0, s, d_descs, n_angles, d_scores);
}

int64_t warp_blocks(int dh, int dw) {
    return (int64_t)((dh + WARP_ROWS - 1) / WARP_ROWS) * ((dw + WARP_COLS - 1) / WARP_COLS);
}

void warp_pages(const WarpDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(warp_pages_kernel, dim3(total_blocks), dim3(64 * WARP_WAVES), 0, s, d_descs, n_pages);
}

}  // namespace k
}  // namespace ocrs
