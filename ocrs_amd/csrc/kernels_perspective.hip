// Perspective correction: the directed edge peaks of resident pages and the projective page warp, each
// for a batch of pages of any mix of sizes in one launch.  A code object of its own, as kernels_deskew.hip is.
// tests/perspective_ref.py is the definition.  The peaks are integer arithmetic from the quantised page onwards and every
// sum is an integer atomic, so they do not depend on schedule, batch or launch shape; the warp is float32 with every
// operation rounded on its own (the tree is built with -ffp-contract=off; `/` is the correctly rounded division).
//
// edge_profiles_kernel  One block = one 64 x 64 tile of a page, four waves; blocks find their page by bisecting the
//   descriptors' block prefix, as skew_profiles_kernel does.  The page is read once (17/16 times, plus one column per tile)
//   for both families and all the angles a block walks.
//   In:    wave w takes the tile's rows 16 w .. 16 w + 15, lane = column.  It carries the bin of the row above in a
//          register; the bin of the column to the right comes from the neighbouring lane (lane 63 loads it).  Per pixel:
//          gH = q(x, y + 1) - q(x, y) and gV = q(x + 1, y) - q(x, y), 0 beyond the page's last row / column and beside a NaN.
//          Each becomes its edge code at once (the offset of its sign's sub-profile, or "no edge": edge_code()): min_step
//          is applied here, once, and the angle loop keeps no per-pixel lane masks alive in scalar registers (as raw steps
//          compared inside the loop they cost 60 spilled SGPRs).  gH's codes go into an LDS tile at pitch 65 dwords; gV's
//          stay in the registers they were made in.
//   Walk:  family H walks COLUMNS of the tile, lane = row, as skew_profiles_kernel does: the read is dword lane * 65 + c,
//          32 banks for the 32 lanes of a half (cdna_hip_programming.md §2); the bin grows by C >> 16 ~ cos per lane, so
//          for |angle| <= 45 degrees the 64 ds_add_u32 of a wave land on 45 .. 64 consecutive dwords.  Family V is
//          family H of the transposed page: lane = column, walking rows, and the registers of the load already have that
//          shape (wave w: rows 16 w .. 16 w + 15 of column `lane`), so it needs no LDS tile.  A pixel is a `+` edge, a
//          `-` edge or neither per family and adds 1 (a count) to the sub-profile of its sign: most pixels add nothing.
//   Bins:  four LDS sub-profiles (family x sign) of EDGE_BINS dwords whose bin 0 is the smallest bin the tile's 64 x 64
//          extent can reach, twice, used alternately as in skew_profiles_kernel: the threads that flush angle a's non-zero
//          bins (atomicAdd, uint32) zero them in the same step while the other set takes angle a + 1: one barrier per
//          angle, at the top level of the angle loop, whose trip count is uniform.
// edge_peaks_kernel     One block per (page, family, sign, angle): the profile row's 16 bands, four to a wave; per band
//   the maximum of (count << 32) | (0xFFFFFFFF - bin) over its non-zero bins: the largest count, and the smallest bin
//   that has it.
// Bounds: as skew_profiles_kernel's: a side is at most 4096 and |S|, |C| <= 65536, so |x S + y C| < 2^29 and, minus t0,
// < 2^30.  A bin is at most h + w - 2 for either family (the transposed page has the same h + w); a profile row has h + w
// dwords and every global add checks its bin against it.  A count is at most h w < 2^24.
//
// project_pages_kernel  warp_pages_kernel with the division: one block = 16 rows x 256 columns of an OUTPUT page, a lane
//   owns four neighbouring columns (one 16-byte store where desc.vec allows).  The taps, `fill` and the lerps are
//   warp_pages_kernel's, operation for operation: with m6 = m7 = 0 the output has its bits.
#include "find_desc.hpp"
#include "kernels.hpp"

namespace ocrs {
namespace k {

constexpr int EDGE_TILE = 64;
constexpr int EDGE_PITCH = 65;    // dwords; = 1 (mod 32)
constexpr int EDGE_WAVES = 4;
constexpr int EDGE_ROWS = EDGE_TILE / EDGE_WAVES;   // rows a wave loads
constexpr int EDGE_BINS = 132;    // >= ((63 * 2 * 65536 + 65535) >> 16) + 2
constexpr int EDGE_SUBS = 4;      // family x sign
constexpr int EDGE_MIN_ANGLES = 8;       // angles a block walks at least (but for the last block of a tile)
constexpr int EDGE_GRID_BLOCKS = 2048;   // blocks the angle deal aims at: 8 per CU
constexpr int EDGE_BANDS = 16;

constexpr int PROJ_COLS = 256;    // 64 lanes x 4
constexpr int PROJ_ROWS = 16;
constexpr int PROJ_WAVES = 4;

typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) uint32_t gword;
typedef __attribute__((address_space(1))) unsigned long long gpeak;
typedef float float4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float4v gquad;

// §7.4's bin of a pixel; -1: NaN
__device__ __forceinline__ int edge_bin(float v) {
    float g = v + 0.5f;
    g = g < 0.0f ? 0.0f : (g > 1.0f ? 1.0f : g);   // NaN stays
    const float t = g * 256.0f;
    if (t != t) return -1;
    float f = floorf(t);
    f = f > 255.0f ? 255.0f : f;
    return (int)f;
}

// What a pixel's step g adds to, as the offset of its sign's sub-profile: 0 (`+`), EDGE_BINS (`-`), EDGE_NONE (no edge).
// One integer per pixel, made once: inside the angle loop the only test is (unsigned)(code + local) < 2 EDGE_BINS, which
// depends on the angle, so no per-pixel lane mask is kept in scalar registers across the loop.
constexpr int EDGE_NONE = 0x40000000;
__device__ __forceinline__ int edge_code(int g, int min_step) {
    return g >= min_step ? 0 : (g <= -min_step ? EDGE_BINS : EDGE_NONE);
}

__global__ void __launch_bounds__(64 * EDGE_WAVES)
edge_profiles_kernel(const EdgeDesc* __restrict__ descs, int n_pages, const int32_t* __restrict__ sc_table, int n_angles, int angles_per_block,
                     int min_step) {
    __shared__ int tile[EDGE_TILE * EDGE_PITCH];
    __shared__ uint32_t prof[2][EDGE_SUBS * EDGE_BINS];
    const int b = (int)blockIdx.x;
    const EdgeDesc d = descs[find_desc(descs, n_pages, b)];
    const int h = d.h, w = d.w;
    const int tiles_x = (w + EDGE_TILE - 1) / EDGE_TILE;
    const int t = b - d.block0;
    const int r0 = (t / tiles_x) * EDGE_TILE, c0 = (t % tiles_x) * EDGE_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gword* __restrict__ out = (gword*)(uintptr_t)d.prof;

    // ---- gH into the tile, gV into registers, each as its edge_code: no edge outside the page, on the page's last row / column and beside a NaN
    int vrow[EDGE_ROWS];   // edge_code of gV of (row 16 wave + i, column lane)
    {
        const int c = c0 + lane;
        const int rw = r0 + wave * EDGE_ROWS;
        int q0 = (c < w && rw < h) ? edge_bin(src[(int64_t)rw * w + c]) : -1;
#pragma unroll   // fully: vrow stays in registers
        for (int i = 0; i < EDGE_ROWS; i++) {
            const int r = rw + i;
            const int q1 = (c < w && r + 1 < h) ? edge_bin(src[(int64_t)(r + 1) * w + c]) : -1;
            int qr = __shfl_down(q0, 1);   // every lane of the wave is here: the loop and its bounds are uniform
            if (lane == 63) qr = (c + 1 < w && r < h) ? edge_bin(src[(int64_t)r * w + c + 1]) : -1;
            tile[(wave * EDGE_ROWS + i) * EDGE_PITCH + lane] = edge_code((q0 >= 0 && q1 >= 0) ? q1 - q0 : 0, min_step);
            vrow[i] = edge_code((q0 >= 0 && qr >= 0) ? qr - q0 : 0, min_step);
            q0 = q1;
        }
    }
    for (int i = threadIdx.x; i < EDGE_SUBS * EDGE_BINS; i += 64 * EDGE_WAVES) prof[0][i] = prof[1][i] = 0u;
    __syncthreads();

    // edge_code of gH of this lane's row of the tile, for every angle
    int hcol[EDGE_TILE / EDGE_WAVES];
#pragma unroll
    for (int j = 0; j < EDGE_TILE / EDGE_WAVES; j++) hcol[j] = tile[lane * EDGE_PITCH + wave + EDGE_WAVES * j];

    const int a_begin = (int)blockIdx.y * angles_per_block, a_end = min(n_angles, a_begin + angles_per_block);
    for (int a = a_begin; a < a_end; a++) {
        const int S = sc_table[2 * a], C = sc_table[2 * a + 1];
        const int ext = min(0, (EDGE_TILE - 1) * S) + min(0, (EDGE_TILE - 1) * C);   // over the tile's whole extent, on the page or not
        // family H: bin = (x S + y C - t0) >> 16
        const int base_h = c0 * S + r0 * C - (min(0, (w - 1) * S) + min(0, (h - 1) * C));
        const int b0_h = (base_h + ext) >> 16;
        // family V, the transposed page (h wide, w high): bin = (y S + x C - t0T) >> 16
        const int base_v = r0 * S + c0 * C - (min(0, (h - 1) * S) + min(0, (w - 1) * C));
        const int b0_v = (base_v + ext) >> 16;
        uint32_t* __restrict__ p = prof[a & 1];
        // the walks step by S (V: a row down) or 4 S (H: four columns on): one running value each, no table of multiples
        int at_h = base_h + lane * C + wave * S, at_v = base_v + lane * C + wave * EDGE_ROWS * S;
        const int step_h = EDGE_WAVES * S;
#pragma unroll
        for (int j = 0; j < EDGE_TILE / EDGE_WAVES; j++) {   // column wave + 4 j
            const int local = (at_h >> 16) - b0_h;
            const int idx = hcol[j] + local;
            if ((unsigned)local < (unsigned)EDGE_BINS && (unsigned)idx < 2u * EDGE_BINS) atomicAdd(&p[idx], 1u);
            at_h += step_h;
        }
#pragma unroll
        for (int i = 0; i < EDGE_ROWS; i++) {   // row 16 wave + i
            const int local = (at_v >> 16) - b0_v;
            const int idx = vrow[i] + local;
            if ((unsigned)local < (unsigned)EDGE_BINS && (unsigned)idx < 2u * EDGE_BINS) atomicAdd(&p[2 * EDGE_BINS + idx], 1u);
            at_v += S;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < EDGE_SUBS * EDGE_BINS; i += 64 * EDGE_WAVES) {
            const uint32_t v = p[i];
            if (v != 0u) {
                p[i] = 0u;
                const int sub = i / EDGE_BINS;
                const int bin = (sub < 2 ? b0_h : b0_v) + (i - sub * EDGE_BINS);
                if ((unsigned)bin < (unsigned)d.nb)
                    __hip_atomic_fetch_add(out + ((int64_t)sub * n_angles + a) * d.nb + bin, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

__global__ void __launch_bounds__(64 * EDGE_WAVES)
edge_peaks_kernel(const EdgeDesc* __restrict__ descs, int n_angles) {
    const int page = (int)blockIdx.y, row = (int)blockIdx.x;   // row = (family * 2 + sign) * n_angles + angle
    const EdgeDesc d = descs[page];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gword* __restrict__ p = (const gword*)(uintptr_t)d.prof + (int64_t)row * d.nb;
    gpeak* __restrict__ peaks = (gpeak*)(uintptr_t)d.peaks + (int64_t)row * EDGE_BANDS;
    for (int k = wave; k < EDGE_BANDS; k += EDGE_WAVES) {
        const int lo = k * d.nb / EDGE_BANDS, hi = (k + 1) * d.nb / EDGE_BANDS;
        unsigned long long best = 0ull;
        for (int i = lo + lane; i < hi; i += 64) {
            const unsigned long long v = p[i];
            const unsigned long long e = v != 0ull ? (v << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i) : 0ull;
            best = e > best ? e : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if (lane == 0) peaks[k] = best;
    }
}

// The taps of one position: warp_pages_kernel's warp_sample from X, Y onwards.
__device__ __forceinline__ float project_taps(const gfloat* __restrict__ page, int ph, int pw, float fill, float X, float Y) {
    const float fix = floorf(X), fiy = floorf(Y);
    const float wx = X - fix, wy = Y - fiy;
    // outside [-1, size]: no tap is on the page (also what keeps a huge or non-finite position out of the int conversion)
    const bool onpage = fix >= -1.0f && fix <= (float)pw && fiy >= -1.0f && fiy <= (float)ph;
    const int ix = onpage ? (int)fix : -2, iy = onpage ? (int)fiy : -2;
    const bool x0in = ix >= 0 && ix < pw, x1in = ix + 1 >= 0 && ix + 1 < pw;
    const bool y0in = iy >= 0 && iy < ph, y1in = iy + 1 >= 0 && iy + 1 < ph;
    const int64_t at = (int64_t)iy * pw + ix;
    const float t00 = (y0in && x0in) ? page[at] : fill;
    const float t01 = (y0in && x1in) ? page[at + 1] : fill;
    const float t10 = (y1in && x0in) ? page[at + pw] : fill;
    const float t11 = (y1in && x1in) ? page[at + pw + 1] : fill;
    const float top = (1.0f - wx) * t00 + wx * t01;
    const float bot = (1.0f - wx) * t10 + wx * t11;
    return (1.0f - wy) * top + wy * bot;
}

__device__ __forceinline__ float project_sample(const gfloat* __restrict__ page, int ph, int pw, const ProjDesc& d, float fx, float fy) {
    const float nx = (d.m[0] + d.m[1] * fx) + d.m[2] * fy, ny = (d.m[3] + d.m[4] * fx) + d.m[5] * fy;
    const float dn = (1.0f + d.m[6] * fx) + d.m[7] * fy;
    if (!(dn > 0.0f && dn <= 3.402823466e38f)) return d.fill;   // behind the camera, at its horizon, or not finite
    return project_taps(page, ph, pw, d.fill, nx / dn, ny / dn);
}

__global__ void __launch_bounds__(64 * PROJ_WAVES)
project_pages_kernel(const ProjDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x;
    const ProjDesc d = descs[find_desc(descs, n_pages, b)];
    const int dh = d.dh, dw = d.dw;
    const int blocks_x = (dw + PROJ_COLS - 1) / PROJ_COLS;
    const int t = b - d.block0;
    const int r0 = (t / blocks_x) * PROJ_ROWS, c0 = (t % blocks_x) * PROJ_COLS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gfloat* __restrict__ dst = (gfloat*)(uintptr_t)d.dst;
    const int c = c0 + 4 * lane;
    if (c >= dw) return;   // no barrier below
    float fx[4];
#pragma unroll
    for (int q = 0; q < 4; q++) fx[q] = (float)(c + q) + 0.5f;
#pragma unroll 2
    for (int lr = wave; lr < PROJ_ROWS; lr += PROJ_WAVES) {
        const int r = r0 + lr;
        if (r >= dh) break;
        const float fy = (float)r + 0.5f;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = (c + q < dw) ? project_sample(src, d.sh, d.sw, d, fx[q], fy) : 0.0f;
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

int64_t edge_tiles(int h, int w) {
    return (int64_t)((h + EDGE_TILE - 1) / EDGE_TILE) * ((w + EDGE_TILE - 1) / EDGE_TILE);
}

void edge_peaks(const EdgeDesc* d_descs, int n_pages, int total_tiles, const int32_t* d_sc_table, int n_angles, int min_step, hipStream_t s) {
    if (n_pages <= 0 || total_tiles <= 0 || n_angles <= 0) return;
    // the angle deal of skew_scores(): a small batch's angles go over blockIdx.y; the sums are integers, so the deal does
    // not show in the result
    const int want_y = max(1, EDGE_GRID_BLOCKS / total_tiles), max_y = (n_angles + EDGE_MIN_ANGLES - 1) / EDGE_MIN_ANGLES;
    const int per_block = (n_angles + min(want_y, max_y) - 1) / min(want_y, max_y);
    const int grid_y = (n_angles + per_block - 1) / per_block;
    hipLaunchKernelGGL(edge_profiles_kernel, dim3(total_tiles, grid_y), dim3(64 * EDGE_WAVES), 0, s, d_descs, n_pages, d_sc_table, n_angles,
                       per_block, min_step);
    hipLaunchKernelGGL(edge_peaks_kernel, dim3(EDGE_SUBS * n_angles, n_pages), dim3(64 * EDGE_WAVES), 0, s, d_descs, n_angles);
}

int64_t project_blocks(int dh, int dw) {
    return (int64_t)((dh + PROJ_ROWS - 1) / PROJ_ROWS) * ((dw + PROJ_COLS - 1) / PROJ_COLS);
}

void project_pages(const ProjDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(project_pages_kernel, dim3(total_blocks), dim3(64 * PROJ_WAVES), 0, s, d_descs, n_pages);
}

}  // namespace k
}  // namespace ocrs
