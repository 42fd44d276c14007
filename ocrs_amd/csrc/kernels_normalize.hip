// Page normalisation: background flattening, levels and polarity of resident pages, for a batch of pages
// of any mix of sizes and parameters.  A code object of its own, as kernels_resample.hip is.  tests/normalize_ref.py is
// the definition; built with -ffp-contract=off, every float32 operation below is rounded on its own, every count is an
// integer and every sum of counts an integer atomic, so the result is defined to the bit whatever the schedule or batch.
//
// Five launches on one stream, no host round trip between them.  Passes 1, 3 and 5 take one block of four waves per T x T
// tile of a page (T = 16 .. 256 per page); blocks find their page by bisecting the descriptors' block prefix (block0,
// ascending; uniform loads).  Passes 2 and 4 take one block per page.
//   1 norm_tiles_kernel   histogram of bin(clamp(v + 0.5)) per tile -> the tile's white bin as it is and read mirrored
//                         (a word per tile), its vote into the page's vote, its counts into the page's histogram.
//   2 norm_grid_kernel    polarity from the vote, Wg from the page's effective histogram, then the level grid: floor at
//                         Wg / 2, maximum over the present tiles of the 3 x 3 neighbourhood.
//   3 norm_hist_kernel    page histogram of u (levels only).
//   4 norm_range_kernel   lo, hi from it; the page's NormInfo.
//   5 norm_map_kernel     the output.
// Passes 3 and 5 compute u through norm_u(), so they cannot disagree.
//
// Histograms (passes 1 and 3).  On a text page most pixels of a tile fall into one or two bins, the paper, and a plain LDS
// atomic per pixel serialises on that address.  So (a) each wave owns a private 256-bin histogram in LDS (4 x 1 KB), and
// (b) before the atomic the lanes of a wave merge runs of equal bins: a lane is a head when its left neighbour's bin
// differs (one __shfl_up), the heads are found with one __ballot, and each head adds the length of its run (the distance
// to the next head bit) in one ds_add.  On a blank stretch that is one atomic per wave-instruction instead of 64.  With
// 16-byte loads a thread holds four neighbouring pixels; the merge runs once per component (lanes of one round are four
// pixels apart, still neighbours on paper).  Bin b of the merged histogram belongs to thread b; a 256-wide inclusive scan
// (shuffles within a wave, the four wave totals through LDS) gives every percentile: thread b owns pct when its
// cumulative count passes the mark and its exclusive count does not.
//
// Loads and stores: 4 B read per pixel in passes 1, 3 and 5, 4 B written in pass 5.  When the page width is a multiple of
// 4 and both buffers are 16-byte aligned (desc.vec, decided on the host) every tile row starts 16-byte aligned (T >= 16):
// dwordx4 accesses, a thread per quad; otherwise the scalar path, a lane per pixel.  Both walk the tile in row-major order
// with a trip count that is uniform in the block, so that the shuffles and ballots see all 64 lanes; pixels outside the
// page carry bin -1.  The barriers are at the top level of each kernel and every thread of every block reaches them.
#include "bilinear.hpp"
#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int NORM_THREADS = 256;
constexpr int NORM_WAVES = NORM_THREADS / 64;

typedef __attribute__((address_space(1))) NormState gstate;
// a tile's record (NormDesc::tiles)
__device__ __forceinline__ uint32_t tile_word(int white_light, int white_dark, bool present) {
    return (uint32_t)white_light | ((uint32_t)white_dark << 8) | (present ? 1u << 16 : 0u);
}
typedef float float4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float4v gquad;

// inclusive scan of one value per thread over the block's 256 threads; *total = the sum.  Holds two barriers.
template <class T>
__device__ __forceinline__ T block_scan(T v, T* __restrict__ wave_sum, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    __syncthreads();   // the previous use of wave_sum is over
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NORM_WAVES; i++) {
        const T s = wave_sum[i];
        all += s;
        if (i < wave) before += s;
    }
    *total = all;
    return v + before;
}

// thread b: does pct(num, den) of a histogram of n > 0 counts fall on my bin?  incl / excl: cumulative counts with / without it
__device__ __forceinline__ bool pct_here(unsigned long long incl, unsigned long long excl, unsigned long long n, unsigned num, unsigned den) {
    return incl * den >= num * n && !(excl * den >= num * n);
}

// what passes 3 and 5 need of a page
struct NormCtx {
    const gbyte* grid;
    int th, tw, dark, flatten;
    float inv_t;
};

__device__ __forceinline__ void grid_axis(int o, float inv_t, int cells, int& i0, int& i1, float& wgt) {
    float f = ((float)o + 0.5f) * inv_t - 0.5f;   // exact: T is a power of two
    const float hi = (float)(cells - 1);
    f = f < 0.0f ? 0.0f : f;
    f = f > hi ? hi : f;
    const int a = (int)f;
    i0 = a;
    i1 = a + 1 < cells ? a + 1 : cells - 1;
    wgt = f - (float)a;
}

__device__ __forceinline__ float level_of(const gbyte* __restrict__ grid, int at) { return (float)((int)grid[at] + 1) * 0.00390625f; }

// u of the pixel (x, y) whose value is v
__device__ __forceinline__ float norm_u(const NormCtx& c, float v, int x, int y) {
    const float g = clamp01(c.dark ? 0.5f - v : v + 0.5f);
    if (!c.flatten) return g;
    int y0, y1, x0, x1;
    float wy, wx;
    grid_axis(y, c.inv_t, c.th, y0, y1, wy);
    grid_axis(x, c.inv_t, c.tw, x0, x1, wx);
    const float bg = bilerp(level_of(c.grid, y0 * c.tw + x0), level_of(c.grid, y0 * c.tw + x1), level_of(c.grid, y1 * c.tw + x0),
                            level_of(c.grid, y1 * c.tw + x1), wx, wy);
    const float q = g / bg;   // bg >= 1/256
    return q > 1.0f ? 1.0f : q;
}

__device__ __forceinline__ NormCtx make_ctx(const NormDesc& d, int dark) {
    NormCtx c;
    c.grid = (const gbyte*)(uintptr_t)d.grid;
    c.th = d.th;
    c.tw = d.tw;
    c.dark = dark;
    c.flatten = d.flatten;
    c.inv_t = 1.0f / (float)(1 << d.tshift);
    return c;
}

// Walks the block's tile and hands every pixel's bin to this wave's histogram.  MODE 0: bin(clamp(v + 0.5)); 1: bin(u).
template <int MODE>
__device__ __forceinline__ void tile_histogram(const NormDesc& d, const NormCtx& c, int t, uint32_t* __restrict__ wave_hist) {
    const int T = 1 << d.tshift, h = d.h, w = d.w;
    const int r0 = (t / d.tw) << d.tshift, c0 = (t % d.tw) << d.tshift;
    const int lane = threadIdx.x & 63;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    if (d.vec) {   // uniform in the block
        const int qshift = d.tshift - 2, quads = T << qshift;   // quads per row: T / 4; in the tile: T * T / 4
        for (int p0 = 0; p0 < quads; p0 += NORM_THREADS) {
            const int p = p0 + (int)threadIdx.x;
            const int y = r0 + (p >> qshift), x = c0 + 4 * (p & ((1 << qshift) - 1));
            const bool in = p < quads && y < h && x < w;   // w % 4 == 0: x < w means x + 3 < w
            float4v v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (in) v = *(const gquad*)(src + (int64_t)y * w + x);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int bin = -1;
                if (in) bin = bin_of(MODE == 0 ? clamp01(v[q] + 0.5f) : norm_u(c, v[q], x + q, y));
                hist_add(wave_hist, bin, lane);
            }
        }
    } else {
        for (int p0 = 0; p0 < T * T; p0 += NORM_THREADS) {
            const int p = p0 + (int)threadIdx.x;
            const int y = r0 + (p >> d.tshift), x = c0 + (p & (T - 1));
            int bin = -1;
            if (y < h && x < w) {
                const float v = src[(int64_t)y * w + x];
                bin = bin_of(MODE == 0 ? clamp01(v + 0.5f) : norm_u(c, v, x, y));
            }
            hist_add(wave_hist, bin, lane);
        }
    }
}

// ---- pass 1
__global__ void __launch_bounds__(NORM_THREADS)
norm_tiles_kernel(const NormDesc* __restrict__ descs, int n_pages) {
    __shared__ uint32_t hist[NORM_WAVES][256];
    __shared__ uint32_t wave_sum[NORM_WAVES];
    __shared__ int found[5];   // p5, p50, p95, white as it is, white mirrored
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const NormDesc d = descs[find_desc(descs, n_pages, b)];
    const int t = b - d.block0;
#pragma unroll
    for (int i = 0; i < NORM_WAVES; i++) hist[i][tid] = 0u;
    if (tid < 5) found[tid] = 0;
    __syncthreads();
    NormCtx none = {};
    tile_histogram<0>(d, none, t, hist[tid >> 6]);
    __syncthreads();
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < NORM_WAVES; i++) mine += hist[i][tid];
    uint32_t n32 = 0;
    const unsigned long long incl = block_scan<uint32_t>(mine, wave_sum, &n32), excl = incl - mine, n = n32;
    if (n > 0) {
        if (pct_here(incl, excl, n, 1, 20)) found[0] = tid;
        if (pct_here(incl, excl, n, 1, 2)) found[1] = tid;
        if (pct_here(incl, excl, n, 19, 20)) found[2] = tid;
        if (pct_here(incl, excl, n, 3, 4)) found[3] = tid;
        // read mirrored, bin m = 255 - b has the cumulative count n - excl(b): pct is the LARGEST b that still passes
        if ((n - excl) * 4 >= 3 * n && !((n - incl) * 4 >= 3 * n)) found[4] = 255 - tid;
    }
    gstate* __restrict__ st = (gstate*)(uintptr_t)d.state;
    if (mine) __hip_atomic_fetch_add((gu64*)&st->hist_v[tid], (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid == 0) {
        ((gword*)(uintptr_t)d.tiles)[t] = tile_word(found[3], found[4], n > 0);
        if (d.polarity == 0 && n > 0) {
            const long long v = (long long)(found[2] + found[0] - 2 * found[1]);
            if (v != 0) __hip_atomic_fetch_add((gu64*)&st->vote, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- pass 2: one block per page
__global__ void __launch_bounds__(NORM_THREADS)
norm_grid_kernel(const NormDesc* __restrict__ descs) {
    __shared__ unsigned long long wave_sum[NORM_WAVES];
    __shared__ int white_s;
    const int tid = (int)threadIdx.x;
    const NormDesc d = descs[blockIdx.x];
    gstate* __restrict__ st = (gstate*)(uintptr_t)d.state;
    const long long vote = st->vote;
    const int dark = d.polarity == 0 ? (vote > 0 ? 1 : 0) : (d.polarity == 2 ? 1 : 0);
    const unsigned long long mine = st->hist_v[dark ? 255 - tid : tid];
    if (tid == 0) white_s = -1;
    unsigned long long n = 0;
    const unsigned long long incl = block_scan<unsigned long long>(mine, wave_sum, &n), excl = incl - mine;
    if (n > 0 && pct_here(incl, excl, n, 3, 4)) white_s = tid;
    __syncthreads();
    const int white = white_s;
    if (tid == 0) {
        st->info.dark = dark;
        st->info.white = white;
        st->info.vote = vote;
        st->info.counted = n;
        st->info.lo = -1;
        st->info.hi = -1;
    }
    if (!d.flatten) return;   // no barrier below
    const gword* __restrict__ tiles = (const gword*)(uintptr_t)d.tiles;
    gbyte* __restrict__ grid = (gbyte*)(uintptr_t)d.grid;
    const int th = d.th, tw = d.tw, floor_bin = white >= 0 ? white >> 1 : 0, empty_bin = white >= 0 ? white : 0;
    for (int64_t i = tid; i < (int64_t)th * tw; i += NORM_THREADS) {
        const int ty = (int)(i / tw), tx = (int)(i % tw);
        int best = empty_bin;
        if (tiles[i] >> 16) {
            best = 0;
            for (int y = ty > 0 ? ty - 1 : 0; y <= (ty + 1 < th ? ty + 1 : th - 1); y++)
                for (int x = tx > 0 ? tx - 1 : 0; x <= (tx + 1 < tw ? tx + 1 : tw - 1); x++) {
                    const uint32_t r = tiles[(int64_t)y * tw + x];
                    if (!(r >> 16)) continue;
                    int v = (int)((dark ? r >> 8 : r) & 255u);
                    v = v > floor_bin ? v : floor_bin;
                    best = v > best ? v : best;
                }
        }
        grid[i] = (uint8_t)best;
    }
}

// ---- pass 3
__global__ void __launch_bounds__(NORM_THREADS)
norm_hist_kernel(const NormDesc* __restrict__ descs, int n_pages) {
    __shared__ uint32_t hist[NORM_WAVES][256];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const NormDesc d = descs[find_desc(descs, n_pages, b)];
    gstate* __restrict__ st = (gstate*)(uintptr_t)d.state;
#pragma unroll
    for (int i = 0; i < NORM_WAVES; i++) hist[i][tid] = 0u;
    __syncthreads();
    if (d.levels) {   // uniform in the block
        const NormCtx c = make_ctx(d, st->info.dark);
        tile_histogram<1>(d, c, b - d.block0, hist[tid >> 6]);
    }
    __syncthreads();
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < NORM_WAVES; i++) mine += hist[i][tid];
    if (mine) __hip_atomic_fetch_add((gu64*)&st->hist_u[tid], (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pass 4: one block per page
__global__ void __launch_bounds__(NORM_THREADS)
norm_range_kernel(const NormDesc* __restrict__ descs, NormInfo* __restrict__ info) {
    __shared__ unsigned long long wave_sum[NORM_WAVES];
    __shared__ int found[2];
    const int tid = (int)threadIdx.x;
    const NormDesc d = descs[blockIdx.x];
    gstate* __restrict__ st = (gstate*)(uintptr_t)d.state;
    const unsigned long long mine = st->hist_u[tid];   // all zero with levels off
    if (tid < 2) found[tid] = -1;
    unsigned long long n = 0;
    const unsigned long long incl = block_scan<unsigned long long>(mine, wave_sum, &n), excl = incl - mine;
    if (n > 0) {
        if (pct_here(incl, excl, n, 1, 100)) found[0] = tid;
        if (pct_here(incl, excl, n, 1, 2)) found[1] = tid;
    }
    __syncthreads();
    if (tid == 0) {
        NormInfo out;
        out.dark = st->info.dark;
        out.white = st->info.white;
        out.lo = found[0];
        out.hi = found[1];
        out.vote = st->info.vote;
        out.counted = st->info.counted;
        st->info.lo = out.lo;
        st->info.hi = out.hi;
        info[blockIdx.x] = out;
    }
}

// ---- pass 5
__device__ __forceinline__ float norm_out(const NormCtx& c, float v, int x, int y, bool stretch, float a, float span) {
    const float u = norm_u(c, v, x, y);
    return (stretch ? clamp01((u - a) / span) : u) - 0.5f;
}

__global__ void __launch_bounds__(NORM_THREADS)
norm_map_kernel(const NormDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x;
    const NormDesc d = descs[find_desc(descs, n_pages, b)];
    const gstate* __restrict__ st = (const gstate*)(uintptr_t)d.state;
    const int dark = st->info.dark, lo = st->info.lo, hi = st->info.hi;
    const NormCtx c = make_ctx(d, dark);
    const bool stretch = d.levels && hi > lo && lo >= 0;
    const float a = (float)lo / 256.0f, span = (float)hi / 256.0f - a;
    const bool words = !d.flatten && !d.levels;   // the page's own words, the sign flipped on a dark page
    const uint32_t flip = dark ? 0x80000000u : 0u;
    const int T = 1 << d.tshift, h = d.h, w = d.w, t = b - d.block0;
    const int r0 = (t / d.tw) << d.tshift, c0 = (t % d.tw) << d.tshift;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gfloat* __restrict__ dst = (gfloat*)(uintptr_t)d.dst;
    if (d.vec) {
        const int qshift = d.tshift - 2, quads = T << qshift;
        for (int p = (int)threadIdx.x; p < quads; p += NORM_THREADS) {
            const int y = r0 + (p >> qshift), x = c0 + 4 * (p & ((1 << qshift) - 1));
            if (y >= h || x >= w) continue;
            const int64_t at = (int64_t)y * w + x;
            const float4v v = *(const gquad*)(src + at);
            float4v o;
#pragma unroll
            for (int q = 0; q < 4; q++)
                o[q] = words ? __uint_as_float(__float_as_uint(v[q]) ^ flip) : norm_out(c, v[q], x + q, y, stretch, a, span);
            *(gquad*)(dst + at) = o;
        }
    } else {
        for (int p = (int)threadIdx.x; p < T * T; p += NORM_THREADS) {
            const int y = r0 + (p >> d.tshift), x = c0 + (p & (T - 1));
            if (y >= h || x >= w) continue;
            const int64_t at = (int64_t)y * w + x;
            if (words) ((gword*)dst)[at] = ((const gword*)src)[at] ^ flip;
            else dst[at] = norm_out(c, src[at], x, y, stretch, a, span);
        }
    }
}

void normalize_pages(const NormDesc* d_descs, int n_pages, int total_blocks, NormInfo* d_info, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(norm_tiles_kernel, dim3(total_blocks), dim3(NORM_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(norm_grid_kernel, dim3(n_pages), dim3(NORM_THREADS), 0, s, d_descs);
    hipLaunchKernelGGL(norm_hist_kernel, dim3(total_blocks), dim3(NORM_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(norm_range_kernel, dim3(n_pages), dim3(NORM_THREADS), 0, s, d_descs, d_info);
    hipLaunchKernelGGL(norm_map_kernel, dim3(total_blocks), dim3(NORM_THREADS), 0, s, d_descs, n_pages);
}

}  // namespace k
}  // namespace ocrs
