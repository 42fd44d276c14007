// Page measurement: how wide the strokes and how tall the text of resident pages are, as exact integer
// histograms, for a batch of pages of any mix of sizes and parameters.  Nothing is made of a page and no pixel of it is
// written.  A code object of its own, as kernels_speckle.hip is.  tests/measure_ref.py is the definition; everything here
// is integer and set arithmetic on one set taken from the page (ink = v < threshold), every count a sum of integers, every
// box a minimum or a maximum, so the record is defined to the bit whatever the schedule or batch.
//
// Five launches on one stream, no host round trip between them.  Every pass takes one block per 64 x 64 tile of a page, a
// lane per pixel and sixteen rows per wave; blocks find their page by bisecting the descriptors' block prefix (block0).
//   1 measure_mask_kernel   ink = v < threshold, one __ballot per 64 pixels -> the ink bit mask; the number of ink pixels from
//                           popcounts; the initial labels of the ink pixels: the start of the pixel's horizontal run inside its
//                           word; area and box words reset at those starts (a root is one of them).  Paper is not labelled.
//   2 measure_runs_kernel   both run-length histograms from the BIT MASK (1/32 of the page's bytes).  A run is counted where it
//                           ENDS, by the lane of its last pixel, so no carry travels along a row or down a column: a horizontal
//                           run's length is its part inside the word (boundary ballot + clz) plus, when it starts at bit 0,
//                           the leading ones of the words to its left, at most four of them (a length counts at min(L, 255));
//                           a vertical run's length is found by walking up the block's column of words, staged in LDS with
//                           the 255 rows above the tile, at most 254 steps.  A 2 x 256 histogram in LDS per block, then one
//                           atomic per bin that is not zero into the page's record.
//   3 measure_merge_kernel  the unions the initial labels lack: across word boundaries along a row, and with the row above
//                           (N, or NW / NE where N is not ink and the run does not already reach them), ink only.  Lock-free
//                           find + atomicMin; the root is the raster-first pixel.
//   4 measure_boxes_kernel  the head of every in-word run of ink finds its root and adds the run's length to area[root], lowers
//                           x0[root], raises x1[root] and y1[root]; consecutive heads of a row with one root are merged first, so
//                           one of them speaks for all.  y0 is free: the root is the raster-first pixel.
//   5 measure_components_kernel  every root counts as a component; one of area >= min_area adds to comp_h, comp_w and
//                           area_by_h: a histogram in LDS per block, then one atomic per bin that is not zero.
// There is no sixth pass: every block adds what it counted to the page's record itself (see DESIGN.md §7.14 for what that
// costs), and the record is zero when the first launch starts.
//
// The only loops that depend on other threads are uf_find / uf_union below (restated from kernels_speckle.hip): a parent is
// only ever lowered, by atomicMin at a root, so every chain strictly descends and ends; no block waits for another.
// Visibility between passes comes from the kernel boundaries.  Every access is predicated on the page.  The barriers are at
// the top level of each kernel and every thread of every block reaches them; ballots and shuffles are reached by whole waves.
#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int MEASURE_THREADS = 256;
constexpr int MEASURE_WAVES = MEASURE_THREADS / 64;
constexpr int MEASURE_ROWS = 64 / MEASURE_WAVES;     // of a tile, per wave
constexpr int MEASURE_ABOVE = MEASURE_BINS - 1;      // rows above a tile that a vertical run counted at most at 255 can reach
constexpr int MEASURE_COLUMN = MEASURE_ABOVE + 64 + 1;   // the staged column of words: those rows, the tile, the row below it
static_assert(MEASURE_THREADS == MEASURE_BINS, "a bin per thread");

typedef __attribute__((address_space(1))) int32_t gint;
typedef __attribute__((address_space(1))) MeasureInfo ginfo;

int64_t measure_tiles(int h, int w) { return (int64_t)((h + 63) / 64) * ((w + 63) / 64); }
size_t measure_mask_words(int h, int w) { return (size_t)h * (size_t)((w + 63) / 64); }

namespace {   // what only this file's kernels use

// ---- the union-find forest: labels are page-local pixel indices, a root is its component's raster-first pixel
__device__ __forceinline__ int uf_find(gint* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;   // p < x: parents only ever point down
    }
}

__device__ __forceinline__ void uf_union(gint* L, int a, int b) {
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // a > b
        if (old == a) return;
        a = old;   // someone else lowered a first: unite what it became with b
    }
}

// the tile of a block and the page's geometry
struct Tile {
    int ty, tx, h, w, ww;
};
__device__ __forceinline__ Tile tile_of(const MeasureDesc& d, int b) {
    Tile t;
    const int i = b - d.block0;
    t.ty = i / d.ww;
    t.tx = i % d.ww;
    t.h = d.h;
    t.w = d.w;
    t.ww = d.ww;
    return t;
}

// bit i of `edges`: pixel i of the word differs from pixel i - 1 (bit 0 always): where the in-word runs start
__device__ __forceinline__ u64 edges_of(u64 word) { return (word ^ (word << 1)) | 1ull; }
__device__ __forceinline__ int run_start(u64 edges, int lane) { return 63 - __builtin_clzll(edges & (~0ull >> (63 - lane))); }

// bit x of row y of the mask, for -1 <= x - 64 tx <= 64 around the word (y, tx); zero outside the page
struct RowBits {
    u64 word;
    uint32_t left, right;   // the last bit of the word before, the first bit of the word after
};
__device__ __forceinline__ RowBits row_bits(const gu64* __restrict__ m, int y, int tx, int h, int ww) {
    RowBits r = {0ull, 0u, 0u};
    if (y >= 0 && y < h) {
        const gu64* __restrict__ row = m + (size_t)y * ww;
        r.word = row[tx];
        r.left = tx > 0 ? (uint32_t)(row[tx - 1] >> 63) : 0u;
        r.right = tx + 1 < ww ? (uint32_t)(row[tx + 1] & 1ull) : 0u;
    }
    return r;
}
}  // namespace

// ---- pass 1
__global__ void __launch_bounds__(MEASURE_THREADS)
measure_mask_kernel(const MeasureDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MeasureDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gu64* __restrict__ mask = (gu64*)(uintptr_t)d.mask;
    gint* __restrict__ labels = (gint*)(uintptr_t)d.labels;
    gword* __restrict__ area = (gword*)(uintptr_t)d.area;
    gword* __restrict__ bx0 = (gword*)(uintptr_t)d.x0;
    gword* __restrict__ bx1 = (gword*)(uintptr_t)d.x1;
    gword* __restrict__ by1 = (gword*)(uintptr_t)d.y1;
    const int x = t.tx * 64 + lane;
    const float thr = d.threshold;
    float px[MEASURE_ROWS];   // all of them on their way before the first is looked at
#pragma unroll
    for (int i = 0; i < MEASURE_ROWS; i++) {
        const int y = t.ty * 64 + i * MEASURE_WAVES + wave;
        px[i] = y < h && x < w ? src[(int64_t)y * w + x] : 0.0f;
    }
    uint32_t inks = 0;   // uniform in the wave
#pragma unroll
    for (int i = 0; i < MEASURE_ROWS; i++) {   // uniform in the block
        const int y = t.ty * 64 + i * MEASURE_WAVES + wave;
        const bool ink = y < h && x < w && px[i] < thr;   // NaN is not ink
        const u64 word = __ballot(ink);
        inks += (uint32_t)__builtin_popcountll(word);
        const int start = run_start(edges_of(word), lane);
        if (ink) {
            const int p = y * w + x;   // h * w < 2^31
            labels[p] = p - (lane - start);
            if (lane == start) {
                area[p] = 0u;
                bx0[p] = 0xFFFFFFFFu;
                bx1[p] = 0u;
                by1[p] = 0u;
            }
        }
        if (lane == 0 && y < h) mask[(size_t)y * t.ww + t.tx] = word;
    }
    if (lane == 0 && inks) {
        ginfo* info = (ginfo*)(uintptr_t)d.info;
        __hip_atomic_fetch_add(&info->ink, (uint64_t)inks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- pass 2
__global__ void __launch_bounds__(MEASURE_THREADS)
measure_runs_kernel(const MeasureDesc* __restrict__ descs, int n_pages) {
    __shared__ u64 col[MEASURE_COLUMN];      // the words (y, tx) for y = 64 ty - 255 .. 64 ty + 64; zero outside the page
    __shared__ uint32_t hist[2][MEASURE_BINS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MeasureDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h;
    const gu64* __restrict__ mask = (const gu64*)(uintptr_t)d.mask;
    hist[0][tid] = 0u;
    hist[1][tid] = 0u;
    for (int r = tid; r < MEASURE_COLUMN; r += MEASURE_THREADS) {
        const int y = t.ty * 64 - MEASURE_ABOVE + r;
        col[r] = y >= 0 && y < h ? mask[(size_t)y * t.ww + t.tx] : 0ull;
    }
    __syncthreads();
    for (int i = 0; i < MEASURE_ROWS; i++) {
        const int r = i * MEASURE_WAVES + wave, y = t.ty * 64 + r;
        if (y >= h) continue;
        const u64 word = col[MEASURE_ABOVE + r];
        if (!((word >> lane) & 1ull)) continue;   // bits past the page's edge are zero: this pixel is ink on the page
        if (!((col[MEASURE_ABOVE + r + 1] >> lane) & 1ull)) {   // a vertical run ends here
            int len = 1;   // col[MEASURE_ABOVE + r - len]: an index of at least 1
            while (len < MEASURE_BINS - 1 && ((col[MEASURE_ABOVE + r - len] >> lane) & 1ull)) len++;
            atomicAdd(&hist[1][len], 1u);
        }
        const gu64* __restrict__ row = mask + (size_t)y * t.ww;
        const bool next = lane < 63 ? (word >> (lane + 1)) & 1ull : (t.tx + 1 < t.ww ? row[t.tx + 1] & 1ull : 0ull);
        if (!next) {   // a horizontal run ends here
            const int start = run_start(edges_of(word), lane);
            int len = lane - start + 1;
            if (start == 0)   // it may have begun in a word to the left
                for (int k = t.tx - 1; k >= 0 && len < MEASURE_BINS - 1; k--) {
                    const u64 left = row[k];
                    const int lead = left == ~0ull ? 64 : __builtin_clzll(~left);   // the ones at the word's high end
                    len += lead;
                    if (lead < 64) break;
                }
            atomicAdd(&hist[0][len < MEASURE_BINS - 1 ? len : MEASURE_BINS - 1], 1u);
        }
    }
    __syncthreads();
    ginfo* info = (ginfo*)(uintptr_t)d.info;
    const uint32_t across = hist[0][tid], down = hist[1][tid];
    if (across) __hip_atomic_fetch_add(&info->run_h[tid], across, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (down) __hip_atomic_fetch_add(&info->run_v[tid], down, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pass 3
__global__ void __launch_bounds__(MEASURE_THREADS)
measure_merge_kernel(const MeasureDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MeasureDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ mask = (const gu64*)(uintptr_t)d.mask;
    gint* L = (gint*)(uintptr_t)d.labels;
    const int x = t.tx * 64 + lane;
    for (int i = 0; i < MEASURE_ROWS; i++) {
        const int y = t.ty * 64 + i * MEASURE_WAVES + wave;
        if (y >= h || x >= w) continue;
        const RowBits cur = row_bits(mask, y, t.tx, h, t.ww), up = row_bits(mask, y - 1, t.tx, h, t.ww);
        if (!((cur.word >> lane) & 1ull)) continue;   // paper is not labelled
        // whether a neighbour is ink; outside the page nothing is (the mask's bits past the edge are zero)
        const bool vW = lane > 0 ? (cur.word >> (lane - 1)) & 1ull : cur.left != 0u;
        const bool vE = lane < 63 ? (cur.word >> (lane + 1)) & 1ull : cur.right != 0u;
        const bool vN = (up.word >> lane) & 1ull;
        const bool vNW = lane > 0 ? (up.word >> (lane - 1)) & 1ull : up.left != 0u;
        const bool vNE = lane < 63 ? (up.word >> (lane + 1)) & 1ull : up.right != 0u;
        const int p = y * w + x;
        if (lane == 0 && vW) uf_union(L, p, p - 1);   // the run goes on from the word before
        // 8-connectivity: N, unless W and NW already carry it; else the diagonals the run does not reach by itself
        if (vN) {
            if (!(vW && vNW)) uf_union(L, p, p - w);
        } else {
            if (vNW && !vW) uf_union(L, p, p - w - 1);
            if (vNE && !vE) uf_union(L, p, p - w + 1);
        }
    }
}

// ---- pass 4
__global__ void __launch_bounds__(MEASURE_THREADS)
measure_boxes_kernel(const MeasureDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MeasureDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ mask = (const gu64*)(uintptr_t)d.mask;
    gint* L = (gint*)(uintptr_t)d.labels;
    gword* area = (gword*)(uintptr_t)d.area;
    gword* bx0 = (gword*)(uintptr_t)d.x0;
    gword* bx1 = (gword*)(uintptr_t)d.x1;
    gword* by1 = (gword*)(uintptr_t)d.y1;
    const int x = t.tx * 64 + lane;
    for (int i = 0; i < MEASURE_ROWS; i++) {   // uniform in the wave: the ballot and the shuffles below are reached by all 64 lanes
        const int y = t.ty * 64 + i * MEASURE_WAVES + wave;
        if (y >= h) continue;
        const u64 word = mask[(size_t)y * t.ww + t.tx];
        const u64 edges = edges_of(word);
        const u64 heads = word & edges;   // where the runs of ink start (ink lies on the page: x < w)
        if (!heads) continue;
        const bool head = (heads >> lane) & 1ull;
        // the run ends where the bits change next: before the page's edge at the latest, the bits past it being zero
        const u64 rest = lane == 63 ? 0ull : edges >> (lane + 1);
        const int run = !head ? 0 : rest ? __builtin_ctzll(rest) + 1 : 64 - lane;
        const int root = head ? uf_find(L, y * w + x) : -1;
        // Consecutive runs of a row mostly belong to one component (the strokes of a glyph): as §7.4 merges equal bins, the
        // first of a series of heads with one root, its leader, speaks for the series.
        const u64 before = heads & ((1ull << lane) - 1ull);
        const int prev_root = __shfl(root, before ? 63 - __builtin_clzll(before) : lane);
        const bool leader = head && (!before || prev_root != root);
        const u64 leaders = __ballot(leader);
        int sum = run;   // inclusive prefix sum of the run lengths; a lane that is no head adds nothing
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int v = __shfl_up(sum, s);
            if (lane >= s) sum += v;
        }
        const u64 upto = heads & (~0ull >> (63 - lane));   // runs lie in ascending order: the largest x1 is the last head's
        const int last_x1 = __shfl(x + run - 1, upto ? 63 - __builtin_clzll(upto) : lane);
        const u64 after = lane == 63 ? 0ull : leaders >> (lane + 1);
        const int end = after ? lane + __builtin_ctzll(after) : 63;   // the lane before the next leader
        const int sum_end = __shfl(sum, end), x1_end = __shfl(last_x1, end);
        if (leader) {
            __hip_atomic_fetch_add(&area[root], (uint32_t)(sum_end - sum + run), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&bx0[root], (uint32_t)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&bx1[root], (uint32_t)x1_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&by1[root], (uint32_t)y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- pass 5
__global__ void __launch_bounds__(MEASURE_THREADS)
measure_components_kernel(const MeasureDesc* __restrict__ descs, int n_pages) {
    __shared__ uint32_t heights[MEASURE_BINS], widths[MEASURE_BINS];
    __shared__ u64 areas[MEASURE_BINS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MeasureDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ mask = (const gu64*)(uintptr_t)d.mask;
    const gint* __restrict__ L = (const gint*)(uintptr_t)d.labels;
    const gword* __restrict__ area = (const gword*)(uintptr_t)d.area;
    const gword* __restrict__ bx0 = (const gword*)(uintptr_t)d.x0;
    const gword* __restrict__ bx1 = (const gword*)(uintptr_t)d.x1;
    const gword* __restrict__ by1 = (const gword*)(uintptr_t)d.y1;
    heights[tid] = 0u;
    widths[tid] = 0u;
    areas[tid] = 0ull;
    __syncthreads();
    const int x = t.tx * 64 + lane;
    const uint32_t min_area = (uint32_t)d.min_area;
    uint32_t roots = 0, counted = 0;   // this thread's
    for (int i = 0; i < MEASURE_ROWS; i++) {
        const int y = t.ty * 64 + i * MEASURE_WAVES + wave;
        if (y >= h) continue;
        const u64 word = mask[(size_t)y * t.ww + t.tx];
        if (!((word & edges_of(word)) >> lane & 1ull)) continue;   // a root is the head of a run of ink
        const int p = y * w + x;
        if (L[p] != p) continue;
        roots++;
        const uint32_t a = area[p];
        if (a < min_area) continue;
        counted++;
        const uint32_t bh = by1[p] - (uint32_t)y + 1u, bw = bx1[p] - bx0[p] + 1u;   // the root's row is the box's first
        const uint32_t ih = bh < MEASURE_BINS - 1 ? bh : MEASURE_BINS - 1, iw = bw < MEASURE_BINS - 1 ? bw : MEASURE_BINS - 1;
        atomicAdd(&heights[ih], 1u);
        atomicAdd(&widths[iw], 1u);
        atomicAdd(&areas[ih], (u64)a);
    }
    __syncthreads();
    ginfo* info = (ginfo*)(uintptr_t)d.info;
    const uint32_t nh = heights[tid], nw = widths[tid];
    const u64 na = areas[tid];
    if (nh) __hip_atomic_fetch_add(&info->comp_h[tid], nh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nw) __hip_atomic_fetch_add(&info->comp_w[tid], nw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (na) __hip_atomic_fetch_add(&info->area_by_h[tid], (uint64_t)na, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t wave_roots = (uint32_t)wave_sum((u64)roots), wave_counted = (uint32_t)wave_sum((u64)counted);   // every wave reaches this
    if (lane == 0 && wave_roots) __hip_atomic_fetch_add(&info->components, wave_roots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0 && wave_counted) __hip_atomic_fetch_add(&info->counted, wave_counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void measure_pages(const MeasureDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(measure_mask_kernel, dim3(total_blocks), dim3(MEASURE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(measure_runs_kernel, dim3(total_blocks), dim3(MEASURE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(measure_merge_kernel, dim3(total_blocks), dim3(MEASURE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(measure_boxes_kernel, dim3(total_blocks), dim3(MEASURE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(measure_components_kernel, dim3(total_blocks), dim3(MEASURE_THREADS), 0, s, d_descs, n_pages);
}

}  // namespace k
}  // namespace ocrs
