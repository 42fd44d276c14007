// Page framing: the ink that is connected to the page frame (scanner bars, the wedge of a skewed sheet,
// the slice of a neighbouring page, a gutter shadow) overwritten with the paper's level, for a batch of pages of any mix
// of sizes and parameters; the ink profiles of a page; rectangles cut out of pages.  A code object of its own, as
// kernels_speckle.hip is.  tests/frame_ref.py is the definition; everything here is integer and set arithmetic on sets
// taken from the input page, every count a sum of integers, so the result is defined to the bit whatever the schedule or
// batch.
//
// R = ink inside the ring of `depth` pixels along the page's edges (depth 0: the whole page).  R is labelled with
// 8-connectivity in a union-find forest over page-local int32 pixel indices, the forest of kernels_speckle.hip; the page
// edge and the ring's inner edge are walls, because only pixels of R are ever united.  A component that holds a pixel of an
// enabled side is touching; touching components of at least min_area pixels are removed.
//
// Six launches on one stream, no host round trip between them.  Passes 1, 3, 4 and 5 take one block per 64 x 64 tile of a
// page, a lane per pixel and sixteen rows per wave; blocks find their page by bisecting the descriptors' block prefix.
//   1 frame_mask_kernel    ink = v < threshold, R = ink in the ring, one __ballot per 64 pixels -> the R bit mask; the
//                          histogram of the paper pixels (neither ink nor NaN) of the whole page in the same read; on R the
//                          initial labels (the start of the pixel's run inside its word), areas and flags zeroed.
//   2 frame_levels_kernel  one block per page: pct(1, 2) of the histogram -> the fill.
//   3 frame_merge_kernel   the unions the initial labels lack: across word boundaries along a row, and with the row above.
//   4 frame_area_kernel    every label of R flattened to its root; the head of every in-word run adds the run's length to
//                          its root's area; a pixel of R on an enabled side stores 1 to its root's flag: an idempotent plain
//                          vector store.
//   5 frame_map_kernel     out = removed ? paper_fill : v on 32-bit words, the byte mask, and the counts of pixels and of
//                          components (counted at their roots), summed over the wave, into the block's record.
//   6 frame_info_kernel    one block per page: the blocks' records added up -> the page's FrameInfo.
// A tile wholly outside the ring has no R: passes 3 and 4 leave it at once, uniformly in the block and before anything
// else; with a depth far smaller than the page only passes 1 and 5 touch the whole page.
//
// The only loops that depend on other threads are uf_find / uf_union below (restated from kernels_speckle.hip): a parent is
// only ever lowered, by atomicMin at a root, so every chain strictly descends and ends; no block waits for another.
// Visibility between passes comes from the kernel boundaries.  Every access is predicated on the page.  The barriers are at
// the top level of each kernel and every thread of every block that reaches them does; shuffles and ballots are reached by
// whole waves.
#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int FRAME_THREADS = 256;
constexpr int FRAME_WAVES = FRAME_THREADS / 64;
constexpr int FRAME_ROWS = 64 / FRAME_WAVES;   // of a tile, per wave
static_assert(FRAME_WAVES == 4 && FRAME_COUNTS == 32, "the layout of a block's counts");

typedef __attribute__((address_space(1))) int32_t gint;
typedef __attribute__((address_space(1))) FrameInfo ginfo;
typedef uint32_t uint4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint4v gquadw;

int64_t frame_tiles(int h, int w) { return (int64_t)((h + 63) / 64) * ((w + 63) / 64); }

// What a page's blocks counted in pass 5, a record of FRAME_COUNTS words per block, [wave][8], every word of it written by
// plain stores; pass 6 adds them up.
enum { FC_REMOVED = 0, FC_KEPT, FC_REMOVED_PX, FC_KEPT_PX, FC_INK, FC_RING_INK, FC_USED, FC_PER_WAVE = 8 };
__device__ __forceinline__ gu64* counts_of(const FrameDesc& d, int tile) { return (gu64*)(uintptr_t)d.counts + (size_t)tile * FRAME_COUNTS; }

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
    int t, ty, tx, h, w, ww;
};
__device__ __forceinline__ Tile tile_of(const FrameDesc& d, int b) {
    Tile t;
    t.t = b - d.block0;
    t.ty = t.t / d.ww;
    t.tx = t.t % d.ww;
    t.h = d.h;
    t.w = d.w;
    t.ww = d.ww;
    return t;
}

__device__ __forceinline__ int min4(int a, int b, int c, int e) {
    const int p = a < b ? a : b, q = c < e ? c : e;
    return p < q ? p : q;
}
// the pixel lies in the ring: nearer than `depth` to the nearest side, or anywhere at depth 0
__device__ __forceinline__ bool in_ring(int depth, int y, int x, int h, int w) {
    return depth == 0 || min4(x, y, w - 1 - x, h - 1 - y) < depth;
}
// some pixel of the tile does (uniform in the block): the nearest to a side is one of the tile's own edges on the page
__device__ __forceinline__ bool tile_in_ring(int depth, const Tile& t) {
    const int x0 = t.tx * 64, y0 = t.ty * 64;
    const int x1 = x0 + 63 < t.w ? x0 + 63 : t.w - 1, y1 = y0 + 63 < t.h ? y0 + 63 : t.h - 1;
    return depth == 0 || min4(x0, y0, t.w - 1 - x1, t.h - 1 - y1) < depth;
}

// ---- pass 1
__global__ void __launch_bounds__(FRAME_THREADS)
frame_mask_kernel(const FrameDesc* __restrict__ descs, int n_pages) {
    __shared__ uint32_t hist[FRAME_WAVES][256];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FrameDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gu64* __restrict__ rmask = (gu64*)(uintptr_t)d.rmask;
    gint* __restrict__ labels = (gint*)(uintptr_t)d.labels;
    gword* __restrict__ area = (gword*)(uintptr_t)d.area;
    gbyte* __restrict__ flag = (gbyte*)(uintptr_t)d.seed_flag;
#pragma unroll
    for (int i = 0; i < FRAME_WAVES; i++) hist[i][tid] = 0u;
    __syncthreads();
    const int x = t.tx * 64 + lane;
    const float thr = d.threshold;
    float px[FRAME_ROWS];   // all of them on their way before the first is looked at
#pragma unroll
    for (int i = 0; i < FRAME_ROWS; i++) {
        const int y = t.ty * 64 + i * FRAME_WAVES + wave;
        px[i] = y < h && x < w ? src[(int64_t)y * w + x] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < FRAME_ROWS; i++) {   // uniform in the block
        const int y = t.ty * 64 + i * FRAME_WAVES + wave;
        const bool in = y < h && x < w;
        const float v = px[i];
        const bool ink = in && v < thr;   // NaN is not ink
        const bool r = ink && in_ring(d.depth, y, x, h, w);
        const u64 word = __ballot(r);
        const int bin = in ? bin_of(clamp01(v + 0.5f)) : -1;
        hist_add(hist[wave], ink ? -1 : bin, lane);
        // the start of this pixel's run of equal bits inside the word: bit i of `edges` = pixel i differs from pixel i - 1
        const u64 edges = (word ^ (word << 1)) | 1ull;
        const int start = 63 - __builtin_clzll(edges & (~0ull >> (63 - lane)));
        if (r) {
            const int p = y * w + x;   // h * w < 2^31
            labels[p] = p - (lane - start);
            area[p] = 0u;
            flag[p] = (uint8_t)0;
        }
        if (lane == 0 && y < h) rmask[(size_t)y * t.ww + t.tx] = word;
    }
    __syncthreads();
    uint32_t paper = 0;
#pragma unroll
    for (int i = 0; i < FRAME_WAVES; i++) paper += hist[i][tid];
    gu64* __restrict__ page_hist = (gu64*)(uintptr_t)d.hist;
    if (paper) __hip_atomic_fetch_add(page_hist + tid, (u64)paper, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pass 2: one block per page
// pct(1, 2) of a histogram of 256 bins, a bin per thread -> (the bin, -1 with nothing counted; the total) in every thread.
// Every thread of the block calls it; `wave_tot` and `found` are the caller's LDS.  (Restated from kernels_speckle.hip.)
__device__ __forceinline__ int median_bin(u64 mine, u64* __restrict__ wave_tot, int* __restrict__ found, u64* __restrict__ total, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    u64 incl = mine;   // inclusive scan over the block's 256 bins
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int lo = __shfl_up((int)(uint32_t)incl, s), hi = __shfl_up((int)(uint32_t)(incl >> 32), s);
        if (lane >= s) incl += (u64)(uint32_t)lo | ((u64)(uint32_t)hi << 32);
    }
    __syncthreads();   // the LDS words are free again
    if (lane == 63) wave_tot[wave] = incl;
    if (tid == 0) *found = -1;
    __syncthreads();
    u64 n = 0;
#pragma unroll
    for (int i = 0; i < FRAME_WAVES; i++) {
        const u64 s = wave_tot[i];
        n += s;
        if (i < wave) incl += s;
    }
    const u64 excl = incl - mine;
    if (n > 0 && incl * 2 >= n && !(excl * 2 >= n)) *found = tid;   // the smallest bin whose cumulative count passes
    __syncthreads();
    *total = n;
    return *found;
}

__global__ void __launch_bounds__(FRAME_THREADS)
frame_levels_kernel(const FrameDesc* __restrict__ descs) {
    __shared__ u64 wave_tot[FRAME_WAVES];
    __shared__ int found;
    const int tid = (int)threadIdx.x;
    const FrameDesc d = descs[blockIdx.x];
    const gu64* __restrict__ page_hist = (const gu64*)(uintptr_t)d.hist;
    u64 counted;
    const int paper_bin = median_bin(page_hist[tid], wave_tot, &found, &counted, tid);
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        const bool paper_given = d.paper == d.paper;
        const int pb = paper_bin < 0 ? 255 : paper_bin;
        info->paper_bin = paper_given ? -1 : pb;
        info->paper_fill = paper_given ? d.paper : (float)(pb + 1) / 256.0f - 0.5f;   // exact
        info->counted = counted;
    }
}

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

// ---- pass 3
__global__ void __launch_bounds__(FRAME_THREADS)
frame_merge_kernel(const FrameDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FrameDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    if (!tile_in_ring(d.depth, t)) return;   // uniform in the block: no R here
    const int h = t.h, w = t.w;
    const gu64* __restrict__ rmask = (const gu64*)(uintptr_t)d.rmask;
    gint* L = (gint*)(uintptr_t)d.labels;
    const int x = t.tx * 64 + lane;
    for (int i = 0; i < FRAME_ROWS; i++) {
        const int y = t.ty * 64 + i * FRAME_WAVES + wave;
        if (y >= h || x >= w) continue;
        const RowBits cur = row_bits(rmask, y, t.tx, h, t.ww);
        if (!((cur.word >> lane) & 1ull)) continue;   // only R is united: whatever is not R is a wall
        const RowBits up = row_bits(rmask, y - 1, t.tx, h, t.ww);
        // the bits of the mask are zero outside the page and outside the ring
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
__global__ void __launch_bounds__(FRAME_THREADS)
frame_area_kernel(const FrameDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FrameDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    if (!tile_in_ring(d.depth, t)) return;   // uniform in the block: no R here
    const int h = t.h, w = t.w;
    const gu64* __restrict__ rmask = (const gu64*)(uintptr_t)d.rmask;
    gint* L = (gint*)(uintptr_t)d.labels;
    gword* area = (gword*)(uintptr_t)d.area;
    gbyte* flag = (gbyte*)(uintptr_t)d.seed_flag;
    const int x = t.tx * 64 + lane;
    // A bar's runs of a tile belong to one component: what the wave's rows add to the root it met first is kept in registers
    // and added once, as speckle_area_kernel does for the paper.
    int common = -1;          // uniform in the wave
    uint32_t common_sum = 0;
    for (int i = 0; i < FRAME_ROWS; i++) {   // uniform in the wave
        const int y = t.ty * 64 + i * FRAME_WAVES + wave;
        if (y >= h) continue;
        const u64 word = rmask[(size_t)y * t.ww + t.tx];   // zero past the page's edge: a run of R ends on the page
        if (!word) continue;
        const u64 edges = (word ^ (word << 1)) | 1ull;   // bit i: a run starts at pixel i
        const bool r = (word >> lane) & 1ull, head = r && ((edges >> lane) & 1ull);
        const int p = y * w + x;
        // after pass 3 a pixel that is no head still points at the head of its run: only heads search
        const int start = 63 - __builtin_clzll(edges & (~0ull >> (63 - lane)));
        const int found = head ? uf_find(L, p) : 0;
        const int root = __shfl(found, start);   // start <= lane: the head of this pixel's run when the pixel is in R
        if (r) L[p] = root;
        const u64 rest = lane == 63 ? 0ull : edges >> (lane + 1);
        const int run = rest ? __builtin_ctzll(rest) + 1 : 64 - lane;
        const u64 heads = __ballot(head);   // not zero: the word is not
        if (common < 0) common = __shfl(root, __builtin_ctzll(heads));
        if (head) {
            if (root == common) common_sum += (uint32_t)run;
            else __hip_atomic_fetch_add(&area[root], (uint32_t)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const bool seed = r && (((d.sides & 1) && x == 0) || ((d.sides & 2) && y == 0) || ((d.sides & 4) && x == w - 1) ||
                                ((d.sides & 8) && y == h - 1));
        if (seed) flag[root] = (uint8_t)1;   // the same 1 from whoever finds it
    }
    const uint32_t total = (uint32_t)wave_sum((u64)common_sum);
    if (lane == 0 && common >= 0) __hip_atomic_fetch_add(&area[common], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pass 5
// What a pixel of R is: bit 0 removed, bit 1 kept, bit 2 in R (the byte of the mask); bit 3: it is the root of its component.
__device__ __forceinline__ uint32_t classify(const FrameDesc& d, const gword* __restrict__ area, const gbyte* __restrict__ flag, int p, int root) {
    uint32_t bits = 4u;
    if (flag[root]) bits |= area[root] >= (uint32_t)d.min_area ? 1u : 2u;
    return bits | (root == p ? 8u : 0u);
}
__device__ __forceinline__ void count_bits(uint32_t* n, uint32_t bits) {
    const uint32_t root = bits >> 3;
    n[FC_REMOVED_PX] += bits & 1u;
    n[FC_KEPT_PX] += (bits >> 1) & 1u;
    n[FC_RING_INK] += (bits >> 2) & 1u;
    n[FC_REMOVED] += root & bits;
    n[FC_KEPT] += root & (bits >> 1);
}

__global__ void __launch_bounds__(FRAME_THREADS)
frame_map_kernel(const FrameDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FrameDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ dst = (gword*)(uintptr_t)d.dst;
    gbyte* __restrict__ bytes = (gbyte*)(uintptr_t)d.mask_out;
    const gu64* __restrict__ rmask = (const gu64*)(uintptr_t)d.rmask;
    const gint* __restrict__ L = (const gint*)(uintptr_t)d.labels;
    const gword* __restrict__ area = (const gword*)(uintptr_t)d.area;
    const gbyte* __restrict__ flag = (const gbyte*)(uintptr_t)d.seed_flag;
    const ginfo* __restrict__ info = (const ginfo*)(uintptr_t)d.info;
    const uint32_t paper_fill = __float_as_uint(info->paper_fill);
    const float thr = d.threshold;
    uint32_t n[FC_USED] = {0u, 0u, 0u, 0u, 0u, 0u};   // this thread's counts, in the order of the record
    if (d.vec) {   // uniform in the block; w % 4 == 0: x < w means x + 3 < w
        uint4v px[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = i * FRAME_THREADS + tid, y = t.ty * 64 + (q >> 4), x = t.tx * 64 + 4 * (q & 15);
            const uint4v none = {0u, 0u, 0u, 0u};
            px[i] = y < h && x < w ? *(const gquadw*)(src + (int64_t)y * w + x) : none;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = i * FRAME_THREADS + tid, r = q >> 4, c = 4 * (q & 15), y = t.ty * 64 + r, x = t.tx * 64 + c;
            if (y >= h || x >= w) continue;
            const int at = y * w + x;
            const uint32_t rs = (uint32_t)(rmask[(size_t)y * t.ww + t.tx] >> c) & 15u;
            uint4v v = px[i];
            uint32_t packed = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                n[FC_INK] += __uint_as_float(v[k]) < thr ? 1u : 0u;
                if (!((rs >> k) & 1u)) continue;
                const uint32_t bits = classify(d, area, flag, at + k, L[at + k]);
                if (bits & 1u) v[k] = paper_fill;
                packed |= (bits & 7u) << (8 * k);
                count_bits(n, bits);
            }
            *(gquadw*)(dst + at) = v;
            if (bytes) *(gword*)(bytes + at) = packed;   // at % 4 == 0
        }
    } else {
        const int x = t.tx * 64 + lane;
        uint32_t px[FRAME_ROWS];
#pragma unroll
        for (int i = 0; i < FRAME_ROWS; i++) {
            const int y = t.ty * 64 + i * FRAME_WAVES + wave;
            px[i] = y < h && x < w ? src[(int64_t)y * w + x] : 0u;
        }
#pragma unroll
        for (int i = 0; i < FRAME_ROWS; i++) {
            const int y = t.ty * 64 + i * FRAME_WAVES + wave;
            if (y >= h || x >= w) continue;
            const int at = y * w + x;
            n[FC_INK] += __uint_as_float(px[i]) < thr ? 1u : 0u;
            uint32_t bits = 0;
            if ((rmask[(size_t)y * t.ww + t.tx] >> lane) & 1ull) {
                bits = classify(d, area, flag, at, L[at]);
                count_bits(n, bits);
            }
            dst[at] = (bits & 1u) ? paper_fill : px[i];
            if (bytes) bytes[at] = (uint8_t)(bits & 7u);
        }
    }
    gu64* __restrict__ rec = counts_of(d, t.t) + wave * FC_PER_WAVE;
#pragma unroll
    for (int i = 0; i < FC_USED; i++) {   // every wave of every block reaches this
        const u64 s = wave_sum((u64)n[i]);
        if (lane == 0) rec[i] = s;
    }
}

// ---- pass 6: one block per page
__global__ void __launch_bounds__(FRAME_THREADS)
frame_info_kernel(const FrameDesc* __restrict__ descs) {
    __shared__ u64 part[FRAME_WAVES][FC_USED];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FrameDesc d = descs[blockIdx.x];
    const int tiles = d.hw * d.ww;
    u64 sum[FC_USED] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (int t = tid; t < tiles; t += FRAME_THREADS) {
        const gu64* __restrict__ c = counts_of(d, t);
#pragma unroll
        for (int wv = 0; wv < FRAME_WAVES; wv++)
#pragma unroll
            for (int i = 0; i < FC_USED; i++) sum[i] += c[wv * FC_PER_WAVE + i];
    }
#pragma unroll
    for (int i = 0; i < FC_USED; i++) {
        sum[i] = wave_sum(sum[i]);
        if (lane == 0) part[wave][i] = sum[i];
    }
    __syncthreads();
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        u64 all[FC_USED];
#pragma unroll
        for (int i = 0; i < FC_USED; i++) {
            all[i] = 0ull;
#pragma unroll
            for (int k = 0; k < FRAME_WAVES; k++) all[i] += part[k][i];
        }
        info->ink = all[FC_INK];
        info->ring_ink = all[FC_RING_INK];
        info->removed = all[FC_REMOVED];
        info->removed_pixels = all[FC_REMOVED_PX];
        info->kept = all[FC_KEPT];
        info->kept_pixels = all[FC_KEPT_PX];
    }
}

void clean_frame_pages(const FrameDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(frame_mask_kernel, dim3(total_blocks), dim3(FRAME_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(frame_levels_kernel, dim3(n_pages), dim3(FRAME_THREADS), 0, s, d_descs);
    hipLaunchKernelGGL(frame_merge_kernel, dim3(total_blocks), dim3(FRAME_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(frame_area_kernel, dim3(total_blocks), dim3(FRAME_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(frame_map_kernel, dim3(total_blocks), dim3(FRAME_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(frame_info_kernel, dim3(n_pages), dim3(FRAME_THREADS), 0, s, d_descs);
}

// ---- ink profiles: one block per 64 x 64 tile, a lane per column and sixteen rows per wave.  A row's count is the popcount
// of its ballot, one atomic add per 64-pixel word; a lane adds up its column over the tile's rows and adds once.  Sums of
// integers: exact whatever the order.
__global__ void __launch_bounds__(FRAME_THREADS)
ink_profiles_kernel(const float* __restrict__ src, int h, int w, int ww, float thr, uint32_t* __restrict__ cols, uint32_t* __restrict__ rows) {
    __shared__ uint32_t col_part[FRAME_WAVES][64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = b / ww, tx = b % ww, x = tx * 64 + lane;
    uint32_t mine = 0;
#pragma unroll 4
    for (int i = 0; i < FRAME_ROWS; i++) {   // uniform in the wave
        const int y = ty * 64 + i * FRAME_WAVES + wave;
        const bool ink = y < h && x < w && src[(int64_t)y * w + x] < thr;   // NaN is not ink
        const u64 word = __ballot(ink);
        mine += ink ? 1u : 0u;
        if (lane == 0 && rows && word) atomicAdd(&rows[y], (uint32_t)__builtin_popcountll(word));   // word != 0: y < h
    }
    col_part[wave][lane] = mine;
    __syncthreads();
    if (wave == 0 && cols && x < w) {
        const uint32_t s = col_part[0][lane] + col_part[1][lane] + col_part[2][lane] + col_part[3][lane];
        if (s) atomicAdd(&cols[x], s);
    }
}

void ink_profiles(const float* src, int h, int w, float threshold, uint32_t* cols, uint32_t* rows, hipStream_t s) {
    const int ww = (w + 63) / 64, hw = (h + 63) / 64;   // each at most 1024
    hipLaunchKernelGGL(ink_profiles_kernel, dim3(hw * ww), dim3(FRAME_THREADS), 0, s, src, h, w, ww, threshold, cols, rows);
}

// ---- crop: one block per 64 x 64 tile of the new page.  The source is read by dwords (x0 misaligns it in general); the
// stores are 16 bytes wide when the new page's rows allow it (desc.vec).
__global__ void __launch_bounds__(FRAME_THREADS)
crop_kernel(const CropDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CropDesc d = descs[find_desc(descs, n_pages, b)];
    const int tw = (d.ow + 63) / 64, tile = b - d.block0, ty = tile / tw, tx = tile % tw;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ dst = (gword*)(uintptr_t)d.dst;
    if (d.vec) {   // uniform in the block; ow % 4 == 0: x < ow means x + 3 < ow
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = i * FRAME_THREADS + tid, y = ty * 64 + (q >> 4), x = tx * 64 + 4 * (q & 15);
            if (y >= d.oh || x >= d.ow) continue;
            const int64_t sy = (int64_t)d.y0 + y, sx = (int64_t)d.x0 + x;
            const bool row_in = sy >= 0 && sy < d.h;
            uint4v v;
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = row_in && sx + k >= 0 && sx + k < d.w ? src[sy * d.w + sx + k] : d.fill;
            *(gquadw*)(dst + (int64_t)y * d.ow + x) = v;
        }
    } else {
        const int x = tx * 64 + lane;
        const int64_t sx = (int64_t)d.x0 + x;
#pragma unroll 4
        for (int i = 0; i < FRAME_ROWS; i++) {
            const int y = ty * 64 + i * FRAME_WAVES + wave;
            if (y >= d.oh || x >= d.ow) continue;
            const int64_t sy = (int64_t)d.y0 + y;
            dst[(int64_t)y * d.ow + x] = sy >= 0 && sy < d.h && sx >= 0 && sx < d.w ? src[sy * d.w + sx] : d.fill;
        }
    }
}

void crop_pages(const CropDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(crop_kernel, dim3(total_blocks), dim3(FRAME_THREADS), 0, s, d_descs, n_pages);
}

}  // namespace k
}  // namespace ocrs
