// Despeckling: the isolated dark specks of resident pages overwritten with the paper's level and, when
// asked for, the light pinholes inside strokes with the ink's level, for a batch of pages of any mix of sizes and
// parameters.  A code object of its own, as kernels_rules.hip is.  tests/despeckle_ref.py is the definition; everything
// here is integer and set arithmetic on sets taken from the input page, every count a sum of integers, so the result is
// defined to the bit whatever the schedule or batch.
//
// What tells a speck from a full stop is the size of its connected component, so the page is labelled: ink with
// 8-connectivity and everything else (NaN included) with 4-connectivity, in ONE union-find forest over page-local int32
// pixel indices (the two classes never unite).  There is no frame node: the page edge is a wall.  The labels are never
// exposed; only areas and flags at the roots are.
//
// Eight launches on one stream, no host round trip between them.  Passes 1, 3, 4, 5, 6 and 7 take one block per 64 x 64
// tile of a page, a lane per pixel and sixteen rows per wave; blocks find their page by bisecting the descriptors' block
// prefix (block0).
//   1 speckle_mask_kernel     ink = v < threshold, one __ballot per 64 pixels -> the INK bit mask; the histograms of the paper
//                             pixels (neither ink nor NaN) and of the ink pixels in the same read; the initial labels: the start
//                             of the pixel's horizontal run inside its word (boundary ballot + clz); areas and flags zeroed.
//   2 speckle_levels_kernel   one block per page: pct(1, 2) of either histogram -> the two fills.
//   3 speckle_merge_kernel    the unions the initial labels lack: across word boundaries along a row, and with the row above
//                             (N, or NW / NE where N is not ink and the run does not already reach them).  Flat, in global
//                             memory, as ccl_merge_kernel is; lock-free find + atomicMin, the root is the raster-first pixel.
//   4 speckle_area_kernel     every pixel's label flattened to its root (the head of every in-word run searches, the run takes its
//                             answer by a shuffle); the head adds the run's length to its root's area: one add per run, not per
//                             pixel, and one per wave for the root the wave meets first (the paper around the text).
//   5 speckle_big_kernel      BIG = ink whose component is larger than max_area, as a bit mask (pages with keep_near > 0 only).
//   6 speckle_near_kernel     NEAR = BIG dilated by keep_near on bit masks (an OR of the rows within keep_near, then shifts with
//                             the neighbouring words' bits); a candidate pixel inside it stores 1 to its root's flag: an
//                             idempotent plain vector store.  (Pages with keep_near > 0 only.)
//   7 speckle_map_kernel      out = speck ? paper_fill : hole ? ink_fill : v on 32-bit words, the byte mask, and the counts of
//                             pixels and of components (counted at their roots), summed over the wave, into the block's record.
//   8 speckle_info_kernel     one block per page: the blocks' records added up -> the page's SpeckleInfo.
//
// The only loops that depend on other threads are uf_find / uf_union below (restated from kernels_ccl.hip): a parent is
// only ever lowered, by atomicMin at a root, so every chain strictly descends and ends; no block waits for another.
// Visibility between passes comes from the kernel boundaries.  Inside pass 3 parents are read by agent-scope atomic loads
// and written by atomics alone; inside pass 4 a flattened label is a plain store of a root, which a concurrent find may
// or may not see: either way it follows a chain of ancestors to the same root, the forest no longer changing.
//
// Loads and stores of the page: dwords in pass 1 (a lane per pixel, so that the ballot is the word); in pass 7 16-byte
// accesses when the page width is a multiple of 4 and both buffers are 16-byte aligned (desc.vec, decided on the host),
// otherwise a lane per pixel.  Every access is predicated on the page.  The barriers are at the top level of each kernel
// and every thread of every block that passes the block-uniform early return reaches them; shuffles and ballots are reached
// by whole waves.
#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int SPECKLE_THREADS = 256;
constexpr int SPECKLE_WAVES = SPECKLE_THREADS / 64;
constexpr int SPECKLE_ROWS = 64 / SPECKLE_WAVES;   // of a tile, per wave
static_assert(SPECKLE_WAVES == 4 && SPECKLE_COUNTS == 32, "the layout of a block's counts");

typedef __attribute__((address_space(1))) int32_t gint;
typedef __attribute__((address_space(1))) SpeckleInfo ginfo;
typedef uint32_t uint4v __attribute__((ext_vector_type(4)));
typedef int32_t int4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint4v gquadw;
typedef __attribute__((address_space(1))) int4v gquadi;

enum { SM_INK = 0, SM_BIG, SM_NEAR, SM_MASKS };

int64_t speckle_tiles(int h, int w) { return (int64_t)((h + 63) / 64) * ((w + 63) / 64); }
size_t speckle_mask_words(int h, int w) { return (size_t)SM_MASKS * (size_t)h * (size_t)((w + 63) / 64); }

__device__ __forceinline__ gu64* mask_of(const SpeckleDesc& d, int m) {
    return (gu64*)(uintptr_t)d.masks + (size_t)m * (size_t)d.h * (size_t)d.ww;
}

// What a page's blocks counted in pass 7, a record of SPECKLE_COUNTS words per block, [wave][8], every word of it written by
// plain stores; pass 8 adds them up.  (Atomics into one cache line per page cost the rule removal 2.4 to 6 times: §7.8.)
enum { SC_SPECKS = 0, SC_KEPT, SC_SPECK_PX, SC_KEPT_PX, SC_HOLES, SC_HOLE_PX, SC_PER_WAVE = 8 };
__device__ __forceinline__ gu64* counts_of(const SpeckleDesc& d, int tile) { return (gu64*)(uintptr_t)d.counts + (size_t)tile * SPECKLE_COUNTS; }

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
__device__ __forceinline__ Tile tile_of(const SpeckleDesc& d, int b) {
    Tile t;
    t.t = b - d.block0;
    t.ty = t.t / d.ww;
    t.tx = t.t % d.ww;
    t.h = d.h;
    t.w = d.w;
    t.ww = d.ww;
    return t;
}

// ---- pass 1
__global__ void __launch_bounds__(SPECKLE_THREADS)
speckle_mask_kernel(const SpeckleDesc* __restrict__ descs, int n_pages) {
    __shared__ uint32_t hist[SPECKLE_WAVES][2][256];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpeckleDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gu64* __restrict__ ink_mask = mask_of(d, SM_INK);
    gint* __restrict__ labels = (gint*)(uintptr_t)d.labels;
    gword* __restrict__ area = (gword*)(uintptr_t)d.area;
    gbyte* __restrict__ flag = (gbyte*)(uintptr_t)d.near_flag;
#pragma unroll
    for (int i = 0; i < SPECKLE_WAVES; i++) {
        hist[i][0][tid] = 0u;
        hist[i][1][tid] = 0u;
    }
    __syncthreads();
    const int x = t.tx * 64 + lane;
    const float thr = d.threshold;
    float px[SPECKLE_ROWS];   // all of them on their way before the first is looked at
#pragma unroll
    for (int i = 0; i < SPECKLE_ROWS; i++) {
        const int y = t.ty * 64 + i * SPECKLE_WAVES + wave;
        px[i] = y < h && x < w ? src[(int64_t)y * w + x] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < SPECKLE_ROWS; i++) {   // uniform in the block
        const int y = t.ty * 64 + i * SPECKLE_WAVES + wave;
        const bool in = y < h && x < w;
        const float v = px[i];
        const bool ink = in && v < thr;   // NaN is not ink
        const u64 word = __ballot(ink);
        const int bin = in ? bin_of(clamp01(v + 0.5f)) : -1;
        hist_add(hist[wave][0], ink ? -1 : bin, lane);
        hist_add(hist[wave][1], ink ? bin : -1, lane);
        // the start of this pixel's run of equal bits inside the word: bit i of `edges` = pixel i differs from pixel i - 1
        const u64 edges = (word ^ (word << 1)) | 1ull;
        const int start = 63 - __builtin_clzll(edges & (~0ull >> (63 - lane)));
        if (in) {
            const int p = y * w + x;   // h * w < 2^31
            labels[p] = p - (lane - start);
            area[p] = 0u;
            flag[p] = (uint8_t)0;
        }
        if (lane == 0 && y < h) ink_mask[(size_t)y * t.ww + t.tx] = word;
    }
    __syncthreads();
    uint32_t paper = 0, inks = 0;
#pragma unroll
    for (int i = 0; i < SPECKLE_WAVES; i++) {
        paper += hist[i][0][tid];
        inks += hist[i][1][tid];
    }
    gu64* __restrict__ page_hist = (gu64*)(uintptr_t)d.hist;
    if (paper) __hip_atomic_fetch_add(page_hist + tid, (u64)paper, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (inks) __hip_atomic_fetch_add(page_hist + 256 + tid, (u64)inks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pass 2: one block per page
// pct(1, 2) of a histogram of 256 bins, a bin per thread -> (the bin, -1 with nothing counted; the total) in every thread.
// Every thread of the block calls it; `wave_tot` and `found` are the caller's LDS.
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
    for (int i = 0; i < SPECKLE_WAVES; i++) {
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

__global__ void __launch_bounds__(SPECKLE_THREADS)
speckle_levels_kernel(const SpeckleDesc* __restrict__ descs) {
    __shared__ u64 wave_tot[SPECKLE_WAVES];
    __shared__ int found;
    const int tid = (int)threadIdx.x;
    const SpeckleDesc d = descs[blockIdx.x];
    const gu64* __restrict__ page_hist = (const gu64*)(uintptr_t)d.hist;
    u64 counted, ink;
    const int paper_bin = median_bin(page_hist[tid], wave_tot, &found, &counted, tid);
    const int ink_bin = median_bin(page_hist[256 + tid], wave_tot, &found, &ink, tid);
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        const bool paper_given = d.paper == d.paper, ink_given = d.ink_level == d.ink_level;
        const int pb = paper_bin < 0 ? 255 : paper_bin, ib = ink_bin < 0 ? 0 : ink_bin;
        info->paper_bin = paper_given ? -1 : pb;
        info->ink_bin = ink_given ? -1 : ib;
        info->paper_fill = paper_given ? d.paper : (float)(pb + 1) / 256.0f - 0.5f;   // exact
        info->ink_fill = ink_given ? d.ink_level : (float)ib / 256.0f - 0.5f;         // exact
        info->ink = ink;
        info->counted = counted;
    }
}

// bit x of row y of a row-major mask, for -1 <= x - 64 tx <= 64 around the word (y, tx); zero outside the page
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
__global__ void __launch_bounds__(SPECKLE_THREADS)
speckle_merge_kernel(const SpeckleDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpeckleDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ ink_mask = mask_of(d, SM_INK);
    gint* L = (gint*)(uintptr_t)d.labels;
    const int x = t.tx * 64 + lane;
    for (int i = 0; i < SPECKLE_ROWS; i++) {
        const int y = t.ty * 64 + i * SPECKLE_WAVES + wave;
        if (y >= h || x >= w) continue;
        const RowBits cur = row_bits(ink_mask, y, t.tx, h, t.ww), up = row_bits(ink_mask, y - 1, t.tx, h, t.ww);
        const bool hasW = x > 0, hasN = y > 0, hasE = x + 1 < w;
        // the class of a neighbour: 1 ink, 0 not ink, -1 outside the page
        const int v = (int)((cur.word >> lane) & 1ull);
        const int vW = !hasW ? -1 : (lane > 0 ? (int)((cur.word >> (lane - 1)) & 1ull) : (int)cur.left);
        const int vE = !hasE ? -1 : (lane < 63 ? (int)((cur.word >> (lane + 1)) & 1ull) : (int)cur.right);
        const int vN = !hasN ? -1 : (int)((up.word >> lane) & 1ull);
        const int vNW = !(hasN && hasW) ? -1 : (lane > 0 ? (int)((up.word >> (lane - 1)) & 1ull) : (int)up.left);
        const int vNE = !(hasN && hasE) ? -1 : (lane < 63 ? (int)((up.word >> (lane + 1)) & 1ull) : (int)up.right);
        const int p = y * w + x;
        if (lane == 0 && vW == v) uf_union(L, p, p - 1);   // the run goes on from the word before
        if (v) {
            // 8-connectivity: N, unless W and NW already carry it; else the diagonals the run does not reach by itself
            if (vN == 1) {
                if (!(vW == 1 && vNW == 1)) uf_union(L, p, p - w);
            } else {
                if (vNW == 1 && vW != 1) uf_union(L, p, p - w - 1);
                if (vNE == 1 && vE != 1) uf_union(L, p, p - w + 1);
            }
        } else {
            if (vN == 0 && !(vW == 0 && vNW == 0)) uf_union(L, p, p - w);   // 4-connectivity
        }
    }
}

// ---- pass 4
__global__ void __launch_bounds__(SPECKLE_THREADS)
speckle_area_kernel(const SpeckleDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpeckleDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ ink_mask = mask_of(d, SM_INK);
    gint* L = (gint*)(uintptr_t)d.labels;
    gword* area = (gword*)(uintptr_t)d.area;
    const int x = t.tx * 64 + lane;
    const int valid = w - t.tx * 64 >= 64 ? 64 : w - t.tx * 64;   // pixels of the word that lie on the page
    // Most runs of a tile belong to one component, the paper around the text: what the wave's rows add to the root it met
    // first is kept in registers and added once (a per-run add to that one word took 466 us in place of the figure of
    // DESIGN.md §7.9 on sixteen pages of 1024 x 1024).
    int common = -1;          // uniform in the wave
    uint32_t common_sum = 0;
    for (int i = 0; i < SPECKLE_ROWS; i++) {   // uniform in the wave
        const int y = t.ty * 64 + i * SPECKLE_WAVES + wave;
        if (y >= h) continue;
        const u64 word = ink_mask[(size_t)y * t.ww + t.tx];
        const u64 edges = (word ^ (word << 1)) | 1ull;   // bit i: a run starts at pixel i
        const bool in = x < w, head = in && ((edges >> lane) & 1ull);
        const int p = y * w + x;
        // after pass 3 a pixel that is no head still points at the head of its run: only heads search
        const int start = 63 - __builtin_clzll(edges & (~0ull >> (63 - lane)));
        const int found = head ? uf_find(L, p) : 0;
        const int root = __shfl(found, start);   // start <= lane: on the page when this lane is
        if (in) L[p] = root;
        const u64 rest = lane == 63 ? 0ull : edges >> (lane + 1);
        int run = rest ? __builtin_ctzll(rest) + 1 : 64 - lane;
        if (lane + run > valid) run = valid - lane;   // the last run ends at the page's edge
        if (common < 0) common = __shfl(root, 0);   // lane 0 is a head on the page
        if (head) {
            if (root == common) common_sum += (uint32_t)run;
            else __hip_atomic_fetch_add(&area[root], (uint32_t)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const uint32_t total = (uint32_t)wave_sum((u64)common_sum);
    if (lane == 0 && common >= 0) __hip_atomic_fetch_add(&area[common], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pass 5: pages with keep_near > 0
__global__ void __launch_bounds__(SPECKLE_THREADS)
speckle_big_kernel(const SpeckleDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpeckleDesc d = descs[find_desc(descs, n_pages, b)];
    if (d.keep_near <= 0) return;   // uniform in the block
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ ink_mask = mask_of(d, SM_INK);
    gu64* __restrict__ big_mask = mask_of(d, SM_BIG);
    const gint* __restrict__ L = (const gint*)(uintptr_t)d.labels;
    const gword* __restrict__ area = (const gword*)(uintptr_t)d.area;
    const int x = t.tx * 64 + lane;
    const uint32_t max_area = (uint32_t)d.max_area;
#pragma unroll 4
    for (int i = 0; i < SPECKLE_ROWS; i++) {   // uniform in the wave
        const int y = t.ty * 64 + i * SPECKLE_WAVES + wave;
        if (y >= h) continue;
        const u64 word = ink_mask[(size_t)y * t.ww + t.tx];
        bool big = false;
        if (x < w && ((word >> lane) & 1ull)) big = area[L[y * w + x]] > max_area;
        const u64 out = __ballot(big);
        if (lane == 0) big_mask[(size_t)y * t.ww + t.tx] = out;
    }
}

// ---- pass 6: pages with keep_near > 0
__global__ void __launch_bounds__(SPECKLE_THREADS)
speckle_near_kernel(const SpeckleDesc* __restrict__ descs, int n_pages) {
    __shared__ u64 rows[64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpeckleDesc d = descs[find_desc(descs, n_pages, b)];
    const int K = d.keep_near;
    if (K <= 0) return;   // uniform in the block
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ ink_mask = mask_of(d, SM_INK);
    const gu64* __restrict__ big_mask = mask_of(d, SM_BIG);
    gu64* __restrict__ near_mask = mask_of(d, SM_NEAR);
    const gint* __restrict__ L = (const gint*)(uintptr_t)d.labels;
    const gword* __restrict__ area = (const gword*)(uintptr_t)d.area;
    gbyte* __restrict__ flag = (gbyte*)(uintptr_t)d.near_flag;
    {   // four threads to a row of the tile: each ORs a quarter of the rows within K, in the word and its two neighbours
        const int r = tid >> 2, q = tid & 3, y = t.ty * 64 + r;
        u64 c = 0ull, l = 0ull, rt = 0ull;
        if (y < h) {
            for (int dy = -K + q; dy <= K; dy += 4) {
                const int yy = y + dy;
                if (yy < 0 || yy >= h) continue;
                const gu64* __restrict__ row = big_mask + (size_t)yy * t.ww;
                c |= row[t.tx];
                if (t.tx > 0) l |= row[t.tx - 1];
                if (t.tx + 1 < t.ww) rt |= row[t.tx + 1];
            }
        }
        c |= shfl_xor64(c, 1);
        l |= shfl_xor64(l, 1);
        rt |= shfl_xor64(rt, 1);
        c |= shfl_xor64(c, 2);
        l |= shfl_xor64(l, 2);
        rt |= shfl_xor64(rt, 2);
        u64 out = c;
        for (int s = 1; s <= K; s++) out |= (c << s) | (l >> (64 - s)) | (c >> s) | (rt << (64 - s));   // K <= 16 < 64
        if (q == 0) {
            rows[r] = out;
            if (y < h) near_mask[(size_t)y * t.ww + t.tx] = out;   // bits past the page's edge may be set here; nobody reads them
        }
    }
    __syncthreads();
    const int x = t.tx * 64 + lane;
    const uint32_t max_area = (uint32_t)d.max_area;
    for (int i = 0; i < SPECKLE_ROWS; i++) {
        const int r = i * SPECKLE_WAVES + wave, y = t.ty * 64 + r;
        if (y >= h || x >= w) continue;
        if (!((rows[r] >> lane) & 1ull)) continue;
        const u64 word = ink_mask[(size_t)y * t.ww + t.tx];
        if (!((word >> lane) & 1ull)) continue;
        const int root = L[y * w + x];
        if (area[root] <= max_area) flag[root] = (uint8_t)1;   // a candidate within K of big ink: kept; the same 1 from whoever finds it
    }
}

// ---- pass 7
// What a pixel is: bit 0 speck, bit 1 hole, bit 2 kept (the byte of the mask); bit 3: it is the root of its component.
__device__ __forceinline__ uint32_t classify(const SpeckleDesc& d, const gword* __restrict__ area, const gbyte* __restrict__ flag, int p,
                                             int root, bool ink) {
    const uint32_t a = area[root];
    uint32_t bits = 0;
    if (ink) {
        if (a <= (uint32_t)d.max_area) bits = d.keep_near > 0 && flag[root] ? 4u : 1u;
    } else if (a <= (uint32_t)d.max_hole) {
        bits = 2u;
    }
    return bits | (root == p ? 8u : 0u);
}

__global__ void __launch_bounds__(SPECKLE_THREADS)
speckle_map_kernel(const SpeckleDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpeckleDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ dst = (gword*)(uintptr_t)d.dst;
    gbyte* __restrict__ bytes = (gbyte*)(uintptr_t)d.mask_out;
    const gu64* __restrict__ ink_mask = mask_of(d, SM_INK);
    const gint* __restrict__ L = (const gint*)(uintptr_t)d.labels;
    const gword* __restrict__ area = (const gword*)(uintptr_t)d.area;
    const gbyte* __restrict__ flag = (const gbyte*)(uintptr_t)d.near_flag;
    const ginfo* __restrict__ info = (const ginfo*)(uintptr_t)d.info;
    const uint32_t paper_fill = __float_as_uint(info->paper_fill), ink_fill = __float_as_uint(info->ink_fill);
    uint32_t n[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // this thread's counts, in the order of the record
    if (d.vec) {   // uniform in the block; w % 4 == 0: x < w means x + 3 < w
        uint4v px[4];
        int4v lab[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = i * SPECKLE_THREADS + tid, y = t.ty * 64 + (q >> 4), x = t.tx * 64 + 4 * (q & 15);
            const uint4v none = {0u, 0u, 0u, 0u};
            const int4v nol = {0, 0, 0, 0};
            const bool in = y < h && x < w;
            px[i] = in ? *(const gquadw*)(src + (int64_t)y * w + x) : none;
            lab[i] = in ? *(const gquadi*)(L + (int64_t)y * w + x) : nol;   // h * w * 4 B from a 16-byte aligned base: at % 4 == 0
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = i * SPECKLE_THREADS + tid, r = q >> 4, c = 4 * (q & 15), y = t.ty * 64 + r, x = t.tx * 64 + c;
            if (y >= h || x >= w) continue;
            const int at = y * w + x;
            const uint32_t inks = (uint32_t)(ink_mask[(size_t)y * t.ww + t.tx] >> c) & 15u;
            uint4v v = px[i];
            uint32_t packed = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t bits = classify(d, area, flag, at + k, lab[i][k], (inks >> k) & 1u);
                if (bits & 1u) v[k] = paper_fill;
                if (bits & 2u) v[k] = ink_fill;
                packed |= (bits & 7u) << (8 * k);
                const uint32_t root = bits >> 3;
                n[SC_SPECK_PX] += bits & 1u;
                n[SC_HOLE_PX] += (bits >> 1) & 1u;
                n[SC_KEPT_PX] += (bits >> 2) & 1u;
                n[SC_SPECKS] += root & bits;
                n[SC_HOLES] += root & (bits >> 1);
                n[SC_KEPT] += root & (bits >> 2);
            }
            *(gquadw*)(dst + at) = v;
            if (bytes) *(gword*)(bytes + at) = packed;   // at % 4 == 0
        }
    } else {
        const int x = t.tx * 64 + lane;
        uint32_t px[SPECKLE_ROWS];
        int lab[SPECKLE_ROWS];
#pragma unroll
        for (int i = 0; i < SPECKLE_ROWS; i++) {
            const int y = t.ty * 64 + i * SPECKLE_WAVES + wave;
            const bool in = y < h && x < w;
            px[i] = in ? src[(int64_t)y * w + x] : 0u;
            lab[i] = in ? L[(int64_t)y * w + x] : 0;
        }
#pragma unroll
        for (int i = 0; i < SPECKLE_ROWS; i++) {
            const int y = t.ty * 64 + i * SPECKLE_WAVES + wave;
            if (y >= h || x >= w) continue;
            const int at = y * w + x;
            const bool ink = (ink_mask[(size_t)y * t.ww + t.tx] >> lane) & 1ull;
            const uint32_t bits = classify(d, area, flag, at, lab[i], ink);
            dst[at] = (bits & 1u) ? paper_fill : (bits & 2u) ? ink_fill : px[i];
            if (bytes) bytes[at] = (uint8_t)(bits & 7u);
            const uint32_t root = bits >> 3;
            n[SC_SPECK_PX] += bits & 1u;
            n[SC_HOLE_PX] += (bits >> 1) & 1u;
            n[SC_KEPT_PX] += (bits >> 2) & 1u;
            n[SC_SPECKS] += root & bits;
            n[SC_HOLES] += root & (bits >> 1);
            n[SC_KEPT] += root & (bits >> 2);
        }
    }
    gu64* __restrict__ rec = counts_of(d, t.t) + wave * SC_PER_WAVE;
#pragma unroll
    for (int i = 0; i < 6; i++) {   // every wave of every block reaches this
        const u64 s = wave_sum((u64)n[i]);
        if (lane == 0) rec[i] = s;
    }
}

// ---- pass 8: one block per page
__global__ void __launch_bounds__(SPECKLE_THREADS)
speckle_info_kernel(const SpeckleDesc* __restrict__ descs) {
    __shared__ u64 part[SPECKLE_WAVES][6];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpeckleDesc d = descs[blockIdx.x];
    const int tiles = d.hw * d.ww;
    u64 sum[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (int t = tid; t < tiles; t += SPECKLE_THREADS) {
        const gu64* __restrict__ c = counts_of(d, t);
#pragma unroll
        for (int wv = 0; wv < SPECKLE_WAVES; wv++)
#pragma unroll
            for (int i = 0; i < 6; i++) sum[i] += c[wv * SC_PER_WAVE + i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        sum[i] = wave_sum(sum[i]);
        if (lane == 0) part[wave][i] = sum[i];
    }
    __syncthreads();
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        u64 all[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            all[i] = 0ull;
#pragma unroll
            for (int k = 0; k < SPECKLE_WAVES; k++) all[i] += part[k][i];
        }
        info->specks = all[SC_SPECKS];
        info->kept = all[SC_KEPT];
        info->speck_pixels = all[SC_SPECK_PX];
        info->kept_pixels = all[SC_KEPT_PX];
        info->holes = all[SC_HOLES];
        info->hole_pixels = all[SC_HOLE_PX];
    }
}

void despeckle_pages(const SpeckleDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(speckle_mask_kernel, dim3(total_blocks), dim3(SPECKLE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(speckle_levels_kernel, dim3(n_pages), dim3(SPECKLE_THREADS), 0, s, d_descs);
    hipLaunchKernelGGL(speckle_merge_kernel, dim3(total_blocks), dim3(SPECKLE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(speckle_area_kernel, dim3(total_blocks), dim3(SPECKLE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(speckle_big_kernel, dim3(total_blocks), dim3(SPECKLE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(speckle_near_kernel, dim3(total_blocks), dim3(SPECKLE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(speckle_map_kernel, dim3(total_blocks), dim3(SPECKLE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(speckle_info_kernel, dim3(n_pages), dim3(SPECKLE_THREADS), 0, s, d_descs);
}

}  // namespace k
}  // namespace ocrs
