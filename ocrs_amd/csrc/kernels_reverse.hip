// Reverse-video repair: the solid dark panels of resident pages that enclose light marks, and what they
// enclose, turned to dark on light by flipping the sign bit of their pixels, for a batch of pages of any mix of sizes and
// parameters.  A code object of its own, as kernels_speckle.hip and kernels_measure.hip are.  tests/reverse_ref.py is the
// definition; everything here is integer and set arithmetic on one set taken from the input page (ink = v < threshold),
// every count a sum of integers, every box a minimum or a maximum, so the result is defined to the bit whatever the
// schedule or batch.  A result pixel is the source's 32-bit word or that word XOR 0x80000000, nothing else.
//
// Two labellings share one forest of page-local int32 pixel indices: first the ink, 8-connected, with areas and boxes at
// the roots (as kernels_measure.hip); then, once the candidates' pixels M are known, everything outside M, 4-connected, with
// areas and an edge flag at the roots (as kernels_frame.hip's cleanup).  The pixels of M keep their ink labels, the others
// are labelled anew; the two classes never unite.
//
// Nine launches on one stream, no host round trip between them.  Every pass but the last takes one block per 64 x 64 tile
// of a page, a lane per pixel and sixteen rows per wave; blocks find their page by bisecting the descriptors' block prefix.
//   1 reverse_mask_kernel        ink = v < threshold, one __ballot per 64 pixels -> the INK bit mask and the count of ink; the
//                                initial labels of the ink: the start of the pixel's run inside its word; area and box words
//                                reset at those starts (a root is one of them).
//   2 reverse_merge_ink_kernel   the unions the initial labels lack, ink only, 8-connected (as measure_merge_kernel).
//   3 reverse_boxes_kernel       the head of every in-word run of ink finds its root; the run takes it by a shuffle and every ink
//                                pixel's label is flattened to the root.  Area and box at the root by atomics, consecutive
//                                heads of one root merged first (as measure_boxes_kernel), and once per wave for the root
//                                the wave meets first (a panel is one component over many tiles).
//   4 reverse_candidates_kernel  a head reads its root's area and box: candidate = bh >= min_height, bw >= min_width and
//                                256 A >= q bh bw in 64-bit integers; the ballot of "my root is a candidate" is the M word.
//                                Components and candidates are counted at their roots.  The initial labels of everything
//                                outside M.  (Nothing that another block reads in this pass is written in it.)
//   5 reverse_merge_rest_kernel  the unions outside M, 4-connected: across words and with the pixel above.  The words of the
//                                second labelling are reset at the heads of the in-word runs: area and edge flag outside M,
//                                the hole counter on M (pass 4 still read them as boxes).
//   6 reverse_rest_area_kernel   outside M: labels flattened to the root, the run's length added to the root's area (once per
//                                wave for the root the wave meets first: the paper around everything); a run that touches the
//                                page's first or last row or column stores 1 to its root's edge flag, an idempotent plain
//                                vector store, as frame_area_kernel does.
//   7 reverse_holes_kernel       every root outside M whose flag is clear is a hole; when it counts (max_hole == 0 or
//                                a <= max_hole) it adds 1 to the counter of its encloser: the root of the pixel west of it.
//   8 reverse_map_kernel         a head decides for its run (panel: counter >= min_holes; hole of a panel), ballots make four
//                                bit words per row in LDS; then the page on 32-bit words, 16 bytes at a time where desc.vec
//                                holds, the byte mask, and the wave's counts into the block's record by plain stores.
//   9 reverse_info_kernel        one block per page: the blocks' records added up -> the page's ReverseInfo.
//
// The only loops that depend on other threads are uf_find / uf_union below (restated from kernels_measure.hip): a parent is
// only ever lowered, by atomicMin at a root, so every chain strictly descends and ends; no block waits for another.
// Visibility between passes comes from the kernel boundaries.  Inside passes 2 and 5 parents are read by agent-scope atomic
// loads and written by atomics alone; inside passes 3 and 6 a flattened label is a plain store of a root, which a concurrent
// find may or may not see: either way it follows a chain of ancestors to the same root, the forest no longer changing.
// Every access is predicated on the page.  The barrier of pass 8 is at the top level and every thread of every block
// reaches it; ballots and shuffles are reached by whole waves.
#include <cmath>

#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int REVERSE_THREADS = 256;
constexpr int REVERSE_WAVES = REVERSE_THREADS / 64;
constexpr int REVERSE_ROWS = 64 / REVERSE_WAVES;   // of a tile, per wave
static_assert(REVERSE_WAVES == 4 && REVERSE_COUNTS == 32, "the layout of a block's counts");

int64_t reverse_tiles(int h, int w) { return (int64_t)((h + 63) / 64) * ((w + 63) / 64); }
size_t reverse_mask_words(int h, int w) { return (size_t)2 * (size_t)h * (size_t)((w + 63) / 64); }
int reverse_fill_q8(float min_fill) { return (int)floorf(256.0f * min_fill + 0.5f); }

namespace {   // what only this file's kernels use

typedef __attribute__((address_space(1))) int32_t gint;
typedef __attribute__((address_space(1))) ReverseInfo ginfo;
typedef uint32_t uint4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint4v gquadw;

// What a page's blocks counted, a record of REVERSE_COUNTS words per block, [wave][8], every word of it written by plain
// stores: RC_INK in pass 1, RC_COMPONENTS and RC_CANDIDATES in pass 4, the rest in pass 8; pass 9 adds them up.
enum { RC_INK = 0, RC_COMPONENTS, RC_CANDIDATES, RC_PANELS, RC_PANEL_PX, RC_HOLES, RC_HOLE_PX, RC_SKIPPED, RC_PER_WAVE = 8 };
__device__ __forceinline__ gu64* counts_of(const ReverseDesc& d, int tile) { return (gu64*)(uintptr_t)d.counts + (size_t)tile * REVERSE_COUNTS; }

__device__ __forceinline__ gu64* ink_mask_of(const ReverseDesc& d) { return (gu64*)(uintptr_t)d.masks; }
__device__ __forceinline__ gu64* m_mask_of(const ReverseDesc& d) { return (gu64*)(uintptr_t)d.masks + (size_t)d.h * (size_t)d.ww; }

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
__device__ __forceinline__ Tile tile_of(const ReverseDesc& d, int b) {
    Tile t;
    t.t = b - d.block0;
    t.ty = t.t / d.ww;
    t.tx = t.t % d.ww;
    t.h = d.h;
    t.w = d.w;
    t.ww = d.ww;
    return t;
}

// bit i of `edges`: pixel i of the word differs from pixel i - 1 (bit 0 always): where the in-word runs start
__device__ __forceinline__ u64 edges_of(u64 word) { return (word ^ (word << 1)) | 1ull; }
__device__ __forceinline__ int run_start(u64 edges, int lane) { return 63 - __builtin_clzll(edges & (~0ull >> (63 - lane))); }
// the length of the in-word run that starts at `lane`, cut at the page's edge (`valid` pixels of the word lie on the page)
__device__ __forceinline__ int run_length(u64 edges, int lane, int valid) {
    const u64 rest = lane == 63 ? 0ull : edges >> (lane + 1);
    const int run = rest ? __builtin_ctzll(rest) + 1 : 64 - lane;
    return lane + run > valid ? valid - lane : run;
}

// bit x of row y of a mask, for -1 <= x - 64 tx <= 64 around the word (y, tx); zero outside the page
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
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_mask_kernel(const ReverseDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gu64* __restrict__ mask = ink_mask_of(d);
    gint* __restrict__ labels = (gint*)(uintptr_t)d.labels;
    gword* __restrict__ area = (gword*)(uintptr_t)d.area;
    gword* __restrict__ bx0 = (gword*)(uintptr_t)d.x0;
    gword* __restrict__ bx1 = (gword*)(uintptr_t)d.x1;
    gword* __restrict__ by1 = (gword*)(uintptr_t)d.y1;
    const int x = t.tx * 64 + lane;
    const float thr = d.threshold;
    float px[REVERSE_ROWS];   // all of them on their way before the first is looked at
#pragma unroll
    for (int i = 0; i < REVERSE_ROWS; i++) {
        const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
        px[i] = y < h && x < w ? src[(int64_t)y * w + x] : 0.0f;
    }
    uint32_t inks = 0;   // uniform in the wave
#pragma unroll
    for (int i = 0; i < REVERSE_ROWS; i++) {   // uniform in the block
        const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
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
    if (lane == 0) counts_of(d, t.t)[wave * RC_PER_WAVE + RC_INK] = (u64)inks;   // every wave of every block
}

// ---- pass 2
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_merge_ink_kernel(const ReverseDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ mask = ink_mask_of(d);
    gint* L = (gint*)(uintptr_t)d.labels;
    const int x = t.tx * 64 + lane;
    for (int i = 0; i < REVERSE_ROWS; i++) {
        const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
        if (y >= h || x >= w) continue;
        const RowBits cur = row_bits(mask, y, t.tx, h, t.ww), up = row_bits(mask, y - 1, t.tx, h, t.ww);
        if (!((cur.word >> lane) & 1ull)) continue;
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

// ---- pass 3
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_boxes_kernel(const ReverseDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ mask = ink_mask_of(d);
    gint* L = (gint*)(uintptr_t)d.labels;
    gword* area = (gword*)(uintptr_t)d.area;
    gword* bx0 = (gword*)(uintptr_t)d.x0;
    gword* bx1 = (gword*)(uintptr_t)d.x1;
    gword* by1 = (gword*)(uintptr_t)d.y1;
    const int x = t.tx * 64 + lane;
    // A panel is one component over many tiles: what the wave's rows add to the root it met first is kept in registers and
    // sent once (as pass 6 and speckle_area_kernel do for the paper; per-series atomics to the one root of an A4 page's
    // band took 489 us in place of the figure of DESIGN.md §7.15).
    int common = -1;   // uniform in the wave
    uint32_t c_area = 0u, c_x0 = 0xFFFFFFFFu, c_x1 = 0u, c_y1 = 0u;
    for (int i = 0; i < REVERSE_ROWS; i++) {   // uniform in the wave: the ballot and the shuffles below are reached by all 64 lanes
        const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
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
        const int mine = __shfl(root, run_start(edges, lane));   // an ink pixel's run starts at a head
        if ((word >> lane) & 1ull) L[y * w + x] = mine;
        if (common < 0) common = __shfl(root, __builtin_ctzll(heads));
        // consecutive runs of a row mostly belong to one component: the first of a series of heads with one root speaks for it
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
            const uint32_t n = (uint32_t)(sum_end - sum + run);
            if (root == common) {
                c_area += n;
                c_x0 = c_x0 < (uint32_t)x ? c_x0 : (uint32_t)x;
                c_x1 = c_x1 > (uint32_t)x1_end ? c_x1 : (uint32_t)x1_end;
                c_y1 = (uint32_t)y;   // the rows ascend
            } else {
                __hip_atomic_fetch_add(&area[root], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_min(&bx0[root], (uint32_t)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(&bx1[root], (uint32_t)x1_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(&by1[root], (uint32_t)y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // every wave reaches this; a lane that added nothing holds the neutral elements
    c_area = (uint32_t)wave_sum((u64)c_area);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o0 = (uint32_t)__shfl_xor((int)c_x0, s), o1 = (uint32_t)__shfl_xor((int)c_x1, s), oy = (uint32_t)__shfl_xor((int)c_y1, s);
        c_x0 = c_x0 < o0 ? c_x0 : o0;
        c_x1 = c_x1 > o1 ? c_x1 : o1;
        c_y1 = c_y1 > oy ? c_y1 : oy;
    }
    if (lane == 0 && common >= 0) {   // a wave with a common root added at least one run to it
        __hip_atomic_fetch_add(&area[common], c_area, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(&bx0[common], c_x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&bx1[common], c_x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&by1[common], c_y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- pass 4
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_candidates_kernel(const ReverseDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ mask = ink_mask_of(d);
    gu64* __restrict__ m_mask = m_mask_of(d);
    gint* __restrict__ L = (gint*)(uintptr_t)d.labels;   // read and written at this thread's own pixel alone
    const gword* __restrict__ area = (const gword*)(uintptr_t)d.area;
    const gword* __restrict__ bx0 = (const gword*)(uintptr_t)d.x0;
    const gword* __restrict__ bx1 = (const gword*)(uintptr_t)d.x1;
    const gword* __restrict__ by1 = (const gword*)(uintptr_t)d.y1;
    const int x = t.tx * 64 + lane;
    const uint32_t min_h = (uint32_t)d.min_height, min_w = (uint32_t)d.min_width;
    const u64 q = (u64)d.fill_q8;
    uint32_t comps = 0, cands = 0;   // uniform in the wave
    for (int i = 0; i < REVERSE_ROWS; i++) {   // uniform in the wave
        const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
        if (y >= h) continue;
        const u64 word = mask[(size_t)y * t.ww + t.tx];
        const u64 edges = edges_of(word);
        const bool ink = (word >> lane) & 1ull, head = ink && ((edges >> lane) & 1ull);
        const int p = y * w + x;
        bool cand = false, is_root = false;
        if (head) {   // pass 3 flattened the labels of ink: this is the root
            const int root = L[p];
            const uint32_t a = area[root], bh = by1[root] - (uint32_t)(root / w) + 1u, bw = bx1[root] - bx0[root] + 1u;
            cand = bh >= min_h && bw >= min_w && 256ull * (u64)a >= q * (u64)bh * (u64)bw;   // q bh bw < 2^41
            is_root = root == p;
        }
        const int of_run = __shfl((int)cand, run_start(edges, lane));
        const u64 m_word = __ballot(ink && of_run);
        comps += (uint32_t)__builtin_popcountll(__ballot(is_root));
        cands += (uint32_t)__builtin_popcountll(__ballot(is_root && cand));
        // everything outside M is labelled anew: the start of the pixel's run of equal M bits inside the word
        if (x < w && !((m_word >> lane) & 1ull)) L[p] = p - (lane - run_start(edges_of(m_word), lane));
        if (lane == 0) m_mask[(size_t)y * t.ww + t.tx] = m_word;
    }
    if (lane == 0) {   // every wave of every block
        gu64* __restrict__ rec = counts_of(d, t.t) + wave * RC_PER_WAVE;
        rec[RC_COMPONENTS] = (u64)comps;
        rec[RC_CANDIDATES] = (u64)cands;
    }
}

// ---- pass 5
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_merge_rest_kernel(const ReverseDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ m_mask = m_mask_of(d);
    gint* L = (gint*)(uintptr_t)d.labels;
    gword* __restrict__ area = (gword*)(uintptr_t)d.area;
    gword* __restrict__ edge_flag = (gword*)(uintptr_t)d.x0;
    gword* __restrict__ hole_count = (gword*)(uintptr_t)d.x1;
    const int x = t.tx * 64 + lane;
    for (int i = 0; i < REVERSE_ROWS; i++) {
        const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
        if (y >= h || x >= w) continue;
        const RowBits cur = row_bits(m_mask, y, t.tx, h, t.ww), up = row_bits(m_mask, y - 1, t.tx, h, t.ww);
        const int p = y * w + x;
        const bool in_m = (cur.word >> lane) & 1ull;
        if ((edges_of(cur.word) >> lane) & 1ull) {   // the head of an in-word run: a root of either class is one
            if (in_m) {
                hole_count[p] = 0u;
            } else {
                area[p] = 0u;
                edge_flag[p] = 0u;
            }
        }
        if (in_m) continue;
        // whether a neighbour lies outside M; a zero bit past the page's edge is no neighbour
        const bool oW = x > 0 && !(lane > 0 ? (cur.word >> (lane - 1)) & 1ull : cur.left != 0u);
        const bool oN = y > 0 && !((up.word >> lane) & 1ull);
        const bool oNW = x > 0 && y > 0 && !(lane > 0 ? (up.word >> (lane - 1)) & 1ull : up.left != 0u);
        if (lane == 0 && oW) uf_union(L, p, p - 1);   // the run goes on from the word before
        if (oN && !(oW && oNW)) uf_union(L, p, p - w);   // 4-connectivity: N, unless W and NW already carry it
    }
}

// ---- pass 6
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_rest_area_kernel(const ReverseDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ m_mask = m_mask_of(d);
    gint* L = (gint*)(uintptr_t)d.labels;
    gword* area = (gword*)(uintptr_t)d.area;
    gword* __restrict__ edge_flag = (gword*)(uintptr_t)d.x0;
    const int x = t.tx * 64 + lane;
    const int valid = w - t.tx * 64 >= 64 ? 64 : w - t.tx * 64;   // pixels of the word that lie on the page
    // Most runs of a tile belong to one component, the paper around everything: what the wave's rows add to the root it met
    // first is kept in registers and added once (DESIGN.md §7.9 has what a per-run add to that one word costs).
    int common = -1;          // uniform in the wave
    uint32_t common_sum = 0;
    for (int i = 0; i < REVERSE_ROWS; i++) {   // uniform in the wave
        const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
        if (y >= h) continue;
        const u64 word = m_mask[(size_t)y * t.ww + t.tx];
        const u64 edges = edges_of(word);
        const bool rest = x < w && !((word >> lane) & 1ull), head = rest && ((edges >> lane) & 1ull);
        const u64 heads = __ballot(head);
        if (!heads) continue;   // a word of M
        const int p = y * w + x;
        const int found = head ? uf_find(L, p) : 0;
        const int root = __shfl(found, run_start(edges, lane));   // a pixel outside M: its run starts at a head
        if (rest) L[p] = root;
        if (common < 0) common = __shfl(found, __builtin_ctzll(heads));
        if (head) {
            const int run = run_length(edges, lane, valid);
            if (root == common) common_sum += (uint32_t)run;
            else __hip_atomic_fetch_add(&area[root], (uint32_t)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // the same 1 from whoever finds it
            if (y == 0 || y == h - 1 || x == 0 || x + run == w) edge_flag[root] = 1u;
        }
    }
    const uint32_t total = (uint32_t)wave_sum((u64)common_sum);   // every wave reaches this
    if (lane == 0 && common >= 0) __hip_atomic_fetch_add(&area[common], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pass 7
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_holes_kernel(const ReverseDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gu64* __restrict__ m_mask = m_mask_of(d);
    const gint* __restrict__ L = (const gint*)(uintptr_t)d.labels;
    const gword* __restrict__ area = (const gword*)(uintptr_t)d.area;
    const gword* __restrict__ edge_flag = (const gword*)(uintptr_t)d.x0;
    gword* hole_count = (gword*)(uintptr_t)d.x1;
    const int x = t.tx * 64 + lane;
    const uint32_t max_hole = (uint32_t)d.max_hole;
    for (int i = 0; i < REVERSE_ROWS; i++) {
        const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
        if (y >= h || x >= w) continue;
        const u64 word = m_mask[(size_t)y * t.ww + t.tx];
        if (((word >> lane) & 1ull) || !((edges_of(word) >> lane) & 1ull)) continue;   // a root is the head of a run outside M
        const int p = y * w + x;
        if (L[p] != p || edge_flag[p]) continue;
        // A hole: it holds no pixel of column 0, so p - 1 is on this row, and p is the hole's raster-first pixel, so p - 1
        // is not of the hole: it is in M, where pass 3 left the root of its candidate.
        if (max_hole == 0u || area[p] <= max_hole)
            __hip_atomic_fetch_add(&hole_count[L[p - 1]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- pass 8
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_map_kernel(const ReverseDesc* __restrict__ descs, int n_pages) {
    enum { B_FLIP = 0, B_M, B_PANEL, B_HOLE, B_WORDS };   // the bits of the byte mask, in its order
    __shared__ u64 rows[B_WORDS][64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[find_desc(descs, n_pages, b)];
    const Tile t = tile_of(d, b);
    const int h = t.h, w = t.w;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ dst = (gword*)(uintptr_t)d.dst;
    gbyte* __restrict__ bytes = (gbyte*)(uintptr_t)d.mask_out;
    const gu64* __restrict__ m_mask = m_mask_of(d);
    const gint* __restrict__ L = (const gint*)(uintptr_t)d.labels;
    const gword* __restrict__ area = (const gword*)(uintptr_t)d.area;
    const gword* __restrict__ edge_flag = (const gword*)(uintptr_t)d.x0;
    const gword* __restrict__ hole_count = (const gword*)(uintptr_t)d.x1;
    const uint32_t max_hole = (uint32_t)d.max_hole, min_holes = (uint32_t)d.min_holes;
    // the page's words on their way before the sets are looked up
    uint4v quad[4];
    uint32_t px[REVERSE_ROWS];
    if (d.vec) {   // uniform in the block; w % 4 == 0: x < w means x + 3 < w
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = i * REVERSE_THREADS + tid, y = t.ty * 64 + (q >> 4), x = t.tx * 64 + 4 * (q & 15);
            const uint4v none = {0u, 0u, 0u, 0u};
            quad[i] = y < h && x < w ? *(const gquadw*)(src + (int64_t)y * w + x) : none;
        }
    } else {
        const int x = t.tx * 64 + lane;
#pragma unroll
        for (int i = 0; i < REVERSE_ROWS; i++) {
            const int y = t.ty * 64 + i * REVERSE_WAVES + wave;
            px[i] = y < h && x < w ? src[(int64_t)y * w + x] : 0u;
        }
    }
    // what each pixel is, decided at the head of its in-word run of equal M bits
    uint32_t n_panels = 0, n_panel_px = 0, n_holes = 0, n_hole_px = 0, n_skipped = 0;   // uniform in the wave
    {
        const int x = t.tx * 64 + lane;
        for (int i = 0; i < REVERSE_ROWS; i++) {   // uniform in the wave
            const int r = i * REVERSE_WAVES + wave, y = t.ty * 64 + r;
            u64 flips = 0ull, word = 0ull, panels = 0ull, holes = 0ull;
            if (y < h) {
                word = m_mask[(size_t)y * t.ww + t.tx];
                const u64 edges = edges_of(word);
                const bool in_m = (word >> lane) & 1ull, head = x < w && ((edges >> lane) & 1ull);
                const int p = y * w + x;
                // bit 0: a panel's pixel, 1: a hole's, 2: the hole counts, 3: its encloser is a panel, 4: this is the root
                uint32_t bits = 0u;
                if (head) {
                    const int root = L[p];   // flattened: by pass 3 on M, by pass 6 outside it
                    if (in_m) {
                        bits = hole_count[root] >= min_holes ? 1u : 0u;
                    } else if (!edge_flag[root]) {
                        bits = 2u;
                        if (max_hole == 0u || area[root] <= max_hole) bits |= 4u;
                        if (hole_count[L[root - 1]] >= min_holes) bits |= 8u;   // root - 1 is in M: see pass 7
                    }
                    if (root == p) bits |= 16u;
                }
                const uint32_t mine = (uint32_t)__shfl((int)bits, run_start(edges, lane));   // past the page's edge: a run outside M
                const bool on = x < w, panel = on && (mine & 1u), hole = on && (mine & 2u), flipped = on && (mine & 14u) == 14u;
                panels = __ballot(panel);
                holes = __ballot(hole);
                flips = panels | __ballot(flipped);
                n_panels += (uint32_t)__builtin_popcountll(__ballot(head && (bits & 17u) == 17u));
                n_holes += (uint32_t)__builtin_popcountll(__ballot(head && (bits & 30u) == 30u));
                n_skipped += (uint32_t)__builtin_popcountll(__ballot(head && (bits & 30u) == 26u));
                n_panel_px += (uint32_t)__builtin_popcountll(panels);
                n_hole_px += (uint32_t)__builtin_popcountll(flips & ~panels);
            }
            if (lane == 0) {
                rows[B_FLIP][r] = flips;
                rows[B_M][r] = word;
                rows[B_PANEL][r] = panels;
                rows[B_HOLE][r] = holes;
            }
        }
    }
    __syncthreads();
    if (d.vec) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = i * REVERSE_THREADS + tid, r = q >> 4, c = 4 * (q & 15), y = t.ty * 64 + r, x = t.tx * 64 + c;
            if (y >= h || x >= w) continue;
            const int at = y * w + x;
            uint32_t set[B_WORDS];
#pragma unroll
            for (int m = 0; m < B_WORDS; m++) set[m] = (uint32_t)(rows[m][r] >> c) & 15u;
            uint4v v = quad[i];
            uint32_t packed = 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                v[k] ^= ((set[B_FLIP] >> k) & 1u) << 31;
#pragma unroll
                for (int m = 0; m < B_WORDS; m++) packed |= ((set[m] >> k) & 1u) << (8 * k + m);
            }
            *(gquadw*)(dst + at) = v;
            if (bytes) *(gword*)(bytes + at) = packed;   // at % 4 == 0
        }
    } else {
        const int x = t.tx * 64 + lane;
#pragma unroll
        for (int i = 0; i < REVERSE_ROWS; i++) {
            const int r = i * REVERSE_WAVES + wave, y = t.ty * 64 + r;
            if (y >= h || x >= w) continue;
            const int at = y * w + x;
            uint32_t byte = 0u;
#pragma unroll
            for (int m = 0; m < B_WORDS; m++) byte |= ((uint32_t)(rows[m][r] >> lane) & 1u) << m;
            dst[at] = px[i] ^ ((byte & 1u) << 31);
            if (bytes) bytes[at] = (uint8_t)byte;
        }
    }
    if (lane == 0) {   // every wave of every block
        gu64* __restrict__ rec = counts_of(d, t.t) + wave * RC_PER_WAVE;
        rec[RC_PANELS] = (u64)n_panels;
        rec[RC_PANEL_PX] = (u64)n_panel_px;
        rec[RC_HOLES] = (u64)n_holes;
        rec[RC_HOLE_PX] = (u64)n_hole_px;
        rec[RC_SKIPPED] = (u64)n_skipped;
    }
}

// ---- pass 9: one block per page
__global__ void __launch_bounds__(REVERSE_THREADS)
reverse_info_kernel(const ReverseDesc* __restrict__ descs) {
    __shared__ u64 part[REVERSE_WAVES][RC_PER_WAVE];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ReverseDesc d = descs[blockIdx.x];
    const int tiles = d.hw * d.ww;
    u64 sum[RC_PER_WAVE] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (int t = tid; t < tiles; t += REVERSE_THREADS) {
        const gu64* __restrict__ c = counts_of(d, t);
#pragma unroll
        for (int wv = 0; wv < REVERSE_WAVES; wv++)
#pragma unroll
            for (int i = 0; i < RC_PER_WAVE; i++) sum[i] += c[wv * RC_PER_WAVE + i];
    }
#pragma unroll
    for (int i = 0; i < RC_PER_WAVE; i++) {
        sum[i] = wave_sum(sum[i]);
        if (lane == 0) part[wave][i] = sum[i];
    }
    __syncthreads();
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        u64 all[RC_PER_WAVE];
#pragma unroll
        for (int i = 0; i < RC_PER_WAVE; i++) {
            all[i] = 0ull;
#pragma unroll
            for (int k = 0; k < REVERSE_WAVES; k++) all[i] += part[k][i];
        }
        info->ink = all[RC_INK];
        info->components = all[RC_COMPONENTS];
        info->candidates = all[RC_CANDIDATES];
        info->panels = all[RC_PANELS];
        info->panel_pixels = all[RC_PANEL_PX];
        info->holes = all[RC_HOLES];
        info->hole_pixels = all[RC_HOLE_PX];
        info->skipped_holes = all[RC_SKIPPED];
        info->inverted = all[RC_PANEL_PX] + all[RC_HOLE_PX];
    }
}

void unreverse_pages(const ReverseDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(reverse_mask_kernel, dim3(total_blocks), dim3(REVERSE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(reverse_merge_ink_kernel, dim3(total_blocks), dim3(REVERSE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(reverse_boxes_kernel, dim3(total_blocks), dim3(REVERSE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(reverse_candidates_kernel, dim3(total_blocks), dim3(REVERSE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(reverse_merge_rest_kernel, dim3(total_blocks), dim3(REVERSE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(reverse_rest_area_kernel, dim3(total_blocks), dim3(REVERSE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(reverse_holes_kernel, dim3(total_blocks), dim3(REVERSE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(reverse_map_kernel, dim3(total_blocks), dim3(REVERSE_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(reverse_info_kernel, dim3(n_pages), dim3(REVERSE_THREADS), 0, s, d_descs);
}

}  // namespace k
}  // namespace ocrs
