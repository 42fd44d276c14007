// Adaptive binarisation: Sauvola's local threshold in exact integers, for a batch of resident pages of
// any mix of sizes and parameters.  A code object of its own, as kernels_speckle.hip is.  tests/binarize_ref.py is the
// definition; the window sums are plain sums of integers and the decision is a comparison of integers of up to 128 bits,
// so the result is defined to the bit whatever the schedule or batch.  No floating-point arithmetic decides anything: the
// only float operations are those of the bin of a pixel (§7.4), restated here.
//
// With r the radius, kq Sauvola's k in 1/256 and R = 128: over the counted (not NaN) pixels of the window
// [y - r, y + r] x [x - r, x + r] clipped to the page, n is their number, S the sum of their bins and Q the sum of the
// squares of their bins.  V = n Q - S^2, A = n R (256 (b n - S) + kq S), B = kq S;  ink <=> A < 0 or A^2 < B^2 V.
//
// Three launches on one stream, no host round trip between them; blocks find their page by bisecting a block prefix of the
// descriptors (row_block0 in pass 1, block0 in pass 2).
//   1 bin_rows_kernel   one read of the page.  A wave owns a row and walks it in rounds of 64 pixels, a lane per pixel: the
//                       bin, an inclusive scan of (n, S, Q) by shuffles, a carry between rounds.  The prefixes go through
//                       a ring of 512 entries per wave in LDS; two rounds later, when the prefix at x + r is there, the
//                       lane of pixel x differences the ring at x + r and x - r - 1 (clipped to the row: the edge is a
//                       wall) and writes the row sums packed in 8 bytes: n << 16 | S, and Q.  The prefixes are kept modulo
//                       2^32 per field; a difference is at most 255, 65 025 and 16 581 375, so it is exact.  No halo is
//                       read twice and the cost does not depend on r.
//   2 bin_cols_kernel   a block owns a strip of 256 columns and a segment of seg_rows rows, a lane per column.  The lane
//                       sums the row records of the window of its first row, then slides: add row y + r, decide, subtract
//                       row y - r.  Every access is coalesced across the lanes.  Per row: the 128-bit decision, the output
//                       word, the mask byte, the counts; summed over the wave into the block's record by plain stores.
//   3 bin_info_kernel   one block per page: the blocks' records added up -> the page's BinInfo.
//
// Loads and stores are one dword (page, pass 1 and 2), one 8-byte record (row sums) or one byte (mask) per lane, consecutive
// across the wave: a lane per pixel is what the scan of pass 1 and the slide of pass 2 are made of, so neither uses 16-byte
// accesses.  Every access is predicated on the page.  The one barrier is in the round loop of pass 1, whose trip count is
// the same for every thread of the block (it depends on the page width alone); shuffles are reached by whole waves.
#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int BIN_THREADS = 256;
constexpr int BIN_WAVES = BIN_THREADS / 64;
constexpr int BIN_RING = 512;   // prefixes a wave keeps: those of the 2 rounds in flight and of the 127 pixels before them
static_assert(BIN_WAVES == BIN_ROWS && BIN_THREADS == BIN_STRIP && BIN_COUNTS == 2 * BIN_WAVES, "the layout of a block");
static_assert(2 * 64 + 64 + BIN_MAX_RADIUS + 1 <= BIN_RING, "the ring holds what a delayed round reads");

typedef __attribute__((address_space(1))) BinInfo ginfo;
typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) uint2v gpair;

int bin_seg_rows(int h, int w, int radius) {
    // The run-in of a segment is 2r + 1 rows of records.  A segment as long as its run-in (rounded up to 32 rows) keeps the
    // records read per pixel at about two; a page that this leaves with fewer than 64 blocks gets shorter segments (halved,
    // not under 32 rows), since a block's rows are walked one after the other and an idle CU costs more than a longer run-in.
    int rows = (2 * radius + 1 + 31) / 32 * 32;
    const int strips = (w + BIN_STRIP - 1) / BIN_STRIP;
    while (rows > 32 && (int64_t)strips * ((h + rows - 1) / rows) < 64) rows /= 2;
    return rows < h ? rows : h;
}
int64_t bin_col_blocks(int h, int w, int radius) {
    const int rows = bin_seg_rows(h, w, radius);
    return (int64_t)((w + BIN_STRIP - 1) / BIN_STRIP) * ((h + rows - 1) / rows);
}
int64_t bin_row_blocks(int h) { return (h + BIN_ROWS - 1) / BIN_ROWS; }

// ---- pass 1
__global__ void __launch_bounds__(BIN_THREADS)
bin_rows_kernel(const BinDesc* __restrict__ descs, int n_pages) {
    __shared__ uint32_t ring[BIN_WAVES][3][BIN_RING];   // prefix i of the row (the sums of pixels 0 .. i - 1) at i % BIN_RING
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BinDesc d = descs[find_desc(descs, n_pages, b, &BinDesc::row_block0)];
    const int h = d.h, w = d.w, r = d.radius;
    const int y = (b - d.row_block0) * BIN_ROWS + wave;
    const bool row = y < h;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    gpair* __restrict__ sums = (gpair*)(uintptr_t)d.sums;
    uint32_t* __restrict__ pn = ring[wave][0];
    uint32_t* __restrict__ ps = ring[wave][1];
    uint32_t* __restrict__ pq = ring[wave][2];
    if (lane == 0) {
        pn[0] = 0u;
        ps[0] = 0u;
        pq[0] = 0u;
    }
    const int rounds = (w + 63) / 64;
    uint32_t cn = 0u, cs = 0u, cq = 0u;   // the carry: the sums of the rounds before, uniform in the wave
    for (int c = 0; c < rounds + 2; c++) {   // uniform in the block
        if (c < rounds) {   // uniform in the block
            const int x = c * 64 + lane;
            const bool in = row && x < w;
            const float v = in ? src[(int64_t)y * w + x] : __uint_as_float(0x7fc00000u);
            const int bin = bin_of(clamp01(v + 0.5f));
            uint32_t n = bin >= 0 ? 1u : 0u, s = bin >= 0 ? (uint32_t)bin : 0u, q = s * s;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {   // inclusive scan over the wave
                const uint32_t an = (uint32_t)__shfl_up((int)n, k), as = (uint32_t)__shfl_up((int)s, k), aq = (uint32_t)__shfl_up((int)q, k);
                if (lane >= k) {
                    n += an;
                    s += as;
                    q += aq;
                }
            }
            n += cn;
            s += cs;
            q += cq;
            const int at = (x + 1) & (BIN_RING - 1);
            pn[at] = n;
            ps[at] = s;
            pq[at] = q;
            cn = (uint32_t)__shfl((int)n, 63);
            cs = (uint32_t)__shfl((int)s, 63);
            cq = (uint32_t)__shfl((int)q, 63);
        }
        __syncthreads();   // the prefixes up to pixel 64 c + 63 are in the ring
        if (c >= 2) {
            const int x = (c - 2) * 64 + lane;
            if (row && x < w) {
                const int lo = x - r < 0 ? 0 : x - r;                   // the first pixel of the window
                const int hi = x + r > w - 1 ? w : x + r + 1;           // one past its last: <= 64 c + 64
                const int a = lo & (BIN_RING - 1), e = hi & (BIN_RING - 1);
                const uint32_t n = pn[e] - pn[a], s = ps[e] - ps[a], q = pq[e] - pq[a];
                uint2v rec;
                rec.x = n << 16 | s;   // n <= 255, s <= 65 025
                rec.y = q;
                sums[(int64_t)y * w + x] = rec;
            }
        }
    }
}

// ---- pass 2
// The local rule on the window sums (the header of this file); b: the pixel's bin.
__device__ __forceinline__ bool is_ink(uint32_t b, uint32_t n, uint32_t S, uint32_t Q, uint32_t kq) {
    const u64 V = (u64)n * Q - (u64)S * S;                                          // < 2^48
    const int64_t t = 256 * ((int64_t)b * n - (int64_t)S) + (int64_t)((u64)kq * S);   // |t| < 2^33
    const int64_t A = (int64_t)n * 128 * t;                                         // |A| < 2^56
    if (A < 0) return true;
    const u64 B = (u64)kq * S, B2 = B * B;                                          // B < 2^32
    const u64 a = (u64)A;
    const u64 lhs_hi = __umul64hi(a, a), lhs_lo = a * a, rhs_hi = __umul64hi(B2, V), rhs_lo = B2 * V;
    return lhs_hi < rhs_hi || (lhs_hi == rhs_hi && lhs_lo < rhs_lo);
}

__global__ void __launch_bounds__(BIN_THREADS)
bin_cols_kernel(const BinDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BinDesc d = descs[find_desc(descs, n_pages, b)];
    const int h = d.h, w = d.w, r = d.radius;
    const int t = b - d.block0, seg = t / d.strips, strip = t % d.strips;
    const int x = strip * BIN_STRIP + tid;
    const bool in = x < w;
    const int y0 = seg * d.seg_rows, y1 = y0 + d.seg_rows < h ? y0 + d.seg_rows : h;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ dst = (gword*)(uintptr_t)d.dst;
    gbyte* __restrict__ bytes = (gbyte*)(uintptr_t)d.mask_out;
    const gpair* __restrict__ sums = (const gpair*)(uintptr_t)d.sums;
    const uint32_t kq = (uint32_t)d.kq, ink_bits = d.ink_bits, paper_bits = d.paper_bits;
    const bool keep_ink = d.keep_ink != 0;
    const uint2v none = {0u, 0u};
    uint32_t n = 0u, S = 0u, Q = 0u;   // over the window of the row at hand: n <= 65 025, S < 2^24, Q < 2^32
    {   // the window of row y0 but for its last row, which the loop below adds
        const int a0 = y0 - r < 0 ? 0 : y0 - r, a1 = y0 + r < h ? y0 + r : h;
#pragma unroll 8
        for (int yy = a0; yy < a1; yy++) {   // uniform in the block
            const uint2v rec = in ? sums[(int64_t)yy * w + x] : none;
            n += rec.x >> 16;
            S += rec.x & 0xffffu;
            Q += rec.y;
        }
    }
    uint32_t counted = 0u, inks = 0u;
#pragma unroll 2
    for (int y = y0; y < y1; y++) {   // uniform in the block
        const uint2v add = in && y + r < h ? sums[(int64_t)(y + r) * w + x] : none;
        const uint2v sub = in && y - r >= 0 ? sums[(int64_t)(y - r) * w + x] : none;
        const uint32_t word = in ? src[(int64_t)y * w + x] : 0x7fc00000u;
        n += add.x >> 16;
        S += add.x & 0xffffu;
        Q += add.y;
        const int bin = bin_of(clamp01(__uint_as_float(word) + 0.5f));
        const bool ink = bin >= 0 && is_ink((uint32_t)bin, n, S, Q, kq);
        if (in) {
            const int64_t at = (int64_t)y * w + x;
            dst[at] = bin < 0 ? word : ink ? (keep_ink ? word : ink_bits) : paper_bits;
            if (bytes) bytes[at] = ink ? (uint8_t)1 : (uint8_t)0;
        }
        counted += bin >= 0 ? 1u : 0u;
        inks += ink ? 1u : 0u;
        n -= sub.x >> 16;
        S -= sub.x & 0xffffu;
        Q -= sub.y;
    }
    // every wave of every block reaches this
    const u64 all = wave_sum((u64)counted), dark = wave_sum((u64)inks);
    if (lane == 0) {
        gu64* __restrict__ rec = (gu64*)(uintptr_t)d.counts + (size_t)t * BIN_COUNTS + wave * 2;
        rec[0] = all;
        rec[1] = dark;
    }
}

// ---- pass 3: one block per page
__global__ void __launch_bounds__(BIN_THREADS)
bin_info_kernel(const BinDesc* __restrict__ descs) {
    __shared__ u64 part[BIN_WAVES][2];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BinDesc d = descs[blockIdx.x];
    const int blocks = d.strips * d.segs;
    const gu64* __restrict__ counts = (const gu64*)(uintptr_t)d.counts;
    u64 all = 0ull, dark = 0ull;
    for (int t = tid; t < blocks; t += BIN_THREADS) {
        const gu64* __restrict__ c = counts + (size_t)t * BIN_COUNTS;
#pragma unroll
        for (int wv = 0; wv < BIN_WAVES; wv++) {
            all += c[wv * 2];
            dark += c[wv * 2 + 1];
        }
    }
    all = wave_sum(all);
    dark = wave_sum(dark);
    if (lane == 0) {
        part[wave][0] = all;
        part[wave][1] = dark;
    }
    __syncthreads();
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        u64 s0 = 0ull, s1 = 0ull;
#pragma unroll
        for (int k = 0; k < BIN_WAVES; k++) {
            s0 += part[k][0];
            s1 += part[k][1];
        }
        info->counted = s0;
        info->ink = s1;
        info->ink_fill = __uint_as_float(d.ink_bits);
        info->paper_fill = __uint_as_float(d.paper_bits);
    }
}

void binarize_pages(const BinDesc* d_descs, int n_pages, int row_blocks, int col_blocks, hipStream_t s) {
    if (n_pages <= 0 || row_blocks <= 0 || col_blocks <= 0) return;
    hipLaunchKernelGGL(bin_rows_kernel, dim3(row_blocks), dim3(BIN_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(bin_cols_kernel, dim3(col_blocks), dim3(BIN_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(bin_info_kernel, dim3(n_pages), dim3(BIN_THREADS), 0, s, d_descs);
}

}  // namespace k
}  // namespace ocrs
