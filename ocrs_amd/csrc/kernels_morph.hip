// Stroke repair: grey-level morphology over a rectangle, for a batch of resident pages of any mix of
// sizes, ops and radii.  A code object of its own, as kernels_binarize.hip is.  tests/morph_ref.py is the definition.  A
// minimum or a maximum picks one of its inputs, so the result is the 32-bit word of some pixel of the source and is
// defined to the bit whatever the schedule or batch.  No floating-point instruction touches a pixel: words are ordered
// through the key  k(w) = ~w if the sign bit is set, else w | 0x80000000,  an order on every word that is not NaN with
// -0.0 under +0.0 and the denormals in their places.  The keys 0 and ~0 belong to NaN words alone.
//
// A stage is `lo` (the least key of the window) or `hi` (the greatest).  Both run as the least of k ^ flip, flip = 0 for lo
// and ~0 for hi, with ~0 as the empty key: what a NaN pixel and every place beyond the page edge hold, the identity of the
// minimum.  The window [y - ry, y + ry] x [x - rx, x + rx] is taken rows first, then columns; the row result is kept at
// every pixel, NaN ones included (there it is the extremum of the counted pixels to both sides, or empty), which is what
// makes the two passes equal to the rectangle.  A NaN pixel is known from the source page and keeps its word.
//
// At most five launches on one stream, no host round trip between them: rows and columns of stage 1, rows and columns of
// stage 2 (blocks of the pages of close and open only), the counts.  Blocks find their page by bisecting a block prefix of
// the descriptors; a page without blocks in a launch shares its prefix with the next page and is never found.
//   morph_rows_kernel   a block owns 4 rows x 256 columns, a wave per row.  The wave stages the keys of its 256 pixels and
//                       of rx more to either side in LDS, six per lane, and doubles: after step j an entry holds the least
//                       of 2^(j+1) keys from its place on.  With 2^p <= 2 rx + 1 < 2^(p+1) the window is the union of the
//                       two spans of 2^p keys that start at x - rx and end at x + rx: an extremum does not mind the
//                       overlap.  p <= 6 steps whatever the radius; what grows with rx is the halo, 2 rx of 256 + 2 rx.
//   morph_cols_kernel   a block is one wave that owns a strip of 64 columns and a segment of seg_rows rows, a lane per
//                       column, every access coalesced across the lanes.  van Herk / Gil-Werman down the column in blocks
//                       of 2 ry + 1 rows: the suffix extrema of a block go to the lane's column of an LDS array (sized
//                       statically for radius 63, or 31, or 7, by the largest ry of the batch: the smaller, the more waves a
//                       CU holds), the prefix extrema of the next block run in a register, and the window of row c is
//                       suffix[c - ry] with prefix[c + ry]: three comparisons a pixel.  The keys read for the prefix are
//                       left in the LDS slots already used up, so the next block's suffix pass reads one new row only:
//                       every key is read once, but for the 2 ry rows of run-in of a segment.  Loads go out eight rows at a
//                       time ahead of their use.  The last stage of a page also writes the mask byte and counts; the wave's
//                       sums go to the block's record by plain stores.
//   morph_info_kernel   one block per page: the blocks' records added up in a fixed order -> the page's MorphInfo.
//
// Loads and stores are one dword or one byte per lane, consecutive across the wave; the doubling and the column walk are
// made of a lane per pixel, so the 16-byte path is not used.  Every access is predicated on the page.  Barriers are in
// morph_rows_kernel alone, in loops whose trip count depends on the page's rx: the same for every thread of the block.
#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int MORPH_ROW_THREADS = 256;
constexpr int MORPH_STAGED = 384;                        // keys a wave stages: MORPH_SEG and the halo, a multiple of 64
constexpr int MORPH_PER_LANE = MORPH_STAGED / 64;
constexpr int MORPH_WINDOW = 2 * MORPH_MAX_RADIUS + 1;   // rows of a van Herk block at the largest radius
constexpr int MORPH_WINDOW_S = 15, MORPH_WINDOW_M = 63;  // ... at ry <= 7 and ry <= 31: less LDS, more waves on a CU
constexpr int MORPH_CHUNK = 8;                           // rows whose loads the vertical pass has in flight together
constexpr uint32_t MORPH_EMPTY = 0xffffffffu;
static_assert(MORPH_ROW_THREADS == 64 * MORPH_ROWS, "a wave per row");
static_assert(MORPH_SEG % 64 == 0 && MORPH_SEG + 2 * MORPH_MAX_RADIUS <= MORPH_STAGED, "the staged row holds the segment and its halo");
static_assert(MORPH_STRIP == 64, "a block of the vertical pass is one wave");
static_assert(MORPH_WINDOW * MORPH_STRIP * 4 <= 64 * 1024, "the suffix array fits the static LDS of a block");

typedef __attribute__((address_space(1))) MorphInfo ginfo;

int morph_seg_rows(int h, int w, int ry) {
    // A segment reads 2 ry rows of run-in beside its own.  Segments of at least two windows and some 256 rows keep that
    // share small; a page that this leaves with fewer than 256 blocks gets shorter segments (halved, not under one window),
    // since a block is one wave that walks its rows one after the other and idle CUs cost more than a longer run-in.  The
    // page is then cut into equal segments of about that length, so that no block is left with a few rows and a whole run-in.
    const int win = 2 * ry + 1;
    int m = (256 + win - 1) / win;
    if (m < 2) m = 2;
    const int strips = (w + MORPH_STRIP - 1) / MORPH_STRIP;
    while (m > 1 && (int64_t)strips * ((h + m * win - 1) / (m * win)) < 256) m /= 2;
    int segs = (2 * h + m * win) / (2 * m * win);   // h / (m win), rounded
    if (segs < 1) segs = 1;
    return (h + segs - 1) / segs;
}
int64_t morph_col_blocks(int h, int w, int ry) {
    const int rows = morph_seg_rows(h, w, ry);
    return (int64_t)((w + MORPH_STRIP - 1) / MORPH_STRIP) * ((h + rows - 1) / rows);
}
int64_t morph_row_blocks(int h, int w) { return (int64_t)((h + MORPH_ROWS - 1) / MORPH_ROWS) * ((w + MORPH_SEG - 1) / MORPH_SEG); }

// block b belongs to the last descriptor whose prefix `first` is <= b.  This is find_desc.hpp's member-pointer form, kept
// as a function of its own: with both searches of morph_cols_kernel going through find_desc the compiler folds them into
// one loop and the kernel's code changes, which would need measuring again.
__device__ __forceinline__ int find_by(const MorphDesc* __restrict__ descs, int n, int b, int32_t MorphDesc::*first) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].*first <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool is_nan_word(uint32_t w) { return (w & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ uint32_t key_of(uint32_t w) { return (w & 0x80000000u) ? ~w : (w | 0x80000000u); }
__device__ __forceinline__ uint32_t word_of(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }
// under 0.0f, for a word that is not NaN: -0.0 is not, a negative denormal is
__device__ __forceinline__ bool is_dark_word(uint32_t w) { return w > 0x80000000u; }
__device__ __forceinline__ uint32_t least(uint32_t a, uint32_t b) { return a < b ? a : b; }

// sum over the wave of 32-bit counts (page_device.hpp has the 64-bit one); all 64 lanes call it together
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// ---- the horizontal pass of stage `stage` (0 or 1)
__global__ void __launch_bounds__(MORPH_ROW_THREADS)
morph_rows_kernel(const MorphDesc* __restrict__ descs, int n_pages, int stage) {
    __shared__ uint32_t staged[MORPH_ROWS][MORPH_STAGED];   // entry s of a wave: the pixel at x0 - rx + s of its row
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MorphDesc d = descs[find_by(descs, n_pages, b, stage ? &MorphDesc::row_block0_2 : &MorphDesc::row_block0)];
    const int h = d.h, w = d.w, r = d.rx, win = 2 * r + 1;
    const int t = b - (stage ? d.row_block0_2 : d.row_block0);
    const int y = (t / d.row_segs) * MORPH_ROWS + wave, x0 = (t % d.row_segs) * MORPH_SEG;
    const bool row = y < h;
    const uint32_t flip = stage ? d.flip[1] : d.flip[0];
    const gword* __restrict__ in = (const gword*)(uintptr_t)(stage ? d.mid : d.src);
    gword* __restrict__ keys = (gword*)(uintptr_t)d.keys;
    uint32_t* __restrict__ mine = staged[wave];
    const int need = MORPH_SEG + 2 * r;   // <= MORPH_STAGED - 2
    uint32_t v[MORPH_PER_LANE];
#pragma unroll
    for (int k = 0; k < MORPH_PER_LANE; k++) {
        const int s = lane + 64 * k, x = x0 - r + s;
        uint32_t key = MORPH_EMPTY;
        if (row && s < need && x >= 0 && x < w) {
            const uint32_t word = in[(int64_t)y * w + x];
            if (!is_nan_word(word)) key = key_of(word) ^ flip;
        }
        v[k] = key;
        mine[s] = key;
    }
    __syncthreads();
    int span = 1;
    for (; span * 2 <= win; span *= 2) {   // uniform in the block: win is the page's
        uint32_t u[MORPH_PER_LANE];
#pragma unroll
        for (int k = 0; k < MORPH_PER_LANE; k++) {
            const int s = lane + 64 * k + span;
            u[k] = s < MORPH_STAGED ? mine[s] : MORPH_EMPTY;
        }
        __syncthreads();   // every entry is read before it is written
#pragma unroll
        for (int k = 0; k < MORPH_PER_LANE; k++) {
            v[k] = least(v[k], u[k]);
            mine[lane + 64 * k] = v[k];
        }
        __syncthreads();
    }
    // an entry holds the least of `span` keys from its place on, span <= win < 2 span: two spans make the window
    const int second = win - span;   // 0 .. 63
#pragma unroll
    for (int k = 0; k < MORPH_SEG / 64; k++) {
        const int s = lane + 64 * k, x = x0 + s;
        if (row && x < w) keys[(int64_t)y * w + x] = least(mine[s], mine[s + second]);   // s + second <= 255 + 63
    }
}

// ---- the vertical pass of stage `stage` (0 or 1); WINDOW: the largest 2 ry + 1 of the batch fits it
template <int WINDOW>
__global__ void __launch_bounds__(MORPH_STRIP)
morph_cols_kernel(const MorphDesc* __restrict__ descs, int n_pages, int stage) {
    __shared__ uint32_t held[WINDOW][MORPH_STRIP];   // a lane's column: suffix extrema, then the keys read after them
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const MorphDesc d = descs[stage ? find_by(descs, n_pages, b, &MorphDesc::block0_2) : find_desc(descs, n_pages, b)];
    const int h = d.h, w = d.w, r = d.ry, win = 2 * r + 1;   // win <= WINDOW: morph_pages picks the kernel by the largest ry
    const int t = b - (stage ? d.block0_2 : d.block0), seg = t / d.strips, strip = t % d.strips;
    const int x = strip * MORPH_STRIP + lane;
    const bool in = x < w;
    const int y0 = seg * d.seg_rows, y1 = y0 + d.seg_rows < h ? y0 + d.seg_rows : h;
    const bool last = stage == d.stages - 1;
    const uint32_t flip = stage ? d.flip[1] : d.flip[0];
    const gword* __restrict__ keys = (const gword*)(uintptr_t)d.keys;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ out = (gword*)(uintptr_t)(last ? d.dst : d.mid);
    gbyte* __restrict__ bytes = last ? (gbyte*)(uintptr_t)d.mask_out : (gbyte*)0;
    uint32_t counted = 0u, changed = 0u, before = 0u, after = 0u;   // a lane sees at most 65535 pixels
    bool have = false;   // held[0 .. win - 2] are the keys of this block's first win - 1 rows, left by the block before
    // Loads go out MORPH_CHUNK rows at a time ahead of their use: a wait for one load also waits for the stores before it,
    // so a load, its use and a store per row would pay a memory latency per row.
    for (int base = y0 - r; base + r < y1; base += win) {   // uniform in the block; rows [base, base + win) are a block
        uint32_t m = MORPH_EMPTY;
        if (!have) {   // the first block of the segment: all its rows come from memory
            for (int top = win; top > 0; top -= MORPH_CHUNK) {   // rows top - 1 down to top - MORPH_CHUNK
                uint32_t key[MORPH_CHUNK];
#pragma unroll
                for (int j = 0; j < MORPH_CHUNK; j++) {
                    const int i = top - 1 - j, yy = base + i;
                    key[j] = i >= 0 && in && yy >= 0 && yy < h ? keys[(int64_t)yy * w + x] : MORPH_EMPTY;
                }
#pragma unroll
                for (int j = 0; j < MORPH_CHUNK; j++) {
                    const int i = top - 1 - j;
                    if (i >= 0) {   // uniform
                        m = least(m, key[j]);
                        held[i][lane] = m;   // the least of rows base + i .. base + win - 1
                    }
                }
            }
        } else {   // one new row; the others were left in their slots
            const int yy = base + win - 1;   // > 0
            m = in && yy < h ? keys[(int64_t)yy * w + x] : MORPH_EMPTY;
            held[win - 1][lane] = m;
#pragma unroll 4
            for (int i = win - 2; i >= 0; i--) {
                m = least(m, held[i][lane]);
                held[i][lane] = m;
            }
        }
        const int rows = y1 - (base + r) < win ? y1 - (base + r) : win;   // rows this block decides: base + r + i, i < rows
        uint32_t p = MORPH_EMPTY;   // the least of rows base + win .. base + win + i - 1
        for (int i0 = 0; i0 < rows; i0 += MORPH_CHUNK) {
            uint32_t key[MORPH_CHUNK], was[MORPH_CHUNK];
#pragma unroll
            for (int j = 0; j < MORPH_CHUNK; j++) {
                const int i = i0 + j, yy = base + win + i - 1;   // yy > 0
                key[j] = i > 0 && i < rows && in && yy < h ? keys[(int64_t)yy * w + x] : MORPH_EMPTY;
                was[j] = i < rows && in ? src[(int64_t)(base + r + i) * w + x] : 0x7fc00000u;
            }
#pragma unroll
            for (int j = 0; j < MORPH_CHUNK; j++) {
                const int i = i0 + j;
                if (i < rows) {   // uniform
                    if (i > 0) {
                        p = least(p, key[j]);
                        held[i - 1][lane] = key[j];   // slot i - 1 was used up a step ago
                    }
                    const uint32_t e = least(held[i][lane], p);
                    if (in) {
                        const int64_t at = (int64_t)(base + r + i) * w + x;
                        const bool nan = is_nan_word(was[j]);
                        const uint32_t now = nan ? was[j] : word_of(e ^ flip);   // a counted pixel is in its own window: e is a key
                        out[at] = now;
                        if (last) {
                            const bool dark = !nan && is_dark_word(now), moved = now != was[j];
                            if (bytes) bytes[at] = (uint8_t)((dark ? 1 : 0) | (moved ? 2 : 0));
                            counted += nan ? 0u : 1u;
                            changed += moved ? 1u : 0u;
                            before += !nan && is_dark_word(was[j]) ? 1u : 0u;
                            after += dark ? 1u : 0u;
                        }
                    }
                }
            }
        }
        have = rows == win;   // otherwise this was the last block
    }
    if (last) {   // uniform in the block
        const uint32_t c0 = wave_sum(counted), c1 = wave_sum(changed), c2 = wave_sum(before), c3 = wave_sum(after);
        if (lane == 0) {
            gu64* __restrict__ rec = (gu64*)(uintptr_t)d.counts + (size_t)t * MORPH_COUNTS;
            rec[0] = c0;
            rec[1] = c1;
            rec[2] = c2;
            rec[3] = c3;
        }
    }
}

// ---- the counts: one block per page
__global__ void __launch_bounds__(MORPH_ROW_THREADS)
morph_info_kernel(const MorphDesc* __restrict__ descs) {
    __shared__ u64 part[MORPH_ROW_THREADS / 64][MORPH_COUNTS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MorphDesc d = descs[blockIdx.x];
    const int blocks = d.strips * d.segs;
    const gu64* __restrict__ counts = (const gu64*)(uintptr_t)d.counts;
    u64 sum[MORPH_COUNTS] = {0ull, 0ull, 0ull, 0ull};
    for (int t = tid; t < blocks; t += MORPH_ROW_THREADS) {
#pragma unroll
        for (int i = 0; i < MORPH_COUNTS; i++) sum[i] += counts[(size_t)t * MORPH_COUNTS + i];
    }
#pragma unroll
    for (int i = 0; i < MORPH_COUNTS; i++) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const int lo = __shfl_xor((int)(uint32_t)sum[i], s), hi = __shfl_xor((int)(uint32_t)(sum[i] >> 32), s);
            sum[i] += (u64)(uint32_t)lo | ((u64)(uint32_t)hi << 32);
        }
        if (lane == 0) part[wave][i] = sum[i];
    }
    __syncthreads();
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        u64 all[MORPH_COUNTS] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int k = 0; k < MORPH_ROW_THREADS / 64; k++)
#pragma unroll
            for (int i = 0; i < MORPH_COUNTS; i++) all[i] += part[k][i];
        info->counted = all[0];
        info->changed = all[1];
        info->ink_before = all[2];
        info->ink_after = all[3];
    }
}

void morph_pages(const MorphDesc* d_descs, int n_pages, const int row_blocks[2], const int col_blocks[2], int max_ry, hipStream_t s) {
    const int win = 2 * max_ry + 1;
    auto cols = win <= MORPH_WINDOW_S ? morph_cols_kernel<MORPH_WINDOW_S> : win <= MORPH_WINDOW_M ? morph_cols_kernel<MORPH_WINDOW_M> : morph_cols_kernel<MORPH_WINDOW>;
    if (n_pages <= 0 || row_blocks[0] <= 0 || col_blocks[0] <= 0 || max_ry > MORPH_MAX_RADIUS) return;
    for (int stage = 0; stage < 2; stage++) {
        if (row_blocks[stage] <= 0 || col_blocks[stage] <= 0) continue;   // no page of two stages
        hipLaunchKernelGGL(morph_rows_kernel, dim3(row_blocks[stage]), dim3(MORPH_ROW_THREADS), 0, s, d_descs, n_pages, stage);
        hipLaunchKernelGGL(cols, dim3(col_blocks[stage]), dim3(MORPH_STRIP), 0, s, d_descs, n_pages, stage);
    }
    hipLaunchKernelGGL(morph_info_kernel, dim3(n_pages), dim3(MORPH_ROW_THREADS), 0, s, d_descs);
}

}  // namespace k
}  // namespace ocrs
