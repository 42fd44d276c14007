// Ruled-line removal: the long thin rules of forms, tables and underlines taken out of resident pages,
// for a batch of pages of any mix of sizes and parameters.  A code object of its own, as kernels_normalize.hip is.
// tests/rules_ref.py is the definition; everything here is integer and set arithmetic, every count a sum of integers, so
// the result is defined to the bit whatever the schedule or batch.
//
// The float page is read twice (passes 1 and 7) and written once (pass 7).  Everything between works on bit masks, 64
// pixels to a word (RulesMask in kernels.hpp): a row-major mask holds the page's rows, a transposed mask its columns, and a
// column operation is the row operation on the transposed mask.  Eight launches on one stream, no host round trip between
// them.  Every launch takes one block per 64 x 64 tile of a page; blocks find their page by bisecting the descriptors'
// block prefix (block0).  Passes 3, 5 and 6 spread the page's word rows or words over the page's blocks.
//   1 rules_mask_kernel       ink = v < threshold, one __ballot per 64 pixels -> INK; the tile's 64 words transposed -> INK_T;
//                             the histogram of the pixels that are neither ink nor NaN, in the same read.
//   2 rules_paper_kernel      one block per page: pct(1, 2) of the histogram -> the fill.
//   3 rules_open_kernel<0>    CH = open(INK, L), CV_T = open(INK_T, L): a wave per word row.
//   4 rules_transpose_kernel  CH -> CH_T, CV_T -> CV.
//   5 rules_open_kernel<1>    RH_T = CH_T \ open(CH_T, T + 1), RV = CV \ open(CV, T + 1).
//   6 rules_sets_kernel       a thread per word: text, the crossing test, D and the margins, in each rule's own direction:
//                             DV, MV from RV (row-major), DH_T, MH_T from RH_T (transposed).
//   7 rules_map_kernel        the tile's transposed words brought back, out = D ? fill : v, the byte mask, |D| and |K|.
//   8 rules_info_kernel       one block per page: what the blocks of passes 1, 6 and 7 counted, added up -> the page's RulesInfo.
//
// open (passes 3 and 5).  A run crosses word boundaries, so a word needs to know how far the ones reach beyond either of
// its ends.  A wave takes 64 words of a row, a word per lane; two segmented scans (six shuffle steps each) over (the word
// is all ones, its ones at the near end) give every lane the ones that end at its left edge and those that start at its
// right edge.  A run inside the word is opened by doubling shifts.  A row of more than 64 words is walked twice: first
// from the right, which leaves in lane c the ones that start at the left edge of chunk c, then from the left with the
// ones that end at the chunk's left edge carried along.
//
// The crossing test (pass 6).  A run of RV (of RH_T) is at most T <= 64 long, so it lies in two neighbouring words at most.
// Its first pixel is marked when text precedes it; adding the marks to the word clears exactly the marked runs (the carry
// runs through the ones and stops behind them), and the carry out of a word goes into the next.  The same on the
// bit-reversed words for the text behind the run.  The margins are shifts by 1 .. M with the neighbouring words' bits.
//
// Loads and stores of the page: dwords in pass 1 (a lane per pixel, so that the ballot is the word); in pass 7 16-byte
// accesses when the page width is a multiple of 4 and both buffers are 16-byte aligned (desc.vec, decided on the host),
// otherwise a lane per pixel.  Both passes have all the tile's loads of a thread on their way before the first is used.
// Every access is predicated on the page.  The barriers are at the top level of each kernel and
// every thread of every block reaches them; shuffles and ballots are reached by whole waves.
#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int RULES_THREADS = 256;
constexpr int RULES_WAVES = RULES_THREADS / 64;
static_assert(RULES_WAVES == 4 && RULES_COUNTS == 16, "the layout of a block's counts");

typedef __attribute__((address_space(1))) RulesInfo ginfo;
typedef uint32_t uint4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint4v gquadw;

int64_t rules_tiles(int h, int w) { return (int64_t)((h + 63) / 64) * ((w + 63) / 64); }
size_t rules_mask_words(int h, int w) {
    return (size_t)RM_ROW_MAJOR * (size_t)h * (size_t)((w + 63) / 64) + (size_t)RM_TRANSPOSED * (size_t)w * (size_t)((h + 63) / 64);
}

// the masks of a page
struct Masks {
    gu64* base;
    size_t n_r, n_t;   // words of a row-major mask, of a transposed one
    __device__ __forceinline__ gu64* r(int m) const { return base + (size_t)m * n_r; }
    __device__ __forceinline__ gu64* t(int m) const { return base + (size_t)RM_ROW_MAJOR * n_r + (size_t)m * n_t; }
};
__device__ __forceinline__ Masks masks_of(const RulesDesc& d) {
    Masks m;
    m.base = (gu64*)(uintptr_t)d.masks;
    m.n_r = (size_t)d.h * (size_t)d.ww;
    m.n_t = (size_t)d.w * (size_t)d.hw;
    return m;
}

// A 64 x 64 bit matrix, row r in lane r (bit c = column c) -> its transpose, row c in lane c.  All 64 lanes call it together.
__device__ __forceinline__ u64 transpose64(u64 a, int lane) {
    const u64 keep[6] = {0x00000000FFFFFFFFull, 0x0000FFFF0000FFFFull, 0x00FF00FF00FF00FFull,
                         0x0F0F0F0F0F0F0F0Full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
    for (int s = 0; s < 6; s++) {
        const int j = 32 >> s;
        const u64 m = keep[s], p = shfl_xor64(a, j);
        a = (lane & j) ? ((a & ~m) | ((p & ~m) >> j)) : ((a & m) | ((p & m) << j));
    }
    return a;
}

// What a page's blocks counted, a record of RULES_COUNTS words (one cache line) per block, every word of it written by
// plain stores: [RC_INK + wave] pass 1, [RC_H + wave] and [RC_V + wave] pass 6, [RC_D] and [RC_K] pass 7.  Pass 8 adds them up.
// (With every wave or block adding into a word of the page's info instead, hundreds of atomics to a page's one cache line,
// pass 1 took 74 us in place of 30 and pass 7 179 us in place of 29 on sixteen pages of 1024 x 1024: DESIGN.md §7.8.)
enum { RC_INK = 0, RC_H = 4, RC_V = 8, RC_D = 12, RC_K = 13 };
__device__ __forceinline__ gu64* counts_of(const RulesDesc& d, int tile) { return (gu64*)(uintptr_t)d.counts + (size_t)tile * RULES_COUNTS; }

__device__ __forceinline__ void count_add(gu64* at, u64 v) {
    if (v) __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pass 1
__global__ void __launch_bounds__(RULES_THREADS)
rules_mask_kernel(const RulesDesc* __restrict__ descs, int n_pages) {
    __shared__ uint32_t hist[RULES_WAVES][256];
    __shared__ u64 rows[64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RulesDesc d = descs[find_desc(descs, n_pages, b)];
    const int t = b - d.block0, ty = t / d.ww, tx = t % d.ww, h = d.h, w = d.w;
    const gfloat* __restrict__ src = (const gfloat*)(uintptr_t)d.src;
    const Masks m = masks_of(d);
#pragma unroll
    for (int i = 0; i < RULES_WAVES; i++) hist[i][tid] = 0u;
    __syncthreads();
    const int x = tx * 64 + lane;
    const float thr = d.threshold;
    constexpr int ROWS = 64 / RULES_WAVES;   // of the tile, per wave
    float px[ROWS];   // all of them on their way before the first is looked at
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
        const int y = ty * 64 + i * RULES_WAVES + wave;
        px[i] = y < h && x < w ? src[(int64_t)y * w + x] : 0.0f;
    }
    u64 n_ink = 0;
#pragma unroll
    for (int i = 0; i < ROWS; i++) {   // uniform in the block
        const int r = i * RULES_WAVES + wave, y = ty * 64 + r;
        const bool in = y < h && x < w;
        const float v = px[i];
        const bool ink = in && v < thr;   // NaN is not ink
        const u64 word = __ballot(ink);
        hist_add(hist[wave], in && !ink ? bin_of(clamp01(v + 0.5f)) : -1, lane);
        n_ink += (u64)__popcll(word);
        if (lane == 0) {
            rows[r] = word;
            if (y < h) m.r(RM_INK)[(size_t)y * d.ww + tx] = word;
        }
    }
    __syncthreads();
    if (wave == 0) {   // the tile's 64 words, transposed: column x's word of the rows 64 ty .. 64 ty + 63
        const u64 col = transpose64(rows[lane], lane);
        if (x < w) m.t(RM_INK_T)[(size_t)x * d.hw + ty] = col;
    }
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < RULES_WAVES; i++) mine += hist[i][tid];
    count_add((gu64*)(uintptr_t)d.hist + tid, (u64)mine);
    if (lane == 0) counts_of(d, t)[RC_INK + wave] = n_ink;
}

// ---- pass 2: one block per page
__global__ void __launch_bounds__(RULES_THREADS)
rules_paper_kernel(const RulesDesc* __restrict__ descs) {
    __shared__ u64 wave_tot[RULES_WAVES];
    __shared__ int found;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RulesDesc d = descs[blockIdx.x];
    const u64 mine = ((const gu64*)(uintptr_t)d.hist)[tid];
    u64 incl = mine;   // inclusive scan over the block's 256 bins
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int lo = __shfl_up((int)(uint32_t)incl, s), hi = __shfl_up((int)(uint32_t)(incl >> 32), s);
        if (lane >= s) incl += (u64)(uint32_t)lo | ((u64)(uint32_t)hi << 32);
    }
    if (lane == 63) wave_tot[wave] = incl;
    if (tid == 0) found = 255;   // nothing counted
    __syncthreads();
    u64 n = 0;
#pragma unroll
    for (int i = 0; i < RULES_WAVES; i++) {
        const u64 s = wave_tot[i];
        n += s;
        if (i < wave) incl += s;
    }
    const u64 excl = incl - mine;
    if (n > 0 && incl * 2 >= n && !(excl * 2 >= n)) found = tid;   // pct(1, 2): the smallest bin whose cumulative count passes
    __syncthreads();
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        const bool given = d.paper == d.paper;
        info->paper_bin = given ? -1 : found;
        info->fill = given ? d.paper : (float)(found + 1) / 256.0f - 0.5f;   // exact
        info->counted = n;
    }
}

// ---- passes 3 and 5
// The runs of at least n (1 .. 64) ones that lie inside a word.
__device__ __forceinline__ u64 open_word(u64 w, int n) {
    u64 e = w;   // bit i: the bits i .. i + n - 1 are all set
    for (int k = 1; k < n;) {
        const int s = k < n - k ? k : n - k;
        e &= e >> s;
        k += s;
    }
    for (int k = 1; k < n;) {
        const int s = k < n - k ? k : n - k;
        e |= e << s;
        k += s;
    }
    return e;
}

// (all ones, ones at the near end) of 64 words, a word per lane, scanned towards lower lanes (DOWN: a lane gathers the lanes
// above it) or towards higher ones -> the ones that start at this word's near end and run on through its far neighbours;
// `beyond`: the same of the word past the chunk's far end.  All 64 lanes call it together.
template <bool DOWN>
__device__ __forceinline__ int reach(bool full, int ones, int beyond, int lane) {
    int f = full ? 1 : 0, len = ones;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int of = DOWN ? __shfl_down(f, s) : __shfl_up(f, s), ol = DOWN ? __shfl_down(len, s) : __shfl_up(len, s);
        const bool has = DOWN ? lane + s < 64 : lane >= s;
        if (has) {
            if (f) len += ol;
            f &= of;
        }
    }
    return f ? len + beyond : len;
}

// One word row [words] of `src`, opened by n: a wave's work.  NOT_OPEN: dst = src \ open(src, n); otherwise dst = open(src, n).
template <bool NOT_OPEN>
__device__ __forceinline__ void open_row(const gu64* __restrict__ src, gu64* __restrict__ dst, int words, int n, int lane) {
    const int chunks = (words + 63) >> 6;
    int from_right = 0;   // lane c: the ones that start at the left edge of chunk c (c >= 1)
    for (int c = chunks - 1; c >= 1; c--) {
        const int j = c * 64 + lane;
        const u64 wd = j < words ? src[j] : 0ull;
        const bool full = wd == ~0ull;
        const int beyond = c + 1 < chunks ? __shfl(from_right, c + 1) : 0;
        const int s = reach<true>(full, full ? 64 : __builtin_ctzll(~wd), beyond, lane);
        const int first = __shfl(s, 0);
        if (lane == c) from_right = first;
    }
    int from_left = 0;    // the ones that end at the left edge of this chunk
    for (int c = 0; c < chunks; c++) {
        const int j = c * 64 + lane;
        const u64 wd = j < words ? src[j] : 0ull;
        const bool full = wd == ~0ull;
        const int head = full ? 64 : __builtin_ctzll(~wd), tail = full ? 64 : __builtin_clzll(~wd);
        const int beyond = c + 1 < chunks ? __shfl(from_right, c + 1) : 0;
        const int s = reach<true>(full, head, beyond, lane);        // starts at my left edge, runs right
        const int e = reach<false>(full, tail, from_left, lane);    // ends at my right edge, runs left
        const int s_next = __shfl_down(s, 1), e_prev = __shfl_up(e, 1);
        const int right_in = lane == 63 ? beyond : s_next, left_in = lane == 0 ? from_left : e_prev;
        u64 out = n <= 64 ? open_word(wd, n) : 0ull;
        if (full) {
            if (left_in + 64 + right_in >= n) out = ~0ull;
        } else {
            if (head > 0 && left_in + head >= n) out |= (1ull << head) - 1ull;
            if (tail > 0 && tail + right_in >= n) out |= ~0ull << (64 - tail);
        }
        if (j < words) dst[j] = NOT_OPEN ? wd & ~out : out;
        from_left = __shfl(e, 63);
    }
}

template <int STAGE>
__global__ void __launch_bounds__(RULES_THREADS)
rules_open_kernel(const RulesDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RulesDesc d = descs[find_desc(descs, n_pages, b)];
    const Masks m = masks_of(d);
    const int n = STAGE == 0 ? d.min_length : d.max_thickness + 1;
    const int64_t rows = (int64_t)d.h + d.w, step = (int64_t)d.hw * d.ww * RULES_WAVES;
    for (int64_t r = (int64_t)(b - d.block0) * RULES_WAVES + wave; r < rows; r += step) {   // uniform in the wave
        if (r < d.h) {   // a row of the page
            const size_t at = (size_t)r * d.ww;
            if (STAGE == 0) open_row<false>(m.r(RM_INK) + at, m.r(RM_CH) + at, d.ww, n, lane);
            else open_row<true>(m.r(RM_CV) + at, m.r(RM_RV) + at, d.ww, n, lane);
        } else {         // a column of the page
            const size_t at = (size_t)(r - d.h) * d.hw;
            if (STAGE == 0) open_row<false>(m.t(RM_INK_T) + at, m.t(RM_CV_T) + at, d.hw, n, lane);
            else open_row<true>(m.t(RM_CH_T) + at, m.t(RM_RH_T) + at, d.hw, n, lane);
        }
    }
}

// ---- pass 4: wave 0 takes the tile of CH to CH_T, wave 1 the tile of CV_T to CV
__global__ void __launch_bounds__(128)
rules_transpose_kernel(const RulesDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const RulesDesc d = descs[find_desc(descs, n_pages, b)];
    const Masks m = masks_of(d);
    const int t = b - d.block0, ty = t / d.ww, tx = t % d.ww;
    const int y = ty * 64 + lane, x = tx * 64 + lane;
    if (wave == 0) {   // uniform in the wave
        const u64 col = transpose64(y < d.h ? m.r(RM_CH)[(size_t)y * d.ww + tx] : 0ull, lane);
        if (x < d.w) m.t(RM_CH_T)[(size_t)x * d.hw + ty] = col;
    } else {
        const u64 row = transpose64(x < d.w ? m.t(RM_CV_T)[(size_t)x * d.hw + ty] : 0ull, lane);
        if (y < d.h) m.r(RM_CV)[(size_t)y * d.ww + tx] = row;
    }
}

// ---- pass 6
// The bits of the rule word r[2] that lie in a run with text right before it and right behind it.  r, t: the rule and the
// text words at j - 2 .. j + 2 (zero outside the row).  Runs are at most 64 long.
__device__ __forceinline__ u64 crossed(const u64* r, const u64* t) {
    // text before the run: mark the first bit of such a run, and let an addition clear the run
    const u64 first_p = r[1] & ~((r[1] << 1) | (r[0] >> 63)) & ((t[1] << 1) | (t[0] >> 63));
    const u64 carry = (r[1] + first_p < r[1]) ? (r[2] & 1ull) : 0ull;   // a marked run of the word before runs on into this one
    const u64 first = r[2] & ~((r[2] << 1) | (r[1] >> 63)) & ((t[2] << 1) | (t[1] >> 63));
    const u64 before = r[2] & ~(r[2] + first + carry);
    // text behind the run: the same, read from the other end
    const u64 last_n = r[3] & ~((r[3] >> 1) | (r[4] << 63)) & ((t[3] >> 1) | (t[4] << 63));
    const u64 rn = __brevll(r[3]);
    const u64 carry_b = (rn + __brevll(last_n) < rn) ? (r[2] >> 63) : 0ull;
    const u64 last = r[2] & ~((r[2] >> 1) | (r[3] << 63)) & ((t[2] >> 1) | (t[3] << 63));
    const u64 rr = __brevll(r[2]);
    const u64 behind = __brevll(rr & ~(rr + __brevll(last) + carry_b));
    return before & behind;
}

__global__ void __launch_bounds__(RULES_THREADS)
rules_sets_kernel(const RulesDesc* __restrict__ descs, int n_pages) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
    const RulesDesc d = descs[find_desc(descs, n_pages, b)];
    const Masks m = masks_of(d);
    const int64_t n_r = (int64_t)m.n_r, total = n_r + (int64_t)m.n_t, step = (int64_t)d.hw * d.ww * RULES_THREADS;
    const int margin = d.margin;
    u64 n_h = 0, n_v = 0;
    for (int64_t i = (int64_t)(b - d.block0) * RULES_THREADS + tid; i < total; i += step) {
        const bool rowwise = i < n_r;   // RV along the page's rows, or RH_T along its columns
        const int words = rowwise ? d.ww : d.hw, len = rowwise ? d.w : d.h;
        const int64_t at = rowwise ? i : i - n_r;
        const int j = (int)((uint32_t)at % (uint32_t)words);   // a mask has fewer than 2^27 words
        const gu64* __restrict__ rule = rowwise ? m.r(RM_RV) : m.t(RM_RH_T);
        const gu64* __restrict__ ink = rowwise ? m.r(RM_INK) : m.t(RM_INK_T);
        const gu64* __restrict__ ch = rowwise ? m.r(RM_CH) : m.t(RM_CH_T);
        const gu64* __restrict__ cv = rowwise ? m.r(RM_CV) : m.t(RM_CV_T);
        u64 r[7], t[7];   // the words j - 3 .. j + 3 of the row
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const int jj = j + k - 3;
            r[k] = jj >= 0 && jj < words ? rule[at + k - 3] : 0ull;
        }
        u64 d_here = 0ull, near = 0ull;
        if (r[2] | r[3] | r[4]) {   // most words of a page hold no rule, nor do their neighbours: nothing to remove, no margin
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const int jj = j + k - 3;
                const int64_t a = at + k - 3;
                t[k] = jj >= 0 && jj < words ? ink[a] & ~(ch[a] | cv[a]) : 0ull;
            }
            const u64 d_prev = r[2] & ~crossed(r, t), d_next = r[4] & ~crossed(r + 2, t + 2);
            d_here = r[3] & ~crossed(r + 1, t + 1);
            for (int s = 1; s <= margin; s++)
                near |= (d_here << s) | (d_prev >> (64 - s)) | (d_here >> s) | (d_next << (64 - s));
            const u64 valid = (j == words - 1 && (len & 63)) ? (1ull << (len & 63)) - 1ull : ~0ull;
            near &= ~ink[at] & valid;
        }
        (rowwise ? m.r(RM_DV) : m.t(RM_DH_T))[at] = d_here;
        (rowwise ? m.r(RM_MV) : m.t(RM_MH_T))[at] = near;
        if (rowwise) n_v += (u64)__popcll(d_here);
        else n_h += (u64)__popcll(d_here);
    }
    n_h = wave_sum(n_h);
    n_v = wave_sum(n_v);
    if (lane == 0) {
        gu64* __restrict__ c = counts_of(d, b - d.block0);
        c[RC_H + (tid >> 6)] = n_h;
        c[RC_V + (tid >> 6)] = n_v;
    }
}

// ---- pass 7
__global__ void __launch_bounds__(RULES_THREADS)
rules_map_kernel(const RulesDesc* __restrict__ descs, int n_pages) {
    __shared__ u64 plane[4][64];   // the tile's rows of Dh, Dv, Mh | Mv, Kh | Kv
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RulesDesc d = descs[find_desc(descs, n_pages, b)];
    const Masks m = masks_of(d);
    const int t = b - d.block0, ty = t / d.ww, tx = t % d.ww, h = d.h, w = d.w;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ dst = (gword*)(uintptr_t)d.dst;
    gbyte* __restrict__ bytes = (gbyte*)(uintptr_t)d.mask_out;
    // the tile's pixels on their way before the masks are looked at: a quad per thread and round (w % 4 == 0: x < w means
    // x + 3 < w), or a pixel per thread and round, sixteen of them
    uint4v px[4];
    if (d.vec) {   // uniform in the block
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int p = i * RULES_THREADS + tid, y = ty * 64 + (p >> 4), x = tx * 64 + 4 * (p & 15);
            const uint4v none = {0u, 0u, 0u, 0u};
            px[i] = y < h && x < w ? *(const gquadw*)(src + (int64_t)y * w + x) : none;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int p = (4 * i + k) * RULES_THREADS + tid, y = ty * 64 + (p >> 6), x = tx * 64 + (p & 63);
                px[i][k] = y < h && x < w ? src[(int64_t)y * w + x] : 0u;
            }
    }
    {
        const int y = ty * 64 + lane, x = tx * 64 + lane;
        const size_t at_r = (size_t)y * d.ww + tx, at_t = (size_t)x * d.hw + ty;
        const bool in_r = y < h, in_t = x < w;
        u64 v;
        if (wave == 0) v = transpose64(in_t ? m.t(RM_DH_T)[at_t] : 0ull, lane);   // uniform in the wave
        else if (wave == 1) v = in_r ? m.r(RM_DV)[at_r] : 0ull;
        else if (wave == 2) v = transpose64(in_t ? m.t(RM_MH_T)[at_t] : 0ull, lane) | (in_r ? m.r(RM_MV)[at_r] : 0ull);
        else v = transpose64(in_t ? m.t(RM_RH_T)[at_t] & ~m.t(RM_DH_T)[at_t] : 0ull, lane) | (in_r ? m.r(RM_RV)[at_r] & ~m.r(RM_DV)[at_r] : 0ull);
        plane[wave][lane] = v;
    }
    __syncthreads();
    const ginfo* __restrict__ info = (const ginfo*)(uintptr_t)d.info;
    if (wave == 0) {
        const u64 n_d = wave_sum((u64)__popcll(plane[0][lane] | plane[1][lane] | plane[2][lane]));
        const u64 n_k = wave_sum((u64)__popcll(plane[3][lane]));
        if (lane == 0) {
            gu64* __restrict__ c = counts_of(d, t);
            c[RC_D] = n_d;
            c[RC_K] = n_k;
        }
    }
    const uint32_t fill = __float_as_uint(info->fill);
    if (d.vec) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int p = i * RULES_THREADS + tid, r = p >> 4, q = p & 15, y = ty * 64 + r, x = tx * 64 + 4 * q;
            if (y >= h || x >= w) continue;
            const int64_t at = (int64_t)y * w + x;
            const uint32_t dh = (uint32_t)(plane[0][r] >> (4 * q)) & 15u, dv = (uint32_t)(plane[1][r] >> (4 * q)) & 15u,
                           mg = (uint32_t)(plane[2][r] >> (4 * q)) & 15u, kp = (uint32_t)(plane[3][r] >> (4 * q)) & 15u;
            const uint32_t gone = dh | dv | mg;
            uint4v v = px[i];
            uint32_t packed = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if ((gone >> k) & 1u) v[k] = fill;
                packed |= (((dh >> k) & 1u) | (((dv >> k) & 1u) << 1) | (((mg >> k) & 1u) << 2) | (((kp >> k) & 1u) << 3)) << (8 * k);
            }
            *(gquadw*)(dst + at) = v;
            if (bytes) *(gword*)(bytes + at) = packed;   // at % 4 == 0
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int p = (4 * i + k) * RULES_THREADS + tid, r = p >> 6, c = p & 63, y = ty * 64 + r, x = tx * 64 + c;
                if (y >= h || x >= w) continue;
                const int64_t at = (int64_t)y * w + x;
                const uint32_t dh = (uint32_t)(plane[0][r] >> c) & 1u, dv = (uint32_t)(plane[1][r] >> c) & 1u,
                               mg = (uint32_t)(plane[2][r] >> c) & 1u, kp = (uint32_t)(plane[3][r] >> c) & 1u;
                dst[at] = (dh | dv | mg) ? fill : px[i][k];
                if (bytes) bytes[at] = (uint8_t)(dh | (dv << 1) | (mg << 2) | (kp << 3));
            }
    }
}

// ---- pass 8: one block per page
__global__ void __launch_bounds__(RULES_THREADS)
rules_info_kernel(const RulesDesc* __restrict__ descs) {
    __shared__ u64 part[RULES_WAVES][5];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RulesDesc d = descs[blockIdx.x];
    const int tiles = d.hw * d.ww;
    u64 sum[5] = {0ull, 0ull, 0ull, 0ull, 0ull};   // ink, Dh, Dv, D, K
    for (int t = tid; t < tiles; t += RULES_THREADS) {
        const gu64* __restrict__ c = counts_of(d, t);
#pragma unroll
        for (int i = 0; i < RULES_WAVES; i++) {
            sum[0] += c[RC_INK + i];
            sum[1] += c[RC_H + i];
            sum[2] += c[RC_V + i];
        }
        sum[3] += c[RC_D];
        sum[4] += c[RC_K];
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
        sum[i] = wave_sum(sum[i]);
        if (lane == 0) part[wave][i] = sum[i];
    }
    __syncthreads();
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        u64 all[5];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            all[i] = 0ull;
#pragma unroll
            for (int k = 0; k < RULES_WAVES; k++) all[i] += part[k][i];
        }
        info->ink = all[0];
        info->h_removed = all[1];
        info->v_removed = all[2];
        info->overwritten = all[3];
        info->kept = all[4];
    }
}

void remove_rules_pages(const RulesDesc* d_descs, int n_pages, int total_blocks, hipStream_t s) {
    if (n_pages <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(rules_mask_kernel, dim3(total_blocks), dim3(RULES_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(rules_paper_kernel, dim3(n_pages), dim3(RULES_THREADS), 0, s, d_descs);
    hipLaunchKernelGGL(rules_open_kernel<0>, dim3(total_blocks), dim3(RULES_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(rules_transpose_kernel, dim3(total_blocks), dim3(128), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(rules_open_kernel<1>, dim3(total_blocks), dim3(RULES_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(rules_sets_kernel, dim3(total_blocks), dim3(RULES_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(rules_map_kernel, dim3(total_blocks), dim3(RULES_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(rules_info_kernel, dim3(n_pages), dim3(RULES_THREADS), 0, s, d_descs);
}

}  // namespace k
}  // namespace ocrs
