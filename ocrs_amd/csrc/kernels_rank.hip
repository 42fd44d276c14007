// Grain removal: a rank filter (median, percentile, either on outliers only) over a rectangle of at most
// 15 x 15, for a batch of resident pages of any mix of sizes and parameters.  A code object of its own, as kernels_morph.hip
// is.  tests/rank_ref.py is the definition.  A rank filter picks one of its inputs, so the result is the 32-bit word of some
// pixel of the source and is defined to the bit whatever the schedule or batch.  No floating-point instruction touches a
// pixel: words are ordered through stroke repair's key  k(w) = ~w if the sign bit is set, else w | 0x80000000.  The key ~0
// belongs to NaN words alone and is the empty key: what a NaN pixel, every place beyond the page edge and every place of a
// padded window outside the page's own radii hold.  It is the greatest key, so it is under no candidate and under no key.
//
// At most three launches on one stream, no host round trip between them: rank_kernel for the pages of the register classes,
// rank_kernel for the pages of the LDS class, the counts.  A page takes blocks in one of the two and shares its prefix in the
// other with the page after it, so that the bisection of find_desc never finds it there.
//   rank_kernel       a block owns a tile of RANK_TILE_H rows x RANK_TILE_W columns and stages the keys of the tile and of
//                     its halo (ry rows, rx columns, the page's own radii) in LDS once.  A wave owns every fourth row of the
//                     tile and a lane a column, so the 64 lanes of every LDS read touch 64 consecutive words.  One counting
//                     pass over the window gives n, lt and le of the pixel's own key for the sparing rule.  The class of a
//                     page (its descriptor's cls) picks how the key of rank a = at(percent) is found, the same way for every
//                     thread of the block; the kernel is a template over registers or LDS, so that the LDS loop does not
//                     carry the registers of the sorting network (74 against 40) and keeps its eight waves per SIMD:
//                     class 2 (any radii) walks the window in LDS and bisects on the key's bits from 31 down to 0: with
//                     candidate = prefix | bit and c the number of window keys under the candidate, c <= a keeps the bit.
//                     After 32 steps the prefix is the greatest value with at most a keys under it, which is s[a].
//                     class 0 (rx, ry <= 1) holds a 3 x 3 window in 9 registers, class 1 (rx, ry <= 2) a 5 x 5 window in
//                     25, the places outside the page's own radii empty.  Batcher's odd-even merge network (28 and 140
//                     compare-exchanges, fixed at compile time) sorts them, the empty keys last, and a chain of selects
//                     takes s[a]: a fifth and a third of the operations the 32 counting passes would take.
//                     No control flow depends on a pixel, nothing is indexed by a value that is not a constant, no scratch.
//                     The same kernel writes the result word and, when asked for, the mask byte, and adds the five counts
//                     over the block (wave sums, then the four waves through LDS) into the block's record by plain stores.
//   rank_info_kernel  one block per page: the blocks' records added up in a fixed order -> the page's RankInfo.
//
// Loads and stores are one dword or one byte per lane, consecutive across the wave; the 16-byte path is not used.  Every
// access is predicated on the page.  The two barriers of rank_kernel are outside every loop.
#include "find_desc.hpp"
#include "kernels.hpp"
#include "page_device.hpp"

namespace ocrs {
namespace k {

constexpr int RANK_THREADS = 256;
constexpr int RANK_WAVES = RANK_THREADS / 64;
constexpr int RANK_PER_LANE = RANK_TILE_H / RANK_WAVES;          // rows of the tile a lane decides
constexpr int RANK_LDS_H = RANK_TILE_H + 2 * RANK_MAX_RADIUS;    // the staged region at the largest radii
constexpr int RANK_LDS_W = RANK_TILE_W + 2 * RANK_MAX_RADIUS;
constexpr uint32_t RANK_EMPTY = 0xffffffffu;
static_assert(RANK_TILE_W == 64, "a lane per column of the tile");
static_assert(RANK_TILE_H % RANK_WAVES == 0, "every wave decides the same number of rows");
static_assert(RANK_LDS_W <= 128, "a wave stages a row of the region in two steps");

typedef __attribute__((address_space(1))) RankInfo ginfo;

int64_t rank_blocks(int h, int w) { return (int64_t)((h + RANK_TILE_H - 1) / RANK_TILE_H) * ((w + RANK_TILE_W - 1) / RANK_TILE_W); }
int rank_class(int rx, int ry) {
    const int r = rx > ry ? rx : ry;
    return r <= 1 ? 0 : r <= 2 ? 1 : 2;
}

__device__ __forceinline__ bool is_nan_word(uint32_t w) { return (w & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ uint32_t key_of(uint32_t w) { return (w & 0x80000000u) ? ~w : (w | 0x80000000u); }
__device__ __forceinline__ uint32_t word_of(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }
// under 0.0f, for a word that is not NaN: -0.0 is not, a negative denormal is
__device__ __forceinline__ bool is_dark_word(uint32_t w) { return w > 0x80000000u; }
__device__ __forceinline__ int rank_at(int p, int n) { return (p * (n - 1) + 50) / 100; }   // n >= 1

// What the passes of a pixel found: the key at rank at(percent), the counted keys of the window, and those under and under or
// equal the pixel's own key.
struct Picked {
    uint32_t key;
    int n, lt, le;
};

// Batcher's odd-even merge sort as a network over N registers, ascending; every index is a constant once unrolled.
template <int N>
__device__ __forceinline__ void sort_keys(uint32_t (&v)[N]) {
#pragma unroll
    for (int p = 1; p < N; p *= 2)
#pragma unroll
        for (int k = p; k >= 1; k /= 2)
#pragma unroll
            for (int j = k % p; j + k < N; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; i++)
                    if (i + j + k < N && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        const uint32_t a = v[i + j], b = v[i + j + k];
                        v[i + j] = a < b ? a : b;
                        v[i + j + k] = a < b ? b : a;
                    }
}

// The window in (2 R + 1)^2 registers; keys outside the page's own radii are empty.  `centre` points at the pixel's key.
template <int R>
__device__ __forceinline__ Picked pick_regs(const uint32_t* __restrict__ centre, int rx, int ry, int percent, uint32_t own) {
    constexpr int W = 2 * R + 1;
    uint32_t key[W * W];
#pragma unroll
    for (int dy = -R; dy <= R; dy++)
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            const uint32_t v = centre[dy * RANK_LDS_W + dx];   // inside the array for every R <= RANK_MAX_RADIUS; garbage outside the staged region
            key[(dy + R) * W + dx + R] = (dy < -ry || dy > ry || dx < -rx || dx > rx) ? RANK_EMPTY : v;
        }
    Picked p = {0u, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < W * W; i++) {
        p.n += key[i] != RANK_EMPTY ? 1 : 0;
        p.lt += key[i] < own ? 1 : 0;
        p.le += key[i] <= own ? 1 : 0;   // own is not empty where this is used
    }
    const int a = rank_at(percent, p.n > 0 ? p.n : 1);   // < n: the empty keys sort behind it
    sort_keys(key);
    p.key = key[0];
#pragma unroll
    for (int i = 1; i < W * W; i++) p.key = a == i ? key[i] : p.key;
    return p;
}

// The window walked in LDS in every pass; rx and ry are the block's, so the trip counts are uniform.
__device__ __forceinline__ Picked pick_lds(const uint32_t* __restrict__ centre, int rx, int ry, int percent, uint32_t own) {
    Picked p = {0u, 0, 0, 0};
    for (int dy = -ry; dy <= ry; dy++)
        for (int dx = -rx; dx <= rx; dx++) {
            const uint32_t v = centre[dy * RANK_LDS_W + dx];
            p.n += v != RANK_EMPTY ? 1 : 0;
            p.lt += v < own ? 1 : 0;
            p.le += v <= own ? 1 : 0;
        }
    const int a = rank_at(percent, p.n > 0 ? p.n : 1);
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t cand = p.key | (1u << bit);
        int c = 0;
        for (int dy = -ry; dy <= ry; dy++)
            for (int dx = -rx; dx <= rx; dx++) c += centre[dy * RANK_LDS_W + dx] < cand ? 1 : 0;
        if (c <= a) p.key = cand;
    }
    return p;
}

template <bool REGS>
__global__ void __launch_bounds__(RANK_THREADS)
rank_kernel(const RankDesc* __restrict__ descs, int n_pages) {
    // entry [7 + j][7 + i] is the key of the pixel (y0 + j, x0 + i): the region [7 - ry, 7 + TILE_H + ry) x [7 - rx, 7 + TILE_W + rx) is staged
    __shared__ uint32_t staged[RANK_LDS_H][RANK_LDS_W];
    __shared__ u64 part[RANK_WAVES][RANK_COUNTS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RankDesc d = descs[find_desc(descs, n_pages, b, REGS ? &RankDesc::reg_block0 : &RankDesc::lds_block0)];
    const int h = d.h, w = d.w, rx = d.rx, ry = d.ry;
    const int t = b - (REGS ? d.reg_block0 : d.lds_block0);
    const int y0 = (t / d.tiles_x) * RANK_TILE_H, x0 = (t % d.tiles_x) * RANK_TILE_W;
    const gword* __restrict__ src = (const gword*)(uintptr_t)d.src;
    gword* __restrict__ dst = (gword*)(uintptr_t)d.dst;
    gbyte* __restrict__ bytes = (gbyte*)(uintptr_t)d.mask_out;

    for (int j = wave - ry; j < RANK_TILE_H + ry; j += RANK_WAVES) {   // uniform in the wave; no barrier inside
        const int y = y0 + j;
#pragma unroll
        for (int step = 0; step < 2; step++) {
            const int i = lane + 64 * step - rx, x = x0 + i;
            if (i < RANK_TILE_W + rx) {
                uint32_t key = RANK_EMPTY;
                if (y >= 0 && y < h && x >= 0 && x < w) {
                    const uint32_t word = src[(int64_t)y * w + x];
                    if (!is_nan_word(word)) key = key_of(word);
                }
                staged[RANK_MAX_RADIUS + j][RANK_MAX_RADIUS + i] = key;
            }
        }
    }
    __syncthreads();

    const int x = x0 + lane;
    uint32_t counted = 0u, changed = 0u, before = 0u, after = 0u, spared = 0u;   // a lane decides RANK_PER_LANE pixels
#pragma unroll 1
    for (int q = 0; q < RANK_PER_LANE; q++) {
        const int j = wave + RANK_WAVES * q, y = y0 + j;
        const uint32_t* __restrict__ centre = &staged[RANK_MAX_RADIUS + j][RANK_MAX_RADIUS + lane];
        const uint32_t own = *centre;
        Picked p;
        if (!REGS) p = pick_lds(centre, rx, ry, d.percent, own);
        else if (d.cls == 0) p = pick_regs<1>(centre, rx, ry, d.percent, own);   // uniform in the block
        else p = pick_regs<2>(centre, rx, ry, d.percent, own);
        if (y < h && x < w) {
            const int64_t at = (int64_t)y * w + x;
            const uint32_t was = src[at];   // the word of a NaN pixel is not in its key
            const bool nan = own == RANK_EMPTY;
            const int n = p.n > 0 ? p.n : 1;
            const bool spare = !nan && d.tail >= 1 && p.lt <= rank_at(100 - d.tail, n) && p.le - 1 >= rank_at(d.tail, n);
            const uint32_t now = nan || spare ? was : word_of(p.key);
            dst[at] = now;
            const bool dark = !nan && is_dark_word(now), moved = now != was;
            if (bytes) bytes[at] = (uint8_t)((dark ? 1 : 0) | (moved ? 2 : 0));
            counted += nan ? 0u : 1u;
            changed += moved ? 1u : 0u;
            before += !nan && is_dark_word(was) ? 1u : 0u;
            after += dark ? 1u : 0u;
            spared += spare ? 1u : 0u;
        }
    }
    const u64 sums[RANK_COUNTS] = {wave_sum((u64)counted), wave_sum((u64)changed), wave_sum((u64)before), wave_sum((u64)after), wave_sum((u64)spared)};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < RANK_COUNTS; i++) part[wave][i] = sums[i];
    }
    __syncthreads();
    if (tid < RANK_COUNTS) {
        u64 all = 0ull;
#pragma unroll
        for (int k = 0; k < RANK_WAVES; k++) all += part[k][tid];
        ((gu64*)(uintptr_t)d.counts)[(size_t)t * RANK_COUNTS + tid] = all;
    }
}

// ---- the counts: one block per page
__global__ void __launch_bounds__(RANK_THREADS)
rank_info_kernel(const RankDesc* __restrict__ descs) {
    __shared__ u64 part[RANK_WAVES][RANK_COUNTS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RankDesc d = descs[blockIdx.x];
    const int blocks = d.tiles_x * d.tiles_y;
    const gu64* __restrict__ counts = (const gu64*)(uintptr_t)d.counts;
    u64 sum[RANK_COUNTS] = {0ull, 0ull, 0ull, 0ull, 0ull};
    for (int t = tid; t < blocks; t += RANK_THREADS) {
#pragma unroll
        for (int i = 0; i < RANK_COUNTS; i++) sum[i] += counts[(size_t)t * RANK_COUNTS + i];
    }
#pragma unroll
    for (int i = 0; i < RANK_COUNTS; i++) {
        sum[i] = wave_sum(sum[i]);
        if (lane == 0) part[wave][i] = sum[i];
    }
    __syncthreads();
    if (tid == 0) {
        ginfo* __restrict__ info = (ginfo*)(uintptr_t)d.info;
        u64 all[RANK_COUNTS] = {0ull, 0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int k = 0; k < RANK_WAVES; k++)
#pragma unroll
            for (int i = 0; i < RANK_COUNTS; i++) all[i] += part[k][i];
        info->counted = all[0];
        info->changed = all[1];
        info->ink_before = all[2];
        info->ink_after = all[3];
        info->spared = all[4];
    }
}

void rank_pages(const RankDesc* d_descs, int n_pages, int reg_blocks, int lds_blocks, hipStream_t s) {
    if (n_pages <= 0 || (reg_blocks <= 0 && lds_blocks <= 0)) return;
    if (reg_blocks > 0) hipLaunchKernelGGL(rank_kernel<true>, dim3(reg_blocks), dim3(RANK_THREADS), 0, s, d_descs, n_pages);
    if (lds_blocks > 0) hipLaunchKernelGGL(rank_kernel<false>, dim3(lds_blocks), dim3(RANK_THREADS), 0, s, d_descs, n_pages);
    hipLaunchKernelGGL(rank_info_kernel, dim3(n_pages), dim3(RANK_THREADS), 0, s, d_descs);
}

}  // namespace k
}  // namespace ocrs
