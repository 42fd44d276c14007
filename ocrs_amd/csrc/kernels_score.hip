// Detection confidence: per external component of the text mask its pixel count and the sum of its
// pixels' probabilities in 24-bit fixed point.  The stage belongs to the component stage of kernels_ccl.hip and reads what
// that stage leaves behind (label forest, raster-sorted roots); it is a translation unit of its own because the component
// kernels of an UNSCORED request ran measurably slower with these kernels in their code object (§7.1, "Cost").
#include "common.hpp"
#include "kernels.hpp"

namespace ocrs {
namespace k {

// Root of x in the label forest as ccl_label leaves it (labels are page-local linear indices; the root of a foreground
// component is its raster-first pixel).  Read-only: the forest is not flattened (kernels_ccl.hip, is_external_root).
__device__ __forceinline__ int uf_find(const int32_t* L, int x) {
    while (x >= 0) {
        int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
    return -1;
}

// ---------------------------------------------------------------------------
// Component scores: per external component its pixel count and the sum of its pixels' probabilities in
// 24-bit fixed point.  Runs after ccl_label: the label forest is walked read-only to the root (no flattening pass: kernels_ccl.hip,
// is_external_root), and a root's slot is its position in the raster-sorted `roots` of its page.  Integer adds commute, so the
// result does not depend on the order in which waves arrive, on the kernel form or on the batch a page is part of.
// ---------------------------------------------------------------------------
// q(p) = floor(clamp(p, 0, 1) * 2^24): the product is exact in fp32 (a 24-bit significand times a power of two)
__device__ __forceinline__ uint32_t score_quant(float p) {
    return (uint32_t)(fminf(fmaxf(p, 0.0f), 1.0f) * 16777216.0f);
}

// sum over the wave's 64 lanes, in every lane (all lanes active)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// Position of `key` in the ascending R[0 .. cnt), or -1.  By the whole wave (uniform arguments, all lanes active): each
// round the lanes probe 64 evenly spaced entries and a ballot picks the interval — 2 rounds up to 4 096 roots, 3 up to
// 262 144, instead of 12-18 dependent loads by one lane.
__device__ __forceinline__ int find_root_slot(const int32_t* __restrict__ R, int cnt, int key, int lane) {
    int lo = 0, span = cnt;
    while (span > 0) {
        const int step = (span + 63) >> 6;
        const int v = (lane * step < span) ? R[lo + lane * step] : 0x7fffffff;
        const unsigned long long le = __ballot(v <= key);
        if (!le) return -1;
        const int k = __popcll(le) - 1;             // ascending: the lanes with v <= key are a prefix
        if (step == 1) return __shfl(v, k) == key ? lo + k : -1;
        lo += k * step;
        span = min(step, span - k * step);
    }
    return -1;
}

// QUAD: four pixels per thread (w % 4 == 0, word-aligned buffers), a wave covers 256 pixels of a row; else one pixel per
// thread and 64 per wave.  r[j] < 0: pixel j contributes nothing.  Both forms add the same integers to the same slots.
template <bool QUAD>
__global__ void __launch_bounds__(256)
component_scores_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ map, const int32_t* __restrict__ labels,
                        int h, int w, const int32_t* __restrict__ n_roots, const int32_t* __restrict__ roots,
                        uint32_t* __restrict__ pixels, unsigned long long* __restrict__ sums, int max_comp) {
    constexpr int PX = QUAD ? 4 : 1;
    const int n = blockIdx.z, y = blockIdx.y;
    const int cnt = n_roots[n];
    if (cnt <= 0 || cnt > max_comp) return;    // > max_comp: the page's component stage is re-run with larger buffers (engine.cpp), scores included
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * PX;
    const int lane = threadIdx.x & 63;
    const int64_t page = (int64_t)n * h * w;
    const int32_t* L = labels + page;
    const int p0 = y * w + x0;
    int r[PX];
    uint32_t q[PX];
#pragma unroll
    for (int j = 0; j < PX; j++) { r[j] = -1; q[j] = 0; }
    if (x0 < w) {                  // QUAD: w % 4 == 0, a thread is inside or outside the row as a whole
        if (QUAD) {
            const uint32_t mv = *reinterpret_cast<const uint32_t*>(mask + page + p0);
            if (mv) {
                const float4 pv = *reinterpret_cast<const float4*>(map + page + p0);
                const float pf[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (!((mv >> (8 * j)) & 0xFF)) continue;
                    // horizontally adjacent foreground pixels are one component: one walk per run
                    const int west = j > 0 ? r[j - 1] : -1;
                    r[j] = west >= 0 ? west : uf_find(L, p0 + j);
                    q[j] = score_quant(pf[j]);
                }
            }
        } else if (mask[page + p0]) {
            r[0] = uf_find(L, p0);
            q[0] = score_quant(map[page + p0]);
        }
    }
    // Almost all foreground pixels of a wave share one or two roots: one round per distinct root, the round's root being
    // the first pending lane's.  Count and sum are reduced over the wave; then one slot search and two atomics per root.
    const int32_t* R = roots + (int64_t)n * max_comp;
    for (;;) {
        int mine = -1;
#pragma unroll
        for (int j = PX - 1; j >= 0; j--) mine = r[j] >= 0 ? r[j] : mine;
        const unsigned long long pending = __ballot(mine >= 0);
        if (!pending) break;
        const int cur = __shfl(mine, __ffsll((long long)pending) - 1);
        uint32_t c = 0, s = 0;     // s <= 4 * 2^24
#pragma unroll
        for (int j = 0; j < PX; j++)
            if (r[j] == cur) { c++; s += q[j]; r[j] = -1; }
        // the wave's sum may reach 2^32: reduced as two 16-bit halves; the count (<= 256) rides above the high half (<= 2^16)
        const uint32_t lo = wave_sum_u32(s & 0xFFFFu);
        const uint32_t hc = wave_sum_u32((s >> 16) | (c << 20));
        const int slot = find_root_slot(R, cnt, cur, lane);
        if (slot >= 0 && lane == 0) {   // not in `roots`: a component inside a hole (not External)
            atomicAdd(&pixels[(int64_t)n * max_comp + slot], hc >> 20);
            atomicAdd(&sums[(int64_t)n * max_comp + slot], ((unsigned long long)(hc & 0xFFFFFu) << 16) + lo);
        }
    }
}

void component_scores(const uint8_t* d_mask, const float* d_map, int n, int h, int w, const CclBuffers& b, int max_comp,
                      hipStream_t s) {
    if (!d_map || !b.score_pixels || !b.score_sums) fail(OCRS_ERR_DEVICE, "internal: component scores without their buffers");
    (void)hipMemsetAsync(b.score_pixels, 0, (size_t)n * max_comp * sizeof(uint32_t), s);
    (void)hipMemsetAsync(b.score_sums, 0, (size_t)n * max_comp * sizeof(unsigned long long), s);
    const bool quad = option(OPT_CCL_QUAD) && (w & 3) == 0 && (((uintptr_t)d_mask) & 3) == 0 && (((uintptr_t)d_map) & 15) == 0;
    if (quad)
        hipLaunchKernelGGL((component_scores_kernel<true>), dim3((w + 1023) / 1024, h, n), dim3(256), 0, s, d_mask, d_map, b.labels,
                           h, w, b.n_roots, b.roots, b.score_pixels, b.score_sums, max_comp);
    else
        hipLaunchKernelGGL((component_scores_kernel<false>), dim3((w + 255) / 256, h, n), dim3(256), 0, s, d_mask, d_map, b.labels,
                           h, w, b.n_roots, b.roots, b.score_pixels, b.score_sums, max_comp);
}

}  // namespace k
}  // namespace ocrs
