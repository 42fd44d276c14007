// What the kernels of the page operations share on the device: kernels_normalize.hip, kernels_rules.hip,
// kernels_speckle.hip, kernels_binarize.hip, kernels_morph.hip, kernels_frame.hip, kernels_rank.hip, kernels_measure.hip, kernels_reverse.hip.  The grey-level bins are part of the bit-exact contract
// with tests/*_ref.py: they are defined here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ocrs {
namespace k {

typedef unsigned long long u64;
// The pointers come out of a descriptor in memory, where the compiler cannot see their address space: say it, so that
// the accesses are global_ instructions and not flat_ ones.  (A file's `ginfo` is its own info record: it stays there.)
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) uint32_t gword;
typedef __attribute__((address_space(1))) uint8_t gbyte;
typedef __attribute__((address_space(1))) u64 gu64;

__device__ __forceinline__ u64 shfl_xor64(u64 v, int mask) {
    const int lo = __shfl_xor((int)(uint32_t)v, mask), hi = __shfl_xor((int)(uint32_t)(v >> 32), mask);
    return (u64)(uint32_t)lo | ((u64)(uint32_t)hi << 32);
}

// sum over the wave; all 64 lanes call it together
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += shfl_xor64(v, d);
    return v;
}

__device__ __forceinline__ float clamp01(float a) { return a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a); }   // NaN stays

// the bin of a grey level, or of normalisation's u (§7.4); -1: NaN, not counted
__device__ __forceinline__ int bin_of(float g) {
    const float t = g * 256.0f;
    if (t != t) return -1;
    float f = floorf(t);
    f = f < 0.0f ? 0.0f : (f > 255.0f ? 255.0f : f);
    return (int)f;
}

// One bin per lane (-1: none) into this wave's histogram, runs of equal bins merged (§7.4).  All 64 lanes call it together.
__device__ __forceinline__ void hist_add(uint32_t* __restrict__ wave_hist, int bin, int lane) {
    const int left = __shfl_up(bin, 1);
    const bool head = lane == 0 || left != bin;
    const u64 heads = __ballot(head);
    if (head && bin >= 0) {
        const u64 rest = lane == 63 ? 0ull : heads >> (lane + 1);
        const int run = rest ? __builtin_ctzll(rest) + 1 : 64 - lane;
        atomicAdd(&wave_hist[bin], (uint32_t)run);
    }
}

}  // namespace k
}  // namespace ocrs
