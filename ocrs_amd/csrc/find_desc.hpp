// The descriptor search of the kernels that take a batch of pages in one launch: block b of the grid
// belongs to the last descriptor whose first block (block0, ascending from 0) is <= b.  Uniform in the block: scalar loads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ocrs {
namespace k {

// the same on any ascending prefix of the descriptors: a kernel whose grid is cut by another count than block0's
template <class Desc>
__device__ __forceinline__ int find_desc(const Desc* __restrict__ descs, int n, int b, int32_t Desc::*first) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].*first <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <class Desc>
__device__ __forceinline__ int find_desc(const Desc* __restrict__ descs, int n, int b) {
    return find_desc(descs, n, b, &Desc::block0);
}

}  // namespace k
}  // namespace ocrs
