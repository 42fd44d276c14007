// The descriptor search of the kernels that take a batch of pages in one launch: block b of the grid
// belongs to the last descriptor whose first block (block0, ascending from 0) is <= b.  Uniform in the block: scalar loads.
#pragma once
#include <hip/hip_runtime.h>

namespace ocrs {
namespace k {

template <class Desc>
__device__ __forceinline__ int find_desc(const Desc* __restrict__ descs, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].block0 <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace k
}  // namespace ocrs
