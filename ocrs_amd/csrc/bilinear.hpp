// Bilinear resize arithmetic, ONNX Resize linear / half_pixel (rten resize_image; detection.rs:168,194, recognition.rs:121),
// shared by the kernels that resize (kernels_image.hip, kernels_resample.hip).  Build with -ffp-contract=off: every
// operation is rounded on its own.
//   c   = clamp((o + 0.5) * (in/out) - 0.5, 0, in-1);  i0 = (int)c; i1 = min(i0+1, in-1)
//   out = (1-wy) * ((1-wx)*tl + wx*tr) + wy * ((1-wx)*bl + wx*br)
#pragma once
#include <hip/hip_runtime.h>

namespace ocrs {
namespace k {

__device__ __forceinline__ void resize_axis(int o, int in_len, int out_len, int& i0, int& i1, float& wgt) {
    float scale = (float)in_len / (float)out_len;
    float c = ((float)o + 0.5f) * scale - 0.5f;
    float hi = (float)(in_len - 1);
    c = c < 0.0f ? 0.0f : c;
    c = c > hi ? hi : c;
    int a = (int)c;
    i0 = a;
    i1 = a + 1 < in_len ? a + 1 : in_len - 1;
    wgt = c - (float)a;
}

__device__ __forceinline__ float bilerp(float tl, float tr, float bl, float br, float wx, float wy) {
    float top = (1.0f - wx) * tl + wx * tr;
    float bot = (1.0f - wx) * bl + wx * br;
    return (1.0f - wy) * top + wy * bot;
}

}  // namespace k
}  // namespace ocrs
