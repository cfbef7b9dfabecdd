// ATen's upsample_bicubic2d(align_corners=False), no antialiasing, stated once for the kernels that restate it (prepare.hip,
// resize_disp.hip): A = -0.75, scale = (float)in / (float)out, src = scale * (dst + 0.5f) - 0.5f (not clamped at 0), i = floor(src),
// t = src - i, taps i-1 .. i+2 clamped into [0, n_in), weights c2(t+1), c1(t), c1(1-t), c2(2-t).  The callers sum the four
// horizontal products left to right, then the four vertical ones.
//
// Every operation is rounded on its own, as the torch ops are: FMA contraction is switched off HERE, at file scope, so it stays
// off for the rest of the including translation unit too — both includers want that.
#pragma once

#pragma clang fp contract(off)

namespace as {

constexpr float kCubicA = -0.75f;

__device__ __forceinline__ float cubic1(float x) { return ((kCubicA + 2.f) * x - (kCubicA + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x) { return ((kCubicA * x - 5.f * kCubicA) * x + 8.f * kCubicA) * x - 4.f * kCubicA; }

// taps and weights of one axis for the resized index d
__device__ __forceinline__ void cubic_axis(int d, float scale, int n_in, int idx[4], float w[4]) {
  const float src = scale * ((float)d + 0.5f) - 0.5f;
  const float fl = floorf(src);
  const float t = src - fl;
  const int i = (int)fl;
#pragma unroll
  for (int k = 0; k < 4; ++k) idx[k] = min(max(i - 1 + k, 0), n_in - 1);
  w[0] = cubic2(t + 1.f);
  w[1] = cubic1(t);
  w[2] = cubic1(1.f - t);
  w[3] = cubic2(2.f - t);
}

}  // namespace as
