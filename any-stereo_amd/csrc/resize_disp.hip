// The interpolation baseline of arbitrary-scale evaluation (evaluation.py:91-100 pad_for_muti_other, :125-146 the `multi_evaothers`
// branch), on the device: a fixed-scale disparity map predicted on the padded low-resolution frame is un-padded, multiplied by the
// scale and resized to the full frame,
//     F.interpolate(padder.unpad(flow_pr) * scale_test, (H, W), mode='bicubic', align_corners=False).
//
// as_resize_disp: out[n, y, x] = bicubic over (src[n, top : top + hc, left : left + wc] * mul) -> [N, H, W], all N maps in one
// launch.  The arithmetic is ATen's upsample_bicubic2d on the product tensor: every tap is multiplied by `mul` first (one rounding,
// the reference's `flow_pr * scale_test`), then four horizontal 4-tap sums and the vertical one with the weights of cubic.h.  The
// taps are clamped to the CROP WINDOW, not to the padded source frame: the reference un-pads before it interpolates, so a value of
// the padding never enters the result.  When the crop already has the output's shape the cubic weights are (0, 1, 0, 0) exactly and
// the kernel is the copy of crop * mul (mul == 1: the crop's bits; the reference skips the resize for scale_test <= 1).
// One thread = one output pixel; a block is a 64 x 4 output tile, so a wave reads runs of one source row and the four rows of a
// tile share their taps through the cache.  All 16 taps are loaded before the first is used.  Offsets are 64-bit.
//
// No FMA contraction in this file (cubic.h switches it off for the translation unit).
#include "common.h"
#include "cubic.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTileX = 64;
constexpr int kTileY = kThreads / kTileX;

template <bool kResize>
__global__ __launch_bounds__(kThreads) void resize_disp_kernel(const float* __restrict__ src, float* __restrict__ out, int Hs, int Ws,
                                                               int top, int left, int hc, int wc, int H, int W, float mul,
                                                               float scale_h, float scale_w) {
  const int x = blockIdx.x * kTileX + (threadIdx.x % kTileX);
  const int y = blockIdx.y * kTileY + (threadIdx.x / kTileX);
  if (x >= W || y >= H) return;
  const long long n = blockIdx.z;
  // first element of the crop of map n; every tap index below lies in [0, hc) x [0, wc), so every load lies inside the crop
  const float* crop = src + n * ((long long)Hs * Ws) + (long long)top * Ws + left;
  float* dst = out + n * ((long long)H * W) + (long long)y * W + x;
  if (!kResize) {  // hc == H, wc == W
    *dst = crop[(long long)y * Ws + x] * mul;
    return;
  }
  int iy[4], ix[4];
  float wy[4], wx[4];
  as::cubic_axis(y, scale_h, hc, iy, wy);
  as::cubic_axis(x, scale_w, wc, ix, wx);
  float v[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[a][k] = crop[(long long)iy[a] * Ws + ix[k]];
  float rows[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
    rows[a] = (v[a][0] * mul) * wx[0] + (v[a][1] * mul) * wx[1] + (v[a][2] * mul) * wx[2] + (v[a][3] * mul) * wx[3];
  *dst = rows[0] * wy[0] + rows[1] * wy[1] + rows[2] * wy[2] + rows[3] * wy[3];
}

}  // namespace

extern "C" {

int as_resize_disp(const float* src, float* out, int N, int Hs, int Ws, int top, int left, int hc, int wc, int H, int W, float mul,
                   void* stream) {
  AS_REQUIRE(src && out, AS_ERR_BAD_ARG, "resize_disp: null pointer");
  AS_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, AS_ERR_BAD_ARG, "resize_disp: non-positive size");
  AS_REQUIRE(hc > 0 && wc > 0, AS_ERR_BAD_SHAPE, "resize_disp: empty crop %dx%d", hc, wc);
  AS_REQUIRE(top >= 0 && left >= 0 && (int64_t)top + hc <= Hs && (int64_t)left + wc <= Ws, AS_ERR_BAD_SHAPE,
             "resize_disp: the crop (top %d, left %d, %dx%d) leaves the %dx%d source", top, left, hc, wc, Hs, Ws);
  AS_REQUIRE(N <= 65535, AS_ERR_BAD_SHAPE, "resize_disp: N=%d above 65535", N);
  const int64_t gy = as::cdiv64(H, kTileY);
  AS_REQUIRE(gy <= 65535, AS_ERR_BAD_SHAPE, "resize_disp: H=%d above %d", H, 65535 * kTileY);
  const dim3 grid((unsigned)as::cdiv64(W, kTileX), (unsigned)gy, (unsigned)N);
  const float sh = (float)hc / (float)H, sw = (float)wc / (float)W;
  hipStream_t s = as::as_stream(stream);
  if (hc != H || wc != W)
    hipLaunchKernelGGL(resize_disp_kernel<true>, grid, dim3(kThreads), 0, s, src, out, Hs, Ws, top, left, hc, wc, H, W, mul, sh, sw);
  else
    hipLaunchKernelGGL(resize_disp_kernel<false>, grid, dim3(kThreads), 0, s, src, out, Hs, Ws, top, left, hc, wc, H, W, mul, sh, sw);
  return as::check_launch("resize_disp");
}

}  // extern "C"
