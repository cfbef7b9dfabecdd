// The step in front of the model for arbitrary-scale evaluation (evaluation.py:67-89 pad_for_multi_train,
// evaluation_validate.py:92-106 pad_for_multi_train_Fixed, models/*/utils/utils.py:7-26 InputPadder), on the device.
//
// as_prepare_pair: bicubic down-scale, replicate pad and optional uint8 -> fp32 of BOTH images in one launch.  A padded output
// pixel (y, x) is the resized pixel at (clamp(y - top, 0, h_lr - 1), clamp(x - left, 0, w_lr - 1)): padding comes after resizing.
// The resize is ATen's upsample_bicubic2d(align_corners=False), no antialiasing: A = -0.75, scale = (float)in / (float)out,
// src = scale * (dst + 0.5f) - 0.5f (not clamped at 0), i = floor(src), t = src - i, taps i-1 .. i+2 clamped into the image, weights
// c2(t+1), c1(t), c1(1-t), c2(2-t); four horizontal sums, then the vertical one; the result is not clamped to 0..255.
// One thread = one padded pixel of all six planes (2 images x 3 channels): the eight weights and the eight clamped tap indices are
// formed once and serve 6 x 16 loads.  A block is a 64 x 4 output tile, so a wave reads runs of one input row (a lane's taps lie
// `scale` <= 3 elements from its neighbour's) and the four rows of a tile share their taps through the cache.  When the low-res
// frame is the input frame (scale 1, the fixed protocol) the kernel is a clamped copy: the bits of F.pad(x.float(), "replicate").
//
// as_query_grid: hr_coord [B, h_want * w_want, 2] of the same protocol, written straight into device memory.  The grid is rank-1:
// channel 0 is a function of the row, channel 1 of the column.  A block owns kRows query rows x kCols columns of one batch element;
// it builds its slice of the two 1-D tables in LDS (make_coord's values of the high-res frame, cropped by the scaled padding and,
// when the crop is not the wanted shape, resized 1-D as ATen's bilinear does) and then only stores: one 16-byte store = two
// queries.  A row starts at query b * Q + y * w_want of the flat output; when that is odd (odd w_want) the row's pairs are shifted
// by one query, so every 16-byte store stays aligned and the row's first / last query goes out as an 8-byte store.
//
// Every operation of the coordinate arithmetic is rounded on its own, as the torch ops it restates are: no FMA contraction in
// this file.
#include "common.h"
#include "cubic.h"
#include "query.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

// ---- as_prepare_pair ----
constexpr int kTileX = 64;
constexpr int kTileY = kThreads / kTileX;
using as::cubic_axis;  // taps and weights of one axis (cubic.h, shared with resize_disp.hip)

template <typename T, bool kResize>
__global__ __launch_bounds__(kThreads) void prepare_pair_kernel(const T* __restrict__ in1, const T* __restrict__ in2,
                                                                float* __restrict__ out1, float* __restrict__ out2, int H, int W,
                                                                int h_lr, int w_lr, int top, int left, int h_pad, int w_pad,
                                                                float scale_h, float scale_w) {
  const int x = blockIdx.x * kTileX + (threadIdx.x % kTileX);
  const int y = blockIdx.y * kTileY + (threadIdx.x / kTileX);
  if (x >= w_pad || y >= h_pad) return;
  const int b = blockIdx.z;
  const int ry = min(max(y - top, 0), h_lr - 1), rx = min(max(x - left, 0), w_lr - 1);  // replicate pad of the resized frame
  const long long plane_in = (long long)H * W, plane_out = (long long)h_pad * w_pad;
  const long long o = (long long)b * 3 * plane_out + (long long)y * w_pad + x;
  const T* src[2] = {in1 + (long long)b * 3 * plane_in, in2 + (long long)b * 3 * plane_in};
  float* dst[2] = {out1 + o, out2 + o};
  if (!kResize) {  // h_lr == H, w_lr == W
    const long long i = (long long)ry * W + rx;
#pragma unroll
    for (int im = 0; im < 2; ++im)
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[im][c * plane_out] = (float)src[im][c * plane_in + i];
    return;
  }
  int iy[4], ix[4];
  float wy[4], wx[4];
  cubic_axis(ry, scale_h, H, iy, wy);
  cubic_axis(rx, scale_w, W, ix, wx);
  long long row_off[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) row_off[a] = (long long)iy[a] * W;
  // The kernel is bound by the issue and the latency of its 96 gathered loads, not by their bytes: all 48 taps of an image
  // (3 planes x 16) are issued before the first is used, so a wave has 48 loads in flight instead of the one or two of a
  // load-multiply-add chain.
#pragma unroll
  for (int im = 0; im < 2; ++im) {
    T v[3][4][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[c][a][k] = src[im][c * plane_in + row_off[a] + ix[k]];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float rows[4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
        rows[a] = (float)v[c][a][0] * wx[0] + (float)v[c][a][1] * wx[1] + (float)v[c][a][2] * wx[2] + (float)v[c][a][3] * wx[3];
      dst[im][c * plane_out] = rows[0] * wy[0] + rows[1] * wy[1] + rows[2] * wy[2] + rows[3] * wy[3];
    }
  }
}

// ---- as_query_grid ----
constexpr int kRows = 8;               // query rows of a block
constexpr int kCols = 2 * kThreads;    // query columns of a block: one pair per thread and row

struct Axis {
  float c0, step;   // make_coord of the high-res frame: seq[i] = c0 + step * i, c0 = fl(-1 + 1/n), step = fl(2/n)
  int lo;           // first index of the crop (the scaled padding in front)
  int n_crop;       // length of the crop
  float scale;      // (float)n_crop / (float)n_want of the 1-D bilinear resize
};

__device__ __forceinline__ float crop_value(const Axis& a, int i) { return a.c0 + a.step * (float)(a.lo + i); }

// value d of the 1-D table of an axis
__device__ __forceinline__ float table_value(const Axis& a, int d, bool resized) {
  if (!resized) return crop_value(a, d);
  const float src = fmaxf(a.scale * ((float)d + 0.5f) - 0.5f, 0.f);
  const int i0 = min((int)floorf(src), a.n_crop - 1);
  const int i1 = min(i0 + 1, a.n_crop - 1);
  const float l1 = src - (float)i0, l0 = 1.f - l1;
  return l0 * crop_value(a, i0) + l1 * crop_value(a, i1);
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void query_grid_kernel(float* __restrict__ out, Axis ah, Axis aw, int h_want, int w_want,
                                                              int resized) {
  __shared__ float col[kCols + 2];  // col[j] = column table at x0 - 1 + j
  __shared__ float row[kRows];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kCols, y0 = blockIdx.y * kRows;
  const int b = blockIdx.z;
  for (int j = tid; j < kCols + 2; j += kThreads) {
    const int x = x0 - 1 + j;
    col[j] = (x >= 0 && x < w_want) ? table_value(aw, x, resized != 0) : 0.f;
  }
  if (tid < kRows) row[tid] = (y0 + tid < h_want) ? table_value(ah, y0 + tid, resized != 0) : 0.f;
  __syncthreads();
  const long long Q = (long long)h_want * w_want;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = y0 + r;
    if (y >= h_want) break;
    const long long q_row = (long long)b * Q + (long long)y * w_want;  // flat query index of (b, y, 0); 2 * B * Q < 2^31
    const int s = kVec ? (int)(q_row & 1) : 0;                         // an odd row start shifts the pairs by one query
    const int xa = x0 + 2 * tid - s, xb = xa + 1;                      // this thread's two queries; col index = x - x0 + 1
    // a pair belongs to the block in which its first query xa lies in [x0 - s, x0 + kCols - s): the blocks of a row tile it exactly
    // (xa = -1 only in the first block of a shifted row; an odd w_want is no multiple of kCols, so the last block reaches w_want - 1)
    const bool va = xa >= 0 && xa < w_want, vb = xb < w_want;
    const float ry = row[r];
    float* p = out + 2 * (q_row + xa);
    if (kVec && va && vb) {
      *reinterpret_cast<float4*>(p) = make_float4(ry, col[2 * tid - s + 1], ry, col[2 * tid - s + 2]);
    } else {
      if (va) *reinterpret_cast<float2*>(p) = make_float2(ry, col[2 * tid - s + 1]);
      if (vb) *reinterpret_cast<float2*>(p + 2) = make_float2(ry, col[2 * tid - s + 2]);
    }
  }
}

inline Axis make_axis(int n_hr, int lo, int n_crop, int n_want) {
  Axis a;
  const as::CoordAxis hr = as::coord_axis(n_hr);  // make_coord of the high-res frame (query.h)
  a.c0 = hr.c0; a.step = hr.s;
  a.lo = lo;
  a.n_crop = n_crop;
  a.scale = (float)n_crop / (float)n_want;
  return a;
}

}  // namespace

extern "C" {

int as_prepare_pair(const void* image1, const void* image2, float* out1, float* out2, int is_uint8, int B, int H, int W, int h_lr,
                    int w_lr, int pad_top, int pad_bottom, int pad_left, int pad_right, void* stream) {
  AS_REQUIRE(image1 && image2 && out1 && out2, AS_ERR_BAD_ARG, "prepare_pair: null pointer");
  AS_REQUIRE(B > 0 && H > 0 && W > 0 && h_lr > 0 && w_lr > 0, AS_ERR_BAD_ARG, "prepare_pair: non-positive size");
  AS_REQUIRE(pad_top >= 0 && pad_bottom >= 0 && pad_left >= 0 && pad_right >= 0, AS_ERR_BAD_ARG, "prepare_pair: negative padding");
  AS_REQUIRE(h_lr <= H && w_lr <= W, AS_ERR_BAD_SHAPE, "prepare_pair: low-res frame %dx%d larger than the image %dx%d (down-scaling only)",
             h_lr, w_lr, H, W);
  const int64_t h_pad = (int64_t)h_lr + pad_top + pad_bottom, w_pad = (int64_t)w_lr + pad_left + pad_right;
  AS_REQUIRE((int64_t)B * 3 * H * W <= 2147483647ll && (int64_t)B * 3 * h_pad * w_pad <= 2147483647ll, AS_ERR_BAD_SHAPE,
             "prepare_pair: more than 2^31-1 elements per tensor");
  AS_REQUIRE(B <= 65535, AS_ERR_BAD_SHAPE, "prepare_pair: B=%d above 65535", B);
  const int64_t gy = as::cdiv64(h_pad, kTileY);
  AS_REQUIRE(gy <= 65535, AS_ERR_BAD_SHAPE, "prepare_pair: padded height %lld above %d", (long long)h_pad, 65535 * kTileY);
  const dim3 grid((unsigned)as::cdiv64(w_pad, kTileX), (unsigned)gy, (unsigned)B);
  const bool resize = h_lr != H || w_lr != W;
  const float sh = (float)H / (float)h_lr, sw = (float)W / (float)w_lr;
  hipStream_t s = as::as_stream(stream);
#define AS_PREPARE_LAUNCH(T, R)                                                                                              \
  hipLaunchKernelGGL((prepare_pair_kernel<T, R>), grid, dim3(kThreads), 0, s, (const T*)image1, (const T*)image2, out1, out2, H, W, \
                     h_lr, w_lr, pad_top, pad_left, (int)h_pad, (int)w_pad, sh, sw)
  if (is_uint8) {
    if (resize) AS_PREPARE_LAUNCH(unsigned char, true); else AS_PREPARE_LAUNCH(unsigned char, false);
  } else {
    if (resize) AS_PREPARE_LAUNCH(float, true); else AS_PREPARE_LAUNCH(float, false);
  }
#undef AS_PREPARE_LAUNCH
  return as::check_launch("prepare_pair");
}

int as_query_grid(float* hr_coord, int B, int h_hr, int w_hr, int p_top, int p_bottom, int p_left, int p_right, int h_want, int w_want,
                  void* stream) {
  AS_REQUIRE(hr_coord, AS_ERR_BAD_ARG, "query_grid: null pointer");
  // a query is stored as one 8-byte pair; 16-byte alignment (any torch allocation) selects the 16-byte stores below
  AS_REQUIRE(reinterpret_cast<uintptr_t>(hr_coord) % 8 == 0, AS_ERR_BAD_ARG, "query_grid: hr_coord is not 8-byte aligned");
  AS_REQUIRE(B > 0 && h_hr > 0 && w_hr > 0 && h_want > 0 && w_want > 0, AS_ERR_BAD_ARG, "query_grid: non-positive size");
  AS_REQUIRE(p_top >= 0 && p_bottom >= 0 && p_left >= 0 && p_right >= 0, AS_ERR_BAD_ARG, "query_grid: negative padding");
  const int64_t h_crop = (int64_t)h_hr - p_top - p_bottom, w_crop = (int64_t)w_hr - p_left - p_right;
  AS_REQUIRE(h_crop > 0 && w_crop > 0, AS_ERR_BAD_SHAPE, "query_grid: the padding (%d,%d,%d,%d) leaves no crop of the %dx%d grid", p_top,
             p_bottom, p_left, p_right, h_hr, w_hr);
  AS_REQUIRE((int64_t)B * h_want * w_want * 2 <= 2147483647ll, AS_ERR_BAD_SHAPE, "query_grid: more than 2^31-1 output elements");
  AS_REQUIRE(B <= 65535, AS_ERR_BAD_SHAPE, "query_grid: B=%d above 65535", B);
  const int64_t gy = as::cdiv64(h_want, kRows);
  AS_REQUIRE(gy <= 65535, AS_ERR_BAD_SHAPE, "query_grid: h_want=%d above %d", h_want, 65535 * kRows);
  const Axis ah = make_axis(h_hr, p_top, (int)h_crop, h_want), aw = make_axis(w_hr, p_left, (int)w_crop, w_want);
  const int resized = (h_crop != h_want || w_crop != w_want) ? 1 : 0;
  const dim3 grid((unsigned)as::cdiv64(w_want, kCols), (unsigned)gy, (unsigned)B);
  hipStream_t s = as::as_stream(stream);
  if (reinterpret_cast<uintptr_t>(hr_coord) % 16 == 0)
    hipLaunchKernelGGL(query_grid_kernel<true>, grid, dim3(kThreads), 0, s, hr_coord, ah, aw, h_want, w_want, resized);
  else
    hipLaunchKernelGGL(query_grid_kernel<false>, grid, dim3(kThreads), 0, s, hr_coord, ah, aw, h_want, w_want, resized);
  return as::check_launch("query_grid");
}

}  // extern "C"
