// libanystereo_augment.so: photometric augmentation and eraser of a stereo pair on the device (include/anystereo_augment.h states
// the arithmetic; it is PIL's and numpy's, byte for byte).
//
//   grey_kernel    pass 1: applies the operations `order` puts before contrast and writes one grey sum per block.  Launched only if a
//                  contrast factor of the chunk is not 1; the blocks of an image whose factor is 1 leave at once.
//   write_kernel   pass 2: reduces the grey partials of its image (of both images of a shared sample) to the contrast level, applies
//                  the four operations and the gamma table, writes the outputs, and writes image2's channel sums per block where a
//                  rectangle follows.
//   rect_kernel    pass 3: one grid row per rectangle; reduces the channel partials to the mean colour and fills the clipped rectangle.
//
// A block is 256 threads and walks tiles of 2048 pixels of one plane triple (grid.x = min(tiles, 1024) blocks per image, tile += grid.x),
// a thread takes 8 consecutive pixels of each of the three planes: one 8-byte load per uint8 plane (two 16-byte loads per fp32 plane)
// where the address allows it, byte (dword) accesses otherwise and in the last, partial group — 8..16 B per lane is where a global
// access is as wide as it pays to be, and at the training shape (4 x 160 x 320) it still leaves 200 blocks for 256 CUs.
// Partial sums are uint64 in the workspace, written by every block that a consumer will read: nothing is cleared, nothing is atomic,
// every total is an integer and independent of the order of summation.
//
// No contraction in this file: blend is a product rounded, then a sum rounded.  fp32 quotients are formed in double and rounded once
// (correctly rounded whatever the fp32 division expands to).  anystereo/harness/augment.py restates every function below.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/anystereo_augment.h"
#include "../host/errstate.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 8;  // pixels of a thread per tile
static_assert(kThreads * kPer == AUG_TILE, "AUG_TILE is one block iteration");
typedef unsigned long long u64;

struct Table {
  aug_sample s[AUG_MAX_BATCH];
};

// ---- the arithmetic ----
__device__ __forceinline__ int grey(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ int blend(int x, int d, float f, bool clip) {
  float t = (float)d + f * (float)(x - d);
  if (clip) t = fminf(fmaxf(t, 0.f), 255.f);
  return (int)t;
}

__device__ __forceinline__ float fdiv(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ void rgb_to_hsv(int r, int g, int b, int& h, int& s, int& v) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  v = maxc;
  if (maxc == minc) {
    h = 0;
    s = 0;
    return;
  }
  const float cr = (float)(maxc - minc);
  const float sf = fdiv(cr, (float)maxc);
  const float rc = fdiv((float)(maxc - r), cr), gc = fdiv((float)(maxc - g), cr), bc = fdiv((float)(maxc - b), cr);
  float hf;
  if (r == maxc)
    hf = bc - gc;
  else if (g == maxc)
    hf = (float)((2.0 + (double)rc) - (double)bc);
  else
    hf = (float)((4.0 + (double)gc) - (double)rc);
  const double x = (double)hf / 6.0 + 1.0;  // in [5/6, 11/6]
  hf = (float)(x - floor(x));               // fmod(x, 1.0), exact
  h = clip8((int)((double)hf * 255.0));
  s = clip8((int)((double)sf * 255.0));
}

__device__ __forceinline__ int round8(double x) { return clip8((int)floor(x + 0.5)); }  // round() of a non-negative double

__device__ __forceinline__ void hsv_to_rgb(int h, int s, int v, int& r, int& g, int& b) {
  if (s == 0) {
    r = g = b = v;
    return;
  }
  const double hd = (double)h * 6.0 / 255.0;
  const double i = floor(hd);
  const float f = (float)(hd - i);
  const float fs = (float)((double)s / 255.0);
  const double vd = (double)v;
  const int p = round8(vd * (1.0 - (double)fs));
  const int q = round8(vd * (1.0 - (double)(fs * f)));
  const int t = round8(vd * (1.0 - (double)fs * (1.0 - (double)f)));
  switch ((int)i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

__device__ __forceinline__ void apply_op(int op, const aug_image_params& P, int level, int& r, int& g, int& b) {
  if (op == AUG_HUE) {
    int h, s, v;
    rgb_to_hsv(r, g, b, h, s, v);
    hsv_to_rgb((h + P.hue_shift) & 255, s, v, r, g, b);
    return;
  }
  const float f = P.factor[op];
  const bool clip = !(f >= 0.f && f <= 1.f);
  const int l = grey(r, g, b);
  const int d = op == AUG_BRIGHTNESS ? 0 : (op == AUG_CONTRAST ? level : l);
  r = blend(r, d, f, clip);
  g = blend(g, d, f, clip);
  b = blend(b, d, f, clip);
}

// ---- 8 pixels of one plane ----
__device__ __forceinline__ int quantise(float x) { return (int)fminf(fmaxf(floorf(x + 0.5f), 0.f), 255.f); }

__device__ __forceinline__ void load8(const unsigned char* p, int n, int* v) {
  if (n == kPer && ((uintptr_t)p & 7) == 0) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = (q.x >> (8 * k)) & 255;
      v[4 + k] = (q.y >> (8 * k)) & 255;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k) v[k] = k < n ? (int)p[k] : 0;
  }
}

__device__ __forceinline__ void load8(const float* p, int n, int* v) {
  if (n == kPer && ((uintptr_t)p & 15) == 0) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    const float x[kPer] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < kPer; ++k) v[k] = quantise(x[k]);
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k) v[k] = k < n ? quantise(p[k]) : 0;
  }
}

__device__ __forceinline__ void store8(unsigned char* p, int n, const int* v) {
  if (n == kPer && ((uintptr_t)p & 7) == 0) {
    uint2 q = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q.x |= (unsigned)v[k] << (8 * k);
      q.y |= (unsigned)v[4 + k] << (8 * k);
    }
    *reinterpret_cast<uint2*>(p) = q;
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (k < n) p[k] = (unsigned char)v[k];
  }
}

__device__ __forceinline__ void store8(float* p, int n, const int* v) {
  if (n == kPer && ((uintptr_t)p & 15) == 0) {
    reinterpret_cast<float4*>(p)[0] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4((float)v[4], (float)v[5], (float)v[6], (float)v[7]);
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (k < n) p[k] = (float)v[k];
  }
}

// the sum of v over the block, returned to every thread; every thread of the block must call this
__device__ __forceinline__ u64 block_sum(u64 v, u64* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const u64 total = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return total;
}

// the sum of count consecutive partials, to every thread
__device__ __forceinline__ u64 reduce_parts(const u64* __restrict__ part, int count, u64* sh) {
  u64 v = 0;
  for (int i = threadIdx.x; i < count; i += kThreads) v += part[i];
  return block_sum(v, sh);
}

// ---- kernels: grid (parts, 2 images, samples of the chunk); ws[sample][5][parts] ----
template <typename TIn>
__global__ __launch_bounds__(kThreads) void grey_kernel(Table tab, const TIn* __restrict__ in1, const TIn* __restrict__ in2, u64* __restrict__ ws,
                                                        int n, int tiles) {
  __shared__ u64 sh[4];
  const int img = blockIdx.y, b = blockIdx.z, parts = gridDim.x;
  const aug_sample& S = tab.s[b];
  const aug_image_params& P = S.img[S.shared ? 0 : img];
  if (P.factor[AUG_CONTRAST] == 1.f) return;  // the whole block: blend(x, m, 1) = x whatever m is, nobody reads this partial
  const TIn* in = (img == 0 ? in1 : in2) + (int64_t)b * 3 * n;
  unsigned sum = 0;  // < 342 tiles x 8 pixels x 255 per thread
  for (int tile = blockIdx.x; tile < tiles; tile += parts) {
    const int i0 = tile * AUG_TILE + threadIdx.x * kPer;
    const int cnt = min(n - i0, kPer);
    if (cnt <= 0) continue;
    int r[kPer], g[kPer], bl[kPer];
    load8(in + i0, cnt, r);
    load8(in + n + i0, cnt, g);
    load8(in + 2 * (int64_t)n + i0, cnt, bl);
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      for (int o = 0; o < 4 && P.order[o] != AUG_CONTRAST; ++o) apply_op(P.order[o], P, 0, r[k], g[k], bl[k]);
      if (k < cnt) sum += (unsigned)grey(r[k], g[k], bl[k]);
    }
  }
  const u64 total = block_sum(sum, sh);
  if (threadIdx.x == 0) ws[((int64_t)b * 5 + img) * parts + blockIdx.x] = total;
}

template <typename TIn, typename TOut>
__global__ __launch_bounds__(kThreads) void write_kernel(Table tab, const TIn* __restrict__ in1, const TIn* __restrict__ in2, TOut* __restrict__ out1,
                                                         TOut* __restrict__ out2, const unsigned char* __restrict__ lut, u64* __restrict__ ws, int n,
                                                         int tiles) {
  __shared__ u64 sh[4];
  __shared__ unsigned char table[256];
  const int img = blockIdx.y, b = blockIdx.z, parts = gridDim.x;
  const aug_sample& S = tab.s[b];
  const int pi = S.shared ? 0 : img;
  const aug_image_params& P = S.img[pi];
  int level = 0;
  if (P.factor[AUG_CONTRAST] != 1.f) {
    const u64 cnt = S.shared ? 2ull * (u64)n : (u64)n;
    const u64 sum = S.shared ? reduce_parts(ws + (int64_t)b * 5 * parts, 2 * parts, sh) : reduce_parts(ws + ((int64_t)b * 5 + img) * parts, parts, sh);
    level = (int)((2 * sum + cnt) / (2 * cnt));
  }
  if (lut != nullptr) {
    table[threadIdx.x] = lut[((int64_t)b * 2 + pi) * 256 + threadIdx.x];
    __syncthreads();
  }
  const TIn* in = (img == 0 ? in1 : in2) + (int64_t)b * 3 * n;
  TOut* out = (img == 0 ? out1 : out2) + (int64_t)b * 3 * n;
  const bool sums = img == 1 && S.n_rects > 0;
  unsigned cs[3] = {0u, 0u, 0u};
  for (int tile = blockIdx.x; tile < tiles; tile += parts) {
    const int i0 = tile * AUG_TILE + threadIdx.x * kPer;
    const int cnt = min(n - i0, kPer);
    if (cnt <= 0) continue;
    int r[kPer], g[kPer], bl[kPer];
    load8(in + i0, cnt, r);
    load8(in + n + i0, cnt, g);
    load8(in + 2 * (int64_t)n + i0, cnt, bl);
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      for (int o = 0; o < 4; ++o) apply_op(P.order[o], P, level, r[k], g[k], bl[k]);
      if (lut != nullptr) {
        r[k] = table[r[k]];
        g[k] = table[g[k]];
        bl[k] = table[bl[k]];
      }
      if (k < cnt) {
        cs[0] += (unsigned)r[k];
        cs[1] += (unsigned)g[k];
        cs[2] += (unsigned)bl[k];
      }
    }
    store8(out + i0, cnt, r);
    store8(out + n + i0, cnt, g);
    store8(out + 2 * (int64_t)n + i0, cnt, bl);
  }
  if (sums) {
    for (int c = 0; c < 3; ++c) {
      const u64 total = block_sum(cs[c], sh);
      if (threadIdx.x == 0) ws[((int64_t)b * 5 + 2 + c) * parts + blockIdx.x] = total;
    }
  }
}

// grid (blocks over the rectangle, AUG_MAX_RECTS, samples of the chunk)
template <typename TOut>
__global__ __launch_bounds__(kThreads) void rect_kernel(Table tab, TOut* __restrict__ out2, const u64* __restrict__ ws, int h, int w, int parts) {
  __shared__ u64 sh[4];
  const int rct = blockIdx.y, b = blockIdx.z;
  const aug_sample& S = tab.s[b];
  if (rct >= S.n_rects) return;
  const int n = h * w;
  const int x0 = S.rect[rct][0], y0 = S.rect[rct][1];
  const int rw = (int)min((int64_t)S.rect[rct][2], (int64_t)(w - x0)), rh = (int)min((int64_t)S.rect[rct][3], (int64_t)(h - y0));
  const int area = rw * rh;
  if ((int64_t)blockIdx.x * kThreads >= area) return;
  int mean[3];
  for (int c = 0; c < 3; ++c) mean[c] = (int)(reduce_parts(ws + ((int64_t)b * 5 + 2 + c) * parts, parts, sh) / (u64)n);
  TOut* out = out2 + (int64_t)b * 3 * n;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < area; i += gridDim.x * kThreads) {
    const int y = i / rw, x = i - y * rw;
    const int64_t o = (int64_t)(y0 + y) * w + (x0 + x);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[o + (int64_t)c * n] = (TOut)mean[c];
  }
}

// ---- host side ----
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// 3 * B * h * w, saturated at 2^31 (no intermediate leaves int64)
inline int64_t elements(int B, int h, int w) {
  const int64_t lim = 1ll << 31, hw = (int64_t)h * w;
  if (hw >= lim || (int64_t)B * hw >= lim) return lim;
  return 3 * (int64_t)B * hw;
}

inline int parts_of(int h, int w) {
  const int64_t tiles = ((int64_t)h * w + AUG_TILE - 1) / AUG_TILE;
  return (int)(tiles < AUG_MAX_PARTS ? tiles : AUG_MAX_PARTS);
}

int check_image_params(int b, int img, const aug_image_params& P) {
  int seen = 0;
  for (int o = 0; o < 4; ++o) {
    REQUIRE(P.order[o] >= 0 && P.order[o] <= 3 && !(seen & (1 << P.order[o])), AUG_ERR_BAD_ARG,
            "aug_photometric_pair: sample %d image %d: order = (%d, %d, %d, %d) is no permutation of 0..3", b, img + 1, P.order[0], P.order[1],
            P.order[2], P.order[3]);
    seen |= 1 << P.order[o];
  }
  for (int k = 0; k < 3; ++k)
    REQUIRE(isfinite(P.factor[k]) && P.factor[k] >= 0.f, AUG_ERR_BAD_ARG, "aug_photometric_pair: sample %d image %d: factor %d = %g must be finite and >= 0", b,
            img + 1, k, (double)P.factor[k]);
  REQUIRE(P.hue_shift >= 0 && P.hue_shift <= 255, AUG_ERR_BAD_ARG, "aug_photometric_pair: sample %d image %d: hue_shift = %d outside 0..255", b, img + 1,
          P.hue_shift);
  return AUG_OK;
}

template <typename TIn, typename TOut>
int launch_chunks(const TIn* in1, const TIn* in2, TOut* out1, TOut* out2, int B, int h, int w, const aug_sample* samples, const unsigned char* lut,
                  u64* ws, hipStream_t stream) {
  const int n = h * w, parts = parts_of(h, w);
  const int tiles = (int)(((int64_t)n + AUG_TILE - 1) / AUG_TILE);
  for (int b0 = 0; b0 < B; b0 += AUG_MAX_BATCH) {
    const int nb = B - b0 < AUG_MAX_BATCH ? B - b0 : AUG_MAX_BATCH;
    Table t;
    bool any_contrast = false;
    int64_t most = 0;  // the largest clipped rectangle of the chunk
    for (int i = 0; i < AUG_MAX_BATCH; ++i) {
      t.s[i] = samples[b0 + (i < nb ? i : 0)];  // unused slots repeat the first sample; no block reads them
      if (i >= nb) continue;
      const aug_sample& S = t.s[i];
      any_contrast = any_contrast || S.img[0].factor[AUG_CONTRAST] != 1.f || (!S.shared && S.img[1].factor[AUG_CONTRAST] != 1.f);
      for (int r = 0; r < S.n_rects; ++r) {
        const int64_t rw = S.rect[r][2] < w - S.rect[r][0] ? S.rect[r][2] : w - S.rect[r][0];
        const int64_t rh = S.rect[r][3] < h - S.rect[r][1] ? S.rect[r][3] : h - S.rect[r][1];
        if (rw * rh > most) most = rw * rh;
      }
    }
    const int64_t off = (int64_t)b0 * 3 * n;
    u64* wsb = ws + (int64_t)b0 * 5 * parts;
    const unsigned char* lutb = lut == nullptr ? nullptr : lut + (int64_t)b0 * 2 * 256;
    const dim3 grid((unsigned)parts, 2u, (unsigned)nb);
    if (any_contrast) {
      hipLaunchKernelGGL((grey_kernel<TIn>), grid, dim3(kThreads), 0, stream, t, in1 + off, in2 + off, wsb, n, tiles);
      if (int rc = check_launch("aug_photometric_pair (grey sums)", AUG_ERR_LAUNCH)) return rc;
    }
    hipLaunchKernelGGL((write_kernel<TIn, TOut>), grid, dim3(kThreads), 0, stream, t, in1 + off, in2 + off, out1 + off, out2 + off, lutb, wsb, n, tiles);
    if (int rc = check_launch("aug_photometric_pair (write-out)", AUG_ERR_LAUNCH)) return rc;
    if (most > 0) {
      int64_t gx = (most + kThreads - 1) / kThreads;
      if (gx > 256) gx = 256;
      hipLaunchKernelGGL((rect_kernel<TOut>), dim3((unsigned)gx, AUG_MAX_RECTS, (unsigned)nb), dim3(kThreads), 0, stream, t, out2 + off, wsb, h, w, parts);
      if (int rc = check_launch("aug_photometric_pair (rectangles)", AUG_ERR_LAUNCH)) return rc;
    }
  }
  return AUG_OK;
}

}  // namespace

extern "C" {

int aug_abi_version(void) { return 1; }

const char* aug_last_error_string(void) { return err_buf(); }

int64_t aug_workspace_bytes(int B, int h, int w) {
  if (B < 1 || h < 1 || w < 1) return -1;
  return (int64_t)B * 5 * parts_of(h, w) * (int64_t)sizeof(u64);
}

int aug_photometric_pair(const void* image1, const void* image2, int in_dtype, void* out1, void* out2, int out_dtype, int B, int h, int w,
                         const aug_sample* samples, const unsigned char* gamma_lut, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* what = "aug_photometric_pair";
  REQUIRE(image1 != nullptr && image2 != nullptr && out1 != nullptr && out2 != nullptr && samples != nullptr && workspace != nullptr, AUG_ERR_BAD_ARG,
          "%s: null pointer", what);
  REQUIRE((in_dtype == AUG_U8 || in_dtype == AUG_F32) && (out_dtype == AUG_U8 || out_dtype == AUG_F32), AUG_ERR_BAD_ARG,
          "%s: in_dtype=%d out_dtype=%d: AUG_U8 or AUG_F32 expected", what, in_dtype, out_dtype);
  REQUIRE(B >= 1 && h >= 1 && w >= 1, AUG_ERR_BAD_ARG, "%s: B=%d h=%d w=%d must be positive", what, B, h, w);
  REQUIRE(elements(B, h, w) < (1ll << 31), AUG_ERR_BAD_SHAPE, "%s: B=%d h=%d w=%d: need 3*B*h*w < 2^31", what, B, h, w);
  REQUIRE(in_dtype == AUG_U8 || (aligned(image1, 4) && aligned(image2, 4)), AUG_ERR_BAD_ARG, "%s: fp32 inputs must be 4-byte aligned", what);
  REQUIRE(out_dtype == AUG_U8 || (aligned(out1, 4) && aligned(out2, 4)), AUG_ERR_BAD_ARG, "%s: fp32 outputs must be 4-byte aligned", what);
  REQUIRE(aligned(workspace, 8), AUG_ERR_BAD_ARG, "%s: the workspace must be 8-byte aligned", what);
  for (int b = 0; b < B; ++b) {  // all samples before the first launch
    const aug_sample& S = samples[b];
    for (int img = 0; img < 2; ++img)
      if (int rc = check_image_params(b, img, S.img[img])) return rc;
    REQUIRE(S.shared == 0 || S.shared == 1, AUG_ERR_BAD_ARG, "%s: sample %d: shared = %d, 0 or 1 expected", what, b, S.shared);
    REQUIRE(S.n_rects >= 0 && S.n_rects <= AUG_MAX_RECTS, AUG_ERR_BAD_ARG, "%s: sample %d: %d rectangles, 0..%d expected", what, b, S.n_rects,
            AUG_MAX_RECTS);
    for (int r = 0; r < S.n_rects; ++r) {
      const int* q = S.rect[r];
      REQUIRE(q[2] > 0 && q[3] > 0, AUG_ERR_BAD_ARG, "%s: sample %d rectangle %d: extent %d x %d must be positive", what, b, r, q[2], q[3]);
      REQUIRE(q[0] >= 0 && q[0] < w && q[1] >= 0 && q[1] < h, AUG_ERR_BAD_ARG, "%s: sample %d rectangle %d: origin (%d, %d) outside the %d x %d frame",
              what, b, r, q[0], q[1], h, w);
    }
  }
  const int64_t need = aug_workspace_bytes(B, h, w);
  REQUIRE(workspace_bytes >= need, AUG_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", what, (long long)workspace_bytes, (long long)need);
  const int64_t elems = 3ll * B * h * w;
  const int64_t nin = elems * (in_dtype == AUG_F32 ? 4 : 1), nout = elems * (out_dtype == AUG_F32 ? 4 : 1);
  const void* outs[2] = {out1, out2};
  for (int o = 0; o < 2; ++o) {
    REQUIRE(!overlap(outs[o], nout, image1, nin) && !overlap(outs[o], nout, image2, nin), AUG_ERR_ALIAS, "%s: out%d overlaps an input", what, o + 1);
    REQUIRE(!overlap(outs[o], nout, workspace, need), AUG_ERR_ALIAS, "%s: out%d overlaps the workspace", what, o + 1);
    REQUIRE(gamma_lut == nullptr || !overlap(outs[o], nout, gamma_lut, (int64_t)B * 512), AUG_ERR_ALIAS, "%s: out%d overlaps gamma_lut", what, o + 1);
  }
  REQUIRE(!overlap(out1, nout, out2, nout), AUG_ERR_ALIAS, "%s: out1 overlaps out2", what);
  REQUIRE(!overlap(workspace, need, image1, nin) && !overlap(workspace, need, image2, nin), AUG_ERR_ALIAS, "%s: the workspace overlaps an input", what);

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  u64* ws = reinterpret_cast<u64*>(workspace);
  if (in_dtype == AUG_U8 && out_dtype == AUG_U8)
    return launch_chunks((const unsigned char*)image1, (const unsigned char*)image2, (unsigned char*)out1, (unsigned char*)out2, B, h, w, samples, gamma_lut, ws, s);
  if (in_dtype == AUG_U8)
    return launch_chunks((const unsigned char*)image1, (const unsigned char*)image2, (float*)out1, (float*)out2, B, h, w, samples, gamma_lut, ws, s);
  if (out_dtype == AUG_U8)
    return launch_chunks((const float*)image1, (const float*)image2, (unsigned char*)out1, (unsigned char*)out2, B, h, w, samples, gamma_lut, ws, s);
  return launch_chunks((const float*)image1, (const float*)image2, (float*)out1, (float*)out2, B, h, w, samples, gamma_lut, ws, s);
}

}  // extern "C"
