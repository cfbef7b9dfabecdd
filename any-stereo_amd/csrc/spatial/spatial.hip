// libanystereo_spatial.so (include/anystereo_spatial.h): the spatial augmentation of a stereo pair — rescale, flip, y-jitter, crop and
// the final bicubic resize of the reference's augmentor — as two gather kernels.  No rescaled frame is materialised: an output pixel
// maps to ONE pixel of the (flipped) rescaled frame by index arithmetic, and that pixel is computed from its four source pixels
// (dense) or searched among the few source pixels that can land on it (sparse).
//
//   image_kernel   out1, out2 [B,3,h_out,w_out]: the crop itself, or with a final resize the 4 x 4 crop pixels of csrc/cubic.h's
//                  taps, each quantised as the reference holds uint8 between its two resizes.  One thread per output pixel and
//                  image, the three planes share the coordinates.
//   truth_kernel   the ragged ground-truth crops: the bilinear rule times scale_x (dense), the last-in-raster-order gather (sparse)
//                  or a bit copy (no rescale).  No atomics: every output element has one writer and one value.
//
// anystereo/harness/spatial.py (`spatial_pair_host`) restates this arithmetic with numpy; an edit of one is an edit of the other.
// FMA contraction is off for the whole file (cubic.h switches it off at file scope; stated again below for the reader).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/anystereo_spatial.h"
#include "../cubic.h"
#include "../host/errstate.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocksX = 1024;  // truth_kernel walks its crop with a grid stride

// what a kernel knows of one sample
struct Dev {
  double inv_x, inv_y;  // 1.0 / scale, computed on the host
  double fx, fy;        // scale_x, scale_y
  float* disp_out;
  unsigned char* valid_out;
  int rescale, flip, y0, x0, ch, cw, dy2;
  int fh, fw;            // the rescaled frame
  float cub_y, cub_x;    // cubic.h's scale of the final resize, (float)ch / (float)out_h and likewise: divided on the host
};

struct Table {
  Dev s[SPT_MAX_BATCH];
};

// ---- the arithmetic ----
__device__ __forceinline__ float quantise(float x) { return fminf(fmaxf(floorf(x + 0.5f), 0.f), 255.f); }
__device__ __forceinline__ float pixel(unsigned char v) { return (float)v; }
__device__ __forceinline__ float pixel(float v) { return quantise(v); }

struct Lin {
  int i0, i1;
  float t;
};

// taps of the rescaled index d on a source axis of n: cv2's source-coordinate rule with the given factor
__device__ __forceinline__ Lin lin_axis(int d, double inv, int n) {
  const float s = (float)(((double)d + 0.5) * inv - 0.5);
  const float fl = floorf(s);
  Lin a;
  a.i0 = (int)fl;
  a.t = s - fl;
  if (a.i0 < 0) {
    a.i0 = 0;
    a.t = 0.f;
  }
  if (a.i0 >= n - 1) {
    a.i0 = n - 1;
    a.t = 0.f;
  }
  a.i1 = min(a.i0 + 1, n - 1);
  return a;
}

__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, float tx, float ty) {
  const float r0 = v00 * (1.f - tx) + v01 * tx;
  const float r1 = v10 * (1.f - tx) + v11 * tx;
  return r0 * (1.f - ty) + r1 * ty;
}

// the frame pixel behind the flipped frame's pixel (y, x)
__device__ __forceinline__ void unflip(const Dev& S, int& y, int& x) {
  if (S.flip == SPT_FLIP_HF || S.flip == SPT_FLIP_H) x = S.fw - 1 - x;
  if (S.flip == SPT_FLIP_V) y = S.fh - 1 - y;
}

// ---- images ----
template <typename TIn, typename TOut, bool kResize>
__global__ __launch_bounds__(kThreads) void image_kernel(Table tab, const TIn* __restrict__ in1, const TIn* __restrict__ in2, TOut* __restrict__ out1,
                                                         TOut* __restrict__ out2, int H, int W, int h_out, int w_out) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= h_out * w_out) return;
  const int im = blockIdx.y, b = blockIdx.z;
  const Dev& S = tab.s[b];
  const long long plane_in = (long long)H * W, plane_out = (long long)h_out * w_out;
  // FLIP_H swaps the images: out1 is made of image2
  const TIn* src = ((im == 0) != (S.flip == SPT_FLIP_H) ? in1 : in2) + (long long)b * 3 * plane_in;
  TOut* dst = (im == 0 ? out1 : out2) + (long long)b * 3 * plane_out + p;
  const int oy = p / w_out, ox = p - oy * w_out;
  const int top = S.y0 + (im == 1 ? S.dy2 : 0);

  constexpr int kTaps = kResize ? 4 : 1;
  int cy[4], cx[4];
  float wy[4], wx[4];
  if (kResize) {
    as::cubic_axis(oy, S.cub_y, S.ch, cy, wy);
    as::cubic_axis(ox, S.cub_x, S.cw, cx, wx);
  } else {
    cy[0] = oy;
    cx[0] = ox;
  }
  // the source taps of the crop's rows and columns
  Lin ay[kTaps], ax[kTaps];
#pragma unroll
  for (int k = 0; k < kTaps; ++k) {
    int y = top + cy[k], x = S.x0 + cx[k];
    unflip(S, y, x);
    if (S.rescale) {
      ay[k] = lin_axis(y, S.inv_y, H);
      ax[k] = lin_axis(x, S.inv_x, W);
    } else {
      ay[k].i0 = ay[k].i1 = y;
      ax[k].i0 = ax[k].i1 = x;
      ay[k].t = ax[k].t = 0.f;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const TIn* P = src + c * plane_in;
    float q[kTaps][kTaps];  // the quantised crop pixels
#pragma unroll
    for (int a = 0; a < kTaps; ++a) {
      const long long r0 = (long long)ay[a].i0 * W, r1 = (long long)ay[a].i1 * W;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        if (S.rescale)
          q[a][k] = quantise(lerp2(pixel(P[r0 + ax[k].i0]), pixel(P[r0 + ax[k].i1]), pixel(P[r1 + ax[k].i0]), pixel(P[r1 + ax[k].i1]), ax[k].t, ay[a].t));
        else
          q[a][k] = pixel(P[r0 + ax[k].i0]);
      }
    }
    float v;
    if (kResize) {
      float rows[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) rows[a] = q[a][0] * wx[0] + q[a][1] * wx[1] + q[a][2] * wx[2] + q[a][3] * wx[3];
      v = quantise(rows[0] * wy[0] + rows[1] * wy[1] + rows[2] * wy[2] + rows[3] * wy[3]);
    } else {
      v = q[0][0];
    }
    dst[c * plane_out] = (TOut)v;
  }
}

// ---- ground truth ----
// the last source pixel in raster order that the sparse rule puts on the frame pixel (Y, X): its flat index, or -1
__device__ __forceinline__ long long sparse_source(const Dev& S, const unsigned char* __restrict__ valid, int H, int W, int Y, int X) {
  if (X <= 0 || Y <= 0) return -1;  // strict at 0, as the reference
  const int xa = max((int)floor(((double)X - 0.5) * S.inv_x) - 1, 0), xb = min((int)ceil(((double)X + 0.5) * S.inv_x) + 1, W - 1);
  const int ya = max((int)floor(((double)Y - 0.5) * S.inv_y) - 1, 0), yb = min((int)ceil(((double)Y + 0.5) * S.inv_y) + 1, H - 1);
  for (int y = yb; y >= ya; --y) {
    if (rint((double)y * S.fy) != (double)Y) continue;
    for (int x = xb; x >= xa; --x) {
      if (rint((double)x * S.fx) != (double)X) continue;
      if (valid[(long long)y * W + x] >= 1) return (long long)y * W + x;
    }
  }
  return -1;
}

template <bool kSparse>
__global__ __launch_bounds__(kThreads) void truth_kernel(Table tab, const float* __restrict__ disp, const unsigned char* __restrict__ valid, int H, int W) {
  const int b = blockIdx.z;
  const Dev& S = tab.s[b];
  const float* D = disp + (long long)b * H * W;
  const unsigned char* V = kSparse ? valid + (long long)b * H * W : nullptr;
  // 64-bit: a crop may be a whole frame of up to 2^31 - 1 pixels, and p steps past n on its last stride
  const long long n = (long long)S.ch * S.cw, stride = (long long)gridDim.x * kThreads;
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < n; p += stride) {
    const int cy = (int)(p / S.cw), cx = (int)(p - (long long)cy * S.cw);
    const int vy = S.y0 + cy, vx = S.x0 + cx;  // validity: never flipped
    int y = vy, x = vx;
    if (S.flip == SPT_FLIP_HF) x = S.fw - 1 - x;  // FLIP_H leaves the ground truth as it is
    if (S.flip == SPT_FLIP_V) y = S.fh - 1 - y;
    float d;
    if (!S.rescale) {
      d = D[(long long)y * W + x];
      if (kSparse) S.valid_out[p] = V[(long long)vy * W + vx];
    } else if (kSparse) {
      const long long at = sparse_source(S, V, H, W, y, x);
      d = at < 0 ? 0.f : (float)((double)D[at] * S.fx);
      const bool same = y == vy && x == vx;
      S.valid_out[p] = (unsigned char)((same ? at : sparse_source(S, V, H, W, vy, vx)) >= 0 ? 1 : 0);
    } else {
      const Lin ay = lin_axis(y, S.inv_y, H), ax = lin_axis(x, S.inv_x, W);
      const long long r0 = (long long)ay.i0 * W, r1 = (long long)ay.i1 * W;
      d = (float)((double)lerp2(D[r0 + ax.i0], D[r0 + ax.i1], D[r1 + ax.i0], D[r1 + ax.i1], ax.t, ay.t) * S.fx);
    }
    S.disp_out[p] = S.flip == SPT_FLIP_HF ? -d : d;
  }
}

// ---- the host side ----
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

int frame_size(const char* what, int H, int W, int rescale, double sx, double sy, int* fh, int* fw) {
  REQUIRE(H >= 1 && W >= 1, SPT_ERR_BAD_ARG, "%s: H=%d W=%d must be positive", what, H, W);
  REQUIRE(rescale == 0 || rescale == 1, SPT_ERR_BAD_ARG, "%s: rescale = %d, 0 or 1 expected", what, rescale);
  if (!rescale) {
    *fh = H;
    *fw = W;
    return SPT_OK;
  }
  REQUIRE(isfinite(sx) && isfinite(sy) && sx >= SPT_MIN_SCALE && sx <= SPT_MAX_SCALE && sy >= SPT_MIN_SCALE && sy <= SPT_MAX_SCALE, SPT_ERR_BAD_ARG,
          "%s: scale_x = %g, scale_y = %g outside [%g, %g]", what, sx, sy, SPT_MIN_SCALE, SPT_MAX_SCALE);
  const double h = rint((double)H * sy), w = rint((double)W * sx);  // half to even: the default rounding mode
  REQUIRE(h >= 1.0 && w >= 1.0, SPT_ERR_BAD_ARG, "%s: an empty rescaled frame %g x %g", what, h, w);
  REQUIRE(h * w < 2147483648.0, SPT_ERR_BAD_SHAPE, "%s: a rescaled frame of %g x %g pixels", what, h, w);
  *fh = (int)h;
  *fw = (int)w;
  return SPT_OK;
}

int validate(const char* what, const spt_sample* samples, int B, int H, int W, int out_h, int out_w) {
  REQUIRE(samples != nullptr, SPT_ERR_BAD_ARG, "%s: null pointer", what);
  REQUIRE(B >= 1 && H >= 1 && W >= 1, SPT_ERR_BAD_ARG, "%s: B=%d H=%d W=%d must be positive", what, B, H, W);
  REQUIRE((out_h == 0 && out_w == 0) || (out_h >= 1 && out_w >= 1), SPT_ERR_BAD_ARG, "%s: out size %d x %d: both 0 or both positive", what, out_h, out_w);
  REQUIRE(elements(B, H, W) < (1ll << 31), SPT_ERR_BAD_SHAPE, "%s: B=%d H=%d W=%d: need 3*B*H*W < 2^31", what, B, H, W);
  for (int b = 0; b < B; ++b) {
    const spt_sample& P = samples[b];
    int fh, fw;
    if (int rc = frame_size(what, H, W, P.rescale, P.scale_x, P.scale_y, &fh, &fw)) return rc;
    REQUIRE(P.flip >= SPT_FLIP_NONE && P.flip <= SPT_FLIP_V, SPT_ERR_BAD_ARG, "%s: sample %d: flip = %d", what, b, P.flip);
    REQUIRE(P.ch >= 1 && P.cw >= 1, SPT_ERR_BAD_ARG, "%s: sample %d: crop %d x %d must be positive", what, b, P.ch, P.cw);
    REQUIRE(P.y0 >= 0 && P.x0 >= 0 && (int64_t)P.y0 + P.ch <= fh && (int64_t)P.x0 + P.cw <= fw, SPT_ERR_CROP,
            "%s: sample %d: the crop %d x %d at (%d, %d) leaves the %d x %d frame", what, b, P.ch, P.cw, P.y0, P.x0, fh, fw);
    REQUIRE((int64_t)P.y0 + P.dy2 >= 0 && (int64_t)P.y0 + P.dy2 + P.ch <= fh, SPT_ERR_CROP,
            "%s: sample %d: image2's crop at y0 + dy2 = %d + %d leaves the %d x %d frame", what, b, P.y0, P.dy2, fh, fw);
    REQUIRE(out_h != 0 || (P.ch == samples[0].ch && P.cw == samples[0].cw), SPT_ERR_CROP,
            "%s: sample %d: crop %d x %d differs from sample 0's %d x %d and there is no out size", what, b, P.ch, P.cw, samples[0].ch, samples[0].cw);
  }
  const int h_out = out_h ? out_h : samples[0].ch, w_out = out_w ? out_w : samples[0].cw;
  REQUIRE(elements(B, h_out, w_out) < (1ll << 31), SPT_ERR_BAD_SHAPE, "%s: B=%d out %d x %d: need 3*B*h*w < 2^31", what, B, h_out, w_out);
  return SPT_OK;
}

template <typename TIn, typename TOut>
int launch_chunks(const TIn* in1, const TIn* in2, const float* disp, const unsigned char* valid, int B, int H, int W, const spt_sample* samples, TOut* out1,
                  TOut* out2, int out_h, int out_w, float* const* disp_out, unsigned char* const* valid_out, hipStream_t stream) {
  const int h_out = out_h ? out_h : samples[0].ch, w_out = out_w ? out_w : samples[0].cw;
  const int64_t plane_in = (int64_t)H * W, plane_out = (int64_t)h_out * w_out;
  for (int b0 = 0; b0 < B; b0 += SPT_MAX_BATCH) {
    const int nb = B - b0 < SPT_MAX_BATCH ? B - b0 : SPT_MAX_BATCH;
    Table t;
    int64_t most = 0;  // the largest crop of the chunk
    for (int i = 0; i < SPT_MAX_BATCH; ++i) {
      const int b = b0 + (i < nb ? i : 0);  // unused slots repeat the first sample; no block reads them
      const spt_sample& P = samples[b];
      Dev& S = t.s[i];
      S.fx = P.rescale ? P.scale_x : 1.0;
      S.fy = P.rescale ? P.scale_y : 1.0;
      S.inv_x = 1.0 / S.fx;
      S.inv_y = 1.0 / S.fy;
      S.disp_out = disp_out[b];
      S.valid_out = valid_out ? valid_out[b] : nullptr;
      S.rescale = P.rescale, S.flip = P.flip, S.y0 = P.y0, S.x0 = P.x0, S.ch = P.ch, S.cw = P.cw, S.dy2 = P.dy2;
      frame_size("spt_spatial_pair", H, W, P.rescale, P.scale_x, P.scale_y, &S.fh, &S.fw);  // validated before
      S.cub_y = (float)P.ch / (float)h_out;
      S.cub_x = (float)P.cw / (float)w_out;
      if (i < nb && (int64_t)P.ch * P.cw > most) most = (int64_t)P.ch * P.cw;
    }
    const TIn* i1 = in1 + (int64_t)b0 * 3 * plane_in;
    const TIn* i2 = in2 + (int64_t)b0 * 3 * plane_in;
    TOut* o1 = out1 + (int64_t)b0 * 3 * plane_out;
    TOut* o2 = out2 + (int64_t)b0 * 3 * plane_out;
    const dim3 grid((unsigned)((plane_out + kThreads - 1) / kThreads), 2u, (unsigned)nb);
    if (out_h)
      hipLaunchKernelGGL((image_kernel<TIn, TOut, true>), grid, dim3(kThreads), 0, stream, t, i1, i2, o1, o2, H, W, h_out, w_out);
    else
      hipLaunchKernelGGL((image_kernel<TIn, TOut, false>), grid, dim3(kThreads), 0, stream, t, i1, i2, o1, o2, H, W, h_out, w_out);
    if (int rc = check_launch("spt_spatial_pair (images)", SPT_ERR_LAUNCH)) return rc;
    int64_t gx = (most + kThreads - 1) / kThreads;
    if (gx > kMaxBlocksX) gx = kMaxBlocksX;
    const dim3 tgrid((unsigned)gx, 1u, (unsigned)nb);
    const float* d = disp + (int64_t)b0 * plane_in;
    if (valid != nullptr)
      hipLaunchKernelGGL((truth_kernel<true>), tgrid, dim3(kThreads), 0, stream, t, d, valid + (int64_t)b0 * plane_in, H, W);
    else
      hipLaunchKernelGGL((truth_kernel<false>), tgrid, dim3(kThreads), 0, stream, t, d, (const unsigned char*)nullptr, H, W);
    if (int rc = check_launch("spt_spatial_pair (ground truth)", SPT_ERR_LAUNCH)) return rc;
  }
  return SPT_OK;
}

}  // namespace

extern "C" {

int spt_abi_version(void) { return 1; }

const char* spt_last_error_string(void) { return err_buf(); }

int spt_frame_size(int H, int W, int rescale, double scale_x, double scale_y, int* fh, int* fw) {
  REQUIRE(fh != nullptr && fw != nullptr, SPT_ERR_BAD_ARG, "spt_frame_size: null pointer");
  return frame_size("spt_frame_size", H, W, rescale, scale_x, scale_y, fh, fw);
}

int spt_validate(const spt_sample* samples, int B, int H, int W, int out_h, int out_w) { return validate("spt_validate", samples, B, H, W, out_h, out_w); }

int spt_spatial_pair(const void* image1, const void* image2, int in_dtype, const float* disp, const unsigned char* valid, int B, int H, int W,
                     const spt_sample* samples, void* out1, void* out2, int out_dtype, int out_h, int out_w, float* const* disp_out,
                     unsigned char* const* valid_out, void* stream) {
  const char* what = "spt_spatial_pair";
  REQUIRE(image1 != nullptr && image2 != nullptr && disp != nullptr && samples != nullptr && out1 != nullptr && out2 != nullptr && disp_out != nullptr,
          SPT_ERR_BAD_ARG, "%s: null pointer", what);
  REQUIRE((valid == nullptr) == (valid_out == nullptr), SPT_ERR_BAD_ARG, "%s: valid and valid_out go together (the sparse form) or are both NULL", what);
  REQUIRE((in_dtype == SPT_U8 || in_dtype == SPT_F32) && (out_dtype == SPT_U8 || out_dtype == SPT_F32), SPT_ERR_BAD_ARG,
          "%s: in_dtype=%d out_dtype=%d: SPT_U8 or SPT_F32 expected", what, in_dtype, out_dtype);
  if (int rc = validate(what, samples, B, H, W, out_h, out_w)) return rc;
  REQUIRE(in_dtype == SPT_U8 || (aligned(image1, 4) && aligned(image2, 4)), SPT_ERR_BAD_ARG, "%s: fp32 inputs must be 4-byte aligned", what);
  REQUIRE(out_dtype == SPT_U8 || (aligned(out1, 4) && aligned(out2, 4)), SPT_ERR_BAD_ARG, "%s: fp32 outputs must be 4-byte aligned", what);
  REQUIRE(aligned(disp, 4), SPT_ERR_BAD_ARG, "%s: disp must be 4-byte aligned", what);
  for (int b = 0; b < B; ++b) {
    REQUIRE(disp_out[b] != nullptr && aligned(disp_out[b], 4), SPT_ERR_BAD_ARG, "%s: disp_out[%d] is NULL or not 4-byte aligned", what, b);
    REQUIRE(valid_out == nullptr || valid_out[b] != nullptr, SPT_ERR_BAD_ARG, "%s: valid_out[%d] is NULL", what, b);
  }
  // aliasing: every output against every input and every other output
  const int h_out = out_h ? out_h : samples[0].ch, w_out = out_w ? out_w : samples[0].cw;
  const int64_t px_in = (int64_t)B * H * W;
  const int64_t nin = 3 * px_in * (in_dtype == SPT_F32 ? 4 : 1), nout = 3ll * B * h_out * w_out * (out_dtype == SPT_F32 ? 4 : 1);
  const void* ins[4] = {image1, image2, disp, valid};
  const int64_t nins[4] = {nin, nin, px_in * 4, valid ? px_in : 0};
  const int n_outs = 2 + B * (valid_out ? 2 : 1);
  auto out_at = [&](int o, const void** p, int64_t* n) {
    if (o < 2) {
      *p = o == 0 ? out1 : out2;
      *n = nout;
    } else if (o < 2 + B) {
      *p = disp_out[o - 2];
      *n = (int64_t)samples[o - 2].ch * samples[o - 2].cw * 4;
    } else {
      *p = valid_out[o - 2 - B];
      *n = (int64_t)samples[o - 2 - B].ch * samples[o - 2 - B].cw;
    }
  };
  for (int o = 0; o < n_outs; ++o) {
    const void* p;
    int64_t n;
    out_at(o, &p, &n);
    for (int i = 0; i < 4; ++i)
      REQUIRE(nins[i] == 0 || !overlap(p, n, ins[i], nins[i]), SPT_ERR_ALIAS, "%s: output %d overlaps input %d", what, o, i);
    for (int o2 = 0; o2 < o; ++o2) {
      const void* p2;
      int64_t n2;
      out_at(o2, &p2, &n2);
      REQUIRE(!overlap(p, n, p2, n2), SPT_ERR_ALIAS, "%s: output %d overlaps output %d", what, o, o2);
    }
  }

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  typedef unsigned char u8;
  if (in_dtype == SPT_U8 && out_dtype == SPT_U8)
    return launch_chunks((const u8*)image1, (const u8*)image2, disp, valid, B, H, W, samples, (u8*)out1, (u8*)out2, out_h, out_w, disp_out, valid_out, s);
  if (in_dtype == SPT_U8)
    return launch_chunks((const u8*)image1, (const u8*)image2, disp, valid, B, H, W, samples, (float*)out1, (float*)out2, out_h, out_w, disp_out, valid_out, s);
  if (out_dtype == SPT_U8)
    return launch_chunks((const float*)image1, (const float*)image2, disp, valid, B, H, W, samples, (u8*)out1, (u8*)out2, out_h, out_w, disp_out, valid_out, s);
  return launch_chunks((const float*)image1, (const float*)image2, disp, valid, B, H, W, samples, (float*)out1, (float*)out2, out_h, out_w, disp_out, valid_out, s);
}

}  // extern "C"
