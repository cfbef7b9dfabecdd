// On-device evaluation pictures (evaluation.py:35-65 Disp_to_color, written at :196,318,434,543 with torchvision's save_image;
// metrics_utils/visualization.py:30-55 disp_error_image_func, used at evaluation.py:187,309,425,533).
//
// as_disp_images: ONE pass over the prediction (and the ground truth) writes up to three 8-bit pictures per image:
//   color [B,H,W,3]  the KITTI disparity colour map, quantised as save_image does: q = (uint8) clamp(fl(fl(v * 255) + 0.5), 0, 255)
//   error [B,H,W,3]  the KITTI error map: ten colour bands over r = min(E / abs_thres, (E / gt) / rel_thres), black where gt <= 0,
//                    the ten-colour legend in the top-left 10 x 200 pixels
//   enc16 [B,H,W,2]  the KITTI 16-bit encoding round(disp * 256), high byte first (PNG's sample order; the inverse of readDispKITTI,
//                    frame_utils.py:124-127)
// A stream without reuse: 4 or 8 bytes per pixel in, up to 8 bytes out.  The three outputs are interleaved and contiguous over the
// batch, so the kernel indexes the flat array of B*H*W pixels: a thread owns 4 consecutive flat pixels, reads disp / gt with one
// 16-byte load each (when the base is 16-byte aligned; four 4-byte loads otherwise), and writes 12 bytes per picture and 8 bytes
// of enc16, each as one store of whole dwords (the outputs are 4-byte aligned and 12 * i, 8 * i keep that).  The last
// B*H*W mod 4 pixels belong to one more thread, which stores bytes.  No LDS, no atomics, no scratch buffer; every byte of a
// requested output is written.
//
// Arithmetic: every step the reference rounds is one fp32 rounding here (__fdiv_rn / __fmul_rn / __fadd_rn / __fsub_rn: IEEE
// division, no FMA contraction), in the reference's order, so the bytes equal the quantised reference.
//   colour  t = clamp(disp / max_disp, 0, 1); k = #{j : t > e_j}, e = (114, 299, 413, 587, 701, 886) / 1000;
//           u = (t - lo_k) * inv_k, lo = (0, e_0..e_5), inv_k = 1 / (w_k / 1000), w = (114, 185, 114, 174, 114, 185, 114);
//           v_c = A[k][c] * (1 - u) + A[k+1][c] * u over the colour rows A = 000, 001, 100, 101, 010, 011, 110, 111 (RGB).
//           (1 - u) + u is NOT folded to 1.  disp < 0 or -inf: black; disp >= max_disp or +inf: white; NaN: (0,0,0) (the reference
//           hands save_image a NaN, whose cast is undefined).
//   error   E = |gt - est|; band i of 10 holds 2^(i-5) <= r < 2^(i-4) (band 0 from 0, band 9 without upper bound but r < +inf);
//           r in no band — NaN or +-inf estimates — and gt <= 0: black.  The band colours are integers c, stored as c / 255 by the
//           reference, and quantising c / 255 gives c back, so the integers are written directly.  The reference's dilation is a
//           TODO there and is not done here.
//   enc16   n = clamp(rint(disp * 256), 0, 65535), ties to even; NaN: 0.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;

struct ColorMap {  // the folded constants of Disp_to_color; each quotient is one IEEE fp32 division (constant-folded by the compiler)
  static constexpr float e0 = 114.f / 1000.f, e1 = 299.f / 1000.f, e2 = 413.f / 1000.f, e3 = 587.f / 1000.f, e4 = 701.f / 1000.f,
                         e5 = 886.f / 1000.f;
  static constexpr float i114 = 1.f / (114.f / 1000.f), i185 = 1.f / (185.f / 1000.f), i174 = 1.f / (174.f / 1000.f);
};
// colour row r as R << 2 | G << 1 | B, three bits per row, row 0 lowest: 000 001 100 101 010 011 110 111
constexpr unsigned kColorRows = 0u | (1u << 3) | (4u << 6) | (5u << 9) | (2u << 12) | (3u << 15) | (6u << 18) | (7u << 21);

constexpr unsigned rgb(unsigned r, unsigned g, unsigned b) { return r | (g << 8) | (b << 16); }
// the error bands' colours (visualization.py:12-22), as R | G << 8 | B << 16
__device__ __forceinline__ unsigned band_color(int i) {
  constexpr unsigned t[10] = {rgb(49, 54, 149),   rgb(69, 117, 180), rgb(116, 173, 209), rgb(171, 217, 233), rgb(224, 243, 248),
                              rgb(254, 224, 144), rgb(253, 174, 97), rgb(244, 109, 67),  rgb(215, 48, 39),   rgb(165, 0, 38)};
  unsigned c = t[0];
#pragma unroll
  for (int j = 1; j < 10; ++j) c = i == j ? t[j] : c;  // selects: no table in memory
  return c;
}

// save_image's quantisation of one channel value
__device__ __forceinline__ unsigned quantize(float v) {
  const float x = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);
  return (unsigned)fminf(fmaxf(x, 0.f), 255.f);  // NaN -> 0; truncation
}

__device__ __forceinline__ unsigned color_pixel(float d, float max_disp) {
  using M = ColorMap;
  const float t = fminf(fmaxf(__fdiv_rn(d, max_disp), 0.f), 1.f);  // NaN -> 0: black
  int k = 0;
  float lo = 0.f, inv = M::i114;
  if (t > M::e0) k = 1, lo = M::e0, inv = M::i185;
  if (t > M::e1) k = 2, lo = M::e1, inv = M::i114;
  if (t > M::e2) k = 3, lo = M::e2, inv = M::i174;
  if (t > M::e3) k = 4, lo = M::e3, inv = M::i114;
  if (t > M::e4) k = 5, lo = M::e4, inv = M::i185;
  if (t > M::e5) k = 6, lo = M::e5, inv = M::i114;
  const float u = __fmul_rn(__fsub_rn(t, lo), inv);
  const float om = __fsub_rn(1.f, u);
  const unsigned a = (kColorRows >> (3 * k)) & 7u, b = (kColorRows >> (3 * k + 3)) & 7u;
  unsigned px = 0u;
#pragma unroll
  for (int c = 0; c < 3; ++c) {  // c = 0: R (bit 2)
    const unsigned bit = 4u >> c;
    // A is 0 or 1: the products are the factor itself or a zero (whose sign does not survive the quantisation)
    const float v = __fadd_rn((a & bit) ? om : 0.f, (b & bit) ? u : 0.f);
    px |= quantize(v) << (8 * c);
  }
  return px;
}

// q = the pixel's index inside its image; the legend is looked at only where q < legend_end = min(10, H) * W (from the host)
__device__ __forceinline__ unsigned error_pixel(float est, float g, unsigned q, unsigned W, unsigned legend_end, float abs_thres,
                                                float rel_thres) {
  if (q < legend_end) {
    const unsigned y = q / W, x = q - y * W;
    if (x < 200u) return band_color((int)(x / 20u));
  }
  if (!(g > 0.f)) return 0u;
  const float e = fabsf(__fsub_rn(g, est));
  const float ra = __fdiv_rn(e, abs_thres), rb = __fdiv_rn(__fdiv_rn(e, g), rel_thres);
  const float r = (ra != ra || rb != rb) ? ra + rb : fminf(ra, rb);  // np.minimum: a NaN on either side stays a NaN
  if (!(r >= 0.f && r < __builtin_inff())) return 0u;               // in no band (NaN, +inf): black
  // band i: 2^(i-5) <= r < 2^(i-4) for 1 <= i <= 8, below: 0, above: 9 -> the biased exponent - 122, clamped (zero and denormals: 0)
  const int ex = (int)((__float_as_uint(r) >> 23) & 0xffu) - 122;
  return band_color(min(max(ex, 0), 9));
}

__device__ __forceinline__ unsigned enc16_pixel(float d) {
  const float x = __fmul_rn(d, 256.f);
  const unsigned n = (unsigned)fminf(fmaxf(rintf(x), 0.f), 65535.f);  // NaN -> 0; rintf: ties to even
  return (n >> 8) | ((n & 0xffu) << 8);                               // high byte first
}

struct U3 { unsigned x, y, z; };  // 12 bytes, 4-byte aligned: one dwordx3 store
struct U2 { unsigned x, y; };     // 8 bytes, 4-byte aligned: one dwordx2 store

// four packed 24-bit pixels -> 12 interleaved bytes
__device__ __forceinline__ U3 pack_rgb4(const unsigned c[4]) {
  return U3{c[0] | (c[1] << 24), (c[1] >> 8) | (c[2] << 16), (c[2] >> 16) | (c[3] << 8)};
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void disp_images_kernel(const float* __restrict__ disp, const float* __restrict__ gt,
                                                               unsigned char* __restrict__ color, unsigned char* __restrict__ error,
                                                               unsigned char* __restrict__ enc16, unsigned total, unsigned HW, unsigned W,
                                                               unsigned legend_end,
                                                               float max_disp, float abs_thres, float rel_thres) {
  const unsigned groups = total / kPerThread;
  const unsigned gid = blockIdx.x * kThreads + threadIdx.x;  // <= groups + kThreads, total <= (2^31-1)/3 (checked by the host)
  if (gid < groups) {
    const unsigned p0 = gid * kPerThread;
    float d[4], g[4] = {0.f, 0.f, 0.f, 0.f};
    if (kVec) {
      const float4 d4 = *reinterpret_cast<const float4*>(disp + p0);
      d[0] = d4.x, d[1] = d4.y, d[2] = d4.z, d[3] = d4.w;
      if (gt) {
        const float4 g4 = *reinterpret_cast<const float4*>(gt + p0);
        g[0] = g4.x, g[1] = g4.y, g[2] = g4.z, g[3] = g4.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = disp[p0 + k];
      if (gt) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gt[p0 + k];
      }
    }
    if (color) {
      unsigned c[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] = color_pixel(d[k], max_disp);
      *reinterpret_cast<U3*>(color + (size_t)p0 * 3) = pack_rgb4(c);
    }
    if (error) {
      unsigned c[4];
      unsigned q = p0 % HW;  // one division per thread; the four pixels may straddle two images
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c[k] = error_pixel(d[k], g[k], q, W, legend_end, abs_thres, rel_thres);
        q = q + 1u == HW ? 0u : q + 1u;
      }
      *reinterpret_cast<U3*>(error + (size_t)p0 * 3) = pack_rgb4(c);
    }
    if (enc16) {
      const unsigned n0 = enc16_pixel(d[0]), n1 = enc16_pixel(d[1]), n2 = enc16_pixel(d[2]), n3 = enc16_pixel(d[3]);
      *reinterpret_cast<U2*>(enc16 + (size_t)p0 * 2) = U2{n0 | (n1 << 16), n2 | (n3 << 16)};
    }
  } else if (gid == groups) {  // the last total mod 4 pixels: byte stores
    for (unsigned p = groups * kPerThread; p < total; ++p) {
      const float dv = disp[p];
      if (color) {
        const unsigned c = color_pixel(dv, max_disp);
        color[(size_t)p * 3 + 0] = (unsigned char)(c & 0xffu);
        color[(size_t)p * 3 + 1] = (unsigned char)((c >> 8) & 0xffu);
        color[(size_t)p * 3 + 2] = (unsigned char)((c >> 16) & 0xffu);
      }
      if (error) {
        const unsigned c = error_pixel(dv, gt[p], p % HW, W, legend_end, abs_thres, rel_thres);
        error[(size_t)p * 3 + 0] = (unsigned char)(c & 0xffu);
        error[(size_t)p * 3 + 1] = (unsigned char)((c >> 8) & 0xffu);
        error[(size_t)p * 3 + 2] = (unsigned char)((c >> 16) & 0xffu);
      }
      if (enc16) {
        const unsigned n = enc16_pixel(dv);
        enc16[(size_t)p * 2 + 0] = (unsigned char)(n & 0xffu);
        enc16[(size_t)p * 2 + 1] = (unsigned char)(n >> 8);
      }
    }
  }
}

inline bool aligned(const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline bool finite_positive(float v) { return v > 0.f && v < __builtin_inff(); }  // false for NaN

}  // namespace

extern "C" {

int as_disp_images(const float* disp, const float* gt, unsigned char* color, unsigned char* error, unsigned char* enc16, int B, int H,
                   int W, float max_disp, float abs_thres, float rel_thres, void* stream) {
  AS_REQUIRE(disp, AS_ERR_BAD_ARG, "disp_images: null disp");
  AS_REQUIRE(color || error || enc16, AS_ERR_BAD_ARG, "disp_images: no output requested");
  AS_REQUIRE(!error || gt, AS_ERR_BAD_ARG, "disp_images: the error picture needs gt");
  AS_REQUIRE(B > 0 && H > 0 && W > 0, AS_ERR_BAD_ARG, "disp_images: non-positive size");
  AS_REQUIRE(finite_positive(max_disp) && finite_positive(abs_thres) && finite_positive(rel_thres), AS_ERR_BAD_ARG,
             "disp_images: max_disp=%g, abs_thres=%g, rel_thres=%g must be finite and positive", (double)max_disp, (double)abs_thres,
             (double)rel_thres);
  AS_REQUIRE(aligned(color, 4) && aligned(error, 4) && aligned(enc16, 4), AS_ERR_BAD_ARG,
             "disp_images: an output is not 4-byte aligned (the kernel stores whole dwords)");
  const int64_t total = (int64_t)B * H * W;
  AS_REQUIRE(3 * total <= 2147483647ll, AS_ERR_BAD_SHAPE, "disp_images: %lld pixels x 3 bytes exceed 2^31-1", (long long)total);
  const unsigned groups = (unsigned)(total / kPerThread);
  const unsigned threads = groups + (total % kPerThread ? 1u : 0u);
  const dim3 grid((unsigned)as::cdiv64(threads, kThreads));
  const unsigned legend_end = (unsigned)((H < 10 ? H : 10) * (int64_t)W);  // the legend's rows, clipped by the image; <= H * W
  hipStream_t s = as::as_stream(stream);
  if (aligned(disp, 16) && aligned(gt, 16))
    hipLaunchKernelGGL(disp_images_kernel<true>, grid, dim3(kThreads), 0, s, disp, gt, color, error, enc16, (unsigned)total,
                       (unsigned)(H * (int64_t)W), (unsigned)W, legend_end, max_disp, abs_thres, rel_thres);
  else
    hipLaunchKernelGGL(disp_images_kernel<false>, grid, dim3(kThreads), 0, s, disp, gt, color, error, enc16, (unsigned)total,
                       (unsigned)(H * (int64_t)W), (unsigned)W, legend_end, max_disp, abs_thres, rel_thres);
  return as::check_launch("disp_images");
}

}  // extern "C"
